"""CPU: the arithmetic of the flow table's text writer (embedding_amd/csrc/flow_text_plan.h) built for the host into a program of its own
(tests/native/flow_text_plan_harness.cpp), plain and once more under -fsanitize=address,undefined: int64 decimals as %lld spells them, a .matrix row without
its zeros — byte offset -> (column, character) against the row spelled out — and row starts above 2^32."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "flow_text_plan_harness.cpp")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("flow_text_plan_" + request.param) / "flow_text_plan_harness")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, SRC])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout, r.stderr)
        return r.stdout.strip()
    return run


def test_decimals_are_sized_and_spelled_as_percent_lld(plan):
    vals = [0, 1, -1, 9, -9, 2 ** 63 - 1, -(2 ** 63 - 1), -2 ** 63, 24 * 2 ** 40, 2 ** 40]
    for k in range(19):
        vals += [10 ** k, -10 ** k, 10 ** k - 1, -(10 ** k - 1), 10 ** k + 1]
    out = plan("decimal", *vals).splitlines()
    assert out == ["%d %d" % (len(str(v)), v) for v in vals]


def test_byte_offset_to_column_and_character_on_random_sparse_rows(plan):
    """n = 1 .. 300 columns, weights of 1 .. 15 digits, three separators, densities from all-zero to nearly full: every byte by itself, the walking cursor from
    three starts, every column's start and every row's length, against snprintf"""
    for seed in (1, 2):
        out = plan("rows", seed).split()
        assert out[0] == "ok" and int(out[1]) > 300 * 300            # bytes compared


def test_rows_above_two_to_the_32_are_found(plan):
    out = plan("far").split()
    assert out[0] == "ok" and int(out[1]) > 0                        # offsets above 2^32 tried
