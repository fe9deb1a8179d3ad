"""GPU: the C++ host mirror's CrossTimeGraph::outputSampleSequence and SpatialGraph::outputSampleSequence sample into a device corpus and let the device
format the lines (dge_walks_write_seq); the program tests/native/host_seq_write_test.cpp compares them with the host loop they replaced, restated there, from
the same seed and across a chunk boundary: identical file bytes, LayeredGraph::rnd at the same position."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_output_sample_sequence_through_the_device_writer_equals_the_host_loop(tmp_path, dge):
    exe = str(tmp_path / "host_seq_write_test")
    libdir = os.path.join(ROOT, "embedding_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "native", "host_seq_write_test.cpp"), "-o", exe,
                           "-L" + libdir, "-l:libdge.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "HOST SEQ WRITE OK" in out.stdout, out.stdout + out.stderr
