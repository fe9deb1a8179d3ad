"""GPU: the C++ host mirror's DeepWalk::learnEmbedding reads its .seq files through the device ingest and trains on the resident corpus; the program
tests/native/host_seq_test.cpp compares it with the stream reader it replaced (DeepWalk::readSentencesHost + dge_train_sgns) on the same files at
workers = 1: identical .vec bytes, identical held-out dge_eval_result."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_learn_embedding_through_the_ingest_equals_the_host_reader(tmp_path, dge):
    exe = str(tmp_path / "host_seq_test")
    libdir = os.path.join(ROOT, "embedding_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "native", "host_seq_test.cpp"), "-o", exe,
                           "-L" + libdir, "-l:libdge.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "HOST SEQ OK" in out.stdout, out.stdout + out.stderr
