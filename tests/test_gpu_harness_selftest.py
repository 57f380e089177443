"""The code the C++ test programs share (tests/cpp/loopback.hpp, host_table.hpp,
bucket_model.hpp), tested directly by tests/cpp/harness_selftest.cpp: the
loopback transport's per-pair sequencing, zero-byte and odd-length messages
and its counters at G = 3; the host table's device round trip at the edges of
the mask word; the host bucket bit fields at every fan-out."""
import subprocess

import pytest

import cpp_programs

pytestmark = pytest.mark.gpu


def test_harness_selftest():
    exe = cpp_programs.build("harness_selftest", include=("include", "csrc"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("HARNESS SELFTEST OK") == 1, r.stdout
    # 8 bucket shapes, the transport, 4 sizes with and without a mask, row_hash
    assert r.stdout.count(": ok\n") == 8 + 1 + 8 + 1, r.stdout
