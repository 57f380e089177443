"""GPU test of the local join's two-level bucket partition, called directly
(dj::bucket_partition2 through tests/cpp/bucket_partition_check.cpp): the
exact counted pass A, which the product reaches only at ~2e9 rows per table,
and the slack pass A with its compact pass B, at the staging-tile edges, with
one block's chunk crossing a tile, and at the F > 256 sub-bucket bit field.
"""
import subprocess

import pytest

import cpp_programs

pytestmark = pytest.mark.gpu


def test_bucket_partition_check():
    exe = cpp_programs.build("bucket_partition_check", include=("csrc",))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "BUCKET PARTITION OK" in r.stdout
    # 7 cases, each on the exact and on the slack pass A
    assert r.stdout.count(": ok\n") == 14, r.stdout
