"""GPU test of the local join's two-level bucket partition, called directly
(dj::bucket_partition2 through tests/cpp/bucket_partition_check.cpp): the
exact counted pass A, which the product reaches only at ~2e9 rows per table,
and the slack pass A with its compact pass B, at the staging-tile edges, with
one block's chunk crossing a tile, and at the F > 256 sub-bucket bit field.
"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_bucket_partition_check():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(repo, "tests", "cpp", "bucket_partition_check")
    if not os.path.exists(exe):
        subprocess.run(
            ["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17",
             "-I", os.path.join(repo, "distributed_join_amd", "csrc"),
             os.path.join(repo, "tests", "cpp", "bucket_partition_check.cpp"),
             "-o", exe, "-L", os.path.join(repo, "distributed_join_amd"), "-ldistjoin",
             "-Wl,-rpath," + os.path.join(repo, "distributed_join_amd")],
            check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "BUCKET PARTITION OK" in r.stdout
    # 7 cases, each on the exact and on the slack pass A
    assert r.stdout.count(": ok\n") == 14, r.stdout
