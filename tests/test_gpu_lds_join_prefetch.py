"""lds_join_kernel's first-row prefetch (both sides' rows loaded ahead of the
table clear, predicated on the side's length), through dj::lds_join and
dj::lds_join_slack (tests/cpp/lds_join_prefetch_check.cpp) on hand-built
buckets that all share one key pool, against a per-bucket host multimap join,
exact: side lengths around the block size, -1 build keys in a bucket's first
block and in its tail, empty and skew-routed buckets between populated ones
inside a group and across the block's trips, a whole empty group, the last
bucket of B with nothing allocated behind it, and slack segments far shorter
than the block — with both table sizes and in both bucket layouts.
"""
import os
import subprocess

import pytest

import cpp_programs

LIB = cpp_programs.LIB

# 6 cases for each of the two table sizes, each in both layouts
CASES = 12
RUNS = 2 * CASES


def _harness():
    return cpp_programs.build("lds_join_prefetch_check", include=("csrc",))


@pytest.mark.gpu
def test_lds_join_prefetch_check():
    r = subprocess.run([_harness()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "LDS JOIN PREFETCH OK" in r.stdout
    assert r.stdout.count(": ok\n") == RUNS, r.stdout[-4000:]


@pytest.mark.skipif(not os.path.exists(LIB), reason="libdistjoin.so has not been built")
def test_lds_join_prefetch_check_inputs():
    """Host side of the harness alone: the cases, the reference, and what each
    case claims about its own layout."""
    r = subprocess.run([_harness(), "--inputs-only"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert f"LDS JOIN PREFETCH INPUTS OK ({CASES} cases)" in r.stdout
