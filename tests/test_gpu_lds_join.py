"""lds_join_kernel called directly (dj::lds_join and dj::lds_join_slack through
tests/cpp/lds_join_check.cpp) on hand-built buckets, against a per-bucket host
multimap join, exact: build lengths at the skew cap, match counts at the stage
watermark and the stage size, a probe chain that wraps the table end, table
reset between buckets, output capacities that cut a flush and a spill, and a
populated group in the grid's second trip — in both bucket layouts.
"""
import os
import subprocess

import pytest

import cpp_programs

LIB = cpp_programs.LIB

# 62 cases (2 build-length edge, 2 table reset, 20 + 30 stage arithmetic,
# 2 wrap-around, 3 duplicates/sentinel, 3 second trip), each in both layouts
RUNS = 124


def _harness():
    return cpp_programs.build("lds_join_check", include=("csrc",))


@pytest.mark.gpu
def test_lds_join_check():
    r = subprocess.run([_harness()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "LDS JOIN OK" in r.stdout
    assert r.stdout.count(": ok\n") == RUNS, r.stdout[-4000:]


@pytest.mark.gpu
def test_lds_join_rejects_b_not_multiple_of_group():
    r = subprocess.run([_harness(), "--bad-b"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "multiple of 4" in r.stderr
    assert "NOT REJECTED" not in r.stdout


@pytest.mark.skipif(not os.path.exists(LIB), reason="libdistjoin.so has not been built")
def test_lds_join_check_inputs():
    """Host side of the harness alone: cases, reference, wrap-around key
    search, and the stage patterns' coverage by arithmetic on match counts."""
    r = subprocess.run([_harness(), "--inputs-only"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "LDS JOIN INPUTS OK (62 cases)" in r.stdout
