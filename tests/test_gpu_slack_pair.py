"""dj::bucket_partition2_slack_pair called directly (tests/cpp/slack_pair_check.cpp):
the hot pass A (bucket_scatter_slack_pair_kernel) and pass B
(bucket_subpart_slack2_pair_kernel) of every single-rank join on two tables at
once, against a host prediction, exact: the overflow word, the cursors, every
bucket length, every stored row's bucket and identity, and poison guards after
tmp, out, lens and the cursors — at every grid split, at the pass-A and pass-B
tile edges (second and third tile, one-row tails, the prefetch copy under a
null payload), at both capacities exactly full and one over, under heavy skew,
at the full fan-outs and on reused scratch.
"""
import os
import subprocess

import pytest

import cpp_programs

LIB = cpp_programs.LIB

# runs (": ok" lines) and cases per set; "special keys" and one pass-B edge run twice
SETS = {
    # 5 grid splits, 5 pass-B group sizes, 4 + 2 capB edges, 3 capA edges, the
    # repeated key, B = 1024, special keys; two of them twice
    "edges": (24, 22),
    # 3 even splits around the pass-A tile, one block three tiles deep with and
    # without payload columns
    "tiles": (5, 5),
    # B = 524288 and B = 1048576
    "fanout": (2, 2),
}
CASES = sum(cases for _, cases in SETS.values())


def _harness():
    return cpp_programs.build("slack_pair_check", include=("csrc",))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SETS))
def test_slack_pair_check(name):
    runs, cases = SETS[name]
    r = subprocess.run([_harness(), "--set", name], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "SLACK PAIR OK (%d cases)" % cases in r.stdout
    assert r.stdout.count(": ok\n") == runs, r.stdout[-4000:]


@pytest.mark.skipif(not os.path.exists(LIB), reason="libdistjoin.so has not been built")
def test_slack_pair_check_inputs():
    """Host side of the harness alone: every case's block split, tiles per
    block, fullest group and bucket against their capacities and predicted
    overflow word; fails if a case misses its target or a named situation
    (third tile, one-row tail, BTILE+1 group, exact fit and one over for both
    capacities, empty group) is absent."""
    r = subprocess.run([_harness(), "--inputs-only"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "SLACK PAIR INPUTS OK (%d cases)" % CASES in r.stdout
