"""The fused wire path's partition steps called directly
(tests/cpp/fused_lists_check.cpp): dj::fused_partition against the host's
MurmurHash3 rank/batch partition and group bits at six (nparts_rank, PA)
shapes, the block-count and staged-tile edges, two seeds, a null payload and
one all-equal table; dj::subpart_lists over hand-built per-peer segment lists
(G up to 8, every F, segment lengths around the staged tile, empty peers and
groups); and the two chained as sender and receiver. Exact: offsets, every
row's slice or bucket and identity, poison guards after every output.
"""
import os
import subprocess

import pytest

import cpp_programs

LIB = cpp_programs.LIB

# 15 fused_partition runs (6 shapes, 6 sizes, second seed, null payload, equal
# keys), 5 hand-built segment lists, the chained case's 2 partitions + 1 list
RUNS = 23


def _harness():
    return cpp_programs.build("fused_lists_check", include=("csrc",))


@pytest.mark.gpu
def test_fused_lists_check():
    r = subprocess.run([_harness()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "FUSED LISTS OK" in r.stdout
    assert r.stdout.count(": ok\n") == RUNS, r.stdout[-4000:]


@pytest.mark.gpu
@pytest.mark.parametrize("f", [32, 96])
def test_subpart_lists_rejects_bad_fanout(f):
    r = subprocess.run([_harness(), "--bad-f", str(f)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "F must be a power of two in [64,1024]" in r.stderr
    assert "NOT REJECTED" not in r.stdout


@pytest.mark.skipif(not os.path.exists(LIB), reason="libdistjoin.so has not been built")
def test_fused_lists_check_inputs():
    """Host side of the harness alone: the fused chunk sizes and the hand-built
    segment lists; fails if a named situation (chunk at tile-1/tile/tile+1,
    every segment length around the tile in one group, an empty peer, a group
    empty everywhere, an empty last group) is absent."""
    r = subprocess.run([_harness(), "--inputs-only"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "FUSED LISTS INPUTS OK" in r.stdout
