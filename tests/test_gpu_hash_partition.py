"""dj::hash_partition and its sub-steps called directly
(tests/cpp/hash_partition_check.cpp): part_count_kernel, part_scan_kernel,
part_offsets_kernel and part_scatter_kernel at every NPL tier against the host's
stable partition, exact: all nparts + 1 offsets, out_keys and out_pay (the
permutation itself), the per-wave prefix table and the totals left in scratch,
and poison guards on both sides of every written buffer — at the wave and
batch edges (a last batch with one valid lane in every wave, empty trailing
waves, rows per wave above the target and no multiple of 64), at the first and
last nparts of each tier, with two populated partitions on one lane, with empty
partitions, with null payloads and on scratch left over from another nparts.
"""
import os
import subprocess

import pytest

import cpp_programs

LIB = cpp_programs.LIB

# cases (one ": ok" line each) per set
SETS = {
    # 17 row counts (0 to 3 * target * wave cap + 12345) at nparts 1, 64, 65, 1024
    "sizes": 68,
    # 17 nparts at a small and at the central row count, and again through the
    # three sub-steps (all 17 at the small one, one per tier at the central one)
    "nparts": 56,
    # nparts 64, 129, 1024 x two row counts x (all rows in one partition,
    # round robin, alternating lane mates, shifted runs, even partitions,
    # MurmurHash3 with three seeds, null input / output payload), and the
    # alternating pattern at 128, 256, 512
    "patterns": 83,
}
CASES = sum(SETS.values())


def _harness():
    return cpp_programs.build("hash_partition_check", include=("csrc",))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SETS))
def test_hash_partition_check(name):
    cases = SETS[name]
    r = subprocess.run([_harness(), "--set", name], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "HASH PARTITION OK (%d cases)" % cases in r.stdout
    assert r.stdout.count(": ok\n") == cases, r.stdout[-4000:]


@pytest.mark.skipif(not os.path.exists(LIB), reason="libdistjoin.so has not been built")
def test_hash_partition_check_inputs():
    """Host side of the harness alone: every case's keys land in the partition
    its pattern names, the host geometry agrees with the scratch size, the
    central case ends every populated wave on a partial batch and leaves waves
    empty; fails if a named situation (a partial batch in each NPL tier, lane
    mates in one batch, an empty partition between populated ones, more waves
    than the scan block is wide) is absent."""
    r = subprocess.run([_harness(), "--inputs-only"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "HASH PARTITION INPUTS OK (%d cases)" % CASES in r.stdout
