"""The global-table join and neg1_cross_join called directly
(tests/cpp/table_join_check.cpp): join_build / join_probe and their pair forms
(pair pointers aligned to 16 bytes only) against a host multimap join, exact:
the table join_build leaves behind (every build row once, every other slot
empty, no empty slot between an entry and its home, the error word), the
counter, every written row and every row that must stay untouched, from start
counters 0 and 1000 and with cap 0, inside one wave's append, one short and
exact — for a probe chain across the table's end, lanes with 0, 1 and 3000
matches in one wave, the special keys, -1 rows, matches past the first trip
of the grid; and the cross product of the -1 rows, larger than one trip of its
emit kernel, cut by cap and behind a non-zero counter. Poison guards on both
sides of the table, the outputs, the counter and the error word.
"""
import os
import subprocess

import pytest

import cpp_programs

LIB = cpp_programs.LIB

# cases (one ": ok" line each) per set
SETS = {
    # ln x rn over {1, 63, 64, 65, 255, 256, 257}
    "sizes": 49,
    # the wrapping chain, the 3000-fold key, special keys, -1 on the probe side
    # and on both, matches past the first trip
    "edges": 6,
    # -1 counts (0, 5), (5, 0), (1, 1), (40, 25), (700, 800), and 3 x 4 past
    # the collect kernel's first trip
    "neg1": 6,
}
CASES = sum(SETS.values())


def _harness():
    return cpp_programs.build("table_join_check", include=("csrc",))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SETS))
def test_table_join_check(name):
    cases = SETS[name]
    r = subprocess.run([_harness(), "--set", name], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "join_table_slots: ok" in r.stdout
    assert "TABLE JOIN OK (%d cases)" % cases in r.stdout
    assert r.stdout.count(": ok\n") == cases + 1, r.stdout[-4000:]


@pytest.mark.skipif(not os.path.exists(LIB), reason="libdistjoin.so has not been built")
def test_table_join_check_inputs():
    """Host side of the harness alone: join_table_slots is the smallest power
    of two >= 2 ln + 1; the wrap chain crosses the table's end, the second
    key's home slot lies inside the 3000-row run, one wave holds lanes with 0,
    1 and 3000 matches, the cut caps fall inside a wave's append group, the
    trip cases have no match (no -1 row) in their first trip, the large cross
    product exceeds one trip of the emit kernel."""
    r = subprocess.run([_harness(), "--inputs-only"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "join_table_slots: ok" in r.stdout
    assert "TABLE JOIN INPUTS OK (%d cases)" % CASES in r.stdout
