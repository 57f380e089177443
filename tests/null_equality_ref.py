"""Host model of null_equality::UNEQUAL (a plain module, not a conftest), built
on the unchanged join_kinds_ref.ref_join by the strip identity:

    UNEQUAL(L, R) = EQUAL(L', R')  plus, for LEFT and LEFT_ANTI, the stripped
                                   left rows (LEFT: with null right-hand cells)

where L' and R' are the tables without the rows that hold a null in any column
of their key tuple. Once those rows are gone no key holds a null, so the
null == null of ref_join has nothing left to act on."""
import numpy as np

import join_kinds_ref as ref
from distributed_join_amd import NULL_EQUAL, NULL_UNEQUAL  # noqa: F401  (the modes modelled)
from join_kinds_ref import Col


def key_valid(table, on):
    """bool[n]: the rows with no null in any key column."""
    n = len(table[0]) if table else 0
    ok = np.ones(n, dtype=bool)
    for c in on:
        if table[c].valid is not None:
            ok &= table[c].valid
    return ok


def take(table, keep):
    """The rows of a list of Col where keep is True; masks stay where they were."""
    idx = np.flatnonzero(keep)
    out = []
    for c in table:
        vals = ([c.values[i] for i in idx] if isinstance(c.values, list)
                else np.asarray(c.values)[idx])
        out.append(Col(c.type_id, vals, None if c.valid is None else c.valid[idx]))
    return out


def ref_join_unequal(kind, left, right, lon, ron):
    """Join of the given kind under null_equality::UNEQUAL; sorted rows."""
    lok, rok = key_valid(left, lon), key_valid(right, ron)
    out = ref.ref_join(kind, take(left, lok), take(right, rok), lon, ron)
    null_rows = ref.host_rows(take(left, ~lok))
    if kind == ref.LEFT:
        out = out + [row + (None,) * len(right) for row in null_rows]
    elif kind == ref.LEFT_ANTI:
        out = out + null_rows
    return sorted(out, key=ref.row_key)


def run_join(dj, comm, kind, left, right, lon, ron, over_decom=1, null_equality=NULL_UNEQUAL):
    """The library's join on one rank under the given null equality -> (cols, masks)."""
    dl, dr = ref.Dev(dj, left), ref.Dev(dj, right)
    try:
        return dj.cpp_distributed_join_ncols_multi(
            comm, kind, dl.cols, len(left[0]), dr.cols, len(right[0]), lon, ron, over_decom,
            null_equality=null_equality)
    finally:
        dl.free()
        dr.free()
