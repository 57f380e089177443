"""null_equality::UNEQUAL on one rank, all four join kinds, against the host
model of tests/null_equality_ref.py (the strip identity over the unchanged
join_kinds_ref.ref_join; sorted rows, None for a null cell).

Semantics under test (include/distributed_join.hpp): a row with a null in any
column of its key tuple matches nothing; the values stored under a null are
never looked at (the tables put valid keys of the other side there); INNER and
LEFT_SEMI drop the null-key left rows, LEFT pads them, LEFT_ANTI keeps them;
null-key right rows are in no result; mask presence follows the kind's rule and
null counts are exact (checked against the masks whenever a table is read
back, and cell by cell through the compared rows)."""
import numpy as np
import pytest

import join_kinds_ref as ref
from join_kinds_ref import Col

pytestmark = pytest.mark.gpu

N = 3000
ALL_KINDS = ["inner", "left", "semi", "anti"]


@pytest.fixture(scope="module")
def dj():
    import distributed_join_amd as dj
    dj.require_gpu()
    return dj


@pytest.fixture(scope="module")
def ne(dj):
    import null_equality_ref
    return null_equality_ref


@pytest.fixture(scope="module")
def comm(dj):
    c = dj.CppCommunicator(0, 1)
    yield c
    c.destroy()


def _strings(rng, n, vocab=300):
    words = [bytes(rng.randint(97, 123, size=rng.randint(0, 12)).astype(np.uint8))
             for _ in range(vocab)]
    return [words[i] for i in rng.randint(0, vocab, n)]


def _with_payloads(dj, rng, lkeys, rkeys):
    """Key columns first, then nullable and mask-free payloads, fixed-width
    and STRING, on both sides."""
    nl, nr = len(lkeys[0]), len(rkeys[0])
    left = list(lkeys) + [
        Col(dj.TYPE_INT16, rng.randint(-3000, 3000, nl).astype(np.int16),
            rng.random_sample(nl) >= 0.5),
        Col(dj.TYPE_INT32, np.arange(nl, dtype=np.int32)),
        Col(dj.TYPE_STRING, _strings(rng, nl), rng.random_sample(nl) >= 0.2),
    ]
    right = list(rkeys) + [
        Col(dj.TYPE_UINT8, rng.randint(1, 256, nr).astype(np.uint8), rng.random_sample(nr) >= 0.4),
        Col(dj.TYPE_INT64, np.arange(nr, dtype=np.int64) + 10 ** 6),
        Col(dj.TYPE_STRING, _strings(rng, nr), rng.random_sample(nr) >= 0.6),
    ]
    return left, right


def _check(dj, ne, comm, kind_name, left, right, lon, ron, over_decom=1):
    kind = ref.KINDS[kind_name]
    want = ne.ref_join_unequal(kind, left, right, lon, ron)
    cols, masks = ne.run_join(dj, comm, kind, left, right, lon, ron, over_decom)
    nrows = ref.check_masks(kind, left, right, cols, masks)
    assert nrows == len(want), (kind_name, nrows, len(want))
    got = ref.rows(cols, masks)
    assert got == want, kind_name
    # exact null counts, column by column (the library's own counts were
    # checked against these masks when the table was read back)
    for c, m in enumerate(masks):
        if m is not None:
            assert int((~m).sum()) == sum(1 for r in want if r[c] is None), (kind_name, c)
    return cols, masks, want


# ------------------------------------------------------------------ key shapes

def _garbage_under_nulls(lk, lvalid, rk, rvalid):
    """The values under the nulls become valid keys of the other side."""
    lnull, rnull = np.flatnonzero(~lvalid), np.flatnonzero(~rvalid)
    if len(lnull) and rvalid.any():
        lk[lnull] = np.resize(rk[rvalid], len(lnull))
    if len(rnull) and lvalid.any():
        rk[rnull] = np.resize(lk[lvalid], len(rnull))


def _int_keys(dj, rng, type_id, dtype):
    """Single nullable integer key, about 20 % null on both sides, duplicates
    on both sides, about a third of the valid left keys absent on the right."""
    lk = rng.randint(0, 1500, N).astype(dtype)
    rk = rng.randint(0, 1000, N).astype(dtype)
    lvalid, rvalid = rng.random_sample(N) >= 0.2, rng.random_sample(N) >= 0.2
    _garbage_under_nulls(lk, lvalid, rk, rvalid)
    return [Col(type_id, lk, lvalid)], [Col(type_id, rk, rvalid)]


def _composite_keys(dj, rng):
    """(INT64, STRING) with about 10 % nulls in either element; the value
    under a null is drawn like any other, so it equals valid elements of the
    other side."""
    vocab = _strings(rng, 30, vocab=30)

    def side(hi):
        return [Col(dj.TYPE_INT64, rng.randint(0, hi, N).astype(np.int64),
                    rng.random_sample(N) >= 0.1),
                Col(dj.TYPE_STRING, [vocab[i] for i in rng.randint(0, 30, N)],
                    rng.random_sample(N) >= 0.1)]
    return side(60), side(40)


def _string_keys(dj, rng):
    words = _strings(rng, 900, vocab=900)
    lk = [words[i] for i in rng.randint(0, 900, N)]
    rk = [words[i] for i in rng.randint(0, 600, N)]   # the words under nulls are shared too
    return ([Col(dj.TYPE_STRING, lk, rng.random_sample(N) >= 0.2)],
            [Col(dj.TYPE_STRING, rk, rng.random_sample(N) >= 0.2)])


SHAPES = {
    "int64": lambda dj, rng: _int_keys(dj, rng, dj.TYPE_INT64, np.int64),
    "int32": lambda dj, rng: _int_keys(dj, rng, dj.TYPE_INT32, np.int32),
    "composite_int64_string": _composite_keys,
    "string": _string_keys,
}

_tables_cache = {}


def _tables(dj, shape):
    """Host tables of a key shape, built once and shared by the four kinds."""
    if shape not in _tables_cache:
        rng = np.random.RandomState(sorted(SHAPES).index(shape) + 400)
        lkeys, rkeys = SHAPES[shape](dj, rng)
        _tables_cache[shape] = _with_payloads(dj, rng, lkeys, rkeys) + (len(lkeys),)
    return _tables_cache[shape]


@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_unequal(dj, ne, comm, shape, kind):
    left, right, nk = _tables(dj, shape)
    on = list(range(nk))
    _, _, want = _check(dj, ne, comm, kind, left, right, on, on)
    lnull = int((~ne.key_valid(left, on)).sum())
    assert 0 < lnull < N and 0 < int((~ne.key_valid(right, on)).sum()) < N
    null_key_rows = sum(1 for r in want if any(r[c] is None for c in on))
    if kind in ("inner", "semi"):
        assert null_key_rows == 0 and 0 < len(want)
    else:
        assert null_key_rows == lnull            # each exactly once
    if kind == "left":
        # matched, unmatched-valid and null-key rows are all there: the right
        # side's mask-free INT64 payload is null exactly in a padded row
        pay = len(left) + nk + 1
        assert lnull < sum(1 for r in want if r[pay] is None) < len(want)
    # and the mode matters on these tables
    assert want != ref.ref_join(ref.KINDS[kind], left, right, on, on)


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_over_decom_gives_the_same_rows(dj, ne, comm, kind):
    left, right, _ = _tables(dj, "int64")
    c1, m1, _ = _check(dj, ne, comm, kind, left, right, [0], [0], over_decom=1)
    c4, m4, _ = _check(dj, ne, comm, kind, left, right, [0], [0], over_decom=4)
    assert ref.rows(c1, m1) == ref.rows(c4, m4)


# ------------------------------------------------------------------ edge cases

@pytest.mark.parametrize("kind", ALL_KINDS)
def test_tuple_with_a_null_element(dj, ne, comm, kind):
    """(a, null) on both sides with equal a: a match under EQUAL, none under
    UNEQUAL. The strings under the nulls are equal too."""
    i64, s = dj.TYPE_INT64, dj.TYPE_STRING
    left = [Col(i64, np.array([5, 5, 6, 7], dtype=np.int64), [True, True, True, False]),
            Col(s, [b"x", b"y", b"z", b"y"], [False, True, True, True]),
            Col(i64, np.arange(4, dtype=np.int64))]
    right = [Col(i64, np.array([5, 5, 6, 7], dtype=np.int64), [True, True, True, False]),
             Col(s, [b"x", b"y", b"q", b"y"], [False, True, True, True]),
             Col(i64, np.arange(4, dtype=np.int64) + 100)]
    k = ref.KINDS[kind]
    cols, masks = ne.run_join(dj, comm, k, left, right, [0, 1], [0, 1],
                              null_equality=dj.NULL_EQUAL)
    equal = ref.rows(cols, masks)
    assert equal == ref.ref_join(k, left, right, [0, 1], [0, 1])
    _, _, unequal = _check(dj, ne, comm, kind, left, right, [0, 1], [0, 1])
    if kind == "inner":
        assert (5, None, 0, 5, None, 100) in equal and (None, b"y", 3, None, b"y", 103) in equal
        assert unequal == [(5, b"y", 1, 5, b"y", 101)]
    if kind == "anti":
        assert equal == [(6, b"z", 2)]
        assert unequal == [(None, b"y", 3), (5, None, 0), (6, b"z", 2)]


@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("where", ["left", "right", "both"])
def test_all_null_key_column(dj, ne, comm, kind, where):
    left, right, _ = _tables(dj, "int64")
    none = np.zeros(N, dtype=bool)
    if where in ("left", "both"):
        left = [Col(left[0].type_id, left[0].values, none)] + left[1:]
    if where in ("right", "both"):
        right = [Col(right[0].type_id, right[0].values, none)] + right[1:]
    _, _, want = _check(dj, ne, comm, kind, left, right, [0], [0])
    assert len(want) == {"inner": 0, "semi": 0, "left": N, "anti": N}[kind]


@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("masks", ["present_without_nulls", "absent"])
def test_no_null_key_equals_the_equal_join(dj, ne, comm, kind, masks):
    left, right, _ = _tables(dj, "int64")
    valid = np.ones(N, dtype=bool) if masks == "present_without_nulls" else None
    left = [Col(left[0].type_id, left[0].values, valid)] + left[1:]
    right = [Col(right[0].type_id, right[0].values, valid)] + right[1:]
    _, _, want = _check(dj, ne, comm, kind, left, right, [0], [0])
    k = ref.KINDS[kind]
    cols, emasks = ne.run_join(dj, comm, k, left, right, [0], [0], null_equality=dj.NULL_EQUAL)
    assert ref.rows(cols, emasks) == want == ref.ref_join(k, left, right, [0], [0])


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_minus_one_keys(dj, ne, comm, kind):
    """The sentinel value -1 is a key like any other when valid, and nothing
    when it sits under a null."""
    rng = np.random.RandomState(41)
    lk = rng.randint(0, 1500, N).astype(np.int64)
    rk = rng.randint(0, 1000, N).astype(np.int64)
    lvalid, rvalid = rng.random_sample(N) >= 0.2, rng.random_sample(N) >= 0.2
    _garbage_under_nulls(lk, lvalid, rk, rvalid)
    lk[:40] = -1
    rk[:30] = -1
    lvalid[:40] = np.arange(40) % 2 == 0        # 20 valid -1 keys, 20 under a null
    rvalid[:30] = np.arange(30) % 3 == 0        # 10 valid, 20 under a null
    left, right = _with_payloads(dj, rng, [Col(dj.TYPE_INT64, lk, lvalid)],
                                 [Col(dj.TYPE_INT64, rk, rvalid)])
    _, _, want = _check(dj, ne, comm, kind, left, right, [0], [0])
    minus_one = sum(1 for r in want if r[0] == -1)
    assert minus_one == {"inner": 200, "left": 200, "semi": 20, "anti": 0}[kind]


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_empty_sides(dj, ne, comm, kind):
    left, right, _ = _tables(dj, "int64")
    empty_l = [c.head(0) for c in left]
    empty_r = [c.head(0) for c in right]
    for l, r in ((empty_l, right), (left, empty_r), (empty_l, empty_r)):
        _, _, want = _check(dj, ne, comm, kind, l, r, [0], [0])
        if kind in ("left", "anti"):
            assert len(want) == len(l[0])       # every left row, whatever the right side
        else:
            assert len(want) == 0


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_many_null_keys_stay_out_of_the_bucket_join(dj, ne, comm, kind):
    """60 000 null-key rows a side, one value under all of them, plus 1 000
    valid rows. Under EQUAL these tables need 3.6e9 output rows, so a result
    at all means the null rows never met in the engine."""
    rng = np.random.RandomState(42)
    nn, nv = 60_000, 1_000

    def side(base):
        keys = np.concatenate([np.full(nn, 7), rng.randint(0, 400, nv)]).astype(np.int64)
        valid = np.concatenate([np.zeros(nn, dtype=bool), np.ones(nv, dtype=bool)])
        order = rng.permutation(nn + nv)
        return [Col(dj.TYPE_INT64, keys[order], valid[order]),
                Col(dj.TYPE_INT64, np.arange(nn + nv, dtype=np.int64) + base)]
    left, right = side(0), side(10 ** 6)
    _, _, want = _check(dj, ne, comm, kind, left, right, [0], [0])
    valid_rows = [r for r in want if r[0] is not None]
    assert valid_rows == ne.ref_join_unequal(
        ref.KINDS[kind], ne.take(left, left[0].valid), ne.take(right, right[0].valid), [0], [0])
    assert len(want) - len(valid_rows) == (nn if kind in ("left", "anti") else 0)


def test_out_of_range_null_equality_raises(dj, ne, comm):
    left, right, _ = _tables(dj, "int64")
    for bad in (2, -1, 7):
        with pytest.raises(ValueError):
            ne.run_join(dj, comm, ref.INNER, left, right, [0], [0], null_equality=bad)
