"""Left outer, left semi and left anti joins on one rank, against the host
reference of tests/join_kinds_ref.py (sorted rows, None for a null cell).

Semantics under test (include/distributed_join.hpp): null keys join with
null == null; a LEFT join pads unmatched rows with null right-hand cells (zero
bytes, empty strings) and masks EVERY right-hand column, with an exact
null_count (checked against the mask whenever a table is read back); SEMI /
ANTI return the left columns only; left-hand columns have a mask exactly when
their source had one."""
import numpy as np
import pytest

import join_kinds_ref as ref
from join_kinds_ref import Col

pytestmark = pytest.mark.gpu

N = 2000
ALL_KINDS = ["inner", "left", "semi", "anti"]


@pytest.fixture(scope="module")
def dj():
    import distributed_join_amd as dj
    dj.require_gpu()
    return dj


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
    """Key columns first, then payloads of widths 1/2/4/8 and STRING on both
    sides; some nullable, the 4-byte (left) and 8-byte (right) ones mask-free."""
    nl, nr = len(lkeys[0]), len(rkeys[0])
    left = list(lkeys) + [
        Col(dj.TYPE_INT8, rng.randint(-128, 128, nl).astype(np.int8), rng.random_sample(nl) >= 0.3),
        Col(dj.TYPE_INT16, rng.randint(-3000, 3000, nl).astype(np.int16),
            rng.random_sample(nl) >= 0.5),
        Col(dj.TYPE_INT32, np.arange(nl, dtype=np.int32)),
        Col(dj.TYPE_INT64, rng.randint(-2 ** 62, 2 ** 62, nl).astype(np.int64),
            rng.random_sample(nl) >= 0.1),
        Col(dj.TYPE_STRING, _strings(rng, nl), rng.random_sample(nl) >= 0.2),
    ]
    right = list(rkeys) + [
        Col(dj.TYPE_UINT8, rng.randint(1, 256, nr).astype(np.uint8), rng.random_sample(nr) >= 0.4),
        Col(dj.TYPE_UINT16, rng.randint(1, 60000, nr).astype(np.uint16)),
        Col(dj.TYPE_UINT32, rng.randint(1, 2 ** 32, nr, dtype=np.uint64).astype(np.uint32),
            rng.random_sample(nr) >= 0.1),
        Col(dj.TYPE_INT64, np.arange(nr, dtype=np.int64) + 10 ** 6),
        Col(dj.TYPE_STRING, _strings(rng, nr), rng.random_sample(nr) >= 0.6),
    ]
    return left, right


def _check(dj, comm, kind_name, left, right, lon, ron, over_decom=1):
    kind = ref.KINDS[kind_name]
    want = ref.ref_join(kind, left, right, lon, ron)
    cols, masks = ref.run_join(dj, comm, kind, left, right, lon, ron, over_decom)
    nrows = ref.check_masks(kind, left, right, cols, masks)
    assert nrows == len(want), (kind_name, nrows, len(want))
    got = ref.rows(cols, masks)
    assert got == want, kind_name
    return cols, masks, want


# ------------------------------------------------------------------ key shapes

def _int64_keys(dj, rng):
    """Mask-free INT64 key, duplicates on both sides, about a third of the
    left keys absent on the right."""
    lk = rng.randint(0, 1500, N).astype(np.int64)
    rk = rng.randint(0, 1000, N).astype(np.int64)
    return [Col(dj.TYPE_INT64, lk)], [Col(dj.TYPE_INT64, rk)]


def _nullable_keys(dj, rng, nulls_left, nulls_right):
    """Nullable INT64 key (both sides carry a mask); the values stored under
    nulls are valid keys of the other side."""
    lk = rng.randint(0, 1500, N).astype(np.int64)
    rk = rng.randint(0, 1000, N).astype(np.int64)
    lvalid = rng.random_sample(N) >= (0.05 if nulls_left else 0.0)
    rvalid = rng.random_sample(N) >= (0.04 if nulls_right else 0.0)
    lnull, rnull = np.nonzero(~lvalid)[0], np.nonzero(~rvalid)[0]
    lk[lnull] = rk[rvalid][:len(lnull)]
    rk[rnull] = lk[lvalid][:len(rnull)]
    return [Col(dj.TYPE_INT64, lk, lvalid)], [Col(dj.TYPE_INT64, rk, rvalid)]


def _composite_keys(dj, rng):
    def side(hi):
        return [Col(dj.TYPE_INT32, rng.randint(0, hi, N).astype(np.int32),
                    rng.random_sample(N) >= 0.15),
                Col(dj.TYPE_STRING, _strings(rng, N, vocab=30), rng.random_sample(N) >= 0.15)]
    return side(60), side(40)


def _string_keys(dj, rng):
    words = _strings(rng, 900, vocab=900)
    lk = [words[i] for i in rng.randint(0, 900, N)]
    rk = [words[i] for i in rng.randint(0, 600, N)]
    return [Col(dj.TYPE_STRING, lk)], [Col(dj.TYPE_STRING, rk)]


def _minus_one_keys(dj, rng, on_right):
    lk = rng.randint(0, 1500, N).astype(np.int64)
    rk = rng.randint(0, 1000, N).astype(np.int64)
    lk[rng.randint(0, N, 25)] = -1
    if on_right:
        rk[rng.randint(0, N, 20)] = -1
    return [Col(dj.TYPE_INT64, lk)], [Col(dj.TYPE_INT64, rk)]


def _skewed_keys(dj, rng):
    """One value on 5000 rows of the build (left) side — more than a bucket
    holds, so the bucket path falls back — and twice on the right."""
    lk = np.concatenate([np.full(5000, 7), rng.randint(100, 1600, 1000)]).astype(np.int64)
    rng.shuffle(lk)
    rk = rng.randint(100, 1100, N).astype(np.int64)
    rk[[3, 1500]] = 7
    return [Col(dj.TYPE_INT64, lk)], [Col(dj.TYPE_INT64, rk)]


SHAPES = {
    "int64": lambda dj, rng: _int64_keys(dj, rng),
    "nullable_both": lambda dj, rng: _nullable_keys(dj, rng, True, True),
    "nullable_left_only": lambda dj, rng: _nullable_keys(dj, rng, True, False),
    "nullable_right_only": lambda dj, rng: _nullable_keys(dj, rng, False, True),
    "composite_int32_string": lambda dj, rng: _composite_keys(dj, rng),
    "string": lambda dj, rng: _string_keys(dj, rng),
    "minus_one_left": lambda dj, rng: _minus_one_keys(dj, rng, False),
    "minus_one_both": lambda dj, rng: _minus_one_keys(dj, rng, True),
    "skewed": lambda dj, rng: _skewed_keys(dj, rng),
}

_tables_cache = {}


def _tables(dj, shape):
    """Host tables of a key shape, built once and shared by the four kinds."""
    if shape not in _tables_cache:
        rng = np.random.RandomState(sorted(SHAPES).index(shape) + 100)
        lkeys, rkeys = SHAPES[shape](dj, rng)
        _tables_cache[shape] = _with_payloads(dj, rng, lkeys, rkeys) + (len(lkeys),)
    return _tables_cache[shape]


@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_join_kinds(dj, comm, shape, kind):
    left, right, nk = _tables(dj, shape)
    on = list(range(nk))
    _, _, want = _check(dj, comm, kind, left, right, on, on)
    if kind == "left":
        # the shape really has matched and unmatched rows: the right side's
        # mask-free INT64 payload is null exactly in a padded row
        pay = len(left) + nk + 3
        assert any(r[pay] is None for r in want) and any(r[pay] is not None for r in want)
    if kind in ("semi", "anti"):
        assert 0 < len(want) < len(left[0])
    if shape.startswith("nullable") and kind == "semi":
        nulls = sum(1 for r in want if r[0] is None)
        left_nulls = int((~left[0].valid).sum())
        right_has_null = bool((~right[0].valid).any())
        assert nulls == (left_nulls if right_has_null else 0)


def test_inner_through_new_entry_equals_existing(dj, comm):
    for shape in ("int64", "nullable_both", "composite_int32_string"):
        left, right, nk = _tables(dj, shape)
        on = list(range(nk))
        cols, masks = ref.run_join(dj, comm, ref.INNER, left, right, on, on)
        dl, dr = ref.Dev(dj, left), ref.Dev(dj, right)
        ocols, omasks = dj.cpp_distributed_inner_join_ncols_multi(
            comm, dl.cols, len(left[0]), dr.cols, len(right[0]), on, on)
        dl.free()
        dr.free()
        assert [m is None for m in masks] == [m is None for m in omasks]
        assert ref.rows(cols, masks) == ref.rows(ocols, omasks)


def test_left_every_row_matched(dj, comm):
    rng = np.random.RandomState(21)
    lk = rng.randint(0, 500, N).astype(np.int64)
    rk = np.concatenate([np.arange(500), rng.randint(0, 500, N - 500)]).astype(np.int64)
    left, right = _with_payloads(dj, rng, [Col(dj.TYPE_INT64, lk)], [Col(dj.TYPE_INT64, rk)])
    right = [Col(c.type_id, c.values) for c in right]  # no mask, no null on the right
    cols, masks, want = _check(dj, comm, "left", left, right, [0], [0])
    for m in masks[len(left):]:
        assert m is not None and m.all()  # masks present, null_count 0
    assert want == ref.ref_join(ref.INNER, left, right, [0], [0])
    icols, imasks = ref.run_join(dj, comm, ref.INNER, left, right, [0], [0])
    assert all(m is None for m in imasks[len(left):])
    assert ref.rows(icols, imasks) == want


def test_left_nothing_matches(dj, comm):
    rng = np.random.RandomState(22)
    lk = rng.randint(0, 500, N).astype(np.int64)
    rk = rng.randint(10 ** 6, 2 * 10 ** 6, N).astype(np.int64)
    left, right = _with_payloads(dj, rng, [Col(dj.TYPE_INT64, lk)], [Col(dj.TYPE_INT64, rk)])
    cols, masks, want = _check(dj, comm, "left", left, right, [0], [0])
    assert len(want) == N
    for c, m in zip(cols[len(left):], masks[len(left):]):
        assert m is not None and not m.any()  # every right cell null
        if isinstance(c, tuple):
            off, chars = c
            assert len(off) == N + 1 and not off.any() and len(chars) == 0
        else:
            assert len(c) == N and not c.any()  # the bytes under the nulls are zero


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_empty_sides(dj, comm, kind):
    left, right, _ = _tables(dj, "nullable_both")
    empty_l = [c.head(0) for c in left]
    empty_r = [c.head(0) for c in right]
    for l, r in ((empty_l, right), (left, empty_r), (empty_l, empty_r)):
        cols, masks, want = _check(dj, comm, kind, l, r, [0], [0])
        if kind in ("left", "anti"):
            assert len(want) == len(l[0])  # every left row, whatever the right side
        else:
            assert len(want) == 0


@pytest.mark.parametrize("kind", ["left", "semi", "anti"])
def test_two_int64_columns(dj, comm, kind):
    """2 x INT64 tables without masks: the shape whose inner join adopts the
    engine's outputs instead of gathering."""
    rng = np.random.RandomState(23)
    left = [Col(dj.TYPE_INT64, rng.randint(0, 1500, N).astype(np.int64)),
            Col(dj.TYPE_INT64, np.arange(N, dtype=np.int64))]
    right = [Col(dj.TYPE_INT64, rng.randint(0, 1000, N).astype(np.int64)),
             Col(dj.TYPE_INT64, np.arange(N, dtype=np.int64) + 10 ** 6)]
    _, _, want = _check(dj, comm, kind, left, right, [0], [0])
    assert 0 < len(want)


@pytest.mark.parametrize("kind", ["left", "semi", "anti"])
def test_over_decom_has_no_effect(dj, comm, kind):
    left, right, _ = _tables(dj, "int64")
    c1, m1, _ = _check(dj, comm, kind, left, right, [0], [0], over_decom=1)
    c4, m4, _ = _check(dj, comm, kind, left, right, [0], [0], over_decom=4)
    assert ref.rows(c1, m1) == ref.rows(c4, m4)
