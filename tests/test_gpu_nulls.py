"""Nullable columns: the validity-mask kernels through their hooks, world-1
joins / shuffles / partitions over nullable column descriptors, and the
multi-rank loopback program.

Semantics under test (include/dj_cudf_types.hpp, csrc/dj_hash.h): cuDF mask
layout; null keys join with null == null (cudf::inner_join's default
null_equality::EQUAL, reference distributed_join.cpp:79); a null key element
places on the element hash 0xFFFFFFFF; values under a null are never compared
or hashed; an output column has a mask exactly when its source had one and its
null_count is exact.

Every expected result comes from the numpy / dict references in this file.
"""
import os
import subprocess
from collections import defaultdict

import numpy as np
import pytest

import cpp_programs

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_HASH = 0xFFFFFFFF


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


# ------------------------------------------------------------ gather kernel

GATHER_N = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4097]


def _source_masks(rng, n_src, ncols):
    """ncols host bool arrays cycling: no mask, all-null, alternating, ~10% null."""
    out = []
    for c in range(ncols):
        kind = c % 4
        if kind == 0:
            out.append(None)
        elif kind == 1:
            out.append(np.zeros(n_src, dtype=bool))
        elif kind == 2:
            out.append((np.arange(n_src) % 2 == (c // 4) % 2))
        else:
            out.append(rng.random_sample(n_src) >= 0.10)
    return out


@pytest.mark.parametrize("n", GATHER_N)
def test_gather_bitmasks(dj, n):
    rng = np.random.RandomState(1000 + n)
    n_src = n + 37  # the source table is not the size of the output
    idx = rng.randint(0, n_src, size=n).astype(np.int64)  # random, with repeats
    if n > 2:
        idx[1] = idx[0]
        idx[-1] = n_src - 1
    d_idx = dj.DeviceArray.from_numpy(idx)
    for ncols in (1, 3, 32):
        host = _source_masks(rng, n_src, ncols)
        if ncols == 1:
            host = [rng.random_sample(n_src) >= 0.10]
        dev = [None if h is None else dj.upload_mask(h) for h in host]
        # the engine's launch grouping, all columns in one launch, and 5 per launch
        for per_launch in sorted({0, ncols, min(ncols, 5)}):
            outs, counts, _, raws = dj.gather_bitmasks(
                [None if d is None else d.ptr for d in dev], d_idx.ptr, n,
                cols_per_launch=per_launch)
            for c in range(ncols):
                want = np.ones(n, dtype=bool) if host[c] is None else host[c][idx]
                assert (outs[c] == want).all(), (n, ncols, c, per_launch)
                assert counts[c] == n - int(want.sum()), (n, ncols, c, per_launch)
                # bits [n, roundup(n, 64)) are written as 0
                tail = dj.unpack_mask(raws[c], len(raws[c]) * 32)[n:]
                assert not tail.any(), (n, ncols, c, per_launch)
        for d in dev:
            if d is not None:
                d.free()
    d_idx.free()


# -------------------------------------------------------- segment copy kernel

class _Source:
    """Device copy of a bit array whose first and last words are guard words
    holding the COMPLEMENT of the neighbouring payload bits: `ptr` points at
    the payload, so a read of a word outside the payload is in bounds but
    brings in wrong bits."""

    def __init__(self, dj, bits):
        self.dj = dj
        self.bits = np.asarray(bits, dtype=bool)
        nwords = (len(self.bits) + 31) // 32
        padded = np.zeros(nwords * 32, dtype=bool)
        padded[:len(self.bits)] = self.bits
        # unused bits of the last payload word: complement of the last bit
        if len(self.bits) % 32:
            padded[len(self.bits):] = not self.bits[-1]
        words = np.packbits(padded, bitorder="little").view(np.uint32)
        lead = np.uint32(0 if self.bits[0] else 0xFFFFFFFF)
        trail = np.uint32(0 if padded[-1] else 0xFFFFFFFF)
        buf = np.concatenate([[lead], words, [trail]]).astype(np.uint32)
        self.base = dj.lib().dj_dmalloc(buf.nbytes)
        dj.lib().dj_memcpy_h2d(self.base, buf.ctypes.data, buf.nbytes)
        self.ptr = self.base + 4

    def free(self):
        self.dj.lib().dj_dfree(self.base)


def _check_segments(dj, segments, sources):
    """segments: (source index or None, src_bit, nbits)."""
    want = []
    for s, sb, nb in segments:
        want.append(np.ones(nb, dtype=bool) if s is None else sources[s].bits[sb:sb + nb])
    want = np.concatenate(want) if want else np.zeros(0, dtype=bool)
    words, got, nulls = dj.copy_bitmask_segments(
        [(None if s is None else sources[s].ptr, sb, nb) for s, sb, nb in segments],
        fill=0x5A5A5A5A)
    assert len(got) == len(want)
    assert (got == want).all(), np.nonzero(got != want)[0][:10]
    assert nulls == len(want) - int(want.sum())
    # whole words are written: the bits past the total are 0
    assert not dj.unpack_mask(words, len(words) * 32)[len(want):].any()


@pytest.mark.parametrize("length", [0, 1, 31, 32, 33, 64, 100])
def test_copy_segments_all_offsets(dj, length):
    """Source bit offsets 0..63 against destination bit offsets 0..63: each
    tested segment follows a filler that moves the destination position to the
    wanted offset (mod 64). The sources end exactly with the last segment that
    reads them."""
    rng = np.random.RandomState(7 + length)
    src = _Source(dj, rng.random_sample(63 + max(length, 1)) >= 0.5)
    segments = []
    pos = 0
    for so in range(64):
        for do in range(64):
            fill = (do - pos) % 64
            segments.append((None, 0, fill))
            segments.append((0, so, length))
            pos += fill + length
    _check_segments(dj, segments, [src])
    src.free()


def test_copy_segments_many_in_one_word(dj):
    """Eight 3-bit segments (eight peers sending 3 rows each) share one word."""
    rng = np.random.RandomState(3)
    srcs = [_Source(dj, rng.random_sample(3 + k) >= 0.5) for k in range(8)]
    _check_segments(dj, [(k, k, 3) for k in range(8)], srcs)
    # and the same behind a 29-bit slice, straddling a word boundary
    _check_segments(dj, [(None, 0, 29)] + [(k, k, 3) for k in range(8)], srcs)
    for s in srcs:
        s.free()


def test_copy_segments_zero_length_and_null_sources(dj):
    rng = np.random.RandomState(5)
    a = _Source(dj, rng.random_sample(100) >= 0.3)
    b = _Source(dj, np.zeros(40, dtype=bool))  # all null
    segments = [(0, 5, 0), (None, 0, 0),                # zero length first
                (0, 0, 100), (None, 0, 7), (1, 3, 37),
                (0, 50, 0), (1, 0, 0), (None, 0, 0),    # ... in the middle
                (None, 0, 33), (1, 0, 40), (0, 99, 1), (None, 0, 64), (0, 31, 33),
                (0, 100, 0), (None, 0, 0)]              # ... and last
    _check_segments(dj, segments, [a, b])
    _check_segments(dj, [(0, 0, 0)], [a])  # nothing at all
    _check_segments(dj, [(0, 7, 0), (1, 39, 1), (0, 0, 0)], [a, b])
    a.free()
    b.free()


# ------------------------------------------------------- tables and references

class _Col:
    """Host column: values (numpy array, or list of bytes for STRING), valid
    (bool array, or None = no mask)."""

    def __init__(self, type_id, values, valid=None):
        self.type_id = type_id
        self.values = values
        self.valid = None if valid is None else np.asarray(valid, dtype=bool)

    def cell(self, i):
        if self.valid is not None and not self.valid[i]:
            return None
        v = self.values[i]
        return v if isinstance(v, bytes) else v.item()


class _Dev:
    """Device copy of a list of _Col; .cols are the nullable descriptors."""

    def __init__(self, dj, cols):
        self.dj = dj
        self.cols, self.plain, self._fixed, self._raw, self._masks = [], [], [], [], []
        for c in cols:
            if c.type_id == dj.TYPE_STRING:
                off, ch, nb = dj.upload_strings(list(c.values))
                self._raw += [off, ch]
                desc = (dj.TYPE_STRING, off, ch, nb)
            else:
                d = dj.upload_column(np.asarray(c.values), c.type_id)
                self._fixed.append(d)
                desc = d.desc
            self.plain.append(desc)
            if c.valid is None:
                self.cols.append(desc)
            else:
                m = dj.upload_mask(c.valid)
                self._masks.append(m)
                self.cols.append(desc + (m,))

    def free(self):
        for d in self._fixed + self._masks:
            d.free()
        for p in self._raw:
            self.dj.lib().dj_dfree(p)


def _decode(col):
    off, ch = col
    raw = ch.tobytes()
    return [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _row_key(row):
    """Total order over rows whose cells are None, bytes or numbers."""
    return tuple((0, b"", 0) if x is None else
                 ((1, x, 0) if isinstance(x, bytes) else (2, b"", x)) for x in row)


def _rows(cols, masks):
    """Output table -> sorted list of row tuples, None for a null cell."""
    lists = []
    for c, m in zip(cols, masks):
        vals = _decode(c) if isinstance(c, tuple) else c.tolist()
        if m is not None:
            vals = [v if ok else None for v, ok in zip(vals, m)]
        lists.append(vals)
    n = len(lists[0]) if lists else 0
    return sorted((tuple(l[i] for l in lists) for i in range(n)), key=_row_key)


def _ref_join(left, right, lon, ron):
    """Inner join, null == null (None == None as a dict key). Sorted rows."""
    n_l = len(left[0].values)
    n_r = len(right[0].values)
    lrows = [tuple(c.cell(i) for c in left) for i in range(n_l)]
    rrows = [tuple(c.cell(j) for c in right) for j in range(n_r)]
    index = defaultdict(list)
    for i, row in enumerate(lrows):
        index[tuple(row[c] for c in lon)].append(i)
    out = []
    for row in rrows:
        for i in index.get(tuple(row[c] for c in ron), ()):
            out.append(lrows[i] + row)
    return sorted(out, key=_row_key)


def _join(dj, comm, left, right, lon, ron, over_decom=1):
    dl, dr = _Dev(dj, left), _Dev(dj, right)
    try:
        cols, masks = dj.cpp_distributed_inner_join_ncols_multi(
            comm, dl.cols, len(left[0].values), dr.cols, len(right[0].values), lon, ron,
            over_decom)
    finally:
        dl.free()
        dr.free()
    # a mask exactly where the source column had one
    for m, c in zip(masks, list(left) + list(right)):
        assert (m is not None) == (c.valid is not None)
    return cols, masks


N_ROWS = 2000


def _strings(rng, n, vocab=300):
    words = [bytes(rng.randint(97, 123, size=rng.randint(0, 12)).astype(np.uint8))
             for _ in range(vocab)]
    return [words[i] for i in rng.randint(0, vocab, n)]


@pytest.fixture(scope="module")
def key_tables():
    """left/right host tables, ~2000 rows each: nullable INT64 key with nulls
    on both sides, whose stored values are keys that are VALID on the other
    side, and -1; nullable payloads of widths 1/2/4/8 and STRING; one
    mask-free column per side."""
    rng = np.random.RandomState(42)
    n = N_ROWS
    lk = rng.randint(0, 1500, n).astype(np.int64)
    rk = rng.randint(0, 1500, n).astype(np.int64)
    lk[rng.randint(0, n, 20)] = -1  # valid -1 keys: the engine's sentinel value
    rk[rng.randint(0, n, 20)] = -1
    lvalid = rng.random_sample(n) >= 0.05
    rvalid = rng.random_sample(n) >= 0.04
    # garbage under nulls: a valid key of the other side, or -1
    lnull, rnull = np.nonzero(~lvalid)[0], np.nonzero(~rvalid)[0]
    lk[lnull] = np.where(np.arange(len(lnull)) % 2 == 0, rk[rvalid][:len(lnull)], -1)
    rk[rnull] = np.where(np.arange(len(rnull)) % 2 == 0, lk[lvalid][:len(rnull)], -1)
    import distributed_join_amd as dj
    left = [
        _Col(dj.TYPE_INT64, lk, lvalid),
        _Col(dj.TYPE_INT64, np.arange(n, dtype=np.int64)),
        _Col(dj.TYPE_INT8, rng.randint(-128, 128, n).astype(np.int8), rng.random_sample(n) >= 0.3),
        _Col(dj.TYPE_INT16, rng.randint(-3000, 3000, n).astype(np.int16),
             rng.random_sample(n) >= 0.5),
        _Col(dj.TYPE_STRING, _strings(rng, n), rng.random_sample(n) >= 0.2),
    ]
    right = [
        _Col(dj.TYPE_INT64, rk, rvalid),
        _Col(dj.TYPE_UINT32, rng.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32),
             rng.random_sample(n) >= 0.1),
        _Col(dj.TYPE_INT64, rng.randint(-2 ** 62, 2 ** 62, n).astype(np.int64),
             rng.random_sample(n) >= 0.6),
        _Col(dj.TYPE_INT32, np.arange(n, dtype=np.int32)),
    ]
    return left, right


def test_join_nullable_key_both_sides(dj, comm, key_tables):
    left, right = key_tables
    want = _ref_join(left, right, [0], [0])
    a, b = int((~left[0].valid).sum()), int((~right[0].valid).sum())
    assert a > 50 and b > 50
    # the reference itself holds the a*b cross product of the null keys
    assert sum(1 for r in want if r[0] is None) == a * b
    cols, masks = _join(dj, comm, left, right, [0], [0])
    got = _rows(cols, masks)
    assert len(got) == len(want)
    assert sum(1 for r in got if r[0] is None and r[5] is None) == a * b
    assert got == want


def test_join_null_key_one_side_only(dj, comm, key_tables):
    left, right = key_tables
    # right keeps its mask but marks nothing null; its values stay what they
    # were, the former garbage (valid keys, -1) included
    right2 = [_Col(right[0].type_id, right[0].values, np.ones(N_ROWS, dtype=bool))] + right[1:]
    want = _ref_join(left, right2, [0], [0])
    assert not any(r[0] is None for r in want)
    cols, masks = _join(dj, comm, left, right2, [0], [0])
    got = _rows(cols, masks)
    assert got == want
    assert masks[0].all() and masks[5].all()  # no null key in the output


def test_mask_without_nulls_equals_no_mask(dj, comm, key_tables):
    """A mask that marks no row null: same join rows as the mask-free entry
    point, and the same partition offsets and row order."""
    left, right = key_tables
    n = N_ROWS
    allv = np.ones(n, dtype=bool)
    lm = [_Col(c.type_id, c.values, allv) for c in left]
    rm = [_Col(c.type_id, c.values, allv) for c in right]
    cols, masks = _join(dj, comm, lm, rm, [0], [0])
    assert all(m.all() for m in masks)
    dl = _Dev(dj, [_Col(c.type_id, c.values) for c in left])
    dr = _Dev(dj, [_Col(c.type_id, c.values) for c in right])
    plain = dj.cpp_distributed_inner_join_cols_multi(comm, dl.plain, n, dr.plain, n, [0], [0])
    assert _rows(cols, masks) == _rows(plain, [None] * len(plain))
    dr.free()
    dm = _Dev(dj, lm)
    for hash_fn in (dj.HASH_MURMUR3, dj.HASH_IDENTITY):
        for on in ([0], [0, 3]):
            if hash_fn == dj.HASH_IDENTITY and len(on) > 1:
                continue
            want_cols, want_off = dj.cpp_partition_cols(dl.plain, n, on, 7, hash_fn, 99)
            (got_cols, got_masks), got_off = dj.cpp_partition_ncols(dm.cols, n, on, 7, hash_fn, 99)
            assert (got_off == want_off).all()
            assert all(m.all() for m in got_masks)
            for g, w in zip(got_cols, want_cols):
                if isinstance(g, tuple):
                    assert _decode(g) == _decode(w)
                else:
                    assert (g == w).all()
    dl.free()
    dm.free()


def test_join_composite_nullable_int32_string(dj, comm):
    rng = np.random.RandomState(77)
    n = N_ROWS

    def side(seed_shift):
        k1 = rng.randint(0, 40, n).astype(np.int32)
        k2 = _strings(rng, n, vocab=30)
        return [
            _Col(dj.TYPE_INT32, k1, rng.random_sample(n) >= 0.15),
            _Col(dj.TYPE_STRING, k2, rng.random_sample(n) >= 0.15),
            _Col(dj.TYPE_INT64, np.arange(n, dtype=np.int64) + seed_shift),
            _Col(dj.TYPE_UINT8, rng.randint(0, 256, n).astype(np.uint8),
                 rng.random_sample(n) >= 0.5),
        ]
    left, right = side(0), side(10 ** 6)
    want = _ref_join(left, right, [0, 1], [0, 1])
    # all four validity combinations of the key tuple occur among the matches
    combos = {(r[0] is None, r[1] is None) for r in want}
    assert combos == {(False, False), (False, True), (True, False), (True, True)}
    cols, masks = _join(dj, comm, left, right, [0, 1], [0, 1])
    assert _rows(cols, masks) == want


def test_join_empty_sides(dj, comm, key_tables):
    left, right = key_tables
    empty_l = [_Col(c.type_id, c.values[:0], None if c.valid is None else c.valid[:0])
               for c in left]
    empty_r = [_Col(c.type_id, c.values[:0], None if c.valid is None else c.valid[:0])
               for c in right]
    for l, r in ((empty_l, right), (left, empty_r), (empty_l, empty_r)):
        cols, masks = _join(dj, comm, l, r, [0], [0])
        assert len(cols) == len(left) + len(right)
        assert all(len(c[0]) == 1 if isinstance(c, tuple) else len(c) == 0 for c in cols)
        assert all(m is None or len(m) == 0 for m in masks)


def test_join_and_partition_33_nullable_columns(dj, comm):
    """More nullable columns than one mask-gather descriptor holds (32): 33
    nullable payloads of mixed widths plus a nullable key, through the world-1
    join and the partition hook."""
    rng = np.random.RandomState(33)
    n = 300
    types = [(dj.TYPE_INT8, np.int8), (dj.TYPE_INT16, np.int16), (dj.TYPE_INT32, np.int32),
             (dj.TYPE_INT64, np.int64)]
    left = [_Col(dj.TYPE_INT64, rng.randint(0, 200, n).astype(np.int64),
                 rng.random_sample(n) >= 0.1),
            _Col(dj.TYPE_INT64, np.arange(n, dtype=np.int64))]
    for c in range(33):
        t, dt = types[c % 4]
        left.append(_Col(t, rng.randint(-100, 100, n).astype(dt),
                         rng.random_sample(n) >= (c + 1) / 40.0))
    right = [_Col(dj.TYPE_INT64, rng.randint(0, 200, n).astype(np.int64),
                  rng.random_sample(n) >= 0.1),
             _Col(dj.TYPE_INT32, np.arange(n, dtype=np.int32), rng.random_sample(n) >= 0.5)]
    assert sum(c.valid is not None for c in left) == 34
    want = _ref_join(left, right, [0], [0])
    cols, masks = _join(dj, comm, left, right, [0], [0])
    assert _rows(cols, masks) == want
    d = _Dev(dj, left)
    (pcols, pmasks), off = dj.cpp_partition_ncols(d.cols, n, [0], 5, dj.HASH_MURMUR3, 3)
    d.free()
    ids = pcols[1]
    assert sorted(ids.tolist()) == list(range(n))
    for c, col in enumerate(left):
        assert (pcols[c] == np.asarray(col.values)[ids]).all(), c
        if col.valid is None:
            assert pmasks[c] is None
        else:
            assert (pmasks[c] == col.valid[ids]).all(), c


def test_join_nonnull_key_nullable_payloads_over_decom(dj, comm, key_tables):
    """A mask-free key with nullable payloads and over_decom_factor 4. One rank
    joins locally whatever the factor; the batched pipeline itself runs with
    masks in the loopback program (over_decom_factor 2, 2-8 ranks)."""
    left, right = key_tables
    l2 = [_Col(left[0].type_id, left[0].values)] + left[1:]
    r2 = [_Col(right[0].type_id, right[0].values)] + right[1:]
    want = _ref_join(l2, r2, [0], [0])
    cols, masks = _join(dj, comm, l2, r2, [0], [0], over_decom=4)
    assert masks[0] is None and masks[len(left)] is None
    assert _rows(cols, masks) == want


# ------------------------------------------------------- shuffle and placement

def _murmur3_int64(keys, seed):
    """dj_murmur3_int64 of csrc/dj_hash.h, vectorised."""
    u = np.asarray(keys).astype(np.int64).view(np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    h = np.full(len(u), seed, dtype=np.uint64)
    for blk in (u & m32, u >> np.uint64(32)):
        k = (blk * np.uint64(0xCC9E2D51)) & m32
        k = ((k << np.uint64(15)) | (k >> np.uint64(17))) & m32
        k = (k * np.uint64(0x1B873593)) & m32
        h ^= k
        h = ((h << np.uint64(13)) | (h >> np.uint64(19))) & m32
        h = (h * np.uint64(5) + np.uint64(0xE6546B64)) & m32
    h ^= np.uint64(8)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m32
    h ^= h >> np.uint64(16)
    return h


def _mix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def _partition_of_rowid(cols, offsets, rowid_col):
    part = {}
    ids = cols[rowid_col]
    for p in range(len(offsets) - 1):
        for r in ids[offsets[p]:offsets[p + 1]].tolist():
            part[r] = p
    return part


def test_shuffle_world1_keeps_null_rows_in_place(dj, comm, key_tables):
    left, _ = key_tables
    d = _Dev(dj, left)
    cols, masks = dj.cpp_shuffle_on_ncols(comm, d.cols, N_ROWS, [0], dj.HASH_MURMUR3, 5)
    plain = dj.cpp_shuffle_on_cols(comm, d.plain, N_ROWS, [0], dj.HASH_MURMUR3, 5)
    d.free()
    # one rank: the stable placement leaves every row, null keys included,
    # where it was; values (also those under nulls) move as bytes
    for c, (g, w) in enumerate(zip(cols, plain)):
        if isinstance(g, tuple):
            assert _decode(g) == _decode(w)
        else:
            assert (g == w).all()
        if left[c].valid is None:
            assert masks[c] is None
        else:
            assert (masks[c] == left[c].valid).all()


@pytest.mark.parametrize("hash_name", ["murmur3", "identity"])
def test_partition_places_valid_rows_as_before_and_nulls_on_null_hash(dj, key_tables, hash_name):
    left, _ = key_tables
    hash_fn = dj.HASH_MURMUR3 if hash_name == "murmur3" else dj.HASH_IDENTITY
    nparts, seed = 7, 12345678
    d = _Dev(dj, left)
    (cols, masks), off = dj.cpp_partition_ncols(d.cols, N_ROWS, [0], nparts, hash_fn, seed)
    pcols, poff = dj.cpp_partition_cols(d.plain, N_ROWS, [0], nparts, hash_fn, seed)
    d.free()
    got = _partition_of_rowid(cols, off, 1)
    before = _partition_of_rowid(pcols, poff, 1)
    valid = left[0].valid
    assert len(got) == N_ROWS
    for r in range(N_ROWS):
        if valid[r]:
            assert got[r] == before[r]
        else:
            assert got[r] == NULL_HASH % nparts
    # and the spec itself for the valid rows
    keys = left[0].values
    h = _murmur3_int64(keys, seed) if hash_name == "murmur3" else \
        keys.view(np.uint64) & np.uint64(0xFFFFFFFF)
    want = (h % np.uint64(nparts)).astype(np.int64)
    assert all(got[r] == want[r] for r in range(N_ROWS) if valid[r])
    # rows keep their input order inside a partition, validity rides along
    ids = cols[1]
    for p in range(nparts):
        seg = ids[off[p]:off[p + 1]]
        assert (np.diff(seg) > 0).all()
    assert (masks[0] == valid[ids]).all()
    assert (masks[2] == left[2].valid[ids]).all()


def test_partition_fused_chain_uses_null_hash(dj):
    """Composite key (nullable INT32, INT64): a null element enters the chain
    h = mix64(h ^ v) as v = 0xFFFFFFFF (csrc/dj_hash.h)."""
    rng = np.random.RandomState(9)
    n, nparts, seed = 1500, 5, 777
    k1 = rng.randint(-50, 50, n).astype(np.int32)
    k2 = rng.randint(0, 1000, n).astype(np.int64)
    valid = rng.random_sample(n) >= 0.3
    k1[~valid] = 17  # garbage under the nulls
    cols = [_Col(dj.TYPE_INT32, k1, valid), _Col(dj.TYPE_INT64, k2),
            _Col(dj.TYPE_INT64, np.arange(n, dtype=np.int64))]
    d = _Dev(dj, cols)
    (out, masks), off = dj.cpp_partition_ncols(d.cols, n, [0, 1], nparts, dj.HASH_MURMUR3, seed)
    d.free()
    v1 = np.where(valid, k1.astype(np.int64), np.int64(NULL_HASH)).view(np.uint64)
    h = np.full(n, 0x9E3779B97F4A7C15, dtype=np.uint64)
    h = _mix64(h ^ v1)
    h = _mix64(h ^ k2.view(np.uint64))
    want = (_murmur3_int64(h.view(np.int64), seed) % np.uint64(nparts)).astype(np.int64)
    got = _partition_of_rowid(out, off, 2)
    assert all(got[r] == want[r] for r in range(n))


# --------------------------------------------------------------- multi-rank

# send/recv calls and bytes of the mask-free part of tests/cpp/null_loopback.cpp
# (its "COUNTS" line), recorded from the commit before validity masks
# existed: (G, rows per rank) -> (sends, recvs, send_bytes, recv_bytes, rows)
COUNTS_BEFORE_MASKS = {
    (2, 5): (98, 98, 17154, 17154, 64),
    (3, 5): (294, 294, 26389, 26389, 120),
    (8, 5): (2744, 2744, 125092, 125092, 378),
    (2, 1000): (98, 98, 122105, 122105, 16134),
    (3, 1000): (294, 294, 243585, 243585, 24358),
    (8, 1000): (2744, 2744, 877642, 877642, 63792),
}


@pytest.mark.parametrize("G,rows", [(2, 5), (3, 5), (8, 5), (2, 1000), (3, 1000), (8, 1000)])
def test_null_loopback(dj, G, rows):
    """G ranks as threads over a counting loopback Communicator
    (tests/cpp/null_loopback.cpp): shuffle and joins of nullable tables against
    a host reference, one rank passing a column without a mask; the mask-free
    tables see the recorded send/recv calls and bytes."""
    exe = cpp_programs.build("null_loopback")
    r = subprocess.run([exe, str(G), str(rows)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("NULL LOOPBACK OK") == 1, r.stdout
    counts = [l for l in r.stdout.splitlines() if l.startswith("COUNTS ")]
    assert len(counts) == 1
    fields = dict(f.split("=") for f in counts[0].split()[1:])
    got = tuple(int(fields[k]) for k in ("sends", "recvs", "send_bytes", "recv_bytes", "rows"))
    assert got == COUNTS_BEFORE_MASKS[(G, rows)], counts[0]
