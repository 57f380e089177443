"""Every capped-grid helper kernel past its first trip, against numpy.

The helper kernels outside the bucket-join core run on a grid capped at a few
thousand blocks and take the rest of their input in further trips of a
grid-stride loop; the scans behind them turn per-tile partials into offsets in
one 1024-thread block, in passes. The other test modules stop far below the
sizes where the second trip (or the second scan pass) begins, so a barrier
missing at the bottom of a trip, a carry read before it is written or a tail
handled on the first trip only would pass them all. Here every family runs at
least two trips deep.

Sizes come from dj.grid_span (dj_grid_span of include/distributed_join.h),
which reports, from the constants the launchers use, what one full grid covers
in one trip (T below) and what one pass of the single-block scan covers (S):
raising a cap moves these tests with it. tests/test_cabi.py pins the values.

Every expected value comes from numpy, from the oracle, or from the Python
MurmurHash3 of test_gpu_string_keys.py — never from the kernel under test.
"""
import numpy as np
import pytest

import oracle
from test_gpu_dtypes import _Dst
from test_gpu_nulls import NULL_HASH, _check_segments, _murmur3_int64, _Source
from test_gpu_rowset import _check_mark, _Words
from test_gpu_string_keys import SEED_HI, murmur  # noqa: F401  (murmur is a fixture)

pytestmark = pytest.mark.gpu


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


def _random_bytes(rng, count):
    return np.frombuffer(rng.bytes(int(count)), dtype=np.uint8)


class _Pool:
    """Device buffers of one test, freed together."""

    def __init__(self, dj):
        self.dj, self.L, self._ptrs = dj, dj.lib(), []

    def alloc(self, nbytes):
        p = self.L.dj_dmalloc(max(int(nbytes), 1))
        self._ptrs.append(p)
        return p

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        if a.nbytes:
            self.L.dj_memcpy_h2d(p, a.ctypes.data, a.nbytes)
        return p

    def mask(self, valid):
        m = self.dj.upload_mask(valid)
        self._ptrs.append(m)
        return m

    def download(self, p, count, dtype):
        out = np.empty(count, dtype=dtype)
        if out.nbytes:
            self.L.dj_memcpy_d2h(out.ctypes.data, p, out.nbytes)
        return out

    def free(self):
        for p in self._ptrs:
            if hasattr(p, "free"):
                p.free()
            else:
                self.L.dj_dfree(p)
        self._ptrs = []


# ------------------------------------------------------------ 1. mask kernels

def test_gather_bitmasks_second_trip(dj):
    T, _ = dj.grid_span("mask_gather")
    n = 2 * T + 64 * 3 + 37          # two full trips, three chunks and a partial chunk
    n_src = n + 37                   # the source table is not the size of the output
    rng = np.random.RandomState(101)
    idx = rng.randint(0, n_src, size=n).astype(np.int64)  # random, with repeats
    idx[1] = idx[0]
    idx[-1] = n_src - 1
    host = [None, rng.random_sample(n_src) >= 0.10, np.arange(n_src) % 2 == 0]
    want = [np.ones(n, dtype=bool) if h is None else h[idx] for h in host]
    d_idx = dj.DeviceArray.from_numpy(idx)
    dev = [None if h is None else dj.upload_mask(h) for h in host]
    ptrs = [None if d is None else d.ptr for d in dev]
    try:
        # the engine's launch grouping, one column per launch, all in one launch
        for per_launch in (0, 1, len(host)):
            outs, counts, _, raws = dj.gather_bitmasks(ptrs, d_idx.ptr, n,
                                                       cols_per_launch=per_launch)
            for c in range(len(host)):
                bad = np.nonzero(outs[c] != want[c])[0]
                assert len(bad) == 0, (per_launch, c, len(bad), bad[:8])
                assert counts[c] == n - int(want[c].sum()), (per_launch, c)
                # bits [n, roundup(n, 64)) are written as 0
                tail = dj.unpack_mask(raws[c], len(raws[c]) * 32)[n:]
                assert len(tail) == (-n) % 64 and not tail.any(), (per_launch, c)
    finally:
        d_idx.free()
        for d in dev:
            if d is not None:
                d.free()


def test_copy_bitmask_segments_second_trip(dj):
    """copy_bitmask_segments and count_unset_bits (the returned null count)
    over more than two trips of destination words. The sources carry guard
    words (test_gpu_nulls._Source), so a read outside one brings in wrong bits."""
    T, _ = dj.grid_span("mask_words")
    total = 2 * T * 32 + 32 * 5 + 13
    n_none, n_last = 99, 3
    n_a = T * 32 - 11                # the first long segment ends inside trip one,
    n_b = total - n_a - n_none - n_last
    assert n_a + n_b > 2 * T * 32    # the second one covers trip two and ends in trip three
    rng = np.random.RandomState(102)
    # both sources end exactly with the last segment that reads them
    a = _Source(dj, _random_bytes(rng, 5 + n_a) < 128)            # ~50% null
    b = _Source(dj, _random_bytes(rng, 37 + n_b) >= 26)           # ~10% null
    segments = [(0, 5, n_a),
                (1, 11, 0),                                       # zero length, in the middle
                (1, 37, n_b),
                (None, 0, n_none),                                # all valid
                (0, 5 + n_a - n_last, n_last)]
    assert sum(s[2] for s in segments) == total
    try:
        _check_segments(dj, segments, [a, b])
    finally:
        a.free()
        b.free()


# ---------------------------------------------------------------- 2. row sets

def _mark_sizes(dj):
    T, _ = dj.grid_span("mark_rows")
    return 2 * T + 64 + 1, 3_000_001


def test_mark_rows_second_trip_random(dj):
    n, nrows = _mark_sizes(dj)
    rng = np.random.RandomState(103)
    _check_mark(dj, rng.randint(0, nrows, size=n), nrows)   # every mode, every word, guards


def test_mark_rows_second_trip_pair_list(dj):
    # runs of neighbouring lanes naming one row, then another: a pair list's shape
    n, nrows = _mark_sizes(dj)
    rng = np.random.RandomState(104)
    _check_mark(dj, np.repeat(rng.randint(0, nrows, size=n // 5 + 1), 5)[:n], nrows)


@pytest.fixture(scope="module")
def select_case(dj):
    """One draw per row (0..9), shared by the two select_rows cases."""
    T, S = dj.grid_span("select_rows")
    tile = dj.select_rows_tile_rows()
    nrows = T + tile + 77            # second grid trip, partial last tile
    ntiles = -(-nrows // tile)
    assert ntiles > T // tile and -(-ntiles // (S // tile)) == 5   # tile_scan's serial chunk
    return nrows, np.random.RandomState(105).randint(0, 10, nrows, dtype=np.uint8)


@pytest.mark.parametrize("density,want_set", [(10, True), (90, False)])
def test_select_rows_second_trip(dj, select_case, density, want_set):
    nrows, draw = select_case
    bits = draw < density // 10      # 10% or 90% of the rows set
    nwords = (nrows + 31) // 32
    padded = np.ones(nwords * 32, dtype=bool)                      # bits past nrows: all ones
    padded[:nrows] = bits
    words = np.packbits(padded, bitorder="little").view(np.uint32)
    want = np.flatnonzero(bits == want_set).astype(np.int64)
    assert 0.09 * nrows < len(want) < 0.11 * nrows                 # ~3.4 M outputs
    w = _Words(dj, words)
    out = dj.DeviceArray.from_numpy(np.full(len(want) + 1, -7, dtype=np.int64))
    try:
        count, _ = dj.select_rows(w.ptr, nrows, want_set, out.ptr)
        got = out.to_numpy()
        assert count == len(want), (count, len(want))
        bad = np.nonzero(got[:-1] != want)[0]
        assert len(bad) == 0, (len(bad), bad[:8], got[bad[:8]], want[bad[:8]])
        assert got[-1] == -7                                       # guard element untouched
        assert (w.read() == words).all()                           # the bitmap is only read
    finally:
        out.free()
        w.free()


# ------------------------------------------------------------ 3. table gather

def test_gather_table_second_trip(dj):
    """One column of each width through the fused kernel (two trips of quads
    and a 3-row scalar tail), the per-column kernel (eight trips) and the
    engine's per-width routing."""
    L = dj.lib()
    T, _ = dj.grid_span("gather_fused")
    Tc, _ = dj.grid_span("gather_column")
    n = 2 * T + 4 * 256 + 3
    assert n % 4 == 3 and n > 2 * Tc
    m = n + 37
    rng = np.random.RandomState(106)
    idx = rng.randint(0, m, size=n).astype(np.int64)
    idx[-1] = m - 1
    widths = (1, 2, 4, 8)
    dtypes = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
    host = [_random_bytes(rng, m * w).view(dtypes[w]) for w in widths]
    want = [h[idx] for h in host]
    d_idx = dj.DeviceArray.from_numpy(idx)
    srcs = [dj.DeviceColumn(h) for h in host]
    try:
        for mode in (dj.GATHER_FUSED, dj.GATHER_PER_COLUMN, dj.GATHER_AUTO):
            dsts = [_Dst(L, n, w) for w in widths]      # 64-byte guard band behind each
            dj.gather_columns([(s.ptr, d.ptr, w) for s, d, w in zip(srcs, dsts, widths)],
                              d_idx.ptr, n, mode)
            for d, w, exp in zip(dsts, widths, want):
                body, guard = d.read()                  # frees the destination
                assert (guard == 0xA5).all(), f"guard band overwritten: width {w} mode {mode}"
                bad = np.nonzero(body != exp)[0]
                assert len(bad) == 0, (mode, w, len(bad), bad[:8])
    finally:
        d_idx.free()
        for s in srcs:
            s.free()


# ----------------------------------------------------- 4. strings column path

def _strings_n(dj):
    T, S = dj.grid_span("string_scan")
    n = T + 4096 + 5                 # second trip of tiles, third pass over the partials
    assert n > 2 * S
    for family in ("string_rows", "string_sum"):
        assert n > 2 * dj.grid_span(family)[0]
    return n


def test_offsets_scan_second_trip(dj):
    n = _strings_n(dj)
    L = dj.lib()
    keys = np.arange(n, dtype=np.int64) * 13 + 5
    dk = dj.DeviceArray.from_numpy(keys)
    off_p, ch_p, nb = dj.gen_test_strings(dk, n)
    try:
        off = np.empty(n + 1, dtype=np.int32)
        L.dj_memcpy_d2h(off.ctypes.data, off_p, (n + 1) * 4)
        want = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(keys % 7 + 1, out=want[1:])
        bad = np.nonzero(off != want)[0]
        assert len(bad) == 0, (len(bad), bad[:8], off[bad[:8]], want[bad[:8]])
        assert nb == int(want[-1])
    finally:
        dk.free()
        L.dj_dfree(off_p)
        L.dj_dfree(ch_p)


def test_string_gather_second_trip(dj):
    """The placement step of shuffle_on on (INT64 key, INT64 row id, STRING):
    gather_sizes_starts, sum_sizes_i64, offsets_from_sizes and
    gather_chars_from_starts over many trips; the scan sees zero sizes and takes
    its third pass over the partials."""
    n = _strings_n(dj)
    nparts = 7
    rng = np.random.RandomState(107)
    sizes = rng.randint(0, 9, n).astype(np.int64)        # zero-length rows are frequent
    sizes[::100_003] = 300                               # rows of many words
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(sizes, out=off[1:])
    total = int(off[-1])
    assert total < 2 ** 31
    chars = _random_bytes(rng, total)
    keys = rng.randint(-2 ** 62, 2 ** 62, n).astype(np.int64)
    rowid = np.arange(n, dtype=np.int64)
    pool = _Pool(dj)
    try:
        cols = [(dj.TYPE_INT64, pool.upload(keys)), (dj.TYPE_INT64, pool.upload(rowid)),
                (dj.TYPE_STRING, pool.upload(off.astype(np.int32)), pool.upload(chars), total)]
        got, got_off = dj.cpp_partition_cols(cols, n, [0], nparts)
    finally:
        pool.free()
    perm = got[1]
    assert len(perm) == n and perm.min() >= 0 and perm.max() < n
    assert (np.bincount(perm, minlength=n) == 1).all()   # a permutation of arange(n)
    # and the very permutation the oracle's stable partition gives
    _, want_perm, want_off = oracle.partition(keys, rowid, nparts, oracle.HASH_MURMUR3, 0)
    assert (got_off == want_off).all()
    assert (perm == want_perm).all()
    assert (got[0] == keys[perm]).all()
    out_off, out_chars = got[2]
    psizes = sizes[perm]
    want_out_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(psizes, out=want_out_off[1:])
    bad = np.nonzero(out_off != want_out_off)[0]
    assert len(bad) == 0, (len(bad), bad[:8])
    assert len(out_chars) == total
    src_pos = np.repeat(off[perm] - want_out_off[:-1], psizes) + np.arange(total, dtype=np.int64)
    bad = np.nonzero(out_chars != chars[src_pos])[0]
    assert len(bad) == 0, (len(bad), bad[:8])


HASH_PERIOD = 4099
HASH_STAGE_BYTES = 32 * 1024     # the LDS staging budget of hash_strings (HS_LDS_BYTES)


def _hash_second_trip(dj, murmur, seed, long_row):
    """n rows of a periodic column: HASH_PERIOD distinct rows of 0..20 random
    bytes (one of them `long_row` bytes and one 13 KiB when given). The period's
    byte length is odd, so successive periods start at every address residue
    modulo 16. The two big rows sit where the period puts them at rows T + 1500
    and T + 300, inside the first tile of the blocks' second trip, whatever T
    is; the periods before bring them to every other place of a tile."""
    T, _ = dj.grid_span("string_hash")
    n = T + 2048 + 5
    P = HASH_PERIOD
    rng = np.random.RandomState(seed)
    lens = rng.randint(0, 21, P).astype(np.int64)
    special = set()
    if long_row:
        assert long_row > HASH_STAGE_BYTES
        special = {(T + 1500) % P, (T + 300) % P}
        lens[(T + 1500) % P] = long_row
        # and a row that still stages, in a 1024-row span (its tile no longer
        # fits the budget as one), and keeps its thread busy long after the
        # rest of the block is ready to restage the image for the next span
        lens[(T + 300) % P] = 13 * 1024 + 77
    if lens.sum() % 2 == 0:
        i = min(set(range(3)) - special)
        lens[i] += 1 if lens[i] < 20 else -1
    if long_row:
        # before any GPU work: past the first trip (rows >= T) there is a row
        # that cannot stage and a multi-KiB row that does
        second = np.tile(lens, -(-n // P))[T:n]
        assert (second > HASH_STAGE_BYTES).any()
        assert ((second > 4096) & (second < HASH_STAGE_BYTES // 2)).any()
    poff = np.zeros(P + 1, dtype=np.int64)
    np.cumsum(lens, out=poff[1:])
    pchars = _random_bytes(rng, poff[-1])
    assert poff[-1] % 2 == 1
    raw = pchars.tobytes()
    rows = [raw[poff[i]:poff[i + 1]] for i in range(P)]
    reps = -(-n // P)
    assert reps >= 16
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.tile(lens, reps)[:n], out=off[1:])
    nbytes = int(off[-1])
    assert nbytes < 2 ** 31
    chars = np.tile(pchars, reps)[:nbytes]
    pool = _Pool(dj)
    try:
        off_p, ch_p = pool.upload(off.astype(np.int32)), pool.upload(chars)
        del chars
        for hseed in (0, SEED_HI):
            got = dj.hash_strings(off_p, ch_p, nbytes, n, hseed)
            ref = np.array([murmur(r, hseed) for r in rows], dtype=np.uint32)
            want = np.tile(ref, reps)[:n]
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, (hex(hseed), len(bad), bad[:8], bad[:8] % P)
    finally:
        pool.free()


def test_hash_strings_second_trip(dj, murmur):
    _hash_second_trip(dj, murmur, 108, long_row=0)


def test_hash_strings_second_trip_long_rows(dj, murmur):
    # one row per period outgrows the 32 KiB staging budget: its 256-row span
    # reads global memory directly. One such row is row T + 1500, so block 0
    # goes staged -> staged -> direct -> staged through the tile of its second
    # trip (asserted on the host in _hash_second_trip)
    _hash_second_trip(dj, murmur, 109, long_row=HASH_STAGE_BYTES + 233)


# --------------------------------------------------------- 5. cascaded codec
#
# Wire size by the format in the header of csrc/dj_compress.hip: a 32-byte
# slice header, then either the raw elements or bitpacked subslices — N values
# of width W take ceil(N / 32) * W * 4 bytes. W is the bit width of the widest
# zigzag value (at least 1). The codec stores raw whenever the encoded form
# would not be smaller.

HDR = 32


def _zigzag_bits(v):
    v = np.asarray(v, dtype=np.int64)
    z = ((v << 1) ^ (v >> 63)).view(np.uint64)
    return max(int(np.bitwise_or.reduce(z)).bit_length(), 1) if len(z) else 1


def _delta(v):
    v = np.asarray(v, dtype=np.int64)
    d = v.copy()
    d[1:] = v[1:] - v[:-1]
    return d


def _packed(n, w):
    return -(-n // 32) * w * 4


def _format_wire(arr, rles, deltas, bp):
    """(wire bytes, stored raw?) of the documented format for this input."""
    n, raw = len(arr), len(arr) * arr.itemsize
    v = arr.astype(np.int64)
    if rles:
        starts = np.flatnonzero(np.concatenate([[True], v[1:] != v[:-1]]))
        lengths = np.diff(np.concatenate([starts, [n]]))
        run_vals = v[starts]
        vbits = _zigzag_bits(_delta(run_vals) if deltas else run_vals) if bp else 64
        lbits = _zigzag_bits(lengths) if bp else 64
        enc = _packed(len(starts), lbits) + _packed(len(starts), vbits)
    elif bp:
        enc = _packed(n, _zigzag_bits(_delta(v) if deltas else v))
    else:
        enc = raw
    return (HDR + raw, True) if enc >= raw else (HDR + enc, False)


def _codec_roundtrip(dj, arr, rles, deltas, bp, want_wire):
    pool = _Pool(dj)
    try:
        d_in, d_out = pool.upload(arr), pool.alloc(arr.nbytes)
        wire = dj.lib().dj_compress_roundtrip(d_in, len(arr), arr.itemsize, rles, deltas, bp,
                                              d_out)
        got = pool.download(d_out, len(arr), arr.dtype)
    finally:
        pool.free()
    bad = np.nonzero(got != arr)[0]
    assert len(bad) == 0, (rles, deltas, bp, len(bad), bad[:8])
    assert wire == want_wire, (rles, deltas, bp, wire, want_wire)


def _codec_count(dj):
    _, S = dj.grid_span("codec_elems")
    return 2 * S + 3 * 2048 + 5      # third pass of the single-block scan


def test_codec_delta_scan_second_pass(dj):
    count = _codec_count(dj)
    rng = np.random.RandomState(110)
    arr = np.sort(rng.randint(0, 10 ** 12, count)).astype(np.int64)
    want, raw = _format_wire(arr, 0, 1, 1)
    assert not raw
    _codec_roundtrip(dj, arr, 0, 1, 1, want)


@pytest.mark.parametrize("deltas", [1, 0])
def test_codec_rle_run_scans_second_pass(dj, deltas):
    """Runs of alternating length 1 and 2 over a slowly rising value: about
    2/3 * count runs, more than one scan pass covers, so the decode scans over
    the runs (offsets from lengths; values from deltas) take a second pass."""
    count = _codec_count(dj)
    _, S = dj.grid_span("codec_elems")
    nruns = 2 * (count // 3) + 2
    r = np.arange(nruns, dtype=np.int64)
    run_vals = 2 * (r // (nruns // 2 + 1)) + (r & 1)      # 0..3, neighbours always differ
    arr = np.repeat(run_vals, np.tile([1, 2], nruns // 2))[:count]
    assert len(arr) == count
    want, raw = _format_wire(arr, 1, deltas, 1)
    # 3-bit lengths and values of at most 3 bits: far smaller than raw, so the
    # RLE path is the one that runs
    assert not raw and want < count * 8 // 10
    assert int((arr[1:] != arr[:-1]).sum()) + 1 > S
    _codec_roundtrip(dj, arr, 1, deltas, 1, want)


def test_codec_bitpack_63_bits(dj):
    # |v| < 2^62 zigzags to 63 bits: packed (63/64 of raw), values across three words
    count = _codec_count(dj)
    rng = np.random.RandomState(111)
    arr = rng.randint(-2 ** 62, 2 ** 62, count).astype(np.int64)
    want, raw = _format_wire(arr, 0, 0, 1)
    assert not raw and want == HDR + _packed(count, 63)
    _codec_roundtrip(dj, arr, 0, 0, 1, want)


def test_codec_raw_fallback_many_trips(dj):
    # full-range values need 64 bits: stored raw, the byte copy runs many trips
    count = _codec_count(dj)
    rng = np.random.RandomState(112)
    arr = _random_bytes(rng, count * 8).view(np.int64)
    want, raw = _format_wire(arr, 0, 0, 1)
    assert raw and want == HDR + count * 8
    assert count * 8 > 2 * dj.grid_span("codec_elems")[0]
    _codec_roundtrip(dj, arr, 0, 0, 1, want)


@pytest.mark.parametrize("deltas", [0, 1])
def test_codec_pack_second_trip_int8(dj, deltas):
    T, _ = dj.grid_span("codec_pack")
    count = T + 32 * 300 + 5         # pack/unpack go past one trip of groups
    rng = np.random.RandomState(113)
    arr = (_random_bytes(rng, count) % 4).astype(np.int8) - 2      # -2..1
    want, raw = _format_wire(arr, 0, deltas, 1)
    assert not raw and want <= HDR + _packed(count, 3)
    _codec_roundtrip(dj, arr, 0, deltas, 1, want)


# ------------------------- 6. engine helper kernels, end to end at world size 1
#
# What runs where at one rank (csrc/dj_local_join.hip local_join,
# csrc/dj_table_ops.hip place_rows; the kernels: csrc/dj_key_helpers.hip):
#   composite or nullable keys  fuse_keys, the tuple filter over the pair list
#   one mask-free narrow key    widen_key on both inputs, narrow_key on the output
#   left join                   mark_rows, select_rows, the null-padded gathers
#   placement, nullable key     nullable_key_hash
#   concat of batch results     rebase_offsets — no single-rank join has a second
#                               batch, so it runs through its own hook

def _join_rows(dj):
    T, _ = dj.grid_span("key_helpers")
    return T + T // 3                # ~700,000: every row kernel's second trip


def _sorted_pairs(li, ri, base):
    """(li, ri) pairs, ri >= -1, as one sorted int64 code per pair."""
    return np.sort(np.asarray(li, dtype=np.int64) * base + np.asarray(ri, dtype=np.int64) + 1)


def _nulls(rng, n, count):
    valid = np.ones(n, dtype=bool)
    valid[rng.choice(n, count, replace=False)] = False
    return valid


def test_composite_key_inner_join_second_trip(dj, comm):
    """Key (nullable INT16, UINT8) over the 2^24 key space."""
    n = _join_rows(dj)
    rng = np.random.RandomState(114)
    rowid = np.arange(n, dtype=np.int64)

    def side():
        k16 = _random_bytes(rng, 2 * n).view(np.int16)
        k8 = _random_bytes(rng, n)
        valid = _nulls(rng, n, n // 1000)        # the values under the nulls stay random
        # collision-free id; a null is a 16-bit value of its own (null == null)
        cid = np.where(valid, k16.astype(np.int64) + 32768, 65536) * 256 + k8
        return k16, k8, valid, cid

    lk16, lk8, lvalid, lid = side()
    rk16, rk8, rvalid, rid = side()
    _, wl, _, wr = oracle.inner_join(lid, rowid, rid, rowid)
    assert len(wl) > 20_000                      # ~30 k matches, ~2 k of them null == null
    pool = _Pool(dj)
    try:
        lcols = [(dj.TYPE_INT16, pool.upload(lk16), pool.mask(lvalid)),
                 (dj.TYPE_UINT8, pool.upload(lk8)), (dj.TYPE_INT64, pool.upload(rowid))]
        rcols = [(dj.TYPE_INT16, pool.upload(rk16), pool.mask(rvalid)),
                 (dj.TYPE_UINT8, pool.upload(rk8)), (dj.TYPE_INT64, pool.upload(rowid))]
        cols, masks = dj.cpp_distributed_inner_join_ncols_multi(comm, lcols, n, rcols, n,
                                                                [0, 1], [0, 1])
    finally:
        pool.free()
    assert [m is None for m in masks] == [False, True, True, False, True, True]
    gl, gr = cols[2], cols[5]
    assert len(gl) == len(wl), (len(gl), len(wl))
    assert (_sorted_pairs(gl, gr, n + 1) == _sorted_pairs(wl, wr, n + 1)).all()
    sides = ((cols[0], cols[1], masks[0], lk16, lk8, lvalid, gl),
             (cols[3], cols[4], masks[3], rk16, rk8, rvalid, gr))
    for key, u8, mask, hk, h8, hvalid, rows in sides:
        assert (mask == hvalid[rows]).all()
        assert (key[mask] == hk[rows][mask]).all()
        assert (u8 == h8[rows]).all()


@pytest.fixture(scope="module")
def int32_tables(dj):
    """INT32 keys of both sides: about a quarter of the left keys repeat on the
    right, 1% of the left rows have no partner. Never modified."""
    n = _join_rows(dj)
    K = n * 4 // 7
    rng = np.random.RandomState(115)
    lk = rng.randint(0, K, n).astype(np.int32)
    lk[rng.choice(n, n // 100, replace=False)] += K
    rk = np.concatenate([np.arange(K), rng.randint(0, K, n - K)]).astype(np.int32)
    rng.shuffle(rk)
    return n, lk, rk, rng


def test_narrow_key_inner_join_second_trip(dj, comm, int32_tables):
    """One mask-free INT32 key: widen_key on both inputs, narrow_key on the
    joined keys of an output larger than either input."""
    n, lk, rk, _ = int32_tables
    rowid = np.arange(n, dtype=np.int64)
    _, wl, _, wr = oracle.inner_join(lk.astype(np.int64), rowid, rk.astype(np.int64), rowid)
    assert len(wl) > n
    pool = _Pool(dj)
    try:
        lcols = [(dj.TYPE_INT32, pool.upload(lk)), (dj.TYPE_INT64, pool.upload(rowid))]
        rcols = [(dj.TYPE_INT32, pool.upload(rk)), (dj.TYPE_INT64, pool.upload(rowid))]
        cols = dj.cpp_distributed_inner_join_cols_multi(comm, lcols, n, rcols, n, [0], [0])
    finally:
        pool.free()
    gl, gr = cols[1], cols[3]
    assert len(gl) == len(wl), (len(gl), len(wl))
    assert (_sorted_pairs(gl, gr, n + 1) == _sorted_pairs(wl, wr, n + 1)).all()
    assert cols[0].dtype == np.int32 and cols[2].dtype == np.int32
    assert (cols[0] == lk[gl]).all() and (cols[2] == rk[gr]).all()


def test_nullable_key_left_join_second_trip(dj, comm, int32_tables):
    """Left join on a nullable INT32 key: the tuple filter over a pair list
    larger than the inputs, mark_rows, select_rows and the null-padded gathers."""
    n, lk, rk, _ = int32_tables
    rng = np.random.RandomState(116)
    rowid = np.arange(n, dtype=np.int64)
    lvalid, rvalid = _nulls(rng, n, 300), _nulls(rng, n, 3)
    null_id = np.int64(2 ** 40)                  # null == null, and no valid key
    lid = np.where(lvalid, lk.astype(np.int64), null_id)
    rid = np.where(rvalid, rk.astype(np.int64), null_id)
    _, wl, _, wr = oracle.inner_join(lid, rowid, rid, rowid)
    unmatched = np.setdiff1d(rowid, wl)
    assert len(wl) > n and len(unmatched) > n // 200
    # ~1.2 M pairs: the filter's second trip, and mark_rows' too
    assert len(wl) > max(dj.grid_span("string_rows")[0], dj.grid_span("mark_rows")[0])
    want = _sorted_pairs(np.concatenate([wl, unmatched]),
                         np.concatenate([wr, np.full(len(unmatched), -1)]), n + 1)
    pool = _Pool(dj)
    try:
        lcols = [(dj.TYPE_INT32, pool.upload(lk), pool.mask(lvalid)),
                 (dj.TYPE_INT64, pool.upload(rowid))]
        rcols = [(dj.TYPE_INT32, pool.upload(rk), pool.mask(rvalid)),
                 (dj.TYPE_INT64, pool.upload(rowid))]
        cols, masks = dj.cpp_distributed_join_ncols_multi(comm, dj.JOIN_LEFT, lcols, n, rcols, n,
                                                          [0], [0])
    finally:
        pool.free()
    # left columns masked as their sources, every right-hand column masked
    assert [m is None for m in masks] == [False, True, False, False]
    matched = masks[3]
    gl, gr = cols[1], np.where(matched, cols[3], -1)
    assert len(gl) == len(want), (len(gl), len(want))
    assert (_sorted_pairs(gl, gr, n + 1) == want).all()
    assert (masks[0] == lvalid[gl]).all()
    assert (cols[0][masks[0]] == lk[gl][masks[0]]).all()
    assert (masks[2] == (matched & rvalid[np.maximum(gr, 0)])).all()
    assert (cols[2][masks[2]] == rk[gr[masks[2]]]).all()
    # the cells of an unmatched row are zero bytes
    assert not cols[2][~matched].any() and not cols[3][~matched].any()


def test_nullable_key_placement_second_trip(dj, int32_tables):
    """nullable_key_hash: valid rows place on the murmur3 hash of the widened
    key, null rows on the null element hash (csrc/dj_hash.h)."""
    n, lk, _, _ = int32_tables
    rng = np.random.RandomState(117)
    nparts, seed = 7, 12345678
    valid = _nulls(rng, n, n // 20)
    rowid = np.arange(n, dtype=np.int64)
    pool = _Pool(dj)
    try:
        cols = [(dj.TYPE_INT32, pool.upload(lk), pool.mask(valid)),
                (dj.TYPE_INT64, pool.upload(rowid))]
        (got, masks), off = dj.cpp_partition_ncols(cols, n, [0], nparts, dj.HASH_MURMUR3, seed)
    finally:
        pool.free()
    h = np.where(valid, _murmur3_int64(lk.astype(np.int64), seed), np.uint64(NULL_HASH))
    want_part = (h % np.uint64(nparts)).astype(np.int64)
    assert off[0] == 0 and off[-1] == n
    assert (np.diff(off) == np.bincount(want_part, minlength=nparts)).all()
    row = got[1]
    assert (np.bincount(row, minlength=n) == 1).all()
    assert (want_part[row] == np.repeat(np.arange(nparts), np.diff(off))).all()
    for p in range(nparts):                      # stable inside a partition
        assert (np.diff(row[off[p]:off[p + 1]]) > 0).all()
    assert (masks[0] == valid[row]).all() and masks[1] is None
    assert (got[0][masks[0]] == lk[row][masks[0]]).all()


def test_concat_rebases_string_offsets_second_trip(dj):
    """rebase_offsets (and the masks' segment copy) on two parts of more rows
    than one trip covers: (INT64 row id, STRING, UINT8), the STRING column
    masked in the second part only."""
    T, _ = dj.grid_span("key_helpers")
    rng = np.random.RandomState(118)
    pool = _Pool(dj)
    parts, host = [], []
    try:
        for p, n in enumerate((T + T // 8 + 5, T + T // 8 + 16)):
            sizes = rng.randint(0, 9, n).astype(np.int64)
            off = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(sizes, out=off[1:])
            chars = _random_bytes(rng, off[-1])
            u8 = _random_bytes(rng, n)
            svalid = rng.random_sample(n) >= 0.2 if p == 1 else None
            uvalid = rng.random_sample(n) >= 0.1
            rowid = np.arange(n, dtype=np.int64) + p * 10 ** 7
            string = (dj.TYPE_STRING, pool.upload(off.astype(np.int32)), pool.upload(chars),
                      int(off[-1]))
            if svalid is not None:
                string += (pool.mask(svalid),)
            parts.append(([(dj.TYPE_INT64, pool.upload(rowid)), string,
                           (dj.TYPE_UINT8, pool.upload(u8), pool.mask(uvalid))], n))
            host.append((rowid, sizes, chars, u8,
                         np.ones(n, dtype=bool) if svalid is None else svalid, uvalid))
        cols, masks = dj.cpp_concat_ncols(parts)
    finally:
        pool.free()
    rowid, sizes, chars, u8, svalid, uvalid = (np.concatenate(x) for x in zip(*host))
    want_off = np.zeros(len(rowid) + 1, dtype=np.int64)
    np.cumsum(sizes, out=want_off[1:])
    assert (cols[0] == rowid).all() and masks[0] is None
    got_off, got_chars = cols[1]
    bad = np.nonzero(got_off != want_off)[0]
    assert len(bad) == 0, (len(bad), bad[:8])
    assert (got_chars == chars).all()
    assert (masks[1] == svalid).all()
    assert (cols[2] == u8).all() and (masks[2] == uvalid).all()
