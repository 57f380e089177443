"""The two kernels behind null_equality::UNEQUAL through their hooks, against
numpy: key_row_validity (csrc/dj_bitmask.hip), the AND of up to four validity
masks with the bits past the row count cleared and the 0 bits counted, and
compact_keyed_rows (csrc/dj_rowset.hip), select_rows for the set bits that also
carries keys[row]. Bit layout: row i is bit i % 32 of uint32 word i / 32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 0xA5A5A5A5
POISON = 0xDEADBEEF


@pytest.fixture(scope="module")
def dj():
    import distributed_join_amd as dj
    dj.require_gpu()
    return dj


class _Words:
    """Device uint32 buffer: a guard word, the payload words, two guard words."""

    def __init__(self, dj, words, guard=GUARD):
        self.dj, self.guard = dj, np.uint32(guard)
        self.nwords = len(words)
        buf = np.concatenate([[guard], np.asarray(words, dtype=np.uint32),
                              [guard, guard]]).astype(np.uint32)
        self.nbytes = buf.nbytes
        self.base = dj.lib().dj_dmalloc(buf.nbytes)
        dj.lib().dj_memcpy_h2d(self.base, buf.ctypes.data, buf.nbytes)
        self.ptr = self.base + 4

    def read(self):
        buf = np.empty(self.nwords + 3, dtype=np.uint32)
        self.dj.lib().dj_memcpy_d2h(buf.ctypes.data, self.base, self.nbytes)
        assert buf[0] == self.guard and (buf[-2:] == self.guard).all(), "wrote outside the words"
        return buf[1:-2]

    def free(self):
        self.dj.lib().dj_dfree(self.base)


def _pack(bits):
    """bool[32 * k] -> k uint32 words."""
    return np.packbits(bits, bitorder="little").view(np.uint32)


def _random_words(rng, nwords, p_valid):
    """nwords * 32 random bits, also past any row count: garbage there."""
    return _pack(rng.random_sample(nwords * 32) < p_valid)


# ------------------------------------------------------------ key_row_validity

def _check_validity(dj, rng, nrows, present, p_valid=0.8):
    """present: one bool per mask slot, False = a null pointer (all valid)."""
    nwords = (nrows + 31) // 32
    srcs = [_Words(dj, _random_words(rng, nwords, p_valid)) if p else None for p in present]
    dst = _Words(dj, np.full(nwords, POISON, dtype=np.uint32), guard=POISON)
    try:
        want = np.ones(nwords * 32, dtype=bool)
        for s in srcs:
            if s is not None:
                want &= np.unpackbits(s.read().view(np.uint8), bitorder="little").astype(bool)
        want[nrows:] = False                       # whatever the sources hold there
        nulls = dj.key_row_validity([s.ptr if s else None for s in srcs], nrows, dst.ptr)
        got = dst.read()                           # also: the two poison words behind are intact
        bad = np.nonzero(got != _pack(want))[0]
        assert len(bad) == 0, (nrows, present, bad[:8])
        assert nulls == nrows - int(want[:nrows].sum()), (nrows, present, nulls)
    finally:
        dst.free()
        for s in srcs:
            if s is not None:
                s.free()


VALIDITY_MASKS = [
    (True,), (False,),
    (True, True), (False, True), (False, False),
    (True, False, True), (True, True, True),
    (True, True, True, True), (False, True, False, True), (False, False, False, False),
]


@pytest.mark.parametrize("nrows", [1, 31, 32, 33, 63, 64, 65, 8191, 8192, 8193])
def test_key_row_validity(dj, nrows):
    rng = np.random.RandomState(nrows)
    for present in VALIDITY_MASKS:
        _check_validity(dj, rng, nrows, present)
    # a source with every row null, and sources that share no valid row
    _check_validity(dj, rng, nrows, (True, True), p_valid=0.0)
    _check_validity(dj, rng, nrows, (True, False, True), p_valid=1.0)


def test_key_row_validity_third_trip(dj):
    T, _ = dj.grid_span("mask_words")
    nrows = 2 * T * 32 + 32 * 5 + 13               # ends in the third trip, inside a word
    assert (nrows + 31) // 32 > 2 * T
    _check_validity(dj, np.random.RandomState(301), nrows, (True, False, True))


# ---------------------------------------------------------- compact_keyed_rows

def _keys_of(rows):
    """A non-monotone function of the row number (odd multiplier mod 2^64)."""
    return (rows.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)


def _check_compact(dj, bits, nrows, garbage):
    """bits: bool[nrows]. The words' bits past nrows are set to `garbage`."""
    nwords = (nrows + 31) // 32
    padded = np.full(nwords * 32, garbage, dtype=bool)
    padded[:nrows] = bits
    words = _pack(padded)
    want = np.flatnonzero(bits).astype(np.int64)
    keys = _keys_of(np.arange(nrows, dtype=np.int64))
    w = _Words(dj, words)
    d_keys = dj.DeviceArray.from_numpy(keys)
    out_idx = dj.DeviceArray.from_numpy(np.full(len(want) + 1, -7, dtype=np.int64))
    out_keys = dj.DeviceArray.from_numpy(np.full(len(want) + 1, -9, dtype=np.int64))
    try:
        count, _ = dj.compact_keyed_rows(w.ptr, nrows, d_keys.ptr, out_idx.ptr, out_keys.ptr)
        gi, gk = out_idx.to_numpy(), out_keys.to_numpy()
        assert count == len(want), (nrows, count, len(want))
        bad = np.nonzero(gi[:-1] != want)[0]       # ascending and exact
        assert len(bad) == 0, (nrows, len(bad), bad[:8], gi[bad[:8]], want[bad[:8]])
        bad = np.nonzero(gk[:-1] != keys[want])[0]
        assert len(bad) == 0, (nrows, len(bad), bad[:8])
        assert gi[-1] == -7 and gk[-1] == -9       # guard elements untouched
        assert (w.read() == words).all()           # the bitmap is only read
    finally:
        out_keys.free()
        out_idx.free()
        d_keys.free()
        w.free()
    return len(want)


@pytest.mark.parametrize("nrows", [1, 8191, 8192, 8193, 3 * 8192 + 5])
def test_compact_keyed_rows(dj, nrows):
    assert dj.select_rows_tile_rows() == 8192      # the sizes above sit around one tile
    rng = np.random.RandomState(nrows)
    last = np.zeros(nrows, dtype=bool)
    last[-1] = True
    for garbage in (True, False):
        _check_compact(dj, np.ones(nrows, dtype=bool), nrows, garbage)
        _check_compact(dj, np.zeros(nrows, dtype=bool), nrows, garbage)
        _check_compact(dj, last, nrows, garbage)
        _check_compact(dj, rng.random_sample(nrows) < 0.5, nrows, garbage)


def test_compact_keyed_rows_third_trip(dj):
    """More than two trips of the tile grid and more than two passes of the
    tile scan. About 1 bit in 64 keeps the read-back small; a dense window
    lies across each trip boundary."""
    T, S = dj.grid_span("select_rows")
    tile = dj.select_rows_tile_rows()
    nrows = 2 * T + tile + 77                      # third trip, partial last tile
    assert -(-nrows // tile) > 2 * (S // tile)
    rng = np.random.RandomState(302)
    bits = rng.randint(0, 64, nrows, dtype=np.uint8) == 0
    for edge in (T, 2 * T):
        bits[edge - tile - 5:edge + tile + 5] = True
    nsel = _check_compact(dj, bits, nrows, True)
    assert nrows // 80 < nsel < nrows // 50
