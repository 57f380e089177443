"""The row-set kernels (csrc/dj_rowset.hip) through their hooks, against numpy:
mark_rows sets bit idx[i] of a zeroed bitmap, select_rows lists the rows whose
bit has the wanted value in ascending order. Bit layout: row i is bit i % 32
of uint32 word i / 32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 0xA5A5A5A5


@pytest.fixture(scope="module")
def dj():
    import distributed_join_amd as dj
    dj.require_gpu()
    return dj


class _Words:
    """Device uint32 buffer: a guard word, nwords payload words, a guard word."""

    def __init__(self, dj, words):
        self.dj = dj
        self.nwords = len(words)
        buf = np.concatenate([[GUARD], np.asarray(words, dtype=np.uint32), [GUARD]])
        buf = buf.astype(np.uint32)
        self.nbytes = buf.nbytes
        self.base = dj.lib().dj_dmalloc(buf.nbytes)
        dj.lib().dj_memcpy_h2d(self.base, buf.ctypes.data, buf.nbytes)
        self.ptr = self.base + 4

    def read(self):
        buf = np.empty(self.nwords + 2, dtype=np.uint32)
        self.dj.lib().dj_memcpy_d2h(buf.ctypes.data, self.base, self.nbytes)
        assert buf[0] == GUARD and buf[-1] == GUARD, "wrote outside the bitmap"
        return buf[1:-1]

    def free(self):
        self.dj.lib().dj_dfree(self.base)


def _want_words(idx, nrows):
    bits = np.zeros((nrows + 31) // 32 * 32, dtype=bool)
    bits[np.asarray(idx, dtype=np.int64)] = True
    return np.packbits(bits, bitorder="little").view(np.uint32)


def _check_mark(dj, idx, nrows):
    idx = np.asarray(idx, dtype=np.int64)
    want = _want_words(idx, nrows)
    d_idx = dj.DeviceArray.from_numpy(idx)
    # the engine's variant and each ablation variant of the benchmark
    for mode in (dj.MARK_ENGINE, dj.MARK_PLAIN, dj.MARK_MERGE, dj.MARK_CHECK,
                 dj.MARK_MERGE | dj.MARK_CHECK):
        w = _Words(dj, np.zeros(len(want), dtype=np.uint32))
        dj.mark_rows(d_idx.ptr, len(idx), w.ptr, mode=mode)
        got = w.read()
        w.free()
        # every word, so also: words that received no index are still zero
        assert (got == want).all(), (mode, len(idx), nrows, np.nonzero(got != want)[0][:8])
    d_idx.free()


@pytest.mark.parametrize("nrows", [1, 32, 33, 100003])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 100003])
def test_mark_rows_random(dj, n, nrows):
    rng = np.random.RandomState(n * 7 + nrows)
    _check_mark(dj, rng.randint(0, nrows, size=n), nrows)


@pytest.mark.parametrize("nrows", [1, 33, 100003])
def test_mark_rows_every_index_equal(dj, nrows):
    # one word, one bit, from every lane of many waves and blocks
    _check_mark(dj, np.full(5000, nrows - 1), nrows)
    _check_mark(dj, np.full(64, nrows // 2), nrows)


def test_mark_rows_one_word_different_bits(dj):
    rng = np.random.RandomState(5)
    nrows = 100003
    for word in (0, 7, (nrows - 1) // 32 - 1):
        _check_mark(dj, word * 32 + rng.randint(0, 32, size=3000), nrows)
        _check_mark(dj, word * 32 + np.arange(32), nrows)
    # runs of neighbouring lanes naming one word, then another: a pair list's shape
    _check_mark(dj, np.repeat(rng.randint(0, nrows, size=700), 5), nrows)


@pytest.mark.parametrize("nrows", [1, 32, 33, 100003])
def test_mark_rows_first_and_last_only(dj, nrows):
    _check_mark(dj, [0, nrows - 1], nrows)
    _check_mark(dj, [nrows - 1, 0, 0, nrows - 1], nrows)


# ------------------------------------------------------------ select_rows

def _select_sizes(tile):
    return [0, 1, 31, 32, 33, 64, tile - 1, tile, tile + 1, 3 * tile + 77]


def _patterns(rng, nrows):
    yield "all", np.ones(nrows, dtype=bool)
    yield "none", np.zeros(nrows, dtype=bool)
    yield "alternating", np.arange(nrows) % 2 == 0
    yield "10%", rng.random_sample(nrows) < 0.10
    yield "90%", rng.random_sample(nrows) < 0.90


def test_select_rows(dj):
    tile = dj.select_rows_tile_rows()
    assert tile % 32 == 0 and tile >= 64
    rng = np.random.RandomState(11)
    for nrows in _select_sizes(tile):
        nwords = (nrows + 31) // 32
        for name, bits in _patterns(rng, nrows):
            padded = np.ones(nwords * 32, dtype=bool)  # bits past nrows: all ones
            padded[:nrows] = bits
            words = np.packbits(padded, bitorder="little").view(np.uint32)
            w = _Words(dj, words)
            for want_set in (True, False):
                want = np.flatnonzero(bits == want_set).astype(np.int64)
                out = dj.DeviceArray.from_numpy(np.full(len(want) + 1, -7, dtype=np.int64))
                count, _ = dj.select_rows(w.ptr, nrows, want_set, out.ptr)
                got = out.to_numpy()
                out.free()
                assert count == len(want), (nrows, name, want_set, count)
                assert (got[:-1] == want).all(), (nrows, name, want_set)
                assert got[-1] == -7, (nrows, name, want_set)  # guard element untouched
            assert (w.read() == words).all()  # the bitmap is only read
            w.free()
