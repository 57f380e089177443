"""STRING key columns through the drop-in path: the row-hash kernel, single
and composite STRING join keys, the byte-exact collision filter, edge
tables, shuffle_on, and the multi-rank loopback program.

Reference semantics: distributed_inner_join / shuffle_on forward arbitrary
key columns to cudf::hash_partition / cudf::inner_join, which accept STRING
columns (distributed_join.cpp:71-132, shuffle_on.cpp:59-60).

Every comparison is bit-exact. The hash reference is an in-test Python
MurmurHash3_x86_32, validated against the published vectors before use; the
join reference is oracle.inner_join on dictionary-encoded key ids.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cpp_programs
import oracle

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
SEED_HI = 0x9747B28C


@pytest.fixture(scope="module")
def dj():
    import distributed_join_amd as dj
    L = dj.lib()
    for sym in ("dj_hash_strings", "dj_cpp_shuffle_on_cols"):
        if not hasattr(L, sym):
            pytest.fail(f"libdistjoin.so does not export {sym}: STRING key columns are "
                        "not supported by this build")
    dj.require_gpu()
    return dj


@pytest.fixture(scope="module")
def comm(dj):
    c = dj.CppCommunicator(0, 1)
    yield c
    c.destroy()


# ------------------------------------------------------------ hash reference

def _murmur3_x86_32(data, seed):
    def rotl(x, r):
        return ((x << r) | (x >> (32 - r))) & 0xFFFFFFFF

    c1, c2 = 0xCC9E2D51, 0x1B873593
    h1 = seed & 0xFFFFFFFF
    nblocks = len(data) // 4
    for i in range(nblocks):
        k1 = int.from_bytes(data[4 * i:4 * i + 4], "little")
        k1 = (k1 * c1) & 0xFFFFFFFF
        k1 = rotl(k1, 15)
        k1 = (k1 * c2) & 0xFFFFFFFF
        h1 ^= k1
        h1 = rotl(h1, 13)
        h1 = (h1 * 5 + 0xE6546B64) & 0xFFFFFFFF
    tail = data[nblocks * 4:]
    k1 = 0
    if len(tail) >= 3:
        k1 ^= tail[2] << 16
    if len(tail) >= 2:
        k1 ^= tail[1] << 8
    if len(tail) >= 1:
        k1 ^= tail[0]
        k1 = (k1 * c1) & 0xFFFFFFFF
        k1 = rotl(k1, 15)
        k1 = (k1 * c2) & 0xFFFFFFFF
        h1 ^= k1
    h1 ^= len(data)
    h1 ^= h1 >> 16
    h1 = (h1 * 0x85EBCA6B) & 0xFFFFFFFF
    h1 ^= h1 >> 13
    h1 = (h1 * 0xC2B2AE35) & 0xFFFFFFFF
    h1 ^= h1 >> 16
    return h1


@pytest.fixture(scope="module")
def murmur():
    """The Python restatement, admitted only after it reproduces every
    published vector."""
    with open(os.path.join(GOLDEN, "murmur3_public_vectors.json")) as fh:
        fixture = json.load(fh)
    assert len(fixture["vectors"]) >= 13
    for vec in fixture["vectors"]:
        data = (bytes.fromhex(vec["data_hex"]) if "data_hex" in vec
                else vec["data_utf8"].encode())
        assert _murmur3_x86_32(data, int(vec["seed"], 16)) == int(vec["hash"], 16), vec
    return _murmur3_x86_32


def _check_hash(dj, murmur, strings, seeds=(0, SEED_HI), shift=0):
    """Hash `strings` on the GPU (chars placed `shift` bytes into their
    allocation) and compare every row with the Python hash."""
    L = dj.lib()
    n = len(strings)
    if shift:
        # one extra leading row owns the first `shift` bytes; the column under
        # test starts after it, at an unaligned chars pointer
        off_p, ch_p, nb = dj.upload_strings([b"\xEE" * shift] + list(strings))
        offsets = np.zeros(n + 1, dtype=np.int32)
        np.cumsum([len(s) for s in strings], out=offsets[1:])
        L.dj_memcpy_h2d(off_p, offsets.ctypes.data, offsets.nbytes)
        chars_p, chars_bytes = ch_p + shift, nb - shift
    else:
        off_p, ch_p, nb = dj.upload_strings(strings)
        chars_p, chars_bytes = ch_p, nb
    try:
        for seed in seeds:
            got = dj.hash_strings(off_p, chars_p, chars_bytes, n, seed)
            want = np.array([murmur(s, seed) for s in strings], dtype=np.uint32)
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, (hex(seed), int(bad[0]), strings[int(bad[0])][:32])
    finally:
        L.dj_dfree(off_p)
        L.dj_dfree(ch_p)


def _random_bytes(rng, length):
    b = bytearray(rng.randint(0, 256, length, dtype=np.int64).astype(np.uint8).tobytes())
    if length >= 2:
        b[rng.randint(0, length)] = 0x00   # embedded zero byte
        b[rng.randint(0, length)] = 0xF3   # byte >= 0x80
    return bytes(b)


def test_hash_every_length_at_every_alignment(dj, murmur):
    # lengths 0..13 (every tail length, 0-3 blocks) at every start alignment
    # 0..7: a pad row moves the next row's start to the wanted residue
    rng = np.random.RandomState(11)
    rows, pos = [], 0
    for align in range(8):
        for length in range(14):
            pad = (align - pos) % 8
            if pad:
                rows.append(_random_bytes(rng, pad))
                pos += pad
            rows.append(_random_bytes(rng, length))
            pos += length
    rows += [b"\x00", b"\x00\x00\x00\x00", b"\xff\xfe\xfd\xfc\xfb", b""]
    # the last row is empty and starts at chars_bytes
    assert rows[-1] == b""
    _check_hash(dj, murmur, rows)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 5000])
def test_hash_row_counts(dj, murmur, n):
    rng = np.random.RandomState(100 + n)
    rows = [_random_bytes(rng, int(k)) for k in rng.randint(0, 14, n)]
    _check_hash(dj, murmur, rows, seeds=(0, SEED_HI, 12345678))


def test_hash_mid_rows_stage_in_smaller_spans(dj, murmur):
    # 3000 rows of 14-26 B: 2048 rows (~40 KiB) exceed the 32 KiB LDS budget,
    # so the block stages 1024-row and shorter spans, several rows per thread
    rng = np.random.RandomState(15)
    rows = [_random_bytes(rng, int(k)) for k in rng.randint(14, 27, 3000)]
    _check_hash(dj, murmur, rows)


def test_hash_long_rows_take_the_direct_path(dj, murmur):
    # 256 rows x ~200 B = ~50 KiB > the 32 KiB LDS budget: the first block
    # reads global memory directly, the 44-row remainder block stages
    rng = np.random.RandomState(12)
    rows = [_random_bytes(rng, int(k)) for k in rng.randint(190, 211, 300)]
    _check_hash(dj, murmur, rows)


def test_hash_one_huge_row_between_short_rows(dj, murmur):
    # blocks 0 and 2 stage; block 1 holds the 100 000-byte row and goes direct
    rng = np.random.RandomState(13)
    rows = [_random_bytes(rng, int(k)) for k in rng.randint(0, 9, 700)]
    rows[300] = _random_bytes(rng, 100_000)
    _check_hash(dj, murmur, rows)


def test_hash_unaligned_chars_pointer(dj, murmur):
    rng = np.random.RandomState(14)
    rows = [_random_bytes(rng, int(k)) for k in rng.randint(0, 30, 1000)] + [b""]
    _check_hash(dj, murmur, rows, shift=3)


# ------------------------------------------------------------- join helpers

def _vocabulary(count):
    """`count` distinct key strings: the empty string, prefixes of each
    other, an embedded zero, equal-length strings that differ only in the
    last byte, bytes >= 0x80, and lengths 0..20."""
    vocab = [b"", b"ab", b"abc", b"ab\x00", b"a", b"abcd", b"abce", b"\x00", b"\x00\x00",
             b"caf\xc3\xa9", b"\xff\xff\xff\xff"]
    stem = b"same-sixteen-byt"
    vocab += [stem + bytes([c]) for c in range(0x30, 0x3A)]
    j = 0
    while len(vocab) < count:
        s = (b"key-%d-" % j) + b"x" * (j % 11)
        vocab.append(s[:20] if j % 3 else s)
        j += 1
    vocab = list(dict.fromkeys(vocab))
    assert len(vocab) >= count
    return vocab[:count]


def _decode(col):
    off, ch = col
    raw = ch.tobytes()
    return [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _ids(strings, index):
    return np.fromiter((index[s] for s in strings), dtype=np.int64, count=len(strings))


class _Dev:
    """Device columns of one test table, freed together."""

    def __init__(self, dj):
        self.dj, self.cols, self._arrays, self._ptrs = dj, [], [], []

    def i64(self, a):
        d = self.dj.DeviceArray.from_numpy(np.asarray(a, dtype=np.int64))
        self._arrays.append(d)
        self.cols.append((self.dj.TYPE_INT64, d.ptr))

    def i32(self, a):
        a32 = np.ascontiguousarray(a, dtype=np.int32)
        d = self.dj.DeviceArray((len(a32) + 1) // 2)
        if len(a32):
            self.dj.lib().dj_memcpy_h2d(d.ptr, a32.ctypes.data, a32.nbytes)
        self._arrays.append(d)
        self.cols.append((self.dj.TYPE_INT32, d.ptr))

    def strs(self, strings):
        off_p, ch_p, nb = self.dj.upload_strings(strings)
        self._ptrs += [off_p, ch_p]
        self.cols.append((self.dj.TYPE_STRING, off_p, ch_p, nb))

    def free(self):
        for d in self._arrays:
            d.free()
        for p in self._ptrs:
            self.dj.lib().dj_dfree(p)


def _assert_rows_equal(got_cols, want_cols):
    got = [np.asarray(c, dtype=np.int64) for c in got_cols]
    want = [np.asarray(c, dtype=np.int64) for c in want_cols]
    assert len(got[0]) == len(want[0]), (len(got[0]), len(want[0]))
    for a, b in zip(oracle.sort_rows(*got), oracle.sort_rows(*want)):
        assert (a == b).all()


def _single_key_case(dj, comm, lkeys, rkeys, vocab):
    """left = (payload INT64, key STRING) joined on column 1;
    right = (key STRING, payload INT64) joined on column 0. Returns the
    decoded output and the oracle's, as id columns."""
    index = {s: i for i, s in enumerate(vocab)}
    lp = np.arange(len(lkeys), dtype=np.int64) * 3 + 1
    rp = np.arange(len(rkeys), dtype=np.int64) * 5 + 2
    left, right = _Dev(dj), _Dev(dj)
    left.i64(lp)
    left.strs(lkeys)
    right.strs(rkeys)
    right.i64(rp)
    try:
        got = dj.cpp_distributed_inner_join_cols_multi(comm, left.cols, len(lkeys), right.cols,
                                                       len(rkeys), [1], [0])
    finally:
        left.free()
        right.free()
    assert len(got) == 4
    assert isinstance(got[1], tuple) and isinstance(got[2], tuple)   # STRING key columns
    got_ids = (_ids(_decode(got[1]), index), got[0], _ids(_decode(got[2]), index), got[3])
    want = oracle.inner_join(_ids(lkeys, index), lp, _ids(rkeys, index), rp)
    return got, got_ids, want


def test_single_string_key_join(dj, comm):
    n = 20_000
    vocab = _vocabulary(3000)
    rng = np.random.RandomState(21)
    lkeys = [vocab[i] for i in rng.randint(0, 3000, n)]
    rkeys = [vocab[i] for i in rng.randint(0, 3000, n)]
    _, got_ids, want = _single_key_case(dj, comm, lkeys, rkeys, vocab)
    assert len(want[0]) > n   # duplicates on both sides
    _assert_rows_equal(got_ids, want)


def _composite_case(dj, comm, n, order, seed):
    """Composite key with a STRING payload on the left.
    order "int_str": keys (INT64, STRING); "str_int": keys (STRING, INT32)."""
    vocab = _vocabulary(60)
    index = {s: i for i, s in enumerate(vocab)}
    rng = np.random.RandomState(seed)
    lnum, rnum = rng.randint(-25, 25, n), rng.randint(-25, 25, n)
    lstr = [vocab[i] for i in rng.randint(0, 60, n)]
    rstr = [vocab[i] for i in rng.randint(0, 60, n)]
    lpay = [b"p%d" % i for i in range(n)]          # STRING payload, decodes to the row
    rp = np.arange(n, dtype=np.int64) * 7
    left, right = _Dev(dj), _Dev(dj)
    if order == "int_str":
        left.i64(lnum)
        left.strs(lstr)
        right.i64(rnum)
        right.strs(rstr)
        num_col, str_col = 0, 1
    else:
        left.strs(lstr)
        left.i32(lnum)
        right.strs(rstr)
        right.i32(rnum)
        num_col, str_col = 1, 0
    left.strs(lpay)
    right.i64(rp)
    try:
        got = dj.cpp_distributed_inner_join_cols_multi(comm, left.cols, n, right.cols, n,
                                                       [0, 1], [0, 1])
    finally:
        left.free()
        right.free()
    assert len(got) == 6
    got_rows = (np.asarray(got[num_col], dtype=np.int64), _ids(_decode(got[str_col]), index),
                np.fromiter((int(s[1:]) for s in _decode(got[2])), dtype=np.int64,
                            count=len(got[3 + num_col])),
                np.asarray(got[3 + num_col], dtype=np.int64),
                _ids(_decode(got[3 + str_col]), index), got[5])
    # oracle on a collision-free combined id: (num + 25) * 64 + string id
    comb_l = (lnum.astype(np.int64) + 25) * 64 + _ids(lstr, index)
    comb_r = (rnum.astype(np.int64) + 25) * 64 + _ids(rstr, index)
    c0, c1, c2, c3 = oracle.inner_join(comb_l, np.arange(n, dtype=np.int64), comb_r, rp)
    want_rows = (c0 // 64 - 25, c0 % 64, c1, c2 // 64 - 25, c2 % 64, c3)
    assert len(c0) > n
    _assert_rows_equal(got_rows, want_rows)
    return len(c0)


@pytest.mark.parametrize("order", ["int_str", "str_int"])
def test_composite_key_with_string(dj, comm, order):
    _composite_case(dj, comm, 20_000, order, seed=31)


def test_string_collision_filter_under_weak_fuse(dj):
    """DJ_TEST_WEAK_FUSE collapses the fused key to 4 bits: nearly every
    candidate pair is a hash collision and the string compare decides.
    Subprocess: the switch is read once per process."""
    script = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import distributed_join_amd as dj
import test_gpu_string_keys as T
dj.require_gpu()
comm = dj.CppCommunicator(0, 1)
rows = T._composite_case(dj, comm, 5000, "int_str", seed=41)
comm.destroy()
print("WEAK_FUSE_STR_OK", rows)
""" % (REPO, os.path.join(REPO, "tests"))
    env = dict(os.environ, DJ_TEST_WEAK_FUSE="1")
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "WEAK_FUSE_STR_OK" in r.stdout


# -------------------------------------------------------------- edge tables

def _assert_typed_empty(got):
    assert len(got) == 4
    assert len(got[0]) == 0 and len(got[3]) == 0
    for c in (got[1], got[2]):
        assert isinstance(c, tuple)
        assert len(c[0]) == 1 and c[0][0] == 0 and len(c[1]) == 0


def test_empty_left(dj, comm):
    vocab = _vocabulary(20)
    got, _, _ = _single_key_case(dj, comm, [], vocab * 5, vocab)
    _assert_typed_empty(got)


def test_empty_right(dj, comm):
    vocab = _vocabulary(20)
    got, _, _ = _single_key_case(dj, comm, vocab * 5, [], vocab)
    _assert_typed_empty(got)


def test_all_keys_empty_strings_cross_join(dj, comm):
    # chars_bytes == 0 on both sides; 300 x 300 rows all match
    got, got_ids, want = _single_key_case(dj, comm, [b""] * 300, [b""] * 300, [b""])
    assert len(want[0]) == 90_000
    assert len(got[1][1]) == 0 and len(got[2][1]) == 0
    _assert_rows_equal(got_ids, want)


def test_no_matches(dj, comm):
    vocab = _vocabulary(400)
    rng = np.random.RandomState(51)
    lkeys = [vocab[i] for i in rng.randint(0, 200, 3000)]
    rkeys = [vocab[i] for i in rng.randint(200, 400, 3000)]
    got, _, want = _single_key_case(dj, comm, lkeys, rkeys, vocab)
    assert len(want[0]) == 0
    _assert_typed_empty(got)


# ----------------------------------------------------------------- shuffle

def test_shuffle_on_string_key_world1(dj, comm):
    """At world 1 the shuffled table is a permutation of the input, with
    and without the compressed wire."""
    n = 5000
    vocab = _vocabulary(500)
    index = {s: i for i, s in enumerate(vocab)}
    rng = np.random.RandomState(61)
    keys = [vocab[i] for i in rng.randint(0, 500, n)]
    pay = np.arange(n, dtype=np.int64)
    want = oracle.sort_rows(_ids(keys, index), pay)
    tbl = _Dev(dj)
    tbl.i64(pay)
    tbl.strs(keys)
    try:
        for compression in (False, True):
            got = dj.cpp_shuffle_on_cols(comm, tbl.cols, n, [1], dj.HASH_MURMUR3,
                                         dj.SEED_INTRA, compression)
            assert len(got) == 2 and len(got[0]) == n
            rows = oracle.sort_rows(_ids(_decode(got[1]), index),
                                    np.asarray(got[0], dtype=np.int64))
            for a, b in zip(rows, want):
                assert (a == b).all()
    finally:
        tbl.free()


# --------------------------------------------------------------- multi-rank

def test_stringkey_loopback(dj):
    """G ranks as threads over a loopback Communicator
    (tests/cpp/stringkey_loopback.cpp): after shuffle_on every distinct key
    string lives on one rank; the concatenated distributed_inner_join equals
    the single-rank result."""
    exe = cpp_programs.build("stringkey_loopback")
    # (G, nvlink_domain_size, compression)
    for args in (["2", "2", "0"], ["4", "4", "0"],
                 ["4", "2", "0"],    # 2-level hierarchy
                 ["4", "1", "0"],    # full shuffle + local join
                 ["2", "2", "1"]):   # compressed wire
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr
        assert "STRINGKEY LOOPBACK OK" in r.stdout
