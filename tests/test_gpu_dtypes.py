"""GPU tests of the fixed-width column types (1/2/4/8 bytes): the table
gather kernel, payload integrity through the join, narrow and unsigned keys,
the -1 sentinel under skew, shuffle placement, the cascaded codec at 1- and
2-byte elements, and the multi-rank loopback harness.

Every comparison is bit-exact: floats are compared through their unsigned
integer view and carry NaN payloads, -0.0, +-inf and denormals, so "moved
verbatim" is what is tested.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cpp_programs
import oracle

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


UINT_OF_WIDTH = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def bits(a):
    """Unsigned-integer view of a column, for bit-exact comparison."""
    return np.ascontiguousarray(a).view(UINT_OF_WIDTH[a.dtype.itemsize])


def random_bits(rng, n, dtype):
    """n elements of dtype with uniformly random bit patterns."""
    dtype = np.dtype(dtype)
    raw = rng.randint(0, 256, n * dtype.itemsize).astype(np.uint8)
    return raw.view(dtype).copy()


def float_column(rng, n, dtype):
    """Random bit patterns (NaNs with payloads included) with the special
    values planted at the front."""
    a = random_bits(rng, n, dtype)
    u = UINT_OF_WIDTH[a.dtype.itemsize]
    if a.dtype == np.float64:
        special = np.array([0x7FF8000000000001, 0xFFF0DEADBEEF0001, 0x7FF0000000000001,
                            0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                            0x0000000000000001, 0x800FFFFFFFFFFFFF, 0], dtype=u)
    else:
        special = np.array([0x7FC00001, 0xFFC0BEEF, 0x7F800001, 0x80000000, 0x7F800000,
                            0xFF800000, 0x00000001, 0x807FFFFF, 0], dtype=u)
    k = min(n, len(special))
    a.view(u)[:k] = special[:k]
    return a


# ------------------------------------------------------------ 1. gather kernel

GUARD = 64  # bytes of known pattern after every destination


class _Dst:
    def __init__(self, L, n, width):
        self.L, self.n, self.width = L, n, width
        self.nbytes = n * width + GUARD
        self.ptr = L.dj_dmalloc(self.nbytes)
        fill = np.full(self.nbytes, 0x5A, dtype=np.uint8)
        fill[n * width:] = 0xA5
        L.dj_memcpy_h2d(self.ptr, fill.ctypes.data, self.nbytes)

    def read(self):
        out = np.empty(self.nbytes, dtype=np.uint8)
        self.L.dj_memcpy_d2h(out.ctypes.data, self.ptr, self.nbytes)
        self.L.dj_dfree(self.ptr)
        body = out[:self.n * self.width].view(UINT_OF_WIDTH[self.width])
        return body, out[self.n * self.width:]


def _gather_case(dj, rng, n, mode, widths, offsets, idx):
    L = dj.lib()
    m = 1000 + n // 2  # fewer source rows than output rows at large n: repeats
    idx = idx % m
    d_idx = dj.DeviceArray.from_numpy(idx)
    srcs, dsts, descs = [], [], []
    for w, off in zip(widths, offsets):
        host = random_bits(rng, m, UINT_OF_WIDTH[w])
        col = dj.DeviceColumn(host, offset_elems=off)
        dst = _Dst(L, n, w)
        srcs.append((host, col))
        dsts.append(dst)
        descs.append((col.ptr, dst.ptr, w))
    dj.gather_columns(descs, d_idx.ptr, n, mode)
    for (host, col), dst, w, off in zip(srcs, dsts, widths, offsets):
        body, guard = dst.read()
        assert (guard == 0xA5).all(), f"guard band overwritten: width {w} n {n} mode {mode}"
        assert (body == host[idx]).all(), f"gather mismatch: width {w} off {off} n {n}"
        col.free()
    d_idx.free()


@pytest.mark.parametrize("mode", [0, 1], ids=["fused", "per_column"])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 7, 63, 64, 65, 1021, 100003])
def test_gather_kernel(dj, n, mode):
    rng = np.random.RandomState(1000 + n)
    idx_kinds = {
        "repeats": rng.randint(0, 1 << 40, n).astype(np.int64),
        "all_equal": np.full(n, 12345, dtype=np.int64),
    }
    for idx in idx_kinds.values():
        # one column, every width x every source offset (0, 1, 3 elements)
        for w in (1, 2, 4, 8):
            for off in (0, 1, 3):
                _gather_case(dj, rng, n, mode, [w], [off], idx)
        # a 9-column mix of all widths in one call, offsets mixed
        _gather_case(dj, rng, n, mode, [8, 1, 4, 2, 1, 8, 2, 4, 1],
                     [0, 1, 3, 1, 3, 1, 0, 0, 0], idx)


@pytest.mark.parametrize("n", [3, 65, 1021, 100003])
def test_gather_engine_routing(dj, n):
    # mode 2: the per-width routing the join and partition paths use
    rng = np.random.RandomState(2000 + n)
    _gather_case(dj, rng, n, 2, [8, 1, 4, 2, 1, 8, 2, 4, 1], [0, 1, 3, 1, 3, 1, 0, 0, 0],
                 rng.randint(0, 1 << 40, n).astype(np.int64))


def test_gather_more_columns_than_one_descriptor(dj):
    # 35 columns: the fused path splits into two launches (32-entry descriptor)
    rng = np.random.RandomState(7)
    n = 1021
    widths = [(1, 2, 4, 8)[i % 4] for i in range(35)]
    _gather_case(dj, rng, n, 0, widths, [i % 3 for i in range(35)],
                 rng.randint(0, 1 << 40, n).astype(np.int64))


# ------------------------------------------ 2. payload integrity through the join

N_JOIN = 50_000


@pytest.fixture(scope="module")
def typed_tables(dj):
    """Host columns + device columns of the two typed tables, and the oracle
    join of their (key, rowid) columns — computed once, never modified."""
    rng = np.random.RandomState(11)
    lk, _ = oracle.gen_build(N_JOIN)
    rk, _ = oracle.gen_probe(N_JOIN, N_JOIN, selectivity=0.3)
    rowid = np.arange(N_JOIN, dtype=np.int64)

    def k2(k):  # a function of the key: (key, k2) equality == key equality
        return (k % 1000 - 500).astype(np.int16)

    left = [(dj.TYPE_INT64, lk), (dj.TYPE_INT64, rowid),
            (dj.TYPE_FLOAT64, float_column(rng, N_JOIN, np.float64)),
            (dj.TYPE_FLOAT32, float_column(rng, N_JOIN, np.float32)),
            (dj.TYPE_INT16, k2(lk)),
            (dj.TYPE_UINT8, random_bits(rng, N_JOIN, np.uint8)),
            (dj.TYPE_BOOL8, (random_bits(rng, N_JOIN, np.uint8) & 1).astype(np.uint8)),
            (dj.TYPE_UINT32, random_bits(rng, N_JOIN, np.uint32))]
    right = [(dj.TYPE_INT64, rk), (dj.TYPE_INT64, rowid),
             (dj.TYPE_FLOAT32, float_column(rng, N_JOIN, np.float32)),
             (dj.TYPE_INT8, random_bits(rng, N_JOIN, np.int8)),
             (dj.TYPE_INT16, k2(rk)),
             (dj.TYPE_UINT16, random_bits(rng, N_JOIN, np.uint16)),
             (dj.TYPE_FLOAT64, float_column(rng, N_JOIN, np.float64)),
             (dj.TYPE_UINT64, random_bits(rng, N_JOIN, np.uint64))]
    dl = [dj.DeviceColumn(a, t) for t, a in left]
    dr = [dj.DeviceColumn(a, t) for t, a in right]
    want = oracle.sort_rows(*oracle.inner_join(lk, rowid, rk, rowid))
    yield left, right, dl, dr, want
    for c in dl + dr:
        c.free()


def _check_typed_result(dj, got, left, right, want):
    nl = len(left)
    assert len(got) == nl + len(right)
    for (t, _), col in zip(left + right, got):
        assert col.dtype == dj.NUMPY_DTYPE[t], (t, col.dtype)
    g = oracle.sort_rows(got[0], got[1], got[nl], got[nl + 1])
    assert len(g[0]) == len(want[0]) and len(want[0]) > 0
    for a, b in zip(g, want):
        assert (a == b).all()
    lrow, rrow = got[1], got[nl + 1]
    for c, (t, host) in enumerate(left):
        assert (bits(got[c]) == bits(host)[lrow]).all(), f"left column {c} (type {t})"
    for c, (t, host) in enumerate(right):
        assert (bits(got[nl + c]) == bits(host)[rrow]).all(), f"right column {c} (type {t})"


@pytest.mark.parametrize("over_decom", [1, 4])
def test_join_payload_integrity(dj, comm, typed_tables, over_decom):
    left, right, dl, dr, want = typed_tables
    got = dj.cpp_distributed_inner_join_cols(comm, [c.desc for c in dl], N_JOIN,
                                             [c.desc for c in dr], N_JOIN,
                                             over_decom=over_decom)
    _check_typed_result(dj, got, left, right, want)


def test_join_payload_integrity_multikey(dj, comm, typed_tables):
    # (INT64 key, INT16 k2) composite key: down the multi-key gather
    left, right, dl, dr, want = typed_tables
    got = dj.cpp_distributed_inner_join_cols_multi(comm, [c.desc for c in dl], N_JOIN,
                                                   [c.desc for c in dr], N_JOIN,
                                                   [0, 4], [0, 4])
    _check_typed_result(dj, got, left, right, want)


# ------------------------------------------------- 3. narrow and unsigned keys

def np_join_pairs(lk, rk):
    """(left row, right row) pairs of the inner join, in numpy."""
    order = np.argsort(rk, kind="stable")
    rs = rk[order]
    lo = np.searchsorted(rs, lk, "left")
    hi = np.searchsorted(rs, lk, "right")
    cnt = hi - lo
    li = np.repeat(np.arange(len(lk), dtype=np.int64), cnt)
    within = np.arange(cnt.sum(), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    ri = order[np.repeat(lo, cnt) + within].astype(np.int64)
    return li, ri


def extend(a):
    """The engine's int64 key of an integer column: sign extension for signed
    types, zero extension for unsigned ones, reinterpretation for uint64."""
    if a.dtype == np.uint64:
        return a.view(np.int64)
    return a.astype(np.int64)


def _key_case(dj, rng, dtype):
    dtype = np.dtype(dtype)
    info = np.iinfo(dtype)
    if dtype.itemsize == 1:
        n = 3000
        lk, rk = random_bits(rng, n, dtype), random_bits(rng, n, dtype)
    elif dtype.itemsize == 2:
        n = 20000
        lk, rk = random_bits(rng, n, dtype), random_bits(rng, n, dtype)
    elif dtype == np.uint32:
        n = 20000
        lk = (2**31 + rng.randint(0, 30000, n)).astype(np.uint32)
        rk = (2**31 + rng.randint(0, 30000, n)).astype(np.uint32)
        lk[:3] = rk[:3] = info.max
    else:
        n = 20000
        lk = (np.uint64(2**63) + rng.randint(0, 30000, n).astype(np.uint64))
        rk = (np.uint64(2**63) + rng.randint(0, 30000, n).astype(np.uint64))
        # 0xFFFF...FFFF is the engine's sentinel after reinterpretation
        lk[:5] = rk[:7] = info.max
    if info.min < 0:
        lk[10:14] = -1
        rk[20:23] = -1
    return n, lk, rk


@pytest.mark.parametrize("dtype", [np.int8, np.uint8, np.int16, np.uint16, np.uint32, np.uint64],
                         ids=lambda d: np.dtype(d).name)
def test_narrow_and_unsigned_keys(dj, comm, dtype):
    rng = np.random.RandomState(31)
    n, lk, rk = _key_case(dj, rng, dtype)
    rowid = np.arange(n, dtype=np.int64)
    dl = [dj.DeviceColumn(lk), dj.DeviceColumn(rowid)]
    dr = [dj.DeviceColumn(rk), dj.DeviceColumn(rowid)]
    got = dj.cpp_distributed_inner_join_cols(comm, [c.desc for c in dl], n,
                                             [c.desc for c in dr], n)
    li, ri = np_join_pairs(extend(lk), extend(rk))
    if np.dtype(dtype).itemsize == 1:
        assert 25_000 < len(li) < 50_000
    assert len(li) > 0
    # output key columns come back in their own dtype, with their own values
    assert got[0].dtype == np.dtype(dtype) and got[2].dtype == np.dtype(dtype)
    assert len(got[1]) == len(li)
    g = oracle.sort_rows(got[1], got[3])
    w = oracle.sort_rows(li, ri)
    assert (g[0] == w[0]).all() and (g[1] == w[1]).all()
    assert (got[0] == lk[got[1]]).all()
    assert (got[2] == rk[got[3]]).all()
    for c in dl + dr:
        c.free()


def test_composite_int16_uint8_key(dj, comm):
    rng = np.random.RandomState(37)
    n = 20000
    l1 = rng.randint(-40, 40, n).astype(np.int16)
    r1 = rng.randint(-40, 40, n).astype(np.int16)
    l2 = rng.randint(200, 256, n).astype(np.uint8)
    r2 = rng.randint(200, 256, n).astype(np.uint8)
    rowid = np.arange(n, dtype=np.int64)
    dl = [dj.DeviceColumn(l1), dj.DeviceColumn(l2), dj.DeviceColumn(rowid)]
    dr = [dj.DeviceColumn(r1), dj.DeviceColumn(r2), dj.DeviceColumn(rowid)]
    got = dj.cpp_distributed_inner_join_cols_multi(comm, [c.desc for c in dl], n,
                                                   [c.desc for c in dr], n, [0, 1], [0, 1])
    li, ri = np_join_pairs(l1.astype(np.int64) * 256 + l2, r1.astype(np.int64) * 256 + r2)
    assert len(li) > 0 and len(got[2]) == len(li)
    g = oracle.sort_rows(got[2], got[5])
    w = oracle.sort_rows(li, ri)
    assert (g[0] == w[0]).all() and (g[1] == w[1]).all()
    assert got[0].dtype == np.int16 and got[1].dtype == np.uint8
    assert (got[0] == l1[got[2]]).all() and (got[1] == l2[got[2]]).all()
    assert (got[3] == r1[got[5]]).all() and (got[4] == r2[got[5]]).all()
    for c in dl + dr:
        c.free()


_RAISE_SCRIPT = """
import sys
sys.path.insert(0, %r)
import numpy as np
import distributed_join_amd as dj
dj.require_gpu()
comm = dj.CppCommunicator(0, 1)
n = 1000
case = sys.argv[1]
rowid = dj.DeviceColumn(np.arange(n, dtype=np.int64))
if case == "float64_key":
    k = dj.DeviceColumn(np.arange(n, dtype=np.float64))
    dj.cpp_distributed_inner_join_cols(comm, [k.desc, rowid.desc], n, [k.desc, rowid.desc], n)
elif case == "float64_shuffle_key":
    k = dj.DeviceColumn(np.arange(n, dtype=np.float64))
    dj.cpp_shuffle_on_cols(comm, [k.desc, rowid.desc], n, [0])
elif case == "int16_with_int32":
    a = dj.DeviceColumn(np.arange(n, dtype=np.int16))
    b = dj.DeviceColumn(np.arange(n, dtype=np.int32))
    dj.cpp_distributed_inner_join_cols(comm, [a.desc, rowid.desc], n, [b.desc, rowid.desc], n)
elif case == "cascaded_on_float64":
    k = dj.DeviceColumn(np.arange(n, dtype=np.int64))
    f = dj.DeviceColumn(np.arange(n, dtype=np.float64))
    dj.cpp_shuffle_on_cols(comm, [k.desc, f.desc], n, [0], compression=3)
print("NO ERROR RAISED")
""" % REPO


@pytest.mark.parametrize("case,message", [
    ("float64_key", "cannot be join/shuffle keys"),
    ("float64_shuffle_key", "cannot be join/shuffle keys"),
    ("int16_with_int32", "must have the same type on both sides"),
    ("cascaded_on_float64", "Unsupported type for cascaded compressor"),
])
def test_loud_errors(case, message):
    # the engine's loud errors end the process: run each in a child
    r = subprocess.run([sys.executable, "-c", _RAISE_SCRIPT, case], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "NO ERROR RAISED" not in r.stdout
    assert message in r.stderr, r.stderr


# ------------------------------------------------------ 4. sentinel under skew

def test_sentinel_under_skew(dj, comm):
    # kJoinBucketRowCap (dj_kernels.hpp) is the LDS join's per-bucket build-row
    # cap: a bucket with more build rows is skew-flagged and joined by the
    # global-table fallback. -1 occurs on the build side more often than twice
    # that cap, so the bucket holding the sentinel takes the fallback, which is
    # then the only place that sees the -1 rows.
    hpp = open(os.path.join(REPO, "distributed_join_amd", "csrc", "dj_kernels.hpp")).read()
    cap = int(re.search(r"kJoinBucketRowCap\s*=\s*(\d+)", hpp).group(1))
    n = 100_000
    n_build_neg1, n_probe_neg1 = 2 * cap + 128, 64
    rng = np.random.RandomState(41)
    bk, _ = oracle.gen_build(n)
    pk, _ = oracle.gen_probe(n, n, selectivity=0.3)
    bk = np.concatenate([bk, np.full(n_build_neg1, -1, dtype=np.int64)])
    pk = np.concatenate([pk, np.full(n_probe_neg1, -1, dtype=np.int64)])
    bk = bk[rng.permutation(len(bk))]
    pk = pk[rng.permutation(len(pk))]
    bp = np.arange(len(bk), dtype=np.int64)
    pp = np.arange(len(pk), dtype=np.int64) + 10**9
    dbk, dbp = dj.DeviceArray.from_numpy(bk), dj.DeviceArray.from_numpy(bp)
    dpk, dpp = dj.DeviceArray.from_numpy(pk), dj.DeviceArray.from_numpy(pp)
    got = dj.cpp_distributed_inner_join(comm, dbk, dbp, len(bk), dpk, dpp, len(pk))
    want = oracle.inner_join(bk, bp, pk, pp)
    g = oracle.sort_rows(*got)
    w = oracle.sort_rows(*want)
    assert int((w[0] == -1).sum()) == n_build_neg1 * n_probe_neg1
    assert len(g[0]) == len(w[0]), (len(g[0]), len(w[0]))
    for a, b in zip(g, w):
        assert (a == b).all()


# -------------------------------------------------------------- 5. shuffle_on

def murmur3_int64(keys, seed):
    """dj_hash.h dj_murmur3_int64, vectorised."""
    u = keys.astype(np.int64).view(np.uint64)
    blocks = [(u & np.uint64(0xFFFFFFFF)).astype(np.uint32), (u >> np.uint64(32)).astype(np.uint32)]
    h = np.full(len(u), seed, dtype=np.uint32)

    def rotl(x, r):
        return (x << np.uint32(r)) | (x >> np.uint32(32 - r))
    with np.errstate(over="ignore"):
        for k in blocks:
            k = k * np.uint32(0xCC9E2D51)
            k = rotl(k, 15)
            k = k * np.uint32(0x1B873593)
            h = h ^ k
            h = rotl(h, 13)
            h = h * np.uint32(5) + np.uint32(0xE6546B64)
        h = h ^ np.uint32(8)
        h ^= h >> np.uint32(16)
        h = h * np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h = h * np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return h


def spec_partition(keys, hash_fn, seed, nparts):
    ext = extend(keys)
    if hash_fn == 1:  # HASH_IDENTITY: (uint32_t) of the extended value
        h = ext.view(np.uint64).astype(np.uint32)
    else:
        h = murmur3_int64(ext, seed)
    return (h % np.uint32(nparts)).astype(np.int64)


def test_murmur3_numpy_matches_oracle():
    ks = np.array([0, 1, -1, 2**40 + 17, -2**62, 255, 65535], dtype=np.int64)
    for seed in (0, 12345678):
        mine = murmur3_int64(ks, seed)
        for k, h in zip(ks, mine):
            assert int(h) == oracle.row_hash(int(k), oracle.HASH_MURMUR3, seed)


@pytest.mark.parametrize("hash_fn", [0, 1], ids=["murmur3", "identity"])
@pytest.mark.parametrize("dtype", [np.int16, np.uint8], ids=["int16", "uint8"])
def test_shuffle_on_narrow_key(dj, comm, dtype, hash_fn):
    rng = np.random.RandomState(53)
    n, nparts, seed = 20011, 7, 12345678
    keys = random_bits(rng, n, dtype)
    f32 = np.arange(n, dtype=np.uint32).view(np.float32)  # bit pattern == row index
    u16 = random_bits(rng, n, np.uint16)
    cols = [dj.DeviceColumn(keys), dj.DeviceColumn(f32), dj.DeviceColumn(u16)]
    descs = [c.desc for c in cols]
    # placement step of shuffle_on over 7 partitions, against the dj_hash.h spec
    got, off = dj.cpp_partition_cols(descs, n, [0], nparts, hash_fn, seed)
    assert off[0] == 0 and off[-1] == n
    want_part = spec_partition(keys, hash_fn, seed, nparts)
    assert (np.diff(off) == np.bincount(want_part, minlength=nparts)).all()
    row = got[1].view(np.uint32).astype(np.int64)
    got_part = np.repeat(np.arange(nparts), np.diff(off))
    assert (want_part[row] == got_part).all()
    assert (np.sort(row) == np.arange(n)).all()          # no row lost
    for p in range(nparts):                               # stable inside a partition
        assert (np.diff(row[off[p]:off[p + 1]]) > 0).all()
    assert got[0].dtype == np.dtype(dtype) and got[2].dtype == np.uint16
    assert (got[0] == keys[row]).all() and (got[2] == u16[row]).all()
    # the whole shuffle_on at world size 1
    sh = dj.cpp_shuffle_on_cols(comm, descs, n, [0], hash_fn, seed)
    row = sh[1].view(np.uint32).astype(np.int64)
    assert (np.sort(row) == np.arange(n)).all()
    assert (sh[0] == keys[row]).all() and (sh[2] == u16[row]).all()
    for c in cols:
        c.free()


# ------------------------------------------------------------------- 6. codec

CASCADE_CONFIGS = [(r, d, b) for r in (0, 1) for d in (0, 1) for b in (0, 1)]


def _patterns(dtype):
    rng = np.random.RandomState(42)
    info = np.iinfo(dtype)
    n = 50_001
    return {
        "runs": np.repeat(rng.randint(0, 50, n // 100 + 1), 100)[:n].astype(dtype),
        "ramp": (np.arange(n) % (int(info.max) + 1)).astype(dtype),
        "sorted": np.sort(rng.randint(info.min, int(info.max) + 1, n)).astype(dtype),
        "random": rng.randint(info.min, int(info.max) + 1, n).astype(dtype),
        "negative": (-rng.randint(1, 100, n)).astype(dtype),
        "all_zero": np.zeros(n, dtype=dtype),
        "tiny": np.array([5], dtype=dtype),
        "odd_count": rng.randint(info.min, int(info.max) + 1, 1023).astype(dtype),
    }


@pytest.mark.parametrize("rles,deltas,bp", CASCADE_CONFIGS)
@pytest.mark.parametrize("dtype", [np.int8, np.int16], ids=["elem1", "elem2"])
def test_cascaded_roundtrip_narrow(dj, dtype, rles, deltas, bp):
    L = dj.lib()
    es = np.dtype(dtype).itemsize
    for name, arr in _patterns(dtype).items():
        n = len(arr)
        col = dj.DeviceColumn(arr)
        dst = _Dst(L, n, es)
        wire = L.dj_compress_roundtrip(col.ptr, n, es, rles, deltas, bp, dst.ptr)
        body, guard = dst.read()
        assert (guard == 0xA5).all(), (name, "store past the element width")
        assert (body == bits(arr)).all(), (name, rles, deltas, bp)
        assert wire <= n * es + 32, (name, wire)   # never larger than raw + header
        col.free()


def test_cascaded_narrow_actually_packs(dj):
    L = dj.lib()
    arr = np.repeat(np.arange(50, dtype=np.int16), 1000)
    col = dj.DeviceColumn(arr)
    dst = _Dst(L, len(arr), 2)
    wire = L.dj_compress_roundtrip(col.ptr, len(arr), 2, 1, 1, 1, dst.ptr)
    body, _ = dst.read()
    assert (body == bits(arr)).all()
    assert wire < len(arr) * 2 // 50
    col.free()


def test_compressed_shuffle_typed_columns(dj, comm):
    rng = np.random.RandomState(61)
    n = 30_001
    host = [np.arange(n, dtype=np.int64),                                  # key == row
            np.repeat(rng.randint(-5, 5, n // 50 + 1), 50)[:n].astype(np.int8),
            np.sort(random_bits(rng, n, np.int16)),
            float_column(rng, n, np.float64),
            (random_bits(rng, n, np.uint8) & 1).astype(np.uint8)]
    types = [dj.TYPE_INT64, dj.TYPE_INT8, dj.TYPE_INT16, dj.TYPE_FLOAT64, dj.TYPE_BOOL8]
    cols = [dj.DeviceColumn(a, t) for a, t in zip(host, types)]
    descs = [c.desc for c in cols]
    plain = dj.cpp_shuffle_on_cols(comm, descs, n, [0], compression=0)
    for mode in (1, 2):   # fixed policy, sampling auto-select
        comp = dj.cpp_shuffle_on_cols(comm, descs, n, [0], compression=mode)
        for a, b in zip(plain, comp):
            assert a.dtype == b.dtype and (bits(a) == bits(b)).all(), mode
    for a, h in zip(plain, host):
        assert (bits(a) == bits(h)[plain[0]]).all()
    for c in cols:
        c.free()


# ------------------------------------------------------------- 7. multi-rank

def test_dtype_loopback():
    exe = cpp_programs.build("dtype_loopback")
    # (G, nvlink_domain_size, compression); G = 3 gives odd slice boundaries
    for args in (["3", "3", "0"], ["4", "1", "0"], ["2", "2", "1"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, " ".join(args) + "\n" + r.stdout + r.stderr
        assert "DTYPE LOOPBACK OK" in r.stdout
