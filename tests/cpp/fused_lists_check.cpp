/*
 * fused_lists_check.cpp — the fused wire path's two partition steps called
 * directly and compared, exactly, with the host: dj::fused_partition
 * (fused_count_kernel, the two scans, fused_scatter_kernel) and
 * dj::subpart_lists over real per-peer segment lists.
 *
 * Host reference: slice of a key = (dj_murmur3_int64(key, seed) % nparts_rank)
 * * PA + groupA, bucket = groupA * F + subF, with groupA and subF the dj_mix64
 * bit fields documented at groupA_of / subF_of in dj_kernels.hip and restated
 * in bucket_model.hpp. Payloads
 * name the input row (7*i+3, or the row index under a null payload pointer),
 * so "the multiset of a slice equals the input's" is checked as: every stored
 * row equals its input row, sits in the slice its key asks for, and no input
 * row is stored twice while the row counts agree.
 *
 * fused_partition, per run: offsets[0] == 0, offsets[P] == n, non-decreasing;
 * every row of slice p*PA+g has murmur % nparts_rank == p and groupA == g; the
 * rows are the input's; 64 guard elements after each output column and 16
 * guard words after offsets[P] keep their poison.
 *
 * subpart_lists, per run, over a hand-built receive buffer laid out as
 * distributed_inner_join_fused's build_segs describes it (G peer slices end
 * to end behind a pad, so no offset is 0; PA runs by groupA inside each;
 * seg_bounds[G][PA+1] absolute; group_base[PA+1] the prefix sum of the group
 * totals): bucket_offsets[0] == 0, [PA*F] == total, non-decreasing; every row
 * of bucket g*F+j has groupA == g and subF == j; the rows are the laid-out
 * rows (never a pad row); 64 guard rows after out_pairs and 16 guard words
 * after bucket_offsets[PA*F] keep their poison.
 *
 * The chained case runs fused_partition on the tables of G = 2 ranks with
 * od = 2 (nparts_rank 4, PA 256), assembles rank 0's receive buffer of batch
 * 1 from the offset arrays as slice_of / subcounts_of index them, and runs
 * subpart_lists on it: the sender's group and the receiver's are the same bits.
 *
 * Sizes derive from dj::bucket_partition_shape().
 *
 * usage: fused_lists_check [--inputs-only | --bad-f F]
 *   --inputs-only: builds every input on the host, prints the chunk and
 *   segment shapes and fails if a named situation is absent (needs no GPU).
 *   --bad-f F: dj::subpart_lists with that F and nothing allocated;
 *   DJ_CHECK_ERROR must end the process with status 1 before any launch.
 * Build/run: tests/test_gpu_fused_lists.py.
 */
#include "bucket_model.hpp"
#include "check.hpp"

#include "dj_kernels.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <string>
#include <vector>

static dj::BucketPartitionShape g_sh;

static double g_slowest_ms = 0;
static size_t g_largest_bytes = 0;

/* ---------------- host reference ---------------- */

struct Fails {
  int bad = 0;
  void operator()(const char* what, long long a, long long b)
  {
    if (bad++ < 6) printf("  FAIL %s (%lld, %lld)\n", what, a, b);
  }
};

/* ---------------- fused_partition ---------------- */

struct FusedCase {
  int npr, PA;
  int64_t n;
  uint32_t seed;
  bool null_pay, all_equal;
};

static std::vector<FusedCase> fused_cases()
{
  const int64_t NB = g_sh.bucket_blocks, ST = g_sh.scatter_tile;
  const uint32_t intra = DJ_SEED_INTRA;
  std::vector<FusedCase> c;
  const int shapes[][2] = {{1, 1}, {4, 256}, {3, 256}, {80, 8}, {1024, 1}, {8, 128}};
  for (auto& s : shapes) c.push_back({s[0], s[1], 100003, intra, false, false});
  for (int64_t n : {(int64_t)1, NB - 1, NB + 1, NB * (ST - 1) - 5, NB * ST, NB * ST + 1})
    c.push_back({4, 256, n, intra, false, false});
  c.push_back({3, 256, 100003, DJ_DEFAULT_HASH_SEED, false, false});
  c.push_back({80, 8, 100003, intra, true, false});
  c.push_back({8, 128, 100003, intra, false, true});
  return c;
}

static void fused_inputs(const FusedCase& c, uint64_t stream, std::vector<int64_t>& keys,
                         std::vector<int64_t>& pay, int64_t pay_base = 0)
{
  keys.resize((size_t)c.n);
  pay.resize((size_t)c.n);
  for (int64_t i = 0; i < c.n; i++) {
    keys[(size_t)i] = hkey(stream, c.all_equal ? 0 : (uint64_t)i);
    pay[(size_t)i] = c.null_pay ? i : 7 * (i + pay_base) + 3;
  }
}

/* runs fused_partition and checks it; hands back the partitioned columns and
 * offsets (the chained case goes on from them) */
static int run_fused(const FusedCase& c, const std::vector<int64_t>& keys,
                     const std::vector<int64_t>& pay, int64_t pay_base,
                     std::vector<int64_t>* out_keys, std::vector<int64_t>* out_pay,
                     std::vector<int64_t>* out_off)
{
  const auto t_start = std::chrono::steady_clock::now();
  const int P = c.npr * c.PA;
  const size_t n = (size_t)c.n;
  int64_t *d_keys, *d_pay, *d_off, *d_ok, *d_op;
  uint32_t *d_counts, *d_totals;
  CHECK(hipMalloc(&d_keys, n * 8));
  CHECK(hipMalloc(&d_pay, n * 8));
  CHECK(hipMalloc(&d_counts, (size_t)g_sh.bucket_blocks * P * 4));
  CHECK(hipMalloc(&d_totals, (size_t)P * 4));
  CHECK(hipMalloc(&d_off, (size_t)(P + 1 + kGuardWords) * 8));
  CHECK(hipMalloc(&d_ok, (n + kGuardRows) * 8));
  CHECK(hipMalloc(&d_op, (n + kGuardRows) * 8));
  const size_t bytes = 2 * n * 8 + (size_t)(g_sh.bucket_blocks + 1) * P * 4 +
                       (size_t)(P + 1 + kGuardWords) * 8 + 2 * (n + kGuardRows) * 8;
  g_largest_bytes = std::max(g_largest_bytes, bytes);
  CHECK(hipMemcpy(d_keys, keys.data(), n * 8, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_pay, pay.data(), n * 8, hipMemcpyHostToDevice));
  CHECK(hipMemset(d_off, kPoison, (size_t)(P + 1 + kGuardWords) * 8));
  CHECK(hipMemset(d_ok, kPoison, (n + kGuardRows) * 8));
  CHECK(hipMemset(d_op, kPoison, (n + kGuardRows) * 8));

  dj::fused_partition(d_keys, c.null_pay ? nullptr : d_pay, c.n, c.npr, c.seed, c.PA, d_counts,
                      d_totals, d_off, d_ok, d_op, nullptr);
  CHECK(hipDeviceSynchronize());

  std::vector<int64_t> off((size_t)P + 1 + kGuardWords), ok(n + kGuardRows), op(n + kGuardRows);
  CHECK(hipMemcpy(off.data(), d_off, off.size() * 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(ok.data(), d_ok, ok.size() * 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(op.data(), d_op, op.size() * 8, hipMemcpyDeviceToHost));
  for (void* p : {(void*)d_keys, (void*)d_pay, (void*)d_counts, (void*)d_totals, (void*)d_off,
                  (void*)d_ok, (void*)d_op})
    CHECK(hipFree(p));

  Fails fail;
  if (!all_poison(off.data() + P + 1, kGuardWords * 8))
    fail("guard after offsets[P] written", 0, 0);
  if (!all_poison(ok.data() + n, kGuardRows * 8)) fail("guard after the key column written", 0, 0);
  if (!all_poison(op.data() + n, kGuardRows * 8))
    fail("guard after the payload column written", 0, 0);
  if (off[0] != 0) fail("offsets[0] != 0", off[0], 0);
  if (off[(size_t)P] != c.n) fail("offsets[P] != n", off[(size_t)P], c.n);
  bool monotone = off[0] == 0 && off[(size_t)P] == c.n;
  for (int s = 0; s < P; s++)
    if (off[(size_t)s + 1] < off[(size_t)s]) {
      fail("offsets decrease at slice", s, off[(size_t)s + 1]);
      monotone = false;
    }
  if (monotone) {
    std::vector<bool> seen(n, false);
    for (int s = 0; s < P; s++)
      for (int64_t i = off[(size_t)s]; i < off[(size_t)s + 1]; i++) {
        const int64_t k = ok[(size_t)i], v = op[(size_t)i];
        const int64_t idx = c.null_pay ? v : (v - 3) / 7 - pay_base;
        if (idx < 0 || idx >= c.n || pay[(size_t)idx] != v || keys[(size_t)idx] != k) {
          fail("stored row is no input row (slice, position)", s, i);
        } else if (seen[(size_t)idx]) {
          fail("input row stored twice (slice, input row)", s, idx);
        } else {
          seen[(size_t)idx] = true;
          if (slice_of_key(k, c.npr, c.seed, c.PA) != (uint32_t)s)
            fail("row in the wrong slice (slice, input row)", s, idx);
        }
      }
  }
  const double ms =
    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  g_slowest_ms = std::max(g_slowest_ms, ms);
  printf("fused nparts_rank=%d PA=%d n=%lld seed=%u%s%s, %.0f ms: %s\n", c.npr, c.PA,
         (long long)c.n, c.seed, c.null_pay ? " null-payload" : "",
         c.all_equal ? " all-keys-equal" : "", ms, fail.bad ? "FAILED" : "ok");
  if (out_keys) {
    ok.resize(n);
    op.resize(n);
    off.resize((size_t)P + 1);
    *out_keys = std::move(ok);
    *out_pay = std::move(op);
    *out_off = std::move(off);
  }
  return fail.bad;
}

/* ---------------- subpart_lists ---------------- */

/* a receive buffer with its segment lists, as build_segs lays them out */
struct Layout {
  std::string name;
  int G, PA, F;
  bool null_pay = false;
  int64_t pad = 0, total = 0;
  std::vector<int64_t> keys, pay; /* pad rows, then the G slices end to end */
  std::vector<int64_t> seg;       /* [G][PA+1] absolute offsets */
  std::vector<int64_t> gbase;     /* [PA+1] */
};

/* seg and gbase from per-peer slice starts and per-peer group counts, exactly
 * as build_segs computes them */
static void build_segs(Layout& L, const std::vector<int64_t>& roff,
                       const std::vector<std::vector<int64_t>>& sub)
{
  L.seg.assign((size_t)L.G * (L.PA + 1), 0);
  L.gbase.assign((size_t)L.PA + 1, 0);
  for (int r = 0; r < L.G; r++) {
    int64_t acc = roff[(size_t)r];
    for (int g = 0; g <= L.PA; g++) {
      L.seg[(size_t)r * (L.PA + 1) + g] = acc;
      if (g < L.PA) acc += sub[(size_t)r][(size_t)g];
    }
    for (int g = 0; g < L.PA; g++) L.gbase[(size_t)g + 1] += sub[(size_t)r][(size_t)g];
  }
  for (int g = 0; g < L.PA; g++) L.gbase[(size_t)g + 1] += L.gbase[(size_t)g];
  L.total = L.gbase[(size_t)L.PA];
}

/* distinct keys on demand per pass-A group */
struct KeySource {
  int PA;
  uint64_t stream, next = 0;
  std::vector<std::deque<int64_t>> q;
  KeySource(int pa, uint64_t s) : PA(pa), stream(s), q((size_t)pa) {}
  int64_t take(int g)
  {
    while (q[(size_t)g].empty()) {
      const int64_t k = hkey(stream, next++);
      q[group_of(k, PA)].push_back(k);
    }
    const int64_t k = q[(size_t)g].front();
    q[(size_t)g].pop_front();
    return k;
  }
};

static Layout hand_built(const std::string& name, int G, int PA, int F,
                         const std::vector<std::vector<int64_t>>& len, int64_t pad,
                         bool null_pay)
{
  Layout L;
  L.name = name;
  L.G = G;
  L.PA = PA;
  L.F = F;
  L.pad = pad;
  L.null_pay = null_pay;
  KeySource src(PA, 3);
  /* pad rows: keys of their own stream, so one that reaches the output shows */
  for (int64_t i = 0; i < pad; i++) L.keys.push_back(hkey(9, (uint64_t)i));
  std::vector<int64_t> roff((size_t)G);
  for (int r = 0; r < G; r++) {
    roff[(size_t)r] = (int64_t)L.keys.size();
    for (int g = 0; g < PA; g++)
      for (int64_t j = 0; j < len[(size_t)r][(size_t)g]; j++) L.keys.push_back(src.take(g));
  }
  build_segs(L, roff, len);
  L.pay.resize(L.keys.size());
  for (size_t i = 0; i < L.keys.size(); i++) L.pay[i] = null_pay ? (int64_t)i : 7 * (int64_t)i + 3;
  return L;
}

static std::vector<std::vector<int64_t>> some_lens(int G, int PA, int64_t modulus, uint64_t salt)
{
  std::vector<std::vector<int64_t>> len((size_t)G, std::vector<int64_t>((size_t)PA));
  for (int r = 0; r < G; r++)
    for (int g = 0; g < PA; g++)
      len[(size_t)r][(size_t)g] =
        (int64_t)(dj_mix64(salt * 1000003 + (uint64_t)r * 4099 + (uint64_t)g) % (uint64_t)modulus);
  return len;
}

static std::vector<Layout> hand_built_layouts()
{
  const int64_t ST = g_sh.scatter_tile;
  std::vector<Layout> v;
  v.push_back(hand_built("lists G=1 PA=4 F=64", 1, 4, 64, some_lens(1, 4, 3000, 1), 37, false));
  v.push_back(
    hand_built("lists G=2 PA=256 F=128", 2, 256, 128, some_lens(2, 256, 61, 2), 37, false));
  {
    /* group 1: every segment length around the staged tile in one run; peer 3,
     * in the middle, sends nothing at all (the last peer does, so a dropped
     * last segment shows); group 2 is empty in every peer */
    auto len = some_lens(8, 4, 700, 3);
    const int64_t edge[8] = {0, 1, ST - 1, 0, ST, ST + 1, 17, 2 * ST + 3};
    for (int r = 0; r < 8; r++) {
      len[(size_t)r][1] = edge[r];
      len[(size_t)r][2] = 0;
    }
    for (int g = 0; g < 4; g++) len[3][(size_t)g] = 0;
    v.push_back(hand_built("lists G=8 PA=4 F=256 tile-edge segments", 8, 4, 256, len, 37, false));
  }
  {
    /* the last group empty: the last block still closes bucket_offsets */
    auto len = some_lens(2, 256, 61, 4);
    len[0][255] = len[1][255] = 0;
    v.push_back(hand_built("lists G=2 PA=256 F=512 last group empty", 2, 256, 512, len, 5, false));
  }
  v.push_back(hand_built("lists G=8 PA=4 F=1024 null-payload", 8, 4, 1024,
                         some_lens(8, 4, 6000, 5), 37, true));
  return v;
}

static int run_lists(const Layout& L)
{
  const auto t_start = std::chrono::steady_clock::now();
  const size_t nin = std::max<size_t>(L.keys.size(), 1), total = (size_t)L.total;
  const int B = L.PA * L.F;
  int64_t *d_keys, *d_pay, *d_seg, *d_gb, *d_off;
  longlong2* d_out;
  CHECK(hipMalloc(&d_keys, nin * 8));
  CHECK(hipMalloc(&d_pay, nin * 8));
  CHECK(hipMalloc(&d_seg, L.seg.size() * 8));
  CHECK(hipMalloc(&d_gb, L.gbase.size() * 8));
  CHECK(hipMalloc(&d_out, (total + kGuardRows) * 16));
  CHECK(hipMalloc(&d_off, (size_t)(B + 1 + kGuardWords) * 8));
  const size_t bytes = 2 * nin * 8 + (L.seg.size() + L.gbase.size()) * 8 +
                       (total + kGuardRows) * 16 + (size_t)(B + 1 + kGuardWords) * 8;
  g_largest_bytes = std::max(g_largest_bytes, bytes);
  CHECK(hipMemcpy(d_keys, L.keys.data(), L.keys.size() * 8, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_pay, L.pay.data(), L.pay.size() * 8, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_seg, L.seg.data(), L.seg.size() * 8, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_gb, L.gbase.data(), L.gbase.size() * 8, hipMemcpyHostToDevice));
  CHECK(hipMemset(d_out, kPoison, (total + kGuardRows) * 16));
  CHECK(hipMemset(d_off, kPoison, (size_t)(B + 1 + kGuardWords) * 8));

  dj::subpart_lists(d_keys, L.null_pay ? nullptr : d_pay, d_seg, L.G, L.PA, L.F, d_gb, d_out,
                    d_off, nullptr);
  CHECK(hipDeviceSynchronize());

  std::vector<longlong2> out(total + kGuardRows);
  std::vector<int64_t> off((size_t)B + 1 + kGuardWords);
  CHECK(hipMemcpy(out.data(), d_out, out.size() * 16, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(off.data(), d_off, off.size() * 8, hipMemcpyDeviceToHost));
  for (void* p : {(void*)d_keys, (void*)d_pay, (void*)d_seg, (void*)d_gb, (void*)d_out,
                  (void*)d_off})
    CHECK(hipFree(p));

  /* payload -> row of the receive buffer */
  std::vector<std::pair<int64_t, int64_t>> by_pay;
  by_pay.reserve(total);
  for (int64_t i = L.pad; i < L.pad + L.total; i++) by_pay.push_back({L.pay[(size_t)i], i});
  std::sort(by_pay.begin(), by_pay.end());

  Fails fail;
  if (!all_poison(out.data() + total, kGuardRows * 16))
    fail("guard rows after out_pairs written", 0, 0);
  if (!all_poison(off.data() + B + 1, kGuardWords * 8))
    fail("guard after bucket_offsets[PA*F] written", 0, 0);
  if (off[0] != 0) fail("bucket_offsets[0] != 0", off[0], 0);
  if (off[(size_t)B] != L.total) fail("bucket_offsets[PA*F] != total", off[(size_t)B], L.total);
  bool monotone = off[0] == 0 && off[(size_t)B] == L.total;
  for (int b = 0; b < B; b++)
    if (off[(size_t)b + 1] < off[(size_t)b]) {
      fail("bucket_offsets decrease at bucket", b, off[(size_t)b + 1]);
      monotone = false;
    }
  if (monotone) {
    std::vector<bool> seen(L.keys.size(), false);
    for (int b = 0; b < B; b++)
      for (int64_t i = off[(size_t)b]; i < off[(size_t)b + 1]; i++) {
        const longlong2 row = out[(size_t)i];
        auto it = std::lower_bound(by_pay.begin(), by_pay.end(),
                                   std::make_pair((int64_t)row.y, (int64_t)INT64_MIN));
        if (it == by_pay.end() || it->first != row.y || L.keys[(size_t)it->second] != row.x) {
          fail("stored row is no laid-out row (bucket, position)", b, i);
        } else if (seen[(size_t)it->second]) {
          fail("laid-out row stored twice (bucket, row)", b, it->second);
        } else {
          seen[(size_t)it->second] = true;
          if (group_of(row.x, L.PA) != (uint32_t)(b / L.F) ||
              sub_of(row.x, L.F) != (uint32_t)(b % L.F))
            fail("row in the wrong bucket (bucket, row)", b, it->second);
        }
      }
  }
  const double ms =
    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  g_slowest_ms = std::max(g_slowest_ms, ms);
  printf("%s total=%lld, %.0f ms: %s\n", L.name.c_str(), (long long)L.total, ms,
         fail.bad ? "FAILED" : "ok");
  return fail.bad;
}

/* rank `rank`'s receive buffer of batch `batch` from the senders' partitioned
 * columns and offsets: sender s ships its slice p = batch * G + rank, rows
 * [pofs[p*PA], pofs[(p+1)*PA]) (slice_of), with group counts
 * pofs[p*PA+g+1] - pofs[p*PA+g] (subcounts_of) */
static Layout chained_layout(int G, int PA, int rank, int batch,
                             const std::vector<std::vector<int64_t>>& pkeys,
                             const std::vector<std::vector<int64_t>>& ppay,
                             const std::vector<std::vector<int64_t>>& pofs)
{
  Layout L;
  L.name = "chained fused_partition -> lists G=2 od=2 PA=256 F=64";
  L.G = G;
  L.PA = PA;
  L.F = 64;
  std::vector<int64_t> roff((size_t)G);
  std::vector<std::vector<int64_t>> sub((size_t)G, std::vector<int64_t>((size_t)PA));
  const size_t p = (size_t)(batch * G + rank);
  for (int s = 0; s < G; s++) {
    roff[(size_t)s] = (int64_t)L.keys.size();
    const auto& o = pofs[(size_t)s];
    for (int64_t i = o[p * PA]; i < o[(p + 1) * PA]; i++) {
      L.keys.push_back(pkeys[(size_t)s][(size_t)i]);
      L.pay.push_back(ppay[(size_t)s][(size_t)i]);
    }
    for (int g = 0; g < PA; g++) sub[(size_t)s][(size_t)g] = o[p * PA + g + 1] - o[p * PA + g];
  }
  build_segs(L, roff, sub);
  return L;
}

/* ---------------- inputs-only ---------------- */

static int check_inputs()
{
  const int64_t NB = g_sh.bucket_blocks, ST = g_sh.scatter_tile;
  bool chunk_lo = false, chunk_eq = false, chunk_hi = false, npow2 = false, one_row = false;
  for (const FusedCase& c : fused_cases()) {
    const int64_t chunk = (c.n + NB - 1) / NB;
    printf("inputs fused nparts_rank=%d PA=%d n=%lld: chunk %lld of tile %lld\n", c.npr, c.PA,
           (long long)c.n, (long long)chunk, (long long)ST);
    chunk_lo |= chunk == ST - 1;
    chunk_eq |= chunk == ST;
    chunk_hi |= chunk == ST + 1;
    const int P = c.npr * c.PA;
    npow2 |= (P & (P - 1)) != 0;
    one_row |= c.n == 1;
    if (P > 1024) {
      printf("BAD TEST INPUTS: nparts_rank * PA > 1024\n");
      return 2;
    }
  }
  bool seg[6] = {false, false, false, false, false, false}, empty_peer = false,
       empty_group = false, last_empty = false;
  for (const Layout& L : hand_built_layouts()) {
    printf("inputs %s: pad %lld total %lld\n", L.name.c_str(), (long long)L.pad,
           (long long)L.total);
    if (L.seg[0] == 0) {
      printf("BAD TEST INPUTS: the first slice starts at offset 0\n");
      return 2;
    }
    const int64_t want[6] = {0, 1, ST - 1, ST, ST + 1, 2 * ST + 3};
    for (int g = 0; g < L.PA; g++) {
      bool have[6] = {false, false, false, false, false, false};
      for (int r = 0; r < L.G; r++) {
        const int64_t* sb = &L.seg[(size_t)r * (L.PA + 1) + g];
        const int64_t len = sb[1] - sb[0];
        for (int k = 0; k < 6; k++) have[k] |= len == want[k];
      }
      if (have[0] && have[1] && have[2] && have[3] && have[4] && have[5])
        for (int k = 0; k < 6; k++) seg[k] = true;
      const int64_t gt = L.gbase[(size_t)g + 1] - L.gbase[(size_t)g];
      if (gt == 0 && g < L.PA - 1) empty_group = true;
      if (gt == 0 && g == L.PA - 1) last_empty = true;
    }
    for (int r = 0; r < L.G; r++)
      if (L.G > 1 && L.seg[(size_t)r * (L.PA + 1) + L.PA] == L.seg[(size_t)r * (L.PA + 1)])
        empty_peer = true;
    /* the rows of each run belong to its group */
    for (int r = 0; r < L.G; r++)
      for (int g = 0; g < L.PA; g++)
        for (int64_t i = L.seg[(size_t)r * (L.PA + 1) + g];
             i < L.seg[(size_t)r * (L.PA + 1) + g + 1]; i++)
          if (group_of(L.keys[(size_t)i], L.PA) != (uint32_t)g) {
            printf("BAD TEST INPUTS: row %lld is not of group %d\n", (long long)i, g);
            return 2;
          }
  }
  const struct {
    bool have;
    const char* what;
  } named[] = {
    {chunk_lo, "a fused chunk of SCATTER_TILE-1 rows"},
    {chunk_eq, "a fused chunk of SCATTER_TILE rows"},
    {chunk_hi, "a fused chunk of SCATTER_TILE+1 rows"},
    {npow2, "a slice count that is no power of two"},
    {one_row, "a one-row table"},
    {seg[0] && seg[5], "one group with segments of 0, 1, tile-1, tile, tile+1, 2*tile+3 rows"},
    {empty_peer, "a peer whose whole slice is empty"},
    {empty_group, "a group empty in every peer"},
    {last_empty, "an empty last group"},
  };
  for (const auto& s : named)
    if (!s.have) {
      printf("BAD TEST INPUTS: no case has %s\n", s.what);
      return 2;
    }
  printf("FUSED LISTS INPUTS OK\n");
  return 0;
}

int main(int argc, char** argv)
{
  if (argc == 3 && strcmp(argv[1], "--bad-f") == 0) {
    const int F = atoi(argv[2]);
    dj::subpart_lists(nullptr, nullptr, nullptr, 1, 4, F, nullptr, nullptr, nullptr, nullptr);
    printf("F = %d WAS NOT REJECTED\n", F);
    return 3;
  }
  const bool inputs_only = argc == 2 && strcmp(argv[1], "--inputs-only") == 0;
  if (argc > 1 && !inputs_only) {
    printf("usage: fused_lists_check [--inputs-only | --bad-f F]\n");
    return 2;
  }
  g_sh = dj::bucket_partition_shape();
  printf("shape: scatter_tile %d bucket_blocks %d\n", g_sh.scatter_tile, g_sh.bucket_blocks);
  if (const int rc = check_inputs()) return rc;
  if (inputs_only) return 0;

  int bad = 0;
  for (const FusedCase& c : fused_cases()) {
    std::vector<int64_t> keys, pay;
    fused_inputs(c, 1, keys, pay);
    bad += run_fused(c, keys, pay, 0, nullptr, nullptr, nullptr);
  }
  for (const Layout& L : hand_built_layouts()) bad += run_lists(L);
  {
    const int G = 2, od = 2, PA = 256;
    const FusedCase c = {G * od, PA, 200000, DJ_SEED_INTRA, false, false};
    std::vector<std::vector<int64_t>> pk((size_t)G), pp((size_t)G), po((size_t)G);
    for (int s = 0; s < G; s++) {
      std::vector<int64_t> keys, pay;
      fused_inputs(c, 5 + (uint64_t)s, keys, pay, (int64_t)s * c.n);
      bad += run_fused(c, keys, pay, (int64_t)s * c.n, &pk[(size_t)s], &pp[(size_t)s],
                       &po[(size_t)s]);
    }
    if (!bad) bad += run_lists(chained_layout(G, PA, 0, 1, pk, pp, po));
  }
  if (bad) {
    printf("FUSED LISTS FAILED: %d checks\n", bad);
    return 1;
  }
  printf("slowest run %.0f ms, largest device footprint %.1f MB\n", g_slowest_ms,
         (double)g_largest_bytes / 1e6);
  printf("FUSED LISTS OK\n");
  return 0;
}
