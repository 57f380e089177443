/*
 * slack_pair_check.cpp — dj::bucket_partition2_slack_pair (the partition of
 * every single-rank join: bucket_scatter_slack_pair_kernel, then
 * bucket_subpart_slack2_pair_kernel) called directly on two tables at once and
 * compared, exactly, with a host prediction.
 *
 * Host reference (bucket_model.hpp): bucket_of(key) = groupA * F + subF from
 * the dj_mix64 bit fields documented at groupA_of / subF_of in dj_kernels.hip
 * (group from >> 40, sub-bucket from >> 32, plus >> 50 when F > 256); per-group and
 * per-bucket counts follow from it. Payloads are 7*i+3 (or the row index i
 * when the payload pointer is null), so a stored row names the input row it
 * must be a copy of: "the multiset of stored rows equals the input's" is
 * checked as "every stored row equals its input row, no input row is stored
 * twice, and the lengths add up".
 *
 * Before each run out, tmp, lens, both cursor arrays and their guards (64
 * rows after tmp[PA*capA] and after out[B*capB], 16 words after lens[B] and
 * after cur[PA]) are filled with 0xEE. Per run and table:
 *   - the overflow word is exactly preset | 2 * (some group count exceeds
 *     slack_capA(n, PA) or some bucket count exceeds capB), over both tables;
 *   - cur[g] == min(count of group g, capA);
 *   - a bucket whose group and whose own count both fit holds lens[b] == its
 *     count (so every lens entry is overwritten, all-zero groups included); a
 *     bucket that alone overflowed holds exactly capB rows; a bucket of an
 *     overflowed group holds at most min(capB, count) rows;
 *   - every stored row belongs to bucket b and is an input row, stored once;
 *   - all guards are untouched.
 * A table without overflow of its own is therefore checked complete and exact
 * whatever the other table does.
 *
 * Every size derives from dj::bucket_partition_shape(); the grid split is the
 * launcher's formula, restated in split_of().
 *
 * usage: slack_pair_check [--inputs-only] [--set edges|tiles|fanout]
 *   --inputs-only: builds every case on the host, prints per case the block
 *   split, tiles per block, the fullest group against capA, the fullest bucket
 *   against capB and the predicted word, and fails if a case misses the word
 *   it was built for or a named situation is absent (needs no GPU).
 * Build/run: tests/test_gpu_slack_pair.py.
 */
#include "bucket_model.hpp"
#include "check.hpp"

#include "dj_kernels.hpp"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <string>
#include <vector>

static dj::BucketPartitionShape g_sh;

constexpr int64_t kCapSlack = 0;     /* capB = slack_capB(n, B), the product's */
constexpr int64_t kCapFullest = -1;  /* capB = host fullest bucket, rounded up to 8 */

struct Table {
  std::vector<int64_t> keys;
  bool null_pay = false;
  int64_t capB = kCapSlack;
};
struct Case {
  std::string name;
  int B = 512;
  Table t[2];
  int preset = 0;
  bool twice = false;
  int want_word = 0; /* the overflow word this case was built to produce */
};

/* ---------------- host reference ---------------- */

static int64_t pay_of(const Table& t, int64_t i) { return t.null_pay ? i : 7 * i + 3; }

struct Pred {
  int PA, F;
  int64_t n, capA, capB;
  std::vector<uint32_t> gcnt, bcnt;
  int64_t gmax, bmax;
  bool ovfA, ovfB;
};
static Pred predict(const Table& t, int B)
{
  Pred p;
  p.PA = dj::bucket_groups_for(B);
  p.F = B / p.PA;
  p.n = (int64_t)t.keys.size();
  p.capA = dj::slack_capA(p.n, p.PA);
  p.gcnt.assign((size_t)p.PA, 0);
  p.bcnt.assign((size_t)B, 0);
  for (int64_t k : t.keys) {
    const uint32_t b = bucket_of(k, p.PA, p.F);
    p.bcnt[b]++;
    p.gcnt[b / (uint32_t)p.F]++;
  }
  p.gmax = *std::max_element(p.gcnt.begin(), p.gcnt.end());
  p.bmax = *std::max_element(p.bcnt.begin(), p.bcnt.end());
  if (t.capB == kCapSlack)
    p.capB = dj::slack_capB(p.n, B);
  else if (t.capB == kCapFullest)
    p.capB = std::max<int64_t>(8, (p.bmax + 7) & ~(int64_t)7);
  else
    p.capB = t.capB;
  p.ovfA = p.gmax > p.capA;
  p.ovfB = p.bmax > p.capB;
  return p;
}

/* the launcher's pass-A grid split (bucket_partition2_slack_pair) */
struct Split {
  int blocks[2];
  int64_t chunk[2], last[2]; /* rows of a full block, rows of the last non-empty one */
  int tiles[2];
};
static Split split_of(int64_t n0, int64_t n1)
{
  Split s;
  const int total = 2 * g_sh.bucket_blocks;
  int b0 = (int)(2.0 * g_sh.bucket_blocks * (double)n0 / (double)(n0 + n1) + 0.5);
  if (b0 < 1) b0 = 1;
  if (b0 > total - 1) b0 = total - 1;
  s.blocks[0] = b0;
  s.blocks[1] = total - b0;
  const int64_t n[2] = {n0, n1};
  for (int t = 0; t < 2; t++) {
    s.chunk[t] = (n[t] + s.blocks[t] - 1) / s.blocks[t];
    s.last[t] = s.chunk[t] ? n[t] - (n[t] - 1) / s.chunk[t] * s.chunk[t] : 0;
    s.tiles[t] = (int)((std::min(s.chunk[t], n[t]) + g_sh.slack_tile - 1) / g_sh.slack_tile);
  }
  return s;
}

/* ---------------- inputs ---------------- */

/* distinct keys: hkey() of bucket_model.hpp */
static Table distinct(int64_t n, uint64_t stream, int64_t capB = kCapSlack)
{
  Table t;
  t.capB = capB;
  t.keys.resize((size_t)n);
  for (int64_t i = 0; i < n; i++) t.keys[(size_t)i] = hkey(stream, (uint64_t)i);
  return t;
}
/* distinct keys with exactly quota[g] rows in pass-A group g, in stream order */
static Table by_group(const std::vector<int64_t>& quota, uint64_t stream,
                      int64_t capB = kCapSlack)
{
  const int PA = (int)quota.size();
  std::vector<int64_t> left = quota;
  int64_t n = 0;
  for (int64_t q : quota) n += q;
  Table t;
  t.capB = capB;
  t.keys.reserve((size_t)n);
  for (uint64_t i = 0; (int64_t)t.keys.size() < n; i++) {
    const int64_t k = hkey(stream, i);
    const uint32_t g = group_of(k, PA);
    if (left[g] > 0) {
      left[g]--;
      t.keys.push_back(k);
    }
  }
  return t;
}
/* the smallest count of the other groups (PA == 2: of group `1 - g`) that
 * keeps a group of c0 rows inside slack_capA */
static int64_t other_group_rows(int64_t c0, int64_t at_least)
{
  int64_t g1 = at_least;
  while (dj::slack_capA(c0 + g1, 2) < c0) g1++;
  return g1;
}
/* base distinct keys plus `dups` more copies of base key 0, evenly spaced */
static Table with_dups(int64_t n_base, int64_t dups, uint64_t stream, int64_t capB)
{
  Table t;
  t.capB = capB;
  const int64_t n = n_base + dups;
  const int64_t stride = dups > 0 ? n / dups : n + 1;
  const int64_t dup_key = hkey(stream, 0);
  int64_t placed = 0, base = 0;
  t.keys.reserve((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    if (placed < dups && (i % stride == stride / 2 || base == n_base)) {
      t.keys.push_back(dup_key);
      placed++;
    } else {
      t.keys.push_back(hkey(stream, (uint64_t)base++));
    }
  }
  return t;
}
/* rows of base key 0's bucket among n_base distinct keys */
static int64_t base_bucket_rows(int64_t n_base, uint64_t stream, int B)
{
  const int PA = dj::bucket_groups_for(B), F = B / PA;
  const uint32_t b = bucket_of(hkey(stream, 0), PA, F);
  int64_t c = 0;
  for (int64_t i = 0; i < n_base; i++) c += bucket_of(hkey(stream, (uint64_t)i), PA, F) == b;
  return c;
}
static Table special_keys(uint64_t stream, int64_t capB)
{
  Table t = distinct(10000, stream, capB);
  t.keys[0] = -1;
  t.keys[1] = 0;
  t.keys[2] = INT64_MIN;
  t.keys[3] = INT64_MAX;
  for (int i = 1000; i < 1300; i++) t.keys[(size_t)i] = t.keys[1000];
  return t;
}

struct Entry {
  const char* set;
  std::function<Case()> make;
};

static Case mk(const std::string& name, int B, Table t0, Table t1, int want_word)
{
  Case c;
  c.name = name;
  c.B = B;
  c.t[0] = std::move(t0);
  c.t[1] = std::move(t1);
  c.want_word = want_word;
  return c;
}

static std::vector<Entry> entries()
{
  std::vector<Entry> e;
  const int64_t ST = g_sh.slack_tile, BT = g_sh.btile, NB = g_sh.bucket_blocks;

  /* 1. grid split */
  const int64_t splits[][2] = {{1, 1}, {1, 3000}, {5000, 1}, {0, 3000}, {300, 300}};
  for (auto& s : splits) {
    const int64_t n0 = s[0], n1 = s[1];
    e.push_back({"edges", [=] {
                   return mk("split n0=" + std::to_string(n0) + " n1=" + std::to_string(n1), 512,
                             distinct(n0, 1), distinct(n1, 2), 0);
                 }});
  }
  /* 2. pass-A tile edges, even split: ceil(n / blocks) = tile-1, tile, tile+1 */
  const int64_t even[] = {NB * (ST - 1) - 5, NB * ST, NB * ST + 1};
  for (int64_t n : even)
    e.push_back({"tiles", [=] {
                   return mk("passA even n=" + std::to_string(n), 512, distinct(n, 1),
                             distinct(n, 2), 0);
                 }});
  /* 3. table 0 in ONE block, three tiles deep; table 1's blocks two tiles */
  for (int nullp = 0; nullp < 2; nullp++)
    e.push_back({"tiles", [=] {
                   const int64_t n0 = 2 * ST + 1;
                   Case c = mk(std::string("passA one block 3 tiles") +
                                 (nullp ? " null-payload" : ""),
                               512, distinct(n0, 1), distinct(700 * n0, 2), 0);
                   c.t[0].null_pay = c.t[1].null_pay = nullp != 0;
                   return c;
                 }});
  /* 4. pass-B tile edges: group 0 of table 0 (group 1 of table 1) holds c0
   * rows; the other group is the smallest that keeps c0 within slack_capA */
  const int64_t bedge[] = {BT - 1, BT, BT + 1, 2 * BT + 1};
  for (int64_t c0 : bedge)
    e.push_back({"edges", [=] {
                   const int64_t g1 = other_group_rows(c0, 300);
                   Case c = mk("passB group rows " + std::to_string(c0), 512,
                               by_group({c0, g1}, 1), by_group({g1, c0}, 2), 0);
                   c.t[0].null_pay = c0 == BT + 1;
                   c.twice = c0 == BT + 1;
                   return c;
                 }});
  e.push_back({"edges", [=] {
                 return mk("passB group 0 empty", 512, by_group({0, 2000}, 1),
                           by_group({2000, 0}, 2), 0);
               }});
  /* 5a. fullest bucket at capB / one over, filled within one pass-B tile */
  for (int over = 0; over < 2; over++)
    for (int preset = 0; preset < 2; preset++)
      e.push_back({"edges", [=] {
                     const int64_t capB = 64, nb = 6000;
                     const int64_t dups = capB - base_bucket_rows(nb, 1, 512) + over;
                     Case c = mk(std::string("capB one tile ") + (over ? "one over" : "exact") +
                                   (preset ? " preset 1" : ""),
                                 512, with_dups(nb, dups, 1, capB), distinct(3000, 2),
                                 preset | (over ? 2 : 0));
                     c.preset = preset;
                     return c;
                   }});
  /* 5a. the same bucket filled across two pass-B tiles: table 1 is ten times
   * larger, so table 0 gets few pass-A blocks and every one of them holds a
   * row of the bucket (checked in spans_two_tiles) */
  for (int over = 0; over < 2; over++)
    e.push_back({"edges", [=] {
                   /* 200 copies over ~94 pass-A blocks, whatever the tile size */
                   const int64_t nb = 3 * BT, capB = base_bucket_rows(nb, 1, 512) + 200;
                   const int64_t dups = 200 + over;
                   return mk(std::string("capB two tiles ") + (over ? "one over" : "exact"), 512,
                             with_dups(nb, dups, 1, capB), distinct(10 * nb, 2), over ? 2 : 0);
                 }});
  /* 5b/5c. fullest pass-A group at slack_capA / one over, in either table */
  for (int over = 0; over < 2; over++)
    for (int tab = 0; tab < 2; tab++) {
      if (!over && tab) continue;
      e.push_back({"edges", [=] {
                     const int64_t n = 20000, capA = dj::slack_capA(n, 2);
                     Table big = by_group({capA + over, n - capA - over}, 1, kCapFullest);
                     Table small = distinct(3000, 2);
                     Case c = mk(std::string("capA ") + (over ? "one over" : "exact") +
                                   " in table " + std::to_string(tab),
                                 512, tab ? small : big, tab ? big : small, over ? 2 : 0);
                     return c;
                   }});
    }
  /* 5d. one key 50 000 times among 5 000 others: both passes overflow */
  e.push_back({"edges", [=] {
                 Table t = with_dups(5000, 50000, 1, kCapSlack);
                 return mk("one key 50000 times", 512, t, distinct(3000, 2), 2);
               }});
  /* 6. fan-out; the middle shape here, the full ones in their own set */
  e.push_back({"edges", [=] {
                 return mk("B=1024", 1024, distinct(50000, 1), distinct(20000, 2), 0);
               }});
  e.push_back({"fanout", [=] {
                 return mk("B=524288", 524288, distinct(2000000, 1, kCapFullest),
                           distinct(1000000, 2, kCapFullest), 0);
               }});
  e.push_back({"fanout", [=] {
                 return mk("B=1048576", 1048576, distinct(2000000, 1, kCapFullest),
                           distinct(1500000, 2, kCapFullest), 0);
               }});
  /* 7./8. -1, 0, the int64 extremes and a run of 300 equal keys; table 0 with
   * room for the run, table 1 at the product's capB, which the run overflows;
   * run twice on the same scratch */
  e.push_back({"edges", [=] {
                 Case c = mk("special keys", 512, special_keys(1, kCapFullest),
                             special_keys(2, kCapSlack), 2);
                 c.twice = true;
                 return c;
               }});
  return e;
}

/* ---------------- inputs-only report ---------------- */

struct Situations {
  bool three_tiles = false, tail_one = false, group_btile1 = false, capB_exact = false,
       capB_over = false, capA_exact = false, capA_over = false, empty_group = false,
       two_tile_bucket = false, table0_one_block = false, last_block_alone = false;
};

/* capB-edge tables: true if the fullest bucket's rows must reach two pass-B
 * tiles whatever order pass A's blocks claim their runs in — every pass-A
 * block of the table holds a row of that bucket, each block has one tile, and
 * both the first tile and the rest of the group's segment are at least two
 * chunks long, so each contains some block's whole run */
static bool spans_two_tiles(const Table& t, const Pred& p, int64_t chunk)
{
  const uint32_t b = (uint32_t)(std::max_element(p.bcnt.begin(), p.bcnt.end()) - p.bcnt.begin());
  const int64_t grows = p.gcnt[b / (uint32_t)p.F];
  if (chunk > g_sh.slack_tile || 2 * chunk > g_sh.btile || grows - g_sh.btile < 2 * chunk)
    return false;
  for (int64_t s = 0; s < p.n; s += chunk) {
    bool has = false;
    for (int64_t i = s; i < std::min(s + chunk, p.n) && !has; i++)
      has = bucket_of(t.keys[(size_t)i], p.PA, p.F) == b;
    if (!has) return false;
  }
  return true;
}

static bool report_inputs(const Case& c, const Pred p[2], Situations& sit)
{
  const Split s = split_of(p[0].n, p[1].n);
  const int word = c.preset | ((p[0].ovfA || p[0].ovfB || p[1].ovfA || p[1].ovfB) ? 2 : 0);
  printf("inputs %s: B=%d\n", c.name.c_str(), c.B);
  for (int t = 0; t < 2; t++) {
    printf("  table %d n=%lld blocks=%d chunk=%lld tiles/block=%d last block=%lld | fullest group "
           "%lld of capA %lld | fullest bucket %lld of capB %lld\n",
           t, (long long)p[t].n, s.blocks[t], (long long)s.chunk[t], s.tiles[t],
           (long long)s.last[t], (long long)p[t].gmax, (long long)p[t].capA,
           (long long)p[t].bmax, (long long)p[t].capB);
    if (s.tiles[t] >= 3) sit.three_tiles = true;
    for (int64_t rows : {s.chunk[t], s.last[t]})
      if (rows > g_sh.slack_tile && rows % g_sh.slack_tile == 1) sit.tail_one = true;
    for (uint32_t g : p[t].gcnt) {
      if (g == (uint32_t)g_sh.btile + 1) sit.group_btile1 = true;
      if (g == 0 && p[t].n > 0) sit.empty_group = true;
    }
    if (p[t].bmax == p[t].capB && !p[t].ovfA) sit.capB_exact = true;
    if (p[t].bmax == p[t].capB + 1 && !p[t].ovfA) sit.capB_over = true;
    if (p[t].gmax == p[t].capA) sit.capA_exact = true;
    if (p[t].gmax == p[t].capA + 1) sit.capA_over = true;
    if ((p[t].bmax == p[t].capB || p[t].bmax == p[t].capB + 1) &&
        spans_two_tiles(c.t[t], p[t], s.chunk[t]))
      sit.two_tile_bucket = true;
  }
  if (s.blocks[0] == 1 && s.tiles[0] >= 3 && s.tiles[1] == 2) sit.table0_one_block = true;
  if (s.blocks[1] == 1 && p[1].n > 0) sit.last_block_alone = true;
  printf("  predicted overflow word %d\n", word);
  if (word != c.want_word) {
    printf("BAD TEST INPUTS: %s was built for word %d\n", c.name.c_str(), c.want_word);
    return false;
  }
  return true;
}

/* ---------------- one run on the device ---------------- */

struct DevTable {
  int64_t *keys = nullptr, *pay = nullptr;
  longlong2 *tmp = nullptr, *out = nullptr;
  uint32_t *cur = nullptr, *lens = nullptr;
  size_t tmp_rows, out_rows;
};

static int run_case(const Case& c, const Pred p[2], double* slowest_ms, size_t* largest_bytes)
{
  const int B = c.B;
  DevTable d[2];
  int* d_ovf;
  size_t bytes = 4;
  for (int t = 0; t < 2; t++) {
    const size_t n = (size_t)p[t].n, n1 = std::max<size_t>(n, 1);
    d[t].tmp_rows = (size_t)p[t].PA * (size_t)p[t].capA;
    d[t].out_rows = (size_t)B * (size_t)p[t].capB;
    CHECK(hipMalloc(&d[t].keys, n1 * 8));
    CHECK(hipMalloc(&d[t].pay, n1 * 8));
    CHECK(hipMalloc(&d[t].tmp, (d[t].tmp_rows + kGuardRows) * 16));
    CHECK(hipMalloc(&d[t].out, (d[t].out_rows + kGuardRows) * 16));
    CHECK(hipMalloc(&d[t].cur, (size_t)(p[t].PA + kGuardWords) * 4));
    CHECK(hipMalloc(&d[t].lens, (size_t)(B + kGuardWords) * 4));
    bytes += 2 * n1 * 8 + (d[t].tmp_rows + d[t].out_rows + 2 * kGuardRows) * 16 +
             (size_t)(p[t].PA + B + 2 * kGuardWords) * 4;
    std::vector<int64_t> pay(n);
    for (size_t i = 0; i < n; i++) pay[i] = pay_of(c.t[t], (int64_t)i);
    CHECK(hipMemcpy(d[t].keys, c.t[t].keys.data(), n * 8, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d[t].pay, pay.data(), n * 8, hipMemcpyHostToDevice));
    CHECK(hipMemset(d[t].tmp, kPoison, (d[t].tmp_rows + kGuardRows) * 16));
    CHECK(hipMemset(d[t].out, kPoison, (d[t].out_rows + kGuardRows) * 16));
    CHECK(hipMemset(d[t].cur, kPoison, (size_t)(p[t].PA + kGuardWords) * 4));
    CHECK(hipMemset(d[t].lens, kPoison, (size_t)(B + kGuardWords) * 4));
  }
  CHECK(hipMalloc(&d_ovf, 4));
  CHECK(hipMemcpy(d_ovf, &c.preset, 4, hipMemcpyHostToDevice));
  *largest_bytes = std::max(*largest_bytes, bytes);
  const int want_word = c.preset | ((p[0].ovfA || p[0].ovfB || p[1].ovfA || p[1].ovfB) ? 2 : 0);

  int bad_total = 0;
  for (int run = 0; run < (c.twice ? 2 : 1); run++) {
    const auto t_start = std::chrono::steady_clock::now();
    /* no reset between the two runs of a `twice` case: the function zeroes
     * its own cursors, and the word only ever gains bits */
    dj::bucket_partition2_slack_pair(
      d[0].keys, c.t[0].null_pay ? nullptr : d[0].pay, p[0].n, d[0].tmp, d[0].cur, p[0].capB,
      d[0].out, d[0].lens, d[1].keys, c.t[1].null_pay ? nullptr : d[1].pay, p[1].n, d[1].tmp,
      d[1].cur, p[1].capB, d[1].out, d[1].lens, B, d_ovf, nullptr);
    CHECK(hipDeviceSynchronize());

    int bad = 0;
    auto fail = [&](const char* what, int t, long long a, long long b) {
      if (bad++ < 6) printf("  FAIL table %d: %s (%lld, %lld)\n", t, what, a, b);
    };
    int word = -1;
    CHECK(hipMemcpy(&word, d_ovf, 4, hipMemcpyDeviceToHost));
    if (word != want_word) fail("overflow word (got, predicted)", -1, word, want_word);

    for (int t = 0; t < 2; t++) {
      const Pred& q = p[t];
      const Table& tab = c.t[t];
      std::vector<longlong2> out(d[t].out_rows + kGuardRows);
      std::vector<longlong2> tmp_guard(kGuardRows);
      std::vector<uint32_t> lens((size_t)B + kGuardWords), cur((size_t)q.PA + kGuardWords);
      CHECK(hipMemcpy(out.data(), d[t].out, out.size() * 16, hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(tmp_guard.data(), d[t].tmp + d[t].tmp_rows, kGuardRows * 16,
                      hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(lens.data(), d[t].lens, lens.size() * 4, hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(cur.data(), d[t].cur, cur.size() * 4, hipMemcpyDeviceToHost));

      if (!all_poison(out.data() + d[t].out_rows, kGuardRows * 16))
        fail("guard rows after out[B*capB] written", t, 0, 0);
      if (!all_poison(tmp_guard.data(), kGuardRows * 16))
        fail("guard rows after tmp[PA*capA] written", t, 0, 0);
      if (!all_poison(lens.data() + B, kGuardWords * 4))
        fail("guard words after lens[B] written", t, 0, 0);
      if (!all_poison(cur.data() + q.PA, kGuardWords * 4))
        fail("guard words after cur[PA] written", t, 0, 0);

      for (int g = 0; g < q.PA; g++) {
        const int64_t want = std::min<int64_t>(q.gcnt[(size_t)g], q.capA);
        if ((int64_t)cur[(size_t)g] != want)
          fail("cursor != min(group count, capA) (group, got)", t, g, cur[(size_t)g]);
      }
      std::vector<bool> seen((size_t)q.n, false);
      int64_t stored = 0;
      for (int b = 0; b < B; b++) {
        const int64_t len = lens[(size_t)b], cnt = q.bcnt[(size_t)b];
        const bool group_fits = (int64_t)q.gcnt[(size_t)(b / q.F)] <= q.capA;
        if (len > q.capB) {
          fail("lens[b] > capB (bucket, len)", t, b, len);
          continue;
        }
        if (group_fits && cnt <= q.capB) {
          if (len != cnt) fail("lens[b] != host count (bucket, len)", t, b, len);
        } else if (group_fits) {
          if (len != q.capB) fail("overflowed bucket not filled to capB (bucket, len)", t, b, len);
        } else if (len > cnt) {
          fail("lens[b] > host count in an overflowed group (bucket, len)", t, b, len);
        }
        for (int64_t j = 0; j < len; j++) {
          const longlong2 row = out[(size_t)b * (size_t)q.capB + (size_t)j];
          const int64_t idx = tab.null_pay ? row.y : (row.y - 3) / 7;
          if (idx < 0 || idx >= q.n || pay_of(tab, idx) != row.y ||
              tab.keys[(size_t)idx] != row.x) {
            fail("stored row is no input row (bucket, slot)", t, b, j);
          } else if (seen[(size_t)idx]) {
            fail("input row stored twice (bucket, input row)", t, b, idx);
          } else {
            seen[(size_t)idx] = true;
            stored++;
            if (bucket_of(row.x, q.PA, q.F) != (uint32_t)b)
              fail("row in the wrong bucket (bucket, input row)", t, b, idx);
          }
        }
      }
      if (!q.ovfA && !q.ovfB && stored != q.n)
        fail("stored rows != input rows (stored, n)", t, stored, q.n);
    }
    const double ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start)
        .count();
    *slowest_ms = std::max(*slowest_ms, ms);
    printf("%s%s: word %d, %.1f MB on the device, %.0f ms: %s\n", c.name.c_str(),
           run ? " (again, same scratch)" : "", want_word, (double)bytes / 1e6, ms,
           bad ? "FAILED" : "ok");
    bad_total += bad;
  }
  for (int t = 0; t < 2; t++)
    for (void* q : {(void*)d[t].keys, (void*)d[t].pay, (void*)d[t].tmp, (void*)d[t].out,
                    (void*)d[t].cur, (void*)d[t].lens})
      CHECK(hipFree(q));
  CHECK(hipFree(d_ovf));
  return bad_total;
}

int main(int argc, char** argv)
{
  bool inputs_only = false;
  std::string set;
  for (int i = 1; i < argc; i++) {
    if (strcmp(argv[i], "--inputs-only") == 0) {
      inputs_only = true;
    } else if (strcmp(argv[i], "--set") == 0 && i + 1 < argc) {
      set = argv[++i];
    } else {
      printf("usage: slack_pair_check [--inputs-only] [--set edges|tiles|fanout]\n");
      return 2;
    }
  }
  g_sh = dj::bucket_partition_shape();
  printf("shape: scatter_tile %d slack_tile %d btile %d bucket_blocks %d bucket_threads %d\n",
         g_sh.scatter_tile, g_sh.slack_tile, g_sh.btile, g_sh.bucket_blocks,
         g_sh.bucket_threads);

  Situations sit;
  int bad = 0, ncases = 0;
  double slowest_ms = 0;
  size_t largest_bytes = 0;
  for (const Entry& e : entries()) {
    if (!set.empty() && set != e.set) continue;
    const Case c = e.make();
    const Pred p[2] = {predict(c.t[0], c.B), predict(c.t[1], c.B)};
    /* every input check comes before the case's launch */
    if (!report_inputs(c, p, sit)) return 2;
    ncases++;
    if (!inputs_only) bad += run_case(c, p, &slowest_ms, &largest_bytes);
  }
  if (ncases == 0) {
    printf("no such set: %s\n", set.c_str());
    return 2;
  }
  if (set.empty()) {
    const struct {
      bool have;
      const char* what;
    } named[] = {
      {sit.three_tiles, "a block with three or more pass-A tiles"},
      {sit.table0_one_block, "table 0 in one block of three tiles beside two-tile blocks"},
      {sit.last_block_alone, "the last block alone owning table 1"},
      {sit.tail_one, "a one-row tail tile in pass A"},
      {sit.group_btile1, "a pass-A group of exactly BTILE+1 rows"},
      {sit.capB_exact, "a fullest bucket of exactly capB rows"},
      {sit.capB_over, "a fullest bucket of capB+1 rows"},
      {sit.two_tile_bucket, "a capB-edge bucket filled across two pass-B tiles"},
      {sit.capA_exact, "a fullest group of exactly slack_capA rows"},
      {sit.capA_over, "a fullest group of slack_capA+1 rows"},
      {sit.empty_group, "an empty pass-A group"},
    };
    for (const auto& s : named)
      if (!s.have) {
        printf("BAD TEST INPUTS: no case has %s\n", s.what);
        return 2;
      }
  }
  if (bad) {
    printf("SLACK PAIR FAILED: %d checks\n", bad);
    return 1;
  }
  if (inputs_only) {
    printf("SLACK PAIR INPUTS OK (%d cases)\n", ncases);
  } else {
    printf("slowest run %.0f ms, largest device footprint %.1f MB\n", slowest_ms,
           (double)largest_bytes / 1e6);
    printf("SLACK PAIR OK (%d cases)\n", ncases);
  }
  return 0;
}
