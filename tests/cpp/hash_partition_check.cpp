/*
 * hash_partition_check.cpp — the stable rank-level partition (dj::hash_partition
 * and its sub-steps partition_count / partition_scan / partition_scatter:
 * part_count_kernel<NPL>, part_scan_kernel, part_offsets_kernel,
 * part_scatter_kernel<NPL>, NPL = 1, 2, 4, 8, 16) called directly and compared,
 * exactly, with a host prediction.
 *
 * Host reference: part(i) = hash(key_i) % nparts, the expected output is the
 * stable partition. For HASH_IDENTITY the hash is stated here, (uint32_t)key,
 * and every key is built to land in the partition its pattern names (checked
 * before the launch); for MurmurHash3 the host calls dj_murmur3_int64, which
 * tests/test_oracle.py pins to public vectors — the subject here is the
 * counting, the scan and the scatter. The payload is the row number, so
 * out_pay is the permutation itself.
 *
 * Checked after every run, exactly:
 *   - offsets[0..nparts] == exclusive scan of the host's partition counts;
 *   - out_keys[0..n) and out_pay[0..n) == the inputs in stable order (with a
 *     null input payload every written payload is 0; with a null output
 *     payload the payload buffer keeps its poison);
 *   - scratch: row w of the [nwaves][nparts] prefix table == the number of rows
 *     of each partition in the waves before w, and totals == the counts; at
 *     n == 0 scratch keeps its 0xFF fill;
 *   - kGuard poisoned elements before and after out_keys, out_pay, offsets and
 *     scratch are untouched.
 * Scratch is filled with 0xFF at the start of a set and before the cases that
 * say so, and otherwise reused as the case before (another nparts) left it.
 *
 * Every size derives from dj::hash_partition_shape(); geom() restates the
 * launcher's wave geometry from those constants.
 *
 * usage: hash_partition_check [--inputs-only] [--set sizes|nparts|patterns]
 *   --inputs-only: builds every case and its host reference, prints the
 *   geometry, and fails if a case misses the situation it is named for or a
 *   named situation is absent from the whole list (needs no GPU).
 * Build/run: tests/test_gpu_hash_partition.py.
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
#include <string>
#include <vector>

static dj::HashPartitionShape g_sh;
constexpr size_t kGuard = 128; /* poisoned elements on either side of a written buffer */
constexpr int kScratchFill = 0xFF;

enum Pattern { kRandom, kAll, kRound, kAlt, kRuns, kEven, kMurmur };

struct Case {
  std::string name;
  const char* set;
  int64_t n;
  int nparts;
  Pattern pat = kRandom;
  int q = 0, q2 = 0; /* kAll: q; kAlt: q and q2 */
  uint32_t seed = 0; /* kMurmur */
  bool substeps = false, null_pay = false, null_out = false, fresh_scratch = false;
  bool want_same_lane = false, want_gap = false;
};

/* ---------------- geometry and host reference ---------------- */

struct Geom {
  int64_t nwaves, rpw;
};
static Geom geom(int64_t n)
{
  const int64_t R = g_sh.target_rows_per_wave, W = g_sh.wave_cap, wpb = g_sh.waves_per_block;
  int64_t nw = std::min(std::max<int64_t>((n + R - 1) / R, 1), W);
  nw = (nw + wpb - 1) / wpb * wpb;
  return {nw, (n + nw - 1) / nw};
}
static int npl_of(int nparts)
{
  return nparts <= 64 ? 1 : nparts <= 128 ? 2 : nparts <= 256 ? 4 : nparts <= 512 ? 8 : 16;
}
static int tier_of(int nparts)
{
  int t = 0;
  for (int npl = npl_of(nparts); npl > 1; npl >>= 1) t++;
  return t;
}

static uint64_t rnd(uint64_t i)
{
  uint64_t r = (uint64_t)hkey(3, i);
  return r ^ (r >> 29);
}
/* a key whose identity hash lands in `part`: the low word is part plus a
 * multiple of nparts, the high word (sign bit included) is arbitrary */
static int64_t key_in(int part, int nparts, uint64_t i)
{
  const uint64_t r = rnd(i);
  const uint32_t low = (uint32_t)part + (uint32_t)nparts * (uint32_t)(r % 3);
  return (int64_t)((r & 0xFFFFFFFF00000000ULL) | low);
}
static int64_t murmur_key(uint64_t i)
{
  static const int64_t special[] = {-1,          0,  INT64_MIN, INT64_MAX, (int64_t)1 << 32,
                                    ((int64_t)1 << 32) + 1, -2, 4294967295LL};
  if (i < sizeof(special) / sizeof(special[0])) return special[i];
  return i % 3 == 0 ? (int64_t)i : hkey(5, i);
}
/* the partition the pattern wants row i in (kMurmur: no wish) */
static int wanted_part(const Case& c, int64_t i)
{
  const int np = c.nparts;
  switch (c.pat) {
    case kRandom: return (int)(rnd((uint64_t)i + 77) % (uint64_t)np);
    case kAll: return c.q;
    case kRound: return (int)(i % np);
    case kAlt: return (i & 1) ? c.q2 : c.q;
    case kRuns: return (int)(((i + 17) / 64) % np);
    case kEven: return 2 * (int)(rnd((uint64_t)i + 99) % (uint64_t)((np + 1) / 2));
    default: return -1;
  }
}

struct Host {
  std::vector<int64_t> keys;
  std::vector<int> part;
  std::vector<int64_t> cnt, off;
};
static bool build_host(const Case& c, Host& h)
{
  h.keys.resize((size_t)c.n);
  h.part.resize((size_t)c.n);
  h.cnt.assign((size_t)c.nparts, 0);
  for (int64_t i = 0; i < c.n; i++) {
    int p;
    if (c.pat == kMurmur) {
      h.keys[(size_t)i] = murmur_key((uint64_t)i);
      p = (int)(dj_murmur3_int64(h.keys[(size_t)i], c.seed) % (uint32_t)c.nparts);
    } else {
      const int want = wanted_part(c, i);
      h.keys[(size_t)i] = key_in(want, c.nparts, (uint64_t)i);
      /* the identity hash, stated here */
      p = (int)((uint32_t)h.keys[(size_t)i] % (uint32_t)c.nparts);
      if (p != want || want < 0 || want >= c.nparts) {
        printf("BAD TEST INPUTS: %s row %lld lands in %d, wanted %d\n", c.name.c_str(),
               (long long)i, p, want);
        return false;
      }
    }
    h.part[(size_t)i] = p;
    h.cnt[(size_t)p]++;
  }
  h.off.assign((size_t)c.nparts + 1, 0);
  for (int p = 0; p < c.nparts; p++) h.off[(size_t)p + 1] = h.off[(size_t)p] + h.cnt[(size_t)p];
  return true;
}

/* ---------------- cases ---------------- */

static std::string nm(const char* what, int64_t n, int nparts)
{
  return std::string(what) + " n=" + std::to_string(n) + " nparts=" + std::to_string(nparts);
}

static std::vector<Case> cases()
{
  std::vector<Case> v;
  const int64_t R = g_sh.target_rows_per_wave, W = g_sh.wave_cap, wpb = g_sh.waves_per_block;
  const int64_t central = R * W + 1, small = 4 * 65 + 3;
  const int all_nparts[] = {1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513,
                            1023, 1024};
  const int64_t all_n[] = {0, 1, 2, 63, 64, 65, 4 * 64 - 1, 4 * 64, 4 * 64 + 1, 4 * 65,
                           R * wpb - 1, R * wpb + 1, R * W - 1, R * W, R * W + 1,
                           R * W + 63 * W + 5, 3 * R * W + 12345};
  auto add = [&](Case c) { v.push_back(std::move(c)); };

  /* the full n list at four nparts */
  for (int np : {1, 64, 65, 1024})
    for (int64_t n : all_n) {
      Case c;
      c.set = "sizes";
      c.name = nm("sizes", n, np);
      c.n = n;
      c.nparts = np;
      c.fresh_scratch = n == 0;
      add(c);
    }
  /* the full nparts list at a small and at the central n, through
   * hash_partition and through the three sub-steps */
  for (int64_t n : {small, central})
    for (int np : all_nparts)
      for (int sub = 0; sub < 2; sub++) {
        if (sub && n == central && np != 64 && np != 129 && np != 257 && np != 513 && np != 1024)
          continue;
        Case c;
        c.set = "nparts";
        c.name = nm(sub ? "sub-steps" : "nparts", n, np);
        c.n = n;
        c.nparts = np;
        c.substeps = sub != 0;
        add(c);
      }
  /* key patterns */
  for (int np : {64, 128, 129, 256, 512, 1024})
    for (int64_t n : {small, central}) {
      const bool core = np == 64 || np == 129 || np == 1024;
      auto pat = [&](const char* what, Pattern p, int q = 0, int q2 = 0) {
        Case c;
        c.set = "patterns";
        c.name = nm(what, n, np);
        c.n = n;
        c.nparts = np;
        c.pat = p;
        c.q = q;
        c.q2 = q2;
        return c;
      };
      const int slots = (np + 63) / 64; /* populated cursor slots of a lane */
      if (slots > 1 && (core || n == small)) {
        /* two partitions of one lane: the next slot, and the last populated one */
        const int q = np == 129 ? 0 : 5;
        Case a = pat("alternate q, q+64", kAlt, q, q + 64);
        a.want_same_lane = true;
        add(a);
        if (slots > 2) {
          Case b = pat("alternate q, last slot", kAlt, q, q + 64 * (slots - 1));
          b.want_same_lane = true;
          add(b);
        }
      }
      if (!core) continue;
      add(pat("all in 0", kAll, 0));
      add(pat("all in last", kAll, np - 1));
      add(pat("all in 63", kAll, 63));
      if (np > 64) add(pat("all in 64", kAll, 64));
      add(pat("round robin", kRound));
      add(pat("runs of 64 shifted 17", kRuns));
      Case e = pat("even partitions only", kEven);
      e.want_gap = true;
      add(e);
      for (uint32_t seed : {0u, 12345678u, 87654321u}) {
        Case m = pat("murmur3", kMurmur);
        m.name += " seed=" + std::to_string(seed);
        m.seed = seed;
        add(m);
      }
      Case np0 = pat("null input payload", kRandom);
      np0.null_pay = true;
      np0.fresh_scratch = true;
      add(np0);
      Case no = pat("null output payload", kRandom);
      no.null_out = true;
      add(no);
    }
  return v;
}

/* ---------------- inputs-only report ---------------- */

struct Situations {
  bool partial_batch[5] = {false, false, false, false, false}; /* per NPL tier */
  bool odd_rpw_multi = false; /* rows_per_wave no multiple of 64, NPL > 1 */
  bool same_lane = false, gap = false, many_waves = false, empty_waves = false;
};

static bool report_inputs(const Case& c, const Host& h, Situations& sit)
{
  const Geom g = geom(c.n);
  const int64_t R = g_sh.target_rows_per_wave, W = g_sh.wave_cap;
  int64_t populated = 0, partial = 0;
  for (int64_t w = 0; w < g.nwaves; w++) {
    const int64_t s = w * g.rpw, e = std::min(s + g.rpw, c.n);
    if (e <= s) continue;
    populated++;
    if ((e - s) % 64) partial++;
  }
  bool same_lane = false;
  for (int64_t w = 0; w < g.nwaves && !same_lane; w++) {
    const int64_t s = w * g.rpw, e = std::min(s + g.rpw, c.n);
    for (int64_t b = s; b < e && !same_lane; b += 64) {
      int seen[64];
      for (int& x : seen) x = -1;
      for (int64_t i = b; i < std::min(b + 64, e); i++) {
        const int p = h.part[(size_t)i];
        if (seen[p & 63] >= 0 && seen[p & 63] != p) same_lane = true;
        seen[p & 63] = p;
      }
    }
  }
  bool gap = false;
  int state = 0; /* 0: nothing populated yet, 1: populated, 2: empty after populated */
  for (int p = 0; p < c.nparts; p++) {
    if (h.cnt[(size_t)p] > 0) {
      if (state == 2) gap = true;
      state = 1;
    } else if (state == 1) {
      state = 2;
    }
  }
  printf("inputs %s: NPL %d, %lld waves of %lld rows, %lld populated, %lld with a partial last "
         "batch%s%s\n",
         c.name.c_str(), npl_of(c.nparts), (long long)g.nwaves, (long long)g.rpw,
         (long long)populated, (long long)partial, same_lane ? ", two partitions on one lane" : "",
         gap ? ", an empty partition between populated ones" : "");
  if (dj::hash_partition_scratch_bytes(c.n, c.nparts) !=
      (size_t)(g.nwaves * c.nparts + c.nparts) * 8) {
    printf("BAD TEST INPUTS: %s: the host geometry disagrees with the scratch size\n",
           c.name.c_str());
    return false;
  }
  if (c.n == R * W + 1 && (partial != populated || populated == g.nwaves || g.rpw != R + 1)) {
    printf("BAD TEST INPUTS: %s: not every populated wave ends on a partial batch, or no wave "
           "is empty\n",
           c.name.c_str());
    return false;
  }
  if ((c.want_same_lane && !same_lane) || (c.want_gap && !gap)) {
    printf("BAD TEST INPUTS: %s misses the situation it is named for\n", c.name.c_str());
    return false;
  }
  if (partial) sit.partial_batch[tier_of(c.nparts)] = true;
  if (g.rpw > R && g.rpw % 64 && npl_of(c.nparts) > 1) sit.odd_rpw_multi = true;
  if (same_lane) sit.same_lane = true;
  if (gap) sit.gap = true;
  if (g.nwaves > g_sh.scan_block) sit.many_waves = true;
  if (populated < g.nwaves && c.n > 0) sit.empty_waves = true;
  return true;
}

/* ---------------- the device side ---------------- */

struct Dev {
  int64_t *keys = nullptr, *pay = nullptr, *okeys = nullptr, *opay = nullptr, *offs = nullptr;
  unsigned char* scratch = nullptr;
  size_t bytes = 0;
};

static Dev alloc_dev(int64_t max_n, size_t max_scratch)
{
  Dev d;
  const size_t n1 = (size_t)std::max<int64_t>(max_n, 1);
  CHECK(hipMalloc(&d.keys, n1 * 8));
  CHECK(hipMalloc(&d.pay, n1 * 8));
  CHECK(hipMalloc(&d.okeys, (n1 + 2 * kGuard) * 8));
  CHECK(hipMalloc(&d.opay, (n1 + 2 * kGuard) * 8));
  CHECK(hipMalloc(&d.offs, ((size_t)dj::kMaxPartitions + 1 + 2 * kGuard) * 8));
  CHECK(hipMalloc(&d.scratch, max_scratch + 2 * kGuard * 8));
  /* the guard before scratch is set once; the one behind it moves with the
   * case's scratch size */
  CHECK(hipMemset(d.scratch, kPoison, kGuard * 8));
  d.bytes = 2 * n1 * 8 + 2 * (n1 + 2 * kGuard) * 8 +
            ((size_t)dj::kMaxPartitions + 1 + 2 * kGuard) * 8 + max_scratch + 2 * kGuard * 8;
  return d;
}

static int run_case(const Case& c, const Host& h, Dev& d, bool fresh_scratch, double* ms_out)
{
  const size_t n = (size_t)c.n, np = (size_t)c.nparts;
  const Geom g = geom(c.n);
  const size_t sbytes = dj::hash_partition_scratch_bytes(c.n, c.nparts);
  int64_t* okeys = d.okeys + kGuard;
  int64_t* opay = d.opay + kGuard;
  int64_t* offs = d.offs + kGuard;
  unsigned char* scratch = d.scratch + kGuard * 8;

  std::vector<int64_t> pay(n);
  for (size_t i = 0; i < n; i++) pay[i] = (int64_t)i;
  CHECK(hipMemcpy(d.keys, h.keys.data(), n * 8, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d.pay, pay.data(), n * 8, hipMemcpyHostToDevice));
  CHECK(hipMemset(d.okeys, kPoison, (n + 2 * kGuard) * 8));
  CHECK(hipMemset(d.opay, kPoison, (n + 2 * kGuard) * 8));
  CHECK(hipMemset(d.offs, kPoison, (np + 1 + 2 * kGuard) * 8));
  if (fresh_scratch) CHECK(hipMemset(scratch, kScratchFill, sbytes));
  CHECK(hipMemset(scratch + sbytes, kPoison, kGuard * 8));
  CHECK(hipDeviceSynchronize());

  const int hash_fn = c.pat == kMurmur ? DJ_HASH_MURMUR3 : DJ_HASH_IDENTITY;
  const int64_t* in_pay = c.null_pay ? nullptr : d.pay;
  int64_t* out_pay = c.null_out ? nullptr : opay;
  const auto t0 = std::chrono::steady_clock::now();
  if (c.substeps) {
    dj::partition_count(d.keys, c.n, c.nparts, hash_fn, c.seed, scratch, nullptr);
    dj::partition_scan(c.n, c.nparts, scratch, offs, nullptr);
    dj::partition_scatter(d.keys, in_pay, c.n, c.nparts, hash_fn, c.seed, offs, scratch, okeys,
                          out_pay, nullptr);
  } else {
    dj::hash_partition(d.keys, in_pay, c.n, c.nparts, hash_fn, c.seed, okeys, out_pay, offs,
                       scratch, nullptr);
  }
  CHECK(hipDeviceSynchronize());
  *ms_out =
    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

  int bad = 0;
  auto fail = [&](const char* what, long long a, long long b, long long e) {
    if (bad++ < 6) printf("  FAIL %s (at %lld: got %lld, expected %lld)\n", what, a, b, e);
  };
  std::vector<int64_t> gk(n + 2 * kGuard), gp(n + 2 * kGuard), go(np + 1 + 2 * kGuard);
  std::vector<unsigned char> gs(sbytes + 2 * kGuard * 8);
  CHECK(hipMemcpy(gk.data(), d.okeys, gk.size() * 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(gp.data(), d.opay, gp.size() * 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(go.data(), d.offs, go.size() * 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(gs.data(), d.scratch, gs.size(), hipMemcpyDeviceToHost));

  if (!all_poison(gk.data(), kGuard * 8)) fail("guard before out_keys written", 0, 0, 0);
  if (!all_poison(gk.data() + kGuard + n, kGuard * 8)) fail("guard after out_keys written", 0, 0, 0);
  if (!all_poison(gp.data(), kGuard * 8)) fail("guard before out_pay written", 0, 0, 0);
  if (!all_poison(gp.data() + kGuard + n, kGuard * 8)) fail("guard after out_pay written", 0, 0, 0);
  if (!all_poison(go.data(), kGuard * 8)) fail("guard before offsets written", 0, 0, 0);
  if (!all_poison(go.data() + kGuard + np + 1, kGuard * 8))
    fail("guard after offsets written", 0, 0, 0);
  if (!all_poison(gs.data(), kGuard * 8)) fail("guard before scratch written", 0, 0, 0);
  if (!all_poison(gs.data() + kGuard * 8 + sbytes, kGuard * 8))
    fail("guard after scratch written", 0, 0, 0);

  for (size_t p = 0; p <= np; p++)
    if (go[kGuard + p] != h.off[p]) fail("offsets", (long long)p, go[kGuard + p], h.off[p]);

  /* the stable partition: row i goes to the next free place of its partition */
  std::vector<int64_t> cur(h.off.begin(), h.off.end() - 1), ek(n), ep(n);
  for (size_t i = 0; i < n; i++) {
    const int64_t dst = cur[(size_t)h.part[i]]++;
    ek[(size_t)dst] = h.keys[i];
    ep[(size_t)dst] = (int64_t)i;
  }
  for (size_t i = 0; i < n; i++)
    if (gk[kGuard + i] != ek[i]) fail("out_keys", (long long)i, gk[kGuard + i], ek[i]);
  if (c.null_out) {
    if (!all_poison(gp.data() + kGuard, n * 8))
      fail("payload buffer written though d_out_pay was null", 0, 0, 0);
  } else {
    for (size_t i = 0; i < n; i++) {
      const int64_t want = c.null_pay ? 0 : ep[i];
      if (gp[kGuard + i] != want) fail("out_pay", (long long)i, gp[kGuard + i], want);
    }
  }

  /* scratch: [nwaves][nparts] exclusive per-partition prefix over the waves,
   * then the totals */
  const int64_t* sc = (const int64_t*)(gs.data() + kGuard * 8);
  if (c.n == 0) {
    for (size_t i = 0; i < sbytes; i++)
      if (gs[kGuard * 8 + i] != kScratchFill) {
        fail("scratch written at n == 0", (long long)i, gs[kGuard * 8 + i], kScratchFill);
        break;
      }
  } else {
    std::vector<int64_t> running(np, 0);
    for (int64_t w = 0; w < g.nwaves; w++) {
      const int64_t* row = sc + (size_t)w * np;
      for (size_t p = 0; p < np; p++)
        if (row[p] != running[p])
          fail("scratch wave prefix (at wave * nparts + partition)", (long long)(w * (int64_t)np + (int64_t)p),
               row[p], running[p]);
      const int64_t s = w * g.rpw, e = std::min(s + g.rpw, c.n);
      for (int64_t i = s; i < e; i++) running[(size_t)h.part[(size_t)i]]++;
    }
    const int64_t* totals = sc + (size_t)g.nwaves * np;
    for (size_t p = 0; p < np; p++)
      if (totals[p] != h.cnt[p]) fail("scratch totals", (long long)p, totals[p], h.cnt[p]);
  }
  return bad;
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
      printf("usage: hash_partition_check [--inputs-only] [--set sizes|nparts|patterns]\n");
      return 2;
    }
  }
  g_sh = dj::hash_partition_shape();
  printf("shape: target rows per wave %d, wave cap %d, waves per block %d, scan block %d\n",
         g_sh.target_rows_per_wave, g_sh.wave_cap, g_sh.waves_per_block, g_sh.scan_block);

  std::vector<Case> all;
  int64_t max_n = 0;
  size_t max_scratch = 0;
  for (Case& c : cases()) {
    if (!set.empty() && set != c.set) continue;
    max_n = std::max(max_n, c.n);
    max_scratch = std::max(max_scratch, dj::hash_partition_scratch_bytes(c.n, c.nparts));
    all.push_back(c);
  }
  if (all.empty()) {
    printf("no such set: %s\n", set.c_str());
    return 2;
  }
  Dev d;
  if (!inputs_only) d = alloc_dev(max_n, max_scratch);

  Situations sit;
  int bad = 0, ncases = 0;
  double slowest_ms = 0;
  std::string slowest;
  Host h;
  for (const Case& c : all) {
    if (!build_host(c, h)) return 2;
    /* every input check comes before the case's launch */
    if (!report_inputs(c, h, sit)) return 2;
    if (!inputs_only) {
      double ms = 0;
      const int b = run_case(c, h, d, c.fresh_scratch || ncases == 0, &ms);
      if (ms > slowest_ms) {
        slowest_ms = ms;
        slowest = c.name;
      }
      printf("%s: %.2f ms: %s\n", c.name.c_str(), ms, b ? "FAILED" : "ok");
      bad += b;
    }
    ncases++;
  }
  if (set.empty()) {
    const struct {
      bool have;
      const char* what;
    } named[] = {
      {sit.partial_batch[0], "a partial last batch at NPL 1"},
      {sit.partial_batch[1], "a partial last batch at NPL 2"},
      {sit.partial_batch[2], "a partial last batch at NPL 4"},
      {sit.partial_batch[3], "a partial last batch at NPL 8"},
      {sit.partial_batch[4], "a partial last batch at NPL 16"},
      {sit.odd_rpw_multi, "rows per wave above the target and no multiple of 64 at NPL > 1"},
      {sit.same_lane, "two populated partitions on one lane within one batch"},
      {sit.gap, "an empty partition between two populated ones"},
      {sit.many_waves, "more waves than the scan block is wide"},
      {sit.empty_waves, "empty trailing waves"},
    };
    for (const auto& s : named)
      if (!s.have) {
        printf("BAD TEST INPUTS: no case has %s\n", s.what);
        return 2;
      }
  }
  if (bad) {
    printf("HASH PARTITION FAILED: %d checks\n", bad);
    return 1;
  }
  if (inputs_only) {
    printf("HASH PARTITION INPUTS OK (%d cases)\n", ncases);
  } else {
    printf("slowest call %.2f ms (%s), device footprint %.1f MB\n", slowest_ms, slowest.c_str(),
           (double)d.bytes / 1e6);
    printf("HASH PARTITION OK (%d cases)\n", ncases);
  }
  return 0;
}
