/*
 * bucket_partition_check.cpp — dj::bucket_partition2 (the two-level bucket
 * partition of the local join) called directly, on both of its pass-A forms:
 * the exact counted one (d_any_overflow == nullptr: count + scan + staged
 * scatter, then pass B over exact segments) and the slack one (non-null:
 * atomic-cursor pass A, then pass B over slack segments; the overflow word
 * must read back 0). B == 256 has a single pass-A group and takes the
 * single-level form either way.
 *
 * Per run: offsets[0] == 0, offsets[B] == n, offsets non-decreasing; every row
 * of bucket b has the host-computed id groupA * F + subF == b (bit fields of
 * dj_mix64 as documented at groupA_of / subF_of in dj_kernels.hip and restated
 * in bucket_model.hpp); the sorted
 * (key, payload) multiset equals the input's.
 *
 * Keys are distinct multiplicative-hash values with one run of 300 equal
 * keys; one case passes d_pay == nullptr (payload = row index). Before any
 * launch the program checks that no pass-A group exceeds slack_capA — a
 * failure there is a fault of these inputs, not of the kernels.
 *
 * usage: bucket_partition_check [--inputs-only]
 *   --inputs-only: host-side input checks alone (needs no GPU); prints the
 *   fullest pass-A group against its capacity for every case.
 * Build/run: tests/test_gpu_bucket_partition.py.
 */
#include "bucket_model.hpp"
#include "check.hpp"

#include "dj_kernels.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

struct Case {
  int B;
  int64_t n;
  bool null_pay;
};

/* B = PA x F: 256 = 1 x 256 around the 4096-row staging tile; 512 = 2 x 256
 * where one pass-A block's chunk (n / 512 blocks) crosses a tile; 524288 =
 * 1024 x 512 for the F > 256 bit field */
static const Case kCases[] = {
  {256, 1, false},      {256, 4095, false},
  {256, 4097, false},   {256, 10000, false},
  {512, 10000, true},   {512, 512 * 4097 + 3, false},
  {524288, 2000000, false},
};

constexpr int64_t kRunStart = 1000, kRunLen = 300;

static void make_inputs(const Case& c, std::vector<int64_t>& keys, std::vector<int64_t>& pay)
{
  keys.resize((size_t)c.n);
  pay.resize((size_t)c.n);
  for (int64_t i = 0; i < c.n; i++) {
    /* odd multiplier: a bijection of the row index, so keys are distinct */
    const int64_t src = (i >= kRunStart && i < kRunStart + kRunLen) ? kRunStart : i;
    keys[(size_t)i] = (int64_t)((uint64_t)(src + 1) * 0x9E3779B97F4A7C15ULL);
    pay[(size_t)i] = c.null_pay ? i : 7 * i + 3;
  }
}

/* fullest pass-A group against slack_capA; false = these inputs are unusable */
static bool check_inputs(const Case& c, const std::vector<int64_t>& keys)
{
  const int PA = dj::bucket_groups_for(c.B);
  std::vector<int64_t> cnt((size_t)PA, 0);
  for (int64_t k : keys) cnt[group_of(k, PA)]++;
  const int64_t fullest = *std::max_element(cnt.begin(), cnt.end());
  const int64_t capA = dj::slack_capA(c.n, PA);
  printf("inputs B=%d n=%lld PA=%d: fullest group %lld of slack_capA %lld\n", c.B,
         (long long)c.n, PA, (long long)fullest, (long long)capA);
  return fullest <= capA;
}

static int run_case(const Case& c, bool slack, const std::vector<int64_t>& keys,
                    const std::vector<int64_t>& pay)
{
  const int B = c.B;
  const int64_t n = c.n;
  const int PA = dj::bucket_groups_for(B);
  const int F = B / PA;
  const size_t tmp_rows =
    std::max<size_t>((size_t)n, (size_t)PA * (size_t)dj::slack_capA(n, PA));

  int64_t *d_keys, *d_pay, *d_segoff, *d_offsets;
  longlong2 *d_tmp, *d_out;
  uint32_t *d_counts, *d_totals;
  int* d_ovf;
  CHECK(hipMalloc(&d_keys, (size_t)n * 8));
  CHECK(hipMalloc(&d_pay, (size_t)n * 8));
  CHECK(hipMalloc(&d_tmp, tmp_rows * 16));
  CHECK(hipMalloc(&d_out, (size_t)n * 16));
  CHECK(hipMalloc(&d_counts, (size_t)dj::kBucketBlocks * PA * 4));
  CHECK(hipMalloc(&d_totals, (size_t)PA * 4));
  CHECK(hipMalloc(&d_segoff, (size_t)(PA + 1) * 8));
  CHECK(hipMalloc(&d_offsets, (size_t)(B + 1) * 8));
  CHECK(hipMalloc(&d_ovf, 4));
  CHECK(hipMemcpy(d_keys, keys.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_pay, pay.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  CHECK(hipMemset(d_out, kPoison, (size_t)n * 16));
  CHECK(hipMemset(d_offsets, kPoison, (size_t)(B + 1) * 8));
  CHECK(hipMemset(d_ovf, 0, 4));

  dj::bucket_partition2(d_keys, c.null_pay ? nullptr : d_pay, n, B, d_tmp, d_counts, d_totals,
                        d_segoff, d_offsets, d_out, slack ? d_ovf : nullptr, nullptr);
  CHECK(hipDeviceSynchronize());

  std::vector<int64_t> off((size_t)B + 1);
  std::vector<longlong2> out((size_t)n);
  int ovf = -1;
  CHECK(hipMemcpy(off.data(), d_offsets, (size_t)(B + 1) * 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(out.data(), d_out, (size_t)n * 16, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(&ovf, d_ovf, 4, hipMemcpyDeviceToHost));
  for (void* p : {(void*)d_keys, (void*)d_pay, (void*)d_tmp, (void*)d_out, (void*)d_counts,
                  (void*)d_totals, (void*)d_segoff, (void*)d_offsets, (void*)d_ovf})
    CHECK(hipFree(p));

  int bad = 0;
  auto fail = [&](const char* what, long long a, long long b) {
    if (bad++ < 5) printf("  FAIL %s (%lld, %lld)\n", what, a, b);
  };
  if (ovf != 0) fail("overflow word not 0", ovf, 0);
  if (off[0] != 0) fail("offsets[0] != 0", off[0], 0);
  if (off[(size_t)B] != n) fail("offsets[B] != n", off[(size_t)B], n);
  bool monotone = off[0] >= 0;
  for (int b = 0; b < B; b++)
    if (off[(size_t)b + 1] < off[(size_t)b]) {
      fail("offsets decrease at bucket", b, off[(size_t)b + 1]);
      monotone = false;
    }
  if (monotone && off[0] == 0 && off[(size_t)B] == n) {
    for (int b = 0; b < B; b++)
      for (int64_t i = off[(size_t)b]; i < off[(size_t)b + 1]; i++)
        if (bucket_of(out[(size_t)i].x, PA, F) != (uint32_t)b)
          fail("row in the wrong bucket (bucket, row)", b, i);
  }
  std::vector<std::pair<int64_t, int64_t>> want((size_t)n), got((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    want[(size_t)i] = {keys[(size_t)i], pay[(size_t)i]};
    got[(size_t)i] = {out[(size_t)i].x, out[(size_t)i].y};
  }
  std::sort(want.begin(), want.end());
  std::sort(got.begin(), got.end());
  if (want != got) fail("row multiset differs from the input's", n, 0);

  printf("B=%d (PA=%d x F=%d) n=%lld %s%s: %s\n", B, PA, F, (long long)n,
         slack ? "slack" : "exact", c.null_pay ? " null-payload" : "", bad ? "FAILED" : "ok");
  return bad;
}

int main(int argc, char** argv)
{
  const bool inputs_only = argc > 1 && strcmp(argv[1], "--inputs-only") == 0;
  int bad = 0;
  for (const Case& c : kCases) {
    std::vector<int64_t> keys, pay;
    make_inputs(c, keys, pay);
    if (!check_inputs(c, keys)) {
      printf("BAD TEST INPUTS: a pass-A group exceeds slack_capA\n");
      return 2;
    }
    if (inputs_only) continue;
    bad += run_case(c, false, keys, pay);
    bad += run_case(c, true, keys, pay);
  }
  if (bad) {
    printf("BUCKET PARTITION FAILED: %d checks\n", bad);
    return 1;
  }
  printf(inputs_only ? "BUCKET PARTITION INPUTS OK\n" : "BUCKET PARTITION OK\n");
  return 0;
}
