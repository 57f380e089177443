/*
 * dtype_loopback.cpp — narrow keys and 1-/2-/4-/8-byte payload columns
 * across G ranks on ONE GPU. Ranks run as host threads, each with the
 * loopback implementation of the public Communicator interface
 * (loopback.hpp) that hands device buffers over through an in-process
 * mailbox; upload and read-back are those of host_table.hpp.
 *
 * Global tables, 40 000 x 40 000 rows:
 *   left  = (key INT16, UINT8, FLOAT64, rowid INT64)
 *   right = (key INT16, FLOAT32, rowid INT64)
 * Keys are a formula of the row in [-10000, 10000] (duplicates on both sides,
 * -1 — the engine's sentinel — included); payloads are bit patterns derived
 * from the rowid (NaN payloads and denormals occur), so every output row can
 * be checked against its rowids.
 *
 * Checks: every output row has equal keys and carries the payloads of its
 * two rowids bit for bit; the concatenated G-rank distributed_inner_join has
 * the row count and the order-insensitive checksum of the 1-rank join of the
 * same global tables, computed in this program. Rank slices are uneven when
 * G does not divide the row count (G = 3: odd boundaries for the 1-byte
 * column).
 *
 * usage: dtype_loopback G nvlink_domain_size compression
 * Build/run: tests/test_gpu_dtypes.py::test_dtype_loopback.
 */
#include "host_table.hpp"
#include "loopback.hpp"

#include "compression.hpp"
#include "distributed_join.hpp"
#include "shuffle_on.hpp"

#include <vector>

/* ---------------- tables ---------------- */

constexpr int64_t kRows = 40000;

static int16_t key_of(int64_t global_row, bool left)
{
  return (int16_t)((int64_t)(dj_mix64((uint64_t)global_row + (left ? 0ull : 7777777ull)) % 20001) -
                   10000);
}
static uint8_t u8_of(int64_t rowid) { return (uint8_t)(dj_mix64((uint64_t)rowid * 3 + 1) & 0xFF); }
static uint64_t f64_bits_of(int64_t rowid) { return dj_mix64((uint64_t)rowid * 5 + 2); }
static uint32_t f32_bits_of(int64_t rowid) { return (uint32_t)dj_mix64((uint64_t)rowid * 7 + 3); }

template <typename T>
static std::unique_ptr<cudf::column> upload(cudf::type_id id, const std::vector<T>& v)
{
  if (width_of(id) != (int)sizeof(T)) FAIL("size_of mismatch for type %d", (int)id);
  return device_fixed(id, v.data(), (int64_t)v.size(), (int)sizeof(T));
}

/* rows [row0, row0 + rows) of a global table */
static std::unique_ptr<cudf::table> make_table(int64_t row0, int64_t rows, bool left)
{
  std::vector<int16_t> key((size_t)rows);
  std::vector<int64_t> rowid((size_t)rows);
  std::vector<uint8_t> u8((size_t)rows);
  std::vector<uint64_t> f64((size_t)rows);
  std::vector<uint32_t> f32((size_t)rows);
  for (int64_t t = 0; t < rows; t++) {
    const int64_t id = row0 + t;
    key[(size_t)t] = key_of(id, left);
    rowid[(size_t)t] = id;
    u8[(size_t)t] = u8_of(id);
    f64[(size_t)t] = f64_bits_of(id);
    f32[(size_t)t] = f32_bits_of(id);
  }
  std::vector<std::unique_ptr<cudf::column>> cols;
  cols.push_back(upload(cudf::type_id::INT16, key));
  if (left) {
    cols.push_back(upload(cudf::type_id::UINT8, u8));
    cols.push_back(upload(cudf::type_id::FLOAT64, f64));
  } else {
    cols.push_back(upload(cudf::type_id::FLOAT32, f32));
  }
  cols.push_back(upload(cudf::type_id::INT64, rowid));
  return std::make_unique<cudf::table>(std::move(cols));
}

template <typename T>
static std::vector<T> host_of(const cudf::column& col, cudf::type_id want)
{
  if (col.type().id() != want)
    FAIL("JOIN OUTPUT SCHEMA WRONG (type %d, want %d)", (int)col.type().id(), (int)want);
  /* from_device sign-extends to 64 bits; narrowing to T gives the bits back */
  const HCol c = from_device(col);
  return std::vector<T>(c.v.begin(), c.v.end());
}

/* verifies every row, then folds (key, lrowid, rrowid) into an
 * order-insensitive checksum */
static void checksum(const cudf::table& t, uint64_t* sum, int64_t* rows)
{
  if (t.num_columns() != 7) {
    printf("JOIN OUTPUT SCHEMA WRONG (%d columns)\n", (int)t.num_columns());
    exit(1);
  }
  auto lk = host_of<int16_t>(t.get_column(0), cudf::type_id::INT16);
  auto lu8 = host_of<uint8_t>(t.get_column(1), cudf::type_id::UINT8);
  auto lf64 = host_of<uint64_t>(t.get_column(2), cudf::type_id::FLOAT64);
  auto lid = host_of<int64_t>(t.get_column(3), cudf::type_id::INT64);
  auto rk = host_of<int16_t>(t.get_column(4), cudf::type_id::INT16);
  auto rf32 = host_of<uint32_t>(t.get_column(5), cudf::type_id::FLOAT32);
  auto rid = host_of<int64_t>(t.get_column(6), cudf::type_id::INT64);
  uint64_t s = 0;
  for (size_t i = 0; i < lk.size(); i++) {
    if (lid[i] < 0 || lid[i] >= kRows || rid[i] < 0 || rid[i] >= kRows) {
      printf("JOIN ROW WITH A ROWID OUT OF RANGE\n");
      exit(1);
    }
    if (lk[i] != rk[i] || lk[i] != key_of(lid[i], true) || rk[i] != key_of(rid[i], false)) {
      printf("JOIN ROW WITH WRONG KEYS at %zu\n", i);
      exit(1);
    }
    if (lu8[i] != u8_of(lid[i]) || lf64[i] != f64_bits_of(lid[i]) ||
        rf32[i] != f32_bits_of(rid[i])) {
      printf("JOIN ROW WITH A PAYLOAD THAT IS NOT ITS ROW'S at %zu\n", i);
      exit(1);
    }
    s += dj_mix64((uint64_t)(uint16_t)lk[i] ^
                  dj_mix64((uint64_t)lid[i] ^ dj_mix64((uint64_t)rid[i] + 0x9e37ull)));
  }
  *sum = s;
  *rows = t.num_rows();
}

int main(int argc, char** argv)
{
  const int G = argc > 1 ? atoi(argv[1]) : 2;
  const int nvl = argc > 2 ? atoi(argv[2]) : G;
  const bool compress = argc > 3 && atoi(argv[3]) != 0;
  if (G < 1 || G > 16) {
    printf("G must be in 1..16\n");
    return 1;
  }
  CHECK(hipSetDevice(0));

  /* single-rank reference on the global tables */
  uint64_t want_sum = 0;
  int64_t want_rows = 0;
  {
    auto left = make_table(0, kRows, true);
    auto right = make_table(0, kRows, false);
    Mailbox mb;
    LoopbackComm comm(0, 1, &mb);
    auto lo = generate_compression_options_distributed(left->view(), false);
    auto ro = generate_compression_options_distributed(right->view(), false);
    auto res = distributed_inner_join(left->view(), right->view(), {0}, {0}, &comm, lo, ro, 1,
                                      false, nullptr, 1);
    checksum(*res, &want_sum, &want_rows);
  }
  if (want_rows < kRows) {
    printf("reference join suspiciously small: %lld rows\n", (long long)want_rows);
    return 1;
  }

  {
    Mailbox mb;
    std::vector<uint64_t> sums((size_t)G, 0);
    std::vector<int64_t> rows((size_t)G, 0);
    run_ranks(G, &mb, [&](int r, Communicator* comm) {
      const int64_t row0 = kRows * r / G, row1 = kRows * (r + 1) / G;
      auto left = make_table(row0, row1 - row0, true);
      auto right = make_table(row0, row1 - row0, false);
      auto lo = generate_compression_options_distributed(left->view(), compress);
      auto ro = generate_compression_options_distributed(right->view(), compress);
      auto res = distributed_inner_join(left->view(), right->view(), {0}, {0}, comm, lo, ro,
                                        2, false, nullptr, nvl);
      checksum(*res, &sums[(size_t)r], &rows[(size_t)r]);
    });
    uint64_t got_sum = 0;
    int64_t got_rows = 0;
    for (int r = 0; r < G; r++) {
      got_sum += sums[(size_t)r];
      got_rows += rows[(size_t)r];
    }
    printf("single-rank: rows=%lld sum=%llx; %d-rank(nvl=%d, comp=%d): rows=%lld sum=%llx\n",
           (long long)want_rows, (unsigned long long)want_sum, G, nvl, (int)compress,
           (long long)got_rows, (unsigned long long)got_sum);
    if (got_rows != want_rows || got_sum != want_sum) {
      printf("DTYPE LOOPBACK MISMATCH\n");
      return 1;
    }
  }
  printf("DTYPE LOOPBACK OK\n");
  return 0;
}
