/*
 * dj_host.hpp — internal: what crosses between the host orchestration units
 * behind the C++ drop-in surface (the headers under include/). One unit per
 * layer:
 *
 *   dj_devmem.hip         caching device allocator, DBuf, scalar read-back
 *   dj_key_helpers.hip    the key helper kernels (launchers in dj_kernels.hpp)
 *   dj_cudf_shim.hip      cudf::column
 *   dj_comm.hip           RCCLCommunicator, the default communicator
 *   dj_compress_opts.hip  compression option checks, generators, broadcasts
 *   dj_all_to_all.hip     CommunicationGroup, size exchange, plan API,
 *                         AllToAllCommunicator
 *   dj_table_ops.hip      key predicates, fuse, gather, partition, concat
 *   dj_local_join.hip     the bucket-join wrapper and the four join kinds
 *   dj_distributed.hip    the distributed routes, shuffle_on, distribute_table
 *   dj_cpp_cabi.hip       the extern "C" entry points over all of it
 *
 * Everything here has external linkage and exactly one definition, so the
 * process-wide state (the allocator pool, the default communicator) exists
 * once however many units use it.
 */
#pragma once

#include "dj_error.hpp"
#include "dj_kernels.hpp"
#include "dj_runtime.hpp"
#include "dj_timing.hpp"

#include "../../include/all_to_all_comm.hpp"
#include "../../include/communicator.hpp"
#include "../../include/compression.hpp"
#include "../../include/distribute_table.hpp"
#include "../../include/distributed_join.hpp"
#include "../../include/distributed_join.h"
#include "../../include/shuffle_on.hpp"

#include "dj_hash.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace dj_host {

/* ------------------------------------------ device memory (dj_devmem.hip) */

/* the one caching allocator of the process (thread-safe) */
void* pool_alloc(size_t bytes);
void pool_free(void* p);

/* small owning device buffer, pool-backed */
struct DBuf {
  void* p{nullptr};
  DBuf() = default;
  explicit DBuf(size_t bytes)
  {
    if (bytes) p = pool_alloc(bytes);
  }
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  DBuf(DBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  DBuf& operator=(DBuf&& o) noexcept
  {
    if (this != &o) {
      pool_free(p);
      p = o.p;
      o.p = nullptr;
    }
    return *this;
  }
  ~DBuf() { pool_free(p); }
  int64_t* i64() { return (int64_t*)p; }
};

void sync_streams();

/* `bytes` bytes at device address d, copied to h on `st`; returns once the
 * stream has been synchronized */
void read_back_bytes(void* h, const void* d, size_t bytes, hipStream_t st);

/* the scalar (or small POD) a kernel enqueued on `st` left at d.
 * Host-synchronous on `st`. */
template <class T>
T read_back(const void* d, hipStream_t st)
{
  T h;
  read_back_bytes(&h, d, sizeof(T), st);
  return h;
}

/* one source range of dj::copy_bitmask_segments: nbits bits of `src` (nullptr
 * = all valid) from bit src_bit on; destination ranges follow one another */
struct BitSeg {
  const uint32_t* src;
  int64_t src_bit;
  int64_t nbits;
};

/* dst bits [0, sum nbits) = the segments back to back, on `st`. Returns the
 * device segment table, which must outlive the kernel: keep it until the
 * stream has been synchronized. */
DBuf copy_bit_segments(std::vector<BitSeg> const& segs, uint32_t* dst, hipStream_t st);

/* --------------------------------------------- communicators (dj_comm.hip) */

/* the communicator default_communicator() hands out when it is set: the last
 * RCCLCommunicator built, or what dj_cpp_comm_create made */
extern Communicator* g_default_comm;

/* size-1 stand-in so the C++ API works single-process without RCCL */
class LocalCommunicator : public Communicator {
 public:
  LocalCommunicator()
  {
    mpi_rank = 0;
    mpi_size = 1;
  }
  void initialize() override {}
  void start() override {}
  void stop() override { sync_streams(); }
  void send(const void*, int64_t, int, int) override
  {
    DJ_CHECK_ERROR(false, "LocalCommunicator cannot send (single process)");
  }
  void recv(void*, int64_t, int, int) override
  {
    DJ_CHECK_ERROR(false, "LocalCommunicator cannot recv (single process)");
  }
  void finalize() override {}
  bool group_by_batch() override { return true; }
};

/* ------------------------------ compression options (dj_compress_opts.hip) */

void validate_compression(std::vector<ColumnCompressionOptions> const& opts);
/* typed check: like the reference's cascaded dispatch (declared for the
 * signed/unsigned integer types only), FLOAT32/FLOAT64/BOOL8 columns refuse
 * a cascaded option instead of packing their bit patterns */
void validate_compression(cudf::table_view t, std::vector<ColumnCompressionOptions> const& opts);
void check_no_compression(std::vector<ColumnCompressionOptions> const& opts);

/* ---------------------------------------------- table ops (dj_table_ops.hip) */

bool is_string(cudf::column_view col);
/* dj::kKey* kind of an integer-rep key column; FLOAT32/FLOAT64 keys refuse
 * loudly */
int key_kind(cudf::data_type t);
void check_key_pairs(cudf::table_view left, cudf::table_view right,
                     std::vector<cudf::size_type> const& lon,
                     std::vector<cudf::size_type> const& ron);
bool any_nullable(cudf::table_view t);
bool any_nullable_key(cudf::table_view t, std::vector<cudf::size_type> const& on);
/* bit c set: column c carries a validity mask (columns 0..31) */
uint32_t nullable_bits(cudf::table_view t);
void check_no_masks(cudf::table_view t, const char* what);
bool any_string_key(cudf::table_view t, std::vector<cudf::size_type> const& on);

/* -> DBuf of n fused int64 keys for the given key columns (<= 4; integer-rep
 * or STRING) */
DBuf fuse_keys(cudf::table_view t, std::vector<cudf::size_type> const& on, hipStream_t st);
/* the engine's int64 view of an integer-rep key column: the column itself
 * when it is 64-bit, else widened on `st` into `dst` (col.size() int64s the
 * caller allocated — nothing is allocated here) */
const int64_t* key_as_i64(cudf::column_view col, int64_t* dst, hipStream_t st);
/* same on the compute stream, allocating `tmp` when the column needs widening */
const int64_t* key_as_i64(cudf::column_view col, DBuf& tmp);

/* a table view over two INT64 device arrays */
cudf::table_view view_i64_pair(const void* c0, const void* c1, int64_t n);
/* both sides of a join have the hot shape (exactly two INT64 columns, no
 * mask) with the key in front */
bool joins_i64_pairs(cudf::table_view left, cudf::table_view right, cudf::size_type left_key,
                     cudf::size_type right_key);

/* output assembly: append to `cols` one n-row column per column of `src`,
 * row i = src row idx[i] (see the definition for key_col / key_vals /
 * null_tail) */
void gather_table_columns(cudf::table_view src, DBuf& idx, int64_t n, cudf::size_type key_col,
                          DBuf* key_vals, std::vector<std::unique_ptr<cudf::column>>& cols,
                          hipStream_t st, int64_t null_tail = -1);

struct PartitionedTable {
  std::unique_ptr<cudf::table> tbl;
  std::vector<cudf::size_type> offsets;  // nparts+1
};
/* stable hash-partition of a table into nparts contiguous ranges. ext_keys:
 * when non-null, placement uses this caller-provided key array (fused
 * multi-column keys) instead of column key_col */
PartitionedTable partition_table(cudf::table_view in, cudf::size_type key_col, int nparts,
                                 int hash_fn, uint32_t seed, const int64_t* ext_keys = nullptr);
/* the placement step of shuffle_on */
PartitionedTable place_rows(cudf::table_view input, std::vector<cudf::size_type> const& on,
                            int nparts, int hash_fn, uint32_t seed);
std::unique_ptr<cudf::table> concat_tables(std::vector<std::unique_ptr<cudf::table>>& parts);

/* -------------------------------------------- local join (dj_local_join.hip) */

/* what one bucket join leaves on the device besides its rows: the match
 * counter and the engine's two flags, in one block so that a single 16-byte
 * copy reads them back */
struct JoinMeta {
  int64_t count;     // matches found (may exceed the capacity written)
  int error;         // sentinel (-1) keys seen and skipped
  int any_overflow;  // skewed buckets skipped
};
static_assert(sizeof(JoinMeta) == 16 && offsetof(JoinMeta, count) == 0 &&
                offsetof(JoinMeta, error) == 8 && offsetof(JoinMeta, any_overflow) == 12,
              "JoinMeta is read back from the device as one 16-byte block");

/* engine outputs of one join, `cap` rows each: o0/o2 the joined key values
 * (left/right), o1/o3 the payloads — source row indices unless the tables
 * are int64 pairs (joins_i64_pairs) */
struct JoinOut {
  DBuf o0, o1, o2, o3, meta;
  int64_t cap{0};
  JoinOut() = default;
  explicit JoinOut(int64_t cap_)
    : o0((size_t)cap_ * 8),
      o1((size_t)cap_ * 8),
      o2((size_t)cap_ * 8),
      o3((size_t)cap_ * 8),
      meta(sizeof(JoinMeta)),
      cap(cap_)
  {
  }
  /* first-try capacity for rn probe rows; the engine counts every match but
   * writes only the first cap, so a count above it means redo */
  static int64_t default_cap(int64_t rn) { return std::max<int64_t>(rn + (rn >> 3), 1024); }
  int64_t* counter() { return &((JoinMeta*)meta.p)->count; }
  int* error() { return &((JoinMeta*)meta.p)->error; }
  int* any_overflow() { return &((JoinMeta*)meta.p)->any_overflow; }
  void clear(hipStream_t st) { DJ_HIP_CALL(hipMemsetAsync(meta.p, 0, sizeof(JoinMeta), st)); }
};

/* the empty table with a join's output schema: left's columns, then right's */
std::unique_ptr<cudf::table> empty_join_result(cudf::table_view left, cudf::table_view right);
/* nout joined rows of an INNER join -> left-cols + right-cols */
std::unique_ptr<cudf::table> assemble_join_output(cudf::table_view left, cudf::table_view right,
                                                  JoinOut& out, int64_t nout,
                                                  cudf::size_type left_key,
                                                  cudf::size_type right_key);
/* local join of two tables via the bucketed-LDS engine, any kind */
std::unique_ptr<cudf::table> local_join(
  join_kind kind, cudf::table_view left, cudf::table_view right,
  std::vector<cudf::size_type> const& lon, std::vector<cudf::size_type> const& ron,
  cudf::null_equality compare_nulls = cudf::null_equality::EQUAL);

/* null_equality::UNEQUAL over several ranks: a table cut into `valid`, its
 * rows without a null in their key tuple, and, when asked for, `null_rows`,
 * the others. Both are null when no key column holds a null. */
struct StrippedTable {
  std::unique_ptr<cudf::table> valid, null_rows;
};
StrippedTable strip_null_keys(cudf::table_view t, std::vector<cudf::size_type> const& on,
                              bool keep_null_rows, const cudf::table_view* pad_with);

}  // namespace dj_host

/* access hook for the fused path (friend declared in all_to_all_comm.hpp);
 * defined in dj_all_to_all.hip */
struct AllToAllCommunicatorAccess {
  static const std::vector<int64_t>& recv_offsets(const AllToAllCommunicator& a);
  /* an AllToAllCommunicator whose row-count exchange carries the join's
   * route tag (join_route_tag, dj_distributed.hip) */
  static std::unique_ptr<AllToAllCommunicator> make(
    cudf::table_view t, std::vector<cudf::size_type> offsets, CommunicationGroup group,
    Communicator* communicator, std::vector<ColumnCompressionOptions> const& opts,
    bool explicit_copy, uint32_t route_tag);
};
