/*
 * distributed_join.hpp — top-level distributed inner join, mirroring the
 * reference's exact signature (reference: src/distributed_join.hpp:65-76)
 * over our re-declared cudf types (dj_cudf_types.hpp).
 *
 * Semantics kept (reference pins):
 *  - collective over all ranks; `left`/`right` are each rank's slice of the
 *    global tables (distributed_join.hpp:30-44 doc)
 *  - result columns: all left columns then all right columns, join keys
 *    duplicated (compare_against_single_gpu.cu:163-165); row order
 *    unspecified; concatenation over ranks is the global join result
 *  - joining with an empty side yields an empty table
 *    (distributed_join.cpp:76-83)
 *  - over_decom_factor batches the exchange+join (distributed_join.cpp:244-329)
 *  - partition seed 12345678 intra-node (distributed_join.cpp:211)
 *
 * The 2-level hierarchy is implemented with the reference's semantics
 * (distributed_join.cpp:55-69,152-199): nvlink_domain_size selects the
 * join-group size via the same divisor search; when it is smaller than the
 * world, both tables are first shuffled across domains (seed 87654321) and
 * the batched pipeline runs within each domain. On one 8x MI355X node
 * (full xGMI mesh) nvlink_domain_size >= world collapses to the flat
 * single-level all-to-all, which is bandwidth-optimal there. The engine
 * below the API is the bucketed-LDS join (dj_kernels.hip), not cuDF.
 */
#pragma once

#include "communicator.hpp"
#include "compression.hpp"
#include "dj_cudf_types.hpp"

#include <cstdint>
#include <memory>
#include <vector>

/* vs the reference signature below: up to 4 key columns are supported, each
 * integer-rep or STRING (a STRING key pairs with a STRING key). Composite
 * keys, and a STRING key even alone, join on a fused key chain — a STRING
 * row enters as the 64-bit hash of its bytes — with a post-join filter that
 * compares the real columns byte for byte, and take the shuffle +
 * local-join route (over_decom_factor is accepted there and has no effect).
 * The key columns, STRING ones included, appear in the output on both
 * sides. nparts = join-group size x over_decom_factor caps at 1024. See
 * INTEGRATION.md "Known restrictions". */
std::unique_ptr<cudf::table> distributed_inner_join(
  cudf::table_view left,
  cudf::table_view right,
  std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on,
  Communicator* communicator,
  std::vector<ColumnCompressionOptions> left_compression_options,
  std::vector<ColumnCompressionOptions> right_compression_options,
  int over_decom_factor            = 1,
  bool report_timing               = false,
  void* preallocated_pinned_buffer = nullptr,
  int nvlink_domain_size           = 1);

/* ---- joins that keep left rows without a partner (additions to the
 * reference's surface; cudf::left_join / left_semi_join / left_anti_join
 * semantics) ----
 *
 * join_kind selects what distributed_join returns on each rank; the
 * concatenation over ranks is the global result, row order unspecified:
 *
 *  INNER      exactly distributed_inner_join (with null_equality::EQUAL the
 *             call is forwarded).
 *  LEFT       all left columns then all right columns. Every matching pair
 *             appears as in the inner join; every left row without a match
 *             appears once with null right-hand cells. EVERY right-hand
 *             output column carries a validity mask, on every rank, also
 *             when nothing was unmatched and when the source column had
 *             none; its null_count is exact (gathered nulls + unmatched
 *             rows). The values under the padded nulls are zero bytes, the
 *             padded STRING rows are empty. Left-hand columns have a mask
 *             exactly when their source had one.
 *  LEFT_SEMI  the left columns of the left rows that have at least one
 *             match, each once.
 *  LEFT_ANTI  the left columns of the left rows that have no match.
 *
 * Null keys, compare_nulls (the trailing argument of distributed_join and its
 * three named siblings; distributed_inner_join keeps the reference's
 * signature and is always EQUAL). Values stored under a null are never looked
 * at in either mode.
 *  null_equality::EQUAL (the default, cuDF's default and what the reference
 *    runs): a null key element matches a null element in the same position of
 *    the tuple and no valid one.
 *  null_equality::UNEQUAL (SQL: NULL = NULL is not true): a row with a null in
 *    any column of its key tuple matches nothing. Null-key right rows are in no
 *    result. Null-key left rows are dropped by INNER and LEFT_SEMI, appear once
 *    each with null right-hand cells in LEFT, and are kept by LEFT_ANTI. Valid
 *    keys join as under EQUAL; without a null in any key column the two modes
 *    give the same rows. Mask presence on output columns follows the kind's
 *    rule above in both modes. On one rank the null-key rows stay out of the
 *    bucket join and a single integer key does not need the fused key chain;
 *    over several ranks each rank strips its tables to their valid-key rows
 *    before anything is communicated (one extra gather of a table whose key
 *    holds nulls), runs the EQUAL route on them, and appends its own null-key
 *    left rows (LEFT, LEFT_ANTI) to its result: null-key rows never reach
 *    the communicator. INNER under UNEQUAL is
 *    distributed_join(join_kind::INNER, ..., null_equality::UNEQUAL).
 * An empty left table gives an empty result of the kind's schema; an empty
 * right table gives LEFT = every left row with an all-null right side,
 * LEFT_SEMI = empty, LEFT_ANTI = every left row.
 *
 * Route: the same validation and inter-domain stage as the inner join, then
 * both tables are shuffled inside the join group and joined locally — after
 * the shuffle every right row that could match a left row is on that row's
 * rank, so no further communication decides matched / unmatched.
 * over_decom_factor is accepted and has no effect (as for composite keys in
 * the inner join). Compression options apply to the shuffles. For LEFT_SEMI
 * and LEFT_ANTI only the right table's key columns are shuffled (with their
 * compression options); right-hand payload bytes never reach the
 * communicator. */
enum class join_kind { INNER, LEFT, LEFT_SEMI, LEFT_ANTI };

std::unique_ptr<cudf::table> distributed_join(
  join_kind kind,
  cudf::table_view left,
  cudf::table_view right,
  std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on,
  Communicator* communicator,
  std::vector<ColumnCompressionOptions> left_compression_options,
  std::vector<ColumnCompressionOptions> right_compression_options,
  int over_decom_factor            = 1,
  bool report_timing               = false,
  void* preallocated_pinned_buffer = nullptr,
  int nvlink_domain_size           = 1,
  cudf::null_equality compare_nulls = cudf::null_equality::EQUAL);

/* distributed_join(join_kind::LEFT, ...) */
std::unique_ptr<cudf::table> distributed_left_join(
  cudf::table_view left,
  cudf::table_view right,
  std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on,
  Communicator* communicator,
  std::vector<ColumnCompressionOptions> left_compression_options,
  std::vector<ColumnCompressionOptions> right_compression_options,
  int over_decom_factor            = 1,
  bool report_timing               = false,
  void* preallocated_pinned_buffer = nullptr,
  int nvlink_domain_size           = 1,
  cudf::null_equality compare_nulls = cudf::null_equality::EQUAL);

/* distributed_join(join_kind::LEFT_SEMI, ...) */
std::unique_ptr<cudf::table> distributed_left_semi_join(
  cudf::table_view left,
  cudf::table_view right,
  std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on,
  Communicator* communicator,
  std::vector<ColumnCompressionOptions> left_compression_options,
  std::vector<ColumnCompressionOptions> right_compression_options,
  int over_decom_factor            = 1,
  bool report_timing               = false,
  void* preallocated_pinned_buffer = nullptr,
  int nvlink_domain_size           = 1,
  cudf::null_equality compare_nulls = cudf::null_equality::EQUAL);

/* distributed_join(join_kind::LEFT_ANTI, ...) */
std::unique_ptr<cudf::table> distributed_left_anti_join(
  cudf::table_view left,
  cudf::table_view right,
  std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on,
  Communicator* communicator,
  std::vector<ColumnCompressionOptions> left_compression_options,
  std::vector<ColumnCompressionOptions> right_compression_options,
  int over_decom_factor            = 1,
  bool report_timing               = false,
  void* preallocated_pinned_buffer = nullptr,
  int nvlink_domain_size           = 1,
  cudf::null_equality compare_nulls = cudf::null_equality::EQUAL);
