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
