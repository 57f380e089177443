/*
 * dj_compress_opts.hip — the compression options of include/compression.hpp:
 * validation, the generators (fixed policy, none, sampling auto-select) and
 * the broadcasts of rank 0's choice. The codec itself is dj_compress.hip.
 */
#include "dj_host.hpp"

#include <stdexcept>

namespace dj_host {

void validate_compression(std::vector<ColumnCompressionOptions> const& opts)
{
  for (auto& o : opts) {
    if (!o.children_compression_options.empty())
      validate_compression(o.children_compression_options);
    if (o.compression_method == CompressionMethod::none) continue;
    if (o.compression_method == CompressionMethod::lz4)
      throw std::runtime_error("lz4 compression is not implemented (cascaded or none)");
    if (o.cascaded_format.num_RLEs < 0 || o.cascaded_format.num_RLEs > 1)
      throw std::runtime_error("cascaded num_RLEs must be 0 or 1 (one RLE pass; "
                               "dj_compress.hip wire format)");
    if (o.cascaded_format.num_deltas < 0 || o.cascaded_format.num_deltas > 1)
      throw std::runtime_error("cascaded num_deltas must be 0 or 1");
  }
}

void validate_compression(cudf::table_view t, std::vector<ColumnCompressionOptions> const& opts)
{
  validate_compression(opts);
  for (cudf::size_type c = 0; c < t.num_columns() && (size_t)c < opts.size(); c++) {
    const cudf::data_type ty = t.column(c).type();
    if (opts[c].compression_method == CompressionMethod::cascaded &&
        ty.id() != cudf::type_id::STRING && !cudf::is_cascaded_supported(ty))
      throw std::runtime_error("Unsupported type for cascaded compressor");
  }
}

/* The GENERIC plan API (append_to_all_to_all_comm_buffers + all_to_all_comm
 * + postprocess_all_to_all_comm) refuses cascaded options BY DESIGN, not as
 * a stub: the reference exchanges compressed slice sizes over an MPI
 * side-channel while the caller's NCCL group is open
 * (all_to_all_comm.cpp:420-478 + communicate_sizes via MPI); RCCL has no
 * such side-channel, and grouped p2p cannot post data recvs whose counts
 * arrive in the same group. Compressed wires therefore run through the
 * self-contained paths — AllToAllCommunicator::launch_communication,
 * shuffle_on, distributed_inner_join — which own their group discipline
 * and DO execute cascaded end to end (the paths the reference's benchmarks
 * exercise). See INTEGRATION.md "Known restrictions". */
void check_no_compression(std::vector<ColumnCompressionOptions> const& opts)
{
  for (auto& o : opts)
    if (o.compression_method != CompressionMethod::none)
      throw std::runtime_error(
        "this entry point executes uncompressed buffers only; use "
        "AllToAllCommunicator::launch_communication for cascaded compression");
}

}  // namespace dj_host

using namespace dj_host;

std::vector<ColumnCompressionOptions> generate_compression_options_distributed(
  cudf::table_view input, bool compression)
{
  if (!compression)
    return std::vector<ColumnCompressionOptions>(
      (size_t)input.num_columns(), ColumnCompressionOptions(CompressionMethod::none));
  /* fixed policy standing in for the reference's nvcomp auto-selector
   * (compression.hpp:253-292): bitpack-only cascaded for fixed-width columns
   * and the row-size wire of STRING columns; chars are never compressed
   * (reference policy, compression.cpp:44-60) */
  std::vector<ColumnCompressionOptions> opts;
  nvcompCascadedFormatOpts bp{};
  bp.num_RLEs = 0;
  bp.num_deltas = 0;
  bp.use_bp = 1;
  for (cudf::size_type c = 0; c < input.num_columns(); c++) {
    const cudf::data_type ty = input.column(c).type();
    if (ty.id() == cudf::type_id::STRING || cudf::is_cascaded_supported(ty))
      opts.emplace_back(CompressionMethod::cascaded, bp);
    else
      opts.emplace_back(CompressionMethod::none);  // FLOAT32/FLOAT64/BOOL8
  }
  return opts;
}

std::vector<ColumnCompressionOptions> generate_none_compression_options(cudf::table_view input)
{
  std::vector<ColumnCompressionOptions> opts;
  for (cudf::size_type c = 0; c < input.num_columns(); c++) {
    if (input.column(c).type().id() == cudf::type_id::STRING) {
      std::vector<ColumnCompressionOptions> kids(
        2, ColumnCompressionOptions(CompressionMethod::none));
      opts.emplace_back(CompressionMethod::none, nvcompCascadedFormatOpts{}, kids);
    } else {
      opts.emplace_back(CompressionMethod::none);
    }
  }
  return opts;
}

/* sampling selector over our executable cascaded schemes ({0|1 RLE} x
 * {0|1 deltas} + bitpack): picks the scheme with the smaller estimated
 * packed total on a host-side sample, in the role of nvcomp's
 * CascadedSelector (reference compression.hpp:253-292,
 * compression.cpp:36-69). Selection is data-dependent, not parity-pinned
 * (nvcomp is absent). */
static nvcompCascadedFormatOpts select_cascaded_on_sample(const void* d_data, int64_t n,
                                                          int esize)
{
  nvcompCascadedFormatOpts o{};
  o.use_bp = 1;
  const int64_t sample = std::min<int64_t>(n, 65536);
  if (sample < 2) return o;
  std::vector<int64_t> h((size_t)sample);
  if (esize == 8) {
    DJ_HIP_CALL(hipMemcpy(h.data(), d_data, (size_t)sample * 8, hipMemcpyDeviceToHost));
  } else {
    /* narrower elements enter as the codec loads them: sign-extended */
    std::vector<int8_t> raw((size_t)sample * esize);
    DJ_HIP_CALL(hipMemcpy(raw.data(), d_data, raw.size(), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < sample; i++)
      h[(size_t)i] = esize == 4   ? (int64_t)((const int32_t*)raw.data())[i]
                     : esize == 2 ? (int64_t)((const int16_t*)raw.data())[i]
                                  : (int64_t)raw[(size_t)i];
  }
  auto zigzag = [](int64_t v) { return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63); };
  auto packed_bits = [&](const std::vector<int64_t>& v, bool delta) {
    uint64_t total = 0;
    const int64_t m = (int64_t)v.size();
    for (int64_t g = 0; g < m; g += 32) {
      int w = 0;
      const int64_t e = std::min<int64_t>(g + 32, m);
      for (int64_t i = g; i < e; i++) {
        int64_t d = delta ? (i ? v[(size_t)i] - v[(size_t)i - 1] : v[0]) : v[(size_t)i];
        uint64_t z = zigzag(d) | 1;
        w = std::max(w, 64 - __builtin_clzll(z));
      }
      total += (uint64_t)w * 32;
    }
    return total;
  };
  /* RLE candidate: run values + run lengths on the sample */
  std::vector<int64_t> rvals, rlens;
  rvals.reserve((size_t)sample);
  for (int64_t i = 0; i < sample; i++) {
    if (i == 0 || h[(size_t)i] != h[(size_t)i - 1]) {
      rvals.push_back(h[(size_t)i]);
      rlens.push_back(1);
    } else {
      rlens.back()++;
    }
  }
  struct Cand {
    int rle, delta;
    uint64_t bits;
  };
  std::vector<Cand> cands;
  cands.push_back({0, 0, packed_bits(h, false)});
  cands.push_back({0, 1, packed_bits(h, true)});
  if ((int64_t)rvals.size() * 2 < sample) {  // only worth considering on runs
    uint64_t lbits = packed_bits(rlens, false);
    cands.push_back({1, 0, packed_bits(rvals, false) + lbits});
    cands.push_back({1, 1, packed_bits(rvals, true) + lbits});
  }
  const Cand* best = &cands[0];
  for (const auto& c : cands)
    if (c.bits < best->bits) best = &c;
  o.num_RLEs = best->rle;
  o.num_deltas = best->delta;
  return o;
}

std::vector<ColumnCompressionOptions> generate_auto_select_compression_options(
  cudf::table_view input_table)
{
  /* reference compression.cpp:36-69: per-column sampling selection; STRING
   * columns: select on the offsets child, never compress chars */
  std::vector<ColumnCompressionOptions> opts;
  for (cudf::size_type c = 0; c < input_table.num_columns(); c++) {
    cudf::column_view col = input_table.column(c);
    if (col.type().id() == cudf::type_id::STRING) {
      std::vector<ColumnCompressionOptions> kids;
      kids.emplace_back(
        CompressionMethod::cascaded,
        select_cascaded_on_sample(col.child(0).head<int32_t>(), col.size() + 1, 4));
      kids.emplace_back(CompressionMethod::none);
      opts.emplace_back(CompressionMethod::none, nvcompCascadedFormatOpts{}, kids);
    } else if (!cudf::is_cascaded_supported(col.type())) {
      /* FLOAT32/FLOAT64/BOOL8: not cascaded-supported, as in the reference */
      opts.emplace_back(CompressionMethod::none);
    } else {
      opts.emplace_back(
        CompressionMethod::cascaded,
        select_cascaded_on_sample(col.head<char>(), col.size(), cudf::size_of(col.type())));
    }
  }
  return opts;
}

ColumnCompressionOptions broadcast_compression_options(cudf::column_view input_column,
                                                       ColumnCompressionOptions input_options,
                                                       Communicator* comm)
{
  /* reference compression.cpp:95-130 used MPI_Bcast on MPI_COMM_WORLD; here
   * rank 0's choices travel over the given Communicator (grouped send/recv
   * of a POD through device staging — RCCL transports device buffers
   * only) */
  struct Pod {
    int method, rles, deltas, bp;
  };
  Pod pod{(int)input_options.compression_method, input_options.cascaded_format.num_RLEs,
          input_options.cascaded_format.num_deltas, input_options.cascaded_format.use_bp};
  if (comm->mpi_size > 1) {
    DBuf stage(sizeof(Pod));
    if (comm->mpi_rank == 0)
      DJ_HIP_CALL(hipMemcpy(stage.p, &pod, sizeof(Pod), hipMemcpyHostToDevice));
    comm->start();
    if (comm->mpi_rank == 0) {
      for (int r = 1; r < comm->mpi_size; r++) comm->send(stage.p, sizeof(Pod), 1, r);
    } else {
      comm->recv(stage.p, sizeof(Pod), 1, 0);
    }
    comm->stop();
    DJ_HIP_CALL(hipMemcpy(&pod, stage.p, sizeof(Pod), hipMemcpyDeviceToHost));
  }
  nvcompCascadedFormatOpts fmt{};
  fmt.num_RLEs = pod.rles;
  fmt.num_deltas = pod.deltas;
  fmt.use_bp = pod.bp;
  std::vector<ColumnCompressionOptions> kids;
  if (input_column.type().id() == cudf::type_id::STRING) {
    for (size_t k = 0; k < 2; k++) {
      ColumnCompressionOptions child;
      if (comm->mpi_rank == 0) {
        DJ_CHECK_ERROR(input_options.children_compression_options.size() == 2,
                       "STRING compression options need 2 children");
        child = input_options.children_compression_options[k];
      }
      kids.push_back(broadcast_compression_options(input_column.child((cudf::size_type)k),
                                                   child, comm));
    }
  }
  return ColumnCompressionOptions((CompressionMethod)pod.method, fmt, kids);
}

std::vector<ColumnCompressionOptions> broadcast_compression_options(
  cudf::table_view input_table, std::vector<ColumnCompressionOptions> input_options,
  Communicator* comm)
{
  std::vector<ColumnCompressionOptions> out;
  for (cudf::size_type c = 0; c < input_table.num_columns(); c++) {
    ColumnCompressionOptions col_opts;
    if (comm->mpi_rank == 0) col_opts = input_options[(size_t)c];
    out.push_back(broadcast_compression_options(input_table.column(c), col_opts, comm));
  }
  return out;
}

ColumnCompressionOptions broadcast_compression_options(cudf::column_view input_column,
                                                       ColumnCompressionOptions input_options)
{
  return broadcast_compression_options(input_column, input_options, default_communicator());
}

std::vector<ColumnCompressionOptions> broadcast_compression_options(
  cudf::table_view input_table, std::vector<ColumnCompressionOptions> input_options)
{
  return broadcast_compression_options(input_table, input_options, default_communicator());
}
