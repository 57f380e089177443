/*
 * dj_distributed.hip — the routes over several ranks: distributed_inner_join
 * (shuffle + local join, the batched pipeline, the fused wire pipeline),
 * distributed_join for the other kinds, shuffle_on, distribute_table and
 * collect_tables (include/distributed_join.hpp, shuffle_on.hpp,
 * distribute_table.hpp).
 */
#include "dj_host.hpp"

#include <chrono>
#include <cmath>
#include <iostream>

using namespace dj_host;

namespace {

/* what batch finalisation needs of a pipeline batch; both pipelines' Batch
 * structs extend it with their own staging */
struct BatchJoin {
  std::unique_ptr<AllToAllCommunicator> latoa, ratoa;
  std::unique_ptr<cudf::table> lrecv, rrecv;  // this rank's share of the batch
  JoinOut out;                                // its join, enqueued by the pipeline
};

/* the end of both batched pipelines, once the compute stream has drained:
 * per batch read the counts, redo the rare failures, assemble the columns;
 * then concatenate. A batch with an empty side had nothing enqueued and its
 * meta block is all zero. The redo goes synchronously through
 * local_join, whose bucket path joins sentinel (-1) keys out-of-band
 * (neg1_cross_join), re-joins skewed buckets via the global-table fallback
 * and sizes the output exactly. The flags are looked at BEFORE the count:
 * the enqueued join skips -1 keys and oversized buckets, so its count can be
 * 0 while the redo still finds rows. */
template <class Batch>
std::unique_ptr<cudf::table> finalize_batches(std::vector<Batch>& batches,
                                              cudf::size_type left_key,
                                              cudf::size_type right_key, bool report_timing,
                                              int rank)
{
  std::vector<std::unique_ptr<cudf::table>> results;
  for (BatchJoin& bt : batches) {
    const cudf::table_view l = bt.lrecv->view(), r = bt.rrecv->view();
    JoinMeta meta;
    DJ_HIP_CALL(hipMemcpy(&meta, bt.out.meta.p, sizeof(meta), hipMemcpyDeviceToHost));
    if (l.num_rows() == 0 || r.num_rows() == 0)
      results.push_back(empty_join_result(l, r));
    else if (meta.error || meta.any_overflow || meta.count > bt.out.cap)
      results.push_back(local_join(join_kind::INNER, l, r, {left_key}, {right_key}));
    else if (meta.count == 0)
      results.push_back(empty_join_result(l, r));
    else
      results.push_back(assemble_join_output(l, r, bt.out, meta.count, left_key, right_key));
  }
  const auto t_cat0 = std::chrono::steady_clock::now();
  auto result = concat_tables(results);
  if (report_timing && batches.size() > 1)
    std::cout << "Rank " << rank << ": concatenation takes "
              << std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() -
                                                           t_cat0)
                   .count()
              << "ms" << std::endl;
  return result;
}

/* The route distributed_inner_join takes depends on nullability, which each
 * rank sees only of its own tables: bit 0 = a key column is nullable (shuffle
 * + local join on the fused key chain), bit 1 = two-column tables carrying a
 * mask (which keeps 2 x INT64 tables off the fused wire path). Every route
 * starts with the row-count exchange of an AllToAllCommunicator over the
 * left table, one count per peer whatever the route, so the tag rides it and
 * ranks that disagree stop loudly there instead of pairing mismatched
 * messages. */
uint32_t join_route_tag(cudf::table_view left, cudf::table_view right,
                        std::vector<cudf::size_type> const& lon,
                        std::vector<cudf::size_type> const& ron)
{
  uint32_t tag = 0;
  if (any_nullable_key(left, lon) || any_nullable_key(right, ron)) tag |= 1u;
  if (left.num_columns() == 2 && right.num_columns() == 2 &&
      (any_nullable(left) || any_nullable(right)))
    tag |= 2u;
  return tag;
}

/* shuffle_on whose row-count exchange carries a route tag */
std::unique_ptr<cudf::table> shuffle_on_tagged(
  cudf::table_view const& input, std::vector<cudf::size_type> const& on_columns,
  CommunicationGroup comm_group, Communicator* communicator,
  std::vector<ColumnCompressionOptions> compression_options, cudf::hash_id hash_function,
  uint32_t hash_seed, bool report_timing, void* preallocated_pinned_buffer, uint32_t route_tag)
{
  DJ_CHECK_ERROR(on_columns.size() >= 1, "shuffle_on: at least one key column");
  const int hash_fn =
    hash_function == cudf::hash_id::HASH_IDENTITY ? DJ_HASH_IDENTITY : DJ_HASH_MURMUR3;
  DJ_CHECK_ERROR(on_columns.size() <= 4, "shuffle_on: up to 4 key columns supported");
  validate_compression(input, compression_options);
  PartitionedTable part = place_rows(input, on_columns, comm_group.size(), hash_fn, hash_seed);
  auto atoa = AllToAllCommunicatorAccess::make(part.tbl->view(), part.offsets, comm_group,
                                               communicator, compression_options, false,
                                               route_tag);
  auto out = atoa->allocate_communicated_table();
  atoa->launch_communication(out->mutable_view(), report_timing, preallocated_pinned_buffer);
  return out;
}

/* exchange per-peer int64 vectors (host) through the communicator */
void exchange_vecs(CommunicationGroup group, Communicator* communicator,
                   const std::vector<std::vector<int64_t>>& send,
                   std::vector<std::vector<int64_t>>& recv)
{
  const int G = group.size();
  const int me = group.get_local_idx();
  const int V = (int)send[0].size();
  recv.assign(G, std::vector<int64_t>(V, 0));
  recv[me] = send[me];
  if (G == 1) return;
  DBuf ds((size_t)G * V * 8), dr((size_t)G * V * 8);
  std::vector<int64_t> flat((size_t)G * V);
  for (int i = 0; i < G; i++)
    std::copy(send[i].begin(), send[i].end(), flat.begin() + (size_t)i * V);
  DJ_HIP_CALL(hipMemcpyAsync(ds.p, flat.data(), flat.size() * 8, hipMemcpyHostToDevice,
                             dj_rt_comm_stream()));
  DJ_HIP_CALL(hipStreamSynchronize(dj_rt_comm_stream()));
  communicator->start();
  for (int i = 0; i < G; i++) {
    if (i == me) continue;
    int peer = group.get_global_rank(i);
    communicator->send(ds.i64() + (size_t)i * V, V, 8, peer);
    communicator->recv(dr.i64() + (size_t)i * V, V, 8, peer);
  }
  communicator->stop();
  DJ_HIP_CALL(hipMemcpyAsync(flat.data(), dr.p, flat.size() * 8, hipMemcpyDeviceToHost,
                             dj_rt_comm_stream()));
  DJ_HIP_CALL(hipStreamSynchronize(dj_rt_comm_stream()));
  for (int i = 0; i < G; i++)
    if (i != me) recv[i].assign(flat.begin() + (size_t)i * V, flat.begin() + (size_t)(i + 1) * V);
}

/* the fused wire path (2 x INT64 columns, keys at column 0): ONE staged
 * scatter produces the rank/batch slices pre-grouped by PA groups; the
 * receiver runs pass B over per-peer segment lists straight into the LDS
 * join — the separate stable rank partition and bucket pass A disappear
 * (DESIGN.md §3 ablation: the partition passes dominated the step). */
std::unique_ptr<cudf::table> distributed_inner_join_fused(
  cudf::table_view left, cudf::table_view right, Communicator* communicator,
  CommunicationGroup group, std::vector<ColumnCompressionOptions> const& lopts,
  std::vector<ColumnCompressionOptions> const& ropts, int od, int PA, bool report_timing,
  void* pinned)
{
  hipStream_t st = dj_rt_stream();
  const int G = group.size();
  const int P = G * od * PA;
  const int64_t ln = left.num_rows(), rn = right.num_rows();

  /* fused partition of both tables (columnar outputs for the wire) */
  DBuf counts((size_t)dj::kBucketBlocks * P * 4), totals((size_t)P * 4);
  DBuf d_poff((size_t)(P + 1) * 8);
  DBuf lkp((size_t)std::max<int64_t>(ln, 1) * 8), lpp((size_t)std::max<int64_t>(ln, 1) * 8);
  DBuf rkp((size_t)std::max<int64_t>(rn, 1) * 8), rpp((size_t)std::max<int64_t>(rn, 1) * 8);
  std::vector<int64_t> lposf(P + 1, 0), rposf(P + 1, 0);
  {
    dj_timing::Scope t(DJ_PHASE_PART_SCATTER, st);
    dj::fused_partition(left.column(0).head<int64_t>(), left.column(1).head<int64_t>(), ln,
                        G * od, DJ_SEED_INTRA, PA, (uint32_t*)counts.p, (uint32_t*)totals.p,
                        d_poff.i64(), lkp.i64(), lpp.i64(), st);
    DJ_HIP_CALL(hipMemcpyAsync(lposf.data(), d_poff.p, (size_t)(P + 1) * 8,
                               hipMemcpyDeviceToHost, st));
    DJ_HIP_CALL(hipStreamSynchronize(st));
    dj::fused_partition(right.column(0).head<int64_t>(), right.column(1).head<int64_t>(), rn,
                        G * od, DJ_SEED_INTRA, PA, (uint32_t*)counts.p, (uint32_t*)totals.p,
                        d_poff.i64(), rkp.i64(), rpp.i64(), st);
    DJ_HIP_CALL(hipMemcpyAsync(rposf.data(), d_poff.p, (size_t)(P + 1) * 8,
                               hipMemcpyDeviceToHost, st));
    DJ_HIP_CALL(hipStreamSynchronize(st));
  }

  cudf::table_view lpart_view = view_i64_pair(lkp.p, lpp.p, ln);
  cudf::table_view rpart_view = view_i64_pair(rkp.p, rpp.p, rn);

  struct Batch : BatchJoin {
    std::vector<std::vector<int64_t>> lsub_recv, rsub_recv;  // [G][PA]
    DBuf lseg, rseg;       // device [G][PA+1]
    DBuf lgb, rgb;         // device [PA+1] group bases
    DBuf lpairs, rpairs;   // bucketed pairs
    DBuf loff, roff;       // int64[B+1]
    DBuf flags;            // u32[B]
    int F{0};
    int join_slots{2048};
    int64_t lrows{0}, rrows{0};
  };
  std::vector<Batch> batches(od);

  auto slice_of = [&](const std::vector<int64_t>& pofs, int b) {
    std::vector<cudf::size_type> sl(G + 1);
    for (int r = 0; r <= G; r++) sl[r] = (cudf::size_type)pofs[(size_t)(b * G + r) * PA];
    return sl;
  };
  auto subcounts_of = [&](const std::vector<int64_t>& pofs, int b) {
    std::vector<std::vector<int64_t>> sc(G, std::vector<int64_t>(PA));
    for (int r = 0; r < G; r++)
      for (int g = 0; g < PA; g++) {
        size_t base = (size_t)(b * G + r) * PA + g;
        sc[r][g] = pofs[base + 1] - pofs[base];
      }
    return sc;
  };

  /* pre-phase: exchanges + allocations */
  for (int b = 0; b < od; b++) {
    Batch& bt = batches[b];
    /* route tag 0: this path runs only on mask-free tables */
    bt.latoa = AllToAllCommunicatorAccess::make(lpart_view, slice_of(lposf, b), group,
                                                communicator, lopts, true, 0u);
    bt.ratoa = AllToAllCommunicatorAccess::make(rpart_view, slice_of(rposf, b), group,
                                                communicator, ropts, true, 0u);
    exchange_vecs(group, communicator, subcounts_of(lposf, b), bt.lsub_recv);
    exchange_vecs(group, communicator, subcounts_of(rposf, b), bt.rsub_recv);
    bt.lrecv = bt.latoa->allocate_communicated_table();
    bt.rrecv = bt.ratoa->allocate_communicated_table();
    bt.lrows = bt.lrecv->num_rows();
    bt.rrows = bt.rrecv->num_rows();
    /* seg bounds + group bases (host -> device) */
    auto build_segs = [&](const std::vector<std::vector<int64_t>>& sub,
                          const AllToAllCommunicator& atoa, DBuf& dseg, DBuf& dgb) {
      const auto& roff = AllToAllCommunicatorAccess::recv_offsets(atoa);
      std::vector<int64_t> seg((size_t)G * (PA + 1));
      std::vector<int64_t> gtot(PA + 1, 0);
      for (int r2 = 0; r2 < G; r2++) {
        int64_t acc = roff[r2];
        for (int g = 0; g <= PA; g++) {
          seg[(size_t)r2 * (PA + 1) + g] = acc;
          if (g < PA) acc += sub[r2][g];
        }
        for (int g = 0; g < PA; g++) gtot[g + 1] += sub[r2][g];
      }
      for (int g = 0; g < PA; g++) gtot[g + 1] += gtot[g];
      dseg = DBuf(seg.size() * 8);
      dgb = DBuf((size_t)(PA + 1) * 8);
      DJ_HIP_CALL(hipMemcpyAsync(dseg.p, seg.data(), seg.size() * 8, hipMemcpyHostToDevice,
                                 st));
      DJ_HIP_CALL(hipMemcpyAsync(dgb.p, gtot.data(), (size_t)(PA + 1) * 8,
                                 hipMemcpyHostToDevice, st));
    };
    build_segs(bt.lsub_recv, *bt.latoa, bt.lseg, bt.lgb);
    build_segs(bt.rsub_recv, *bt.ratoa, bt.rseg, bt.rgb);
    DJ_HIP_CALL(hipStreamSynchronize(st));
    /* sub-bucket fanout: target ~760 rows per final bucket. F caps at 1024
     * (the staged span's one-group-per-thread scan); when buckets then run
     * big (e.g. G=8 od=1: 100M over PA*F=65536 => ~1526 rows) the join
     * switches to its 4096-slot table instead of overflowing every bucket. */
    int64_t maxn = std::max(bt.lrows, bt.rrows);
    int F = 64;
    while (F < 1024 && (int64_t)PA * F * 760 < maxn) F <<= 1;
    bt.F = F;
    if (const char* ff = getenv("DJ_FORCE_FUSED_F")) {
      /* TEST HOOK (tests/test_gpu_cpp_api.py::test_fused_big_buckets): force
       * a small fan-out so the 4096-slot join path is exercisable on one
       * GPU without an 8-rank 100M-row workload */
      int v = atoi(ff);
      if (v >= 64 && v <= 1024 && (v & (v - 1)) == 0) F = bt.F = v;
    }
    bt.join_slots = (maxn / ((int64_t)PA * F) > 1300) ? 4096 : 2048;
    int64_t B = (int64_t)PA * F;
    bt.lpairs = DBuf((size_t)std::max<int64_t>(bt.lrows, 1) * 16);
    bt.rpairs = DBuf((size_t)std::max<int64_t>(bt.rrows, 1) * 16);
    bt.loff = DBuf((size_t)(B + 1) * 8);
    bt.roff = DBuf((size_t)(B + 1) * 8);
    bt.flags = DBuf((size_t)B * 4);
    bt.out = JoinOut(JoinOut::default_cap(bt.rrows));
  }

  /* pipeline: comm(b) then enqueue passB+join(b); comm(b+1) overlaps */
  for (int b = 0; b < od; b++) {
    Batch& bt = batches[b];
    bt.latoa->launch_communication(bt.lrecv->mutable_view(), report_timing, pinned);
    bt.ratoa->launch_communication(bt.rrecv->mutable_view(), report_timing, pinned);
    bt.out.clear(st);
    if (bt.lrows == 0 || bt.rrows == 0) continue;
    int64_t B = (int64_t)PA * bt.F;
    DJ_HIP_CALL(hipMemsetAsync(bt.flags.p, 0, (size_t)B * 4, st));
    {
      dj_timing::Scope t(DJ_PHASE_BUCKET_SCATTER, st);
      dj::subpart_lists((const int64_t*)bt.lrecv->get_column(0).head(),
                        (const int64_t*)bt.lrecv->get_column(1).head(), bt.lseg.i64(), G, PA,
                        bt.F, bt.lgb.i64(), (longlong2*)bt.lpairs.p, bt.loff.i64(), st);
      dj::subpart_lists((const int64_t*)bt.rrecv->get_column(0).head(),
                        (const int64_t*)bt.rrecv->get_column(1).head(), bt.rseg.i64(), G, PA,
                        bt.F, bt.rgb.i64(), (longlong2*)bt.rpairs.p, bt.roff.i64(), st);
    }
    {
      dj_timing::Scope t(DJ_PHASE_JOIN_FUSED, st);
      dj::lds_join((const longlong2*)bt.lpairs.p, bt.loff.i64(),
                   (const longlong2*)bt.rpairs.p, bt.roff.i64(), (int)B, bt.join_slots,
                   bt.out.o0.i64(), bt.out.o1.i64(), bt.out.o2.i64(), bt.out.o3.i64(),
                   bt.out.cap, bt.out.counter(), (uint32_t*)bt.flags.p, bt.out.any_overflow(),
                   bt.out.error(), st);
    }
  }
  DJ_HIP_CALL(hipStreamSynchronize(st));
  return finalize_batches(batches, 0, 0, false, communicator->mpi_rank);
}

/* ---- what distributed_inner_join and distributed_join share ---- */

void check_join_args(cudf::table_view left, cudf::table_view right,
                     std::vector<cudf::size_type> const& left_on,
                     std::vector<cudf::size_type> const& right_on,
                     std::vector<ColumnCompressionOptions> const& left_compression_options,
                     std::vector<ColumnCompressionOptions> const& right_compression_options)
{
  DJ_CHECK_ERROR(left_on.size() == right_on.size() && !left_on.empty(),
                 "left_on/right_on must name the same number of key columns");
  DJ_CHECK_ERROR(left_on.size() <= 4, "up to 4 join key columns supported");
  validate_compression(left, left_compression_options);
  validate_compression(right, right_compression_options);
  check_key_pairs(left, right, left_on, right_on);
}

/* replicates the reference's divisor search exactly
 * (distributed_join.cpp:55-69, including its sqrt starting point) */
int get_nvl_partition_size(int mpi_size, int nvlink_domain_size)
{
  if (nvlink_domain_size >= mpi_size) return mpi_size;
  for (int size = (int)ceil(sqrt((double)mpi_size)); size > 0; size--)
    if (mpi_size % size == 0 && size <= nvlink_domain_size) return size;
  return 1;
}

/* 2-level hierarchy (distributed_join.cpp:152-199): when the join group is
 * smaller than the world, first shuffle both tables across domains (the
 * reference's InfiniBand stage, seed 87654321); the join then runs within
 * each domain (seed 12345678). On one xGMI node nvlink_domain_size >= world
 * collapses this to the flat path. `left` and `right` come back as views of
 * the shuffled tables, which the stage owns; nvl is the join-group size. */
struct InterDomainStage {
  int nvl;
  std::unique_ptr<cudf::table> l_ib, r_ib;
};

InterDomainStage inter_domain_stage(
  cudf::table_view& left, cudf::table_view& right, std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on, Communicator* communicator,
  std::vector<ColumnCompressionOptions> const& left_compression_options,
  std::vector<ColumnCompressionOptions> const& right_compression_options, bool report_timing,
  void* preallocated_pinned_buffer, int nvlink_domain_size)
{
  InterDomainStage s;
  const int world = communicator->mpi_size;
  s.nvl = get_nvl_partition_size(world, nvlink_domain_size < 1 ? 1 : nvlink_domain_size);
  if (s.nvl != world) {
    CommunicationGroup inter(world, s.nvl, communicator->mpi_rank);
    s.l_ib = shuffle_on(left, left_on, inter, communicator, left_compression_options,
                        cudf::hash_id::HASH_MURMUR3, DJ_SEED_INTER, report_timing,
                        preallocated_pinned_buffer);
    s.r_ib = shuffle_on(right, right_on, inter, communicator, right_compression_options,
                        cudf::hash_id::HASH_MURMUR3, DJ_SEED_INTER, report_timing,
                        preallocated_pinned_buffer);
    left = s.l_ib->view();
    right = s.r_ib->view();
  }
  return s;
}

/* shuffle both tables within the join group (seed 12345678, placement on the
 * fused key chain for composite, STRING and nullable keys), then join
 * locally: after the shuffle every right row that could match a left row
 * sits on that row's rank, so matched / unmatched is decided locally;
 * collisions are filtered in the local join. over_decom_factor has no effect
 * on this route. */
std::unique_ptr<cudf::table> shuffle_then_local_join(
  join_kind kind, cudf::table_view left, cudf::table_view right,
  std::vector<cudf::size_type> const& left_on, std::vector<cudf::size_type> const& right_on,
  int nvl, Communicator* communicator,
  std::vector<ColumnCompressionOptions> const& left_compression_options,
  std::vector<ColumnCompressionOptions> const& right_compression_options, bool report_timing,
  void* preallocated_pinned_buffer, uint32_t route_tag, cudf::null_equality compare_nulls)
{
  CommunicationGroup g2(nvl, 1, communicator->mpi_rank);
  auto ls = shuffle_on_tagged(left, left_on, g2, communicator, left_compression_options,
                              cudf::hash_id::HASH_MURMUR3, DJ_SEED_INTRA, report_timing,
                              preallocated_pinned_buffer, route_tag);
  auto rs = shuffle_on_tagged(right, right_on, g2, communicator, right_compression_options,
                              cudf::hash_id::HASH_MURMUR3, DJ_SEED_INTRA, report_timing,
                              preallocated_pinned_buffer, route_tag);
  return local_join(kind, ls->view(), rs->view(), left_on, right_on, compare_nulls);
}

}  // namespace

/* --------------------------------------------------- distributed_inner_join */

std::unique_ptr<cudf::table> distributed_inner_join(
  cudf::table_view left,
  cudf::table_view right,
  std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on,
  Communicator* communicator,
  std::vector<ColumnCompressionOptions> left_compression_options,
  std::vector<ColumnCompressionOptions> right_compression_options,
  int over_decom_factor,
  bool report_timing,
  void* preallocated_pinned_buffer,
  int nvlink_domain_size)
{
  check_join_args(left, right, left_on, right_on, left_compression_options,
                  right_compression_options);
  const InterDomainStage stage = inter_domain_stage(
    left, right, left_on, right_on, communicator, left_compression_options,
    right_compression_options, report_timing, preallocated_pinned_buffer, nvlink_domain_size);
  const int nvl = stage.nvl;
  if (nvl == 1) return local_join(join_kind::INNER, left, right, left_on, right_on);

  /* composite keys, any STRING key and any nullable key join on the fused
   * key chain; nullability is read after the inter-domain shuffle, which
   * gives a column a mask when it had one on any rank of that group */
  const uint32_t route_tag = join_route_tag(left, right, left_on, right_on);
  const bool fused_keys = left_on.size() > 1 || any_string_key(left, left_on) ||
                          any_string_key(right, right_on) || (route_tag & 1u);

  /* multi-column keys, and STRING keys even alone, take the shuffle +
   * local-join route; the batched od pipeline stays single-integer-key —
   * the hot shape the reference benchmarks */
  if (fused_keys)
    return shuffle_then_local_join(join_kind::INNER, left, right, left_on, right_on, nvl,
                                   communicator, left_compression_options,
                                   right_compression_options, report_timing,
                                   preallocated_pinned_buffer, route_tag,
                                   cudf::null_equality::EQUAL);

  const int G = nvl;
  CommunicationGroup group(nvl, 1, communicator->mpi_rank);
  const int nparts = G * over_decom_factor;
  DJ_CHECK_ERROR(nparts <= dj::kMaxPartitions,
                 "join-group size x over_decom_factor must be <= 1024");

  /* fused wire path for the hot shape (2 x INT64 columns, key at 0):
   * partitions carry the bucket grouping on the wire, removing the separate
   * stable rank partition and bucket pass A */
  const cudf::size_type left_key = left_on[0], right_key = right_on[0];
  const bool fast2 = joins_i64_pairs(left, right, left_key, right_key);
  if (fast2) {
    int pa = 1;
    while (pa * 2 * nparts <= 1024) pa *= 2;
    if (pa >= 4)
      return distributed_inner_join_fused(left, right, communicator, group,
                                          left_compression_options, right_compression_options,
                                          over_decom_factor, pa, report_timing,
                                          preallocated_pinned_buffer);
  }

  /* report_timing mirrors the reference's per-phase prints
   * (distributed_join.cpp:120-130, 235-240) */
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](auto a, auto b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
  };
  auto t_part0 = now();

  /* rank-level stable partition, seed 12345678 (distributed_join.cpp:211-226) */
  PartitionedTable lpart =
    partition_table(left, left_key, nparts, DJ_HASH_MURMUR3, DJ_SEED_INTRA);
  PartitionedTable rpart =
    partition_table(right, right_key, nparts, DJ_HASH_MURMUR3, DJ_SEED_INTRA);
  if (report_timing)
    std::cout << "Rank " << communicator->mpi_rank << ": hash partition takes "
              << ms(t_part0, now()) << "ms" << std::endl;

  /* --- pre-phase: size exchanges + every allocation (pool allocs sync the
   * compute stream, so none happen inside the pipeline) --- */
  struct Batch : BatchJoin {
    DBuf lkw, rkw;  // widened keys, where the key column is narrower than 64 bits
    int64_t ln{0}, rn{0};
  };
  std::vector<Batch> batches(over_decom_factor);
  int64_t max_ln = 1, max_rn = 1;
  for (int b = 0; b < over_decom_factor; b++) {
    Batch& bt = batches[b];
    std::vector<cudf::size_type> lslice(lpart.offsets.begin() + b * G,
                                        lpart.offsets.begin() + b * G + G + 1);
    std::vector<cudf::size_type> rslice(rpart.offsets.begin() + b * G,
                                        rpart.offsets.begin() + b * G + G + 1);
    bt.latoa = AllToAllCommunicatorAccess::make(lpart.tbl->view(), lslice, group, communicator,
                                                left_compression_options, true, route_tag);
    bt.ratoa = AllToAllCommunicatorAccess::make(rpart.tbl->view(), rslice, group, communicator,
                                                right_compression_options, true, route_tag);
    bt.lrecv = bt.latoa->allocate_communicated_table();
    bt.rrecv = bt.ratoa->allocate_communicated_table();
    bt.ln = bt.lrecv->num_rows();
    bt.rn = bt.rrecv->num_rows();
    max_ln = std::max(max_ln, bt.ln);
    max_rn = std::max(max_rn, bt.rn);
    bt.out = JoinOut(JoinOut::default_cap(bt.rn));
    if (bt.ln && cudf::size_of(left.column(left_key).type()) < 8)
      bt.lkw = DBuf((size_t)bt.ln * 8);
    if (bt.rn && cudf::size_of(right.column(right_key).type()) < 8)
      bt.rkw = DBuf((size_t)bt.rn * 8);
  }
  DBuf scratch((size_t)dj_bucket_join_scratch_bytes(max_ln, max_rn));
  hipStream_t st = dj_rt_stream();

  /* --- pipeline: comm of batch b on the comm stream overlaps the join of
   * batch b-1 on the compute stream (the host blocks only in
   * launch_communication's stop; join kernels are enqueued without syncs) —
   * replaces the reference's join thread + atomic-flag busy wait
   * (distributed_join.cpp:283-329) with stream ordering --- */
  auto t_pipe0 = now();
  for (int b = 0; b < over_decom_factor; b++) {
    Batch& bt = batches[b];
    auto t_comm0 = now();
    bt.latoa->launch_communication(bt.lrecv->mutable_view(), report_timing,
                                   preallocated_pinned_buffer);
    bt.ratoa->launch_communication(bt.rrecv->mutable_view(), report_timing,
                                   preallocated_pinned_buffer);
    if (report_timing)
      std::cout << "Rank " << communicator->mpi_rank << ": all-to-all communication (batch "
                << b << ") takes " << ms(t_comm0, now()) << "ms" << std::endl;
    bt.out.clear(st);
    if (bt.ln == 0 || bt.rn == 0) continue;
    const cudf::table_view l = bt.lrecv->view(), r = bt.rrecv->view();
    /* narrow keys widen into the buffers of the pre-phase; int64 pairs carry
     * their payloads through the join, every other shape the row index,
     * which the partition kernels synthesize (pay == nullptr) */
    const int64_t* lk = key_as_i64(l.column(left_key), bt.lkw.i64(), st);
    const int64_t* rk = key_as_i64(r.column(right_key), bt.rkw.i64(), st);
    const int64_t* lp = fast2 ? l.column(1).head<int64_t>() : nullptr;
    const int64_t* rp = fast2 ? r.column(1).head<int64_t>() : nullptr;
    dj_bucket_local_join_enqueue(lk, lp, bt.ln, rk, rp, bt.rn, bt.out.o0.i64(),
                                 bt.out.o1.i64(), bt.out.o2.i64(), bt.out.o3.i64(), bt.out.cap,
                                 bt.out.counter(), bt.out.error(), bt.out.any_overflow(),
                                 scratch.p);
  }
  DJ_HIP_CALL(hipStreamSynchronize(st));
  if (report_timing)
    std::cout << "Rank " << communicator->mpi_rank
              << ": communication + local join pipeline takes " << ms(t_pipe0, now()) << "ms"
              << std::endl;

  return finalize_batches(batches, left_key, right_key, report_timing, communicator->mpi_rank);
}

/* ------------------------------------------- left / left semi / left anti */

std::unique_ptr<cudf::table> distributed_join(
  join_kind kind,
  cudf::table_view left,
  cudf::table_view right,
  std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on,
  Communicator* communicator,
  std::vector<ColumnCompressionOptions> left_compression_options,
  std::vector<ColumnCompressionOptions> right_compression_options,
  int over_decom_factor,
  bool report_timing,
  void* preallocated_pinned_buffer,
  int nvlink_domain_size,
  cudf::null_equality compare_nulls)
{
  const bool sql = compare_nulls == cudf::null_equality::UNEQUAL;
  if (kind == join_kind::INNER && !sql)
    return distributed_inner_join(left, right, left_on, right_on, communicator,
                                  std::move(left_compression_options),
                                  std::move(right_compression_options), over_decom_factor,
                                  report_timing, preallocated_pinned_buffer, nvlink_domain_size);
  DJ_CHECK_ERROR(kind == join_kind::INNER || kind == join_kind::LEFT ||
                   kind == join_kind::LEFT_SEMI || kind == join_kind::LEFT_ANTI,
                 "distributed_join: unknown join kind");
  check_join_args(left, right, left_on, right_on, left_compression_options,
                  right_compression_options);

  /* a semi / anti join asks of the right table only whether a key exists:
   * its other columns stay home, before any stage that communicates */
  std::vector<cudf::size_type> ron = right_on;
  if (kind == join_kind::LEFT_SEMI || kind == join_kind::LEFT_ANTI) {
    std::vector<cudf::column_view> key_cols;
    std::vector<ColumnCompressionOptions> key_opts;
    for (size_t k = 0; k < right_on.size(); k++) {
      key_cols.push_back(right.column(right_on[k]));
      if ((size_t)right_on[k] < right_compression_options.size())
        key_opts.push_back(right_compression_options[(size_t)right_on[k]]);
      ron[k] = (cudf::size_type)k;
    }
    if (key_opts.size() != key_cols.size()) key_opts.clear();
    right = cudf::table_view(std::move(key_cols));
    right_compression_options = std::move(key_opts);
  }

  /* one rank: the local join keeps the null-key rows out of the engine
   * itself, without compacting a column */
  if (communicator->mpi_size == 1)
    return local_join(kind, left, right, left_on, ron, compare_nulls);

  /* null_equality::UNEQUAL over several ranks: null-key rows never reach the
   * communicator. Each rank strips its tables to their valid-key rows before
   * the first stage that communicates (a local step that leaves the schema,
   * mask presence included, as it is, so the route and its tag are those of
   * the EQUAL join of the stripped tables) and, for LEFT and LEFT_ANTI,
   * appends its own null-key left rows to its result. */
  if (sql) {
    const bool keep = kind == join_kind::LEFT || kind == join_kind::LEFT_ANTI;
    StrippedTable l =
      strip_null_keys(left, left_on, keep, kind == join_kind::LEFT ? &right : nullptr);
    StrippedTable r = strip_null_keys(right, ron, false, nullptr);
    if (l.valid) left = l.valid->view();
    if (r.valid) right = r.valid->view();
    auto joined =
      distributed_join(kind, left, right, left_on, ron, communicator, left_compression_options,
                       right_compression_options, over_decom_factor, report_timing,
                       preallocated_pinned_buffer, nvlink_domain_size);
    if (!l.null_rows) return joined;
    std::vector<std::unique_ptr<cudf::table>> parts;
    parts.push_back(std::move(joined));
    parts.push_back(std::move(l.null_rows));
    return concat_tables(parts);
  }

  /* the same inter-domain stage as the inner join's */
  const InterDomainStage stage = inter_domain_stage(
    left, right, left_on, ron, communicator, left_compression_options,
    right_compression_options, report_timing, preallocated_pinned_buffer, nvlink_domain_size);
  if (stage.nvl == 1) return local_join(kind, left, right, left_on, ron);

  /* shuffle + local join, the route composite and nullable keys take in the
   * inner join. Every rank takes this route whatever its masks, so there is
   * no route to disagree on (tag 0). */
  return shuffle_then_local_join(kind, left, right, left_on, ron, stage.nvl, communicator,
                                 left_compression_options, right_compression_options,
                                 report_timing, preallocated_pinned_buffer, 0u,
                                 cudf::null_equality::EQUAL);
}

std::unique_ptr<cudf::table> distributed_left_join(
  cudf::table_view left, cudf::table_view right, std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on, Communicator* communicator,
  std::vector<ColumnCompressionOptions> left_compression_options,
  std::vector<ColumnCompressionOptions> right_compression_options, int over_decom_factor,
  bool report_timing, void* preallocated_pinned_buffer, int nvlink_domain_size,
  cudf::null_equality compare_nulls)
{
  return distributed_join(join_kind::LEFT, left, right, left_on, right_on, communicator,
                          std::move(left_compression_options),
                          std::move(right_compression_options), over_decom_factor,
                          report_timing, preallocated_pinned_buffer, nvlink_domain_size,
                          compare_nulls);
}

std::unique_ptr<cudf::table> distributed_left_semi_join(
  cudf::table_view left, cudf::table_view right, std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on, Communicator* communicator,
  std::vector<ColumnCompressionOptions> left_compression_options,
  std::vector<ColumnCompressionOptions> right_compression_options, int over_decom_factor,
  bool report_timing, void* preallocated_pinned_buffer, int nvlink_domain_size,
  cudf::null_equality compare_nulls)
{
  return distributed_join(join_kind::LEFT_SEMI, left, right, left_on, right_on, communicator,
                          std::move(left_compression_options),
                          std::move(right_compression_options), over_decom_factor,
                          report_timing, preallocated_pinned_buffer, nvlink_domain_size,
                          compare_nulls);
}

std::unique_ptr<cudf::table> distributed_left_anti_join(
  cudf::table_view left, cudf::table_view right, std::vector<cudf::size_type> const& left_on,
  std::vector<cudf::size_type> const& right_on, Communicator* communicator,
  std::vector<ColumnCompressionOptions> left_compression_options,
  std::vector<ColumnCompressionOptions> right_compression_options, int over_decom_factor,
  bool report_timing, void* preallocated_pinned_buffer, int nvlink_domain_size,
  cudf::null_equality compare_nulls)
{
  return distributed_join(join_kind::LEFT_ANTI, left, right, left_on, right_on, communicator,
                          std::move(left_compression_options),
                          std::move(right_compression_options), over_decom_factor,
                          report_timing, preallocated_pinned_buffer, nvlink_domain_size,
                          compare_nulls);
}

/* ------------------------------------------------------------- shuffle_on */

std::unique_ptr<cudf::table> shuffle_on(cudf::table_view const& input,
                                        std::vector<cudf::size_type> const& on_columns,
                                        CommunicationGroup comm_group,
                                        Communicator* communicator,
                                        std::vector<ColumnCompressionOptions> compression_options,
                                        cudf::hash_id hash_function,
                                        uint32_t hash_seed,
                                        bool report_timing,
                                        void* preallocated_pinned_buffer)
{
  return shuffle_on_tagged(input, on_columns, comm_group, communicator,
                           std::move(compression_options), hash_function, hash_seed,
                           report_timing, preallocated_pinned_buffer, 0u);
}

std::unique_ptr<cudf::table> shuffle_on(cudf::table_view const& input,
                                        std::vector<cudf::size_type> const& on_columns,
                                        Communicator* communicator,
                                        std::vector<ColumnCompressionOptions> compression_options,
                                        cudf::hash_id hash_function,
                                        uint32_t hash_seed,
                                        bool report_timing,
                                        void* preallocated_pinned_buffer)
{
  return shuffle_on(input, on_columns,
                    CommunicationGroup(communicator->mpi_size, 1, communicator->mpi_rank),
                    communicator, std::move(compression_options), hash_function, hash_seed,
                    report_timing, preallocated_pinned_buffer);
}

/* --------------------------------------------------------- distribute_table */

using dj::kMaxSchemaCols;

std::unique_ptr<cudf::table> distribute_table(cudf::table_view global_table,
                                              Communicator* communicator)
{
  const int G = communicator->mpi_size;
  const int rank = communicator->mpi_rank;
  hipStream_t st = dj_rt_stream();
  check_no_masks(global_table, "distribute_table");

  /* schema + per-rank row counts: root sends [nrows_r, ncols, dtype ids...] */
  std::vector<int64_t> header(2 + kMaxSchemaCols, 0);
  if (rank == 0) {
    DJ_CHECK_ERROR(global_table.num_columns() <= kMaxSchemaCols, "too many columns");
    header[1] = global_table.num_columns();
    for (cudf::size_type c = 0; c < global_table.num_columns(); c++)
      header[2 + c] = (int64_t)global_table.column(c).type().id();
  }
  int64_t total = rank == 0 ? global_table.num_rows() : 0;
  DBuf d_hdr((size_t)header.size() * 8 * (rank == 0 ? G : 1));
  if (G > 1) {
    if (rank == 0) {
      std::vector<int64_t> all;
      for (int r = 0; r < G; r++) {
        int64_t rows_r = total / G + (r < total % G ? 1 : 0);
        header[0] = rows_r;
        all.insert(all.end(), header.begin(), header.end());
      }
      DJ_HIP_CALL(hipMemcpyAsync(d_hdr.p, all.data(), all.size() * 8, hipMemcpyHostToDevice, st));
      DJ_HIP_CALL(hipStreamSynchronize(st));
    }
    communicator->start();
    if (rank == 0) {
      for (int r = 1; r < G; r++)
        communicator->send(d_hdr.i64() + (size_t)r * header.size(), header.size(), 8, r);
    } else {
      communicator->recv(d_hdr.i64(), header.size(), 8, 0);
    }
    communicator->stop();
    if (rank != 0) {
      DJ_HIP_CALL(hipMemcpyAsync(header.data(), d_hdr.p, header.size() * 8,
                                 hipMemcpyDeviceToHost, st));
      DJ_HIP_CALL(hipStreamSynchronize(st));
    } else {
      header[0] = total / G + (0 < total % G ? 1 : 0);
    }
  } else {
    header[0] = total;
  }

  const int64_t my_rows = header[0];
  const int ncols = (int)header[1];
  std::vector<std::unique_ptr<cudf::column>> cols;
  for (int c = 0; c < ncols; c++)
    cols.push_back(std::make_unique<cudf::column>(
      cudf::data_type((cudf::type_id)header[2 + c]), (cudf::size_type)my_rows));
  auto local = std::make_unique<cudf::table>(std::move(cols));

  /* row data: root sends each rank its contiguous slice */
  communicator->start();
  if (rank == 0) {
    int64_t row0 = 0;
    for (int r = 0; r < G; r++) {
      int64_t rows_r = total / G + (r < total % G ? 1 : 0);
      for (int c = 0; c < ncols; c++) {
        const int esize = cudf::size_of(global_table.column(c).type());
        const int8_t* src = global_table.column(c).head<int8_t>() + row0 * esize;
        if (r == 0) {
          DJ_HIP_CALL(hipMemcpyAsync(local->get_column(c).head(), src, (size_t)rows_r * esize,
                                     hipMemcpyDeviceToDevice, dj_rt_comm_stream()));
        } else {
          communicator->send(src, rows_r, esize, r);
        }
      }
      row0 += rows_r;
    }
  } else {
    for (int c = 0; c < ncols; c++) {
      const int esize = cudf::size_of(local->get_column(c).type());
      communicator->recv(local->get_column(c).head(), my_rows, esize, 0);
    }
  }
  communicator->stop();
  return local;
}

std::unique_ptr<cudf::table> collect_tables(cudf::table_view table, Communicator* communicator)
{
  const int G = communicator->mpi_size;
  const int rank = communicator->mpi_rank;
  CommunicationGroup group(G, 1, rank);
  check_no_masks(table, "collect_tables");

  /* per-rank row counts to root via communicate_sizes (send all rows to
   * local rank 0) */
  std::vector<int64_t> send_offset(G + 1, (int64_t)table.num_rows());
  send_offset[0] = 0;
  std::vector<int64_t> recv_offset;
  communicate_sizes(send_offset, recv_offset, group, communicator);

  std::unique_ptr<cudf::table> merged;
  if (rank == 0) {
    std::vector<std::unique_ptr<cudf::column>> cols;
    for (cudf::size_type c = 0; c < table.num_columns(); c++)
      cols.push_back(std::make_unique<cudf::column>(table.column(c).type(),
                                                    (cudf::size_type)recv_offset.back()));
    merged = std::make_unique<cudf::table>(std::move(cols));
  }

  communicator->start();
  for (cudf::size_type c = 0; c < table.num_columns(); c++) {
    const int esize = cudf::size_of(table.column(c).type());
    if (rank == 0) {
      for (int r = 0; r < G; r++) {
        int64_t count = recv_offset[r + 1] - recv_offset[r];
        int8_t* dst = (int8_t*)merged->get_column(c).head() + recv_offset[r] * esize;
        if (r == 0) {
          DJ_HIP_CALL(hipMemcpyAsync(dst, table.column(c).head<int8_t>(),
                                     (size_t)count * esize, hipMemcpyDeviceToDevice,
                                     dj_rt_comm_stream()));
        } else {
          communicator->recv(dst, count, esize, r);
        }
      }
    } else {
      communicator->send(table.column(c).head<int8_t>(), table.num_rows(), esize, 0);
    }
  }
  communicator->stop();
  return merged;  // nullptr on non-root ranks
}
