/*
 * dj_all_to_all.hip — include/all_to_all_comm.hpp: CommunicationGroup, the
 * size exchange, the generic plan API and AllToAllCommunicator with its
 * exchange (plain, cascaded-compressed and validity-mask wires).
 */
#include "dj_host.hpp"

#include <iostream>

using namespace dj_host;

/* ------------------------------------------------------ CommunicationGroup */

CommunicationGroup::CommunicationGroup(int grid_size, int stride)
  : CommunicationGroup(grid_size, stride, default_communicator()->mpi_rank)
{
}

CommunicationGroup::CommunicationGroup(int grid_size_, int stride_, int mpi_rank_)
  : mpi_rank(mpi_rank_), grid_size(grid_size_), stride(stride_)
{
  DJ_CHECK_ERROR(stride > 0 && grid_size % stride == 0,
                 "Group size should be a multiple of stride");
  group_start = mpi_rank / grid_size * grid_size + mpi_rank % stride;
}

/* ------------------------------------------------------- communicate_sizes */

/* communicate_sizes, optionally carrying `extra` (33 bits) above bit 30 of
 * every count: the internal exchange of AllToAllCommunicator, whose counts
 * are size_type rows, agrees on column nullability this way without a
 * message of its own. peer_extra (G entries) receives every rank's word. */
static void exchange_sizes(std::vector<int64_t> const& send_offset,
                           std::vector<int64_t>& recv_offset, CommunicationGroup comm_group,
                           Communicator* communicator, bool fold, uint64_t extra,
                           std::vector<uint64_t>* peer_extra)
{
  const int G = comm_group.size();
  const int me = comm_group.get_local_idx();
  std::vector<int64_t> send_counts(G);
  for (int i = 0; i < G; i++) {
    send_counts[i] = send_offset[i + 1] - send_offset[i];
    if (fold) {
      DJ_CHECK_ERROR(send_counts[i] >= 0 && send_counts[i] <= (int64_t)INT32_MAX,
                     "all-to-all: a slice's row count exceeds size_type");
      if (i != me) send_counts[i] |= (int64_t)(extra << 31);
    }
  }
  std::vector<int64_t> recv_counts(G, 0);
  recv_counts[me] = send_counts[me];
  if (peer_extra) {
    peer_extra->assign(G, 0);
    (*peer_extra)[me] = extra;
  }
  if (G > 1) {
    /* counts move through the communicator via a small device staging
     * buffer (the reference kept them on MPI host buffers,
     * all_to_all_comm.cpp:68-69; RCCL wants device memory) */
    DBuf d_send((size_t)G * 8), d_recv((size_t)G * 8);
    DJ_HIP_CALL(hipMemcpyAsync(d_send.p, send_counts.data(), (size_t)G * 8,
                               hipMemcpyHostToDevice, dj_rt_comm_stream()));
    DJ_HIP_CALL(hipStreamSynchronize(dj_rt_comm_stream()));
    communicator->start();
    for (int i = 0; i < G; i++) {
      if (i == me) continue;
      int peer = comm_group.get_global_rank(i);
      communicator->send(d_send.i64() + i, 1, 8, peer);
      communicator->recv(d_recv.i64() + i, 1, 8, peer);
    }
    communicator->stop();
    std::vector<int64_t> got(G);
    DJ_HIP_CALL(hipMemcpyAsync(got.data(), d_recv.p, (size_t)G * 8, hipMemcpyDeviceToHost,
                               dj_rt_comm_stream()));
    DJ_HIP_CALL(hipStreamSynchronize(dj_rt_comm_stream()));
    for (int i = 0; i < G; i++) {
      if (i == me) continue;
      recv_counts[i] = fold ? (got[i] & (int64_t)0x7FFFFFFF) : got[i];
      if (fold && peer_extra) (*peer_extra)[i] = (uint64_t)got[i] >> 31;
    }
  }
  recv_offset.resize(G + 1);
  recv_offset[0] = 0;
  for (int i = 0; i < G; i++) recv_offset[i + 1] = recv_offset[i] + recv_counts[i];
}

void communicate_sizes(std::vector<int64_t> const& send_offset,
                       std::vector<int64_t>& recv_offset,
                       CommunicationGroup comm_group,
                       Communicator* communicator)
{
  exchange_sizes(send_offset, recv_offset, comm_group, communicator, false, 0, nullptr);
}

void communicate_sizes(std::vector<cudf::size_type> const& send_offset,
                       std::vector<int64_t>& recv_offset,
                       CommunicationGroup comm_group,
                       Communicator* communicator)
{
  std::vector<int64_t> wide(send_offset.begin(), send_offset.end());
  communicate_sizes(wide, recv_offset, comm_group, communicator);
}

void warmup_all_to_all(Communicator* communicator)
{
  /* mirrors all_to_all_comm.cpp:191-233: a throwaway all-to-all to
   * establish RCCL channels before the timed region */
  const int G = communicator->mpi_size;
  if (G <= 1) return;
  const int64_t per_peer = 1 << 18;
  DBuf d_send((size_t)G * per_peer * 8), d_recv((size_t)G * per_peer * 8);
  communicator->start();
  for (int p = 0; p < G; p++) {
    if (p == communicator->mpi_rank) continue;
    communicator->send(d_send.i64() + p * per_peer, per_peer, 8, p);
    communicator->recv(d_recv.i64() + p * per_peer, per_peer, 8, p);
  }
  communicator->stop();
}

/* --------------------------------------------------------- all_to_all plan */

void append_to_all_to_all_comm_buffers(cudf::table_view input,
                                       cudf::mutable_table_view output,
                                       std::vector<cudf::size_type> const& send_offsets,
                                       std::vector<int64_t> const& recv_offsets,
                                       std::vector<AllToAllCommBuffer>& all_to_all_comm_buffers,
                                       std::vector<ColumnCompressionOptions> compression_options)
{
  check_no_compression(compression_options);
  check_no_masks(input, "append_to_all_to_all_comm_buffers");
  for (cudf::size_type c = 0; c < input.num_columns(); c++) {
    DJ_CHECK_ERROR(cudf::size_of(input.column(c).type()) > 0,
                   "all-to-all: fixed-width columns only through the generic plan API");
    std::vector<int64_t> soff(send_offsets.begin(), send_offsets.end());
    all_to_all_comm_buffers.emplace_back(
      input.column(c).head<int8_t>(), output.column(c).head<int8_t>(), soff, recv_offsets,
      input.column(c).type(), compression_options[c].compression_method,
      compression_options[c].cascaded_format);
  }
}

void all_to_all_comm(std::vector<AllToAllCommBuffer>& all_to_all_comm_buffers,
                     CommunicationGroup comm_group,
                     Communicator* communicator,
                     bool include_current_rank,
                     bool report_timing,
                     void* preallocated_pinned_buffer)
{
  (void)report_timing;
  (void)preallocated_pinned_buffer;
  const int G = comm_group.size();
  const int me = comm_group.get_local_idx();
  for (auto& buf : all_to_all_comm_buffers) {
    const int esize = cudf::size_of(buf.dtype);
    for (int i = 0; i < G; i++) {
      int64_t scount = buf.send_offsets[i + 1] - buf.send_offsets[i];
      int64_t rcount = buf.recv_offsets[i + 1] - buf.recv_offsets[i];
      const int8_t* src = (const int8_t*)buf.send_buffer + buf.send_offsets[i] * esize;
      int8_t* dst = (int8_t*)buf.recv_buffer + buf.recv_offsets[i] * esize;
      if (i == me) {
        if (include_current_rank && scount > 0) {
          /* self-partition: direct D2D on the comm stream (the reference's
           * explicit copy, all_to_all_comm.cpp:610-653) */
          DJ_HIP_CALL(hipMemcpyAsync(dst, src, (size_t)scount * esize,
                                     hipMemcpyDeviceToDevice, dj_rt_comm_stream()));
        }
        continue;
      }
      int peer = comm_group.get_global_rank(i);
      communicator->send(src, scount, esize, peer);
      communicator->recv(dst, rcount, esize, peer);
    }
  }
}

void postprocess_all_to_all_comm(std::vector<AllToAllCommBuffer>& all_to_all_comm_buffers,
                                 CommunicationGroup comm_group,
                                 Communicator* communicator,
                                 bool include_current_rank,
                                 bool report_timing)
{
  /* nothing to do: the generic plan path transfers raw buffers only
   * (cascaded refused at append — see check_no_compression); string
   * columns and compressed wires run through launch_communication, which
   * does its own receiver-side decompress + offsets rebuild */
  (void)all_to_all_comm_buffers;
  (void)comm_group;
  (void)communicator;
  (void)include_current_rank;
  (void)report_timing;
}

/* ---------------------------------------------------- AllToAllCommunicator */

namespace {

/* per string column: char-offset boundaries per peer + device row-size
 * buffers (reference all_to_all_comm.hpp:349-360 members; sizes, not
 * offsets, go on the wire — offsets rebuilt receiver-side by scan,
 * strings_column.cu:111-131) */
struct StringWires {
  std::vector<std::vector<int64_t>> send_char_offsets;  // [col][G+1]
  std::vector<std::vector<int64_t>> recv_char_offsets;  // [col][G+1]
  std::vector<DBuf> sizes_to_send;                      // [col] int32[n]
  std::vector<DBuf> sizes_received;                     // [col] int32[n_recv]
};

}  // namespace

struct AllToAllCommunicator::StringsState : StringWires {};

AllToAllCommunicator::AllToAllCommunicator(
  cudf::table_view input_table_,
  std::vector<cudf::size_type> offsets,
  CommunicationGroup comm_group_,
  Communicator* communicator_,
  std::vector<ColumnCompressionOptions> compression_options_,
  bool explicit_copy_to_current_rank_)
  : AllToAllCommunicator(input_table_, std::move(offsets), comm_group_, communicator_,
                         std::move(compression_options_), explicit_copy_to_current_rank_, 0u)
{
}

AllToAllCommunicator::AllToAllCommunicator(
  cudf::table_view input_table_,
  std::vector<cudf::size_type> offsets,
  CommunicationGroup comm_group_,
  Communicator* communicator_,
  std::vector<ColumnCompressionOptions> compression_options_,
  bool explicit_copy_to_current_rank_,
  uint32_t route_tag)
  : input_table(input_table_),
    comm_group(comm_group_),
    communicator(communicator_),
    explicit_copy_to_current_rank(explicit_copy_to_current_rank_),
    send_offsets(std::move(offsets)),
    compression_options(std::move(compression_options_))
{
  validate_compression(input_table, compression_options);
  DJ_CHECK_ERROR((int)send_offsets.size() == comm_group.size() + 1,
                 "AllToAllCommunicator: offsets must have comm_group.size()+1 entries");
  /* row counts, with this rank's per-column nullability (and the caller's
   * route tag) folded above them: the ranks must agree on which columns ship
   * a mask, or the slice sizes of the exchange would not pair up. A column
   * is shipped with a mask when it has one on ANY rank of the group; a rank
   * whose column has none sends all-valid slices. */
  {
    const int ncols = input_table.num_columns();
    DJ_CHECK_ERROR(!any_nullable(input_table) || ncols <= dj::kMaxSchemaCols,
                   "all-to-all: nullable columns need a table of at most 32 columns");
    const uint32_t my_bits = nullable_bits(input_table);
    DJ_CHECK_ERROR(!(route_tag & 2u) || ncols < 32, "all-to-all: route tag needs a free bit");
    const uint64_t extra = (uint64_t)(route_tag & 1u) | ((uint64_t)my_bits << 1) |
                           ((uint64_t)((route_tag >> 1) & 1u) << 32);
    std::vector<int64_t> wide(send_offsets.begin(), send_offsets.end());
    std::vector<uint64_t> peers;
    exchange_sizes(wide, recv_offsets, comm_group, communicator, true, extra, &peers);
    const uint32_t col_bits = ncols >= 32 ? 0xFFFFFFFFu : ((1u << ncols) - 1u);
    for (uint64_t e : peers) {
      nullable_cols |= (uint32_t)(e >> 1) & col_bits;
      const uint32_t tag = (uint32_t)(e & 1u) | (ncols < 32 ? (uint32_t)((e >> 32) & 1u) << 1 : 0u);
      DJ_CHECK_ERROR(tag == route_tag,
                     "all-to-all: the ranks of the group passed different route tags. In "
                     "distributed_inner_join this means they disagree on whether a key column "
                     "(or a column of a 2 x INT64 table) is nullable, which selects the join "
                     "route; pass a mask (all valid) for that column on every rank");
    }
  }

  /* strings columns: exchange per-peer char byte counts; precompute the row
   * sizes to send (gather_string_offsets + calculate_string_sizes_from_offsets
   * roles, strings_column.cu:39-109) */
  const int G = comm_group.size();
  const int64_t n = input_table.num_rows();
  const int64_t n_recv = recv_offsets.back();
  hipStream_t st = dj_rt_stream();
  for (cudf::size_type c = 0; c < input_table.num_columns(); c++) {
    if (input_table.column(c).type().id() != cudf::type_id::STRING) {
      if (strings) {
        strings->send_char_offsets.emplace_back();
        strings->recv_char_offsets.emplace_back();
        strings->sizes_to_send.emplace_back();
        strings->sizes_received.emplace_back();
      }
      continue;
    }
    if (!strings) {
      strings = std::make_shared<StringsState>();
      for (cudf::size_type cc = 0; cc < c; cc++) {
        strings->send_char_offsets.emplace_back();
        strings->recv_char_offsets.emplace_back();
        strings->sizes_to_send.emplace_back();
        strings->sizes_received.emplace_back();
      }
    }
    auto col = input_table.column(c);
    /* row sizes first: launch_communication copies the self slice of them on
     * the COMM stream, which is not ordered after this compute-stream
     * kernel — the stream syncs of the boundary reads below complete it
     * before the constructor returns */
    DBuf sizes((size_t)(n > 0 ? n : 1) * 4);
    dj::sizes_from_offsets(col.head<int32_t>(), n, (int32_t*)sizes.p, st);
    /* char offsets at the G+1 send row boundaries */
    std::vector<int64_t> soff(G + 1);
    for (int k = 0; k <= G; k++)
      soff[k] = read_back<int32_t>(col.head<int32_t>() + send_offsets[k], st);
    std::vector<int64_t> roff;
    communicate_sizes(soff, roff, comm_group, communicator);
    /* the received column keeps the int32 offsets convention: refuse loudly
     * if the gathered slices' chars exceed it (same cap as the reference's
     * cuDF 0.19; the receiver-side scan would otherwise wrap) */
    DJ_CHECK_ERROR(roff.empty() || roff.back() <= (int64_t)INT32_MAX,
                   "all-to-all: received string chars exceed 2^31 (int32 offsets limit)");
    strings->send_char_offsets.push_back(std::move(soff));
    strings->recv_char_offsets.push_back(std::move(roff));
    strings->sizes_to_send.push_back(std::move(sizes));
    strings->sizes_received.push_back(DBuf((size_t)(n_recv > 0 ? n_recv : 1) * 4));
  }
}

AllToAllCommunicator::AllToAllCommunicator(
  cudf::table_view input_table_,
  std::vector<cudf::size_type> offsets,
  Communicator* communicator_,
  std::vector<ColumnCompressionOptions> compression_options_,
  bool explicit_copy_to_current_rank_)
  : AllToAllCommunicator(input_table_,
                         std::move(offsets),
                         CommunicationGroup(communicator_->mpi_size, 1, communicator_->mpi_rank),
                         communicator_,
                         std::move(compression_options_),
                         explicit_copy_to_current_rank_)
{
}

std::unique_ptr<cudf::table> AllToAllCommunicator::allocate_communicated_table()
{
  std::vector<std::unique_ptr<cudf::column>> cols;
  cudf::size_type nrows = (cudf::size_type)recv_offsets.back();
  for (cudf::size_type c = 0; c < input_table.num_columns(); c++) {
    if (input_table.column(c).type().id() == cudf::type_id::STRING)
      cols.push_back(std::make_unique<cudf::column>(
        nrows, strings->recv_char_offsets[c].back()));
    else
      cols.push_back(std::make_unique<cudf::column>(input_table.column(c).type(), nrows));
    /* filled by launch_communication's merge, self slice included */
    if ((nullable_cols >> c) & 1u) cols.back()->allocate_null_mask();
  }
  auto out = std::make_unique<cudf::table>(std::move(cols));
  if (explicit_copy_to_current_rank) {
    /* copy the self partition now, outside launch_communication, so the
     * comm phase moves only remote slices (all_to_all_comm.cpp:701-729) */
    const int me = comm_group.get_local_idx();
    for (cudf::size_type c = 0; c < input_table.num_columns(); c++) {
      int64_t scount = (int64_t)send_offsets[me + 1] - send_offsets[me];
      if (scount <= 0) continue;
      if (input_table.column(c).type().id() == cudf::type_id::STRING) {
        /* self slice of row SIZES into sizes_received + chars slice */
        DJ_HIP_CALL(hipMemcpyAsync(
          (int32_t*)strings->sizes_received[c].p + recv_offsets[me],
          (const int32_t*)strings->sizes_to_send[c].p + send_offsets[me],
          (size_t)scount * 4, hipMemcpyDeviceToDevice, dj_rt_stream()));
        int64_t cbytes =
          strings->send_char_offsets[c][me + 1] - strings->send_char_offsets[c][me];
        if (cbytes > 0)
          DJ_HIP_CALL(hipMemcpyAsync(
            (uint8_t*)out->get_column(c).chars() + strings->recv_char_offsets[c][me],
            (const uint8_t*)input_table.column(c).chars() +
              strings->send_char_offsets[c][me],
            (size_t)cbytes, hipMemcpyDeviceToDevice, dj_rt_stream()));
      } else {
        const int esize = cudf::size_of(input_table.column(c).type());
        DJ_HIP_CALL(hipMemcpyAsync(
          (int8_t*)out->get_column(c).head() + recv_offsets[me] * esize,
          input_table.column(c).head<int8_t>() + (int64_t)send_offsets[me] * esize,
          (size_t)scount * esize, hipMemcpyDeviceToDevice, dj_rt_stream()));
      }
    }
    DJ_HIP_CALL(hipStreamSynchronize(dj_rt_stream()));
  }
  return out;
}

/* ------------------------------------------- launch_communication, in steps */

namespace {

/* one buffer of the exchange: peer i is sent send_count(i) elements of
 * `esize` bytes from element soff[i] of src and its slice is received at
 * element roff[i] of dst. A plain buffer sends whole ranges (soff has G+1
 * entries, like roff); a compressed one is the same thing over bytes, its
 * send slices sitting at the start of bound-sized slots. */
struct Wire {
  const int8_t* src;
  int8_t* dst;
  int esize;
  const std::vector<int64_t>* soff;              // send offsets (G+1)
  const std::vector<int64_t>* roff;              // receive offsets (G+1)
  const std::vector<int64_t>* scount = nullptr;  // per-peer send counts, where the
                                                 // slices do not fill their ranges
  int64_t send_count(int i) const
  {
    return scount ? (*scount)[i] : (*soff)[i + 1] - (*soff)[i];
  }
};

/* a cascaded-compressed buffer (the reference's compression branch,
 * all_to_all_comm.cpp:358-478: compress -> exchange compressed sizes ->
 * exchange compressed slices -> decompress receiver-side) */
struct CompWire {
  const uint8_t* src;  // uncompressed source buffer
  uint8_t* dst;        // uncompressed destination
  int esize;
  int rles, delta, bp;
  const std::vector<int64_t>* soff;  // element offsets (source)
  const std::vector<int64_t>* roff;  // element offsets (destination)
  DBuf comp;                         // compressed send slices (bound-sized slots)
  std::vector<int64_t> slot;         // slot byte offsets (G+1)
  std::vector<int64_t> csize;        // compressed bytes per peer
  std::vector<int64_t> csend_off;    // prefix of csize (G+1)
  std::vector<int64_t> crecv_off;    // recv byte offsets (G+1)
  DBuf comp_recv;
  Wire wire() const
  {
    return Wire{(const int8_t*)comp.p, (int8_t*)comp_recv.p, 1, &slot, &crecv_off, &csize};
  }
};

/* the validity mask of one column nullable anywhere in the group: each
 * peer's row slice is cut out of the column's mask into a word-aligned
 * packed slice of one staging buffer (dj::copy_bitmask_segments) and
 * travels raw, as uint32 words, behind the data buffers; the receiver
 * merges the G slices at recv_offsets. Never compressed. The self slice
 * does not travel: the merge reads it from the input mask. */
struct MaskWire {
  cudf::size_type col;
  DBuf send_stage, recv_stage;
  std::vector<int64_t> swo, rwo;  // word offsets per peer (G+1), self empty
};

/* one launch_communication: the steps in the order they run */
class Exchange {
 public:
  Exchange(cudf::table_view in_, cudf::mutable_table_view out_, CommunicationGroup group_,
           Communicator* communicator_, std::vector<cudf::size_type> const& send_offsets,
           std::vector<int64_t> const& recv_offsets_, uint32_t nullable_cols_,
           bool include_self_)
    : in(in_),
      out(out_),
      group(group_),
      communicator(communicator_),
      G(group_.size()),
      me(group_.get_local_idx()),
      include_self(include_self_),
      nullable_cols(nullable_cols_),
      st(dj_rt_stream()),
      soff(send_offsets.begin(), send_offsets.end()),
      recv_offsets(recv_offsets_)
  {
  }

  /* wire plan: per column one or two buffers, each either plain or
   * cascaded-compressed */
  void build_wire_plan(std::vector<ColumnCompressionOptions> const& opts, StringWires* strings)
  {
    for (cudf::size_type c = 0; c < in.num_columns(); c++) {
      auto ic = in.column(c);
      auto oc = out.column(c);
      if (ic.type().id() == cudf::type_id::STRING) {
        /* sizes on the wire take the OFFSETS CHILD's options — the reference
         * applies children[0] to the offsets buffer (all_to_all_comm.cpp:
         * 269-279); generate_auto_select emits parent=none, child[0]=cascaded,
         * so using the parent here would silently send sizes uncompressed.
         * Chars (children[1]) are never compressed (compression.cpp:44-60). */
        const ColumnCompressionOptions& sizes_opt =
          opts[c].children_compression_options.empty() ? opts[c]
                                                       : opts[c].children_compression_options[0];
        add_buffer(strings->sizes_to_send[c].p, strings->sizes_received[c].p, 4, &soff,
                   &recv_offsets, sizes_opt);
        plains.push_back(Wire{(const int8_t*)ic.chars(), (int8_t*)oc.chars(), 1,
                              &strings->send_char_offsets[c], &strings->recv_char_offsets[c]});
      } else {
        add_buffer(ic.head<int8_t>(), oc.head<int8_t>(), cudf::size_of(ic.type()), &soff,
                   &recv_offsets, opts[c]);
      }
    }
  }

  /* cut every peer's slice out of the masks of the nullable columns; the
   * staged slices join the plain buffers */
  void stage_mask_slices()
  {
    mwires.reserve((size_t)in.num_columns());
    for (cudf::size_type c = 0; c < in.num_columns() && nullable_cols; c++) {
      if (!((nullable_cols >> c) & 1u)) continue;
      DJ_CHECK_ERROR(out.column(c).null_mask() != nullptr,
                     "launch_communication: the communicated table lacks the mask of a nullable "
                     "column (allocate it with allocate_communicated_table)");
      mwires.emplace_back();
      MaskWire& w = mwires.back();
      w.col = c;
      w.swo.assign(G + 1, 0);
      w.rwo.assign(G + 1, 0);
      std::vector<BitSeg> segs;
      const uint32_t* mask = in.column(c).null_mask();
      for (int i = 0; i < G; i++) {
        const int64_t scount = i == me ? 0 : soff[i + 1] - soff[i];
        const int64_t rcount = i == me ? 0 : recv_offsets[i + 1] - recv_offsets[i];
        const int64_t swords = (scount + 31) / 32;
        w.swo[i + 1] = w.swo[i] + swords;
        w.rwo[i + 1] = w.rwo[i] + (rcount + 31) / 32;
        segs.push_back(BitSeg{mask, soff[i], scount});
        segs.push_back(BitSeg{nullptr, 0, swords * 32 - scount});  // pad to the word
      }
      w.send_stage = DBuf((size_t)std::max<int64_t>(w.swo[G], 1) * 4);
      w.recv_stage = DBuf((size_t)std::max<int64_t>(w.rwo[G], 1) * 4);
      seg_tables.push_back(copy_bit_segments(segs, (uint32_t*)w.send_stage.p, st));
      plains.push_back(
        Wire{(const int8_t*)w.send_stage.p, (int8_t*)w.recv_stage.p, 4, &w.swo, &w.rwo});
    }
    if (!mwires.empty()) DJ_HIP_CALL(hipStreamSynchronize(st));
  }

  /* compress send slices (compute stream), read their final sizes, and
   * exchange those */
  void compress_and_exchange_sizes()
  {
    if (comps.empty()) return;
    int64_t max_send_count = 1;
    for (auto& c : comps)
      for (int i = 0; i < G; i++)
        max_send_count = std::max(max_send_count, (*c.soff)[i + 1] - (*c.soff)[i]);
    DBuf cscratch(dj::compress_scratch_bytes(max_send_count));
    for (auto& c : comps) {
      c.slot.resize(G + 1);
      size_t acc = 0;
      for (int i = 0; i < G; i++) {
        c.slot[i] = (int64_t)acc;
        int64_t cnt = (*c.soff)[i + 1] - (*c.soff)[i];
        acc += (dj::compress_bound(cnt, c.esize) + 255) & ~(size_t)255;
      }
      c.slot[G] = (int64_t)acc;
      c.comp = DBuf(acc);
      for (int i = 0; i < G; i++) {
        if (i == me && !include_self) continue;
        int64_t cnt = (*c.soff)[i + 1] - (*c.soff)[i];
        dj::compress_slice_async(c.src + (*c.soff)[i] * c.esize, cnt, c.esize, c.rles, c.delta,
                                 c.bp, (uint8_t*)c.comp.p + c.slot[i], cscratch.p, st);
      }
    }
    DJ_HIP_CALL(hipStreamSynchronize(st));
    for (auto& c : comps) {
      c.csize.assign(G, 0);
      c.csend_off.assign(G + 1, 0);
      for (int i = 0; i < G; i++) {
        if (!(i == me && !include_self)) {
          dj::CompSliceHeader h;
          DJ_HIP_CALL(hipMemcpy(&h, (uint8_t*)c.comp.p + c.slot[i], sizeof(h),
                                hipMemcpyDeviceToHost));
          /* wire slices are padded to 4 bytes (inside the slot's bound) so
           * every received slice's packed words stay dword-aligned behind a
           * raw 1-/2-byte slice of odd length */
          c.csize[i] = ((int64_t)dj::compressed_size_from_header(h, c.esize) + 3) & ~(int64_t)3;
        }
        c.csend_off[i + 1] = c.csend_off[i] + c.csize[i];
      }
      /* exchange compressed byte counts (communicate_sizes over bytes) */
      communicate_sizes(c.csend_off, c.crecv_off, group, communicator);
      c.comp_recv = DBuf((size_t)std::max<int64_t>(c.crecv_off.back(), 1));
      for (int i = 0; i < G; i++)
        max_recv_count = std::max(max_recv_count, (*c.roff)[i + 1] - (*c.roff)[i]);
    }
  }

  /* one group: per buffer and per peer a send then a recv, plain buffers
   * before compressed ones. Ranks pair messages by order. */
  void exchange()
  {
    dj_timing::Scope t(DJ_PHASE_COMM, dj_rt_comm_stream());
    communicator->start();
    for (auto& b : plains) exchange_wire(b);
    for (auto& c : comps) exchange_wire(c.wire());
    communicator->stop();  // blocks the host (all_to_all_comm.hpp:331 contract)
  }

  /* decompress received slices */
  void decompress(bool report_timing)
  {
    if (comps.empty()) return;
    DBuf scratch(dj::compress_scratch_bytes(std::max<int64_t>(max_recv_count, 1)));
    for (auto& c : comps) {
      for (int i = 0; i < G; i++) {
        int64_t rbytes = c.crecv_off[i + 1] - c.crecv_off[i];
        int64_t rcount = (*c.roff)[i + 1] - (*c.roff)[i];
        if (rbytes == 0 || rcount == 0) continue;
        dj::CompSliceHeader h;
        DJ_HIP_CALL(hipMemcpy(&h, (uint8_t*)c.comp_recv.p + c.crecv_off[i], sizeof(h),
                              hipMemcpyDeviceToHost));
        DJ_CHECK_ERROR((int64_t)h.count == rcount,
                       "cascaded: received slice count mismatch");
        dj::decompress_slice_async((uint8_t*)c.comp_recv.p + c.crecv_off[i], h, c.esize,
                                   c.dst + (*c.roff)[i] * c.esize, scratch.p, st);
      }
    }
    DJ_HIP_CALL(hipStreamSynchronize(st));
    if (report_timing) {
      int64_t raw = 0, wire = 0;
      for (auto& c : comps) {
        for (int i = 0; i < G; i++) {
          if (i == me) continue;
          raw += ((*c.soff)[i + 1] - (*c.soff)[i]) * c.esize;
          wire += c.csize[i];
        }
      }
      if (raw > 0)
        std::cout << "Rank " << communicator->mpi_rank << ": cascaded wire "
                  << wire / 1.0e6 << "MB from " << raw / 1.0e6 << "MB ("
                  << (double)raw / (wire ? wire : 1) << "x)" << std::endl;
    }
  }

  /* receiver-side: merge the received mask slices, and this rank's own
   * slice, into the column's mask at recv_offsets; the column counts its
   * nulls when next asked (its mutable view forgot the count) */
  void merge_masks()
  {
    for (auto& w : mwires) {
      std::vector<BitSeg> segs;
      for (int i = 0; i < G; i++) {
        const int64_t rcount = recv_offsets[i + 1] - recv_offsets[i];
        if (i == me)
          segs.push_back(BitSeg{in.column(w.col).null_mask(), soff[me], rcount});
        else
          segs.push_back(BitSeg{(const uint32_t*)w.recv_stage.p + w.rwo[i], 0, rcount});
      }
      seg_tables.push_back(copy_bit_segments(segs, out.column(w.col).null_mask(), st));
    }
    if (!mwires.empty()) DJ_HIP_CALL(hipStreamSynchronize(st));
  }

  /* receiver-side: rebuild string offsets from the received sizes by scan
   * with offset[0]=0 (strings_column.cu:111-131) */
  void rebuild_string_offsets(StringWires const& strings)
  {
    const int64_t n_recv = recv_offsets.back();
    for (cudf::size_type c = 0; c < in.num_columns(); c++) {
      if (in.column(c).type().id() != cudf::type_id::STRING) continue;
      DBuf scr(dj::offsets_from_sizes_scratch_bytes(n_recv));
      dj::offsets_from_sizes((const int32_t*)strings.sizes_received[c].p, n_recv,
                             out.column(c).head<int32_t>(), scr.p, st);
      DJ_HIP_CALL(hipStreamSynchronize(st));  // scr freed on return; scan must be done
    }
  }

 private:
  void add_buffer(const void* src, void* dst, int esize, const std::vector<int64_t>* so,
                  const std::vector<int64_t>* ro, const ColumnCompressionOptions& opt)
  {
    if (opt.compression_method == CompressionMethod::cascaded) {
      CompWire c;
      c.src = (const uint8_t*)src;
      c.dst = (uint8_t*)dst;
      c.esize = esize;
      c.rles = opt.cascaded_format.num_RLEs;
      c.delta = opt.cascaded_format.num_deltas;
      c.bp = opt.cascaded_format.use_bp;
      c.soff = so;
      c.roff = ro;
      comps.push_back(std::move(c));
    } else {
      plains.push_back(Wire{(const int8_t*)src, (int8_t*)dst, esize, so, ro});
    }
  }

  /* the per-peer loop of one buffer; the self slice is a copy on the comm
   * stream */
  void exchange_wire(const Wire& b)
  {
    for (int i = 0; i < G; i++) {
      int64_t scount = b.send_count(i);
      int64_t rcount = (*b.roff)[i + 1] - (*b.roff)[i];
      const int8_t* src = b.src + (*b.soff)[i] * b.esize;
      int8_t* dst = b.dst + (*b.roff)[i] * b.esize;
      if (i == me) {
        if (include_self && scount > 0)
          DJ_HIP_CALL(hipMemcpyAsync(dst, src, (size_t)scount * b.esize,
                                     hipMemcpyDeviceToDevice, dj_rt_comm_stream()));
        continue;
      }
      int peer = group.get_global_rank(i);
      communicator->send(src, scount, b.esize, peer);
      communicator->recv(dst, rcount, b.esize, peer);
    }
  }

  cudf::table_view in;
  cudf::mutable_table_view out;
  CommunicationGroup group;
  Communicator* communicator;
  const int G, me;
  const bool include_self;
  const uint32_t nullable_cols;
  hipStream_t st;
  const std::vector<int64_t> soff;  // send row offsets (G+1)
  std::vector<int64_t> const& recv_offsets;
  std::vector<Wire> plains;
  std::vector<CompWire> comps;
  std::vector<MaskWire> mwires;
  std::vector<DBuf> seg_tables;  // live until the exchange is over
  int64_t max_recv_count{0};
};

}  // namespace

void AllToAllCommunicator::launch_communication(cudf::mutable_table_view communicated_table,
                                                bool report_timing,
                                                void* preallocated_pinned_buffer)
{
  (void)preallocated_pinned_buffer;
  Exchange x(input_table, communicated_table, comm_group, communicator, send_offsets,
             recv_offsets, nullable_cols, !explicit_copy_to_current_rank);
  x.build_wire_plan(compression_options, strings.get());
  x.stage_mask_slices();
  x.compress_and_exchange_sizes();
  x.exchange();
  x.decompress(report_timing);
  x.merge_masks();
  if (strings) x.rebuild_string_offsets(*strings);
}

/* ------------------------------------------- AllToAllCommunicatorAccess */

const std::vector<int64_t>& AllToAllCommunicatorAccess::recv_offsets(
  const AllToAllCommunicator& a)
{
  return a.recv_offsets;
}

std::unique_ptr<AllToAllCommunicator> AllToAllCommunicatorAccess::make(
  cudf::table_view t, std::vector<cudf::size_type> offsets, CommunicationGroup group,
  Communicator* communicator, std::vector<ColumnCompressionOptions> const& opts,
  bool explicit_copy, uint32_t route_tag)
{
  return std::unique_ptr<AllToAllCommunicator>(new AllToAllCommunicator(
    t, std::move(offsets), group, communicator, opts, explicit_copy, route_tag));
}
