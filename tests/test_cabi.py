"""CPU-side checks of the C-ABI library: it builds, loads, and exports every
symbol include/distributed_join.h declares. No compute calls (no GPU here).
"""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "distributed_join.h")
SO = os.path.join(REPO, "distributed_join_amd", "libdistjoin.so")


def _build():
    if not os.path.exists(SO):
        subprocess.run(["make", "-C", os.path.join(REPO, "distributed_join_amd", "csrc")],
                       check=True, capture_output=True)


def _declared_symbols():
    src = open(HEADER).read()
    # function declarations: return type then dj_name(
    return sorted(set(re.findall(r"\b(dj_\w+)\s*\(", src)))


def test_library_loads_and_exports_all_header_symbols():
    _build()
    lib = ctypes.CDLL(SO)
    syms = _declared_symbols()
    assert len(syms) >= 25
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, f"missing exports: {missing}"


def test_cpp_drop_in_headers_compile_for_user_code(tmp_path):
    """A user translation unit written against the reference's interface
    (distributed_inner_join / shuffle_on / Communicator / AllToAllCommunicator
    / distribute_table — SURVEY.md §8b list) must compile against our
    headers unchanged and link against libdistjoin.so."""
    src = tmp_path / "user.cpp"
    src.write_text(r"""
#include "communicator.hpp"
#include "compression.hpp"
#include "all_to_all_comm.hpp"
#include "distributed_join.hpp"
#include "shuffle_on.hpp"
#include "distribute_table.hpp"

#include <memory>
#include <vector>

std::unique_ptr<cudf::table> user_join(cudf::table_view left, cudf::table_view right,
                                       Communicator* communicator)
{
  auto lopts = generate_compression_options_distributed(left, false);
  auto ropts = generate_compression_options_distributed(right, false);
  return distributed_inner_join(left, right, {0}, {0}, communicator, lopts, ropts,
                                /*over_decom_factor=*/4, /*report_timing=*/false,
                                /*preallocated_pinned_buffer=*/nullptr,
                                /*nvlink_domain_size=*/1);
}

std::unique_ptr<cudf::table> user_shuffle(cudf::table_view input, Communicator* comm)
{
  CommunicationGroup group(comm->mpi_size, 1, comm->mpi_rank);
  auto opts = generate_compression_options_distributed(input, false);
  return shuffle_on(input, {0}, group, comm, opts, cudf::hash_id::HASH_MURMUR3,
                    cudf::DEFAULT_HASH_SEED);
}

std::unique_ptr<cudf::table> user_distribute(cudf::table_view global, Communicator* comm)
{
  auto local = distribute_table(global, comm);
  return collect_tables(local->view(), comm);
}

std::vector<ColumnCompressionOptions> user_compression_options(cudf::table_view t, int rank)
{
  auto none = generate_none_compression_options(t);
  auto chosen = rank == 0 ? generate_auto_select_compression_options(t) : none;
  return broadcast_compression_options(t, chosen);
}

void user_all_to_all(cudf::table_view t, Communicator* comm,
                     std::vector<cudf::size_type> offsets)
{
  AllToAllCommunicator atoa(t, offsets, comm,
                            generate_compression_options_distributed(t, false), true);
  auto out = atoa.allocate_communicated_table();
  atoa.launch_communication(out->mutable_view());
  std::vector<int64_t> recv;
  communicate_sizes(offsets, recv, CommunicationGroup(comm->mpi_size), comm);
  warmup_all_to_all(comm);
}
""")
    obj = tmp_path / "user.o"
    r = subprocess.run(
        ["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC",
         "-I", os.path.join(REPO, "include"), "-c", str(src), "-o", str(obj)],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # link check: user object + our library resolves all symbols
    exe = tmp_path / "user.so"
    r = subprocess.run(
        ["hipcc", "--offload-arch=gfx950", "-shared", str(obj),
         "-L", os.path.join(REPO, "distributed_join_amd"), "-ldistjoin",
         "-o", str(exe)],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_device_count_callable_without_gpu():
    _build()
    import distributed_join_amd as dj
    n = dj.lib().dj_device_count()
    assert n >= 0  # 0 in this container


# family -> (items one full grid covers in one trip, items one pass of the
# single-block scan covers or 0). tests/test_gpu_second_trip.py sizes its
# inputs from dj_grid_span, so its tests follow a changed cap; this table makes
# such a change a visible, deliberate edit.
GRID_SPANS = {
    "mask_gather": (524_288, 0),
    "mask_words": (524_288, 0),            # = 16,777,216 bits
    "mark_rows": (1_048_576, 0),
    "select_rows": (33_554_432, 8_388_608),
    "gather_fused": (2_097_152, 0),
    "gather_column": (524_288, 0),
    "string_rows": (524_288, 0),
    "string_sum": (262_144, 0),
    "string_scan": (8_388_608, 4_194_304),
    "string_hash": (8_388_608, 0),
    "codec_elems": (524_288, 2_097_152),
    "codec_pack": (16_777_216, 0),
    "key_helpers": (524_288, 0),
}


def test_grid_span_hook_matches_the_recorded_caps():
    _build()
    import distributed_join_amd as dj
    assert set(dj.SPAN_FAMILIES) == set(GRID_SPANS)
    assert sorted(dj.SPAN_FAMILIES.values()) == list(range(len(GRID_SPANS)))
    # the Python numbering is the header's, name by name (several families
    # share a span, so the values alone would not show two of them swapped)
    defines = dict(re.findall(r"#define\s+DJ_SPAN_(\w+)\s+(\d+)", open(HEADER).read()))
    assert int(defines.pop("FAMILIES")) == len(GRID_SPANS)
    assert {k.lower(): int(v) for k, v in defines.items()} == dj.SPAN_FAMILIES
    for family, want in GRID_SPANS.items():
        assert dj.grid_span(family) == want, family
    trip, scan = ctypes.c_int64(-1), ctypes.c_int64(-1)
    for unknown in (-1, len(GRID_SPANS)):
        assert dj.lib().dj_grid_span(unknown, ctypes.byref(trip), ctypes.byref(scan)) == -1
        assert trip.value == -1 and scan.value == -1


def test_product_path_fails_loudly_without_gpu():
    _build()
    import distributed_join_amd as dj
    if dj.lib().dj_device_count() == 0:
        with pytest.raises(dj.ExtensionMissing):
            dj.require_gpu()
