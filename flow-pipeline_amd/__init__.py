"""flow-pipeline_amd - MI355X-native flow-aggregation stage (host binding).

Thin ctypes binding over the C-ABI of ``libflowagg.so`` (``include/flowagg.h``).
The library replaces one hot path of cloudflare/flow-pipeline: Kafka message
bytes -> proto3 FlowMessage decode -> 15-column projection -> 5-minute
(SrcAS, DstAS) sum(Bytes)/sum(Packets)/count() rollup, i.e. the ClickHouse chain
``flows -> flows_raw -> flows_5m`` of ``compose/clickhouse/create.sh:5-110``.

There is no CPU fallback: if the HIP library is missing or no GPU is present the
calls raise.  (The directory name contains a hyphen; load it with
``_pkg.load()`` from the repository root or ``importlib`` - see ``_pkg.py``.)
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import dist, schema, spill  # noqa: F401  (re-export)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libflowagg.so")
if os.environ.get("FA_LIB_VARIANT"):  # A/B experiments only (tools/): libflowagg_<variant>.so built with make OUT=... EXTRA=...
    LIB_PATH = os.path.join(_HERE, "libflowagg_%s.so" % os.environ["FA_LIB_VARIANT"])

FA_KEYS_AS_PAIR = 1
FA_KEYS_SRCADDR_CMS = 2
FA_KEYS_DSTADDR_CMS = 4
FA_KEYS_ADDR_PORT_PROTO = 8
FA_KEYS_PORT_HIST = 16
FA_KEYS_MINUTE_SERIES = 32
ALL_TIMESLOTS = 0xFFFFFFFF

MOCK_MOCKER, MOCK_ASPAIRS, MOCK_ZIPF, MOCK_GOFLOW, MOCK_DISTINCT, MOCK_REVERSED = 0, 1, 2, 3, 4, 5
T0 = 1_600_000_200  # multiple of 300

ERRORS = {
    -1: "FA_ERR_ARG", -2: "FA_ERR_NO_DEVICE", -3: "FA_ERR_HIP", -4: "FA_ERR_NOMEM",
    -5: "FA_ERR_TABLE_FULL", -6: "FA_ERR_CAPACITY", -7: "FA_ERR_FRAMING", -8: "FA_ERR_UNSUPPORTED",
}


class FlowAggError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "FA_ERR"), code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [
        ("device", C.c_int32), ("window_secs", C.c_uint32), ("subwindow_secs", C.c_uint32),
        ("table_capacity_log2", C.c_uint32), ("cms_depth", C.c_uint32),
        ("cms_width_log2", C.c_uint32), ("cms_seed", C.c_uint64), ("key_sets", C.c_uint32),
        ("framed", C.c_int32), ("max_batch_records", C.c_uint32), ("topk_capacity_log2", C.c_uint32),
        ("wide_capacity_log2", C.c_uint32), ("topk_mode", C.c_uint32), ("topk_track", C.c_uint32), ("reserved", C.c_uint32 * 1),
    ]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "records_ok", "records_bad", "records_slow", "bytes_in", "batches", "table_used",
        "table_capacity", "kernel_ns", "kernel_ns_total", "kernel_launches", "batch_ns_total",
        "records_direct", "records_retried", "wide_used", "wide_capacity", "wave_tile_launches",
        "compact_tuple_launches", "records_misfit_compact", "decode_ns_total", "decode_launches",
        "records_late", "wide_log_chunks", "wide_log_bytes", "wide_log_records", "wide_log_recorded", "wide_log_folded",
        "wide_log_replayed", "wide_log_dropped", "wide_log_watermark_moves", "wide_log_nomem_folds", "wide_log_mode",
        "topk_theta_src", "topk_theta_dst", "topk_candidates_src", "topk_candidates_dst", "learnt_order_launches",
        "host_ingest_ns", "host_stage_wait_ns", "host_stage_copy_ns")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class TalkersStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "used_src", "used_dst", "capacity_src", "capacity_dst", "records_folded", "records_absorbed", "grows",
        "fold_launches", "fold_ns_total")]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["used"] = [d.pop("used_src"), d.pop("used_dst")]
        d["capacity"] = [d.pop("capacity_src"), d.pop("capacity_dst")]
        return d


class PortsStats(TalkersStats):
    """fa_ports_stats_t: fa_talkers_stats_t's members over the bucketed port tables (SrcPort, DstPort)."""


class RawPart(C.Structure):
    """fa_raw_part: one flows_raw part (a Native block of one Date) inside the bytes a take returned."""
    _fields_ = [("date", C.c_uint32), ("t_min", C.c_uint32), ("t_max", C.c_uint32), ("_pad", C.c_uint32),
                ("rows", C.c_uint64), ("offset", C.c_uint64), ("bytes", C.c_uint64)]


class RawStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "records_in", "records_bad", "rows_out", "parts_out", "bytes_out", "chunks", "pending_parts", "pending_bytes",
        "build_ns_total", "build_launches")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RawLz4Stats(C.Structure):
    """fa_raw_lz4_stats_t: what the ctx's LZ4 compressions (raw_take_lz4, lz4_frame_device) have done so far."""
    _fields_ = [(n, C.c_uint64) for n in (
        "frames", "blocks", "stored_blocks", "bytes_in", "bytes_out", "compress_launches", "device_ns", "block_ns", "pack_ns")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RawLoadStats(C.Structure):
    """fa_raw_load_stats_t: what the ctx's decodes and loads (lz4_decode_device, raw_columns, raw_load) have done so far."""
    _fields_ = [(n, C.c_uint64) for n in (
        "calls", "frames", "blocks", "stored_blocks", "bytes_in", "bytes_decoded", "parts", "rows_loaded", "launches",
        "decode_ns", "unpack_ns", "fold_ns")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RollupStats(C.Structure):
    """fa_rollup_stats_t: what the ctx's rollup folds (rollup_fold_columns, raw_load_rollup) have done so far."""
    _fields_ = [(n, C.c_uint64) for n in ("calls", "records_in", "records_bad", "records_folded", "launches", "fold_ns")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SketchFoldStats(C.Structure):
    """fa_sketch_fold_stats_t: what the ctx's sketch folds (sketch_fold_columns, raw_restore) have done so far."""
    _fields_ = [(n, C.c_uint64) for n in ("calls", "records_in", "records_bad", "records_folded", "batches", "launches", "fold_ns")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RawRangeStats(C.Structure):
    """fa_raw_range_stats_t: what the ctx's ranged loads (raw_range_probe, raw_restore_range) have done so far."""
    _fields_ = [(n, C.c_uint64) for n in (
        "calls", "parts_seen", "parts_skipped_date", "parts_empty", "blocks_seen", "blocks_decoded", "rows_seen", "rows_loaded",
        "launches", "probe_ns", "range_ns", "decode_ns")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RawSelectStats(C.Structure):
    """fa_raw_select_stats_t: what the ctx's selects of rows (raw_select) have done so far."""
    _fields_ = [(n, C.c_uint64) for n in (
        "calls", "rows_scanned", "rows_matched", "rows_out", "parts_out", "bytes_out", "launches", "select_ns", "emit_ns", "gather_ns")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RawFilter(C.Structure):
    """fa_raw_filter (include/flowagg.h "selecting rows of flows_raw parts"): 96 bytes; a member whose RAW_F_* bit is clear is not read."""
    _fields_ = [("fields", C.c_uint32), ("t_lo", C.c_uint32), ("t_hi", C.c_uint32), ("tf_lo", C.c_uint32), ("tf_hi", C.c_uint32),
                ("src_as", C.c_uint32), ("dst_as", C.c_uint32), ("etype", C.c_uint32), ("proto", C.c_uint32),
                ("src_port_lo", C.c_uint32), ("src_port_hi", C.c_uint32), ("dst_port_lo", C.c_uint32), ("dst_port_hi", C.c_uint32),
                ("src_prefix_len", C.c_uint8), ("dst_prefix_len", C.c_uint8), ("_pad", C.c_uint8 * 2),
                ("src_addr", C.c_uint8 * 16), ("dst_addr", C.c_uint8 * 16), ("limit", C.c_uint64)]


RAW_F_FLOW_START, RAW_F_SRC_AS, RAW_F_DST_AS, RAW_F_ETYPE, RAW_F_PROTO, RAW_F_SRC_PORT = 1, 2, 4, 8, 16, 32
RAW_F_DST_PORT, RAW_F_SRC_ADDR, RAW_F_DST_ADDR, RAW_F_EITHER, RAW_F_COUNT_ONLY = 64, 128, 256, 512, 1024
assert C.sizeof(RawFilter) == 96 and C.sizeof(RawSelectStats) == 80


def raw_filter(t_lo=0, t_hi=0xFFFFFFFF, *, flow_start=None, src_as=None, dst_as=None, etype=None, proto=None, src_port=None, dst_port=None,
               src_net=None, dst_net=None, either=False, limit=0, count_only=False) -> RawFilter:
    """The RawFilter of FlowAgg.raw_select's keywords: flow_start and the ports are (lo, hi), the nets (16 bytes, prefix_len)."""
    f = RawFilter()
    f.t_lo, f.t_hi, f.limit = t_lo, t_hi, limit
    if flow_start is not None:
        f.fields |= RAW_F_FLOW_START
        f.tf_lo, f.tf_hi = flow_start
    for name, bit, v in (("src_as", RAW_F_SRC_AS, src_as), ("dst_as", RAW_F_DST_AS, dst_as), ("etype", RAW_F_ETYPE, etype), ("proto", RAW_F_PROTO, proto)):
        if v is not None:
            f.fields |= bit
            setattr(f, name, v)
    for name, bit, v in (("src_port", RAW_F_SRC_PORT, src_port), ("dst_port", RAW_F_DST_PORT, dst_port)):
        if v is not None:
            f.fields |= bit
            setattr(f, name + "_lo", v[0]), setattr(f, name + "_hi", v[1])
    for name, bit, v in (("src", RAW_F_SRC_ADDR, src_net), ("dst", RAW_F_DST_ADDR, dst_net)):
        if v is not None:
            addr, plen = v
            if len(addr) != 16 or not 0 <= plen <= 255:
                raise ValueError("a net is (16 bytes, prefix_len)")
            f.fields |= bit
            setattr(f, name + "_addr", (C.c_uint8 * 16)(*bytes(addr))), setattr(f, name + "_prefix_len", plen)
    f.fields |= (RAW_F_EITHER if either else 0) | (RAW_F_COUNT_ONLY if count_only else 0)
    return f


class RawQuery(C.Structure):
    """fa_raw_query_t (include/flowagg.h "grouped queries over flows_raw parts"): 104 bytes."""
    _fields_ = [("where", RawFilter), ("groups", C.c_uint32), ("flags", C.c_uint32)]


class RawQueryStats(C.Structure):
    """fa_raw_query_stats_t: what the ctx's grouped queries (raw_query and its reads) have done so far."""
    _fields_ = [(n, C.c_uint64) for n in (
        "calls", "rows_scanned", "rows_matched", "updates", "absorbed", "groups", "grows", "launches", "fold_ns", "order_ns")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RawQueryMergeStats(C.Structure):
    """fa_raw_query_merge_stats_t: the raw_query_merge calls that added their rows, and the rows."""
    _fields_ = [("merge_calls", C.c_uint64), ("rows_merged", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


RAW_G_SRC_ADDR, RAW_G_DST_ADDR, RAW_G_SRC_PORT, RAW_G_DST_PORT, RAW_G_MINUTE, RAW_G_SRC_AS, RAW_G_DST_AS, RAW_G_PROTO, RAW_G_TOTAL = (1 << i for i in range(9))
RAW_G_ALL = 511
RAW_Q_KEEP = 1
RAW_O_WEIGHT, RAW_O_KEY = 0, 1
QUERY_ROW_DTYPE = np.dtype([("key", "u1", 16), ("etype", "<u4"), ("value", "<u4"), ("weight", "<u8"), ("count", "<u8")])  # fa_query_row
assert C.sizeof(RawQuery) == 104 and C.sizeof(RawQueryStats) == 80 and QUERY_ROW_DTYPE.itemsize == 40


class RawPendingStats(C.Structure):
    """fa_raw_pending_stats_t: what the ctx's calls over its pending parts (raw_pending_probe, raw_query_pending, raw_select_pending)
    have done so far."""
    _fields_ = [(n, C.c_uint64) for n in (
        "calls", "parts_seen", "parts_skipped", "parts_whole", "parts_searched", "rows_seen", "rows_in_range", "bounds_launches", "bounds_ns")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


assert C.sizeof(RawPendingStats) == 72


class RawMergeStats(C.Structure):
    """fa_raw_merge_stats_t: what the ctx's merges of pending parts (raw_merge) have done so far."""
    _fields_ = [(n, C.c_uint64) for n in (
        "merges", "parts_in", "parts_out", "rows", "bytes_in", "bytes_out", "launches", "order_ns", "gather_ns")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


LZ4_SPAN_DTYPE = np.dtype([("offset", "<u8"), ("bytes", "<u8")])  # fa_lz4_span
RAW_RANGE_DTYPE = np.dtype([("date", "<u4"), ("t_min", "<u4"), ("t_max", "<u4"), ("_pad", "<u4"), ("rows", "<u8"), ("r_lo", "<u8"), ("r_hi", "<u8")])  # fa_raw_range
assert RAW_RANGE_DTYPE.itemsize == 40 and C.sizeof(RawRangeStats) == 96


class MockParams(C.Structure):
    _fields_ = [
        ("mode", C.c_uint32), ("framed", C.c_uint32), ("seed", C.c_uint64),
        ("n_total", C.c_uint64), ("t0", C.c_uint64), ("span_secs", C.c_uint32),
        ("per_sec", C.c_uint32), ("zipf_log2_universe", C.c_uint32), ("zipf_s_x100", C.c_uint32),
    ]


class Columns(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "time_received", "time_flow_start", "sampling_rate", "bytes", "packets",
        "sequence_num", "src_as", "dst_as", "etype", "proto", "src_port", "dst_port",
        "sampler_address", "src_addr", "dst_addr", "status")]


class DeviceState(C.Structure):
    _fields_ = [("cms_src", C.c_void_p), ("cms_dst", C.c_void_p), ("cms_words", C.c_size_t),
                ("port_hist", C.c_void_p), ("port_hist_words", C.c_size_t),
                ("cms_src_merged", C.c_void_p), ("cms_dst_merged", C.c_void_p)]


ROW5M_DTYPE = np.dtype([
    ("date", "<u4"), ("timeslot", "<u4"), ("src_as", "<u4"), ("dst_as", "<u4"),
    ("etype", "<u4"), ("_pad", "<u4"), ("bytes", "<u8"), ("packets", "<u8"), ("count", "<u8"),
])
FLOW_ROW_DTYPE = np.dtype([
    ("time_received", "<u8"), ("time_flow_start", "<u8"), ("sampling_rate", "<u8"),
    ("bytes", "<u8"), ("packets", "<u8"), ("sequence_num", "<u4"), ("src_as", "<u4"),
    ("dst_as", "<u4"), ("etype", "<u4"), ("proto", "<u4"), ("src_port", "<u4"),
    ("dst_port", "<u4"), ("status", "<u4"), ("sampler_address", "u1", 16),
    ("src_addr", "u1", 16), ("dst_addr", "u1", 16),
])
TOPK_DTYPE = np.dtype([("key", "u1", 16), ("weight", "<u8")])
ROW_APP_DTYPE = np.dtype([
    ("date", "<u4"), ("timeslot", "<u4"), ("src_addr", "u1", 16), ("dst_port", "<u4"), ("proto", "<u4"),
    ("bytes", "<u8"), ("packets", "<u8"), ("count", "<u8"),
])
ROW_APP48_DTYPE = np.dtype([("src_addr", "u1", 16), ("dst_port", "<u4"), ("proto", "<u4"), ("bytes", "<u8"), ("packets", "<u8"), ("count", "<u8")])
PORT_ROW_DTYPE = np.dtype([("port", "<u4"), ("_pad", "<u4"), ("weight", "<u8"), ("count", "<u8")])
MINUTE_ROW_DTYPE = np.dtype([("minute", "<u4"), ("_pad", "<u4"), ("weight", "<u8"), ("count", "<u8")])
TALKER_ROW_DTYPE = np.dtype([("key", "u1", 16), ("etype", "<u4"), ("_pad", "<u4"), ("weight", "<u8"), ("count", "<u8")])
RAW_PART_DTYPE = np.dtype([("date", "<u4"), ("t_min", "<u4"), ("t_max", "<u4"), ("_pad", "<u4"), ("rows", "<u8"), ("offset", "<u8"), ("bytes", "<u8")])
assert RAW_PART_DTYPE.itemsize == C.sizeof(RawPart) == 40 and C.sizeof(RawStats) == 80
assert TALKER_ROW_DTYPE.itemsize == 40
# geometry of the fold kernel (csrc/talkers.cuh): threads per workgroup, LDS cache entries per direction, workgroups per CU
TALK_BLOCK, TALK_LDS_ENTRIES, TALK_WG_PER_CU = 512, 512, 2
# ... and of the port fold kernel (csrc/ports.cuh)
PORT_BLOCK, PORT_LDS_ENTRIES, PORT_WG_PER_CU = 512, 512, 2
assert ROW5M_DTYPE.itemsize == 48 and FLOW_ROW_DTYPE.itemsize == 120
assert ROW_APP_DTYPE.itemsize == 56 and PORT_ROW_DTYPE.itemsize == 24 and MINUTE_ROW_DTYPE.itemsize == 24
ROW_DTYPES = [ROW5M_DTYPE, ROW_APP_DTYPE, PORT_ROW_DTYPE, PORT_ROW_DTYPE, MINUTE_ROW_DTYPE, TOPK_DTYPE, TOPK_DTYPE,
              None, TALKER_ROW_DTYPE, TALKER_ROW_DTYPE, None, None, QUERY_ROW_DTYPE, QUERY_ROW_DTYPE]  # by row kind (7, 10 and 11 are none)

# every symbol include/flowagg.h declares (checked by the CPU test-suite)
EXPORTS = [
    "fa_abi_version", "fa_create", "fa_destroy", "fa_last_error", "fa_ingest", "fa_ingest_device",
    "fa_sync", "fa_decode", "fa_decode_device", "fa_open_timeslots", "fa_close_window",
    "fa_read_window", "fa_window_rows_device", "fa_merge_rows_device", "fa_topk", "fa_topk_merge_keys", "fa_cms_query", "fa_cms_read", "fa_cms_reset",
    "fa_device_state_get", "fa_merged_view_set", "fa_merge_rows", "fa_merge_allreduce", "fa_stats",
    "fa_mock_generate_device", "fa_mock_generate_host",
    "fa_read_window_app", "fa_close_window_app", "fa_merge_rows_app", "fa_top_ports", "fa_merge_ports",
    "fa_minute_series", "fa_merge_minutes", "fa_dashboard_reset", "fa_rows_to_rowbinary", "fa_format_addr",
    "fa_row_bytes", "fa_rows_device", "fa_rows_merge_device", "fa_rows_fetch", "fa_drop_window", "fa_rows_partition_device", "fa_drop_range",
    "fa_group_create", "fa_group_destroy", "fa_group_last_error", "fa_group_size", "fa_group_transport", "fa_group_open_timeslots",
    "fa_group_read_window", "fa_group_close_window", "fa_group_read_window_partitioned", "fa_group_close_window_partitioned",
    "fa_group_allreduce_sketches", "fa_group_topk", "fa_group_stats", "fa_read_window_app48", "fa_close_window_app48",
    "fa_reserve_ingest",
    "fa_talkers_enable", "fa_talkers_fold_columns_device", "fa_top_talkers", "fa_merge_talkers", "fa_talkers_reset", "fa_talkers_stats",
    "fa_merge_talkers_device", "fa_group_top_talkers",
    "fa_talkers_enable_buckets", "fa_top_talkers_range", "fa_talkers_range_rows_device", "fa_talkers_buckets", "fa_talkers_drop_before",
    "fa_group_top_talkers_range",
    "fa_ports_enable_buckets", "fa_ports_fold_columns_device", "fa_top_ports_range", "fa_ports_range_rows_device", "fa_ports_buckets",
    "fa_ports_drop_before", "fa_ports_reset", "fa_ports_stats", "fa_group_top_ports_range",
    "fa_raw_part_bytes", "fa_flow_rows_to_native", "fa_raw_enable", "fa_raw_build_columns_device", "fa_raw_take", "fa_raw_take_device",
    "fa_raw_reset", "fa_raw_stats", "fa_raw_merge", "fa_raw_merge_stats",
    "fa_raw_take_lz4", "fa_raw_take_lz4_device", "fa_lz4_frame_device", "fa_lz4_frame", "fa_lz4_frame_bound", "fa_raw_lz4_stats",
    "fa_lz4_decode", "fa_lz4_decode_device", "fa_raw_columns_device", "fa_raw_load", "fa_raw_load_stats", "fa_raw_load_reset",
    "fa_rollup_fold_columns_device", "fa_raw_load_rollup", "fa_rollup_stats",
    "fa_sketch_fold_columns_device", "fa_raw_restore", "fa_sketch_fold_stats",
    "fa_raw_range_probe", "fa_raw_restore_range", "fa_raw_range_stats",
    "fa_raw_select", "fa_raw_selection_device", "fa_raw_selection_fetch", "fa_raw_select_stats",
    "fa_raw_query", "fa_raw_query_rows", "fa_raw_query_rows_device", "fa_raw_query_reset", "fa_raw_query_stats",
    "fa_raw_pending_probe", "fa_raw_query_pending", "fa_raw_select_pending", "fa_raw_pending_stats",
    "fa_raw_query_merge_device", "fa_raw_query_merge_rows", "fa_raw_query_merge_stats",
    "fa_group_raw_query_pending", "fa_group_raw_query_rows", "fa_group_raw_query_reset",
]
GROUP_PEER, GROUP_RCCL = 0, 1
TOPK_EXACT, TOPK_CANDIDATES = 0, 1
# row kinds of the device-resident window close (include/flowagg.h, ABI 5)
ROWS_5M, ROWS_APP, ROWS_PORT_SRC, ROWS_PORT_DST, ROWS_MINUTE, ROWS_TOPK_SRC, ROWS_TOPK_DST = range(7)
ROWS_TALKERS_SRC, ROWS_TALKERS_DST = 8, 9  # (ABI 8, addition; 7 is unassigned)
ROWS_QUERY_WEIGHT, ROWS_QUERY_KEY = 12, 13  # query rows in raw_query_rows' two orders (ABI 8, addition; 10 and 11 are unassigned)

_LIB = None


def build(force=False):
    """Compile libflowagg.so for gfx950 with hipcc (cross-compiles without a GPU).

    Safe under `torch.distributed.run` (every rank calls it): the staleness check and the compile run under an
    exclusive file lock, the compiler writes to a private name and the result is renamed into place, so a rank
    never loads a half-written library and at most one rank compiles."""
    import fcntl
    srcdir = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(srcdir, f) for f in os.listdir(srcdir) if not f.endswith(".so")] + [
        os.path.join(_HERE, "..", "include", "flowagg.h")]

    stamp = LIB_PATH + ".srchash"  # the sources the library was built from (a copy of the tree may reset every mtime)

    def stamped():
        try:
            with open(stamp) as f:
                return f.read().strip()
        except OSError:
            return None

    def stale():
        if not os.path.exists(LIB_PATH):
            return True
        if stamped() == source_hash():
            return False  # (built from exactly these sources, whatever the mtimes say)
        return stamped() is not None or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)

    def write_stamp():
        try:
            with open(stamp + ".tmp.%d" % os.getpid(), "w") as f:
                f.write(source_hash() + "\n")
            os.replace(stamp + ".tmp.%d" % os.getpid(), stamp)
        except OSError:
            pass

    if os.environ.get("FA_LIB_VARIANT"):  # A/B libraries are built by hand with their own EXTRA flags: never rebuilt here
        if not os.path.exists(LIB_PATH):
            raise FlowAggError(-2, "%s is not built" % LIB_PATH)
        return LIB_PATH
    if not (force or stale()):
        if stamped() is None:
            write_stamp()  # (a library built by hand with make, newer than its sources: remember what it was built from)
        return LIB_PATH
    with open(os.path.join(_HERE, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if force or stale():
                tmp = LIB_PATH + ".tmp.%d" % os.getpid()
                try:
                    subprocess.check_call(["make", "-C", srcdir, "-B", "OUT=" + tmp], stdout=subprocess.DEVNULL)
                    os.replace(tmp, LIB_PATH)
                    write_stamp()
                finally:
                    if os.path.exists(tmp):
                        os.unlink(tmp)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB_PATH


def source_hash() -> str:
    """sha256 (first 16 hex digits) over the library's sources: stamps profiles (tools/prof_summary.py) so that
    bench.py only quotes PMC traffic measured on the code it is running."""
    import hashlib
    srcdir = os.path.join(_HERE, "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(srcdir)) + [os.path.join("..", "..", "include", "flowagg.h")]:
        if f.endswith((".cuh", ".hip", ".h", ".inc", "Makefile")):
            with open(os.path.join(srcdir, f), "rb") as fh:
                h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def lib():
    """Load libflowagg.so.  Raises (never falls back) when it is not built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise FlowAggError(-2, "libflowagg.so is not built (run `python -c 'import __graft_entry__ as g; "
                               "g.build()'` or `make -C flow-pipeline_amd/csrc`); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, sz, u32, u64 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64
    szp = C.POINTER(C.c_size_t)
    L.fa_abi_version.restype = u32
    L.fa_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.fa_destroy.argtypes = [vp]
    L.fa_destroy.restype = None
    L.fa_last_error.argtypes = [vp]
    L.fa_last_error.restype = C.c_char_p
    L.fa_ingest.argtypes = [vp, vp, sz, vp, sz]
    L.fa_ingest_device.argtypes = [vp, vp, sz, vp, sz]
    L.fa_sync.argtypes = [vp]
    L.fa_reserve_ingest.argtypes = [vp, sz, sz]
    L.fa_decode.argtypes = [vp, vp, sz, vp, sz, vp]
    L.fa_decode_device.argtypes = [vp, vp, sz, vp, sz, C.POINTER(Columns)]
    L.fa_open_timeslots.argtypes = [vp, vp, sz, szp]
    L.fa_close_window.argtypes = [vp, u32, vp, sz, szp]
    L.fa_read_window.argtypes = [vp, u32, vp, sz, szp]
    L.fa_window_rows_device.argtypes = [vp, u32, C.POINTER(vp), szp]
    L.fa_merge_rows_device.argtypes = [vp, vp, sz]
    L.fa_topk.argtypes = [vp, u32, sz, vp, sz, szp]
    L.fa_topk_merge_keys.argtypes = [vp, u32, vp, sz]
    L.fa_cms_query.argtypes = [vp, u32, C.c_char_p, C.POINTER(u64)]
    L.fa_cms_read.argtypes = [vp, u32, vp, sz]
    L.fa_cms_reset.argtypes = [vp, u32]
    L.fa_device_state_get.argtypes = [vp, C.POINTER(DeviceState)]
    L.fa_merged_view_set.argtypes = [vp, C.c_int]
    L.fa_merge_rows.argtypes = [vp, vp, sz]
    L.fa_merge_allreduce.argtypes = [vp, vp]
    L.fa_stats.argtypes = [vp, C.POINTER(Stats)]
    L.fa_mock_generate_device.argtypes = [vp, C.POINTER(MockParams), u64, u64, vp, sz, vp, C.POINTER(u64)]
    L.fa_mock_generate_host.argtypes = [C.POINTER(MockParams), u64, u64, vp, sz, vp, C.POINTER(u64)]
    L.fa_read_window_app.argtypes = [vp, u32, vp, sz, szp]
    L.fa_close_window_app.argtypes = [vp, u32, vp, sz, szp]
    L.fa_merge_rows_app.argtypes = [vp, vp, sz]
    L.fa_top_ports.argtypes = [vp, C.c_int, sz, vp, sz, szp]
    L.fa_merge_ports.argtypes = [vp, C.c_int, vp, sz]
    L.fa_minute_series.argtypes = [vp, vp, sz, szp]
    L.fa_merge_minutes.argtypes = [vp, vp, sz]
    L.fa_dashboard_reset.argtypes = [vp]
    L.fa_rows_to_rowbinary.argtypes = [vp, sz, vp, sz, szp]
    L.fa_format_addr.argtypes = [C.c_char_p, u32, C.c_char_p, sz]
    L.fa_row_bytes.argtypes = [C.c_int]
    L.fa_row_bytes.restype = sz
    L.fa_rows_device.argtypes = [vp, C.c_int, u32, sz, C.POINTER(vp), szp]
    L.fa_rows_merge_device.argtypes = [vp, C.c_int, vp, sz, sz, C.POINTER(vp), szp]
    L.fa_rows_fetch.argtypes = [vp, C.c_int, vp, sz, vp, sz]
    L.fa_rows_partition_device.argtypes = [vp, C.c_int, vp, sz, u32, C.POINTER(vp), szp]
    L.fa_drop_window.argtypes = [vp, C.c_int, u32]
    L.fa_drop_range.argtypes = [vp, C.c_int, u32, u32]
    L.fa_read_window_app48.argtypes = [vp, u32, vp, sz, szp, C.POINTER(u32)]
    L.fa_close_window_app48.argtypes = [vp, u32, vp, sz, szp, C.POINTER(u32)]
    L.fa_group_create.argtypes = [C.POINTER(vp), sz, u32, C.POINTER(vp)]
    L.fa_group_destroy.argtypes = [vp]
    L.fa_group_destroy.restype = None
    L.fa_group_last_error.argtypes = [vp]
    L.fa_group_last_error.restype = C.c_char_p
    L.fa_group_size.argtypes = [vp]
    L.fa_group_size.restype = sz
    L.fa_group_transport.argtypes = [vp]
    L.fa_group_open_timeslots.argtypes = [vp, vp, sz, szp]
    L.fa_group_read_window.argtypes = [vp, C.c_int, u32, sz, vp, sz, szp]
    L.fa_group_close_window.argtypes = [vp, C.c_int, u32, vp, sz, szp]
    L.fa_group_read_window_partitioned.argtypes = [vp, C.c_int, u32, vp, sz, szp, szp]
    L.fa_group_close_window_partitioned.argtypes = [vp, C.c_int, u32, vp, sz, szp, szp]
    L.fa_group_allreduce_sketches.argtypes = [vp]
    L.fa_group_topk.argtypes = [vp, u32, sz, vp, sz, szp]
    L.fa_group_stats.argtypes = [vp, C.POINTER(Stats)]
    L.fa_talkers_enable.argtypes = [vp, u32]
    L.fa_talkers_fold_columns_device.argtypes = [vp, C.POINTER(Columns), sz]
    L.fa_top_talkers.argtypes = [vp, C.c_int, sz, vp, sz, szp]
    L.fa_merge_talkers.argtypes = [vp, C.c_int, vp, sz]
    L.fa_talkers_reset.argtypes = [vp]
    L.fa_talkers_stats.argtypes = [vp, C.POINTER(TalkersStats)]
    L.fa_merge_talkers_device.argtypes = [vp, C.c_int, vp, sz]
    L.fa_group_top_talkers.argtypes = [vp, C.c_int, sz, vp, sz, szp]
    L.fa_talkers_enable_buckets.argtypes = [vp, u32, u32]
    L.fa_top_talkers_range.argtypes = [vp, C.c_int, u32, u32, sz, vp, sz, szp]
    L.fa_talkers_range_rows_device.argtypes = [vp, C.c_int, u32, u32, sz, C.POINTER(C.c_void_p), szp]
    L.fa_talkers_buckets.argtypes = [vp, vp, sz, szp]
    L.fa_talkers_drop_before.argtypes = [vp, u32]
    L.fa_group_top_talkers_range.argtypes = [vp, C.c_int, u32, u32, sz, vp, sz, szp]
    L.fa_ports_enable_buckets.argtypes = [vp, u32, u32]
    L.fa_ports_fold_columns_device.argtypes = [vp, C.POINTER(Columns), sz]
    L.fa_top_ports_range.argtypes = [vp, C.c_int, u32, u32, sz, vp, sz, szp]
    L.fa_ports_range_rows_device.argtypes = [vp, C.c_int, u32, u32, sz, C.POINTER(C.c_void_p), szp]
    L.fa_ports_buckets.argtypes = [vp, vp, sz, szp]
    L.fa_ports_drop_before.argtypes = [vp, u32]
    L.fa_ports_reset.argtypes = [vp]
    L.fa_ports_stats.argtypes = [vp, C.POINTER(PortsStats)]
    L.fa_group_top_ports_range.argtypes = [vp, C.c_int, u32, u32, sz, vp, sz, szp]
    L.fa_raw_part_bytes.argtypes = [u64]
    L.fa_raw_part_bytes.restype = sz
    L.fa_flow_rows_to_native.argtypes = [vp, sz, vp, sz, szp]
    L.fa_raw_enable.argtypes = [vp, u32]
    L.fa_raw_build_columns_device.argtypes = [vp, C.POINTER(Columns), sz]
    L.fa_raw_take.argtypes = [vp, vp, sz, szp, vp, sz, szp]
    L.fa_raw_take_device.argtypes = [vp, C.POINTER(vp), szp, vp, sz, szp]
    L.fa_raw_reset.argtypes = [vp]
    L.fa_raw_stats.argtypes = [vp, C.POINTER(RawStats)]
    L.fa_raw_take_lz4.argtypes = [vp, vp, sz, szp, vp, sz, szp]
    L.fa_raw_take_lz4_device.argtypes = [vp, C.POINTER(vp), szp, vp, sz, szp]
    L.fa_lz4_frame_device.argtypes = [vp, vp, sz, C.POINTER(vp), szp]
    L.fa_lz4_frame.argtypes = [vp, sz, vp, sz, szp]
    L.fa_lz4_frame_bound.argtypes = [sz]
    L.fa_lz4_frame_bound.restype = sz
    L.fa_raw_lz4_stats.argtypes = [vp, C.POINTER(RawLz4Stats)]
    L.fa_lz4_decode.argtypes = [vp, sz, vp, sz, szp]
    L.fa_lz4_decode_device.argtypes = [vp, vp, sz, C.POINTER(vp), vp, sz, szp]
    L.fa_raw_columns_device.argtypes = [vp, vp, sz, C.POINTER(Columns), szp]
    L.fa_raw_load.argtypes = [vp, vp, sz]
    L.fa_raw_load_stats.argtypes = [vp, C.POINTER(RawLoadStats)]
    L.fa_raw_load_reset.argtypes = [vp]
    L.fa_rollup_fold_columns_device.argtypes = [vp, C.POINTER(Columns), sz, u32]
    L.fa_raw_load_rollup.argtypes = [vp, vp, sz, u32, C.c_int]
    L.fa_rollup_stats.argtypes = [vp, C.POINTER(RollupStats)]
    L.fa_sketch_fold_columns_device.argtypes = [vp, C.POINTER(Columns), sz, u32]
    L.fa_raw_restore.argtypes = [vp, vp, sz, u32, C.c_int]
    L.fa_sketch_fold_stats.argtypes = [vp, C.POINTER(SketchFoldStats)]
    L.fa_raw_range_probe.argtypes = [vp, vp, sz, u32, u32, vp, sz, szp]
    L.fa_raw_restore_range.argtypes = [vp, vp, sz, u32, u32, u32, C.c_int]
    L.fa_raw_range_stats.argtypes = [vp, C.POINTER(RawRangeStats)]
    L.fa_raw_select.argtypes = [vp, vp, sz, C.POINTER(RawFilter), vp, sz, szp, szp]
    L.fa_raw_selection_device.argtypes = [vp, C.POINTER(C.c_void_p), szp]
    L.fa_raw_selection_fetch.argtypes = [vp, vp, sz, szp]
    L.fa_raw_select_stats.argtypes = [vp, C.POINTER(RawSelectStats)]
    L.fa_raw_query.argtypes = [vp, vp, sz, C.POINTER(RawQuery)]
    L.fa_raw_query_rows.argtypes = [vp, C.c_uint32, C.c_int, sz, vp, sz, szp]
    L.fa_raw_query_rows_device.argtypes = [vp, C.c_uint32, C.c_int, sz, C.POINTER(C.c_void_p), szp]
    L.fa_raw_query_reset.argtypes = [vp]
    L.fa_raw_query_stats.argtypes = [vp, C.POINTER(RawQueryStats)]
    L.fa_raw_pending_probe.argtypes = [vp, u32, u32, vp, sz, szp]
    L.fa_raw_query_pending.argtypes = [vp, C.POINTER(RawQuery)]
    L.fa_raw_query_merge_device.argtypes = [vp, C.c_uint32, vp, sz]
    L.fa_raw_query_merge_rows.argtypes = [vp, C.c_uint32, vp, sz]
    L.fa_raw_query_merge_stats.argtypes = [vp, C.POINTER(RawQueryMergeStats)]
    L.fa_group_raw_query_pending.argtypes = [vp, C.POINTER(RawQuery)]
    L.fa_group_raw_query_rows.argtypes = [vp, C.c_uint32, C.c_int, sz, vp, sz, szp]
    L.fa_group_raw_query_reset.argtypes = [vp]
    L.fa_raw_select_pending.argtypes = [vp, C.POINTER(RawFilter), vp, sz, szp, szp]
    L.fa_raw_pending_stats.argtypes = [vp, C.POINTER(RawPendingStats)]
    L.fa_raw_merge.argtypes = [vp]
    L.fa_raw_merge_stats.argtypes = [vp, C.POINTER(RawMergeStats)]
    _LIB = L
    return L


def mock_params(mode=MOCK_MOCKER, framed=1, seed=1, n_total=0, t0=T0, span_secs=900, per_sec=4,
                zipf_log2_universe=24, zipf_s_x100=110):
    return MockParams(mode, framed, seed, n_total, t0, span_secs, per_sec, zipf_log2_universe,
                      zipf_s_x100)


def mock_record_cap(mode: int) -> int:
    """Upper bound of the mean framed record size of a generator mode (buffer sizing)."""
    return 200 if mode == MOCK_GOFLOW else 96


def mock_generate_host(mp: MockParams, i0: int, n: int):
    """Host twin of the device producer -> (bytes uint8[], offsets uint64[n+1])."""
    buf = np.empty(n * mock_record_cap(mp.mode) + 256, dtype=np.uint8)
    off = np.empty(n + 1, dtype=np.uint64)
    w = C.c_uint64()
    rc = lib().fa_mock_generate_host(C.byref(mp), i0, n, buf.ctypes.data, buf.size,
                                     off.ctypes.data, C.byref(w))
    if rc:
        raise FlowAggError(rc, "fa_mock_generate_host")
    return buf[:w.value].copy(), off


def rows_to_rowbinary(rows: np.ndarray) -> bytes:
    """flows_5m rows -> `INSERT INTO flows_5m FORMAT RowBinary` payload (create.sh:70-90 column list)."""
    r = np.ascontiguousarray(rows, dtype=ROW5M_DTYPE)
    out = np.empty(len(r) * 70, dtype=np.uint8)
    n = C.c_size_t()
    rc = lib().fa_rows_to_rowbinary(r.ctypes.data, len(r), out.ctypes.data, out.size, C.byref(n))
    if rc:
        raise FlowAggError(rc, "fa_rows_to_rowbinary")
    return out[:n.value].tobytes()


def flow_rows_to_native(rows: np.ndarray) -> bytes:
    """Decoded rows of ONE Date (status 0, ascending 32-bit TimeReceived) -> one flows_raw part: a ClickHouse Native block for
    `INSERT INTO flows_raw FORMAT Native` (create.sh:36-62 column list).  Host code, no GPU."""
    r = np.ascontiguousarray(rows, dtype=FLOW_ROW_DTYPE)
    out = np.empty(lib().fa_raw_part_bytes(len(r)), dtype=np.uint8)
    n = C.c_size_t()
    rc = lib().fa_flow_rows_to_native(r.ctypes.data, len(r), out.ctypes.data, out.size, C.byref(n))
    if rc:
        raise FlowAggError(rc, "fa_flow_rows_to_native")
    return out[:n.value].tobytes()


def lz4_frame(data) -> bytes:
    """Bytes -> one LZ4 frame of the form raw_take_lz4 writes (independent 64 KiB blocks, no checksums): fa_lz4_frame, the
    host twin of the device encoder.  Host code, no GPU."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.empty(lib().fa_lz4_frame_bound(a.size), dtype=np.uint8)
    n = C.c_size_t()
    rc = lib().fa_lz4_frame(a.ctypes.data if a.size else None, a.size, out.ctypes.data, out.size, C.byref(n))
    if rc:
        raise FlowAggError(rc, "fa_lz4_frame")
    return out[:n.value].tobytes()


def lz4_decode(data) -> bytes:
    """A concatenation of LZ4 frames of the form the library writes -> their decoded bytes: fa_lz4_decode, the host twin of
    lz4_decode_device (the same per-sequence step function) and the C twin of spill.lz4_frames_decode.  No GPU, no ctx."""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    n = C.c_size_t()
    rc = lib().fa_lz4_decode(a.ctypes.data if a.size else None, a.size, None, 0, C.byref(n))
    if rc == 0:
        return b""
    if rc != -6:
        raise FlowAggError(rc, "fa_lz4_decode: not a concatenation of LZ4 frames the library reads")
    out = np.empty(n.value, dtype=np.uint8)
    rc = lib().fa_lz4_decode(a.ctypes.data, a.size, out.ctypes.data, out.size, C.byref(n))
    if rc:
        raise FlowAggError(rc, "fa_lz4_decode")
    return out[:n.value].tobytes()


def _host_bytes(data):
    return np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)


def format_addr(addr, etype: int) -> str:
    """The dashboards' address string (viz-ch.json:233,479): dotted IPv4 of the first four bytes when
    EType = 0x800, ClickHouse IPv6NumToString of the FixedString(16) otherwise."""
    a = bytes(addr)
    if len(a) != 16:
        raise ValueError("FixedString(16) expected")
    out = C.create_string_buffer(46)
    rc = lib().fa_format_addr(a, etype, out, 46)
    if rc:
        raise FlowAggError(rc, "fa_format_addr")
    return out.value.decode("ascii")


def rowbinary_to_rows(blob: bytes) -> np.ndarray:
    """Inverse of rows_to_rowbinary (plain Python decoder, for tests and offline checks)."""
    import struct
    out = []
    p = 0
    while p < len(blob):
        date, ts, sa, da = struct.unpack_from("<HIII", blob, p)
        p += 14
        arr = []
        for fmt, size in (("<I", 4), ("<Q", 8), ("<Q", 8), ("<Q", 8)):
            if blob[p] != 1:
                raise ValueError("ETypeMap arrays hold exactly one element")
            arr.append(struct.unpack_from(fmt, blob, p + 1)[0])
            p += 1 + size
        b, pk, c = struct.unpack_from("<QQQ", blob, p)
        p += 24
        if (b, pk, c) != tuple(arr[1:]):
            raise ValueError("ETypeMap values differ from the scalar columns")
        out.append((date, ts, sa, da, arr[0], 0, b, pk, c))
    return np.array(out, dtype=ROW5M_DTYPE)


_ROWBINARY_DTYPE = np.dtype([  # one flows_5m row of fa_rows_to_rowbinary (create.sh:70-90 column list), packed: 70 bytes
    ("date", "<u2"), ("timeslot", "<u4"), ("src_as", "<u4"), ("dst_as", "<u4"),
    ("n_etype", "u1"), ("m_etype", "<u4"), ("n_bytes", "u1"), ("m_bytes", "<u8"), ("n_packets", "u1"), ("m_packets", "<u8"), ("n_count", "u1"), ("m_count", "<u8"),
    ("bytes", "<u8"), ("packets", "<u8"), ("count", "<u8")])
assert _ROWBINARY_DTYPE.itemsize == 70


def rowbinary_to_rows_fast(blob) -> np.ndarray:
    """rowbinary_to_rows for large outputs (numpy, no Python loop): the rows of fa_rows_to_rowbinary all have the same shape
    (one element per ETypeMap array) - anything else raises."""
    b = np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else np.ascontiguousarray(blob, dtype=np.uint8)
    if b.size % 70:
        raise ValueError("not a whole number of 70-byte flows_5m RowBinary rows")
    r = b.view(_ROWBINARY_DTYPE)
    if not ((r["n_etype"] == 1) & (r["n_bytes"] == 1) & (r["n_packets"] == 1) & (r["n_count"] == 1)).all():
        raise ValueError("ETypeMap arrays hold exactly one element")
    if not ((r["m_bytes"] == r["bytes"]) & (r["m_packets"] == r["packets"]) & (r["m_count"] == r["count"])).all():
        raise ValueError("ETypeMap values differ from the scalar columns")
    out = np.zeros(len(r), dtype=ROW5M_DTYPE)
    for f in ("date", "timeslot", "src_as", "dst_as", "bytes", "packets", "count"):
        out[f] = r[f]
    out["etype"] = r["m_etype"]
    return out


def _rows_with_room(call, chk, dtype, cap, fresh=np.empty):
    """call(out, cap, n) -> rc fills a fresh array of `dtype` with room for `cap` rows and leaves the row count in n; on
    FA_ERR_CAPACITY (-6) n holds the rows needed and the call is made again with that much room.  -> the rows written."""
    n = C.c_size_t()
    while True:
        out = fresh(cap, dtype=dtype)
        rc = call(out, cap, n)
        if rc == -6:
            cap = n.value
            continue
        chk(rc)
        return out[:n.value]


NO_UPPER_BOUND = 0xFFFFFFFF  # t_hi of a talker or port range: to the end of the 32-bit time axis, its last bucket included


def _talker_range(t_lo, t_hi):
    return (0 if t_lo is None else int(t_lo)), (NO_UPPER_BOUND if t_hi is None else int(t_hi))


class FlowAgg:
    """One aggregation context = one (Kafka partition, GPU) pair."""

    def __init__(self, device=0, window_secs=300, subwindow_secs=0, table_capacity_log2=20,
                 key_sets=FA_KEYS_AS_PAIR, framed=True, cms_depth=4, cms_width_log2=20,
                 cms_seed=0x5EED, max_batch_records=0, topk_capacity_log2=0, wide_capacity_log2=0, topk_mode=0, topk_track=0):
        self._L = lib()
        self.cfg = Config(device, window_secs, subwindow_secs, table_capacity_log2, cms_depth,
                          cms_width_log2, cms_seed, key_sets, 1 if framed else 0, max_batch_records,
                          topk_capacity_log2, wide_capacity_log2, topk_mode, topk_track)
        h = C.c_void_p()
        rc = self._L.fa_create(C.byref(self.cfg), C.byref(h))
        if rc:
            raise FlowAggError(rc, (self._L.fa_last_error(None) or b"").decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.fa_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc:
            raise FlowAggError(rc, (self._L.fa_last_error(self._h) or b"").decode())

    # -- ingest ---------------------------------------------------------------
    def ingest(self, buf, offsets=None):
        """Host bytes (bytes / uint8 array) + uint64 offsets (n+1) or None (framed stream)."""
        b = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else \
            np.ascontiguousarray(buf, dtype=np.uint8)
        if offsets is None:
            self._chk(self._L.fa_ingest(self._h, b.ctypes.data, b.size, None, 0))
        else:
            o = np.ascontiguousarray(offsets, dtype=np.uint64)
            self._chk(self._L.fa_ingest(self._h, b.ctypes.data, b.size, o.ctypes.data, len(o) - 1))

    def ingest_device(self, d_buf_ptr: int, nbytes: int, d_off_ptr: int, n: int):
        """Device-resident batch: raw device pointers (e.g. torch tensor .data_ptr())."""
        self._chk(self._L.fa_ingest_device(self._h, d_buf_ptr, nbytes, d_off_ptr, n))

    def sync(self):
        self._chk(self._L.fa_sync(self._h))

    def reserve_ingest(self, nbytes: int, records: int):
        """Allocates the pinned staging slots (and their device twins) for host batches of up to nbytes / records now."""
        self._chk(self._L.fa_reserve_ingest(self._h, nbytes, records))

    # -- decode / projection -----------------------------------------------------
    def decode(self, buf, offsets) -> np.ndarray:
        b = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else \
            np.ascontiguousarray(buf, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(o) - 1
        out = np.zeros(n, dtype=FLOW_ROW_DTYPE)
        self._chk(self._L.fa_decode(self._h, b.ctypes.data, b.size, o.ctypes.data, n, out.ctypes.data))
        return out

    def decode_device(self, d_buf_ptr: int, nbytes: int, d_off_ptr: int, n: int) -> Columns:
        cols = Columns()
        self._chk(self._L.fa_decode_device(self._h, d_buf_ptr, nbytes, d_off_ptr, n, C.byref(cols)))
        return cols

    # -- window close ---------------------------------------------------------------
    def _rows_call(self, fn, timeslot, dtype=ROW5M_DTYPE):
        # one call in the common case: the table's group count bounds the rows of any window (a too small buffer
        # would make the library extract and sort the window a second time)
        st = self.stats()
        cap = max(1 << 12, int(st["table_used"] if dtype is ROW5M_DTYPE else st["wide_used"]))
        return _rows_with_room(lambda out, cap, n: fn(self._h, timeslot, out.ctypes.data, cap, C.byref(n)), self._chk, dtype, cap)

    def read_window(self, timeslot=ALL_TIMESLOTS) -> np.ndarray:
        return self._rows_call(self._L.fa_read_window, timeslot)

    def close_window(self, timeslot=ALL_TIMESLOTS) -> np.ndarray:
        return self._rows_call(self._L.fa_close_window, timeslot)

    def window_rows_device(self, timeslot=ALL_TIMESLOTS):
        """-> (device pointer, n): the window's rows sorted in HBM (valid until the ctx's next window / ingest call)."""
        p, n = C.c_void_p(), C.c_size_t()
        self._chk(self._L.fa_window_rows_device(self._h, timeslot, C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def merge_rows_device(self, d_rows_ptr: int, n: int):
        self._chk(self._L.fa_merge_rows_device(self._h, d_rows_ptr, n))

    # -- device-resident window close (ABI 5) -----------------------------------------------
    def rows_device(self, kind: int, timeslot=ALL_TIMESLOTS, k: int = 0):
        """-> (device pointer, n): this ctx's result for (kind, timeslot) as the matching read call returns it, left
        in HBM (valid until the ctx's next call)."""
        p, n = C.c_void_p(), C.c_size_t()
        self._chk(self._L.fa_rows_device(self._h, kind, timeslot, k, C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def rows_merge_device(self, kind: int, d_rows_ptr: int, n: int, k: int = 0):
        """Merges n rows in HBM (several ranks' rows_device results back to back) -> (device pointer, n) in emit order."""
        p, m = C.c_void_p(), C.c_size_t()
        self._chk(self._L.fa_rows_merge_device(self._h, kind, d_rows_ptr, n, k, C.byref(p), C.byref(m)))
        return p.value or 0, m.value

    def rows_fetch(self, kind: int, d_rows_ptr: int, n: int, out: np.ndarray | None = None) -> np.ndarray:
        """n rows of `kind` from HBM to the host (large results leave through the ctx's pinned buffer in pieces).  out: a
        buffer of the kind's dtype to reuse (a consumer keeps one per row kind: fresh pages cost more than the copy)."""
        if out is None or len(out) < n or out.dtype != ROW_DTYPES[kind]:
            out = np.empty(n, dtype=ROW_DTYPES[kind])
        if n:
            self._chk(self._L.fa_rows_fetch(self._h, kind, d_rows_ptr, n, out.ctypes.data, len(out)))
        return out[:n]

    @staticmethod
    def pinned_rows(kind: int, n: int) -> np.ndarray:
        """A row buffer of `kind` in page-locked host memory (torch's pinned allocator): fa_rows_fetch / the window reads then
        write into it with ONE copy-engine transfer instead of relaying through the ctx's pinned slots with host threads (57 against
        54 GB/s, and no host core busy)."""
        import torch
        dt = ROW_DTYPES[kind]
        t = torch.empty(max(n, 1) * dt.itemsize, dtype=torch.uint8, pin_memory=True)
        return t.numpy().view(dt)  # (the array keeps the tensor alive through .base)

    def rows_partition_device(self, kind: int, d_rows_ptr: int, n: int, world: int):
        """n rows in HBM regrouped by owning rank (hash of the key) -> (device pointer, counts per rank)."""
        p = C.c_void_p()
        counts = (C.c_size_t * world)()
        self._chk(self._L.fa_rows_partition_device(self._h, kind, d_rows_ptr, n, world, C.byref(p), counts))
        return p.value or 0, [int(x) for x in counts]

    def drop_window(self, kind: int, timeslot=ALL_TIMESLOTS):
        """Removes what close_window / close_window_app would remove after emitting `timeslot`."""
        self._chk(self._L.fa_drop_window(self._h, kind, timeslot))

    def drop_range(self, kind: int, timeslot_lo: int, timeslot_hi: int):
        """Removes every (sub-)bucket whose start lies in [timeslot_lo, timeslot_hi) in one pass (tumbling closes over sub-buckets)."""
        self._chk(self._L.fa_drop_range(self._h, kind, timeslot_lo, timeslot_hi))

    def open_timeslots(self) -> np.ndarray:
        return _rows_with_room(lambda out, cap, n: self._L.fa_open_timeslots(self._h, out.ctypes.data, cap, C.byref(n)), self._chk, np.uint32, 1 << 10, np.zeros).copy()

    def merge_rows(self, rows: np.ndarray):
        r = np.ascontiguousarray(rows, dtype=ROW5M_DTYPE)
        self._chk(self._L.fa_merge_rows(self._h, r.ctypes.data, len(r)))

    # -- second exact key set: (SrcAddr, DstPort, Proto) -------------------------------
    def read_window_app(self, timeslot=ALL_TIMESLOTS, out: np.ndarray | None = None) -> np.ndarray:
        # With pending log chunks the table's row count says nothing about the size of a window (and a too small buffer
        # makes the library collect and sort the window twice): the result is left in HBM first, then fetched.
        if out is None and self.stats()["wide_log_chunks"] == 0:
            return self._rows_call(self._L.fa_read_window_app, timeslot, ROW_APP_DTYPE)
        ptr, n = self.rows_device(ROWS_APP, timeslot)
        return self.rows_fetch(ROWS_APP, ptr, n, out=out)

    def close_window_app(self, timeslot=ALL_TIMESLOTS, out: np.ndarray | None = None) -> np.ndarray:
        if out is None and self.stats()["wide_log_chunks"] == 0:
            return self._rows_call(self._L.fa_close_window_app, timeslot, ROW_APP_DTYPE)
        rows = self.read_window_app(timeslot, out=out)
        self.drop_window(ROWS_APP, timeslot)
        return rows

    def read_window_app48(self, timeslot: int, out: np.ndarray | None = None, close=False):
        """ONE window's (SrcAddr,DstPort,Proto) rows without the date / timeslot they share: 48-byte rows -> (rows, date)."""
        fn = self._L.fa_close_window_app48 if close else self._L.fa_read_window_app48
        n, date = C.c_size_t(), C.c_uint32()
        cap = len(out) if out is not None else 1 << 12
        while True:  # (its own ask-again loop: a caller's buffer is reused when it has room, and the date is a second result)
            if out is None or len(out) < cap or out.dtype != ROW_APP48_DTYPE:
                out = np.empty(cap, dtype=ROW_APP48_DTYPE)
            rc = fn(self._h, timeslot, out.ctypes.data, len(out), C.byref(n), C.byref(date))
            if rc == -6:
                cap = n.value
                out = None
                continue
            self._chk(rc)
            return out[:n.value], date.value

    def merge_rows_app(self, rows: np.ndarray):
        r = np.ascontiguousarray(rows, dtype=ROW_APP_DTYPE)
        self._chk(self._L.fa_merge_rows_app(self._h, r.ctypes.data, len(r)))

    # -- dashboard read side -------------------------------------------------------------
    def top_ports(self, dst: int, k=1 << 32) -> np.ndarray:
        """GROUP BY SrcPort (dst=0) / DstPort (dst=1) ORDER BY sum(Bytes*SamplingRate) DESC, first k rows."""
        return _rows_with_room(lambda out, cap, n: self._L.fa_top_ports(self._h, dst, min(int(k), 1 << 40), out.ctypes.data, cap, C.byref(n)),
                               self._chk, PORT_ROW_DTYPE, 1 << 12, np.zeros).copy()

    def merge_ports(self, dst: int, rows: np.ndarray):
        r = np.ascontiguousarray(rows, dtype=PORT_ROW_DTYPE)
        self._chk(self._L.fa_merge_ports(self._h, dst, r.ctypes.data, len(r)))

    def minute_series(self) -> np.ndarray:
        return _rows_with_room(lambda out, cap, n: self._L.fa_minute_series(self._h, out.ctypes.data, cap, C.byref(n)), self._chk, MINUTE_ROW_DTYPE, 1 << 10, np.zeros).copy()

    def merge_minutes(self, rows: np.ndarray):
        r = np.ascontiguousarray(rows, dtype=MINUTE_ROW_DTYPE)
        self._chk(self._L.fa_merge_minutes(self._h, r.ctypes.data, len(r)))

    def dashboard_reset(self):
        self._chk(self._L.fa_dashboard_reset(self._h))

    # -- exact top talkers (opt-in second pass) ---------------------------------------------
    def talkers_enable(self, capacity_log2=0, bucket_secs=0):
        """From now on every ingest also folds its records' SrcAddr / DstAddr into two exact tables, grouped as the
        dashboards' top-talker panels group them (viz-ch.json:233,479).  bucket_secs > 0: the tables get a time axis
        (fa_talkers_enable_buckets) - top_talkers(t_lo, t_hi), talkers_buckets and talkers_drop_before work on it."""
        if bucket_secs:
            self._chk(self._L.fa_talkers_enable_buckets(self._h, capacity_log2, bucket_secs))
        else:
            self._chk(self._L.fa_talkers_enable(self._h, capacity_log2))

    def fold_columns_device(self, cols: Columns, n: int):
        """The same fold for columns that are already decoded (device pointers; src_addr, dst_addr, etype, bytes,
        sampling_rate and status are read)."""
        self._chk(self._L.fa_talkers_fold_columns_device(self._h, C.byref(cols), n))

    def top_talkers(self, dst: int, k: int = 0, t_lo=None, t_hi=None) -> np.ndarray:
        """GROUP BY the rendered SrcAddr (dst=0) / DstAddr (dst=1) ORDER BY sum(Bytes*SamplingRate) DESC, key bytes, etype:
        every group (k=0) or the first k.  format_addr(row["key"], row["etype"]) is the string the panel shows.
        t_lo / t_hi (a bucketed ctx): only the records with t_lo <= TimeFlowStart (32 bits) < t_hi; either one alone
        leaves the other end open (0 / NO_UPPER_BOUND)."""
        if t_lo is None and t_hi is None:
            call = lambda out, cap, n: self._L.fa_top_talkers(self._h, dst, int(k), out.ctypes.data, cap, C.byref(n))
        else:
            lo, hi = _talker_range(t_lo, t_hi)
            call = lambda out, cap, n: self._L.fa_top_talkers_range(self._h, dst, lo, hi, int(k), out.ctypes.data, cap, C.byref(n))
        return _rows_with_room(call, self._chk, TALKER_ROW_DTYPE, max(int(k), 1) if k else 1 << 12, np.zeros).copy()

    def talkers_range_rows_device(self, dst: int, t_lo=None, t_hi=None, k: int = 0):
        """-> (device pointer, n): top_talkers(dst, k, t_lo, t_hi) left in HBM (valid until the ctx's next call) - rows of
        kind ROWS_TALKERS_SRC / _DST for rows_partition_device / rows_merge_device."""
        lo, hi = _talker_range(t_lo, t_hi)
        p, n = C.c_void_p(), C.c_size_t()
        self._chk(self._L.fa_talkers_range_rows_device(self._h, dst, lo, hi, int(k), C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def talkers_buckets(self) -> np.ndarray:
        """The bucket starts held in either table, ascending."""
        return _rows_with_room(lambda out, cap, n: self._L.fa_talkers_buckets(self._h, out.ctypes.data, cap, C.byref(n)), self._chk, np.uint32, 1 << 10, np.zeros).copy()

    def talkers_drop_before(self, t: int):
        """Removes every bucket that starts below t (on the bucket grid).  Records below t that arrive later open their bucket again."""
        self._chk(self._L.fa_talkers_drop_before(self._h, int(t)))

    def merge_talkers(self, dst: int, rows: np.ndarray):
        r = np.ascontiguousarray(rows, dtype=TALKER_ROW_DTYPE)
        self._chk(self._L.fa_merge_talkers(self._h, dst, r.ctypes.data, len(r)))

    def merge_talkers_device(self, dst: int, d_rows_ptr: int, n: int):
        """merge_talkers for n rows that sit in HBM (another ctx's rows_device(ROWS_TALKERS_*) result, an exchanged share)."""
        self._chk(self._L.fa_merge_talkers_device(self._h, dst, d_rows_ptr, n))

    def talkers_reset(self):
        self._chk(self._L.fa_talkers_reset(self._h))

    def talkers_stats(self) -> dict:
        s = TalkersStats()
        self._chk(self._L.fa_talkers_stats(self._h, C.byref(s)))
        return s.as_dict()

    # -- exact top ports for a time range (opt-in, the same second pass) ---------------------
    def ports_enable_buckets(self, capacity_log2=0, bucket_secs=60):
        """From now on every ingest also folds its records' SrcPort / DstPort into two exact tables keyed by
        (bucket of TimeFlowStart, port) - what the port panels group by under $timeFilter (viz-ch.json:358,604).
        Independent of FA_KEYS_PORT_HIST and of the talkers; top_ports / merge_ports / dashboard_reset never see these tables."""
        self._chk(self._L.fa_ports_enable_buckets(self._h, capacity_log2, bucket_secs))

    def ports_fold_columns_device(self, cols: Columns, n: int):
        """The same fold for columns that are already decoded (device pointers; src_port, dst_port, bytes, sampling_rate,
        status and time_flow_start are read)."""
        self._chk(self._L.fa_ports_fold_columns_device(self._h, C.byref(cols), n))

    def top_ports_range(self, dst: int, k: int = 0, t_lo=None, t_hi=None) -> np.ndarray:
        """GROUP BY SrcPort (dst=0) / DstPort (dst=1) over the records with t_lo <= TimeFlowStart (32 bits) < t_hi, ORDER BY
        sum(Bytes*SamplingRate) DESC, port: every port (k=0) or the first k.  Either bound alone leaves the other end open."""
        lo, hi = _talker_range(t_lo, t_hi)
        call = lambda out, cap, n: self._L.fa_top_ports_range(self._h, dst, lo, hi, int(k), out.ctypes.data, cap, C.byref(n))
        return _rows_with_room(call, self._chk, PORT_ROW_DTYPE, max(int(k), 1) if k else 1 << 12, np.zeros).copy()

    def ports_range_rows_device(self, dst: int, t_lo=None, t_hi=None, k: int = 0):
        """-> (device pointer, n): top_ports_range(dst, k, t_lo, t_hi) left in HBM (valid until the ctx's next call) - rows of
        kind ROWS_PORT_SRC / _DST for rows_partition_device / rows_merge_device."""
        lo, hi = _talker_range(t_lo, t_hi)
        p, n = C.c_void_p(), C.c_size_t()
        self._chk(self._L.fa_ports_range_rows_device(self._h, dst, lo, hi, int(k), C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def ports_buckets(self) -> np.ndarray:
        """The bucket starts held in either port table, ascending."""
        return _rows_with_room(lambda out, cap, n: self._L.fa_ports_buckets(self._h, out.ctypes.data, cap, C.byref(n)), self._chk, np.uint32, 1 << 10, np.zeros).copy()

    def ports_drop_before(self, t: int):
        """Removes every bucket that starts below t (on the bucket grid).  Records below t that arrive later open their bucket again."""
        self._chk(self._L.fa_ports_drop_before(self._h, int(t)))

    def ports_reset(self):
        self._chk(self._L.fa_ports_reset(self._h))

    def ports_stats(self) -> dict:
        s = PortsStats()
        self._chk(self._L.fa_ports_stats(self._h, C.byref(s)))
        return s.as_dict()

    # -- flows_raw parts: sorted Native blocks per Date (opt-in, the same second pass) ---------
    def raw_enable(self, chunk_records=0):
        """From now on every ingest also builds flows_raw parts from its decoded columns: per chunk of at most chunk_records
        records (0: 2^20) one ClickHouse Native block per Date, rows in stable order of the 32-bit TimeReceived, malformed
        records dropped (create.sh:36-68).  The parts wait in HBM until raw_take."""
        self._chk(self._L.fa_raw_enable(self._h, chunk_records))

    def raw_build_columns(self, cols: Columns, n: int):
        """The same build for columns that are already decoded (device pointers; all 15 columns and status are read).
        Synchronous: the columns are not referenced after the call."""
        self._chk(self._L.fa_raw_build_columns_device(self._h, C.byref(cols), n))

    def raw_take(self, out: np.ndarray | None = None):
        """-> (bytes, parts): every pending part back to back, in build order - the payload of `INSERT INTO flows_raw FORMAT
        Native` - and their descriptions (RAW_PART_DTYPE: date, t_min, t_max, rows, offset, bytes); the pending parts are
        cleared.  out: a uint8 buffer to fill (page-locked: one copy-engine transfer); bytes is then a view of it."""
        nbytes, nparts = C.c_size_t(), C.c_size_t()
        st = self.raw_stats()
        cap, pcap = int(st["pending_bytes"]), max(int(st["pending_parts"]), 1)
        while True:  # (its own ask-again loop: two buffers, and a caller's byte buffer is reused when it has room)
            buf = out if out is not None and out.dtype == np.uint8 and out.size >= cap else np.empty(cap, dtype=np.uint8)
            parts = np.zeros(pcap, dtype=RAW_PART_DTYPE)
            rc = self._L.fa_raw_take(self._h, buf.ctypes.data if buf.size else None, buf.size, C.byref(nbytes), parts.ctypes.data, pcap, C.byref(nparts))
            if rc == -6:
                cap, pcap = nbytes.value, max(nparts.value, 1)
                continue
            self._chk(rc)
            data = buf[:nbytes.value]
            return (data if out is not None and buf is out else data.tobytes()), parts[:nparts.value]

    def raw_take_device(self):
        """-> (device pointer, bytes, parts): raw_take with the bytes left in HBM (valid until the ctx's next ingest / raw call)."""
        st = self.raw_stats()
        pcap = max(int(st["pending_parts"]), 1)
        parts = np.zeros(pcap, dtype=RAW_PART_DTYPE)
        p, nbytes, nparts = C.c_void_p(), C.c_size_t(), C.c_size_t()
        self._chk(self._L.fa_raw_take_device(self._h, C.byref(p), C.byref(nbytes), parts.ctypes.data, pcap, C.byref(nparts)))
        return p.value or 0, nbytes.value, parts[:nparts.value]

    def raw_take_lz4(self, out: np.ndarray | None = None):
        """raw_take with every part delivered as one LZ4 frame, compressed in HBM (include/flowagg.h "LZ4 frames of the flows_raw
        parts"): -> (bytes, parts); the bytes are a valid LZ4 stream, parts[i]'s offset / bytes describe its frame, which decodes
        to the part (spill.lz4_frames_decode)."""
        nbytes, nparts = C.c_size_t(), C.c_size_t()
        cap, pcap = 0, max(int(self.raw_stats()["pending_parts"]), 1)
        while True:  # (the first call learns the size: the frames are kept, the second call only copies)
            buf = out if out is not None and out.dtype == np.uint8 and out.size >= cap else np.empty(cap, dtype=np.uint8)
            parts = np.zeros(pcap, dtype=RAW_PART_DTYPE)
            rc = self._L.fa_raw_take_lz4(self._h, buf.ctypes.data if buf.size else None, buf.size, C.byref(nbytes), parts.ctypes.data, pcap, C.byref(nparts))
            if rc == -6:
                cap, pcap = nbytes.value, max(nparts.value, 1)
                continue
            self._chk(rc)
            data = buf[:nbytes.value]
            return (data if out is not None and buf is out else data.tobytes()), parts[:nparts.value]

    def raw_take_lz4_device(self):
        """-> (device pointer, bytes, parts): raw_take_lz4 with the frames left in HBM (valid until the ctx's next ingest, raw or lz4 call)."""
        pcap = max(int(self.raw_stats()["pending_parts"]), 1)
        parts = np.zeros(pcap, dtype=RAW_PART_DTYPE)
        p, nbytes, nparts = C.c_void_p(), C.c_size_t(), C.c_size_t()
        self._chk(self._L.fa_raw_take_lz4_device(self._h, C.byref(p), C.byref(nbytes), parts.ctypes.data, pcap, C.byref(nparts)))
        return p.value or 0, nbytes.value, parts[:nparts.value]

    def lz4_frame_device(self, d_in_ptr: int, n: int):
        """n bytes in HBM -> (device pointer, bytes) of ONE LZ4 frame in HBM (owned by the ctx, valid until its next ingest, raw or
        lz4 call).  Works without raw_enable."""
        p, nbytes = C.c_void_p(), C.c_size_t()
        self._chk(self._L.fa_lz4_frame_device(self._h, d_in_ptr or None, n, C.byref(p), C.byref(nbytes)))
        return p.value or 0, nbytes.value

    def raw_lz4_stats(self) -> dict:
        s = RawLz4Stats()
        self._chk(self._L.fa_raw_lz4_stats(self._h, C.byref(s)))
        return s.as_dict()

    # -- loading flows_raw parts back (include/flowagg.h "loading flows_raw parts") -------------
    def lz4_decode_device(self, data):
        """LZ4 frames in host memory -> (device pointer, spans): the decoded bytes in HBM (owned by the ctx, valid until its next
        load, lz4 or raw call) and one (offset, bytes) per frame (LZ4_SPAN_DTYPE; every offset a multiple of 65536)."""
        a = _host_bytes(data)
        p, nf = C.c_void_p(), C.c_size_t()
        cap = 16
        while True:  # (too few spans: the library's host walk says how many before anything is copied or decoded)
            spans = np.zeros(cap, dtype=LZ4_SPAN_DTYPE)
            rc = self._L.fa_lz4_decode_device(self._h, a.ctypes.data if a.size else None, a.size, C.byref(p), spans.ctypes.data, cap, C.byref(nf))
            if rc == -6:
                cap = nf.value
                continue
            self._chk(rc)
            return p.value or 0, spans[:nf.value]

    def raw_columns(self, data):
        """flows_raw parts (LZ4 frames, one part each, or plain Native blocks) -> (Columns, rows): every part unpacked into one
        column block in HBM, parts in input order, status 0, the two times zero-extended.  Valid until the ctx's next decode or
        load call.  No fold."""
        a = _host_bytes(data)
        cols, rows = Columns(), C.c_size_t()
        self._chk(self._L.fa_raw_columns_device(self._h, a.ctypes.data if a.size else None, a.size, C.byref(cols), C.byref(rows)))
        return cols, rows.value

    def raw_load(self, data):
        """Folds every part of `data` (what raw_take_lz4 or raw_take delivered) into every enabled fold of the ctx: the talkers,
        plain or bucketed, and the bucketed ports.  A refused input (FlowAggError -7) folds nothing."""
        a = _host_bytes(data)
        self._chk(self._L.fa_raw_load(self._h, a.ctypes.data if a.size else None, a.size))

    def raw_load_reset(self):
        """Releases the buffers of lz4_decode_device / raw_columns / raw_load (and of the LZ4 compressions); works without raw_enable."""
        self._chk(self._L.fa_raw_load_reset(self._h))

    def raw_load_stats(self) -> dict:
        s = RawLoadStats()
        self._chk(self._L.fa_raw_load_stats(self._h, C.byref(s)))
        return s.as_dict()

    # -- the rollups from columns and from parts (include/flowagg.h, the section of that name) ----
    def rollup_fold_columns(self, cols: Columns, n: int, key_sets: int = 0):
        """n decoded records (device pointers) into flows_5m and the exact dashboard key sets: what an ingest of the same records
        leaves.  key_sets: 0 = every exact key set of the ctx, or a subset of them (a sketch bit: FlowAggError -8).  Synchronous."""
        self._chk(self._L.fa_rollup_fold_columns_device(self._h, C.byref(cols) if cols is not None else None, n, key_sets))

    def raw_load_rollup(self, data, key_sets: int = 0, folds: bool = False):
        """Every part of `data` (what raw_take_lz4 or raw_take delivered) into flows_5m and the exact dashboard key sets;
        folds=True: also into the enabled talker and port folds, as raw_load does.  A refused input (FlowAggError -7) folds nothing."""
        a = _host_bytes(data)
        self._chk(self._L.fa_raw_load_rollup(self._h, a.ctypes.data if a.size else None, a.size, key_sets, 1 if folds else 0))

    def rollup_stats(self) -> dict:
        s = RollupStats()
        self._chk(self._L.fa_rollup_stats(self._h, C.byref(s)))
        return s.as_dict()

    # -- the sketches from columns and from parts (include/flowagg.h, the section of that name) ----
    def sketch_fold_columns(self, cols: Columns, n: int, key_sets: int = 0):
        """n decoded records (device pointers) into the address sketches and the distinct-address sets behind topk: what an ingest
        of the same records leaves.  key_sets: 0 = every sketch of the ctx, or a subset of them (any other bit: FlowAggError -1).
        In the candidates mode every chunk of at most max_batch_records is one batch.  Synchronous."""
        self._chk(self._L.fa_sketch_fold_columns_device(self._h, C.byref(cols) if cols is not None else None, n, key_sets))

    def raw_restore(self, data, key_sets: int = 0, folds: bool = False):
        """Every part of `data` (what raw_take_lz4 or raw_take delivered) into everything selected: key_sets = 0 is every key set
        of the ctx, exact ones and sketches alike, or a subset; folds=True: also the enabled talker and port folds.  Each chunk
        is unpacked once.  A refused input (FlowAggError -7) folds nothing."""
        a = _host_bytes(data)
        self._chk(self._L.fa_raw_restore(self._h, a.ctypes.data if a.size else None, a.size, key_sets, 1 if folds else 0))

    def sketch_fold_stats(self) -> dict:
        s = SketchFoldStats()
        self._chk(self._L.fa_sketch_fold_stats(self._h, C.byref(s)))
        return s.as_dict()

    # -- ranged loads of flows_raw parts (include/flowagg.h, the section of that name) ----
    def raw_range_probe(self, data, t_lo: int, t_hi: int, cap: int = None):
        """One RAW_RANGE_DTYPE entry per part of `data`, input order: date, rows and the rows [r_lo, r_hi) whose
        (uint32)TimeReceived lies in [t_lo, t_hi) (t_hi = 0xFFFFFFFF: to the end), t_min / t_max of those rows.  Only the blocks the
        headers and the TimeReceived columns of the parts selected by Date lie in are decoded; no fold.  An unsorted part or a row of
        another Date is FlowAggError -7.  cap: the entries there is room for (default: asked for first)."""
        a = _host_bytes(data)
        ptr = a.ctypes.data if a.size else None
        need = C.c_size_t()
        if cap is None:
            rc = self._L.fa_raw_range_probe(self._h, ptr, a.size, t_lo, t_hi, None, 0, C.byref(need))
            if rc == 0:  # (no part at all)
                return np.zeros(0, dtype=RAW_RANGE_DTYPE)
            if rc != -6:
                self._chk(rc)
            cap = need.value
        out = np.zeros(cap, dtype=RAW_RANGE_DTYPE)
        self._chk(self._L.fa_raw_range_probe(self._h, ptr, a.size, t_lo, t_hi, out.ctypes.data if cap else None, cap, C.byref(need)))
        return out[:need.value]

    def raw_restore_range(self, data, t_lo: int, t_hi: int, key_sets: int = 0, folds: bool = False):
        """raw_restore for the rows of `data` whose (uint32)TimeReceived lies in [t_lo, t_hi) (t_hi = 0xFFFFFFFF: to the end): the
        parts' sort key, not TimeFlowStart.  Only the blocks that hold those rows, the headers and the TimeReceived columns are decoded.
        A refused input (FlowAggError -7: also an unsorted part or a row of another Date) folds nothing."""
        a = _host_bytes(data)
        self._chk(self._L.fa_raw_restore_range(self._h, a.ctypes.data if a.size else None, a.size, t_lo, t_hi, key_sets, 1 if folds else 0))

    def raw_range_stats(self) -> dict:
        s = RawRangeStats()
        self._chk(self._L.fa_raw_range_stats(self._h, C.byref(s)))
        return s.as_dict()

    # -- selecting rows of flows_raw parts (include/flowagg.h, the section of that name) ----
    def raw_select(self, data, t_lo=0, t_hi=0xFFFFFFFF, *, flow_start=None, src_as=None, dst_as=None, etype=None, proto=None, src_port=None,
                   dst_port=None, src_net=None, dst_net=None, either=False, limit=0, count_only=False, out=None, filter=None):
        """-> (bytes, parts): the rows of `data` (what raw_take_lz4 or raw_take delivered) whose (uint32)TimeReceived lies in
        [t_lo, t_hi) and that meet every condition given, as one plain Native part per input part with a match, in input order, rows
        in the input's order (RAW_PART_DTYPE descriptions).  flow_start and the ports are (lo, hi) - the ports inclusive at both
        ends -, the nets (16 bytes, prefix_len); either: "between A and B in either direction"; limit: the first rows of the call;
        count_only: the descriptions alone, bytes is then b"".  out: a uint8 buffer to fill (page-locked: one copy-engine transfer);
        bytes is then a view of it.  filter: a RawFilter that stands for all the keywords.  A refused input is FlowAggError -7."""
        f = filter if filter is not None else raw_filter(t_lo, t_hi, flow_start=flow_start, src_as=src_as, dst_as=dst_as, etype=etype, proto=proto, src_port=src_port,
                                                         dst_port=dst_port, src_net=src_net, dst_net=dst_net, either=either, limit=limit, count_only=count_only)
        a = _host_bytes(data)
        ptr = a.ctypes.data if a.size else None
        nparts, nbytes = C.c_size_t(), C.c_size_t()
        pcap = 16
        while True:  # (too few descriptions: the library's host walk says how many before anything is copied)
            parts = np.zeros(pcap, dtype=RAW_PART_DTYPE)
            rc = self._L.fa_raw_select(self._h, ptr, a.size, C.byref(f), parts.ctypes.data, pcap, C.byref(nparts), C.byref(nbytes))
            if rc == -6:
                pcap = nparts.value
                continue
            self._chk(rc)
            break
        parts = parts[:nparts.value]
        if f.fields & RAW_F_COUNT_ONLY:
            return b"", parts
        buf = out if out is not None and out.dtype == np.uint8 and out.size >= nbytes.value else np.empty(nbytes.value, dtype=np.uint8)
        self._chk(self._L.fa_raw_selection_fetch(self._h, buf.ctypes.data if buf.size else None, buf.size, C.byref(nbytes)))
        sel = buf[:nbytes.value]
        return (sel if out is not None and buf is out else sel.tobytes()), parts

    def raw_selection_device(self):
        """-> (device pointer, bytes): the last raw_select's parts where they lie in HBM (0, 0 when there is none); valid until the
        ctx's next select, decode, load, restore or range call."""
        p, nbytes = C.c_void_p(), C.c_size_t()
        self._chk(self._L.fa_raw_selection_device(self._h, C.byref(p), C.byref(nbytes)))
        return p.value or 0, nbytes.value

    def raw_select_stats(self) -> dict:
        s = RawSelectStats()
        self._chk(self._L.fa_raw_select_stats(self._h, C.byref(s)))
        return s.as_dict()

    # -- grouped queries over flows_raw parts (include/flowagg.h, the section of that name) ----
    def raw_query(self, data, groups, t_lo=0, t_hi=0xFFFFFFFF, *, keep=False, filter=None, **conditions):
        """WHERE and one GROUP BY per RAW_G_* bit of `groups` over the rows of `data` (what raw_take_lz4 or raw_take delivered), all
        kinds in one pass; the result stays in HBM until the next raw_query without keep (read it with raw_query_rows).  The
        conditions are raw_filter's keywords (no limit, no count_only); filter: a RawFilter that stands for them and the time
        range.  keep: add to the result held.  A refused input is FlowAggError -7."""
        q = RawQuery()
        q.where = filter if filter is not None else raw_filter(t_lo, t_hi, **conditions)
        q.groups, q.flags = groups, RAW_Q_KEEP if keep else 0
        a = _host_bytes(data)
        self._chk(self._L.fa_raw_query(self._h, a.ctypes.data if a.size else None, a.size, C.byref(q)))

    def raw_query_rows(self, group, k=0, order=RAW_O_WEIGHT) -> np.ndarray:
        """QUERY_ROW_DTYPE rows of one kind of the last raw_query: every group (k = 0) or the first k in `order` (RAW_O_WEIGHT:
        weight descending; RAW_O_KEY: value, key bytes, etype ascending), ordered and cut on the device."""
        need = C.c_size_t()
        rc = self._L.fa_raw_query_rows(self._h, group, order, k, None, 0, C.byref(need))
        if rc != -6:
            self._chk(rc)
            return np.zeros(0, dtype=QUERY_ROW_DTYPE)
        out = np.zeros(need.value, dtype=QUERY_ROW_DTYPE)
        self._chk(self._L.fa_raw_query_rows(self._h, group, order, k, out.ctypes.data, out.size, C.byref(need)))
        return out[:need.value]

    def raw_query_rows_device(self, group, k=0, order=RAW_O_WEIGHT):
        """-> (device pointer, rows): raw_query_rows' rows where they lie in HBM (0, 0 when there is none); valid until the ctx's
        next query call."""
        p, n = C.c_void_p(), C.c_size_t()
        self._chk(self._L.fa_raw_query_rows_device(self._h, group, order, k, C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def raw_query_reset(self):
        self._chk(self._L.fa_raw_query_reset(self._h))

    def raw_query_stats(self) -> dict:
        s = RawQueryStats()
        self._chk(self._L.fa_raw_query_stats(self._h, C.byref(s)))
        return s.as_dict()

    def raw_query_merge(self, group, rows_or_device_ptr, n=None):
        """Adds rows of ONE kind to the result this ctx holds: another ctx's raw_query_rows(group, k=0) (a QUERY_ROW_DTYPE array),
        or its raw_query_rows_device pointer with n rows.  Every row is checked before any is added; afterwards raw_query_rows
        answers for both, and a later query with keep goes on adding."""
        if isinstance(rows_or_device_ptr, np.ndarray):
            rows = np.ascontiguousarray(rows_or_device_ptr, dtype=QUERY_ROW_DTYPE)
            m = len(rows) if n is None else int(n)
            self._chk(self._L.fa_raw_query_merge_rows(self._h, group, rows.ctypes.data if m else None, m))
        else:
            self._chk(self._L.fa_raw_query_merge_device(self._h, group, int(rows_or_device_ptr) or None, int(n or 0)))

    def raw_query_merge_stats(self) -> dict:
        s = RawQueryMergeStats()
        self._chk(self._L.fa_raw_query_merge_stats(self._h, C.byref(s)))
        return s.as_dict()

    # -- the pending parts as input (include/flowagg.h "the pending flows_raw parts as input") ----
    def raw_pending_probe(self, t_lo: int, t_hi: int) -> np.ndarray:
        """raw_range_probe over the ctx's pending parts, read where they lie in HBM: one RAW_RANGE_DTYPE entry per pending part,
        build order.  Nothing is copied, taken or changed."""
        need = C.c_size_t()
        cap = self.raw_stats()["pending_parts"]
        out = np.zeros(cap, dtype=RAW_RANGE_DTYPE)
        self._chk(self._L.fa_raw_pending_probe(self._h, t_lo, t_hi, out.ctypes.data if cap else None, cap, C.byref(need)))
        return out[:need.value]

    def raw_query_pending(self, groups, t_lo=0, t_hi=0xFFFFFFFF, *, keep=False, filter=None, **conditions):
        """raw_query over the ctx's pending parts, read where they lie in HBM; the result is read with raw_query_rows.
        keep: add to the result held - raw_query(bytes of older files) followed by raw_query_pending(keep=True) is one answer over
        stored and live rows.  The pending parts and the ctx's selection stay as they are."""
        q = RawQuery()
        q.where = filter if filter is not None else raw_filter(t_lo, t_hi, **conditions)
        q.groups, q.flags = groups, RAW_Q_KEEP if keep else 0
        self._chk(self._L.fa_raw_query_pending(self._h, C.byref(q)))

    def raw_select_pending(self, t_lo=0, t_hi=0xFFFFFFFF, *, flow_start=None, src_as=None, dst_as=None, etype=None, proto=None, src_port=None,
                           dst_port=None, src_net=None, dst_net=None, either=False, limit=0, count_only=False, out=None, filter=None):
        """-> (bytes, parts): raw_select over the ctx's pending parts, read where they lie in HBM: one plain Native part per pending
        part with a match, build order.  The keywords and the return are raw_select's.  The pending parts stay as they are; the
        selection is a copy and replaces the ctx's selection."""
        f = filter if filter is not None else raw_filter(t_lo, t_hi, flow_start=flow_start, src_as=src_as, dst_as=dst_as, etype=etype, proto=proto, src_port=src_port,
                                                         dst_port=dst_port, src_net=src_net, dst_net=dst_net, either=either, limit=limit, count_only=count_only)
        nparts, nbytes = C.c_size_t(), C.c_size_t()
        pcap = 16
        while True:  # (too few descriptions: the library says how many before anything is launched)
            parts = np.zeros(pcap, dtype=RAW_PART_DTYPE)
            rc = self._L.fa_raw_select_pending(self._h, C.byref(f), parts.ctypes.data, pcap, C.byref(nparts), C.byref(nbytes))
            if rc == -6:
                pcap = nparts.value
                continue
            self._chk(rc)
            break
        parts = parts[:nparts.value]
        if f.fields & RAW_F_COUNT_ONLY:
            return b"", parts
        buf = out if out is not None and out.dtype == np.uint8 and out.size >= nbytes.value else np.empty(nbytes.value, dtype=np.uint8)
        self._chk(self._L.fa_raw_selection_fetch(self._h, buf.ctypes.data if buf.size else None, buf.size, C.byref(nbytes)))
        sel = buf[:nbytes.value]
        return (sel if out is not None and buf is out else sel.tobytes()), parts

    def raw_pending_stats(self) -> dict:
        s = RawPendingStats()
        self._chk(self._L.fa_raw_pending_stats(self._h, C.byref(s)))
        return s.as_dict()

    def raw_reset(self):
        self._chk(self._L.fa_raw_reset(self._h))

    def raw_stats(self) -> dict:
        s = RawStats()
        self._chk(self._L.fa_raw_stats(self._h, C.byref(s)))
        return s.as_dict()

    # -- merging the pending parts (include/flowagg.h "merging the pending flows_raw parts") ----
    def raw_merge(self):
        """Replaces the pending parts by one part per Date, rows in stable t32 order over the parts laid end to end: the bytes
        ONE chunk holding all those records would have built.  The takes deliver the merged parts."""
        self._chk(self._L.fa_raw_merge(self._h))

    def raw_merge_stats(self) -> dict:
        s = RawMergeStats()
        self._chk(self._L.fa_raw_merge_stats(self._h, C.byref(s)))
        return s.as_dict()

    # -- sketches -------------------------------------------------------------------
    def cms_read(self, key_set) -> np.ndarray:
        words = self.cfg.cms_depth << self.cfg.cms_width_log2
        out = np.zeros(words, dtype=np.uint64)
        self._chk(self._L.fa_cms_read(self._h, key_set, out.ctypes.data, words))
        return out.reshape(self.cfg.cms_depth, -1)

    def cms_query(self, key_set, key: bytes) -> int:
        w = C.c_uint64()
        self._chk(self._L.fa_cms_query(self._h, key_set, key, C.byref(w)))
        return w.value

    def cms_reset(self, key_set):
        self._chk(self._L.fa_cms_reset(self._h, key_set))

    def topk(self, key_set, k) -> np.ndarray:
        """k heaviest addresses by Count-Min estimate of sum(Bytes*SamplingRate): (key, weight) rows."""
        k = min(int(k), 1 << (self.cfg.topk_capacity_log2 or 20))
        out = np.zeros(k, dtype=TOPK_DTYPE)
        n = C.c_size_t()
        self._chk(self._L.fa_topk(self._h, key_set, k, out.ctypes.data, k, C.byref(n)))
        return out[:n.value].copy()

    def topk_merge_keys(self, key_set, keys: np.ndarray):
        """Adds candidate keys (uint8[n,16]) found by other contexts / ranks."""
        kk = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 16)
        self._chk(self._L.fa_topk_merge_keys(self._h, key_set, kk.ctypes.data, len(kk)))

    def device_state(self) -> DeviceState:
        st = DeviceState()
        self._chk(self._L.fa_device_state_get(self._h, C.byref(st)))
        return st

    def merged_view_set(self, valid: bool):
        """Declare the merged sketch view (device_state().cms_*_merged) valid / stale."""
        self._chk(self._L.fa_merged_view_set(self._h, 1 if valid else 0))

    def merge_allreduce(self, rccl_comm_ptr: int):
        """In-library RCCL path: ncclAllReduce of the sketches into the merged view (out of place, idempotent)."""
        self._chk(self._L.fa_merge_allreduce(self._h, rccl_comm_ptr))

    def stats(self) -> dict:
        s = Stats()
        self._chk(self._L.fa_stats(self._h, C.byref(s)))
        return s.as_dict()

    # -- synthetic producer ------------------------------------------------------------
    def mock_generate_device(self, mp: MockParams, i0: int, n: int, d_buf_ptr: int, cap: int,
                             d_off_ptr: int) -> int:
        w = C.c_uint64()
        self._chk(self._L.fa_mock_generate_device(self._h, C.byref(mp), i0, n, d_buf_ptr, cap,
                                                  d_off_ptr, C.byref(w)))
        return w.value


class FlowGroup:
    """The window close of several contexts inside ONE process (ABI 7+, fa_group_*): one FlowAgg per (Kafka partition, GPU),
    results merged in HBM.  The multi-process twin is flow-pipeline_amd.dist (one rank per GPU under torchrun)."""

    def __init__(self, members, transport=GROUP_PEER):
        self._L = lib()
        self.members = list(members)
        arr = (C.c_void_p * len(self.members))(*[m._h for m in self.members])
        h = C.c_void_p()
        rc = self._L.fa_group_create(arr, len(self.members), transport, C.byref(h))
        if rc:
            raise FlowAggError(rc, (self._L.fa_group_last_error(None) or b"").decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.fa_group_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc:
            raise FlowAggError(rc, (self._L.fa_group_last_error(self._h) or b"").decode())

    @property
    def transport(self) -> int:
        return self._L.fa_group_transport(self._h)

    def _rows(self, call, kind, cap=1 << 12):
        return _rows_with_room(call, self._chk, ROW_DTYPES[kind], cap)

    def open_timeslots(self) -> np.ndarray:
        return _rows_with_room(lambda out, cap, n: self._L.fa_group_open_timeslots(self._h, out.ctypes.data, cap, C.byref(n)), self._chk, np.uint32, 1 << 10, np.zeros).copy()

    def read_window(self, kind=ROWS_5M, timeslot=ALL_TIMESLOTS, k=0, cap=1 << 12) -> np.ndarray:
        return self._rows(lambda out, c, n: self._L.fa_group_read_window(self._h, kind, timeslot, k, out.ctypes.data, c, C.byref(n)), kind, cap)

    def close_window(self, kind=ROWS_5M, timeslot=ALL_TIMESLOTS, cap=1 << 12) -> np.ndarray:
        return self._rows(lambda out, c, n: self._L.fa_group_close_window(self._h, kind, timeslot, out.ctypes.data, c, C.byref(n)), kind, cap)

    def _part(self, fn, kind, timeslot, cap):
        shares = (C.c_size_t * len(self.members))()
        rows = self._rows(lambda out, c, n: fn(self._h, kind, timeslot, out.ctypes.data, c, shares, C.byref(n)), kind, cap)
        return rows, [int(v) for v in shares]

    def read_window_partitioned(self, kind=ROWS_APP, timeslot=ALL_TIMESLOTS, cap=1 << 12):
        """-> (rows, share sizes): the members' shares back to back, share 0 first; a key lives in exactly one share."""
        return self._part(self._L.fa_group_read_window_partitioned, kind, timeslot, cap)

    def close_window_partitioned(self, kind=ROWS_APP, timeslot=ALL_TIMESLOTS, cap=1 << 12):
        return self._part(self._L.fa_group_close_window_partitioned, kind, timeslot, cap)

    def allreduce_sketches(self):
        self._chk(self._L.fa_group_allreduce_sketches(self._h))

    def topk(self, key_set, k) -> np.ndarray:
        out = np.zeros(max(int(k), 1), dtype=TOPK_DTYPE)
        n = C.c_size_t()
        self._chk(self._L.fa_group_topk(self._h, key_set, int(k), out.ctypes.data, len(out), C.byref(n)))
        return out[:n.value].copy()

    def top_talkers(self, dst: int, k: int = 0, cap=None, t_lo=None, t_hi=None) -> np.ndarray:
        """FlowAgg.top_talkers of ONE ctx that folded every member's partition, byte for byte: exact, merged in HBM.
        t_lo / t_hi: FlowAgg.top_talkers' range (every member bucketed, with one bucket_secs)."""
        kind = ROWS_TALKERS_DST if dst else ROWS_TALKERS_SRC
        cap = cap if cap is not None else (max(int(k), 1) if k else 1 << 12)
        if t_lo is None and t_hi is None:
            return self._rows(lambda out, c, n: self._L.fa_group_top_talkers(self._h, dst, int(k), out.ctypes.data, c, C.byref(n)), kind, cap)
        lo, hi = _talker_range(t_lo, t_hi)
        return self._rows(lambda out, c, n: self._L.fa_group_top_talkers_range(self._h, dst, lo, hi, int(k), out.ctypes.data, c, C.byref(n)), kind, cap)

    def top_ports_range(self, dst: int, k: int = 0, cap=None, t_lo=None, t_hi=None) -> np.ndarray:
        """FlowAgg.top_ports_range of ONE ctx that folded every member's partition (every member enabled, with one bucket_secs)."""
        kind = ROWS_PORT_DST if dst else ROWS_PORT_SRC
        cap = cap if cap is not None else (max(int(k), 1) if k else 1 << 12)
        lo, hi = _talker_range(t_lo, t_hi)
        return self._rows(lambda out, c, n: self._L.fa_group_top_ports_range(self._h, dst, lo, hi, int(k), out.ctypes.data, c, C.byref(n)), kind, cap)

    def raw_query_pending(self, groups, t_lo=0, t_hi=0xFFFFFFFF, *, keep=False, filter=None, **conditions):
        """FlowAgg.raw_query_pending on every member (each needs raw_enable); keep is passed through per member.  Read the answer
        over the whole topic with raw_query_rows."""
        q = RawQuery()
        q.where = filter if filter is not None else raw_filter(t_lo, t_hi, **conditions)
        q.groups, q.flags = groups, RAW_Q_KEEP if keep else 0
        self._chk(self._L.fa_group_raw_query_pending(self._h, C.byref(q)))

    def raw_query_rows(self, group, k=0, order=RAW_O_WEIGHT, cap=None) -> np.ndarray:
        """FlowAgg.raw_query_rows of ONE ctx whose result covers what every member holds, byte for byte: exact, merged in HBM, k
        rows cross PCIe.  The members' results are not changed."""
        cap = cap if cap is not None else (max(int(k), 1) if k else 1 << 12)
        return _rows_with_room(lambda out, c, n: self._L.fa_group_raw_query_rows(self._h, group, order, int(k), out.ctypes.data, c, C.byref(n)), self._chk, QUERY_ROW_DTYPE, cap,
                               np.zeros)

    def raw_query_reset(self):
        self._chk(self._L.fa_group_raw_query_reset(self._h))

    def stats(self) -> dict:
        s = Stats()
        self._chk(self._L.fa_group_stats(self._h, C.byref(s)))
        return s.as_dict()
