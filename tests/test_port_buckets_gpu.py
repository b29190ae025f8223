"""GPU parity of the bucketed port tables (fa_ports_enable_buckets, fa_top_ports_range, fa_ports_range_rows_device,
fa_ports_fold_columns_device, fa_ports_buckets, fa_ports_drop_before, fa_ports_reset, fa_ports_stats, fa_group_top_ports_range,
dist.top_ports_merged(t_lo, t_hi); include/flowagg.h "ABI 8, addition: exact top ports for a time range").
Expected rows are never taken from the code under test: they are po.top_ports(rows[in_range], status[in_range], dst) on the
oracle's decode (po.decode_batch) or on hand-made columns, with the in_range filter on time_flow_start & 0xFFFFFFFF that
tests/test_talker_buckets_gpu.py states.  Every comparison is np.array_equal on port, weight and count."""
import ctypes as C
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = ("port", "weight", "count")
NO_UPPER = 0xFFFFFFFF
ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -6, -8
SENTINEL = 0x5A5A5A5A
PORT_COLUMNS = ("src_port", "dst_port", "bytes", "sampling_rate", "status", "time_flow_start")


def _same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for c in COLS:
        assert np.array_equal(got[c], want[c]), (c, np.nonzero(got[c] != want[c])[0][:10])


def t32_of(rows):
    return (rows["time_flow_start"] & np.uint64(0xFFFFFFFF)).astype(np.uint64)


def in_range(rows, t_lo, t_hi):
    """t_lo <= t32 < t_hi; t_hi = 0xFFFFFFFF: no upper bound; t_lo == t_hi: nothing."""
    t = t32_of(rows)
    if t_lo == t_hi:
        return np.zeros(len(rows), dtype=bool)
    m = t >= np.uint64(t_lo)
    return m if t_hi == NO_UPPER else m & (t < np.uint64(t_hi))


def restate(po, rows, status, dst, t_lo=0, t_hi=NO_UPPER, k=0):
    m = in_range(rows, t_lo, t_hi)
    out = po.top_ports(rows[m], status[m], dst)
    return out[:k] if k else out


def pairs(po, rows, status, dst, bs, t_floor=0):
    """the number of (bucket, port) groups: what used[dst] counts"""
    r = rows[(status == 0) & (t32_of(rows) >= np.uint64(t_floor))]
    t = t32_of(r)
    idx, _ = po._group_sum([t - t % np.uint64(bs), r["dst_port" if dst else "src_port"].astype(np.uint64)], [np.ones(len(r), dtype=np.uint64)])
    return len(idx)


def buckets_of(rows, status, bs):
    t = t32_of(rows[status == 0])
    return np.unique(t - t % np.uint64(bs)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _stream(mode, n, seed, zs=110, lu=24):
    """One generated framed stream and its decode - computed once, shared, read-only."""
    import _pkg
    po = _pkg.load_oracle()
    gp = po.gen_params(mode=mode, framed=1, seed=seed, n_total=n, span_secs=900, per_sec=60, zipf_s_x100=zs, zipf_log2_universe=lu)
    buf, off = po.gen_records(gp, 0, n)
    rows, status = po.decode_batch(buf, off, 1)
    assert int(status.sum()) == 0
    for a in (buf, off, rows, status):
        a.setflags(write=False)
    return buf, off, rows, status


def check_ranges(po, agg, rows, status, ranges, ks=(0,), dirs=(0, 1)):
    for t_lo, t_hi in ranges:
        for d in dirs:
            want = restate(po, rows, status, d, t_lo, t_hi)  # (once per range: k only cuts)
            for k in ks:
                _same(agg.top_ports_range(d, k, t_lo, t_hi), want[:k] if k else want)


def err(fa, agg):
    return (fa.lib().fa_last_error(agg._h) or b"").decode()


def _fold(fa, agg, rows, status, leave_out=None, shift=None):
    """Hand-made columns: the six columns the fold reads, uploaded with the dtypes of tests/device_columns.py."""
    import torch
    from device_columns import COLUMNS
    dtypes = {name: dt for name, dt, _ in COLUMNS}
    n = len(rows)
    keep, cols = [], fa.Columns()
    for name in PORT_COLUMNS:
        a = np.ascontiguousarray((status if name == "status" else rows[name]).astype(dtypes[name]))
        t = torch.zeros(max(n, 1) * a.dtype.itemsize + 16, dtype=torch.uint8, device="cuda")
        if n:
            t[:a.nbytes].copy_(torch.from_numpy(a.view(np.uint8).copy()))
        keep.append(t)
        if name != leave_out:
            setattr(cols, name, t.data_ptr() + (shift[1] if shift and shift[0] == name else 0))
    try:
        agg.ports_fold_columns_device(cols, n)
    finally:
        agg.sync()  # (the tensors may go once the stream has read them)


# ---- generated streams, bucket_secs = 60, tables that start at 2^8 slots ---------------------------------------------------------
@pytest.mark.parametrize("mode,seed", [(0, 71), (2, 72)], ids=["mocker", "zipf"])
def test_stream_every_bucket_prefix_and_suffix(gpu_lib, fa, po, mode, seed):
    n, T0 = 20000, po.T0
    buf, off, rows, status = _stream(mode, n, seed, zs=110, lu=16)
    starts = [int(b) for b in buckets_of(rows, status, 60)]
    assert len(starts) >= 5 and starts[0] == T0
    with fa.FlowAgg(framed=True) as none, fa.FlowAgg(framed=True) as agg:
        agg.ports_enable_buckets(8, 60)
        for x in (none, agg):
            x.ingest(buf, off)
        ranges = [(b, b + 60) for b in starts] + [(T0, b + 60) for b in starts] + [(b, NO_UPPER) for b in starts]
        ranges += [(0, NO_UPPER), (T0 + 120, T0 + 120), (starts[-1] + 60, starts[-1] + 600)]
        check_ranges(po, agg, rows, status, ranges, ks=(0, 1, 100))
        for d in (0, 1):
            assert len(agg.top_ports_range(d, 0, T0 + 120, T0 + 120)) == 0 and len(agg.top_ports_range(d, 0, starts[-1] + 60, NO_UPPER)) == 0
            ptr, m = agg.ports_range_rows_device(d, T0 + 60, T0 + 180, 100)
            _same(agg.rows_fetch(fa.ROWS_PORT_SRC + d, ptr, m), restate(po, rows, status, d, T0 + 60, T0 + 180, 100))
        assert np.array_equal(agg.ports_buckets(), buckets_of(rows, status, 60))
        ps = agg.ports_stats()
        assert ps["used"] == [pairs(po, rows, status, d, 60) for d in (0, 1)]
        assert ps["grows"] >= 4 and ps["records_folded"] == n and all(c >= 2 * u for c, u in zip(ps["capacity"], ps["used"]))
        assert agg.read_window().tobytes() == none.read_window().tobytes()  # flows_5m beside a ctx that did not enable


# ---- hand-made columns -------------------------------------------------------------------------------------------------------------
EDGE_PORTS = np.array([0, 1, 65535, 65536, 0xFFFFFFFF, 70000, 443], dtype=np.uint32)


def _handmade(po, n, seed, bs):
    """The first records are fixed (as many as fit): (index 0, port 0) beside (the last index, port 0xFFFFFFFF), a large port in
    two neighbouring buckets, a malformed record between good ones, a time with high bits; the rest is drawn from the edges."""
    rng = np.random.default_rng(seed)
    T0 = po.T0
    last = 0xFFFFFFFF  # (t32 of the axis' last second: index 0xFFFFFFFF with bucket_secs = 1)
    times = np.array([0, bs - 1, T0, T0 + bs - 1, T0 + bs, T0 + 2 * bs, last - bs, last], dtype=np.uint64)
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    rows["src_port"] = rng.choice(EDGE_PORTS, size=n)
    rows["dst_port"] = rng.choice(EDGE_PORTS, size=n)
    rows["bytes"] = rng.integers(0, 1 << 62, size=n, dtype=np.uint64) * np.uint64(5)  # x 2^30 below: sums wrap mod 2^64
    rows["sampling_rate"] = rng.choice(np.array([0, 1, 1000, 1 << 30], dtype=np.uint64), size=n)
    t = rng.choice(times, size=n)
    t += rng.integers(0, 3, size=n).astype(np.uint64) << np.uint64(32)  # the narrowing: high words that must not matter
    rows["time_flow_start"] = t
    status = (rng.random(n) < 0.1).astype(np.uint32)
    fixed = [(0, 0xFFFFFFFF, 0, 0), (0xFFFFFFFF, 0, last, 0), (65536, 65536, T0, 0), (7, 7, 12345, 1), (65536, 65536, T0 + bs, 0),
             (1, 1, (7 << 32) | T0, 0), (0xFFFFFFFF, 0xFFFFFFFF, last, 0), (0, 0, 0, 0)]
    for i, (sp, dp, tt, st) in enumerate(fixed[:n]):
        rows["src_port"][i], rows["dst_port"][i], rows["time_flow_start"][i], status[i] = sp, dp, tt, st
    rows["sampling_rate"][(rows["src_port"] == 1) | (rows["dst_port"] == 1)] = 0  # port 1: every weight 0 in both directions - still a row
    bad = status != 0
    rows["time_flow_start"][bad] = rng.integers(0, 1 << 63, size=int(bad.sum()), dtype=np.uint64)  # malformed rows carry garbage
    rows["src_port"][bad] = 31337
    return rows, status


@pytest.mark.parametrize("bs", [1, 60])
def test_handmade_columns_edges(gpu_lib, fa, po, bs):
    B, T0 = fa.PORT_BLOCK, po.T0
    last = 0xFFFFFFFF // bs * bs  # the start of the axis' last bucket: reached only through t_hi = 0xFFFFFFFF
    ranges = [(0, NO_UPPER), (0, bs), (T0, T0 + 2 * bs), (T0, T0 + bs), (T0 + bs, T0 + bs), (0, last), (last - bs, NO_UPPER),
              (last if bs > 1 else last - 1, NO_UPPER), (T0 + 2 * bs, last)]
    with fa.FlowAgg(framed=True) as agg:
        agg.ports_enable_buckets(8, bs)
        for n in (1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 3):
            rows, status = _handmade(po, n, 200 + n, bs)
            agg.ports_reset()
            _fold(fa, agg, rows, status)
            check_ranges(po, agg, rows, status, ranges)
            check_ranges(po, agg, rows, status, ranges[:3], ks=(1, 3))
            assert np.array_equal(agg.ports_buckets(), buckets_of(rows, status, bs))
            assert agg.ports_stats()["used"] == [pairs(po, rows, status, d, bs) for d in (0, 1)]
            if n >= 63:  # what the cases above are there for, stated on the restatement
                w = restate(po, rows, status, 0)
                assert {0, 1, 65535, 65536, 0xFFFFFFFF} <= set(int(p) for p in w["port"])
                assert (w["weight"][w["port"] == 1] == 0).all() and (w["count"][w["port"] == 1] > 0).all()
                two = restate(po, rows, status, 0, T0, T0 + 2 * bs)
                one = restate(po, rows, status, 0, T0, T0 + bs)
                assert int(two["count"][two["port"] == 65536][0]) > int(one["count"][one["port"] == 65536][0])  # the merge folded two buckets' rows
                assert (t32_of(rows[status == 0]) == 0xFFFFFFFF).any() and (rows["time_flow_start"][status == 0] >> np.uint64(32)).any()
                assert 31337 not in w["port"]
                big = rows[(status == 0) & (rows["src_port"] == 0)]
                exact = sum(int(b) * int(s) for b, s in zip(big["bytes"], big["sampling_rate"]))
                assert exact >= 1 << 64 and int(w["weight"][w["port"] == 0][0]) == exact % (1 << 64)  # a sum that wrapped
            if n >= 8 and bs == 1:  # (index 0, port 0) and (index 0xFFFFFFFF, port 0xFFFFFFFF) in one table
                first = agg.top_ports_range(0, 0, 0, 1)
                tail = agg.top_ports_range(0, 0, 0xFFFFFFFE, NO_UPPER)
                assert 0 in first["port"] and 0xFFFFFFFF in tail["port"]
                assert len(agg.top_ports_range(0, 0, 0xFFFFFFFF, NO_UPPER)) == 0  # (bucket_secs = 1: t_lo == t_hi is the empty range)


def test_thousand_ports_of_equal_weight_order_by_port(gpu_lib, fa, po):
    n, T0 = 1000, po.T0
    rows = np.zeros(3 * n, dtype=po.ROW_DTYPE)
    ports = (65000 + np.arange(n, dtype=np.uint32))[np.random.default_rng(5).permutation(n)]  # both sides of 65536
    rows["src_port"] = np.tile(ports, 3)
    rows["dst_port"] = np.tile(ports[::-1], 3)
    rows["bytes"], rows["sampling_rate"] = 100, 3
    rows["time_flow_start"] = np.uint64(T0) + np.repeat(np.arange(3, dtype=np.uint64), n) * np.uint64(60)
    status = np.zeros(len(rows), dtype=np.uint32)
    with fa.FlowAgg(framed=True) as agg:
        agg.ports_enable_buckets(8, 60)
        _fold(fa, agg, rows, status)
        for d in (0, 1):
            got = agg.top_ports_range(d, 0, T0, T0 + 180)
            assert np.array_equal(got["port"], 65000 + np.arange(n, dtype=np.uint32)) and (got["weight"] == 900).all() and (got["count"] == 3).all()
        check_ranges(po, agg, rows, status, [(0, NO_UPPER), (T0 + 60, T0 + 120)], ks=(0, 10))


# ---- the two paths of the fold: the LDS cache and the global table ---------------------------------------------------------------
def test_every_record_on_one_key_is_absorbed(gpu_lib, fa, po):
    n, T0 = 100000, po.T0
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    rows["src_port"], rows["dst_port"] = 443, 70000
    rows["bytes"], rows["sampling_rate"] = (1 << 63) + 3, 1 << 30
    rows["time_flow_start"] = T0 + 7
    status = np.zeros(n, dtype=np.uint32)
    with fa.FlowAgg(framed=True) as agg:
        agg.ports_enable_buckets(8, 60)
        _fold(fa, agg, rows, status)
        ps = agg.ports_stats()
        # every (record, direction) update ended in a cache; the table saw the flushes alone
        assert ps["records_absorbed"] == 2 * n and ps["used"] == [1, 1] and ps["records_folded"] == n
        check_ranges(po, agg, rows, status, [(0, NO_UPPER), (T0, T0 + 60), (T0 + 60, T0 + 120)])
        got = agg.top_ports_range(1, 0, T0, T0 + 60)
        assert len(got) == 1 and int(got["count"][0]) == n and int(got["weight"][0]) == (((1 << 63) + 3) * (1 << 30) * n) % (1 << 64)


def test_all_distinct_keys_overflow_every_cache_and_grow(gpu_lib, fa, po):
    """Distinct (bucket, port) keys numbering four times the LDS entries of every workgroup a launch can hold, per chunk: most
    updates take the global path, and the tables grow inside the call."""
    import torch
    T0 = po.T0
    wgs = torch.cuda.get_device_properties(0).multi_processor_count * fa.PORT_WG_PER_CU
    chunk = 4 * fa.PORT_LDS_ENTRIES * wgs  # 2^20 on 256 CUs
    log2 = int(np.log2(chunk)) + 2  # (a chunk is at most capacity / 4)
    assert 1 << (log2 - 2) == chunk and log2 <= 24
    n = 2 * chunk + 65536  # the third chunk finds the tables half full: they double
    i = np.arange(n, dtype=np.uint64)
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    rows["src_port"] = (i % np.uint64(65536)).astype(np.uint32)
    rows["dst_port"] = (np.uint64(65536) + i % np.uint64(65536)).astype(np.uint32)  # the same count of keys on the large-port side
    rows["bytes"] = i + np.uint64(1)
    rows["sampling_rate"] = 2
    rows["time_flow_start"] = np.uint64(T0) + (i // np.uint64(65536)) * np.uint64(60)
    status = np.zeros(n, dtype=np.uint32)
    with fa.FlowAgg(framed=True) as agg:
        agg.ports_enable_buckets(log2, 60)
        _fold(fa, agg, rows, status)
        ps = agg.ports_stats()
        assert ps["used"] == [n, n] and ps["grows"] >= 2 and ps["capacity"] == [1 << (log2 + 1)] * 2
        assert ps["fold_launches"] == 3 and ps["records_absorbed"] < n  # (at most 2 x entries x workgroups per launch fit the caches)
        check_ranges(po, agg, rows, status, [(T0, T0 + 60), (T0 + 60 * 16, T0 + 60 * 19), (T0 + 60 * 32, NO_UPPER)])
        assert len(agg.ports_buckets()) == (n + 65535) // 65536


def test_largest_merge_input_every_dense_port_in_two_buckets(gpu_lib, fa, po):
    T0 = po.T0
    p = np.arange(65536, dtype=np.uint32)
    rows = np.zeros(2 * 65536, dtype=po.ROW_DTYPE)
    rows["src_port"] = np.tile(p, 2)
    rows["dst_port"] = np.tile(p[::-1], 2)
    rows["bytes"] = np.tile((p % 1000).astype(np.uint64), 2)  # many ties, and 66 ports of weight 0
    rows["sampling_rate"] = 1
    rows["time_flow_start"] = np.uint64(T0) + np.repeat(np.arange(2, dtype=np.uint64), 65536) * np.uint64(60)
    status = np.zeros(len(rows), dtype=np.uint32)
    with fa.FlowAgg(framed=True) as agg:
        agg.ports_enable_buckets(16, 60)
        _fold(fa, agg, rows, status)
        for d in (0, 1):
            got = agg.top_ports_range(d, 0, T0, T0 + 120)
            assert len(got) == 65536 and (got["count"] == 2).all()
            _same(got, restate(po, rows, status, d, T0, T0 + 120))  # every row, in order
        check_ranges(po, agg, rows, status, [(T0 + 60, T0 + 120)], ks=(0, 100))
        assert agg.ports_stats()["used"] == [131072, 131072]


# ---- every ingest door -----------------------------------------------------------------------------------------------------------
def test_ingest_doors_with_small_chunks(gpu_lib, fa, po, monkeypatch):
    import torch
    n, T0 = 30000, po.T0
    buf, off, rows, status = _stream(2, n, 73, zs=100, lu=14)
    monkeypatch.setenv("FA_TALK_CHUNK", "4096")
    nbytes = int(off[-1])
    d_buf = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
    d_buf[:nbytes].copy_(torch.from_numpy(np.array(buf[:nbytes])))
    d_off = torch.from_numpy(off.astype(np.uint32).view(np.int32).copy()).cuda()
    step = 1 << 13

    def device_with_offsets(a):
        for i in range(0, n, step):
            m = min(step, n - i)
            a.ingest_device(d_buf.data_ptr(), nbytes, d_off.data_ptr() + 4 * i, m)

    def columns(a):
        for i in range(0, n, step):
            m = min(step, n - i)
            cols = a.decode_device(d_buf.data_ptr(), nbytes, d_off.data_ptr() + 4 * i, m)
            a.ports_fold_columns_device(cols, m)
        a.sync()
    doors = [lambda a: a.ingest(buf, off), lambda a: a.ingest(buf, None), device_with_offsets, lambda a: a.ingest_device(d_buf.data_ptr(), nbytes, None, 0), columns]
    with fa.FlowAgg(framed=True, max_batch_records=step) as none:
        none.ingest(buf, off)
        flows = none.read_window().tobytes()
    for i, door in enumerate(doors):
        with fa.FlowAgg(framed=True, max_batch_records=step) as agg:
            agg.ports_enable_buckets(10, 60)
            door(agg)
            check_ranges(po, agg, rows, status, [(0, NO_UPPER), (T0 + 60, T0 + 120), (T0 + 240, T0 + 840)])
            check_ranges(po, agg, rows, status, [(T0 + 240, T0 + 840)], ks=(10,))
            ps = agg.ports_stats()
            assert ps["fold_launches"] >= n // 4096 and ps["records_folded"] == n
            if door is not columns:
                assert agg.read_window().tobytes() == flows


# ---- beside the talkers and the FA_KEYS_PORT_HIST state ----------------------------------------------------------------------------
def test_talkers_ports_and_port_hist_side_by_side(gpu_lib, fa, po):
    n, T0 = 30000, po.T0
    buf, off, rows, status = _stream(2, n, 73, zs=100, lu=14)
    ks = fa.FA_KEYS_AS_PAIR | fa.FA_KEYS_PORT_HIST
    with fa.FlowAgg(framed=True, key_sets=ks) as talk, fa.FlowAgg(framed=True, key_sets=ks) as port, fa.FlowAgg(framed=True, key_sets=ks) as both:
        talk.talkers_enable(10, 60)
        port.ports_enable_buckets(10, 60)
        both.talkers_enable(10, 60)
        both.ports_enable_buckets(10, 60)
        h = n // 3
        for x in (talk, port, both):
            x.ingest(buf[:int(off[h])], off[:h + 1])
            x.ingest(buf[int(off[h]):], off[h:] - off[h])
        assert both.stats()["decode_launches"] == talk.stats()["decode_launches"] > 0  # one decode per chunk, shared
        ts, tt = both.talkers_stats(), talk.talkers_stats()  # (times differ, and which updates a cache absorbs is up to the lanes' order)
        assert all(ts[f] == tt[f] for f in ("used", "capacity", "records_folded", "grows", "fold_launches"))
        for d in (0, 1):
            for lo, hi, k in ((0, NO_UPPER, 0), (T0 + 120, T0 + 300, 0), (T0 + 120, T0 + 300, 10)):
                assert both.top_talkers(d, k, lo, hi).tobytes() == talk.top_talkers(d, k, lo, hi).tobytes()
                _same(both.top_ports_range(d, k, lo, hi), restate(po, rows, status, d, lo, hi, k))
                _same(port.top_ports_range(d, k, lo, hi), restate(po, rows, status, d, lo, hi, k))
            # the un-ranged call reads the FA_KEYS_PORT_HIST state: over the same records it is the range "everything"
            assert both.top_ports(d).tobytes() == both.top_ports_range(d, 0, 0, NO_UPPER).tobytes() == port.top_ports(d).tobytes()
        assert both.ports_stats()["used"] == port.ports_stats()["used"]
        # neither state clears the other
        both.dashboard_reset()
        assert len(both.top_ports(0)) == 0
        _same(both.top_ports_range(0, 0, 0, NO_UPPER), restate(po, rows, status, 0))
        port.ports_reset()
        assert len(port.top_ports_range(0)) == 0
        _same(port.top_ports(0), restate(po, rows, status, 0))


# ---- retention -------------------------------------------------------------------------------------------------------------------
def test_drop_before_late_records_and_reset(gpu_lib, fa, po):
    n, T0 = 30000, po.T0
    buf, off, rows, status = _stream(2, n, 73, zs=100, lu=14)
    floor = T0 + 300
    kept = t32_of(rows) >= np.uint64(floor)
    assert 0 < kept.sum() < n
    with fa.FlowAgg(framed=True) as agg:
        agg.ports_enable_buckets(10, 60)
        agg.ingest(buf, off)
        cap = agg.ports_stats()["capacity"]
        assert np.array_equal(agg.ports_buckets(), T0 + 60 * np.arange(15, dtype=np.uint32))
        agg.ports_drop_before(floor)
        assert np.array_equal(agg.ports_buckets(), floor + 60 * np.arange(10, dtype=np.uint32))
        ps = agg.ports_stats()
        assert ps["capacity"] == cap and ps["used"] == [pairs(po, rows, status, d, 60, floor) for d in (0, 1)]
        for d in (0, 1):
            assert len(agg.top_ports_range(d, 0, T0, floor)) == 0 and len(agg.top_ports_range(d, 0, T0 + 240, floor)) == 0
        check_ranges(po, agg, rows, status, [(floor, floor + 60), (floor + 120, NO_UPPER), (floor, T0 + 900)])
        check_ranges(po, agg, rows[kept], status[kept], [(0, NO_UPPER), (T0 + 240, T0 + 360)])
        # the first 5 000 records again: late, below the floor too - folded like any others, their buckets open again
        late = 5000
        agg.ingest(buf[:int(off[late])], off[:late + 1])
        both = np.concatenate([rows[kept], rows[:late]])
        st = np.zeros(len(both), dtype=status.dtype)
        assert (t32_of(rows[:late]) < np.uint64(floor)).any()
        check_ranges(po, agg, both, st, [(0, NO_UPPER), (T0, floor), (T0, T0 + 60), (floor, NO_UPPER)], ks=(0, 10))
        assert np.array_equal(agg.ports_buckets(), buckets_of(both, st, 60))
        ps = agg.ports_stats()
        assert ps["used"] == [pairs(po, both, st, d, 60) for d in (0, 1)] and ps["capacity"] == cap
        # a drop past everything: empty tables that still ingest
        agg.ports_drop_before(T0 + 86400)
        assert len(agg.ports_buckets()) == 0 and agg.ports_stats()["used"] == [0, 0]
        assert len(agg.top_ports_range(0)) == 0
        agg.ingest(buf, off)
        check_ranges(po, agg, rows, status, [(0, NO_UPPER), (T0 + 120, T0 + 300)])
        # reset keeps the size and the bucket size
        folded = agg.ports_stats()["records_folded"]
        agg.ports_reset()
        ps = agg.ports_stats()
        assert len(agg.ports_buckets()) == 0 and ps["used"] == [0, 0] and ps["capacity"] == cap and ps["records_folded"] == folded
        agg.ingest(buf, off)
        check_ranges(po, agg, rows, status, [(T0 + 120, T0 + 300)])


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_error_table(gpu_lib, fa, po):
    n, T0 = 20000, po.T0
    buf, off, rows, status = _stream(0, n, 71, zs=110, lu=16)
    L = fa.lib()
    row = np.zeros(4, dtype=fa.PORT_ROW_DTYPE)
    u32 = np.zeros(4, dtype=np.uint32)
    with fa.FlowAgg(framed=True, key_sets=fa.FA_KEYS_AS_PAIR | fa.FA_KEYS_PORT_HIST) as off_ctx, fa.FlowAgg(framed=True) as agg:
        # not enabled (FA_KEYS_PORT_HIST does not enable it): -8 from every call, outputs untouched
        off_ctx.ingest(buf, off)
        n_out, p = C.c_size_t(SENTINEL), C.c_void_p(SENTINEL)
        h = off_ctx._h
        assert L.fa_top_ports_range(h, 0, T0, T0 + 60, 0, row.ctypes.data, 4, C.byref(n_out)) == ERR_UNSUPPORTED and n_out.value == SENTINEL
        assert L.fa_ports_range_rows_device(h, 0, T0, T0 + 60, 0, C.byref(p), C.byref(n_out)) == ERR_UNSUPPORTED and (p.value, n_out.value) == (SENTINEL, SENTINEL)
        assert L.fa_ports_buckets(h, u32.ctypes.data, 4, C.byref(n_out)) == ERR_UNSUPPORTED and n_out.value == SENTINEL
        assert L.fa_ports_drop_before(h, T0) == ERR_UNSUPPORTED and L.fa_ports_reset(h) == ERR_UNSUPPORTED
        assert L.fa_ports_stats(h, C.byref(fa.PortsStats())) == ERR_UNSUPPORTED
        assert L.fa_ports_fold_columns_device(h, C.byref(fa.Columns()), 4) == ERR_UNSUPPORTED and "fa_ports_enable_buckets" in err(fa, off_ctx)
        _same(off_ctx.top_ports(0), restate(po, rows, status, 0))
        # bucket_secs, capacity, enabling twice
        for cap_log2, bs in ((0, 0), (0, 7), (0, 86401), (7, 60), (31, 60)):
            assert L.fa_ports_enable_buckets(agg._h, cap_log2, bs) == ERR_ARG
        assert L.fa_ports_stats(agg._h, C.byref(fa.PortsStats())) == ERR_UNSUPPORTED  # (the refused calls enabled nothing)
        agg.ports_enable_buckets(0, 60)
        assert L.fa_ports_enable_buckets(agg._h, 0, 60) == ERR_ARG and L.fa_ports_enable_buckets(agg._h, 0, 300) == ERR_ARG
        assert agg.ports_stats()["capacity"] == [1 << 16, 1 << 16]
        agg.ingest(buf, off)
        state = lambda: ([agg.top_ports_range(d).tobytes() for d in (0, 1)], agg.ports_buckets().tobytes(), agg.ports_stats()["used"])
        before = state()
        # off-grid bounds, t_lo > t_hi, a direction that is none
        for lo, hi in ((T0 + 1, T0 + 60), (T0, T0 + 61), (T0 + 120, T0 + 60), (T0, 0xFFFFFFFE)):
            n_out, p = C.c_size_t(SENTINEL), C.c_void_p(SENTINEL)
            assert L.fa_top_ports_range(agg._h, 0, lo, hi, 0, row.ctypes.data, 4, C.byref(n_out)) == ERR_ARG and n_out.value == SENTINEL
            assert L.fa_ports_range_rows_device(agg._h, 1, lo, hi, 0, C.byref(p), C.byref(n_out)) == ERR_ARG and (p.value, n_out.value) == (SENTINEL, SENTINEL)
        assert L.fa_ports_drop_before(agg._h, T0 + 61) == ERR_ARG
        assert L.fa_top_ports_range(agg._h, 2, T0, T0 + 60, 0, row.ctypes.data, 4, C.byref(n_out)) == ERR_ARG
        # a buffer one row short: the rows needed come back
        for lo, hi, k in ((T0, T0 + 60, 0), (0, NO_UPPER, 10)):
            need = len(restate(po, rows, status, 0, lo, hi, k))
            out, n_out = np.zeros(need, dtype=fa.PORT_ROW_DTYPE), C.c_size_t(SENTINEL)
            assert need > 1 and L.fa_top_ports_range(agg._h, 0, lo, hi, k, out.ctypes.data, need - 1, C.byref(n_out)) == ERR_CAPACITY
            assert n_out.value == need
        n_out = C.c_size_t(SENTINEL)
        held = len(buckets_of(rows, status, 60))
        assert held > 4 and L.fa_ports_buckets(agg._h, u32.ctypes.data, 4, C.byref(n_out)) == ERR_CAPACITY and n_out.value == held
        # missing and misaligned columns
        r, st = rows[:100], status[:100]
        for name in PORT_COLUMNS:
            with pytest.raises(fa.FlowAggError) as ei:
                _fold(fa, agg, r, st, leave_out=name)
            assert ei.value.code == ERR_ARG
        for name, by in (("src_port", 2), ("dst_port", 1), ("bytes", 4), ("sampling_rate", 4), ("time_flow_start", 4)):
            with pytest.raises(fa.FlowAggError) as ei:
                _fold(fa, agg, r, st, shift=(name, by))
            assert ei.value.code == ERR_ARG and "aligned" in str(ei.value)
        assert state() == before


# ---- groups of ctxs on one GPU ---------------------------------------------------------------------------------------------------
def _cut(buf, off, lo, hi):
    return buf[int(off[lo]):int(off[hi])], off[lo:hi + 1] - off[lo]


def _planted(po, parts, T0):
    """One port that no partition ranks first but that leads overall: in every partition it weighs a little less than that
    partition's own private port."""
    out = []
    for p in range(parts):
        r = np.zeros(2, dtype=po.ROW_DTYPE)
        r["src_port"] = r["dst_port"] = [100000 + p, 99999]  # (the private port first, then the planted one - both large ports)
        r["bytes"] = [1 << 50, (1 << 50) - 1]
        r["sampling_rate"] = 1
        r["time_flow_start"] = T0 + 130 + 60 * (p % 2)
        out.append(r)
    return out


@pytest.mark.parametrize("size", [1, 2, 3, 8])
def test_group_equals_one_ctx_that_folded_everything(gpu_lib, fa, po, size):
    n, T0 = 30000, po.T0
    buf, off, rows, status = _stream(2, n, 73, zs=100, lu=14)
    parts = max(size - 1, 1)  # with more than one member the last one is idle
    cuts = np.linspace(0, n, parts + 1).astype(int)
    extra = _planted(po, parts, T0)
    members = [fa.FlowAgg(framed=True) for _ in range(size)]
    try:
        with fa.FlowAgg(framed=True) as whole:
            whole.ports_enable_buckets(10, 60)
            whole.ingest(buf, off)
            for i, m in enumerate(members):
                m.ports_enable_buckets(8 + i % 3, 60)
                if i < parts:
                    m.ingest(*_cut(buf, off, cuts[i], cuts[i + 1]))
                    for x in (m, whole):
                        _fold(fa, x, extra[i], np.zeros(2, dtype=np.uint32))
            all_rows = np.concatenate([rows] + extra)
            all_status = np.zeros(len(all_rows), dtype=np.uint32)
            with fa.FlowGroup(members) as g:
                for d in (0, 1):
                    for lo, hi in ((T0 + 120, T0 + 300), (T0 + 600, NO_UPPER), (0, NO_UPPER), (T0 + 60, T0 + 60)):
                        want = restate(po, all_rows, all_status, d, lo, hi)
                        for k in (0, 1, 10):
                            got = g.top_ports_range(d, k, t_lo=lo, t_hi=hi)
                            _same(got, want[:k] if k else want)
                            assert got.tobytes() == whole.top_ports_range(d, k, lo, hi).tobytes()
                    if parts > 1:
                        assert int(g.top_ports_range(d, 1, t_lo=T0 + 120, t_hi=T0 + 300)["port"][0]) == 99999
                        assert all(int(m.top_ports_range(d, 1, T0 + 120, T0 + 300)["port"][0]) != 99999 for m in members[:parts])
                    need = len(restate(po, all_rows, all_status, d, T0 + 120, T0 + 300))
                    out, n_out = np.zeros(need, dtype=fa.PORT_ROW_DTYPE), C.c_size_t(SENTINEL)
                    assert fa.lib().fa_group_top_ports_range(g._h, d, T0 + 120, T0 + 300, 0, out.ctypes.data, need - 1, C.byref(n_out)) == ERR_CAPACITY
                    assert n_out.value == need
    finally:
        for m in members:
            m.close()


def test_group_members_that_do_not_fit(gpu_lib, fa, po):
    n, T0 = 30000, po.T0
    buf, off, rows, status = _stream(2, n, 73, zs=100, lu=14)
    L = fa.lib()
    for odd, code, text in ((lambda m: None, ERR_UNSUPPORTED, "not enabled"), (lambda m: m.ports_enable_buckets(10, 300), ERR_ARG, "bucket_secs differs")):
        members = [fa.FlowAgg(framed=True) for _ in range(3)]
        try:
            for i, m in enumerate(members):
                if i == 2:
                    odd(m)
                else:
                    m.ports_enable_buckets(10, 60)
                m.ingest(*_cut(buf, off, i * 10000, (i + 1) * 10000))
            before = [[m.top_ports_range(d).tobytes() for d in (0, 1)] for m in members[:2]]
            with fa.FlowGroup(members) as g:
                stats = [m.stats()["kernel_launches"] for m in members]
                for m in members:
                    L.fa_rows_fetch(m._h, 7, 0, 0, 0, 0)  # (each member's last error: something else)
                with pytest.raises(fa.FlowAggError) as ei:
                    g.top_ports_range(0, 10, t_lo=T0, t_hi=T0 + 300)
                assert ei.value.code == code
                msg = (L.fa_group_last_error(g._h) or b"").decode()
                assert "member 2" in msg and text in msg
                for m in members:
                    assert "member 2" in err(fa, m) and text in err(fa, m)
                assert [m.stats()["kernel_launches"] for m in members] == stats  # nothing was collected or exchanged
            assert [[m.top_ports_range(d).tobytes() for d in (0, 1)] for m in members[:2]] == before
        finally:
            for m in members:
                m.close()


# ---- across processes: two gloo ranks on one GPU -----------------------------------------------------------------------------------
TWO_RANK_WORKER = r'''
import hashlib, json, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np, torch, torch.distributed as dist
import _pkg
import test_port_buckets_gpu as T
fa, po = _pkg.load(), _pkg.load_oracle()
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)   # both ranks share the one GPU; the exchange goes over gloo
dist.init_process_group("gloo")
T0 = po.T0
n = 30000
buf, off, rows, status = T._stream(2, n, 73, zs=100, lu=14)
extra = T._planted(po, world, T0)
all_rows = np.concatenate([rows] + extra)
all_status = np.zeros(len(all_rows), dtype=np.uint32)
report = {"results": {}, "failure": "none", "afterwards": False}  # (a file per rank: the ranks' lines on stdout interleave)
with fa.FlowAgg(framed=True) as agg, fa.FlowAgg(framed=True) as off_ctx:
    agg.ports_enable_buckets(10, 60)
    h = n // 2
    agg.ingest(*T._cut(buf, off, rank * h, (rank + 1) * h))
    T._fold(fa, agg, extra[rank], np.zeros(2, dtype=np.uint32))
    for d in (0, 1):
        for lo, hi in ((T0 + 120, T0 + 300), (T0 + 600, None), (None, T0 + 60), (0, None)):
            for k in (1, 10, 0):
                want = T.restate(po, all_rows, all_status, d, 0 if lo is None else lo, T.NO_UPPER if hi is None else hi, k)
                got = fa.dist.top_ports_merged(agg, d, k, t_lo=lo, t_hi=hi)
                T._same(got, want)
                report["results"]["%%d/%%s/%%s/%%d" %% (d, lo, hi, k)] = hashlib.sha256(got.tobytes()).hexdigest()
        assert int(fa.dist.top_ports_merged(agg, d, 1, t_lo=T0 + 120, t_hi=T0 + 300)["port"][0]) == 99999
        assert int(agg.top_ports_range(d, 1, T0 + 120, T0 + 300)["port"][0]) != 99999  # no rank ranks it first
    # a rank that fails (rank 1's ctx was never enabled) takes both down: its own error there, RankFailed on the other
    try:
        fa.dist.top_ports_merged(agg if rank == 0 else off_ctx, 0, 10, t_lo=T0, t_hi=T0 + 60)
    except fa.FlowAggError as e:
        report["failure"] = "own %%d" %% e.code
    except fa.dist.RankFailed:
        report["failure"] = "other"
    # ... and the next close works again
    T._same(fa.dist.top_ports_merged(agg, 1, 5, t_lo=0), T.restate(po, all_rows, all_status, 1, k=5))
    report["afterwards"] = True
dist.destroy_process_group()
with open(os.path.join(%(out)r, "rank%%d.json" %% rank), "w") as f:
    json.dump(report, f)
'''


@pytest.fixture(scope="module")
def two_rank_run(tmp_path_factory):
    """ONE run of two fresh rank processes (torch.distributed.run, under a timeout) shared by the tests below -> each rank's report."""
    out = tmp_path_factory.mktemp("port_ranks")
    script = out / "two_rank_worker.py"
    script.write_text(TWO_RANK_WORKER % {"root": ROOT, "out": str(out)})
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return [json.load(open(out / ("rank%d.json" % rank))) for rank in (0, 1)]


def test_two_ranks_top_ports_merged(gpu_lib, two_rank_run):
    """(each rank compared every result with the restatement itself: a mismatch fails the run)"""
    reports = two_rank_run
    assert len(reports[0]["results"]) == 2 * 4 * 3
    assert reports[0]["results"] == reports[1]["results"]  # identical on both ranks


def test_two_ranks_a_failing_rank_takes_both_down(gpu_lib, two_rank_run):
    reports = two_rank_run
    assert [r["failure"] for r in reports] == ["other", "own %d" % ERR_UNSUPPORTED]  # rank 1's ctx was not enabled
    assert all(r["afterwards"] for r in reports)
