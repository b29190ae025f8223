"""GPU parity of the bucketed top talkers (fa_talkers_enable_buckets, fa_top_talkers_range, fa_talkers_range_rows_device,
fa_talkers_buckets, fa_talkers_drop_before, fa_group_top_talkers_range; include/flowagg.h "ABI 8, addition"): exact
GROUP BY SrcAddr / DstAddr for a time range.  Expected rows are restated here on the oracle's decode (po.decode_batch), its
group-by helper (po._group_sum), a filter on time_flow_start & 0xFFFFFFFF and the canonicalisation, the way
tests/test_talkers_gpu.py restates the un-ranged result.  Every comparison is np.array_equal on key, etype, weight and count,
for both directions; nothing is compared with the code under test except where a bucketed ctx's un-ranged result must be a
plain ctx's, byte for byte (the contract of the un-ranged calls on a bucketed ctx)."""
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
COLS = ("key", "etype", "weight", "count")
U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_UPPER = 0xFFFFFFFF
ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -6, -8
SENTINEL = 0x5A5A5A5A


def _same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for c in COLS:
        assert np.array_equal(got[c], want[c]), (c, np.nonzero((got[c] != want[c]).reshape(len(got), -1).any(axis=1))[0][:10])


def t32_of(rows):
    return (rows["time_flow_start"] & np.uint64(0xFFFFFFFF)).astype(np.uint64)


def in_range(rows, t_lo, t_hi):
    """t_lo <= t32 < t_hi; t_hi = 0xFFFFFFFF: no upper bound; t_lo == t_hi: nothing."""
    t = t32_of(rows)
    if t_lo == t_hi:
        return np.zeros(len(rows), dtype=bool)
    m = t >= np.uint64(t_lo)
    return m if t_hi == NO_UPPER else m & (t < np.uint64(t_hi))


def _canon(rows, dst):
    addr = np.ascontiguousarray(rows["dst_addr" if dst else "src_addr"]).copy().reshape(-1, 16)
    v4 = rows["etype"] == 0x800
    addr[v4, 4:] = 0
    fam = np.where(v4, 0x800, 0).astype(np.uint64)
    hi = addr[:, :8].copy().view(">u8").reshape(-1).astype(np.uint64)
    lo = addr[:, 8:].copy().view(">u8").reshape(-1).astype(np.uint64)
    return addr, fam, hi, lo


def restate(fa, po, rows, status, dst, t_lo=0, t_hi=NO_UPPER, k=0):
    """the well-formed records of the range, canonicalised, grouped by (key, family), ordered by weight DESC, key, family"""
    r = rows[(status == 0) & in_range(rows, t_lo, t_hi)]
    addr, fam, hi, lo = _canon(r, dst)
    with np.errstate(over="ignore"):
        w = r["bytes"] * r["sampling_rate"]
    idx, (ws, cs) = po._group_sum([hi, lo, fam], [w, np.ones(len(r), dtype=np.uint64)])
    out = np.zeros(len(idx), dtype=fa.TALKER_ROW_DTYPE)
    out["key"] = addr[idx]
    out["etype"] = fam[idx]
    out["weight"], out["count"] = ws, cs
    order = np.lexsort((fam[idx], lo[idx], hi[idx], U64MAX - out["weight"]))
    out = out[order]
    return out[:k] if k else out


def pairs(po, rows, status, dst, bs, t_floor=0):
    """the number of (bucket, key, family) groups: what used[dst] counts"""
    r = rows[(status == 0) & (t32_of(rows) >= np.uint64(t_floor))]
    _, fam, hi, lo = _canon(r, dst)
    t = t32_of(r)
    idx, _ = po._group_sum([t - t % np.uint64(bs), hi, lo, fam], [np.ones(len(r), dtype=np.uint64)])
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


def check_ranges(fa, po, agg, rows, status, ranges, ks=(0,)):
    for t_lo, t_hi in ranges:
        for d in (0, 1):
            for k in ks:
                _same(agg.top_talkers(d, k, t_lo, t_hi), restate(fa, po, rows, status, d, t_lo, t_hi, k))


def err(fa, agg):
    return (fa.lib().fa_last_error(agg._h) or b"").decode()


# ---- the mocker stream, bucket_secs = 60 ---------------------------------------------------------------------------------------
def test_mocker_stream_every_minute(gpu_lib, fa, po):
    n, T0 = 20000, po.T0
    buf, off, rows, status = _stream(0, n, 71)
    minutes = po.minute_series(rows, status)
    assert len(minutes) == 6 and int(minutes["minute"][0]) == T0
    with fa.FlowAgg(framed=True) as none, fa.FlowAgg(framed=True) as plain, fa.FlowAgg(framed=True) as agg:
        plain.talkers_enable()
        agg.talkers_enable(0, 60)
        for x in (none, plain, agg):
            x.ingest(buf, off)
        ranges = [(0, NO_UPPER), (T0, T0 + 360), (T0 + 120, T0 + 300), (T0 + 600, T0 + 900), (T0 + 120, T0 + 120), (T0, NO_UPPER)]
        ranges += [(int(m), int(m) + 60) for m in minutes["minute"]]
        check_ranges(fa, po, agg, rows, status, ranges, ks=(0, 10))
        for d in (0, 1):
            assert len(agg.top_talkers(d, 0, T0 + 600, T0 + 900)) == 0 and len(agg.top_talkers(d, 0, T0 + 120, T0 + 120)) == 0
            for m in minutes:  # an independent statement of the bucket rule: the minute series' row
                got = agg.top_talkers(d, 0, int(m["minute"]), int(m["minute"]) + 60)
                with np.errstate(over="ignore"):
                    assert int(got["weight"].sum(dtype=np.uint64)) == int(m["weight"]) and int(got["count"].sum(dtype=np.uint64)) == int(m["count"])
            # un-ranged on a bucketed ctx: every bucket held = a plain ctx's result, as bytes
            assert agg.top_talkers(d).tobytes() == plain.top_talkers(d).tobytes()
            assert agg.top_talkers(d, 10).tobytes() == plain.top_talkers(d, 10).tobytes()
            _same(agg.top_talkers(d), restate(fa, po, rows, status, d))
            ptr, m = agg.rows_device(fa.ROWS_TALKERS_SRC + d)
            assert agg.rows_fetch(fa.ROWS_TALKERS_SRC + d, ptr, m).tobytes() == plain.top_talkers(d).tobytes()
            ptr, m = agg.talkers_range_rows_device(d, T0 + 120, T0 + 300, 10)
            _same(agg.rows_fetch(fa.ROWS_TALKERS_SRC + d, ptr, m), restate(fa, po, rows, status, d, T0 + 120, T0 + 300, 10))
        assert np.array_equal(agg.talkers_buckets(), buckets_of(rows, status, 60))
        ts = agg.talkers_stats()
        assert ts["records_absorbed"] > 0 and ts["records_folded"] == n
        assert ts["used"] == [pairs(po, rows, status, d, 60) for d in (0, 1)]
        assert agg.read_window().tobytes() == none.read_window().tobytes() == plain.read_window().tobytes()


def test_zipf_with_growth(gpu_lib, fa, po):
    n, T0 = 200000, po.T0
    buf, off, rows, status = _stream(2, n, 72, zs=80, lu=16)
    with fa.FlowAgg(framed=True) as agg:
        agg.talkers_enable(8, 60)
        h = n // 3
        agg.ingest(buf[:int(off[h])], off[:h + 1])
        agg.ingest(buf[int(off[h]):], off[h:] - off[h])
        ts = agg.talkers_stats()
        assert ts["grows"] >= 2
        for d in (0, 1):
            assert ts["used"][d] == pairs(po, rows, status, d, 60)
            assert ts["capacity"][d] >= 2 * ts["used"][d]
        check_ranges(fa, po, agg, rows, status, [(T0, T0 + 60), (T0 + 300, T0 + 600), (T0 + 840, NO_UPPER)])
        check_ranges(fa, po, agg, rows, status, [(0, NO_UPPER)], ks=(10,))
        assert ts["records_folded"] == n


# ---- hand-made columns through fa_talkers_fold_columns_device -------------------------------------------------------------------
def _fold(fa, agg, rows, status, with_time=True):
    import torch
    n = len(rows)
    dev = torch.device("cuda", 0)

    def up(a, view):
        a = np.ascontiguousarray(a)
        if len(a) == 0:
            a = np.zeros((1,) + a.shape[1:], dtype=a.dtype)
        return torch.from_numpy(a.view(view).copy()).to(dev)
    keep = [up(rows["src_addr"], np.uint8), up(rows["dst_addr"], np.uint8), up(rows["etype"].astype(np.uint32), np.int32),
            up(rows["bytes"].astype(np.uint64), np.int64), up(rows["sampling_rate"].astype(np.uint64), np.int64), up(status.astype(np.uint8), np.uint8),
            up(rows["time_flow_start"].astype(np.uint64), np.int64)]
    cols = fa.Columns()
    cols.src_addr, cols.dst_addr, cols.etype, cols.bytes, cols.sampling_rate, cols.status = [t.data_ptr() for t in keep[:6]]
    if with_time:
        cols.time_flow_start = keep[6].data_ptr()
    try:
        agg.fold_columns_device(cols, n)
    finally:
        agg.sync()  # (the tensors may go once the stream has read them)


def _bucket_indices(bs):
    return [1, 5, 1_600_000_200 // bs, 0xFFFFFFFF // bs - 1]


def _handmade(po, n, seed, bs, pool=40):
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    keys = rng.integers(0, 256, size=(pool, 16), dtype=np.uint8)
    keys[: pool // 2, 4:] = rng.integers(0, 2, size=(pool // 2, 12), dtype=np.uint8)  # equal heads, differing tails
    keys[: pool // 2, :3] = 10
    keys[: pool // 2, 3] = rng.integers(0, 4, size=pool // 2, dtype=np.uint8)
    pick = rng.integers(0, pool, size=(n, 2))
    rows["src_addr"] = keys[pick[:, 0]]
    rows["dst_addr"] = keys[pick[:, 1]]
    rows["etype"] = rng.choice(np.array([0x800, 0x86dd, 0, 0x1234], dtype=np.uint32), size=n)
    rows["bytes"] = rng.integers(0, 1 << 62, size=n, dtype=np.uint64) * np.uint64(5)
    rows["sampling_rate"] = rng.choice(np.array([0, 1, 1000, 1 << 30], dtype=np.uint64), size=n)
    rows["sampling_rate"][pick[:, 0] < 3] = 0  # groups whose records all have weight 0 are still rows
    # times at the edges of a few buckets (b * bs - 1, b * bs, b * bs + bs - 1) and the last second of the axis ...
    times = [b * bs + o for b in _bucket_indices(bs) for o in (-1, 0, bs - 1)] + [0xFFFFFFFF]
    t = rng.choice(np.array(times, dtype=np.uint64), size=n)
    t += rng.integers(0, 3, size=n).astype(np.uint64) << np.uint64(32)  # ... a third of them above 2^32 each way: the narrowing
    rows["time_flow_start"] = t
    status = (rng.random(n) < 0.1).astype(np.uint8)  # malformed rows carry garbage that must be skipped, garbage times included
    bad = status != 0
    rows["time_flow_start"][bad] = rng.integers(0, 1 << 63, size=int(bad.sum()), dtype=np.uint64)
    return rows, status


@pytest.mark.parametrize("bs", [1, 60, 86400])
def test_handmade_columns_bucket_edges(gpu_lib, fa, po, bs):
    sizes = [0, 1, 63, 64, 65, fa.TALK_BLOCK - 1, fa.TALK_BLOCK, fa.TALK_BLOCK + 1]
    b = _bucket_indices(bs)
    last = 0xFFFFFFFF // bs * bs  # the start of the axis' last bucket: reached only through t_hi = 0xFFFFFFFF
    ranges = [(0, NO_UPPER), (b[0] * bs, b[0] * bs + bs), (b[0] * bs - bs, b[1] * bs), (b[2] * bs, b[2] * bs), (b[2] * bs, NO_UPPER),
              (b[3] * bs, last), (0, last), (b[3] * bs + bs if bs > 1 else last - 1, NO_UPPER), (last, NO_UPPER)]
    with fa.FlowAgg(framed=True, max_batch_records=1 << 16) as agg:
        agg.talkers_enable(8, bs)
        for n in sizes:
            rows, status = _handmade(po, n, 100 + n, bs)
            st = status.astype(np.uint32)
            agg.talkers_reset()
            _fold(fa, agg, rows, status)
            check_ranges(fa, po, agg, rows, st, ranges)
            check_ranges(fa, po, agg, rows, st, ranges[:2], ks=(3,))
            assert np.array_equal(agg.talkers_buckets(), buckets_of(rows, st, bs))
            assert agg.talkers_stats()["used"] == [pairs(po, rows, st, d, bs) for d in (0, 1)]
            if n >= fa.TALK_BLOCK - 1:
                want = restate(fa, po, rows, st, 0)
                assert (want["weight"] == 0).any() and (want["count"][want["weight"] == 0] > 0).all()  # zero-weight groups are rows
                t = t32_of(rows[st == 0])
                assert (t == 0xFFFFFFFF).any() and (rows["time_flow_start"][st == 0] > np.uint64(1 << 32)).any()
                if bs > 1:  # the last second of the axis is in no range with an upper bound on the grid
                    assert len(restate(fa, po, rows, st, 0, last, NO_UPPER)) > 0
                else:  # bucket_secs = 1: 0xFFFFFFFF is on the grid and still means "no upper bound"
                    assert len(restate(fa, po, rows, st, 0, last - 1, NO_UPPER)) > 0 and len(agg.top_talkers(0, 0, last, NO_UPPER)) == 0


def test_handmade_one_key_in_eight_buckets_wraps(gpu_lib, fa, po):
    per, nb, T0 = 100000, 8, po.T0
    n = per * nb
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    rows["src_addr"] = np.arange(1, 17, dtype=np.uint8)
    rows["dst_addr"] = np.arange(1, 17, dtype=np.uint8)
    rows["etype"] = 0x86dd
    rows["bytes"] = (1 << 63) + 3
    rows["sampling_rate"] = 1 << 30
    rows["time_flow_start"] = np.uint64(T0) + (np.arange(n, dtype=np.uint64) % np.uint64(nb)) * np.uint64(60)  # neighbours in a workgroup: other buckets
    status = np.zeros(n, dtype=np.uint8)
    one = (((1 << 63) + 3) * (1 << 30) * per) % (1 << 64)
    with fa.FlowAgg(framed=True, max_batch_records=1 << 16) as agg:
        agg.talkers_enable(8, 60)
        _fold(fa, agg, rows, status)
        ts = agg.talkers_stats()
        assert ts["used"] == [nb, nb] and ts["records_absorbed"] > 0  # the LDS cache absorbed, and did not merge buckets
        for d in (0, 1):
            for b in range(nb):
                got = agg.top_talkers(d, 0, T0 + 60 * b, T0 + 60 * b + 60)
                assert len(got) == 1 and int(got["count"][0]) == per and int(got["weight"][0]) == one
            got = agg.top_talkers(d, 0, T0 + 60, T0 + 240)
            assert len(got) == 1 and int(got["count"][0]) == 3 * per and int(got["weight"][0]) == (3 * one) % (1 << 64)
            got = agg.top_talkers(d)
            assert len(got) == 1 and int(got["count"][0]) == n and int(got["weight"][0]) == (nb * one) % (1 << 64)
        check_ranges(fa, po, agg, rows, status.astype(np.uint32), [(0, NO_UPPER), (T0 + 60, T0 + 240)])
        assert np.array_equal(agg.talkers_buckets(), T0 + 60 * np.arange(nb, dtype=np.uint32))


def test_one_key_in_48_buckets_takes_the_long_run_path(gpu_lib, fa, po):
    """A key held in more buckets than the row merge's heads walk serially (RUN_SERIAL = 32): 48 minutes of one address, beside
    keys held in 1, 31, 32 and 33 buckets."""
    T0, nb = po.T0, 48
    spans = [48, 1, 31, 32, 33, 40]
    parts = []
    for i, span in enumerate(spans):
        per = 7 + i
        r = np.zeros(span * per, dtype=po.ROW_DTYPE)
        a = np.zeros(16, dtype=np.uint8)
        a[0], a[15] = 10 + i, 0xC0 + i
        r["src_addr"], r["dst_addr"] = a, a[::-1].copy()
        r["etype"] = 0x86dd if i % 2 else 0x800
        r["bytes"] = (1 << 63) + 1000 * i + np.arange(len(r), dtype=np.uint64)
        r["sampling_rate"] = 3
        r["time_flow_start"] = np.uint64(T0) + (np.arange(len(r), dtype=np.uint64) % np.uint64(span)) * np.uint64(60) + np.uint64(i)
        parts.append(r)
    rows = np.concatenate(parts)
    rows = rows[np.random.default_rng(48).permutation(len(rows))]
    status = np.zeros(len(rows), dtype=np.uint32)
    with fa.FlowAgg(framed=True, max_batch_records=1 << 16) as agg:
        agg.talkers_enable(10, 60)
        _fold(fa, agg, rows, status.astype(np.uint8))
        assert agg.talkers_stats()["used"] == [sum(spans), sum(spans)]
        ranges = [(0, NO_UPPER), (T0, T0 + 60 * nb), (T0, T0 + 60 * 32), (T0, T0 + 60 * 33), (T0 + 60, T0 + 60 * 34), (T0 + 60 * 40, NO_UPPER)]
        check_ranges(fa, po, agg, rows, status, ranges, ks=(0, 2))
        for d in (0, 1):
            _same(agg.top_talkers(d), restate(fa, po, rows, status, d))
            got = agg.top_talkers(d, 0, T0, T0 + 60 * nb)
            assert len(got) == len(spans) and sorted(int(c) for c in got["count"]) == sorted(span * (7 + i) for i, span in enumerate(spans))


def test_order_at_a_million_groups(gpu_lib, fa, po):
    """1.3 M groups in three buckets: every row of the un-ranged and of a ranged read in fa_top_talkers' order, against the
    restatement and - un-ranged - against a plain ctx's fa_top_talkers as bytes; the row kinds of the plain ctx too.  Read three
    times each: an order that changes from call to call must not pass by luck."""
    T0 = po.T0
    keys, again = 1_300_000, 100_000
    n = keys + again
    rng = np.random.default_rng(1300)
    ids = np.concatenate([np.arange(keys, dtype=np.uint64), rng.integers(0, keys, size=again).astype(np.uint64)])
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    src = np.zeros((n, 16), dtype=np.uint8)
    src[:, :8] = (ids * np.uint64(0x9E3779B97F4A7C15)).view(np.uint8).reshape(n, 8)  # odd multiplier: a bijection
    src[:, 8:] = ids.view(np.uint8).reshape(n, 8)
    rows["src_addr"] = src
    rows["dst_addr"] = src[:, ::-1]
    rows["etype"] = np.where(ids % np.uint64(3) == 0, 0x800, 0x86dd)
    # (a third of the records take the IPv4 branch: keys that agree in their first four bytes are one group)
    rows["bytes"] = (np.uint64(3_000_000_000_000) // (np.uint64(1) + ids)) + rng.integers(0, 1000, size=n).astype(np.uint64)  # Zipf-like: most weights small and close
    rows["sampling_rate"] = 1
    rows["time_flow_start"] = np.uint64(T0) + rng.integers(0, 180, size=n).astype(np.uint64)
    status = np.zeros(n, dtype=np.uint32)
    want_all = restate(fa, po, rows, status, 0)
    want_mid = restate(fa, po, rows, status, 0, T0 + 60, T0 + 180)
    assert len(want_all) > 1_000_000 and int((want_all["weight"][1:] > want_all["weight"][:-1]).sum()) == 0
    with fa.FlowAgg(framed=True, max_batch_records=1 << 16) as plain, fa.FlowAgg(framed=True, max_batch_records=1 << 16) as agg:
        plain.talkers_enable(22)
        agg.talkers_enable(23, 60)
        st8 = status.astype(np.uint8)
        _fold(fa, plain, rows, st8)
        _fold(fa, agg, rows, st8)
        exact = [plain.top_talkers(d) for d in (0, 1)]
        _same(exact[0], want_all)
        for _ in range(3):
            _same(agg.top_talkers(0), want_all)
            _same(agg.top_talkers(0, 0, T0 + 60, T0 + 180), want_mid)
            _same(agg.top_talkers(0, 100, T0 + 60, T0 + 180), want_mid[:100])
            for d in (0, 1):
                assert agg.top_talkers(d).tobytes() == exact[d].tobytes()
                assert agg.top_talkers(d, 100).tobytes() == exact[d][:100].tobytes()
                ptr, m = plain.rows_device(fa.ROWS_TALKERS_SRC + d)
                assert plain.rows_fetch(fa.ROWS_TALKERS_SRC + d, ptr, m).tobytes() == exact[d].tobytes()


# ---- every ingest door -----------------------------------------------------------------------------------------------------------
def test_ingest_doors_with_small_chunks(gpu_lib, fa, po, monkeypatch):
    n, T0 = 30000, po.T0
    buf, off, rows, status = _stream(2, n, 73, zs=100, lu=14)
    monkeypatch.setenv("FA_TALK_CHUNK", "4096")
    for door in (lambda a: a.ingest(buf, off), lambda a: a.ingest(buf, None)):
        with fa.FlowAgg(framed=True, max_batch_records=1 << 13) as agg:
            agg.talkers_enable(10, 60)
            door(agg)
            check_ranges(fa, po, agg, rows, status, [(0, NO_UPPER), (T0 + 60, T0 + 120), (T0 + 240, T0 + 840)])
            check_ranges(fa, po, agg, rows, status, [(T0 + 240, T0 + 840)], ks=(10,))
            ts = agg.talkers_stats()
            assert ts["fold_launches"] >= n // 4096 and ts["records_folded"] == n


# ---- retention -------------------------------------------------------------------------------------------------------------------
def test_drop_before_and_late_records(gpu_lib, fa, po):
    n, T0 = 30000, po.T0
    buf, off, rows, status = _stream(2, n, 73, zs=100, lu=14)
    floor = T0 + 300
    kept = t32_of(rows) >= np.uint64(floor)
    assert 0 < kept.sum() < n
    with fa.FlowAgg(framed=True) as agg:
        agg.talkers_enable(10, 60)
        agg.ingest(buf, off)
        cap = agg.talkers_stats()["capacity"]
        assert np.array_equal(agg.talkers_buckets(), T0 + 60 * np.arange(15, dtype=np.uint32))
        agg.talkers_drop_before(floor)
        assert np.array_equal(agg.talkers_buckets(), floor + 60 * np.arange(10, dtype=np.uint32))
        ts = agg.talkers_stats()
        assert ts["capacity"] == cap and ts["used"] == [pairs(po, rows, status, d, 60, floor) for d in (0, 1)]
        for d in (0, 1):
            assert len(agg.top_talkers(d, 0, T0, floor)) == 0 and len(agg.top_talkers(d, 0, T0 + 240, floor)) == 0
            _same(agg.top_talkers(d), restate(fa, po, rows[kept], status[kept], d))
        check_ranges(fa, po, agg, rows, status, [(floor, floor + 60), (floor + 120, NO_UPPER), (floor, T0 + 900)])
        check_ranges(fa, po, agg, rows[kept], status[kept], [(0, NO_UPPER), (T0 + 240, T0 + 360)])
        # the first 5 000 records again: late, below the floor too - folded like any others, their buckets open again
        late = 5000
        agg.ingest(buf[:int(off[late])], off[:late + 1])
        both = np.concatenate([rows[kept], rows[:late]])
        st = np.zeros(len(both), dtype=status.dtype)
        assert (t32_of(rows[:late]) < np.uint64(floor)).any()
        check_ranges(fa, po, agg, both, st, [(0, NO_UPPER), (T0, floor), (T0, T0 + 60), (floor, NO_UPPER)], ks=(0, 10))
        assert np.array_equal(agg.talkers_buckets(), buckets_of(both, st, 60))
        assert agg.talkers_stats()["used"] == [pairs(po, both, st, d, 60) for d in (0, 1)]
        # a drop past everything: empty tables that still ingest
        agg.talkers_drop_before(T0 + 86400)
        assert len(agg.talkers_buckets()) == 0 and agg.talkers_stats()["used"] == [0, 0]
        for d in (0, 1):
            assert len(agg.top_talkers(d)) == 0 and len(agg.top_talkers(d, 0, T0, NO_UPPER)) == 0
        agg.ingest(buf, off)
        check_ranges(fa, po, agg, rows, status, [(0, NO_UPPER), (T0 + 120, T0 + 300)])
        # reset keeps the bucket size
        agg.talkers_reset()
        assert len(agg.talkers_buckets()) == 0
        agg.ingest(buf, off)
        check_ranges(fa, po, agg, rows, status, [(T0 + 120, T0 + 300)])


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_change_nothing(gpu_lib, fa, po):
    n, T0 = 20000, po.T0
    buf, off, rows, status = _stream(0, n, 71)
    L = fa.lib()
    row = np.zeros(4, dtype=fa.TALKER_ROW_DTYPE)
    u32 = np.zeros(4, dtype=np.uint32)

    def bucket_calls(h):
        n_out, p = C.c_size_t(SENTINEL), C.c_void_p(SENTINEL)
        yield L.fa_top_talkers_range(h, 0, T0, T0 + 60, 0, row.ctypes.data, 4, C.byref(n_out)), n_out.value
        yield L.fa_talkers_range_rows_device(h, 0, T0, T0 + 60, 0, C.byref(p), C.byref(n_out)), (p.value, n_out.value)
        yield L.fa_talkers_buckets(h, u32.ctypes.data, 4, C.byref(n_out)), n_out.value
        yield L.fa_talkers_drop_before(h, T0), None
    with fa.FlowAgg(framed=True) as off_ctx, fa.FlowAgg(framed=True) as plain, fa.FlowAgg(framed=True) as agg:
        # not enabled, and enabled without buckets: -8, outputs untouched
        plain.talkers_enable()
        plain.ingest(buf, off)
        before = [plain.top_talkers(d).tobytes() for d in (0, 1)]
        for x in (off_ctx, plain):
            for rc, outs in bucket_calls(x._h):
                assert rc == ERR_UNSUPPORTED
                assert outs in (None, SENTINEL, (SENTINEL, SENTINEL))
        assert [plain.top_talkers(d).tobytes() for d in (0, 1)] == before
        # bucket_secs, and enabling twice in every order of the two calls
        assert L.fa_talkers_enable_buckets(agg._h, 0, 0) == ERR_ARG and L.fa_talkers_enable_buckets(agg._h, 0, 7) == ERR_ARG
        assert L.fa_talkers_enable_buckets(agg._h, 7, 60) == ERR_ARG
        assert L.fa_talkers_stats(agg._h, C.byref(fa.TalkersStats())) == ERR_UNSUPPORTED  # (the refused calls enabled nothing)
        assert L.fa_talkers_enable_buckets(plain._h, 0, 60) == ERR_ARG and L.fa_talkers_enable(plain._h, 0) == ERR_ARG
        assert L.fa_top_talkers_range(plain._h, 0, T0, T0 + 60, 0, row.ctypes.data, 4, C.byref(C.c_size_t())) == ERR_UNSUPPORTED  # (still plain)
        agg.talkers_enable(0, 60)
        assert L.fa_talkers_enable(agg._h, 0) == ERR_ARG and L.fa_talkers_enable_buckets(agg._h, 0, 60) == ERR_ARG
        assert L.fa_talkers_enable_buckets(agg._h, 0, 300) == ERR_ARG
        agg.ingest(buf, off)
        want = [restate(fa, po, rows, status, d) for d in (0, 1)]
        state = lambda: ([agg.top_talkers(d).tobytes() for d in (0, 1)], agg.talkers_buckets().tobytes(), agg.talkers_stats()["used"])
        before = state()
        for d in (0, 1):
            _same(agg.top_talkers(d), want[d])
        # off-grid values, t_lo > t_hi
        n_out, p = C.c_size_t(SENTINEL), C.c_void_p(SENTINEL)
        for lo, hi in ((T0 + 1, T0 + 60), (T0, T0 + 61), (T0 + 120, T0 + 60), (T0, 0xFFFFFFFE)):
            assert L.fa_top_talkers_range(agg._h, 0, lo, hi, 0, row.ctypes.data, 4, C.byref(n_out)) == ERR_ARG and n_out.value == SENTINEL
            assert L.fa_talkers_range_rows_device(agg._h, 1, lo, hi, 0, C.byref(p), C.byref(n_out)) == ERR_ARG and (p.value, n_out.value) == (SENTINEL, SENTINEL)
        assert L.fa_talkers_drop_before(agg._h, T0 + 61) == ERR_ARG
        assert L.fa_top_talkers_range(agg._h, 2, T0, T0 + 60, 0, row.ctypes.data, 4, C.byref(n_out)) == ERR_ARG
        # the fold without the time column
        r, st = rows[:100], status[:100].astype(np.uint8)
        with pytest.raises(fa.FlowAggError) as ei:
            _fold(fa, agg, r, st, with_time=False)
        assert ei.value.code == ERR_ARG
        import torch
        dev = [torch.zeros(16 * 16 + 16, dtype=torch.uint8, device="cuda") for _ in range(7)]  # (16-byte aligned allocations)
        cols = fa.Columns()
        cols.src_addr, cols.dst_addr, cols.etype, cols.bytes, cols.sampling_rate, cols.status = [x.data_ptr() for x in dev[:6]]
        cols.time_flow_start = dev[6].data_ptr() + 4  # the time column is read as 8-byte words
        assert dev[6].data_ptr() % 8 == 0 and L.fa_talkers_fold_columns_device(agg._h, C.byref(cols), 16) == ERR_ARG and "8-byte aligned" in err(fa, agg)
        cols.time_flow_start = dev[6].data_ptr()
        cols.status = dev[5].data_ptr()
        dev[5].fill_(1)  # (every record malformed: an aligned call is taken and folds nothing)
        assert L.fa_talkers_fold_columns_device(agg._h, C.byref(cols), 16) == 0
        agg.sync()
        # rows carry no time: no merge into bucketed tables
        d_rows = torch.zeros(4 * 40, dtype=torch.uint8, device="cuda")
        assert L.fa_merge_talkers(agg._h, 0, row.ctypes.data, 4) == ERR_UNSUPPORTED and "no time" in err(fa, agg)
        assert L.fa_merge_talkers_device(agg._h, 0, d_rows.data_ptr(), 4) == ERR_UNSUPPORTED and "no time" in err(fa, agg)
        # a buffer one row short: the rows needed come back
        for lo, hi, k in ((T0, T0 + 60, 0), (0, NO_UPPER, 10)):
            need = len(restate(fa, po, rows, status, 0, lo, hi, k))
            out, n_out = np.zeros(need, dtype=fa.TALKER_ROW_DTYPE), C.c_size_t(SENTINEL)
            assert need > 1 and L.fa_top_talkers_range(agg._h, 0, lo, hi, k, out.ctypes.data, need - 1, C.byref(n_out)) == ERR_CAPACITY
            assert n_out.value == need
        n_out = C.c_size_t(SENTINEL)
        assert L.fa_talkers_buckets(agg._h, u32.ctypes.data, 4, C.byref(n_out)) == ERR_CAPACITY and n_out.value == 6
        assert state() == before


# ---- groups of ctxs on one GPU ---------------------------------------------------------------------------------------------------
def _cut(buf, off, lo, hi):
    return buf[int(off[lo]):int(off[hi])], off[lo:hi + 1] - off[lo]


@pytest.mark.parametrize("size", [3, 8])
def test_group_range_equals_the_restatement(gpu_lib, fa, po, size):
    n, T0 = 30000, po.T0
    buf, off, rows, status = _stream(2, n, 73, zs=100, lu=14)
    cuts = np.linspace(0, n, size).astype(int)  # size - 1 partitions: the last member holds no records
    members = [fa.FlowAgg(framed=True) for _ in range(size)]
    try:
        for i, m in enumerate(members):
            m.talkers_enable(10, 60)
            if i < size - 1:
                m.ingest(*_cut(buf, off, cuts[i], cuts[i + 1]))
        with fa.FlowGroup(members) as g:
            for d in (0, 1):
                kind = fa.ROWS_TALKERS_SRC + d
                for lo, hi in ((T0 + 120, T0 + 300), (T0 + 600, NO_UPPER)):
                    for k in (0, 10):
                        want = restate(fa, po, rows, status, d, lo, hi, k)
                        assert len(want) > 0
                        _same(g.top_talkers(d, k, t_lo=lo, t_hi=hi), want)
                    # the same close composed by hand: ranged rows -> by owner -> every owner's share merged -> the shares merged
                    want = restate(fa, po, rows, status, d, lo, hi)
                    world = 2
                    sent = [[None] * world for _ in members]
                    for i, m in enumerate(members):
                        ptr, cnt = m.talkers_range_rows_device(d, lo, hi)
                        pptr, counts = m.rows_partition_device(kind, ptr, cnt, world)
                        got = m.rows_fetch(kind, pptr, cnt)
                        at = 0
                        for r in range(world):
                            sent[i][r] = got[at:at + counts[r]]
                            at += counts[r]
                    import torch
                    shares = []
                    for r in range(world):
                        mine = np.concatenate([sent[i][r] for i in range(size)])
                        t = torch.from_numpy(mine.view(np.uint8).reshape(-1).copy()).cuda() if len(mine) else torch.zeros(64, dtype=torch.uint8, device="cuda")
                        mptr, mn = members[r].rows_merge_device(kind, t.data_ptr(), len(mine))
                        shares.append(members[r].rows_fetch(kind, mptr, mn).copy())
                    allr = np.concatenate(shares)
                    assert len(allr) == len(want)  # a key lives in exactly one share
                    t = torch.from_numpy(allr.view(np.uint8).reshape(-1).copy()).cuda()
                    mptr, mn = members[0].rows_merge_device(kind, t.data_ptr(), len(allr))
                    _same(members[0].rows_fetch(kind, mptr, mn), want)
                for k in (0, 10):  # un-ranged on bucketed members: every bucket
                    _same(g.top_talkers(d, k), restate(fa, po, rows, status, d, k=k))
                need = len(restate(fa, po, rows, status, d, T0 + 120, T0 + 300))
                out, n_out = np.zeros(need, dtype=fa.TALKER_ROW_DTYPE), C.c_size_t(SENTINEL)
                assert fa.lib().fa_group_top_talkers_range(g._h, d, T0 + 120, T0 + 300, 0, out.ctypes.data, need - 1, C.byref(n_out)) == ERR_CAPACITY
                assert n_out.value == need
    finally:
        for m in members:
            m.close()


def test_group_members_that_do_not_fit(gpu_lib, fa, po):
    n, T0 = 30000, po.T0
    buf, off, rows, status = _stream(2, n, 73, zs=100, lu=14)
    L = fa.lib()
    for odd, code, text in ((lambda m: m.talkers_enable(10), ERR_UNSUPPORTED, "no time axis"), (lambda m: m.talkers_enable(10, 300), ERR_ARG, "bucket_secs differs")):
        members = [fa.FlowAgg(framed=True) for _ in range(3)]
        try:
            for i, m in enumerate(members):
                if i == 2:
                    odd(m)
                else:
                    m.talkers_enable(10, 60)
                m.ingest(*_cut(buf, off, i * 10000, (i + 1) * 10000))
            before = [[m.top_talkers(d).tobytes() for d in (0, 1)] for m in members]
            with fa.FlowGroup(members) as g:
                stats = [m.stats()["kernel_launches"] for m in members]
                for m in members:
                    L.fa_rows_fetch(m._h, 7, 0, 0, 0, 0)  # (each member's last error: something else)
                with pytest.raises(fa.FlowAggError) as ei:
                    g.top_talkers(0, 10, t_lo=T0, t_hi=T0 + 300)
                assert ei.value.code == code
                msg = (L.fa_group_last_error(g._h) or b"").decode()
                assert "member 2" in msg and text in msg
                for m in members:
                    assert "member 2" in err(fa, m) and text in err(fa, m)
                assert [m.stats()["kernel_launches"] for m in members] == stats
            assert [[m.top_talkers(d).tobytes() for d in (0, 1)] for m in members] == before
        finally:
            for m in members:
                m.close()


# ---- dist.top_talkers_merged(t_lo, t_hi) at world 1 -------------------------------------------------------------------------------
WORKER = r'''
import json, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np, torch, torch.distributed as dist
import _pkg
import test_talker_buckets_gpu as T
fa, po = _pkg.load(), _pkg.load_oracle()
torch.cuda.set_device(0)
dist.init_process_group("gloo")
assert dist.get_world_size() == 1
T0 = po.T0
buf, off, rows, status = T._stream(2, 30000, 73, zs=100, lu=14)
checked = 0
with fa.FlowAgg(framed=True) as agg, fa.FlowAgg(framed=True) as plain:
    agg.talkers_enable(10, 60)
    agg.ingest(buf, off)
    for d in (0, 1):
        for lo, hi in ((T0 + 120, T0 + 300), (T0 + 600, None), (None, T0 + 60)):
            for k in (0, 10):
                want = T.restate(fa, po, rows, status, d, 0 if lo is None else lo, T.NO_UPPER if hi is None else hi, k)
                T._same(fa.dist.top_talkers_merged(agg, d, k, t_lo=lo, t_hi=hi), want)
                checked += 1
        T._same(fa.dist.top_talkers_merged(agg, d, 10), T.restate(fa, po, rows, status, d, k=10))
    plain.talkers_enable(10)
    try:
        fa.dist.top_talkers_merged(plain, 0, 10, t_lo=T0, t_hi=T0 + 60)
        code = 0
    except fa.FlowAggError as e:
        code = e.code
dist.destroy_process_group()
with open(os.path.join(%(out)r, "report.json"), "w") as f:
    json.dump({"checked": checked, "plain": code}, f)
'''


def test_dist_top_talkers_merged_range_world_1(gpu_lib, tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"root": ROOT, "out": str(tmp_path)})
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    report = json.load(open(tmp_path / "report.json"))
    assert report == {"checked": 12, "plain": ERR_UNSUPPORTED}
