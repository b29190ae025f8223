"""The talker row kinds (FA_ROWS_TALKERS_SRC / _DST = 8 / 9) in the device-resident close: fa_rows_device / _merge_device /
_partition_device / _fetch, fa_merge_talkers_device, fa_group_top_talkers and dist.top_talkers_merged.  The reference is
fa_top_talkers of ONE ctx that folded everything (itself checked against the oracle in test_talkers_gpu.py); every
comparison is byte for byte."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A
ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -6, -8
ALIAS = "rows to merge alias the ctx's result buffer (copy them first)"
NOT_CANONICAL = "fa_merge_talkers: a row is not canonical (etype 0 or 0x800; bytes 4..15 zero under 0x800)"
NOT_ENABLED = "top talkers are not enabled on this ctx (fa_talkers_enable)"
KW = dict(framed=True, max_batch_records=1 << 16)


def _load():
    import _pkg
    return _pkg.load(), _pkg.load_oracle()


# ---- streams: built once, shared, read-only ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def zipf_records(n=6000):
    """A few thousand generated Zipf records (framed wire bytes + offsets): they enter through fa_ingest_device."""
    fa, po = _load()
    gp = po.gen_params(mode=2, framed=1, seed=91, n_total=n, span_secs=900, per_sec=60, zipf_s_x100=90, zipf_log2_universe=13)
    buf, off = po.gen_records(gp, 0, n)
    for a in (buf, off):
        a.setflags(write=False)
    return buf, off


@functools.lru_cache(maxsize=None)
def edge_columns():
    """Hand-made columns: 1 000 groups of equal weight (among them the same 16 bytes under both families), one group whose
    weight wraps mod 2^64, groups of weight 0 - shuffled, so that both halves of the stream hold most keys."""
    fa, po = _load()
    rng = np.random.default_rng(9)
    a = np.zeros((1000, 16), dtype=np.uint8)
    et = np.zeros(1000, dtype=np.uint32)
    a[0:250, :15] = rng.integers(1, 256, size=15, dtype=np.uint8)
    a[0:250, 15] = rng.permutation(256)[:250]
    a[250:500, 0] = np.arange(250)
    et[0:500] = 0x86dd
    a[500:750, :3] = 7
    a[500:750, 3] = rng.permutation(256)[:250]
    a[750:1000, 0] = np.arange(250)  # the canonical bytes of rows 250..499, under the other family
    a[500:1000, 4:] = rng.integers(0, 256, size=(500, 12), dtype=np.uint8)
    et[500:1000] = 0x800
    n = 1000 + 6 + 40
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    rows["src_addr"][:1000], rows["etype"][:1000] = a, et
    rows["bytes"][:1000], rows["sampling_rate"][:1000] = 7, 1
    rows["src_addr"][1000:1006] = 0xEE  # six records of 2^63 + 5: the sum is 30 mod 2^64
    rows["etype"][1000:1006] = 0x86dd
    rows["bytes"][1000:1006], rows["sampling_rate"][1000:1006] = (1 << 63) + 5, 1
    rows["src_addr"][1006:, 0] = 0xDD   # twenty keys that never weigh anything, two records each
    rows["src_addr"][1006:, 1] = np.arange(40) % 20
    rows["src_addr"][1006:, 2] = 1      # (no key of the tie block looks like this)
    rows["etype"][1006:] = 0x800
    rows["bytes"][1006:], rows["sampling_rate"][1006:] = 1500, 0
    rows["dst_addr"] = rows["src_addr"][:, ::-1]
    rows = rows[rng.permutation(n)]
    status = np.zeros(n, dtype=np.uint8)
    for x in (rows, status):
        x.setflags(write=False)
    return rows, status


def talker_rows_of(fa, rows, status, dst):
    """One fa_talker_row per well-formed record (canonical key, weight = Bytes * SamplingRate, count 1)."""
    r = rows[status == 0]
    out = np.zeros(len(r), dtype=fa.TALKER_ROW_DTYPE)
    out["key"] = r["dst_addr" if dst else "src_addr"]
    v4 = r["etype"] == 0x800
    out["key"][v4, 4:] = 0
    out["etype"] = np.where(v4, 0x800, 0)
    with np.errstate(over="ignore"):
        out["weight"] = r["bytes"].astype(np.uint64) * r["sampling_rate"].astype(np.uint64)
    out["count"] = 1
    return out


PLANTED = bytes([0x20, 1, 0xd, 0xb8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x4b, 0x1d])


@functools.lru_cache(maxsize=None)
def partitions():
    """8 partitions x 4 096 records (Zipf-drawn shared keys, both families), each with 12 heavy keys of its own - and ONE
    planted key that every partition sees once, below its own heavy keys: outside every partition's top 10, first overall."""
    fa, po = _load()
    rng = np.random.default_rng(17)
    universe = rng.integers(0, 256, size=(2000, 16), dtype=np.uint8)
    parts = []
    for p in range(8):
        n = 4096
        rows = np.zeros(n, dtype=po.ROW_DTYPE)
        ids = np.minimum(rng.zipf(1.1, size=n) - 1, 1999)
        rows["src_addr"] = universe[ids]
        rows["etype"] = rng.choice(np.array([0x800, 0x86dd], dtype=np.uint32), size=n)
        rows["bytes"] = rng.integers(1, 100, size=n, dtype=np.uint64)
        rows["sampling_rate"] = 1
        heavy = np.zeros((12, 16), dtype=np.uint8)
        heavy[:, 0], heavy[:, 1], heavy[:, 15] = 0xFD, p, np.arange(12)
        rows["src_addr"][-13:-1], rows["etype"][-13:-1] = heavy, 0x86dd
        rows["bytes"][-13:-1] = 150000 + np.arange(12)
        rows["src_addr"][-1], rows["etype"][-1], rows["bytes"][-1] = np.frombuffer(PLANTED, dtype=np.uint8), 0x86dd, 100000
        rows["dst_addr"] = rows["src_addr"][:, ::-1]
        rows = rows[rng.permutation(n)]
        rows.setflags(write=False)
        parts.append(rows)
    # the property the group tests rest on, from numpy alone
    for d in (0, 1):
        key = PLANTED[::-1] if d else PLANTED
        for rows in parts:
            local = fa.dist.merge_talkers_host([talker_rows_of(fa, rows, np.zeros(len(rows), dtype=np.uint8), d)])
            at = [i for i, r in enumerate(local) if r["key"].tobytes() == key]
            assert len(at) == 1 and at[0] >= 10, at
        whole = fa.dist.merge_talkers_host([talker_rows_of(fa, rows, np.zeros(len(rows), dtype=np.uint8), d) for rows in parts])
        assert whole["key"][0].tobytes() == key and int(whole["weight"][0]) == 800000 and int(whole["count"][0]) == 8
    return tuple(parts)


# ---- feeding a ctx, moving rows ------------------------------------------------------------------------------------------
def fold(fa, agg, rows, status=None):
    import torch
    n = len(rows)
    if n == 0:
        return
    status = np.zeros(n, dtype=np.uint8) if status is None else status
    dev = torch.device("cuda", 0)
    up = lambda a, view: torch.from_numpy(np.ascontiguousarray(a).view(view).copy()).to(dev)
    keep = [up(rows["src_addr"], np.uint8), up(rows["dst_addr"], np.uint8), up(rows["etype"].astype(np.uint32), np.int32),
            up(rows["bytes"].astype(np.uint64), np.int64), up(rows["sampling_rate"].astype(np.uint64), np.int64), up(status.astype(np.uint8), np.uint8)]
    cols = fa.Columns()
    cols.src_addr, cols.dst_addr, cols.etype, cols.bytes, cols.sampling_rate, cols.status = [t.data_ptr() for t in keep]
    agg.fold_columns_device(cols, n)
    agg.sync()  # (the tensors may go once the stream has read them)


def ingest_device(agg, buf, off, i, j):
    import torch
    dev = torch.device("cuda", 0)
    lo, hi = int(off[i]), int(off[j])
    d_buf = torch.zeros(hi - lo + 64, dtype=torch.uint8, device=dev)
    d_buf[:hi - lo] = torch.from_numpy(np.array(buf[lo:hi])).to(dev)
    d_off = torch.from_numpy((off[i:j + 1] - off[i]).astype(np.uint32).view(np.int32)).to(dev)
    agg.ingest_device(d_buf.data_ptr(), hi - lo, d_off.data_ptr(), j - i)
    agg.sync()


def feed(fa, agg, stream, part, nparts):
    """Part `part` of `nparts` of a stream: "zipf" (wire records through fa_ingest_device) or "edge" (columns)."""
    if stream == "zipf":
        buf, off = zipf_records()
        n = len(off) - 1
        ingest_device(agg, buf, off, n * part // nparts, n * (part + 1) // nparts)
    else:
        rows, status = edge_columns()
        n = len(rows)
        fold(fa, agg, rows[n * part // nparts:n * (part + 1) // nparts], status[n * part // nparts:n * (part + 1) // nparts])


def upload(rows):
    """host rows -> uint8 cuda tensor (never empty: a pointer is wanted)"""
    import torch
    t = torch.zeros(max(rows.nbytes, 64), dtype=torch.uint8, device="cuda")
    if rows.nbytes:
        t[:rows.nbytes] = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    return t


def device_copy(fa, ptr, n):
    """n talker rows at a ctx-owned device pointer -> a tensor of the test's own"""
    import torch
    if not n:
        return torch.zeros(64, dtype=torch.uint8, device="cuda")
    t = torch.as_tensor(fa.dist._DevArray(ptr, n * 40, "|u1"), device="cuda").clone()
    torch.cuda.synchronize()
    return t


def device_rows(fa, agg, kind, k=0):
    ptr, n = agg.rows_device(kind, k=k)
    return agg.rows_fetch(kind, ptr, n)


def err(fa, agg):
    return (fa.lib().fa_last_error(agg._h) or b"").decode()


# ---- 1. one ctx: the row kinds against fa_top_talkers ---------------------------------------------------------------------
@pytest.mark.parametrize("stream", ["zipf", "edge"])
def test_rows_device_equals_top_talkers(gpu_lib, fa, stream):
    with fa.FlowAgg(**KW) as agg:
        agg.talkers_enable(8)  # (2^8 slots: the tables grow on the way)
        for d in (0, 1):  # an empty table: no rows, no error
            assert len(device_rows(fa, agg, fa.ROWS_TALKERS_SRC + d)) == 0
        feed(fa, agg, stream, 0, 1)
        st = agg.talkers_stats()
        assert st["grows"] >= 2 and min(st["used"]) > 100
        if stream == "zipf":
            assert max(st["capacity"]) >= 2 * 4096  # more than one workgroup round of the collect kernel
        for d in (0, 1):
            used = st["used"][d]
            want = agg.top_talkers(d)
            assert len(want) == used
            if stream == "edge" and d == 0:  # the edge rows are there: the wrapped sum, weightless groups, the tie block
                assert int(want["weight"][0]) == 30 and int(want["count"][0]) == 6 and (want["weight"] == 7).sum() == 1000
                assert (want["weight"] == 0).sum() == 20 and (want["count"][want["weight"] == 0] == 2).all()
            for k in (0, 1, 7, used, used + 5):
                got = device_rows(fa, agg, fa.ROWS_TALKERS_SRC + d, k)
                assert got.tobytes() == agg.top_talkers(d, k).tobytes() == want[:k or used].tobytes(), (d, k)


def test_rows_device_of_a_table_smaller_than_a_round(gpu_lib, fa):
    rows, status = edge_columns()
    with fa.FlowAgg(**KW) as agg:
        agg.talkers_enable(8)
        fold(fa, agg, rows[:100], status[:100])
        st = agg.talkers_stats()
        assert st["capacity"] == [256, 256] and st["grows"] == 0  # 256 slots: a sixteenth of a workgroup's round
        for d in (0, 1):
            assert device_rows(fa, agg, fa.ROWS_TALKERS_SRC + d).tobytes() == agg.top_talkers(d).tobytes()
            assert device_rows(fa, agg, fa.ROWS_TALKERS_SRC + d, 3).tobytes() == agg.top_talkers(d, 3).tobytes()


# ---- 2. merge ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", ["zipf", "edge"])
def test_merge_of_two_halves_equals_one_ctx(gpu_lib, fa, stream):
    import torch
    with fa.FlowAgg(**KW) as a, fa.FlowAgg(**KW) as b, fa.FlowAgg(**KW) as whole:
        for x in (a, b, whole):
            x.talkers_enable(10)
        feed(fa, a, stream, 0, 2)
        feed(fa, b, stream, 1, 2)
        feed(fa, whole, stream, 0, 1)
        for d in (0, 1):
            kind = fa.ROWS_TALKERS_SRC + d
            own = a.top_talkers(d)
            pieces = []
            for x in (a, b):
                ptr, m = x.rows_device(kind)
                pieces.append(device_copy(fa, ptr, m)[:m * 40])
            both = torch.cat(pieces)  # the two results back to back, on the device
            n = both.numel() // 40
            want = whole.top_talkers(d)
            assert n > len(want)  # keys that both halves hold
            for k in (0, 1, 10, len(want) + 3):
                ptr, m = a.rows_merge_device(kind, both.data_ptr(), n, k)
                assert a.rows_fetch(kind, ptr, m).tobytes() == want[:k or len(want)].tobytes(), (d, k)
            # the numpy restatement agrees
            assert fa.dist.merge_talkers_host([a.top_talkers(d), b.top_talkers(d)]).tobytes() == want.tobytes()
            assert a.top_talkers(d).tobytes() == own.tobytes()  # (the merge does not touch the ctx's own table)
        # n = 0
        ptr, m = a.rows_merge_device(fa.ROWS_TALKERS_SRC, 0, 0, 0)
        assert (ptr, m) == (0, 0)


def test_merge_long_run_bad_rows_and_alias(gpu_lib, fa):
    L = fa.lib()
    with fa.FlowAgg(**KW) as agg:
        agg.talkers_enable(8)
        h = agg._h
        # 40 copies of one row between two others: a run longer than RUN_SERIAL = 32 (the tail kernel on 40-byte rows)
        rows = np.zeros(42, dtype=fa.TALKER_ROW_DTYPE)
        rows["key"][:, 0] = 9
        rows["key"][0, 0], rows["key"][41, 0] = 1, 200
        rows["weight"], rows["count"] = (1 << 62) + 11, (1 << 63) + 1
        rows["weight"][[0, 41]], rows["count"][[0, 41]] = [5, 6], [1, 2]
        rows["_pad"] = 77
        t = upload(rows)
        ptr, m = agg.rows_merge_device(fa.ROWS_TALKERS_DST, t.data_ptr(), 42, 0)
        got = agg.rows_fetch(fa.ROWS_TALKERS_DST, ptr, m)
        assert m == 3 and not got["_pad"].any()
        assert [int(w) for w in got["weight"]] == [(40 * ((1 << 62) + 11)) % (1 << 64), 6, 5]
        assert [int(c) for c in got["count"]] == [(40 * ((1 << 63) + 1)) % (1 << 64), 2, 1]
        assert [int(k) for k in got["key"][:, 0]] == [9, 200, 1]
        assert got.tobytes() == fa.dist.merge_talkers_host([rows]).tobytes()
        # a row that is not canonical, anywhere in the input: FA_ERR_ARG before anything is merged, the outputs untouched
        for at, et, byte in ((0, 0x86dd, None), (41, 0x800, 4), (20, 0x800, 15)):
            bad = rows.copy()
            bad["etype"][at] = et
            if byte is not None:
                bad["key"][at, byte] = 1
            tb = upload(bad)
            p, n_out = C.c_void_p(SENTINEL), C.c_size_t(SENTINEL)
            assert L.fa_rows_merge_device(h, fa.ROWS_TALKERS_SRC, tb.data_ptr(), 42, 0, C.byref(p), C.byref(n_out)) == ERR_ARG, (at, et)
            assert (err(fa, agg), p.value, n_out.value) == (NOT_CANONICAL, SENTINEL, SENTINEL)
        # the ctx's own result fed back
        ptr, m = agg.rows_merge_device(fa.ROWS_TALKERS_SRC, t.data_ptr(), 42, 0)
        p, n_out = C.c_void_p(SENTINEL), C.c_size_t(SENTINEL)
        assert L.fa_rows_merge_device(h, fa.ROWS_TALKERS_SRC, ptr, m, 0, C.byref(p), C.byref(n_out)) == ERR_ARG
        assert (err(fa, agg), p.value, n_out.value) == (ALIAS, None, 0)
        fold(fa, agg, edge_columns()[0][:64])
        ptr, m = agg.rows_device(fa.ROWS_TALKERS_SRC)
        assert m > 0 and L.fa_rows_merge_device(h, fa.ROWS_TALKERS_SRC, ptr, m, 0, C.byref(p), C.byref(n_out)) == ERR_ARG
        assert err(fa, agg) == ALIAS


# ---- 3. partition -----------------------------------------------------------------------------------------------------------
def test_partition_follows_the_host_restatement(gpu_lib, fa):
    with fa.FlowAgg(**KW) as agg:
        agg.talkers_enable(10)
        feed(fa, agg, "zipf", 0, 1)
        feed(fa, agg, "edge", 0, 1)
        for d in (0, 1):
            kind = fa.ROWS_TALKERS_SRC + d
            rows = agg.top_talkers(d)
            for world in (1, 2, 3, 8):
                ptr, n = agg.rows_device(kind)
                pptr, counts = agg.rows_partition_device(kind, ptr, n, world)
                got = agg.rows_fetch(kind, pptr, n)
                assert n == len(rows) and sum(counts) == n and len(counts) == world
                owner = fa.dist.partition_rows_host(got, kind, world)
                assert np.array_equal(owner, np.repeat(np.arange(world), counts)), world
                assert sorted(r.tobytes() for r in got) == sorted(r.tobytes() for r in rows)  # the same multiset of rows
                if world > 1:
                    assert min(counts) > 0


# ---- 4. fa_merge_talkers_device ---------------------------------------------------------------------------------------------
def test_merge_talkers_device_equals_the_host_merge(gpu_lib, fa):
    L = fa.lib()
    with fa.FlowAgg(**KW) as a, fa.FlowAgg(**KW) as b, fa.FlowAgg(**KW) as c, fa.FlowAgg(**KW) as whole:
        a.talkers_enable(8)
        b.talkers_enable(12)
        c.talkers_enable(8)
        whole.talkers_enable(12)
        for x in (a, c):
            feed(fa, x, "edge", 0, 2)
        feed(fa, b, "edge", 1, 2)
        feed(fa, b, "zipf", 0, 1)
        feed(fa, whole, "edge", 0, 1)
        feed(fa, whole, "zipf", 0, 1)
        grows0 = a.talkers_stats()["grows"]
        for d in (0, 1):
            ptr, n = b.rows_device(fa.ROWS_TALKERS_SRC + d)
            a.merge_talkers_device(d, ptr, n)                 # straight from b's result buffer
            c.merge_talkers(d, b.top_talkers(d))
        assert a.talkers_stats()["grows"] > grows0  # (b holds more keys than a's table had room for)
        for d in (0, 1):
            assert a.top_talkers(d).tobytes() == c.top_talkers(d).tobytes() == whole.top_talkers(d).tobytes()
        # the canonical check refuses - wherever the row sits - and merges nothing
        good = b.top_talkers(0)[:50].copy()
        for at, et, byte in ((0, 0x86dd, 15), (49, 0x800, 4), (25, 0x800, 15)):
            bad = good.copy()
            bad["etype"][at] = et
            bad["key"][at, byte] = 1
            t = upload(bad)
            assert L.fa_merge_talkers_device(a._h, 0, t.data_ptr(), 50) == ERR_ARG, (at, et)
            assert err(fa, a) == NOT_CANONICAL
        assert L.fa_merge_talkers_device(a._h, 2, 0, 0) == ERR_ARG
        a.merge_talkers_device(0, 0, 0)  # no rows: nothing to do
        assert a.top_talkers(0).tobytes() == whole.top_talkers(0).tobytes()


# ---- 5. groups --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 2, 3, 8])
def test_group_top_talkers_equals_one_ctx(gpu_lib, fa, size):
    L = fa.lib()
    parts = partitions()
    members = [fa.FlowAgg(**KW) for _ in range(size)]
    whole = fa.FlowAgg(**KW)
    try:
        for x in members + [whole]:
            x.talkers_enable(10)
        for p, rows in enumerate(parts):
            fold(fa, members[p % size], rows)
            fold(fa, whole, rows)
        before = [[m.top_talkers(d).tobytes() for d in (0, 1)] for m in members]
        with fa.FlowGroup(members) as g:
            for d in (0, 1):
                want = whole.top_talkers(d)
                assert want["key"][0].tobytes() == (PLANTED[::-1] if d else PLANTED)
                if size == 8:  # no member ranks the planted key among its first 10
                    assert all(want["key"][0].tobytes() not in {r["key"].tobytes() for r in m.top_talkers(d, 10)} for m in members)
                for k in (1, 10, 0):
                    assert g.top_talkers(d, k).tobytes() == want[:k or len(want)].tobytes(), (d, k)
                    assert g.read_window(fa.ROWS_TALKERS_SRC + d, 12345, k).tobytes() == want[:k or len(want)].tobytes(), (d, k)
                # a buffer one row short: the rows needed come back
                for k, need in ((10, 10), (0, len(want))):
                    out, n_out = np.zeros(need, dtype=fa.TALKER_ROW_DTYPE), C.c_size_t(SENTINEL)
                    assert L.fa_group_top_talkers(g._h, d, k, out.ctypes.data, need - 1, C.byref(n_out)) == ERR_CAPACITY
                    assert n_out.value == need
            with pytest.raises(fa.FlowAggError) as ei:
                g.close_window(fa.ROWS_TALKERS_SRC)
            assert ei.value.code == ERR_ARG
        assert [[m.top_talkers(d).tobytes() for d in (0, 1)] for m in members] == before  # a read: nothing removed
    finally:
        for x in members + [whole]:
            x.close()


def test_group_member_not_enabled(gpu_lib, fa):
    L = fa.lib()
    parts = partitions()
    members = [fa.FlowAgg(**KW) for _ in range(3)]
    try:
        for i in (0, 1):
            members[i].talkers_enable(10)
            fold(fa, members[i], parts[i])
        before = [[members[i].top_talkers(d).tobytes() for d in (0, 1)] for i in (0, 1)]
        with fa.FlowGroup(members) as g:
            for call in (lambda: g.top_talkers(0, 10), lambda: g.read_window(fa.ROWS_TALKERS_DST, 0, 10)):
                for m in members:
                    L.fa_rows_fetch(m._h, 7, 0, 0, 0, 0)  # (each member's last error: something else)
                with pytest.raises(fa.FlowAggError) as ei:
                    call()
                assert ei.value.code == ERR_UNSUPPORTED
                text = (L.fa_group_last_error(g._h) or b"").decode()
                assert "member 2" in text and NOT_ENABLED in text
                for m in members:
                    assert "member 2" in err(fa, m) and NOT_ENABLED in err(fa, m)
        assert [[members[i].top_talkers(d).tobytes() for d in (0, 1)] for i in (0, 1)] == before
    finally:
        for x in members:
            x.close()


# ---- 6. the doors on a ctx that was not enabled; kind 7 -----------------------------------------------------------------------
def test_doors_not_enabled_and_kind_7(gpu_lib, fa):
    L = fa.lib()
    d = upload(np.zeros(4, dtype=fa.TALKER_ROW_DTYPE))
    out = np.zeros(64, dtype=fa.TALKER_ROW_DTYPE)
    with fa.FlowAgg(**KW) as plain, fa.FlowAgg(**KW) as on:
        on.talkers_enable(8)
        for agg, kinds, code, text in ((plain, (8, 9), ERR_UNSUPPORTED, NOT_ENABLED), (plain, (7,), ERR_ARG, "unknown row kind"), (on, (7,), ERR_ARG, "unknown row kind")):
            h = agg._h
            for kind in kinds:
                p, n_out, counts = C.c_void_p(SENTINEL), C.c_size_t(SENTINEL), (C.c_size_t * 2)(SENTINEL, SENTINEL)
                assert L.fa_rows_device(h, kind, 0, 0, C.byref(p), C.byref(n_out)) == code and err(fa, agg) == text
                assert (p.value, n_out.value) == (None, 0)
                p, n_out = C.c_void_p(SENTINEL), C.c_size_t(SENTINEL)
                assert L.fa_rows_merge_device(h, kind, d.data_ptr(), 4, 0, C.byref(p), C.byref(n_out)) == code and err(fa, agg) == text
                assert (p.value, n_out.value) == (SENTINEL, SENTINEL)
                assert L.fa_rows_partition_device(h, kind, d.data_ptr(), 4, 2, C.byref(p), counts) == code and err(fa, agg) == text
                assert list(counts) == [SENTINEL, SENTINEL]
                assert L.fa_rows_fetch(h, kind, d.data_ptr(), 4, out.ctypes.data, 64) == code and err(fa, agg) == text
        assert L.fa_merge_talkers_device(plain._h, 0, d.data_ptr(), 4) == ERR_UNSUPPORTED and err(fa, plain) == NOT_ENABLED
        # the enabled ctx takes the same four calls
        ptr, n = on.rows_merge_device(8, d.data_ptr(), 4, 0)
        assert n == 1 and on.rows_fetch(8, ptr, n).tobytes() == bytes(40)
        pptr, counts = on.rows_partition_device(9, d.data_ptr(), 4, 2)
        assert sum(counts) == 4 and max(counts) == 4


# ---- 7. across processes ----------------------------------------------------------------------------------------------------
TWO_RANK_WORKER = r'''
import hashlib, json, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np, torch, torch.distributed as dist
import _pkg
import test_talker_rows_gpu as T
fa = _pkg.load()
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)   # both ranks share the one GPU; the exchange goes over gloo
dist.init_process_group("gloo")
parts = T.partitions()
report = {"results": {}, "failure": "none", "afterwards": False}  # (a file per rank: the ranks' lines on stdout interleave)
with fa.FlowAgg(**T.KW) as agg, fa.FlowAgg(**T.KW) as whole, fa.FlowAgg(**T.KW) as off:
    agg.talkers_enable(10)
    whole.talkers_enable(10)
    for p, rows in enumerate(parts):
        if p %% world == rank:
            T.fold(fa, agg, rows)
        T.fold(fa, whole, rows)
    for d in (0, 1):
        want = whole.top_talkers(d)
        assert want["key"][0].tobytes() == (T.PLANTED[::-1] if d else T.PLANTED)
        for k in (1, 10, 0):
            got = fa.dist.top_talkers_merged(agg, d, k)
            assert got.tobytes() == want[:k or len(want)].tobytes(), (d, k)
            report["results"]["%%d/%%d" %% (d, k)] = hashlib.sha256(got.tobytes()).hexdigest()
    # a rank that fails (rank 1's ctx was never enabled) takes both down: its own error there, RankFailed on the other
    try:
        fa.dist.top_talkers_merged(agg if rank == 0 else off, 0, 10)
    except fa.FlowAggError as e:
        report["failure"] = "own %%d" %% e.code
    except fa.dist.RankFailed:
        report["failure"] = "other"
    # ... and the next close works again
    assert fa.dist.top_talkers_merged(agg, 1, 5).tobytes() == whole.top_talkers(1, 5).tobytes()
    report["afterwards"] = True
dist.destroy_process_group()
with open(os.path.join(%(out)r, "rank%%d.json" %% rank), "w") as f:
    json.dump(report, f)
'''


@pytest.fixture(scope="module")
def two_rank_run(tmp_path_factory):
    """ONE run of two fresh rank processes (torch.distributed.run, under a timeout) shared by the tests below
    -> (the run, each rank's report)."""
    import json
    import socket
    out = tmp_path_factory.mktemp("talker_ranks")
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
    return r, [json.load(open(out / ("rank%d.json" % rank))) for rank in (0, 1)]


def test_two_ranks_top_talkers_merged(gpu_lib, two_rank_run):
    """(each rank compared every result with the single-ctx answer itself: a mismatch fails the run)"""
    _, reports = two_rank_run
    assert sorted(reports[0]["results"]) == sorted("%d/%d" % (d, k) for d in (0, 1) for k in (1, 10, 0))
    assert reports[0]["results"] == reports[1]["results"]  # identical on both ranks


def test_two_ranks_a_failing_rank_takes_both_down(gpu_lib, two_rank_run):
    _, reports = two_rank_run
    assert [r["failure"] for r in reports] == ["other", "own %d" % ERR_UNSUPPORTED]  # rank 1's ctx was not enabled
    assert all(r["afterwards"] for r in reports)
