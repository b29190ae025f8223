"""GPU tests of the rollups from columns and from parts (fa_rollup_fold_columns_device, fa_raw_load_rollup, fa_rollup_stats;
include/flowagg.h "ABI 8, addition: the rollups from columns and from parts").

Expected values never come from the code under test: they are the reads of a ctx that INGESTED the same records' wire bytes, the
oracle's (po.Rollup, po.rollup_app, po.top_ports, po.minute_series), or a numpy group-by of the rows the test wrote
(tests/raw_load_cases.py: random_rows, native_part).  Every comparison is bit-exact.

One deviation from the sizes the feature's description names for the growth test: fa_create refuses table_capacity_log2 below 10
and wide_capacity_log2 below 8 (FA_ERR_ARG), so the growth test starts from those - the smallest tables a ctx can have - and
5 000 distinct groups per key set still outgrow both several times over."""
import numpy as np
import pytest

import raw_load_cases as R
from test_raw_load_gpu import _as_rows
from test_raw_parts_gpu import D0, DAY, _midnight, _upload

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_FRAMING, ERR_UNSUPPORTED = -1, -7, -8
KS4 = 1 | 8 | 16 | 32  # FA_KEYS_AS_PAIR | ADDR_PORT_PROTO | PORT_HIST | MINUTE_SERIES
NO_UPPER = 0xFFFFFFFF


def _reads(agg):
    return dict(rows=agg.read_window(), app=agg.read_window_app(), sport=agg.top_ports(0), dport=agg.top_ports(1),
                minutes=agg.minute_series(), slots=agg.open_timeslots())


def _equal_reads(a, b, nonempty=True):
    assert a.keys() == b.keys()
    for k in a:
        assert len(a[k]) == len(b[k]) and a[k].tobytes() == b[k].tobytes(), k
    assert not nonempty or all(len(v) > 0 for v in a.values())


def _rollup_np(fa, po, rows, status, gran=300):
    """flows_5m of hand-made rows: GROUP BY Timeslot, SrcAS, DstAS, EType -> wrapping sums, in key order"""
    r = rows[status == 0]
    t32 = (r["time_received"] & np.uint64(0xFFFFFFFF)).astype(np.uint64)
    ts = t32 - t32 % np.uint64(gran)
    keys = [ts] + [r[c].astype(np.uint64) for c in ("src_as", "dst_as", "etype")]
    first, (b, p, c) = po._group_sum(keys, [r["bytes"], r["packets"], np.ones(len(r), dtype=np.uint64)])
    out = np.zeros(len(first), dtype=fa.ROW5M_DTYPE)
    out["timeslot"], out["date"] = ts[first], ts[first] // np.uint64(DAY)
    for col in ("src_as", "dst_as", "etype"):
        out[col] = r[col][first]
    out["bytes"], out["packets"], out["count"] = b, p, c
    return out


def _by_key(rows):
    return rows[np.lexsort((rows["etype"], rows["dst_as"], rows["src_as"], rows["timeslot"]))]


def _check_against_rows(fa, po, agg, rows, status, gran=300):
    """every read of a four-set ctx against the group-bys of the rows it was given"""
    got = agg.read_window()
    want = _rollup_np(fa, po, rows, status, gran)
    assert int(got["count"].sum()) == int((status == 0).sum())  # every record once
    assert _by_key(got).tobytes() == want.tobytes()
    assert agg.read_window_app().tobytes() == po.rollup_app(rows, status, gran).tobytes()
    for d in (0, 1):
        assert agg.top_ports(d).tobytes() == po.top_ports(rows, status, d).tobytes(), d
    assert agg.minute_series().tobytes() == po.minute_series(rows, status).tobytes()


def _fold_rows(fa, agg, rows, status, key_sets=0):
    cols, keep = _upload(fa, rows, status)
    agg.rollup_fold_columns(cols, len(rows), key_sets)
    del keep


def _wire(fa, rows):
    """hand-made rows -> framed protobuf records (every projected field, ascending field numbers) and their offsets"""
    recs = []
    ev = fa.schema.encode_varint
    for r in rows:
        f = [(2, int(r["time_received"])), (3, int(r["sampling_rate"])), (4, int(r["sequence_num"])), (6, bytes(r["src_addr"])), (7, bytes(r["dst_addr"])),
             (9, int(r["bytes"])), (10, int(r["packets"])), (11, bytes(r["sampler_address"])), (14, int(r["src_as"])), (15, int(r["dst_as"])),
             (20, int(r["proto"])), (21, int(r["src_port"])), (22, int(r["dst_port"])), (30, int(r["etype"])), (38, int(r["time_flow_start"]))]
        out = bytearray()
        for num, v in f:
            if isinstance(v, bytes):
                out += ev((num << 3) | 2) + ev(len(v)) + v
            elif v:
                out += ev(num << 3) + ev(v)
        recs.append(fa.schema.frame(bytes(out)))
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in recs])
    return np.frombuffer(b"".join(recs), dtype=np.uint8), off


def _decode_on_device(agg, buf, off):
    """the wire bytes decoded by fa_decode_device on `agg` -> (Columns, the tensors that own the input)"""
    import torch
    d_buf = torch.zeros(len(buf) + 64, dtype=torch.uint8, device="cuda")
    d_buf[:len(buf)].copy_(torch.from_numpy(np.array(buf)))
    d_off = torch.from_numpy(off.astype(np.uint32).view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    return agg.decode_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), len(off) - 1), (d_buf, d_off)


# ---- ctx A: the midnight stream ingested, its parts four ways --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ingested(gpu_lib, fa, po):
    buf, off, rows, status = _midnight(bad_every=97)
    out = {}
    for form in ("plain", "lz4", "plain_merged", "lz4_merged"):
        with fa.FlowAgg(framed=True, key_sets=KS4) as a:
            a.raw_enable(7000)  # three chunks x two Dates
            a.ingest(buf, off)
            if form.endswith("_merged"):
                a.raw_merge()
            data, parts = a.raw_take_lz4() if form.startswith("lz4") else a.raw_take()
            assert len(parts) == (2 if form.endswith("_merged") else 6)
            out[form] = bytes(data)
            out[form + "_parts"] = parts
            if "reads" not in out:
                out["reads"] = _reads(a)
                out["stats"] = a.stats()
    out["good"] = int((status == 0).sum())
    ref = po.Rollup(300)
    assert ref.ingest(buf, off, 1) == len(rows) - out["good"]
    out["oracle"] = ref.rows()
    return out


# ---- 1: equal to ingest, through parts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "lz4", "plain_merged", "lz4_merged"])
def test_parts_equal_ingest(gpu_lib, fa, ingested, form):
    with fa.FlowAgg(framed=True, key_sets=KS4) as b:
        assert b.rollup_stats() == dict(calls=0, records_in=0, records_bad=0, records_folded=0, launches=0, fold_ns=0)
        b.raw_load_rollup(ingested[form])
        _equal_reads(_reads(b), ingested["reads"])
        assert b.read_window().tobytes() == ingested["oracle"].tobytes()
        st, rs, ls = b.stats(), b.rollup_stats(), b.raw_load_stats()
        assert rs["calls"] == 1 and rs["records_in"] == rs["records_folded"] == ingested["good"] and rs["records_bad"] == 0
        assert rs["launches"] == ls["parts"] == (2 if form.endswith("_merged") else 6) and rs["fold_ns"] > 0 and ls["rows_loaded"] == ingested["good"]
        # wire-record counters do not move; the tables' do
        assert st["records_ok"] == st["records_bad"] == st["bytes_in"] == 0
        assert st["table_used"] == ingested["stats"]["table_used"] and st["wide_used"] == ingested["stats"]["wide_used"]


# ---- 2: equal to ingest, through columns ----------------------------------------------------------------------------------------------------
def _time_edge_rows(po, n, seed, received_high, start_high):
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    base = D0 * DAY
    rows["time_received"] = base + rng.integers(0, 900, n)
    rows["time_flow_start"] = base - rng.integers(0, 1200, n)
    if received_high:  # at and above 2^32: the DateTime narrowing keeps the low 32 bits
        rows["time_received"] = np.where(np.arange(n) % 3 == 0, np.uint64(1 << 32), np.uint64(1 << 32) + rows["time_received"] + (np.arange(n) % 5 << 33).astype(np.uint64))
    if start_high:
        rows["time_flow_start"] += (np.uint64(1) << np.uint64(32)) * (1 + np.arange(n) % 7).astype(np.uint64)
    for c, hi in (("sampling_rate", 1 << 12), ("bytes", 1 << 40), ("packets", 1 << 20), ("sequence_num", 1 << 32), ("src_as", 70), ("dst_as", 3),
                  ("proto", 300), ("src_port", 70000), ("dst_port", 70000)):
        rows[c] = rng.integers(0, hi, n)
    rows["etype"] = np.where(np.arange(n) % 2 == 0, 0x800, 0x86DD)
    for c in ("sampler_address", "src_addr", "dst_addr"):
        rows[c] = rng.integers(0, 256, (40, 16), dtype=np.uint8)[rng.integers(0, 40, n)]
    return rows


@pytest.mark.parametrize("case", ["midnight", "received_high", "start_high"])
def test_columns_equal_ingest(gpu_lib, fa, po, case):
    if case == "midnight":
        buf, off, rows, status = _midnight(bad_every=97)
    else:
        rows = _time_edge_rows(po, 3000, 5, case == "received_high", case == "start_high")
        buf, off = _wire(fa, rows)
        back, status = po.decode_batch(buf, off, 1)
        assert not status.any() and back.tobytes() == rows.tobytes()  # the test's encoder writes what it was given
    with fa.FlowAgg(framed=True, key_sets=KS4) as a, fa.FlowAgg(framed=True, key_sets=KS4) as b:
        a.ingest(buf, off)
        cols, keep = _decode_on_device(b, buf, off)
        b.rollup_fold_columns(cols, len(rows))
        _equal_reads(_reads(b), _reads(a))
        _check_against_rows(fa, po, b, rows, status)
        rs, nbad = b.rollup_stats(), int((status != 0).sum())
        assert (rs["calls"], rs["records_in"], rs["records_bad"], rs["records_folded"], rs["launches"]) == (1, len(rows), nbad, len(rows) - nbad, 1)
        assert b.stats()["records_ok"] == 0 and a.stats()["records_bad"] == nbad
        del keep


# ---- 3: slice edges --------------------------------------------------------------------------------------------------------------------------
EDGES = (0, 1, 63, 64, 65, 255, 256, 257, 3 * 256 - 1, 3 * 256, 3 * 256 + 1, 2 * 3 * 256 + 65)


def _edge_rows(po, n, seed):
    rows = _as_rows(po, R.random_rows(seed, n, keys=60))
    status = (np.arange(n) % 11 == 5).astype(np.uint8)  # the skipped ones carry values all the same
    return rows, status


def test_slice_edges_small_grid(gpu_lib, fa, po, monkeypatch):
    monkeypatch.setenv("FA_ROLLUP_GRID", "3")
    for n in EDGES:
        rows, status = _edge_rows(po, n, 100 + n)
        with fa.FlowAgg(framed=True, key_sets=KS4) as agg:
            _fold_rows(fa, agg, rows, status)
            if n:
                _check_against_rows(fa, po, agg, rows, status)
            else:
                assert all(len(v) == 0 for v in _reads(agg).values())
            rs = agg.rollup_stats()
            assert rs["launches"] == (1 if n else 0) and rs["records_in"] == n and rs["records_bad"] == int(status.sum()), n


def test_slice_edges_full_grid(gpu_lib, fa, po, monkeypatch):
    monkeypatch.delenv("FA_ROLLUP_GRID", raising=False)
    n = (1 << 18) + 1
    rows, status = _edge_rows(po, n, 9)
    with fa.FlowAgg(framed=True, key_sets=KS4) as agg:
        _fold_rows(fa, agg, rows, status)
        _check_against_rows(fa, po, agg, rows, status)
        assert agg.rollup_stats()["records_folded"] == n - int(status.sum())


# ---- 4: hit and miss paths --------------------------------------------------------------------------------------------------------------------
def _path_rows(po, n, seed, groups):
    """n rows over `groups` (SrcAS, DstAS) pairs; 40 minutes of TimeFlowStart; ports on both sides of 65536; weights and sums that
    wrap past 2^64; an EType outside the compact dictionary and AS numbers at and above 2^20"""
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    g = rng.integers(0, groups, n)
    rows["time_received"] = D0 * DAY + rng.integers(0, 600, n)
    rows["time_flow_start"] = D0 * DAY - rng.integers(0, 40 * 60, n)
    rows["src_as"] = np.where(g % 5 == 0, (1 << 20) + g, g)
    rows["dst_as"] = np.where(g % 7 == 0, 0xFFFFFFF0 + g % 16, 64512 + g % 3)
    rows["etype"] = np.choose(g % 4, [0x800, 0x86DD, 0x8847, 0])
    rows["bytes"] = np.where(rng.random(n) < 0.5, np.uint64(1 << 63) + rng.integers(0, 1 << 20, n).astype(np.uint64), rng.integers(0, 1 << 17, n).astype(np.uint64))
    rows["packets"] = np.where(rng.random(n) < 0.5, np.uint64((1 << 63) + 1), rng.integers(0, 512, n).astype(np.uint64))
    rows["sampling_rate"] = np.array([1, 1 << 33, (1 << 64) - 1], dtype=np.uint64)[rng.integers(0, 3, n)]
    ports = np.array([0, 80, 65535, 65536, 65537, 70000, 0xFFFFFFFF], dtype=np.uint64)
    rows["src_port"], rows["dst_port"] = ports[rng.integers(0, len(ports), n)], ports[rng.integers(0, len(ports), n)]
    rows["proto"] = rng.integers(0, 3, n) * 200
    rows["src_addr"] = rng.integers(0, 256, (30, 16), dtype=np.uint8)[rng.integers(0, 30, n)]
    return rows


@pytest.mark.parametrize("grid", ["1", ""])
@pytest.mark.parametrize("groups", [1, 9, 1000])
def test_hit_and_miss_paths(gpu_lib, fa, po, monkeypatch, grid, groups):
    if grid:
        monkeypatch.setenv("FA_ROLLUP_GRID", grid)  # one workgroup: more AS pairs than LDS slots (256), more minutes than LdsMinutes holds (16)
    else:
        monkeypatch.delenv("FA_ROLLUP_GRID", raising=False)
    n = 6000
    rows = _path_rows(po, n, 3 + groups, groups)
    status = np.zeros(n, dtype=np.uint8)
    assert len(np.unique(rows["time_flow_start"] // 60)) > 16 and (groups < 1000 or len(np.unique(rows["src_as"])) > 256)
    with np.errstate(over="ignore"):
        assert int(rows["packets"].sum(dtype=np.uint64)) != sum(int(x) for x in rows["packets"])  # the sums do wrap
    with fa.FlowAgg(framed=True, key_sets=KS4) as agg:
        _fold_rows(fa, agg, rows, status)
        _check_against_rows(fa, po, agg, rows, status)
    if groups == 9:  # the mocker's own 9 groups (mocker.go:61-62), against a ctx that ingested them
        gp = po.gen_params(mode=po.GEN_MOCKER, framed=1, seed=4, n_total=n, per_sec=20)
        buf, off = po.gen_records(gp, 0, n)
        with fa.FlowAgg(framed=True, key_sets=KS4) as a, fa.FlowAgg(framed=True, key_sets=KS4) as b:
            a.ingest(buf, off)
            cols, keep = _decode_on_device(b, buf, off)
            b.rollup_fold_columns(cols, n)
            _equal_reads(_reads(b), _reads(a))
            assert len(np.unique(b.read_window()[["src_as", "dst_as"]])) == 9
            del keep


# ---- 5: growth -------------------------------------------------------------------------------------------------------------------------------
def test_growth(gpu_lib, fa, po):
    n = 5000
    rows = _as_rows(po, R.random_rows(21, n))  # every bit random: every record its own group in every key set
    rows["time_received"] = D0 * DAY + np.arange(n) % 300
    rows["time_flow_start"] = np.arange(n, dtype=np.uint64) * 60  # 5 000 minutes
    rows["src_port"] |= 1 << 16  # hashed ports on both sides
    rows["dst_port"] |= 1 << 17
    status = np.zeros(n, dtype=np.uint8)
    with fa.FlowAgg(framed=True, key_sets=KS4, table_capacity_log2=10, wide_capacity_log2=8) as agg:
        assert agg.stats()["table_capacity"] == 1 << 10 and agg.stats()["wide_capacity"] == 1 << 8
        _fold_rows(fa, agg, rows, status)  # (FA_ERR_TABLE_FULL would raise)
        st = agg.stats()
        assert st["table_used"] == len(_rollup_np(fa, po, rows, status)) > n - 3 and st["table_capacity"] >= 2 * st["table_used"]
        assert st["wide_used"] > 3 * n and st["wide_capacity"] >= 2 * st["wide_used"]
        _check_against_rows(fa, po, agg, rows, status)
        assert agg.rollup_stats()["launches"] == 1


# ---- 6: additive, and another granule ----------------------------------------------------------------------------------------------------------
def test_additive(gpu_lib, fa):
    buf, off, rows, status = _midnight(bad_every=97)
    h = len(rows) // 2
    b1, o1 = buf[:int(off[h])], off[:h + 1]
    b2, o2 = buf[int(off[h]):], off[h:] - off[h]
    with fa.FlowAgg(framed=True, key_sets=KS4) as c:
        c.raw_enable()
        c.ingest(b2, o2)
        frames2, _ = c.raw_take_lz4()
    with fa.FlowAgg(framed=True, key_sets=KS4) as a, fa.FlowAgg(framed=True, key_sets=KS4) as b:
        a.ingest(b1, o1)
        a.ingest(b2, o2)
        b.ingest(b1, o1)
        b.raw_load_rollup(frames2)
        _equal_reads(_reads(b), _reads(a))


@pytest.mark.parametrize("cfg", [dict(window_secs=3600), dict(window_secs=300, subwindow_secs=60)], ids=["3600", "sub60"])
def test_another_granule(gpu_lib, fa, po, ingested, cfg):
    buf, off, rows, status = _midnight(bad_every=97)
    gran = cfg.get("subwindow_secs") or cfg["window_secs"]
    ref = po.Rollup(granule=gran)
    ref.ingest(buf, off, 1)
    with fa.FlowAgg(framed=True, key_sets=KS4, **cfg) as b:
        b.raw_load_rollup(ingested["lz4_merged"])  # parts a 300 s ctx wrote
        got = b.read_window()
        assert len(got) > 0 and got.tobytes() == ref.rows().tobytes()
        assert b.read_window_app().tobytes() == po.rollup_app(rows, status, gran).tobytes()
        assert np.array_equal(b.open_timeslots(), np.unique(ref.rows()["timeslot"]))  # (the granule's buckets: 1 hour, or 10 minutes of 60 s)


# ---- 7: masks and refusals ------------------------------------------------------------------------------------------------------------------
def test_masks_and_refusals(gpu_lib, fa, ingested):
    with fa.FlowAgg(framed=True, key_sets=KS4) as b:
        b.raw_load_rollup(ingested["lz4"], key_sets=1)  # FA_KEYS_AS_PAIR alone
        r = _reads(b)
        assert r["rows"].tobytes() == ingested["reads"]["rows"].tobytes()
        assert len(r["app"]) == len(r["sport"]) == len(r["dport"]) == len(r["minutes"]) == 0 and b.stats()["wide_used"] == 0
    with fa.FlowAgg(framed=True, key_sets=1 | 16) as b:
        def reads2():  # (the reads of the key sets this ctx has)
            return dict(rows=b.read_window(), sport=b.top_ports(0), dport=b.top_ports(1), slots=b.open_timeslots())

        empty, before = reads2(), b.rollup_stats()
        cols, keep = _upload(fa, *_edge_rows(_po(), 100, 1))
        for door in (lambda ks: b.raw_load_rollup(ingested["lz4"], key_sets=ks), lambda ks: b.rollup_fold_columns(cols, 100, ks)):
            for ks, code in ((8, ERR_ARG), (32, ERR_ARG), (1 | 8, ERR_ARG), (64, ERR_ARG), (2, ERR_UNSUPPORTED), (4, ERR_UNSUPPORTED), (1 | 2, ERR_UNSUPPORTED), (8 | 4, ERR_UNSUPPORTED)):
                with pytest.raises(fa.FlowAggError, match="wire bytes only" if code == ERR_UNSUPPORTED else "not created with") as e:
                    door(ks)
                assert e.value.code == code, ks
        with pytest.raises(fa.FlowAggError, match="neither fa_talkers_enable") as e:
            b.raw_load_rollup(ingested["lz4"], folds=True)
        assert e.value.code == ERR_UNSUPPORTED
        # null and misaligned columns
        for name, value in (("bytes", None), ("status", None), ("src_port", None), ("time_received", cols.time_received + 4), ("src_as", cols.src_as + 2),
                            ("src_addr", cols.src_addr + 8)):  # (src_addr is not read by these key sets: whatever is given must be aligned)
            bad = fa.Columns()
            for f, _ in fa.Columns._fields_:
                setattr(bad, f, getattr(cols, f))
            setattr(bad, name, value)
            with pytest.raises(fa.FlowAggError, match="naturally aligned") as e:
                b.rollup_fold_columns(bad, 100)
            assert e.value.code == ERR_ARG, name
        with pytest.raises(fa.FlowAggError) as e:
            b.rollup_fold_columns(None, 100)
        assert e.value.code == ERR_ARG
        b.rollup_fold_columns(None, 0)  # n == 0: FA_OK, nothing looked at
        # a two-frame input whose second frame is broken: nothing is folded, the first frame included
        frames = ingested["lz4_merged"]
        cut = int(ingested["lz4_merged_parts"]["offset"][1])
        assert frames[cut:cut + 4] == b"\x04\x22\x4d\x18"
        broken = frames[:cut] + frames[cut:-9]
        with pytest.raises(fa.FlowAggError) as e:
            b.raw_load_rollup(broken)
        assert e.value.code == ERR_FRAMING
        _equal_reads(reads2(), empty, nonempty=False)
        assert b.rollup_stats() == before and before["calls"] == 0
        b.raw_load_rollup(frames)  # the ctx is usable
        assert b.read_window().tobytes() == ingested["reads"]["rows"].tobytes()
        assert b.top_ports(0).tobytes() == ingested["reads"]["sport"].tobytes() and b.top_ports(1).tobytes() == ingested["reads"]["dport"].tobytes()
        del keep


def _po():
    import _pkg
    return _pkg.load_oracle()


# ---- 8: folds=True ------------------------------------------------------------------------------------------------------------------------------
def test_with_folds(gpu_lib, fa, ingested):
    def ctx():
        a = fa.FlowAgg(framed=True, key_sets=KS4)
        a.talkers_enable(0, bucket_secs=60)
        a.ports_enable_buckets(0, bucket_secs=60)
        return a

    def ranged(a):
        return [a.top_talkers(d, 100, 0, NO_UPPER).tobytes() for d in (0, 1)] + [a.top_ports_range(d, 100, 0, NO_UPPER).tobytes() for d in (0, 1)]

    with ctx() as a, ctx() as b:
        a.raw_load(ingested["lz4"])
        b.raw_load_rollup(ingested["lz4"], folds=True)
        assert ranged(b) == ranged(a) and all(len(x) > 0 for x in ranged(b))
        _equal_reads(_reads(b), ingested["reads"])
        assert len(a.read_window()) == 0  # fa_raw_load keeps its contract: it never touches flows_5m
        assert b.talkers_stats()["records_folded"] == b.ports_stats()["records_folded"] == b.rollup_stats()["records_folded"] == ingested["good"]


# ---- 9: late -------------------------------------------------------------------------------------------------------------------------------------
def test_late_records(gpu_lib, fa, po, ingested):
    buf, off, rows, status = _midnight(bad_every=97)
    first = D0 * DAY - 300  # the stream's first timeslot
    t32 = (rows["time_received"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    k = int(((status == 0) & (t32 < first + 300)).sum())
    assert 0 < k < ingested["good"]
    with fa.FlowAgg(framed=True, key_sets=KS4) as b:
        b.ingest(buf, off)
        assert int(b.open_timeslots()[0]) == first
        closed = b.close_window(first)
        assert len(closed) > 0 and len(b.read_window(first)) == 0 and b.stats()["records_late"] == 0
        b.raw_load_rollup(ingested["plain"])
        assert b.stats()["records_late"] == k
        assert b.read_window(first).tobytes() == closed.tobytes()  # those rows are back: folded all the same
