"""GPU parity of the exact top talkers (fa_talkers_enable / fa_top_talkers, include/flowagg.h "ABI 8, addition"):
GROUP BY the rendered SrcAddr / DstAddr as the dashboards' panels do (viz-ch.json:233,479), bit-exact against a
restatement built here on the oracle's decode (po.decode_batch) and its group-by helper (po._group_sum) the way
pyoracle.top_ports is built.  Every comparison is np.array_equal on every column."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COLS = ("key", "etype", "weight", "count")
U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def concat(records):
    off = np.zeros(len(records) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in records])
    return np.frombuffer(b"".join(records), dtype=np.uint8), off


def _same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for c in COLS:
        assert np.array_equal(got[c], want[c]), (c, np.nonzero((got[c] != want[c]).reshape(len(got), -1).any(axis=1))[0][:10])


def restate(fa, po, rows, status, dst):
    """canonicalise; group by (key hi, key lo as big-endian words, family); order by inverted weight, key, family."""
    r = rows[status == 0]
    addr = np.ascontiguousarray(r["dst_addr" if dst else "src_addr"]).copy().reshape(-1, 16)
    v4 = r["etype"] == 0x800
    addr[v4, 4:] = 0
    fam = np.where(v4, 0x800, 0).astype(np.uint64)
    hi = addr[:, :8].copy().view(">u8").reshape(-1).astype(np.uint64)
    lo = addr[:, 8:].copy().view(">u8").reshape(-1).astype(np.uint64)
    with np.errstate(over="ignore"):
        w = r["bytes"] * r["sampling_rate"]
    idx, (ws, cs) = po._group_sum([hi, lo, fam], [w, np.ones(len(r), dtype=np.uint64)])
    out = np.zeros(len(idx), dtype=fa.TALKER_ROW_DTYPE)
    out["key"] = addr[idx]
    out["etype"] = fam[idx]
    out["weight"], out["count"] = ws, cs
    order = np.lexsort((fam[idx], lo[idx], hi[idx], U64MAX - out["weight"]))
    return out[order]


@functools.lru_cache(maxsize=None)
def _stream(mode, n, seed, zs=110, lu=24):
    """One generated framed stream, its decode and the expected rows of both directions - computed once, shared, read-only."""
    import _pkg
    fa, po = _pkg.load(), _pkg.load_oracle()
    gp = po.gen_params(mode=mode, framed=1, seed=seed, n_total=n, span_secs=900, per_sec=60, zipf_s_x100=zs, zipf_log2_universe=lu)
    buf, off = po.gen_records(gp, 0, n)
    rows, status = po.decode_batch(buf, off, 1)
    want = [restate(fa, po, rows, status, d) for d in (0, 1)]
    for a in (buf, off, rows, status, *want):
        a.setflags(write=False)
    return buf, off, rows, status, want


def test_mocker_stream_and_existing_results_untouched(gpu_lib, fa, po):
    n = 20000
    buf, off, rows, status, want = _stream(0, n, 71)
    ref = po.Rollup(300)
    ref.ingest(buf, off, 1)
    with fa.FlowAgg(framed=True) as plain, fa.FlowAgg(framed=True) as agg:
        plain.ingest(buf, off)
        agg.talkers_enable()
        agg.ingest(buf, off)
        for d in (0, 1):
            _same(agg.top_talkers(d), want[d])
        ts = agg.talkers_stats()
        assert ts["records_absorbed"] > 0  # a handful of addresses: the cache must be doing the work
        assert ts["records_folded"] == n - int(status.sum())
        assert agg.read_window().tobytes() == plain.read_window().tobytes() == ref.rows().tobytes()
        assert agg.stats()["records_ok"] == plain.stats()["records_ok"] == n - int(status.sum())


def test_zipf_with_growth(gpu_lib, fa, po):
    n = 200000
    buf, off, rows, status, want = _stream(2, n, 72, zs=80, lu=16)
    with fa.FlowAgg(framed=True) as agg:
        agg.talkers_enable(8)
        h = n // 3
        agg.ingest(buf[:int(off[h])], off[:h + 1])
        agg.ingest(buf[int(off[h]):], off[h:] - off[h])
        for d in (0, 1):
            _same(agg.top_talkers(d), want[d])
            _same(agg.top_talkers(d, 10), want[d][:10])
        ts = agg.talkers_stats()
        for d in (0, 1):
            assert ts["used"][d] == len(want[d])
            assert ts["capacity"][d] >= 2 * ts["used"][d]
        assert ts["grows"] >= 2
        assert ts["records_folded"] == agg.stats()["records_ok"] == n - int(status.sum())


# ---- hand-made columns through fa_talkers_fold_columns_device -------------------------------------------------------
def _fold(fa, agg, rows, status):
    """rows: po.ROW_DTYPE-shaped array (src_addr, dst_addr, etype, bytes, sampling_rate are used), status: uint8."""
    import torch
    n = len(rows)
    dev = torch.device("cuda", 0)

    def up(a, view):
        a = np.ascontiguousarray(a)
        if len(a) == 0:
            a = np.zeros((1,) + a.shape[1:], dtype=a.dtype)
        return torch.from_numpy(a.view(view).copy()).to(dev)
    keep = [up(rows["src_addr"], np.uint8), up(rows["dst_addr"], np.uint8), up(rows["etype"].astype(np.uint32), np.int32),
            up(rows["bytes"].astype(np.uint64), np.int64), up(rows["sampling_rate"].astype(np.uint64), np.int64), up(status.astype(np.uint8), np.uint8)]
    cols = fa.Columns()
    cols.src_addr, cols.dst_addr, cols.etype, cols.bytes, cols.sampling_rate, cols.status = [t.data_ptr() for t in keep]
    agg.fold_columns_device(cols, n)
    agg.sync()  # (the tensors may go once the stream has read them)


def _handmade(po, n, seed, pool=40):
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
    zero = pick[:, 0] < 3  # groups whose records all have weight 0 are still rows
    rows["sampling_rate"][zero] = 0
    status = (rng.random(n) < 0.1).astype(np.uint8)  # malformed rows carry garbage that must be skipped
    return rows, status


def test_handmade_columns_sizes_around_the_workgroup(gpu_lib, fa, po):
    sizes = [0, 1, 63, 64, 65, fa.TALK_BLOCK - 1, fa.TALK_BLOCK, fa.TALK_BLOCK + 1]
    with fa.FlowAgg(framed=True, max_batch_records=1 << 16) as agg:
        agg.talkers_enable(8)
        for n in sizes:
            rows, status = _handmade(po, n, 100 + n)
            agg.talkers_reset()
            _fold(fa, agg, rows, status)
            for d in (0, 1):
                want = restate(fa, po, rows, status.astype(np.uint32), d)
                got = agg.top_talkers(d)
                _same(got, want)
                if d == 0 and n >= fa.TALK_BLOCK - 1:  # zero-weight groups are rows, with their counts
                    assert (want["weight"] == 0).any() and (want["count"][want["weight"] == 0] > 0).all()


def test_handmade_one_key_wraps(gpu_lib, fa, po):
    n = 100000
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    rows["src_addr"] = np.arange(1, 17, dtype=np.uint8)
    rows["dst_addr"] = np.arange(1, 17, dtype=np.uint8)
    rows["etype"] = 0x86dd
    rows["bytes"] = (1 << 63) + 3
    rows["sampling_rate"] = 1 << 30
    status = np.zeros(n, dtype=np.uint8)
    with fa.FlowAgg(framed=True, max_batch_records=1 << 16) as agg:
        agg.talkers_enable(8)
        _fold(fa, agg, rows, status)
        for d in (0, 1):
            got = agg.top_talkers(d)
            _same(got, restate(fa, po, rows, status.astype(np.uint32), d))
            assert len(got) == 1 and int(got["count"][0]) == n
            assert int(got["weight"][0]) == (((1 << 63) + 3) * (1 << 30) * n) % (1 << 64)
        assert agg.talkers_stats()["records_absorbed"] > 0


def test_handmade_all_distinct_takes_the_global_path(gpu_lib, fa, po):
    import torch
    wgs = torch.cuda.get_device_properties(0).multi_processor_count * fa.TALK_WG_PER_CU
    n = 4 * fa.TALK_LDS_ENTRIES * wgs  # four times what every launched workgroup's cache holds
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    ids = np.arange(n, dtype=np.uint64)
    src = np.zeros((n, 16), dtype=np.uint8)
    src[:, :8] = (ids * np.uint64(0x9E3779B97F4A7C15)).view(np.uint8).reshape(n, 8)  # odd multiplier: a bijection
    src[:, 8:] = ids.view(np.uint8).reshape(n, 8)
    rows["src_addr"] = src
    rows["dst_addr"] = src[:, ::-1]
    rows["etype"] = 0x86dd
    rows["bytes"] = ids + np.uint64(1)
    rows["sampling_rate"] = 3
    status = np.zeros(n, dtype=np.uint8)
    log2 = int(np.ceil(np.log2(4 * n)))
    with fa.FlowAgg(framed=True, max_batch_records=1 << 16) as agg:
        agg.talkers_enable(log2)  # (chunk = capacity / 4 = n records: one launch, every workgroup sees 4 x its cache)
        _fold(fa, agg, rows, status)
        ts = agg.talkers_stats()
        assert 0 < ts["records_absorbed"] < 2 * n
        assert ts["used"] == [n, n] and ts["records_folded"] == n
        for d in (0, 1):
            _same(agg.top_talkers(d), restate(fa, po, rows, status.astype(np.uint32), d))


def test_handmade_tie_order(gpu_lib, fa, po):
    """1 000 distinct groups of equal weight: the order is key bytes ascending (memcmp), then etype ascending."""
    rng = np.random.default_rng(9)
    n = 1000
    a = np.zeros((n, 16), dtype=np.uint8)
    et = np.zeros(n, dtype=np.uint32)
    a[0:250, :15] = rng.integers(1, 256, size=15, dtype=np.uint8)  # IPv6 branch: keys that differ in the last byte only
    a[0:250, 15] = rng.permutation(256)[:250]
    a[250:500, 0] = np.arange(250)                                  # ... in the first byte only
    et[0:500] = 0x86dd
    a[500:750, :3] = 7                                              # IPv4 branch: heads that differ in their last byte
    a[500:750, 3] = rng.permutation(256)[:250]
    a[750:1000, 0] = np.arange(250)                                 # ... the same 16 canonical bytes as rows 250..499: told apart by the family
    a[500:1000, 4:] = rng.integers(0, 256, size=(500, 12), dtype=np.uint8)  # (tails the IPv4 branch ignores)
    et[500:1000] = 0x800
    shuffle = rng.permutation(n)
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    rows["src_addr"] = a[shuffle]
    rows["etype"] = et[shuffle]
    rows["dst_addr"] = a[shuffle]
    rows["bytes"] = 7
    rows["sampling_rate"] = 1
    status = np.zeros(n, dtype=np.uint8)
    with fa.FlowAgg(framed=True, max_batch_records=1 << 16) as agg:
        agg.talkers_enable(12)
        _fold(fa, agg, rows, status)
        for d in (0, 1):
            want = restate(fa, po, rows, status.astype(np.uint32), d)
            assert len(want) == n and (want["weight"] == 7).all() and (want["count"] == 1).all()
            _same(agg.top_talkers(d), want)
            _same(agg.top_talkers(d, 17), want[:17])


# ---- edge records through fa_ingest -------------------------------------------------------------------------------
def _enc(fa, fields):
    out = bytearray()
    for f, v in fields:
        if isinstance(v, (bytes, bytearray)):
            out += fa.schema.encode_varint((f << 3) | 2) + fa.schema.encode_varint(len(v)) + bytes(v)
        else:
            out += fa.schema.encode_varint(f << 3) + fa.schema.encode_varint(int(v))
    return bytes(out)


def test_edge_records_through_ingest(gpu_lib, fa, po):
    t0 = po.T0
    v4 = bytes([198, 51, 100, 7])
    v6 = bytes([0x20, 1, 0xd, 0xb8] + [0] * 11 + [9])

    def rec(src, dst, et, by=1500, sr=10, extra=()):
        f = [(2, t0 + 5), (3, sr)]
        if src is not None:
            f.append((6, src))
        if dst is not None:
            f.append((7, dst))
        f += [(9, by), (10, 3), (14, 64512), (15, 64600), (20, 6), (21, 443), (22, 53), (30, et)]
        f += list(extra)
        return [(k, v) for k, v in f if isinstance(v, (bytes, bytearray)) or v != 0]
    recs = []
    for i in range(8):  # EType 0x800, differing bytes 4..15 -> one group
        recs.append(_enc(fa, rec(v4 + bytes([i] * 12), v4 + bytes(11) + bytes([i]), 0x800)))
    for et in (0x800, 0x86dd):  # the same 16 bytes under both families -> two groups
        recs.append(_enc(fa, rec(v4 + bytes(12), v6, et)))
    for et in (0, 0x86dd, 0x1234):  # one group
        recs.append(_enc(fa, rec(v6, v4 + bytes([1] * 12), et)))
    for et in (0x800, 0x86dd, 0):  # missing address fields -> the 0.0.0.0 / :: groups
        recs.append(_enc(fa, rec(None, None, et)))
        recs.append(_enc(fa, rec(None, v6, et)))
    for et in (0x800, 0x86dd):  # a 4-byte address field
        recs.append(_enc(fa, rec(v4, v4, et)))
    recs.append(_enc(fa, rec(v6 + b"\x01", v6, 0x86dd)))  # an address field longer than 16 bytes: a bad record, dropped
    recs.append(_enc(fa, rec(v6, v6 + bytes(4), 0x800)))
    for et in (0x800, 0x86dd):  # fields in descending order
        recs.append(_enc(fa, rec(v6, v4 + bytes(12), et)[::-1]))
    whole = _enc(fa, rec(v6, v6, 0x86dd))
    recs.append(whole[:-1] + b"\xff")  # truncated varint
    recs.append(whole[:9])             # cut inside the SrcAddr field
    for et in (0x800, 0x86dd):  # SamplingRate 0 (and absent): weight 0, still counted
        recs.append(_enc(fa, rec(v4 + bytes(12), v6, et, sr=0)))
    recs.append(_enc(fa, rec(bytes([1, 1, 1, 1]) + bytes(12), bytes([2, 2, 2, 2]) + bytes(12), 0x800, sr=0)))  # groups of weight 0 only
    recs = recs * 3
    buf, off = concat(recs)
    rows, status = po.decode_batch(buf, off, 0)
    assert 0 < status.sum() < len(recs)
    want = [restate(fa, po, rows, status, d) for d in (0, 1)]
    render = lambda w: {(fa.format_addr(r["key"].tobytes(), int(r["etype"]))) for r in w}
    assert {"198.51.100.7", "c633:6407::", "2001:db8::9", "0.0.0.0", "::", "1.1.1.1"} <= render(want[0])
    assert {"2.2.2.2", "32.1.13.184"} <= render(want[1])
    assert (want[0]["weight"] == 0).any()
    with fa.FlowAgg(framed=False) as agg:
        agg.talkers_enable(8)
        agg.ingest(buf, off)
        for d in (0, 1):
            _same(agg.top_talkers(d), want[d])
        assert agg.talkers_stats()["records_folded"] == agg.stats()["records_ok"] == len(recs) - int(status.sum())


# ---- every ingest door ---------------------------------------------------------------------------------------------
def _pieces(buf, off, limit):
    """The stream cut at record boundaries into pieces of at most `limit` bytes."""
    out, i = [], 0
    n = len(off) - 1
    while i < n:
        j = int(np.searchsorted(off, off[i] + np.uint64(limit), side="right")) - 1
        j = min(max(j, i + 1), n)
        out.append((i, j))
        i = j
    return out


def test_every_ingest_door(gpu_lib, fa, po, monkeypatch):
    import torch
    n = 30000
    buf, off, rows, status, want = _stream(2, n, 73, zs=100, lu=14)
    assert len(buf) > (1 << 20)

    def check(agg):
        for d in (0, 1):
            _same(agg.top_talkers(d), want[d])
        assert agg.talkers_stats()["records_folded"] == n - int(status.sum())

    def door_offsets(agg):
        agg.ingest(buf, off)

    def door_host_walk(agg):
        for i, j in _pieces(buf, off, (1 << 20) - 1):
            assert int(off[j] - off[i]) < (1 << 20)
            agg.ingest(buf[int(off[i]):int(off[j])], None)

    def door_device_split(agg):
        agg.ingest(buf, None)

    def door_device(agg):
        dev = torch.device("cuda", 0)
        d_buf = torch.zeros(len(buf) + 64, dtype=torch.uint8, device=dev)
        d_buf[:len(buf)] = torch.from_numpy(np.array(buf)).to(dev)
        d_off = torch.from_numpy(off.astype(np.uint32).view(np.int32)).to(dev)
        agg.ingest_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), n)
        agg.sync()
    for door in (door_offsets, door_host_walk, door_device_split, door_device):
        with fa.FlowAgg(framed=True) as agg:
            agg.talkers_enable()
            door(agg)
            check(agg)
    # chunk and launch boundaries inside the stream
    monkeypatch.setenv("FA_TALK_CHUNK", "4096")
    for door in (door_offsets, door_device_split):
        with fa.FlowAgg(framed=True, max_batch_records=1 << 13) as agg:
            agg.talkers_enable(10)
            door(agg)
            check(agg)
            assert agg.talkers_stats()["fold_launches"] >= n // 4096


# ---- merge, reset, not enabled -----------------------------------------------------------------------------------------
def test_merge_reset_and_unsupported(gpu_lib, fa, po):
    n = 30000
    buf, off, rows, status, want = _stream(2, n, 73, zs=100, lu=14)
    h = n // 2
    with fa.FlowAgg(framed=True) as a, fa.FlowAgg(framed=True) as b:
        a.talkers_enable(10)
        b.talkers_enable()
        a.ingest(buf[:int(off[h])], off[:h + 1])
        b.ingest(buf[int(off[h]):], off[h:] - off[h])
        for d in (0, 1):
            a.merge_talkers(d, b.top_talkers(d))
        for d in (0, 1):
            _same(a.top_talkers(d), want[d])
        # a row that is not canonical: error -1, nothing merged
        bad = b.top_talkers(0)[:3].copy()
        for et, key4 in ((0x86dd, 0), (0x800, 1)):
            r = bad.copy()
            r["etype"][2] = et
            r["key"][2, 4] = key4
            if et == 0x800:
                r["key"][2, 5:] = 0
            with pytest.raises(fa.FlowAggError) as ei:
                a.merge_talkers(0, r)
            assert ei.value.code == -1
        for d in (0, 1):
            _same(a.top_talkers(d), want[d])
        a.talkers_reset()
        for d in (0, 1):
            assert len(a.top_talkers(d)) == 0
        assert a.talkers_stats()["used"] == [0, 0]
        a.ingest(buf, off)
        for d in (0, 1):
            _same(a.top_talkers(d), want[d])
    with fa.FlowAgg(framed=True) as plain:
        L, hnd = fa.lib(), plain._h
        n_out = C.c_size_t()
        row = np.zeros(1, dtype=fa.TALKER_ROW_DTYPE)
        cols = fa.Columns()
        st = fa.TalkersStats()
        assert L.fa_talkers_fold_columns_device(hnd, C.byref(cols), 1) == -8
        assert L.fa_top_talkers(hnd, 0, 0, row.ctypes.data, 1, C.byref(n_out)) == -8
        assert L.fa_merge_talkers(hnd, 0, row.ctypes.data, 1) == -8
        assert L.fa_talkers_reset(hnd) == -8
        assert L.fa_talkers_stats(hnd, C.byref(st)) == -8
        assert L.fa_talkers_enable(hnd, 7) == -1 and L.fa_talkers_enable(hnd, 31) == -1
        plain.talkers_enable()
        assert L.fa_talkers_enable(hnd, 0) == -1  # a second call
        assert len(plain.top_talkers(0)) == 0
