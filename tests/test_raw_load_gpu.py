"""GPU tests of loading flows_raw parts back (fa_lz4_decode_device, fa_raw_columns_device, fa_raw_load, fa_raw_load_stats; include/
flowagg.h "ABI 8, addition: loading flows_raw parts").

Expected bytes never come from the code under test: decoded bytes are the inputs the frames were made of (or what the tests'
own assembler built, tests/raw_load_cases.py), columns are the rows the tests' own numpy encoder wrote into the parts, and fold
results are those of a ctx that INGESTED the records, or a numpy group-by of the rows."""
import numpy as np
import pytest

import lz4_cases as Z
import raw_load_cases as R
from device_columns import fetch_columns
from test_raw_lz4_gpu import _fetch, _frame_device
from test_raw_parts_gpu import D0, DAY, _midnight
from test_talker_buckets_gpu import NO_UPPER, _same, restate

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_FRAMING, ERR_UNSUPPORTED = -1, -7, -8
M = D0 * DAY  # the midnight the ingested stream straddles
RANGES = ((0, NO_UPPER), (M - 60, M), (M - 120, M + 120), (M, M))  # every bucket, a single one, across the boundary, empty


def _decode(agg, frames):
    """lz4_decode_device -> the decoded bytes per frame; the spans' contract is asserted"""
    ptr, spans = agg.lz4_decode_device(frames)
    out, at = [], 0
    for s in spans:
        assert int(s["offset"]) % 65536 == 0 and int(s["offset"]) >= at
        out.append(_fetch(ptr + int(s["offset"]), int(s["bytes"])))
        at = int(s["offset"]) + int(s["bytes"])
    return out


def _stored(frames):
    return sum(1 for f in frames for stored, _ in Z.walk_frames(f)[0][1] if stored)


# ---- 1: decode edges -------------------------------------------------------------------------------------------------------------------
def test_decode_edges(gpu_lib, fa):
    inputs = [Z.pattern(p, n) for p in Z.PATTERNS for n in Z.EDGE_SIZES]
    with fa.FlowAgg(framed=True) as agg:  # (no fold, no fa_raw_enable: the door works on any ctx)
        host = [fa.lz4_frame(d) for d in inputs]
        dev = [_frame_device(agg, d) for d in inputs]
        for d, fh, fd in zip(inputs, host, dev):
            assert _decode(agg, fh) == [d] and _decode(agg, fd) == [d], len(d)
        st = agg.raw_load_stats()
        frames = host + dev
        assert st["calls"] == len(frames) and st["frames"] == len(frames)  # (an empty input still has a frame: header + EndMark)
        assert st["blocks"] == 2 * sum((len(d) + 65535) // 65536 for d in inputs) and st["stored_blocks"] == _stored(frames)
        assert st["bytes_in"] == sum(len(f) for f in frames) and st["bytes_decoded"] == 2 * sum(len(d) for d in inputs)
        assert st["parts"] == 0 and st["rows_loaded"] == 0 and st["launches"] == sum(1 for d in inputs if d) * 2 and st["decode_ns"] > 0
        # many frames in one call: every frame at its own 64 KiB-aligned base, in order
        assert _decode(agg, b"".join(dev)) == inputs
        st2 = agg.raw_load_stats()  # (more frames than the binding's first span buffer holds: refused by the host's walk, counted once)
        assert st2["calls"] == st["calls"] + 1 and st2["frames"] == st["frames"] + len(dev) and st2["bytes_in"] == st["bytes_in"] + sum(len(f) for f in dev)
        assert st2["launches"] == st["launches"] + 1
        assert _decode(agg, b"") == []
        # the buffers go without fa_raw_enable, the counters stay, the next call allocates again
        agg.raw_load_reset()
        assert agg.raw_load_stats() == st2
        assert _decode(agg, host[40]) == [inputs[40]]


# ---- 2: mixed inputs, another encoder's frames, assembled blocks -------------------------------------------------------------------------
def test_mixed_foreign_assembled(gpu_lib, fa):
    import test_raw_load_cpu as T
    with fa.FlowAgg(framed=True) as agg:
        mixed = list(Z.mixed_inputs())
        frames = [_frame_device(agg, d) for d in mixed]
        assert _decode(agg, b"".join(frames)) == mixed
        golden = T.golden_frames()
        assert _decode(agg, b"".join(f for _, _, f in golden)) == [d for _, d, _ in golden]
        valid = [(n, f, d) for n, f, d in R.assembled() if d is not None]
        got = _decode(agg, b"".join(f for _, f, _ in valid))
        for (name, _, d), g in zip(valid, got):
            assert g == d, name
        for name, f, d in R.assembled():
            if d is None:
                with pytest.raises(fa.FlowAggError, match="more than 65536") as e:
                    agg.lz4_decode_device(f)
                assert e.value.code == ERR_FRAMING, name


# ---- parts and contexts ---------------------------------------------------------------------------------------------------------------------
def _folds(fa, bucketed=True, raw=False, cap=0, **kw):
    agg = fa.FlowAgg(framed=True, **kw)
    agg.talkers_enable(cap, bucket_secs=60 if bucketed else 0)
    agg.ports_enable_buckets(cap, bucket_secs=60)
    if raw:
        agg.raw_enable()
    return agg


def _reads(agg, ranges=RANGES, bucketed=True):
    """every ranged read of both folds, both directions: {name: rows}"""
    out = {}
    for d in (0, 1):
        for lo, hi in ranges:
            if bucketed:
                out["talkers", d, lo, hi] = agg.top_talkers(d, 0, lo, hi)
            out["ports", d, lo, hi] = agg.top_ports_range(d, 0, lo, hi)
        if not bucketed:
            out["talkers", d] = agg.top_talkers(d)
    return out


def _equal_reads(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert sum(len(v) for v in a.values()) > 0


@pytest.fixture(scope="module")
def ingested(gpu_lib, fa):
    """ctx A of test 5, once: the midnight stream with a malformed record every 97th, ingested; its parts as frames and plain"""
    buf, off, rows, status = _midnight(bad_every=97)
    good = int((status == 0).sum())
    with _folds(fa, raw=True) as a:
        a.ingest(buf, off)
        frames, parts = a.raw_take_lz4()
        reads = _reads(a)
        stats = a.talkers_stats(), a.ports_stats()
    with _folds(fa, raw=True) as a:
        a.ingest(buf, off)
        plain, pparts = a.raw_take()
    with _folds(fa, bucketed=False) as a:
        a.ingest(buf, off)
        unbucketed = _reads(a, bucketed=False)
    assert len(parts) == len(pparts) == 2 and int(parts["rows"].sum()) == good and [int(x) for x in parts["date"]] == [D0 - 1, D0]
    return dict(frames=frames, parts=parts, plain=plain, reads=reads, stats=stats, good=good, unbucketed=unbucketed)


# ---- 3: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_lib, fa, ingested):
    cases = R.malformed(fa.spill._xxh32)
    with _folds(fa) as b:
        before = b.talkers_stats(), b.ports_stats()
        for name, data, text in cases:
            for door in (b.raw_load, b.raw_columns, b.lz4_decode_device):
                with pytest.raises(fa.FlowAggError, match=text) as e:
                    door(data)
                assert e.value.code == ERR_FRAMING, name
            # behind a valid frame too: the valid one is not folded either
            with pytest.raises(fa.FlowAggError, match=text) as e:
                b.raw_load(ingested["frames"] + data)
            assert e.value.code == ERR_FRAMING, name
        assert (b.talkers_stats(), b.ports_stats()) == before and b.raw_load_stats()["rows_loaded"] == 0
        b.raw_load(ingested["frames"])  # the ctx is usable
        _equal_reads(_reads(b), ingested["reads"])


# ---- 4: alignment sweep --------------------------------------------------------------------------------------------------------------------
SWEEP = tuple(range(1, 41)) + (127, 128, 129, 16383, 16384)


def _check_columns(got, rows, n):
    for name, _, _, field, dt in R.NATIVE_COLUMNS[1:]:
        want = rows[name]
        if dt == "V16":
            assert np.array_equal(got[field], want), name
        else:
            assert got[field].dtype == np.dtype(dt) and np.array_equal(got[field], want.astype(dt)), name  # (the two times: zero-extended)
    assert got["status"].shape == (n,) and not got["status"].any()


def test_alignment_sweep(gpu_lib, fa):
    # The sweep covers every byte phase mod 16 a column can start at in the image, and headers of every length below 2^21 rows.
    # A part alone starts at an aligned base (11 of the 16 phases occur for each column); the parts of up to 129 rows back to
    # back in ONE call (below: eight rounds, a part of 2 rows between them moves the next round by 2 bytes) start at every phase.
    small = [n for n in SWEEP if n <= 129]
    order = (small + [2]) * 8
    starts = {c: set() for c in range(1, 16)}
    base = 0
    for n in order:
        at = base + 1 + len(R.varuint(n))
        for c, (name, ctype, dt, _, _) in enumerate(R.NATIVE_COLUMNS):
            at += 2 + len(name) + len(ctype)
            if c:
                starts[c].add(at % 16)
            at += n * np.dtype(dt).itemsize
        base = at
    assert all(len(s) == 16 for s in starts.values()), {c: sorted(s) for c, s in starts.items()}
    assert {len(R.varuint(n)) for n in SWEEP} == {1, 2, 3}
    rows = {n: R.random_rows(1000 + n, n) for n in SWEEP}
    parts = {n: R.native_part(rows[n]) for n in SWEEP}
    assert all(len(parts[n]) == R.part_bytes(n) for n in SWEEP)
    with fa.FlowAgg(framed=True) as agg:
        for n in SWEEP:
            for data in (parts[n], fa.lz4_frame(parts[n])):
                cols, k = agg.raw_columns(data)
                assert k == n
                _check_columns(fetch_columns(cols, n), rows[n], n)
        # every part of the call in ONE block, in input order: a part then starts at any element of the arrays
        total = sum(order)
        for data in (b"".join(parts[n] for n in order), b"".join(fa.lz4_frame(parts[n]) for n in small)):
            cols, k = agg.raw_columns(data)
            want = order if data[0] == 0x10 else small
            assert k == sum(want) and (want is small or k == total)
            _check_columns(fetch_columns(cols, k), R.concat_rows([rows[n] for n in want]), k)
        assert agg.raw_columns(b"") [1] == 0
        st = agg.raw_load_stats()
        assert st["parts"] == 2 * len(SWEEP) + len(order) + len(small) and st["rows_loaded"] == 0


# ---- 5: load parity across a Date boundary -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["frames", "plain"])
def test_load_parity_across_midnight(gpu_lib, fa, ingested, form):
    with _folds(fa) as b:
        b.raw_load(ingested[form])
        _equal_reads(_reads(b), ingested["reads"])
        ts, ps = b.talkers_stats(), b.ports_stats()
        assert ts["records_folded"] == ps["records_folded"] == ingested["good"]
        assert ts["used"] == ingested["stats"][0]["used"] and ps["used"] == ingested["stats"][1]["used"]
        st = b.raw_load_stats()
        assert st["calls"] == 1 and st["parts"] == 2 and st["rows_loaded"] == ingested["good"] and st["bytes_in"] == len(ingested[form])
        assert st["frames"] == (2 if form == "frames" else 0) and st["unpack_ns"] > 0 and st["fold_ns"] > 0
        assert (st["bytes_decoded"] == len(ingested["plain"])) if form == "frames" else (st["blocks"] == 0)
    with _folds(fa, bucketed=False) as b:  # plain fa_talkers_enable
        b.raw_load(ingested[form])
        _equal_reads(_reads(b, bucketed=False), ingested["unbucketed"])
        b.raw_load_reset()  # a ctx that only loads has no fa_raw_enable: its buffers are released here, the folded state stays
        _equal_reads(_reads(b, bucketed=False), ingested["unbucketed"])
        with pytest.raises(fa.FlowAggError) as e:
            b.raw_reset()
        assert e.value.code == ERR_ARG


# ---- 6: chunk seams --------------------------------------------------------------------------------------------------------------------------
def _as_rows(po, r):
    out = np.zeros(len(r["TimeReceived"]), dtype=po.ROW_DTYPE)
    for name, _, _, field, _ in R.NATIVE_COLUMNS[1:]:
        out[field] = r[name]
    return out


def _port_group_by(fa, r, dst):
    port = r["DstPort" if dst else "SrcPort"].astype(np.uint64)
    with np.errstate(over="ignore"):
        w = r["Bytes"] * r["SamplingRate"]
    keys, inv = np.unique(port, return_inverse=True)
    ws, cs = np.zeros(len(keys), dtype=np.uint64), np.zeros(len(keys), dtype=np.uint64)
    np.add.at(ws, inv, w)
    np.add.at(cs, inv, np.uint64(1))
    out = np.zeros(len(keys), dtype=fa.PORT_ROW_DTYPE)
    out["port"], out["weight"], out["count"] = keys, ws, cs
    return out[np.lexsort((keys, np.uint64(0xFFFFFFFFFFFFFFFF) - ws))]


@pytest.mark.parametrize("n", [65535, 65536, 65537, 200000])
def test_chunk_seams(gpu_lib, fa, po, monkeypatch, n):
    r = R.random_rows(77 + n, n, keys=5000)
    part = R.native_part(r)
    monkeypatch.setenv("FA_TALK_CHUNK", "65536")
    with _folds(fa) as b:
        b.raw_load(fa.lz4_frame(part))
        chunked = _reads(b, ranges=((0, NO_UPPER),))
        assert b.talkers_stats()["fold_launches"] == (n + 65535) // 65536 == b.ports_stats()["fold_launches"]
    monkeypatch.delenv("FA_TALK_CHUNK")
    with _folds(fa, cap=20) as b:  # chunks of up to 2^18 rows: the whole part in one
        b.raw_load(part)
        single = _reads(b, ranges=((0, NO_UPPER),))
        assert b.talkers_stats()["fold_launches"] == 1
    _equal_reads(chunked, single)
    rows = _as_rows(po, r)
    status = np.zeros(n, dtype=np.uint8)
    for d in (0, 1):
        _same(single["talkers", d, 0, NO_UPPER], restate(fa, po, rows, status, d))
        want = _port_group_by(fa, r, d)
        got = single["ports", d, 0, NO_UPPER]
        assert all(np.array_equal(got[c], want[c]) for c in ("port", "weight", "count"))


# ---- 7: several parts in one call ----------------------------------------------------------------------------------------------------------
def test_several_parts_and_adding(gpu_lib, fa, ingested):
    buf, off, rows, status = _midnight(bad_every=97)
    with fa.FlowAgg(framed=True) as a:
        a.raw_enable(7000)  # three chunks x two Dates
        a.ingest(buf, off)
        frames, parts = a.raw_take_lz4()
    assert len(parts) == 6 and len(set(int(d) for d in parts["date"])) == 2
    with _folds(fa) as b:
        b.raw_load(b"")  # n == 0: nothing
        assert b.talkers_stats()["records_folded"] == 0
        b.raw_load(frames)
        _equal_reads(_reads(b), ingested["reads"])
        assert b.raw_load_stats()["parts"] == 6
    cut = int(parts["offset"][3])
    with _folds(fa) as b:  # two loads of halves
        b.raw_load(frames[:cut])
        b.raw_load(frames[cut:])
        _equal_reads(_reads(b), ingested["reads"])
    with _folds(fa) as b:  # on top of ingested state: sums commute
        b.ingest(buf, off)
        b.raw_load(frames)
        twice = _reads(b)
        for k, want in ingested["reads"].items():
            want = want.copy()
            want["weight"] *= 2
            want["count"] *= 2
            assert twice[k].tobytes() == want.tobytes(), k


# ---- 8: Native refusals ------------------------------------------------------------------------------------------------------------------------
def test_native_refusals(gpu_lib, fa, ingested):
    r = R.random_rows(9, 300, keys=50)
    good = R.native_part(r)
    bad = [
        ("a wrong name", R.native_part(r, names={6: "SrcAddx"}), "column 6 has a wrong name"),
        ("a wrong type", R.native_part(r, types={14: "UInt32"}), "column 14 has a wrong type"),
        ("15 columns", R.native_part(r, ncols=15), "16 columns|no row count|row count"),
        ("a size that fits no row count", good[:-7], "no row count|does not fit"),
        ("a trailing byte", good + b"\x00", "no row count|no such block starts|trailing"),
    ]
    with _folds(fa, raw=True) as b:
        before = b.talkers_stats(), b.ports_stats()
        for name, data, text in bad:
            for payload in (data, fa.lz4_frame(data), good + data, fa.lz4_frame(good) + fa.lz4_frame(data)):  # alone, and behind a valid FIRST part
                for door in (b.raw_load, b.raw_columns):
                    with pytest.raises(fa.FlowAggError, match=text) as e:
                        door(payload)
                    assert e.value.code == ERR_FRAMING, name
        for payload, text in ((fa.lz4_frame(good) + good, "no frame magic"), (good + fa.lz4_frame(good), "no such block starts")):  # the two forms mixed
            with pytest.raises(fa.FlowAggError, match=text) as e:
                b.raw_load(payload)
            assert e.value.code == ERR_FRAMING
        with pytest.raises(fa.FlowAggError, match="neither an LZ4 frame nor") as e:
            b.raw_load(b"\x00\x01\x02\x03\x04")
        assert e.value.code == ERR_FRAMING
        assert (b.talkers_stats(), b.ports_stats()) == before  # nothing was folded, the valid first parts included
        # a ctx with fa_raw_enable that loads gets no pending part: loading parts does not produce parts
        b.raw_load(ingested["frames"])
        rs = b.raw_stats()
        assert rs["pending_parts"] == 0 and rs["records_in"] == 0 and rs["parts_out"] == 0
        _equal_reads(_reads(b), ingested["reads"])
    with fa.FlowAgg(framed=True) as c:  # no fold enabled
        with pytest.raises(fa.FlowAggError, match="neither fa_talkers_enable") as e:
            c.raw_load(ingested["frames"])
        assert e.value.code == ERR_UNSUPPORTED
        cols, k = c.raw_columns(ingested["frames"])  # ... the doors without a fold work on any ctx
        assert k == ingested["good"]
