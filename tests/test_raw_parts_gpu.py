"""GPU tests of the flows_raw parts (fa_raw_enable, fa_raw_build_columns_device, fa_raw_take, fa_raw_take_device, fa_raw_reset,
fa_raw_stats, the host program's -out.raw.native; include/flowagg.h "flows_raw parts built on the device").

The expected bytes are never taken from the code under test and not from flow-pipeline_amd/spill.py either: they are the
oracle's decode (po.decode_batch) or hand-made columns run through the numpy encoder below - rows[status == 0], a stable argsort
of t32 = TimeReceived & 0xFFFFFFFF, a split where t32 // 86400 changes, header + columns concatenated.  Whole parts are compared
with == on bytes.

The alignment sweep uses the row counts 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1025 and, because
those alone do not reach every start residue a part below 2^21 rows can have (computed in the test: a column's start moves by an
even number of bytes per row and by one byte per varuint step of the row count), also 6, 130 .. 134 and 16384.  Parts of 2^21
rows or more (a 4-byte varuint, chunk_records above the default) are not swept: they would put the Date column at residue 15 too.
Every count is built twice: at the image's aligned base, and behind a pending part of odd size."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_CAPACITY = -1, -6
DAY = 86400
D0 = 19000  # a Date; D0 * DAY is the midnight the streams straddle

# (name, type, numpy dtype of the values, field of the oracle's rows)
FORMAT = (("Date", "Date", "<u2", None), ("TimeReceived", "DateTime", "<u4", None), ("TimeFlowStart", "DateTime", "<u4", "time_flow_start"),
          ("SequenceNum", "UInt32", "<u4", "sequence_num"), ("SamplingRate", "UInt64", "<u8", "sampling_rate"),
          ("SamplerAddress", "FixedString(16)", "u1", "sampler_address"), ("SrcAddr", "FixedString(16)", "u1", "src_addr"),
          ("DstAddr", "FixedString(16)", "u1", "dst_addr"), ("SrcAS", "UInt32", "<u4", "src_as"), ("DstAS", "UInt32", "<u4", "dst_as"),
          ("EType", "UInt32", "<u4", "etype"), ("Proto", "UInt32", "<u4", "proto"), ("SrcPort", "UInt32", "<u4", "src_port"),
          ("DstPort", "UInt32", "<u4", "dst_port"), ("Bytes", "UInt64", "<u8", "bytes"), ("Packets", "UInt64", "<u8", "packets"))
WIDTH = {"<u2": 2, "<u4": 4, "<u8": 8, "u1": 16}


def varuint(v):
    out = b""
    while v >= 128:
        out += bytes([(v & 127) | 128])
        v >>= 7
    return out + bytes([v])


def t32_of(rows):
    return (rows["time_received"] & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def encode_part(r):
    """rows of one Date, already in their final order -> the part's bytes"""
    t = t32_of(r)
    out = [varuint(16), varuint(len(r))]
    for name, ctype, dt, field in FORMAT:
        out.append(varuint(len(name)) + name.encode() + varuint(len(ctype)) + ctype.encode())
        if name == "Date":
            col = (t // np.uint32(DAY)).astype("<u2")
        elif name == "TimeReceived":
            col = t.astype("<u4")
        elif name == "TimeFlowStart":
            col = (r[field] & np.uint64(0xFFFFFFFF)).astype("<u4")
        else:
            col = np.ascontiguousarray(r[field]).astype(dt)
        out.append(col.tobytes())
    return b"".join(out)


def expected_parts(rows, status):
    """-> [(date, rows of the part in order, bytes)] for ONE chunk"""
    r = rows[status == 0]
    r = r[np.argsort(t32_of(r), kind="stable")]
    date = t32_of(r) // np.uint32(DAY)
    cuts = [0] + (np.nonzero(date[1:] != date[:-1])[0] + 1).tolist() + [len(r)]
    return [(int(date[a]), r[a:b], encode_part(r[a:b])) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def column_starts(nrows):
    """byte offset of every column's first value inside a part of nrows rows"""
    o, out = 1 + len(varuint(nrows)), []
    for name, ctype, dt, _ in FORMAT:
        o += 2 + len(name) + len(ctype)
        out.append(o)
        o += nrows * WIDTH[dt]
    return out, o


def check_parts(data, parts, want):
    """the taken bytes and their descriptions against expected_parts' list (several chunks: the lists back to back)"""
    assert len(parts) == len(want), (len(parts), len(want))
    at = 0
    for p, (date, r, blob) in zip(parts, want):
        assert (int(p["date"]), int(p["rows"]), int(p["offset"]), int(p["bytes"])) == (date, len(r), at, len(blob))
        t = t32_of(r)
        assert (int(p["t_min"]), int(p["t_max"])) == (int(t[0]), int(t[-1]))
        got = bytes(data[at:at + len(blob)])
        if got != blob:
            bad = next(i for i in range(len(blob)) if got[i] != blob[i])
            starts, _ = column_starts(len(r))
            raise AssertionError("part of Date %d, %d rows: first differing byte %d (column starts %s)" % (date, len(r), bad, starts))
        at += len(blob)
    assert at == len(data)


@functools.lru_cache(maxsize=None)
def _midnight(n=20000, bad_every=0):
    """n GEN_ASPAIRS records whose TimeReceived runs from 300 s before a midnight to 300 s after it (33 per second), their
    slices permuted by a seeded permutation; bad_every: every such record truncated inside a LEN field.  Computed once, read-only."""
    import _pkg
    po = _pkg.load_oracle()
    gp = po.gen_params(mode=po.GEN_ASPAIRS, framed=1, seed=31, n_total=n, t0=D0 * DAY - 300, span_secs=600)
    buf, off = po.gen_records(gp, 0, n)
    raw = bytes(buf)
    recs = [raw[int(off[i]):int(off[i + 1])] for i in range(n)]
    if bad_every:
        for i in range(bad_every - 1, n, bad_every):
            recs[i] = _truncate_in_len_field(recs[i])
    recs = [recs[i] for i in np.random.default_rng(7).permutation(n)]
    buf = np.frombuffer(b"".join(recs), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    rows, status = po.decode_batch(buf, off, 1)
    for a in (buf, off, rows, status):
        a.setflags(write=False)
    return buf, off, rows, status


def _read_varint(b, p):
    v = s = 0
    while True:
        x = b[p]
        p += 1
        v |= (x & 127) << s
        s += 7
        if x < 128:
            return v, p


def _truncate_in_len_field(framed):
    """A framed record cut in the middle of its first length-delimited field's value, framed again with its new length."""
    _, p = _read_varint(framed, 0)
    payload = framed[p:]
    q = 0
    while q < len(payload):
        tag, q = _read_varint(payload, q)
        wt = tag & 7
        if wt == 0:
            _, q = _read_varint(payload, q)
        elif wt == 1:
            q += 8
        elif wt == 5:
            q += 4
        else:
            assert wt == 2
            ln, q = _read_varint(payload, q)
            assert ln >= 2
            cut = payload[:q + ln // 2]
            return varuint(len(cut)) + cut
    raise AssertionError("no LEN field in the record")


def _as_flow_rows(fa, r):
    out = np.zeros(len(r), dtype=fa.FLOW_ROW_DTYPE)
    for f in r.dtype.names:
        if f != "_pad":
            out[f] = r[f]
    return out


def _blocks_equal(fa, data, want):
    blocks = fa.spill.read_native(data)
    assert len(blocks) == len(want)
    for b, (date, r, _) in zip(blocks, want):
        assert (b["Date"] == date).all() and np.array_equal(b["TimeReceived"], t32_of(r))
        for name, _, _, field in FORMAT[2:]:
            col = (r[field] & np.uint64(0xFFFFFFFF)).astype(np.uint32) if name == "TimeFlowStart" else r[field]
            assert np.array_equal(b[name], col), name


# ---- 1, 2: one ingest of a shuffled stream across a midnight ---------------------------------------------------------------
def test_midnight_shuffled(gpu_lib, fa, po):
    buf, off, rows, status = _midnight()
    assert int(status.sum()) == 0
    want = expected_parts(rows, status)
    assert [w[0] for w in want] == [D0 - 1, D0]
    with fa.FlowAgg(framed=True) as agg:
        agg.raw_enable()
        agg.ingest(buf, off)
        data, parts = agg.raw_take()
        st = agg.raw_stats()
    assert len(parts) == 2
    check_parts(data, parts, want)
    assert st["records_in"] == st["rows_out"] == len(rows) and st["records_bad"] == 0 and st["parts_out"] == 2 and st["bytes_out"] == len(data)
    assert st["pending_parts"] == 0 and st["pending_bytes"] == 0
    # stability: inside equal t32 the rows keep the input's order, which SequenceNum (the generator's record index) shows
    blocks = fa.spill.read_native(data)
    inp = rows[np.argsort(t32_of(rows), kind="stable")]
    assert np.array_equal(np.concatenate([b["SequenceNum"] for b in blocks]), inp["sequence_num"])
    t = np.concatenate([b["TimeReceived"] for b in blocks])
    assert (np.diff(t.astype(np.int64)) >= 0).all() and (np.diff(t.astype(np.int64)) == 0).sum() > len(rows) // 2  # ties are plentiful
    _blocks_equal(fa, data, want)
    for _, r, blob in want:  # the host encoder over the oracle's rows of each part
        assert fa.flow_rows_to_native(_as_flow_rows(fa, r)) == blob


def test_bad_records_are_dropped(gpu_lib, fa, po):
    buf, off, rows, status = _midnight(bad_every=97)
    nbad = len(rows) // 97
    assert int(status.sum()) == nbad
    want = expected_parts(rows, status)
    with fa.FlowAgg(framed=True) as agg:
        agg.raw_enable()
        agg.ingest(buf, off)
        data, parts = agg.raw_take()
        st, ist = agg.raw_stats(), agg.stats()
    check_parts(data, parts, want)
    assert st["records_in"] == len(rows) and st["records_bad"] == nbad and st["rows_out"] + st["records_bad"] == st["records_in"]
    assert ist["records_bad"] == nbad
    assert sum(int(p["rows"]) for p in parts) == len(rows) - nbad


# ---- hand-made columns through fa_raw_build_columns_device -------------------------------------------------------------------
def _random_rows(po, n, seed, t):
    """n rows with random bytes in every column and the given TimeReceived values"""
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    raw = rng.integers(0, 256, size=(n, po.ROW_DTYPE.itemsize), dtype=np.uint8)
    rows[:] = raw.view(po.ROW_DTYPE).reshape(n)
    rows["_pad"] = 0
    rows["time_received"] = np.asarray(t, dtype=np.uint64)
    return rows


def _upload(fa, rows, status):
    """the 15 columns and status as torch tensors -> (Columns, the tensors that own the memory)"""
    import torch
    from device_columns import COLUMNS
    keep, cols = [], fa.Columns()
    for name, dt, _ in COLUMNS:
        a = np.ascontiguousarray((status if name == "status" else rows[name]).astype(dt))
        t = torch.zeros(max(a.nbytes, 1) + 16, dtype=torch.uint8, device="cuda")
        if a.nbytes:
            t[:a.nbytes].copy_(torch.from_numpy(a.view(np.uint8).reshape(-1).copy()))
        keep.append(t)
        setattr(cols, name, t.data_ptr())
    torch.cuda.synchronize()
    return cols, keep


def _build(fa, agg, rows, status):
    """fa_raw_build_columns_device is synchronous - "the columns are not referenced after the call": the columns are overwritten
    the moment it returns, on another stream and without any fa_sync, and every caller then compares the parts byte for byte."""
    import torch
    cols, keep = _upload(fa, rows, status)
    try:
        agg.raw_build_columns(cols, len(rows))
    finally:
        for t in keep:
            t.fill_(0xA5)
        torch.cuda.synchronize()


SWEEP = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1025)
SWEEP_EXTRA = (6, 130, 131, 132, 133, 134, 16384)


def test_alignment_sweep(gpu_lib, fa, po):
    # every start residue mod 16 of a part below 2^21 rows, per column: a start is 1 + len(varuint(rows)) + headers + rows * (an even
    # number), so it depends on rows mod 8 and on the varuint's length - 1, 2 or 3 bytes here; the 4-byte step (2^21 rows and more,
    # which only a chunk_records above the default reaches) is NOT swept, and would add residue 15 for the Date column
    producible = [set() for _ in FORMAT]
    for nrows in list(range(1, 17)) + list(range(128, 144)) + list(range(16384, 16400)):
        for c, s in enumerate(column_starts(nrows)[0]):
            producible[c].add(s % 16)
    swept = [set() for _ in FORMAT]
    for nrows in SWEEP + SWEEP_EXTRA:
        for c, s in enumerate(column_starts(nrows)[0]):
            swept[c].add(s % 16)
    assert swept == producible and all(len(s) == 16 for s in producible[1:]) and producible[0] == {12, 13, 14}
    with fa.FlowAgg(framed=True) as agg:
        agg.raw_enable()
        for nrows in SWEEP + SWEEP_EXTRA:
            t = D0 * DAY + np.random.default_rng(nrows).integers(0, 50, size=nrows)  # one Date, unsorted, ties
            rows = _random_rows(po, nrows, 100 + nrows, t)
            status = np.zeros(nrows, dtype=np.uint32)
            _build(fa, agg, rows, status)
            data, parts = agg.raw_take()  # (taken after every build: the part starts at the image's 256-byte aligned base)
            assert len(data) == column_starts(nrows)[1]
            check_parts(data, parts, expected_parts(rows, status))
        # once more behind a pending part of odd size: the absolute residue of a start differs from its offset inside the part
        fronts = set()
        for i, nrows in enumerate(SWEEP + SWEEP_EXTRA):
            nfront = 1 + i % 3
            front = _random_rows(po, nfront, 7, np.full(nfront, (D0 - 1) * DAY + 3))
            t = D0 * DAY + np.random.default_rng(nrows).integers(0, 50, size=nrows)
            rows = _random_rows(po, nrows, 200 + nrows, t)
            want = []
            for r in (front, rows):
                _build(fa, agg, r, np.zeros(len(r), dtype=np.uint32))
                want += expected_parts(r, np.zeros(len(r), dtype=np.uint32))
            fronts.add(len(want[0][2]) % 16)
            data, parts = agg.raw_take()
            check_parts(data, parts, want)
        assert len(fronts) == 3 and any(f % 2 for f in fronts)


def _date_cases(po):
    rng = np.random.default_rng(5)
    three = np.concatenate([np.full(40, (D0 + d) * DAY) + rng.integers(0, DAY, size=40) for d in (0, 1, 5)])
    edge = np.array([65536, 86399, 86400, 2**32 - 1], dtype=np.uint64)
    return {
        "three dates, two not adjacent": rng.permutation(three),
        "one row per date": np.array([(D0 + 5) * DAY + 7, D0 * DAY, (D0 + 1) * DAY + DAY - 1]),
        "one t32": np.full(300, D0 * DAY + 12345),
        "edges of the axis": rng.permutation(np.repeat(edge, 25)),
        "beyond 32 bits": rng.permutation(np.concatenate([np.full(20, 2**32 + D0 * DAY + 5), np.full(20, 7 * 2**32 + (D0 + 1) * DAY), np.full(20, D0 * DAY + 4)])),
    }


@pytest.mark.parametrize("case", ["three dates, two not adjacent", "one row per date", "one t32", "edges of the axis", "beyond 32 bits"])
def test_dates(gpu_lib, fa, po, case):
    t = _date_cases(po)[case].astype(np.uint64)
    rows = _random_rows(po, len(t), 11, t)
    status = np.zeros(len(t), dtype=np.uint32)
    if case == "edges of the axis":
        status[::9] = 1  # bad records carry the sort key 2^32 - 1 behind the good ones: a good record with that t32 stays in front
    want = expected_parts(rows, status)
    ndates = {"three dates, two not adjacent": 3, "one row per date": 3, "one t32": 1, "edges of the axis": 3, "beyond 32 bits": 2}[case]
    assert len(want) == ndates
    if case == "beyond 32 bits":  # narrowed: the three values fold onto two Dates of the 32-bit axis, and t32 drops the high word
        assert [w[0] for w in want] == [D0, D0 + 1] and int(t32_of(want[0][1]).max()) == D0 * DAY + 5 and len(want[0][1]) == 40
    if case == "edges of the axis":
        assert [w[0] for w in want] == [0, 1, 49710]
    with fa.FlowAgg(framed=True) as agg:
        agg.raw_enable()
        _build(fa, agg, rows, status)
        data, parts = agg.raw_take()
    check_parts(data, parts, want)
    assert [int(p["date"]) for p in parts] == sorted(int(p["date"]) for p in parts)


# ---- 5: chunk seams ------------------------------------------------------------------------------------------------------------
def test_chunk_seams(gpu_lib, fa, po):
    buf, off, rows, status = _midnight(bad_every=97)
    n = 10000
    end = int(off[n])
    want = []
    for a in range(0, n, 4096):
        want += expected_parts(rows[a:min(a + 4096, n)], status[a:min(a + 4096, n)])
    assert len(want) == 6  # three chunks, both Dates in each
    with fa.FlowAgg(framed=True) as agg:
        agg.raw_enable(chunk_records=4096)
        agg.ingest(buf[:end], off[:n + 1])
        st = agg.raw_stats()
        assert st["pending_parts"] == 6 and st["chunks"] == 3
        data, parts = agg.raw_take()
    check_parts(data, parts, want)


# ---- 6: the ingest is untouched, the decode is shared ------------------------------------------------------------------------------
def test_ingest_untouched_and_decode_shared(gpu_lib, fa, po):
    buf, off, rows, status = _midnight(bad_every=97)
    with fa.FlowAgg(framed=True) as plain, fa.FlowAgg(framed=True) as raw:
        raw.raw_enable()
        for x in (plain, raw):
            x.ingest(buf, off)
        assert raw.read_window().tobytes() == plain.read_window().tobytes()
    with fa.FlowAgg(framed=True) as talk, fa.FlowAgg(framed=True) as twin, fa.FlowAgg(framed=True) as full:
        talk.talkers_enable(0)
        for x in (twin, full):
            x.talkers_enable(0)
            x.ports_enable_buckets(0, 60)
        full.raw_enable()
        for x in (talk, twin, full):
            x.ingest(buf, off)
        for d in (0, 1):
            assert full.top_talkers(d).tobytes() == twin.top_talkers(d).tobytes() and len(full.top_talkers(d)) > 0
            assert full.top_ports_range(d).tobytes() == twin.top_ports_range(d).tobytes() and len(full.top_ports_range(d)) > 0
        assert full.read_window().tobytes() == twin.read_window().tobytes()
        assert full.stats()["decode_launches"] == talk.stats()["decode_launches"] >= 1
        data, parts = full.raw_take()
    check_parts(data, parts, expected_parts(rows, status))


# ---- 7: the take protocol ------------------------------------------------------------------------------------------------------------
def test_take_protocol(gpu_lib, fa, po):
    L = gpu_lib
    t = np.concatenate([np.full(30, D0 * DAY + 9), np.full(50, (D0 + 2) * DAY + 1)]).astype(np.uint64)
    rows = _random_rows(po, len(t), 21, t)
    status = np.zeros(len(t), dtype=np.uint32)
    want = expected_parts(rows, status)
    total = sum(len(w[2]) for w in want)
    nb, npart = C.c_size_t(), C.c_size_t()

    def take(agg, out, cap, parts, pcap):
        nb.value = npart.value = 12345
        return L.fa_raw_take(agg._h, out.ctypes.data if out is not None else None, cap, C.byref(nb), parts.ctypes.data, pcap, C.byref(npart))

    with fa.FlowAgg(framed=True) as off_ctx:  # not enabled: FA_ERR_ARG with a text, from every call but the enable
        parts = np.zeros(4, dtype=fa.RAW_PART_DTYPE)
        out = np.zeros(total, dtype=np.uint8)
        assert take(off_ctx, out, total, parts, 4) == ERR_ARG and b"fa_raw_enable" in L.fa_last_error(off_ctx._h)
        p = C.c_void_p()
        assert L.fa_raw_take_device(off_ctx._h, C.byref(p), C.byref(nb), parts.ctypes.data, 4, C.byref(npart)) == ERR_ARG
        assert L.fa_raw_reset(off_ctx._h) == ERR_ARG and L.fa_raw_stats(off_ctx._h, C.byref(fa.RawStats())) == ERR_ARG
        assert L.fa_raw_build_columns_device(off_ctx._h, C.byref(fa.Columns()), 0) == ERR_ARG
        off_ctx.raw_enable()
        assert L.fa_raw_enable(off_ctx._h, 0) == ERR_ARG  # a second enable
    with fa.FlowAgg(framed=True) as agg:
        agg.raw_enable()
        parts = np.zeros(4, dtype=fa.RAW_PART_DTYPE)
        out = np.zeros(total + 8, dtype=np.uint8)
        assert take(agg, out, out.size, parts, 4) == 0 and (nb.value, npart.value) == (0, 0)  # nothing pending
        assert L.fa_raw_build_columns_device(agg._h, C.byref(fa.Columns()), 0) == 0             # n == 0
        _build(fa, agg, rows, np.ones(len(t), dtype=np.uint32))                                # an all-bad chunk
        assert take(agg, out, out.size, parts, 4) == 0 and (nb.value, npart.value) == (0, 0)
        assert agg.raw_stats()["records_bad"] == len(t) and agg.raw_stats()["parts_out"] == 0
        _build(fa, agg, rows, status)
        for o, cap, pcap in ((out, total - 1, 4), (out, total, 1), (None, 0, 4)):
            assert take(agg, o, cap, parts, pcap) == ERR_CAPACITY and (nb.value, npart.value) == (total, 2)
            st = agg.raw_stats()
            assert st["pending_parts"] == 2 and st["pending_bytes"] == total  # nothing was consumed
        assert take(agg, out, total, parts, 2) == 0 and (nb.value, npart.value) == (total, 2)
        check_parts(out[:total], parts[:2], want)
        assert take(agg, out, total, parts, 2) == 0 and (nb.value, npart.value) == (0, 0)
        # fa_raw_reset drops what is pending
        _build(fa, agg, rows, status)
        assert agg.raw_stats()["pending_parts"] == 2
        agg.raw_reset()
        assert agg.raw_stats()["pending_parts"] == 0 and agg.raw_stats()["pending_bytes"] == 0
        assert take(agg, out, total, parts, 2) == 0 and (nb.value, npart.value) == (0, 0)
        # fa_raw_take_device + a copy == fa_raw_take
        _build(fa, agg, rows, status)
        ptr, nbytes, dparts = agg.raw_take_device()
        assert nbytes == total and ptr
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        dev = np.zeros(total, dtype=np.uint8)
        assert hip.hipMemcpy(dev.ctypes.data, ptr, total, 2) == 0  # hipMemcpyDeviceToHost
        check_parts(dev, dparts, want)
        assert dev.tobytes() == out[:total].tobytes() and agg.raw_stats()["pending_parts"] == 0


# ---- 8: the host program ---------------------------------------------------------------------------------------------------------------
def test_consumer_writes_native_blocks(gpu_lib, fa, po, tmp_path):
    buf, off, rows, status = _midnight(bad_every=97)
    exe = os.path.join(ROOT, "flow-pipeline_amd", "host", "inserter_gpu")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)], stdout=subprocess.DEVNULL)
    raw = bytes(buf)
    paths = []
    for p in range(2):  # record i lives in partition i mod 2
        path = tmp_path / ("p%d.log" % p)
        with open(path, "wb") as f:
            for k in range(p, len(rows), 2):
                f.write(raw[int(off[k]):int(off[k + 1])])
        paths.append(str(path))
    native, m = tmp_path / "flows_raw.native", tmp_path / "metrics.txt"
    r = subprocess.run([exe, "-input.files=" + ",".join(paths), "-flush.count=3000", "-gpu.batch.bytes=0", "-out.raw.native=%s" % native,
                        "-metrics.dump=%s" % m, "-gpu.devices=1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    blocks = fa.spill.read_native(open(native, "rb").read())
    assert len(blocks) >= 2 * 4  # two partitions, four flushes each, one or two Dates per flush
    for b in blocks:
        assert len(np.unique(b["Date"])) == 1 and (b["Date"] == b["TimeReceived"] // DAY).all()
        assert (np.diff(b["TimeReceived"].astype(np.int64)) >= 0).all()
    # rows as 110-byte strings, the values in column order: the file's against the oracle's good rows, as multisets
    got = np.concatenate([np.hstack([np.ascontiguousarray(b[name]).view(np.uint8).reshape(len(b["Date"]), -1) for name, _, _, _ in FORMAT]) for b in blocks])
    good = rows[status == 0]
    t = t32_of(good)
    cols = {"Date": (t // np.uint32(DAY)).astype("<u2"), "TimeReceived": t, "TimeFlowStart": (good["time_flow_start"] & np.uint64(0xFFFFFFFF)).astype("<u4")}
    want = np.hstack([np.ascontiguousarray(cols[name] if name in cols else good[field]).view(np.uint8).reshape(len(good), -1) for name, _, _, field in FORMAT])
    assert got.shape == want.shape == (len(rows) - len(rows) // 97, 110)
    assert sorted(r.tobytes() for r in got) == sorted(r.tobytes() for r in want)
    met = {l.split()[0]: int(l.split()[1]) for l in open(m) if not l.startswith("#")}
    assert met["flowagg_raw_rows_out"] == len(want) and met["flowagg_records_bad"] == len(rows) // 97
