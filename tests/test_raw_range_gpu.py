"""Ranged loads of flows_raw parts (include/flowagg.h "ranged loads of flows_raw parts") on the GPU: fa_raw_restore_range equals a
twin that ingested only the wire records of the range, in four forms of the input and over the ranges that matter; the probe's row
ranges equal numpy.searchsorted at every byte phase of the TimeReceived column; an unsorted part or a row of another Date is
refused by both doors and by neither whole-file door; only the blocks the three stages need are decoded; refusals and counters."""
import ctypes as C
import functools
import struct

import numpy as np
import pytest

from test_raw_parts_gpu import D0, DAY, _as_flow_rows, _midnight, column_starts, t32_of, varuint, FORMAT, WIDTH
from test_sketch_fold_gpu import SRC, DST, SETS, _all_reads, _check_oracle, _ctx, _full_ctx, _oracle

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_FRAMING = -1, -6, -7
NO_UPPER = 0xFFFFFFFF
MID = D0 * DAY  # the midnight the stream straddles
SLOT = 65536
FORMS = ("lz4", "lz4_merged", "plain", "plain_merged")


def _same(got, want, nonempty=None):
    assert got.keys() == want.keys()
    for k in got:
        assert got[k].tobytes() == want[k].tobytes(), k
    if nonempty is not None:
        assert any(len(v) for k, v in got.items() if k[0] != "cms") == nonempty  # (a sketch's counters always have their length)


def _subset(buf, off, keep):
    """the wire records `keep` (a boolean mask), in their order -> (bytes, offsets)"""
    idx = np.nonzero(keep)[0]
    raw = bytes(buf)
    recs = [raw[int(off[i]):int(off[i + 1])] for i in idx]
    o = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)
    return np.frombuffer(b"".join(recs), dtype=np.uint8), o


def _in_range(t, lo, hi):
    return (t >= lo) & ((t < hi) | (hi == NO_UPPER))


# ---- 1: equal to a twin ---------------------------------------------------------------------------------------------------------------------------
N1 = 6000


@pytest.fixture(scope="module")
def stream(gpu_lib, fa):
    buf, off, rows, status = _midnight(n=N1, bad_every=97)
    out = dict(buf=buf, off=off, t=t32_of(rows), good=status == 0)
    for form in FORMS:
        with fa.FlowAgg(framed=True) as a:
            a.raw_enable(2100)  # three chunks x two Dates
            a.ingest(buf, off)
            if form.endswith("_merged"):
                a.raw_merge()
            data, parts = a.raw_take_lz4() if form.startswith("lz4") else a.raw_take()
            assert len(parts) == (2 if form.endswith("_merged") else 6)
            out[form] = bytes(data)
    return out


def _ranges(stream):
    t = stream["t"][stream["good"]]
    tmin, tmax = int(t.min()), int(t.max())
    vals, counts = np.unique(t, return_counts=True)
    busy = int(vals[np.argmax(counts)])
    assert counts.max() > 5 and tmin < MID - 100 and tmax > MID + 100
    return {"everything": (0, NO_UPPER), "empty": (MID, MID), "before all": (0, tmin), "after all": (tmax + 1, NO_UPPER), "one second": (busy, busy + 1),
            "[t_min, t_max + 1)": (tmin, tmax + 1), "[t_min + 1, t_max)": (tmin + 1, tmax), "across midnight": (MID - 40, MID + 25), "one Date": (MID, MID + DAY),
            "the other Date, to the end of its rows": (MID - DAY, MID)}


@functools.lru_cache(maxsize=None)
def _twin_reads(fa, lo, hi):
    buf, off, rows, status = _midnight(n=N1, bad_every=97)
    keep = (status == 0) & _in_range(t32_of(rows), lo, hi)
    with _full_ctx(fa) as a:
        if keep.any():
            a.ingest(*_subset(buf, off, keep))
        return _all_reads(a), int(keep.sum())


@pytest.mark.parametrize("form", FORMS)
def test_equal_to_a_twin(gpu_lib, fa, stream, form):
    for name, (lo, hi) in _ranges(stream).items():
        want, n = _twin_reads(fa, lo, hi)
        with _full_ctx(fa) as b:
            b.raw_restore_range(stream[form], lo, hi, 0, True)
            _same(_all_reads(b), want, nonempty=n > 0)
            st, ls = b.raw_range_stats(), b.raw_load_stats()
            assert st["rows_loaded"] == ls["rows_loaded"] == n, name
            assert st["calls"] == 1 and st["rows_seen"] == int(stream["good"].sum()) and st["parts_seen"] == (2 if form.endswith("_merged") else 6)
            assert b.stats()["records_ok"] == b.stats()["bytes_in"] == 0


def test_two_ranges_in_either_order_equal_their_union(gpu_lib, fa, stream):
    a_, b_, c_ = MID - 200, MID - 10, MID + 150
    want, n = _twin_reads(fa, a_, c_)
    assert n > 0
    for first, second in (((a_, b_), (b_, c_)), ((b_, c_), (a_, b_))):
        with _full_ctx(fa) as x:
            x.raw_restore_range(stream["lz4_merged"], *first, 0, True)
            x.raw_restore_range(stream["plain"], *second, 0, True)
            _same(_all_reads(x), want, nonempty=True)


def test_candidates_chunks_of_ranged_rows_are_batches(gpu_lib, fa, po, stream):
    """the documented chunk cuts are the batches: each part's slice, cut at the cap (max_batch_records = 300 here)"""
    buf, off, rows, status = _midnight(n=N1, bad_every=97)
    lo, hi, cap = MID - 150, MID + 120, 300
    from test_raw_parts_gpu import expected_parts
    parts = [r for c0 in range(0, len(rows), 2100) for _, r, _ in expected_parts(rows[c0:c0 + 2100], status[c0:c0 + 2100])]  # the six parts' rows, in take order
    slices = [r[_in_range(t32_of(r), lo, hi)] for r in parts]
    assert len(parts) == 6 and max(len(s) for s in slices) > cap and min(len(s) for s in slices) > 0
    batches = [s[i:i + cap] for s in slices for i in range(0, len(s), cap)]
    track, tcap = 64, 12
    with _ctx(fa, key_sets=1 | SRC | DST, cap=tcap, topk_mode=fa.TOPK_CANDIDATES, topk_track=track, max_batch_records=cap) as b:
        b.raw_restore_range(stream["plain"], lo, hi, SRC | DST)
        _check_oracle(po, b, batches, "ranged parts", track, tcap)
        fs = b.sketch_fold_stats()
        assert fs["batches"] == len(batches) and fs["records_in"] == sum(len(s) for s in slices)
        assert len(b.read_window()) == 0  # flows_5m was not selected


# ---- 2: probe geometry ------------------------------------------------------------------------------------------------------------------------------
ROWS2 = (1, 2, 3, 4, 5, 63, 64, 65) + tuple(range(120, 136)) + tuple(range(1023, 1033)) + tuple(range(16380, 16391))
SMALL2 = 65


@pytest.fixture(scope="module")
def geometry(gpu_lib, fa, po):
    """plain parts of one Date, one per row count (the varuint(rows) steps at 128 and 16384 shift the column's phase), runs of equal
    times -> [(the part, its times)]"""
    rng = np.random.default_rng(5)
    out = []
    for n in ROWS2:
        t = np.sort(MID + 1000 + rng.integers(0, max(2, n // 3), n)).astype(np.uint64)
        rows = np.zeros(n, dtype=po.ROW_DTYPE)
        rows["time_received"] = t
        rows["bytes"] = rng.integers(1, 1000, n)
        blob = fa.flow_rows_to_native(_as_flow_rows(fa, rows))
        assert len(blob) == column_starts(n)[1]
        out.append((blob, t.astype(np.uint32)))
    return out


def _probe_all(fa, a, parts, pairs):
    """every part in ONE call per pair of bounds: the probe answers per part"""
    data, times = b"".join(p for p, _ in parts), [t for _, t in parts]
    for lo, hi in pairs:
        got = a.raw_range_probe(data, lo, hi)
        assert len(got) == len(times)
        hi_ex = 1 << 32 if hi == NO_UPPER else hi
        meets = max(lo, MID) < min(hi_ex, MID + DAY)  # the Date can meet the range: otherwise the part is skipped, (0, 0)
        for g, t in zip(got, times):
            r_lo = int(np.searchsorted(t, lo, side="left")) if meets else 0
            r_hi = (len(t) if hi == NO_UPPER else int(np.searchsorted(t, hi, side="left"))) if meets else 0
            sel = t[r_lo:r_hi]
            want = (D0, len(t), r_lo, r_hi, int(sel.min()) if len(sel) else 0, int(sel.max()) if len(sel) else 0)
            assert (int(g["date"]), int(g["rows"]), int(g["r_lo"]), int(g["r_hi"]), int(g["t_min"]), int(g["t_max"])) == want, (lo, hi, len(t))


def _pairs(bounds, steps):
    bounds = sorted(bounds)
    return sorted({(bounds[i], bounds[min(i + d, len(bounds) - 1)]) for i in range(len(bounds)) for d in steps})


def test_probe_equals_searchsorted(gpu_lib, fa, geometry):
    edges = {0, NO_UPPER, MID - 1, MID, MID + DAY - 1, MID + DAY, MID + DAY + 1}
    light = [p for p in geometry if len(p[1]) < 2000]   # every pair of bounds goes to these in one call of 1.3 MB ...
    heavy = [p for p in geometry if len(p[1]) >= 2000]  # ... and a shorter list to the eleven parts of 1.8 MB each
    assert len(light) + len(heavy) == len(ROWS2) and len(heavy) == 11
    bounds = set(edges)
    for i, (_, t) in enumerate(light):
        if len(t) <= SMALL2:  # one below, at and one above every distinct time of the small parts
            for v in np.unique(t):
                bounds |= {int(v) - 1, int(v), int(v) + 1}
        elif i % 2 == 0:
            bounds |= {int(t[0]), int(t[-1]), int(t[len(t) // 2])}  # the first row, the last row, inside a run
    light_pairs = _pairs(bounds, (0, 1, len(bounds)))
    bounds = set(edges)
    for _, t in (heavy[0], heavy[4], heavy[-1]):  # 16380, 16384, 16390 rows
        bounds |= {int(t[0]), int(t[-1]), int(t[len(t) // 2]), int(t[len(t) // 2]) + 1}
    heavy_pairs = _pairs(bounds, (0, 1, len(bounds)))
    assert 100 < len(light_pairs) and len(heavy_pairs) > 20 and len(light_pairs) + len(heavy_pairs) <= 300
    with fa.FlowAgg(framed=True) as a:
        _probe_all(fa, a, light, light_pairs)
        _probe_all(fa, a, heavy, heavy_pairs)
        st = a.raw_range_stats()
        assert st["calls"] == len(light_pairs) + len(heavy_pairs) and st["parts_seen"] == len(light_pairs) * len(light) + len(heavy_pairs) * len(heavy)
        assert st["rows_loaded"] == 0 and st["blocks_seen"] == 0 and a.raw_load_stats()["rows_loaded"] == 0


def test_probe_of_a_part_whose_row_count_takes_four_bytes(gpu_lib, fa, po):
    """from 2^21 rows on varuint(rows) has four bytes and Date[0] stands at bytes 15 and 16 of the part: behind the first 16"""
    n = (1 << 21) + 3
    rows = np.zeros(n, dtype=fa.FLOW_ROW_DTYPE)
    t = (MID + np.arange(n, dtype=np.uint64) // 25).astype(np.uint32)  # 25 rows a second: 83 887 s, one Date
    rows["time_received"] = t
    part = fa.flow_rows_to_native(rows)
    del rows
    assert part[:5] == bytes([16]) + varuint(n) and len(varuint(n)) == 4 and part[15:17] == struct.pack("<H", D0)
    lo, hi = MID + 40000, MID + 40010
    with fa.FlowAgg(framed=True) as a:
        (g,) = a.raw_range_probe(part, lo, hi)
        want = (D0, n, int(np.searchsorted(t, lo)), int(np.searchsorted(t, hi)), lo, hi - 1)
        assert (int(g["date"]), int(g["rows"]), int(g["r_lo"]), int(g["r_hi"]), int(g["t_min"]), int(g["t_max"])) == want
        (g,) = a.raw_range_probe(part, MID + DAY, NO_UPPER)  # skipped by Date
        assert (int(g["date"]), int(g["rows"]), int(g["r_lo"]), int(g["r_hi"])) == (D0, n, 0, 0)


# ---- 3: order and Date refusals---------------------------------------------------------------------------------------------------------------------
ROWS3 = 1500


def _strict_part(fa, po, n=ROWS3):
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    rows["time_received"] = MID + 100 + 3 * np.arange(n, dtype=np.uint64)  # strictly ascending: a swap of neighbours is ONE descent
    rows["bytes"] = 1 + np.arange(n) % 7
    rows["sampling_rate"] = 1
    return fa.flow_rows_to_native(_as_flow_rows(fa, rows))


def _set_time(part, n, row, value):
    at = column_starts(n)[0][1] + 4 * row
    struct.pack_into("<I", part, at, value)


def _get_time(part, n, row):
    return struct.unpack_from("<I", part, column_starts(n)[0][1] + 4 * row)[0]


@pytest.mark.parametrize("row", [3, 63, 255, 1023, ROWS3 - 2])
@pytest.mark.parametrize("lz4", [False, True], ids=["plain", "lz4"])
def test_a_descending_pair_is_refused(gpu_lib, fa, po, row, lz4):
    good = _strict_part(fa, po)
    bad = bytearray(good)
    x, y = _get_time(bad, ROWS3, row), _get_time(bad, ROWS3, row + 1)
    _set_time(bad, ROWS3, row, y)
    _set_time(bad, ROWS3, row + 1, x)
    data = fa.lz4_frame(bytes(bad)) if lz4 else bytes(bad)
    with _full_ctx(fa) as a:
        a.raw_restore_range(good, 0, NO_UPPER, 0, True)
        before, st0 = _all_reads(a), (a.raw_load_stats()["rows_loaded"], a.raw_range_stats()["calls"])
        for door in (lambda: a.raw_restore_range(data, MID, MID + DAY, 0, True), lambda: a.raw_range_probe(data, 0, NO_UPPER)):
            with pytest.raises(fa.FlowAggError, match=r"descends behind row %d\b" % row) as e:
                door()
            assert e.value.code == ERR_FRAMING
        _same(_all_reads(a), before, nonempty=True)
        assert (a.raw_load_stats()["rows_loaded"], a.raw_range_stats()["calls"]) == st0
        a.raw_restore(data, 0, True)  # the whole-file door never needed the order: its contract did not move
        assert a.raw_load_stats()["rows_loaded"] == 2 * ROWS3


def test_a_row_of_the_next_date_is_refused(gpu_lib, fa, po):
    good = _strict_part(fa, po)
    bad = bytearray(good)
    _set_time(bad, ROWS3, ROWS3 - 1, MID + DAY + 7)  # still ascending
    data = bytes(bad)
    with _full_ctx(fa) as a:
        for door in (lambda: a.raw_restore_range(data, 0, NO_UPPER, 0, True), lambda: a.raw_range_probe(data, MID, MID + 50)):
            with pytest.raises(fa.FlowAggError, match=r"row %d does not lie in the part's Date %d\b" % (ROWS3 - 1, D0)) as e:
                door()
            assert e.value.code == ERR_FRAMING
        assert not any(len(v) for k, v in _all_reads(a).items() if k[0] != "cms") and a.raw_load_stats()["rows_loaded"] == 0
        a.raw_restore(data, 0, True)
        assert a.raw_load_stats()["rows_loaded"] == ROWS3


# ---- 4: pruning -------------------------------------------------------------------------------------------------------------------------------------
N4 = 1 << 18


def _gen(po, seed, n, t0, span):
    gp = po.gen_params(mode=po.GEN_ASPAIRS, framed=1, seed=seed, n_total=n, t0=t0, span_secs=span)
    buf, off = po.gen_records(gp, 0, n)
    rows, status = po.decode_batch(buf, off, 1)
    assert int(status.sum()) == 0
    return buf, off, t32_of(rows)


def _merged_lz4(fa, streams):
    with fa.FlowAgg(framed=True) as a:
        a.raw_enable(1 << 17)
        for buf, off, _ in streams:
            a.ingest(buf, off)
        a.raw_merge()
        data, parts = a.raw_take_lz4()
        return bytes(data), parts


@pytest.fixture(scope="module")
def big(gpu_lib, fa, po):
    """one merged LZ4 part of 2^18 rows over one Date and a small part of the next Date; a second file of the same shape"""
    one = _gen(po, 41, N4, MID + 1000, 40000)
    small = _gen(po, 42, 500, MID + DAY + 50, 100)
    other = _gen(po, 43, N4, MID + 1000, 40000)  # (another file of the same size: what an earlier call leaves in the slots)
    data, parts = _merged_lz4(fa, [one, small])
    data2, parts2 = _merged_lz4(fa, [other, small])
    assert [int(p["rows"]) for p in parts] == [int(p["rows"]) for p in parts2] == [N4, 500] and [int(p["date"]) for p in parts] == [D0, D0 + 1]
    return dict(one=one, small=small, other=other, data=data, parts=parts, data2=data2)


def _frames(data):
    """an LZ4 stream of the library's form -> per frame the list of (offset of the block's size word, size, stored)"""
    out, p = [], 0
    while p < len(data):
        assert data[p:p + 4] == b"\x04\x22\x4d\x18"
        p += 7
        blocks = []
        while True:
            word, = struct.unpack_from("<I", data, p)
            if word == 0:
                p += 4
                break
            blocks.append((p, word & 0x7FFFFFFF, bool(word >> 31)))
            p += 4 + (word & 0x7FFFFFFF)
        out.append(blocks)
    return out


def _blocks_of(spans):
    return {b for lo, hi in spans if hi > lo for b in range(lo // SLOT, (hi - 1) // SLOT + 1)}


def _needed_blocks(n, r_lo, r_hi):
    """the union of the three stage sets of a part of n rows, from the layout documented in flowagg.h (column_starts: this suite's own
    statement of it): first and last block; the part's and the 16 columns' headers and the TimeReceived values; rows [r_lo, r_hi) of
    the 14 columns behind TimeReceived"""
    starts, size = column_starts(n)
    spans = [(0, 1 + len(varuint(n))), (size - 1, size)]
    for (name, ctype, dt, _), s in zip(FORMAT, starts):
        spans.append((s - (2 + len(name) + len(ctype)), s))
    spans.append((starts[1], starts[1] + 4 * n))
    for (name, ctype, dt, _), s in list(zip(FORMAT, starts))[2:]:
        spans.append((s + r_lo * WIDTH[dt], s + r_hi * WIDTH[dt]))
    return _blocks_of(spans)


LO4, HI4 = MID + 1000 + 20000, MID + 1000 + 20300


def test_only_the_needed_blocks_are_decoded(gpu_lib, fa, big):
    buf, off, t = big["one"]
    keep = _in_range(t, LO4, HI4)
    n_sel = int(keep.sum())
    assert 0 < n_sel < N4 // 100
    ts = np.sort(t)
    r_lo, r_hi = int(np.searchsorted(ts, LO4)), int(np.searchsorted(ts, HI4))
    frames = _frames(big["data"])
    assert len(frames) == 2 and len(frames[0]) == -(-column_starts(N4)[1] // SLOT) > 430 and len(frames[1]) == 1
    need = len(_needed_blocks(N4, r_lo, r_hi)) + 1  # + the small part's only block: probed, then skipped by Date
    sel = _subset(buf, off, keep)
    with _full_ctx(fa) as twin:
        twin.ingest(*sel)
        want1 = _all_reads(twin)
        twin.ingest(*sel)
        want2 = _all_reads(twin)
    with _full_ctx(fa) as a:
        a.raw_restore_range(big["data"], LO4, HI4, 0, True)
        st = a.raw_range_stats()
        assert st["blocks_seen"] == len(frames[0]) + 1 and st["blocks_decoded"] == need and st["blocks_decoded"] < st["blocks_seen"] // 4
        assert st["parts_seen"] == 2 and st["parts_skipped_date"] == 1 and st["parts_empty"] == 0
        assert st["rows_seen"] == N4 + 500 and st["rows_loaded"] == n_sel == r_hi - r_lo
        ls = a.raw_load_stats()
        assert ls["blocks"] == need and ls["parts"] == 1 and ls["rows_loaded"] == n_sel and ls["bytes_decoded"] <= need * SLOT
        _same(_all_reads(a), want1, nonempty=True)
        (g0, g1) = a.raw_range_probe(big["data"], LO4, HI4)
        assert (int(g0["r_lo"]), int(g0["r_hi"]), int(g0["t_min"]), int(g0["t_max"])) == (r_lo, r_hi, int(ts[r_lo]), int(ts[r_hi - 1]))
        assert (int(g1["date"]), int(g1["rows"]), int(g1["r_lo"]), int(g1["r_hi"])) == (D0 + 1, 500, 0, 0)
        # every slot now gets other bytes: the second call must not read a slot it has not decoded itself
        cols, n2 = a.raw_columns(big["data2"])  # (decoded and unpacked, not folded)
        assert n2 == N4 + 500
        a.raw_restore_range(big["data"], LO4, HI4, 0, True)
        _same(_all_reads(a), want2, nonempty=True)
        assert a.raw_range_stats()["blocks_decoded"] == 2 * need + len(_needed_blocks(N4, 0, 0)) + 1  # (the probe: stages A and B)


# ---- 5: refusals and counters -----------------------------------------------------------------------------------------------------------------------
def _break_block(data, block):
    """a compressed block whose first sequence has offset 0: refused by the decoder, invisible to the host's frame walk"""
    at, size, stored = block
    assert not stored and size >= 3
    out = bytearray(data)
    out[at + 4:at + 7] = b"\x0f\x00\x00"  # token: no literals, match length 19; offset 0
    return bytes(out)


def test_refusals_and_counters(gpu_lib, fa, big, stream):
    L = fa.lib()
    data = big["data"]
    arr = np.frombuffer(data, dtype=np.uint8)
    with _ctx(fa, key_sets=1 | SRC) as a:
        for call in (lambda: a.raw_restore_range(data, 5, 4), lambda: a.raw_range_probe(data, MID + 1, MID)):
            with pytest.raises(fa.FlowAggError, match="t_lo > t_hi") as e:
                call()
            assert e.value.code == ERR_ARG
        with pytest.raises(fa.FlowAggError, match="not created with") as e:
            a.raw_restore_range(data, 0, NO_UPPER, DST)
        assert e.value.code == ERR_ARG
        need = C.c_size_t(99)
        out = np.zeros(2, dtype=fa.RAW_RANGE_DTYPE)
        assert L.fa_raw_range_probe(a._h, None, 5, 0, 1, out.ctypes.data, 2, C.byref(need)) == ERR_ARG
        assert L.fa_raw_range_probe(a._h, arr.ctypes.data, arr.size, 0, 1, out.ctypes.data, 2, None) == ERR_ARG
        assert L.fa_raw_range_probe(a._h, arr.ctypes.data, arr.size, 0, 1, None, 2, C.byref(need)) == ERR_ARG
        assert L.fa_raw_restore_range(a._h, None, 5, 0, 1, 0, 0) == ERR_ARG
        assert L.fa_raw_range_stats(a._h, None) == ERR_ARG
        assert L.fa_raw_range_probe(a._h, arr.ctypes.data, arr.size, 0, 1, out.ctypes.data, 1, C.byref(need)) == ERR_CAPACITY and need.value == 2
        assert a.raw_range_stats() == dict.fromkeys(a.raw_range_stats(), 0) and a.raw_load_stats()["calls"] == 0
        assert len(a.raw_range_probe(b"", 0, NO_UPPER)) == 0
        a.raw_restore_range(b"", 0, NO_UPPER)
        a.raw_restore_range(data, MID + 5, MID + 5)  # the empty range: probed, nothing loaded
        st = a.raw_range_stats()
        assert st["calls"] == 3 and st["parts_seen"] == 2 and st["parts_skipped_date"] == 2 and st["rows_loaded"] == 0 and len(a.read_window()) == 0
    # a frame without blocks (header + EndMark) behind valid parts: no part, refused by the host's walk before anything is launched
    empty_frame = stream["lz4_merged"][:7] + b"\0\0\0\0"
    with _ctx(fa, key_sets=1 | SRC) as a:
        for tail in (stream["lz4_merged"] + empty_frame, empty_frame + stream["lz4_merged"], empty_frame):
            for call in (lambda: a.raw_restore_range(tail, 0, NO_UPPER), lambda: a.raw_range_probe(tail, 0, NO_UPPER), lambda: a.raw_range_probe(tail, 0, NO_UPPER, cap=8)):
                with pytest.raises(fa.FlowAggError, match=r"frame \d: 0 bytes fit no row count") as e:
                    call()
                assert e.value.code == ERR_FRAMING
        assert a.raw_range_stats() == dict.fromkeys(a.raw_range_stats(), 0) and a.raw_load_stats() == dict.fromkeys(a.raw_load_stats(), 0)
        assert len(a.read_window()) == 0
    frames = _frames(data)
    t = np.sort(big["one"][2])
    r_lo, r_hi = int(np.searchsorted(t, LO4)), int(np.searchsorted(t, HI4))
    needed = _needed_blocks(N4, r_lo, r_hi)
    time_block = (column_starts(N4)[0][1] + 4 * (N4 // 2)) // SLOT  # in the TimeReceived column: stage B
    date_block = 3                                                    # in the Date column: no stage needs it
    load_block = max(needed - _needed_blocks(N4, 0, 0))               # a block of the slice of a late column: stage C alone
    assert time_block in needed and date_block not in needed
    with _full_ctx(fa) as a:
        for blk in (time_block, load_block):
            with pytest.raises(fa.FlowAggError, match="LZ4 block: offset 0") as e:
                a.raw_restore_range(_break_block(data, frames[0][blk]), LO4, HI4, 0, True)
            assert e.value.code == ERR_FRAMING
            assert not any(len(v) for k, v in _all_reads(a).items() if k[0] != "cms") and a.raw_load_stats()["rows_loaded"] == 0
        with pytest.raises(fa.FlowAggError) as e:
            a.raw_restore(_break_block(data, frames[0][date_block]), 0, True)  # (the whole-file door sees it)
        assert e.value.code == ERR_FRAMING
        a.raw_restore_range(_break_block(data, frames[0][date_block]), LO4, HI4, 0, True)  # documented: a block outside the needed set is not seen
        with _full_ctx(fa) as twin:
            twin.ingest(*_subset(big["one"][0], big["one"][1], _in_range(big["one"][2], LO4, HI4)))
            _same(_all_reads(a), _all_reads(twin), nonempty=True)
    # the counters add up over calls of every kind: parts_seen = skipped + empty + loaded
    with _full_ctx(fa) as a:
        a.raw_restore_range(stream["lz4"], MID - 40, MID + 25, 0, True)    # six parts, all with rows in range
        a.raw_restore_range(stream["plain"], MID + 10, MID + 20, 0, True)  # three skipped by Date
        a.raw_restore_range(stream["lz4_merged"], MID - DAY, MID - DAY + 5, 0, True)  # one skipped, one selected but empty
        st, ls = a.raw_range_stats(), a.raw_load_stats()
        assert st["calls"] == ls["calls"] == 3 and st["parts_seen"] == 14 and st["parts_skipped_date"] == 4 and st["parts_empty"] == 1 and ls["parts"] == 9
        assert st["parts_seen"] == st["parts_skipped_date"] + st["parts_empty"] + ls["parts"]
        assert st["rows_loaded"] == ls["rows_loaded"] == int((_in_range(stream["t"], MID - 40, MID + 25) & stream["good"]).sum()) + int((_in_range(stream["t"], MID + 10, MID + 20) & stream["good"]).sum())
        assert st["blocks_decoded"] == ls["blocks"] <= st["blocks_seen"] and st["launches"] == ls["launches"] and st["range_ns"] > 0
