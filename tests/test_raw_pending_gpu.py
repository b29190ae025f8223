"""The pending flows_raw parts of a live ctx as input (include/flowagg.h "the pending flows_raw parts as input") on the GPU, through
the C-ABI.  Every expected value comes from the tests' own numpy restatements (raw_select_cases.match / expected,
raw_query_cases.groups_of / check_reads, numpy.searchsorted, test_raw_pending_cpu.classify) or from the file doors over the bytes
a twin ctx takes - never from the doors under test: a seeded differential; the bounds at the wave, step and row-count edges; the
end of the 32-bit axis; many small parts and the skipped / whole / searched counts; a live ctx whose other reads must not move
and whose image is reallocated; a merged ctx; KEEP across stored and pending rows; the protocol."""
import ctypes as C

import numpy as np
import pytest

import raw_query_cases as Q
import raw_select_cases as S
from raw_query_cases import G, G_ALL, O_KEY
from raw_select_cases import MID, NO_UPPER
from test_raw_parts_gpu import DAY, _midnight, _upload, check_parts, encode_part, expected_parts, t32_of
from test_raw_pending_cpu import classify
from test_sketch_fold_gpu import _all_reads, _full_ctx

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY = -1, -6
PANELS = G["SRC_ADDR"] | G["DST_ADDR"] | G["SRC_PORT"] | G["DST_PORT"] | G["MINUTE"]


def _build(fa, a, rows):
    """rows of status 0 -> pending parts of ctx a (one per Date and chunk), through fa_raw_build_columns_device"""
    cols, keep = _upload(fa, rows, np.zeros(len(rows), dtype=np.uint8))
    a.raw_build_columns(cols, len(rows))
    del keep


def _pending(fa, parts, chunk_records=0):
    """a ctx whose pending parts are `parts` (each the sorted rows of one Date): one build call per part"""
    a = fa.FlowAgg(framed=True)
    a.raw_enable(chunk_records)
    for r in parts:
        _build(fa, a, r)
    return a


def _result(a, groups):
    """every kind's rows in key order, as bytes"""
    return {bit: a.raw_query_rows(bit, 0, O_KEY).tobytes() for bit in G.values() if groups & bit}


def _want_parts(parts):
    return [(int(t32_of(r)[0]) // DAY, r, encode_part(r)) for r in parts]


def _bounds(t, lo, hi):
    """a part's sorted times -> [r_lo, r_hi) by numpy.searchsorted"""
    r_lo = int(np.searchsorted(t, lo, "left"))
    return r_lo, len(t) if hi == NO_UPPER else int(np.searchsorted(t, hi, "left"))


def _check_probe(probe, times, lo, hi):
    """fa_raw_pending_probe's entries against searchsorted over every part's times"""
    assert len(probe) == len(times)
    for p, t in zip(probe, times):
        r_lo, r_hi = _bounds(t, lo, hi)
        assert (int(p["date"]), int(p["rows"])) == (int(t[0]) // DAY, len(t))
        if r_lo < r_hi:
            assert (int(p["r_lo"]), int(p["r_hi"]), int(p["t_min"]), int(p["t_max"])) == (r_lo, r_hi, int(t[r_lo]), int(t[r_hi - 1])), (lo, hi, len(t))
        else:
            assert int(p["r_lo"]) == int(p["r_hi"]), (lo, hi, len(t))


def _total(a):
    tot = a.raw_query_rows(G["TOTAL"])
    return int(tot["count"][0]) if len(tot) else 0


# ---- 1: seeded differential -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(16))
def test_seeded_differential(gpu_lib, fa, seed):
    parts, fl = S.fuzz_case(seed)  # (the select's filter: with the seed's limit)
    f = {k: v for k, v in fl.items() if k != "limit"}
    want = Q.matching(parts, f)
    with _pending(fa, parts) as a, _pending(fa, parts) as twin:
        data, tparts = twin.raw_take()
        data = bytes(data)
        check_parts(data, tparts, _want_parts(parts))
        takes0 = a.raw_stats()
        # the query: against the restatement, and kind for kind, byte for byte against the file door over the twin's bytes
        a.raw_query_pending(G_ALL, **f)
        Q.check_reads(a, want, G_ALL)
        twin.raw_query(data, G_ALL, **f)
        assert _result(a, G_ALL) == _result(twin, G_ALL)
        qs = a.raw_query_stats()
        assert qs["calls"] == 1 and qs["rows_matched"] == len(want) and qs["updates"] == 9 * len(want)
        # the select
        sel, sparts = a.raw_select_pending(**fl)
        check_parts(sel, sparts, S.expected(parts, fl))
        # the probe
        lo, hi = f.get("t_lo", 0), f.get("t_hi", NO_UPPER)
        got, ref = a.raw_pending_probe(lo, hi), twin.raw_range_probe(data, lo, hi)
        assert len(got) == len(ref) == len(parts)
        for p, r in zip(got, ref):
            assert (int(p["date"]), int(p["rows"])) == (int(r["date"]), int(r["rows"]))
            if int(r["r_lo"]) < int(r["r_hi"]):
                assert p.tobytes() == r.tobytes()
            else:
                assert int(p["r_lo"]) == int(p["r_hi"])
        _check_probe(got, [t32_of(r) for r in parts], lo, hi)
        # nothing was loaded, nothing was taken or changed
        assert a.raw_load_stats()["calls"] == 0 and a.raw_range_stats()["calls"] == 0 and a.raw_stats() == takes0
        mine, mparts = a.raw_take()
        assert bytes(mine) == data and mparts.tobytes() == tparts.tobytes()


# ---- 2: bounds edges --------------------------------------------------------------------------------------------------------------------
def _run_times(n, run):
    """n ascending times in runs of `run` equal values, two seconds apart: every odd offset is absent"""
    return (MID + 1000 + 2 * (np.arange(n, dtype=np.uint64) // np.uint64(run))).astype(np.uint64)


@pytest.mark.parametrize("n,run", [(1, 3), (2, 3), (63, 3), (64, 3), (65, 3), (66, 70), (4095, 3), (4096, 70), (4097, 3), (4226, 70), (4226, 3), (262145, 70)])
def test_bounds_edges(gpu_lib, fa, n, run):
    r = S.make_rows(np.random.default_rng(40 + n), n, span=1)
    r["time_received"] = _run_times(n, run)
    t = t32_of(r)
    # below the minimum, on it, inside runs (those that straddle rows 64, 65, 4096, 4225 and the middle), absent values, the maximum, above it
    at = sorted({0, n // 2, n - 1} | {i for i in (62, 63, 64, 65, 66, 4095, 4096, 4097, 4224, 4225, 4226) if i < n})
    edges = {int(t[0]) - 5, int(t[-1]) + 1, int(t[-1]) + 9, NO_UPPER}
    for i in at:
        edges |= {int(t[i]), int(t[i]) + 1}
    edges = sorted(edges)
    if n > 100000:  # (the large part: the same kinds of edges, fewer pairs)
        edges = edges[:3] + edges[len(edges) // 2 - 1:len(edges) // 2 + 1] + edges[-4:]
    with _pending(fa, [r]) as a:
        searched = 0
        for lo in edges:
            for hi in edges:
                if lo > hi:
                    continue
                r_lo, r_hi = _bounds(t, lo, hi)
                if lo == hi:
                    assert r_lo == r_hi
                _check_probe(a.raw_pending_probe(lo, hi), [t], lo, hi)
                a.raw_query_pending(G["TOTAL"], lo, hi)
                assert _total(a) == r_hi - r_lo, (lo, hi)
                searched += classify(t, lo, hi) == "searched"
        st = a.raw_pending_stats()
        assert st["parts_searched"] == 2 * searched and st["bounds_launches"] == 2 * searched and st["parts_seen"] == st["calls"]
        assert searched > 0 or n == 1 or int(t[0]) == int(t[-1])


# ---- 3: the end of the axis -------------------------------------------------------------------------------------------------------------
def test_the_end_of_the_axis(gpu_lib, fa):
    n = 200
    r = S.make_rows(np.random.default_rng(43), n, span=1)
    t = np.full(n, 0xFFFFFFFF, dtype=np.uint64)
    t[:150] = 0xFFFFFFFE
    t[:100] = 0xFFFFFF00 + np.arange(100) // 2
    r["time_received"] = t
    with _pending(fa, [r]) as a:
        for lo, hi, count in ((0, NO_UPPER, 200), (0, 0xFFFFFFFE, 100), (0xFFFFFFFE, NO_UPPER, 100), (NO_UPPER, NO_UPPER, 50), (0xFFFFFFFE, 0xFFFFFFFE, 0), (0xFFFFFF10, 0xFFFFFFFE, 68)):
            assert int(S.in_range(t32_of(r), lo, hi).sum()) == count
            a.raw_query_pending(G["TOTAL"], lo, hi)
            assert _total(a) == count, (lo, hi)
            f = dict(t_lo=lo, t_hi=hi)
            sel, sparts = a.raw_select_pending(**f)
            check_parts(sel, sparts, S.expected([r], f))
            _check_probe(a.raw_pending_probe(lo, hi), [t32_of(r)], lo, hi)


# ---- 4: many small parts ----------------------------------------------------------------------------------------------------------------
def test_many_small_parts(gpu_lib, fa):
    rng = np.random.default_rng(44)
    n, chunk = 3000, 16
    rows = np.concatenate([S.make_rows(rng, n // 3, t0=MID + d * DAY + 1000, span=4000) for d in range(3)])
    rows = rows[rng.permutation(n)]
    zero = np.zeros(chunk, dtype=np.uint8)
    parts = [p[1] for i in range(0, n, chunk) for p in expected_parts(rows[i:i + chunk], zero[:len(rows[i:i + chunk])])]
    times = [t32_of(p) for p in parts]
    with fa.FlowAgg(framed=True) as a:
        a.raw_enable(chunk_records=chunk)
        _build(fa, a, rows)
        assert a.raw_stats()["pending_parts"] == len(parts) > 500
        lo, hi = MID + DAY + 2000, MID + 2 * DAY + 2500  # skips the first Date, cuts parts of the second and the third
        kinds = [classify(t, lo, hi) for t in times]
        counts = {k: kinds.count(k) for k in ("skipped", "whole", "searched")}
        assert min(counts.values()) > 20, counts
        f = dict(t_lo=lo, t_hi=hi, proto=6)
        a.raw_query_pending(G_ALL, **f)
        Q.check_reads(a, Q.matching(parts, f), G_ALL, ks=(3,))
        st = a.raw_pending_stats()
        assert st["calls"] == 1 and st["parts_seen"] == len(parts) == st["parts_skipped"] + st["parts_whole"] + st["parts_searched"]
        assert (st["parts_skipped"], st["parts_whole"], st["parts_searched"]) == (counts["skipped"], counts["whole"], counts["searched"])
        assert st["rows_seen"] == n and st["rows_in_range"] == sum(b - a_ for a_, b in (_bounds(t, lo, hi) for t in times)) and st["bounds_launches"] == 1
        _check_probe(a.raw_pending_probe(lo, hi), times, lo, hi)
        sel, sparts = a.raw_select_pending(limit=700, **f)
        check_parts(sel, sparts, S.expected(parts, dict(f, limit=700)))
        # a range over everything, and one over nothing: no bounds launch
        st = a.raw_pending_stats()
        a.raw_query_pending(G["TOTAL"])
        assert _total(a) == n
        a.raw_query_pending(G["TOTAL"], 5, MID)
        assert _total(a) == 0
        st2 = a.raw_pending_stats()
        assert st2["bounds_launches"] == st["bounds_launches"] == 3 and st2["bounds_ns"] == st["bounds_ns"] and st2["parts_searched"] == st["parts_searched"]
        assert st2["parts_whole"] == st["parts_whole"] + len(parts) and st2["parts_skipped"] == st["parts_skipped"] + len(parts) and st2["calls"] == st["calls"] + 2


# ---- 5: a live ctx ----------------------------------------------------------------------------------------------------------------------
def test_a_live_ctx(gpu_lib, fa):
    buf, off, rows, status = _midnight(n=6000, bad_every=97)
    buf2, off2, rows2, status2 = _midnight()
    good, good2 = rows[status == 0], rows2[status2 == 0]
    f = dict(t_lo=MID - 100, t_hi=MID + 150, dst_port=(0, 65536))
    with _full_ctx(fa) as a:
        a.raw_enable(2100)
        a.ingest(buf, off)
        before, raw0 = _all_reads(a), a.raw_stats()
        assert raw0["pending_parts"] > 0 and any(len(v) for v in before.values())
        a.raw_query_pending(G_ALL, **f)
        Q.check_reads(a, Q.matching([good], f), G_ALL, ks=(3,))
        src_as = int(good["src_as"][len(good) // 2])  # (a value the stream holds)
        sel, sparts = a.raw_select_pending(src_as=src_as, **f)
        assert 0 < sum(int(p["rows"]) for p in sparts) == int(S.match(good, dict(f, src_as=src_as)).sum()) < len(good)
        after = _all_reads(a)
        assert a.raw_stats() == raw0 and after.keys() == before.keys() and all(after[k].tobytes() == before[k].tobytes() for k in before)
        assert a.raw_load_stats()["calls"] == 0 and a.raw_range_stats()["calls"] == 0
        # more rows: the image grows and is reallocated; the selection is a copy and stays, the next query sees every row
        a.ingest(buf2, off2)
        assert a.raw_stats()["pending_bytes"] > (1 << 20) > raw0["pending_bytes"]
        again = np.empty(len(sel), dtype=np.uint8)
        n = C.c_size_t()
        assert fa.lib().fa_raw_selection_fetch(a._h, again.ctypes.data, again.size, C.byref(n)) == 0 and n.value == len(sel) and again.tobytes() == sel
        a.raw_query_pending(G_ALL, **f)
        Q.check_reads(a, Q.matching([good, good2], f), G_ALL, ks=(3,))
        assert fa.lib().fa_raw_selection_fetch(a._h, again.ctypes.data, again.size, C.byref(n)) == 0 and again.tobytes() == sel  # (a pending query drops no selection)


# ---- 6: after a merge -------------------------------------------------------------------------------------------------------------------
def test_after_a_merge(gpu_lib, fa):
    rng = np.random.default_rng(46)
    pool = S.address_pool(rng)
    parts = [S.make_rows(rng, n, t0=MID + d * DAY + 1000, span=900, pool=pool) for d, n in ((0, 700), (0, 300), (1, 65), (0, 1500), (1, 4100))]
    f = dict(t_lo=MID + 1300, t_hi=MID + DAY + 1500, src_port=(53, 65535))
    with _pending(fa, parts) as a:
        a.raw_query_pending(G_ALL, **f)
        one = _result(a, G_ALL)
        Q.check_reads(a, Q.matching(parts, f), G_ALL, ks=(3,))
        sel, sparts = a.raw_select_pending(**f)
        rows_before = np.concatenate([S.rows_of_block(b) for b in fa.spill.read_native(sel)])
        assert len(sparts) == 5
        a.raw_merge()
        assert a.raw_stats()["pending_parts"] == 2
        st0 = a.raw_pending_stats()
        a.raw_query_pending(G_ALL, **f)
        assert _result(a, G_ALL) == one
        st1 = a.raw_pending_stats()
        assert st1["parts_searched"] - st0["parts_searched"] == 2 and st1["bounds_launches"] == st0["bounds_launches"] + 1  # (the range lies inside both merged parts)
        sel2, sparts2 = a.raw_select_pending(**f)
        rows_after = np.concatenate([S.rows_of_block(b) for b in fa.spill.read_native(sel2)])
        assert len(sparts2) == 2 and len(rows_after) == len(rows_before) == len(Q.matching(parts, f))
        key = lambda r: np.argsort(r, order=("time_received", "sequence_num", "bytes", "packets"), kind="stable")  # noqa: E731
        assert rows_after[key(rows_after)].tobytes() == rows_before[key(rows_before)].tobytes()
        merged = [np.concatenate([p for p in parts if int(p["time_received"][0]) // DAY == d]) for d in (MID // DAY, MID // DAY + 1)]
        merged = [m[np.argsort(t32_of(m), kind="stable")] for m in merged]
        check_parts(sel2, sparts2, S.expected(merged, f))


# ---- 7: KEEP across stored and pending rows ---------------------------------------------------------------------------------------------
def test_keep_across_stored_and_pending(gpu_lib, fa):
    rng = np.random.default_rng(47)
    pool = S.address_pool(rng)
    first = S.make_rows(rng, 1200, t0=MID + 1000, span=600, pool=pool)
    second = S.make_rows(rng, 900, t0=MID + 1500, span=600, pool=pool)
    f = dict(t_lo=MID + 1100, t_hi=MID + 1900, etype=0x86DD)
    with fa.FlowAgg(framed=True) as a:
        a.raw_enable()
        _build(fa, a, first)
        stored, _ = a.raw_take()
        stored = bytes(stored)
        _build(fa, a, second)
        a.raw_query(stored, PANELS, **f)
        a.raw_query_pending(PANELS, keep=True, **f)
        Q.check_reads(a, Q.matching([first, second], f), PANELS)
        both = _result(a, PANELS)
        with pytest.raises(fa.FlowAggError, match="fa_raw_query_pending: KEEP with groups") as e:
            a.raw_query_pending(G["TOTAL"], keep=True, **f)
        assert e.value.code == ERR_ARG and _result(a, PANELS) == both
        a.raw_query_pending(PANELS, **f)  # without KEEP the pending rows alone
        Q.check_reads(a, Q.matching([second], f), PANELS)


# ---- 8: protocol ------------------------------------------------------------------------------------------------------------------------
def _query(fa, groups, flags=0, **f):
    q = fa.RawQuery()
    q.where = fa.raw_filter(**f)
    q.groups, q.flags = groups, flags
    return q


def test_protocol(gpu_lib, fa):
    L = fa.lib()
    rng = np.random.default_rng(48)
    parts = [S.make_rows(rng, n, t0=MID + d * DAY + 1000, span=300) for d, n in ((0, 400), (1, 300), (2, 70))]
    n, nb = C.c_size_t(77), C.c_size_t(77)
    rng_out = np.zeros(8, dtype=fa.RAW_RANGE_DTYPE)
    pout = np.zeros(8, dtype=fa.RAW_PART_DTYPE)
    flt = fa.raw_filter(proto=6)
    with fa.FlowAgg(framed=True) as a:  # not enabled: FA_ERR_ARG from all four
        ps = fa.RawPendingStats()
        for rc in (L.fa_raw_pending_probe(a._h, 0, NO_UPPER, rng_out.ctypes.data, 8, C.byref(n)), L.fa_raw_query_pending(a._h, C.byref(_query(fa, G_ALL))),
                   L.fa_raw_select_pending(a._h, C.byref(flt), pout.ctypes.data, 8, C.byref(n), C.byref(nb)), L.fa_raw_pending_stats(a._h, C.byref(ps))):
            assert rc == ERR_ARG and b"fa_raw_enable was not called" in bytes(L.fa_last_error(a._h))
    with fa.FlowAgg(framed=True) as a:
        a.raw_enable()
        assert a.raw_pending_stats() == dict.fromkeys(a.raw_pending_stats(), 0)
        # no pending parts: FA_OK, no rows; a result held is cleared without KEEP
        a.raw_query(encode_part(parts[0]), G["TOTAL"])
        assert _total(a) == 400
        a.raw_query_pending(G["TOTAL"], keep=True)
        assert _total(a) == 400
        a.raw_query_pending(G["TOTAL"] | G["PROTO"])
        assert _total(a) == 0 and len(a.raw_query_rows(G["PROTO"])) == 0
        sel, sparts = a.raw_select_pending()
        assert sel == b"" and len(sparts) == 0 and len(a.raw_pending_probe(0, NO_UPPER)) == 0
        for r in parts:
            _build(fa, a, r)
        load0, range0 = a.raw_load_stats(), a.raw_range_stats()
        a.raw_query_pending(PANELS | G["TOTAL"], proto=6)
        held = _result(a, PANELS | G["TOTAL"])
        Q.check_reads(a, Q.matching(parts, dict(proto=6)), PANELS | G["TOTAL"])
        # what a query refuses; the result held stays under each
        bad = [("limit", _query(fa, PANELS, proto=6, limit=5)), ("COUNT_ONLY", _query(fa, PANELS, count_only=True)), ("groups is 0", _query(fa, 0)),
               ("an unknown bit in groups", _query(fa, 512)), ("an unknown flag", _query(fa, PANELS, 2)), ("KEEP with groups", _query(fa, G["TOTAL"], 1)),
               ("t_lo > t_hi", _query(fa, PANELS, t_lo=5, t_hi=4))]
        for text, q in bad:
            assert L.fa_raw_query_pending(a._h, C.byref(q)) == ERR_ARG, text
            err = bytes(L.fa_last_error(a._h))
            assert b"fa_raw_query_pending: " in err and text.encode() in err, (text, err)
            assert _result(a, PANELS | G["TOTAL"]) == held
        assert L.fa_raw_query_pending(a._h, None) == ERR_ARG and L.fa_raw_pending_stats(a._h, None) == ERR_ARG
        assert L.fa_raw_pending_probe(a._h, 5, 4, rng_out.ctypes.data, 8, C.byref(n)) == ERR_ARG and b"t_lo > t_hi" in bytes(L.fa_last_error(a._h))
        assert L.fa_raw_pending_probe(a._h, 0, NO_UPPER, rng_out.ctypes.data, 2, C.byref(n)) == ERR_CAPACITY and n.value == 3
        assert L.fa_raw_pending_probe(a._h, 0, NO_UPPER, rng_out.ctypes.data, 8, None) == ERR_ARG
        # COUNT_ONLY: the descriptions, no selection
        f = dict(t_lo=MID + 1100, t_hi=MID + DAY + 1200, proto=6)
        sel, sparts = a.raw_select_pending(count_only=True, **f)
        want = S.expected(parts, f)
        assert sel == b"" and a.raw_selection_device() == (0, 0)
        assert [(int(p["date"]), int(p["rows"]), int(p["bytes"])) for p in sparts] == [(d, len(r), len(b)) for d, r, b in want] and len(want) == 2
        # a selection; a pending QUERY leaves it fetchable; parts_cap too small: FA_ERR_CAPACITY with the part count, and the selection is gone
        sel, sparts = a.raw_select_pending(**f)
        check_parts(sel, sparts, want)
        a.raw_query_pending(G["TOTAL"], **f)
        assert _total(a) == sum(len(r) for _, r, _ in want) and a.raw_selection_device()[1] == len(sel)
        assert L.fa_raw_select_pending(a._h, C.byref(flt), pout.ctypes.data, 2, C.byref(n), C.byref(nb)) == ERR_CAPACITY and n.value == 3 and nb.value == 0
        assert a.raw_selection_device() == (0, 0)
        bad_f = fa.raw_filter(src_port=(5, 4))
        a.raw_select_pending(**f)
        assert L.fa_raw_select_pending(a._h, C.byref(bad_f), pout.ctypes.data, 8, C.byref(n), C.byref(nb)) == ERR_ARG and b"fa_raw_select_pending: src_port_lo > src_port_hi" in bytes(L.fa_last_error(a._h))
        assert a.raw_selection_device() == (0, 0)  # (a refused call leaves none)
        assert L.fa_raw_select_pending(a._h, None, pout.ctypes.data, 8, C.byref(n), C.byref(nb)) == ERR_ARG
        # the select's counters move as the file door's do; nothing was loaded
        ss = a.raw_select_stats()
        assert ss["calls"] == 4 and ss["rows_matched"] == 3 * sum(len(r) for _, r, _ in want) and ss["rows_out"] == ss["rows_matched"] and ss["launches"] > 0
        assert a.raw_load_stats() == load0 and a.raw_range_stats() == range0
        # after a take: no pending parts again
        taken, tparts = a.raw_take()
        check_parts(bytes(taken), tparts, _want_parts(parts))
        a.raw_query_pending(G["TOTAL"])
        assert _total(a) == 0 and a.raw_select_pending()[0] == b"" and len(a.raw_pending_probe(0, NO_UPPER)) == 0
        st = a.raw_pending_stats()
        assert st["parts_seen"] == st["parts_skipped"] + st["parts_whole"] + st["parts_searched"] and st["bounds_launches"] <= st["calls"]
        a.raw_reset()
        assert a.raw_pending_stats()["calls"] == st["calls"]  # (the buffers go, the counters go on)
