"""Grouped queries over flows_raw parts (include/flowagg.h "grouped queries over flows_raw parts") on the GPU, through the C-ABI,
row for row and byte for byte against the tests' own numpy restatement (tests/raw_query_cases.py over raw_select_cases.match):
a seeded differential over every kind in both orders; the dashboards' grouping rule; wrapping sums, zero weights and the numeric
order of scalars; one key at the wave and workgroup edges; growth of the tables; slices over three Dates; KEEP; that nothing else
of the ctx moves; the protocol."""
import ctypes as C

import numpy as np
import pytest

import raw_query_cases as Q
import raw_select_cases as S
from raw_query_cases import G, G_ALL, O_KEY, O_WEIGHT
from raw_select_cases import MID, NO_UPPER
from test_raw_parts_gpu import D0, DAY, _midnight, encode_part, t32_of
from test_sketch_fold_gpu import _all_reads, _full_ctx

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_FRAMING = -1, -6, -7
PANELS = G["SRC_ADDR"] | G["DST_ADDR"] | G["SRC_PORT"] | G["DST_PORT"] | G["MINUTE"]


def _forms(fa, blobs):
    """the parts' bytes -> {form: the input}"""
    return {"plain": b"".join(blobs), "lz4": b"".join(fa.lz4_frame(b) for b in blobs)}


def _result(a, groups):
    """every kind's rows in key order, as bytes"""
    return {bit: a.raw_query_rows(bit, 0, O_KEY).tobytes() for bit in G.values() if groups & bit}


# ---- 1: seeded differential -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(32))
def test_seeded_differential(gpu_lib, fa, seed):
    parts, f = Q.query_case(seed)
    want = Q.matching(parts, f)
    with fa.FlowAgg(framed=True) as a:
        for form, data in _forms(fa, [encode_part(r) for r in parts]).items():
            a.raw_query(data, G_ALL, **f)
            Q.check_reads(a, want, G_ALL)
            st = a.raw_query_stats()
            assert st["groups"] == sum(len(Q.groups_of(want, bit)) for bit in G.values()), form
        assert st["calls"] == 2 and st["rows_matched"] == 2 * len(want) and st["updates"] == 2 * 9 * len(want)


# ---- 2: the grouping rule ---------------------------------------------------------------------------------------------------------------
def test_the_grouping_rule(gpu_lib, fa):
    rng = np.random.default_rng(21)
    r = S.make_rows(rng, 600)
    x = np.arange(1, 17, dtype=np.uint8) * 7  # 16 bytes, none of them zero
    y = x.copy()
    y[4:] ^= 0x5A  # differs from x in bytes 4..15 only
    r["src_addr"][:], r["dst_addr"][:] = x, x
    et = np.array([0x800, 0x86DD, 0, 0x1234, 0x800], dtype=np.uint32)[np.arange(600) % 5]
    r["etype"] = et
    r["src_addr"][np.arange(600) % 5 == 4] = y  # 0x800 rows that differ in bytes 4..15 only
    with fa.FlowAgg(framed=True) as a:
        a.raw_query(encode_part(r), G["SRC_ADDR"] | G["DST_ADDR"])
        Q.check_reads(a, r, G["SRC_ADDR"] | G["DST_ADDR"])
        for bit in (G["SRC_ADDR"], G["DST_ADDR"]):
            got = a.raw_query_rows(bit, 0, O_KEY)
            # the same 16 bytes under EType 0x800 and 0x86DD are two groups; 0x800 rows that differ only in bytes 4..15 are one;
            # ETypes 0, 0x1234 and 0x86DD with equal bytes are one
            assert len(got) == 2 and sorted(got["etype"].tolist()) == [0, 0x800] and sorted(got["count"].tolist()) == [240, 360]
            v4, v6 = got[got["etype"] == 0x800][0], got[got["etype"] == 0][0]
            assert int(v4["count"]) == 240 and bytes(v4["key"]) == bytes(x[:4]) + bytes(12) and bytes(v6["key"]) == bytes(x) and (got["value"] == 0).all()
            assert fa.format_addr(v4["key"], int(v4["etype"])) == "7.14.21.28"
            assert fa.format_addr(v6["key"], int(v6["etype"])) == fa.format_addr(x, 0x86DD) != fa.format_addr(x, 0x800)


# ---- 3: arithmetic and order ------------------------------------------------------------------------------------------------------------
def test_arithmetic_and_order(gpu_lib, fa):
    rng = np.random.default_rng(22)
    ports = [255, 256, 65535, 65536, 0xFFFFFFFF]
    r = S.make_rows(rng, 40)
    r["dst_port"] = 99
    r["dst_port"][9:39] = np.array(ports, dtype=np.uint32)[np.arange(30) % 5]
    r["bytes"], r["sampling_rate"] = 1000, 1  # equal weights on the five ports: six rows each
    r["src_port"] = 7
    r["src_port"][:3] = 1, 2, 2
    r["bytes"][0], r["sampling_rate"][0] = (1 << 63) + 5, 3  # a product that wraps
    r["bytes"][1:3], r["sampling_rate"][1:3] = 1 << 63, 1    # a group whose sum wraps to 0
    r["src_as"] = 65000
    r["src_as"][5:9] = 65001
    r["bytes"][5:9] = 0  # a group of weight 0 is still a row
    r["time_flow_start"] = np.array([59, 60, 61, 0xFFFFFFFF], dtype=np.uint64)[np.arange(40) % 4]
    groups = G["DST_PORT"] | G["SRC_PORT"] | G["SRC_AS"] | G["MINUTE"] | G["TOTAL"]
    with fa.FlowAgg(framed=True) as a:
        a.raw_query(fa.lz4_frame(encode_part(r)), groups)
        Q.check_reads(a, r, groups)
        sp = a.raw_query_rows(G["SRC_PORT"], 0, O_KEY)
        assert sp["value"].tolist() == [1, 2, 7] and sp["weight"][:2].tolist() == [(((1 << 63) + 5) * 3) % (1 << 64), 0] and sp["count"][:2].tolist() == [1, 2]
        zero = a.raw_query_rows(G["SRC_AS"], 0, O_WEIGHT)
        assert zero["value"].tolist() == [65000, 65001] and int(zero["weight"][1]) == 0 and int(zero["count"][1]) == 4
        for order in (O_WEIGHT, O_KEY):  # equal weights: the ports in numeric order, not in the order of their little-endian bytes
            dp = a.raw_query_rows(G["DST_PORT"], 0, order)
            eq = dp[dp["value"] != 99]
            assert eq["value"].tolist() == ports and len(set(eq["weight"].tolist())) == 1 and (dp["key"] == 0).all() and (dp["etype"] == 0).all()
        assert a.raw_query_rows(G["MINUTE"], 0, O_KEY)["value"].tolist() == [0, 60, 0xFFFFFFFF - 0xFFFFFFFF % 60]
        tot = a.raw_query_rows(G["TOTAL"])
        assert len(tot) == 1 and int(tot["count"][0]) == 40 and int(tot["value"][0]) == 0


# ---- 4: one key, wave and workgroup edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 5000])
def test_one_key_and_wave_edges(gpu_lib, fa, n):
    r = S.make_rows(np.random.default_rng(23), n, span=n)
    r["time_received"] = MID + 1000 + np.arange(n, dtype=np.uint64)  # one row a second
    for field in ("src_addr", "dst_addr", "src_as", "dst_as", "etype", "src_port", "dst_port"):
        r[field] = r[field][0]
    r["time_flow_start"] = MID + 960  # one minute
    r["proto"] = np.where(np.arange(n) % 2 == 0, 6, 17)  # every second row is filtered out
    data = encode_part(r)
    with fa.FlowAgg(framed=True) as a:
        a.raw_query(data, G_ALL, proto=6)
        want = r[S.match(r, dict(proto=6))]
        assert Q.check_reads(a, want, G_ALL) == 9 and len(want) == (n + 1) // 2
        tot = a.raw_query_rows(G["TOTAL"])
        _, desc = a.raw_select(data, proto=6, count_only=True)
        assert int(tot["count"][0]) == len(want) == int(desc["rows"].sum())
        a.raw_query(data, G_ALL, MID + 1000 + n // 3, NO_UPPER, proto=6)  # a slice whose first row is lane 0 of a wave or not
        Q.check_reads(a, Q.matching([r], dict(t_lo=MID + 1000 + n // 3, proto=6)), G_ALL)


# ---- 5: growth --------------------------------------------------------------------------------------------------------------------------
def test_growth(gpu_lib, fa):
    n = 70000
    rng = np.random.default_rng(24)
    r = S.make_rows(rng, n, span=20000)
    ids = np.arange(n, dtype=np.uint32)
    for field, mul in (("src_addr", 1), ("dst_addr", 3)):
        addr = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        addr[:, :4] = ((ids * np.uint32(mul)) & np.uint32(0xFFFFFFFF)).astype(">u4").view(np.uint8).reshape(-1, 4)  # distinct in bytes 0..3: under both families
        r[field] = addr
    groups = G["SRC_ADDR"] | G["DST_ADDR"] | G["SRC_PORT"]
    with fa.FlowAgg(framed=True) as a:
        a.raw_query(fa.lz4_frame(encode_part(r)), groups)
        total = Q.check_reads(a, r, groups, ks=(3,))
        st = a.raw_query_stats()
        assert total == 2 * n + len(S.PORTS) and st["groups"] == total and st["grows"] >= 1  # more than 2^16 slots hold at half load
        assert st["rows_scanned"] == st["rows_matched"] == n and st["updates"] == 3 * n


# ---- 6: slices --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three_dates(gpu_lib, fa):
    """seven parts over three Dates across two midnights (the fixture of tests/test_raw_select_gpu.py, restated)"""
    rng = np.random.default_rng(25)
    pool = S.address_pool(rng)
    parts = []
    for day, n, t0, span in ((0, 900, DAY - 300, 300), (0, 300, DAY - 100, 100), (1, 1200, 0, 400), (1, 70, 100, 50), (1, 2500, 0, DAY), (2, 64, 0, 10), (2, 1000, 5, 600)):
        parts.append(S.make_rows(rng, n, t0=MID + day * DAY + t0, span=span, pool=pool))
    merged = []
    for day in (0, 1, 2):
        m = np.concatenate([r for r in parts if int(r["time_received"][0]) // DAY == D0 + day])
        merged.append(m[np.argsort(t32_of(m), kind="stable")])
    return dict(parts=parts, merged=merged, data=_forms(fa, [encode_part(r) for r in parts]), merged_data=_forms(fa, [encode_part(r) for r in merged]))


@pytest.mark.parametrize("form", ["plain", "lz4"])
def test_slices_over_three_dates(gpu_lib, fa, three_dates, form):
    parts, data = three_dates["parts"], three_dates["data"][form]
    ranges = [(MID + DAY - 50, MID + DAY + 120), (MID + DAY, MID + 2 * DAY), (MID + DAY - 137, MID + 2 * DAY + 333), (0, NO_UPPER), (MID + 2 * DAY + 3, NO_UPPER)]
    cuts = {int(np.searchsorted(t32_of(r), t)) for r in parts for lo, hi in ranges for t in (lo, hi)}
    assert any(c % 64 for c in cuts) and any(c % 256 for c in cuts)  # slices that start and end off the wave and the workgroup
    with fa.FlowAgg(framed=True) as a:
        for lo, hi in ranges:
            f = dict(t_lo=lo, t_hi=hi, dst_port=(0, 65535))
            a.raw_query(data, G_ALL, **f)
            want = Q.matching(parts, f)
            assert len(want) > 0
            Q.check_reads(a, want, G_ALL)
        for lo, hi in ((MID + 3 * DAY + 5, NO_UPPER), (5, 6), (MID + DAY + 7, MID + DAY + 7), (0, 0)):  # no row; t_lo == t_hi
            a.raw_query(data, G_ALL, lo, hi)
            assert all(len(a.raw_query_rows(bit, 0, order)) == 0 for bit in G.values() for order in (O_WEIGHT, O_KEY))
            assert a.raw_query_stats()["groups"] == 0
        assert a.raw_query_rows_device(G["TOTAL"]) == (0, 0)


def test_merged_and_unmerged_inputs_give_the_same_rows(gpu_lib, fa, three_dates):
    f = dict(t_lo=MID + DAY - 80, t_hi=MID + 2 * DAY + 200, src_port=(53, 65535), etype=0x86DD)
    with fa.FlowAgg(framed=True) as a:
        a.raw_query(three_dates["merged_data"]["lz4"], G_ALL, **f)
        one = _result(a, G_ALL)
        Q.check_reads(a, Q.matching(three_dates["merged"], f), G_ALL)
        a.raw_query(three_dates["data"]["lz4"], G_ALL, **f)
        assert _result(a, G_ALL) == one and len(one[G["SRC_ADDR"]]) > 40


# ---- 7: KEEP ----------------------------------------------------------------------------------------------------------------------------
def test_keep(gpu_lib, fa, three_dates):
    parts = three_dates["parts"]
    first, second = parts[:3], parts[3:]
    d1, d2 = (b"".join(fa.lz4_frame(encode_part(r)) for r in p) for p in (first, second))
    f = dict(proto=6, either=True, src_as=64501)
    unsorted = parts[0].copy()  # the descending pair of tests/test_raw_range_gpu.py
    unsorted["time_received"][[10, 11]] = unsorted["time_received"][[11, 10]] + np.array([1, 0], dtype=np.uint64)
    assert unsorted["time_received"][10] > unsorted["time_received"][11]
    with fa.FlowAgg(framed=True) as a:
        a.raw_query(d1 + d2, PANELS, **f)
        both = _result(a, PANELS)
        Q.check_reads(a, Q.matching(parts, f), PANELS)
        a.raw_query(d1, PANELS, keep=True, **f)  # (KEEP replaces nothing: the result held is added to ... so drop it first)
        assert _result(a, PANELS) != both
        a.raw_query_reset()
        a.raw_query(d1, PANELS, keep=True, **f)  # KEEP on a ctx that holds nothing starts a result
        a.raw_query(d2, PANELS, keep=True, **f)
        assert _result(a, PANELS) == both
        # KEEP with other groups: refused, the result stays
        with pytest.raises(fa.FlowAggError, match="KEEP with groups other than") as e:
            a.raw_query(d2, PANELS | G["TOTAL"], keep=True, **f)
        assert e.value.code == ERR_ARG and _result(a, PANELS) == both
        # a KEEP call whose input is refused folds nothing
        st0 = a.raw_query_stats()
        with pytest.raises(fa.FlowAggError, match=r"frame 1 \(part 1\): TimeReceived descends behind row 10\b") as e:
            a.raw_query(fa.lz4_frame(encode_part(parts[1])) + fa.lz4_frame(encode_part(unsorted)), PANELS, keep=True, **f)
        assert e.value.code == ERR_FRAMING and a.raw_query_stats() == st0 and _result(a, PANELS) == both
        # without KEEP the second replaces the first
        a.raw_query(d2, PANELS, **f)
        Q.check_reads(a, Q.matching(second, f), PANELS)
        assert _result(a, PANELS) != both


# ---- 8: nothing else moves --------------------------------------------------------------------------------------------------------------
def _state(a):
    out = _all_reads(a)
    for ts in a.open_timeslots():
        out["window", int(ts)] = a.read_window(int(ts))
    for d in (0, 1):
        out["talkers all", d] = a.top_talkers(d)
        out["ports range", d] = a.top_ports_range(d, 0, MID - 60, MID + 120)
    return out, a.raw_stats(), a.talkers_stats()["used"]


def test_nothing_else_moves(gpu_lib, fa, three_dates):
    buf, off, rows, status = _midnight(n=6000, bad_every=97)
    data, parts = three_dates["data"]["lz4"], three_dates["parts"]
    f = dict(t_lo=MID + DAY - 200, t_hi=MID + DAY + 300, dst_port=(53, 65536))
    want = Q.matching(parts, f)
    with _full_ctx(fa) as a:
        a.raw_enable(2100)
        a.ingest(buf, off)
        before, raw0, used0 = _state(a)
        assert raw0["pending_parts"] > 0 and sum(used0) > 0 and any(len(v) for v in before.values())
        a.raw_query(data, G_ALL, **f)
        Q.check_reads(a, want, G_ALL)
        after, raw1, used1 = _state(a)
        assert raw1 == raw0 and list(used1) == list(used0) and after.keys() == before.keys()
        assert all(after[k].tobytes() == before[k].tobytes() for k in before)
        held = _result(a, G_ALL)
        # the selection is gone after a query; the query's result survives a following select and a restore
        sel, _ = a.raw_select(data, proto=6)
        assert a.raw_selection_device()[1] == len(sel) > 0
        a.raw_query(data, G_ALL, **f)
        assert a.raw_selection_device() == (0, 0)
        a.raw_select(data, proto=17)
        a.raw_restore_range(data, MID + DAY, MID + DAY + 5, 0, True)
        assert _result(a, G_ALL) == held
        a.raw_load_reset()  # ... and ends here
        with pytest.raises(fa.FlowAggError) as e:
            a.raw_query_rows(G["TOTAL"])
        assert e.value.code == ERR_ARG
    with fa.FlowAgg(framed=True) as b:  # nothing enabled
        b.raw_query(data, G_ALL, **f)
        assert _result(b, G_ALL) == held


# ---- 9: protocol ------------------------------------------------------------------------------------------------------------------------
def _query(fa, groups, flags=0, **f):
    q = fa.RawQuery()
    q.where = fa.raw_filter(**f)
    q.groups, q.flags = groups, flags
    return q


def test_protocol(gpu_lib, fa, three_dates):
    L = fa.lib()
    data, parts = three_dates["data"]["lz4"], three_dates["parts"]
    arr = np.frombuffer(data, dtype=np.uint8)
    n = C.c_size_t(77)
    out = np.zeros(64, dtype=fa.QUERY_ROW_DTYPE)
    with fa.FlowAgg(framed=True) as a:
        assert a.raw_query_stats() == dict.fromkeys(a.raw_query_stats(), 0)
        # rows before any query
        assert L.fa_raw_query_rows(a._h, 1, 0, 0, out.ctypes.data, 64, C.byref(n)) == ERR_ARG and n.value == 0
        assert b"no query result" in bytes(L.fa_last_error(a._h))
        a.raw_query_reset()
        groups = G["DST_PORT"] | G["TOTAL"]
        a.raw_query(data, groups, proto=6)
        held = _result(a, groups)
        want = Q.groups_of(Q.matching(parts, dict(proto=6)), G["DST_PORT"])
        assert len(want) == len(S.PORTS)
        # every refusal of the query's arguments; the result held stays under each
        bad = [("limit", _query(fa, groups, proto=6, limit=5)), ("COUNT_ONLY", _query(fa, groups, proto=6, count_only=True)), ("groups is 0", _query(fa, 0)),
               ("an unknown bit in groups", _query(fa, 512)), ("an unknown bit in groups", _query(fa, groups | 1 << 31)), ("an unknown flag", _query(fa, groups, 2)),
               ("KEEP with groups", _query(fa, G["TOTAL"], 1)), ("t_lo > t_hi", _query(fa, groups, t_lo=5, t_hi=4)), ("an unknown bit in fields", _query(fa, groups))]
        bad[-1][1].where.fields = 2048
        for text, q in bad:
            assert L.fa_raw_query(a._h, arr.ctypes.data, arr.size, C.byref(q)) == ERR_ARG, text
            err = bytes(L.fa_last_error(a._h))
            assert b"fa_raw_query: " in err and text.encode() in err, (text, err)
            assert _result(a, groups) == held
        assert L.fa_raw_query(a._h, arr.ctypes.data, arr.size, None) == ERR_ARG and L.fa_raw_query(a._h, None, 5, C.byref(_query(fa, groups))) == ERR_ARG
        # a kind the query did not name, no bit, two bits, an unknown order
        for group, order in ((G["SRC_PORT"], 0), (0, 0), (groups, 0), (512, 0), (G["TOTAL"], 2), (G["TOTAL"], -1)):
            assert L.fa_raw_query_rows(a._h, group, order, 0, out.ctypes.data, 64, C.byref(n)) == ERR_ARG, (group, order)
            p = C.c_void_p(5)
            assert L.fa_raw_query_rows_device(a._h, group, order, 0, C.byref(p), C.byref(n)) == ERR_ARG and not p.value
        assert L.fa_raw_query_rows(a._h, G["TOTAL"], 0, 0, out.ctypes.data, 64, None) == ERR_ARG and L.fa_raw_query_rows(a._h, G["TOTAL"], 0, 0, None, 4, C.byref(n)) == ERR_ARG
        assert L.fa_raw_query_rows_device(a._h, G["TOTAL"], 0, 0, None, C.byref(n)) == ERR_ARG and L.fa_raw_query_stats(a._h, None) == ERR_ARG
        # FA_ERR_CAPACITY with the count; k cuts what is needed
        assert L.fa_raw_query_rows(a._h, G["DST_PORT"], O_KEY, 0, out.ctypes.data, len(want) - 1, C.byref(n)) == ERR_CAPACITY and n.value == len(want)
        assert L.fa_raw_query_rows(a._h, G["DST_PORT"], O_KEY, 0, None, 0, C.byref(n)) == ERR_CAPACITY and n.value == len(want)
        assert L.fa_raw_query_rows(a._h, G["DST_PORT"], O_KEY, 2, out.ctypes.data, 2, C.byref(n)) == 0 and n.value == 2 and out[:2].tobytes() == want[:2].tobytes()
        assert L.fa_raw_query_rows(a._h, G["DST_PORT"], O_KEY, 100, out.ctypes.data, 64, C.byref(n)) == 0 and n.value == len(want)
        # the rows in HBM equal the rows copied out
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        for order in (O_WEIGHT, O_KEY):
            ptr, rows = a.raw_query_rows_device(G["DST_PORT"], 0, order)
            dev = np.zeros(rows, dtype=fa.QUERY_ROW_DTYPE)
            assert ptr and rows == len(want) and hip.hipMemcpy(dev.ctypes.data, ptr, dev.nbytes, 2) == 0  # hipMemcpyDeviceToHost
            assert dev.tobytes() == a.raw_query_rows(G["DST_PORT"], 0, order).tobytes() == Q.ordered(want, order).tobytes()
        # the counters add up; a query counts as a ranged call that loads nothing, never as a select
        st, ls, rs = a.raw_query_stats(), a.raw_load_stats(), a.raw_range_stats()
        assert st["calls"] == 1 and st["updates"] == st["rows_matched"] * 2 and st["rows_matched"] == len(Q.matching(parts, dict(proto=6))) <= st["rows_scanned"]
        assert st["rows_scanned"] == sum(len(r) for r in parts) and st["groups"] == len(want) + 1 and st["absorbed"] <= st["updates"] and st["launches"] > 0
        assert ls["calls"] == rs["calls"] == 1 and ls["rows_loaded"] == rs["rows_loaded"] == 0 and a.raw_select_stats()["calls"] == 0
        # reset: no result, the counters go on
        a.raw_query_reset()
        assert L.fa_raw_query_rows(a._h, G["TOTAL"], 0, 0, out.ctypes.data, 64, C.byref(n)) == ERR_ARG
        st2 = a.raw_query_stats()
        assert st2["groups"] == 0 and st2["calls"] == 1 and st2["rows_matched"] == st["rows_matched"]
        a.raw_query(b"", groups)  # an empty input: FA_OK, a result without rows
        assert len(a.raw_query_rows(G["TOTAL"])) == 0
        a.raw_query(data, groups, proto=6)
        assert _result(a, groups) == held
