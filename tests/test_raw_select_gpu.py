"""Selecting rows of flows_raw parts (include/flowagg.h "selecting rows of flows_raw parts") on the GPU, through the C-ABI and byte
for byte: the selection equals the rows the tests' own numpy restatement of the filter picks (tests/raw_select_cases.py), encoded by
encode_part of tests/test_raw_parts_gpu.py - never by the code under test.  Sizes at every start residue of the columns, plain and
LZ4, alone and back to back; hand-made patterns at the wave and workgroup seams; every condition; parts over three Dates, more than
512 parts; the limit; the round trip through fa_raw_load; no decode beyond the ranged load's; the protocol; a seeded differential."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import raw_load_cases as R
import raw_select_cases as S
from raw_select_cases import MID, NO_UPPER
from test_raw_parts_gpu import D0, DAY, SWEEP, SWEEP_EXTRA, check_parts, column_starts, encode_part, t32_of

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_FRAMING = -1, -6, -7
WG = 256  # rows per workgroup of the select kernels


def _forms(fa, blobs):
    """the parts' bytes -> {form: the input}"""
    return {"plain": b"".join(blobs), "lz4": b"".join(fa.lz4_frame(b) for b in blobs)}


def _check(a, data, parts, f):
    """one select of `data` (whose parts' rows are `parts`) against the restatement"""
    want = S.expected(parts, f)
    got, desc = a.raw_select(data, **f)
    check_parts(got, desc, want)
    return want


# ---- 1: sizes ---------------------------------------------------------------------------------------------------------------------------
SIZES = tuple(sorted(set(range(1, 41)) | set(SWEEP) | set(SWEEP_EXTRA) | {63, 64, 65, 255, 256, 257, 1023, 1025, 16383, 16384, 65537, 200000}))
ALONE = (1, 2, 63, 64, 65, 257, 1025, 65537)


@pytest.fixture(scope="module")
def sized(gpu_lib, fa):
    """one part per row count, all of one Date: 1000 seconds each, so that a time range cuts every larger part off a multiple of 64"""
    rng = np.random.default_rng(11)
    pool = S.address_pool(rng)
    parts = [S.make_rows(rng, n, pool=pool) for n in SIZES]
    blobs = [encode_part(r) for r in parts]
    assert all(len(b) == column_starts(len(r))[1] for b, r in zip(blobs, parts))
    # every column of a part below 2^21 rows starts at every residue mod 16 over these sizes (the sweep of test_raw_parts_gpu.py)
    starts = {(c, column_starts(n)[0][c] % 16) for n in SIZES for c in range(1, 16)}
    assert all(len({r for c, r in starts if c == col}) >= 8 for col in range(1, 16))
    return dict(parts=parts, blobs=blobs, pool=pool, forms=_forms(fa, blobs))


@pytest.mark.parametrize("form", ["plain", "lz4"])
def test_sizes_back_to_back(gpu_lib, fa, sized, form):
    parts, data = sized["parts"], sized["forms"][form]
    big = parts[-1]
    cut = int(np.searchsorted(t32_of(big), MID + 1137))
    assert cut % 64 and int(np.searchsorted(t32_of(big), MID + 1873)) % 64  # the large slices start and end off a multiple of 64
    with fa.FlowAgg(framed=True) as a:
        for f in (dict(t_lo=MID + 1137, t_hi=MID + 1873, dst_port=(53, 443)), dict(proto=17, either=True, src_as=64501),
                  dict(t_lo=MID + 1500, t_hi=NO_UPPER, src_net=(bytes(sized["pool"][3]), 33), either=True)):
            want = _check(a, data, parts, f)
            assert len(want) > len(SIZES) // 2 and 0 < sum(len(r) for _, r, _ in want) < sum(len(r) for r in parts)
        st = a.raw_select_stats()
        assert st["calls"] == 3 and st["parts_out"] > len(SIZES) and st["rows_out"] == st["rows_matched"] < st["rows_scanned"]


def test_sizes_alone(gpu_lib, fa, sized):
    with fa.FlowAgg(framed=True) as a:
        for n in ALONE:
            i = SIZES.index(n)
            for data in (sized["blobs"][i], fa.lz4_frame(sized["blobs"][i])):
                _check(a, data, [sized["parts"][i]], dict(t_lo=MID + 1100, t_hi=MID + 1900, etype=0x86DD))
                _check(a, data, [sized["parts"][i]], dict(dst_port=(0, 65535)))


# ---- 2: patterns at the seams --------------------------------------------------------------------------------------------------------------
def _pattern_part(n, on):
    r = S.make_rows(np.random.default_rng(12), n, span=n)
    r["time_received"] = MID + 1000 + np.arange(n, dtype=np.uint64)  # one row a second: a time range is a row range
    r["proto"] = np.where(on, 6, 17)
    return r


def test_patterns(gpu_lib, fa):
    n = 6 * WG + 77
    rows = np.arange(n)
    patterns = {"every other row": rows % 2 == 0, "64 on, 64 off": (rows // 64) % 2 == 0, "64 off, 64 on": (rows // 64) % 2 == 1, "runs of 256": (rows // WG) % 2 == 1}
    with fa.FlowAgg(framed=True) as a:
        for r_lo in (0, 37):  # the slice's first row: lane 0 of a wave, or not
            singles = {"the first row": r_lo, "the last row": n - 1, "lane 63 of a wave": r_lo + 63, "the last row of a workgroup": r_lo + WG - 1,
                       "the first row of the next workgroup": r_lo + WG, "lane 63 of the last full wave": r_lo + (n - r_lo) // 64 * 64 - 1}
            cases = dict(patterns, **{k: rows == v for k, v in singles.items()})
            for name, on in cases.items():
                r = _pattern_part(n, on)
                f = dict(t_lo=MID + 1000 + r_lo, t_hi=NO_UPPER, proto=6)
                want = _check(a, encode_part(r), [r], f)
                assert sum(len(x) for _, x, _ in want) == int(on[r_lo:].sum()) > 0, name


# ---- 3: extremes --------------------------------------------------------------------------------------------------------------------------
def test_no_row_and_every_row(gpu_lib, fa, sized):
    i = SIZES.index(1025)
    r, blob = sized["parts"][i], sized["blobs"][i]
    with fa.FlowAgg(framed=True) as a:
        for data in (blob, fa.lz4_frame(blob)):
            got, desc = a.raw_select(data, proto=99)
            assert got == b"" and len(desc) == 0 and a.raw_selection_device() == (0, 0)
            got, desc = a.raw_select(data)  # the whole time axis, no condition: the input part itself
            assert got == blob and len(desc) == 1 and int(desc[0]["rows"]) == 1025
            lo, hi = MID + 1200, MID + 1800
            got, desc = a.raw_select(data, lo, hi)  # every row of a slice: the slice's re-encoding
            sl = r[S.in_range(t32_of(r), lo, hi)]
            assert 0 < len(sl) < 1025 and got == encode_part(sl)
        st = a.raw_select_stats()
        assert st["calls"] == 6 and st["rows_scanned"] == 2 * (1025 + 1025 + len(sl)) and st["rows_matched"] == 2 * (1025 + len(sl))


# ---- 4: conditions ------------------------------------------------------------------------------------------------------------------------
LENS = (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128)


def _flip(addr, bit):
    out = bytearray(addr)
    out[bit // 8] ^= 0x80 >> (bit % 8)
    return bytes(out)


def test_each_condition_and_all_together(gpu_lib, fa, sized):
    i = SIZES.index(16383)
    r, blob, pool = sized["parts"][i], sized["blobs"][i], sized["pool"]
    tfs = np.sort(r["time_flow_start"])
    conds = dict(flow_start=(int(tfs[3000]), int(tfs[9000])), src_as=64500, dst_as=64503, etype=0x800, proto=1, src_port=(53, 65535), dst_port=(65536, NO_UPPER),
                 src_net=(bytes(pool[1]), 24), dst_net=(bytes(pool[2]), 9))
    with fa.FlowAgg(framed=True) as a:
        for k, v in conds.items():
            for either in (False, True):
                want = _check(a, blob, [r], {k: v, "either": either})
                assert 0 < len(want[0][1]) < len(r), k
        allf = dict(conds, flow_start=(0, NO_UPPER), src_net=(bytes(pool[1]), 1), dst_net=(bytes(pool[2]), 1), src_port=(0, NO_UPPER), dst_port=(0, 65536))
        for either in (False, True):
            want = _check(a, blob, [r], dict(allf, either=either, t_lo=MID + 1001, t_hi=MID + 1999))
            assert want and len(want[0][1]) > 0


def test_prefix_lengths_with_neighbours(gpu_lib, fa):
    """a part whose addresses are one address and its neighbours that differ in ONE bit: for every length the rows that differ in
    the last bit inside are out, the rows that differ in the first bit outside are in; bits behind the prefix in the filter are ignored"""
    rng = np.random.default_rng(13)
    base = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    bits = sorted({b for n in LENS for b in (n - 1, n) if 0 <= b < 128})
    pool = np.stack([np.frombuffer(x, dtype=np.uint8) for x in [base] + [_flip(base, b) for b in bits]])
    r = S.make_rows(rng, 3000, pool=pool)
    blob = encode_part(r)
    with fa.FlowAgg(framed=True) as a:
        for n in LENS:
            noisy = bytearray(base)
            for b in range(n, 128):
                if rng.integers(0, 2):
                    noisy[b // 8] ^= 0x80 >> (b % 8)
            for f in (dict(src_net=(bytes(noisy), n)), dict(dst_net=(bytes(noisy), n)), dict(src_net=(bytes(noisy), n), dst_net=(base, 128 - n), either=True)):
                want = _check(a, blob, [r], f)
                if "either" not in f:
                    side = "src_addr" if "src_net" in f else "dst_addr"
                    sel = want[0][1] if want else r[:0]
                    inside = np.array([bytes(x) == _flip(base, n - 1) for x in r[side]]) if n else np.zeros(len(r), dtype=bool)
                    outside = np.array([bytes(x) == _flip(base, n) for x in r[side]]) if n < 128 else np.zeros(len(r), dtype=bool)
                    assert not set(r["sequence_num"][inside]) & set(sel["sequence_num"]) and set(r["sequence_num"][outside]) <= set(sel["sequence_num"])
                    assert n == 0 or inside.sum() > 0


def test_either_with_only_the_swapped_direction(gpu_lib, fa):
    rng = np.random.default_rng(14)
    pool = S.address_pool(rng)
    r = S.make_rows(rng, 2000, pool=pool)
    A, B = bytes(pool[0]), bytes(pool[5])
    r["src_addr"][:] = pool[7]
    r["dst_addr"][:] = pool[8]
    back = np.arange(2000) % 7 == 3  # only these rows run from B to A
    r["src_addr"][back], r["dst_addr"][back] = pool[5], pool[0]
    r["src_port"][back], r["dst_port"][back] = 443, 53
    f = dict(src_net=(A, 128), dst_net=(B, 128), src_port=(53, 53), dst_port=(443, 443))
    blob = encode_part(r)
    with fa.FlowAgg(framed=True) as a:
        assert a.raw_select(blob, **f)[0] == b""
        want = _check(a, blob, [r], dict(f, either=True))
        assert len(want[0][1]) == int(back.sum())
        want = _check(a, blob, [r], dict(src_net=(A, 128), either=True))  # "this host on either side"
        assert len(want[0][1]) == int(back.sum())


def test_flow_start_against_time_received(gpu_lib, fa):
    rng = np.random.default_rng(15)
    r = S.make_rows(rng, 5000, against=True)
    assert (np.diff(r["time_flow_start"].astype(np.int64)) <= 0).all() and r["time_flow_start"][0] > r["time_flow_start"][-1]
    tfs = np.sort(r["time_flow_start"])
    blob = fa.lz4_frame(encode_part(r))
    with fa.FlowAgg(framed=True) as a:
        for fs in ((int(tfs[100]), int(tfs[4000])), (int(tfs[4000]), NO_UPPER), (0, int(tfs[100])), (int(tfs[7]), int(tfs[7]))):
            _check(a, blob, [r], dict(flow_start=fs))
            _check(a, blob, [r], dict(flow_start=fs, t_lo=MID + 1300, t_hi=MID + 1700))


def test_time_bounds_and_the_ends_of_the_axis(gpu_lib, fa):
    rng = np.random.default_rng(16)
    first = S.make_rows(rng, 700, t0=0, span=3)           # Date 0: the first seconds of the axis
    last = S.make_rows(rng, 900, t0=0xFFFFFFFF - 2, span=3)  # Date 49710: the last seconds
    mid = S.make_rows(rng, 800)
    assert int(t32_of(first)[0]) == 0 and int(t32_of(last)[-1]) == 0xFFFFFFFF
    last["time_flow_start"] = last["time_received"]
    parts = [first, mid, last]
    data = b"".join(encode_part(r) for r in parts)
    with fa.FlowAgg(framed=True) as a:
        for lo, hi in ((0, 1), (0, 0), (0, NO_UPPER), (0xFFFFFFFF, NO_UPPER), (0xFFFFFFFE, NO_UPPER), (0xFFFFFFFE, 0xFFFFFFFE), (1, 0xFFFFFFFE), (MID + 1500, MID + 1500),
                       (MID + 1500, NO_UPPER), (0, MID + 1500)):
            _check(a, data, parts, dict(t_lo=lo, t_hi=hi))
            _check(a, data, parts, dict(t_lo=lo, t_hi=hi, proto=6, flow_start=(0xFFFFFFFE, NO_UPPER), either=True))
        want = _check(a, data, parts, dict(t_lo=0, t_hi=1))
        assert len(want) == 1 and want[0][0] == 0
        want = _check(a, data, parts, dict(t_lo=0xFFFFFFFF, t_hi=NO_UPPER))
        assert len(want) == 1 and want[0][0] == 49710 and (t32_of(want[0][1]) == 0xFFFFFFFF).all()


# ---- 5: parts -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three_dates(gpu_lib, fa):
    """seven parts over three Dates across two midnights; the second part of the middle Date has no row of proto 1"""
    rng = np.random.default_rng(17)
    pool = S.address_pool(rng)
    parts = []
    for day, n, t0, span in ((0, 900, DAY - 300, 300), (0, 300, DAY - 100, 100), (1, 1200, 0, 400), (1, 70, 100, 50), (1, 2500, 0, DAY), (2, 64, 0, 10), (2, 1000, 5, 600)):
        parts.append(S.make_rows(rng, n, t0=MID + day * DAY + t0, span=span, pool=pool))
    parts[3]["proto"] = 6
    base = 0
    for r in parts:  # SequenceNum names a row over the call
        r["sequence_num"] = base + np.arange(len(r))
        base += len(r)
    merged = []
    for day in (0, 1, 2):
        m = np.concatenate([r for r in parts if int(r["time_received"][0]) // DAY == D0 + day])
        merged.append(m[np.argsort(t32_of(m), kind="stable")])
    return dict(parts=parts, merged=merged, pool=pool, data=_forms(fa, [encode_part(r) for r in parts]), merged_data=_forms(fa, [encode_part(r) for r in merged]))


@pytest.mark.parametrize("form", ["plain", "lz4"])
def test_three_dates(gpu_lib, fa, three_dates, form):
    parts, data = three_dates["parts"], three_dates["data"][form]
    with fa.FlowAgg(framed=True) as a:
        # across the first midnight: the third Date's parts are skipped by Date
        want = _check(a, data, parts, dict(t_lo=MID + DAY - 50, t_hi=MID + DAY + 120, dst_port=(0, 443)))
        assert [d for d, _, _ in want][:4] == [D0, D0, D0 + 1, D0 + 1] and a.raw_range_stats()["parts_skipped_date"] == 2
        # the middle Date alone; its second part has no row of proto 1: no empty part is emitted
        want = _check(a, data, parts, dict(t_lo=MID + DAY, t_hi=MID + 2 * DAY, proto=1))
        assert [len(r) > 0 for _, r, _ in want] == [True, True] and a.raw_range_stats()["parts_skipped_date"] == 2 + 4
        want = _check(a, data, parts, dict(proto=1, either=True))
        assert [d for d, _, _ in want] == [D0, D0, D0 + 1, D0 + 1, D0 + 2, D0 + 2]
        _check(a, data, parts, dict(t_lo=MID + 2 * DAY + 3, t_hi=NO_UPPER, src_as=64502))


def test_merged_and_unmerged_inputs_give_the_same_rows(gpu_lib, fa, three_dates):
    f = dict(t_lo=MID + DAY - 80, t_hi=MID + 2 * DAY + 200, src_port=(53, 65535), etype=0x86DD)
    with fa.FlowAgg(framed=True) as a:
        _check(a, three_dates["merged_data"]["lz4"], three_dates["merged"], f)
        one, _ = a.raw_select(three_dates["merged_data"]["lz4"], **f)
        two, _ = a.raw_select(three_dates["data"]["lz4"], **f)
    rows = []
    for sel in (one, two):
        r = np.concatenate([S.rows_of_block(b) for b in fa.spill.read_native(sel)])
        rows.append(r[np.argsort(r["sequence_num"], kind="stable")])
    assert len(rows[0]) > 100 and rows[0].tobytes() == rows[1].tobytes()


def test_more_than_512_input_parts(gpu_lib, fa):
    """more sources than the gather's LDS table holds: its global-memory table"""
    rng = np.random.default_rng(18)
    pool = S.address_pool(rng)
    parts = [S.make_rows(rng, int(rng.integers(1, 40)), t0=MID + 1000 + 5 * i, span=5, pool=pool) for i in range(600)]
    data = b"".join(encode_part(r) for r in parts)
    with fa.FlowAgg(framed=True) as a:
        want = _check(a, data, parts, dict(proto=17))
        assert len(want) > 512
        want = _check(a, data, parts, dict(t_lo=MID + 1000 + 5 * 20 + 2, t_hi=MID + 1000 + 5 * 580 + 3, dst_as=64501, either=True))
        assert len(want) > 400
        mixed = b"".join(fa.lz4_frame(encode_part(r)) for r in parts)
        _check(a, mixed, parts, dict(src_port=(0, 80), limit=3000))


# ---- 6: the limit, COUNT_ONLY ----------------------------------------------------------------------------------------------------------------
def test_limit_and_count_only(gpu_lib, fa, three_dates):
    parts, data = three_dates["parts"][:3], b"".join(encode_part(r) for r in three_dates["parts"][:3])
    f = dict(proto=6)
    counts = [int(S.match(r, f).sum()) for r in parts]
    total = sum(counts)
    assert min(counts) > 10
    with fa.FlowAgg(framed=True) as a:
        for limit in (1, total - 1, total, total + 1, counts[0], counts[0] + 1, counts[0] + counts[1] // 2, counts[0] + counts[1]):
            want = _check(a, data, parts, dict(f, limit=limit))
            assert sum(len(r) for _, r, _ in want) == min(limit, total)
        assert len(_check(a, data, parts, dict(f, limit=counts[0] + counts[1] // 2))) == 2  # it runs out inside the second of three parts
        st0 = a.raw_select_stats()
        for g in (f, dict(f, limit=counts[0] + 5), dict(f, t_lo=MID + DAY - 20, t_hi=MID + DAY + 30)):
            sel, desc = a.raw_select(data, **g)
            none, only = a.raw_select(data, count_only=True, **g)
            assert none == b"" and a.raw_selection_device() == (0, 0)
            assert only.tobytes() == desc.tobytes() and int(only["bytes"].sum()) == len(sel) > 0
        st = a.raw_select_stats()
        assert st["calls"] == st0["calls"] + 6 and st["gather_ns"] >= st0["gather_ns"] and st["rows_matched"] > st["rows_out"]


# ---- 7: round trip --------------------------------------------------------------------------------------------------------------------------
def _folds(fa):
    agg = fa.FlowAgg(framed=True)
    agg.talkers_enable(0, bucket_secs=60)
    agg.ports_enable_buckets(0, bucket_secs=60)
    return agg


def _reads(agg):
    out = {}
    for d in (0, 1):
        for lo, hi in ((None, None), (MID + DAY - 120, MID + DAY + 180)):
            out["talkers", d, lo] = agg.top_talkers(d, 0, lo, hi)
            out["ports", d, lo] = agg.top_ports_range(d, 0, lo, hi)
    return out


def test_round_trip_through_raw_load(gpu_lib, fa, three_dates):
    f = dict(t_lo=MID + DAY - 200, t_hi=MID + DAY + 300, etype=0x86DD, dst_port=(53, 65536))
    want = S.expected(three_dates["parts"], f)
    with _folds(fa) as twin:
        twin.raw_load(b"".join(blob for _, _, blob in want))
        ref = _reads(twin)
    with _folds(fa) as a:
        sel, desc = a.raw_select(three_dates["data"]["lz4"], **f)
        a.raw_load(sel)
        got = _reads(a)
        assert a.raw_load_stats()["rows_loaded"] == sum(len(r) for _, r, _ in want) == int(desc["rows"].sum())
    assert got.keys() == ref.keys() and all(got[k].tobytes() == ref[k].tobytes() for k in got) and sum(len(v) for v in got.values()) > 0
    with fa.FlowAgg(framed=True) as a:  # a selection is itself a valid input of the select
        again, _ = a.raw_select(sel, **f)
        assert again == sel


# ---- 8: no decoding added -------------------------------------------------------------------------------------------------------------------
def test_no_decode_beyond_the_ranged_load(gpu_lib, fa, sized):
    i = SIZES.index(200000)
    data = fa.lz4_frame(sized["blobs"][i])
    lo, hi = MID + 1400, MID + 1430
    with _folds(fa) as twin:
        twin.raw_restore_range(data, lo, hi, 0, True)
        ref, rl = twin.raw_range_stats(), twin.raw_load_stats()
    with fa.FlowAgg(framed=True) as a:
        _check(a, data, [sized["parts"][i]], dict(t_lo=lo, t_hi=hi, src_net=(bytes(sized["pool"][2]), 64), either=True))
        st, ls = a.raw_range_stats(), a.raw_load_stats()
        assert st["blocks_decoded"] == ref["blocks_decoded"] < st["blocks_seen"] // 4 and st["blocks_seen"] == ref["blocks_seen"]
        assert ls["blocks"] == rl["blocks"] and ls["bytes_decoded"] == rl["bytes_decoded"] and ls["calls"] == st["calls"] == 1 and ls["rows_loaded"] == st["rows_loaded"] == 0


# ---- 9: protocol ----------------------------------------------------------------------------------------------------------------------------
def _raw(fa, a, arr, f, cap):
    parts = np.zeros(max(cap, 1), dtype=fa.RAW_PART_DTYPE)
    nparts, nbytes = C.c_size_t(99), C.c_size_t(99)
    rc = fa.lib().fa_raw_select(a._h, arr.ctypes.data, arr.size, C.byref(f), parts.ctypes.data, cap, C.byref(nparts), C.byref(nbytes))
    return rc, nparts.value, nbytes.value


def test_protocol(gpu_lib, fa, three_dates):
    L = fa.lib()
    parts, data = three_dates["parts"], three_dates["data"]["lz4"]
    arr = np.frombuffer(data, dtype=np.uint8)
    good = dict(proto=6)
    with _folds(fa) as a:
        sel, desc = a.raw_select(data, **good)
        p, n = a.raw_selection_device()
        assert p and n == len(sel) > 0
        st0, ls0, rs0 = a.raw_select_stats(), a.raw_load_stats(), a.raw_range_stats()
        # a fetch with too small a buffer returns the size and consumes nothing
        out = np.zeros(len(sel), dtype=np.uint8)
        need = C.c_size_t()
        assert L.fa_raw_selection_fetch(a._h, out.ctypes.data, len(sel) - 1, C.byref(need)) == ERR_CAPACITY and need.value == len(sel)
        assert L.fa_raw_selection_fetch(a._h, None, 0, C.byref(need)) == ERR_CAPACITY and need.value == len(sel)
        assert L.fa_raw_selection_fetch(a._h, out.ctypes.data, len(sel), C.byref(need)) == 0 and out.tobytes() == sel
        assert L.fa_raw_selection_fetch(a._h, out.ctypes.data, len(sel), None) == ERR_ARG and L.fa_raw_select_stats(a._h, None) == ERR_ARG
        assert a.raw_selection_device() == (p, n)
        # refused calls: no selection afterwards, the counters unmoved
        f = fa.raw_filter(**good)
        rc, np_, nb = _raw(fa, a, arr, f, len(parts) - 1)  # parts_cap below the input's parts: found before anything is copied
        assert (rc, np_, nb) == (ERR_CAPACITY, len(parts), 0) and a.raw_selection_device() == (0, 0)
        a.raw_select(data, **good)
        bad = []
        for k, v in (("fields", 2048), ("fields", 1 << 31), ("_pad", (C.c_uint8 * 2)(0, 1)), ("src_prefix_len", 129), ("dst_prefix_len", 200)):
            g = fa.raw_filter(src_net=(bytes(16), 8), dst_net=(bytes(16), 8))
            setattr(g, k, v)
            bad.append((k, g))
        bad += [("t_lo > t_hi", fa.raw_filter(5, 4)), ("tf_lo > tf_hi", fa.raw_filter(flow_start=(5, 4))), ("src_port", fa.raw_filter(src_port=(2, 1))),
                ("dst_port", fa.raw_filter(dst_port=(65536, 65535)))]
        for name, g in bad:
            a.raw_select(data, **good)
            rc, np_, nb = _raw(fa, a, arr, g, 16)
            assert (rc, np_, nb) == (ERR_ARG, 0, 0) and a.raw_selection_device() == (0, 0), name
            assert b"fa_raw_select: " in bytes(fa.lib().fa_last_error(a._h)), name
        ignored = fa.raw_filter(proto=6)  # a member whose bit is clear is not read
        ignored.tf_lo, ignored.tf_hi, ignored.src_port_lo, ignored.src_prefix_len = 5, 4, 9, 255
        assert _raw(fa, a, arr, ignored, 16)[0] == 0
        name, frame, text = R.malformed(fa.spill._xxh32)[0]
        unsorted = parts[0].copy()
        unsorted["time_received"][[10, 11]] = unsorted["time_received"][[11, 10]] + np.array([1, 0], dtype=np.uint64)
        assert unsorted["time_received"][10] > unsorted["time_received"][11]
        n_sel = a.raw_select_stats()["calls"]
        for inp, text in ((frame, text), (data + frame, text), (encode_part(unsorted), r"TimeReceived descends behind row 10\b"),
                          (fa.lz4_frame(encode_part(parts[1])) + fa.lz4_frame(encode_part(unsorted)), r"frame 1 \(part 1\): TimeReceived descends behind row 10\b")):
            a.raw_select(data, **good)
            n_sel += 1
            before = a.raw_select_stats(), a.raw_range_stats()["calls"], a.raw_load_stats()["calls"]
            with pytest.raises(fa.FlowAggError, match=text) as e:
                a.raw_select(inp, **good)
            assert e.value.code == ERR_FRAMING and a.raw_selection_device() == (0, 0)
            assert (a.raw_select_stats(), a.raw_range_stats()["calls"], a.raw_load_stats()["calls"]) == before and before[0]["calls"] == n_sel
        assert L.fa_raw_select(a._h, None, 5, C.byref(f), None, 0, C.byref(need), C.byref(need)) == ERR_ARG
        assert L.fa_raw_select(a._h, arr.ctypes.data, arr.size, None, None, 0, C.byref(need), C.byref(need)) == ERR_ARG
        assert L.fa_raw_select(a._h, arr.ctypes.data, arr.size, C.byref(f), None, 4, C.byref(need), C.byref(need)) == ERR_ARG
        # the counters of the calls that succeeded: one ranged call each, nothing loaded
        st, ls, rs = a.raw_select_stats(), a.raw_load_stats(), a.raw_range_stats()
        assert rs["calls"] - rs0["calls"] == ls["calls"] - ls0["calls"] == st["calls"] - st0["calls"] and ls["rows_loaded"] == rs["rows_loaded"] == 0
        # the selection is dead after the next load call, of any kind; the ctx goes on
        for door in (lambda: a.raw_load(encode_part(parts[3])), lambda: a.raw_range_probe(data, 0, NO_UPPER), lambda: a.raw_columns(encode_part(parts[3])),
                     lambda: a.raw_restore_range(data, MID, MID + 5, 0, True), lambda: a.raw_load_reset()):
            again, _ = a.raw_select(data, **good)
            assert again == sel and a.raw_selection_device()[1] == len(sel)
            door()
            assert a.raw_selection_device() == (0, 0)
            assert L.fa_raw_selection_fetch(a._h, out.ctypes.data, len(sel), C.byref(need)) == 0 and need.value == 0
        assert a.raw_select(b"")[0] == b"" and len(a.raw_select(b"")[1]) == 0
    with fa.FlowAgg(framed=True) as a:  # a ctx that never selected
        assert a.raw_selection_device() == (0, 0) and a.raw_select_stats() == dict.fromkeys(a.raw_select_stats(), 0)


def test_page_locked_out(gpu_lib, fa, three_dates):
    import torch
    f = dict(proto=17, either=True)
    want = b"".join(blob for _, _, blob in S.expected(three_dates["parts"], f))
    pinned = torch.empty(len(want) + 100, dtype=torch.uint8).pin_memory().numpy()
    with fa.FlowAgg(framed=True) as a:
        got, desc = a.raw_select(three_dates["data"]["plain"], out=pinned, **f)
        assert got.base is not None and np.shares_memory(got, pinned) and got.tobytes() == want


# ---- 10: seeded differential -----------------------------------------------------------------------------------------------------------------
DEFAULT_SEEDS = 12


def test_the_generator_selects_some_rows_and_not_all():
    """a condition on the generator, computed by the restatement alone: at least a third of the default seeds' filters select more than
    0 and fewer than all rows of their slice (10 of 12 when this was written)"""
    some = 0
    for seed in range(DEFAULT_SEEDS):
        parts, f = S.fuzz_case(seed)
        rows = np.concatenate(parts)
        in_slice = int(S.in_range(t32_of(rows), f["t_lo"], f["t_hi"]).sum())
        some += 0 < int(S.match(rows, f).sum()) < in_slice
    assert 3 * some >= DEFAULT_SEEDS


@pytest.mark.parametrize("seed", range(int(os.environ.get("FA_FUZZ_SEEDS", str(DEFAULT_SEEDS)))))  # (soak runs: FA_FUZZ_SEEDS=200)
def test_seeded_differential(gpu_lib, fa, seed):
    parts, f = S.fuzz_case(seed)
    blobs = [encode_part(r) for r in parts]
    with fa.FlowAgg(framed=True) as a:
        for data in _forms(fa, blobs).values():
            _check(a, data, parts, f)
        _check(a, blobs[-1], parts[-1:], f)  # the last part alone
