"""GPU tests of the sketches from columns and from parts (fa_sketch_fold_columns_device, fa_raw_restore, fa_sketch_fold_stats;
include/flowagg.h "ABI 8, addition: the sketches from columns and from parts").

Expected values never come from the code under test: they are po.cms_sketch_numpy / po.cms_estimates_numpy / po.topk_candidates
(oracle/pyoracle.py), the reads of a twin ctx that INGESTED the same records' wire bytes, or numpy over the rows the test wrote.
Every comparison is bit-exact.  Sketches are small (cms_width_log2 = 12 unless a test says otherwise)."""
import numpy as np
import pytest

import raw_load_cases as R
from test_raw_load_gpu import _as_rows
from test_raw_parts_gpu import D0, DAY, _midnight, _upload, expected_parts
from test_rollup_fold_gpu import _wire

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_FRAMING, ERR_UNSUPPORTED = -1, -7, -8
SRC, DST = 2, 4  # FA_KEYS_SRCADDR_CMS, FA_KEYS_DSTADDR_CMS
SETS = (("src_addr", SRC, "src"), ("dst_addr", DST, "dst"))
DEPTH, WL2, SEED = 4, 12, 0x5EED
CACHE = 256  # entries per direction of the fold kernel's LDS cache (csrc/sketch_fold.cuh, SKETCH_ENTRIES)
NO_UPPER = 0xFFFFFFFF
ZERO_STATS = dict(calls=0, records_in=0, records_bad=0, records_folded=0, batches=0, launches=0, fold_ns=0)


def _ctx(fa, key_sets=1 | SRC | DST, depth=DEPTH, wl2=WL2, cap=12, **kw):
    return fa.FlowAgg(framed=True, key_sets=key_sets, cms_depth=depth, cms_width_log2=wl2, cms_seed=SEED, topk_capacity_log2=cap, **kw)


def _weights(rows):
    with np.errstate(over="ignore"):
        return rows["bytes"] * rows["sampling_rate"]


def _sketch_np(po, rows, status, col, depth=DEPTH, wl2=WL2):
    r = rows[status == 0]
    return po.cms_sketch_numpy(r[col], _weights(r), depth, wl2, SEED)


def _ranked(keys, est):
    """weight descending, ties by key bytes ascending -> [(key, weight)]"""
    return [(k, -e) for e, k in sorted(zip((-est.astype(object)).tolist(), [bytes(k) for k in keys]))]


def _ranking_np(po, rows, status, col, depth=DEPTH, wl2=WL2):
    r = rows[status == 0]
    keys = np.unique(np.ascontiguousarray(r[col]), axis=0)
    return _ranked(keys, po.cms_estimates_numpy(_sketch_np(po, rows, status, col, depth, wl2), keys, depth, wl2, SEED))


def _got(topk):
    return [(bytes(r["key"]), int(r["weight"])) for r in topk]


def _fold(fa, agg, rows, status=None, key_sets=0):
    status = np.zeros(len(rows), dtype=np.uint8) if status is None else status
    cols, keep = _upload(fa, rows, status)
    agg.sketch_fold_columns(cols, len(rows), key_sets)
    del keep


def _check_np(po, agg, rows, status=None, depth=DEPTH, wl2=WL2, sets=SETS):
    """both sketches and the full rankings of a ctx against numpy over the rows it was given"""
    status = np.zeros(len(rows), dtype=np.uint8) if status is None else status
    for col, ks, _ in sets:
        assert np.array_equal(agg.cms_read(ks).reshape(-1), _sketch_np(po, rows, status, col, depth, wl2)), col
        assert _got(agg.topk(ks, 1 << 20)) == _ranking_np(po, rows, status, col, depth, wl2), col


def _stats_add_up(agg, records_in, records_bad, batches, calls):
    """the fold's counters add up; the wire-record counters have not moved"""
    s = agg.sketch_fold_stats()
    assert (s["calls"], s["records_in"], s["records_bad"], s["records_folded"], s["batches"], s["launches"]) == \
        (calls, records_in, records_bad, records_in - records_bad, batches, batches), s
    assert (s["fold_ns"] > 0) == (batches > 0)


def _hand_rows(po, n, seed, src, dst=None):
    """n rows with the given uint8[n,16] addresses; weights below 2^32, everything else plain"""
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    rows["time_received"] = D0 * DAY + rng.integers(0, 300, n)
    rows["time_flow_start"] = rows["time_received"]
    rows["bytes"], rows["sampling_rate"], rows["packets"] = rng.integers(1, 1 << 20, n), rng.integers(1, 1 << 12, n), 1
    rows["src_as"], rows["dst_as"], rows["etype"], rows["proto"] = 65000, 65001, 0x800, 6
    rows["src_addr"] = src
    rows["dst_addr"] = src if dst is None else dst
    return rows


def _pool(seed, k):
    return np.random.default_rng(seed).integers(0, 256, (k, 16), dtype=np.uint8)


def _wire_checked(fa, po, rows):
    """the test's encoder writes what it was given: the twin ingests exactly these rows"""
    buf, off = _wire(fa, rows)
    back, status = po.decode_batch(buf, off, 1)
    assert not status.any() and back.tobytes() == rows.tobytes()
    return buf, off


# ---- 1: exact mode, three ways equal ------------------------------------------------------------------------------------------------------
def test_exact_mode_three_ways_equal(gpu_lib, fa, po):
    n = 1000
    rows = _as_rows(po, R.random_rows(11, n, keys=60))
    status = (np.arange(n) % 97 == 96).astype(np.uint8)
    buf, off = _wire_checked(fa, po, rows[status == 0])
    with _ctx(fa) as a, _ctx(fa) as twin:
        assert a.sketch_fold_stats() == ZERO_STATS
        _fold(fa, a, rows, status)
        twin.ingest(buf, off)
        for col, ks, _ in SETS:
            sk = a.cms_read(ks)
            assert np.array_equal(sk.reshape(-1), _sketch_np(po, rows, status, col)) and np.array_equal(sk, twin.cms_read(ks))
            want = _ranking_np(po, rows, status, col)
            for k in (1, 10, len(want)):
                got = a.topk(ks, k)
                assert got.tobytes() == twin.topk(ks, k).tobytes() and _got(got) == want[:k], (col, k)
        _stats_add_up(a, n, int(status.sum()), 1, 1)
        assert a.stats()["records_ok"] == 0 and a.stats()["batches"] == 0 and len(a.read_window()) == 0  # flows_5m is not this door's


# ---- 2: geometry ----------------------------------------------------------------------------------------------------------------------------
def test_geometry_small_grid(gpu_lib, fa, po, monkeypatch):
    monkeypatch.setenv("FA_SKETCH_GRID", "2")
    for n in (1, 63, 64, 65, 255, 256, 257, 1025, 5000):
        rows = _as_rows(po, R.random_rows(200 + n, n, keys=60))
        status = (np.arange(n) % 11 == 5).astype(np.uint8)
        with _ctx(fa) as a:
            _fold(fa, a, rows, status)
            _check_np(po, a, rows, status)
            _stats_add_up(a, n, int(status.sum()), 1, 1)


# ---- 3: cache edges (one workgroup sees everything; once more without the cache) ----------------------------------------------------------
def _edge_case(po, name):
    if name == "one_address":  # 5 000 records of ONE address in both directions
        return _hand_rows(po, 5000, 1, np.tile(_pool(2, 1), (5000, 1)))
    if name == "more_than_the_cache":  # four times the cache's entries, and one heavy address: misses and the flush, by counting
        pool = _pool(3, 4 * CACHE + 1)
        idx = np.concatenate([np.arange(4 * CACHE + 1), np.arange(4 * CACHE), np.full(2000, 4 * CACHE)])
        np.random.default_rng(4).shuffle(idx)
        rows = _hand_rows(po, len(idx), 5, pool[idx], pool[idx[::-1]])
        assert len(np.unique(rows["src_addr"], axis=0)) == 4 * CACHE + 1 > CACHE
        return rows
    if name == "zero_address":  # an absent address field: a key like any other
        pool = _pool(6, 20)
        pool[7] = 0
        rows = _hand_rows(po, 400, 7, pool[np.arange(400) % 20], pool[(np.arange(400) * 3) % 20])
        assert not rows["src_addr"][7].any()
        return rows
    if name == "zero_sums":  # weights that sum to 0 mod 2^64, and an address with Bytes = 0 only: rows of the ranking all the same
        pool = _pool(8, 12)
        rows = _hand_rows(po, 240, 9, pool[np.arange(240) % 12])
        x, y = rows["src_addr"][0].copy(), rows["src_addr"][1].copy()
        isx, isy = (rows["src_addr"] == x).all(axis=1), (rows["src_addr"] == y).all(axis=1)
        rows = rows[~isx | (np.cumsum(isx) <= 2)]  # two records of x
        isx, isy = (rows["src_addr"] == x).all(axis=1), (rows["src_addr"] == y).all(axis=1)
        rows["bytes"][isx], rows["sampling_rate"][isx] = np.uint64(1 << 63), 1
        rows["bytes"][isy] = 0
        assert isx.sum() == 2 and int(_weights(rows)[isx].sum(dtype=np.uint64)) == 0 and isy.sum() > 2 and not _weights(rows)[isy].any()
        return rows
    if name == "wrapping_product":  # Bytes = 2^40, SamplingRate = 2^30
        pool = _pool(10, 9)
        rows = _hand_rows(po, 300, 11, pool[np.arange(300) % 9])
        rows["bytes"][::2], rows["sampling_rate"][::2] = np.uint64(1 << 40), np.uint64(1 << 30)
        assert int(rows["bytes"][0]) * int(rows["sampling_rate"][0]) >= 1 << 64
        return rows
    if name == "etype_is_no_part_of_the_key":  # one address with EType 0x800 and with 0x86DD: one key
        rows = _hand_rows(po, 200, 12, np.tile(_pool(13, 1), (200, 1)))
        rows["etype"] = np.where(np.arange(200) % 2 == 0, 0x800, 0x86DD)
        return rows
    raise KeyError(name)


EDGE_CASES = ("one_address", "more_than_the_cache", "zero_address", "zero_sums", "wrapping_product", "etype_is_no_part_of_the_key")


@pytest.mark.parametrize("lds", ["", "0"], ids=["cache", "no_cache"])
@pytest.mark.parametrize("name", EDGE_CASES)
def test_cache_edges(gpu_lib, fa, po, monkeypatch, name, lds):
    monkeypatch.setenv("FA_SKETCH_GRID", "1")
    if lds:
        monkeypatch.setenv("FA_SKETCH_LDS", lds)
    else:
        monkeypatch.delenv("FA_SKETCH_LDS", raising=False)
    rows = _edge_case(po, name)
    with _ctx(fa) as a:
        _fold(fa, a, rows)
        _check_np(po, a, rows)
        full = _got(a.topk(SRC, 1 << 20))
        if name == "zero_address":
            assert bytes(16) in [k for k, _ in full] and bytes(16) in [k for k, _ in _got(a.topk(DST, 1 << 20))]
        if name == "zero_sums":  # both addresses are rows, with the estimate numpy gives (>= 0: other keys' collisions only)
            assert len(full) == 12 and {bytes(rows["src_addr"][0]), bytes(rows["src_addr"][1])} <= {k for k, _ in full}
        if name in ("one_address", "etype_is_no_part_of_the_key"):
            assert len(full) == 1
        _stats_add_up(a, len(rows), 0, 1, 1)


# ---- 4: sketch geometries: the smallest fa_create takes, a non-scatterable one, the smallest scatterable one, the default ------------------
@pytest.mark.parametrize("depth,wl2", [(1, 4), (16, 8), (4, 12), (4, 20)])
def test_sketch_geometries(gpu_lib, fa, po, depth, wl2):
    n = 2000
    pool = _pool(20, 300)
    rng = np.random.default_rng(21)
    rows = _hand_rows(po, n, 22, pool[rng.integers(0, 300, n)], pool[rng.integers(0, 300, n)])
    with _ctx(fa, depth=depth, wl2=wl2) as a:
        _fold(fa, a, rows)
        _check_np(po, a, rows, depth=depth, wl2=wl2)


# ---- 5: selection ----------------------------------------------------------------------------------------------------------------------------
def test_selection(gpu_lib, fa, po):
    rows = _as_rows(po, R.random_rows(31, 700, keys=40))
    zero = np.zeros(len(rows), dtype=np.uint8)
    with _ctx(fa) as a:
        _fold(fa, a, rows, key_sets=SRC)
        assert not a.cms_read(DST).any() and len(a.topk(DST, 100)) == 0
        _check_np(po, a, rows, sets=SETS[:1])
    with _ctx(fa) as a:
        _fold(fa, a, rows, key_sets=0)
        _check_np(po, a, rows)
    with _ctx(fa, key_sets=1 | DST) as a:  # created with the DstAddr sketch only: SrcAddr is not read
        cols, keep = _upload(fa, rows, zero)
        cols.src_addr = None
        a.sketch_fold_columns(cols, len(rows))
        _check_np(po, a, rows, sets=SETS[1:])
        _stats_add_up(a, len(rows), 0, 1, 1)
        del keep


# ---- 6: additive --------------------------------------------------------------------------------------------------------------------------------
def test_additive_in_both_orders(gpu_lib, fa, po):
    n = 1200
    rows = _as_rows(po, R.random_rows(41, n, keys=80))
    h = n // 2
    buf, off = _wire_checked(fa, po, rows)
    ba, oa = buf[:int(off[h])], off[:h + 1]
    bb, ob = buf[int(off[h]):], off[h:] - off[h]
    with _ctx(fa) as x, _ctx(fa) as y, _ctx(fa) as twin:
        twin.ingest(buf, off)
        x.ingest(ba, oa)
        _fold(fa, x, rows[h:])
        _fold(fa, y, rows[:h])
        y.ingest(bb, ob)
        for c in (x, y):
            for _, ks, _ in SETS:
                assert np.array_equal(c.cms_read(ks), twin.cms_read(ks)) and c.topk(ks, 1 << 20).tobytes() == twin.topk(ks, 1 << 20).tobytes()
            _check_np(po, c, rows)
            assert c.stats()["records_ok"] == h
        for c in (x, y, twin):
            c.cms_reset(SRC), c.cms_reset(DST)
        twin.ingest(bb, ob)
        _fold(fa, x, rows[h:])
        for _, ks, _ in SETS:
            assert not y.cms_read(ks).any() and len(y.topk(ks, 10)) == 0
            assert np.array_equal(x.cms_read(ks), twin.cms_read(ks)) and x.topk(ks, 1 << 20).tobytes() == twin.topk(ks, 1 << 20).tobytes()
        _check_np(po, x, rows[h:])
        _stats_add_up(x, 2 * (n - h), 0, 2, 2)


# ---- 7: candidates mode ---------------------------------------------------------------------------------------------------------------------------
TRACK, CAP = 8, 8


def _zipf_batches(po, nb=4, m=3000, seed=51, universe=600):
    """nb batches of m hand-made rows whose addresses follow a Zipf-1.1 law over `universe` addresses (both directions, independently)"""
    rng = np.random.default_rng(seed)
    pool = _pool(seed + 1, universe)
    p = 1.0 / np.arange(1, universe + 1) ** 1.1
    p /= p.sum()
    return [_hand_rows(po, m, seed + 2 + b, pool[rng.choice(universe, m, p=p)], pool[rng.choice(universe, m, p=p)]) for b in range(nb)]


def _oracle(po, batches, col, track=TRACK, cap=CAP):
    return po.topk_candidates([(b[col], _weights(b)) for b in batches], DEPTH, WL2, SEED, track=track, capacity_log2=cap)


def _cand_ctx(fa, **kw):
    return _ctx(fa, cap=CAP, topk_mode=fa.TOPK_CANDIDATES, topk_track=TRACK, **kw)


def _check_oracle(po, agg, batches, what="", track=TRACK, cap=CAP):
    st = agg.stats()
    for col, ks, tag in SETS:
        sk, cand, est, thetas = _oracle(po, batches, col, track, cap)
        assert np.array_equal(agg.cms_read(ks).reshape(-1), sk), (what, col)
        assert _got(agg.topk(ks, 1 << cap)) == _ranked(cand, est), (what, col)
        assert st["topk_theta_" + tag] == thetas[-1] and st["topk_candidates_" + tag] == len(cand), (what, col)


def test_candidates_batch_by_batch(gpu_lib, fa, po):
    batches = _zipf_batches(po)
    for col, _, _ in SETS:  # from the oracle alone: the stream admits some addresses, not all
        _, cand, _, thetas = _oracle(po, batches, col)
        assert 0 < len(cand) < len(np.unique(np.concatenate([b[col] for b in batches]), axis=0)) and len(thetas) == 4
        assert len(_oracle(po, batches[:1], col)[1]) == 0  # nothing is admitted in the first batch
    with _cand_ctx(fa) as a, _cand_ctx(fa) as twin:
        for t, b in enumerate(batches):
            _fold(fa, a, b)
            twin.ingest(*_wire_checked(fa, po, b))
            sa, st = a.stats(), twin.stats()
            for _, ks, tag in SETS:
                assert np.array_equal(a.cms_read(ks), twin.cms_read(ks)) and a.topk(ks, TRACK).tobytes() == twin.topk(ks, TRACK).tobytes(), (t, tag)
                assert sa["topk_theta_" + tag] == st["topk_theta_" + tag] and sa["topk_candidates_" + tag] == st["topk_candidates_" + tag], (t, tag)
            _check_oracle(po, a, batches[:t + 1], t)
        _stats_add_up(a, 4 * 3000, 0, 4, 4)
        assert a.stats()["kernel_launches"] == 0 and twin.stats()["kernel_launches"] == 4


def test_candidates_chunks_are_batches(gpu_lib, fa, po):
    rows = np.concatenate(_zipf_batches(po, nb=1, m=3500, seed=61))
    with _cand_ctx(fa, max_batch_records=1000) as a:
        _fold(fa, a, rows)
        _check_oracle(po, a, [rows[0:1000], rows[1000:2000], rows[2000:3000], rows[3000:]])
        _stats_add_up(a, 3500, 0, 4, 1)
    for col, _, _ in SETS:  # (the cut matters: one batch of 3 500 admits nothing)
        assert len(_oracle(po, [rows], col)[1]) == 0 < len(_oracle(po, [rows[0:1000], rows[1000:2000], rows[2000:3000], rows[3000:]], col)[1])


def test_candidates_ingest_then_fold_on_one_ctx(gpu_lib, fa, po):
    batches = _zipf_batches(po, seed=71)
    with _cand_ctx(fa) as a:
        a.ingest(*_wire_checked(fa, po, batches[0]))  # the ctx's first batch is an ingest launch: nothing admitted
        assert len(a.topk(SRC, TRACK)) == 0
        for b in batches[1:]:
            _fold(fa, a, b)  # admitted against the bits the ingest launch's boundary left
        _check_oracle(po, a, batches)
        assert len(a.topk(SRC, TRACK)) > 0
    with _cand_ctx(fa) as a:  # and the other way round
        for b in batches[:3]:
            _fold(fa, a, b)
        a.ingest(*_wire_checked(fa, po, batches[3]))
        _check_oracle(po, a, batches)


# ---- 8: from parts ------------------------------------------------------------------------------------------------------------------------------
KS6 = 1 | 2 | 4 | 8 | 16 | 32
FORMS = ("plain", "lz4", "plain_merged", "lz4_merged")


def _full_ctx(fa, **kw):
    a = _ctx(fa, key_sets=KS6, cap=16, **kw)
    a.talkers_enable(0, bucket_secs=60)
    a.ports_enable_buckets(0, bucket_secs=60)
    return a


def _all_reads(agg):
    out = dict(rows=agg.read_window(), app=agg.read_window_app(), sport=agg.top_ports(0), dport=agg.top_ports(1), minutes=agg.minute_series())
    for d in (0, 1):
        out["talkers", d] = agg.top_talkers(d, 100, 0, NO_UPPER)
        out["ports", d] = agg.top_ports_range(d, 100, 0, NO_UPPER)
    for _, ks, tag in SETS:
        out["cms", tag] = agg.cms_read(ks)
        out["topk", tag] = agg.topk(ks, 1 << 16)
    return out


@pytest.fixture(scope="module")
def ingested(gpu_lib, fa):
    buf, off, rows, status = _midnight(bad_every=97)
    out = {}
    for form in FORMS:
        with _full_ctx(fa) as a:
            a.raw_enable(7000)  # three chunks x two Dates
            a.ingest(buf, off)
            if form.endswith("_merged"):
                a.raw_merge()
            data, parts = a.raw_take_lz4() if form.startswith("lz4") else a.raw_take()
            assert len(parts) == (2 if form.endswith("_merged") else 6)
            out[form] = bytes(data)
            if "reads" not in out:
                out["reads"] = _all_reads(a)
    out["good"] = int((status == 0).sum())
    return out


@pytest.mark.parametrize("form", FORMS)
def test_restore_equals_ingest(gpu_lib, fa, ingested, form):
    with _full_ctx(fa) as b:
        b.raw_restore(ingested[form], 0, folds=True)
        got, want = _all_reads(b), ingested["reads"]
        assert got.keys() == want.keys()
        for k in got:
            assert len(got[k]) > 0 and got[k].tobytes() == want[k].tobytes(), k
        nparts = 2 if form.endswith("_merged") else 6
        _stats_add_up(b, ingested["good"], 0, nparts, 1)
        rs, ls, st = b.rollup_stats(), b.raw_load_stats(), b.stats()
        assert rs["calls"] == 1 and rs["records_in"] == ingested["good"] and rs["launches"] == nparts
        assert ls["calls"] == 1 and ls["parts"] == nparts and ls["rows_loaded"] == ingested["good"]
        assert b.talkers_stats()["records_folded"] == b.ports_stats()["records_folded"] == ingested["good"]
        assert st["records_ok"] == st["records_bad"] == st["bytes_in"] == st["batches"] == 0


def test_restore_candidates_cut_at_parts_and_cap(gpu_lib, fa, po, ingested):
    """the documented chunk cuts are the batches: part boundaries and the cap (max_batch_records = 3 000 here)"""
    buf, off, rows, status = _midnight(bad_every=97)
    cap = 3000
    parts = [r for c0 in range(0, len(rows), 7000) for _, r, _ in expected_parts(rows[c0:c0 + 7000], status[c0:c0 + 7000])]  # the six parts' rows, in take order
    assert len(parts) == 6 and sum(len(r) for r in parts) == ingested["good"] and max(len(r) for r in parts) > cap
    batches = [r[i:i + cap] for r in parts for i in range(0, len(r), cap)]
    track, tcap = 64, 12  # (this stream has 10 000 light addresses: a threshold low enough to admit some of them)
    for col, _, _ in SETS:
        assert 0 < len(_oracle(po, batches, col, track, tcap)[1]) < len(np.unique(rows[col][status == 0], axis=0))
    with _ctx(fa, key_sets=1 | SRC | DST, cap=tcap, topk_mode=fa.TOPK_CANDIDATES, topk_track=track, max_batch_records=cap) as b:
        b.raw_restore(ingested["plain"], SRC | DST)
        _check_oracle(po, b, batches, "parts", track, tcap)
        _stats_add_up(b, ingested["good"], 0, len(batches), 1)
        assert len(b.read_window()) == 0 and b.rollup_stats()["calls"] == 0  # flows_5m was not selected


# ---- 9: refusals, each leaving the ctx usable and nothing folded -----------------------------------------------------------------------------------
def test_refusals(gpu_lib, fa, po, ingested):
    rows = _as_rows(po, R.random_rows(81, 100, keys=20))
    zero = np.zeros(100, dtype=np.uint8)
    cols, keep = _upload(fa, rows, zero)

    def refused(call, code, match=None):
        with pytest.raises(fa.FlowAggError, match=match) as e:
            call()
        assert e.value.code == code

    with fa.FlowAgg(framed=True, key_sets=1 | 16) as a:  # a ctx without a sketch
        refused(lambda: a.sketch_fold_columns(cols, 100), ERR_UNSUPPORTED, "without a sketch")
        assert a.sketch_fold_stats() == ZERO_STATS
    with _ctx(fa, key_sets=1 | SRC) as a:
        for ks in (1, 8, 1 | SRC, DST, SRC | DST, 64):  # an exact bit, a sketch bit the ctx lacks, a bit above the six
            refused(lambda: a.sketch_fold_columns(cols, 100, ks), ERR_ARG, "not a sketch this ctx was created with")
        refused(lambda: a.raw_restore(ingested["lz4"], DST), ERR_ARG, "not created with")
        for name, value in (("bytes", None), ("status", None), ("sampling_rate", None), ("src_addr", None), ("bytes", cols.bytes + 4), ("src_addr", cols.src_addr + 8),
                            ("dst_addr", cols.dst_addr + 8), ("src_as", cols.src_as + 2)):  # (dst_addr, src_as are not read: whatever is given must be aligned)
            bad = fa.Columns()
            for f, _ in fa.Columns._fields_:
                setattr(bad, f, getattr(cols, f))
            setattr(bad, name, value)
            refused(lambda: a.sketch_fold_columns(bad, 100), ERR_ARG, "naturally aligned")
        refused(lambda: a.sketch_fold_columns(None, 100), ERR_ARG)
        a.sketch_fold_columns(None, 0)  # n == 0: FA_OK, nothing looked at, no launch counted
        a.sketch_fold_columns(cols, 0)
        assert a.sketch_fold_stats() == ZERO_STATS and not a.cms_read(SRC).any()
        # a frame with a flipped header byte: nothing is folded, every counter stays
        frames = bytearray(ingested["lz4"])
        frames[4] ^= 0x40
        before = (a.sketch_fold_stats(), a.rollup_stats(), a.raw_load_stats())
        refused(lambda: a.raw_restore(bytes(frames)), ERR_FRAMING)
        assert (a.sketch_fold_stats(), a.rollup_stats(), a.raw_load_stats()) == before
        assert not a.cms_read(SRC).any() and len(a.topk(SRC, 10)) == 0 and len(a.read_window()) == 0
        _fold(fa, a, rows)  # the ctx is usable
        _check_np(po, a, rows, sets=SETS[:1])
        _stats_add_up(a, 100, 0, 1, 1)
    with fa.FlowAgg(framed=True, key_sets=1) as a:  # a ctx without a sketch restores what it has: key_sets = 0 selects flows_5m alone
        a.raw_restore(ingested["lz4"])
        assert len(a.read_window()) > 0 and a.sketch_fold_stats() == ZERO_STATS
    del keep


# ---- 10: merged view --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feed", ["fold", "ingest"])
def test_a_fold_makes_the_merged_view_stale(gpu_lib, fa, po, feed):
    import torch
    rows = _as_rows(po, R.random_rows(91, 300, keys=20))
    with _ctx(fa) as a:
        st = a.device_state()
        for merged in (st.cms_src_merged, st.cms_dst_merged):
            torch.as_tensor(fa.dist._DevArray(merged, st.cms_words), device="cuda").fill_(7)
        torch.cuda.synchronize()
        a.merged_view_set(True)
        assert (a.cms_read(SRC) == 7).all() and (a.cms_read(DST) == 7).all()  # the reads answer from the merged view
        if feed == "fold":
            _fold(fa, a, rows)
        else:
            a.ingest(*_wire_checked(fa, po, rows))
        _check_np(po, a, rows)  # ... and from the ctx's own sketch again
