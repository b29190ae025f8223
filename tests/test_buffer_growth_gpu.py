"""Every growing buffer of a ctx grows at least once, and the results stay bit-exact: one ctx created with the smallest
legal capacities takes three rounds of 1 000, 65 537 and 1 000 records.  The second round crosses every minimum of the
host side's sizing rules (2^16 records for the deferral lists and the columns, 1 MiB of staging, every scratch buffer
the first round sized) and makes both tables and the talker tables grow.  After every round the flows_5m window, the
(SrcAddr,DstPort,Proto) rows, the top ports, the top-k and the top talkers are compared with the oracle as
tests/test_gpu_parity.py, tests/test_wide_keysets_gpu.py and tests/test_talkers_gpu.py compare them.  Then the ctx is
destroyed and a second one repeats the first round.  No failure is provoked."""
import functools

import numpy as np
import pytest

from test_gpu_parity import assert_decode_equal
from test_talkers_gpu import _same as same_talkers, restate
from test_wide_keysets_gpu import APP_COLS, _same

pytestmark = pytest.mark.gpu

ROUNDS = (1000, 65537, 1000)
DEPTH, WL2, SEED = 4, 10, 0xBEEF


@functools.lru_cache(maxsize=None)
def _stream():
    """The generated stream and its oracle decode - computed once, read-only."""
    import _pkg
    po = _pkg.load_oracle()
    n = sum(ROUNDS)
    gp = po.gen_params(mode=2, framed=1, seed=91, n_total=n, span_secs=900, per_sec=60, zipf_s_x100=100, zipf_log2_universe=6)
    buf, off = po.gen_records(gp, 0, n)
    rows, status = po.decode_batch(buf, off, 1)
    for a in (buf, off, rows, status):
        a.setflags(write=False)
    return buf, off, rows, status


def _want_topk(po, rows, col):
    """Every distinct address ranked by its Count-Min estimate: weight descending, then key bytes (test_topk_matches_oracle)."""
    with np.errstate(over="ignore"):
        w = rows["bytes"] * rows["sampling_rate"]
    cms = po.cms_sketch_numpy(np.ascontiguousarray(rows[col]), w, DEPTH, WL2, SEED)
    keys = {bytes(k) for k in np.unique(np.ascontiguousarray(rows[col]).view([("k", "u1", 16)]).reshape(-1)).view(np.uint8).reshape(-1, 16)}
    return sorted(((po.cms_query(cms, DEPTH, WL2, SEED, k), k) for k in keys), key=lambda t: (-t[0], t[1]))


def _round(fa, po, agg, ref, lo, hi):
    """Records [lo, hi) through fa_ingest and fa_decode; every read against the oracle's state after records [0, hi)."""
    buf, off, rows, status = _stream()
    piece, poff = buf[int(off[lo]):int(off[hi])], off[lo:hi + 1] - off[lo]
    agg.ingest(piece, poff)
    assert_decode_equal(agg.decode(piece, poff), rows[lo:hi], status[lo:hi])
    ref.ingest(piece, poff, 1)
    r, s = rows[:hi], status[:hi]
    assert agg.read_window().tobytes() == ref.rows().tobytes()
    _same(agg.read_window_app(), po.rollup_app(r, s, 300), APP_COLS)
    for d in (0, 1):
        _same(agg.top_ports(d), po.top_ports(r, s, d), ("port", "weight", "count"))
        same_talkers(agg.top_talkers(d), restate(fa, po, r, s, d))
    for col, ks in (("src_addr", fa.FA_KEYS_SRCADDR_CMS), ("dst_addr", fa.FA_KEYS_DSTADDR_CMS)):
        want = _want_topk(po, r[s == 0], col)
        got = agg.topk(ks, 1 << 8)
        assert [(int(g["weight"]), bytes(g["key"])) for g in got] == want, col


def _ctx(fa):
    agg = fa.FlowAgg(framed=True, key_sets=63, table_capacity_log2=10, wide_capacity_log2=8, topk_capacity_log2=8,
                     cms_depth=DEPTH, cms_width_log2=WL2, cms_seed=SEED)
    agg.talkers_enable(8)
    return agg


def test_three_rounds_across_every_minimum_then_a_second_ctx(gpu_lib, fa, po):
    _, _, _, status = _stream()
    assert status.sum() == 0
    with _ctx(fa) as agg:
        first = agg.stats()
        assert first["table_capacity"] == 1 << 10 and first["wide_capacity"] == 1 << 8
        ref, lo = po.Rollup(300), 0
        for n in ROUNDS:
            _round(fa, po, agg, ref, lo, lo + n)
            lo += n
        st = agg.stats()
        assert st["table_capacity"] > 1 << 10 and st["wide_capacity"] > 1 << 8
        assert agg.talkers_stats()["grows"] > 0
        assert st["records_bad"] == 0 and st["records_ok"] == sum(ROUNDS)
    with _ctx(fa) as agg:
        _round(fa, po, agg, po.Rollup(300), 0, ROUNDS[0])
        assert agg.stats()["records_bad"] == 0
