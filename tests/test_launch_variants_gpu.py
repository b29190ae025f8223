"""Every arm of the ingest launch dispatch (ingest_host.inc: the LaunchPlan of a launch, launch_plan.h: ks_variant /
with_variant), one small launch each: which kernel family ran is read from the three launch counters of fa_stats, what it
computed is compared bit for bit with the CPU oracle.

A characterisation test: it was written against the sources BEFORE the dispatch was rewritten, passed there unchanged, and
pins what the rewrite must keep.  Every case is one ctx and one fa_ingest_device call of 4096 records (64 wave tiles: several
workgroups, every sink), mocker records for flows_5m alone and Zipf addresses for every other mask.  Nothing about the
expectations had to be corrected after the run on the earlier sources.
"""
import numpy as np
import pytest

from device_columns import fetch_columns
from test_record_lengths_gpu import APP_COLS, CMS, _assert_decoded, _reference, _same, _upload
from test_topk_gpu import _ranked

pytestmark = pytest.mark.gpu

N = 4096
MASKS = (1, 2, 3, 4, 5, 6, 7, 9, 63)
ENV = ("FA_SINK", "FA_TUPLE", "FA_SEQ", "FA_WIDE", "FA_CMS")
TOPK = dict(topk_capacity_log2=12, topk_track=64)


class _Stream:
    """n generator records, uploaded once; the oracle's answers per key-set mask, computed once and never changed."""

    def __init__(self, po, kind, n):
        gp = po.gen_params(mode=po.GEN_MOCKER if kind == "mocker" else po.GEN_ZIPF, framed=1, seed=77, n_total=n, span_secs=600)
        self.buf, self.off = po.gen_records(gp, 0, n)
        self.n, self.po, self.refs, self.dev = n, po, {}, None

    def ref(self, ks):
        if ks not in self.refs:
            self.refs[ks] = _reference(self.po, self.buf, self.off, ks)
        return self.refs[ks]

    def device(self):
        if self.dev is None:
            self.dev = _upload(self.buf, self.off)
        return self.dev


@pytest.fixture(scope="module")
def streams(po):
    made = {}

    def get(ks, n=N):
        key = ("mocker" if ks == 1 else "zipf", n)
        if key not in made:
            made[key] = _Stream(po, *key)
        return made[key]
    return get


def _env(monkeypatch, **kw):
    for k in ENV:
        monkeypatch.setenv(k, kw[k]) if kw.get(k) else monkeypatch.delenv(k, raising=False)


def _assert_reads(fa, agg, ks, ref):
    """Every read the mask enables == the oracle's."""
    if ks & 1:
        assert agg.read_window().tobytes() == ref["rollup"].tobytes()
    if ks & 2:
        assert np.array_equal(agg.cms_read(fa.FA_KEYS_SRCADDR_CMS).reshape(-1), ref["cms_src"])
    if ks & 4:
        assert np.array_equal(agg.cms_read(fa.FA_KEYS_DSTADDR_CMS).reshape(-1), ref["cms_dst"])
    if ks & 8:
        _same(agg.read_window_app(), ref["app"], APP_COLS)
    if ks & 16:
        for d in (0, 1):
            _same(agg.top_ports(d), ref["ports"][d], ("port", "weight", "count"))
    if ks & 32:
        _same(agg.minute_series(), ref["minutes"], ("minute", "weight", "count"))


def _launch(fa, s, ks, counters, after=None, **cfg):
    """One ctx, one fa_ingest_device of the whole stream, fa_stats, the reads, the launch counters."""
    d_buf, d_off = s.device()
    with fa.FlowAgg(framed=True, key_sets=ks, max_batch_records=s.n, **CMS, **cfg) as agg:
        agg.ingest_device(d_buf.data_ptr(), len(s.buf), d_off.data_ptr(), s.n)
        st = agg.stats()
        assert st["records_ok"] == s.n and st["records_bad"] == 0, (st["records_ok"], st["records_bad"])
        _assert_reads(fa, agg, ks, s.ref(ks))
        got = (st["wave_tile_launches"], st["compact_tuple_launches"], st["learnt_order_launches"])
        assert got == counters, (got, counters)
        if after:
            after(agg, st)
    return st


@pytest.mark.parametrize("fmt", ["8", "16"])
@pytest.mark.parametrize("sink", ["scatter", "direct"])
@pytest.mark.parametrize("ks", MASKS)
def test_every_variant_through_both_sinks_and_tuple_formats(gpu_lib, fa, streams, monkeypatch, ks, sink, fmt):
    """The wave-tile kernel runs iff the scatter sink is asked for AND the mask has the flows_5m rollup (masks 2, 4 and 6 have
    no tuples to scatter: the workgroup-tile kernel whatever FA_SINK says); compact tuples iff that and FA_TUPLE=8."""
    _env(monkeypatch, FA_SINK=sink, FA_TUPLE=fmt)
    wave = int(sink == "scatter" and (ks & 1) != 0)
    _launch(fa, streams(ks), ks, (wave, int(wave and fmt == "8"), 0))


@pytest.mark.parametrize("ks", [3, 5, 7])
def test_sketch_variants_in_the_candidates_mode(gpu_lib, fa, po, streams, monkeypatch, ks):
    """topk_mode = FA_TOPK_CANDIDATES: the kernels compiled for that contract, the aggregation on the side stream.  fa_topk ==
    the restatement of the contract (oracle/pyoracle.py topk_candidates) with this launch as its only batch."""
    _env(monkeypatch, FA_SINK="scatter")
    s = streams(ks)
    rows = s.ref(ks)["rows"]
    with np.errstate(over="ignore"):
        w = rows["bytes"] * rows["sampling_rate"]

    def topk(agg, st):
        for col, key_set in (("src_addr", fa.FA_KEYS_SRCADDR_CMS), ("dst_addr", fa.FA_KEYS_DSTADDR_CMS)):
            if ks & key_set:
                _, cand, est, _ = po.topk_candidates([(rows[col], w)], CMS["cms_depth"], CMS["cms_width_log2"], CMS["cms_seed"],
                                                     track=TOPK["topk_track"], capacity_log2=TOPK["topk_capacity_log2"])
                got = agg.topk(key_set, 1 << 20)
                assert [(bytes(r["key"]), int(r["weight"])) for r in got] == [(k, -e) for e, k in _ranked(cand, est)], col
    _launch(fa, s, ks, (1, 1, 0), after=topk, topk_mode=fa.TOPK_CANDIDATES, **TOPK)


@pytest.mark.parametrize("fmt", ["8", "16"])
def test_learnt_order_variant_forced(gpu_lib, fa, streams, monkeypatch, fmt):
    _env(monkeypatch, FA_SINK="scatter", FA_TUPLE=fmt, FA_SEQ="1")
    _launch(fa, streams(1), 1, (1, int(fmt == "8"), 1))


@pytest.mark.parametrize("wide", ["atomic", "scatter", "log"])
def test_wide_sink_modes(gpu_lib, fa, streams, monkeypatch, wide):
    """flows_5m + (SrcAddr,DstPort,Proto): wide-table updates through atomics, through the scatter sink's fold, and kept as a
    log chunk - the window read (table rows and chunk tuples) equals the oracle in all three."""
    _env(monkeypatch, FA_SINK="scatter", FA_WIDE=wide)
    st = _launch(fa, streams(9), 9, (1, 1, 0))
    assert st["wide_log_recorded"] == (1 if wide == "log" else 0), st["wide_log_recorded"]


@pytest.mark.parametrize("n,wave", [(32767, 0), (32768, 1)])
def test_auto_threshold_between_the_sinks(gpu_lib, fa, streams, monkeypatch, n, wave):
    """No FA_SINK: batches below 2^15 records go straight to the device-wide table, from 2^15 on through the scatter sink."""
    _env(monkeypatch)
    _launch(fa, streams(1, n), 1, (wave, wave, 0))


def test_decode_right_after_a_scatter_ingest(gpu_lib, fa, streams, monkeypatch):
    """fa_decode_device on a ctx whose last launch was a wave-tile one (the decode launch once read that launch's flags out
    of the ctx): the columns are the oracle's, no counter of the ingest moves, the rollup is untouched."""
    _env(monkeypatch, FA_SINK="scatter")
    s = streams(1)
    ref, m = s.ref(1), 300

    def decode(agg, st):
        d_buf, d_off = s.device()
        cols = agg.decode_device(d_buf.data_ptr(), len(s.buf), d_off.data_ptr(), m)
        agg.sync()
        _assert_decoded(fetch_columns(cols, m), ref["rows"][:m], ref["status"][:m])
        after = agg.stats()
        for k in ("wave_tile_launches", "compact_tuple_launches", "learnt_order_launches", "records_ok"):
            assert after[k] == st[k], k
        assert agg.read_window().tobytes() == ref["rollup"].tobytes()
    _launch(fa, s, 1, (1, 1, 0), after=decode)
