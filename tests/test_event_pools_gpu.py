"""GPU tests of the bounded event pools behind the load doors (csrc/events.h; the limits: LOAD_EV_MAX in raw_load_host.inc,
ROLLUP_EV_MAX in rollup_host.inc, SKETCH_EV_MAX in sketch_fold_host.inc, the keyed tables' 1024 pairs in keytab_host.inc).

Every pool whose limit is reached waits for the stream, reads its pending times and starts over.  FA_TALK_CHUNK = 8 makes 8 rows
the chunk of every load door (table_room_chunk_cap), so one part of a few thousand rows crosses every limit in one call.  Expected
reads are those of a second ctx that restored the same part with the default chunk: one chunk, no pool near its limit."""
import numpy as np
import pytest

import raw_load_cases as R
from test_sketch_fold_gpu import _all_reads, _full_ctx

pytestmark = pytest.mark.gpu

CHUNK = 8


def _part(seed, n):
    return R.native_part(R.random_rows(seed, n, keys=60))


def test_restore_crosses_every_pool_limit(gpu_lib, fa, monkeypatch):
    n = 9001  # 1 126 chunks, the last of one row: above 256 chunks, 256 rollup and sketch launches, 1 024 talker and port launches
    chunks = (n + CHUNK - 1) // CHUNK
    assert chunks > 1024
    part = _part(101, n)
    monkeypatch.delenv("FA_TALK_CHUNK", raising=False)
    with _full_ctx(fa) as ref:
        ref.raw_restore(part, 0, folds=True)
        want = _all_reads(ref)
        assert ref.rollup_stats()["launches"] == ref.sketch_fold_stats()["launches"] == ref.talkers_stats()["fold_launches"] == 1
    monkeypatch.setenv("FA_TALK_CHUNK", str(CHUNK))  # (read by the enables)
    with _full_ctx(fa) as a:
        a.raw_restore(part, 0, folds=True)
        got = _all_reads(a)
        assert got.keys() == want.keys()
        for k in got:
            assert len(got[k]) > 0 and got[k].tobytes() == want[k].tobytes(), k
        ls, rs, ss, ts, ps = a.raw_load_stats(), a.rollup_stats(), a.sketch_fold_stats(), a.talkers_stats(), a.ports_stats()
        print("load", ls, "rollup", rs, "sketch", ss, "talkers", ts, "ports", ps)
        assert ls["calls"] == 1 and ls["parts"] == 1 and ls["rows_loaded"] == n
        assert rs["launches"] == ss["launches"] == ss["batches"] == ts["fold_launches"] == ps["fold_launches"] == chunks
        assert rs["records_in"] == ss["records_in"] == ts["records_folded"] == ps["records_folded"] == n
        assert rs["records_bad"] == ss["records_bad"] == 0 and rs["calls"] == ss["calls"] == 1
        assert ls["unpack_ns"] > 0 and ls["fold_ns"] > 0 and rs["fold_ns"] > 0 and ss["fold_ns"] > 0
        assert ts["fold_ns_total"] > 0 and ps["fold_ns_total"] > 0


def test_load_crosses_the_chunk_limit(gpu_lib, fa, monkeypatch):
    n = 2101  # 263 chunks: above LOAD_EV_MAX's 256
    chunks = (n + CHUNK - 1) // CHUNK
    assert chunks > 256
    part = _part(102, n)
    reads = lambda agg: {(w, d): f(d, 0, 0, 0xFFFFFFFF) for w, f in (("talkers", agg.top_talkers), ("ports", agg.top_ports_range)) for d in (0, 1)}
    monkeypatch.delenv("FA_TALK_CHUNK", raising=False)
    with _full_ctx(fa) as ref:
        ref.raw_load(part)
        want = reads(ref)
    monkeypatch.setenv("FA_TALK_CHUNK", str(CHUNK))
    with _full_ctx(fa) as a:
        a.raw_load(part)
        got = reads(a)
        for k in got:
            assert len(got[k]) > 0 and got[k].tobytes() == want[k].tobytes(), k
        ls, ts, ps = a.raw_load_stats(), a.talkers_stats(), a.ports_stats()
        print("load", ls, "talkers", ts, "ports", ps)
        assert ls["calls"] == 1 and ls["rows_loaded"] == n and ls["launches"] == 1 + chunks  # the header check, one unpack per chunk
        assert ts["fold_launches"] == ps["fold_launches"] == chunks and ts["records_folded"] == ps["records_folded"] == n
        assert ls["unpack_ns"] > 0 and ls["fold_ns"] > 0 and ts["fold_ns_total"] > 0 and ps["fold_ns_total"] > 0
        assert a.rollup_stats()["calls"] == a.sketch_fold_stats()["calls"] == 0 and len(a.read_window()) == 0  # this door feeds the folds alone
