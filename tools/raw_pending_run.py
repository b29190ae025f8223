#!/usr/bin/env python3
"""What a query or a select over the PENDING flows_raw parts of a live ctx costs (fa_raw_query_pending, fa_raw_select_pending;
include/flowagg.h "the pending flows_raw parts as input"), on tools/raw_query_run.py's stream: framed FlowMessages, Zipf-1.1
addresses over 2^24, generated in HBM, 2^23 records over 900 s of ONE Date.  One child process under a time limit - one box, one
session:
  * variant "chunks": a ctx with fa_raw_enable that ingested the stream - its pending parts are those of the chunks; variant
    "merged": the same after fa_raw_merge (one part).  The ctx lives through the run, as an ingesting ctx does.
  * the five panels (SRC_ADDR | DST_ADDR | SRC_PORT | DST_PORT | MINUTE, the first 100 rows of each by weight) in one
    fa_raw_query_pending, over 1/8 of the time axis, over the last 1/64 and over the whole axis; and fa_raw_select_pending with the
    DstPort condition of tools/raw_select_run.py (about 1 % of the rows) over the 1/8; wall clock around the call and its reads /
    its fetch; three interleaved rounds, who goes first rotating; medians;
  * beside it, in the same round, today's route on a TWIN ctx that ingested the same stream: fa_raw_take_lz4 + fa_raw_query of the
    frames, and fa_raw_take + fa_raw_query of the plain bytes (a take empties the twin: every round a fresh twin ingests again,
    outside the clock; the take is timed once per round, every case's query of the taken bytes after it; the querying ctx lives
    through the run as the live ctx does);
  * per case the stage times (fa_raw_pending_stats: bounds; fa_raw_query_stats: fold, order - the reads), parts skipped / whole /
    searched;
  * checks_ok: in every round every kind's rows of every route equal, byte for byte, this tool's numpy group-by over
    spill.read_native of the taken plain bytes; the pending select's bytes equal fa_raw_select's over the taken bytes and its
    row count numpy's.
No time is gated.  Writes profiles/raw_pending_run.json."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _pkg  # noqa: E402
import numpy as np  # noqa: E402
from raw_query_run import K, KIND_NAMES, NO_UPPER, PANELS, in_range, numpy_rows  # noqa: E402


def step(args):
    import torch
    fa = _pkg.load()
    fa.build()
    L = fa.lib()
    dev = torch.device("cuda", 0)
    n, chunk = args.records, args.chunk
    mp = fa.mock_params(mode=fa.MOCK_ZIPF, framed=1, seed=3, n_total=n, span_secs=900, zipf_log2_universe=args.universe_log2, zipf_s_x100=110)
    out, checks = {"records": n, "chunk_records": chunk, "k": K}, {}
    cap = chunk * 96 + 4096
    d_buf = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off = torch.empty(chunk + 1, dtype=torch.int32, device=dev)

    def ingested(merged):
        agg = fa.FlowAgg(framed=True, max_batch_records=chunk, key_sets=1)
        agg.raw_enable(chunk)
        for i0 in range(0, n, chunk):
            m = min(chunk, n - i0)
            w = agg.mock_generate_device(mp, i0, m, d_buf.data_ptr(), cap, d_off.data_ptr())
            agg.ingest_device(d_buf.data_ptr(), w, d_off.data_ptr(), m)
        agg.sync()
        if merged:
            agg.raw_merge()
        return agg

    live = {"chunks": ingested(False), "merged": ingested(True)}
    pend = {v: live[v].raw_stats() for v in live}
    nbytes = max(int(p["pending_bytes"]) for p in pend.values())
    maxparts = max(int(p["pending_parts"]) for p in pend.values())
    out.update(part_bytes=nbytes, pending_parts={v: int(p["pending_parts"]) for v, p in pend.items()})
    h_plain = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True).numpy()
    h_frames = torch.empty(L.fa_lz4_frame_bound(nbytes) + 15 * maxparts, dtype=torch.uint8, pin_memory=True).numpy()
    parts = np.zeros(maxparts, dtype=fa.RAW_PART_DTYPE)
    nb, npart = C.c_size_t(), C.c_size_t()

    def take(agg, lz4):
        """-> (seconds, the taken bytes: a view of the page-locked buffer)"""
        buf = h_frames if lz4 else h_plain
        agg.sync()
        t0 = time.perf_counter()
        rc = (L.fa_raw_take_lz4 if lz4 else L.fa_raw_take)(agg._h, buf.ctypes.data, buf.size, C.byref(nb), parts.ctypes.data, maxparts, C.byref(npart))
        dt = time.perf_counter() - t0
        assert rc == 0, (rc, L.fa_last_error(agg._h))
        return dt, buf[:nb.value]

    # ---- the rows as spill.read_native delivers a merged twin's plain bytes; the cases and what numpy makes of them
    with ingested(True) as twin:
        _, data = take(twin, False)
        (block,) = fa.spill.read_native(data.tobytes())
    t = block["TimeReceived"]
    rows = len(t)
    assert (np.diff(t.astype(np.int64)) >= 0).all()
    out["rows"] = rows
    lo, hi = int(t[rows // 2 - rows // 16]), int(t[min(rows - 1, rows // 2 + rows // 16)])  # the seconds around the middle that hold 1/8 of the rows
    last = int(t[rows - rows // 64])
    ports, shares = np.unique(block["DstPort"][in_range(t, lo, hi)], return_counts=True)  # (tools/raw_select_run.py's 1 % condition)
    shares = shares / shares.sum()
    q = int(np.searchsorted(np.cumsum(shares), 0.01))
    one = int(np.argmin(np.abs(shares - 0.01)))
    if abs(float(shares[:q + 1].sum()) - 0.01) <= abs(float(shares[one]) - 0.01):
        p_lo, p_hi = int(ports[0]), int(ports[q])
    else:
        p_lo = p_hi = int(ports[one])
    cases = {"1/8 of the axis": dict(t_lo=lo, t_hi=hi), "the last 1/64": dict(t_lo=last, t_hi=NO_UPPER), "the whole axis": dict(t_lo=0, t_hi=NO_UPPER)}
    sel_f = dict(t_lo=lo, t_hi=hi, dst_port=(p_lo, p_hi))
    want, info = {}, {}
    for name, f in cases.items():
        mask = in_range(t, f["t_lo"], f["t_hi"])
        want[name] = {bit: numpy_rows(fa, block, mask, bit, K)[0] for bit in KIND_NAMES}
        info[name] = dict(rows_in_range=int(mask.sum()), filter=f)
    sel_rows = int((in_range(t, lo, hi) & (block["DstPort"] >= p_lo) & (block["DstPort"] <= p_hi)).sum())
    info["select, 1/8 of the axis, 1 % DstPort"] = dict(rows_matched=sel_rows, filter=sel_f)
    del block

    def read_all(agg):
        got, buf, cnt = {}, np.zeros(K, dtype=fa.QUERY_ROW_DTYPE), C.c_size_t()
        for bit in KIND_NAMES:
            rc = L.fa_raw_query_rows(agg._h, bit, fa.RAW_O_WEIGHT, K, buf.ctypes.data, K, C.byref(cnt))
            assert rc == 0, (rc, L.fa_last_error(agg._h))
            got[bit] = buf[:cnt.value].copy()
        return got

    def delta(a, b):
        return {k: b[k] - a[k] for k in b}

    def pending_query(agg, f):
        p0, q0 = agg.raw_pending_stats(), agg.raw_query_stats()
        agg.sync()
        t0 = time.perf_counter()
        agg.raw_query_pending(PANELS, **f)
        got = read_all(agg)
        dt = time.perf_counter() - t0
        return dt, got, dict(pending=delta(p0, agg.raw_pending_stats()), query=delta(q0, agg.raw_query_stats()))

    def file_query(agg, data, f):
        q0, r0 = agg.raw_query_stats(), agg.raw_range_stats()
        agg.sync()
        t0 = time.perf_counter()
        agg.raw_query(data, PANELS, **f)
        got = read_all(agg)
        dt = time.perf_counter() - t0
        return dt, got, dict(query=delta(q0, agg.raw_query_stats()), range=delta(r0, agg.raw_range_stats()))

    sel_out = torch.empty(max(sel_rows, 1) * 128 + 4096, dtype=torch.uint8, pin_memory=True).numpy()

    def pending_select(agg):
        p0, s0 = agg.raw_pending_stats(), agg.raw_select_stats()
        agg.sync()
        t0 = time.perf_counter()
        sel, sparts = agg.raw_select_pending(out=sel_out, **sel_f)
        dt = time.perf_counter() - t0
        return dt, bytes(sel), int(sparts["rows"].sum()), dict(pending=delta(p0, agg.raw_pending_stats()), select=delta(s0, agg.raw_select_stats()))

    def file_select(agg, data):
        agg.sync()
        t0 = time.perf_counter()
        sel, sparts = agg.raw_select(data, out=sel_out, **sel_f)
        dt = time.perf_counter() - t0
        return dt, bytes(sel), int(sparts["rows"].sum())

    SEL = "select, 1/8 of the axis, 1 % DstPort"
    routes = ("pending", "take_lz4 + query", "take + query")
    times = {(v, c, r): [] for v in live for c in list(cases) + [SEL] for r in routes}
    takes = {(v, r): [] for v in live for r in routes[1:]}
    stats = {}
    readers = {(v, r): fa.FlowAgg(framed=True) for v in live for r in routes[1:]}  # today's route: the ctx that reads the taken bytes
    order = [(v, r) for v in live for r in routes]
    for rnd in range(args.rounds):
        for v, route in order[rnd % len(order):] + order[:rnd % len(order)]:  # (who goes first rotates)
            sel_ref = None
            if route == "pending":
                agg = live[v]
                for name, f in cases.items():
                    dt, got, st = pending_query(agg, f)
                    times[v, name, route].append(dt)
                    stats[v, name, route] = st
                    checks["%s / %s / %s / round %d" % (v, name, route, rnd)] = all(got[b].tobytes() == want[name][b].tobytes() for b in KIND_NAMES)
                dt, sel, nrows, st = pending_select(agg)
                times[v, SEL, route].append(dt)
                stats[v, SEL, route] = st
                with fa.FlowAgg(framed=True) as ref, ingested(v == "merged") as twin:  # (outside the clock: the same rows through the file door)
                    sel_ref = file_select(ref, take(twin, False)[1])[1]
                checks["%s / %s / %s / round %d" % (v, SEL, route, rnd)] = nrows == sel_rows and sel == sel_ref
                continue
            lz4 = route.startswith("take_lz4")
            with ingested(v == "merged") as twin:
                dt, data = take(twin, lz4)
            takes[v, route].append(dt)
            agg = readers[v, route]
            for name, f in cases.items():
                dt, got, st = file_query(agg, data, f)
                times[v, name, route].append(dt)
                stats[v, name, route] = st
                checks["%s / %s / %s / round %d" % (v, name, route, rnd)] = all(got[b].tobytes() == want[name][b].tobytes() for b in KIND_NAMES)
            dt, sel, nrows = file_select(agg, data)
            times[v, SEL, route].append(dt)
            checks["%s / %s / %s / round %d" % (v, SEL, route, rnd)] = nrows == sel_rows
    res = {}
    for v in live:
        res[v] = {"take_ms": {r: [x * 1e3 for x in takes[v, r]] for r in routes[1:]}}
        for name in list(cases) + [SEL]:
            c = dict(info[name])
            for route in routes:
                x = times[v, name, route]
                r = dict(ms=[y * 1e3 for y in x], ms_median=statistics.median(x) * 1e3)
                st = stats.get((v, name, route), {})
                if "pending" in st:
                    p = st["pending"]
                    r.update(bounds_ms=p["bounds_ns"] / 1e6, bounds_launches=p["bounds_launches"], parts_skipped=p["parts_skipped"], parts_whole=p["parts_whole"],
                             parts_searched=p["parts_searched"], rows_in_range=p["rows_in_range"])
                if "query" in st:
                    r.update(fold_ms=st["query"]["fold_ns"] / 1e6, reads_ms=st["query"]["order_ns"] / 1e6, rows_scanned=st["query"]["rows_scanned"])
                if "range" in st:
                    r.update(decode_ms=st["range"]["decode_ns"] / 1e6, range_ms=st["range"]["range_ns"] / 1e6)
                if "select" in st:
                    s = st["select"]
                    r.update(select_ms=s["select_ns"] / 1e6, emit_ms=s["emit_ns"] / 1e6, gather_ms=s["gather_ns"] / 1e6)
                if route != "pending":  # today's route is the take and the query of what it took
                    r["ms_with_take"] = [a + b * 1e3 for a, b in zip(r["ms"], takes[v, route])]
                    r["ms_with_take_median"] = statistics.median(r["ms_with_take"])
                c[route] = r
            p = c["pending"]["ms"]
            c["pending_below_todays_route_in_every_round"] = all(p[i] < c[r]["ms_with_take"][i] for r in routes[1:] for i in range(len(p)))
            c["pending_below_the_query_of_taken_bytes_in_every_round"] = all(p[i] < c[r]["ms"][i] for r in routes[1:] for i in range(len(p)))
            res[v][name] = c
    for a in list(live.values()) + list(readers.values()):
        a.close()
    out["variants"] = res
    out["checks"] = {k: bool(x) for k, x in checks.items()}
    out["checks_ok"] = all(out["checks"].values())
    print("PENDING_STEP " + json.dumps(out))
    return 0 if out["checks_ok"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="records per fa_ingest_device call and per raw chunk")
    ap.add_argument("--universe-log2", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds")
    ap.add_argument("--step-timeout", type=int, default=540, help="seconds for the GPU step")
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_pending_run.json"))
    args = ap.parse_args()
    if args.step:
        sys.exit(step(args))
    res = {"config": "framed FlowMessages, Zipf-1.1 over 2^%d addresses, %d records over 900 s of one Date, generated in HBM; a live ctx per variant, a fresh twin per take; "
                     "one box, one run" % (args.universe_log2, args.records)}
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--records", str(args.records), "--chunk", str(args.chunk), "--universe-log2", str(args.universe_log2),
           "--rounds", str(args.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        print("the GPU step exceeded its %d s limit: stopping" % args.step_timeout, file=sys.stderr)
        sys.exit(124)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("PENDING_STEP ")]
    if not line:
        sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
        print("the GPU step failed (exit status %d): stopping" % p.returncode, file=sys.stderr)
        sys.exit(p.returncode or 1)
    res.update(json.loads(line[-1][len("PENDING_STEP "):]))
    res["source_hash"] = _pkg.load().source_hash()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({v: {c: {r: x[r]["ms_median"] for r in ("pending", "take_lz4 + query", "take + query")} for c, x in cs.items() if c != "take_ms"}
                      for v, cs in res["variants"].items()} | {"checks_ok": res["checks_ok"]}))
    sys.exit(0 if res["checks_ok"] else 1)


if __name__ == "__main__":
    main()
