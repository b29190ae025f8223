#!/usr/bin/env python3
"""What a grouped query over flows_raw parts costs (fa_raw_query + fa_raw_query_rows; include/flowagg.h "grouped queries over
flows_raw parts"), on tools/raw_select_run.py's input: framed FlowMessages, Zipf-1.1 addresses over 2^24, generated in HBM, 2^23
records over 900 s of ONE Date; one ctx with fa_raw_enable ingests them, merges its parts (one sorted part) and delivers it as one
LZ4 frame into page-locked memory.  One child process under a time limit - one box, one session:
  * the five panels of the dashboard (SRC_ADDR | DST_ADDR | SRC_PORT | DST_PORT | MINUTE, the first 100 rows of each by weight) in
    ONE query and as FIVE single-kind queries, over 1/8 of the time axis with no condition, over 1/8 with a DstPort condition that
    selects about 1 % of the rows, and over the whole axis; each variant in a fresh ctx (it pays the allocation of its buffers),
    wall clock around the query calls and their reads; three interleaved rounds, who goes first rotating; medians;
  * beside them the route a user had before: with no condition fa_raw_restore_range into a fresh ctx with bucketed talkers and
    ports and its four ranged reads; with the filter fa_raw_select + fa_raw_columns_device of the selection + the fold doors of a
    scratch ctx + its four reads (neither route has a minute series without the wide table: four panels against five);
  * per variant the stage times (fa_raw_range_stats: probe, range, decode; fa_raw_query_stats: fold, order), the fold's ns per
    scanned row and per update, the share of updates the LDS caches absorbed, growths;
  * checks_ok: in every round every kind's rows equal, byte for byte, this tool's numpy group-by over spill.read_native of the input
    (decoded by the HOST decoder), and the four kinds the older route has equal its rows.
No time is gated.  Writes profiles/raw_query_run.json."""
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
import _pkg  # noqa: E402
import numpy as np  # noqa: E402

NO_UPPER = 0xFFFFFFFF
K = 100
KIND_NAMES = {1: "SRC_ADDR", 2: "DST_ADDR", 4: "SRC_PORT", 8: "DST_PORT", 16: "MINUTE"}
PANELS = 31


def in_range(t, lo, hi):
    return (t >= lo) & ((t < hi) | (hi == NO_UPPER))


def group_by(cols, w):
    """cols: uint64 key columns, most significant first; w: uint64 weights -> (the distinct keys' columns ascending, weight, count)"""
    if not len(w):
        return [c[:0] for c in cols], w[:0], np.zeros(0, dtype=np.uint64)
    order = np.lexsort(cols[::-1])
    s = [c[order] for c in cols]
    new = np.zeros(len(w), dtype=bool)
    new[0] = True
    for c in s:
        new[1:] |= c[1:] != c[:-1]
    starts = np.nonzero(new)[0]
    with np.errstate(over="ignore"):
        weight = np.add.reduceat(w[order], starts)
    count = np.diff(np.append(starts, len(w))).astype(np.uint64)
    return [c[starts] for c in s], weight, count


def numpy_rows(fa, b, mask, group, k):
    """a block of spill.read_native, the matching rows' mask, one kind -> its first k fa_query_rows by weight (this tool's own
    statement of the grouping rule, the minute and the order)"""
    with np.errstate(over="ignore"):
        w = b["Bytes"][mask].astype(np.uint64) * b["SamplingRate"][mask].astype(np.uint64)
    if group in (1, 2):
        a = np.ascontiguousarray(b["SrcAddr" if group == 1 else "DstAddr"][mask]).copy()
        v4 = b["EType"][mask] == 0x800
        a[v4, 4:] = 0
        cols = [a[:, :8].copy().view(">u8").reshape(-1).astype(np.uint64), a[:, 8:].copy().view(">u8").reshape(-1).astype(np.uint64), np.where(v4, 0x800, 0).astype(np.uint64)]
    elif group == 16:
        t = b["TimeFlowStart"][mask].astype(np.uint64) & np.uint64(0xFFFFFFFF)
        cols = [t - t % np.uint64(60)]
    else:
        cols = [b["SrcPort" if group == 4 else "DstPort"][mask].astype(np.uint64)]
    keys, weight, count = group_by(cols, w)
    top = np.argsort(~weight, kind="stable")[:k]  # weight descending, ties in key order
    out = np.zeros(len(top), dtype=fa.QUERY_ROW_DTYPE)
    if group in (1, 2):
        out["key"][:, :8] = keys[0][top].astype(">u8").view(np.uint8).reshape(-1, 8)
        out["key"][:, 8:] = keys[1][top].astype(">u8").view(np.uint8).reshape(-1, 8)
        out["etype"] = keys[2][top]
    else:
        out["value"] = keys[0][top]
    out["weight"], out["count"] = weight[top], count[top]
    return out, len(weight)


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
    with fa.FlowAgg(framed=True, max_batch_records=chunk, key_sets=1) as src:
        src.raw_enable(chunk)
        for i0 in range(0, n, chunk):
            m = min(chunk, n - i0)
            d_buf = torch.empty(cap, dtype=torch.uint8, device=dev)
            d_off = torch.empty(chunk + 1, dtype=torch.int32, device=dev)
            w = src.mock_generate_device(mp, i0, m, d_buf.data_ptr(), cap, d_off.data_ptr())
            src.ingest_device(d_buf.data_ptr(), w, d_off.data_ptr(), m)
        src.sync()
        src.raw_merge()
        pending = src.raw_stats()
        nbytes, nparts = int(pending["pending_bytes"]), int(pending["pending_parts"])
        assert nparts == 1, "the stream lies in one Date: one merged part"
        h_frames = torch.empty(L.fa_lz4_frame_bound(nbytes) + 15 * nparts, dtype=torch.uint8, pin_memory=True).numpy()
        parts = np.zeros(nparts, dtype=fa.RAW_PART_DTYPE)
        nb, npart = C.c_size_t(), C.c_size_t()
        rc = L.fa_raw_take_lz4(src._h, h_frames.ctypes.data, h_frames.size, C.byref(nb), parts.ctypes.data, nparts, C.byref(npart))
        assert rc == 0 and npart.value == nparts, rc
        frames = h_frames[:nb.value]
        rows = int(parts["rows"].sum())
    out.update(rows=rows, lz4_bytes=int(nb.value), part_bytes=nbytes)

    # ---- the input as the HOST decoder and spill.read_native deliver it; the cases and what numpy makes of them
    (block,) = fa.spill.read_native(fa.lz4_decode(frames.tobytes()))
    t = block["TimeReceived"]
    assert len(t) == rows and (np.diff(t.astype(np.int64)) >= 0).all()
    lo, hi = int(t[rows // 2 - rows // 16]), int(t[min(rows - 1, rows // 2 + rows // 16)])  # the seconds around the middle that hold 1/8 of the rows
    in_slice = in_range(t, lo, hi)
    ports, shares = np.unique(block["DstPort"][in_slice], return_counts=True)  # (tools/raw_select_run.py's 1 % condition)
    shares = shares / shares.sum()
    q = int(np.searchsorted(np.cumsum(shares), 0.01))
    one = int(np.argmin(np.abs(shares - 0.01)))
    if abs(float(shares[:q + 1].sum()) - 0.01) <= abs(float(shares[one]) - 0.01):
        p_lo, p_hi = int(ports[0]), int(ports[q])
    else:
        p_lo = p_hi = int(ports[one])
    cases = {
        "1/8 of the axis, no condition": dict(t_lo=lo, t_hi=hi),
        "1/8 of the axis, 1 % DstPort": dict(t_lo=lo, t_hi=hi, dst_port=(p_lo, p_hi)),
        "the whole axis, no condition": dict(t_lo=0, t_hi=NO_UPPER),
    }
    want, info = {}, {}
    for name, f in cases.items():
        mask = in_range(t, f["t_lo"], f["t_hi"])
        scanned = int(mask.sum())
        if "dst_port" in f:
            mask &= (block["DstPort"] >= p_lo) & (block["DstPort"] <= p_hi)
        want[name], groups = {}, {}
        for bit, kind in KIND_NAMES.items():
            want[name][bit], groups[kind] = numpy_rows(fa, block, mask, bit, K)
        info[name] = dict(rows_scanned=scanned, rows_matched=int(mask.sum()), groups=groups, filter=f)
    del block

    def read_all(agg, kinds, got):
        buf = np.zeros(K, dtype=fa.QUERY_ROW_DTYPE)
        cnt = C.c_size_t()
        for bit in kinds:
            rc = L.fa_raw_query_rows(agg._h, bit, fa.RAW_O_WEIGHT, K, buf.ctypes.data, K, C.byref(cnt))
            assert rc == 0, (rc, L.fa_last_error(agg._h))
            got[bit] = buf[:cnt.value].copy()

    def one_query(f):
        got = {}
        with fa.FlowAgg(framed=True) as agg:
            agg.sync()
            t0 = time.perf_counter()
            agg.raw_query(frames, PANELS, **f)
            read_all(agg, KIND_NAMES, got)
            dt = time.perf_counter() - t0
            return dt, got, dict(query=agg.raw_query_stats(), range=agg.raw_range_stats())

    def five_queries(f):
        got = {}
        with fa.FlowAgg(framed=True) as agg:
            agg.sync()
            t0 = time.perf_counter()
            for bit in KIND_NAMES:
                agg.raw_query(frames, bit, **f)
                read_all(agg, (bit,), got)
            dt = time.perf_counter() - t0
            return dt, got, dict(query=agg.raw_query_stats(), range=agg.raw_range_stats())

    def as_query_rows(talkers=None, ports=None):
        src = talkers if talkers is not None else ports
        o = np.zeros(len(src), dtype=fa.QUERY_ROW_DTYPE)
        if talkers is not None:
            o["key"], o["etype"] = talkers["key"], talkers["etype"]
        else:
            o["value"] = ports["port"]
        o["weight"], o["count"] = src["weight"], src["count"]
        return o

    def four_reads(agg, ranged):
        talk = (lambda d: agg.top_talkers(d, K, 0, NO_UPPER)) if ranged else (lambda d: agg.top_talkers(d, K))
        return {1: as_query_rows(talkers=talk(0)), 2: as_query_rows(talkers=talk(1)), 4: as_query_rows(ports=agg.top_ports_range(0, K, 0, NO_UPPER)),
                8: as_query_rows(ports=agg.top_ports_range(1, K, 0, NO_UPPER))}

    def restore_route(f):
        """fa_raw_restore_range into a fresh ctx with bucketed talkers and ports, its four ranged reads"""
        with fa.FlowAgg(framed=True) as agg:
            agg.talkers_enable(0, bucket_secs=60)
            agg.ports_enable_buckets(0, bucket_secs=60)
            agg.sync()
            t0 = time.perf_counter()
            agg.raw_restore_range(frames, f["t_lo"], f["t_hi"], 0, True)
            got = four_reads(agg, True)
            dt = time.perf_counter() - t0
            return dt, got, dict(range=agg.raw_range_stats(), load=agg.raw_load_stats())

    def select_route(f):
        """fa_raw_select + fa_raw_columns_device of the selection + the fold doors of a scratch ctx + its reads"""
        with fa.FlowAgg(framed=True) as agg, fa.FlowAgg(framed=True) as scratch:
            scratch.talkers_enable(0)
            scratch.ports_enable_buckets(0, bucket_secs=60)
            agg.sync()
            t0 = time.perf_counter()
            sel, _ = agg.raw_select(frames, **f)
            cols, nrows = agg.raw_columns(sel)
            if nrows:
                scratch.fold_columns_device(cols, nrows)
                scratch.ports_fold_columns_device(cols, nrows)
            got = four_reads(scratch, False)
            dt = time.perf_counter() - t0
            return dt, got, dict(range=agg.raw_range_stats(), select=agg.raw_select_stats())

    variants = {}
    for name, f in cases.items():
        variants[name, "one query"] = lambda f=f: one_query(f)
        variants[name, "five queries"] = lambda f=f: five_queries(f)
        variants[name, "the route before"] = (lambda f=f: select_route(f)) if "dst_port" in f else (lambda f=f: restore_route(f))
    order = list(variants)
    times, stats = {k: [] for k in order}, {}
    for rnd in range(args.rounds):
        for which in order[rnd % len(order):] + order[:rnd % len(order)]:  # (who goes first rotates)
            dt, got, st = variants[which]()
            times[which].append(dt)
            stats[which] = st
            ok = all(got[bit].tobytes() == want[which[0]][bit].tobytes() for bit in got) and len(got) == (4 if which[1] == "the route before" else 5)
            checks["%s / %s / round %d" % (which[0], which[1], rnd)] = ok
    res = {}
    for name in cases:
        res[name] = dict(info[name])
        for which in order:
            if which[0] != name:
                continue
            v = times[which]
            r = dict(ms=[x * 1e3 for x in v], ms_median=statistics.median(v) * 1e3, ms_min=min(v) * 1e3)
            g = stats[which]["range"]
            r.update(blocks_seen=g["blocks_seen"], blocks_decoded=g["blocks_decoded"], probe_ms=g["probe_ns"] / 1e6, range_ms=g["range_ns"] / 1e6, decode_ms=g["decode_ns"] / 1e6)
            if "query" in stats[which]:
                s = stats[which]["query"]
                r.update(calls=s["calls"], fold_ms=s["fold_ns"] / 1e6, order_ms=s["order_ns"] / 1e6, launches=s["launches"], grows=s["grows"], updates=s["updates"],
                         absorbed_share=s["absorbed"] / s["updates"] if s["updates"] else None, fold_ns_per_scanned_row=s["fold_ns"] / max(s["rows_scanned"], 1),
                         fold_ns_per_update=s["fold_ns"] / s["updates"] if s["updates"] else None)
            res[name][which[1]] = r
        res[name]["one_query_faster_than_five"] = res[name]["one query"]["ms_median"] < res[name]["five queries"]["ms_median"]
        res[name]["one_query_faster_than_the_route_before"] = res[name]["one query"]["ms_median"] < res[name]["the route before"]["ms_median"]
    out["cases"] = res
    out["wave_pre_sum"] = "not built"
    out["checks"] = {k: bool(v) for k, v in checks.items()}
    out["checks_ok"] = all(out["checks"].values())
    print("QUERY_STEP " + json.dumps(out))
    return 0 if out["checks_ok"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="records per fa_ingest_device call and per raw chunk")
    ap.add_argument("--universe-log2", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds")
    ap.add_argument("--step-timeout", type=int, default=540, help="seconds for the GPU step")
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_query_run.json"))
    args = ap.parse_args()
    if args.step:
        sys.exit(step(args))
    res = {"config": "framed FlowMessages, Zipf-1.1 over 2^%d addresses, %d records over 900 s of one Date, generated in HBM, one merged LZ4 part; fresh ctx per variant; "
                     "one box, one run" % (args.universe_log2, args.records)}
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--records", str(args.records), "--chunk", str(args.chunk), "--universe-log2", str(args.universe_log2),
           "--rounds", str(args.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        print("the GPU step exceeded its %d s limit: stopping" % args.step_timeout, file=sys.stderr)
        sys.exit(124)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("QUERY_STEP ")]
    if not line:
        sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
        print("the GPU step failed (exit status %d): stopping" % p.returncode, file=sys.stderr)
        sys.exit(p.returncode or 1)
    res.update(json.loads(line[-1][len("QUERY_STEP "):]))
    res["source_hash"] = _pkg.load().source_hash()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {v: c[v]["ms_median"] for v in ("one query", "five queries", "the route before")} for k, c in res["cases"].items()} | {"checks_ok": res["checks_ok"]}))
    sys.exit(0 if res["checks_ok"] else 1)


if __name__ == "__main__":
    main()
