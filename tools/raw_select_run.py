#!/usr/bin/env python3
"""What selecting rows of flows_raw parts costs (fa_raw_select + fa_raw_selection_fetch; include/flowagg.h "selecting rows of
flows_raw parts"), on tools/raw_range_run.py's stream: framed FlowMessages, Zipf-1.1 addresses over 2^24, generated in HBM, 2^23
records over 900 s of ONE Date; one ctx with fa_raw_enable ingests them, merges its parts (one sorted part) and delivers it as one
LZ4 frame into page-locked memory.  One child process under a time limit - one box, one session:
  * ONE time range that holds 1/8 of the rows with each of: no condition; one DstPort condition that selects about 1 % of the rows;
    the stream's heaviest SrcAddr with EITHER; a /64 prefix; a filter that matches nothing; COUNT_ONLY (of the 1 % filter); then the
    whole time axis with the 1 % filter.  Each call into a fresh ctx (it pays the allocation of its buffers), select + fetch into
    page-locked memory, wall clock around the two calls; three interleaved rounds, who goes first rotating; medians;
  * per case: the stage times (fa_raw_range_stats: probe, range, decode; fa_raw_select_stats: select, emit, gather), raw_select_kernel's
    ns per scanned row (its hipEvent pair also holds the scan and the totals kernel) beside the bytes the filter makes it read per
    row, emit and gather ns per output row, blocks decoded;
  * checks_ok: in every round every selection equals, byte for byte, this tool's numpy filter over spill.read_native of the input
    (decoded by the HOST decoder), re-encoded by spill.native_from_rows;
  * required: the 1 % filter over 1/8 of the time axis has its median below the FASTEST round of the route a user has today -
    fa_raw_columns_device of the file, the download of the eight columns the filter and README.md:144's projection need (TimeReceived,
    TimeFlowStart, SrcAddr, DstAddr, EType, DstPort, Bytes, Packets) into page-locked memory, the numpy filter.  Everything else is
    recorded, not gated.
Writes profiles/raw_select_run.json."""
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
ROUTE_COLUMNS = dict(time_received=8, time_flow_start=8, src_addr=16, dst_addr=16, etype=4, dst_port=4, bytes=8, packets=8)
FIELDS = {"SequenceNum": "sequence_num", "SamplingRate": "sampling_rate", "SamplerAddress": "sampler_address", "SrcAddr": "src_addr", "DstAddr": "dst_addr", "SrcAS": "src_as",
          "DstAS": "dst_as", "EType": "etype", "Proto": "proto", "SrcPort": "src_port", "DstPort": "dst_port", "Bytes": "bytes", "Packets": "packets",
          "TimeReceived": "time_received", "TimeFlowStart": "time_flow_start"}
WIDTH = {"flow_start": 4, "src_as": 4, "dst_as": 4, "etype": 4, "proto": 4, "src_port": 4, "dst_port": 4, "src_net": 16, "dst_net": 16}
OTHER = {"src_as": "dst_as", "dst_as": "src_as", "src_port": "dst_port", "dst_port": "src_port", "src_net": "dst_net", "dst_net": "src_net"}


def in_range(t, lo, hi):
    return (t >= lo) & ((t < hi) | (hi == NO_UPPER))


def prefix_eq(addr, net):
    want, plen = net
    full, rest = divmod(plen, 8)
    ref = np.frombuffer(bytes(want), dtype=np.uint8)
    ok = (addr[:, :full] == ref[:full]).all(axis=1)
    if rest:
        ok &= (addr[:, full] >> (8 - rest)) == (ref[full] >> (8 - rest))
    return ok


def numpy_filter(b, f):
    """a block of spill.read_native, raw_select's keywords -> the mask of matching rows (this tool's own statement of the filter)"""
    ok = in_range(b["TimeReceived"], f.get("t_lo", 0), f.get("t_hi", NO_UPPER))
    for key, col in (("etype", "EType"), ("proto", "Proto")):
        if key in f:
            ok &= b[col] == f[key]
    if "flow_start" in f:
        ok &= in_range(b["TimeFlowStart"], *f["flow_start"])

    def way(s, d):
        w = np.ones(len(ok), dtype=bool)
        for side, who in (("src", s), ("dst", d)):
            if side + "_as" in f:
                w &= b[who + "AS"] == f[side + "_as"]
            if side + "_port" in f:
                w &= (b[who + "Port"] >= f[side + "_port"][0]) & (b[who + "Port"] <= f[side + "_port"][1])
            if side + "_net" in f:
                w &= prefix_eq(b[who + "Addr"], f[side + "_net"])
        return w
    return ok & (way("Src", "Dst") | way("Dst", "Src") if f.get("either") else way("Src", "Dst"))


def bytes_read_per_row(f):
    """the bytes raw_select_kernel must read per row: the columns the filter names, both sides of a pair under EITHER"""
    keys = {k for k in f if k in WIDTH}
    if f.get("either"):
        keys |= {OTHER[k] for k in keys if k in OTHER}
    return sum(WIDTH[k] for k in keys)


def step(args):
    import torch
    fa = _pkg.load()
    fa.build()
    L = fa.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    dev = torch.device("cuda", 0)
    n, chunk = args.records, args.chunk
    mp = fa.mock_params(mode=fa.MOCK_ZIPF, framed=1, seed=3, n_total=n, span_secs=900, zipf_log2_universe=args.universe_log2, zipf_s_x100=110)
    out, checks = {"records": n, "chunk_records": chunk}, {}
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

    # ---- the input as the HOST decoder and spill.read_native deliver it; the filters
    (block,) = fa.spill.read_native(fa.lz4_decode(frames.tobytes()))
    t = block["TimeReceived"]
    assert len(t) == rows and (np.diff(t.astype(np.int64)) >= 0).all()
    lo, hi = int(t[rows // 2 - rows // 16]), int(t[min(rows - 1, rows // 2 + rows // 16)])  # the seconds around the middle that hold 1/8 of the rows
    in_slice = in_range(t, lo, hi)
    # one DstPort condition that selects about 1 % of the slice: the lowest ports up to the 1 % quantile, or - where few ports carry
    # the stream and that range holds far more - the single port whose share is nearest to 1 %
    ports, shares = np.unique(block["DstPort"][in_slice], return_counts=True)
    shares = shares / shares.sum()
    q = int(np.searchsorted(np.cumsum(shares), 0.01))
    one = int(np.argmin(np.abs(shares - 0.01)))
    if abs(float(shares[:q + 1].sum()) - 0.01) <= abs(float(shares[one]) - 0.01):
        p_lo, p_hi = int(ports[0]), int(ports[q])
    else:
        p_lo = p_hi = int(ports[one])
    keys, counts = np.unique(np.ascontiguousarray(block["SrcAddr"][in_slice]).view([("hi", "<u8"), ("lo", "<u8")]).ravel(), return_counts=True)
    heavy = keys[np.argmax(counts)].tobytes()
    one_pct = dict(dst_port=(p_lo, p_hi))
    cases = {
        "time range only": dict(t_lo=lo, t_hi=hi),
        "1 % DstPort": dict(t_lo=lo, t_hi=hi, **one_pct),
        "heaviest SrcAddr, EITHER": dict(t_lo=lo, t_hi=hi, src_net=(heavy, 128), either=True),
        "a /64 prefix": dict(t_lo=lo, t_hi=hi, src_net=(heavy, 64)),
        "nothing matches": dict(t_lo=lo, t_hi=hi, proto=0xFFFFFFFF, src_as=0xFFFFFFFF),
        "COUNT_ONLY": dict(t_lo=lo, t_hi=hi, count_only=True, **one_pct),
        "whole axis, 1 % DstPort": dict(t_lo=0, t_hi=NO_UPPER, **one_pct),
    }
    want, info = {}, {}
    for name, f in cases.items():
        mask = numpy_filter(block, f)
        sel = np.zeros(int(mask.sum()), dtype=fa.FLOW_ROW_DTYPE)
        for col, field in FIELDS.items():
            sel[field] = block[col][mask]
        want[name] = fa.spill.native_from_rows(sel)
        scanned = int(in_range(t, f["t_lo"], f["t_hi"]).sum())
        info[name] = dict(rows_scanned=scanned, rows_matched=len(sel), fraction_of_scanned=len(sel) / scanned, bytes_read_per_row=bytes_read_per_row(f),
                          filter={k: (v if not (isinstance(v, tuple) and isinstance(v[0], bytes)) else [v[0].hex(), v[1]]) for k, v in f.items()})
    checks["the_nothing_filter_matches_nothing"] = info["nothing matches"]["rows_matched"] == 0
    pinned = torch.empty(max(len(w) for w in want.values()) + 4096, dtype=torch.uint8, pin_memory=True).numpy()
    route_host = {k: torch.empty(rows * w, dtype=torch.uint8, pin_memory=True).numpy() for k, w in ROUTE_COLUMNS.items()}

    def todays_route():
        """fa_raw_columns_device of the file, the eight columns to the host, the numpy filter -> the matching rows' projection"""
        with fa.FlowAgg(framed=True) as agg:
            agg.sync()
            t0 = time.perf_counter()
            cols, nrows = agg.raw_columns(frames)
            for k, w in ROUTE_COLUMNS.items():
                assert hip.hipMemcpy(route_host[k].ctypes.data, getattr(cols, k), nrows * w, 2) == 0  # hipMemcpyDeviceToHost
            tr = route_host["time_received"].view("<u8")
            port = route_host["dst_port"].view("<u4")
            keep = (tr >= lo) & (tr < hi) & (port >= p_lo) & (port <= p_hi)
            got = {k: route_host[k].reshape(nrows, w)[keep] for k, w in ROUTE_COLUMNS.items()}
            dt = time.perf_counter() - t0
        return dt, int(keep.sum()), got

    # ---- end to end, interleaved
    order = list(cases) + ["today's route"]
    times = {k: [] for k in order}
    stats = {}
    for rnd in range(args.rounds):
        for which in order[rnd % len(order):] + order[:rnd % len(order)]:  # (who goes first rotates)
            if which == "today's route":
                dt, nkeep, got = todays_route()
                times[which].append(dt)
                checks["route_round_%d_rows" % rnd] = nkeep == info["1 % DstPort"]["rows_matched"]
                continue
            f = fa.raw_filter(**cases[which])
            with fa.FlowAgg(framed=True) as agg:
                agg.sync()
                desc = np.zeros(4, dtype=fa.RAW_PART_DTYPE)
                nparts_out, nbytes_out = C.c_size_t(), C.c_size_t()
                t0 = time.perf_counter()
                rc = L.fa_raw_select(agg._h, frames.ctypes.data, frames.size, C.byref(f), desc.ctypes.data, 4, C.byref(nparts_out), C.byref(nbytes_out))
                rc2 = L.fa_raw_selection_fetch(agg._h, pinned.ctypes.data, pinned.size, C.byref(nbytes_out)) if rc == 0 and not cases[which].get("count_only") else 0
                times[which].append(time.perf_counter() - t0)
                assert rc == 0 and rc2 == 0, (which, rc, rc2, L.fa_last_error(agg._h))
                if cases[which].get("count_only"):
                    checks["%s_round_%d" % (which, rnd)] = int(desc["bytes"][:nparts_out.value].sum()) == len(want[which]) and int(desc["rows"][:nparts_out.value].sum()) == info[which]["rows_matched"]
                else:
                    checks["%s_round_%d" % (which, rnd)] = pinned[:nbytes_out.value].tobytes() == want[which]
                stats[which] = dict(select=agg.raw_select_stats(), range=agg.raw_range_stats())
    res = {}
    for which in order:
        v = times[which]
        r = dict(ms=[x * 1e3 for x in v], ms_median=statistics.median(v) * 1e3, ms_min=min(v) * 1e3)
        if which in stats:
            s, g = stats[which]["select"], stats[which]["range"]
            r.update(info[which])
            r.update(rows_out=s["rows_out"], bytes_out=s["bytes_out"], launches=s["launches"], blocks_seen=g["blocks_seen"], blocks_decoded=g["blocks_decoded"],
                     probe_ms=g["probe_ns"] / 1e6, range_ms=g["range_ns"] / 1e6, decode_ms=g["decode_ns"] / 1e6, select_ms=s["select_ns"] / 1e6, emit_ms=s["emit_ns"] / 1e6,
                     gather_ms=s["gather_ns"] / 1e6, select_ns_per_scanned_row=s["select_ns"] / max(s["rows_scanned"], 1),
                     emit_ns_per_output_row=s["emit_ns"] / s["rows_out"] if s["rows_out"] else None, gather_ns_per_output_row=s["gather_ns"] / s["rows_out"] if s["rows_out"] else None)
        else:
            r.update(bytes_downloaded=rows * sum(ROUTE_COLUMNS.values()))
        res[which] = r
    out["cases"] = res
    out["required_1pct_median_below_fastest_route"] = res["1 % DstPort"]["ms_median"] < res["today's route"]["ms_min"]
    out["checks"] = {k: bool(v) for k, v in checks.items()}
    out["checks_ok"] = all(out["checks"].values())
    print("SELECT_STEP " + json.dumps(out))
    return 0 if out["checks_ok"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="records per fa_ingest_device call and per raw chunk")
    ap.add_argument("--universe-log2", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds")
    ap.add_argument("--step-timeout", type=int, default=540, help="seconds for the GPU step")
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_select_run.json"))
    args = ap.parse_args()
    if args.step:
        sys.exit(step(args))
    res = {"config": "framed FlowMessages, Zipf-1.1 over 2^%d addresses, %d records over 900 s of one Date, generated in HBM, one merged LZ4 part; fresh ctx per call; "
                     "one box, one run" % (args.universe_log2, args.records)}
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--records", str(args.records), "--chunk", str(args.chunk), "--universe-log2", str(args.universe_log2),
           "--rounds", str(args.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        print("the GPU step exceeded its %d s limit: stopping" % args.step_timeout, file=sys.stderr)
        sys.exit(124)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("SELECT_STEP ")]
    if not line:
        sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
        print("the GPU step failed (exit status %d): stopping" % p.returncode, file=sys.stderr)
        sys.exit(p.returncode or 1)
    res.update(json.loads(line[-1][len("SELECT_STEP "):]))
    res["source_hash"] = _pkg.load().source_hash()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {x: v.get(x) for x in ("ms_median", "ms_min", "rows_matched", "select_ns_per_scanned_row")} for k, v in res["cases"].items()}
                     | {"checks_ok": res["checks_ok"], "required": res["required_1pct_median_below_fastest_route"]}))
    sys.exit(0 if res["checks_ok"] and res["required_1pct_median_below_fastest_route"] else 1)


if __name__ == "__main__":
    main()
