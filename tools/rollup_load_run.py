#!/usr/bin/env python3
"""What rebuilding flows_5m and the dashboard key sets from flows_raw parts costs (fa_raw_load_rollup; include/flowagg.h "the
rollups from columns and from parts"), on tools/raw_load_run.py's stream: a device-generated BASELINE config 2 stream kept in
HBM, 2^23 records in calls of 2^21.  One ctx with the four exact key sets and fa_raw_enable ingests it and delivers its parts as
LZ4 frames (fa_raw_take_lz4) into page-locked memory.  One child process under a time limit - one box, one session:
  * fa_raw_load_rollup of those frames, end to end (ONE call: copy in, decode, header check, unpack, fold, settle), into a fresh
    ctx of the same configuration each round;
  * beside it the route without this feature: fa_ingest_device of the same records' wire bytes (already in HBM: no copy in) into
    a fresh ctx of the same configuration, interleaved round by round;
  * the fold kernel's ns per record from the library's hipEvents (fa_rollup_stats.fold_ns), for flows_5m alone (key_sets =
    FA_KEYS_AS_PAIR) and for all four exact key sets, each into a fresh ctx each round;
  * checks_ok: every read of the loaded ctx - flows_5m, (SrcAddr,DstPort,Proto), both port rankings, the minute series, the open
    timeslots - equals the ingesting ctx's.
Medians of the rounds.  Nothing is gated on the times.  Writes profiles/rollup_load_run.json."""
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

KS4 = 1 | 8 | 16 | 32


def step(args):
    import torch
    fa = _pkg.load()
    fa.build()
    L = fa.lib()
    dev = torch.device("cuda", 0)
    n, chunk = args.records, args.chunk
    mp = fa.mock_params(mode=fa.MOCK_ASPAIRS, framed=1, seed=3, n_total=n, span_secs=900)
    kw = dict(framed=True, max_batch_records=chunk, key_sets=KS4)
    out, checks = {}, {}

    def reads(agg):
        return [agg.read_window().tobytes(), agg.read_window_app().tobytes(), agg.top_ports(0).tobytes(), agg.top_ports(1).tobytes(),
                agg.minute_series().tobytes(), agg.open_timeslots().tobytes()]

    with fa.FlowAgg(**kw) as src:
        src.raw_enable()
        cap = chunk * 96 + 4096
        batches = []
        for i0 in range(0, n, chunk):
            m = min(chunk, n - i0)
            d_buf = torch.empty(cap, dtype=torch.uint8, device=dev)
            d_off = torch.empty(chunk + 1, dtype=torch.int32, device=dev)
            w = src.mock_generate_device(mp, i0, m, d_buf.data_ptr(), cap, d_off.data_ptr())
            batches.append((d_buf, d_off, w, m))

        def ingest(agg):
            for d_buf, d_off, w, m in batches:
                agg.ingest_device(d_buf.data_ptr(), w, d_off.data_ptr(), m)
            agg.sync()

        ingest(src)
        pending = src.raw_stats()
        nbytes, nparts = int(pending["pending_bytes"]), int(pending["pending_parts"])
        h_frames = torch.empty(L.fa_lz4_frame_bound(nbytes) + 15 * nparts, dtype=torch.uint8, pin_memory=True).numpy()
        parts = np.zeros(nparts, dtype=fa.RAW_PART_DTYPE)
        nb, npart = C.c_size_t(), C.c_size_t()
        rc = L.fa_raw_take_lz4(src._h, h_frames.ctypes.data, h_frames.size, C.byref(nb), parts.ctypes.data, nparts, C.byref(npart))
        assert rc == 0 and npart.value == nparts, rc
        frames = h_frames[:nb.value]
        want = reads(src)
        rows = int(parts["rows"].sum())
        groups = dict(zip(("flows_5m", "app", "src_ports", "dst_ports", "minutes"), (len(want[0]) // 48, len(want[1]) // 56, len(want[2]) // 24, len(want[3]) // 24, len(want[4]) // 24)))
    out.update(records=n, rows=rows, parts=nparts, lz4_bytes=int(nb.value), wire_bytes=int(sum(b[2] for b in batches)), rows_read=groups)
    t_load, t_ingest, fold_all, fold_5m, stats = [], [], [], [], None
    for r in range(args.rounds):
        for which in (("load", "ingest") if r % 2 == 0 else ("ingest", "load")):  # (who goes first alternates)
            with fa.FlowAgg(**kw) as agg:
                agg.sync()
                t0 = time.perf_counter()
                if which == "load":
                    rc = L.fa_raw_load_rollup(agg._h, frames.ctypes.data, frames.size, 0, 0)
                    t_load.append(time.perf_counter() - t0)
                    assert rc == 0, (rc, L.fa_last_error(agg._h))
                    stats = dict(agg.raw_load_stats(), **{"rollup_" + k: v for k, v in agg.rollup_stats().items()})
                    fold_all.append(stats["rollup_fold_ns"] / stats["rollup_records_folded"])
                    checks["load_round_%d_rows" % r] = stats["rollup_records_folded"] == rows
                else:
                    ingest(agg)
                    t_ingest.append(time.perf_counter() - t0)
                checks["%s_round_%d_equals_the_source" % (which, r)] = reads(agg) == want
        with fa.FlowAgg(**kw) as agg:  # flows_5m alone: the compile-time variant of the fold kernel
            rc = L.fa_raw_load_rollup(agg._h, frames.ctypes.data, frames.size, 1, 0)
            assert rc == 0, (rc, L.fa_last_error(agg._h))
            rs = agg.rollup_stats()
            fold_5m.append(rs["fold_ns"] / rs["records_folded"])
            checks["flows_5m_alone_round_%d" % r] = agg.read_window().tobytes() == want[0] and agg.stats()["wide_used"] == 0
    out["load_ms"] = [t * 1e3 for t in t_load]
    out["ingest_ms"] = [t * 1e3 for t in t_ingest]
    out["load_ms_median"] = statistics.median(t_load) * 1e3
    out["ingest_ms_median"] = statistics.median(t_ingest) * 1e3
    out["load_over_ingest"] = statistics.median(t_load) / statistics.median(t_ingest)
    out["load_ns_per_row"] = statistics.median(t_load) * 1e9 / rows
    out["ingest_ns_per_record"] = statistics.median(t_ingest) * 1e9 / n
    out["fold_kernel_ns_per_record_all_four"] = statistics.median(fold_all)
    out["fold_kernel_ns_per_record_flows_5m_alone"] = statistics.median(fold_5m)
    out["fold_kernel_ns_per_record_rounds"] = dict(all_four=fold_all, flows_5m_alone=fold_5m)
    out["stats_last_round"] = stats
    out["device_ms_of_a_load"] = {k: stats[k] / 1e6 for k in ("decode_ns", "unpack_ns", "fold_ns", "rollup_fold_ns")}
    out["checks"] = {k: bool(v) for k, v in checks.items()}
    out["checks_ok"] = all(out["checks"].values())
    print("ROLLUP_STEP " + json.dumps(out))
    return 0 if out["checks_ok"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="records per fa_ingest_device call")
    ap.add_argument("--rounds", type=int, default=3, help="interleaved loads and re-ingests")
    ap.add_argument("--step-timeout", type=int, default=540, help="seconds for the GPU step")
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollup_load_run.json"))
    args = ap.parse_args()
    if args.step:
        sys.exit(step(args))
    res = {"config": "framed FlowMessages, BASELINE config 2 (65 536 AS pairs x 2 ETypes over 900 s), %d records in calls of %d, generated in HBM; "
                     "key sets flows_5m + (SrcAddr,DstPort,Proto) + ports + minutes, default capacities; raw chunk 2^20; one box, one run" % (args.records, args.chunk)}
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--records", str(args.records), "--chunk", str(args.chunk), "--rounds", str(args.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        print("the GPU step exceeded its %d s limit: stopping" % args.step_timeout, file=sys.stderr)
        sys.exit(124)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ROLLUP_STEP ")]
    if not line:
        sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
        print("the GPU step failed (exit status %d): stopping" % p.returncode, file=sys.stderr)
        sys.exit(p.returncode or 1)
    res.update(json.loads(line[-1][len("ROLLUP_STEP "):]))
    res["source_hash"] = _pkg.load().source_hash()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res.get(k) for k in ("rows", "load_ms_median", "ingest_ms_median", "load_over_ingest", "fold_kernel_ns_per_record_all_four",
                                              "fold_kernel_ns_per_record_flows_5m_alone", "checks_ok")}))
    sys.exit(0 if res["checks_ok"] else 1)


if __name__ == "__main__":
    main()
