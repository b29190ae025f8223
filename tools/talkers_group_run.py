#!/usr/bin/env python3
"""Exact top talkers over 8 partitions: the close in HBM (fa_group_top_talkers) beside the host route it replaces, on
tools/talkers_run.py's stream (framed FlowMessages, Zipf-1.1 addresses over 2^24, 2^23 records generated in HBM) cut into 8
partitions, one ctx each, all on one GPU:
  * fa_group_top_talkers(100) per direction - the first call and the median of the following ones;
  * in the same process the route without it: every member's fa_top_talkers(0) (every row crosses PCIe), fa_merge_talkers
    into one more ctx, its fa_top_talkers(100) - the results of both routes must be identical;
  * for one ctx: fa_rows_device(kind, k = 100) + fa_rows_fetch beside fa_top_talkers(100);
  * the FA_VERBOSE step times of one more group call per direction.
The GPU work is a child process under its own time limit.  Writes profiles/talkers_group_run.json."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402

NPARTS = 8


def timed(f, reps):
    """-> (result of the last call, {"first_ms", "median_ms" of the calls after the first})"""
    ms, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return res, {"first_ms": round(ms[0], 3), "median_ms": round(statistics.median(ms[1:] or ms), 3), "calls": reps}


def step(args):
    import torch
    fa = _pkg.load()
    fa.build()
    dev = torch.device("cuda", 0)
    n, per = args.records, args.records // NPARTS
    mp = fa.mock_params(mode=fa.MOCK_ZIPF, framed=1, seed=3, n_total=n, span_secs=900, zipf_log2_universe=args.universe_log2, zipf_s_x100=110)
    kw = dict(framed=True, max_batch_records=per)
    members = [fa.FlowAgg(**kw) for _ in range(NPARTS)]
    target = fa.FlowAgg(**kw)
    out = {"records": n, "partitions": NPARTS}
    try:
        cap = per * 96 + 4096
        d_buf = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_off = torch.empty(per + 1, dtype=torch.int32, device=dev)
        for p, m in enumerate(members):
            m.talkers_enable(args.capacity_log2)
            w = m.mock_generate_device(mp, p * per, per, d_buf.data_ptr(), cap, d_off.data_ptr())
            m.sync()
            m.ingest_device(d_buf.data_ptr(), w, d_off.data_ptr(), per)
            m.sync()
        target.talkers_enable(args.capacity_log2)
        out["groups_per_member"] = [m.talkers_stats()["used"] for m in members]
        same = True
        with fa.FlowGroup(members) as g:
            for d in (0, 1):
                name = "dst" if d else "src"
                got, out["group_top100_%s" % name] = timed(lambda: g.top_talkers(d, 100), args.reps)

                def host_route():
                    t0 = time.perf_counter()
                    rows = [m.top_talkers(d, 0) for m in members]
                    t1 = time.perf_counter()
                    target.talkers_reset()
                    for r in rows:
                        target.merge_talkers(d, r)
                    t2 = time.perf_counter()
                    top = target.top_talkers(d, 100)
                    t3 = time.perf_counter()
                    host_route.parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
                    return top
                host_route.parts = []
                want, out["host_route_top100_%s" % name] = timed(host_route, max(2, args.reps // 2))
                fetch, merge, top = (statistics.median(x[j] for x in host_route.parts[1:]) for j in range(3))
                out["host_route_top100_%s" % name].update(median_fetch_all_rows_ms=round(fetch, 3), median_merge_ms=round(merge, 3), median_top_ms=round(top, 3),
                                                          rows_over_pcie=int(sum(len(m.top_talkers(d, 0)) for m in members)))
                out["groups_%s" % name] = int(target.talkers_stats()["used"][d])
                same = same and got.tobytes() == want.tobytes() and len(got) == 100
                os.environ["FA_VERBOSE"] = "1"  # (read at every call: the step times of one more close, on stderr)
                g.top_talkers(d, 100)
                del os.environ["FA_VERBOSE"]
        out["routes_identical"] = bool(same)
        one = members[0]
        for d in (0, 1):
            name = "dst" if d else "src"
            kind = fa.ROWS_TALKERS_DST if d else fa.ROWS_TALKERS_SRC

            def rows_route():
                ptr, m = one.rows_device(kind, k=100)
                return one.rows_fetch(kind, ptr, m)
            a, out["one_ctx_rows_device_top100_%s" % name] = timed(rows_route, args.reps)
            b, out["one_ctx_top_talkers_top100_%s" % name] = timed(lambda: one.top_talkers(d, 100), args.reps)
            same = same and a.tobytes() == b.tobytes()
        out["one_ctx_routes_identical"] = bool(same)
    finally:
        for x in members + [target]:
            x.close()
    print("TALKERS_GROUP_STEP " + json.dumps(out))
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--universe-log2", type=int, default=24)
    ap.add_argument("--capacity-log2", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7, help="calls per measured route (the first is reported on its own)")
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds for the GPU step")
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "talkers_group_run.json"))
    args = ap.parse_args()
    if args.step:
        sys.exit(step(args))
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--records", str(args.records), "--universe-log2", str(args.universe_log2),
           "--capacity-log2", str(args.capacity_log2), "--reps", str(args.reps)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        print("the GPU step exceeded its %d s limit: stopping" % args.step_timeout, file=sys.stderr)
        sys.exit(124)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("TALKERS_GROUP_STEP ")]
    if not line:
        sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
        print("the GPU step failed (exit status %d)" % p.returncode, file=sys.stderr)
        sys.exit(p.returncode or 1)
    res = {"config": "framed FlowMessages, Zipf-1.1 over 2^%d addresses, %d records generated in HBM, %d partitions = %d ctxs on one GPU, talkers only beside flows_5m"
                     % (args.universe_log2, args.records, NPARTS, NPARTS)}
    res.update(json.loads(line[-1][len("TALKERS_GROUP_STEP "):]))
    res["verbose_step_times"] = [ln.strip() for ln in p.stderr.splitlines() if "[flowagg group] top talkers" in ln]
    for name in ("src", "dst"):
        res["host_route_over_group_median_%s" % name] = round(res["host_route_top100_%s" % name]["median_ms"] / res["group_top100_%s" % name]["median_ms"], 3)
    res["source_hash"] = _pkg.load().source_hash()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in res if k.startswith(("group_top100", "host_route_top100", "host_route_over", "routes_identical", "one_ctx"))}))
    sys.exit(0 if res["routes_identical"] and res["one_ctx_routes_identical"] and p.returncode == 0 else 1)


if __name__ == "__main__":
    main()
