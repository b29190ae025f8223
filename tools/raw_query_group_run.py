#!/usr/bin/env python3
"""What a query over the whole topic costs (fa_group_raw_query_pending + fa_group_raw_query_rows; include/flowagg.h "queries over
the whole topic"), on tools/raw_query_run.py's stream: framed FlowMessages, Zipf-1.1 addresses over 2^24, generated in HBM, 2^23
records over 900 s of ONE Date, cut into 8 members ON ONE GPU (chunk c of 2^18 records goes to member c mod 8; every member merges
its parts).  One child process under a time limit - one box, one session:
  * the five panels (SRC_ADDR | DST_ADDR | SRC_PORT | DST_PORT | MINUTE, the first 100 rows of each by weight) over 1/8 of the time
    axis and over the whole axis; wall clock around the calls and their reads; three interleaved rounds, who goes first rotating;
    medians;
  * route "group": fa_group_raw_query_pending + five fa_group_raw_query_rows; after the timed rounds once more under FA_VERBOSE
    for the steps' times (a verbose read synchronises at every mark: its lines are not the timed run);
  * route "host": what a caller has without the group door - every member's fa_raw_query_pending, its five kinds with k = 0 fetched
    over PCIe, dist.merge_query_host per kind, the first 100 rows;
  * route "one ctx": ONE ctx that ingested all records: fa_raw_query_pending + five fa_raw_query_rows;
  * the merge kernel: every member's SrcAddr rows of the whole axis (fa_raw_query_rows_device, k = 0) added to a fresh result with
    fa_raw_query_merge_device - hipEvent time of the add launches per row, the wall clock of the calls beside it;
  * checks_ok: in every round every route's rows of every kind equal, byte for byte, this tool's numpy group-by
    (tools/raw_query_run.py, numpy_rows) over spill.read_native of a twin's taken bytes; and the merged result's SrcAddr rows.
Members on several GPUs - the exchange over xGMI instead of copies inside one HBM - are NOT measured here.  No time is gated.
Writes profiles/raw_query_group_run.json."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _pkg  # noqa: E402
import numpy as np  # noqa: E402
from raw_query_run import K, KIND_NAMES, NO_UPPER, PANELS, in_range, numpy_rows  # noqa: E402

MEMBERS = 8


def step(args):
    import torch
    fa = _pkg.load()
    fa.build()
    L = fa.lib()
    dev = torch.device("cuda", 0)
    n, chunk = args.records, args.chunk
    mp = fa.mock_params(mode=fa.MOCK_ZIPF, framed=1, seed=3, n_total=n, span_secs=900, zipf_log2_universe=args.universe_log2, zipf_s_x100=110)
    out, checks = {"records": n, "chunk_records": chunk, "k": K, "members": MEMBERS}, {}
    cap = chunk * 96 + 4096
    d_buf = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off = torch.empty(chunk + 1, dtype=torch.int32, device=dev)

    def ingested(member=None):
        """a ctx with fa_raw_enable that ingested the stream (member: only the chunks c with c mod MEMBERS == member), parts merged"""
        agg = fa.FlowAgg(framed=True, max_batch_records=chunk, key_sets=1)
        agg.raw_enable(chunk)
        for c, i0 in enumerate(range(0, n, chunk)):
            if member is not None and c % MEMBERS != member:
                continue
            m = min(chunk, n - i0)
            w = agg.mock_generate_device(mp, i0, m, d_buf.data_ptr(), cap, d_off.data_ptr())
            agg.ingest_device(d_buf.data_ptr(), w, d_off.data_ptr(), m)
        agg.sync()
        agg.raw_merge()
        return agg

    members = [ingested(i) for i in range(MEMBERS)]
    whole = ingested()
    group = fa.FlowGroup(members)
    out["member_pending_bytes"] = [int(m.raw_stats()["pending_bytes"]) for m in members]

    # ---- the rows as spill.read_native delivers a twin's plain bytes; the cases and what numpy makes of them
    with ingested() as twin:
        data, _ = twin.raw_take()
        (block,) = fa.spill.read_native(bytes(data))
        del data
    t = block["TimeReceived"]
    rows = len(t)
    assert (np.diff(t.astype(np.int64)) >= 0).all()
    out["rows"] = rows
    lo, hi = int(t[rows // 2 - rows // 16]), int(t[min(rows - 1, rows // 2 + rows // 16)])  # the seconds around the middle that hold 1/8 of the rows
    cases = {"1/8 of the axis": dict(t_lo=lo, t_hi=hi), "the whole axis": dict(t_lo=0, t_hi=NO_UPPER)}
    want, info = {}, {}
    for name, f in cases.items():
        mask = in_range(t, f["t_lo"], f["t_hi"])
        want[name], groups = {}, {}
        for bit, kind in KIND_NAMES.items():
            want[name][bit], groups[kind] = numpy_rows(fa, block, mask, bit, K)
        info[name] = dict(rows_in_range=int(mask.sum()), groups=groups, filter=f)
    del block

    buf, cnt = np.zeros(K, dtype=fa.QUERY_ROW_DTYPE), C.c_size_t()

    def sync_all():
        for a in members + [whole]:
            a.sync()

    def group_route(f):
        sync_all()
        t0 = time.perf_counter()
        group.raw_query_pending(PANELS, **f)
        t1 = time.perf_counter()
        got = {}
        for bit in KIND_NAMES:
            rc = L.fa_group_raw_query_rows(group._h, bit, fa.RAW_O_WEIGHT, K, buf.ctypes.data, K, C.byref(cnt))
            assert rc == 0, (rc, L.fa_group_last_error(group._h))
            got[bit] = buf[:cnt.value].copy()
        t2 = time.perf_counter()
        return t2 - t0, got, dict(query_ms=(t1 - t0) * 1e3, reads_ms=(t2 - t1) * 1e3)

    def host_route(f):
        sync_all()
        t0 = time.perf_counter()
        parts = {bit: [] for bit in KIND_NAMES}
        for m in members:
            m.raw_query_pending(PANELS, **f)
            for bit in KIND_NAMES:
                parts[bit].append(m.raw_query_rows(bit, 0, fa.RAW_O_WEIGHT))
        t1 = time.perf_counter()
        got = {bit: fa.dist.merge_query_host(parts[bit], fa.RAW_O_WEIGHT)[:K] for bit in KIND_NAMES}
        t2 = time.perf_counter()
        return t2 - t0, got, dict(queries_and_fetch_ms=(t1 - t0) * 1e3, host_merge_ms=(t2 - t1) * 1e3, rows_fetched={KIND_NAMES[b]: int(sum(len(p) for p in parts[b])) for b in KIND_NAMES},
                                  bytes_fetched=int(sum(p.nbytes for ps in parts.values() for p in ps)))

    def one_ctx_route(f):
        sync_all()
        t0 = time.perf_counter()
        whole.raw_query_pending(PANELS, **f)
        got = {}
        for bit in KIND_NAMES:
            rc = L.fa_raw_query_rows(whole._h, bit, fa.RAW_O_WEIGHT, K, buf.ctypes.data, K, C.byref(cnt))
            assert rc == 0, (rc, L.fa_last_error(whole._h))
            got[bit] = buf[:cnt.value].copy()
        return time.perf_counter() - t0, got, {}

    routes = {"group": group_route, "host": host_route, "one ctx": one_ctx_route}
    order = [(c, r) for c in cases for r in routes]
    times, stats = {k: [] for k in order}, {}
    for rnd in range(args.rounds):
        for which in order[rnd % len(order):] + order[:rnd % len(order)]:  # (who goes first rotates)
            dt, got, st = routes[which[1]](cases[which[0]])
            times[which].append(dt)
            stats[which] = st
            checks["%s / %s / round %d" % (which[0], which[1], rnd)] = all(got[b].tobytes() == want[which[0]][b].tobytes() for b in KIND_NAMES)

    # ---- the steps of the group reads, once per case, under FA_VERBOSE (stderr of the library, through a file)
    verbose = {}
    for name, f in cases.items():
        group.raw_query_pending(PANELS, **f)
        with tempfile.TemporaryFile() as tmp:
            sys.stderr.flush()
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            os.environ["FA_VERBOSE"] = "1"
            try:
                for bit in KIND_NAMES:
                    L.fa_group_raw_query_rows(group._h, bit, fa.RAW_O_WEIGHT, K, buf.ctypes.data, K, C.byref(cnt))
            finally:
                del os.environ["FA_VERBOSE"]
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            verbose[name] = [ln for ln in tmp.read().decode(errors="replace").splitlines() if ln.startswith("[flowagg group]")]

    # ---- the merge kernel: every member's SrcAddr rows of the whole axis into one fresh result
    group.raw_query_pending(PANELS, **cases["the whole axis"])
    merge = {}
    with fa.FlowAgg(framed=True) as sink:
        sink.raw_enable(0)
        sink.raw_query_pending(PANELS)  # (no pending parts: an empty result with the five kinds)
        q0 = sink.raw_query_stats()
        wall = 0.0
        for m in members:
            ptr, cnt_rows = m.raw_query_rows_device(1, 0, fa.RAW_O_KEY)
            sink.sync()
            t0 = time.perf_counter()
            sink.raw_query_merge(1, ptr, cnt_rows)
            wall += time.perf_counter() - t0
        q1, ms = sink.raw_query_stats(), sink.raw_query_merge_stats()
        merged_top = sink.raw_query_rows(1, K, fa.RAW_O_WEIGHT)
        checks["merge kernel / SRC_ADDR of the whole axis"] = merged_top.tobytes() == want["the whole axis"][1].tobytes()
        merge = dict(rows_merged=ms["rows_merged"], calls=ms["merge_calls"], groups=q1["groups"], add_launches_ms=(q1["fold_ns"] - q0["fold_ns"]) / 1e6,
                     kernel_ns_per_row=(q1["fold_ns"] - q0["fold_ns"]) / max(ms["rows_merged"], 1), calls_wall_ms=wall * 1e3, calls_wall_ns_per_row=wall * 1e9 / max(ms["rows_merged"], 1),
                     grows=q1["grows"] - q0["grows"], launches=q1["launches"] - q0["launches"])
    res = {}
    for name in cases:
        c = dict(info[name])
        for r in routes:
            x = times[name, r]
            c[r] = dict(ms=[y * 1e3 for y in x], ms_median=statistics.median(x) * 1e3, **stats[name, r])
        c["group_verbose_steps"] = verbose[name]
        c["group_faster_than_host_route"] = c["group"]["ms_median"] < c["host"]["ms_median"]
        c["group_faster_than_one_ctx"] = c["group"]["ms_median"] < c["one ctx"]["ms_median"]
        res[name] = c
    group.close()
    for a in members + [whole]:
        a.close()
    out["cases"] = res
    out["merge_kernel"] = merge
    out["not_measured"] = "members on several GPUs (the exchange over xGMI); all 8 members share one GPU here, so their queries and merges also share its CUs"
    out["checks"] = {k: bool(v) for k, v in checks.items()}
    out["checks_ok"] = all(out["checks"].values())
    print("GROUP_QUERY_STEP " + json.dumps(out))
    return 0 if out["checks_ok"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--chunk", type=int, default=1 << 18, help="records per fa_ingest_device call and per raw chunk; chunk c belongs to member c mod 8")
    ap.add_argument("--universe-log2", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds for the GPU step")
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_query_group_run.json"))
    args = ap.parse_args()
    if args.step:
        sys.exit(step(args))
    res = {"config": "framed FlowMessages, Zipf-1.1 over 2^%d addresses, %d records over 900 s of one Date, generated in HBM; %d members on ONE GPU (chunks of %d records dealt "
                     "round-robin, parts merged), one ctx with all records beside them; one box, one run" % (args.universe_log2, args.records, MEMBERS, args.chunk)}
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--records", str(args.records), "--chunk", str(args.chunk), "--universe-log2", str(args.universe_log2),
           "--rounds", str(args.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        print("the GPU step exceeded its %d s limit: stopping" % args.step_timeout, file=sys.stderr)
        sys.exit(124)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("GROUP_QUERY_STEP ")]
    if not line:
        sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
        print("the GPU step failed (exit status %d): stopping" % p.returncode, file=sys.stderr)
        sys.exit(p.returncode or 1)
    res.update(json.loads(line[-1][len("GROUP_QUERY_STEP "):]))
    res["source_hash"] = _pkg.load().source_hash()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {v: c[v]["ms_median"] for v in ("group", "host", "one ctx")} for k, c in res["cases"].items()}
                     | {"merge_kernel_ns_per_row": res["merge_kernel"]["kernel_ns_per_row"], "checks_ok": res["checks_ok"]}))
    sys.exit(0 if res["checks_ok"] else 1)


if __name__ == "__main__":
    main()
