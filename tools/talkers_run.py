#!/usr/bin/env python3
"""What the exact top talkers (fa_talkers_enable: a second pass per ingest call) cost, on a device-generated Zipf stream of
BASELINE config 3's shape (framed FlowMessages, Zipf-1.1 addresses over 2^24, key_sets = flows_5m + both sketches):
  * records/s of fa_ingest_device on a ctx WITHOUT talkers (what every existing caller gets);
  * the same on a ctx with talkers enabled, and the added cost per record relative to the run above;
  * the fold kernel's own time per record (fa_talkers_stats: fold_ns_total) against the 53 bytes per record it must read;
  * parity of the top 100 of both directions against a numpy group-by of the decoded columns (fa_decode of the same bytes).
Every GPU step is a child process under its own time limit; the first failure ends the run.  Writes profiles/talkers_run.json."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402

FOLD_BYTES_PER_RECORD = 16 + 16 + 4 + 8 + 8 + 1  # src_addr, dst_addr, etype, bytes, sampling_rate, status


def group_talkers(fa, rows, dst):
    """numpy GROUP BY of decoded rows (FLOW_ROW_DTYPE), grouped as the dashboards do -> (key bytes, family, weight, count), unordered."""
    r = rows[rows["status"] == 0]
    addr = np.ascontiguousarray(r["dst_addr" if dst else "src_addr"]).copy().reshape(-1, 16)
    v4 = r["etype"] == 0x800
    addr[v4, 4:] = 0
    k = np.zeros(len(r), dtype=[("hi", ">u8"), ("lo", ">u8"), ("fam", "<u4")])
    k["hi"] = addr[:, :8].copy().view(">u8").reshape(-1)
    k["lo"] = addr[:, 8:].copy().view(">u8").reshape(-1)
    k["fam"] = np.where(v4, 0x800, 0)
    with np.errstate(over="ignore"):
        w = r["bytes"] * r["sampling_rate"]
    return k, w, np.ones(len(r), dtype=np.uint64)


def reduce_groups(k, w, c):
    order = np.lexsort((k["fam"], k["lo"], k["hi"]))
    k, w, c = k[order], w[order], c[order]
    first = np.ones(len(k), dtype=bool)
    first[1:] = k[1:] != k[:-1]
    starts = np.nonzero(first)[0]
    with np.errstate(over="ignore"):
        return k[starts], np.add.reduceat(w, starts), np.add.reduceat(c, starts)


def step(args):
    """One GPU step in this process: prints one JSON line."""
    import torch
    fa = _pkg.load()
    fa.build()
    dev = torch.device("cuda", 0)
    n, chunk = args.records, args.chunk
    mp = fa.mock_params(mode=fa.MOCK_ZIPF, framed=1, seed=3, n_total=n, span_secs=900, zipf_log2_universe=args.universe_log2, zipf_s_x100=110)
    talk = args.step == "talkers"
    out = {}
    with fa.FlowAgg(framed=True, key_sets=7, topk_mode=fa.TOPK_CANDIDATES, topk_capacity_log2=16, max_batch_records=chunk) as agg:
        if talk:
            agg.talkers_enable(args.capacity_log2)
        cap = chunk * 96 + 4096
        d_buf = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_off = torch.empty(chunk + 1, dtype=torch.int32, device=dev)
        secs = []
        for i0 in range(0, n, chunk):
            m = min(chunk, n - i0)
            w = agg.mock_generate_device(mp, i0, m, d_buf.data_ptr(), cap, d_off.data_ptr())
            agg.sync()
            t0 = time.perf_counter()
            agg.ingest_device(d_buf.data_ptr(), w, d_off.data_ptr(), m)
            agg.sync()
            secs.append((time.perf_counter() - t0, m))
        st = agg.stats()
        assert st["records_ok"] == n and st["records_bad"] == 0, st
        steady = secs[1:] if len(secs) > 1 else secs  # (the first call pays the ctx's allocations, and the first table growths)
        out["records"] = n
        out["chunk_records"] = chunk
        out["ingest_wall_s_per_chunk"] = [round(s, 6) for s, _ in secs]
        out["records_per_s"] = sum(m for _, m in steady) / sum(s for s, _ in steady)
        if talk:
            ts = agg.talkers_stats()
            out["talkers_stats"] = ts
            out["fold_ns_per_record"] = ts["fold_ns_total"] / max(1, ts["records_folded"])
            out["fold_GBps_of_the_53_bytes_it_reads"] = FOLD_BYTES_PER_RECORD / max(1e-9, out["fold_ns_per_record"])
            out["fold_roofline_frac"] = out["fold_GBps_of_the_53_bytes_it_reads"] * 1e9 / 8e12
            out["decode_ns_per_record_second_pass"] = st["decode_ns_total"] / n
            tops = [agg.top_talkers(d, 100) for d in (0, 1)]
            t0 = time.perf_counter()
            agg.top_talkers(0, 100)
            out["top100_ms_per_call"] = (time.perf_counter() - t0) * 1e3
            # parity: the same bytes from the host twin of the generator, decoded (fa_decode), grouped with numpy
            parts = [[], []]
            for i0 in range(0, n, chunk):
                m = min(chunk, n - i0)
                hb, ho = fa.mock_generate_host(mp, i0, m)
                rows = agg.decode(hb, ho)
                for d in (0, 1):
                    parts[d].append(reduce_groups(*group_talkers(fa, rows, d)))
            ok = True
            for d in (0, 1):
                k, w, c = reduce_groups(*[np.concatenate([p[j] for p in parts[d]]) for j in range(3)])
                order = np.lexsort((k["fam"], k["lo"], k["hi"], np.uint64(0xFFFFFFFFFFFFFFFF) - w))[:100]
                want = np.zeros(len(order), dtype=fa.TALKER_ROW_DTYPE)
                be = lambda v: np.ascontiguousarray(v).astype(">u8").reshape(-1, 1).view(np.uint8)  # the words' bytes in address order
                want["key"] = np.concatenate([be(k["hi"][order]), be(k["lo"][order])], axis=1)
                want["etype"], want["weight"], want["count"] = k["fam"][order], w[order], c[order]
                same = len(tops[d]) == len(want) and all(np.array_equal(tops[d][f], want[f]) for f in ("key", "etype", "weight", "count"))
                ok = ok and same and ts["used"][d] == len(k)
                out["groups_%s" % ("dst" if d else "src")] = int(len(k))
            out["top100_parity"] = bool(ok)
    print("TALKERS_STEP " + json.dumps(out))
    return 0 if (not talk or out["top100_parity"]) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="records per fa_ingest_device call")
    ap.add_argument("--universe-log2", type=int, default=24)
    ap.add_argument("--capacity-log2", type=int, default=0, help="fa_talkers_enable's initial table size (0: the library's default)")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--step", choices=["plain", "talkers"], help="(internal) run one step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "talkers_run.json"))
    args = ap.parse_args()
    if args.step:
        sys.exit(step(args))
    res = {"config": "BASELINE config 3's shape: framed FlowMessages, Zipf-1.1 over 2^%d addresses, key_sets = flows_5m + both sketches (candidates mode), "
                     "%d records in calls of %d, generated in HBM" % (args.universe_log2, args.records, args.chunk)}
    for name in ("plain", "talkers"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--records", str(args.records), "--chunk", str(args.chunk),
               "--universe-log2", str(args.universe_log2), "--capacity-log2", str(args.capacity_log2)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print("step %s exceeded its %d s limit: stopping" % (name, args.step_timeout), file=sys.stderr)
            sys.exit(124)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("TALKERS_STEP ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
            print("step %s failed (exit status %d): stopping" % (name, p.returncode), file=sys.stderr)
            sys.exit(p.returncode or 1)
        res[name] = json.loads(line[-1][len("TALKERS_STEP "):])
    a, b = res["plain"]["records_per_s"], res["talkers"]["records_per_s"]
    res["records_per_s_without_talkers"] = a
    res["records_per_s_with_talkers"] = b
    res["added_ns_per_record"] = 1e9 / b - 1e9 / a
    res["added_cost_relative_to_the_run_without"] = a / b - 1.0
    res["fold_ns_per_record"] = res["talkers"]["fold_ns_per_record"]
    res["top100_parity"] = res["talkers"]["top100_parity"]
    res["source_hash"] = _pkg.load().source_hash()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("records_per_s_without_talkers", "records_per_s_with_talkers", "added_cost_relative_to_the_run_without",
                                          "fold_ns_per_record", "top100_parity")}))
    sys.exit(0 if res["top100_parity"] else 1)


if __name__ == "__main__":
    main()
