#!/usr/bin/env python3
"""What the bucketed port tables cost (fa_ports_enable_buckets, bucket_secs = 60), by tools/talker_buckets_run.py's method: a
device-generated Zipf-1.1 stream with BASELINE config 3's key sets (flows_5m + both sketches) spanning 900 s (15 buckets), kept
in HBM and ingested with fa_ingest_device in calls of 2^21 records.  One child process under a time limit - one box, one session:
  * fa_ingest_device records/s of a ctx WITHOUT the second pass and of a ctx WITH the port pass, interleaved round by round over
    the same buffers (the port tables are emptied, untimed, before each round; the first round also pays their growth);
  * the fold kernel's ns per record (fa_ports_stats);
  * fa_top_ports_range(k = 100) over every bucket and over one bucket; fa_ports_drop_before of a third of the buckets;
  * fa_top_ports of a FA_KEYS_PORT_HIST ctx over the same stream, for comparison;
  * with talkers and ports both enabled: decode launches per ingest call beside a talkers-only ctx's.  The second pass decodes a
    chunk once for every enabled fold, and a chunk is as long as the smallest cap of the enabled folds allows - both ctxs' tables
    start at 2^22 slots here so that FA_TALK_CHUNK is that cap in both, and the counts must be equal.
None of the times is gated: nobody had measured them before this tool.  checks_ok - every result equal to a numpy restatement on
the decoded columns (fetched from the ctx's own fa_decode_device), every row in order - also sets the exit status.
Reads are timed as the median of 5 calls after one warm-up call.  Writes profiles/port_buckets_run.json."""
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

BUCKET_SECS = 60
NO_UPPER = 0xFFFFFFFF
U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def timed(call, reps=5):
    call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def np_top_ports(port, weight, keep, k=0):
    """GROUP BY port over the records of `keep`: (port, sum of weight mod 2^64, count) ORDER BY weight DESC, port."""
    p, w = port[keep].astype(np.uint64), weight[keep]
    order = np.argsort(p, kind="stable")
    p, w = p[order], w[order]
    starts = np.nonzero(np.concatenate([[True], p[1:] != p[:-1]]))[0] if len(p) else np.zeros(0, dtype=np.int64)
    with np.errstate(over="ignore"):
        ws = np.add.reduceat(w, starts) if len(p) else w
    cs = np.diff(np.concatenate([starts, [len(p)]])).astype(np.uint64)
    ports = p[starts]
    o = np.lexsort((ports, U64MAX - ws))
    rows = np.stack([ports[o], ws[o], cs[o]], axis=1)
    return rows[:k] if k else rows


def as_triples(rows):
    return np.stack([rows["port"].astype(np.uint64), rows["weight"], rows["count"]], axis=1)


def step(args):
    import torch
    fa = _pkg.load()
    fa.build()
    dev = torch.device("cuda", 0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    n, chunk = args.records, args.chunk
    mp = fa.mock_params(mode=fa.MOCK_ZIPF, framed=1, seed=3, n_total=n, span_secs=900, zipf_log2_universe=args.universe_log2, zipf_s_x100=110)
    kw = dict(framed=True, topk_mode=fa.TOPK_CANDIDATES, topk_capacity_log2=16, max_batch_records=chunk)
    out, checks = {}, {}
    with fa.FlowAgg(key_sets=7, **kw) as none, fa.FlowAgg(key_sets=7, **kw) as port, fa.FlowAgg(key_sets=7 | fa.FA_KEYS_PORT_HIST, **kw) as hist, \
            fa.FlowAgg(key_sets=7, **kw) as talk, fa.FlowAgg(key_sets=7, **kw) as both:
        port.ports_enable_buckets(args.capacity_log2, BUCKET_SECS)
        talk.talkers_enable(22, BUCKET_SECS)
        both.talkers_enable(22, BUCKET_SECS)
        both.ports_enable_buckets(22, BUCKET_SECS)
        # the stream, generated once and kept in HBM; its decoded columns on the host for the restatement
        cap = chunk * 96 + 4096
        batches, cols = [], {name: [] for name in ("src_port", "dst_port", "bytes", "sampling_rate", "time_flow_start", "status")}
        dtypes = dict(src_port=np.uint32, dst_port=np.uint32, bytes=np.uint64, sampling_rate=np.uint64, time_flow_start=np.uint64, status=np.uint8)
        for i0 in range(0, n, chunk):
            m = min(chunk, n - i0)
            d_buf = torch.empty(cap, dtype=torch.uint8, device=dev)
            d_off = torch.empty(chunk + 1, dtype=torch.int32, device=dev)
            w = none.mock_generate_device(mp, i0, m, d_buf.data_ptr(), cap, d_off.data_ptr())
            batches.append((d_buf, d_off, w, m))
            c = none.decode_device(d_buf.data_ptr(), w, d_off.data_ptr(), m)
            none.sync()
            for name in cols:
                a = np.zeros(m, dtype=dtypes[name])
                assert hip.hipMemcpy(a.ctypes.data, getattr(c, name), a.nbytes, 2) == 0  # hipMemcpyDeviceToHost
                cols[name].append(a)
        cols = {k: np.concatenate(v) for k, v in cols.items()}
        ok = cols["status"] == 0
        with np.errstate(over="ignore"):
            weight = cols["bytes"] * cols["sampling_rate"]
        t32 = cols["time_flow_start"] & np.uint64(0xFFFFFFFF)
        bucket = t32 - t32 % np.uint64(BUCKET_SECS)

        def ingest(agg):
            t0 = time.perf_counter()
            for d_buf, d_off, w, m in batches:
                agg.ingest_device(d_buf.data_ptr(), w, d_off.data_ptr(), m)
            agg.sync()
            return n / (time.perf_counter() - t0)
        rates = {"none": [], "port": []}
        for _ in range(args.rounds):
            port.ports_reset()
            for name, agg in (("none", none), ("port", port)):
                rates[name].append(ingest(agg))
        out["ingest_records_per_s_without_the_pass"] = rates["none"]
        out["ingest_records_per_s_with_the_port_pass"] = rates["port"]
        out["ingest_records_per_s_median"] = {k: statistics.median(v) for k, v in rates.items()}
        ps = port.ports_stats()
        out["ports_stats"] = ps
        out["fold_ns_per_record"] = ps["fold_ns_total"] / max(1, ps["records_folded"])
        checks["records_folded"] = ps["records_folded"] == args.rounds * int(ok.sum())
        b = port.ports_buckets()
        held = np.unique(bucket[ok]).astype(np.uint32)
        checks["buckets"] = np.array_equal(b, held)
        out["buckets"] = int(len(b))
        lo, end, mid = int(b[0]), int(b[-1]) + BUCKET_SECS, int(b[len(b) // 2])
        for d, name in ((0, "src_port"), (1, "dst_port")):
            pairs = len(np.unique((bucket[ok] << np.uint64(32)) | cols[name][ok].astype(np.uint64)))
            checks["used_%d" % d] = ps["used"][d] == pairs
            every = np_top_ports(cols[name], weight, ok)
            checks["all_buckets_every_row_%d" % d] = np.array_equal(as_triples(port.top_ports_range(d, 0, lo, end)), every)
            checks["no_upper_bound_every_row_%d" % d] = np.array_equal(as_triples(port.top_ports_range(d, 0, 0, NO_UPPER)), every)
            checks["all_buckets_k100_%d" % d] = np.array_equal(as_triples(port.top_ports_range(d, 100, lo, end)), every[:100])
            one = np_top_ports(cols[name], weight, ok & (bucket == np.uint64(mid)))
            checks["one_bucket_every_row_%d" % d] = np.array_equal(as_triples(port.top_ports_range(d, 0, mid, mid + BUCKET_SECS)), one)
            checks["one_bucket_k100_%d" % d] = np.array_equal(as_triples(port.top_ports_range(d, 100, mid, mid + BUCKET_SECS)), one[:100])
        out["groups_all_buckets"] = int(len(port.top_ports_range(0, 0, lo, end)))
        out["range_all_buckets_k100_ms"] = timed(lambda: port.top_ports_range(0, 100, lo, end))
        out["range_one_bucket_k100_ms"] = timed(lambda: port.top_ports_range(0, 100, mid, mid + BUCKET_SECS))
        # the un-ranged call of a FA_KEYS_PORT_HIST ctx over the same records
        ingest(hist)
        for d, name in ((0, "src_port"), (1, "dst_port")):
            checks["fa_top_ports_%d" % d] = np.array_equal(as_triples(hist.top_ports(d)), np_top_ports(cols[name], weight, ok))
        out["fa_top_ports_k100_ms"] = timed(lambda: hist.top_ports(0, 100))
        # retention: a third of the buckets
        floor = int(b[len(b) // 3])
        t0 = time.perf_counter()
        port.ports_drop_before(floor)
        out["drop_before_a_third_of_the_buckets_ms"] = (time.perf_counter() - t0) * 1e3
        after = port.ports_stats()
        out["used_after_drop"] = after["used"]
        checks["capacity_kept"] = after["capacity"] == ps["capacity"]
        checks["first_bucket_after_drop_is_the_floor"] = int(port.ports_buckets()[0]) == floor
        for d, name in ((0, "src_port"), (1, "dst_port")):
            left = np_top_ports(cols[name], weight, ok & (bucket >= np.uint64(floor)))
            checks["after_drop_every_row_%d" % d] = np.array_equal(as_triples(port.top_ports_range(d)), left)
        # the shared decode
        launches = {}
        for name, agg in (("talkers_only", talk), ("talkers_and_ports", both)):
            before = agg.stats()["decode_launches"]
            ingest(agg)
            launches[name] = (agg.stats()["decode_launches"] - before) / len(batches)
        out["decode_launches_per_call"] = launches
        checks["decode_is_shared"] = launches["talkers_only"] == launches["talkers_and_ports"] > 0
        for d, name in ((0, "src_port"), (1, "dst_port")):
            checks["both_enabled_k100_%d" % d] = np.array_equal(as_triples(both.top_ports_range(d, 100)), np_top_ports(cols[name], weight, ok, 100))
            checks["both_enabled_talkers_%d" % d] = both.top_talkers(d, 100).tobytes() == talk.top_talkers(d, 100).tobytes()
        out["checks"] = {k: bool(v) for k, v in checks.items()}
        out["checks_ok"] = all(out["checks"].values())
    print("PORTS_STEP " + json.dumps(out))
    return 0 if out["checks_ok"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="records per fa_ingest_device call")
    ap.add_argument("--rounds", type=int, default=3, help="interleaved ingest rounds per ctx")
    ap.add_argument("--universe-log2", type=int, default=24)
    ap.add_argument("--capacity-log2", type=int, default=0, help="the measured ctx's initial table size (0: the library's default)")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds for the GPU step")
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "port_buckets_run.json"))
    args = ap.parse_args()
    if args.step:
        sys.exit(step(args))
    res = {"config": "framed FlowMessages, Zipf-1.1 over 2^%d addresses, 900 s, key_sets = flows_5m + both sketches (BASELINE config 3), %d records in calls "
                     "of %d, generated in HBM; bucket_secs = %d; one box, one run" % (args.universe_log2, args.records, args.chunk, BUCKET_SECS)}
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--records", str(args.records), "--chunk", str(args.chunk), "--rounds", str(args.rounds),
           "--universe-log2", str(args.universe_log2), "--capacity-log2", str(args.capacity_log2)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        print("the GPU step exceeded its %d s limit: stopping" % args.step_timeout, file=sys.stderr)
        sys.exit(124)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("PORTS_STEP ")]
    if not line:
        sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
        print("the GPU step failed (exit status %d): stopping" % p.returncode, file=sys.stderr)
        sys.exit(p.returncode or 1)
    res.update(json.loads(line[-1][len("PORTS_STEP "):]))
    res["source_hash"] = _pkg.load().source_hash()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("ingest_records_per_s_median", "fold_ns_per_record", "range_all_buckets_k100_ms", "range_one_bucket_k100_ms",
                                          "drop_before_a_third_of_the_buckets_ms", "fa_top_ports_k100_ms", "decode_launches_per_call", "checks_ok")}))
    sys.exit(0 if res["checks_ok"] else 1)


if __name__ == "__main__":
    main()
