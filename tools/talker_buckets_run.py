#!/usr/bin/env python3
"""What the time axis of the exact top talkers costs (fa_talkers_enable_buckets, bucket_secs = 60), on tools/talkers_run.py's
stream and by its method: a device-generated Zipf-1.1 stream over 2^24 addresses spanning 900 s (15 buckets), ingested with
fa_ingest_device in calls of 2^21 records.  Two steps, each a child process under its own time limit:
  * plain     fa_talkers_enable: the fold kernel's ns per record (fa_talkers_stats), fa_top_talkers(k = 100);
  * bucketed  fa_talkers_enable_buckets(60): the same two figures, fa_top_talkers_range for 1 of the 15 minutes and for all of
              them, fa_talkers_drop_before of the first 5 minutes.
Checked on the way, all of it part of checks_ok and of the exit status: the bucketed ctx's un-ranged result is the plain ctx's
byte for byte - every row in order, and the first 100 of both directions -, read three times; the range over every bucket is
the un-ranged result in the same sense; a minute's counts add up to the records of that minute; what a drop leaves.  Reads are timed as the median of 5 calls after
one warm-up call.  Writes profiles/talker_buckets_run.json."""
import argparse
import hashlib
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


def timed(call, reps=5):
    call()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def by_key(rows):
    """the rows in key order: two results hold the same groups with the same sums iff these are equal"""
    return rows[np.lexsort((rows["etype"],) + tuple(rows["key"][:, i] for i in range(15, -1, -1)))]


def step(args):
    import torch
    fa = _pkg.load()
    fa.build()
    dev = torch.device("cuda", 0)
    n, chunk = args.records, args.chunk
    mp = fa.mock_params(mode=fa.MOCK_ZIPF, framed=1, seed=3, n_total=n, span_secs=900, zipf_log2_universe=args.universe_log2, zipf_s_x100=110)
    bucketed = args.step == "bucketed"
    out = {}
    with fa.FlowAgg(framed=True, key_sets=7, topk_mode=fa.TOPK_CANDIDATES, topk_capacity_log2=16, max_batch_records=chunk) as agg:
        agg.talkers_enable(args.capacity_log2, BUCKET_SECS if bucketed else 0)
        cap = chunk * 96 + 4096
        d_buf = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_off = torch.empty(chunk + 1, dtype=torch.int32, device=dev)
        for i0 in range(0, n, chunk):
            m = min(chunk, n - i0)
            w = agg.mock_generate_device(mp, i0, m, d_buf.data_ptr(), cap, d_off.data_ptr())
            agg.ingest_device(d_buf.data_ptr(), w, d_off.data_ptr(), m)
            agg.sync()
        st = agg.stats()
        assert st["records_ok"] == n and st["records_bad"] == 0, st
        ts = agg.talkers_stats()
        out["talkers_stats"] = ts
        out["fold_ns_per_record"] = ts["fold_ns_total"] / max(1, ts["records_folded"])
        top = agg.top_talkers(0, 100)
        out["top100_sha256"] = hashlib.sha256(top.tobytes() + agg.top_talkers(1, 100).tobytes()).hexdigest()
        ordered = agg.top_talkers(0)
        every = by_key(ordered)
        out["groups"] = int(len(every))
        out["groups_sha256"] = hashlib.sha256(every.tobytes()).hexdigest()
        out["rows_in_order_sha256"] = hashlib.sha256(ordered.tobytes()).hexdigest()
        out["weight_inversions"] = int((ordered["weight"][1:] > ordered["weight"][:-1]).sum())
        # (an order that changes from call to call must not pass by luck)
        out["reads_repeat"] = all(agg.top_talkers(0).tobytes() == ordered.tobytes() and agg.top_talkers(0, 100).tobytes() == top.tobytes() for _ in range(3))
        out["top_talkers_k100_ms"] = timed(lambda: agg.top_talkers(0, 100))
        if bucketed:
            b = agg.talkers_buckets()
            out["buckets"] = int(len(b))
            lo, end = int(b[0]), int(b[-1]) + BUCKET_SECS
            mid = int(b[len(b) // 2])
            out["range_all_buckets_k100_ms"] = timed(lambda: agg.top_talkers(0, 100, lo, end))
            out["range_one_bucket_k100_ms"] = timed(lambda: agg.top_talkers(0, 100, mid, mid + BUCKET_SECS))
            checks = {"range_over_every_bucket_is_the_unranged_result": all(agg.top_talkers(0, 0, lo, end).tobytes() == ordered.tobytes() for _ in range(3)),
                      "range_over_every_bucket_top100": agg.top_talkers(0, 100, lo, end).tobytes() == top.tobytes(),
                      "no_weight_inversion": out["weight_inversions"] == 0, "reads_repeat": out["reads_repeat"]}
            per_minute = [int(agg.top_talkers(0, 0, int(t), int(t) + BUCKET_SECS)["count"].sum()) for t in b]
            checks["minutes_add_up_to_the_records"] = sum(per_minute) == n
            floor = int(b[min(5, len(b) - 1)])
            t0 = time.perf_counter()
            agg.talkers_drop_before(floor)
            out["drop_before_5_buckets_ms"] = (time.perf_counter() - t0) * 1e3
            after = agg.talkers_stats()
            out["used_after_drop"] = after["used"]
            checks["first_bucket_after_drop_is_the_floor"] = int(agg.talkers_buckets()[0]) == floor
            checks["records_left_after_drop"] = int(agg.top_talkers(0)["count"].sum()) == sum(per_minute[min(5, len(b) - 1):])
            out["records_per_minute"] = per_minute
            out["checks"] = {k: bool(v) for k, v in checks.items()}
            out["checks_ok"] = all(out["checks"].values())
    print("BUCKETS_STEP " + json.dumps(out))
    return 0 if (not bucketed or out["checks_ok"]) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="records per fa_ingest_device call")
    ap.add_argument("--universe-log2", type=int, default=24)
    ap.add_argument("--capacity-log2", type=int, default=0, help="the initial table size (0: the library's default)")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--step", choices=["plain", "bucketed"], help="(internal) run one step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "talker_buckets_run.json"))
    args = ap.parse_args()
    if args.step:
        sys.exit(step(args))
    res = {"config": "tools/talkers_run.py's stream: framed FlowMessages, Zipf-1.1 over 2^%d addresses, 900 s, key_sets = flows_5m + both sketches, "
                     "%d records in calls of %d, generated in HBM; bucket_secs = %d" % (args.universe_log2, args.records, args.chunk, BUCKET_SECS)}
    for name in ("plain", "bucketed"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--records", str(args.records), "--chunk", str(args.chunk),
               "--universe-log2", str(args.universe_log2), "--capacity-log2", str(args.capacity_log2)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print("step %s exceeded its %d s limit: stopping" % (name, args.step_timeout), file=sys.stderr)
            sys.exit(124)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("BUCKETS_STEP ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
            print("step %s failed (exit status %d): stopping" % (name, p.returncode), file=sys.stderr)
            sys.exit(p.returncode or 1)
        res[name] = json.loads(line[-1][len("BUCKETS_STEP "):])
    res["fold_ns_per_record_plain"] = res["plain"]["fold_ns_per_record"]
    res["fold_ns_per_record_bucketed"] = res["bucketed"]["fold_ns_per_record"]
    res["slots_plain"] = res["plain"]["talkers_stats"]["used"]
    res["slots_bucketed"] = res["bucketed"]["talkers_stats"]["used"]
    res["unranged_groups_equal"] = res["plain"]["groups_sha256"] == res["bucketed"]["groups_sha256"]
    res["unranged_rows_in_order_equal"] = res["plain"]["rows_in_order_sha256"] == res["bucketed"]["rows_in_order_sha256"]
    res["top100_order_equal"] = res["plain"]["top100_sha256"] == res["bucketed"]["top100_sha256"]
    res["checks_ok"] = bool(res["bucketed"]["checks_ok"] and res["unranged_groups_equal"] and res["unranged_rows_in_order_equal"] and res["top100_order_equal"]
                            and res["plain"]["weight_inversions"] == 0 and res["plain"]["reads_repeat"])
    res["source_hash"] = _pkg.load().source_hash()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res[k] for k in ("fold_ns_per_record_plain", "fold_ns_per_record_bucketed", "slots_plain", "slots_bucketed", "checks_ok", "top100_order_equal")}))
    sys.exit(0 if res["checks_ok"] else 1)


if __name__ == "__main__":
    main()
