#!/usr/bin/env python3
"""What the flows_raw parts cost (fa_raw_enable; include/flowagg.h "flows_raw parts built on the device"), by
tools/port_buckets_run.py's method: a device-generated BASELINE config 2 stream (65 536 AS pairs x 2 ETypes, key_sets = flows_5m)
kept in HBM and ingested with fa_ingest_device in calls of 2^21 records.  One child process under a time limit - one box, one
session:
  * fa_ingest_device records/s of a ctx WITHOUT the second pass and of a ctx WITH the raw pass, interleaved round by round over
    the same buffers (the pending parts are taken in HBM, untimed, after each round);
  * the build's ns per record, split into order (compaction, radix sort, part list) and gather, from the library's hipEvents
    (the child runs with FA_VERBOSE and the ctx reports both sums when it is destroyed);
  * fa_raw_take of one round's parts into page-locked memory, GB/s;
  * beside these, the route to a flows_raw row without this feature: fa_decode of one call's records into fa_flow_row, rows/s.
Nothing is gated on the times.  checks_ok - one call's taken parts equal to spill.native_from_rows over the columns of the
ctx's own fa_decode_device, chunk by chunk - also sets the exit status.  Writes profiles/raw_parts_run.json."""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkg  # noqa: E402
import numpy as np  # noqa: E402

COLUMNS = (("time_received", np.uint64, 1), ("time_flow_start", np.uint64, 1), ("sampling_rate", np.uint64, 1), ("bytes", np.uint64, 1),
           ("packets", np.uint64, 1), ("sequence_num", np.uint32, 1), ("src_as", np.uint32, 1), ("dst_as", np.uint32, 1), ("etype", np.uint32, 1),
           ("proto", np.uint32, 1), ("src_port", np.uint32, 1), ("dst_port", np.uint32, 1), ("sampler_address", np.uint8, 16),
           ("src_addr", np.uint8, 16), ("dst_addr", np.uint8, 16), ("status", np.uint8, 1))
RAW_CHUNK = 1 << 20  # fa_raw_enable's default chunk


def step(args):
    import torch
    fa = _pkg.load()
    fa.build()
    dev = torch.device("cuda", 0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    n, chunk = args.records, args.chunk
    mp = fa.mock_params(mode=fa.MOCK_ASPAIRS, framed=1, seed=3, n_total=n, span_secs=900)
    kw = dict(framed=True, max_batch_records=chunk)
    out, checks = {}, {}
    with fa.FlowAgg(**kw) as none, fa.FlowAgg(**kw) as raw, fa.FlowAgg(**kw) as chk:
        raw.raw_enable()
        chk.raw_enable()
        cap = chunk * 96 + 4096
        batches = []
        for i0 in range(0, n, chunk):
            m = min(chunk, n - i0)
            d_buf = torch.empty(cap, dtype=torch.uint8, device=dev)
            d_off = torch.empty(chunk + 1, dtype=torch.int32, device=dev)
            w = none.mock_generate_device(mp, i0, m, d_buf.data_ptr(), cap, d_off.data_ptr())
            batches.append((d_buf, d_off, w, m))

        # the check: the first call's parts against the numpy encoder over the same call's decoded columns
        d_buf, d_off, w, m = batches[0]
        c = none.decode_device(d_buf.data_ptr(), w, d_off.data_ptr(), m)
        none.sync()
        rows = np.zeros(m, dtype=fa.FLOW_ROW_DTYPE)
        for name, dt, width in COLUMNS:
            a = np.zeros((m, width) if width > 1 else m, dtype=dt)
            assert hip.hipMemcpy(a.ctypes.data, getattr(c, name), a.nbytes, 2) == 0  # hipMemcpyDeviceToHost
            rows[name] = a
        chk.ingest_device(d_buf.data_ptr(), w, d_off.data_ptr(), m)
        data, parts = chk.raw_take()
        want = b"".join(fa.spill.native_from_rows(rows[a:a + RAW_CHUNK]) for a in range(0, m, RAW_CHUNK))
        checks["first_call_parts_equal_numpy"] = data == want
        checks["part_list"] = int(parts["rows"].sum()) == int((rows["status"] == 0).sum()) and int(parts["bytes"].sum()) == len(data)
        out["first_call"] = {"records": m, "parts": int(len(parts)), "bytes": len(data)}

        def ingest(agg):
            t0 = time.perf_counter()
            for d_buf, d_off, w, m in batches:
                agg.ingest_device(d_buf.data_ptr(), w, d_off.data_ptr(), m)
            agg.sync()
            return n / (time.perf_counter() - t0)
        rates = {"none": [], "raw": []}
        for _ in range(args.rounds):
            for name, agg in (("none", none), ("raw", raw)):
                rates[name].append(ingest(agg))
            if _ + 1 < args.rounds:
                raw.raw_take_device()  # (untimed: the next round starts with an empty image)
        out["ingest_records_per_s_without_the_pass"] = rates["none"]
        out["ingest_records_per_s_with_the_raw_pass"] = rates["raw"]
        out["ingest_records_per_s_median"] = {k: statistics.median(v) for k, v in rates.items()}
        st = raw.raw_stats()
        out["raw_stats"] = st
        out["build_ns_per_record"] = st["build_ns_total"] / max(1, st["records_in"])
        checks["rows_out"] = st["rows_out"] + st["records_bad"] == st["records_in"] == args.rounds * n
        # the last round's parts into page-locked memory
        pinned = torch.empty(st["pending_bytes"], dtype=torch.uint8, pin_memory=True).numpy()
        t0 = time.perf_counter()
        data, parts = raw.raw_take(out=pinned)
        dt = time.perf_counter() - t0
        out["take_pinned"] = {"bytes": int(len(data)), "parts": int(len(parts)), "ms": dt * 1e3, "GB_per_s": len(data) / dt / 1e9}
        checks["take_is_whole"] = len(data) == st["pending_bytes"] and len(parts) == st["pending_parts"]

        # without the feature: fa_decode of one call's records into fa_flow_row (sixteen pageable copies and a host gather per chunk)
        hb, ho = fa.mock_generate_host(mp, 0, batches[0][3])
        none.decode(hb, ho)
        t0 = time.perf_counter()
        hrows = none.decode(hb, ho)
        out["fa_decode_rows_per_s"] = len(hrows) / (time.perf_counter() - t0)
        out["checks"] = {k: bool(v) for k, v in checks.items()}
        out["checks_ok"] = all(out["checks"].values())
    print("RAW_STEP " + json.dumps(out))
    return 0 if out["checks_ok"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="records per fa_ingest_device call")
    ap.add_argument("--rounds", type=int, default=3, help="interleaved ingest rounds per ctx")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds for the GPU step")
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_parts_run.json"))
    args = ap.parse_args()
    if args.step:
        sys.exit(step(args))
    res = {"config": "framed FlowMessages, BASELINE config 2 (65 536 AS pairs x 2 ETypes over 900 s), key_sets = flows_5m, %d records in calls of %d, "
                     "generated in HBM; raw chunk 2^20; one box, one run" % (args.records, args.chunk)}
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--records", str(args.records), "--chunk", str(args.chunk), "--rounds", str(args.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout, env=dict(os.environ, FA_VERBOSE="1"))
    except subprocess.TimeoutExpired:
        print("the GPU step exceeded its %d s limit: stopping" % args.step_timeout, file=sys.stderr)
        sys.exit(124)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RAW_STEP ")]
    if not line:
        sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
        print("the GPU step failed (exit status %d): stopping" % p.returncode, file=sys.stderr)
        sys.exit(p.returncode or 1)
    res.update(json.loads(line[-1][len("RAW_STEP "):]))
    # the measured ctx's report (the one that saw the most records): order and gather, hipEvent sums
    reports = [tuple(int(x) for x in mt.groups()) for mt in re.finditer(r"raw parts: (\d+) records in (\d+) chunks, order (\d+) ns, gather (\d+) ns", p.stderr)]
    if reports:
        recs, chunks, order, gather = max(reports)
        res["order_ns_per_record"] = order / max(1, recs)
        res["gather_ns_per_record"] = gather / max(1, recs)
    res["source_hash"] = _pkg.load().source_hash()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res.get(k) for k in ("ingest_records_per_s_median", "build_ns_per_record", "order_ns_per_record", "gather_ns_per_record", "take_pinned",
                                              "fa_decode_rows_per_s", "checks_ok")}))
    sys.exit(0 if res["checks_ok"] else 1)


if __name__ == "__main__":
    main()
