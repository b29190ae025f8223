#!/usr/bin/env python3
"""What loading flows_raw parts back costs (fa_raw_load; include/flowagg.h "loading flows_raw parts"), on tools/raw_lz4_run.py's
stream: a device-generated BASELINE config 2 stream kept in HBM, 2^23 records in calls of 2^21.  One ctx with bucketed talkers
(60 s), bucketed ports (60 s) and fa_raw_enable ingests it and delivers its parts as LZ4 frames (fa_raw_take_lz4) into
page-locked memory.  One child process under a time limit - one box, one session:
  * fa_raw_load of those frames, end to end (ONE call: copy in, decode, header check, unpack, fold), into a fresh ctx with the
    same folds each round;
  * beside it the route without this feature: fa_ingest_device of the same records' wire bytes (already in HBM: no copy in)
    into a fresh ctx with the same folds, interleaved round by round;
  * the decode kernel's ns per decoded byte, the unpack kernel's ns per row and the folds' time from the library's hipEvents;
    beside the decode the host twin fa_lz4_decode and, where the machine has liblz4, LZ4F_decompress over the first frame;
  * checks_ok: the loaded ctx's ranged top 100 of talkers and ports, both directions, over the whole axis and over a middle
    range, equal the ingesting ctx's.
Nothing is gated on the times.  Writes profiles/raw_load_run.json."""
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

sys.path.insert(0, os.path.join(ROOT, "tools"))
from raw_lz4_run import liblz4, liblz4_decode  # noqa: E402


def step(args):
    import torch
    fa = _pkg.load()
    fa.build()
    L = fa.lib()
    dev = torch.device("cuda", 0)
    n, chunk = args.records, args.chunk
    mp = fa.mock_params(mode=fa.MOCK_ASPAIRS, framed=1, seed=3, n_total=n, span_secs=900)
    kw = dict(framed=True, max_batch_records=chunk)
    out, checks = {}, {}

    def folds(raw=False):
        agg = fa.FlowAgg(**kw)
        agg.talkers_enable(0, bucket_secs=60)
        agg.ports_enable_buckets(0, bucket_secs=60)
        if raw:
            agg.raw_enable()
        return agg

    def reads(agg):
        t0 = int(mp.t0)
        return [agg.top_talkers(d, 100, lo, hi).tobytes() for d in (0, 1) for lo, hi in ((0, fa.NO_UPPER_BOUND), (t0 + 300, t0 + 600))] + \
               [agg.top_ports_range(d, 100, lo, hi).tobytes() for d in (0, 1) for lo, hi in ((0, fa.NO_UPPER_BOUND), (t0 + 300, t0 + 600))]

    with folds(raw=True) as src:
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
    out.update(records=n, rows=rows, parts=nparts, plain_bytes=nbytes, lz4_bytes=int(nb.value), wire_bytes=int(sum(b[2] for b in batches)))
    t_load, t_ingest, stats = [], [], None
    for r in range(args.rounds):
        for which in (("load", "ingest") if r % 2 == 0 else ("ingest", "load")):  # (who goes first alternates)
            with folds() as agg:
                agg.sync()
                t0 = time.perf_counter()
                if which == "load":
                    rc = L.fa_raw_load(agg._h, frames.ctypes.data, frames.size)
                    t_load.append(time.perf_counter() - t0)
                    assert rc == 0, (rc, L.fa_last_error(agg._h))
                    stats = agg.raw_load_stats()
                else:
                    ingest(agg)
                    t_ingest.append(time.perf_counter() - t0)
                got = reads(agg)
                checks["%s_round_%d_equals_the_source" % (which, r)] = got == want
                checks["%s_round_%d_rows" % (which, r)] = agg.talkers_stats()["records_folded"] == rows
    out["load_ms"] = [t * 1e3 for t in t_load]
    out["ingest_ms"] = [t * 1e3 for t in t_ingest]
    out["load_ms_median"] = statistics.median(t_load) * 1e3
    out["ingest_ms_median"] = statistics.median(t_ingest) * 1e3
    out["load_ns_per_row"] = statistics.median(t_load) * 1e9 / rows
    out["ingest_ns_per_record"] = statistics.median(t_ingest) * 1e9 / n
    out["load_is_faster_than_reingesting"] = bool(statistics.median(t_load) < statistics.median(t_ingest))
    out["raw_load_stats_last_round"] = stats
    out["decode_kernel_ns_per_decoded_byte"] = stats["decode_ns"] / stats["bytes_decoded"]
    out["decode_kernel_GB_per_s_decoded"] = stats["bytes_decoded"] / stats["decode_ns"]
    out["unpack_kernel_ns_per_row"] = stats["unpack_ns"] / stats["rows_loaded"]
    out["fold_ns_per_row"] = stats["fold_ns"] / stats["rows_loaded"]
    out["device_ms_of_a_load"] = {k: stats[k] / 1e6 for k in ("decode_ns", "unpack_ns", "fold_ns")}
    # ---- the host twin and liblz4 over the first frame
    first = frames[int(parts["offset"][0]):int(parts["offset"][0]) + int(parts["bytes"][0])]
    t0 = time.perf_counter()
    dec = fa.lz4_decode(first.tobytes())
    out["host_twin_ns_per_decoded_byte"] = (time.perf_counter() - t0) * 1e9 / len(dec)
    lz = liblz4()
    if lz is not None:
        t0 = time.perf_counter()
        ref = liblz4_decode(lz, first, len(dec))
        out["liblz4_ns_per_decoded_byte"] = (time.perf_counter() - t0) * 1e9 / len(dec)
        checks["host_twin_equals_liblz4"] = ref.tobytes() == dec
    else:
        out["liblz4_ns_per_decoded_byte"] = None
    out["checks"] = {k: bool(v) for k, v in checks.items()}
    out["checks_ok"] = all(out["checks"].values())
    print("LOAD_STEP " + json.dumps(out))
    return 0 if out["checks_ok"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="records per fa_ingest_device call")
    ap.add_argument("--rounds", type=int, default=3, help="interleaved loads and re-ingests")
    ap.add_argument("--step-timeout", type=int, default=540, help="seconds for the GPU step")
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_load_run.json"))
    args = ap.parse_args()
    if args.step:
        sys.exit(step(args))
    res = {"config": "framed FlowMessages, BASELINE config 2 (65 536 AS pairs x 2 ETypes over 900 s), %d records in calls of %d, generated in HBM; "
                     "bucketed talkers and ports (60 s), default capacities; raw chunk 2^20; one box, one run" % (args.records, args.chunk)}
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--records", str(args.records), "--chunk", str(args.chunk), "--rounds", str(args.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        print("the GPU step exceeded its %d s limit: stopping" % args.step_timeout, file=sys.stderr)
        sys.exit(124)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("LOAD_STEP ")]
    if not line:
        sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
        print("the GPU step failed (exit status %d): stopping" % p.returncode, file=sys.stderr)
        sys.exit(p.returncode or 1)
    res.update(json.loads(line[-1][len("LOAD_STEP "):]))
    res["source_hash"] = _pkg.load().source_hash()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res.get(k) for k in ("rows", "lz4_bytes", "load_ms_median", "ingest_ms_median", "decode_kernel_ns_per_decoded_byte", "host_twin_ns_per_decoded_byte",
                                              "liblz4_ns_per_decoded_byte", "unpack_kernel_ns_per_row", "fold_ns_per_row", "checks_ok")}))
    sys.exit(0 if res["checks_ok"] else 1)


if __name__ == "__main__":
    main()
