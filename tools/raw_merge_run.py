#!/usr/bin/env python3
"""What merging the pending flows_raw parts costs and gives (fa_raw_merge; include/flowagg.h "merging the pending flows_raw
parts"), on tools/raw_lz4_run.py's stream: a device-generated BASELINE config 2 stream kept in HBM, 2^23 records ingested with
fa_ingest_device in calls of 2^21 into TWO contexts with fa_raw_enable, which therefore hold identical parts; one of them merges
before every take.  One child process under a time limit - one box, one session.  Per round (medians of the rounds are reported):
  * fa_raw_merge end to end, and the order and gather device times per row from the library's hipEvents; parts before and after;
  * fa_raw_take of the merged parts beside fa_raw_take of the unmerged ones, into page-locked memory, who goes first alternating;
  * after a second ingest, fa_raw_take_lz4 of both the same way, and the frame bytes both ways;
  * fa_raw_load of the merged frames beside the unmerged ones into fresh contexts with bucketed talkers and ports.
checks_ok: the merged bytes and part descriptions equal those of a third context that built the whole stream as ONE chunk (one
ingest call, chunk_records = the record count), and the ranged top 100 of talkers and ports are equal after either load.
Nothing is gated on the times.  Writes profiles/raw_merge_run.json."""
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
    med = statistics.median

    def generate(agg, i0, m):
        cap = m * 96 + 4096
        d_buf = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_off = torch.empty(m + 1, dtype=torch.int32, device=dev)
        return d_buf, d_off, agg.mock_generate_device(mp, i0, m, d_buf.data_ptr(), cap, d_off.data_ptr()), m

    def folds():
        agg = fa.FlowAgg(**kw)
        agg.talkers_enable(0, bucket_secs=60)
        agg.ports_enable_buckets(0, bucket_secs=60)
        return agg

    def reads(agg):
        t0 = int(mp.t0)
        return [agg.top_talkers(d, 100, lo, hi).tobytes() for d in (0, 1) for lo, hi in ((0, fa.NO_UPPER_BOUND), (t0 + 300, t0 + 600))] + \
               [agg.top_ports_range(d, 100, lo, hi).tobytes() for d in (0, 1) for lo, hi in ((0, fa.NO_UPPER_BOUND), (t0 + 300, t0 + 600))]

    nb, npart = C.c_size_t(), C.c_size_t()

    def take(agg, lz4, host, parts):
        fn = L.fa_raw_take_lz4 if lz4 else L.fa_raw_take
        t0 = time.perf_counter()
        rc = fn(agg._h, host.ctypes.data, host.size, C.byref(nb), parts.ctypes.data, len(parts), C.byref(npart))
        dt = time.perf_counter() - t0
        assert rc == 0, (rc, L.fa_last_error(agg._h))
        return dt, nb.value, npart.value

    # ---- the reference: the whole stream as ONE chunk
    with fa.FlowAgg(framed=True, max_batch_records=n) as one:
        one.raw_enable(n)
        d_buf, d_off, w, m = generate(one, 0, n)
        one.ingest_device(d_buf.data_ptr(), w, d_off.data_ptr(), m)
        one.sync()
        ref_bytes, ref_parts = one.raw_take()
        ref_bytes = ref_bytes.tobytes() if hasattr(ref_bytes, "tobytes") else bytes(ref_bytes)
        del d_buf, d_off
    torch.cuda.empty_cache()

    with fa.FlowAgg(**kw) as um, fa.FlowAgg(**kw) as mg:
        um.raw_enable()
        mg.raw_enable()
        batches = [generate(um, i0, min(chunk, n - i0)) for i0 in range(0, n, chunk)]

        def ingest(agg):
            for d_buf, d_off, w, m in batches:
                agg.ingest_device(d_buf.data_ptr(), w, d_off.data_ptr(), m)
            agg.sync()

        ingest(um)
        pending = um.raw_stats()
        nbytes, nparts = int(pending["pending_bytes"]), int(pending["pending_parts"])
        host = {k: torch.empty(L.fa_lz4_frame_bound(nbytes) + 15 * nparts, dtype=torch.uint8, pin_memory=True).numpy() for k in ("um", "mg")}
        parts = {k: np.zeros(nparts, dtype=fa.RAW_PART_DTYPE) for k in ("um", "mg")}
        t = {k: [] for k in ("merge", "take_um", "take_mg", "lz4_um", "lz4_mg", "load_um", "load_mg")}
        frame_bytes, merged_parts, merged_bytes = {}, 0, 0
        frames = {}
        for r in range(args.rounds):
            order = ("um", "mg") if r % 2 == 0 else ("mg", "um")  # (who goes first alternates)
            for lz4 in (False, True):
                if r or lz4:
                    ingest(um)
                ingest(mg)
                t0 = time.perf_counter()
                mg.raw_merge()
                t["merge"].append(time.perf_counter() - t0)
                for k in order:
                    dt, got, np_got = take(um if k == "um" else mg, lz4, host[k], parts[k])
                    t[("lz4_" if lz4 else "take_") + k].append(dt)
                    if lz4:
                        frame_bytes[k] = got
                        frames[k] = host[k][:got]
                    elif k == "mg":
                        merged_parts, merged_bytes = np_got, got
                        if r == 0:
                            checks["merged_bytes_equal_the_one_chunk_build"] = host[k][:got].tobytes() == ref_bytes
                            checks["merged_part_descriptions_equal_the_one_chunk_build"] = parts[k][:np_got].tobytes() == ref_parts.tobytes()
                    else:
                        assert (got, np_got) == (nbytes, nparts)
            # ---- the load of this round's frames, into fresh contexts
            got = {}
            for k in order:
                with folds() as agg:
                    agg.sync()
                    t0 = time.perf_counter()
                    rc = L.fa_raw_load(agg._h, frames[k].ctypes.data, frames[k].size)
                    t["load_" + k].append(time.perf_counter() - t0)
                    assert rc == 0, (rc, L.fa_last_error(agg._h))
                    got[k] = reads(agg)
            checks["round_%d_ranged_top_100_equal_after_either_load" % r] = got["um"] == got["mg"] and sum(len(x) for x in got["mg"]) > 0
        ms = mg.raw_merge_stats()
    rows = int(ref_parts["rows"].sum())
    out.update(records=n, rows=rows, parts_before=nparts, parts_after=merged_parts, bytes_before=nbytes, bytes_after=merged_bytes,
               merges=ms["merges"], launches_per_merge=ms["launches"] / ms["merges"])
    out["order_ns_per_row"] = ms["order_ns"] / ms["rows"]
    out["gather_ns_per_row"] = ms["gather_ns"] / ms["rows"]
    out["gather_GB_per_s_written"] = ms["bytes_out"] / ms["gather_ns"]
    out["merge_device_ms"] = (ms["order_ns"] + ms["gather_ns"]) / ms["merges"] / 1e6
    for k, v in t.items():
        out[k + "_ms"] = [x * 1e3 for x in v]
        out[k + "_ms_median"] = med(v) * 1e3
    out["merge_ns_per_row"] = med(t["merge"]) * 1e9 / rows
    out["lz4_bytes_unmerged"], out["lz4_bytes_merged"] = frame_bytes["um"], frame_bytes["mg"]
    out["merge_plus_take_ms_median"] = out["merge_ms_median"] + out["take_mg_ms_median"]
    out["merge_plus_lz4_take_ms_median"] = out["merge_ms_median"] + out["lz4_mg_ms_median"]
    out["merge_pays_for_itself_plain_take"] = bool(out["merge_plus_take_ms_median"] < out["take_um_ms_median"])
    out["merge_pays_for_itself_lz4_take"] = bool(out["merge_plus_lz4_take_ms_median"] < out["lz4_um_ms_median"])
    out["merge_pays_for_itself_with_the_load"] = bool(out["merge_plus_lz4_take_ms_median"] + out["load_mg_ms_median"] < out["lz4_um_ms_median"] + out["load_um_ms_median"])
    out["raw_merge_stats"] = ms
    out["checks"] = {k: bool(v) for k, v in checks.items()}
    out["checks_ok"] = all(out["checks"].values()) and len(checks) == 2 + args.rounds
    print("MERGE_STEP " + json.dumps(out))
    return 0 if out["checks_ok"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="records per fa_ingest_device call")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=540, help="seconds for the GPU step")
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_merge_run.json"))
    args = ap.parse_args()
    if args.step:
        sys.exit(step(args))
    res = {"config": "framed FlowMessages, BASELINE config 2 (65 536 AS pairs x 2 ETypes over 900 s), key_sets = flows_5m, %d records in calls of %d, "
                     "generated in HBM; raw chunk 2^20; two contexts with identical parts, one merges before every take; medians of %d rounds; one box, one run"
                     % (args.records, args.chunk, args.rounds)}
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--records", str(args.records), "--chunk", str(args.chunk), "--rounds", str(args.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        print("the GPU step exceeded its %d s limit: stopping" % args.step_timeout, file=sys.stderr)
        sys.exit(124)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("MERGE_STEP ")]
    if not line:
        sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
        print("the GPU step failed (exit status %d): stopping" % p.returncode, file=sys.stderr)
        sys.exit(p.returncode or 1)
    res.update(json.loads(line[-1][len("MERGE_STEP "):]))
    res["source_hash"] = _pkg.load().source_hash()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res.get(k) for k in ("parts_before", "parts_after", "order_ns_per_row", "gather_ns_per_row", "merge_ms_median", "take_um_ms_median",
                                              "take_mg_ms_median", "lz4_um_ms_median", "lz4_mg_ms_median", "lz4_bytes_unmerged", "lz4_bytes_merged",
                                              "load_um_ms_median", "load_mg_ms_median", "checks_ok")}))
    sys.exit(0 if res["checks_ok"] else 1)


if __name__ == "__main__":
    main()
