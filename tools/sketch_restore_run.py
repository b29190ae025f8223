#!/usr/bin/env python3
"""What rebuilding the address sketches and the distinct-address sets from flows_raw parts costs (fa_sketch_fold_columns_device,
fa_raw_restore; include/flowagg.h "the sketches from columns and from parts"), on tools/talkers_run.py's stream: BASELINE config
3's shape - framed FlowMessages, Zipf-1.1 addresses over 2^24, key_sets = flows_5m + both sketches - generated in HBM, 2^23
records in calls of 2^21.  Per top-k contract (exact, candidates) one ctx with fa_raw_enable ingests the stream and delivers its
parts as LZ4 frames (fa_raw_take_lz4) into page-locked memory; the raw chunk is the ingest call, so that a part is a batch.  One
child process under a time limit - one box, one session:
  * the fold kernel's ns per record from the library's hipEvents (fa_sketch_fold_stats.fold_ns) over the parts' columns in HBM
    (fa_raw_columns_device), with the workgroups' LDS cache and without it (FA_SKETCH_LDS=0), each into a fresh ctx each round;
  * fa_raw_restore of all key sets, end to end (ONE call: copy in, decode, header check, unpack, both folds, settle), beside
    fa_raw_load_rollup of the same frames (flows_5m alone: what the chain could do before) and beside fa_ingest_device of the same
    records' wire bytes (already in HBM: no copy in), each into a fresh ctx, interleaved round by round;
  * checks_ok: every read of the restored ctx - flows_5m, both sketches, both top-100 rankings, in the candidates mode the
    thresholds and the candidates held - equals the ingesting ctx's; the folds from columns leave the same sketches and rankings,
    with and without the cache.  (Candidates mode: the rankings are compared when every part is one ingest call's records - the
    contract is per batch; candidates_batches_match says whether they were.)
Medians of the rounds.  Nothing is gated on the times.  Writes profiles/sketch_restore_run.json."""
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

KS3 = 1 | 2 | 4  # BASELINE config 3: flows_5m + both sketches
SRC, DST = 2, 4


def step(args):
    import torch
    fa = _pkg.load()
    fa.build()
    L = fa.lib()
    dev = torch.device("cuda", 0)
    n, chunk = args.records, args.chunk
    mp = fa.mock_params(mode=fa.MOCK_ZIPF, framed=1, seed=3, n_total=n, span_secs=900, zipf_log2_universe=args.universe_log2, zipf_s_x100=110)
    out, checks = {"records": n, "chunk_records": chunk}, {}
    cap = chunk * 96 + 4096
    batches = []

    def reads(agg, candidates):
        r = [agg.read_window().tobytes(), agg.cms_read(SRC).tobytes(), agg.cms_read(DST).tobytes()]
        ranks = [agg.topk(SRC, 100).tobytes(), agg.topk(DST, 100).tobytes()]
        if candidates:
            st = agg.stats()
            ranks.append(json.dumps([st[k] for k in ("topk_theta_src", "topk_theta_dst", "topk_candidates_src", "topk_candidates_dst")]).encode())
        return r, ranks

    for mode in ("exact", "candidates"):
        candidates = mode == "candidates"
        kw = dict(framed=True, max_batch_records=chunk, key_sets=KS3, topk_mode=fa.TOPK_CANDIDATES if candidates else fa.TOPK_EXACT,
                  topk_capacity_log2=16 if candidates else args.universe_log2 - 1)
        res = {}
        with fa.FlowAgg(**kw) as src:
            src.raw_enable(chunk)
            if not batches:
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
            want, want_ranks = reads(src, candidates)
            rows = int(parts["rows"].sum())
            match = [int(x) for x in parts["rows"]] == [m for _, _, _, m in batches]  # every part is one ingest call's records
        res.update(rows=rows, parts=nparts, lz4_bytes=int(nb.value), wire_bytes=int(sum(b[2] for b in batches)), candidates_batches_match=match)
        compare_ranks = match or not candidates

        def same(agg, what):
            got, ranks = reads(agg, candidates)
            checks["%s_%s_sketches" % (mode, what)] = got[1:] == want[1:]
            if what.startswith("restore") or what.startswith("ingest"):
                checks["%s_%s_flows_5m" % (mode, what)] = got[0] == want[0]
            if compare_ranks:
                checks["%s_%s_rankings" % (mode, what)] = ranks == want_ranks
            return ranks

        # ---- the fold kernel alone, over the parts' columns in HBM, with and without the LDS cache
        fold = {"cache": [], "no_cache": []}
        with fa.FlowAgg(framed=True) as holder:
            cols, nrows = holder.raw_columns(frames)
            assert nrows == rows
            for r in range(args.rounds):
                ranks = {}
                for which in (("cache", "no_cache") if r % 2 == 0 else ("no_cache", "cache")):
                    if which == "no_cache":
                        os.environ["FA_SKETCH_LDS"] = "0"  # (read at the ctx's first sketch fold)
                    else:
                        os.environ.pop("FA_SKETCH_LDS", None)
                    with fa.FlowAgg(**kw) as agg:
                        agg.sketch_fold_columns(cols, rows)
                        s = agg.sketch_fold_stats()
                        fold[which].append(s["fold_ns"] / s["records_folded"])
                        checks["%s_fold_%s_round_%d_rows" % (mode, which, r)] = s["records_folded"] == rows and s["batches"] == (rows + chunk - 1) // chunk
                        ranks[which] = same(agg, "fold_%s_round_%d" % (which, r))
                os.environ.pop("FA_SKETCH_LDS", None)
                checks["%s_fold_round_%d_cache_and_no_cache_rank_alike" % (mode, r)] = ranks["cache"] == ranks["no_cache"]
        res["fold_kernel_ns_per_record"] = {k: statistics.median(v) for k, v in fold.items()}
        res["fold_kernel_ns_per_record_rounds"] = fold
        res["cache_speedup"] = res["fold_kernel_ns_per_record"]["no_cache"] / res["fold_kernel_ns_per_record"]["cache"]

        # ---- end to end: restore (everything), load_rollup (flows_5m alone), ingest of the wire bytes
        t = {"restore": [], "load_rollup": [], "ingest": []}
        stats = None
        order = ["restore", "load_rollup", "ingest"]
        for r in range(args.rounds):
            for which in order[r % 3:] + order[:r % 3]:  # (who goes first rotates)
                with fa.FlowAgg(**kw) as agg:
                    agg.sync()
                    t0 = time.perf_counter()
                    if which == "restore":
                        rc = L.fa_raw_restore(agg._h, frames.ctypes.data, frames.size, 0, 0)
                        t[which].append(time.perf_counter() - t0)
                        assert rc == 0, (rc, L.fa_last_error(agg._h))
                        stats = dict(agg.raw_load_stats(), **{"rollup_" + k: v for k, v in agg.rollup_stats().items()}, **{"sketch_" + k: v for k, v in agg.sketch_fold_stats().items()})
                        checks["%s_restore_round_%d_rows" % (mode, r)] = stats["sketch_records_folded"] == rows and stats["rollup_records_folded"] == rows
                        same(agg, "restore_round_%d" % r)
                    elif which == "load_rollup":
                        rc = L.fa_raw_load_rollup(agg._h, frames.ctypes.data, frames.size, 0, 0)
                        t[which].append(time.perf_counter() - t0)
                        assert rc == 0, (rc, L.fa_last_error(agg._h))
                        checks["%s_load_rollup_round_%d_flows_5m" % (mode, r)] = agg.read_window().tobytes() == want[0] and not agg.cms_read(SRC).any()
                    else:
                        ingest(agg)
                        t[which].append(time.perf_counter() - t0)
                        same(agg, "ingest_round_%d" % r)
        for k, v in t.items():
            res[k + "_ms"] = [x * 1e3 for x in v]
            res[k + "_ms_median"] = statistics.median(v) * 1e3
        res["restore_over_ingest"] = statistics.median(t["restore"]) / statistics.median(t["ingest"])
        res["restore_over_load_rollup"] = statistics.median(t["restore"]) / statistics.median(t["load_rollup"])
        res["restore_ns_per_row"] = statistics.median(t["restore"]) * 1e9 / rows
        res["stats_last_restore"] = stats
        res["device_ms_of_a_restore"] = {k: stats[k] / 1e6 for k in ("decode_ns", "unpack_ns", "fold_ns", "rollup_fold_ns", "sketch_fold_ns")}
        out[mode] = res
    out["checks"] = {k: bool(v) for k, v in checks.items()}
    out["checks_ok"] = all(out["checks"].values())
    print("SKETCH_STEP " + json.dumps(out))
    return 0 if out["checks_ok"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="records per fa_ingest_device call, per raw chunk and per batch")
    ap.add_argument("--universe-log2", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds")
    ap.add_argument("--step-timeout", type=int, default=540, help="seconds for the GPU step")
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sketch_restore_run.json"))
    args = ap.parse_args()
    if args.step:
        sys.exit(step(args))
    res = {"config": "BASELINE config 3's shape: framed FlowMessages, Zipf-1.1 over 2^%d addresses, key_sets = flows_5m + both sketches (default 4 x 2^20), "
                     "%d records in calls of %d, generated in HBM; raw chunk = the call; one box, one run" % (args.universe_log2, args.records, args.chunk)}
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--records", str(args.records), "--chunk", str(args.chunk), "--universe-log2", str(args.universe_log2),
           "--rounds", str(args.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        print("the GPU step exceeded its %d s limit: stopping" % args.step_timeout, file=sys.stderr)
        sys.exit(124)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("SKETCH_STEP ")]
    if not line:
        sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
        print("the GPU step failed (exit status %d): stopping" % p.returncode, file=sys.stderr)
        sys.exit(p.returncode or 1)
    res.update(json.loads(line[-1][len("SKETCH_STEP "):]))
    res["source_hash"] = _pkg.load().source_hash()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({m: {k: res[m].get(k) for k in ("rows", "fold_kernel_ns_per_record", "restore_ms_median", "load_rollup_ms_median", "ingest_ms_median")}
                      for m in ("exact", "candidates")} | {"checks_ok": res["checks_ok"]}))
    sys.exit(0 if res["checks_ok"] else 1)


if __name__ == "__main__":
    main()
