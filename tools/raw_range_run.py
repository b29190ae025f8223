#!/usr/bin/env python3
"""What a ranged restore of flows_raw parts costs beside the whole one (fa_raw_restore_range, fa_raw_restore; include/flowagg.h
"ranged loads of flows_raw parts"), on tools/sketch_restore_run.py's stream: BASELINE config 3's shape - framed FlowMessages,
Zipf-1.1 addresses over 2^24, key_sets = flows_5m + both sketches - generated in HBM, 2^23 records over 900 s of ONE Date.  One ctx
with fa_raw_enable ingests the stream, merges its parts (fa_raw_merge: one sorted part) and delivers it as one LZ4 frame into
page-locked memory.  One child process under a time limit - one box, one session:
  * fa_raw_restore of the whole frame and fa_raw_restore_range for the ranges that hold 1/64, 1/8, 1/2 and all of the rows, each
    into a fresh ctx (so each pays the allocation of its buffers, the decoded image's slots included), interleaved round by round,
    who goes first rotating; wall clock around the one call;
  * per range: the blocks decoded, the three stage times (fa_raw_range_stats: hipEvent times of stage A's kernels, of
    raw_range_kernel, of the decode launches of stages B and C), raw_range_kernel's ns per row, the rows loaded;
  * checks_ok: in every round every read of the ranged ctx - flows_5m, both sketches, both top-100 rankings - equals a twin's that
    folded rows [r_lo, r_hi) of the part's columns (fa_raw_columns_device, sliced by numpy.searchsorted over the TimeReceived column
    the HOST decoder delivers: nothing of the ranged door takes part in the twin); the whole restore equals the ingesting ctx.
  * required: the 1/64 range's median is below the FASTEST round of the whole restore.  The other fractions, and the full range
    against the whole restore (it pays two more waits and the scan), are recorded, not gated.
Writes profiles/raw_range_run.json."""
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
NO_UPPER = 0xFFFFFFFF
FRACTIONS = (("1/64", 64), ("1/8", 8), ("1/2", 2), ("all", 1))
COL_WIDTH = dict(time_received=8, time_flow_start=8, sampling_rate=8, bytes=8, packets=8, sequence_num=4, src_as=4, dst_as=4, etype=4, proto=4, src_port=4, dst_port=4,
                 sampler_address=16, src_addr=16, dst_addr=16, status=1)


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
    kw = dict(framed=True, max_batch_records=chunk, key_sets=KS3, topk_capacity_log2=args.universe_log2 - 1)

    def reads(agg):
        return [agg.read_window().tobytes(), agg.cms_read(SRC).tobytes(), agg.cms_read(DST).tobytes(), agg.topk(SRC, 100).tobytes(), agg.topk(DST, 100).tobytes()]

    with fa.FlowAgg(**kw) as src:
        src.raw_enable(chunk)
        for i0 in range(0, n, chunk):
            m = min(chunk, n - i0)
            d_buf = torch.empty(cap, dtype=torch.uint8, device=dev)
            d_off = torch.empty(chunk + 1, dtype=torch.int32, device=dev)
            w = src.mock_generate_device(mp, i0, m, d_buf.data_ptr(), cap, d_off.data_ptr())
            src.ingest_device(d_buf.data_ptr(), w, d_off.data_ptr(), m)
        src.sync()
        src.raw_merge()
        pending = src.raw_stats()
        nbytes, nparts = int(pending["pending_bytes"]), int(pending["pending_parts"])
        assert nparts == 1, "the stream lies in one Date: one merged part"
        h_frames = torch.empty(L.fa_lz4_frame_bound(nbytes) + 15 * nparts, dtype=torch.uint8, pin_memory=True).numpy()
        parts = np.zeros(nparts, dtype=fa.RAW_PART_DTYPE)
        nb, npart = C.c_size_t(), C.c_size_t()
        rc = L.fa_raw_take_lz4(src._h, h_frames.ctypes.data, h_frames.size, C.byref(nb), parts.ctypes.data, nparts, C.byref(npart))
        assert rc == 0 and npart.value == nparts, rc
        frames = h_frames[:nb.value]
        want_whole = reads(src)
        rows = int(parts["rows"].sum())
    out.update(rows=rows, lz4_bytes=int(nb.value), part_bytes=nbytes)

    # ---- the ranges, from the TimeReceived column as the HOST decoder delivers it
    part = np.frombuffer(fa.lz4_decode(frames.tobytes()), dtype=np.uint8)
    start = 1 + len(fa.schema.encode_varint(rows)) + (2 + 4 + 4) + 2 * rows + (2 + 12 + 8)  # behind the block's and Date's headers, the Dates, TimeReceived's header
    t = np.frombuffer(part[start:start + 4 * rows].tobytes(), dtype="<u4")
    assert (np.diff(t.astype(np.int64)) >= 0).all() and len(np.unique(t // 86400)) == 1
    del part
    ranges = {}
    for name, div in FRACTIONS:
        if div == 1:
            lo, hi = 0, NO_UPPER
        else:  # the seconds around the middle of the part that hold rows / div rows, as nearly as whole seconds can
            lo = int(t[rows // 2 - rows // (2 * div)])
            hi = int(t[min(rows - 1, rows // 2 + rows // (2 * div))])
        r_lo = int(np.searchsorted(t, lo, side="left"))
        r_hi = rows if hi == NO_UPPER else int(np.searchsorted(t, hi, side="left"))
        ranges[name] = dict(t_lo=lo, t_hi=hi, r_lo=r_lo, r_hi=r_hi, rows=r_hi - r_lo, fraction=(r_hi - r_lo) / rows)

    # ---- the twins: rows [r_lo, r_hi) of the part's columns through the folds from columns
    with fa.FlowAgg(framed=True) as holder:
        cols, nrows = holder.raw_columns(frames)
        assert nrows == rows
        for name, r in ranges.items():
            sl = fa.Columns()
            for f, width in COL_WIDTH.items():
                setattr(sl, f, getattr(cols, f) + r["r_lo"] * width)
            with fa.FlowAgg(**kw) as twin:
                twin.rollup_fold_columns(sl, r["rows"])
                twin.sketch_fold_columns(sl, r["rows"])
                r["_want"] = reads(twin)
    checks["the_full_range_twin_equals_the_ingest"] = ranges["all"]["_want"] == want_whole

    # ---- end to end, interleaved
    times = {"whole": []}
    times.update({name: [] for name, _ in FRACTIONS})
    stats = {}
    order = ["whole"] + [name for name, _ in FRACTIONS]
    for rnd in range(args.rounds):
        for which in order[rnd % len(order):] + order[:rnd % len(order)]:  # (who goes first rotates)
            with fa.FlowAgg(**kw) as agg:
                agg.sync()
                t0 = time.perf_counter()
                if which == "whole":
                    rc = L.fa_raw_restore(agg._h, frames.ctypes.data, frames.size, 0, 0)
                else:
                    rc = L.fa_raw_restore_range(agg._h, frames.ctypes.data, frames.size, ranges[which]["t_lo"], ranges[which]["t_hi"], 0, 0)
                times[which].append(time.perf_counter() - t0)
                assert rc == 0, (which, rc, L.fa_last_error(agg._h))
                got = reads(agg)
                if which == "whole":
                    checks["whole_round_%d" % rnd] = got == want_whole
                    stats[which] = agg.raw_load_stats()
                else:
                    st = agg.raw_range_stats()
                    checks["%s_round_%d_reads" % (which, rnd)] = got == ranges[which]["_want"]
                    checks["%s_round_%d_rows" % (which, rnd)] = st["rows_loaded"] == ranges[which]["rows"] and st["rows_seen"] == rows
                    stats[which] = dict(st, load=agg.raw_load_stats())
    res = {}
    for which in order:
        v = times[which]
        r = dict(ms=[x * 1e3 for x in v], ms_median=statistics.median(v) * 1e3, ms_min=min(v) * 1e3)
        if which != "whole":
            st = stats[which]
            r.update({k: ranges[which][k] for k in ("t_lo", "t_hi", "r_lo", "r_hi", "rows", "fraction")})
            r.update(blocks_seen=st["blocks_seen"], blocks_decoded=st["blocks_decoded"], probe_ms=st["probe_ns"] / 1e6, range_ms=st["range_ns"] / 1e6, decode_ms=st["decode_ns"] / 1e6,
                     range_kernel_ns_per_row=st["range_ns"] / rows, unpack_ms=st["load"]["unpack_ns"] / 1e6, fold_ms=st["load"]["fold_ns"] / 1e6, launches=st["launches"],
                     over_whole=statistics.median(v) / statistics.median(times["whole"]))
        else:
            r.update(blocks=stats[which]["blocks"], decode_ms=stats[which]["decode_ns"] / 1e6, unpack_ms=stats[which]["unpack_ns"] / 1e6, fold_ms=stats[which]["fold_ns"] / 1e6)
        res[which] = r
    out["restore"] = res
    out["required_1_64_median_below_fastest_whole"] = res["1/64"]["ms_median"] < res["whole"]["ms_min"]
    out["checks"] = {k: bool(v) for k, v in checks.items()}
    out["checks_ok"] = all(out["checks"].values())
    print("RANGE_STEP " + json.dumps(out))
    return 0 if out["checks_ok"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="records per fa_ingest_device call and per raw chunk")
    ap.add_argument("--universe-log2", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3, help="interleaved rounds")
    ap.add_argument("--step-timeout", type=int, default=540, help="seconds for the GPU step")
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_range_run.json"))
    args = ap.parse_args()
    if args.step:
        sys.exit(step(args))
    res = {"config": "BASELINE config 3's shape: framed FlowMessages, Zipf-1.1 over 2^%d addresses, key_sets = flows_5m + both sketches (default 4 x 2^20), "
                     "%d records over 900 s of one Date, generated in HBM, one merged LZ4 part; fresh ctx per call; one box, one run" % (args.universe_log2, args.records)}
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--records", str(args.records), "--chunk", str(args.chunk), "--universe-log2", str(args.universe_log2),
           "--rounds", str(args.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        print("the GPU step exceeded its %d s limit: stopping" % args.step_timeout, file=sys.stderr)
        sys.exit(124)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RANGE_STEP ")]
    if not line:
        sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
        print("the GPU step failed (exit status %d): stopping" % p.returncode, file=sys.stderr)
        sys.exit(p.returncode or 1)
    res.update(json.loads(line[-1][len("RANGE_STEP "):]))
    res["source_hash"] = _pkg.load().source_hash()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {x: v.get(x) for x in ("ms_median", "ms_min", "blocks_decoded", "range_kernel_ns_per_row")} for k, v in res["restore"].items()}
                     | {"checks_ok": res["checks_ok"], "required": res["required_1_64_median_below_fastest_whole"]}))
    sys.exit(0 if res["checks_ok"] and res["required_1_64_median_below_fastest_whole"] else 1)


if __name__ == "__main__":
    main()
