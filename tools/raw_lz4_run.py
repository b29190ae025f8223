#!/usr/bin/env python3
"""What the LZ4 take of the flows_raw parts costs and gives (fa_raw_take_lz4; include/flowagg.h "LZ4 frames of the flows_raw
parts"), on tools/raw_parts_run.py's stream: a device-generated BASELINE config 2 stream kept in HBM, 2^23 records ingested with
fa_ingest_device in calls of 2^21 into TWO contexts with fa_raw_enable, which therefore hold identical parts.  One child process
under a time limit - one box, one session:
  * end to end, interleaved round by round: fa_raw_take of one ctx and fa_raw_take_lz4 of the other, each ONE call into
    page-locked memory that is large enough (the LZ4 call compresses and copies);
  * the compression's device time per input byte from the library's hipEvents, lz4_block_kernel and scan + lz4_pack_kernel apart;
  * blocks, stored blocks, the compressed size, and beside it LZ4_compress_default per 64 KiB block over the same image where
    the machine has liblz4 (otherwise null: that half is then run on a CPU over the same seeded stream and entered by hand);
  * checks_ok: every frame decodes to the bytes of its part in the plain take (LZ4F_decompress where liblz4 is found, else
    spill.lz4_frames_decode), and the part lists agree.
Nothing is gated on the times.  Writes profiles/raw_lz4_run.json."""
import argparse
import ctypes as C
import ctypes.util
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

BLOCK = 65536


def liblz4():
    name = ctypes.util.find_library("lz4")
    if not name:
        return None
    L = C.CDLL(name)
    L.LZ4_compress_default.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.LZ4_compressBound.argtypes = [C.c_int]
    L.LZ4F_isError.argtypes = [C.c_size_t]
    L.LZ4F_createDecompressionContext.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    L.LZ4F_createDecompressionContext.restype = C.c_size_t
    L.LZ4F_freeDecompressionContext.argtypes = [C.c_void_p]
    L.LZ4F_decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
    L.LZ4F_decompress.restype = C.c_size_t
    return L


def liblz4_blocks(L, image: np.ndarray, parts) -> int:
    """sum of LZ4_compress_default over the 64 KiB blocks of every part (a block that does not shrink counts as stored), + 4 per
    block and 11 per part: the size of the same frames written by liblz4's block compressor"""
    dst = np.empty(L.LZ4_compressBound(BLOCK), dtype=np.uint8)
    total = 0
    for p in parts:
        lo, hi = int(p["offset"]), int(p["offset"]) + int(p["bytes"])
        total += 11
        for at in range(lo, hi, BLOCK):
            n = min(BLOCK, hi - at)
            c = L.LZ4_compress_default(image[at:at + n].ctypes.data, dst.ctypes.data, n, dst.size)
            total += 4 + (c if 0 < c < n else n)
    return total


def liblz4_decode(L, frames: np.ndarray, expect: int) -> np.ndarray:
    ctx = C.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(C.byref(ctx), 100))
    out = np.empty(expect + 1, dtype=np.uint8)
    sp = dp = 0
    try:
        while sp < frames.size:
            s, d = C.c_size_t(frames.size - sp), C.c_size_t(out.size - dp)
            rc = L.LZ4F_decompress(ctx, out[dp:].ctypes.data, C.byref(d), frames[sp:].ctypes.data, C.byref(s), None)
            if L.LZ4F_isError(rc) or not (s.value or d.value):
                return out[:0]
            sp += s.value
            dp += d.value
    finally:
        L.LZ4F_freeDecompressionContext(ctx)
    return out[:dp]


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
    lz = liblz4()
    with fa.FlowAgg(**kw) as plain, fa.FlowAgg(**kw) as packed:
        plain.raw_enable()
        packed.raw_enable()
        cap = chunk * 96 + 4096
        batches = []
        for i0 in range(0, n, chunk):
            m = min(chunk, n - i0)
            d_buf = torch.empty(cap, dtype=torch.uint8, device=dev)
            d_off = torch.empty(chunk + 1, dtype=torch.int32, device=dev)
            w = plain.mock_generate_device(mp, i0, m, d_buf.data_ptr(), cap, d_off.data_ptr())
            batches.append((d_buf, d_off, w, m))

        def ingest(agg):
            for d_buf, d_off, w, m in batches:
                agg.ingest_device(d_buf.data_ptr(), w, d_off.data_ptr(), m)
            agg.sync()

        ingest(plain)
        pending = plain.raw_stats()
        nbytes, nparts = int(pending["pending_bytes"]), int(pending["pending_parts"])
        h_plain = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True).numpy()
        h_packed = torch.empty(L.fa_lz4_frame_bound(nbytes) + 11 * nparts + 4 * nparts, dtype=torch.uint8, pin_memory=True).numpy()
        parts_p, parts_l = np.zeros(nparts, dtype=fa.RAW_PART_DTYPE), np.zeros(nparts, dtype=fa.RAW_PART_DTYPE)
        nb, npart = C.c_size_t(), C.c_size_t()
        t_plain, t_lz4, sizes = [], [], []
        for r in range(args.rounds):
            if r:
                ingest(plain)
            ingest(packed)
            before = packed.raw_lz4_stats()
            for which in (("plain", "lz4") if r % 2 == 0 else ("lz4", "plain")):  # (who goes first alternates)
                t0 = time.perf_counter()
                if which == "plain":
                    rc = L.fa_raw_take(plain._h, h_plain.ctypes.data, h_plain.size, C.byref(nb), parts_p.ctypes.data, nparts, C.byref(npart))
                    t_plain.append(time.perf_counter() - t0)
                    assert rc == 0 and nb.value == nbytes and npart.value == nparts, (rc, nb.value, npart.value)
                else:
                    rc = L.fa_raw_take_lz4(packed._h, h_packed.ctypes.data, h_packed.size, C.byref(nb), parts_l.ctypes.data, nparts, C.byref(npart))
                    t_lz4.append(time.perf_counter() - t0)
                    assert rc == 0 and npart.value == nparts, (rc, nb.value, npart.value)
                    sizes.append(nb.value)
            after = packed.raw_lz4_stats()
            if r == 0:
                first = {k: after[k] - before[k] for k in after}
        st = packed.raw_lz4_stats()
        out["parts"] = nparts
        out["plain_bytes"] = nbytes
        out["lz4_bytes"] = sizes
        out["ratio"] = nbytes / sizes[-1]
        out["blocks_per_take"] = first["blocks"]
        out["stored_blocks_per_take"] = first["stored_blocks"]
        out["compress_launches_per_take"] = first["compress_launches"]
        out["block_kernel_ns_per_input_byte"] = st["block_ns"] / st["bytes_in"]
        out["scan_and_pack_ns_per_input_byte"] = st["pack_ns"] / st["bytes_in"]
        out["compress_device_ms_per_take"] = st["device_ns"] / args.rounds / 1e6
        out["compress_GB_per_s_of_input"] = st["bytes_in"] / st["device_ns"]
        out["take_plain_ms"] = [t * 1e3 for t in t_plain]
        out["take_lz4_ms"] = [t * 1e3 for t in t_lz4]
        out["take_plain_ms_median"] = statistics.median(t_plain) * 1e3
        out["take_lz4_ms_median"] = statistics.median(t_lz4) * 1e3
        out["take_plain_GB_per_s"] = nbytes / statistics.median(t_plain) / 1e9
        out["take_lz4_GB_per_s_of_plain_bytes"] = nbytes / statistics.median(t_lz4) / 1e9
        out["lz4_take_is_faster_end_to_end"] = bool(statistics.median(t_lz4) < statistics.median(t_plain))
        out["raw_lz4_stats"] = st
        # ---- the checks: the last round's frames against the last round's plain bytes
        frames = h_packed[:sizes[-1]]
        checks["part_lists_agree"] = all(np.array_equal(parts_p[f], parts_l[f]) for f in ("date", "t_min", "t_max", "rows"))
        checks["frames_tile_the_bytes"] = (int(parts_l["offset"][0]) == 0 and np.array_equal(parts_l["offset"][1:], np.cumsum(parts_l["bytes"])[:-1])
                                           and int(parts_l["bytes"].sum()) == sizes[-1])
        t0 = time.perf_counter()
        if lz is not None:
            out["decoder"] = "liblz4 LZ4F_decompress"
            checks["frames_decode_to_the_plain_bytes"] = np.array_equal(liblz4_decode(lz, frames, nbytes), h_plain)
        else:
            out["decoder"] = "spill.lz4_frames_decode (no liblz4 on this machine)"
            ok = True
            for pl, pp in zip(parts_l, parts_p):
                got = fa.spill.lz4_frames_decode(frames[int(pl["offset"]):int(pl["offset"]) + int(pl["bytes"])].tobytes())
                ok = ok and got == h_plain[int(pp["offset"]):int(pp["offset"]) + int(pp["bytes"])].tobytes()
            checks["frames_decode_to_the_plain_bytes"] = ok
        out["decode_check_s"] = time.perf_counter() - t0
        if lz is not None:
            ref = liblz4_blocks(lz, h_plain, parts_p)
            out["liblz4_blocks_bytes"] = ref
            out["liblz4_blocks_ratio"] = nbytes / ref
            out["size_against_liblz4"] = sizes[-1] / ref
        else:
            out["liblz4_blocks_bytes"] = out["liblz4_blocks_ratio"] = out["size_against_liblz4"] = None
        out["checks"] = {k: bool(v) for k, v in checks.items()}
        out["checks_ok"] = all(out["checks"].values())
    print("LZ4_STEP " + json.dumps(out))
    return 0 if out["checks_ok"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="records per fa_ingest_device call")
    ap.add_argument("--rounds", type=int, default=3, help="interleaved takes per ctx")
    ap.add_argument("--step-timeout", type=int, default=540, help="seconds for the GPU step")
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_lz4_run.json"))
    args = ap.parse_args()
    if args.step:
        sys.exit(step(args))
    res = {"config": "framed FlowMessages, BASELINE config 2 (65 536 AS pairs x 2 ETypes over 900 s), key_sets = flows_5m, %d records in calls of %d, "
                     "generated in HBM; raw chunk 2^20; two contexts with identical parts; one box, one run" % (args.records, args.chunk)}
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "--records", str(args.records), "--chunk", str(args.chunk), "--rounds", str(args.rounds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        print("the GPU step exceeded its %d s limit: stopping" % args.step_timeout, file=sys.stderr)
        sys.exit(124)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("LZ4_STEP ")]
    if not line:
        sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
        print("the GPU step failed (exit status %d): stopping" % p.returncode, file=sys.stderr)
        sys.exit(p.returncode or 1)
    res.update(json.loads(line[-1][len("LZ4_STEP "):]))
    res["source_hash"] = _pkg.load().source_hash()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res.get(k) for k in ("plain_bytes", "lz4_bytes", "ratio", "size_against_liblz4", "stored_blocks_per_take", "block_kernel_ns_per_input_byte",
                                              "scan_and_pack_ns_per_input_byte", "take_plain_ms_median", "take_lz4_ms_median", "checks_ok")}))
    sys.exit(0 if res["checks_ok"] else 1)


if __name__ == "__main__":
    main()
