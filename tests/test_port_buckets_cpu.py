"""CPU tests of the bucketed port tables (include/flowagg.h "ABI 8, addition: exact top ports for a time range"): the ABI surface
of the new calls; the (bucket index, port) key and the range rule compiled for the host (tests/host_port_buckets.hip) against
statements in this file; and the restatement the GPU tests compare with against a dictionary group-by.  No GPU needed."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PORT_FUNCS = ["fa_ports_enable_buckets", "fa_ports_fold_columns_device", "fa_top_ports_range", "fa_ports_range_rows_device", "fa_ports_buckets",
              "fa_ports_drop_before", "fa_ports_reset", "fa_ports_stats", "fa_group_top_ports_range"]
NO_UPPER = 0xFFFFFFFF


def test_abi_surface(fa):
    if not os.path.exists(fa.LIB_PATH):
        fa.build()
    L = C.CDLL(fa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "flowagg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    bound = fa.lib()
    for f in PORT_FUNCS:
        assert hasattr(L, f), "libflowagg.so does not export %s" % f
        assert re.search(r"\bint\s+%s\s*\(" % f, code), "flowagg.h does not declare %s" % f
        assert f in fa.EXPORTS
        assert getattr(bound, f).argtypes, "%s has no argtypes" % f
    u32, sz, vp = C.c_uint32, C.c_size_t, C.c_void_p
    assert list(bound.fa_ports_enable_buckets.argtypes) == [vp, u32, u32]
    assert list(bound.fa_top_ports_range.argtypes)[:5] == [vp, C.c_int, u32, u32, sz]
    assert list(bound.fa_group_top_ports_range.argtypes)[:5] == [vp, C.c_int, u32, u32, sz]
    assert list(bound.fa_ports_drop_before.argtypes) == [vp, u32]
    # no new row kind, no new ABI version, and the pinned sizes stay put
    assert bound.fa_row_bytes(10) == 0 and bound.fa_row_bytes(2) == bound.fa_row_bytes(3) == 24 == fa.PORT_ROW_DTYPE.itemsize
    assert bound.fa_abi_version() == 8 and C.sizeof(fa.Config) == 64 and C.sizeof(fa.Stats) == 312 and C.sizeof(fa.PortsStats) == 72
    assert "ABI 8, addition: exact top ports for a time range" in hdr
    # the doors of the binding
    import inspect
    for name in ("ports_enable_buckets", "top_ports_range", "ports_range_rows_device", "ports_fold_columns_device", "ports_buckets", "ports_drop_before",
                 "ports_reset", "ports_stats"):
        assert callable(getattr(fa.FlowAgg, name))
    for cls in (fa.FlowAgg, fa.FlowGroup):
        assert {"t_lo", "t_hi", "k"} <= set(inspect.signature(cls.top_ports_range).parameters)
    assert {"t_lo", "t_hi", "k", "group"} <= set(inspect.signature(fa.dist.top_ports_merged).parameters)
    # the geometry the GPU tests size their cases with is the kernel's
    src = open(os.path.join(ROOT, "flow-pipeline_amd", "csrc", "ports.cuh")).read()
    assert int(re.search(r"constexpr int PORT_BLOCK = (\d+);", src).group(1)) == fa.PORT_BLOCK
    assert int(re.search(r"#define FA_PORT_LDS_ENTRIES (\d+)", src).group(1)) == fa.PORT_LDS_ENTRIES
    assert int(re.search(r"constexpr int PORT_WG_PER_CU = (\d+);", src).group(1)) == fa.PORT_WG_PER_CU


def _host_program():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_port_buckets")
    src = os.path.join(ROOT, "tests", "host_port_buckets.hip")
    csrc = os.path.join(ROOT, "flow-pipeline_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("ports.cuh", "bucket_range.h", "table.cuh")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", exe, src])
    return exe, out


def _run(mode, payload, n):
    exe, out = _host_program()
    fin, fout = os.path.join(out, "host_port_buckets_%s.in" % mode), os.path.join(out, "host_port_buckets_%s.out" % mode)
    with open(fin, "wb") as f:
        f.write(payload)
    res = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.startswith("OK %d" % n), res.stdout + res.stderr
    got = np.fromfile(fout, dtype="<u4").reshape(-1, 4)
    assert len(got) == n
    return got


EDGES = [0, 1, 0xFF, 0xFFFF, 0x10000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]
BUCKET_SECS = [1, 60, 300, 3600, 86400]


def test_key_round_trip_and_empty_rule():
    """(bucket index, port) -> two key words -> the same pair, for every pair of edge values - (0, 0) and (0xFFFFFFFF, 0xFFFFFFFF)
    among them - and random ones; neither word is ever EMPTY (checked inside the program, which fails on any of it); the bucket
    index of a TimeFlowStart is the 32-bit narrowing divided by bucket_secs."""
    rng = random.Random(20261019)
    cases = [(i, p, bs, (hi << 32) | t) for i in EDGES for p in EDGES for bs, t, hi in ((1, i, 0), (60, p, 7), (86400, i ^ p, 0xFFFFFFFF))]
    while len(cases) < 20000:
        cases.append((rng.getrandbits(32), rng.choice(EDGES) if rng.random() < 0.3 else rng.getrandbits(32), rng.choice(BUCKET_SECS), rng.getrandbits(64)))
    got = _run("keys", b"".join(struct.pack("<IIIIQ", i, p, bs, 0, t) for i, p, bs, t in cases), len(cases))
    for (i, p, bs, t), g in zip(cases, got):
        assert (int(g[0]), int(g[1]), int(g[2])) == (i, p, (t & 0xFFFFFFFF) // bs), (i, p, bs, t)
    assert {(0, 0), (0xFFFFFFFF, 0xFFFFFFFF)} <= {(i, p) for i, p, _, _ in cases}


def test_range_helper_bounds():
    """bucket_range_of against the rule as the header states it: t_lo <= t32 < t_hi, both on the grid, t_hi = 0xFFFFFFFF no upper
    bound, t_lo == t_hi empty, off-grid and t_lo > t_hi refused - checked through membership: t32 is selected exactly when its
    bucket index lies in [index_lo, index_last]."""
    rng = random.Random(7)
    cases = []
    for bs in BUCKET_SECS:
        last = NO_UPPER // bs * bs
        grid = [0, bs, 2 * bs, 1_600_000_200 // bs * bs, last - bs, last]
        cases += [(bs, lo, hi) for lo in grid for hi in grid + [NO_UPPER]]
        cases += [(bs, lo + 1, hi) for lo in grid[:3] for hi in grid[3:]] + [(bs, lo, hi + 1) for lo in grid[:3] for hi in grid[3:5]] + [(bs, 0, 0xFFFFFFFE)]
        cases += [(bs, rng.randrange(0, 1 << 20) * bs % (1 << 32), rng.randrange(0, 1 << 20) * bs % (1 << 32)) for _ in range(200)]
    got = _run("ranges", b"".join(struct.pack("<III", *c) for c in cases), len(cases))
    seen = set()
    for (bs, lo, hi), (rc, index_lo, index_last, empty) in zip(cases, got.tolist()):
        off_grid = lo % bs != 0 or (hi != NO_UPPER and hi % bs != 0)
        want_rc = 1 if off_grid else 2 if lo > hi else 0
        assert rc == want_rc, (bs, lo, hi)
        seen.add(want_rc)
        if rc:
            continue
        assert empty == (1 if lo == hi else 0)
        if empty:
            continue
        probes = {0, lo, lo + bs - 1, max(lo, 1) - 1, NO_UPPER, NO_UPPER // bs * bs, NO_UPPER // bs * bs - 1}
        if hi != NO_UPPER:
            probes |= {hi - 1, hi, min(hi + bs, NO_UPPER)}
        for t in probes:
            selected = lo <= t and (hi == NO_UPPER or t < hi)
            assert selected == (index_lo <= t // bs <= index_last), (bs, lo, hi, t)
    assert seen == {0, 1, 2}


def test_restatement_against_a_dictionary_group_by(po):
    """What the GPU tests compare with - po.top_ports over the in_range filter (tests/test_port_buckets_gpu.py: restate, pairs,
    buckets_of) - against a group-by written with a dictionary."""
    import test_port_buckets_gpu as T
    rng = np.random.default_rng(11)
    n, bs, T0 = 5000, 60, po.T0
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    rows["src_port"] = rng.choice(np.array([0, 1, 80, 443, 65535, 65536, 0xFFFFFFFF], dtype=np.uint32), size=n)
    rows["dst_port"] = rng.integers(0, 50, size=n).astype(np.uint32) * np.uint32(3000)
    rows["bytes"] = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    rows["sampling_rate"] = rng.choice(np.array([0, 1, 1 << 20], dtype=np.uint64), size=n)
    rows["time_flow_start"] = (rng.integers(0, 4, size=n).astype(np.uint64) << np.uint64(32)) | (np.uint64(T0) + rng.integers(0, 600, size=n).astype(np.uint64))
    rows["time_flow_start"][:50] = 0xFFFFFFFF
    status = (rng.random(n) < 0.1).astype(np.uint32)
    for dst in (0, 1):
        for lo, hi, k in ((0, NO_UPPER, 0), (T0 + 60, T0 + 180, 0), (T0 + 60, T0 + 180, 5), (T0 + 120, T0 + 120, 0), (NO_UPPER // bs * bs, NO_UPPER, 0)):
            groups, held = {}, set()
            for r, st in zip(rows, status):
                t = int(r["time_flow_start"]) & 0xFFFFFFFF
                if st:
                    continue
                held.add((t - t % bs, int(r["dst_port" if dst else "src_port"])))
                if lo == hi or t < lo or (hi != NO_UPPER and t >= hi):
                    continue
                p = int(r["dst_port" if dst else "src_port"])
                w, c = groups.get(p, (0, 0))
                groups[p] = ((w + int(r["bytes"]) * int(r["sampling_rate"])) % (1 << 64), c + 1)
            want = sorted(((p, w, c) for p, (w, c) in groups.items()), key=lambda x: (-x[1], x[0]))
            want = want[:k] if k else want
            got = T.restate(po, rows, status, dst, lo, hi, k)
            assert [(int(g["port"]), int(g["weight"]), int(g["count"])) for g in got] == want
            assert T.pairs(po, rows, status, dst, bs) == len(held)
    assert list(T.buckets_of(rows, status, bs)) == sorted({b for b, _ in held})
