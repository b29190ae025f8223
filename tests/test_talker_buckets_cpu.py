"""CPU tests of the bucketed top talkers (include/flowagg.h "ABI 8, addition: exact top talkers for a time range"): the ABI
surface of the new calls, and the bucketed group key - talkers.cuh compiled for the host (tests/host_talker_buckets.hip)
against a restatement in this file.  No GPU needed."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUCKET_FUNCS = ["fa_talkers_enable_buckets", "fa_top_talkers_range", "fa_talkers_range_rows_device", "fa_talkers_buckets",
                "fa_talkers_drop_before", "fa_group_top_talkers_range"]


def test_abi_surface(fa):
    if not os.path.exists(fa.LIB_PATH):
        fa.build()
    L = C.CDLL(fa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "flowagg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    bound = fa.lib()
    for f in BUCKET_FUNCS:
        assert hasattr(L, f), "libflowagg.so does not export %s" % f
        assert re.search(r"\bint\s+%s\s*\(" % f, code), "flowagg.h does not declare %s" % f
        assert f in fa.EXPORTS
        assert getattr(bound, f).argtypes, "%s has no argtypes" % f
    u32, sz, vp = C.c_uint32, C.c_size_t, C.c_void_p
    assert list(bound.fa_talkers_enable_buckets.argtypes) == [vp, u32, u32]
    assert list(bound.fa_top_talkers_range.argtypes)[:5] == [vp, C.c_int, u32, u32, sz]
    assert list(bound.fa_talkers_drop_before.argtypes) == [vp, u32]
    # no new row kind, and the pinned sizes stay put
    assert bound.fa_row_bytes(10) == 0 and bound.fa_row_bytes(8) == bound.fa_row_bytes(9) == 40
    assert bound.fa_abi_version() == 8 and C.sizeof(fa.Config) == 64 and C.sizeof(fa.Stats) == 312 and C.sizeof(fa.TalkersStats) == 72
    # the doors of the binding
    import inspect
    assert "bucket_secs" in inspect.signature(fa.FlowAgg.talkers_enable).parameters
    for cls in (fa.FlowAgg, fa.FlowGroup):
        assert {"t_lo", "t_hi"} <= set(inspect.signature(cls.top_talkers).parameters)
    assert {"t_lo", "t_hi"} <= set(inspect.signature(fa.dist.top_talkers_merged).parameters)
    for name in ("talkers_range_rows_device", "talkers_buckets", "talkers_drop_before"):
        assert callable(getattr(fa.FlowAgg, name))


def canon(addr: bytes, etype: int):
    if etype == 0x800:
        return addr[:4] + bytes(12), 0x800
    return bytes(addr), 0


def _cases():
    rng = random.Random(20261019)
    v4 = bytes([192, 168, 1, 1])
    # every address bit that lives in the third key word (bits 126, 127 of the 128: the top two bits of byte 15), alone and together
    addrs = [bytes(16), b"\xff" * 16, v4 + bytes(12), v4 + bytes(11) + b"\x80", v4 + bytes(11) + b"\x40", v4 + bytes(11) + b"\xc0",
             bytes(15) + b"\x80", bytes(15) + b"\x40", bytes(15) + b"\xc0", bytes(15) + b"\x3f", bytes(7) + b"\x80" + bytes(8), bytes(8) + b"\x01" + bytes(7)]
    etypes = [0x800, 0x86dd, 0, 0x1234]
    indices = [0, 1, 0xFF, 0x100, 0x00FFFFFF, 0x01000000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF] + [0xFFFFFFFF // bs for bs in (1, 60, 300, 3600, 86400)]
    cases = [(a, e, i) for a in addrs for e in etypes for i in indices]
    while len(cases) < 20000:
        a = bytes(rng.getrandbits(8) for _ in range(16)) if rng.random() < 0.7 else bytes([10, 0, 0, rng.randrange(4)]) + bytes(rng.choice((0, 0xff)) for _ in range(12))
        i = rng.choice(indices) if rng.random() < 0.2 else rng.getrandbits(32) if rng.random() < 0.5 else 1_600_000_200 // 60 + rng.randrange(1 << 12)
        cases.append((a, rng.choice(etypes), i))
    return cases


def test_bucketed_key_round_trip(fa):
    """tests/host_talker_buckets.hip: (address, family, bucket index) -> three key words -> the same triple; every word keeps
    bit 63; index 0 packs to the plain tkey_pack's words (checked inside the program, which fails on any of them)."""
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_talker_buckets")
    src = os.path.join(ROOT, "tests", "host_talker_buckets.hip")
    csrc = os.path.join(ROOT, "flow-pipeline_amd", "csrc")
    deps = [src, os.path.join(csrc, "talkers.cuh"), os.path.join(csrc, "table.cuh")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", exe, src])
    cases = _cases()
    assert len(cases) >= 20000
    fin, fout = os.path.join(out, "host_talker_buckets.in"), os.path.join(out, "host_talker_buckets.out")
    with open(fin, "wb") as f:
        f.write(b"".join(a + struct.pack("<II", e, i) for a, e, i in cases))
    res = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.startswith("OK %d" % len(cases)), res.stdout + res.stderr
    got = np.fromfile(fout, dtype=np.dtype([("key", "u1", 16), ("family", "<u4"), ("index", "<u4")]))
    assert len(got) == len(cases)
    seen = set()
    for (a, e, i), g in zip(cases, got):
        key, fam = canon(a, e)
        assert (g["key"].tobytes(), int(g["family"]), int(g["index"])) == (key, fam, i), (a.hex(), hex(e), i)
        seen.add((key, fam, i))
    assert {i for _, _, i in seen} >= {0, 0xFFFFFFFF, 0xFFFFFFFF // 60, 0xFFFFFFFF // 86400}
