"""CPU tests of the exact top talkers (include/flowagg.h "ABI 8, addition"): the ABI surface, and the group key
"grouped as the dashboards do" - talkers.cuh compiled for the host against a restatement in this file and against
the string fa_format_addr renders.  No GPU needed."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TALKER_FUNCS = ["fa_talkers_enable", "fa_talkers_fold_columns_device", "fa_top_talkers", "fa_merge_talkers",
                "fa_talkers_reset", "fa_talkers_stats"]


def canon(addr: bytes, etype: int):
    """The restatement: EType 0x800 -> (bytes 0..3 + twelve zero bytes, 0x800); anything else -> (all 16 bytes, 0)."""
    if etype == 0x800:
        return addr[:4] + bytes(12), 0x800
    return bytes(addr), 0


def test_abi_surface(fa):
    if not os.path.exists(fa.LIB_PATH):
        fa.build()
    L = C.CDLL(fa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "flowagg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for f in TALKER_FUNCS:
        assert hasattr(L, f), "libflowagg.so does not export %s" % f
        assert re.search(r"\bint\s+%s\s*\(" % f, code), "flowagg.h does not declare %s" % f
        assert f in fa.EXPORTS
    assert fa.TALKER_ROW_DTYPE.itemsize == 40
    assert fa.TALKER_ROW_DTYPE.fields["etype"][1] == 16 and fa.TALKER_ROW_DTYPE.fields["weight"][1] == 24 and fa.TALKER_ROW_DTYPE.fields["count"][1] == 32
    # sizeof(fa_talkers_stats_t) from the header's own member list: uint64_t members, arrays counted
    m = re.search(r"typedef struct \{([^}]*)\}\s*fa_talkers_stats_t;", code, flags=re.S)
    assert m, "fa_talkers_stats_t is not declared"
    words = 0
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        assert decl.startswith("uint64_t"), decl
        for name in decl[len("uint64_t"):].split(","):
            dim = re.search(r"\[(\d+)\]", name)
            words += int(dim.group(1)) if dim else 1
    assert words * 8 == C.sizeof(fa.TalkersStats) == 72
    # the ABI the issue pins stays put
    assert fa.lib().fa_abi_version() == 8 and C.sizeof(fa.Config) == 64 and C.sizeof(fa.Stats) == 312


def _cases():
    rng = random.Random(20251018)
    v4 = bytes([192, 168, 1, 1])
    addrs = [
        bytes(16),                                          # "::" / "0.0.0.0"
        bytes(15) + b"\x01",
        bytes(10) + b"\xff\xff" + v4,                        # IPv4-mapped
        bytes(12) + v4,                                      # IPv4-compatible
        bytes(10) + b"\xff\xfe" + v4,
        v4 + bytes(12),                                      # what GoFlow stores for IPv4
        v4 + b"\x01" * 12, v4 + bytes(11) + b"\x01", v4 + b"\x80" + bytes(11),   # equal first four bytes, different tails
        v4 + bytes(3) + b"\x80" + bytes(8), v4 + bytes(4) + b"\x80" + bytes(7),   # ... bit 63 of the low word, bit 0 of the high word
        v4 + bytes(11) + b"\x80", v4 + bytes(11) + b"\x40",                     # ... the bits that live in the third key word
        b"\xff" * 16, b"\x00\x01" + bytes(14), struct.pack("<I", 3232235777) + bytes(12),
    ]
    etypes = [0x800, 0x86dd, 0, 0x806, 0x1234, 0x8000800, 0xffffffff, 1]
    cases = [(a, e) for a in addrs for e in etypes]         # the same bytes under 0x800 / 0x86dd / 0 / ...
    while len(cases) < 20000:
        kind = rng.randrange(4)
        if kind == 0:
            a = bytes(rng.getrandbits(8) for _ in range(16))
        elif kind == 1:  # few distinct heads, random tails: collisions of the first four bytes
            a = bytes([10, 0, 0, rng.randrange(4)]) + bytes(rng.choice((0, 0, 1, 0xff)) for _ in range(12))
        elif kind == 2:  # sparse 16-bit groups (zero runs: what IPv6NumToString compresses)
            a = struct.pack(">8H", *[rng.choice((0, 0, 0, 1, 0xff, 0x100, 0xffff, rng.getrandbits(16))) for _ in range(8)])
        else:
            a = bytes([rng.randrange(3), 0, 0, rng.randrange(3)]) + bytes(12)
        cases.append((a, rng.choice(etypes[:5]) if rng.random() < 0.9 else rng.getrandbits(32)))
    return cases


def test_group_key_is_the_rendered_strings_preimage(fa):
    """tests/host_talkers.hip (talkers.cuh on the host) == the restatement, and the defining property: two inputs
    have equal (key, family) iff fa.format_addr renders them to equal strings."""
    if not os.path.exists(fa.LIB_PATH):
        fa.build()
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_talkers")
    src = os.path.join(ROOT, "tests", "host_talkers.hip")
    csrc = os.path.join(ROOT, "flow-pipeline_amd", "csrc")
    deps = [src, os.path.join(csrc, "talkers.cuh"), os.path.join(csrc, "table.cuh")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", exe, src])
    cases = _cases()
    assert len(cases) >= 20000
    fin, fout = os.path.join(out, "host_talkers.in"), os.path.join(out, "host_talkers.out")
    with open(fin, "wb") as f:
        f.write(b"".join(a + struct.pack("<I", e) for a, e in cases))
    res = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.startswith("OK"), res.stdout + res.stderr
    got = np.fromfile(fout, dtype=np.dtype([("key", "u1", 16), ("family", "<u4")]))
    assert len(got) == len(cases)
    by_key, by_str = {}, {}
    for (a, e), g in zip(cases, got):
        want = canon(a, e)
        assert (g["key"].tobytes(), int(g["family"])) == want, (a.hex(), hex(e))
        s = fa.format_addr(a, e)
        assert fa.format_addr(want[0], want[1]) == s          # the row's (key, etype) renders to the group's string
        assert by_key.setdefault(want, s) == s, (a.hex(), hex(e))        # equal keys -> equal strings
        assert by_str.setdefault(s, want) == want, (a.hex(), hex(e), s)  # equal strings -> equal keys
    assert len(by_key) == len(by_str) > 5000
