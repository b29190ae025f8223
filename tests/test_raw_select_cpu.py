"""CPU tests of selecting rows of flows_raw parts (include/flowagg.h "selecting rows of flows_raw parts").

tests/host_raw_select.hip instantiates on the host what the select decides without a GPU (csrc/raw_select.cuh): the prefix
comparison against a bit-by-bit loop for every length 0 .. 128 (random pairs, pairs that differ only in the last bit inside or only
in the first bit outside); the predicate against a naive restatement over 10^5 seeded rows x 200 seeded filters (every bit alone,
EITHER with each direction satisfied alone, ports at 0 / 65535 / 65536 / 0xFFFFFFFF with lo == hi); the position rule over random
masks of 1 .. 5 workgroups with a limit below, at and above the count; and every byte the select and emit kernels load for a slice
against the blocks stages B and C of a ranged load planned, over the row counts of host_raw_range.hip's grid.  It is built plain and
with the host's AddressSanitizer + UBSan and run as a program.  The library's part: the four new symbols are exported and declared,
their argtypes, the structures' sizes and member lists, the ABI is still 8.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-g"]
SELECT_FUNCS = ["fa_raw_select", "fa_raw_selection_device", "fa_raw_selection_fetch", "fa_raw_select_stats"]


def _program(sanitize):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_raw_select" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "host_raw_select.hip")
    deps = [src, os.path.join(ROOT, "include", "flowagg.h")] + [os.path.join(ROOT, "flow-pipeline_amd", "csrc", f) for f in (
        "raw_select.cuh", "raw_merge.cuh", "raw_range_plan.h", "raw.cuh", "align16.cuh")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1" if sanitize else "-O2", "-std=c++17"] + (SANITIZE if sanitize else []) + ["-o", exe, src])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_predicate_positions_and_loads(sanitize):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")  # (the process loads the HIP runtime, which keeps its allocations)
    res = subprocess.run([_program(sanitize)], capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0 and res.stdout.startswith("OK "), res.stdout + res.stderr[-4000:]
    assert int(re.findall(r"\d+", res.stdout)[0]) > 4 * 10 ** 7  # 2 * 10^7 predicate checks, and the prefix, position and load checks all ran


def test_library_exports_the_select_doors(fa):
    if not os.path.exists(fa.LIB_PATH):
        fa.build()
    L = C.CDLL(fa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "flowagg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    bound = fa.lib()
    for f in SELECT_FUNCS:
        assert hasattr(L, f), "libflowagg.so does not export %s" % f
        assert re.search(r"\bint\s+%s\s*\(" % f, code), "flowagg.h does not declare %s" % f
        assert f in fa.EXPORTS
        assert getattr(bound, f).argtypes, "%s has no argtypes" % f
    vp, sz, szp = C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)
    assert list(bound.fa_raw_select.argtypes) == [vp, vp, sz, C.POINTER(fa.RawFilter), vp, sz, szp, szp]
    assert list(bound.fa_raw_selection_device.argtypes) == [vp, C.POINTER(C.c_void_p), szp]
    assert list(bound.fa_raw_selection_fetch.argtypes) == [vp, vp, sz, szp]
    assert list(bound.fa_raw_select_stats.argtypes) == [vp, C.POINTER(fa.RawSelectStats)]
    assert "ABI 8, addition: selecting rows of flows_raw parts" in hdr
    # no new ABI version, and the pinned sizes stay put
    assert bound.fa_abi_version() == 8 and C.sizeof(fa.Config) == 64 and C.sizeof(fa.Stats) == 312
    assert C.sizeof(fa.RawLoadStats) == 96 and C.sizeof(fa.RawRangeStats) == 96 and fa.RAW_PART_DTYPE.itemsize == 40
    # fa_raw_filter: 96 bytes, the header's member list and the offsets it gives
    m = re.search(r"typedef struct \{([^}]*)\}\s*fa_raw_filter;", code, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == (
        "uint32_t fields; uint32_t t_lo, t_hi; uint32_t tf_lo, tf_hi; uint32_t src_as, dst_as, etype, proto; "
        "uint32_t src_port_lo, src_port_hi, dst_port_lo, dst_port_hi; uint8_t src_prefix_len, dst_prefix_len, _pad[2]; "
        "uint8_t src_addr[16], dst_addr[16]; uint64_t limit;")
    names = ["fields", "t_lo", "t_hi", "tf_lo", "tf_hi", "src_as", "dst_as", "etype", "proto", "src_port_lo", "src_port_hi", "dst_port_lo", "dst_port_hi",
             "src_prefix_len", "dst_prefix_len", "_pad", "src_addr", "dst_addr", "limit"]
    assert [n for n, _ in fa.RawFilter._fields_] == names and C.sizeof(fa.RawFilter) == 96
    assert [getattr(fa.RawFilter, n).offset for n in names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 53, 54, 56, 72, 88]
    bits = dict(re.findall(r"#define FA_RAW_F_([A-Z_]+) (\d+)u", code))
    want = dict(FLOW_START=1, SRC_AS=2, DST_AS=4, ETYPE=8, PROTO=16, SRC_PORT=32, DST_PORT=64, SRC_ADDR=128, DST_ADDR=256, EITHER=512, COUNT_ONLY=1024)
    assert {k: int(v) for k, v in bits.items() if k != "ALL"} == want and int(bits["ALL"]) == sum(want.values())
    assert all(getattr(fa, "RAW_F_" + k) == v for k, v in want.items())
    # fa_raw_select_stats_t: ten uint64_t, the header's order
    fields = ["calls", "rows_scanned", "rows_matched", "rows_out", "parts_out", "bytes_out", "launches", "select_ns", "emit_ns", "gather_ns"]
    assert [n for n, _ in fa.RawSelectStats._fields_] == fields and C.sizeof(fa.RawSelectStats) == 80
    m = re.search(r"typedef struct \{([^}]*)\}\s*fa_raw_select_stats_t;", code, flags=re.S)
    assert m and re.findall(r"\b(?!uint64_t\b)[a-z_]+\b", m.group(1)) == fields
    for name in ("raw_select", "raw_selection_device", "raw_select_stats"):
        assert callable(getattr(fa.FlowAgg, name))
    # the keywords' filter
    f = fa.raw_filter(5, 9, flow_start=(1, 2), src_as=3, dst_port=(80, 443), src_net=(bytes(range(16)), 24), either=True, limit=7, count_only=True)
    assert f.fields == 1 | 2 | 64 | 128 | 512 | 1024 and (f.t_lo, f.t_hi, f.tf_lo, f.tf_hi, f.src_as, f.dst_port_lo, f.dst_port_hi) == (5, 9, 1, 2, 3, 80, 443)
    assert bytes(f.src_addr) == bytes(range(16)) and f.src_prefix_len == 24 and f.limit == 7 and bytes(f._pad) == b"\0\0"
