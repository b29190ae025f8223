"""CPU tests of the ranged loads of flows_raw parts (include/flowagg.h "ranged loads of flows_raw parts").

tests/host_raw_range.hip instantiates on the host what a ranged load decides without a GPU (csrc/raw_range_plan.h): over rows
0 .. 300 and the row counts around 2^7, 2^14, a block's 595.78 rows and the 65536-byte edges of the columns, and a grid of slices
each - every byte raw_unpack_kernel loads for the slice (its address arithmetic, aligned words included), every header byte, every
TimeReceived byte and every load of raw_range_kernel lies in a planned block; every planned block holds a needed byte; no block
stands in two stages' decode lists; the kernel's element predicate over random sorted and unsorted columns gives std::lower_bound
and the first descent.  It is built plain and with the host's AddressSanitizer + UBSan and run as a program.  The library's part:
the three new symbols are exported, the ABI is still 8, the structures' sizes.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-g"]
RANGE_FUNCS = ["fa_raw_range_probe", "fa_raw_restore_range", "fa_raw_range_stats"]


def _program(sanitize):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_raw_range" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "host_raw_range.hip")
    deps = [src] + [os.path.join(ROOT, "flow-pipeline_amd", "csrc", f) for f in ("raw_range_plan.h", "raw.cuh", "align16.cuh")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1" if sanitize else "-O2", "-std=c++17"] + (SANITIZE if sanitize else []) + ["-o", exe, src])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_block_sets_and_predicate(sanitize):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")  # (the process loads the HIP runtime, which keeps its allocations)
    res = subprocess.run([_program(sanitize)], capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0 and res.stdout.startswith("OK "), res.stdout + res.stderr[-4000:]
    assert int(re.findall(r"\d+", res.stdout)[0]) > 10 ** 6  # the block-set, load and predicate checks all ran


def test_library_exports_the_range_doors(fa):
    if not os.path.exists(fa.LIB_PATH):
        fa.build()
    L = C.CDLL(fa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "flowagg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    bound = fa.lib()
    for f in RANGE_FUNCS:
        assert hasattr(L, f), "libflowagg.so does not export %s" % f
        assert re.search(r"\bint\s+%s\s*\(" % f, code), "flowagg.h does not declare %s" % f
        assert f in fa.EXPORTS
        assert getattr(bound, f).argtypes, "%s has no argtypes" % f
    vp, sz, u32, szp = C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_size_t)
    assert list(bound.fa_raw_range_probe.argtypes) == [vp, vp, sz, u32, u32, vp, sz, szp]
    assert list(bound.fa_raw_restore_range.argtypes) == [vp, vp, sz, u32, u32, u32, C.c_int]
    assert "ABI 8, addition: ranged loads of flows_raw parts" in hdr
    # no new ABI version, and the pinned sizes stay put
    assert bound.fa_abi_version() == 8 and C.sizeof(fa.Config) == 64 and C.sizeof(fa.Stats) == 312 and C.sizeof(fa.RawLoadStats) == 96
    # fa_raw_range: 40 bytes, the header's member list
    m = re.search(r"typedef struct \{([^}]*)\}\s*fa_raw_range;", code, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "uint32_t date, t_min, t_max, _pad; uint64_t rows, r_lo, r_hi;"
    assert fa.RAW_RANGE_DTYPE.itemsize == 40 and fa.RAW_RANGE_DTYPE.names == ("date", "t_min", "t_max", "_pad", "rows", "r_lo", "r_hi")
    assert [fa.RAW_RANGE_DTYPE.fields[n][1] for n in fa.RAW_RANGE_DTYPE.names] == [0, 4, 8, 12, 16, 24, 32]
    # fa_raw_range_stats_t: twelve uint64_t, the header's order
    fields = ["calls", "parts_seen", "parts_skipped_date", "parts_empty", "blocks_seen", "blocks_decoded", "rows_seen", "rows_loaded", "launches", "probe_ns", "range_ns", "decode_ns"]
    assert [n for n, _ in fa.RawRangeStats._fields_] == fields and C.sizeof(fa.RawRangeStats) == 96
    m = re.search(r"typedef struct \{([^}]*)\}\s*fa_raw_range_stats_t;", code, flags=re.S)
    assert m and re.findall(r"\b(?!uint64_t\b)[a-z_]+\b", m.group(1)) == fields
    for name in ("raw_range_probe", "raw_restore_range", "raw_range_stats"):
        assert callable(getattr(fa.FlowAgg, name))
