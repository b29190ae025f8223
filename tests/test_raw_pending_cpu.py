"""CPU tests of the pending flows_raw parts as input (include/flowagg.h "the pending flows_raw parts as input").

tests/host_raw_bounds.hip runs on the host what these doors decide without a GPU: the step arithmetic of raw_bounds_kernel
(csrc/raw_bounds.cuh) - the very text, with 64 simulated lanes - against std::lower_bound over every row count 0 .. 300, the counts
around 4096, 65^2 and 2^18, columns that are all equal, strictly ascending, runs of 3 and of 70 and random, keys below, at, between
and above the values and at the ends of the axis, the column at byte phases 0 .. 3 in a heap block of exactly its size, and the step
count against the stated bound; and the classification of csrc/raw_pending_plan.h against a naive scan of the rows.  It is built
plain and with the host's AddressSanitizer + UBSan and run as a program.  The library's part: the four new symbols are exported and
declared, their argtypes, the statistics' size and member list, the ABI is still 8.  And a condition on the seeded generator the GPU
differential rests on.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-g"]
PENDING_FUNCS = ["fa_raw_pending_probe", "fa_raw_query_pending", "fa_raw_select_pending", "fa_raw_pending_stats"]
NO_UPPER = 0xFFFFFFFF


def _program(sanitize):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_raw_bounds" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "host_raw_bounds.hip")
    deps = [src, os.path.join(ROOT, "include", "flowagg.h")] + [os.path.join(ROOT, "flow-pipeline_amd", "csrc", f) for f in (
        "raw_bounds.cuh", "raw_pending_plan.h", "raw_select.cuh", "raw_merge.cuh", "raw.cuh", "align16.cuh")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1" if sanitize else "-O2", "-std=c++17"] + (SANITIZE if sanitize else []) + ["-o", exe, src])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_search_steps_and_classification(sanitize):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")  # (the process loads the HIP runtime, which keeps its allocations)
    res = subprocess.run([_program(sanitize)], capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0 and res.stdout.startswith("OK "), res.stdout + res.stderr[-4000:]
    assert int(re.findall(r"\d+", res.stdout)[0]) > 10 ** 8  # the search and the classification checks all ran


def classify(t, t_lo, t_hi):
    """the tests' own restatement over a part's sorted 32-bit times: 'skipped' / 'whole' / 'searched' from the first and last value"""
    upper = (1 << 32) if t_hi == NO_UPPER else t_hi
    lo, hi = int(t[0]), int(t[-1])
    if t_lo >= upper or hi < t_lo or lo >= upper:
        return "skipped"
    return "whole" if lo >= t_lo and hi < upper else "searched"


def test_the_generator_reaches_every_branch():
    """a condition on raw_query_cases.query_case, computed by the restatement alone: of the seeds 0 .. 15 at least 12 have a
    matching row, at least 8 a part that needs a search, at least 4 a whole part and at least 8 a skipped part (13, 9, 5 and 10
    when this was written)"""
    import raw_query_cases as Q
    from test_raw_parts_gpu import t32_of
    some = searched = whole = skipped = 0
    for seed in range(16):
        parts, f = Q.query_case(seed)
        some += len(Q.matching(parts, f)) > 0
        kinds = {classify(t32_of(r), f.get("t_lo", 0), f.get("t_hi", NO_UPPER)) for r in parts}
        searched += "searched" in kinds
        whole += "whole" in kinds
        skipped += "skipped" in kinds
    assert some >= 12 and searched >= 8 and whole >= 4 and skipped >= 8, (some, searched, whole, skipped)


def test_library_exports_the_pending_doors(fa):
    if not os.path.exists(fa.LIB_PATH):
        fa.build()
    L = C.CDLL(fa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "flowagg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    bound = fa.lib()
    for f in PENDING_FUNCS:
        assert hasattr(L, f), "libflowagg.so does not export %s" % f
        assert re.search(r"\bint\s+%s\s*\(" % f, code), "flowagg.h does not declare %s" % f
        assert f in fa.EXPORTS
        assert getattr(bound, f).argtypes, "%s has no argtypes" % f
    vp, sz, szp, u32 = C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_uint32
    assert list(bound.fa_raw_pending_probe.argtypes) == [vp, u32, u32, vp, sz, szp]
    assert list(bound.fa_raw_query_pending.argtypes) == [vp, C.POINTER(fa.RawQuery)]
    assert list(bound.fa_raw_select_pending.argtypes) == [vp, C.POINTER(fa.RawFilter), vp, sz, szp, szp]
    assert list(bound.fa_raw_pending_stats.argtypes) == [vp, C.POINTER(fa.RawPendingStats)]
    assert "ABI 8, addition: the pending flows_raw parts as input" in hdr
    # no new ABI version, and the sizes test_raw_query_cpu.py pins stay put
    assert bound.fa_abi_version() == 8 and C.sizeof(fa.Config) == 64 and C.sizeof(fa.Stats) == 312
    assert C.sizeof(fa.RawLoadStats) == 96 and C.sizeof(fa.RawRangeStats) == 96 and fa.RAW_PART_DTYPE.itemsize == 40
    assert C.sizeof(fa.RawFilter) == 96 and C.sizeof(fa.RawSelectStats) == 80
    assert C.sizeof(fa.RawQuery) == 104 and fa.QUERY_ROW_DTYPE.itemsize == 40 and C.sizeof(fa.RawQueryStats) == 80 and fa.RAW_RANGE_DTYPE.itemsize == 40
    # fa_raw_pending_stats_t: nine uint64_t, the header's order
    fields = ["calls", "parts_seen", "parts_skipped", "parts_whole", "parts_searched", "rows_seen", "rows_in_range", "bounds_launches", "bounds_ns"]
    assert [n for n, _ in fa.RawPendingStats._fields_] == fields and C.sizeof(fa.RawPendingStats) == 72
    assert all(t is C.c_uint64 for _, t in fa.RawPendingStats._fields_)
    m = re.search(r"typedef struct \{([^}]*)\}\s*fa_raw_pending_stats_t;", code, flags=re.S)
    assert m and re.findall(r"\b(?!uint64_t\b)[a-z_]+\b", m.group(1)) == fields
    for name in ("raw_pending_probe", "raw_query_pending", "raw_select_pending", "raw_pending_stats"):
        assert callable(getattr(fa.FlowAgg, name))


def test_the_restated_classification_on_hand_made_parts():
    t = np.array([100, 100, 105, 110], dtype=np.uint32)
    assert classify(t, 0, NO_UPPER) == "whole" and classify(t, 100, 111) == "whole" and classify(t, 100, 110) == "searched"
    assert classify(t, 111, NO_UPPER) == "skipped" and classify(t, 0, 100) == "skipped" and classify(t, 105, 105) == "skipped"
    assert classify(t, 101, 105) == "searched"  # (a range between two values: searched, and no row is in it)
    end = np.array([NO_UPPER, NO_UPPER], dtype=np.uint32)
    assert classify(end, 0, NO_UPPER) == "whole" and classify(end, 0, NO_UPPER - 1) == "skipped" and classify(end, NO_UPPER, NO_UPPER) == "whole"
