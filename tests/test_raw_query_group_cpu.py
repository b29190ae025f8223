"""CPU tests of the queries over the whole topic (include/flowagg.h "queries over the whole topic").

tests/host_raw_query_merge.hip instantiates on the host what the merge decides without a GPU: for records of every kind the fold's
key, turned into a row and back through the merge's key rebuild, is the identical TKey; the two row validations against naive
restatements; RowOpsQuery's key words against a memcmp-based comparator of the documented order (255 / 256, the families).  It is
built plain and with the host's AddressSanitizer + UBSan and run as a program.  The library's part: the new symbols are exported
and declared, their argtypes, the statistics' size, the row kinds' size; the ABI is still 8.  dist.merge_query_host and
dist.partition_rows_host for the query kinds against raw_query_cases, and the exact-k stream's precondition.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-g"]
NEW_FUNCS = ["fa_raw_query_merge_device", "fa_raw_query_merge_rows", "fa_raw_query_merge_stats", "fa_group_raw_query_pending", "fa_group_raw_query_rows",
             "fa_group_raw_query_reset"]


def _program(sanitize):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_raw_query_merge" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "host_raw_query_merge.hip")
    deps = [src, os.path.join(ROOT, "include", "flowagg.h")] + [os.path.join(ROOT, "flow-pipeline_amd", "csrc", f) for f in (
        "raw_query.cuh", "merge.cuh", "raw_select.cuh", "talkers.cuh", "keytab.cuh", "table.cuh", "rowplan.cuh", "maintenance.cuh")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1" if sanitize else "-O2", "-std=c++17"] + (SANITIZE if sanitize else []) + ["-o", exe, src])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_keys_validation_and_order(sanitize):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")  # (the process loads the HIP runtime, which keeps its allocations)
    res = subprocess.run([_program(sanitize)], capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0 and res.stdout.startswith("OK "), res.stdout + res.stderr[-4000:]
    assert int(re.findall(r"\d+", res.stdout)[0]) > 5 * 10 ** 6  # the round trips, the validations and the order all ran


def test_the_library_declares_the_doors(fa):
    L = fa.lib()
    header = open(os.path.join(ROOT, "include", "flowagg.h")).read()
    assert L.fa_abi_version() == 8 and "#define FA_ABI_VERSION 8" in header
    for name in NEW_FUNCS:
        assert name in fa.EXPORTS and hasattr(L, name) and re.search(r"\bint %s\(" % name, header), name
    assert (fa.ROWS_QUERY_WEIGHT, fa.ROWS_QUERY_KEY) == (12, 13) and "FA_ROWS_QUERY_WEIGHT = 12, FA_ROWS_QUERY_KEY = 13" in header
    assert L.fa_row_bytes(12) == L.fa_row_bytes(13) == 40 == fa.QUERY_ROW_DTYPE.itemsize and L.fa_row_bytes(14) == 0
    assert L.fa_row_bytes(7) == L.fa_row_bytes(10) == L.fa_row_bytes(11) == 0  # (unassigned, as they were)
    assert fa.ROW_DTYPES[12] is fa.QUERY_ROW_DTYPE and fa.ROW_DTYPES[13] is fa.QUERY_ROW_DTYPE and fa.ROW_DTYPES[10] is None and fa.ROW_DTYPES[11] is None
    assert C.sizeof(fa.RawQueryMergeStats) == 16 and [n for n, _ in fa.RawQueryMergeStats._fields_] == ["merge_calls", "rows_merged"]
    assert C.sizeof(fa.RawQueryStats) == 80  # (the query's own statistics did not grow)
    assert L.fa_raw_query_merge_device.argtypes[1] is C.c_uint32 and len(L.fa_group_raw_query_rows.argtypes) == 7
    for text in ("a group or dist door",):  # the three NOT-built lists no longer name what is built now
        assert text not in header
    assert fa.dist.QUERY_ROW_DTYPE == fa.QUERY_ROW_DTYPE


def test_merge_query_host_and_partition_against_the_restatement(fa):
    import raw_query_cases as Q
    import raw_query_group_cases as GC
    d = fa.dist
    for seed, n in ((1, 2), (2, 3), (3, 8)):
        rows, f = GC.seeded_stream(seed, 900)
        shares = GC.deal(rows, n)
        want = Q.matching([rows], f)
        assert len(want) > 50
        for bit in Q.G.values():
            parts = [Q.groups_of(Q.matching([s], f), bit) for s in shares]
            by_key = Q.groups_of(want, bit)
            for order in (Q.O_WEIGHT, Q.O_KEY):
                got = d.merge_query_host([p[::-1] for p in parts], order)  # (any input order)
                assert got.dtype == fa.QUERY_ROW_DTYPE and got.tobytes() == Q.ordered(by_key, order).tobytes(), (seed, bit, order)
            # the owner is a function of (value, key, etype) alone: every share's rows of one group name one owner, and it is in range
            for world in (1, 3, 8):
                owners = {}
                for p in parts:
                    dest = d.partition_rows_host(p, fa.ROWS_QUERY_WEIGHT, world)
                    assert (dest == d.partition_rows_host(p, fa.ROWS_QUERY_KEY, world)).all() and ((dest >= 0) & (dest < world)).all()
                    for r, o in zip(p, dest):
                        assert owners.setdefault((int(r["value"]), r["key"].tobytes(), int(r["etype"])), int(o)) == int(o)
                if world == 8 and len(by_key) >= 64:
                    assert len(set(owners.values())) > 1  # (the hash spreads)
    assert len(d.merge_query_host([], 0)) == 0 and len(d.merge_query_host([np.zeros(0, dtype=fa.QUERY_ROW_DTYPE)], 1)) == 0
    with pytest.raises(ValueError):
        d.merge_query_host([], 2)


def test_merge_query_host_by_hand(fa):
    """255 / 256 and 65535 / 65536 in numeric order; a tie in weight decided by the value; a sum that wraps; value is kept"""
    import raw_query_cases as Q
    def row(value, weight, count=1):
        r = np.zeros(1, dtype=Q.ROW)
        r["value"], r["weight"], r["count"] = value, weight, count
        return r
    a = np.concatenate([row(256, 5), row(255, 5), row(65536, (1 << 63) + 1)])
    b = np.concatenate([row(65535, 9), row(65536, (1 << 63) + 2, 4)])
    by_key = fa.dist.merge_query_host([a, b], Q.O_KEY)
    assert [(int(r["value"]), int(r["weight"]), int(r["count"])) for r in by_key] == [(255, 5, 1), (256, 5, 1), (65535, 9, 1), (65536, 3, 5)]
    by_weight = fa.dist.merge_query_host([a, b], Q.O_WEIGHT)
    assert [int(r["value"]) for r in by_weight] == [65535, 255, 256, 65536]


def test_the_exact_k_stream():
    import raw_query_group_cases as GC
    assert GC.exact_k_precondition(GC.exact_k_members()) == 30
