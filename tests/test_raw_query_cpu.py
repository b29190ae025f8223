"""CPU tests of grouped queries over flows_raw parts (include/flowagg.h "grouped queries over flows_raw parts").

tests/host_raw_query.hip instantiates on the host what a query decides without a GPU (csrc/raw_query.cuh): the key text - the
canonical address words, the minute, the scalar pack and unpack, packed order == numeric order over random and edge values -
against naive restatements over bytes; the rows of a launch against table_room_fits for 1 .. 9 kinds and the host's chunk loop
restated; the persistent walk over the tiles; and every byte the fold kernel loads for a slice (predicate columns, key columns,
Bytes, SamplingRate) against the blocks stages B and C of a ranged load planned, over the row counts of host_raw_range.hip's grid.
It is built plain and with the host's AddressSanitizer + UBSan and run as a program.  The library's part: the five new symbols are
exported and declared, their argtypes, the structures' sizes and member lists, the ABI is still 8.  And a condition on the seeded
generator the GPU differential rests on.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-g"]
QUERY_FUNCS = ["fa_raw_query", "fa_raw_query_rows", "fa_raw_query_rows_device", "fa_raw_query_reset", "fa_raw_query_stats"]


def _program(sanitize):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_raw_query" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "host_raw_query.hip")
    deps = [src, os.path.join(ROOT, "include", "flowagg.h")] + [os.path.join(ROOT, "flow-pipeline_amd", "csrc", f) for f in (
        "raw_query.cuh", "raw_select.cuh", "raw_merge.cuh", "raw_range_plan.h", "raw.cuh", "align16.cuh", "talkers.cuh", "keytab.cuh", "table.cuh", "table_room.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1" if sanitize else "-O2", "-std=c++17"] + (SANITIZE if sanitize else []) + ["-o", exe, src])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_keys_room_walk_and_loads(sanitize):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")  # (the process loads the HIP runtime, which keeps its allocations)
    res = subprocess.run([_program(sanitize)], capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0 and res.stdout.startswith("OK "), res.stdout + res.stderr[-4000:]
    assert int(re.findall(r"\d+", res.stdout)[0]) > 10 ** 7  # the key, room, walk and load checks all ran


def test_the_generator_matches_rows_and_groups():
    """a condition on raw_select_cases.fuzz_case, computed by the restatement alone: of the seeds 0 .. 31 at least 24 have a matching
    row and at least 16 have two or more SrcPort groups (25 and 19 when this was written)"""
    import raw_query_cases as Q
    some = ports = 0
    for seed in range(32):
        parts, f = Q.query_case(seed)
        assert "limit" not in f
        want = Q.matching(parts, f)
        some += len(want) > 0
        ports += len(Q.groups_of(want, Q.G["SRC_PORT"])) >= 2
    assert some >= 24 and ports >= 16, (some, ports)


def test_the_restatement_on_a_hand_made_case():
    """raw_query_cases against values worked out by hand: the grouping rule, a wrapping sum, the numeric order"""
    import raw_query_cases as Q
    import raw_select_cases as S
    r = np.zeros(5, dtype=S.ROWS)
    r["src_addr"][:] = np.arange(1, 17, dtype=np.uint8)
    r["src_addr"][1, 4:] = 0xEE
    r["etype"] = [0x800, 0x800, 0x86DD, 0, 0x1234]
    r["bytes"], r["sampling_rate"] = [1 << 63, 1 << 63, 5, 6, 7], [1, 1, 2, 2, 2]
    r["dst_port"] = [256, 255, 65536, 255, 256]
    r["time_flow_start"] = [59, 60, 61, 0xFFFFFFFF, 119]
    src = Q.groups_of(r, Q.G["SRC_ADDR"])
    assert [(bytes(x["key"]), int(x["etype"]), int(x["weight"]), int(x["count"])) for x in src] == [
        (bytes([1, 2, 3, 4]) + bytes(12), 0x800, 0, 2), (bytes(range(1, 17)), 0, 36, 3)]
    dp = Q.groups_of(r, Q.G["DST_PORT"])
    assert dp["value"].tolist() == [255, 256, 65536] and dp["count"].tolist() == [2, 2, 1] and dp["weight"].tolist() == [(1 << 63) + 12, (1 << 63) + 14, 10]
    assert Q.ordered(dp, Q.O_WEIGHT)["value"].tolist() == [256, 255, 65536]
    assert Q.groups_of(r, Q.G["MINUTE"])["value"].tolist() == [0, 60, 4294967280]
    tot = Q.groups_of(r, Q.G["TOTAL"])
    assert len(tot) == 1 and int(tot["weight"][0]) == 36 and int(tot["count"][0]) == 5 and not tot["key"].any()
    assert len(Q.groups_of(r[:0], Q.G["TOTAL"])) == 0


def test_library_exports_the_query_doors(fa):
    if not os.path.exists(fa.LIB_PATH):
        fa.build()
    L = C.CDLL(fa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "flowagg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    bound = fa.lib()
    for f in QUERY_FUNCS:
        assert hasattr(L, f), "libflowagg.so does not export %s" % f
        assert re.search(r"\bint\s+%s\s*\(" % f, code), "flowagg.h does not declare %s" % f
        assert f in fa.EXPORTS
        assert getattr(bound, f).argtypes, "%s has no argtypes" % f
    vp, sz, szp = C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)
    assert list(bound.fa_raw_query.argtypes) == [vp, vp, sz, C.POINTER(fa.RawQuery)]
    assert list(bound.fa_raw_query_rows.argtypes) == [vp, C.c_uint32, C.c_int, sz, vp, sz, szp]
    assert list(bound.fa_raw_query_rows_device.argtypes) == [vp, C.c_uint32, C.c_int, sz, C.POINTER(C.c_void_p), szp]
    assert list(bound.fa_raw_query_reset.argtypes) == [vp]
    assert list(bound.fa_raw_query_stats.argtypes) == [vp, C.POINTER(fa.RawQueryStats)]
    assert "ABI 8, addition: grouped queries over flows_raw parts" in hdr
    # no new ABI version, and the pinned sizes stay put - the select's among them
    assert bound.fa_abi_version() == 8 and C.sizeof(fa.Config) == 64 and C.sizeof(fa.Stats) == 312
    assert C.sizeof(fa.RawLoadStats) == 96 and C.sizeof(fa.RawRangeStats) == 96 and fa.RAW_PART_DTYPE.itemsize == 40
    assert C.sizeof(fa.RawFilter) == 96 and C.sizeof(fa.RawSelectStats) == 80
    # fa_raw_query_t: 104 bytes; fa_query_row: 40 bytes, the header's member list and the offsets it gives
    assert C.sizeof(fa.RawQuery) == 104 and [n for n, _ in fa.RawQuery._fields_] == ["where", "groups", "flags"]
    assert [getattr(fa.RawQuery, n).offset for n in ("where", "groups", "flags")] == [0, 96, 100]
    assert re.search(r"typedef struct \{ fa_raw_filter where; uint32_t groups, flags; \} fa_raw_query_t;", code)
    assert re.search(r"typedef struct \{ uint8_t key\[16\]; uint32_t etype, value; uint64_t weight, count; \} fa_query_row;", code)
    d = fa.QUERY_ROW_DTYPE
    assert d.itemsize == 40 and d.names == ("key", "etype", "value", "weight", "count") and [d.fields[n][1] for n in d.names] == [0, 16, 20, 24, 32]
    # the constants: no FA_RAW_F_ prefix (the select's test pins those), the header's values, the Python names
    bits = dict(re.findall(r"#define FA_RAW_G_([A-Z_]+)\s+(\d+)u", code))
    want = dict(SRC_ADDR=1, DST_ADDR=2, SRC_PORT=4, DST_PORT=8, MINUTE=16, SRC_AS=32, DST_AS=64, PROTO=128, TOTAL=256)
    assert {k: int(v) for k, v in bits.items() if k != "ALL"} == want and int(bits["ALL"]) == sum(want.values()) == fa.RAW_G_ALL
    assert all(getattr(fa, "RAW_G_" + k) == v for k, v in want.items())
    assert re.search(r"#define FA_RAW_Q_KEEP 1u", code) and re.search(r"#define FA_RAW_O_WEIGHT 0\b", code) and re.search(r"#define FA_RAW_O_KEY\s+1\b", code)
    assert (fa.RAW_Q_KEEP, fa.RAW_O_WEIGHT, fa.RAW_O_KEY) == (1, 0, 1)
    assert int(dict(re.findall(r"#define FA_RAW_F_([A-Z_]+) (\d+)u", code))["ALL"]) == 2047
    # fa_raw_query_stats_t: ten uint64_t, the header's order
    fields = ["calls", "rows_scanned", "rows_matched", "updates", "absorbed", "groups", "grows", "launches", "fold_ns", "order_ns"]
    assert [n for n, _ in fa.RawQueryStats._fields_] == fields and C.sizeof(fa.RawQueryStats) == 80
    m = re.search(r"typedef struct \{([^}]*)\}\s*fa_raw_query_stats_t;", code, flags=re.S)
    assert m and re.findall(r"\b(?!uint64_t\b)[a-z_]+\b", m.group(1)) == fields
    for name in ("raw_query", "raw_query_rows", "raw_query_rows_device", "raw_query_reset", "raw_query_stats"):
        assert callable(getattr(fa.FlowAgg, name))
