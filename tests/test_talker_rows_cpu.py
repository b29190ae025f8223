"""CPU side of the talker row kinds (FA_ROWS_TALKERS_SRC / _DST = 8 / 9; include/flowagg.h "ABI 8, addition"): the row size,
the two new entry points in header, library and binding, and the numpy restatements dist.py keeps of the device code -
the owner of a row (merge.cuh row_dest) and the merge (RowOpsTalk)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1


def test_row_bytes_of_the_new_kinds_and_the_hole(fa):
    if not os.path.exists(fa.LIB_PATH):
        fa.build()
    L = fa.lib()
    assert (fa.ROWS_TALKERS_SRC, fa.ROWS_TALKERS_DST) == (8, 9)
    assert L.fa_row_bytes(8) == L.fa_row_bytes(9) == 40 == fa.TALKER_ROW_DTYPE.itemsize
    assert L.fa_row_bytes(7) == 0 and L.fa_row_bytes(10) == 0 and L.fa_row_bytes(-1) == 0
    assert fa.ROW_DTYPES[8] is fa.TALKER_ROW_DTYPE and fa.ROW_DTYPES[9] is fa.TALKER_ROW_DTYPE and fa.ROW_DTYPES[7] is None
    assert L.fa_abi_version() == 8  # an addition: the ABI number does not move


def test_header_exports_and_binding_agree_on_the_new_calls(fa):
    if not os.path.exists(fa.LIB_PATH):
        fa.build()
    txt = open(os.path.join(ROOT, "include", "flowagg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = C.CDLL(fa.LIB_PATH)
    for name in ("fa_merge_talkers_device", "fa_group_top_talkers"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in fa.EXPORTS and hasattr(L, name), name
        assert getattr(fa.lib(), name).argtypes, name
    assert re.search(r"FA_ROWS_TALKERS_SRC\s*=\s*8\s*,\s*FA_ROWS_TALKERS_DST\s*=\s*9", code)
    assert not re.search(r"FA_ROWS_\w+\s*=\s*7\b", code)  # kind 7 stays unassigned ...
    assert re.search(r"7[^\n]*unassigned", txt)             # ... and the header says so
    assert re.search(r"#define\s+FA_ABI_VERSION\s+8\b", code)
    assert callable(fa.FlowAgg.merge_talkers_device) and callable(fa.FlowGroup.top_talkers)
    assert callable(fa.dist.top_talkers_merged) and callable(fa.dist.merge_talkers_host)


def _rows(fa, n, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=fa.TALKER_ROW_DTYPE)
    r["key"] = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    r["etype"] = rng.choice(np.array([0, 0x800], dtype=np.uint32), size=n)
    r["key"][r["etype"] == 0x800, 4:] = 0
    r["weight"] = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    r["count"] = rng.integers(1, 1000, size=n, dtype=np.uint64)
    return r


def test_partition_rows_host_on_talker_rows(fa):
    part = fa.dist.partition_rows_host
    rows = _rows(fa, 5000, 1)
    for kind in (fa.ROWS_TALKERS_SRC, fa.ROWS_TALKERS_DST):
        for world in (1, 2, 3, 8, 1024):
            own = part(rows, kind, world)
            assert own.min() >= 0 and own.max() < world
            if world == 1:
                assert not own.any()
            else:
                assert len(np.unique(own)) > min(world, 64) // 2  # (spread over the owners)
            # the owner is a function of key and etype alone
            other = rows.copy()
            other["weight"] = ~rows["weight"]
            other["count"] += np.uint64(7)
            other["_pad"] = 0xdeadbeef
            assert np.array_equal(part(other, kind, world), own)
    # both talker kinds and nothing else: the same function (one RowOps instantiation)
    assert np.array_equal(part(rows, 8, 8), part(rows, 9, 8))
    # the same 16 bytes under the two families are two keys: their owners may differ
    a = np.zeros(4096, dtype=fa.TALKER_ROW_DTYPE)
    a["key"][:, :4] = np.arange(4096, dtype=np.uint32).view(np.uint8).reshape(-1, 4)
    b = a.copy()
    b["etype"] = 0x800
    assert (part(a, 8, 8) != part(b, 8, 8)).any()
    # ... and the talker words are not the top-k words: etype takes part
    words = fa.dist._key_words(b, 8)
    assert len(words) == 3 and np.array_equal(words[0], np.full(4096, 0x800, dtype=np.uint64))
    assert len(fa.dist._key_words(np.zeros(1, dtype=fa.TOPK_DTYPE), fa.ROWS_TOPK_SRC)) == 2
    # the restatement, restated once more in plain Python for a few rows (merge.cuh: row_dest, mix64)
    def mix(z):
        z ^= z >> 30
        z = z * 0xbf58476d1ce4e5b9 & U64
        z ^= z >> 27
        z = z * 0x94d049bb133111eb & U64
        return z ^ (z >> 31)
    for r, own in zip(rows[:50], part(rows[:50], 8, 3)):
        k = r["key"].tobytes()
        h = 0x9E3779B97F4A7C15
        for w in (int(r["etype"]), int.from_bytes(k[8:], "big"), int.from_bytes(k[:8], "big")):
            h = mix(h ^ w)
        assert ((h >> 32) * 3) >> 32 == own


def test_merge_talkers_host_against_a_dict(fa):
    base = _rows(fa, 300, 2)
    rng = np.random.default_rng(3)
    parts = []
    for p in range(4):
        r = base[rng.integers(0, len(base), size=500)].copy()
        r["weight"] = rng.integers(0, 1 << 64, size=len(r), dtype=np.uint64)  # (sums of a few of these wrap)
        r["count"] = rng.integers(0, 1 << 64, size=len(r), dtype=np.uint64)
        r["_pad"] = p + 1  # (dropped by the merge)
        parts.append(r)
    # one group whose sum wraps exactly: (2^64 - 1) + 2 = 1
    w = np.zeros(2, dtype=fa.TALKER_ROW_DTYPE)
    w["key"][:, 0] = 0xfe
    w["weight"] = [U64, 2]
    w["count"] = [U64, 3]
    parts.append(w)
    parts.append(np.zeros(0, dtype=fa.TALKER_ROW_DTYPE))
    groups = {}
    for r in np.concatenate(parts):
        k = (r["key"].tobytes(), int(r["etype"]))
        a = groups.get(k, (0, 0))
        groups[k] = ((a[0] + int(r["weight"])) & U64, (a[1] + int(r["count"])) & U64)
    assert groups[(w["key"][0].tobytes(), 0)] == (1, 2)
    want = sorted(groups.items(), key=lambda kv: (-kv[1][0], kv[0][0], kv[0][1]))
    got = fa.dist.merge_talkers_host(parts)
    assert len(got) == len(want) and not got["_pad"].any()
    for g, ((key, et), (wt, cnt)) in zip(got, want):
        assert (g["key"].tobytes(), int(g["etype"]), int(g["weight"]), int(g["count"])) == (key, et, wt, cnt)
    assert len(fa.dist.merge_talkers_host([])) == 0 and fa.dist.merge_talkers_host([]).dtype == fa.TALKER_ROW_DTYPE
    # merging is associative: parts merged pairwise first give the same rows
    two = [fa.dist.merge_talkers_host(parts[:2]), fa.dist.merge_talkers_host(parts[2:])]
    assert fa.dist.merge_talkers_host(two).tobytes() == got.tobytes()
