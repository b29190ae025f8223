"""Shared by tests/test_raw_query_gpu.py and tests/test_raw_query_cpu.py: the tests' OWN numpy restatement of a grouped query
(include/flowagg.h "grouped queries over flows_raw parts").  The rows that match come from raw_select_cases.match; the canonical
address rule, the minute and the two orders are restated here.  Nothing comes from the code under test."""
import numpy as np

import raw_select_cases as S

G = dict(SRC_ADDR=1, DST_ADDR=2, SRC_PORT=4, DST_PORT=8, MINUTE=16, SRC_AS=32, DST_AS=64, PROTO=128, TOTAL=256)
G_ALL = 511
O_WEIGHT, O_KEY = 0, 1
ROW = np.dtype([("key", "u1", (16,)), ("etype", "<u4"), ("value", "<u4"), ("weight", "<u8"), ("count", "<u8")])  # fa_query_row
SCALAR_FIELD = {4: "src_port", 8: "dst_port", 32: "src_as", 64: "dst_as", 128: "proto"}
assert ROW.itemsize == 40


def keys_of(r, group):
    """ROWS, one kind -> (key uint8[n, 16], etype uint32[n], value uint32[n]) of every row"""
    n = len(r)
    key, etype, value = np.zeros((n, 16), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    if group in (1, 2):  # the rendered string's preimage: EType 0x800 -> the first four bytes, family 0x800; else all 16 bytes, family 0
        key[:] = r["src_addr" if group == 1 else "dst_addr"]
        v4 = r["etype"] == 0x800
        key[v4, 4:] = 0
        etype[v4] = 0x800
    elif group == 16:  # toStartOfMinute of the stored 32-bit TimeFlowStart
        t = (r["time_flow_start"] & np.uint64(0xFFFFFFFF)).astype(np.uint64)
        value[:] = (t - t % np.uint64(60)).astype(np.uint32)
    elif group != 256:
        value[:] = r[SCALAR_FIELD[group]]
    return key, etype, value


def groups_of(r, group):
    """the matching rows, one kind -> its fa_query_rows in FA_RAW_O_KEY order: value ascending (numeric), key bytes ascending
    (memcmp), etype ascending; weight = sum(Bytes*SamplingRate) mod 2^64, count = count()"""
    key, etype, value = keys_of(r, group)
    if not len(r):
        return np.zeros(0, dtype=ROW)
    packed = np.concatenate([value.astype(">u4").view(np.uint8).reshape(-1, 4), key, etype.astype(">u4").view(np.uint8).reshape(-1, 4)], axis=1)
    uniq, inv = np.unique(packed, axis=0, return_inverse=True)  # (rows sorted as byte strings: big-endian value, key, big-endian etype)
    inv = inv.reshape(-1)
    with np.errstate(over="ignore"):
        w = r["bytes"].astype(np.uint64) * r["sampling_rate"].astype(np.uint64)
        weight = np.zeros(len(uniq), dtype=np.uint64)
        np.add.at(weight, inv, w)
    out = np.zeros(len(uniq), dtype=ROW)
    out["value"] = np.ascontiguousarray(uniq[:, :4]).view(">u4").reshape(-1)
    out["key"] = uniq[:, 4:20]
    out["etype"] = np.ascontiguousarray(uniq[:, 20:]).view(">u4").reshape(-1)
    out["weight"], out["count"] = weight, np.bincount(inv, minlength=len(uniq))
    return out


def ordered(rows_in_key_order, order):
    """FA_RAW_O_WEIGHT: weight descending, ties in FA_RAW_O_KEY order"""
    if order == O_KEY:
        return rows_in_key_order
    return rows_in_key_order[np.argsort(~rows_in_key_order["weight"], kind="stable")]


def matching(parts, f):
    """the parts' rows, a filter (raw_select_cases' dict, without a limit) -> the rows a query folds"""
    rows = np.concatenate(parts) if len(parts) else np.zeros(0, dtype=S.ROWS)
    return rows[S.match(rows, f)]


def check_reads(a, want_rows, groups, ks=(1, 3)):
    """every kind of `groups` of ctx a's result against the restatement: k = 0 in both orders row for row, byte for byte; the cuts"""
    total = 0
    for name, bit in G.items():
        if not groups & bit:
            continue
        by_key = groups_of(want_rows, bit)
        total += len(by_key)
        for order in (O_WEIGHT, O_KEY):
            want = ordered(by_key, order)
            got = a.raw_query_rows(bit, 0, order)
            assert got.dtype.itemsize == 40 and got.tobytes() == want.tobytes(), (name, order, len(got), len(want))
            for k in ks:
                assert a.raw_query_rows(bit, k, order).tobytes() == want[:k].tobytes(), (name, order, k)
    return total


def query_case(seed):
    """raw_select_cases.fuzz_case without its limit"""
    parts, f = S.fuzz_case(seed)
    f = {k: v for k, v in f.items() if k != "limit"}
    return parts, f
