"""Shared by tests/test_raw_query_group_gpu.py, tests/test_raw_query_group_cpu.py and tests/test_dist_query_gpu.py: the record
streams of the queries over the whole topic (include/flowagg.h "queries over the whole topic"), dealt to members, and the
conditions on them that the restatement of raw_query_cases alone decides.  Nothing here comes from the code under test."""
import numpy as np

import raw_query_cases as Q
import raw_select_cases as S
from raw_select_cases import MID
from test_raw_parts_gpu import DAY

V4, V6 = 0x800, 0x86DD


def deal(rows, n):
    """records round-robin to n members (each share keeps the records' order, so it is sorted as they are)"""
    return [rows[i::n] for i in range(n)]


def seeded_stream(seed, n=1800):
    """records of two Dates, IPv4 and IPv6 with the same leading bytes (make_rows draws the EType apart from the address), ports at
    and above 2^16 -> (rows, a filter: a time range that cuts both parts, and one WHERE condition)"""
    rng = np.random.default_rng(9100 + seed)
    pool = S.address_pool(rng, 24)
    parts = [S.make_rows(rng, n // 3, t0=MID + 1000, span=600, pool=pool), S.make_rows(rng, n - n // 3, t0=MID + DAY + 1000, span=600, pool=pool, against=True)]
    rows = np.concatenate(parts)
    f = dict(t_lo=MID + 1200, t_hi=MID + DAY + 1400, proto=6)
    return rows, f


def made_rows(specs, t0=MID + 1000):
    """[(16 address bytes, EType, weight, SrcPort)] -> records of one Date with SamplingRate 1 and Bytes = weight, one per spec, in order"""
    r = S.make_rows(np.random.default_rng(5), len(specs), t0=t0, span=1)
    for i, (addr, etype, weight, port) in enumerate(specs):
        r["src_addr"][i] = np.frombuffer(bytes(addr), dtype=np.uint8)
        r["etype"][i], r["bytes"][i], r["sampling_rate"][i], r["src_port"][i] = etype, weight, 1, port
    return r


def addr(*head):
    return bytes(head) + bytes(16 - len(head))


EXACT_K = 2


def exact_k_members():
    """Three members, k = 2, GROUP BY SrcAddr.  X is third in every member (10 behind 12 and 11) and first overall (30).  Ties across
    members: T4 and T6 are the same 16 bytes under the two families with 9 + 9 each - only the etype decides -, and P and Q total
    7 + 7 each - only the key bytes decide.  A_i, B_i live in one member, X in all three."""
    x = addr(10, 0, 0, 1)
    t = addr(10, 0, 0, 2)
    p, q = addr(0x20, 1, 0, 0, 0, 0, 0, 7), addr(0x20, 1, 0, 0, 0, 0, 0, 6)
    members = []
    for i in range(3):
        specs = [(x, V4, 10, 80), (addr(172, 16, i, 1), V4, 12, 255), (addr(172, 16, i, 2), V6, 11, 256)]
        if i < 2:
            specs += [(t, V4, 9, 65535), (t, V6, 9, 65536), (p, V6, 7, 53), (q, V6, 7, 53)]
        members.append(made_rows(specs))
    return members


def exact_k_precondition(members, k=EXACT_K, group=Q.G["SRC_ADDR"]):
    """the global first key by weight is in NO member's own first k - decided by the restatement alone"""
    first = Q.ordered(Q.groups_of(np.concatenate(members), group), Q.O_WEIGHT)[0]
    ident = (first["key"].tobytes(), int(first["etype"]), int(first["value"]))
    for m in members:
        own = Q.ordered(Q.groups_of(m, group), Q.O_WEIGHT)[:k]
        assert len(own) == k and all((r["key"].tobytes(), int(r["etype"]), int(r["value"])) != ident for r in own)
    total = Q.ordered(Q.groups_of(np.concatenate(members), group), Q.O_WEIGHT)
    w = total["weight"]
    ties = [(a, b) for a, b in zip(total[:-1], total[1:]) if a["weight"] == b["weight"]]
    assert any(a["key"].tobytes() == b["key"].tobytes() and a["etype"] != b["etype"] for a, b in ties), "a tie only the etype decides"
    assert any(a["key"].tobytes() != b["key"].tobytes() and a["etype"] == b["etype"] for a, b in ties), "a tie only the key bytes decide"
    return int(w[0])


def scalar_edge_members():
    """two members whose SrcPort values 255 / 256 and 65535 / 65536 put byte order against numeric order, one port per member and
    one in both; and a key whose two weights sum past 2^64"""
    a = addr(192, 0, 2, 1)
    m0 = made_rows([(a, V4, (1 << 63) + 5, 255), (a, V4, 3, 65536), (addr(192, 0, 2, 9), V4, 1, 65535)])
    m1 = made_rows([(a, V4, (1 << 63) + 6, 256), (a, V4, 4, 65536), (addr(192, 0, 2, 9), V6, 1, 255)])
    return [m0, m1]
