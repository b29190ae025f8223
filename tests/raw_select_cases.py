"""Shared by tests/test_raw_select_gpu.py: the tests' OWN numpy restatement of fa_raw_filter (include/flowagg.h "selecting rows of
flows_raw parts"), the seeded row and filter generators, and the expected output parts - rows picked by the restatement, encoded by
encode_part of tests/test_raw_parts_gpu.py.  Nothing here comes from the code under test.

A filter is a dict of FlowAgg.raw_select's keywords: t_lo, t_hi, flow_start=(lo, hi), src_as, dst_as, etype, proto,
src_port=(lo, hi), dst_port=(lo, hi), src_net=(16 bytes, prefix_len), dst_net, either, limit, count_only."""
import numpy as np

from test_raw_parts_gpu import D0, DAY, encode_part, t32_of

NO_UPPER = 0xFFFFFFFF
MID = D0 * DAY
# rows of a part, with the fields encode_part reads
ROWS = np.dtype([("time_received", "<u8"), ("time_flow_start", "<u8"), ("sequence_num", "<u4"), ("sampling_rate", "<u8"), ("sampler_address", "u1", (16,)),
                 ("src_addr", "u1", (16,)), ("dst_addr", "u1", (16,)), ("src_as", "<u4"), ("dst_as", "<u4"), ("etype", "<u4"), ("proto", "<u4"),
                 ("src_port", "<u4"), ("dst_port", "<u4"), ("bytes", "<u8"), ("packets", "<u8")])
# what spill.read_native calls a column -> the row field
FIELDS = {"TimeReceived": "time_received", "TimeFlowStart": "time_flow_start", "SequenceNum": "sequence_num", "SamplingRate": "sampling_rate",
          "SamplerAddress": "sampler_address", "SrcAddr": "src_addr", "DstAddr": "dst_addr", "SrcAS": "src_as", "DstAS": "dst_as", "EType": "etype",
          "Proto": "proto", "SrcPort": "src_port", "DstPort": "dst_port", "Bytes": "bytes", "Packets": "packets"}
PORTS = np.array([0, 53, 80, 443, 65535, 65536, 0xFFFFFFFF], dtype=np.uint32)


def rows_of_block(block):
    """one block of spill.read_native -> ROWS"""
    r = np.zeros(len(block["TimeReceived"]), dtype=ROWS)
    for name, field in FIELDS.items():
        r[field] = block[name]
    return r


def in_range(t, lo, hi):
    """lo <= t < hi over 32-bit times; hi = 0xFFFFFFFF: to the end, that second included"""
    t = t.astype(np.uint64)
    return (t >= lo) & ((t < hi) | (hi == NO_UPPER))


def prefix_eq(addr, net):
    """addr: uint8[n, 16]; net = (16 bytes, prefix_len): the first prefix_len bits, from byte 0 and most significant bit first"""
    want, plen = net
    bits = np.unpackbits(np.ascontiguousarray(addr), axis=1)  # (most significant bit first)
    ref = np.unpackbits(np.frombuffer(bytes(want), dtype=np.uint8))
    return (bits[:, :plen] == ref[:plen]).all(axis=1)


def _direction(r, f, s, d):
    """P(s, d): the AS, port and address conditions that are set, the src_* members on side s, the dst_* members on side d"""
    ok = np.ones(len(r), dtype=bool)
    for side, who in (("src", s), ("dst", d)):
        if f.get(side + "_as") is not None:
            ok &= r[who + "_as"] == f[side + "_as"]
        if f.get(side + "_port") is not None:
            lo, hi = f[side + "_port"]
            ok &= (r[who + "_port"].astype(np.uint64) >= lo) & (r[who + "_port"].astype(np.uint64) <= hi)
        if f.get(side + "_net") is not None:
            ok &= prefix_eq(r[who + "_addr"], f[side + "_net"])
    return ok


def match(r, f):
    """ROWS, a filter -> the boolean mask of the rows that match (the limit is not applied here)"""
    ok = in_range(t32_of(r), f.get("t_lo", 0), f.get("t_hi", NO_UPPER))
    if f.get("flow_start") is not None:
        ok &= in_range((r["time_flow_start"] & np.uint64(0xFFFFFFFF)).astype(np.uint32), *f["flow_start"])
    if f.get("etype") is not None:
        ok &= r["etype"] == f["etype"]
    if f.get("proto") is not None:
        ok &= r["proto"] == f["proto"]
    way = _direction(r, f, "src", "dst")
    if f.get("either"):
        way |= _direction(r, f, "dst", "src")
    return ok & way


def expected(parts, f):
    """the input parts' rows (a list of ROWS, each one sorted part of one Date), a filter -> [(date, rows, bytes)] as
    check_parts of tests/test_raw_parts_gpu.py takes it: one output part per input part with a match, the limit counted over the
    call in input order"""
    left = f.get("limit") or (1 << 62)
    out = []
    for r in parts:
        sel = r[match(r, f)][:left]
        if len(sel):
            left -= len(sel)
            out.append((int(t32_of(sel)[0]) // DAY, sel, encode_part(sel)))
    return out


# ---- generators ---------------------------------------------------------------------------------------------------------------------
def address_pool(rng, k=12):
    """k addresses that share prefixes of many lengths: each is an earlier one with one bit flipped"""
    pool = [rng.integers(0, 256, 16, dtype=np.uint8)]
    flips = [0, 127, 64, 33, 24, 9, 120, 63, 8, 31, 32, 65, 7, 1]
    while len(pool) < k:
        a = pool[int(rng.integers(0, len(pool)))].copy()
        bit = flips[len(pool) % len(flips)]
        a[bit // 8] ^= 0x80 >> (bit % 8)
        pool.append(a)
    return np.stack(pool)


def make_rows(rng, n, t0=MID + 1000, span=1000, pool=None, against=False):
    """n rows of one Date, TimeReceived ascending over [t0, t0 + span) with runs of equal times; the filterable columns from small
    sets, so that every condition selects some rows and not all.  against: TimeFlowStart runs against TimeReceived."""
    pool = address_pool(rng) if pool is None else pool
    r = np.zeros(n, dtype=ROWS)
    t = np.sort(rng.integers(t0, t0 + max(span, 1), n)).astype(np.uint64)
    r["time_received"] = t
    r["time_flow_start"] = (2 * t0 + span - t) if against else t - rng.integers(0, 90, n).astype(np.uint64)
    r["sequence_num"] = np.arange(n)
    r["sampling_rate"] = rng.integers(1, 5000, n)
    r["sampler_address"] = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    r["src_addr"] = pool[rng.integers(0, len(pool), n)]
    r["dst_addr"] = pool[rng.integers(0, len(pool), n)]
    r["src_as"] = rng.integers(64500, 64504, n)
    r["dst_as"] = rng.integers(64500, 64504, n)
    r["etype"] = np.where(rng.integers(0, 3, n) == 0, 0x800, 0x86DD)
    r["proto"] = np.array([6, 17, 1], dtype=np.uint32)[rng.integers(0, 3, n)]
    r["src_port"] = PORTS[rng.integers(0, len(PORTS), n)]
    r["dst_port"] = PORTS[rng.integers(0, len(PORTS), n)]
    r["bytes"] = rng.integers(40, 1 << 40, n)
    r["packets"] = rng.integers(1, 1 << 20, n)
    return r


def random_filter(rng, rows, pool):
    """a filter of one to three conditions drawn from the values make_rows draws from, over a time range inside the rows' own"""
    t = np.sort(t32_of(rows))
    tfs = np.sort((rows["time_flow_start"] & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    i, j = sorted(int(x) for x in rng.integers(0, len(t), 2))  # (bounds at rows' own times: Dates lie a day apart, a random second hits none)
    f = dict(t_lo=int(t[i]), t_hi=int(t[j]) + int(rng.integers(0, 2)) if rng.integers(0, 4) else NO_UPPER)
    if rng.integers(0, 5) == 0:
        f = dict(t_lo=0, t_hi=NO_UPPER)
    lens = (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128)
    kinds = ["flow_start", "src_as", "dst_as", "etype", "proto", "src_port", "dst_port", "src_net", "dst_net"]
    for kind in (str(k) for k in rng.choice(kinds, size=int(rng.integers(1, 4)), replace=False)):
        if kind == "flow_start":
            x, y = sorted(int(v) for v in rng.integers(0, len(tfs), 2))
            f[kind] = (int(tfs[x]), int(tfs[y]) + 1)
        elif kind in ("src_as", "dst_as"):
            f[kind] = int(rng.integers(64500, 64504))
        elif kind == "etype":
            f[kind] = 0x800 if rng.integers(0, 2) else 0x86DD
        elif kind == "proto":
            f[kind] = int((6, 17, 1)[int(rng.integers(0, 3))])
        elif kind in ("src_port", "dst_port"):
            x, y = sorted(int(v) for v in PORTS[rng.integers(0, len(PORTS), 2)])
            f[kind] = (x, y if rng.integers(0, 2) else x)
        else:
            addr = pool[int(rng.integers(0, len(pool)))].copy()
            plen = int(lens[int(rng.integers(0, len(lens)))])
            for bit in range(plen, 128):  # the bits behind the prefix are ignored
                if rng.integers(0, 2):
                    addr[bit // 8] ^= 0x80 >> (bit % 8)
            f[kind] = (bytes(addr), plen)
    if rng.integers(0, 2):
        f["either"] = True
    if rng.integers(0, 4) == 0:
        f["limit"] = int(rng.integers(1, max(2, len(rows))))
    return f


def fuzz_case(seed):
    """-> (the parts' rows, the filter): one to four parts over up to three Dates"""
    rng = np.random.default_rng(7000 + seed)
    pool = address_pool(rng)
    parts = []
    for i in range(int(rng.integers(1, 5))):
        n = int(rng.choice([1, 2, 63, 64, 65, 200, 256, 257, 700, 1500, 5000]))
        day = int(rng.integers(0, 3))
        parts.append(make_rows(rng, n, t0=MID + day * DAY + 1000, span=int(rng.choice([1, 30, 1000])), pool=pool, against=bool(rng.integers(0, 2))))
    parts.sort(key=lambda r: int(r["time_received"][0]) // DAY)  # (ascending Date, as a take delivers them; equal Dates keep their order)
    f = random_filter(rng, np.concatenate(parts), pool)
    return parts, f
