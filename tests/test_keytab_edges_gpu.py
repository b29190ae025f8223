"""The capacity rule of the keyed tables (csrc/table_room.h, keytab_host.inc) pinned exactly at the smallest table, 2^8 slots,
for the three states the core serves: plain talkers, bucketed talkers (60 s) and the bucketed port tables.  Hand-made device
columns go through fa_talkers_fold_columns_device / fa_ports_fold_columns_device; the keys of a direction are distinct
throughout, so `used` is the number of records folded so far.

    128 keys: half of 256 - no growth;  129 keys in a fresh ctx: both tables double;  127 more: exactly half of 512, no growth;
    1 more: both double again;  then 1000 records on one key (the LDS cache absorbs them) and a weight-0 record on a new key.

The bound the host keeps counts RECORDS (a chunk of m records adds at most m keys), so the last step asks for room for 1001 keys
beside the 257 held: (257 + 1001) * 2 = 2516 slots, two doublings of 1024 per table.

Expected rows are never taken from the code under test: a Python dict groups everything folded so far, and the rows are
compared bit for bit in emit order (talkers: weight DESC, key bytes, etype; ports: weight DESC, port).  The port tables have no
un-ranged read of their own (fa_top_ports reads the dense histograms): their read is the ranged one over all buckets."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T0 = 1_700_000_040  # on the 60 s grid
BS = 60
NO_UPPER = 0xFFFFFFFF
M64 = (1 << 64) - 1
STATES = ("talkers", "talker_buckets", "port_buckets")


def record(j, weight=None):
    """Record j: keys no other record has, in either direction and for either kind of table; times over three buckets.
    Many records share a weight, and records 4i / 4i + 2 carry the same four address bytes under the two families."""
    v4 = j % 4 == 0
    if v4:  # bytes 4..15 are not part of the key under 0x800
        src = struct.pack("<I", j + 1) + bytes([0xEE] * 12)
        dst = struct.pack("<I", 0x80000000 | j) + bytes([j & 0xFF] * 12)
    elif j % 4 == 2:  # the same 16 canonical bytes as record j - 2, family 0
        src = struct.pack("<I", j - 1) + bytes(12)
        dst = struct.pack("<I", 0x80000000 | (j - 2)) + bytes(12)
    else:
        src = struct.pack("<QQ", 0x0120 | (j << 20), 0xFFFFFFFFFFFFFFFF - j)
        dst = struct.pack("<QQ", (1 << 63) | j, j)
    b, rate = ((j // 4 % 5) + 1, 1000) if weight is None else (weight, 1)  # (records 4i .. 4i + 3 tie)
    return dict(src_addr=src, dst_addr=dst, etype=0x800 if v4 else (0x86DD, 0, 0x1234)[j % 3], bytes=b, sampling_rate=rate,
                time_flow_start=T0 + BS * (j % 3) + (j % BS) + (1 << 32) * (j % 2),  # (only the low 32 bits are the time)
                src_port=j if j % 4 else 65536 + 7 * j, dst_port=0xFFFFFFFF - j if j % 3 == 0 else 2 * j + 1)


class Model:
    """GROUP BY of everything folded so far: {direction: {(bucket start, key): [weight, count]}}."""

    def __init__(self, state):
        self.state, self.groups, self.records = state, ({}, {}), 0

    def key(self, r, d):
        if self.state == "port_buckets":
            return r["dst_port" if d else "src_port"]
        a = r["dst_addr" if d else "src_addr"]
        return (a[:4] + bytes(12), 0x800) if r["etype"] == 0x800 else (a, 0)

    def fold(self, recs):
        for r in recs:
            t32 = r["time_flow_start"] & 0xFFFFFFFF
            bucket = 0 if self.state == "talkers" else t32 - t32 % BS
            for d in (0, 1):
                g = self.groups[d].setdefault((bucket, self.key(r, d)), [0, 0])
                g[0] = (g[0] + r["bytes"] * r["sampling_rate"]) & M64
                g[1] += 1
        self.records += len(recs)

    def drop_before(self, t):
        for d in (0, 1):
            for k in [k for k in self.groups[d] if k[0] < t]:
                del self.groups[d][k]

    def used(self):
        return [len(self.groups[d]) for d in (0, 1)]

    def buckets(self):
        return sorted({k[0] for d in (0, 1) for k in self.groups[d]})

    def rows(self, fa, d):
        """the read over every bucket held, in emit order"""
        tot = {}
        for (_, key), (w, c) in self.groups[d].items():
            g = tot.setdefault(key, [0, 0])
            g[0], g[1] = (g[0] + w) & M64, g[1] + c
        if self.state == "port_buckets":
            out = np.zeros(len(tot), dtype=fa.PORT_ROW_DTYPE)
            for i, (port, (w, c)) in enumerate(sorted(tot.items(), key=lambda kv: (-kv[1][0], kv[0]))):
                out[i] = (port, 0, w, c)
            return out
        out = np.zeros(len(tot), dtype=fa.TALKER_ROW_DTYPE)
        for i, ((key, fam), (w, c)) in enumerate(sorted(tot.items(), key=lambda kv: (-kv[1][0], kv[0][0], kv[0][1]))):
            out[i] = (np.frombuffer(key, dtype=np.uint8), fam, 0, w, c)
        return out


class Ctx:
    """One ctx of `state` at 2^8 slots and its model."""

    def __init__(self, fa, state):
        self.fa, self.state, self.model = fa, state, Model(state)
        self.agg = fa.FlowAgg(framed=True)
        if state == "port_buckets":
            self.agg.ports_enable_buckets(8, BS)
        else:
            self.agg.talkers_enable(8, BS if state == "talker_buckets" else 0)

    def close(self):
        self.agg.close()

    def fold(self, recs):
        import torch
        from device_columns import COLUMNS
        names = ("src_port", "dst_port") if self.state == "port_buckets" else ("src_addr", "dst_addr", "etype")
        keep, cols = [], self.fa.Columns()
        for name, dt, w in COLUMNS:
            if name not in names + ("bytes", "sampling_rate", "status", "time_flow_start"):
                continue
            if w > 1:
                a = np.frombuffer(b"".join(r[name] for r in recs), dtype=np.uint8)
            else:
                a = np.array([0 if name == "status" else r[name] for r in recs], dtype=dt)
            t = torch.from_numpy(a.view(np.uint8).copy()).cuda()
            keep.append(t)
            setattr(cols, name, t.data_ptr())
        try:
            (self.agg.ports_fold_columns_device if self.state == "port_buckets" else self.agg.fold_columns_device)(cols, len(recs))
        finally:
            self.agg.sync()  # (the tensors may go once the stream has read them)
        self.model.fold(recs)

    def stats(self):
        return self.agg.ports_stats() if self.state == "port_buckets" else self.agg.talkers_stats()

    def reads(self, d, k=0):
        """every read of the tables over all they hold"""
        if self.state == "port_buckets":
            return [self.agg.top_ports_range(d, k, 0, NO_UPPER)]
        out = [self.agg.top_talkers(d, k)]
        if self.state == "talker_buckets":
            out.append(self.agg.top_talkers(d, k, 0, NO_UPPER))
        return out

    def check(self, grows, capacity):
        st = self.stats()
        assert (st["grows"], st["capacity"]) == (grows, [capacity] * 2), st
        assert st["used"] == self.model.used() and st["records_folded"] == self.model.records, st
        for d in (0, 1):
            want = self.model.rows(self.fa, d)
            for got in self.reads(d):
                assert got.tobytes() == want.tobytes(), (self.state, d, len(got), len(want))
        return st


@pytest.mark.parametrize("state", STATES)
def test_capacity_rule_at_the_smallest_table(gpu_lib, fa, state):
    first = Ctx(fa, state)
    try:
        first.fold([record(j) for j in range(128)])
        assert first.check(0, 256)["used"] == [128, 128]  # exactly half: no growth
    finally:
        first.close()
    x = Ctx(fa, state)
    try:
        x.fold([record(j) for j in range(129)])
        assert x.check(2, 512)["used"] == [129, 129]  # one key over half of 256: both tables doubled
        x.fold([record(j) for j in range(129, 256)])
        assert x.check(2, 512)["used"] == [256, 256]  # exactly half of 512
        x.fold([record(256)])
        assert x.check(4, 1024)["used"] == [257, 257]
        x.fold([record(5, weight=3)] * 1000 + [record(257, weight=0)])
        st = x.check(8, 4096)  # (the bound counts records: room for 257 + 1001 keys)
        assert st["used"] == [258, 258] and st["records_absorbed"] > 0
        for d in (0, 1):  # the weight-0 key is a row (the last one: every other weight is positive)
            for got in x.reads(d):
                assert got[-1]["weight"] == 0 and got[-1]["count"] == 1
        if state == "talkers":  # fa_top_talkers(k) over a plain table: the first k of the same order, ties included
            for d in (0, 1):
                want = x.model.rows(fa, d)
                w = want["weight"]
                assert np.any((w[1:] == w[:-1]) & (want["key"][1:] == want["key"][:-1]).all(axis=1))  # tied down to the etype
                for k in (0, 1, 258, 259):
                    assert x.agg.top_talkers(d, k).tobytes() == (want[:k] if k else want).tobytes(), (d, k)
        else:  # retention: the second of the three buckets becomes the first
            buckets = x.agg.ports_buckets() if state == "port_buckets" else x.agg.talkers_buckets()
            assert list(buckets) == x.model.buckets() == [T0, T0 + BS, T0 + 2 * BS]
            (x.agg.ports_drop_before if state == "port_buckets" else x.agg.talkers_drop_before)(T0 + BS)
            x.model.drop_before(T0 + BS)
            buckets = x.agg.ports_buckets() if state == "port_buckets" else x.agg.talkers_buckets()
            assert list(buckets) == [T0 + BS, T0 + 2 * BS]
            st = x.check(8, 4096)  # used is counted again
            assert 0 < st["used"][0] < 258 and 0 < st["used"][1] < 258
        (x.agg.ports_reset if state == "port_buckets" else x.agg.talkers_reset)()
        folded = x.model.records
        x.model = Model(state)
        x.model.records = folded  # (the statistics go on counting)
        assert x.check(8, 4096)["used"] == [0, 0]
    finally:
        x.close()
