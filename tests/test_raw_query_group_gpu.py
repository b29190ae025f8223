"""Queries over the whole topic (include/flowagg.h "queries over the whole topic") on the GPU: the query row kinds of the exchange
steps, fa_raw_query_merge_device / _rows, and the group doors fa_group_raw_query_pending / _rows / _reset.  All members sit on one
GPU.  Every expected row comes from a SINGLE ctx that holds every record (fa_raw_query_pending + fa_raw_query_rows) and from the
numpy restatement of raw_query_cases over all records - byte for byte, never from the doors under test."""
import ctypes as C

import numpy as np
import pytest

import raw_query_cases as Q
import raw_query_group_cases as GC
import raw_select_cases as S
from raw_query_cases import G, G_ALL, O_KEY, O_WEIGHT
from test_raw_pending_gpu import _build, _pending, _result

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -6, -8
SENTINEL = 0x5A5A5A5A
ADDR = G["SRC_ADDR"] | G["DST_ADDR"]


def _member(fa, rows, enable=True):
    a = fa.FlowAgg(framed=True)
    if enable:
        a.raw_enable(0)
        if len(rows):
            _build(fa, a, rows)
    return a


class _Topic:
    """n members holding `shares`, and the twin: one ctx that ingested every record"""

    def __init__(self, fa, shares):
        self.fa, self.shares = fa, shares
        self.members = [_member(fa, r) for r in shares]
        self.twin = _member(fa, np.concatenate(shares) if len(shares) else np.zeros(0, dtype=S.ROWS))
        self.group = fa.FlowGroup(self.members)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.group.close()
        for m in self.members + [self.twin]:
            m.close()

    def query(self, groups, **f):
        self.group.raw_query_pending(groups, **f)
        self.twin.raw_query_pending(groups, **f)
        return Q.matching([np.concatenate(self.shares)], f)

    def check(self, want_rows, groups, ks=(0, 1, 3, 1 << 20)):
        """every kind, both orders, every k: the group's rows == the twin's == the restatement's"""
        for name, bit in G.items():
            if not groups & bit:
                continue
            by_key = Q.groups_of(want_rows, bit)
            for order in (O_WEIGHT, O_KEY):
                want = Q.ordered(by_key, order)
                for k in ks:
                    got = self.group.raw_query_rows(bit, k, order).tobytes()
                    cut = want[:k] if k else want
                    assert got == cut.tobytes(), (name, order, k, len(got) // 40, len(cut))
                    assert got == self.twin.raw_query_rows(bit, k, order).tobytes(), (name, order, k)


def _err(fa, agg):
    return (fa.lib().fa_last_error(agg._h) or b"").decode()


def _gerr(fa, g):
    return (fa.lib().fa_group_last_error(g._h) or b"").decode()


def _dev(rows):
    """host rows -> (a torch tensor that owns them in HBM, its pointer)"""
    import torch
    t = torch.zeros(max(rows.nbytes, 8), dtype=torch.uint8, device="cuda")
    if rows.nbytes:
        t[:rows.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).reshape(-1).copy()))
    torch.cuda.synchronize()
    return t, t.data_ptr()


# ---- 1: seeded differential ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_seeded_differential(gpu_lib, fa, n):
    rows, f = GC.seeded_stream(n)
    with _Topic(fa, GC.deal(rows, n)) as t:
        want = t.query(G_ALL, **f)
        assert len(want) > 100 and len(Q.groups_of(want, G["SRC_ADDR"])) > 3
        own = [_result(m, G_ALL) for m in t.members]
        t.check(want, G_ALL)
        assert [_result(m, G_ALL) for m in t.members] == own  # the members' results did not move


# ---- 2: the exact k -----------------------------------------------------------------------------------------------------------------
def test_exact_k(gpu_lib, fa):
    members = GC.exact_k_members()
    assert GC.exact_k_precondition(members) == 30  # (before the library is called)
    with _Topic(fa, members) as t:
        want = t.query(G["SRC_ADDR"] | G["SRC_PORT"])
        t.check(want, G["SRC_ADDR"] | G["SRC_PORT"], ks=(0, 1, GC.EXACT_K, 4, 5, 6, 100))
        first = t.group.raw_query_rows(G["SRC_ADDR"], 1)[0]
        assert bytes(first["key"][:4]) == bytes([10, 0, 0, 1]) and int(first["weight"]) == 30 and int(first["count"]) == 3
        for m in t.members:  # ... which no member's own first k holds
            assert all(int(r["weight"]) != 10 for r in m.raw_query_rows(G["SRC_ADDR"], GC.EXACT_K))


# ---- 3: edges -----------------------------------------------------------------------------------------------------------------------
def test_empty_members(gpu_lib, fa):
    rows, f = GC.seeded_stream(77, 300)
    empty = np.zeros(0, dtype=S.ROWS)
    with _Topic(fa, [rows[0::2], empty, rows[1::2]]) as t:  # one member without pending rows
        t.check(t.query(G_ALL, **f), G_ALL, ks=(0, 2))
    with _Topic(fa, [empty, empty, empty]) as t:  # all of them: zero rows, and nothing is fetched
        t.query(G_ALL)
        for bit in G.values():
            for order in (O_WEIGHT, O_KEY):
                assert len(t.group.raw_query_rows(bit, 0, order)) == 0 and len(t.group.raw_query_rows(bit, 5, order)) == 0
        n_out = C.c_size_t(SENTINEL)
        assert fa.lib().fa_group_raw_query_rows(t.group._h, 1, 0, 0, None, 0, C.byref(n_out)) == 0 and n_out.value == 0


def test_scalar_edges_wrap_and_capacity(gpu_lib, fa):
    members = GC.scalar_edge_members()
    groups = G["SRC_ADDR"] | G["SRC_PORT"] | G["TOTAL"]
    with _Topic(fa, members) as t:
        want = t.query(groups)
        t.check(want, groups, ks=(0, 1, 2, 3))
        ports = t.group.raw_query_rows(G["SRC_PORT"], 0, O_KEY)
        assert [int(v) for v in ports["value"]] == [255, 256, 65535, 65536]  # numeric order, not the order of little-endian bytes
        a = t.group.raw_query_rows(G["SRC_ADDR"], 0, O_KEY)
        wrapped = a[(a["key"][:, 3] == 1) & (a["etype"] == 0x800)]
        assert len(wrapped) == 1 and int(wrapped[0]["weight"]) == 18 and int(wrapped[0]["count"]) == 4  # 2 x 2^63 + 18 mod 2^64
        # cap too small: the rows needed, nothing written; the second call with that cap succeeds
        L = fa.lib()
        out, n_out = np.zeros(4, dtype=fa.QUERY_ROW_DTYPE), C.c_size_t(SENTINEL)
        out.view(np.uint8)[:] = 0xEE
        assert L.fa_group_raw_query_rows(t.group._h, G["SRC_PORT"], O_KEY, 0, out.ctypes.data, 1, C.byref(n_out)) == ERR_CAPACITY
        assert n_out.value == 4 and (out.view(np.uint8) == 0xEE).all()
        assert L.fa_group_raw_query_rows(t.group._h, G["SRC_PORT"], O_KEY, 0, out.ctypes.data, 4, C.byref(n_out)) == 0
        assert n_out.value == 4 and out.tobytes() == ports.tobytes()


# ---- 4: state -----------------------------------------------------------------------------------------------------------------------
def test_state_repeat_keep_and_reset(gpu_lib, fa):
    rows, f = GC.seeded_stream(5, 900)
    stored, f2 = GC.seeded_stream(6, 600)
    groups = ADDR | G["DST_PORT"] | G["MINUTE"]
    shares, files = GC.deal(rows, 3), GC.deal(stored, 3)
    with _Topic(fa, shares) as t:
        want = t.query(groups, **f)
        first = {(bit, o): t.group.raw_query_rows(bit, 3, o).tobytes() for bit in (1, 2, 8, 16) for o in (O_WEIGHT, O_KEY)}
        again = {(bit, o): t.group.raw_query_rows(bit, 3, o).tobytes() for bit in (1, 2, 8, 16) for o in (O_WEIGHT, O_KEY)}
        assert first == again  # a repeated group read is identical
        # stored files member by member, then the pending rows with KEEP: one answer over stored and live rows
        blobs = []
        for m, r in zip(t.members, files):
            day1 = r["time_received"] >= S.MID + 86400
            with _pending(fa, [r[~day1], r[day1]]) as src:
                data, _ = src.raw_take()
                blobs.append(bytes(data))
            m.raw_query(blobs[-1], groups, **f)
        t.group.raw_query_pending(groups, keep=True, **f)
        t.twin.raw_query_reset()
        for i, b in enumerate(blobs):
            t.twin.raw_query(b, groups, keep=i > 0, **f)
        t.twin.raw_query_pending(groups, keep=True, **f)
        both = np.concatenate([want, Q.matching([stored], f)])
        t.check(both, groups, ks=(0, 3))
        # reset: no member holds a result
        t.group.raw_query_reset()
        for m in t.members:
            with pytest.raises(fa.FlowAggError) as e:
                m.raw_query_rows(1)
            assert e.value.code == ERR_ARG
        with pytest.raises(fa.FlowAggError) as e:
            t.group.raw_query_rows(1)
        assert e.value.code == ERR_ARG and "member 0" in str(e.value) and "holds no query result" in str(e.value)


# ---- 5: fa_raw_query_merge_device / _rows ------------------------------------------------------------------------------------------------
def test_merge_into_a_held_result(gpu_lib, fa):
    rows, f = GC.seeded_stream(11, 1200)
    ra, rb = GC.deal(rows, 2)
    with _member(fa, ra) as a, _member(fa, rb) as b:
        a.raw_query_pending(G_ALL, **f)
        b.raw_query_pending(G_ALL, **f)
        launches0 = b.raw_query_stats()["launches"]
        for j, bit in enumerate(G.values()):
            if j & 1:  # the rows where they lie in A's HBM
                ptr, n = a.raw_query_rows_device(bit, 0, O_KEY)
                b.raw_query_merge(bit, ptr, n)
            else:  # host rows, in the other order
                b.raw_query_merge(bit, a.raw_query_rows(bit, 0, O_WEIGHT))
        Q.check_reads(b, Q.matching([rows], f), G_ALL)
        ms = b.raw_query_merge_stats()
        assert ms["merge_calls"] == 9 and ms["rows_merged"] == sum(len(a.raw_query_rows(bit)) for bit in G.values())
        assert b.raw_query_stats()["launches"] >= launches0 + 18 and a.raw_query_merge_stats() == dict(merge_calls=0, rows_merged=0)
        # ... and a pending query with KEEP still adds
        b.raw_query_pending(G_ALL, keep=True, **f)
        Q.check_reads(b, Q.matching([np.concatenate([ra, rb, rb])], f), G_ALL)


def test_merge_more_rows_than_a_launch(gpu_lib, fa):
    n = (1 << 20) + 1  # the smallest count that needs a second launch
    rows = np.zeros(n, dtype=fa.QUERY_ROW_DTYPE)
    rows["value"], rows["weight"], rows["count"] = np.arange(n), np.arange(n) + 7, 1
    with _member(fa, np.zeros(0, dtype=S.ROWS)) as c:
        c.raw_query_pending(G["SRC_PORT"])
        st0 = c.raw_query_stats()
        c.raw_query_merge(G["SRC_PORT"], rows[::-1].copy())
        st1 = c.raw_query_stats()
        assert st1["groups"] == n and st1["launches"] - st0["launches"] >= 3  # the check, two adds (and the rehashes)
        assert c.raw_query_rows(G["SRC_PORT"], 0, O_KEY).tobytes() == rows.tobytes()
        assert c.raw_query_merge_stats() == dict(merge_calls=1, rows_merged=n)


def _row(key=bytes(16), etype=0, value=0, weight=1, count=1):
    r = np.zeros(1, dtype=np.dtype(Q.ROW))
    r["key"][0] = np.frombuffer(bytes(key), dtype=np.uint8)
    r["etype"], r["value"], r["weight"], r["count"] = etype, value, weight, count
    return r


def test_merge_refusals_change_nothing(gpu_lib, fa):
    rows, f = GC.seeded_stream(12, 400)
    groups = G["SRC_ADDR"] | G["SRC_PORT"] | G["MINUTE"] | G["TOTAL"]
    v4 = bytes([10, 1, 2, 3]) + bytes(12)
    good = {1: _row(v4, 0x800), 4: _row(value=70000), 16: _row(value=600), 256: _row()}
    bad = [(1, _row(bytes([10, 1, 2, 3, 0, 9]) + bytes(10), 0x800)), (1, _row(v4, 0x86DD)), (1, _row(v4, 0x800, value=1)), (1, _row(v4, 0, value=4)),
           (4, _row(v4, 0, value=80)), (4, _row(etype=0x800, value=80)), (16, _row(value=601)), (16, _row(key=bytes(15) + b"\1", value=600)), (256, _row(value=1)),
           (256, _row(etype=0x800))]
    with _member(fa, rows) as a, _member(fa, rows) as none:
        with pytest.raises(fa.FlowAggError) as e:  # no result held
            none.raw_query_merge(1, good[1])
        assert e.value.code == ERR_ARG and "no query result" in str(e.value)
        a.raw_query_pending(groups, **f)
        held = _result(a, groups)
        st0 = a.raw_query_merge_stats()
        for bit, r in bad:
            many = np.concatenate([np.repeat(good[bit], 70), r])  # (the bad row last: every row is looked at before the first is added)
            for form in ("host", "device"):
                with pytest.raises(fa.FlowAggError) as e:
                    if form == "host":
                        a.raw_query_merge(bit, many)
                    else:
                        keep, ptr = _dev(many)
                        a.raw_query_merge(bit, ptr, len(many))
                assert e.value.code == ERR_ARG and "nothing was added" in str(e.value), (bit, r)
                assert _result(a, groups) == held
        for group in (0, 3, 2, 512, 8):  # no bit, two bits, a bit the result lacks, an unknown bit
            with pytest.raises(fa.FlowAggError) as e:
                a.raw_query_merge(group, good[1])
            assert e.value.code == ERR_ARG and "exactly one bit" in str(e.value)
        assert fa.lib().fa_raw_query_merge_rows(a._h, 1, None, 3) == ERR_ARG and fa.lib().fa_raw_query_merge_device(a._h, 1, None, 3) == ERR_ARG
        assert _result(a, groups) == held and a.raw_query_merge_stats() == st0
        for bit, r in good.items():  # the good rows themselves are taken
            a.raw_query_merge(bit, r)
        assert a.raw_query_merge_stats()["rows_merged"] == st0["rows_merged"] + 4 and _result(a, groups) != held


# ---- 6: the row kinds, directly ------------------------------------------------------------------------------------------------------
def test_row_kinds_merge_partition_and_refusals(gpu_lib, fa):
    dist = fa.dist
    rows, f = GC.seeded_stream(13, 1500)
    ra, rb = GC.deal(rows, 2)
    want = Q.matching([rows], f)
    L = fa.lib()
    assert L.fa_row_bytes(fa.ROWS_QUERY_WEIGHT) == L.fa_row_bytes(fa.ROWS_QUERY_KEY) == 40
    with _member(fa, ra) as a, _member(fa, rb) as b, fa.FlowAgg(framed=True) as plain:  # plain: nothing enabled, never queried
        a.raw_query_pending(G_ALL, **f)
        b.raw_query_pending(G_ALL, **f)
        for bit in (G["SRC_ADDR"], G["DST_ADDR"], G["SRC_PORT"], G["MINUTE"], G["TOTAL"]):
            both = np.concatenate([a.raw_query_rows(bit, 0, O_WEIGHT), b.raw_query_rows(bit, 0, O_KEY)])
            keep, ptr = _dev(both)
            by_key = Q.groups_of(want, bit)
            for kind, order in ((fa.ROWS_QUERY_WEIGHT, O_WEIGHT), (fa.ROWS_QUERY_KEY, O_KEY)):
                for k in (0, 1, 3):
                    mptr, m = plain.rows_merge_device(kind, ptr, len(both), k)
                    exp = Q.ordered(by_key, order)
                    exp = exp[:k] if k else exp
                    assert plain.rows_fetch(kind, mptr, m).tobytes() == exp.tobytes(), (bit, order, k)
                assert dist.merge_query_host([both[:5], both[5:]], order).tobytes() == Q.ordered(by_key, order).tobytes()
            # the partition: the counts add up, a key lies in one share only, and the host stand-in names the same owner
            for world in (1, 3, 8):
                pptr, counts = plain.rows_partition_device(fa.ROWS_QUERY_KEY, ptr, len(both), world)
                assert sum(counts) == len(both) and len(counts) == world
                got = plain.rows_fetch(fa.ROWS_QUERY_KEY, pptr, len(both))
                owner = np.repeat(np.arange(world), counts)
                assert (dist.partition_rows_host(got, fa.ROWS_QUERY_KEY, world) == owner).all()
                ident = [(r["value"], r["key"].tobytes(), r["etype"]) for r in got]
                seen = {}
                for i, o in zip(ident, owner):
                    assert seen.setdefault(i, o) == o
                assert sorted(got.tobytes()[i:i + 40] for i in range(0, 40 * len(got), 40)) == sorted(both.tobytes()[i:i + 40] for i in range(0, 40 * len(both), 40))
        # a row no query produces: FA_ERR_ARG, nothing merged, the outputs untouched
        v4 = bytes([10, 1, 2, 3]) + bytes(12)
        for r in (_row(v4, 0x86DD), _row(v4, 1), _row(bytes([10, 1, 2, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]), 0x800), _row(v4, 0x800, value=5), _row(v4, 0, value=5),
                  _row(etype=0x800, value=5)):
            keep, ptr = _dev(np.concatenate([np.repeat(_row(v4, 0x800), 70), r]))
            for kind in (fa.ROWS_QUERY_WEIGHT, fa.ROWS_QUERY_KEY):
                p, n_out = C.c_void_p(SENTINEL), C.c_size_t(SENTINEL)
                assert L.fa_rows_merge_device(plain._h, kind, ptr, 71, 0, C.byref(p), C.byref(n_out)) == ERR_ARG
                assert (p.value, n_out.value) == (SENTINEL, SENTINEL) and "no query produces" in _err(fa, plain)
        # fa_rows_device has no place for the group bit
        for kind in (fa.ROWS_QUERY_WEIGHT, fa.ROWS_QUERY_KEY):
            with pytest.raises(fa.FlowAggError) as e:
                a.rows_device(kind)
            assert e.value.code == ERR_UNSUPPORTED and "fa_raw_query_rows_device" in str(e.value)


# ---- 7: refusals of the group calls ------------------------------------------------------------------------------------------------------
def test_group_refusals(gpu_lib, fa):
    rows, f = GC.seeded_stream(14, 300)
    L = fa.lib()
    with _member(fa, rows[0::2]) as a, _member(fa, rows[1::2]) as b, _member(fa, rows, enable=False) as off:
        with fa.FlowGroup([a, off, b]) as g:  # a member without fa_raw_enable: before any member runs
            a.raw_query_pending(G["TOTAL"])
            held = _result(a, G["TOTAL"])
            with pytest.raises(fa.FlowAggError) as e:
                g.raw_query_pending(G_ALL, **f)
            assert e.value.code == ERR_UNSUPPORTED and "member 1" in str(e.value) and "fa_raw_enable" in str(e.value)
            assert all("member 1" in _err(fa, m) for m in (a, off, b))
            assert _result(a, G["TOTAL"]) == held and a.raw_query_stats()["calls"] == 1 and b.raw_query_stats()["calls"] == 0
        with fa.FlowGroup([a, b]) as g:
            out, n_out = np.zeros(8, dtype=fa.QUERY_ROW_DTYPE), C.c_size_t(SENTINEL)
            # a member without a result
            b.raw_query_reset()
            with pytest.raises(fa.FlowAggError) as e:
                g.raw_query_rows(G["TOTAL"])
            assert e.value.code == ERR_ARG and "member 1" in str(e.value) and "holds no query result" in str(e.value)
            assert all("member 1" in _err(fa, m) for m in (a, b)) and _result(a, G["TOTAL"]) == held
            # a member whose result lacks the bit
            b.raw_query_pending(G["SRC_PORT"])
            held_b = _result(b, G["SRC_PORT"])
            launches = [m.raw_query_stats()["launches"] for m in (a, b)]
            for bit, who in ((G["TOTAL"], "member 1"), (G["SRC_PORT"], "member 0")):
                with pytest.raises(fa.FlowAggError) as e:
                    g.raw_query_rows(bit)
                assert e.value.code == ERR_ARG and who in str(e.value) and "not among the groups" in str(e.value)
            # a bad group bit or order, null arguments
            g.raw_query_pending(G["TOTAL"] | G["SRC_PORT"])
            held, held_b = _result(a, G["TOTAL"] | G["SRC_PORT"]), _result(b, G["TOTAL"] | G["SRC_PORT"])
            launches = [m.raw_query_stats()["launches"] for m in (a, b)]
            for bit in (0, 12, 512, 1 << 31):
                assert L.fa_group_raw_query_rows(g._h, bit, 0, 0, out.ctypes.data, 8, C.byref(n_out)) == ERR_ARG and "exactly one" in _gerr(fa, g)
            for order in (-1, 2):
                assert L.fa_group_raw_query_rows(g._h, 4, order, 0, out.ctypes.data, 8, C.byref(n_out)) == ERR_ARG and "order" in _gerr(fa, g)
            assert L.fa_group_raw_query_rows(g._h, 4, 0, 0, None, 8, C.byref(n_out)) == ERR_ARG
            assert L.fa_group_raw_query_rows(g._h, 4, 0, 0, out.ctypes.data, 8, None) == ERR_ARG
            assert L.fa_group_raw_query_rows(None, 4, 0, 0, out.ctypes.data, 8, C.byref(n_out)) == ERR_ARG
            assert L.fa_group_raw_query_pending(g._h, None) == ERR_ARG and L.fa_group_raw_query_pending(None, None) == ERR_ARG
            assert L.fa_group_raw_query_reset(None) == ERR_ARG
            assert [m.raw_query_stats()["launches"] for m in (a, b)] == launches  # no member's state moved: nothing was launched
            assert _result(a, G["TOTAL"] | G["SRC_PORT"]) == held and _result(b, G["TOTAL"] | G["SRC_PORT"]) == held_b
            # a bad query is the members' refusal, named
            with pytest.raises(fa.FlowAggError) as e:
                g.raw_query_pending(0)
            assert e.value.code == ERR_ARG and "member" in str(e.value) and "groups is 0" in str(e.value)
