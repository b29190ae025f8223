"""Record lengths at the byte limits of both tile kernels, and broken offsets inside tiles that are staged in pieces.

Both ingest kernels stage records into fixed LDS buffers; what happens to a record or a tile that does not fit is decided by
byte arithmetic on the caller's offsets (ingest.cuh: `staged` / `rest` / `hopeless` in wtile_kernel, tile_fits and the
multi-pass loop in tile_kernel).  The streams here put records on both sides of every such limit, at every start alignment,
inside tiles of every size the host picks (64 / a few / one record per wave tile, 256 / a few / one per workgroup tile), and
then break offsets inside tiles that take several parts.  The reference is always the CPU oracle on the same bytes, bit for
bit.

A record of an exact length = [unknown LEN field 1000: filler] + a generator record + a second Bytes field (field 9, two
varint bytes), framed.  The filler goes IN FRONT (as the big record of test_large_records_beyond_lds_tile) and the record's
last byte is the top of a value every key set sums: a comparison moved by one byte that lets a record through whose last
byte was never staged changes a sum, not just a field nobody reads.  A short record with 0-15 filler bytes in an unknown
field of its own (1001) sets the start alignment of the record behind it.
"""
import math
import os
import re

import numpy as np
import pytest

from device_columns import fetch_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the geometry, mirrored from flow-pipeline_amd/csrc/sinks.cuh (wt_stride(), TILE_BYTES).  It centres the sweeps and
# gives the records_slow lower bounds; test_geometry_and_streams_cpu pins it to the source.  No equality assertion on a
# result depends on it.
WT_STRIDE = {1: 4864, 9: 4736, 7: 5056, 63: 4896}  # key_sets -> bytes of a wave's tile buffer (lean, lean + APP, sketch, KS_ALL)
TILE_BYTES = 21760                                 # the workgroup-tile kernel's buffer
KEYSETS = (1, 9, 7, 63)
CAP_MIN = min(WT_STRIDE.values()) - 16
STRIDE_MAX = max(WT_STRIDE.values())

COLS = ("time_received", "time_flow_start", "sampling_rate", "bytes", "packets", "sequence_num", "src_as", "dst_as", "etype",
        "proto", "src_port", "dst_port", "sampler_address", "src_addr", "dst_addr")
APP_COLS = ("date", "timeslot", "src_addr", "dst_port", "proto", "bytes", "packets", "count")
CMS = dict(cms_depth=4, cms_width_log2=16, cms_seed=0xFEED)


def _kind(ks):
    return "aspairs" if ks == 1 else "zipf"


# ---- what the host computes (launch_plan.h: wtile_recs_for, tile_recs_for), restated; test_launch_plan_cpu.py compares ----
def _wt_tile_recs(nbytes, n, stride):
    avg = nbytes / n
    cap = stride - 16.0 - 15.0
    r = cap / avg
    r = (cap - 2.0 * 12.0 * math.sqrt(min(r, 64.0))) / avg
    return 64 if r >= 64.0 else 1 if r < 1.0 else int(r)


def _wg_tile_recs(nbytes, n):
    r = (TILE_BYTES - 15.0) / (nbytes / n + 0.5)
    return 256 if r >= 256.0 else 1 if r < 1.0 else int(r)


def _parts(off, r0, nrec, cap):
    """Record indices at which the parts (passes) of tile [r0, r0 + nrec) start: a part is staged from its first record's
    start rounded down to 16 and holds every record that ends within `cap` bytes of that."""
    starts, i, end = [], r0, r0 + nrec
    while i < end:
        cbase = int(off[i]) & ~15
        j = i
        while j < end and int(off[j + 1]) - cbase <= cap:
            j += 1
        starts.append(i)
        i = max(j, i + 1)  # (a record that does not fit an empty buffer leaves alone, to the generic path)
    return starts


# ---- streams ------------------------------------------------------------------------------------------------------------
_POOLS = {}


def _pool(po, kind, small=False):
    """Framed generator records (ASPAIRS / Zipf); small: only the IPv4 ones (below 70 bytes), to keep a stream's mean low."""
    key = (kind, small)
    if key not in _POOLS:
        n = 120_000 if small else 60_000
        gp = po.gen_params(mode=po.GEN_ASPAIRS if kind == "aspairs" else po.GEN_ZIPF, framed=1, seed=61, n_total=n, span_secs=600)
        buf, off = po.gen_records(gp, 0, n)
        lens = np.diff(off).astype(np.int64)
        assert lens.max() <= 109  # (one-byte frame prefix, also with the alignment filler)
        if small:
            keep = np.nonzero(lens < 70)[0]
            l2 = lens[keep]
            o2 = np.zeros(len(keep) + 1, dtype=np.int64)
            o2[1:] = np.cumsum(l2)
            src = np.repeat(off[keep].astype(np.int64) - o2[:-1], l2) + np.arange(o2[-1])
            buf, off = buf[src], o2.astype(np.uint64)
        _POOLS[key] = (np.ascontiguousarray(buf), off.astype(np.int64))
    return _POOLS[key]


class _Builder:
    def __init__(self, fa, pool):
        self.fa, (self.pbuf, self.poff) = fa, pool
        self.pn = len(self.poff) - 1
        self.chunks, self.lens, self.pos, self.n, self.cur = [], [], 0, 0, 0
        self.tag1000 = fa.schema.encode_varint((1000 << 3) | 2)
        self.tag1001 = fa.schema.encode_varint((1001 << 3) | 2)

    def _body(self):  # the next generator record, unframed
        i = self.cur
        self.cur = (self.cur + 1) % self.pn
        return self.pbuf[self.poff[i] + 1:self.poff[i + 1]].tobytes()

    def shorts(self, k):  # k generator records as they are
        while k > 0:
            m = min(k, self.pn - self.cur)
            a, b = self.poff[self.cur], self.poff[self.cur + m]
            self.chunks.append(self.pbuf[a:b].tobytes())
            self.lens.append(np.diff(self.poff[self.cur:self.cur + m + 1]))
            self.pos += int(b - a)
            self.n += m
            self.cur = (self.cur + m) % self.pn
            k -= m

    def raw(self, rec):
        self.chunks.append(rec)
        self.lens.append(np.array([len(rec)], dtype=np.int64))
        self.pos += len(rec)
        self.n += 1
        return self.n - 1

    def aligner(self, a):  # a short record behind which the stream stands at `a` mod 16
        g = self._body()
        k = (a - (self.pos + 1 + len(g) + 3)) % 16
        return self.raw(self.fa.schema.frame(g + self.tag1001 + bytes([k]) + b"\xcd" * k))

    def exact(self, length):  # a framed record of exactly `length` bytes (see the module docstring)
        ev = self.fa.schema.encode_varint
        g = self._body()
        tail = b"\x48" + ev(128 + (self.n * 37) % 16000)
        for fl in (1, 2, 3):
            body_len = length - fl
            if body_len < 0 or len(ev(body_len)) != fl:
                continue
            for extra in (b"", self.tag1001 + b"\x00", (self.tag1001 + b"\x00") * 2):
                room = body_len - len(g) - len(tail) - len(extra) - len(self.tag1000)
                for pl in (1, 2, 3):
                    p = room - pl
                    if p >= 0 and len(ev(p)) == pl:
                        rec = self.fa.schema.frame(self.tag1000 + ev(p) + b"\xab" * p + extra + g + tail)
                        assert len(rec) == length
                        return self.raw(rec)
        raise ValueError("no framed record of %d bytes" % length)

    def pad_to(self, tile, align=None):  # shorts up to the next multiple of `tile` records (the last one an aligner)
        k = (-self.n) % tile
        if align is None:
            self.shorts(k)
            return
        k = k or tile
        self.shorts(k - 1)
        self.aligner(align)

    def build(self):
        buf = np.frombuffer(bytearray(b"".join(self.chunks)), dtype=np.uint8)
        off = np.zeros(self.n + 1, dtype=np.uint64)
        off[1:] = np.cumsum(np.concatenate(self.lens))
        assert int(off[-1]) == len(buf) == self.pos
        return buf, off


def _s1(fa, po, kind):
    """Capacity sweep of the wave-tile kernel: every framed length from 40 below the smallest CAP to 40 above the largest
    stride at each of the 16 start alignments, each long record followed by 7 generator records."""
    b = _Builder(fa, _pool(po, kind))
    long_idx = []
    b.shorts(7)
    for length in range(CAP_MIN - 40, STRIDE_MAX + 40 + 1):
        for a in range(16):
            b.aligner(a)
            long_idx.append(b.exact(length))
            b.shorts(6)
    buf, off = b.build()
    return buf, off, {"long": np.array(long_idx)}


def _s2(fa, po, ks):
    """Full 64-record tiles that overflow (wave-tile kernel, tile_recs == 64): whole tiles of 100-300 byte records (2, 3 and
    4 or more parts), one record of CAP - 16 .. CAP + 1 bytes at lane 0 / 31 / 63 of a short tile, zero-length records."""
    cap = WT_STRIDE[ks] - 16
    b = _Builder(fa, _pool(po, _kind(ks), small=True))
    info = {"multi": [], "edge": [], "zero": []}
    b.shorts(64 * 4)
    for base in (100, 160, 300):
        for rep in range(5):
            assert b.n % 64 == 0
            info["multi"].append(b.n)
            for j in range(64):
                b.exact(base + (j + rep) % 7)
            b.shorts(64 * 2)
    for lane in (0, 31, 63):
        for length in range(cap - 16, cap + 2):
            if lane == 0:
                b.pad_to(64, align=0)
            else:
                b.pad_to(64)
                b.shorts(lane - 1)
                b.aligner(0)
            assert b.n % 64 == lane and b.pos % 16 == 0
            info["edge"].append(b.exact(length))
    # zero-length framed records (a bare 0x00, one byte on the wire): first of a tile; first of a rest part - behind records
    # that fill the buffer to its last byte, and behind a record that no buffer holds; right before a record that does not
    # fit what is left of the buffer
    b.pad_to(64)
    info["zero"].append(b.raw(b"\x00"))
    b.pad_to(64, align=0)
    start = b.pos
    b.shorts(20)
    b.exact(cap - (b.pos - start))
    info["zero"].append(b.raw(b"\x00"))
    b.pad_to(64)
    b.shorts(10)
    b.exact(STRIDE_MAX + 150)
    info["zero"].append(b.raw(b"\x00"))
    b.pad_to(64)
    b.shorts(40)
    info["zero"].append(b.raw(b"\x00"))
    b.exact(3000)
    b.pad_to(64)
    b.shorts(max(0, 49152 - b.n))
    buf, off = b.build()
    return buf, off, info


def _s3(fa, po, kind, which, reps=3000):
    """One record per wave tile: 'big' 5.5-6 KB (nothing fits a buffer), 'mid' about 2.5 KB (everything does), 'mix'."""
    b = _Builder(fa, _pool(po, kind))
    for i in range(reps):
        big = which == "big" or (which == "mix" and i % 2 == 0)
        b.exact(5500 + (i * 7) % 500 if big else 2400 + (i * 3) % 200)
    buf, off = b.build()
    return buf, off, {}


def _s4_sweep(fa, po, kind, alone):
    """Capacity sweep of the workgroup-tile kernel: TILE_BYTES - 40 .. + 40 at the 16 alignments; each long record behind
    40-42 short ones (met inside a multi-pass tile), or - alone - behind a single aligner (tile_recs == 1)."""
    b = _Builder(fa, _pool(po, kind))
    long_idx = []
    for length in range(TILE_BYTES - 40, TILE_BYTES + 40 + 1):
        for a in range(16):
            if not alone:
                b.shorts(39 + len(long_idx) % 3)
            b.aligner(a)
            long_idx.append(b.exact(length))
    buf, off = b.build()
    return buf, off, {"long": np.array(long_idx)}


def _s4_multi(fa, po, kind):
    """256-record tiles whose bytes need 3 or more passes (runs of 1.5 KB records inside short ones); in the first two the
    run starts the tile at a multiple of 16 and its 15th record ends exactly at / one byte behind the first pass's limit."""
    b = _Builder(fa, _pool(po, kind, small=True))
    info = {"multi": [], "at_limit": []}
    for last in (TILE_BYTES - 14 * 1500, TILE_BYTES - 14 * 1500 + 1):
        b.pad_to(256, align=0)
        info["multi"].append(b.n)
        for _ in range(14):
            b.exact(1500)
        info["at_limit"].append(b.exact(last))
        for _ in range(25):
            b.exact(1500)
    for t in range(14):
        b.pad_to(256)
        info["multi"].append(b.n)
        b.shorts(20 + 13 * t)
        for j in range(26):
            b.exact(1500 + (j + t) % 9)
    b.pad_to(256)
    while b.pos / b.n + 0.5 > 83.0:  # dilute: the mean must leave the host at 256 records per tile
        b.shorts(256)
    buf, off = b.build()
    return buf, off, info


class _Streams:
    """Streams by name, each with its references by key set.  Every small stream stays for the module; of the big ones
    (30 MB) only the one asked for last."""

    def __init__(self):
        self.kept, self.big = {}, None

    def get(self, name, make):
        if name in self.kept:
            return self.kept[name]
        if self.big is not None and self.big["name"] == name:
            return self.big
        buf, off, info = make()
        s = dict(name=name, buf=buf, off=off, info=info, ref={})
        if len(buf) < 8 << 20:
            self.kept[name] = s
        else:
            self.big = s
        return s


@pytest.fixture(scope="module")
def streams():
    return _Streams()


def _reference(po, buf, off, ks):
    rows, status = po.decode_batch(buf, off, 1)
    assert int(status.sum()) == 0
    ref = {"rows": rows, "status": status}
    r = po.Rollup(300)
    assert r.ingest(buf, off, 1) == 0
    ref["rollup"] = r.rows()
    with np.errstate(over="ignore"):
        w = rows["bytes"] * rows["sampling_rate"]
    if ks & 2:
        ref["cms_src"] = po.cms_sketch_numpy(rows["src_addr"], w, CMS["cms_depth"], CMS["cms_width_log2"], CMS["cms_seed"])
    if ks & 4:
        ref["cms_dst"] = po.cms_sketch_numpy(rows["dst_addr"], w, CMS["cms_depth"], CMS["cms_width_log2"], CMS["cms_seed"])
    if ks & 8:
        ref["app"] = po.rollup_app(rows, status, 300)
    if ks & 16:
        ref["ports"] = [po.top_ports(rows, status, d) for d in (0, 1)]
    if ks & 32:
        ref["minutes"] = po.minute_series(rows, status)
    return ref


def _ref_for(po, s, ks):
    if ks not in s["ref"]:
        s["ref"][ks] = _reference(po, s["buf"], s["off"], ks)
    return s["ref"][ks]


def _same(got, want, cols):
    assert len(got) == len(want), (len(got), len(want))
    for c in cols:
        assert np.array_equal(got[c], want[c]), (c, np.nonzero((got[c] != want[c]).reshape(len(got), -1).any(axis=1))[0][:10])


def _assert_key_sets(fa, agg, ks, ref):
    assert agg.read_window().tobytes() == ref["rollup"].tobytes()
    if ks & 2:
        assert np.array_equal(agg.cms_read(fa.FA_KEYS_SRCADDR_CMS).reshape(-1), ref["cms_src"])
    if ks & 4:
        assert np.array_equal(agg.cms_read(fa.FA_KEYS_DSTADDR_CMS).reshape(-1), ref["cms_dst"])
    if ks & 8:
        _same(agg.read_window_app(), ref["app"], APP_COLS)
    if ks & 16:
        for d in (0, 1):
            _same(agg.top_ports(d), ref["ports"][d], ("port", "weight", "count"))
    if ks & 32:
        _same(agg.minute_series(), ref["minutes"], ("minute", "weight", "count"))


def _upload(buf, off):
    import torch
    d_buf = torch.zeros(len(buf) + 64, dtype=torch.uint8, device="cuda")
    d_buf[:len(buf)] = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off).astype(np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()  # (torch's fills and copies run on its stream, the library's kernels on the ctx's)
    return d_buf, d_off


def _ingest_and_check(fa, po, s, ks, slow_at_least=0, wave_tiles=True):
    buf, off = s["buf"], s["off"]
    n = len(off) - 1
    ref = _ref_for(po, s, ks)
    d_buf, d_off = _upload(buf, off)
    with fa.FlowAgg(framed=True, key_sets=ks, max_batch_records=n, **CMS) as agg:
        agg.ingest_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), n)
        st = agg.stats()
        assert st["records_ok"] == n and st["records_bad"] == 0, (st["records_ok"], st["records_bad"], n)
        _assert_key_sets(fa, agg, ks, ref)
    assert (st["wave_tile_launches"] >= 1) == wave_tiles, st["wave_tile_launches"]
    assert st["records_slow"] >= slow_at_least, (st["records_slow"], slow_at_least)
    return st


def _assert_decoded(got, rows, status):
    assert np.array_equal(got["status"], status.astype(np.uint8)), np.nonzero(got["status"] != status)[0][:10]
    for c in COLS:
        assert np.array_equal(got[c], rows[c]), (c, np.nonzero((got[c] != rows[c]).reshape(len(rows), -1).any(axis=1))[0][:10])


def _decode_and_check(fa, po, s):
    buf, off = s["buf"], s["off"]
    n = len(off) - 1
    ref = _ref_for(po, s, 1)
    d_buf, d_off = _upload(buf, off)
    with fa.FlowAgg(framed=True, max_batch_records=n) as agg:
        cols = agg.decode_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), n)
        agg.sync()
        got = fetch_columns(cols, n)
    _assert_decoded(got, ref["rows"], ref["status"])


# ---- 0. CPU: the mirrored geometry is the source's, and every stream has the property its test relies on ----------------
def _both_sides(off, idx, limit):
    """Among the records `idx`: at every start alignment one that ends exactly at `limit` bytes from its start rounded down
    to 16, and one that ends one byte behind it."""
    a = off[idx].astype(np.int64) & 15
    span = a + (off[idx + 1] - off[idx]).astype(np.int64)
    return all(((a == k) & (span == limit)).any() and ((a == k) & (span == limit + 1)).any() for k in range(16))


def test_geometry_and_streams_cpu(fa, po):
    src = open(os.path.join(ROOT, "flow-pipeline_amd", "csrc", "sinks.cuh")).read()
    lean = int(re.search(r"#define FA_WT_STRIDE (\d+)", src).group(1))
    cms = int(re.search(r"constexpr int WT_STRIDE_CMS = (\d+);", src).group(1))
    m = re.search(r"\(wt_lean\(key_sets\) \? WT_STRIDE : WT_STRIDE_CMS\) - \(\(key_sets & FA_KEYS_ADDR_PORT_PROTO\) \? \(wt_lean\(key_sets\) \? (\d+) : (\d+)\) : 0\)", src)
    assert {1: lean, 9: lean - int(m.group(1)), 7: cms, 63: cms - int(m.group(2))} == WT_STRIDE
    assert int(re.search(r"constexpr int TILE_BYTES = (\d+);", src).group(1)) == TILE_BYTES
    assert re.search(r"constexpr int WT_RECS = 64;", src) and re.search(r"constexpr int BLOCK = 256;", src)

    def ok(buf, off):  # the oracle decodes every record
        _, status = po.decode_batch(buf, off, 1)
        return int(status.sum()) == 0

    # 1: the sweep straddles every variant's CAP at every alignment; 640 records no variant can stage
    for kind in ("aspairs", "zipf"):
        buf, off, info = _s1(fa, po, kind)
        assert ok(buf, off)
        for ks in KEYSETS:
            assert _both_sides(off, info["long"], WT_STRIDE[ks] - 16)
            assert 1 < _wt_tile_recs(len(buf), len(off) - 1, WT_STRIDE[ks]) < 64
        assert int((np.diff(off)[info["long"]] > STRIDE_MAX).sum()) == 40 * 16
    # 2: 64 records per tile, tiles of 2, 3 and 4 or more parts, CAP and CAP + 1 at lanes 0, 31 and 63
    for ks in KEYSETS:
        buf, off, info = _s2(fa, po, ks)
        n, cap = len(off) - 1, WT_STRIDE[ks] - 16
        assert ok(buf, off) and n >= 1 << 15
        assert _wt_tile_recs(len(buf), n, WT_STRIDE[ks]) == 64
        nparts = [len(_parts(off, r0, 64, cap)) for r0 in info["multi"]]
        assert 2 in nparts and 3 in nparts and max(nparts) >= 4 and min(nparts) >= 2, nparts
        e = np.array(info["edge"])
        span = ((off[e].astype(np.int64) & 15) + np.diff(off)[e].astype(np.int64)).reshape(3, 18)
        assert (e.reshape(3, 18) % 64 == np.array([[0], [31], [63]])).all()
        assert (span == np.arange(cap - 16, cap + 2)).all()
        z = info["zero"]
        assert all(off[i] + 1 == off[i + 1] and buf[int(off[i])] == 0 for i in z) and z[0] % 64 == 0
        assert off[z[1]] - off[z[1] - z[1] % 64] == cap and off[z[1] - z[1] % 64] % 16 == 0  # the buffer is full to its last byte:
        assert _parts(off, z[1] - z[1] % 64, 64, cap)[1] == z[1]                             # it starts the second part
        assert off[z[2]] - off[z[2] - 1] > STRIDE_MAX  # behind a record no buffer holds: it starts that tile's third part
        assert _parts(off, z[2] - z[2] % 64, 64, cap)[2] == z[2]
        assert z[3] + 1 in _parts(off, z[3] - z[3] % 64, 64, cap)  # the record behind it starts a part; itself it was staged
    # 3: one record per tile
    for kind in ("aspairs", "zipf"):
        for which in ("big", "mid", "mix"):
            buf, off, _ = _s3(fa, po, kind, which, reps=200)
            assert ok(buf, off)
            lens = np.diff(off).astype(np.int64)
            for ks in KEYSETS:
                assert _wt_tile_recs(len(buf), len(off) - 1, WT_STRIDE[ks]) == 1
            if which != "mid":
                assert lens.max() <= 6000 and (lens >= 5500).sum() == (200 if which == "big" else 100)
            if which != "big":
                assert lens.min() >= 2400 and (lens < 2600).sum() == (200 if which == "mid" else 100)
    # 4: TILE_BYTES at every alignment, inside multi-pass tiles and alone; 256-record tiles of 3 or more passes
    for alone in (False, True):
        buf, off, info = _s4_sweep(fa, po, "aspairs", alone)
        n = len(off) - 1
        assert ok(buf, off) and _both_sides(off, info["long"], TILE_BYTES)
        tr = _wg_tile_recs(len(buf), n)
        assert tr == 1 if alone else 30 <= tr <= 42, tr
        if not alone:
            assert n >= 1 << 15 and (np.diff(info["long"]) >= 41).all()
            assert max(len(_parts(off, r0, min(tr, n - r0), TILE_BYTES)) for r0 in range(0, n, tr)) >= 3
    for kind in ("aspairs", "zipf"):
        buf, off, info = _s4_multi(fa, po, kind)
        n = len(off) - 1
        assert ok(buf, off) and n < 1 << 15 and n % 256 == 0 and _wg_tile_recs(len(buf), n) == 256
        assert all(r0 % 256 == 0 and len(_parts(off, r0, 256, TILE_BYTES)) >= 3 for r0 in info["multi"])
        for r0, i, over in zip(info["multi"][:2], info["at_limit"], (0, 1)):
            assert off[r0] % 16 == 0 and off[i + 1] - off[r0] == TILE_BYTES + over
            assert _parts(off, r0, 256, TILE_BYTES)[1] == i + 1 - over


# ---- 1. wave-tile kernel, capacity sweep ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ks,fmt", [(1, ""), (1, "8"), (1, "16"), (9, ""), (7, ""), (63, "")])
def test_wave_tile_capacity_sweep(gpu_lib, fa, po, streams, monkeypatch, ks, fmt):
    """Every framed length around every variant's CAP at each start alignment, one ingest_device call, scatter sink."""
    monkeypatch.setenv("FA_SINK", "scatter")
    monkeypatch.setenv("FA_TUPLE", fmt) if fmt else monkeypatch.delenv("FA_TUPLE", raising=False)
    s = streams.get("s1-" + _kind(ks), lambda: _s1(fa, po, _kind(ks)))
    never = int((np.diff(s["off"])[s["info"]["long"]] > STRIDE_MAX).sum())  # longer than the largest stride: no variant stages them
    assert never == 640
    _ingest_and_check(fa, po, s, ks, slow_at_least=never)


# ---- 2. wave-tile kernel, full tiles that overflow ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ks", KEYSETS)
def test_wave_tile_full_tiles_that_overflow(gpu_lib, fa, po, streams, monkeypatch, ks):
    """tile_recs == 64 and n >= 2^15 (the sink the library chooses itself): tiles of 2, 3 and more parts, a record of
    CAP - 16 .. CAP + 1 bytes at lanes 0, 31 and 63, zero-length records at a tile's start, a part's start and in front of
    a record that does not fit."""
    monkeypatch.delenv("FA_SINK", raising=False)
    monkeypatch.delenv("FA_TUPLE", raising=False)
    s = streams.get("s2-%d" % ks, lambda: _s2(fa, po, ks))
    never = int((np.diff(s["off"]) > STRIDE_MAX).sum())
    assert never == 1
    _ingest_and_check(fa, po, s, ks, slow_at_least=never)


# ---- 3. wave-tile kernel, one record per tile ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["big", "mid", "mix"])
@pytest.mark.parametrize("ks", [1, 63])
def test_wave_tile_one_record_per_tile(gpu_lib, fa, po, streams, monkeypatch, ks, which):
    monkeypatch.setenv("FA_SINK", "scatter")
    monkeypatch.delenv("FA_TUPLE", raising=False)
    s = streams.get("s3-%s-%s" % (_kind(ks), which), lambda: _s3(fa, po, _kind(ks), which))
    n = len(s["off"]) - 1
    never = int((np.diff(s["off"]) > STRIDE_MAX).sum())
    assert never == {"big": n, "mid": 0, "mix": n // 2}[which]
    st = _ingest_and_check(fa, po, s, ks, slow_at_least=never)
    if which == "big":
        assert st["records_slow"] == n


# ---- 4. workgroup-tile kernel: the same edges around TILE_BYTES ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("alone", [False, True], ids=["in-tiles", "alone"])
def test_workgroup_tile_capacity_sweep(gpu_lib, fa, po, streams, monkeypatch, alone):
    """TILE_BYTES - 40 .. + 40 at the 16 alignments, behind 40 short records (multi-pass tiles) and alone (tile_recs == 1,
    the single-record tile_fits boundary): ingest through the direct sink, and decode_device."""
    monkeypatch.setenv("FA_SINK", "direct")
    s = streams.get("s4-sweep-%d" % alone, lambda: _s4_sweep(fa, po, "aspairs", alone))
    never = int((np.diff(s["off"]) > TILE_BYTES).sum())
    assert never == 40 * 16
    _ingest_and_check(fa, po, s, 1, slow_at_least=never, wave_tiles=False)
    _decode_and_check(fa, po, s)


@pytest.mark.gpu
@pytest.mark.parametrize("ks", [1, 63])
def test_workgroup_tile_multi_pass_tiles(gpu_lib, fa, po, streams, monkeypatch, ks):
    """256-record tiles of 3 and more passes, one with a record that ends exactly at the first pass's limit and one a byte
    behind it: ingest (fewer than 2^15 records: the direct sink by the library's own choice), and decode_device."""
    monkeypatch.delenv("FA_SINK", raising=False)
    s = streams.get("s4-multi-" + _kind(ks), lambda: _s4_multi(fa, po, _kind(ks)))
    _ingest_and_check(fa, po, s, ks, wave_tiles=False)
    _decode_and_check(fa, po, s)


# ---- 5. broken device offsets inside tiles staged in pieces (last in the file) ---------------------------------------------------
def _break_offsets(off, tiles, tile, cap):
    """Breaks one interior offset in each of 15 multi-part tiles: the three kinds of
    test_broken_device_offsets_are_bad_records_not_faults at five positions.  -> (broken uint32 offsets, bad records)

    Not all 15 reach the code that stages a tile in pieces.  In the workgroup-tile kernel a first bound beyond the buffer
    or at 0xfffffff0 makes the tile's own range (and the previous tile's end) insane, and both tiles go to the generic
    path record by record before any pass; only the backwards kind enters the multi-pass loop through that position.  The
    loop's handling of a broken bound is covered by the other four positions (12 cases)."""
    off32 = off.astype(np.uint32)
    broken = off32.copy()
    end = int(off[-1])
    bad = set()
    assert len(tiles) >= 15
    for t, r0 in enumerate(tiles[:15]):
        parts = _parts(off, r0, tile, cap)
        assert len(parts) >= 2 and parts[1] - r0 >= 4
        later = parts[min(1 + t % 2, len(parts) - 1)]  # the first record of the second or of the third part
        k = [r0, r0 + (parts[1] - r0) // 2, later, later - 1, r0 + tile - 1][t % 5]
        kind = t // 5
        broken[k] = [end + 5000, 0xfffffff0, int(off32[k]) - 5000 if off32[k] > 5000 else end + 77][kind]
        bad.update((k - 1, k))
    return broken, bad


def _without(buf, off, bad):
    good = np.array(sorted(set(range(len(off) - 1)) - bad))
    lens = np.diff(off).astype(np.int64)[good]
    o = np.zeros(len(good) + 1, dtype=np.int64)
    o[1:] = np.cumsum(lens)
    src = np.repeat(off[good].astype(np.int64) - o[:-1], lens) + np.arange(o[-1])
    return buf[src], o.astype(np.uint64)


def _broken_ingest(fa, po, s, ks, broken, bad, wave_tiles):
    buf, off = s["buf"], s["off"]
    n = len(off) - 1
    ref = _reference(po, *_without(buf, off, bad), ks)
    d_buf, d_off = _upload(buf, broken)
    with fa.FlowAgg(framed=True, key_sets=ks, max_batch_records=n, **CMS) as agg:
        agg.ingest_device(d_buf.data_ptr(), len(buf), d_off.data_ptr(), n)
        st = agg.stats()
        assert st["records_bad"] == len(bad) and st["records_ok"] == n - len(bad), (st["records_bad"], len(bad), st["records_ok"], n)
        _assert_key_sets(fa, agg, ks, ref)
    assert (st["wave_tile_launches"] >= 1) == wave_tiles


@pytest.mark.gpu
@pytest.mark.parametrize("ks", KEYSETS)
def test_broken_offsets_in_multi_part_wave_tiles(gpu_lib, fa, po, streams, monkeypatch, ks):
    """The records on either side of a broken bound are bad, every other record of the tile - in whichever part it is staged -
    is aggregated exactly once (the stream of test_wave_tile_full_tiles_that_overflow)."""
    monkeypatch.delenv("FA_SINK", raising=False)
    monkeypatch.delenv("FA_TUPLE", raising=False)
    s = streams.get("s2-%d" % ks, lambda: _s2(fa, po, ks))
    broken, bad = _break_offsets(s["off"], s["info"]["multi"], 64, WT_STRIDE[ks] - 16)
    assert len(bad) == 30
    _broken_ingest(fa, po, s, ks, broken, bad, wave_tiles=True)


@pytest.mark.gpu
@pytest.mark.parametrize("ks", [1, 63])
def test_broken_offsets_in_multi_pass_workgroup_tiles_ingest(gpu_lib, fa, po, streams, monkeypatch, ks):
    """The same through tile_kernel's multi-pass loop (the stream of test_workgroup_tile_multi_pass_tiles): a pass works on
    the leading run of records that fit, a record with a broken bound ends the run and goes to the generic path alone."""
    monkeypatch.delenv("FA_SINK", raising=False)
    s = streams.get("s4-multi-" + _kind(ks), lambda: _s4_multi(fa, po, _kind(ks)))
    broken, bad = _break_offsets(s["off"], s["info"]["multi"], 256, TILE_BYTES)
    assert len(bad) == 28  # (these tiles follow one another: a tile's last bound and the next one's first share a record, twice)
    _broken_ingest(fa, po, s, ks, broken, bad, wave_tiles=False)


@pytest.mark.gpu
def test_broken_offsets_in_multi_pass_workgroup_tiles_decode(gpu_lib, fa, po, streams):
    """decode_device: a clean batch first (the ctx-owned columns then hold data), the broken one behind it on the same ctx -
    bad records show status 1 and all-zero members, every other row is the oracle's."""
    s = streams.get("s4-multi-aspairs", lambda: _s4_multi(fa, po, "aspairs"))
    buf, off = s["buf"], s["off"]
    n = len(off) - 1
    ref = _ref_for(po, s, 1)
    broken, bad = _break_offsets(off, s["info"]["multi"], 256, TILE_BYTES)
    rows, status = ref["rows"].copy(), ref["status"].copy()
    b = np.array(sorted(bad))
    rows[b] = np.zeros(1, dtype=rows.dtype)
    status[b] = 1
    d_buf, d_clean = _upload(buf, off)
    _, d_broken = _upload(buf[:0], broken)
    with fa.FlowAgg(framed=True, max_batch_records=n) as agg:
        cols = agg.decode_device(d_buf.data_ptr(), len(buf), d_clean.data_ptr(), n)
        agg.sync()
        _assert_decoded(fetch_columns(cols, n), ref["rows"], ref["status"])
        cols = agg.decode_device(d_buf.data_ptr(), len(buf), d_broken.data_ptr(), n)
        agg.sync()
        got = fetch_columns(cols, n)
    _assert_decoded(got, rows, status)
