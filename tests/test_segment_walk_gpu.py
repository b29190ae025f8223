"""The segment walk of the three tuple-aggregation kernels (csrc/segwalk.cuh under agg_kernel, agg8_kernel, cms_agg_kernel) at
small launches, through the C ABI and bit-exact against the oracle's rollup and the CPU sketch.  Always FA_SINK=scatter.

Grids.  A scatter-sink launch has one tuple segment per ingest workgroup, so the number of workgroups is the number of segments
the walk deals out in groups of 2, 4, 16 or 32.  launch_plan.h: a wave takes wtile_recs_for() = 64 records per tile whenever the
mean record is short enough (these records are ~30 bytes; the restatement below checks it), and wtile_grid() =
ceil(ceil(n / 64) / waves) workgroups, waves = 12 for flows_5m alone and 16 with a sketch.  So n = 64 * 12 * (G - 1) + 384 records
- the last workgroup half full - give G = 1, 3, 17, 33 workgroups for n = 384, 1920, 12672, 24960: segment counts that are no
multiple of any group size, so that the last group of every pass is partly (and for the other waves wholly) padding.  The sketch
case runs 17 workgroups of 16 waves: n = 64 * 16 * 16 + 512 = 16896.  (Confirmed once on an MI355X: with FA_VERBOSE the library
reports 1, 3, 17 and 33 segments per partition for the four streams of either format, 17 for the sketch case, and 13-20 % of the
tuples in whole store units, the rest single.)

Streams.  256 partitions x G segments leave two or three tuples per segment of a uniform stream - nothing but back parts.  Half of
the records therefore carry keys of twelve partitions with geometric weights (table.cuh: the partition of a compact tuple is
SrcAS[7:0] ^ mix8(rest of the key), of a wide one key_hash >> 24 - restated below to pick the keys): their segments range from
over-full (front part, back part and the overflow fallback all used) to a handful of tuples, beside the sparse rest.  Segments
hold 40 tuples at these sizes whether FA_SEG_CAP says so or not: a front part is a single level."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRIDS = (1, 3, 17, 33)
HOT_PARTS = (0, 7, 31, 64, 100, 128, 129, 130, 200, 254, 255, 77)


def _grid(n, nbytes, lean):
    """launch_plan.h: wtile_recs_for + wtile_grid (below the chip's workgroup limit)"""
    avg, cap = nbytes / n, (4864 if lean else 5056) - 16.0 - 15.0
    r = (cap - 2.0 * 12.0 * math.sqrt(min(cap / avg, 64.0))) / avg
    tile_recs = 64 if r >= 64 else max(1, int(r))
    waves = 12 if lean else 16
    return -(-(-(-n // tile_recs)) // waves)


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & np.uint64(0xffffffff)


def _part_compact(src, dst, tb, et):
    code = np.where(et == 0x0800, 1, 2).astype(np.uint64)  # (0x0800 / 0x86dd only)
    lo = dst | ((src >> np.uint64(8)) << np.uint64(20))
    kh = (tb & np.uint64(15)) | (code << np.uint64(4))
    mix = _u32(_u32(lo ^ _u32(kh << np.uint64(26))) * np.uint64(0x9E3779B1)) >> np.uint64(24)
    return ((src & np.uint64(0xff)) ^ mix).astype(np.int64)


def _part_wide(src, dst, tb, et):
    a, b, c, d = src, dst | np.uint64(0x80000000), et, (tb & np.uint64(0x7ffffff)) | np.uint64(0x80000000)
    h = _u32(a * np.uint64(0x9E3779B1) + b)
    h ^= h >> np.uint64(15)
    h = _u32((h ^ c ^ _u32((d << np.uint64(13)) | (d >> np.uint64(19)))) * np.uint64(0x85EBCA6B))
    h ^= h >> np.uint64(13)
    h = _u32(h * np.uint64(0xC2B2AE35))
    h ^= h >> np.uint64(16)
    return (h >> np.uint64(24)).astype(np.int64)


def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def _stream(po_t0, fmt, grid):
    """(buf, off) of n framed records whose keys concentrate on HOT_PARTS of the format's partition function"""
    n = 64 * 12 * (grid - 1) + 384
    rng = np.random.default_rng(1000 * int(fmt) + grid)
    m = 300_000  # candidate keys: ~1170 per partition
    src = rng.integers(1, 1 << 20, m).astype(np.uint64)
    dst = rng.integers(1, 1 << 20, m).astype(np.uint64)
    secs = rng.integers(0, 600, m).astype(np.uint64)  # two 5-minute buckets
    et = np.where(rng.random(m) < 0.7, 0x0800, 0x86dd).astype(np.uint64)
    tb = (np.uint64(po_t0) + secs) // np.uint64(300)
    part = (_part_compact if fmt == "8" else _part_wide)(src, dst, tb, et)
    order = np.argsort(part, kind="stable")
    start = np.searchsorted(part[order], np.arange(257))
    w = 0.7 ** np.arange(len(HOT_PARTS))
    hot = rng.random(n) < 0.5
    target = np.where(hot, np.asarray(HOT_PARTS)[rng.choice(len(HOT_PARTS), n, p=w / w.sum())], rng.integers(0, 256, n))
    pool = np.minimum(start[target + 1] - start[target], np.where(hot, 600, 40))  # keys repeat: groups hold several tuples
    assert (pool > 0).all()
    pick = order[start[target] + rng.integers(0, 1 << 30, n) % pool]
    by, pk = rng.integers(1, 1 << 17, n), rng.integers(1, 1 << 9, n)
    recs = []
    for i, k in enumerate(pick.tolist()):
        payload = (b"\x10" + _varint(po_t0 + int(secs[k])) + b"\x18\x01" + b"\x48" + _varint(int(by[i])) + b"\x50" + _varint(int(pk[i]))
                   + b"\x70" + _varint(int(src[k])) + b"\x78" + _varint(int(dst[k])) + b"\xf0\x01" + _varint(int(et[k])))
        recs.append(_varint(len(payload)) + payload)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    buf = np.frombuffer(b"".join(recs), dtype=np.uint8)
    assert _grid(n, len(buf), True) == grid
    return buf, off


@pytest.mark.parametrize("seg_cap", [None, "40"])
@pytest.mark.parametrize("fmt,passes", [("8", "1"), ("8", "2"), ("8", "8"), ("16", None)])
def test_small_grids_fold_exactly(gpu_lib, fa, po, monkeypatch, fmt, passes, seg_cap):
    """One ctx, four launches of 1, 3, 17 and 33 workgroups: after every launch the rows are the oracle's rollup of everything
    ingested so far - compact tuples in 1, 2 and 8 passes of agg8_kernel, wide tuples through agg_kernel."""
    monkeypatch.setenv("FA_SINK", "scatter")
    monkeypatch.setenv("FA_TUPLE", fmt)
    for name, v in (("FA_AGG_PASSES", passes), ("FA_SEG_CAP", seg_cap)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    ref = po.Rollup(300)
    with fa.FlowAgg(framed=True) as agg:
        for launches, grid in enumerate(GRIDS, 1):
            buf, off = _stream(po.T0, fmt, grid)
            assert ref.ingest(buf, off, 1) == 0
            agg.ingest(buf, off)
            assert agg.read_window().tobytes() == ref.rows().tobytes(), grid
            st = agg.stats()
            assert st["wave_tile_launches"] == launches and st["compact_tuple_launches"] == (launches if fmt == "8" else 0), st
            assert st["records_bad"] == 0 and st["records_misfit_compact"] == 0, st


def test_sketch_tuples_fold_exactly_with_slices(gpu_lib, fa, po, monkeypatch):
    """AS pairs + both Count-Min sketches on a Zipf-1.1 stream, 17 workgroups, two launches: the second launch of
    cms_agg_kernel draws its schedule from the first one's partition sizes and cuts the heavy hitters' partitions into slices.
    Sketches and rows equal the CPU's, counter for counter."""
    monkeypatch.setenv("FA_SINK", "scatter")
    for name in ("FA_TUPLE", "FA_AGG_PASSES", "FA_SEG_CAP", "FA_CMS"):
        monkeypatch.delenv(name, raising=False)
    n, depth, wl2, seed = 64 * 16 * 16 + 512, 4, 14, 0xC0FFEE
    gp = po.gen_params(mode=po.GEN_ZIPF, framed=1, seed=57, n_total=n, zipf_log2_universe=12, zipf_s_x100=110)
    buf, off = po.gen_records(gp, 0, n)
    assert _grid(n, len(buf), False) == 17
    rows, status = po.decode_batch(buf, off, 1)
    assert status.sum() == 0
    with np.errstate(over="ignore"):
        w = rows["bytes"] * rows["sampling_rate"]
    ref = po.Rollup(300)
    with fa.FlowAgg(framed=True, key_sets=7, cms_depth=depth, cms_width_log2=wl2, cms_seed=seed, topk_capacity_log2=14) as agg:
        for launches in (1, 2):
            agg.ingest(buf, off)
            assert ref.ingest(buf, off, 1) == 0
            for col, key_set in (("src_addr", fa.FA_KEYS_SRCADDR_CMS), ("dst_addr", fa.FA_KEYS_DSTADDR_CMS)):
                want = po.cms_sketch_numpy(rows[col], w, depth, wl2, seed) * np.uint64(launches)
                assert np.array_equal(agg.cms_read(key_set).reshape(-1), want), (col, launches)
            assert agg.read_window().tobytes() == ref.rows().tobytes(), launches
        assert agg.stats()["wave_tile_launches"] == 2
