"""GPU tests of the merge of pending flows_raw parts (fa_raw_merge, fa_raw_merge_stats, the host program's -out.raw.merge;
include/flowagg.h "merging the pending flows_raw parts").

The contract is one sentence: the merged bytes are bit for bit what ONE chunk holding all those records would have built.  So
the expected bytes are those of test_raw_parts_gpu's numpy encoder (never the code under test) over the sources' rows laid end to
end in build order: rows[status == 0], a stable argsort of t32, a split where t32 // 86400 changes.  Whole parts and their
descriptions are compared with ==.  Every source is built by one fa_raw_build_columns_device call of hand-made columns (random
bytes in every column, so any two rows differ and a wrong tie order shows in the bytes), or by an ingest with a small
chunk_records.

A failed allocation inside fa_raw_merge (FA_ERR_NOMEM, nothing changed) and the limit of 2^31 - 1 pending rows have no test:
the library has no seam that forces an allocation to fail, and the rows would need 220 GiB.  Both are reasoned from
raw_merge_host.inc: every allocation and the row count are checked before the first launch, and the pending list, the image and
its size change only in the last five statements, behind the final synchronisation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_raw_parts_gpu as R
from test_raw_lz4_gpu import _check_lz4_parts, _fetch
from test_raw_parts_gpu import D0, DAY

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_CAPACITY = -1, -6
LDS_SRCS = 512  # RAW_MERGE_LDS_SRCS of csrc/raw_merge.cuh: the sources whose first rows the gather keeps in LDS


def _ok(n):
    return np.zeros(n, dtype=np.uint32)


def _sources(po, times, seed=1):
    """one source per array of TimeReceived values: [(rows, status)]"""
    return [(R._random_rows(po, len(t), seed * 1000 + i, np.asarray(t, dtype=np.uint64)), _ok(len(t))) for i, t in enumerate(times)]


def _one_chunk(sources):
    """what ONE chunk holding all the sources' records builds: [(date, rows, bytes)]"""
    return R.expected_parts(np.concatenate([r for r, _ in sources]), np.concatenate([s for _, s in sources]))


def _build_all(fa, agg, sources):
    for rows, status in sources:
        R._build(fa, agg, rows, status)


def _merged(fa, sources, chunk_records=0):
    """the sources built one by one into a fresh ctx, merged, taken -> (bytes, parts, raw_merge_stats, pending parts before)"""
    with fa.FlowAgg(framed=True) as agg:
        agg.raw_enable(chunk_records)
        _build_all(fa, agg, sources)
        before = agg.raw_stats()["pending_parts"]
        agg.raw_merge()
        data, parts = agg.raw_take()
        return data, parts, agg.raw_merge_stats(), before


def _check(fa, sources, chunk_records=0):
    data, parts, ms, before = _merged(fa, sources, chunk_records)
    want = _one_chunk(sources)
    R.check_parts(data, parts, want)
    return data, parts, ms, before, want


# ---- equal to the one-chunk build ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad_every", [0, 97], ids=["midnight shuffled", "bad records sprinkled in"])
def test_equal_to_the_one_chunk_build(gpu_lib, fa, po, bad_every):
    buf, off, rows, status = R._midnight(bad_every=bad_every)
    want = R.expected_parts(rows, status)
    with fa.FlowAgg(framed=True) as small, fa.FlowAgg(framed=True) as whole:
        small.raw_enable(chunk_records=1500)
        whole.raw_enable(chunk_records=1 << 15)
        for x in (small, whole):
            x.ingest(buf, off)
        st = small.raw_stats()
        assert st["pending_parts"] == 28 and st["chunks"] == 14 and whole.raw_stats()["pending_parts"] == 2
        small.raw_merge()
        after, ms = small.raw_stats(), small.raw_merge_stats()
        data, parts = small.raw_take()
        wdata, wparts = whole.raw_take()
    assert bytes(data) == bytes(wdata) and parts.tobytes() == wparts.tobytes()
    R.check_parts(data, parts, want)
    # the pending counters show the merged state, the built-so-far counters did not move
    assert (after["pending_parts"], after["pending_bytes"]) == (2, len(data))
    for k in ("records_in", "records_bad", "rows_out", "parts_out", "bytes_out", "chunks", "build_launches"):
        assert after[k] == st[k], k
    good = int((status == 0).sum())
    assert (ms["merges"], ms["parts_in"], ms["parts_out"], ms["rows"]) == (1, 28, 2, good)
    assert (ms["bytes_in"], ms["bytes_out"]) == (st["pending_bytes"], len(data)) and ms["bytes_out"] < ms["bytes_in"]
    assert ms["launches"] == 3 + 2 and ms["order_ns"] > 0 and ms["gather_ns"] > 0


# ---- row counts where the layout changes ------------------------------------------------------------------------------------------
MERGED_ROWS = (1, 2, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 16383, 16384)
SOURCE_ROWS = (3, 128, 1, 2, 127, 129, 255, 256, 257, 1023, 1024, 1025, 16383)  # (3 then 128: the source phases 7 and 15)


def _split(total):
    """`total` rows over sources of uneven sizes: each of SOURCE_ROWS that still fits, in that order, the rest in the last one"""
    out = []
    for s in SOURCE_ROWS:
        if sum(out) + s <= total:
            out.append(s)
    if sum(out) < total:
        out.append(total - sum(out))
    return out


def _source_phases(sizes):
    """the address phases (mod 16) at which the three FixedString(16) columns of back-to-back sources start (the image's base is
    aligned to 256 bytes and more): raw_col_offset arithmetic, restated in test_raw_parts_gpu.column_starts"""
    at, out = 0, set()
    for n in sizes:
        starts, size = R.column_starts(n)
        out |= {(at + starts[c]) % 16 for c in (5, 6, 7)}
        at += size
    return out


def test_sweep_reaches_every_source_phase():
    """(no GPU work) the sources of test_row_counts start their 16-byte columns at all 16 byte phases between them"""
    assert [sum(_split(n)) for n in MERGED_ROWS] == list(MERGED_ROWS)
    assert _split(1) == [1] and _split(2) == [1, 1] and _split(257) == [3, 128, 1, 2, 123] and len(_split(16384)) == 13
    phases = set()
    for n in MERGED_ROWS:
        phases |= _source_phases(_split(n))
    assert phases == set(range(16))


@pytest.mark.parametrize("total", MERGED_ROWS)
def test_row_counts(gpu_lib, fa, po, total):
    sizes = _split(total)
    rng = np.random.default_rng(total)
    sources = _sources(po, [D0 * DAY + rng.integers(0, 50, size=n) for n in sizes], seed=total)  # one Date, unsorted, ties
    data, parts, ms, before, want = _check(fa, sources)
    assert before == len(sizes) and len(parts) == 1 and int(parts[0]["rows"]) == total
    assert len(data) == R.column_starts(total)[1]
    assert ms["merges"] == (1 if len(sizes) > 1 else 0)  # a single source is a single part: nothing to do


# ---- number of sources --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsrc", [1, 2, 3, 17, LDS_SRCS + 1, 2 * (LDS_SRCS + 1)])
def test_number_of_sources(gpu_lib, fa, po, nsrc):
    # chunk_records = 1: every row is a chunk and a source; two Dates, so the merged parts have nsrc / 2 sources each and the
    # search runs over all of them (above LDS_SRCS: in global memory)
    rng = np.random.default_rng(nsrc)
    t = np.where(np.arange(nsrc) % 2 == 0, D0 * DAY, (D0 + 1) * DAY) + rng.integers(0, 20, size=nsrc)
    sources = _sources(po, [t], seed=nsrc)
    data, parts, ms, before, want = _check(fa, sources, chunk_records=1)
    assert before == nsrc and len(parts) == min(nsrc, 2)
    if nsrc <= 2:  # one part per Date already, in ascending Date
        assert ms["merges"] == 0 and ms["launches"] == 0
    else:
        assert (ms["merges"], ms["parts_in"], ms["parts_out"], ms["rows"]) == (1, nsrc, 2, nsrc)


# ---- ties and interleaving -----------------------------------------------------------------------------------------------------------
def _tie_cases():
    base = D0 * DAY
    return {
        "one t32": [np.full(300, base + 12345), np.full(77, base + 12345), np.full(130, base + 12345)],
        "same keys in both": [base + np.repeat(np.arange(100), 3), base + np.repeat(np.arange(100), 3)],
        "even and odd seconds": [base + 2 * np.arange(500), base + 2 * np.arange(500) + 1],
        "disjoint, reverse build order": [base + 3000 + np.arange(400), base + 2000 + np.arange(300), base + np.arange(200)],
        "t32 = 0": [np.zeros(150), np.zeros(3), np.zeros(129)],
        "t32 = 0xFFFFFFFF": [np.full(140, 2**32 - 1), np.full(131, 2**32 - 1)],
        "beyond 32 bits": [np.full(60, 2**32 + base + 5), np.concatenate([np.full(40, 7 * 2**32 + base + 5), np.full(30, base + 4)]), np.full(20, 3 * 2**32 + base + 6)],
    }


@pytest.mark.parametrize("case", list(_tie_cases()))
def test_ties_and_interleaving(gpu_lib, fa, po, case):
    sources = _sources(po, _tie_cases()[case], seed=7)
    for i, (rows, _) in enumerate(sources):
        rows["sequence_num"] = 100000 * i + np.arange(len(rows))  # (source, row in the source)
    data, parts, ms, before, want = _check(fa, sources)
    assert before == len(sources) and len(parts) == 1 and ms["merges"] == 1
    (blk,) = fa.spill.read_native(data)
    seq, t = blk["SequenceNum"].astype(np.int64), blk["TimeReceived"].astype(np.int64)
    assert (np.diff(t) >= 0).all()
    tied = np.diff(t) == 0
    assert (np.diff(seq)[tied] > 0).all()  # inside one t32: source A's rows in front of source B's, each in row order
    if case == "same keys in both":
        assert tied.sum() == 500 and seq[:6].tolist() == [0, 1, 2, 100000, 100001, 100002]
    if case == "even and odd seconds":
        assert seq[:4].tolist() == [0, 100000, 1, 100001]
    if case == "disjoint, reverse build order":
        assert seq[0] == 200000 and seq[-1] == 399
    if case == "beyond 32 bits":  # narrowed: one Date, t32 drops the high word
        assert int(parts[0]["date"]) == D0 and (int(parts[0]["t_min"]), int(parts[0]["t_max"])) == (D0 * DAY + 4, D0 * DAY + 6)
    if case == "t32 = 0xFFFFFFFF":
        assert int(parts[0]["date"]) == 49710


# ---- Dates --------------------------------------------------------------------------------------------------------------------------------
def test_three_dates_one_in_a_single_source(gpu_lib, fa, po):
    rng = np.random.default_rng(3)
    a = np.concatenate([(D0 + 2) * DAY + rng.integers(0, DAY, size=90), D0 * DAY + rng.integers(0, DAY, size=130)])
    b = np.concatenate([(D0 + 1) * DAY + rng.integers(0, DAY, size=70), D0 * DAY + rng.integers(0, DAY, size=129)])
    sources = _sources(po, [rng.permutation(a), rng.permutation(b)], seed=3)
    data, parts, ms, before, want = _check(fa, sources)
    # built as [D0, D0 + 2] then [D0, D0 + 1]: the result stands in ascending Date; D0 + 1 and D0 + 2 have one source each (copied)
    assert before == 4 and [int(p["date"]) for p in parts] == [D0, D0 + 1, D0 + 2] and [int(p["rows"]) for p in parts] == [259, 70, 90]
    assert ms["launches"] == 3 + 1


def test_one_row_per_date_across_40_dates(gpu_lib, fa, po):
    rng = np.random.default_rng(40)
    t = rng.permutation((D0 + 3 * np.arange(40)) * DAY + rng.integers(0, DAY - 1, size=40))
    data, parts, ms, before, want = _check(fa, _sources(po, [t], seed=40), chunk_records=1)
    assert before == 40 and len(parts) == 40 and all(int(p["rows"]) == 1 for p in parts)
    assert [int(p["date"]) for p in parts] == sorted(int(x) // DAY for x in t)
    assert ms["merges"] == 1 and ms["launches"] == 3  # the order alone: every Date has a single source
    # ... and with every Date in two sources
    t2 = np.concatenate([t, rng.permutation(t) + 1])
    data, parts, ms, before, want = _check(fa, _sources(po, [t2], seed=41), chunk_records=1)
    assert before == 80 and len(parts) == 40 and all(int(p["rows"]) == 2 for p in parts) and ms["launches"] == 3 + 40


def test_midnight_split_over_two_sources(gpu_lib, fa, po):
    sources = _sources(po, [np.array([86400, 86399] * 70), np.array([86399] * 30 + [86400] * 99)], seed=5)
    data, parts, ms, before, want = _check(fa, sources)
    assert before == 4 and [(int(p["date"]), int(p["rows"]), int(p["t_min"]), int(p["t_max"])) for p in parts] == [(0, 100, 86399, 86399), (1, 169, 86400, 86400)]


# ---- protocol ------------------------------------------------------------------------------------------------------------------------------
def _two_sources(po, seed):
    rng = np.random.default_rng(seed)
    return _sources(po, [np.concatenate([D0 * DAY + rng.integers(0, 99, size=n), (D0 + 2) * DAY + rng.integers(0, 99, size=n + 30)]) for n in (700, 450)], seed=seed)


def test_protocol(gpu_lib, fa, po):
    L = gpu_lib
    first, more = _two_sources(po, 1), _two_sources(po, 2)
    with fa.FlowAgg(framed=True) as off_ctx:  # not enabled
        assert L.fa_raw_merge(off_ctx._h) == ERR_ARG and b"fa_raw_enable" in L.fa_last_error(off_ctx._h)
        assert L.fa_raw_merge_stats(off_ctx._h, C.byref(fa.RawMergeStats())) == ERR_ARG
    with fa.FlowAgg(framed=True) as agg:
        agg.raw_enable()
        zero = {k: 0 for k in agg.raw_merge_stats()}
        assert len(zero) == 9
        # nothing pending: nothing changes
        agg.raw_merge()
        assert agg.raw_merge_stats() == zero and agg.raw_stats()["pending_parts"] == 0
        data, parts = agg.raw_take()
        assert len(data) == 0 and len(parts) == 0
        # a merge, and a second one that has nothing to do: the same bytes, `merges` unchanged
        _build_all(fa, agg, first)
        built = agg.raw_stats()
        assert built["pending_parts"] == 4
        agg.raw_merge()
        ms, st = agg.raw_merge_stats(), agg.raw_stats()
        assert (ms["merges"], ms["parts_in"], ms["parts_out"], ms["launches"]) == (1, 4, 2, 5)
        agg.raw_merge()
        assert agg.raw_merge_stats() == ms and agg.raw_stats() == st
        want = _one_chunk(first)
        assert (st["pending_parts"], st["pending_bytes"]) == (2, sum(len(w[2]) for w in want))
        for k in ("records_in", "rows_out", "parts_out", "bytes_out", "chunks"):
            assert st[k] == built[k], k
        # merge, ingest more, merge again: the merged part and the new parts become one part
        _build_all(fa, agg, more)
        assert agg.raw_stats()["pending_parts"] == 6
        agg.raw_merge()
        ms = agg.raw_merge_stats()
        assert (ms["merges"], ms["parts_in"], ms["parts_out"]) == (2, 4 + 6, 2 + 2)
        data, parts = agg.raw_take()
        R.check_parts(data, parts, _one_chunk(first + more))
        # the take cleared the pending list
        st = agg.raw_stats()
        assert (st["pending_parts"], st["pending_bytes"]) == (0, 0) and st["parts_out"] == 8
        agg.raw_merge()
        assert agg.raw_merge_stats() == ms
        data, parts = agg.raw_take()
        assert len(data) == 0 and len(parts) == 0
        # fa_raw_reset releases the merge's buffers, the counters go on counting, the next merge works
        _build_all(fa, agg, first)
        agg.raw_reset()
        assert agg.raw_merge_stats() == ms
        _build_all(fa, agg, first)
        agg.raw_merge()
        assert agg.raw_merge_stats()["merges"] == 3
        ptr, nbytes, dparts = agg.raw_take_device()
        R.check_parts(np.frombuffer(_fetch(ptr, nbytes), dtype=np.uint8), dparts, want)


def test_lz4_takes_deliver_the_merged_parts(gpu_lib, fa, po):
    L = gpu_lib
    sources = _two_sources(po, 3)
    want = _one_chunk(sources)
    with fa.FlowAgg(framed=True) as agg:
        agg.raw_enable()
        _build_all(fa, agg, sources)
        agg.raw_merge()
        data, parts = agg.raw_take_lz4()
        _check_lz4_parts(fa, data, parts, want)
        assert fa.spill.lz4_frames_decode(bytes(data)) == b"".join(w[2] for w in want)
        assert agg.raw_stats()["pending_parts"] == 0
        # a capacity-refused take keeps its frames; a merge makes them stale: the next take's frames hold the merged parts
        _build_all(fa, agg, sources)
        nb, npart = C.c_size_t(), C.c_size_t()
        held = np.zeros(8, dtype=fa.RAW_PART_DTYPE)
        assert L.fa_raw_take_lz4(agg._h, None, 0, C.byref(nb), held.ctypes.data, 8, C.byref(npart)) == ERR_CAPACITY and npart.value == 4
        frames = agg.raw_lz4_stats()["frames"]
        agg.raw_merge()
        data, parts = agg.raw_take_lz4()
        assert agg.raw_lz4_stats()["frames"] == frames + 2
        _check_lz4_parts(fa, data, parts, want)
        _build_all(fa, agg, sources)
        agg.raw_merge()
        ptr, nbytes, dparts = agg.raw_take_lz4_device()
        _check_lz4_parts(fa, _fetch(ptr, nbytes), dparts, want)


def test_load_of_merged_parts_gives_the_same_ranged_rows(gpu_lib, fa, po):
    from test_raw_load_gpu import _equal_reads, _folds, _reads
    buf, off, rows, status = R._midnight(bad_every=97)
    taken = {}
    for merge in (False, True):
        with fa.FlowAgg(framed=True) as agg:
            agg.raw_enable(chunk_records=4096)
            agg.ingest(buf, off)
            if merge:
                agg.raw_merge()
            taken[merge] = agg.raw_take()
    assert len(taken[False][1]) == 10 and len(taken[True][1]) == 2
    R.check_parts(taken[True][0], taken[True][1], R.expected_parts(rows, status))
    reads = {}
    for merge in (False, True):
        with _folds(fa) as agg:
            agg.raw_load(taken[merge][0])
            reads[merge] = _reads(agg)
    _equal_reads(reads[False], reads[True])


# ---- the consumer -------------------------------------------------------------------------------------------------------------------------
def test_consumer_merges_before_the_take(gpu_lib, fa, po, tmp_path):
    buf, off, rows, status = R._midnight(bad_every=97)
    exe = os.path.join(ROOT, "flow-pipeline_amd", "host", "inserter_gpu")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)], stdout=subprocess.DEVNULL)
    raw = bytes(buf)
    paths, flushes = [], set()
    for p in range(2):  # record i lives in partition i mod 2; a flush takes 3000 of a partition's records
        path = tmp_path / ("p%d.log" % p)
        mine = range(p, len(rows), 2)
        with open(path, "wb") as f:
            for k in mine:
                f.write(raw[int(off[k]):int(off[k + 1])])
        paths.append(str(path))
        for j, k in enumerate(mine):
            if status[k] == 0:
                flushes.add((p, j // 3000, int(R.t32_of(rows[k:k + 1])[0]) // DAY))
    blocks = {}
    for merge in (False, True):
        native = tmp_path / ("flows_raw_%d.native" % merge)
        r = subprocess.run([exe, "-input.files=" + ",".join(paths), "-flush.count=3000", "-gpu.batch.bytes=0", "-out.raw.native=%s" % native, "-gpu.devices=1"]
                           + (["-out.raw.merge"] if merge else []), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        blocks[merge] = fa.spill.read_native(open(native, "rb").read())
    assert len(blocks[True]) == len(flushes)  # one part per (partition, flush, Date)
    for b in blocks[True]:
        assert len(np.unique(b["Date"])) == 1 and (b["Date"] == b["TimeReceived"] // DAY).all()
        assert (np.diff(b["TimeReceived"].astype(np.int64)) >= 0).all()

    def row_strings(bs):
        return sorted(r.tobytes() for b in bs for r in np.hstack([np.ascontiguousarray(b[name]).view(np.uint8).reshape(len(b["Date"]), -1) for name, _, _, _ in R.FORMAT]))

    got = row_strings(blocks[True])
    assert len(got) == len(rows) - len(rows) // 97 and got == row_strings(blocks[False])
    # given alone the flag is a usage error
    r = subprocess.run([exe, "-input.files=" + ",".join(paths), "-out.raw.merge"], capture_output=True, text=True)
    assert r.returncode == 2 and "-out.raw.merge" in r.stderr and "out.raw.native" in r.stderr
