"""GPU tests of the LZ4 frames (fa_raw_take_lz4, fa_raw_take_lz4_device, fa_lz4_frame_device, fa_raw_lz4_stats, the host program's
-out.raw.native.lz4; include/flowagg.h "ABI 8, addition: LZ4 frames of the flows_raw parts").

The expected bytes never come from the code under test: every frame is walked and decoded by tests/lz4_cases.py - a decoder
that asserts the block format's rules - and compared with the input, or with the numpy encoder of test_raw_parts_gpu.py for
parts.  Where the machine has liblz4, the same frames are decoded by LZ4F_decompress too, in tests of their own that skip
visibly without it.

Part sizes (test_parts_*): a part is 110 * rows + 284 + len(varuint(rows)) bytes, which is EVEN only for 128 <= rows < 16384
(and again from 2^21 rows, 230 MB).  In that range the last 64 KiB block of a part is 14 bytes long at 4168 rows and the part is
an exact multiple of 65536 at 6551 rows; last blocks of 2 and of 12 bytes do not exist for any part below 2^21 rows (the search
in the test shows it).  Those two lengths are therefore driven with the first 65536 + 2 and 65536 + 12 bytes of a real part
through fa_lz4_frame_device, and parts with last blocks of 3 and 13 bytes (20254 and 23233 rows; 1 and 11 bytes need more than
32768 rows) through fa_raw_take_lz4: a last block under 13 bytes, and the shortest one that is not."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import lz4_cases as Z

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_CAPACITY = -1, -6


@functools.lru_cache(maxsize=None)
def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def _fetch(ptr, n):
    out = np.zeros(n, dtype=np.uint8)
    if n:
        assert _hip().hipMemcpy(out.ctypes.data, ptr, n, 2) == 0  # hipMemcpyDeviceToHost
    return out.tobytes()


def _frame_device(agg, data):
    """data -> its frame, compressed on the device (the input sits in a device buffer of exactly its size)"""
    import torch
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda() if len(data) else torch.zeros(0, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptr, n = agg.lz4_frame_device(t.data_ptr() if len(data) else 0, len(data))
    assert n <= agg._L.fa_lz4_frame_bound(len(data))
    return _fetch(ptr, n)


@pytest.fixture(scope="module")
def edge_frames(gpu_lib, fa):
    """every edge size x pattern through fa_lz4_frame_device, once: [(pattern, n, input, frame)]"""
    out = []
    with fa.FlowAgg(framed=True) as agg:  # (no fa_raw_enable: the door works on any ctx)
        for p in Z.PATTERNS:
            for n in Z.EDGE_SIZES:
                d = Z.pattern(p, n)
                out.append((p, n, d, _frame_device(agg, d)))
        st = agg.raw_lz4_stats()
    assert st["frames"] == len(out) and st["bytes_in"] == sum(len(d) for _, _, d, _ in out) and st["bytes_out"] == sum(len(f) for _, _, _, f in out)
    return out


@pytest.fixture(scope="module")
def mixed_frames(gpu_lib, fa):
    with fa.FlowAgg(framed=True) as agg:
        return [(d, _frame_device(agg, d)) for d in Z.mixed_inputs()]


# ---- 1: edge sizes -------------------------------------------------------------------------------------------------------------------
def test_edge_sizes(edge_frames):
    assert len(edge_frames) == len(Z.PATTERNS) * len(Z.EDGE_SIZES)
    for p, n, data, frame in edge_frames:
        (got, blocks), = Z.walk_frames(frame)
        assert got == data, (p, n)
        assert len(blocks) == (n + Z.BLOCK - 1) // Z.BLOCK
        if n == 0:
            assert frame == Z.HEADER + Z.ENDMARK and len(frame) == 11
        if p == "random" or n < 13:
            assert all(s for s, _ in blocks), (p, n)  # nothing to find, or under 13 bytes: stored
        if p in ("one byte", "period 2", "period 3", "period 16", "period 64") and n >= 65535:
            assert not blocks[0][0], (p, n)  # position 0 against an empty slot included: the repetition is found
        if p == "period 65536" and n > 65536:
            assert blocks[0][0]  # block 2 equals block 1, and still decodes alone


def test_edge_sizes_liblz4(edge_frames):
    if Z.liblz4() is None:
        pytest.skip("no liblz4 on this machine: the frames were checked with the tests' own decoder only")
    for p, n, data, frame in edge_frames:
        assert Z.liblz4_decode(frame, n) == data, (p, n)


# ---- 2: seeded mixed inputs ------------------------------------------------------------------------------------------------------------
def test_mixed_inputs(mixed_frames):
    assert len(mixed_frames) == 200
    stored = compressed = 0
    for k, (data, frame) in enumerate(mixed_frames):
        (got, blocks), = Z.walk_frames(frame)
        assert got == data, "input %d (%d bytes)" % (k, len(data))
        stored += sum(1 for s, _ in blocks if s)
        compressed += sum(1 for s, _ in blocks if not s)
    assert compressed > 100, (stored, compressed)


def test_mixed_inputs_liblz4(mixed_frames):
    if Z.liblz4() is None:
        pytest.skip("no liblz4 on this machine: the frames were checked with the tests' own decoder only")
    for data, frame in mixed_frames:
        assert Z.liblz4_decode(frame, len(data)) == data
    joined = b"".join(d for d, _ in mixed_frames[::9])
    assert Z.liblz4_decode(b"".join(f for _, f in mixed_frames[::9]), len(joined)) == joined


# ---- 3: redundancy is found ------------------------------------------------------------------------------------------------------------
def test_redundancy_is_found(edge_frames):
    """A full block of one repeated byte, and one of a repeating 16-byte pattern: at most 1024 bytes each.  The format's minimum
    for such a block is about 262 bytes, 257 of them length bytes; the wave-parallel search adds at most two steps of 64
    literals; liblz4 gives 267 and 283."""
    for p in ("one byte", "period 16"):
        frame = next(f for pp, n, _, f in edge_frames if pp == p and n == 65536)
        size = int.from_bytes(frame[7:11], "little")
        print("%s: block of %d bytes" % (p, size))
        assert size <= 1024 and len(frame) == 7 + 4 + size + 4


# ---- 4: parts ------------------------------------------------------------------------------------------------------------------------
def _part_size(rows):
    v, n = rows, 1
    while v >= 128:
        v >>= 7
        n += 1
    return 110 * rows + 284 + n


def _rows_for_last_block(length):
    """the smallest row count up to 32768 whose part ends in a block of `length` bytes (0: an exact multiple), or None"""
    return next((r for r in range(1, 32769) if _part_size(r) % Z.BLOCK == length and _part_size(r) > Z.BLOCK), None)


def _check_lz4_parts(fa, data, parts, want, plain_parts=None):
    """every frame decodes to the numpy encoder's bytes of its part; offset / bytes tile the compressed bytes"""
    assert len(parts) == len(want)
    at = 0
    for i, (p, (date, r, blob)) in enumerate(zip(parts, want)):
        assert int(p["offset"]) == at and int(p["bytes"]) > 0
        frame = bytes(data[at:at + int(p["bytes"])])
        got = Z.decode_one(frame)
        assert got == blob, "part %d of Date %d, %d rows" % (i, date, len(r))
        assert (int(p["date"]), int(p["rows"])) == (date, len(r)) and len(blob) == fa.lib().fa_raw_part_bytes(len(r))
        if plain_parts is not None:
            for f in ("date", "t_min", "t_max", "rows"):
                assert p[f] == plain_parts[i][f]
        at += int(p["bytes"])
    assert at == len(data)


def test_parts_stream(gpu_lib, fa, po):
    """two Dates, bad records, several chunks: the stream of test_raw_parts_gpu.py's chunk-seam test"""
    import test_raw_parts_gpu as R
    buf, off, rows, status = R._midnight(bad_every=97)
    n = 10000
    end = int(off[n])
    want = []
    for a in range(0, n, 4096):
        want += R.expected_parts(rows[a:min(a + 4096, n)], status[a:min(a + 4096, n)])
    assert len(want) == 6 and len({w[0] for w in want}) == 2
    with fa.FlowAgg(framed=True) as agg, fa.FlowAgg(framed=True) as plain:
        for x in (agg, plain):
            x.raw_enable(chunk_records=4096)
            x.ingest(buf[:end], off[:n + 1])
        data, parts = agg.raw_take_lz4()
        pdata, pparts = plain.raw_take()
        assert agg.raw_stats()["pending_parts"] == 0 and agg.raw_stats()["pending_bytes"] == 0
        st = agg.raw_lz4_stats()
    R.check_parts(pdata, pparts, want)
    _check_lz4_parts(fa, data, parts, want, pparts)
    assert fa.spill.lz4_frames_decode(data) == bytes(pdata)
    assert len(fa.spill.read_native(data)) == 6
    assert st["frames"] == 6 and st["bytes_in"] == len(pdata) and st["bytes_out"] == len(data) and st["compress_launches"] == 3
    assert st["blocks"] == sum((len(w[2]) + Z.BLOCK - 1) // Z.BLOCK for w in want) and st["device_ns"] == st["block_ns"] + st["pack_ns"] > 0
    if Z.liblz4() is not None:
        assert Z.liblz4_decode(data, len(pdata)) == bytes(pdata)


def test_parts_last_block_lengths(gpu_lib, fa, po):
    import test_raw_parts_gpu as R
    found = {length: _rows_for_last_block(length) for length in (2, 12, 14, 0, 3, 13)}
    assert found == {2: None, 12: None, 14: 4168, 0: 6551, 3: 20254, 13: 23233}  # (the module's docstring)
    with fa.FlowAgg(framed=True) as agg:
        agg.raw_enable(chunk_records=1 << 16)
        want = []
        for length in (14, 0, 3, 13):
            nrows = found[length]
            assert fa.lib().fa_raw_part_bytes(nrows) == _part_size(nrows) and _part_size(nrows) % Z.BLOCK == length
            t = R.D0 * R.DAY + np.sort(np.random.default_rng(nrows).integers(0, 600, size=nrows))
            rows = R._random_rows(po, nrows, 300 + length, t)
            rows["src_as"] = 65000 + (rows["src_as"] % 3)  # (some columns compress, the random ones are stored)
            rows["dst_as"] = 65001
            rows["sampling_rate"] = 1
            status = np.zeros(nrows, dtype=np.uint32)
            R._build(fa, agg, rows, status)
            want += R.expected_parts(rows, status)
        data, parts = agg.raw_take_lz4()
        _check_lz4_parts(fa, data, parts, want)
        at = 0
        for length, p in zip((14, 0, 3, 13), parts):
            (_, blocks), = Z.walk_frames(data[at:at + int(p["bytes"])])
            assert blocks[-1][1] == (length or Z.BLOCK), (length, blocks[-1])
            if 0 < length < 13:
                assert blocks[-1][0]  # a last block under 13 bytes is stored
            assert any(not s for s, _ in blocks) and any(s for s, _ in blocks)
            at += int(p["bytes"])
        if Z.liblz4() is not None:
            assert Z.liblz4_decode(data, sum(len(w[2]) for w in want)) == b"".join(w[2] for w in want)
        # last blocks of 2 and 12 bytes, which no part has: the head of a real part through the other door
        blob = want[0][2]
        for extra in (2, 12):
            d = blob[:Z.BLOCK + extra]
            (got, blocks), = Z.walk_frames(_frame_device(agg, d))
            assert got == d and blocks[-1] == (True, extra)


# ---- 5: ratio floor on a mock-shaped part -------------------------------------------------------------------------------------------------
def _mock_shaped_rows(po, n=20000, seed=1):
    import test_raw_parts_gpu as R
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, dtype=po.ROW_DTYPE)
    t = np.sort(R.D0 * R.DAY + 40000 + rng.integers(0, 600, size=n)).astype(np.uint64)
    rows["time_received"] = t
    rows["time_flow_start"] = t
    rows["sequence_num"] = np.arange(n)
    rows["sampling_rate"] = 1
    for f in ("src_addr", "dst_addr"):
        a = np.zeros((n, 16), dtype=np.uint8)
        a[:, :8] = [0x20, 0x01, 0x0D, 0xB8, 0, 0, 0, 1]
        a[:, 15] = rng.integers(0, 256, size=n)
        rows[f] = a
    rows["src_as"] = 65000 + rng.integers(0, 3, size=n)
    rows["dst_as"] = 65000 + rng.integers(0, 3, size=n)
    rows["etype"] = 0x86DD
    rows["proto"] = 0
    rows["src_port"] = rng.integers(0, 65536, size=n)
    rows["dst_port"] = rng.integers(0, 65536, size=n)
    rows["bytes"] = rng.integers(0, 1500, size=n)
    rows["packets"] = rng.integers(0, 100, size=n)
    return rows


def test_ratio_floor_on_a_mock_shaped_part(gpu_lib, fa, po):
    """Guards against a kernel that quietly stores everything: the frame of a mock-shaped part of 20000 rows is at most half
    the part's bytes (liblz4 alone reaches 1 / 3.82 on this shape in 64 KiB blocks).  A condition, not the measurement."""
    import test_raw_parts_gpu as R
    rows = _mock_shaped_rows(po)
    status = np.zeros(len(rows), dtype=np.uint32)
    (date, r, blob), = R.expected_parts(rows, status)
    assert len(blob) == 110 * 20000 + 287
    with fa.FlowAgg(framed=True) as agg:
        agg.raw_enable(chunk_records=1 << 16)
        R._build(fa, agg, rows, status)
        data, parts = agg.raw_take_lz4()
        st = agg.raw_lz4_stats()
    _check_lz4_parts(fa, data, parts, [(date, r, blob)])
    print("mock-shaped part: %d bytes -> %d (ratio %.3f), %d of %d blocks stored" % (len(blob), len(data), len(blob) / len(data), st["stored_blocks"], st["blocks"]))
    assert 2 * len(data) <= len(blob)
    assert st["stored_blocks"] == sum(1 for s, _ in Z.walk_frames(data)[0][1] if s)


# ---- 6: the capacity protocol ----------------------------------------------------------------------------------------------------------
def _two_date_rows(po, seed):
    import test_raw_parts_gpu as R
    t = np.concatenate([np.full(700, R.D0 * R.DAY + 9), np.full(900, (R.D0 + 2) * R.DAY + 1)]).astype(np.uint64)
    rows = R._random_rows(po, len(t), seed, t)
    rows["sampling_rate"] = 1
    rows["etype"] = 0x800
    return rows, np.zeros(len(t), dtype=np.uint32)


def test_capacity_protocol(gpu_lib, fa, po):
    import test_raw_parts_gpu as R
    L = gpu_lib
    rows, status = _two_date_rows(po, 21)
    more, more_status = _two_date_rows(po, 22)
    want, want_more = R.expected_parts(rows, status), R.expected_parts(more, more_status)
    nb, npart = C.c_size_t(), C.c_size_t()
    parts = np.zeros(8, dtype=fa.RAW_PART_DTYPE)
    out = np.zeros(2 * sum(len(w[2]) for w in want + want_more), dtype=np.uint8)

    def take(agg, o, cap, pcap):
        nb.value = npart.value = 12345
        return L.fa_raw_take_lz4(agg._h, o.ctypes.data if o is not None else None, cap, C.byref(nb), parts.ctypes.data, pcap, C.byref(npart))

    with fa.FlowAgg(framed=True) as agg:
        agg.raw_enable()
        R._build(fa, agg, rows, status)
        assert take(agg, out, 10, 8) == ERR_CAPACITY and npart.value == 2  # a too small `out`
        total = nb.value
        assert 11 * 2 < total < sum(len(w[2]) for w in want) + 2 * 11 + 8 * 4
        assert b"fa_raw_take_lz4" in L.fa_last_error(agg._h)
        launches = agg.raw_lz4_stats()["compress_launches"]
        assert launches == 3
        for o, cap, pcap in ((out, total - 1, 8), (out, total, 1), (None, 0, 8)):  # ... by one byte, too few parts, no buffer
            assert take(agg, o, cap, pcap) == ERR_CAPACITY and (nb.value, npart.value) == (total, 2)
            st = agg.raw_stats()
            assert st["pending_parts"] == 2 and st["pending_bytes"] == sum(len(w[2]) for w in want)  # nothing was consumed
        assert agg.raw_lz4_stats()["compress_launches"] == launches
        assert take(agg, out, total, 2) == 0 and (nb.value, npart.value) == (total, 2)
        assert agg.raw_lz4_stats()["compress_launches"] == launches  # the retry compressed nothing
        _check_lz4_parts(fa, out[:total], parts[:2], want)
        assert agg.raw_stats()["pending_parts"] == 0
        # one more chunk between the failure and the retry: all parts, in order; only the new ones are compressed
        R._build(fa, agg, rows, status)
        assert take(agg, out, 0, 8) == ERR_CAPACITY and npart.value == 2
        total = nb.value
        frames_before = agg.raw_lz4_stats()["frames"]
        R._build(fa, agg, more, more_status)
        assert take(agg, out, total, 8) == ERR_CAPACITY and npart.value == 4 and nb.value > total
        assert agg.raw_lz4_stats()["frames"] == frames_before + 2
        total4 = nb.value
        assert take(agg, out, out.size, 8) == 0 and (nb.value, npart.value) == (total4, 4)
        _check_lz4_parts(fa, out[:total4], parts[:4], want + want_more)
        assert take(agg, out, out.size, 8) == 0 and (nb.value, npart.value) == (0, 0)
        # fa_raw_take_lz4_device + a copy == fa_raw_take_lz4
        R._build(fa, agg, rows, status)
        ptr, nbytes, dparts = agg.raw_take_lz4_device()
        assert nbytes > 22 and ptr
        dev = _fetch(ptr, nbytes)
        _check_lz4_parts(fa, dev, dparts, want)
        assert agg.raw_stats()["pending_parts"] == 0


# ---- 7: mixing ---------------------------------------------------------------------------------------------------------------------------
def test_mixing_with_the_plain_take(gpu_lib, fa, po):
    import test_raw_parts_gpu as R
    L = gpu_lib
    rows, status = _two_date_rows(po, 31)
    want = R.expected_parts(rows, status)
    nb, npart = C.c_size_t(), C.c_size_t()
    parts = np.zeros(8, dtype=fa.RAW_PART_DTYPE)
    out = np.zeros(8, dtype=np.uint8)
    with fa.FlowAgg(framed=True) as agg:
        agg.raw_enable()
        # nothing pending: 0 bytes, 0 parts
        assert L.fa_raw_take_lz4(agg._h, out.ctypes.data, out.size, C.byref(nb), parts.ctypes.data, 8, C.byref(npart)) == 0 and (nb.value, npart.value) == (0, 0)
        data, p = agg.raw_take_lz4()
        assert data == b"" and len(p) == 0
        # a plain take after a failed LZ4 take: the plain bytes, and nothing is left for either
        R._build(fa, agg, rows, status)
        assert L.fa_raw_take_lz4(agg._h, out.ctypes.data, out.size, C.byref(nb), parts.ctypes.data, 8, C.byref(npart)) == ERR_CAPACITY and npart.value == 2
        pdata, pparts = agg.raw_take()
        R.check_parts(pdata, pparts, want)
        assert agg.raw_stats()["pending_parts"] == 0
        data, p = agg.raw_take_lz4()
        assert data == b"" and len(p) == 0
        # the kept frames of the taken parts are not delivered for the next ones
        other, other_status = _two_date_rows(po, 32)
        R._build(fa, agg, other, other_status)
        data, p = agg.raw_take_lz4()
        _check_lz4_parts(fa, data, p, R.expected_parts(other, other_status))
        # reset (after a failed LZ4 take), then a build, then a take
        R._build(fa, agg, rows, status)
        assert L.fa_raw_take_lz4(agg._h, out.ctypes.data, out.size, C.byref(nb), parts.ctypes.data, 8, C.byref(npart)) == ERR_CAPACITY
        agg.raw_reset()
        assert agg.raw_stats()["pending_parts"] == 0
        data, p = agg.raw_take_lz4()
        assert data == b"" and len(p) == 0
        R._build(fa, agg, rows, status)
        frames = agg.raw_lz4_stats()["frames"]
        data, p = agg.raw_take_lz4()
        _check_lz4_parts(fa, data, p, want)
        assert agg.raw_lz4_stats()["frames"] == frames + 2  # (the counters went on counting across the reset)
        # fa_lz4_frame_device in between leaves the parts alone
        R._build(fa, agg, rows, status)
        assert Z.decode_one(_frame_device(agg, b"abcd" * 5000)) == b"abcd" * 5000
        data, p = agg.raw_take_lz4()
        _check_lz4_parts(fa, data, p, want)
    with fa.FlowAgg(framed=True) as off_ctx:  # without fa_raw_enable: FA_ERR_ARG from both takes, FA_OK from fa_lz4_frame_device
        assert L.fa_raw_take_lz4(off_ctx._h, out.ctypes.data, out.size, C.byref(nb), parts.ctypes.data, 8, C.byref(npart)) == ERR_ARG
        assert b"fa_raw_enable" in L.fa_last_error(off_ctx._h)
        ptr = C.c_void_p()
        assert L.fa_raw_take_lz4_device(off_ctx._h, C.byref(ptr), C.byref(nb), parts.ctypes.data, 8, C.byref(npart)) == ERR_ARG
        assert L.fa_lz4_frame_device(off_ctx._h, None, 0, C.byref(ptr), C.byref(nb)) == 0 and nb.value == 11
        assert _fetch(ptr.value, 11) == Z.HEADER + Z.ENDMARK
        assert L.fa_lz4_frame_device(off_ctx._h, None, 5, C.byref(ptr), C.byref(nb)) == ERR_ARG
        assert L.fa_lz4_frame_device(off_ctx._h, None, 0, None, C.byref(nb)) == ERR_ARG
        assert L.fa_raw_lz4_stats(off_ctx._h, None) == ERR_ARG
        assert off_ctx.raw_lz4_stats()["frames"] == 1


# ---- 8: the host program ---------------------------------------------------------------------------------------------------------------
def test_consumer_writes_both_files(gpu_lib, fa, po, tmp_path):
    import test_raw_parts_gpu as R
    buf, off, rows, status = R._midnight(bad_every=97)
    exe = os.path.join(ROOT, "flow-pipeline_amd", "host", "inserter_gpu")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.dirname(exe)], stdout=subprocess.DEVNULL)
    raw = bytes(buf)
    n = 6000
    path = tmp_path / "p0.log"
    with open(path, "wb") as f:
        f.write(raw[:int(off[n])])
    a, b, only = tmp_path / "flows_raw.native", tmp_path / "flows_raw.native.lz4", tmp_path / "only.native.lz4"
    common = [exe, "-input.files=%s" % path, "-flush.count=2500", "-gpu.batch.bytes=0", "-gpu.devices=1"]
    r = subprocess.run(common + ["-out.raw.native=%s" % a, "-out.raw.native.lz4=%s" % b], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    plain, packed = open(a, "rb").read(), open(b, "rb").read()
    assert len(plain) > 110 * (n - n // 97 - 1) and fa.spill.lz4_frames_decode(packed) == plain
    frames = Z.walk_frames(packed)
    assert b"".join(d for d, _ in frames) == plain and len(frames) == len(fa.spill.read_native(plain)) >= 3
    assert len(packed) < len(plain)
    r = subprocess.run(common + ["-out.raw.native.lz4=%s" % only], capture_output=True, text=True)  # the LZ4 file alone
    assert r.returncode == 0, r.stderr
    assert fa.spill.lz4_frames_decode(open(only, "rb").read()) == plain
    # the plain file beside the LZ4 one is the file the plain take writes
    alone = tmp_path / "alone.native"
    r = subprocess.run(common + ["-out.raw.native=%s" % alone], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(alone, "rb").read() == plain
