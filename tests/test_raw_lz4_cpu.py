"""CPU tests of the LZ4 frames (include/flowagg.h "ABI 8, addition: LZ4 frames of the flows_raw parts"): the ABI surface; the host
twin fa_lz4_frame over the edge sizes, patterns and mixed inputs the GPU tests compress on the device (tests/lz4_cases.py), decoded
with the tests' own decoder and, where the machine has it, liblz4's; the header bytes; spill.lz4_frames_decode over frames that
liblz4 wrote; and the helpers the kernel shares with the host (tests/host_lz4.hip) against statements in this file.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import lz4_cases as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LZ4_FUNCS = ["fa_raw_take_lz4", "fa_raw_take_lz4_device", "fa_lz4_frame_device", "fa_lz4_frame", "fa_raw_lz4_stats"]
ERR_ARG, ERR_CAPACITY = -1, -6


def test_abi_surface(fa):
    if not os.path.exists(fa.LIB_PATH):
        fa.build()
    L = C.CDLL(fa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "flowagg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    bound = fa.lib()
    for f in LZ4_FUNCS + ["fa_lz4_frame_bound"]:
        assert hasattr(L, f), "libflowagg.so does not export %s" % f
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % f, code), "flowagg.h does not declare %s" % f
        assert f in fa.EXPORTS
        assert getattr(bound, f).argtypes, "%s has no argtypes" % f
    vp, sz, szp = C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)
    assert list(bound.fa_raw_take_lz4.argtypes) == list(bound.fa_raw_take.argtypes) == [vp, vp, sz, szp, vp, sz, szp]
    assert list(bound.fa_raw_take_lz4_device.argtypes) == list(bound.fa_raw_take_device.argtypes)
    assert list(bound.fa_lz4_frame.argtypes) == [vp, sz, vp, sz, szp] and bound.fa_lz4_frame_bound.restype is sz
    # no new ABI version, and the pinned sizes stay put
    assert bound.fa_abi_version() == 8 and C.sizeof(fa.Config) == 64 and C.sizeof(fa.Stats) == 312
    assert C.sizeof(fa.RawPart) == 40 == fa.RAW_PART_DTYPE.itemsize and C.sizeof(fa.RawStats) == 80 and C.sizeof(fa.RawLz4Stats) == 72
    assert bound.fa_row_bytes(10) == 0 and bound.fa_row_bytes(8) == bound.fa_row_bytes(9) == 40
    assert "ABI 8, addition: LZ4 frames of the flows_raw parts" in hdr
    m = re.search(r"typedef struct \{([^}]*)\} fa_raw_lz4_stats_t;", code)
    assert re.findall(r"\b(\w+)\s*[,;]", m.group(1)) == [n for n, _ in fa.RawLz4Stats._fields_]
    # the doors of the binding
    for name in ("raw_take_lz4", "raw_take_lz4_device", "lz4_frame_device", "raw_lz4_stats"):
        assert callable(getattr(fa.FlowAgg, name))
    assert "out" in inspect.signature(fa.FlowAgg.raw_take_lz4).parameters
    assert callable(fa.spill.lz4_frames_decode) and callable(fa.lz4_frame)
    # null arguments
    n = C.c_size_t()
    assert bound.fa_lz4_frame(None, 5, None, 0, C.byref(n)) == ERR_ARG and bound.fa_lz4_frame(None, 0, None, 0, None) == ERR_ARG
    assert bound.fa_raw_take_lz4(None, None, 0, C.byref(n), None, 0, C.byref(n)) == ERR_ARG


def _twin(fa, data):
    L = fa.lib()
    a = np.frombuffer(data, dtype=np.uint8)
    bound = L.fa_lz4_frame_bound(len(data))
    assert bound == len(data) + 11 + 4 * ((len(data) + Z.BLOCK - 1) // Z.BLOCK)
    out = np.full(bound + 16, 0xEE, dtype=np.uint8)
    n = C.c_size_t()
    assert L.fa_lz4_frame(a.ctypes.data if len(data) else None, len(data), out.ctypes.data, bound, C.byref(n)) == 0
    assert n.value <= bound and (out[n.value:] == 0xEE).all(), "the bound is exceeded or bytes are written behind the frame"
    return out[:n.value].tobytes()


def _edge_cases():
    return [(p, n) for p in Z.PATTERNS for n in Z.EDGE_SIZES]


@pytest.fixture(scope="module")
def twin_frames(fa):
    """fa_lz4_frame over every input, once: [(input, frame)]"""
    inputs = [Z.pattern(p, n) for p, n in _edge_cases()] + list(Z.mixed_inputs())
    return [(d, _twin(fa, d)) for d in inputs]


def test_host_twin_round_trips(fa, twin_frames):
    assert len(twin_frames) == len(Z.PATTERNS) * len(Z.EDGE_SIZES) + 200
    stored = compressed = 0
    for data, frame in twin_frames:
        frames = Z.walk_frames(frame)
        assert len(frames) == 1 and frames[0][0] == data, "%d bytes do not come back" % len(data)
        assert len(frames[0][1]) == (len(data) + Z.BLOCK - 1) // Z.BLOCK
        stored += sum(1 for s, _ in frames[0][1] if s)
        compressed += sum(1 for s, _ in frames[0][1] if not s)
        assert fa.spill.lz4_frames_decode(frame) == data
    assert stored > 30 and compressed > 150  # both kinds of block are there in numbers
    # a block under 13 bytes is stored, a block of one repeated byte is not
    for n in (1, 4, 5, 12):
        assert Z.walk_frames(_twin(fa, Z.pattern("one byte", n)))[0][1] == [(True, n)]
    assert Z.walk_frames(_twin(fa, Z.pattern("one byte", 65536)))[0][1] == [(False, 65536)]
    assert len(_twin(fa, Z.pattern("one byte", 65536))) <= 11 + 4 + 300
    # concatenated frames decode in order
    some = twin_frames[5::37]
    assert fa.spill.lz4_frames_decode(b"".join(f for _, f in some)) == b"".join(d for d, _ in some)
    assert fa.lz4_frame(b"abc" * 1000) == _twin(fa, b"abc" * 1000)


def test_host_twin_against_liblz4(fa, twin_frames):
    if Z.liblz4() is None:
        pytest.skip("no liblz4 on this machine: the frames were checked with the tests' own decoder only")
    for data, frame in twin_frames:
        assert Z.liblz4_decode(frame, len(data)) == data
    some = twin_frames[3::29]
    joined = b"".join(d for d, _ in some)
    assert Z.liblz4_decode(b"".join(f for _, f in some), len(joined)) == joined


def test_host_twin_capacity(fa):
    L = fa.lib()
    data = Z.pattern("period 16", 70000)
    a = np.frombuffer(data, dtype=np.uint8)
    need = len(_twin(fa, data))
    n = C.c_size_t()
    out = np.full(need, 0xEE, dtype=np.uint8)
    assert L.fa_lz4_frame(a.ctypes.data, len(data), out.ctypes.data, need - 1, C.byref(n)) == ERR_CAPACITY and n.value == need
    assert (out == 0xEE).all()
    assert L.fa_lz4_frame(a.ctypes.data, len(data), None, 0, C.byref(n)) == ERR_CAPACITY and n.value == need
    assert L.fa_lz4_frame(a.ctypes.data, len(data), out.ctypes.data, need, C.byref(n)) == 0 and n.value == need
    assert Z.decode_one(out.tobytes()) == data


def test_header_bytes(fa):
    empty = _twin(fa, b"")
    assert empty == bytes([0x04, 0x22, 0x4D, 0x18, 0x60, 0x40, 0x82, 0, 0, 0, 0]) == Z.HEADER + Z.ENDMARK
    assert fa.spill.lz4_frames_decode(empty) == b"" and fa.spill.lz4_frames_decode(b"") == b""
    assert (fa.spill._xxh32(bytes([0x60, 0x40])) >> 8) & 0xFF == 0x82
    # xxHash32's published test values: the empty input, and one of each loop of the function
    assert fa.spill._xxh32(b"") == 0x02CC5D05 and fa.spill._xxh32(b"a") == 0x550D7456 and fa.spill._xxh32(b"abc") == 0x32D153FF
    assert fa.spill._xxh32(b"Nobody inspects the spammish repetition") == 0xE2293B2F


def test_header_against_liblz4(fa):
    if Z.liblz4() is None:
        pytest.skip("no liblz4 on this machine: the header was compared with the bytes the format states only")
    assert Z.liblz4_frame(b"", block_size_id=4, independent=True) == _twin(fa, b"")


def test_spill_decodes_liblz4_frames(fa):
    if Z.liblz4() is None:
        pytest.skip("no liblz4 on this machine: nothing to write the foreign frames with")
    dec = fa.spill.lz4_frames_decode
    datas = [Z.pattern("period 16", 300000), Z.mixed_inputs()[1], Z.pattern("random", 70000), b"", Z.pattern("period 3", 5 << 20)]
    frames = []
    for bsid in (4, 5, 6, 7):
        for d in datas:
            f = Z.liblz4_frame(d, block_size_id=bsid, independent=True)
            assert dec(f) == d
            frames.append((d, f))
    assert dec(b"".join(f for _, f in frames)) == b"".join(d for d, _ in frames)
    big = datas[0]
    with pytest.raises(ValueError, match="linked blocks"):
        dec(Z.liblz4_frame(big, block_size_id=0, independent=False))  # liblz4's defaults
    with pytest.raises(ValueError, match="content checksum"):
        dec(Z.liblz4_frame(big, independent=True, content_checksum=True))
    good = Z.liblz4_frame(big, independent=True)
    with pytest.raises(ValueError, match="header checksum"):
        dec(good[:6] + bytes([good[6] ^ 1]) + good[7:])
    for cut in (3, 6, 9, len(good) // 2, len(good) - 4, len(good) - 1):
        with pytest.raises(ValueError, match="truncated|no frame magic"):
            dec(good[:cut])
    with pytest.raises(ValueError, match="skippable"):
        dec(struct.pack("<II", 0x184D2A50, 4) + b"abcd" + good)
    # read_native takes LZ4 input by its magic
    rows = np.zeros(3, dtype=fa.FLOW_ROW_DTYPE)
    rows["time_received"] = 19000 * 86400 + np.arange(3)
    part = fa.flow_rows_to_native(rows)
    blocks = fa.spill.read_native(Z.liblz4_frame(part, independent=True) + fa.lz4_frame(part))
    assert len(blocks) == 2 and all((b["TimeReceived"] == rows["time_received"]).all() for b in blocks)


def test_spill_refuses_what_the_library_does_not_write(fa):
    """(the same refusals without liblz4: frames made by hand from the host twin's)"""
    dec = fa.spill.lz4_frames_decode
    data = Z.pattern("period 16", 70000)
    good = _twin(fa, data)
    assert dec(good) == data

    def with_flg(flg, extra=b""):
        hc = (fa.spill._xxh32(bytes([flg, 0x40]) + extra) >> 8) & 0xFF
        return good[:4] + bytes([flg, 0x40]) + extra + bytes([hc]) + good[7:]

    for flg, extra, text in ((0x40, b"", "linked blocks"), (0x70, b"", "block checksums"), (0x68, bytes(8), "content size"),
                             (0x64, b"", "content checksum"), (0x61, bytes(4), "dictionary id")):
        with pytest.raises(ValueError, match=text):
            dec(with_flg(flg, extra))
    with pytest.raises(ValueError, match="header checksum"):
        dec(good[:6] + b"\x83" + good[7:])
    for cut in (2, 5, 8, 40, len(good) - 4, len(good) - 2):
        with pytest.raises(ValueError, match="truncated|no frame magic"):
            dec(good[:cut])
    with pytest.raises(ValueError, match="no frame magic"):
        dec(good + b"\x01")
    with pytest.raises(ValueError, match="skippable"):
        dec(struct.pack("<II", 0x184D2A5F, 0) + good)
    # a block that points in front of itself is refused, not resolved against the block before it
    two = _twin(fa, Z.pattern("period 65536", 131072))
    (d, blocks), = Z.walk_frames(two)
    assert len(blocks) == 2 and d == Z.pattern("period 65536", 131072)
    bad = Z.HEADER + struct.pack("<I", 10) + bytes([0x10, 0x41, 0x05, 0x00, 0x50, 1, 2, 3]) + bytes([4, 5]) + Z.ENDMARK
    with pytest.raises(ValueError, match="offset 5"):
        dec(bad)


# ---- the helpers the kernel shares with the host -------------------------------------------------------------------------------------
def _host_program():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_lz4")
    src = os.path.join(ROOT, "tests", "host_lz4.hip")
    deps = [src, os.path.join(ROOT, "flow-pipeline_amd", "csrc", "lz4.cuh")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", exe, src])
    return exe, out


def _run(mode, payload, n):
    exe, out = _host_program()
    fin, fout = os.path.join(out, "host_lz4_%s.in" % mode), os.path.join(out, "host_lz4_%s.out" % mode)
    args = [exe, mode, fout]
    if payload is not None:
        with open(fin, "wb") as f:
            f.write(payload)
        args = [exe, mode, fin, fout]
    res = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.startswith("OK %d" % n), res.stdout + res.stderr
    return open(fout, "rb").read()


def _length_bytes(x):
    """the bytes behind a length nibble: none below 15, else (x - 15) // 255 bytes of 255 and one of (x - 15) % 255"""
    return b"" if x < 15 else b"\xff" * ((x - 15) // 255) + bytes([(x - 15) % 255])


LENGTH_EDGES = (14, 15, 16, 269, 270, 271, 524, 525)


def test_emit_helpers_over_length_edges():
    lits = (0, 1) + LENGTH_EDGES + (65535,)
    matches = (0, 4, 5, 18, 19, 20) + tuple(m + 4 for m in LENGTH_EDGES) + LENGTH_EDGES + (65535,)
    cases = [(lit, m, off) for lit in lits for m in matches for off in (1, 255, 256, 65535)]
    got = _run("emit", b"".join(struct.pack("<III", *c) for c in cases), len(cases))
    p = 0
    for lit, m, off in cases:
        n, = struct.unpack_from("<I", got, p)
        seq = got[p + 4:p + 4 + n]
        p += 4 + n
        want = bytes([(min(lit, 15) << 4) | (min(m - 4, 15) if m else 0)]) + _length_bytes(lit) + bytes((7 * i + 3) & 255 for i in range(lit))
        if m:
            want += struct.pack("<H", off) + _length_bytes(m - 4)
        assert seq == want, (lit, m, off)
    assert p == len(got)
    # the statement itself, at the edges: 14 has no length byte, 15 one of 0, 269 one of 254, 270 two (255, 0), 525 three (255, 255, 0)
    assert [_length_bytes(x) for x in (14, 15, 269, 270, 524, 525)] == [b"", b"\x00", b"\xfe", b"\xff\x00", b"\xff\xfe", b"\xff\xff\x00"]


def test_end_rules_and_header():
    sizes = list(range(0, 40)) + [63, 64, 65, 65535, 65536]
    got = np.frombuffer(_run("rules", struct.pack("<%dI" % len(sizes), *sizes), len(sizes)), dtype="<u4").reshape(-1, 2)
    for n, (starts, end) in zip(sizes, got.tolist()):
        # a block under 13 bytes is all literals; otherwise positions 0 .. n - 12 may start a match and a match ends at n - 5 at most
        assert (starts, end) == ((0, 0) if n < 13 else (n - 12 + 1, n - 5)), n
    assert _run("header", None, 1) == Z.HEADER
