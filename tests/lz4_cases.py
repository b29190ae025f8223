"""Shared by tests/test_raw_lz4_cpu.py and tests/test_raw_lz4_gpu.py: the inputs, the tests' OWN LZ4 frame walker and block decoder
(nothing here comes from the code under test), and liblz4's frame decoder through ctypes where the machine has it.

The decoder asserts the format's rules instead of tolerating violations: every offset is >= 1 and <= the bytes decoded in THIS
block, the last sequence is literals only, a block that has a match ends with >= 5 literals and no match starts within its last
12 bytes, a stored block's size is its input, a block's input is <= 65536 bytes, the seven header bytes and the EndMark match."""
import ctypes as C
import ctypes.util
import functools

import numpy as np

HEADER = bytes([0x04, 0x22, 0x4D, 0x18, 0x60, 0x40, 0x82])
ENDMARK = bytes(4)
BLOCK = 65536

EDGE_SIZES = (0, 1, 4, 5, 12, 13, 16, 63, 64, 65, 128, 65535, 65536, 65537, 65548, 65549, 131072 + 5)
PATTERNS = ("one byte", "period 2", "period 3", "period 16", "period 64", "period 65536", "random")


def pattern(name, n):
    rng = np.random.default_rng(1234)
    if name == "random":
        return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    period = 1 if name == "one byte" else int(name.split()[1])
    unit = rng.integers(0, 256, size=period, dtype=np.uint8).tobytes()
    return (unit * (n // period + 1))[:n]


RUNS = (0, 1, 14, 15, 16, 254, 255, 256, 269, 270, 271)
DISTANCES = (1, 2, 3, 4, 15, 16, 255, 256, 65534, 65535, 65536, 70000)
COPIES = (4, 5, 18, 19, 20, 273, 274, 275, 70000)
MIXED_MAX = 200_000


@functools.lru_cache(maxsize=None)
def mixed_inputs():
    """200 seeded inputs of at most 200 KB: random runs (lengths from RUNS) and copies (distances from DISTANCES, lengths from
    COPIES; a copy longer than its distance overlaps itself, as an LZ4 match does).  Computed once, immutable."""
    rng = np.random.default_rng(20261020)
    out = []
    for k in range(200):
        target = int(rng.integers(1, MIXED_MAX + 1)) if k % 4 else int(rng.integers(1, 3000))
        b = bytearray()
        while len(b) < target:
            if rng.random() < 0.5 or not b:
                b += rng.integers(0, 256, size=int(rng.choice(RUNS)), dtype=np.uint8).tobytes()
            else:
                d, ln = int(rng.choice(DISTANCES)), int(rng.choice(COPIES))
                if d > len(b):
                    continue
                start = len(b) - d
                if d >= ln:
                    b += b[start:start + ln]
                else:
                    unit = bytes(b[start:])
                    b += (unit * (ln // d + 1))[:ln]
        out.append(bytes(b[:MIXED_MAX]))
    assert max(len(x) for x in out) > 190_000 and min(len(x) for x in out) < 3000
    return tuple(out)


def _length(src, p, nibble):
    v = nibble
    if nibble == 15:
        while True:
            assert p < len(src), "length bytes run past the block"
            v += src[p]
            p += 1
            if src[p - 1] != 255:
                break
    return v, p


def decode_block(src):
    """One compressed block -> its bytes; the block format's rules are asserted."""
    out, p, n = bytearray(), 0, len(src)
    match_starts = []
    while True:
        assert p < n, "the block ends where a token is expected"
        token = src[p]
        lit, p = _length(src, p + 1, token >> 4)
        assert p + lit <= n, "literals run past the block"
        out += src[p:p + lit]
        p += lit
        if p == n:
            assert token & 15 == 0, "the last sequence carries a match length"
            last_literals = lit
            break
        assert p + 2 <= n, "the block ends inside an offset"
        offset = src[p] | (src[p + 1] << 8)
        mlen, p = _length(src, p + 2, token & 15)
        mlen += 4
        assert 1 <= offset <= len(out), "offset %d with %d bytes decoded in this block" % (offset, len(out))
        match_starts.append(len(out))
        start = len(out) - offset
        if offset >= mlen:
            out += out[start:start + mlen]
        else:
            unit = bytes(out[start:])
            out += (unit * (mlen // offset + 1))[:mlen]
    total = len(out)
    assert total <= BLOCK, "a block of %d input bytes" % total
    if match_starts:
        assert last_literals >= 5, "the block ends with %d literals" % last_literals
        assert match_starts[-1] + 12 <= total, "a match starts %d bytes before the block's end" % (total - match_starts[-1])
    return bytes(out)


def walk_frames(data):
    """A concatenation of the library's frames -> [(decoded bytes, [(stored, input bytes) per block])] per frame."""
    data = bytes(data)
    frames, p = [], 0
    while p < len(data):
        assert data[p:p + 7] == HEADER, "frame header %s at byte %d" % (data[p:p + 7].hex(), p)
        p += 7
        parts, blocks = [], []
        while True:
            assert p + 4 <= len(data), "no EndMark"
            word = int.from_bytes(data[p:p + 4], "little")
            p += 4
            if word == 0:
                break
            size = word & 0x7FFFFFFF
            assert 0 < size <= BLOCK and p + size <= len(data), "block size word %#x at byte %d" % (word, p - 4)
            if word >> 31:
                parts.append(data[p:p + size])  # stored: the size is the input's
            else:
                d = decode_block(data[p:p + size])
                assert size < len(d), "a compressed block of %d bytes for %d input bytes is not stored" % (size, len(d))
                parts.append(d)
            blocks.append((bool(word >> 31), len(parts[-1])))
            p += size
        # every block but the last holds exactly 65536 input bytes
        assert all(n == BLOCK for _, n in blocks[:-1]), "block inputs %s" % [n for _, n in blocks]
        frames.append((b"".join(parts), blocks))
    return frames


def decode_one(frame):
    frames = walk_frames(frame)
    assert len(frames) == 1, "%d frames where one is expected" % len(frames)
    return frames[0][0]


# ---- liblz4, where the machine has it ------------------------------------------------------------------------------------------
class _Prefs(C.Structure):  # LZ4F_preferences_t (lz4frame.h, 1.9.x)
    _fields_ = [("blockSizeID", C.c_int), ("blockMode", C.c_int), ("contentChecksumFlag", C.c_int), ("frameType", C.c_int),
                ("contentSize", C.c_ulonglong), ("dictID", C.c_uint), ("blockChecksumFlag", C.c_int),
                ("compressionLevel", C.c_int), ("autoFlush", C.c_uint), ("favorDecSpeed", C.c_uint), ("reserved", C.c_uint * 3)]


@functools.lru_cache(maxsize=None)
def liblz4():
    name = ctypes.util.find_library("lz4")
    if not name:
        return None
    L = C.CDLL(name)
    L.LZ4F_isError.argtypes = [C.c_size_t]
    L.LZ4F_createDecompressionContext.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    L.LZ4F_createDecompressionContext.restype = C.c_size_t
    L.LZ4F_freeDecompressionContext.argtypes = [C.c_void_p]
    L.LZ4F_decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
    L.LZ4F_decompress.restype = C.c_size_t
    L.LZ4F_compressFrameBound.argtypes = [C.c_size_t, C.POINTER(_Prefs)]
    L.LZ4F_compressFrameBound.restype = C.c_size_t
    L.LZ4F_compressFrame.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(_Prefs)]
    L.LZ4F_compressFrame.restype = C.c_size_t
    L.LZ4_compress_default.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.LZ4_compressBound.argtypes = [C.c_int]
    return L


def liblz4_decode(data, expect):
    """LZ4F_decompress over a concatenation of frames -> the decoded bytes (expect: their number, for the buffer)."""
    L = liblz4()
    data = bytes(data)
    ctx = C.c_void_p()
    assert not L.LZ4F_isError(L.LZ4F_createDecompressionContext(C.byref(ctx), 100))
    try:
        src = C.create_string_buffer(data, len(data))
        dst = C.create_string_buffer(expect + 1)
        sp = dp = 0
        while sp < len(data):
            s, d = C.c_size_t(len(data) - sp), C.c_size_t(expect + 1 - dp)
            rc = L.LZ4F_decompress(ctx, C.byref(dst, dp), C.byref(d), C.byref(src, sp), C.byref(s), None)
            assert not L.LZ4F_isError(rc), "LZ4F_decompress refuses the stream at byte %d" % sp
            assert s.value or d.value, "LZ4F_decompress makes no progress at byte %d" % sp
            sp += s.value
            dp += d.value
        assert rc == 0, "LZ4F_decompress expects %d more bytes: the last frame is not complete" % rc
        return dst.raw[:dp]
    finally:
        L.LZ4F_freeDecompressionContext(ctx)


def liblz4_frame(data, block_size_id=4, independent=True, content_checksum=False):
    L = liblz4()
    prefs = _Prefs(blockSizeID=block_size_id, blockMode=1 if independent else 0, contentChecksumFlag=1 if content_checksum else 0)
    cap = L.LZ4F_compressFrameBound(len(data), C.byref(prefs))
    dst = C.create_string_buffer(cap)
    n = L.LZ4F_compressFrame(dst, cap, bytes(data), len(data), C.byref(prefs))
    assert not L.LZ4F_isError(n)
    return dst.raw[:n]
