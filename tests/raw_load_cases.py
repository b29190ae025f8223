"""Shared by tests/test_raw_load_cpu.py and tests/test_raw_load_gpu.py: the tests' OWN LZ4 sequence assembler (blocks built from
(literals, offset, match length) lists, their bytes known by construction), the fixed list of malformed frames, and the tests'
own numpy encoder of flows_raw Native parts.  Nothing here comes from the code under test."""
import functools
import struct

import numpy as np

import lz4_cases as Z

OFFSETS = (1, 2, 3, 4, 15, 16, 63, 64, 65, 255, 65535)
MATCHES = (4, 18, 19, 20, 63, 64, 65, 273, 274, 275, 529)
RUNS = (0, 14, 15, 16, 269, 270, 271)
# A block holds at most 65536 bytes and a match at least 4, so an offset of 65535 can never be valid: the case with it must be
# refused.  65524 is the largest offset a block that keeps the end rules (no match within its last 12 bytes) can hold.
LARGEST_VALID_OFFSET = 65524


def length_bytes(x):
    return b"" if x < 15 else b"\xff" * ((x - 15) // 255) + bytes([(x - 15) % 255])


def assemble(seqs, tail):
    """[(literal bytes, offset, match length)], the last sequence's literals -> (the block, what it decodes to).  The decoded
    bytes are built here, byte by byte; offsets are NOT checked (malformed blocks are assembled too: their second value is junk)."""
    blk, out = bytearray(), bytearray()
    for lit, off, mlen in seqs:
        blk += bytes([(min(len(lit), 15) << 4) | min(mlen - 4, 15)]) + length_bytes(len(lit)) + lit
        blk += struct.pack("<H", off) + length_bytes(mlen - 4)
        out += lit
        if 1 <= off <= len(out):
            unit = bytes(out[len(out) - off:])
            out += (unit * (mlen // off + 1))[:mlen]
    blk += bytes([min(len(tail), 15) << 4]) + length_bytes(len(tail)) + tail
    return bytes(blk), bytes(out + tail)


def frame(blocks, header=Z.HEADER, endmark=Z.ENDMARK):
    """[(data, stored)] -> one frame"""
    return header + b"".join(struct.pack("<I", len(d) | (0x80000000 if s else 0)) + d for d, s in blocks) + endmark


def blocks_of(f):
    """one frame of this module -> its blocks' data"""
    out, p = [], 7
    while True:
        word, = struct.unpack_from("<I", f, p)
        p += 4
        if word == 0:
            return out
        out.append(f[p:p + (word & 0x7FFFFFFF)])
        p += word & 0x7FFFFFFF


def _bytes(rng, n):
    return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def assembled():
    """-> ((name, frame, decoded bytes or None = must be refused), ...): every offset x every match length, the literal runs
    cycling; an offset equal to the bytes decoded so far; a block of exactly 65536 bytes.  Valid blocks keep the end rules
    (Z.decode_block asserts them): they end with 12 literals."""
    rng = np.random.default_rng(20261021)
    out, k = [], 0
    # (a run of one byte brings the bytes in: 65524 literals would not fit a block's 65536 input bytes)
    blk, dec = assemble([(_bytes(rng, 1), 1, LARGEST_VALID_OFFSET - 5), (_bytes(rng, 4), LARGEST_VALID_OFFSET, 4)], _bytes(rng, 8))
    assert len(dec) == 65536 and dec[-12:-8] == dec[:4]
    out.append(("offset %d" % LARGEST_VALID_OFFSET, frame([(blk, False)]), dec))
    for off in OFFSETS:
        for mlen in MATCHES:
            run = RUNS[k % len(RUNS)]
            k += 1
            # a first sequence brings `off - run` bytes in (at least 1 when the run is 0), the second carries the run and the offset
            lead = max(off - run, 1 if run == 0 else 0)
            seqs = [(_bytes(rng, lead), 1, 4)] if lead else []
            if off == 65535:  # (a run of one byte brings 65535 - run bytes in: the offset is in reach, the match leaves the block)
                seqs = [(_bytes(rng, 1), 1, off - run - 1)]
            seqs.append((_bytes(rng, run), off, mlen))
            blk, dec = assemble(seqs, _bytes(rng, 12))
            valid = off != 65535
            out.append(("offset %d match %d run %d" % (off, mlen, run), frame([(blk, False)]), dec if valid else None))
    for n in (1, 7, 64, 300):  # the offset reaches back to the block's first byte
        blk, dec = assemble([(_bytes(rng, n), n, 100)], _bytes(rng, 12))
        out.append(("offset = decoded = %d" % n, frame([(blk, False)]), dec))
    blk, dec = assemble([(_bytes(rng, 16), 16, 65536 - 16 - 12)], _bytes(rng, 12))
    assert len(dec) == 65536
    out.append(("exactly 65536", frame([(blk, False)]), dec))
    blk2, dec2 = assemble([(_bytes(rng, 3), 3, 40)], _bytes(rng, 12))
    out.append(("a full block, then a short one", frame([(blk, False), (blk2, False)]), dec + dec2))
    return tuple(out)


def malformed(xxh32):
    """-> [(name, bytes, regex the refusal's text matches)]: the fixed list.  xxh32: a plain xxHash32 (spill._xxh32) for the
    header checksums of the frames whose FLG is changed, so that the FLG bit is the first thing wrong with them."""
    lits = b"abcdefgh"
    tail5 = bytes([0x50]) + b"vwxyz"

    def blk(raw):
        return frame([(raw, False)])

    def with_flg(flg, extra=b""):
        hc = (xxh32(bytes([flg, 0x40]) + extra) >> 8) & 0xFF
        return Z.HEADER[:4] + bytes([flg, 0x40]) + extra + bytes([hc]) + struct.pack("<I", 5 | 0x80000000) + b"hello" + Z.ENDMARK

    good = frame([(b"hello world, hello", True)])
    cases = [
        ("offset 0", blk(bytes([0x40]) + lits[:4] + b"\x00\x00" + tail5), "offset 0"),
        ("offset = decoded + 1", blk(bytes([0x40]) + lits[:4] + b"\x05\x00" + tail5), "offset"),
        ("literals past the input's end", blk(bytes([0xF0, 0x10]) + b"abc"), "literals run past"),
        ("a length chain past the end", blk(bytes([0xF0, 0xFF, 0xFF])), "length chain"),
        ("a match length chain past the end", blk(bytes([0x1F]) + b"a" + b"\x01\x00" + b"\xff\xff"), "length chain"),
        ("a truncated offset", blk(bytes([0x14]) + b"a" + b"\x01"), "truncated offset"),
        ("a match past 65536", blk(assemble([(lits * 2, 16, 65521)], b"vwxyz")[0]), "more than 65536"),
        ("literals past 65536", frame([(assemble([(lits * 2, 16, 65520)], b"v")[0], False)]), "more than 65536"),
        ("a last sequence that carries a match", blk(bytes([0x51]) + b"vwxyz"), "last sequence carries a match"),
        ("a block that ends behind a match", blk(bytes([0x40]) + lits[:4] + b"\x04\x00"), "token is missing"),
        ("a non-last block of 65535 bytes", frame([(bytes(65535), True), (b"0123456789", True)]), "not the last of its frame"),
        ("a size word of 65537", frame([(bytes(65537), True)]), "maximum is 65536"),
        ("a wrong header checksum", good[:6] + b"\x83" + good[7:], "header checksum"),
        ("FLG: linked blocks", with_flg(0x40), "linked blocks"),
        ("FLG: block checksums", with_flg(0x70), "block checksums"),
        ("FLG: a content size", with_flg(0x68, bytes(8)), "content size"),
        ("FLG: a content checksum", with_flg(0x64), "content checksum"),
        ("FLG: a dictionary id", with_flg(0x61, bytes(4)), "dictionary id"),
        ("FLG: the reserved bit", with_flg(0x62), "reserved"),
        ("FLG: version 0", with_flg(0x20), "version"),
        ("a missing EndMark", good[:-4], "no EndMark"),
        ("a truncated block", good[:-9], "truncated block"),
        ("a skippable frame", struct.pack("<II", 0x184D2A50, 4) + b"abcd" + good, "skippable"),
    ]
    return cases


# ---- flows_raw Native parts, the tests' own encoder -----------------------------------------------------------------------------
# (name, ClickHouse type, numpy dtype in the part, fa_columns member, dtype there)
NATIVE_COLUMNS = (
    ("Date", "Date", "<u2", None, None), ("TimeReceived", "DateTime", "<u4", "time_received", "<u8"),
    ("TimeFlowStart", "DateTime", "<u4", "time_flow_start", "<u8"), ("SequenceNum", "UInt32", "<u4", "sequence_num", "<u4"),
    ("SamplingRate", "UInt64", "<u8", "sampling_rate", "<u8"), ("SamplerAddress", "FixedString(16)", "V16", "sampler_address", "V16"),
    ("SrcAddr", "FixedString(16)", "V16", "src_addr", "V16"), ("DstAddr", "FixedString(16)", "V16", "dst_addr", "V16"),
    ("SrcAS", "UInt32", "<u4", "src_as", "<u4"), ("DstAS", "UInt32", "<u4", "dst_as", "<u4"), ("EType", "UInt32", "<u4", "etype", "<u4"),
    ("Proto", "UInt32", "<u4", "proto", "<u4"), ("SrcPort", "UInt32", "<u4", "src_port", "<u4"), ("DstPort", "UInt32", "<u4", "dst_port", "<u4"),
    ("Bytes", "UInt64", "<u8", "bytes", "<u8"), ("Packets", "UInt64", "<u8", "packets", "<u8"),
)


def varuint(v):
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def part_bytes(rows):
    """the size of a part: 110 bytes per row, the 16 column headers and the column count (284), the row count's varuint"""
    return 110 * rows + 284 + len(varuint(rows))


def random_rows(seed, n, t0=19000 * 86400 + 1000, span=3000, keys=None):
    """-> {column name: array}: n seeded rows of one Date, TimeReceived ascending.  keys: draw addresses, ports and the like from
    that many values (so that groups repeat); None: every bit random."""
    rng = np.random.default_rng(seed)
    rows = {}
    tr = np.sort(rng.integers(t0, t0 + span, size=n)).astype("<u4")
    rows["Date"] = (tr // 86400).astype("<u2")
    rows["TimeReceived"] = tr
    rows["TimeFlowStart"] = (tr - rng.integers(0, 900, size=n)).astype("<u4")
    for name, _, dt, _, _ in NATIVE_COLUMNS[3:]:
        if dt == "V16":
            a = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
            if keys:
                a = rng.integers(0, 256, size=(keys, 16), dtype=np.uint8)[rng.integers(0, keys, size=n)]
                a[:, 4:] = np.where((np.arange(n) % 3 == 0)[:, None], 0, a[:, 4:])
            rows[name] = np.ascontiguousarray(a)
        elif name == "EType":
            rows[name] = np.where(np.arange(n) % 3 == 0, 0x800, 0x86DD).astype(dt) if keys else rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(dt)
        elif keys and name in ("SrcPort", "DstPort"):
            rows[name] = rng.integers(0, keys, size=n).astype(dt)
        elif keys and name in ("Bytes", "SamplingRate"):
            rows[name] = rng.integers(1, 1 << 20, size=n).astype(dt)
        else:
            rows[name] = rng.integers(0, np.iinfo(np.dtype(dt)).max, size=n, dtype=np.uint64, endpoint=True).astype(dt)
    return rows


def native_part(rows, names=None, types=None, ncols=16):
    """{column name: array} -> one Native block.  names / types: {index: replacement} for the refusal tests."""
    n = len(rows["TimeReceived"])
    out = bytearray(varuint(ncols) + varuint(n))
    for i, (name, ctype, dt, _, _) in enumerate(NATIVE_COLUMNS[:ncols]):
        nm, ty = (names or {}).get(i, name), (types or {}).get(i, ctype)
        out += varuint(len(nm)) + nm.encode() + varuint(len(ty)) + ty.encode()
        out += np.ascontiguousarray(rows[name]).tobytes()
    return bytes(out)


def concat_rows(parts):
    return {name: np.concatenate([p[name] for p in parts]) for name, *_ in NATIVE_COLUMNS}
