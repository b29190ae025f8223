"""Columnar spill of the decoded projection: `flows_raw`-equivalent Parquet files, and the reader / plain encoder of the
ClickHouse Native blocks the library builds on the device (``read_native``, ``native_from_rows``; numpy only).

The dashboards of the reference scan ``flows_raw`` (``viz-ch.json:74-604``); with the
ClickHouse Kafka-engine table and its materialized views gone, the raw rows
have no home unless the stage writes them somewhere.  ``spill_parquet`` turns the rows
``fa_decode`` returns (the 15 projected columns, ``compose/clickhouse/create.sh:7-27``) into
one Parquet file with the column list and types of ``flows_raw`` (``create.sh:36-62``):

    Date Date, TimeReceived DateTime, TimeFlowStart DateTime, SequenceNum UInt32,
    SamplingRate UInt64, SamplerAddress/SrcAddr/DstAddr FixedString(16), SrcAS, DstAS, EType,
    Proto, SrcPort, DstPort UInt32, Bytes, Packets UInt64

``Date = toDate(TimeReceived)`` (``create.sh:66``) and the UInt64 -> DateTime narrowing of the two
time columns are applied here as ClickHouse applies them in ``flows_raw_view``; malformed records
(status != 0) are dropped (``inserter/inserter.go:125-126``).  ClickHouse loads such a file with
``INSERT INTO flows_raw FORMAT Parquet``; offline checks read it with pyarrow / pandas.
Host-side Python only (pyarrow for the Parquet half): nothing here is on the hot path.
"""
from __future__ import annotations

import numpy as np

COLUMNS = ["Date", "TimeReceived", "TimeFlowStart", "SequenceNum", "SamplingRate", "SamplerAddress", "SrcAddr",
           "DstAddr", "SrcAS", "DstAS", "EType", "Proto", "SrcPort", "DstPort", "Bytes", "Packets"]


def to_arrow(rows: np.ndarray):
    """rows: structured array with the fields of FLOW_ROW_DTYPE (``status`` optional) -> pyarrow.Table."""
    import pyarrow as pa
    if "status" in rows.dtype.names:
        rows = rows[rows["status"] == 0]
    t_recv = (rows["time_received"] & np.uint64(0xFFFFFFFF)).astype(np.uint32)   # DateTime (create.sh:39)
    t_flow = (rows["time_flow_start"] & np.uint64(0xFFFFFFFF)).astype(np.uint32)  # DateTime (create.sh:40)

    def fixed16(col):
        flat = np.ascontiguousarray(rows[col]).reshape(-1)
        return pa.FixedSizeBinaryArray.from_buffers(pa.binary(16), len(rows), [None, pa.py_buffer(flat.tobytes())])

    cols = {
        "Date": pa.array((t_recv // np.uint32(86400)).astype(np.int32), type=pa.date32()),  # toDate, UTC (create.sh:66)
        # DateTime = UInt32 seconds; Parquet has no second-resolution timestamp (pyarrow would widen to ms), and
        # ClickHouse reads a UInt32 Parquet column into a DateTime column as is
        "TimeReceived": pa.array(t_recv, type=pa.uint32()),
        "TimeFlowStart": pa.array(t_flow, type=pa.uint32()),
        "SequenceNum": pa.array(rows["sequence_num"], type=pa.uint32()),
        "SamplingRate": pa.array(rows["sampling_rate"], type=pa.uint64()),
        "SamplerAddress": fixed16("sampler_address"),
        "SrcAddr": fixed16("src_addr"),
        "DstAddr": fixed16("dst_addr"),
        "SrcAS": pa.array(rows["src_as"], type=pa.uint32()),
        "DstAS": pa.array(rows["dst_as"], type=pa.uint32()),
        "EType": pa.array(rows["etype"], type=pa.uint32()),
        "Proto": pa.array(rows["proto"], type=pa.uint32()),
        "SrcPort": pa.array(rows["src_port"], type=pa.uint32()),
        "DstPort": pa.array(rows["dst_port"], type=pa.uint32()),
        "Bytes": pa.array(rows["bytes"], type=pa.uint64()),
        "Packets": pa.array(rows["packets"], type=pa.uint64()),
    }
    return pa.table([cols[c] for c in COLUMNS], names=COLUMNS)


def spill_parquet(rows: np.ndarray, path: str, compression="zstd") -> int:
    """Writes one flows_raw-shaped Parquet file; returns the number of rows written."""
    import pyarrow.parquet as pq
    table = to_arrow(rows)
    pq.write_table(table, path, compression=compression)
    return table.num_rows


# ---- ClickHouse Native blocks of flows_raw (numpy only) ----------------------------------------------------------------------
# One part = one Native block without BlockInfo: varuint(16) varuint(rows), then per column of COLUMNS
# varuint(len(name)) name varuint(len(type)) type and `rows` little-endian values (format restated from the ClickHouse
# documentation; no server was available to load it into).  The library builds such blocks on the device (fa_raw_*); this
# is the reader for offline checks and the plain encoder behind the CPU tests.
NATIVE_TYPES = {"Date": ("Date", "<u2"), "TimeReceived": ("DateTime", "<u4"), "TimeFlowStart": ("DateTime", "<u4"),
                "SequenceNum": ("UInt32", "<u4"), "SamplingRate": ("UInt64", "<u8"), "SamplerAddress": ("FixedString(16)", "u1"),
                "SrcAddr": ("FixedString(16)", "u1"), "DstAddr": ("FixedString(16)", "u1"), "SrcAS": ("UInt32", "<u4"),
                "DstAS": ("UInt32", "<u4"), "EType": ("UInt32", "<u4"), "Proto": ("UInt32", "<u4"), "SrcPort": ("UInt32", "<u4"),
                "DstPort": ("UInt32", "<u4"), "Bytes": ("UInt64", "<u8"), "Packets": ("UInt64", "<u8")}
_ROW_FIELDS = {"SequenceNum": "sequence_num", "SamplingRate": "sampling_rate", "SamplerAddress": "sampler_address", "SrcAddr": "src_addr",
               "DstAddr": "dst_addr", "SrcAS": "src_as", "DstAS": "dst_as", "EType": "etype", "Proto": "proto", "SrcPort": "src_port",
               "DstPort": "dst_port", "Bytes": "bytes", "Packets": "packets"}


def _varuint(v: int) -> bytes:
    out = bytearray()
    while v >= 128:
        out.append((v & 127) | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def _read_varuint(b: np.ndarray, p: int):
    v = shift = 0
    while True:
        if p >= len(b) or shift > 63:
            raise ValueError("truncated or overlong varuint at byte %d" % p)
        x = int(b[p])
        p += 1
        v |= (x & 127) << shift
        shift += 7
        if x < 128:
            return v, p


# ---- LZ4 frames of the parts (pure Python) ---------------------------------------------------------------------------------------
# The library delivers a part as one LZ4 frame (fa_raw_take_lz4; format in include/flowagg.h, restated from the LZ4 frame and
# block format specifications): magic, FLG, BD, header checksum, blocks of a 4-byte size + data, EndMark.  This is the reader
# for offline checks; it reads what the library writes and says clearly what it does not.
LZ4_MAGIC = b"\x04\x22\x4d\x18"
_M32 = 0xFFFFFFFF


def _xxh32(data: bytes, seed: int = 0) -> int:
    """xxHash32 (restated from the xxHash specification)."""
    P1, P2, P3, P4, P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & _M32
    n, p = len(data), 0
    if n >= 16:
        v = [(seed + P1 + P2) & _M32, (seed + P2) & _M32, seed, (seed - P1) & _M32]
        while p + 16 <= n:
            for i in range(4):
                v[i] = rotl((v[i] + int.from_bytes(data[p + 4 * i:p + 4 * i + 4], "little") * P2) & _M32, 13) * P1 & _M32
            p += 16
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & _M32
    else:
        h = (seed + P5) & _M32
    h = (h + n) & _M32
    while p + 4 <= n:
        h = rotl((h + int.from_bytes(data[p:p + 4], "little") * P3) & _M32, 17) * P4 & _M32
        p += 4
    while p < n:
        h = rotl((h + data[p] * P5) & _M32, 11) * P1 & _M32
        p += 1
    h ^= h >> 15
    h = h * P2 & _M32
    h ^= h >> 13
    h = h * P3 & _M32
    return h ^ (h >> 16)


def _lz4_block_decode(src: bytes, limit: int) -> bytes:
    """One LZ4 block, decoded alone (no history in front of it), to at most `limit` bytes."""
    out, p, n = bytearray(), 0, len(src)
    while True:
        if p >= n:
            raise ValueError("LZ4 block: truncated (a sequence's token is missing)")
        token = src[p]
        p += 1
        lit = token >> 4
        if lit == 15:
            while True:
                if p >= n:
                    raise ValueError("LZ4 block: truncated literal length")
                lit += src[p]
                p += 1
                if src[p - 1] != 255:
                    break
        if p + lit > n:
            raise ValueError("LZ4 block: literals run past the block's end")
        out += src[p:p + lit]
        p += lit
        if p == n:  # the last sequence has no match
            break
        if p + 2 > n:
            raise ValueError("LZ4 block: truncated offset")
        offset = src[p] | (src[p + 1] << 8)
        p += 2
        mlen = (token & 15) + 4
        if token & 15 == 15:
            while True:
                if p >= n:
                    raise ValueError("LZ4 block: truncated match length")
                mlen += src[p]
                p += 1
                if src[p - 1] != 255:
                    break
        if offset == 0 or offset > len(out):
            raise ValueError("LZ4 block: offset %d with %d bytes decoded (blocks must decode alone)" % (offset, len(out)))
        if len(out) + mlen > limit:
            raise ValueError("LZ4 block: decodes to more than %d bytes" % limit)
        start = len(out) - offset
        if offset >= mlen:
            out += out[start:start + mlen]
        else:  # an overlapping match repeats its last `offset` bytes
            pattern = bytes(out[start:])
            out += (pattern * (mlen // offset + 1))[:mlen]
    if len(out) > limit:
        raise ValueError("LZ4 block: decodes to more than %d bytes" % limit)
    return bytes(out)


def lz4_frames_decode(data) -> bytes:
    """A concatenation of LZ4 frames as the library writes them -> the decoded bytes of all of them, in order.  The header
    checksum is verified and every block is decoded alone.  ValueError, with a text that names the reason, on anything the
    library does not write: linked blocks, block or content checksums, a content size, a dictionary id, a skippable or legacy
    frame, a block larger than the frame's maximum, a truncated stream."""
    b = bytes(data) if not isinstance(data, bytes) else data
    out, p = [], 0
    while p < len(b):
        magic = b[p:p + 4]
        if len(magic) == 4 and 0x184D2A50 <= int.from_bytes(magic, "little") <= 0x184D2A5F:
            raise ValueError("LZ4 stream: a skippable frame at byte %d (the library writes none)" % p)
        if magic != LZ4_MAGIC:
            raise ValueError("LZ4 stream: no frame magic at byte %d" % p)
        if p + 7 > len(b):
            raise ValueError("LZ4 stream: truncated frame header at byte %d" % p)
        flg, bd, hc = b[p + 4], b[p + 5], b[p + 6]
        if flg >> 6 != 1:
            raise ValueError("LZ4 frame: version %d (01 is the only one)" % (flg >> 6))
        for bit, what in ((0x20, None), (0x10, "block checksums"), (0x08, "a content size"), (0x04, "a content checksum"), (0x01, "a dictionary id")):
            if what is None:
                if not flg & bit:
                    raise ValueError("LZ4 frame: linked blocks (the library writes independent blocks, each decodes alone)")
            elif flg & bit:
                raise ValueError("LZ4 frame: %s (the library writes none)" % what)
        if flg & 0x02 or bd & 0x8F or not 4 <= bd >> 4 <= 7:
            raise ValueError("LZ4 frame: reserved bits set or an invalid block size id (FLG %#04x BD %#04x)" % (flg, bd))
        if (_xxh32(b[p + 4:p + 6]) >> 8) & 0xFF != hc:
            raise ValueError("LZ4 frame: header checksum %#04x does not match FLG / BD" % hc)
        block_max = 1 << (8 + 2 * (bd >> 4))
        p += 7
        while True:
            if p + 4 > len(b):
                raise ValueError("LZ4 stream: truncated (no EndMark)")
            word = int.from_bytes(b[p:p + 4], "little")
            p += 4
            if word == 0:
                break
            size = word & 0x7FFFFFFF
            if size > block_max:
                raise ValueError("LZ4 frame: a block of %d bytes, the frame's maximum is %d" % (size, block_max))
            if p + size > len(b):
                raise ValueError("LZ4 stream: truncated block")
            out.append(b[p:p + size] if word >> 31 else _lz4_block_decode(b[p:p + size], block_max))
            p += size
    return b"".join(out)


def read_native(data) -> list:
    """A concatenation of flows_raw Native blocks -> one {column: array} per block, in order (FixedString(16) columns as
    uint8[rows, 16]).  Anything that is not a whole number of blocks with the 16 columns and types of flows_raw - a trailing
    byte included - raises ValueError.  Input that starts with the LZ4 frame magic is decoded first (lz4_frames_decode)."""
    if bytes(data[:4]) == LZ4_MAGIC:
        data = lz4_frames_decode(data)
    b = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
    blocks, p = [], 0
    while p < len(b):
        ncols, p = _read_varuint(b, p)
        rows, p = _read_varuint(b, p)
        if ncols != len(COLUMNS):
            raise ValueError("a flows_raw block has %d columns, this one %d" % (len(COLUMNS), ncols))
        block = {}
        for want in COLUMNS:
            got = []
            for _ in range(2):
                n, p = _read_varuint(b, p)
                if p + n > len(b):
                    raise ValueError("truncated column header")
                got.append(bytes(b[p:p + n]).decode("ascii", "replace"))
                p += n
            ctype, dt = NATIVE_TYPES[want]
            if got != [want, ctype]:
                raise ValueError("column %s %s where %s %s is expected" % (got[0], got[1], want, ctype))
            width = 16 if dt == "u1" else np.dtype(dt).itemsize
            if p + rows * width > len(b):
                raise ValueError("truncated column %s" % want)
            col = b[p:p + rows * width]
            block[want] = col.reshape(rows, 16).copy() if dt == "u1" else col.copy().view(dt)
            p += rows * width
        blocks.append(block)
    return blocks


def native_from_rows(rows: np.ndarray) -> bytes:
    """Decoded rows (the fields of FLOW_ROW_DTYPE; ``status`` optional) -> flows_raw Native blocks as the library builds them
    for ONE chunk: malformed rows dropped, the rest in stable order of the 32-bit TimeReceived, one block per Date in ascending
    Date, no block without rows."""
    if "status" in rows.dtype.names:
        rows = rows[rows["status"] == 0]
    t32 = (rows["time_received"] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    order = np.argsort(t32, kind="stable")
    rows, t32 = rows[order], t32[order]
    date = t32 // np.uint32(86400)
    cuts = [0] + [int(i) for i in np.nonzero(date[1:] != date[:-1])[0] + 1] + [len(rows)]
    out = bytearray()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi == lo:
            continue
        r = rows[lo:hi]
        out += _varuint(len(COLUMNS)) + _varuint(hi - lo)
        for name in COLUMNS:
            ctype, dt = NATIVE_TYPES[name]
            out += _varuint(len(name)) + name.encode() + _varuint(len(ctype)) + ctype.encode()
            if name == "Date":
                col = date[lo:hi].astype("<u2")
            elif name == "TimeReceived":
                col = t32[lo:hi].astype("<u4")
            elif name == "TimeFlowStart":
                col = (r["time_flow_start"] & np.uint64(0xFFFFFFFF)).astype("<u4")
            else:
                col = np.ascontiguousarray(r[_ROW_FIELDS[name]]).astype(dt, copy=False)
            out += np.ascontiguousarray(col).tobytes()
    return bytes(out)
