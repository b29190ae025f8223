"""CPU tests of the flows_raw part format (include/flowagg.h "flows_raw parts built on the device"): the host encoder
fa_flow_rows_to_native, fa_raw_part_bytes, and spill.read_native / spill.native_from_rows.  One part is one ClickHouse Native
block without BlockInfo: varuint(16) varuint(rows), then per column varuint(len(name)) name varuint(len(type)) type and the
little-endian values.  The golden bytes below are written out by hand from that rule."""
import ctypes as C
import os

import numpy as np
import pytest

ERR_ARG, ERR_CAPACITY = -1, -6

# two rows of one Date (19987 = 0x4e13); the second TimeReceived is 2^32 + ...: the DateTime narrowing keeps the low 32 bits
GOLDEN_ROWS = [
    dict(time_received=1726899900, time_flow_start=1726899890, sampling_rate=1000, bytes=1499, packets=99, sequence_num=7,
         src_as=65001, dst_as=65002, etype=0x86DD, proto=6, src_port=443, dst_port=50000,
         sampler_address=bytes(range(16)), src_addr=bytes.fromhex("20010db8000000000000000000000001"), dst_addr=bytes([192, 168, 1, 1]) + bytes(12)),
    dict(time_received=(1 << 32) + 1726899901, time_flow_start=1726899901, sampling_rate=1, bytes=2**64 - 1, packets=2**63, sequence_num=0xFFFFFFFF,
         src_as=1, dst_as=2, etype=0x800, proto=17, src_port=65536, dst_port=0,
         sampler_address=bytes(16), src_addr=b"\xff" * 16, dst_addr=bytes([10, 0, 0, 1]) + bytes(12)),
]
GOLDEN = b"".join([
    b"\x10", b"\x02",
    b"\x04Date\x04Date", bytes.fromhex("134e" "134e"),
    b"\x0cTimeReceived\x08DateTime", bytes.fromhex("bc66ee66" "bd66ee66"),
    b"\x0dTimeFlowStart\x08DateTime", bytes.fromhex("b266ee66" "bd66ee66"),
    b"\x0bSequenceNum\x06UInt32", bytes.fromhex("07000000" "ffffffff"),
    b"\x0cSamplingRate\x06UInt64", bytes.fromhex("e803000000000000" "0100000000000000"),
    b"\x0eSamplerAddress\x0fFixedString(16)", bytes.fromhex("000102030405060708090a0b0c0d0e0f" + "00" * 16),
    b"\x07SrcAddr\x0fFixedString(16)", bytes.fromhex("20010db8000000000000000000000001" + "ff" * 16),
    b"\x07DstAddr\x0fFixedString(16)", bytes.fromhex("c0a80101" + "00" * 12 + "0a000001" + "00" * 12),
    b"\x05SrcAS\x06UInt32", bytes.fromhex("e9fd0000" "01000000"),
    b"\x05DstAS\x06UInt32", bytes.fromhex("eafd0000" "02000000"),
    b"\x05EType\x06UInt32", bytes.fromhex("dd860000" "00080000"),
    b"\x05Proto\x06UInt32", bytes.fromhex("06000000" "11000000"),
    b"\x07SrcPort\x06UInt32", bytes.fromhex("bb010000" "00000100"),
    b"\x07DstPort\x06UInt32", bytes.fromhex("50c30000" "00000000"),
    b"\x05Bytes\x06UInt64", bytes.fromhex("db05000000000000" "ffffffffffffffff"),
    b"\x07Packets\x06UInt64", bytes.fromhex("6300000000000000" "0000000000000080"),
])
HEADER_BYTES = len(GOLDEN) - 2 * 110  # the 2 block-header bytes of a part below 128 rows + the 16 column headers


def _rows(fa, dicts):
    rows = np.zeros(len(dicts), dtype=fa.FLOW_ROW_DTYPE)
    for i, d in enumerate(dicts):
        for k, v in d.items():
            rows[k][i] = np.frombuffer(v, dtype=np.uint8) if isinstance(v, bytes) else v
    return rows


def _lib(fa):
    if not os.path.exists(fa.LIB_PATH):
        fa.build()
    return fa.lib()


def test_two_row_golden(fa):
    _lib(fa)
    rows = _rows(fa, GOLDEN_ROWS)
    assert len(GOLDEN) == 2 + 220 + sum(2 + len(n) + len(fa.spill.NATIVE_TYPES[n][0]) for n in fa.spill.COLUMNS)
    assert fa.flow_rows_to_native(rows) == GOLDEN
    assert fa.spill.native_from_rows(rows) == GOLDEN
    (blk,) = fa.spill.read_native(GOLDEN)
    assert list(blk) == fa.spill.COLUMNS
    assert blk["Date"].tolist() == [19987, 19987] and blk["TimeReceived"].tolist() == [1726899900, 1726899901]
    assert blk["Packets"].tolist() == [99, 2**63] and bytes(blk["DstAddr"][1]) == bytes([10, 0, 0, 1]) + bytes(12)
    # the capacity protocol of the RowBinary twin
    L, n = fa.lib(), C.c_size_t()
    out = np.zeros(len(GOLDEN), dtype=np.uint8)
    assert L.fa_flow_rows_to_native(rows.ctypes.data, 2, out.ctypes.data, len(GOLDEN) - 1, C.byref(n)) == ERR_CAPACITY and n.value == len(GOLDEN)
    assert L.fa_flow_rows_to_native(rows.ctypes.data, 2, None, 0, C.byref(n)) == ERR_CAPACITY and n.value == len(GOLDEN)
    assert L.fa_flow_rows_to_native(rows.ctypes.data, 2, out.ctypes.data, len(GOLDEN), C.byref(n)) == 0 and out.tobytes() == GOLDEN


def test_part_bytes_at_the_varuint_steps(fa):
    L = _lib(fa)
    for rows, vl in ((0, 1), (1, 1), (127, 1), (128, 2), (16383, 2), (16384, 3)):
        assert L.fa_raw_part_bytes(rows) == HEADER_BYTES - 1 + vl + 110 * rows, rows


def test_encoder_refusals(fa):
    L, n = _lib(fa), C.c_size_t()
    out = np.zeros(4096, dtype=np.uint8)

    def rc(rows):
        return L.fa_flow_rows_to_native(rows.ctypes.data, len(rows), out.ctypes.data, out.size, C.byref(n))

    good = _rows(fa, GOLDEN_ROWS)
    assert rc(good) == 0
    assert rc(good[::-1].copy()) == ERR_ARG  # unsorted
    mixed = good.copy()
    mixed["time_received"][1] = 19988 * 86400  # the next Date
    assert rc(mixed) == ERR_ARG
    bad = good.copy()
    bad["status"][1] = 1
    assert rc(bad) == ERR_ARG
    same = good.copy()
    same["time_received"][1] = same["time_received"][0]  # equal t32 is ascending
    assert rc(same) == 0
    with pytest.raises(fa.FlowAggError):
        fa.flow_rows_to_native(bad)


def test_read_native_round_trip(fa, po):
    n = 5000
    gp = po.gen_params(mode=po.GEN_ASPAIRS, framed=1, seed=5, n_total=n, t0=19000 * 86400 - 300, span_secs=600, per_sec=40)
    orows, status = po.decode_batch(*po.gen_records(gp, 0, n), 1)
    assert int(status.sum()) == 0
    rows = np.zeros(n, dtype=fa.FLOW_ROW_DTYPE)
    for f in orows.dtype.names:
        if f != "_pad":
            rows[f] = orows[f]
    rows = rows[np.random.default_rng(3).permutation(n)]
    data = fa.spill.native_from_rows(rows)
    blocks = fa.spill.read_native(data)
    assert len(blocks) == 2 and sum(len(b["Date"]) for b in blocks) == n
    t32 = (rows["time_received"] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    srt = rows[np.argsort(t32, kind="stable")]
    at = byte_at = 0
    for b, date in zip(blocks, (18999, 19000)):
        m = len(b["Date"])
        r = srt[at:at + m]
        at += m
        part = data[byte_at:byte_at + fa.lib().fa_raw_part_bytes(m)]
        byte_at += len(part)
        assert fa.flow_rows_to_native(r) == part  # the C encoder, block by block
        assert (b["Date"] == date).all() and np.array_equal(b["TimeReceived"], r["time_received"].astype(np.uint32))
        assert (np.diff(b["TimeReceived"].astype(np.int64)) >= 0).all()
        assert np.array_equal(b["TimeFlowStart"], r["time_flow_start"].astype(np.uint32))
        for col, f in fa.spill._ROW_FIELDS.items():
            assert np.array_equal(b[col], r[f]), col
    assert at == n and byte_at == len(data)


def test_read_native_rejects_trailing_and_foreign_bytes(fa):
    rn = fa.spill.read_native
    assert rn(b"") == [] and len(rn(GOLDEN + GOLDEN)) == 2
    for bad in (GOLDEN + b"\x00", GOLDEN + GOLDEN[:-1], GOLDEN[:-1], GOLDEN + b"\x10", b"\x0f" + GOLDEN[1:],
                GOLDEN.replace(b"SrcPort", b"SrcPorT"), GOLDEN.replace(b"\x06UInt64", b"\x06UInt32", 1)):
        with pytest.raises(ValueError):
            rn(bad)
