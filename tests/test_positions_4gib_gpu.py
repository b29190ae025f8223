"""Ingest and decode at the top of the 32-bit offset range: one device batch of 2^32 - 1 bytes.

The C-ABI takes device batches up to the limit of its 32-bit offsets (fa_ingest_device with offsets: len < 2^32; without:
len < 2^32 - 1; fa_decode_device: len < 2^32).  The buffer holds ~26 M GoFlow-shaped records from the device generator (two
calls: records [0, nA) below 2^31 and [nA, n) above it; one oracle run covers both) and hand-built pieces between and behind
them: markers (unique SrcAS / DstAS / Bytes in a timeslot of their own) across 2^31, across the last 16 KiB block boundaries,
in the last 256 bytes and ending exactly at len; descending-field-order records and records with 3-byte tags (the deferred
kernel, at absolute positions near 2^32); a record larger than the LDS tile (the exotic path); and, in one case, malformed records whose LEN field claims up
to 2^20 - 1 bytes, one of them the batch's last record.  Every case compares with the CPU oracle."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from device_columns import fetch_columns

pytestmark = pytest.mark.gpu

TOP = 0xFFFFFFFF          # the largest len of the offsets path
HALF = 1 << 31
SLACK = 64 * 1024         # behind 2^32: an over-read by a regression stays inside the allocation
FS_BLOCK = 16384
MID_BYTES = 2 * 1024 * 1024   # hand-built pieces between the generator's two calls (across 2^31)
TAIL_MIN = 3 * 1024 * 1024    # ... and behind the second call, up to len


def _enc(fa, fields):
    out = bytearray()
    for f, v in fields:
        if isinstance(v, (bytes, bytearray)):
            out += fa.schema.encode_varint((f << 3) | 2) + fa.schema.encode_varint(len(v)) + bytes(v)
        else:
            out += fa.schema.encode_varint(f << 3) + fa.schema.encode_varint(int(v))
    return bytes(out)


class Pieces:
    """Framed records placed at exact positions; the gaps between them are filled with short records (<= 120 bytes: device
    framing settles) padded by an unknown LEN field 200 (above every schema field, placed last)."""

    def __init__(self, fa, t_mark):
        self.fa, self.t = fa, t_mark
        self.recs = []  # (position, framed bytes)
        self.k = 0

    def _padded(self, fields, size):
        base = _enc(self.fa, fields)
        pad = size - 1 - len(base) - 3
        assert 0 <= pad <= 127 - len(base) - 3, (size, len(base))
        rec = self.fa.schema.frame(base + _enc(self.fa, [(200, b"\x00" * pad)]))
        assert len(rec) == size
        return rec

    def filler(self, size):
        self.k += 1
        k = self.k
        return self._padded([(2, self.t + 600 + k % 50), (9, 100 + k % 7), (10, 1), (14, 64512), (15, 64513), (30, 0x800)], size)

    def marker(self, size=50):
        self.k += 1
        k = self.k
        return self._padded([(2, self.t + k % 200), (9, 1_000_003 * (k % 1000 + 1)), (10, 1 + k % 5), (14, 70_000 + k), (15, 80_000 + k),
                             (30, 0x86dd)], size)

    def odd(self):
        """A valid record no LDS tier is sure about (a field of number 5000: a tag of three bytes): the deferred kernel's."""
        self.k += 1
        k = self.k
        return self.fa.schema.frame(_enc(self.fa, [(2, self.t + 11), (9, 5_000 + k), (10, 2), (14, 95_000 + k), (15, 95_001), (30, 0x800),
                                                   (5000, 1 << 50)]))

    def malformed(self, claim, size=None):
        """A frame whose payload ends in a LEN field 100 claiming `claim` bytes of which only a few are there."""
        self.k += 1
        body = _enc(self.fa, [(2, self.t + 7), (14, 90_000 + self.k), (15, 90_001)]) + self.fa.schema.encode_varint((100 << 3) | 2) + \
            self.fa.schema.encode_varint(claim) + b"\xab" * 5
        return self.fa.schema.frame(body)

    def fill(self, lo, hi):
        """Fillers over [lo, hi) exactly (hi - lo == 0 or >= 40)."""
        g = hi - lo
        assert g == 0 or g >= 40, (lo, hi)
        if g == 0:
            return
        parts = -(-g // 120)
        sizes = [g // parts + (1 if i < g % parts else 0) for i in range(parts)]
        p = lo
        for s in sizes:
            self.recs.append((p, self.filler(s)))
            p += s

    def lay(self, lo, hi, fixed):
        """[lo, hi) = the fixed records (position -> bytes, no overlaps) and fillers between them."""
        p = lo
        for pos, rec in sorted(fixed):
            assert pos >= p, (pos, p)
            self.fill(p, pos)
            self.recs.append((pos, rec))
            p = pos + len(rec)
        assert p <= hi
        self.fill(p, hi)

    def region(self, lo, hi):
        """the region's bytes and its records' absolute offsets (without hi)"""
        recs = sorted(r for r in self.recs if lo <= r[0] < hi)
        buf = np.zeros(hi - lo, dtype=np.uint8)
        offs = []
        for pos, rec in recs:
            buf[pos - lo:pos - lo + len(rec)] = np.frombuffer(rec, dtype=np.uint8)
            offs.append(pos)
        return buf, np.array(offs, dtype=np.uint64)


def _host_positions_ok(po):
    """The host position harness (tests/host_positions.hip, CPU only, seconds): the parsers must not wrap before malformed
    records near 2^32 go to the GPU (a parser that walks back to the start of the batch would stall every wave for minutes)."""
    import test_host_parsers
    exe = test_host_parsers.build_host_positions(po)
    res = subprocess.run([exe, "1000"], capture_output=True, text=True, timeout=300)
    if res.returncode != 0 or not res.stdout.strip().endswith("OK"):
        pytest.fail("host position harness failed - not sending wrapping records to the GPU:\n" + res.stdout[-3000:] + res.stderr)


@pytest.fixture(scope="module")
def big(gpu_lib, fa, po):
    import torch
    dev = torch.device("cuda", 0)
    mode, seed, span, per_sec = fa.MOCK_GOFLOW, 71, 900, 50_000
    n_total = 28_000_000  # (records [0, n) of this stream are used, n ~ 26 M: their sizes grow with the index)
    d_buf = torch.zeros(TOP + 1 + SLACK, dtype=torch.uint8, device=dev)
    d_off_a = torch.empty(n_total + 1, dtype=torch.int32, device=dev)
    d_off_b = torch.empty(n_total + 1, dtype=torch.int32, device=dev)
    mp = fa.mock_params(mode=mode, framed=1, seed=seed, n_total=n_total, span_secs=span, per_sec=per_sec)
    with fa.FlowAgg(framed=True) as g:
        def size(i0, k):  # the generator's exact byte count for records [i0, i0 + k), asked with a buffer of 0 bytes
            w = C.c_uint64()
            rc = fa.lib().fa_mock_generate_device(g._h, C.byref(mp), i0, k, d_buf.data_ptr(), 0, d_off_b.data_ptr(), C.byref(w))
            assert rc == -6  # FA_ERR_CAPACITY, with the size
            return w.value

        def fit(i0, room):  # the most records from i0 on whose bytes stay within room - 256 KiB
            k = int(room / (size(i0, 1_000_000) / 1e6))
            for _ in range(20):
                w = size(i0, k)
                if room - (1 << 20) <= w <= room - (1 << 18):
                    return k
                k += int((room - (3 << 18) - w) / 170)
            pytest.fail("no record count fits %d bytes" % room)

        b_start = HALF + MID_BYTES // 2
        n_a = fit(0, HALF - MID_BYTES // 2)
        n_b = fit(n_a, TOP - TAIL_MIN - b_start)
        n = n_a + n_b
        assert n <= n_total
        w_a = g.mock_generate_device(mp, 0, n_a, d_buf.data_ptr(), HALF - MID_BYTES // 2, d_off_a.data_ptr())
        w_b = g.mock_generate_device(mp, n_a, n_b, d_buf.data_ptr() + b_start, TOP - TAIL_MIN - b_start, d_off_b.data_ptr())
    torch.cuda.synchronize()
    assert w_a < HALF - 200_000 and b_start + w_b < TOP - (1 << 20) - 200_000 and n < (1 << 25) - 200_000, (w_a, w_b, n)
    gp = po.gen_params(mode=po.GEN_GOFLOW, framed=1, seed=seed, n_total=n_total, span_secs=span, per_sec=per_sec)
    want = po.bench_rollup_ex(gp, 0, n, 16, want_rows=True)
    assert want["wire_bytes"] == w_a + w_b and want["bad"] == 0
    off_a = d_off_a.cpu().numpy().view(np.uint32)[:n_a].astype(np.uint64)
    off_b = d_off_b.cpu().numpy().view(np.uint32)[:n_b].astype(np.uint64) + b_start
    t_mark = (fa.T0 // 300 + 24) * 300  # two hours behind the bulk's 900 s: a timeslot of the pieces alone
    return dict(d_buf=d_buf, n=n, w_a=w_a, b_start=b_start, b_end=b_start + w_b, off_a=off_a, off_b=off_b,
                rows=want["rows"], t_mark=t_mark, dev=dev)


def _layout(fa, big, len_, mid_exact=False, big_record=True, reversed_records=True, malformed=False, po=None):
    """Writes the hand-built pieces for a batch of len_ bytes into the device buffer.  -> (offsets uint64[N + 1] of the whole
    batch, Pieces, pieces' rollup rows, pieces' bytes/offsets for the oracle)"""
    import torch
    P = Pieces(fa, big["t_mark"])
    # across 2^31: a marker straddling it, or one starting exactly there
    mid_lo, mid_hi = big["w_a"], big["b_start"]
    fixed = [(HALF, P.marker(60))] if mid_exact else [(HALF - 25, P.marker(50))]
    fixed += [(HALF - 4000, P.marker(45)), (HALF + 4000, P.marker(55))]
    P.lay(mid_lo, mid_hi, fixed)
    # behind the bulk, up to len_
    tail_lo = big["b_end"]
    fixed = []
    last_block = (len_ - 1) // FS_BLOCK * FS_BLOCK
    for j in range(0, 4):  # straddling the last block boundaries
        fixed.append((last_block - j * FS_BLOCK - 20, P.marker(48)))
    fixed.append((last_block - 4 * FS_BLOCK - 1, P.marker(52)))  # its length prefix is the last byte of a block
    fixed += [(len_ - 700_000 + 997 * i, P.marker(44 + i)) for i in range(8)]  # in the last MiB
    if reversed_records:  # descending field order (the learnt-order walk, parse_fast) and 3-byte tags (the deferred kernel), near 2^32
        fixed += [(len_ - 680_000 + 100 * i, P.odd()) for i in range(300)]
        rb, ro = po.gen_records(po.gen_params(mode=po.GEN_REVERSED, framed=1, seed=5, n_total=3000, t0=big["t_mark"], span_secs=60, per_sec=50), 0, 3000)
        at = len_ - 1_000_000
        for i in range(3000):
            fixed.append((at + int(ro[i]), bytes(rb[int(ro[i]):int(ro[i + 1])])))
    if big_record:  # larger than the LDS tile: the exotic path
        body = _enc(fa, [(2, big["t_mark"] + 3), (9, 777), (10, 7), (14, 99_999), (15, 99_998), (30, 0x800), (1000, b"\xcd" * 40000)])
        fixed.append((len_ - 600_000, fa.schema.frame(body)))
    if malformed:  # truncated LEN claims in the last MiB; the last is the batch's last record
        for i, claim in enumerate((0xFFFF0, 0xFFFFF, 0x80000, 40_000, 0xFFFF0)):
            fixed.append((len_ - 500_000 + 50_021 * i, P.malformed(claim)))
    # several records starting in the last 256 bytes, the last one ending exactly at len_
    if malformed:
        bad_last = P.malformed(0xFFFF0)
        tail_end = len_ - len(bad_last)
        fixed += [(tail_end - 200 + 50 * i, P.marker(50)) for i in range(4)]
        fixed.append((tail_end, bad_last))
    else:
        fixed += [(len_ - 250 + 50 * i, P.marker(50)) for i in range(5)]
    P.lay(tail_lo, len_, fixed)
    mid_buf, mid_off = P.region(mid_lo, mid_hi)
    tail_buf, tail_off = P.region(tail_lo, len_)
    d = big["d_buf"]
    d[mid_lo:mid_hi].copy_(torch.from_numpy(mid_buf))
    d[tail_lo:len_].copy_(torch.from_numpy(tail_buf))
    torch.cuda.synchronize()
    off = np.concatenate([big["off_a"], mid_off, big["off_b"], tail_off, np.array([len_], dtype=np.uint64)])
    assert (np.diff(off.astype(np.int64)) > 0).all() and off[-1] == len_
    # the pieces alone, for the oracle
    pb = np.concatenate([mid_buf, tail_buf])
    po_off = np.concatenate([mid_off - mid_lo, tail_off - tail_lo + len(mid_buf), np.array([len(pb)], dtype=np.uint64)])
    return off, P, pb, po_off


def _want_rows(po, big, pb, po_off):
    ref = po.Rollup(300)
    bad = ref.ingest(pb, po_off, 1)
    pr = ref.rows()
    assert pr["timeslot"].min() > big["rows"]["timeslot"].max()
    return np.concatenate([big["rows"], pr]), bad


def _d_off(big, off):
    import torch
    return torch.from_numpy(off.astype(np.uint32).view(np.int32)).to(big["dev"])


def test_offsets_path_at_len_2_32_minus_1(gpu_lib, fa, po, big):
    """len = 2^32 - 1: bulk rows == the oracle's, the pieces' timeslot == po.Rollup over them; exact counters; the deferred
    kernel (descending field order) and the exotic path (a record beyond the LDS tile) both ran near 2^32."""
    off, P, pb, po_off = _layout(fa, big, TOP, po=po)
    want, bad = _want_rows(po, big, pb, po_off)
    assert bad == 0
    n = len(off) - 1
    with fa.FlowAgg(framed=True, max_batch_records=n) as agg:
        agg.ingest_device(big["d_buf"].data_ptr(), TOP, _d_off(big, off).data_ptr(), n)
        rows = agg.read_window()
        st = agg.stats()
    assert rows.tobytes() == want.tobytes()
    assert st["records_ok"] == n and st["records_bad"] == 0 and st["bytes_in"] == TOP, st
    assert st["records_retried"] > 0 and st["records_slow"] > 0, st


def test_malformed_records_in_the_last_mib(gpu_lib, fa, po, big):
    """The same batch plus truncated LEN claims (up to 2^20 - 1) in the last MiB, the last of them ending at len: counted bad,
    nothing else changes; fa_decode_device over the top 100 k records == po.decode_batch, status included."""
    _host_positions_ok(po)
    off, P, pb, po_off = _layout(fa, big, TOP, malformed=True, po=po)
    want, bad = _want_rows(po, big, pb, po_off)
    assert bad == 6
    n = len(off) - 1
    d_off = _d_off(big, off)
    with fa.FlowAgg(framed=True, max_batch_records=n) as agg:
        agg.ingest_device(big["d_buf"].data_ptr(), TOP, d_off.data_ptr(), n)
        rows = agg.read_window()
        st = agg.stats()
    assert rows.tobytes() == want.tobytes()
    assert st["records_ok"] == n - 6 and st["records_bad"] == 6 and st["bytes_in"] == TOP, st
    # decode: absolute offsets of the top records, the full len
    k = 100_000
    top = off[n - k:]
    with fa.FlowAgg(framed=True, max_batch_records=k) as agg:
        cols = agg.decode_device(big["d_buf"].data_ptr(), TOP, d_off.data_ptr() + 4 * (n - k), k)
        agg.sync()
        got = fetch_columns(cols, k)
    host = big["d_buf"][int(top[0]):TOP].cpu().numpy()
    wrows, wstatus = po.decode_batch(host, top - top[0], framed=1)
    assert (got["status"] == wstatus).all() and int(wstatus.sum()) == 6
    for name in ("time_received", "time_flow_start", "sampling_rate", "bytes", "packets", "sequence_num", "src_as", "dst_as", "etype",
                 "proto", "src_port", "dst_port", "sampler_address", "src_addr", "dst_addr"):
        assert np.array_equal(got[name], wrows[name]), name


@pytest.mark.parametrize("len_", [TOP - 1, 0xFFFFFF80], ids=["2^32-2", "2^32-128"])
def test_device_framing_at_the_top(gpu_lib, fa, po, big, len_, capfd, monkeypatch):
    """Without offsets (the device cuts the frames): len = 2^32 - 2, and a len in (2^32 - 16384, 2^32) with frames in its last
    256 bytes.  The device kernels settle (no host walk); rows and counters == a ctx fed the same bytes with the offsets, and ==
    the oracle; once more as several launches (small max_batch_records) whose offsets are all high."""
    off, P, pb, po_off = _layout(fa, big, len_, mid_exact=True, big_record=False, reversed_records=False, po=po)
    want, bad = _want_rows(po, big, pb, po_off)
    assert bad == 0 and (off[-8:-1] >= 0xFFFFFF00).sum() >= 2
    n = len(off) - 1
    monkeypatch.setenv("FA_VERBOSE", "1")
    results = []
    for mbr in ((1 << 25) - 1, 4_000_000):
        with fa.FlowAgg(framed=True, max_batch_records=mbr) as agg:
            capfd.readouterr()
            agg.ingest_device(big["d_buf"].data_ptr(), len_, 0, 0)
            agg.sync()
            log = capfd.readouterr().err
            assert "[flowagg framing]" in log and " settled" in log and "NOT settled" not in log, log
            results.append((agg.read_window(), agg.stats()))
    with fa.FlowAgg(framed=True, max_batch_records=n) as agg:
        agg.ingest_device(big["d_buf"].data_ptr(), len_, _d_off(big, off).data_ptr(), n)
        ref_rows, ref_st = agg.read_window(), agg.stats()
    assert ref_rows.tobytes() == want.tobytes()
    for rows, st in results:
        assert rows.tobytes() == ref_rows.tobytes()
        for key in ("records_ok", "records_bad", "bytes_in"):
            assert st[key] == ref_st[key], (key, st, ref_st)
    assert results[1][1]["wave_tile_launches"] > results[0][1]["wave_tile_launches"] and ref_st["records_ok"] == n


def test_refusals_on_the_real_buffer(gpu_lib, fa, big):
    """The offsets path refuses len = 2^32, the offsets-free path len = 2^32 - 1 (FA_ERR_ARG)."""
    import torch
    d_off = torch.zeros(2, dtype=torch.int32, device=big["dev"])
    with fa.FlowAgg(framed=True) as agg:
        with pytest.raises(fa.FlowAggError) as e:
            agg.ingest_device(big["d_buf"].data_ptr(), 1 << 32, d_off.data_ptr(), 1)
        assert e.value.code == -1
    with fa.FlowAgg(framed=True) as agg:
        with pytest.raises(fa.FlowAggError) as e:
            agg.ingest_device(big["d_buf"].data_ptr(), TOP, 0, 0)
        assert e.value.code == -1
