"""CPU tests of loading flows_raw parts back (include/flowagg.h "ABI 8, addition: loading flows_raw parts"): the ABI surface; the
host twin fa_lz4_decode against spill.lz4_frames_decode on valid and refused inputs; the size-to-rows rule; and the stand-alone
program tests/host_lz4_decode.hip - the per-sequence step function the decode kernel runs and the twin over it - built plain and
with the host's AddressSanitizer + UBSan, over (a) frames of fa_lz4_frame and liblz4, (b) blocks the tests assemble themselves,
(c) the malformed list and 20 000 seeded mutations.  Expected bytes never come from the code under test.  No GPU needed."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import lz4_cases as Z
import raw_load_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOAD_FUNCS = ["fa_lz4_decode", "fa_lz4_decode_device", "fa_raw_columns_device", "fa_raw_load", "fa_raw_load_stats", "fa_raw_load_reset"]
ERR_ARG, ERR_CAPACITY, ERR_FRAMING = -1, -6, -7
GOLDEN = os.path.join(ROOT, "tests", "golden", "lz4_foreign_frames.npz")


def golden_frames():
    g = np.load(GOLDEN)
    cut = lambda a, o: [a[int(o[i]):int(o[i + 1])].tobytes() for i in range(len(o) - 1)]
    return list(zip([str(n) for n in g["names"]], cut(g["inputs"], g["input_off"]), cut(g["frames"], g["frame_off"])))


def test_abi_surface(fa):
    if not os.path.exists(fa.LIB_PATH):
        fa.build()
    L = C.CDLL(fa.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "flowagg.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    bound = fa.lib()
    for f in LOAD_FUNCS:
        assert hasattr(L, f), "libflowagg.so does not export %s" % f
        assert re.search(r"\bint\s+%s\s*\(" % f, code), "flowagg.h does not declare %s" % f
        assert f in fa.EXPORTS
        assert getattr(bound, f).argtypes, "%s has no argtypes" % f
    vp, sz, szp = C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)
    assert list(bound.fa_lz4_decode.argtypes) == list(bound.fa_lz4_frame.argtypes) == [vp, sz, vp, sz, szp]
    assert list(bound.fa_raw_load.argtypes) == [vp, vp, sz]
    # no new ABI version, and the pinned sizes stay put
    assert bound.fa_abi_version() == 8 and C.sizeof(fa.Config) == 64 and C.sizeof(fa.Stats) == 312 and C.sizeof(fa.RawLz4Stats) == 72
    assert C.sizeof(fa.RawLoadStats) == 96 and fa.LZ4_SPAN_DTYPE.itemsize == 16
    assert "ABI 8, addition: loading flows_raw parts" in hdr
    m = re.search(r"typedef struct \{([^}]*)\} fa_raw_load_stats_t;", code)
    assert re.findall(r"\b(\w+)\s*[,;]", m.group(1)) == [n for n, _ in fa.RawLoadStats._fields_]
    m = re.search(r"typedef struct \{([^}]*)\} fa_lz4_span;", code)
    assert re.findall(r"\b(\w+)\s*[,;]", m.group(1)) == list(fa.LZ4_SPAN_DTYPE.names)
    for name in ("lz4_decode_device", "raw_columns", "raw_load", "raw_load_stats", "raw_load_reset"):
        assert callable(getattr(fa.FlowAgg, name))
    assert callable(fa.lz4_decode)
    # null arguments (no ctx: nothing touches a device)
    n = C.c_size_t()
    assert bound.fa_lz4_decode(None, 5, None, 0, C.byref(n)) == ERR_ARG and bound.fa_lz4_decode(None, 0, None, 0, None) == ERR_ARG
    assert bound.fa_raw_load(None, None, 0) == ERR_ARG and bound.fa_raw_load_stats(None, None) == ERR_ARG and bound.fa_raw_load_reset(None) == ERR_ARG
    assert bound.fa_lz4_decode_device(None, None, 0, None, None, 0, None) == ERR_ARG and bound.fa_raw_columns_device(None, None, 0, None, None) == ERR_ARG


def _decode(fa, data):
    """fa_lz4_decode -> (rc, bytes): the size first, then into a guarded buffer of exactly that size"""
    L = fa.lib()
    a = np.frombuffer(data, dtype=np.uint8)
    n = C.c_size_t(12345)
    rc = L.fa_lz4_decode(a.ctypes.data if len(data) else None, len(data), None, 0, C.byref(n))
    if rc not in (0, ERR_CAPACITY):
        return rc, None
    need = n.value
    if rc == 0:
        assert need == 0
        return 0, b""
    out = np.full(need + 16, 0xEE, dtype=np.uint8)
    if need > 1:  # one byte short: the size again, nothing written
        assert L.fa_lz4_decode(a.ctypes.data, len(data), out.ctypes.data, need - 1, C.byref(n)) == ERR_CAPACITY and n.value == need and (out == 0xEE).all()
    assert L.fa_lz4_decode(a.ctypes.data, len(data), out.ctypes.data, need, C.byref(n)) == 0 and n.value == need
    assert (out[need:] == 0xEE).all(), "bytes are written behind the decoded ones"
    return 0, out[:need].tobytes()


def test_twin_against_spill_on_valid_frames(fa):
    dec = fa.spill.lz4_frames_decode
    inputs = [Z.pattern(p, n) for p in Z.PATTERNS for n in Z.EDGE_SIZES] + list(Z.mixed_inputs()[::5])
    frames = [fa.lz4_frame(d) for d in inputs]
    for d, f in zip(inputs, frames):
        assert _decode(fa, f) == (0, d) and dec(f) == d
    some = list(zip(inputs, frames))[3::17]
    assert _decode(fa, b"".join(f for _, f in some)) == (0, b"".join(d for d, _ in some))
    assert _decode(fa, b"") == (0, b"") and fa.lz4_decode(b"") == b"" and fa.lz4_decode(frames[20]) == inputs[20]
    for name, d, f in golden_frames():  # frames another encoder wrote
        assert _decode(fa, f) == (0, d) and dec(f) == d, name
    for name, f, want in R.assembled():
        if want is not None:
            assert b"".join(Z.decode_block(b) for b in R.blocks_of(f)) == want, name  # each is first checked with the tests' decoder
            assert _decode(fa, f) == (0, want) and dec(f) == want, name
        else:
            with pytest.raises(AssertionError):
                Z.decode_block(R.blocks_of(f)[0])
            assert _decode(fa, f)[0] == ERR_FRAMING, name
            with pytest.raises(ValueError):
                dec(f)


def test_twin_refuses_what_spill_refuses(fa):
    dec = fa.spill.lz4_frames_decode
    stricter = ("a non-last block of 65535 bytes", "a last sequence that carries a match")  # (the twin's additions to that reader's list)
    cases = R.malformed(fa.spill._xxh32)
    assert len(cases) >= 20
    for name, data, text in cases:
        assert _decode(fa, data)[0] == ERR_FRAMING, name
        with pytest.raises(fa.FlowAggError):
            fa.lz4_decode(data)
        if name not in stricter:
            with pytest.raises(ValueError):
                dec(data)
    # frames of larger block size ids are read while their blocks hold at most 65536 bytes
    if Z.liblz4() is not None:
        d = Z.pattern("period 16", 70000)
        assert _decode(fa, Z.liblz4_frame(d[:60000], block_size_id=5))[1] == d[:60000]
        assert _decode(fa, Z.liblz4_frame(d, block_size_id=5))[0] == ERR_FRAMING  # one block of 70000 input bytes


NAMED_ROWS = (0, 1, 127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21)


def _rows_program(sizes):
    """tests/host_raw_rows.hip - raw_rows_from_bytes, the function raw_header_check_kernel runs - over `sizes` -> [(fits, rows)]"""
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_raw_rows")
    src = os.path.join(ROOT, "tests", "host_raw_rows.hip")
    deps = [src] + [os.path.join(ROOT, "flow-pipeline_amd", "csrc", f) for f in ("raw.cuh", "align16.cuh")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", exe, src])
    fin, fout = os.path.join(out, "host_raw_rows.in"), os.path.join(out, "host_raw_rows.out")
    np.asarray(sizes, dtype="<u8").tofile(fin)
    res = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.startswith("OK %d" % len(sizes)), res.stdout + res.stderr
    return [tuple(int(x) for x in r) for r in np.fromfile(fout, dtype="<u8").reshape(-1, 2)]


def test_size_to_rows_rule(fa):
    """bytes = 110 rows + 284 + len(varuint(rows)) is strictly increasing: the named rows' sizes give their rows back, the sizes
    1 .. 109 bytes to either side of each - no part has them - are refused; so is every size below the empty part's, and every
    size up to 40 rows is what a table of the tests' own sizes says."""
    L = fa.lib()
    sizes, want = [], []
    for rows in NAMED_ROWS:
        size = R.part_bytes(rows)
        assert size == L.fa_raw_part_bytes(rows) == 110 * rows + 284 + len(R.varuint(rows))
        assert R.part_bytes(rows + 1) - size in (110, 111) and (rows == 0 or size - R.part_bytes(rows - 1) in (110, 111))
        sizes.append(size)
        want.append((1, rows))
        for k in range(1, 110):
            sizes += [size + k, size - k]
            want += [(0, 0), (0, 0)]
    assert {len(R.varuint(r)) for r in NAMED_ROWS} == {1, 2, 3, 4}  # every header length below 2^28 rows, each edge from both sides
    table = {R.part_bytes(r): r for r in range(41)}
    for size in range(0, R.part_bytes(40) + 1):
        sizes.append(size)
        want.append((1, table[size]) if size in table else (0, 0))
    for rows in ((1 << 28) - 1, 1 << 28, (1 << 31), (1 << 35) + 12345):  # 4-to-5-byte headers and beyond
        sizes += [R.part_bytes(rows), R.part_bytes(rows) + 1]
        want += [(1, rows), (0, 0)]
    got = _rows_program(sizes)
    bad = [(s, g, w) for s, g, w in zip(sizes, got, want) if g != w]
    assert not bad, bad[:10]
    rows = R.random_rows(5, 129)
    part = R.native_part(rows)
    assert len(part) == R.part_bytes(129)
    got, = fa.spill.read_native(part)  # the tests' encoder writes what the offline reader reads
    assert (got["TimeFlowStart"] == rows["TimeFlowStart"]).all() and (got["SrcAddr"] == rows["SrcAddr"]).all() and (got["Packets"] == rows["Packets"]).all()


# ---- the stand-alone program: plain, and under the host's sanitizers ---------------------------------------------------------------
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-g"]


def _program(sanitize):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_lz4_decode" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "host_lz4_decode.hip")
    deps = [src] + [os.path.join(ROOT, "flow-pipeline_amd", "csrc", f) for f in ("lz4.cuh", "lz4_decode.cuh", "align16.cuh")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1" if sanitize else "-O2", "-std=c++17"] + (SANITIZE if sanitize else []) + ["-o", exe, src])
    return exe, out


def _records(items):
    """[(frames, expected bytes or None)] -> the program's input"""
    return b"".join(struct.pack("<II", len(f), 0xFFFFFFFF if d is None else len(d)) + f + (d or b"") for f, d in items)


def _run(sanitize, mode, name, payload, extra=()):
    exe, out = _program(sanitize)
    fin = os.path.join(out, "host_lz4_decode_%s%s.in" % (name, "_san" if sanitize else ""))
    with open(fin, "wb") as f:
        f.write(payload)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")  # (the process loads the HIP runtime, which keeps its allocations)
    res = subprocess.run([exe, mode, fin] + list(extra), capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0 and res.stdout.startswith("OK "), res.stdout + res.stderr[-4000:]
    return [int(x) for x in re.findall(r"\d+", res.stdout)]


@pytest.fixture(scope="module")
def valid_items(fa):
    """(a) frames from fa_lz4_frame and, where the machine has it, liblz4 (the golden ones everywhere); (b) the assembled blocks"""
    inputs = [Z.pattern(p, n) for p in Z.PATTERNS for n in Z.EDGE_SIZES] + list(Z.mixed_inputs())
    items = [(fa.lz4_frame(d), d) for d in inputs]
    if Z.liblz4() is not None:
        items += [(Z.liblz4_frame(d), d) for d in inputs]
    items += [(f, d) for _, d, f in golden_frames()]
    items += [(f, d) for _, f, d in R.assembled()]
    return items


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_program_valid_and_malformed(fa, valid_items, sanitize):
    n, refused = _run(sanitize, "cases", "valid", _records(valid_items))
    assert n == len(valid_items) and refused == sum(1 for _, d in valid_items if d is None) == len(R.MATCHES)
    bad = [(f, None) for _, f, _ in R.malformed(fa.spill._xxh32)]
    assert _run(sanitize, "cases", "malformed", _records(bad)) == [len(bad), len(bad)]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_program_mutations(fa, sanitize):
    seeds = [fa.lz4_frame(Z.pattern(p, n)) for p, n in (("period 3", 700), ("period 16", 65549), ("random", 300), ("period 64", 4000))]
    seeds += [fa.lz4_frame(d) for d in Z.mixed_inputs() if len(d) < 3000][:8]
    seeds += [f for _, f, d in R.assembled()[::9] if d is not None]
    n, refused = _run(sanitize, "mutate", "mutate", _records([(f, b"") for f in seeds]), ["20261021", "20000"])
    assert n == 20000 and 2000 < refused < 20000  # both outcomes occur in numbers


def test_golden_file_is_what_its_script_makes():
    items = golden_frames()
    assert len(items) >= 10 and os.path.getsize(GOLDEN) < 256 << 10 and max(len(d) for _, d, _ in items) == 131077
    for name, d, f in items:
        assert Z.decode_one(f) == d, name  # the tests' own decoder
    if Z.liblz4() is not None:
        for name, d, f in items:
            assert Z.liblz4_frame(d) == f, name
