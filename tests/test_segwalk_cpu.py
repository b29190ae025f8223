"""CPU test of the segment geometry the three tuple-aggregation kernels share (flow-pipeline_amd/csrc/segwalk.cuh: which 16-byte
piece of a segment a lane reads at a level, which of its tuples belong to the part, how many levels a count needs), run on the
host by tests/host_segwalk.hip.  The program checks the rule itself - every tuple of a part visited exactly once, nothing
outside it, every piece inside the segment, nothing from the last level on - for front and back parts, one and two tuples per
piece, capq in {2 TPL, 8, 40, 64, 130} and every count; this file checks the program's verdict and compares what it printed -
exactly - with the restatements below, which are the formulas the kernels' three separate fetch functions used to carry.  The
program is built twice, the second time with the host's address and undefined-behaviour sanitizers, and both binaries are run
directly.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPQS = {1: (2, 8, 40, 64, 130), 2: (4, 8, 40, 64, 130)}


def levels_of(back, tpl, c):
    """levels a part of c tuples needs: 64 pieces per level in front, 8 at the back (two-tuple pieces: c tuples span up to
    c // 2 + 1 pieces)"""
    if not back:
        return (c + 63) >> 6 if tpl == 1 else (c + 127) >> 7
    if tpl == 1:
        return (c + 7) >> 3
    return (c // 2 + 1 + 7) >> 3 if c else 0


def piece_of(back, tpl, capq, c, j, lane):
    """(piece, valid mask) of a lane at level j: the wide-tuple fetch (tpl 1) and the compact-tuple fetch (tpl 2) as they stood"""
    per = 8 if back else 64
    first = capq - c if back else 0
    if tpl == 1:
        q = first + per * j + (lane % per if back else lane)
        valid = int(first <= q < first + c)
        return (q if valid else 0), valid
    piece = first // 2 + per * j + (lane % per if back else lane)
    q = piece * 2
    valid = int(first <= q < first + c) | (int(first <= q + 1 < first + c) << 1)
    return (piece if valid else 0), valid


def _run(sanitize):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_segwalk" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "host_segwalk.hip")
    deps = [src, os.path.join(ROOT, "flow-pipeline_amd", "csrc", "segwalk.cuh")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-fsanitize=address,undefined"] if sanitize else []
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1" if sanitize else "-O2", "-g", "-std=c++17"] + flags + ["-o", exe, src])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-500:] + res.stderr[-2000:]
    return [line.split() for line in res.stdout.splitlines()]


@pytest.fixture(scope="module")
def lines():
    plain = _run(False)
    assert _run(True) == plain  # the sanitized build: no report, the same answers
    return plain


def test_every_tuple_of_a_part_is_visited_exactly_once(lines):
    got = {(int(l[1]), int(l[2]), int(l[3])): tuple(int(x) for x in l[4:]) for l in lines if l[0] == "geom"}
    assert sorted(got) == sorted((back, tpl, capq) for back in (0, 1) for tpl in (1, 2) for capq in CAPQS[tpl])
    for (back, tpl, capq), (cases, tuples, fails) in got.items():
        assert fails == 0, (back, tpl, capq)
        assert cases == capq + 1  # every count 0 .. capq, so c = 1, c = capq and every odd `first` of a two-tuple part
        # every count's c tuples once, in each of the segments a load covers
        assert tuples == (8 if back else 1) * capq * (capq + 1) // 2, (back, tpl, capq)


def test_levels_are_the_kernels_rule(lines):
    got = {(int(l[1]), int(l[2]), int(l[3])): int(l[4]) for l in lines if l[0] == "levels"}
    assert len(got) == 4 * 131
    for (back, tpl, c), v in got.items():
        assert v == levels_of(back, tpl, c), (back, tpl, c)
    # what the rule must guarantee: the levels hold the pieces a part can span
    for (back, tpl, c), v in got.items():
        pieces = c // 2 + 1 if back and tpl == 2 and c else -(-c // tpl)  # (an odd `first`: the part's first piece straddles its start)
        assert v * (8 if back else 64) >= pieces and (v == 0) == (c == 0)


def test_pieces_are_bit_for_bit_the_former_fetch_functions(lines):
    n = 0
    for l in lines:
        if l[0] != "piece":
            continue
        back, tpl, capq, c, j, lane, piece, valid = (int(x) for x in l[1:])
        assert (piece, valid) == piece_of(back, tpl, capq, c, j, lane), l
        n += 1
    # every (capq <= 40, count, level below the count's + 3, lane)
    want = sum(64 * (levels_of(back, tpl, c) + 3) for back in (0, 1) for tpl in (1, 2) for capq in CAPQS[tpl] if capq <= 40 for c in range(capq + 1))
    assert n == want
