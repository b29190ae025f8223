"""CPU test of the capacity rule of the keyed tables (flow-pipeline_amd/csrc/table_room.h: the talker and the port tables end
every launch at or below half full, which is why their unbounded probe loops end), run on the host by tests/host_table_room.hip
and compared - exactly - with the restatement below.  The program is built twice, the second time with the host's address and
undefined-behaviour sanitizers, and both binaries are run directly.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LOG2 = 30


def fits(used_ub, m, log2):
    return (used_ub + m) * 2 <= 1 << log2


def grow_to(used, m, log2):
    """the smallest log2 at or above the table's own at which the rule holds; None = full"""
    for nl in range(log2, MAX_LOG2 + 1):
        if fits(used, m, nl):
            return nl
    return None


def chunk_cap(chunk, log2_a, log2_b):
    return min(chunk, max(1 << 16, (1 << min(log2_a, log2_b)) // 4))


def _run(sanitize):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_table_room" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "host_table_room.hip")
    deps = [src, os.path.join(ROOT, "flow-pipeline_amd", "csrc", "table_room.h")]
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


def test_half_full_fits_and_one_more_does_not(lines):
    got = {(int(l[1]), int(l[2]), int(l[3])): int(l[4]) for l in lines if l[0] == "fits"}
    for log2 in range(8, 31):
        half = 1 << (log2 - 1)
        for used in (0, half // 3, half):
            assert got[(used, half - used, log2)] == 1, (used, log2)
            assert got[(used, half - used + 1, log2)] == 0, (used, log2)
    assert len(got) == 23 * 3 * 2
    for (used, m, log2), v in got.items():
        assert v == int(fits(used, m, log2))


def test_grow_to_is_the_smallest_log2_that_fits_and_never_31(lines):
    got = {(int(l[1]), int(l[2]), int(l[3])): l[4] for l in lines if l[0] == "grow"}
    assert len(got) >= 23 * 8
    for (used, m, log2), v in got.items():
        want = grow_to(used, m, log2)
        assert v == ("full" if want is None else str(want)), (used, m, log2)
        if want is not None:
            assert log2 <= want <= MAX_LOG2 and fits(used, m, want) and (want == log2 or not fits(used, m, want - 1))
    for log2 in range(8, 31):  # at half: stays; one more: doubles once, or is full at the limit
        half = 1 << (log2 - 1)
        assert got[(0, half, log2)] == str(log2)
        assert got[(half, 1, log2)] == (str(log2 + 1) if log2 < 30 else "full")
        assert got[(half, 1, 8)] == (str(log2 + 1) if log2 < 30 else "full")  # from the smallest table in one step
    assert got[(1 << 29, 1, 30)] == got[(1 << 29, 1, 8)] == got[(0, (1 << 29) + 1, 16)] == got[(1 << 40, 1 << 40, 8)] == "full"
    assert got[(0, 1 << 29, 8)] == "30"
    assert "31" not in got.values()


def test_chunk_cap(lines):
    got = {(int(l[1]), int(l[2]), int(l[3])): int(l[4]) for l in lines if l[0] == "cap"}
    caps, chunks = (8, 18, 19, 30), (1, 1 << 16, 1 << 20, 1 << 28)
    assert sorted(got) == sorted((ch, a, b) for a in caps for b in caps for ch in chunks)
    for (ch, a, b), v in got.items():
        assert v == chunk_cap(ch, a, b), (ch, a, b)
    # the values the rule was written for: a small table steps by 2^16, 2^19 slots by 2^17, the knob bounds a large one
    assert got[(1 << 20, 8, 8)] == 1 << 16 and got[(1 << 20, 18, 18)] == 1 << 16 and got[(1 << 20, 19, 19)] == 1 << 17
    assert got[(1 << 20, 30, 30)] == 1 << 20 and got[(1 << 28, 30, 30)] == 1 << 28 and got[(1, 30, 8)] == 1
