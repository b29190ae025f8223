"""CPU test of the ingest path's adaptive feedback (flow-pipeline_amd/csrc/ingest_feedback.h: which tuple format, which kernel
variant, which sink for (SrcAddr,DstPort,Proto) and how many passes of agg8_kernel the next launches get) and of the plain-value
functions behind a launch's plan and the launch guard (launch_plan.h), run on the host by tests/host_ingest_feedback.hip.

Three kinds of check.  The differential one is made inside the program: the value against the rules as they stood before they
became one - the old format_feedback and the old inline conditions, transcribed over a struct of the old members - over generated
sequences of looks; one difference is a failure.  The scenarios below assert values that follow from the rules themselves, and
the plan and guard tables assert decisions per input, the ones tests/test_launch_variants_gpu.py pins on a card among them.
The program is built twice, the second time with the host's address and undefined-behaviour sanitizers, and both binaries are
run directly.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 1 << 20  # records (or folded tuples) a verdict on the wide key set wants
HALF = 4096 // 2  # half of agg8_kernel's LDS table (AGG8_SLOTS / 2)
WAGG_MAX_NWG = 1536


def _exe(sanitize):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_ingest_feedback" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "host_ingest_feedback.hip")
    csrc = os.path.join(ROOT, "flow-pipeline_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("ingest_feedback.h", "launch_plan.h", "sinks.cuh")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        flags = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-fsanitize=address,undefined"] if sanitize else []
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1" if sanitize else "-O2", "-g", "-std=c++17"] + flags + ["-o", exe, src])
    return exe


def _run(mode, lines=()):
    """the program's answer lines in that mode - the same from the plain and from the sanitized build (no report)"""
    outs = []
    for sanitize in (False, True):
        res = subprocess.run([_exe(sanitize), mode], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        outs.append(res.stdout.splitlines())
    assert outs[0] == outs[1]
    return outs[0]


def _pairs(line):
    w = line.split()
    return w[0], {k: int(v) for k, v in zip(w[1::2], w[2::2])}


def knobs(wide_mode=0, t8_mode=0, seq_mode=0, forced=0, plog2=8, wide_table=1, log_allowed=1):
    return "knobs %d %d %d %d %d %d %d" % (wide_mode, t8_mode, seq_mode, forced, plog2, wide_table, log_allowed)


def look(ok=0, misfit8=0, retried=0, wused=0, wfold_n=0, agg_launches=0, agg_groups=0, batches=0):
    return "look %d %d %d %d %d %d %d %d" % (ok, misfit8, retried, wused, wfold_n, agg_launches, agg_groups, batches)


def looks(*lines):
    """the state and the answers behind every line"""
    got = _run("looks", lines)
    assert len(got) == len(lines)
    return [_pairs(g)[1] for g in got]


# ---- differential ----------------------------------------------------------------------------------------------------------
def test_the_value_equals_the_rules_it_replaced_over_generated_looks():
    head, reached = (_pairs(l) for l in _run("diff"))
    assert head[0] == "diff" and head[1]["mismatches"] == 0
    assert head[1]["combos"] == 4 * 3 * 3 * 5 * 2 * 2 and head[1]["looks"] == head[1]["combos"] * 3 * 400
    # the sequences were not idle: every rule fired in both directions and every restart was met
    assert reached[0] == "reached" and len(reached[1]) == 12 and all(v > 100 for v in reached[1].values()), reached


# ---- scenarios -------------------------------------------------------------------------------------------------------------
def test_no_wide_verdict_below_2_20_records():
    # every record opens a row: one record short of 2^20 nothing is decided, at 2^20 it is the log
    (short,) = looks(knobs(), look(ok=M - 1, wused=M - 1))[1:]
    assert (short["defer"], short["log_mode"], short["seen_ok_w"], short["seen_wused"]) == (0, 0, 0, 0)
    (full,) = looks(knobs(), look(ok=M, wused=M))[1:]
    assert (full["defer"], full["log_mode"], full["seen_ok_w"], full["seen_wused"]) == (1, 1, M, M)
    # ... counted from the last verdict, not from the last look: 2^20 - 1 more records in two looks, then the one that completes them
    a, b, c, d = looks(knobs(log_allowed=0), look(ok=M), look(ok=M + 5, wused=5), look(ok=2 * M - 1, wused=M - 1), look(ok=2 * M, wused=M))[1:]
    assert (a["scatter"], a["seen_ok_w"]) == (0, M)  # (no record opened a row: atomics)
    assert (b["scatter"], b["seen_ok_w"], c["scatter"], c["seen_ok_w"], c["seen_wused"]) == (0, M, 0, M, 0)
    assert (d["scatter"], d["seen_ok_w"], d["seen_wused"], d["wide_scatter_sink"]) == (1, 2 * M, M, 1)


@pytest.mark.parametrize("start", [0, 1])
def test_scatter_or_atomics_thresholds(start):
    """dn = 5 * 2^18 = 10 * 2^17 records behind the last verdict.  dw * 5 == dn and dw * 10 == dn change nothing, whichever sink
    was chosen before; one more row than a fifth is the scatter sink, one fewer than a tenth is atomics."""
    dn = 5 << 18
    first = look(ok=M, wused=M // 4 if start else 0)  # a quarter opened rows: scatter sink; none did: atomics
    for dw, want in ((dn // 5, start), (dn // 5 + 1, 1), (dn // 10, start), (dn // 10 - 1, 0), (dn // 5 - 1, start), (dn // 10 + 1, start)):
        w0 = M // 4 if start else 0
        a, b = looks(knobs(log_allowed=0), first, look(ok=M + dn, wused=w0 + dw))[1:]
        assert a["scatter"] == start and b["seen_ok_w"] == M + dn
        assert (b["scatter"], b["wide_scatter_sink"]) == (want, want), (dw, want)


@pytest.mark.parametrize("wide_mode", [0, 1, 2, 3])
@pytest.mark.parametrize("log_allowed", [0, 1])
def test_log_mode_is_entered_above_half_only_when_allowed_and_adaptive(wide_mode, log_allowed):
    at_half, above = (looks(knobs(wide_mode=wide_mode, log_allowed=log_allowed), look(ok=M, wused=w))[1] for w in (M // 2, M // 2 + 1))
    assert at_half["defer"] == 0
    assert above["defer"] == int(wide_mode == 0 and log_allowed == 1)
    assert above["seen_ok_w"] == M and above["scatter"] == 1
    # the answer: FA_WIDE=log is the log whatever the counters say, the adaptive ctx by its verdict, the other two never
    assert above["log_mode"] == int(wide_mode == 3 or above["defer"]) and at_half["log_mode"] == int(wide_mode == 3)
    assert above["left_log_mode"] == int(wide_mode == 0 and not above["defer"])
    assert above["wide_scatter_sink"] == int(wide_mode in (0, 2, 3))


def test_log_mode_is_left_when_fewer_than_half_of_2_20_folded_tuples_open_rows():
    enter = look(ok=M, wused=M)
    for wfold, dw, left, verdict in ((M, M // 2 - 1, 1, 1), (M, M // 2, 0, 1), (M - 1, 0, 0, 0), (M, M, 0, 1)):
        a, b = looks(knobs(), enter, look(ok=3 * M, wused=M + dw, wfold_n=wfold))[1:]
        assert (a["defer"], a["seen_wfold"], a["left_log_mode"]) == (1, 0, 0)
        assert (b["defer"], b["log_mode"], b["left_log_mode"]) == (1 - left, 1 - left, left), (wfold, dw)
        assert (b["seen_wfold"], b["seen_wused"]) == ((wfold, M + dw) if verdict else (0, M))
        assert b["seen_ok_w"] == (3 * M if left else M)  # (the next verdict on the sinks counts from here)
    # a table rebuilt (wused starts over) or a fold counter that restarts: no verdict from that look, whatever it shows
    a, b = looks(knobs(), look(ok=M, wused=M, wfold_n=7), look(ok=3 * M, wused=5, wfold_n=7 + M))[1:]
    assert (b["defer"], b["seen_wused"], b["seen_wfold"]) == (1, 5, 7 + M)
    a, b = looks(knobs(), look(ok=M, wused=M, wfold_n=7), look(ok=3 * M, wused=M, wfold_n=3))[1:]
    assert (b["defer"], b["seen_wused"], b["seen_wfold"]) == (1, M, 3)


def test_wide_tuples_and_learnt_order_for_exactly_64_batches():
    # misfits: 1/16 of the look's records changes nothing, one more gives wide tuples for the batches 10 .. 73
    same, wide = (looks(knobs(), look(ok=1600, misfit8=m, batches=10))[1] for m in (100, 101))
    assert (same["t8_wide_until"], same["compact_tuples"]) == (0, 1)
    assert (wide["t8_wide_until"], wide["compact_tuples"]) == (74, 0)
    at = looks(knobs(), look(ok=1600, misfit8=101, batches=10), "at 73", "at 74")
    assert [a["compact_tuples"] for a in at[1:]] == [0, 0, 1]
    assert [a["learnt_order"] for a in at[1:]] == [0, 0, 0]
    # second-chance records: half of the look's records changes nothing, one more gives the learnt-order variant for 64 batches
    same, seq = (looks(knobs(), look(ok=1000, retried=r, batches=7))[1] for r in (500, 501))
    assert (same["seq_until"], same["learnt_order"]) == (0, 0)
    assert (seq["seq_until"], seq["learnt_order"]) == (71, 1)
    at = looks(knobs(), look(ok=1000, retried=501, batches=7), "at 70", "at 71")
    assert [a["learnt_order"] for a in at[1:]] == [1, 1, 0]
    assert [a["compact_tuples"] for a in at[1:]] == [1, 1, 1]
    # a look without new records decides nothing; retried starting over counts from zero
    a, b = looks(knobs(), look(ok=1000, retried=400, batches=1), look(ok=1000, retried=900, misfit8=900, batches=2))[1:]
    assert (b["seq_until"], b["t8_wide_until"]) == (0, 0)
    a, b = looks(knobs(), look(ok=1000, retried=400, batches=1), look(ok=2000, retried=300, batches=2))[1:]
    assert (b["seq_until"], b["seen_retried"]) == (0, 300)
    # the knobs override the counters
    for t8_mode, seq_mode, want in ((1, 2, (1, 0)), (2, 1, (0, 1))):
        a = looks(knobs(t8_mode=t8_mode, seq_mode=seq_mode), look(ok=1000, misfit8=1000, retried=1000, batches=3))[1]
        assert (a["compact_tuples"], a["learnt_order"]) == want


@pytest.mark.parametrize("plog2", [8, 4])
def test_pass_count_rises_a_doubling_per_look_and_falls_only_when_clearly_below(plog2):
    def groups(per_part):
        return per_part << plog2
    k = knobs(plog2=plog2)
    # up: at half the LDS table per partition one pass is enough, one group more wants two; far above: one doubling per look
    at, above = (looks(k, look(agg_launches=1, agg_groups=groups(p)))[1] for p in (HALF, HALF + 1))
    assert (at["agg_passes"], at["passes"], above["agg_passes"], above["passes"]) == (1, 1, 2, 2)
    big = groups(8 * HALF)
    up = looks(k, *(look(agg_launches=i, agg_groups=i * big) for i in (1, 2, 3, 4)))[1:]
    assert [u["passes"] for u in up] == [2, 4, 8, 8]
    # down from 8: want = 4 for both, but only per_part * 3 < 8 * HALF moves (a step at a time)
    edge = (8 * HALF - 1) // 3  # the largest per_part with per_part * 3 < 8 * HALF
    assert 2 * HALF < edge < 4 * HALF
    for per_part, want in ((edge, 4), (edge + 1, 8)):
        down = looks(k, *(look(agg_launches=i, agg_groups=i * big) for i in (1, 2, 3)), look(agg_launches=4, agg_groups=3 * big + groups(per_part)))[-1]
        assert down["passes"] == want, per_part
    # ... and a tiny launch behind 8 passes: 8 -> 4 -> 2 -> 1
    tiny = looks(k, *(look(agg_launches=i, agg_groups=i * big) for i in (1, 2, 3)), *(look(agg_launches=3 + i, agg_groups=3 * big + i) for i in (1, 2, 3, 4)))[-4:]
    assert [t["passes"] for t in tiny] == [4, 2, 1, 1]
    # no launch since the last look: nothing moves; counters that start over are measured from zero
    a, b = looks(k, look(agg_launches=1, agg_groups=big), look(agg_launches=1, agg_groups=2 * big))[1:]
    assert (b["agg_passes"], b["seen_agg_groups"]) == (2, big)
    a, b = looks(k, look(agg_launches=5, agg_groups=5 * big), look(agg_launches=1, agg_groups=big))[1:]
    assert (a["agg_passes"], b["agg_passes"], b["seen_agg_launches"], b["seen_agg_groups"]) == (2, 4, 1, big)
    # a forced value is what the launch gets, whatever the rule has learnt
    for forced in (1, 2, 4, 8):
        f = looks(knobs(plog2=plog2, forced=forced), look(agg_launches=1, agg_groups=big))[1]
        assert (f["agg_passes"], f["passes"]) == (2, forced)


def test_the_probe_is_wanted_once_by_an_adaptive_ctx_outside_log_mode():
    for wide_mode in (0, 1, 2, 3):
        fresh, marked = looks(knobs(wide_mode=wide_mode), "probed")
        assert (fresh["wants_probe"], marked["wants_probe"], marked["probed"]) == (int(wide_mode == 0), 0, 1)
    in_log = looks(knobs(), look(ok=M, wused=M))[1]
    assert (in_log["defer"], in_log["probed"], in_log["wants_probe"]) == (1, 0, 0)


# ---- the plan ----------------------------------------------------------------------------------------------------------------
SINK = {None: 0, "direct": 1, "scatter": 2}
TUPLE = {None: 0, "8": 1, "16": 2}
SEQ = {None: 0, "1": 1, "0": 2}
WIDE = {None: 0, "atomic": 1, "scatter": 2, "log": 3}


def plan(ks, sink=None, n=4096, plog2=8, grid=512, cms_atomic=0, cms_ok=1, wtab=None, cand=0, wide=None, fmt=None, seq=None, batches=0, t8_until=0,
         seq_until=0, scatter=1, defer=0):
    wtab = int((ks & 56) != 0) if wtab is None else wtab  # (a ctx with a wide key set has the wide table)
    return "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (ks, SINK[sink], n, plog2, grid, cms_atomic, cms_ok, wtab, cand, WIDE[wide], TUPLE[fmt], SEQ[seq],
                                                                  batches, t8_until, seq_until, scatter, defer)


def plans(cases):
    """cases: (input line, expected decisions) - compared key by key, every other decision of the plan must be 0"""
    got = [_pairs(l)[1] for l in _run("plan", [c[0] for c in cases])]
    assert len(got) == len(cases)
    for (line, want), g in zip(cases, got):
        variant = g.pop("variant")
        assert variant == want.pop("variant", variant)
        assert g == dict(dict.fromkeys(g, 0), **want), (line, g, want)


def test_plan_of_every_pinned_setting():
    cases = []
    # every variant through both sinks and tuple formats (FA_SINK x FA_TUPLE x mask, launches of 4096 records)
    for ks in (1, 2, 3, 4, 5, 6, 7, 9, 63):
        for sink in ("scatter", "direct"):
            for fmt in ("8", "16"):
                wave = int(sink == "scatter" and ks & 1)
                want = dict(variant=ks if ks != 63 else 255, wave_tiles=wave, t8=int(wave and fmt == "8"), cms_segments=int(wave and (ks & 6) != 0),
                            wide_segments=int(wave and (ks & 8) != 0))
                cases.append((plan(ks, sink=sink, fmt=fmt), want))
    # the sketch variants in the candidates mode: the aggregation on the side stream
    for ks in (3, 5, 7):
        cases.append((plan(ks, sink="scatter", cand=1), dict(wave_tiles=1, t8=1, cms_segments=1, side=1)))
    # the learnt-order variant forced, both tuple formats
    for fmt in ("8", "16"):
        cases.append((plan(1, sink="scatter", fmt=fmt, seq="1"), dict(wave_tiles=1, t8=int(fmt == "8"), seq_variant=1)))
    # the wide sink modes
    cases.append((plan(9, sink="scatter", wide="atomic"), dict(wave_tiles=1, t8=1)))
    cases.append((plan(9, sink="scatter", wide="scatter"), dict(wave_tiles=1, t8=1, wide_segments=1)))
    cases.append((plan(9, sink="scatter", wide="log"), dict(wave_tiles=1, t8=1, wide_segments=1, wlog=1)))
    # no FA_SINK: the threshold between the sinks
    cases.append((plan(1, n=32767), dict()))
    cases.append((plan(1, n=32768), dict(wave_tiles=1, t8=1)))
    plans(cases)


def test_plan_direct_path_grid_limit_and_the_feedback():
    big = 1 << 20
    cases = [
        # n < 2^15 without FA_SINK: the direct path whatever else is set - no tuples, so nothing that needs them
        (plan(63, n=32767, cand=1, wide="log", fmt="8", seq="1"), dict(variant=255)),
        (plan(1, n=32767, fmt="8", seq="1"), dict()),
        (plan(9, sink="direct", n=big, wide="log"), dict()),
        # more workgroups than wagg_kernel takes segments of: the wide updates keep the atomic path - and there is no log chunk
        (plan(9, n=big, grid=WAGG_MAX_NWG, wide="log"), dict(wave_tiles=1, t8=1, wide_segments=1, wlog=1)),
        (plan(9, n=big, grid=WAGG_MAX_NWG + 1, wide="log"), dict(wave_tiles=1, t8=1)),
        (plan(9, n=big, grid=WAGG_MAX_NWG + 1, wide="scatter"), dict(wave_tiles=1, t8=1)),
        (plan(9, n=big, grid=WAGG_MAX_NWG + 1, defer=1), dict(wave_tiles=1, t8=1)),
        # the adaptive wide key set: by the feedback's verdicts
        (plan(9, n=big, scatter=1), dict(wave_tiles=1, t8=1, wide_segments=1)),
        (plan(9, n=big, scatter=0), dict(wave_tiles=1, t8=1)),
        (plan(9, n=big, scatter=1, defer=1), dict(wave_tiles=1, t8=1, wide_segments=1, wlog=1)),
        (plan(9, n=big, scatter=0, defer=1), dict(wave_tiles=1, t8=1)),  # (nothing to keep without segments)
        (plan(9, n=big, wide="atomic", scatter=1, defer=1), dict(wave_tiles=1, t8=1)),
        (plan(9, n=big, wide="scatter", scatter=0, defer=1), dict(wave_tiles=1, t8=1, wide_segments=1)),
        (plan(9, n=big, wtab=0, wide="log"), dict(wave_tiles=1, t8=1)),
        (plan(17, n=big, wide="log"), dict(variant=255, wave_tiles=1, t8=1)),  # (a wide table without the (SrcAddr,DstPort,Proto) key set)
        # compact tuples: 256 partitions only, and not before the batch the feedback names
        (plan(1, n=big, plog2=7), dict(wave_tiles=1)),
        (plan(1, n=big, plog2=7, fmt="8"), dict(wave_tiles=1)),
        (plan(1, n=big, batches=73, t8_until=74), dict(wave_tiles=1)),
        (plan(1, n=big, batches=74, t8_until=74), dict(wave_tiles=1, t8=1)),
        (plan(1, n=big, batches=73, t8_until=74, fmt="8"), dict(wave_tiles=1, t8=1)),
        (plan(1, n=big, batches=74, t8_until=74, fmt="16"), dict(wave_tiles=1)),
        # the learnt-order kernel: flows_5m alone, before the batch the feedback names
        (plan(1, n=big, batches=70, seq_until=71), dict(wave_tiles=1, t8=1, seq_variant=1)),
        (plan(1, n=big, batches=71, seq_until=71), dict(wave_tiles=1, t8=1)),
        (plan(1, n=big, batches=70, seq_until=71, seq="0"), dict(wave_tiles=1, t8=1)),
        (plan(3, n=big, batches=70, seq_until=71), dict(wave_tiles=1, t8=1, cms_segments=1)),
        (plan(9, n=big, seq="1"), dict(wave_tiles=1, t8=1, wide_segments=1)),
        (plan(1, n=1000, seq="1"), dict()),
        # sketch tuples: not with FA_CMS=atomic, not with a geometry the scatter sink does not fit; the side stream: candidates mode only
        (plan(7, n=big), dict(wave_tiles=1, t8=1, cms_segments=1)),
        (plan(7, n=big, cms_atomic=1, cand=1), dict(wave_tiles=1, t8=1)),
        (plan(7, n=big, cms_ok=0, cand=1), dict(wave_tiles=1, t8=1)),
        (plan(6, n=big, cand=1), dict()),  # (no flows_5m rollup: no wave tiles)
    ]
    plans(cases)


# ---- the launch guard ----------------------------------------------------------------------------------------------------------
GO, WAIT, SETTLE = 0, 1, 2


def guard(spill_count=0, wspill_count=0, used=0, wused=0, used_base=0, wused_base=0, slots=1 << 20, wslots=1 << 20, spill_cap=(1 << 25) + (1 << 21),
          wspill_cap=1 << 25, wtab=1, per_record=4, in_flight=0, n=0):
    return "%d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (spill_count, wspill_count, used, wused, used_base, wused_base, slots, wslots, spill_cap, wspill_cap, wtab,
                                                         per_record, in_flight, n)


def test_guard_verdicts_at_their_boundaries():
    cap, wcap = (1 << 25) + (1 << 21), 1 << 25
    room = cap - M  # records whose updates fit the spill buffer beside the 2^20 of slack
    wroom = (wcap - M) // 4
    assert (wcap - M) % 4 == 0
    cases = [
        (guard(), GO),
        # parked updates could outgrow the spill buffer: pot + 2^20 equal to its capacity goes, one record more waits
        (guard(wtab=0, n=room), GO),
        (guard(wtab=0, n=room + 1), WAIT),
        (guard(wtab=0, in_flight=room - 10, n=10), GO),
        (guard(wtab=0, in_flight=room - 10, n=11), WAIT),
        (guard(wtab=0, in_flight=room + 1, n=0), WAIT),
        # ... the wide table's, at wide_per_record updates per record - only with a wide table
        (guard(n=wroom), GO),
        (guard(n=wroom + 1), WAIT),
        (guard(in_flight=wroom, n=1), WAIT),
        (guard(wtab=0, n=wroom + 1), GO),
        (guard(per_record=1, n=wroom + 1), GO),
        (guard(per_record=1, n=wcap - M), GO),
        (guard(per_record=1, n=wcap - M + 1), WAIT),
        # load: exactly half goes, one row above is settled - counted with the rows of earlier counter epochs
        (guard(used=1 << 19), GO),
        (guard(used=(1 << 19) + 1), SETTLE),
        (guard(used=1 << 18, used_base=1 << 18), GO),
        (guard(used=1 << 18, used_base=(1 << 18) + 1), SETTLE),
        (guard(slots=1 << 21, used=(1 << 19) + 1), GO),
        (guard(wused=1 << 19), GO),
        (guard(wused=(1 << 19) + 1), SETTLE),
        (guard(wused=1, wused_base=1 << 19), SETTLE),
        (guard(wused=(1 << 19) + 1, wtab=0), GO),
        (guard(wslots=1 << 30, wused=1 << 29), GO),
        (guard(wslots=1 << 30, wused=(1 << 29) + 1), SETTLE),
        # anything parked is settled; settling comes before waiting
        (guard(spill_count=1), SETTLE),
        (guard(wspill_count=1), SETTLE),
        (guard(spill_count=1, n=room + 1), SETTLE),
        (guard(used=(1 << 19) + 1, n=room + 1), SETTLE),
    ]
    got = [_pairs(l)[1]["guard"] for l in _run("guard", [c[0] for c in cases])]
    assert got == [c[1] for c in cases], [(c, g) for c, g in zip(cases, got) if c[1] != g]
