"""The reads and closes of a group of contexts (csrc/group_host.inc): which steps a call took, what it returned, and what its
error paths answer.

A characterisation test in the manner of test_read_paths_gpu.py: it was written against the sources BEFORE the group close was
recomposed from shared steps (one gather-and-merge, one emit) and pins what that rewrite must keep.

* WHICH STEPS a call took is the `[flowagg group] ...; ms: <label> <ms> ...` line that FA_VERBOSE=1 prints to stderr: the member
  count, k, the rows out and the ordered labels are exact, the millisecond figures are dropped.
* WHAT it returned is compared byte for byte with ONE ctx that ingested every member's records.
* The verbose clock only reads the time, but every read is still done a second time with FA_VERBOSE unset - on a twin group fed
  the same records - and must return the same bytes.

1, 2 and 3 members on the one GPU, 20 000 generated records each, key_sets = 9, talkers enabled at 2^10 slots.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^\[flowagg group\] (.*); ms:(.*)$")
LABEL = re.compile(r" (.+?) -?\d+\.\d\d(?= |$)")
SENTINEL = 12345  # what *n_out holds before a call that may leave it alone
ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -6, -8
KW = dict(framed=True, key_sets=9)
PER_MEMBER = 20_000
SHARES = ["rows + partition", "exchange buffers", "exchange", "merge"]
MARK = "FA_KEYS_PORT_HIST not enabled"  # a member's last error before a group call (a text no group call produces)
SMALL = "output buffer too small"
NOT_ENABLED = "top talkers are not enabled on this ctx (fa_talkers_enable)"


@functools.lru_cache(maxsize=None)
def parts():
    """60 000 Zipf records over three windows, dealt round robin into three partitions (record i -> partition i % 3): every
    partition holds every window and most of the hot keys.  Built once, read-only."""
    import _pkg
    po = _pkg.load_oracle()
    n = 3 * PER_MEMBER
    gp = po.gen_params(mode=po.GEN_ZIPF, framed=1, seed=3101, n_total=n, zipf_log2_universe=13, span_secs=900)
    buf, off = po.gen_records(gp, 0, n)
    raw = bytes(buf)
    out = []
    for p in range(3):
        recs = [raw[int(off[k]):int(off[k + 1])] for k in range(p, n, 3)]
        o = np.zeros(len(recs) + 1, dtype=np.uint64)
        o[1:] = np.cumsum([len(r) for r in recs])
        b = np.frombuffer(b"".join(recs), dtype=np.uint8)
        b.setflags(write=False)
        o.setflags(write=False)
        out.append((b, o))
    return tuple(out)


def _ctx(fa, records=()):
    agg = fa.FlowAgg(**KW)
    agg.talkers_enable(10)
    for b, o in records:
        agg.ingest(b, o)
    return agg


class _Groups:
    """Two groups fed the same records - `loud` reads with FA_VERBOSE=1 and its lines are kept, `quiet` reads without - and
    `whole`: one ctx that ingested everything.  held[i]: the partitions member i ingests."""

    def __init__(self, fa, capfd, monkeypatch, held):
        self.fa, self.capfd, self.mp = fa, capfd, monkeypatch
        self.ctxs = []
        sides = []
        for _ in range(2):
            members = [_ctx(fa, [parts()[p] for p in ps]) for ps in held]
            self.ctxs += members
            sides.append(members)
        self.whole = _ctx(fa, [parts()[p] for ps in held for p in ps])
        self.ctxs.append(self.whole)
        self.members = sides[0]
        self.loud, self.quiet = fa.FlowGroup(sides[0]), fa.FlowGroup(sides[1])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.loud.close()
        self.quiet.close()
        for x in self.ctxs:
            x.close()

    def read(self, f):
        """-> (what f returned, the [text, [label, ...]] of every [flowagg group] line it printed)"""
        self.mp.setenv("FA_VERBOSE", "1")
        self.capfd.readouterr()
        got = f(self.loud)
        err = self.capfd.readouterr().err
        self.mp.delenv("FA_VERBOSE")
        lines = [[m.group(1), LABEL.findall(m.group(2))] for m in map(LINE.match, err.splitlines()) if m]
        assert _raw(f(self.quiet)) == _raw(got), "the quiet read differs from the verbose one"
        return got, lines


def _raw(x):
    return b"|".join(_raw(y) for y in x) if isinstance(x, tuple) else x.tobytes() if isinstance(x, np.ndarray) else repr(x).encode()


def _sorted_app(rows):
    addr = np.ascontiguousarray(rows["src_addr"])
    hi, lo = addr[:, :8].copy().view(">u8").reshape(-1), addr[:, 8:].copy().view(">u8").reshape(-1)
    return rows[np.lexsort((rows["proto"], rows["dst_port"], lo, hi, rows["timeslot"], rows["date"]))]


def _check_shares(fa, rows, shares, want, n):
    """the shares back to back, share 0 first; a key in exactly one share, the share of its owner; together: the single ctx's rows"""
    assert len(shares) == n and sum(shares) == len(rows) == len(want)
    assert fa.dist.partition_rows_host(rows, fa.ROWS_APP, n).tolist() == np.repeat(np.arange(n), shares).tolist()
    assert _sorted_app(rows).tobytes() == want.tobytes()


# ---- the verbose lines -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_steps_of_every_read(gpu_lib, fa, capfd, monkeypatch, n):
    with _Groups(fa, capfd, monkeypatch, [[p] for p in range(n)]) as t:
        ts = int(t.whole.open_timeslots()[0])
        # merged reads: no line of the group's
        got, lines = t.read(lambda g: g.read_window(fa.ROWS_5M))
        assert got.tobytes() == t.whole.read_window().tobytes() and len(got) > 0 and lines == []
        got, lines = t.read(lambda g: g.read_window(fa.ROWS_APP, ts))
        assert got.tobytes() == t.whole.read_window_app(ts).tobytes() and len(got) > 0 and lines == []
        # partitioned read
        want = t.whole.read_window_app(ts)
        (rows, shares), lines = t.read(lambda g: g.read_window_partitioned(fa.ROWS_APP, ts, cap=1 << 16))
        _check_shares(fa, rows, shares, want, n)
        assert lines == [["partitioned read of kind 1, %d members, %d rows out" % (n, len(want)), SHARES + ["fetch"]]]
        # talkers
        for d, name in ((0, "SrcAddr"), (1, "DstAddr")):
            whole = t.whole.top_talkers(d)
            assert len(whole) > 100
            for k in (10, 0):
                want = whole[:k or len(whole)]
                got, lines = t.read(lambda g: g.top_talkers(d, k, cap=1 << 16))
                assert got.tobytes() == want.tobytes()
                steps = ["rows", "fetch"] if n == 1 else SHARES + ["gather", "merge of the shares", "fetch"]
                assert lines == [["top talkers (%s), %d members, k %d, %d rows out" % (name, n, k, len(want)), steps]], (d, k)
            got, lines = t.read(lambda g: g.read_window(fa.ROWS_TALKERS_SRC + d, 777, 10))  # (the same call by its row kind)
            assert got.tobytes() == whole[:10].tobytes() and [x[1] for x in lines] == [steps]


# ---- every root ----------------------------------------------------------------------------------------------------------------
def test_every_root_returns_the_same_bytes(gpu_lib, fa):
    """merged reads rotate their root over the members: 2n + 1 consecutive reads pass every member at least twice"""
    n = 3
    members = [_ctx(fa, [parts()[p]]) for p in range(n)]
    whole = _ctx(fa, parts())
    try:
        with fa.FlowGroup(members) as g:
            want = whole.read_window().tobytes()
            assert [g.read_window(fa.ROWS_5M).tobytes() for _ in range(2 * n + 1)] == [want] * (2 * n + 1)
            want = whole.top_talkers(0, 50).tobytes()
            assert [g.top_talkers(0, 50).tobytes() for _ in range(2 * n + 1)] == [want] * (2 * n + 1)
    finally:
        for x in members + [whole]:
            x.close()


# ---- idle and empty members ----------------------------------------------------------------------------------------------------
def test_a_member_without_records(gpu_lib, fa, capfd, monkeypatch):
    """one member of three never ingested: it still owns a share of the keys (whatever the hash gives it), and every read is
    the single ctx's"""
    with _Groups(fa, capfd, monkeypatch, [[0], [], [1]]) as t:
        ts = int(t.whole.open_timeslots()[0])
        for _ in range(3):  # (every member is the root once - the idle one too)
            assert t.read(lambda g: g.read_window(fa.ROWS_5M))[0].tobytes() == t.whole.read_window().tobytes()
            assert t.read(lambda g: g.read_window(fa.ROWS_APP, ts))[0].tobytes() == t.whole.read_window_app(ts).tobytes()
            for d in (0, 1):
                for k in (10, 0):
                    assert t.read(lambda g: g.top_talkers(d, k))[0].tobytes() == t.whole.top_talkers(d, k).tobytes()
        (rows, shares), _ = t.read(lambda g: g.read_window_partitioned(fa.ROWS_APP, ts))
        _check_shares(fa, rows, shares, t.whole.read_window_app(ts), 3)


@pytest.mark.parametrize("n", [1, 3])
def test_nothing_to_return(gpu_lib, fa, capfd, monkeypatch, n):
    """a timeslot nobody holds; talker tables with nothing folded: FA_OK and no rows, from all three entry points"""
    L = fa.lib()
    with _Groups(fa, capfd, monkeypatch, [[p] for p in range(n)]) as t, _Groups(fa, capfd, monkeypatch, [[]] * n) as fresh:
        nobody = int(t.whole.open_timeslots()[0]) - 86400
        for grp, ts in ((t, nobody), (fresh, nobody), (fresh, fa.ALL_TIMESLOTS)):
            for kind in (fa.ROWS_5M, fa.ROWS_APP):
                assert len(grp.read(lambda g: g.read_window(kind, ts))[0]) == 0
                rows, shares = grp.read(lambda g: g.read_window_partitioned(kind, ts))[0]
                assert len(rows) == 0 and shares == [0] * n
        for d, name in ((0, "SrcAddr"), (1, "DstAddr")):
            for k in (0, 10):
                # (a group of one fetches its no rows and says so; several members stop behind their empty shares, without a line)
                said = [["top talkers (%s), 1 members, k %d, 0 rows out" % (name, k), ["rows", "fetch"]]] if n == 1 else []
                got, lines = fresh.read(lambda g: g.top_talkers(d, k))
                assert len(got) == 0 and lines == said
                got, lines = fresh.read(lambda g: g.read_window(fa.ROWS_TALKERS_SRC + d, 0, k))
                assert len(got) == 0 and lines == said
        got, lines = fresh.read(lambda g: g.read_window_partitioned(fa.ROWS_APP, nobody))
        assert lines == [["partitioned read of kind 1, %d members, 0 rows out" % n, SHARES + ["fetch"]]]
        # the raw calls: FA_OK, *n_out = 0 (not left alone)
        out = np.zeros(4, dtype=fa.ROW_APP_DTYPE)
        g = fresh.loud._h
        for call in (lambda n_out: L.fa_group_read_window(g, fa.ROWS_APP, nobody, 0, out.ctypes.data, 4, n_out),
                     lambda n_out: L.fa_group_read_window_partitioned(g, fa.ROWS_APP, nobody, out.ctypes.data, 4, None, n_out),
                     lambda n_out: L.fa_group_top_talkers(g, 0, 10, out.ctypes.data, 4, n_out)):
            n_out = C.c_size_t(SENTINEL)
            assert call(C.byref(n_out)) == 0 and n_out.value == 0


# ---- the error table -----------------------------------------------------------------------------------------------------------
def _gerr(L, g):
    return (L.fa_group_last_error(g) or b"").decode()


def _merr(L, members):
    return [(L.fa_last_error(m._h) or b"").decode() for m in members]


def _mark(fa, members):
    """leaves MARK as every member's last error"""
    out, n_out = np.zeros(4, dtype=fa.PORT_ROW_DTYPE), C.c_size_t()
    for m in members:
        assert fa.lib().fa_top_ports(m._h, 0, 1, out.ctypes.data, 4, C.byref(n_out)) == ERR_ARG
    assert _merr(fa.lib(), members) == [MARK] * len(members)


@pytest.mark.parametrize("n", [1, 3])
def test_error_paths_of_the_group(gpu_lib, fa, n):
    """Return code, fa_group_last_error, every member's fa_last_error and *n_out of each refused call - and that a read behind
    it returns what it returned before: nothing was dropped."""
    L = fa.lib()
    members = [_ctx(fa, [parts()[p]]) for p in range(n)]
    whole = _ctx(fa, parts()[:n])
    try:
        with fa.FlowGroup(members) as grp:
            g = grp._h
            ts = int(whole.open_timeslots()[0])
            R5, RA, T0 = fa.ROWS_5M, fa.ROWS_APP, fa.ROWS_TALKERS_SRC

            def state():  # (the window every close below names, and the first talkers)
                return b"".join([grp.read_window(R5, ts, cap=1 << 15).tobytes(), grp.read_window(RA, ts, cap=1 << 15).tobytes(), grp.top_talkers(1, 50).tobytes()])
            before = state()
            assert before == b"".join([whole.read_window(ts).tobytes(), whole.read_window_app(ts).tobytes(), whole.top_talkers(1, 50).tobytes()])
            need5, needa, needt = len(whole.read_window(ts)), len(whole.read_window_app(ts)), len(whole.top_talkers(1))
            assert min(need5, needa, needt) > 1
            out = np.zeros(max(need5, needa, needt), dtype=fa.ROW_APP_DTYPE)  # (56-byte rows: room for every kind)
            p, shares = out.ctypes.data, (C.c_size_t * n)()

            def calls(kind5, kinda):
                """every entry point that writes rows, as f(out, cap, n_out), with the rows it needs"""
                return [("read", lambda o, c, m: L.fa_group_read_window(g, kind5, ts, 0, o, c, m), need5),
                        ("close", lambda o, c, m: L.fa_group_close_window(g, kind5, ts, o, c, m), need5),
                        ("close app", lambda o, c, m: L.fa_group_close_window(g, kinda, ts, o, c, m), needa),
                        ("read partitioned", lambda o, c, m: L.fa_group_read_window_partitioned(g, kinda, ts, o, c, shares, m), needa),
                        ("close partitioned", lambda o, c, m: L.fa_group_close_window_partitioned(g, kinda, ts, o, c, None, m), needa),
                        ("close partitioned 5m", lambda o, c, m: L.fa_group_close_window_partitioned(g, kind5, ts, o, c, shares, m), need5),
                        ("top talkers", lambda o, c, m: L.fa_group_top_talkers(g, 1, 0, o, c, m), needt),
                        ("top talkers k", lambda o, c, m: L.fa_group_top_talkers(g, 0, 7, o, c, m), 7),
                        ("talkers by kind", lambda o, c, m: L.fa_group_read_window(g, T0 + 1, 0, 0, o, c, m), needt)]

            def refused(name, call, code, text, n_want, member_text=None):
                _mark(fa, members)
                was = _gerr(L, g)
                n_out = C.c_size_t(SENTINEL)
                assert call(C.byref(n_out)) == code, name
                assert _gerr(L, g) == (was if text is None else text), name
                assert n_out.value == n_want, name
                assert _merr(L, members) == [member_text or MARK] * n, name
                assert state() == before, name

            # a buffer one row short; no buffer at all: the rows needed come back, nothing is removed
            for name, f, need in calls(R5, RA):
                refused(name + ", one short", lambda m: f(p, need - 1, m), ERR_CAPACITY, SMALL, need)
                refused(name + ", no buffer", lambda m: f(None, 0, m), ERR_CAPACITY, SMALL, need)
            # a NULL n_out, a buffer of no address: FA_ERR_ARG before anything else (the group's text is left alone)
            for name, f, need in calls(R5, RA):
                _mark(fa, members)
                was = _gerr(L, g)
                assert f(p, need, None) == ERR_ARG and _gerr(L, g) == was and _merr(L, members) == [MARK] * n, name
                refused(name + ", NULL out", lambda m: f(None, 4, m), ERR_ARG, None, SENTINEL)
            # kinds that are not windowed, to both closes
            for kind in (fa.ROWS_PORT_SRC, fa.ROWS_MINUTE, fa.ROWS_TOPK_DST, T0, 7, 99):
                refused("close %d" % kind, lambda m: L.fa_group_close_window(g, kind, ts, p, need5, m), ERR_ARG,
                        "fa_group_close_window: not a windowed row kind", SENTINEL)
                refused("close partitioned %d" % kind, lambda m: L.fa_group_close_window_partitioned(g, kind, ts, p, need5, shares, m), ERR_ARG,
                        "fa_group_close_window_partitioned: not a windowed row kind", SENTINEL)
            # kinds that do not exist, to both reads
            for kind in (7, 99):
                refused("read %d" % kind, lambda m: L.fa_group_read_window(g, kind, ts, 0, p, need5, m), ERR_ARG, "unknown row kind", SENTINEL)
                refused("read partitioned %d" % kind, lambda m: L.fa_group_read_window_partitioned(g, kind, ts, p, need5, shares, m), ERR_ARG,
                        "unknown row kind", SENTINEL)
            # top-k
            refused("top-k rows, k = 0", lambda m: L.fa_group_read_window(g, fa.ROWS_TOPK_SRC, 0, 0, p, 8, m), ERR_ARG, "top-k rows need k > 0", SENTINEL)
            for ks in (0, 1, 6, 8):
                refused("topk key set %d" % ks, lambda m: L.fa_group_topk(g, ks, 10, p, 8, m), ERR_ARG, "fa_group_topk: key set", SENTINEL)
            refused("topk, k = 0", lambda m: L.fa_group_topk(g, fa.FA_KEYS_SRCADDR_CMS, 0, p, 8, m), 0, None, 0)
            assert L.fa_group_topk(g, fa.FA_KEYS_SRCADDR_CMS, 0, p, 8, None) == ERR_ARG
            assert L.fa_group_topk(None, 99, 0, p, 8, None) == ERR_ARG
            # talkers
            for dst in (2, -1):
                refused("talkers dst %d" % dst, lambda m: L.fa_group_top_talkers(g, dst, 10, p, 16, m), ERR_ARG, "fa_group_top_talkers: bad argument", SENTINEL)
        # a member that was never enabled (the last one): FA_ERR_UNSUPPORTED, and every member says which one
        off = fa.FlowAgg(**KW)
        members.append(off)
        with fa.FlowGroup(members) as grp:
            g = grp._h
            text = "top talkers: member %d: %s" % (n, NOT_ENABLED)
            for call in (lambda m: L.fa_group_top_talkers(g, 0, 10, p, 16, m), lambda m: L.fa_group_read_window(g, T0 + 1, 0, 10, p, 16, m)):
                _mark(fa, members)
                n_out = C.c_size_t(SENTINEL)
                assert call(C.byref(n_out)) == ERR_UNSUPPORTED
                assert (_gerr(L, g), n_out.value) == (text, 0)
                assert _merr(L, members) == ["group: " + text] * (n + 1)
            assert grp.read_window(R5).tobytes() == whole.read_window().tobytes()
        for d in (0, 1):
            assert fa.dist.merge_talkers_host([m.top_talkers(d) for m in members[:n]]).tobytes() == whole.top_talkers(d).tobytes()
    finally:
        for x in members + [whole]:
            x.close()
