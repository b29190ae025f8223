"""CPU tests of bench.py's command line and of --dump-outputs' two helpers (the GPU run itself:
tests/test_ingest_sinks_gpu.py::test_bench_plain_run_dumps_the_rows_of_its_steps)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_command_line():
    r = subprocess.run([sys.executable, "bench.py", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--stage", "decode", "--dump-outputs", "x"]):
        r = subprocess.run([sys.executable, "bench.py"] + bad, capture_output=True, text=True, cwd=ROOT, timeout=120)
        assert r.returncode == 2 and "error" in r.stderr, bad


def _step_rows(po, steps, n=50_000):
    """The oracle's flows_5m rows after `steps` passes over the same records (what the timed context holds)."""
    gp = po.gen_params(mode=po.GEN_ASPAIRS, framed=1, seed=5, n_total=n, span_secs=900, per_sec=400_000)
    buf, off = po.gen_records(gp, 0, n)
    r = po.Rollup(300)
    for _ in range(steps):
        assert r.ingest(buf, off, 1) == 0
    return r.rows()


def test_rows_added_is_what_the_later_steps_ingested(po):
    import bench
    one, three, five = _step_rows(po, 1), _step_rows(po, 3), _step_rows(po, 5)
    assert bench.rows_added(three, five).tobytes() == bench.rows_added(one, three).tobytes()
    two = one.copy()
    for f in ("bytes", "packets", "count"):
        two[f] = one[f] * np.uint64(2)
    assert bench.rows_added(three, five).tobytes() == two.tobytes()
    assert bench.rows_added(one[:0], three).tobytes() == three.tobytes()  # no settle steps: the window was empty
    with pytest.raises(RuntimeError):
        bench.rows_added(one[1:], three)


def test_dump_outputs_writes_every_field_exactly_and_samples_above_the_limit(po, tmp_path, monkeypatch):
    import bench
    rows = _step_rows(po, 3)
    bench.dump_outputs(str(tmp_path / "all"), rows)
    names = sorted(os.listdir(tmp_path / "all"))
    assert names == sorted("flows_5m_%s.npy" % f for f in rows.dtype.names if not f.startswith("_"))
    for f in ("timeslot", "src_as", "bytes", "count"):
        a = np.load(tmp_path / "all" / ("flows_5m_%s.npy" % f))
        assert a.dtype == np.float64 and np.array_equal(a.astype(np.uint64), rows[f])
    assert sum(os.path.getsize(tmp_path / "all" / x) for x in names) < 64 * 10**6
    # above the limit: a fixed seeded sample of the rows, key order kept, the same rows every time
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 * 100)
    bench.dump_outputs(str(tmp_path / "a"), rows)
    bench.dump_outputs(str(tmp_path / "b"), rows)
    ts = [np.load(tmp_path / d / "flows_5m_timeslot.npy") for d in ("a", "b")]
    sa = np.load(tmp_path / "a" / "flows_5m_src_as.npy")
    assert len(ts[0]) == 100 and np.array_equal(ts[0], ts[1])
    assert np.all(np.isin(sa, rows["src_as"].astype(np.float64))) and np.all(np.diff(ts[0]) >= 0)
