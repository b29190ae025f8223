"""CPU test of the plain-value functions behind a launch's plan (flow-pipeline_amd/csrc/launch_plan.h): the key-set mask ->
kernel instantiation mapping, the tile buffer each instantiation has, and the two records-per-tile rules, run on the host by
tests/host_launch_plan.hip and compared - exactly - with the mirrors tests/test_record_lengths_gpu.py centres its streams
on.  Both sides compute in IEEE doubles with a correctly rounded square root: one differing value is a failure.  No GPU needed."""
import os
import subprocess

from test_record_lengths_gpu import WT_STRIDE, _wg_tile_recs, _wt_tile_recs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 63, 64, 65, 256, 4096)
MEANS = range(1, 6001)


def _run():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_launch_plan")
    src = os.path.join(ROOT, "tests", "host_launch_plan.hip")
    csrc = os.path.join(ROOT, "flow-pipeline_amd", "csrc")
    deps = [src, os.path.join(csrc, "launch_plan.h"), os.path.join(csrc, "ingest_feedback.h"), os.path.join(csrc, "sinks.cuh")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-o", exe, src])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-500:] + res.stderr[-2000:]
    return [line.split() for line in res.stdout.splitlines()]


def test_launch_plan_functions_equal_their_mirrors():
    lines = _run()
    variants = {int(l[1]): int(l[2]) for l in lines if l[0] == "variant"}
    assert variants == {m: m if m in (1, 2, 3, 4, 5, 6, 7, 9) else 255 for m in range(64)}
    strides = {int(l[1]): int(l[2]) for l in lines if l[0] == "stride"}
    assert strides == WT_STRIDE
    wg = {int(l[1]): [int(v) for v in l[2:]] for l in lines if l[0] == "wg"}
    assert sorted(wg) == sorted(NS)
    for n in NS:
        assert wg[n] == [_wg_tile_recs(mean * n, n) for mean in MEANS], n
    wt = {(int(l[1]), int(l[2])): [int(v) for v in l[3:]] for l in lines if l[0] == "wt"}
    assert sorted(wt) == sorted((m, n) for m in WT_STRIDE for n in NS)
    for (m, n), got in wt.items():
        assert got == [_wt_tile_recs(mean * n, n, WT_STRIDE[m]) for mean in MEANS], (m, n)
