"""The closes of flow-pipeline_amd/dist.py across two rank processes: what every close returns, and what a failing rank does
to both.  A characterisation test: written against the sources BEFORE the three closes were recomposed from shared stages, it
pins what that rewrite must keep.

ONE run of two fresh processes (torch.distributed.run, gloo, both on the one GPU, under a timeout) is shared by the tests:
each rank ingests its partition into a ctx, a second ctx per rank ingests both and is the reference, byte for byte."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1

WORKER = r'''
import hashlib, json, os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
import _pkg
fa, po = _pkg.load(), _pkg.load_oracle()
d = fa.dist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)   # both ranks share the one GPU; the exchange goes over gloo
dist.init_process_group("gloo")
n = 40000
gp = po.gen_params(mode=po.GEN_ZIPF, framed=1, seed=3201, n_total=n, zipf_log2_universe=13, span_secs=900)
buf, off = po.gen_records(gp, 0, n)
raw = bytes(buf)
parts = []
for p in range(world):  # record i belongs to partition i %% world
    recs = [raw[int(off[k]):int(off[k + 1])] for k in range(p, n, world)]
    o = np.zeros(len(recs) + 1, dtype=np.uint64)
    o[1:] = np.cumsum([len(r) for r in recs])
    parts.append((np.frombuffer(b"".join(recs), dtype=np.uint8), o))
report = {"results": {}, "failures": [], "afterwards": False}  # (a file per rank: the ranks' lines on stdout interleave)
sha = lambda rows: hashlib.sha256(rows.tobytes()).hexdigest()
KW = dict(framed=True, key_sets=57)
with fa.FlowAgg(**KW) as agg, fa.FlowAgg(**KW) as whole, fa.FlowAgg(framed=True, key_sets=49) as narrow:
    agg.ingest(*parts[rank])
    narrow.ingest(*parts[rank])
    for b, o in parts:
        whole.ingest(b, o)
    ts = int(whole.open_timeslots()[0])
    # every kind, gathered: identical on every rank, the single ctx's rows
    want = {"5m": whole.read_window(), "app": whole.read_window_app(), "app window": whole.read_window_app(ts), "ports src": whole.top_ports(0),
            "ports dst": whole.top_ports(1), "minutes": whole.minute_series()}
    got = {"5m": d.rows_merged(agg, fa.ROWS_5M), "app": d.rows_merged(agg, fa.ROWS_APP), "app window": d.rows_merged(agg, fa.ROWS_APP, ts),
           "ports src": d.rows_merged(agg, fa.ROWS_PORT_SRC), "ports dst": d.rows_merged(agg, fa.ROWS_PORT_DST), "minutes": d.rows_merged(agg, fa.ROWS_MINUTE)}
    for name in want:
        assert len(want[name]) > 0 and got[name].tobytes() == want[name].tobytes(), name
        report["results"][name] = sha(got[name])
    assert d.top_ports_merged(agg, 1, 20).tobytes() == whole.top_ports(1, 20).tobytes()
    assert d.minute_series_merged(agg).tobytes() == want["minutes"].tobytes()
    # by owner: this rank's share - its keys only, complete, in emit order; the shares together are the gathered rows
    share = d.rows_merged_partitioned(agg, fa.ROWS_APP, ts)
    assert (d.partition_rows_host(share, fa.ROWS_APP, world) == rank).all() and 0 < len(share) < len(want["app window"])
    assert d.merge_rows_app_host([share]).tobytes() == share.tobytes()
    union = d.merge_rows_app_host(d.allgather_struct(share, d.ROW_APP_DTYPE, device="cpu"))
    assert union.tobytes() == want["app window"].tobytes()
    report["results"]["share of rank %%d" %% rank] = len(share)
    # a rank that fails (rank 1's ctx lacks the key set) takes both down: its own error there, RankFailed on the other
    for close in (lambda a: d.rows_merged(a, fa.ROWS_APP), lambda a: d.rows_merged_partitioned(a, fa.ROWS_APP)):
        try:
            close(agg if rank == 0 else narrow)
            report["failures"].append("none")
        except fa.FlowAggError as e:
            report["failures"].append("own %%d" %% e.code)
        except d.RankFailed:
            report["failures"].append("other")
    # ... and the next closes work, and drop what the single ctx's closes drop
    assert d.close_window_merged(agg, ts).tobytes() == whole.close_window(ts).tobytes()
    assert d.rows_merged(agg, fa.ROWS_5M).tobytes() == whole.read_window().tobytes()
    share = d.close_window_app_partitioned(agg, ts)
    assert (d.partition_rows_host(share, fa.ROWS_APP, world) == rank).all()
    union = d.merge_rows_app_host(d.allgather_struct(share, d.ROW_APP_DTYPE, device="cpu"))
    assert union.tobytes() == whole.close_window_app(ts).tobytes()
    left = d.rows_merged(agg, fa.ROWS_APP)
    assert left.tobytes() == whole.read_window_app().tobytes() and 0 < len(left) < len(want["app"])
    assert len(d.rows_merged(agg, fa.ROWS_APP, ts)) == 0 and len(d.rows_merged_partitioned(agg, fa.ROWS_APP, ts)) == 0
    report["afterwards"] = True
dist.destroy_process_group()
with open(os.path.join(%(out)r, "rank%%d.json" %% rank), "w") as f:
    json.dump(report, f)
'''


@pytest.fixture(scope="module")
def two_rank_run(tmp_path_factory):
    """-> each rank's report (every comparison with the single ctx is made inside the ranks: a mismatch fails the run)"""
    out = tmp_path_factory.mktemp("dist_paths")
    script = out / "worker.py"
    script.write_text(WORKER % {"root": ROOT, "out": str(out)})
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return [json.load(open(out / ("rank%d.json" % rank))) for rank in (0, 1)]


def test_two_ranks_every_close_equals_one_ctx(gpu_lib, two_rank_run):
    a, b = two_rank_run
    kinds = ["5m", "app", "app window", "ports src", "ports dst", "minutes"]
    assert all(a["results"][k] == b["results"][k] for k in kinds)  # identical on both ranks
    assert a["results"]["share of rank 0"] > 0 and b["results"]["share of rank 1"] > 0
    assert a["afterwards"] and b["afterwards"]


def test_two_ranks_a_failing_rank_takes_both_down(gpu_lib, two_rank_run):
    """gathered, then by owner: rank 1 raises its own FlowAggError, rank 0 RankFailed; nobody waited (the run came back)"""
    assert [r["failures"] for r in two_rank_run] == [["other", "other"], ["own %d" % ERR_ARG] * 2]
