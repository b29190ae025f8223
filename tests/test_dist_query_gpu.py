"""dist.raw_query_merged across two rank processes: one address kind and one scalar kind against the single-ctx twin, and what a
rank without a result does to both.

ONE run of two fresh processes (torch.distributed.run, gloo, both on the one GPU, under a timeout): each rank builds its share of
the records into a ctx with fa_raw_enable and queries its pending parts; a second ctx per rank holds every record and is the
reference, byte for byte, beside the numpy restatement of raw_query_cases."""
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
import json, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np, torch, torch.distributed as dist
import _pkg
fa = _pkg.load()
import raw_query_cases as Q
import raw_query_group_cases as GC
from test_raw_parts_gpu import _upload
d = fa.dist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)   # both ranks share the one GPU; the exchange goes over gloo
dist.init_process_group("gloo")
def ctx(rows):
    a = fa.FlowAgg(framed=True)
    a.raw_enable(0)
    cols, keep = _upload(fa, rows, np.zeros(len(rows), dtype=np.uint8))
    a.raw_build_columns(cols, len(rows))
    return a
rows, f = GC.seeded_stream(21, 1500)
groups = Q.G["SRC_ADDR"] | Q.G["SRC_PORT"]
want = Q.matching([rows], f)
report = {"checked": 0, "failures": [], "afterwards": False}
with ctx(GC.deal(rows, world)[rank]) as agg, ctx(rows) as whole, fa.FlowAgg(framed=True) as none:
    agg.raw_query_pending(groups, **f)
    whole.raw_query_pending(groups, **f)
    own = {bit: agg.raw_query_rows(bit, 0, Q.O_KEY).tobytes() for bit in (1, 4)}
    for bit in (Q.G["SRC_ADDR"], Q.G["SRC_PORT"]):
        by_key = Q.groups_of(want, bit)
        assert len(by_key) > 3
        for order in (Q.O_WEIGHT, Q.O_KEY):
            for k in (0, 1, 3, 1 << 20):
                got = d.raw_query_merged(agg, bit, k, order)
                exp = Q.ordered(by_key, order)
                exp = exp[:k] if k else exp
                assert got.tobytes() == exp.tobytes() == whole.raw_query_rows(bit, k, order).tobytes(), (bit, order, k)
                report["checked"] += 1
    assert {bit: agg.raw_query_rows(bit, 0, Q.O_KEY).tobytes() for bit in (1, 4)} == own  # the rank's own result did not move
    # a rank that fails (rank 1's ctx holds no result) takes both down: its own error there, RankFailed on the other
    for bit in (Q.G["SRC_ADDR"], Q.G["SRC_PORT"]):
        try:
            d.raw_query_merged(agg if rank == 0 else none, bit, 3)
            report["failures"].append("none")
        except fa.FlowAggError as e:
            report["failures"].append("own %%d" %% e.code)
        except d.RankFailed:
            report["failures"].append("other")
    # ... and the next merged read works
    assert d.raw_query_merged(agg, Q.G["SRC_PORT"], 2).tobytes() == whole.raw_query_rows(Q.G["SRC_PORT"], 2).tobytes()
    report["afterwards"] = True
dist.destroy_process_group()
with open(os.path.join(%(out)r, "rank%%d.json" %% rank), "w") as fh:
    json.dump(report, fh)
'''


@pytest.fixture(scope="module")
def two_rank_run(tmp_path_factory):
    """-> each rank's report (every comparison with the single ctx is made inside the ranks: a mismatch fails the run)"""
    out = tmp_path_factory.mktemp("dist_query")
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


def test_two_ranks_merged_queries_equal_one_ctx(gpu_lib, two_rank_run):
    a, b = two_rank_run
    assert a["checked"] == b["checked"] == 16 and a["afterwards"] and b["afterwards"]


def test_two_ranks_a_rank_without_a_result_takes_both_down(gpu_lib, two_rank_run):
    """by owner, then gathered: rank 1 raises its own FlowAggError, rank 0 RankFailed; nobody waited (the run came back)"""
    assert [r["failures"] for r in two_rank_run] == [["other", "other"], ["own %d" % ERR_ARG] * 2]
