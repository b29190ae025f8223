"""CPU tests of the merge of pending flows_raw parts (include/flowagg.h "merging the pending flows_raw parts").

tests/host_raw_merge.hip instantiates the two __host__ __device__ lookups of csrc/raw_merge.cuh on the host - the text the
kernels run - against a linear scan and against raw_col_offset arithmetic, and enumerates the part writer's tile walk and LDS
staging with the geometry functions of csrc/raw.cuh (again the kernels' text) over the merged row counts of the GPU test.  It is
built plain and with the host's AddressSanitizer + UBSan and run as a program.  The
library's part: the two new symbols are exported and the ABI is still 8.  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-g"]


def _program(sanitize):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_raw_merge" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "host_raw_merge.hip")
    deps = [src] + [os.path.join(ROOT, "flow-pipeline_amd", "csrc", f) for f in ("raw_merge.cuh", "raw.cuh", "align16.cuh")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1" if sanitize else "-O2", "-std=c++17"] + (SANITIZE if sanitize else []) + ["-o", exe, src])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_lookups_and_tile_walk(sanitize):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")  # (the process loads the HIP runtime, which keeps its allocations)
    res = subprocess.run([_program(sanitize)], capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0 and res.stdout.startswith("OK "), res.stdout + res.stderr[-4000:]
    assert int(re.findall(r"\d+", res.stdout)[0]) > 10 ** 6  # the find, offset and tile checks all ran


def test_library_exports_the_merge(fa):
    if not os.path.exists(fa.LIB_PATH):
        fa.build()
    L = fa.lib()
    assert L.fa_abi_version() == 8
    for name in ("fa_raw_merge", "fa_raw_merge_stats"):
        assert getattr(L, name) is not None
    assert [n for n, _ in fa.RawMergeStats._fields_] == ["merges", "parts_in", "parts_out", "rows", "bytes_in", "bytes_out", "launches", "order_ns", "gather_ns"]
