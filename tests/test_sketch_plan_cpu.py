"""CPU tests of the sketches from columns and from parts (include/flowagg.h "the sketches from columns and from parts").

tests/host_sketch_plan.hip instantiates on the host what the sketch fold and the restore decide without a GPU
(csrc/sketch_plan.h): sketch_mask_check over every (created, asked) pair of the 6-bit masks against the truth table, the restore's
mask split, the chunk caps over the destinations' caps - and the key layout of the fold kernel's LDS cache (csrc/sketch_fold.cuh:
no key makes an EMPTY word, the all-zero address included).  It is built plain and with the host's AddressSanitizer + UBSan and
run as a program.  The library's part: the three new symbols are exported and the ABI is still 8.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-Xarch_host", "-g"]


def _program(sanitize):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_sketch_plan" + ("_san" if sanitize else ""))
    src = os.path.join(ROOT, "tests", "host_sketch_plan.hip")
    deps = [src] + [os.path.join(ROOT, "flow-pipeline_amd", "csrc", f) for f in ("sketch_fold.cuh", "sketch_plan.h", "rollup.cuh", "rollup_plan.h", "keytab.cuh", "sinks.cuh", "table.cuh")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1" if sanitize else "-O2", "-std=c++17"] + (SANITIZE if sanitize else []) + ["-o", exe, src])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_masks_chunks_words(sanitize):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")  # (the process loads the HIP runtime, which keeps its allocations)
    res = subprocess.run([_program(sanitize)], capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0 and res.stdout.startswith("OK "), res.stdout + res.stderr[-4000:]
    assert int(re.findall(r"\d+", res.stdout)[0]) > 10 ** 5  # the mask, chunk and key-word checks all ran


def test_library_exports_the_sketch_doors(fa):
    if not os.path.exists(fa.LIB_PATH):
        fa.build()
    L = fa.lib()
    assert L.fa_abi_version() == 8
    for name in ("fa_sketch_fold_columns_device", "fa_raw_restore", "fa_sketch_fold_stats"):
        assert getattr(L, name) is not None
    assert [n for n, _ in fa.SketchFoldStats._fields_] == ["calls", "records_in", "records_bad", "records_folded", "batches", "launches", "fold_ns"]
    assert C.sizeof(fa.SketchFoldStats) == 56
    for name in ("sketch_fold_columns", "raw_restore", "sketch_fold_stats"):
        assert callable(getattr(fa.FlowAgg, name))
