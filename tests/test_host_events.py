"""CPU test of the library's event owner (flow-pipeline_amd/csrc/events.h): tests/host_events.cpp is compiled with the host
C++ compiler under AddressSanitizer (which includes LeakSanitizer) and UndefinedBehaviorSanitizer and run as a program of its
own.  No GPU, no ROCm header, nothing loaded into python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_event_pool_owns_takes_rewinds_and_never_leaks(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "host_events")  # (built afresh every time: a second of compiling, no stale program)
    src = os.path.join(ROOT, "tests", "host_events.cpp")
    # (the sanitizer runtimes are linked statically - clang's default: the program does not depend on the order in which
    # the dynamic loader brings libraries in)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all"] + static + ["-o", exe, src])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout + res.stderr
    assert "Sanitizer" not in res.stderr, res.stderr
