"""The single chain's work-buffer layout (csrc/host_layout.h) under the sanitizers: tests/work_layout_main.cpp is a
stand-alone program that includes that header alone; it is built with the host compiler and run under the address
and undefined-behaviour sanitizers.  Nothing is preloaded, nothing goes through python; no GPU."""
import os
import subprocess

from test_feed_queue_host import _cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "work_layout_main.cpp")


def test_work_layout_under_sanitizers(tmp_path):
    cxx = _cxx()
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "work_layout_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-fsanitize=address,undefined",
           SRC, "-o", exe]
    if "clang" not in os.path.basename(cxx):
        # (the sanitizer's runtime inside the program, as clang links it: it need not come first among the libraries)
        cmd += ["-static-libasan", "-static-libubsan"]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, env=env, timeout=300)
    print(run.stdout[-6000:])
    assert run.returncode == 0, run.stdout[-6000:]
    assert "ALL OK" in run.stdout and "FAIL" not in run.stdout
    assert "ERROR: AddressSanitizer" not in run.stdout and "runtime error" not in run.stdout
