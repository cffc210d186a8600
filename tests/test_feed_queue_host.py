"""The waiting of the trajectory feeder (csrc/host_feedq.h) under the sanitizers: tests/feed_queue_main.cpp is a
stand-alone program with stub draw and run functions; it is built with the host compiler and run, once under the
thread sanitizer and once under the address and undefined-behaviour sanitizers.  Nothing is preloaded, nothing goes
through python; no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "feed_queue_main.cpp")


def _cxx():
    # ROCm's clang first: the thread sanitizer's runtime of a recent compiler-rt checks the address-space layout it
    # finds at start-up (and starts again without randomisation where it does not fit); the one of GCC 11 takes
    # the layout for granted and dies before main on hosts that map memory elsewhere
    for cand in (os.environ.get("CXX"), "/opt/rocm/lib/llvm/bin/clang++", "clang++", "g++"):
        path = shutil.which(cand) if cand else None
        if path:
            return path
    return None


@pytest.mark.parametrize("flags", ["-fsanitize=thread", "-fsanitize=address,undefined"], ids=["tsan", "asan_ubsan"])
def test_feed_queue_under_sanitizers(tmp_path, flags):
    cxx = _cxx()
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "feed_queue_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", flags, SRC, "-o", exe, "-pthread"]
    if "clang" not in os.path.basename(cxx):
        # (the sanitizer's runtime inside the program, as clang links it: it need not come first among the libraries)
        cmd += ["-static-libtsan"] if "thread" in flags else ["-static-libasan", "-static-libubsan"]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout[-4000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66", ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, env=env, timeout=300)
    print(run.stdout[-6000:])
    assert run.returncode == 0, run.stdout[-6000:]
    assert "ALL OK" in run.stdout and "FAIL" not in run.stdout
    assert "WARNING: ThreadSanitizer" not in run.stdout and "ERROR: AddressSanitizer" not in run.stdout
    assert "runtime error" not in run.stdout
