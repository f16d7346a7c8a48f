"""ccvpe_amd/csrc/dev_cache.h, the per-device grow-only integer behind every launcher's dynamic-LDS opt-in and num_cus(), checked
on the host: tests/host/dev_cache_main.cpp (own main, no HIP) is compiled with the host compiler and run — per-device slots,
grow-only raises, ordinals outside the table, eight racing threads — and once more under ThreadSanitizer as a stand-alone
binary where the toolchain links that runtime."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "dev_cache_main.cpp")
INC = os.path.join(ROOT, "ccvpe_amd", "csrc")


def _host_compiler():
    for name in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(name)
        if path:
            return path
    return None


def _build(tmp_path, name, extra):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler on this box")
    exe = str(tmp_path / name)
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", "-I", INC, SRC, "-o", exe] + extra,
                         capture_output=True, text=True, timeout=300)
    return exe, res


def test_dev_cache_host_program(tmp_path):
    exe, res = _build(tmp_path, "dev_cache_main", [])
    assert res.returncode == 0, res.stdout + res.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "dev_cache ok" in run.stdout, run.stdout + run.stderr


def test_dev_cache_host_program_under_thread_sanitizer(tmp_path):
    exe, res = _build(tmp_path, "dev_cache_tsan", ["-fsanitize=thread"])
    if res.returncode != 0:
        pytest.skip("this toolchain does not link the ThreadSanitizer runtime")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if "FATAL: ThreadSanitizer" in run.stderr:
        pytest.skip("the ThreadSanitizer runtime does not start on this box: " + run.stderr.strip().splitlines()[0])
    assert run.returncode == 0 and "dev_cache ok" in run.stdout, run.stdout + run.stderr
