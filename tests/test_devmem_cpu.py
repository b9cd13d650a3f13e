"""The device-buffer pool (csrc/lqro_devmem.hpp) on the CPU.

lqro_ctx and the one-shot entry points leave every device buffer to a DevPool;
nothing on a GPU notices a buffer freed twice or never.  The pool reaches the
device through three functions only, so tests/cpp/lqro_devmem_main.cpp, which
includes nothing of the project but that header, supplies malloc-backed ones
that count live buffers and can fail the k-th allocation, and checks: all
freed at scope exit, an early release frees once, a failing allocation or fill
returns its code and leaves the earlier buffers owned, the fill covers the
buffer, a zero-element request yields one element.  Built with g++ twice, plain
and with AddressSanitizer + UBSan (a stand-alone host program: leaks, double
frees and writes past a buffer end the run).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "cpp", "lqro_devmem_main.cpp")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "asan_ubsan"])
def test_pool_owns_and_frees(tmp_path, flags):
    exe = str(tmp_path / "lqro_devmem_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, MAIN, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "devmem ok"
