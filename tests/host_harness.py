"""Building a host harness (tests/host/*.cpp: kernel source compiled for the CPU) as a shared library, for the
test_*_kernel_on_host.py files.  A plain module: imported by name like the other test modules, no fixtures of its own."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def build_shared(src, out):
    """g++ src -> the shared library out (float32 arithmetic as written: -ffp-contract=off); skips without a host compiler."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-Wno-unused-value",
                    "-Wno-unknown-pragmas", "-I", os.path.join(HERE, "host", "stub"), src, "-o", out], check=True)
    return out
