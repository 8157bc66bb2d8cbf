"""The workspaces' byte layouts (csrc/ikg_ws_layout.hpp, nothing from HIP):
tests/ws_layout_main.cpp declares each of them at B = 1, 63 and 4,096 in fp64
and fp32 sizes and compares offsets and totals with literals worked out by
hand.  Built with g++ under ASan + UBSan and run directly."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _gxx(tmp_path, src, out):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *SAN,
                           "-I", os.path.join(PKG, "csrc"), src, "-o", out],
                          capture_output=True, text=True, timeout=120)


def test_workspace_layouts_under_asan_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if _gxx(tmp_path, str(probe), str(tmp_path / "probe")).returncode != 0:
        pytest.skip("g++ lacks the sanitizer runtimes")
    exe = str(tmp_path / "ws_layout")
    r = _gxx(tmp_path, os.path.join(HERE, "ws_layout_main.cpp"), exe)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ws layout ok" in r.stdout, r.stdout + r.stderr
