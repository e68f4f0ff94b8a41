"""CPU (no GPU): the host side of the frame products kept across forward calls (align3r_amd/csrc/dedup.h: the depth priors' own
FrameCacheTable, prior_lists -- which prior runs, which is stored, where every row finds its rows -- and SiteMask, the site list
with gaps of the statistics pass), in a stand-alone C++ program (tests/frame_products_main.cpp, its own main, not loaded into
Python) built with -fsanitize=address,undefined: random hit / miss / evict / flush sequences against a naive model."""
import os
import shutil
import subprocess

from conftest import REPO


def test_frame_products_host_side_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "frame_products_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", os.path.join(REPO, "align3r_amd", "csrc"), os.path.join(REPO, "tests", "frame_products_main.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
