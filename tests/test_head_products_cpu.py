"""CPU (no GPU): the host side of the head products kept across forward calls (align3r_amd/csrc/dedup.h: the (entry, side) bits
beside the frame cache's FrameCacheTable, and head_lists -- which frames of a side run, which are stored, where every slot finds its
blocks), in a stand-alone C++ program (tests/head_products_main.cpp, its own main, not loaded into Python) built with
-fsanitize=address,undefined: random hit / miss / evict / flush sequences against a naive model."""
import os
import shutil
import subprocess

from conftest import REPO


def test_head_products_host_side_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "head_products_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", os.path.join(REPO, "align3r_amd", "csrc"), os.path.join(REPO, "tests", "head_products_main.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
