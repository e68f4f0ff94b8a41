"""CPU (no GPU): the per-side host grouping of the duplicate detection (align3r_amd/csrc/dedup.h, dedup_group_side: the image kind's
representatives -> each side's distinct frames + slot map, which the DPT heads' level-0 branch runs on) in a stand-alone C++ program
(tests/dedup_side_main.cpp, its own main, not loaded into Python) built with -fsanitize=address,undefined: all equal, all distinct,
one side constant, B = 1, representatives that sit on the other side (a side's list still names slots of its own side), and
malformed tables are refused."""
import os
import shutil
import subprocess

from conftest import REPO


def test_per_side_grouping_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "dedup_side_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", os.path.join(REPO, "align3r_amd", "csrc"), os.path.join(REPO, "tests", "dedup_side_main.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
