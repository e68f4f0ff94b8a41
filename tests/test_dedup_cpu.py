"""CPU (no GPU): the host grouping of the duplicate detection (align3r_amd/csrc/dedup.h: representatives -> distinct list + slot
map) in a stand-alone C++ program (tests/dedup_group_main.cpp, its own main, not loaded into Python) built with
-fsanitize=address,undefined: keys all equal, all distinct, interleaved groups, the representative is the smallest index, the map
is a surjection onto 0..U-1, one and two slots, and malformed tables are refused."""
import os
import shutil
import subprocess

from conftest import REPO


def test_host_grouping_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "dedup_group_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", os.path.join(REPO, "align3r_amd", "csrc"), os.path.join(REPO, "tests", "dedup_group_main.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
