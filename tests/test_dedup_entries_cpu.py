"""CPU (no GPU): the entry grouping of the duplicate detection (align3r_amd/csrc/dedup.h, dedup_group_entries: the slot maps of the
image and the depth-prior kind -> each side's distinct (image, prior) entries + slot map, padded to one count, which decoder block 0
runs its frame-only half on) in a stand-alone C++ program (tests/dedup_entries_main.cpp, its own main, not loaded into Python) built
with -fsanitize=address,undefined: all distinct, all equal, one image with two priors and one prior with two images (the entry is the
pair), unequal counts on the two sides (padding), representatives that sit on the other side, and malformed tables are refused."""
import os
import shutil
import subprocess

from conftest import REPO


def test_entry_grouping_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "dedup_entries_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", os.path.join(REPO, "align3r_amd", "csrc"), os.path.join(REPO, "tests", "dedup_entries_main.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
