"""CPU (no GPU): the tile table and the tile chooser of the fh2 GEMM (align3r_amd/csrc/fh2_chooser.h) in a stand-alone C++ program
(tests/fh2_chooser_main.cpp, its own main, not loaded into Python) built with -fsanitize=address,undefined: on the distinct-row and
per-slot shapes of the bench's step (the two lists of tools/bench_fh2.py) the tile counts and waves of every tile shape, the choice
against the measured fastest tile (profiles/fh2_tiles.json), and a forced tile out of range is refused."""
import os
import shutil
import subprocess

from conftest import REPO


def test_chooser_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "fh2_chooser_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", os.path.join(REPO, "align3r_amd", "csrc"), os.path.join(REPO, "tests", "fh2_chooser_main.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
