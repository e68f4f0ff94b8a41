"""CPU (no GPU): the host table of the frames kept across forward calls (align3r_amd/csrc/dedup.h, FrameCacheTable: hits, misses,
victims in least-recently-used order, never an entry the same call reads, more misses than entries) and the layout of the caller's
storage, in a stand-alone C++ program (tests/frame_cache_main.cpp, its own main, not loaded into Python) built with
-fsanitize=address,undefined: random hit / miss / evict / flush sequences against a naive model, malformed answers refused."""
import os
import shutil
import subprocess

from conftest import REPO


def test_frame_cache_table_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "frame_cache_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", os.path.join(REPO, "align3r_amd", "csrc"), os.path.join(REPO, "tests", "frame_cache_main.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
