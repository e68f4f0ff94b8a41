"""CPU (no GPU): the host planner of a pair-forward call (align3r_amd/csrc/dedup.h: plan_call -- the grouping of the slots, the
tables of the frame cache and of the stored priors, the head products' bits and every list of CallLists, together), in a
stand-alone C++ program (tests/call_plan_main.cpp, its own main, not loaded into Python) built with -fsanitize=address,undefined:
random call sequences against a content model in which every slot must find its own frame, prior and head products through the
lists, plus the eviction-then-reuse, capacity, absent-store, flush and malformed-table cases."""
import os
import shutil
import subprocess

from conftest import REPO


def test_call_plan_host_side_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "call_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", os.path.join(REPO, "align3r_amd", "csrc"), os.path.join(REPO, "tests", "call_plan_main.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
