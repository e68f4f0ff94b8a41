"""CPU (no GPU): the workspace sizes built on compact_offsets_bytes (align3r_amd/csrc/compact.h) in a stand-alone program
(tests/compact_sizes_main.cpp, its own main, not loaded into Python): the host code of scene.hip, voxel.hip, tsdf.hip, match.hip and
capi.cpp compiled with the address and undefined-behaviour sanitizers on the host side only (the device code is built plain),
their size functions called at boundary sizes (0, 1, 1024, 1025, the largest each accepts) and compared with the formulas the files held before the header existed.  Nothing in it touches a device."""
import os
import subprocess

from conftest import REPO

CSRC = os.path.join(REPO, "align3r_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
FLAGS = ["-std=c++17", "-O1", "-g", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unused-function",
         "-Wno-unused-variable", "-Wno-unused-result", "-I", CSRC] + SANITIZE


def test_sizes_under_sanitizers(tmp_path):
    sources = [os.path.join(CSRC, f) for f in ("scene.hip", "voxel.hip", "tsdf.hip", "match.hip", "capi.cpp")]
    sources.append(os.path.join(REPO, "tests", "compact_sizes_main.cpp"))
    objects = [str(tmp_path / (os.path.basename(s) + ".o")) for s in sources]
    jobs = [subprocess.Popen([HIPCC] + FLAGS + ["-x", "hip", "-c", s, "-o", o]) for s, o in zip(sources, objects)]
    assert [j.wait() for j in jobs] == [0] * len(jobs)
    exe = str(tmp_path / "compact_sizes_main")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined"] + objects + ["-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout
