"""Launch routing without a GPU (csrc/sn_route.h): a host compiler takes the header as it is, and the stand-alone program
tests/c/route_check.cpp checks it -- the clip's plan and the decision of a launch against values written out by hand on both
sides of every boundary, the refusals' texts, the pause after failed frames, prefer_pool against recorded answers -- once plain
and once under AddressSanitizer and UBSan.  tests/test_small_planes_cpu.py puts its tables to the same program as queries."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc")


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
def test_routes_match_values_written_out_by_hand(tmp_path, sanitized):
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else []
    exe = str(tmp_path / ("route_check" + ("_san" if sanitized else "")))
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, *extra, os.path.join(ROOT, "tests", "c", "route_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-3000:], r.stderr[-2000:])
    # ... and a query: a 4:2:0 clip of 400 lines, one frame -- luma in twelve bands, chroma by the pool kernels
    q = "1 8 3 1 1 256 400 0 1 1 0 0 0 0 0 0  1 0 4 0 0 0 0 0 0 0 0 2 0 0".split()
    r = subprocess.run([exe] + q, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and " route=coupled_banded nbands=12 " in r.stdout and " stop=200,101,100 " in r.stdout, (r.stdout, r.stderr[-2000:])
