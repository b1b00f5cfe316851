"""The plan of an anti-aliasing call without a GPU (csrc/sn_aa_plan.h): a host compiler takes the header as it is, and the
stand-alone program tests/c/aa_plan_check.cpp checks it -- geometry against numbers and step lists against lines written out by
hand, invariants over every accepted combination of options, the chunk size, every refusal of the option structs -- once plain
and once under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc")


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_matches_numbers_and_lines_written_out_by_hand(tmp_path, sanitized):
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else []
    exe = str(tmp_path / ("aa_plan_check" + ("_san" if sanitized else "")))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC, *extra,
                           os.path.join(ROOT, "tests", "c", "aa_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-3000:], r.stderr[-2000:])
