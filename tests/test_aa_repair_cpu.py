"""The rank repair of the anti-aliasing call, the parts that need no GPU: the ABI of sn_aa_repair and the three new symbols,
the refusals made before a device is touched, the plan with the stage (tests/c/aa_repair_plan_check.cpp on the host
compiler), the numpy model (tests/repair_model.py) pinned by answers written out by hand, the selection the kernel uses walked
over every 0-1 input, and the conditions that keep the GPU tests from passing trivially: on frame 0 of every row every repaired
plane has samples clamped to each bound, and frame 0 of every kernel launch holds samples below, above and within."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNomAA, SangNomAAHost, SangNomError, capi, clip_format
from tests import fields_cases as fc
from tests import repair_cases as rc
from tests.repair_model import repair_bounds, repair_model, repair_plane
from tests.util import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avisynth_sangnom2_amd", "csrc")
NAMES = ("sn_aa_create_ex7", "sn_aa_get_repair", "sn_repair_device")
RANKS = (1, 2, 3, 4)


def _cfg(**kw):
    base = dict(struct_size=ctypes.sizeof(capi.SnConfig), width=64, height=32, bytes_per_sample=1, bits_per_sample=8, num_planes=1, sub_w=0,
                sub_h=0, order=1, aa=48, aac=0, dh=0, luma=1, chroma=1, device=0, max_batch=1, mode=0, host_depth=0, isolated_planes=0,
                fresh_pool=0, stream=None)
    base.update(kw)
    return capi.SnConfig(**base)


# ---- ABI -------------------------------------------------------------------------------------------------------------------------

def test_sn_aa_repair_as_a_c_compiler_lays_it_out(tmp_path):
    src = tmp_path / "layout.c"
    fields = ("struct_size", "rank", "chroma", "reserved")
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sangnom_hip.h"\n'
                   'int main(void) { printf("%d ' + "%d " * len(fields) + '\\n", (int)sizeof(sn_aa_repair), '
                   + ", ".join(f"(int)offsetof(sn_aa_repair, {f})" for f in fields) + "); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    assert [int(x) for x in out] == [32, 0, 4, 8, 12]
    M = capi.SnAARepair
    assert ctypes.sizeof(M) == 32
    assert [getattr(M, f).offset for f in fields] == [0, 4, 8, 12]
    s = capi.aa_repair(3, True)
    assert (s.struct_size, s.rank, s.chroma, list(s.reserved)) == (32, 3, 1, [0] * 5)
    assert (capi.aa_repair().rank, capi.aa_repair(None, True).rank, capi.aa_repair(0).rank) == (0, 0, 0)
    for bad in (-1, 5, 2.0, "2", True):
        with pytest.raises(ValueError):
            capi.aa_repair(bad)


def test_the_three_symbols_are_declared_exported_and_mirrored(hip_lib):
    header = open(os.path.join(ROOT, "include", "sangnom_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared"
        assert hasattr(hip_lib, name), f"libsangnom_hip.so does not export {name}"
        assert name in capi.EXPORTS + capi.EXPORTS_NUMBERED and getattr(hip_lib, name).argtypes, f"capi.py does not mirror {name}"
    assert hip_lib.sn_abi_version() == 4
    assert re.search(r"#define SN_ABI_VERSION 4\b", header)
    assert "launch_repair" in open(os.path.join(CSRC, "sn_internal.h")).read()
    assert "sn_repair.hip" in open(os.path.join(CSRC, "Makefile")).read()


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def _create(hip_lib, cfg, repair, aopt=None):
    h = ctypes.c_void_p()
    rc_ = hip_lib.sn_aa_create_ex7(ctypes.byref(cfg), None, None, ctypes.byref(aopt) if aopt is not None else None, None, None, None, None,
                                   ctypes.byref(repair) if repair is not None else None, ctypes.byref(h))
    assert not h.value
    return rc_, hip_lib.sn_aa_last_error(None).decode()


def _repair(**kw):
    base = dict(struct_size=ctypes.sizeof(capi.SnAARepair), rank=2, chroma=0)
    base.update(kw)
    return capi.SnAARepair(**base)


@pytest.mark.parametrize("kw,field", [(dict(struct_size=28), "struct_size"), (dict(struct_size=0), "struct_size"), (dict(struct_size=28, rank=0), "struct_size"),
                                      (dict(rank=-1), "rank"), (dict(rank=5), "rank"), (dict(chroma=2), "chroma"), (dict(chroma=-1), "chroma")])
def test_a_bad_struct_is_refused_naming_the_field(hip_lib, kw, field):
    code, msg = _create(hip_lib, _cfg(), _repair(**kw))
    assert code == capi.SN_ERR_INVALID_ARG and "sn_aa_repair." + field in msg, msg


def test_reserved_words_and_the_source_size_rule(hip_lib):
    for word in range(5):
        s = _repair()
        s.reserved[word] = 1
        code, msg = _create(hip_lib, _cfg(), s)
        assert code == capi.SN_ERR_INVALID_ARG and "sn_aa_repair.reserved" in msg
    for rank in RANKS:
        code, msg = _create(hip_lib, _cfg(dh=1), _repair(rank=rank, chroma=rank & 1))
        assert code == capi.SN_ERR_CONFIG
        assert msg == "SangNomAA: repair needs the frame at source size (dh=false, or dh=true with reduce)"
    # with a reduction, and with rank 0 and junk in the other words, the call gets as far as the device (or succeeds where there is one)
    off = _repair(rank=0, chroma=7)
    off.reserved[3] = 9
    for cfg, repair, aopt in ((_cfg(dh=1), _repair(rank=4, chroma=1), capi.aa_options("halfband")), (_cfg(dh=1), _repair(), capi.aa_options("tent")),
                              (_cfg(dh=1), off, None), (_cfg(), off, None)):
        h = ctypes.c_void_p()
        code = hip_lib.sn_aa_create_ex7(ctypes.byref(cfg), None, None, ctypes.byref(aopt) if aopt is not None else None, None, None, None, None,
                                        ctypes.byref(repair), ctypes.byref(h))
        assert code in (capi.SN_OK, capi.SN_ERR_HIP, capi.SN_ERR_NO_DEVICE), hip_lib.sn_aa_last_error(None).decode()
        if h.value:
            hip_lib.sn_aa_destroy(h)
    assert hip_lib.sn_aa_get_repair(None, ctypes.byref(_repair())) == capi.SN_ERR_INVALID_ARG
    assert hip_lib.sn_repair_device(None, 1, 1, None, 0, 0, None, 0, 0, 1, 1, None, 0, 0) == capi.SN_ERR_INVALID_ARG


@pytest.mark.parametrize("cls", [SangNomAA, SangNomAAHost])
def test_the_filters_take_the_keywords(hip_lib, cls):
    clip = clip_format("YUV420P8", 128, 64)
    with pytest.raises(SangNomError) as e:
        cls(clip, dh=True, repair=2, repair_chroma=True)
    assert e.value.code == capi.SN_ERR_CONFIG and "repair needs the frame at source size" in str(e.value)
    with pytest.raises(ValueError):
        cls(clip, repair=5)


# ---- the plan ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
def test_the_plan_with_repair_on_the_host_compiler(tmp_path, sanitized):
    extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else []
    exe = str(tmp_path / ("aa_repair_plan_check" + ("_san" if sanitized else "")))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC, *extra,
                           os.path.join(ROOT, "tests", "c", "aa_repair_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-3000:], r.stderr[-2000:])


def test_the_existing_host_checks_still_build_against_the_changed_headers(tmp_path):
    """Every tests/c/*.cpp from before, compiled (not run: their own tests run them) with the flags their tests use."""
    files = sorted(f for f in glob.glob(os.path.join(ROOT, "tests", "c", "*.cpp")) if not f.endswith("aa_repair_plan_check.cpp"))
    assert len(files) >= 7
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")  # (some of them reach hip_runtime.h's types through sn_internal.h)
    for f in files:
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                               "-I", os.path.join(ROOT, "include"), "-I", CSRC, f])


# ---- the model, pinned by hand ---------------------------------------------------------------------------------------------------

def _plane(rows, dtype=np.uint8):
    return np.array(rows, dtype)


@pytest.mark.parametrize("dtype,scale", [(np.uint8, 1), (np.uint16, 257), (np.float32, 1 / 256)])
def test_nine_distinct_values_by_hand(dtype, scale):
    """S = 10 .. 90.  The centre sees all nine: [a[k], a[10 - k]] = [10 k, 100 - 10 k].  The corner (0, 0) sees, with the
    clamp, 10 four times, 20 and 40 twice each and 50: 10 10 10 10 20 20 40 40 50."""
    S = (_plane([[10, 20, 30], [40, 50, 60], [70, 80, 90]], np.float64) * scale).astype(dtype)
    v = lambda x: np.array(x * scale).astype(dtype)
    corner = {1: (10, 50), 2: (10, 40), 3: (10, 40), 4: (10, 20)}
    for rank in RANKS:
        lo, hi = repair_bounds(S, rank)
        assert (lo[1, 1], hi[1, 1]) == (v(10 * rank), v(100 - 10 * rank))
        assert (lo[0, 0], hi[0, 0]) == (v(corner[rank][0]), v(corner[rank][1]))
        for r, want_c, want_0 in ((5, 10 * rank, 10), (50, 50, None), (95, 100 - 10 * rank, corner[rank][1])):
            R = np.full((3, 3), v(r), dtype)
            out = repair_plane(S, R, rank, 16)
            assert out.dtype == dtype and out[1, 1] == v(want_c)
            if want_0 is not None:
                assert out[0, 0] == v(want_0)
        # inside at the corner: 30 lies within [10, 40] and [10, 50], and above [10, 20]
        assert repair_plane(S, np.full((3, 3), v(30), dtype), rank, 16)[0, 0] == v(30 if rank < 4 else 20)


def test_ties_by_hand():
    S = np.full((4, 5), 7, np.uint8)
    for rank in RANKS:
        for r in (0, 7, 255):
            assert (repair_plane(S, np.full((4, 5), r, np.uint8), rank) == 7).all()
    # five equal values: 1 2 5 5 5 5 5 8 9
    S = _plane([[5, 5, 5], [5, 5, 1], [2, 8, 9]])
    want = {1: (1, 9), 2: (2, 8), 3: (5, 5), 4: (5, 5)}
    for rank in RANKS:
        lo, hi = repair_bounds(S, rank)
        assert (lo[1, 1], hi[1, 1]) == want[rank]
        assert repair_plane(S, np.zeros((3, 3), np.uint8), rank)[1, 1] == want[rank][0]
        assert repair_plane(S, np.full((3, 3), 200, np.uint8), rank)[1, 1] == want[rank][1]
        assert repair_plane(S, np.full((3, 3), 5, np.uint8), rank)[1, 1] == 5


def test_planes_narrower_than_the_window_by_hand():
    """1 x 1: nine times the one sample.  1 x 3 (10 20 30): column 0 sees 10 six times and 20 three times, column 1 each value
    three times, column 2 20 three times and 30 six times."""
    for rank in RANKS:
        for r in (0, 42, 200):
            assert repair_plane(_plane([[42]]), _plane([[r]]), rank)[0, 0] == 42
    S = _plane([[10, 20, 30]])
    want = {1: [(10, 20), (10, 30), (20, 30)], 2: [(10, 20), (10, 30), (20, 30)], 3: [(10, 20), (10, 30), (20, 30)], 4: [(10, 10), (20, 20), (30, 30)]}
    for rank in RANKS:
        assert repair_plane(S, _plane([[0, 0, 0]]), rank).tolist() == [[lo for lo, _ in want[rank]]]
        assert repair_plane(S, _plane([[255, 255, 255]]), rank).tolist() == [[hi for _, hi in want[rank]]]
        assert repair_plane(S, _plane([[15, 15, 25]]), rank).tolist() == [[15, 15, 25] if rank < 4 else [10, 20, 30]]
    # and a column: 3 x 1
    assert repair_plane(S.T.copy(), _plane([[0], [0], [0]]), 4).tolist() == [[10], [20], [30]]


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_nan_infinities_and_negative_zero_by_hand():
    f = np.float32
    # a NaN in S: every sample that sees it keeps R bit for bit -- at the centre of a 3 x 3 plane that is every sample
    S = np.arange(9, dtype=f).reshape(3, 3)
    S[1, 1] = np.nan
    R = np.full((3, 3), 100, f)
    R[2, 2] = -0.0
    for rank in RANKS:
        assert np.array_equal(_bits(repair_plane(S, R, rank)), _bits(R))
    # ... in a 5 x 5 plane only the samples within one of it
    S = np.arange(25, dtype=f).reshape(5, 5)
    S[0, 0] = np.nan
    out = repair_plane(S, np.full((5, 5), 100, f), 1)
    assert (out[:2, :2] == 100).all() and (np.delete(out, [0, 1], 0) < 100).all() and (np.delete(out, [0, 1], 1) < 100).all()
    # a NaN in R comes back with its payload, whatever S holds
    S = np.arange(9, dtype=f).reshape(3, 3)
    R = np.full((3, 3), -5, f)
    R.view(np.uint32)[1, 1] = 0xFFC01234
    R.view(np.uint32)[0, 2] = 0x7F800001
    out = repair_plane(S, R, 2)
    assert _bits(out)[1, 1] == 0xFFC01234 and _bits(out)[0, 2] == 0x7F800001 and out[0, 0] == 0 and out[2, 2] == 5  # the nine at (2, 2): 4 5 5 7 7 8 8 8 8
    # infinities are ordinary values
    S = np.arange(9, dtype=f).reshape(3, 3)
    S[1, 1], S[0, 0] = np.inf, -np.inf
    hi = {1: np.inf, 2: 8, 3: 7, 4: 6}
    lo = {1: -np.inf, 2: 1, 3: 2, 4: 3}
    for rank in RANKS:
        assert repair_plane(S, np.full((3, 3), np.inf, f), rank)[1, 1] == hi[rank]
        assert repair_plane(S, np.full((3, 3), -np.inf, f), rank)[1, 1] == lo[rank]
        assert repair_plane(S, np.full((3, 3), 1e30, f), rank)[1, 1] == (f(1e30) if rank == 1 else hi[rank])
        assert not np.isnan(repair_plane(S, np.full((3, 3), 4.5, f), rank)).any()
    # -0.0 as a bound is written as +0.0; R = -0.0 or +0.0 inside [-0.0, +0.0] keeps its bits
    S = np.full((3, 3), -0.0, f)
    for rank in RANKS:
        assert (_bits(repair_plane(S, np.full((3, 3), -1, f), rank)) == 0).all()
        assert (_bits(repair_plane(S, np.full((3, 3), 1, f), rank)) == 0).all()
        assert (_bits(repair_plane(S, np.full((3, 3), -0.0, f), rank)) == 0x80000000).all()
        assert (_bits(repair_plane(S, np.zeros((3, 3), f), rank)) == 0).all()
        assert (_bits(repair_plane(np.zeros((3, 3), f), np.full((3, 3), -0.0, f), rank)) == 0x80000000).all()
    S = np.where(np.arange(9).reshape(3, 3) % 2 == 0, f(-0.0), f(0.0)).astype(f)  # zeros of both signs around: still one value
    assert (_bits(repair_plane(S, np.full((3, 3), -0.0, f), 1)) == 0x80000000).all()
    assert (_bits(repair_plane(S, np.full((3, 3), -1e-30, f), 3)) == 0).all()


def test_chroma_and_processed_select_the_planes():
    rng = np.random.default_rng(5)
    fr = [rng.integers(0, 256, (8, 8)).astype(np.uint8) for _ in range(3)]
    res = [rng.integers(0, 256, (8, 8)).astype(np.uint8) for _ in range(3)]
    full = [repair_plane(s, r, 2) for s, r in zip(fr, res)]
    assert all(not same(a, b) for a, b in zip(full, res))
    got = repair_model(fr, res, 2, False)
    assert same(got[0], full[0]) and got[1] is res[1] and got[2] is res[2]
    got = repair_model(fr, res, 2, True)
    assert all(same(a, b) for a, b in zip(got, full))
    got = repair_model(fr, res, 2, True, processed=[False, True, True])
    assert got[0] is res[0] and same(got[1], full[1]) and same(got[2], full[2])
    # rank 1 leaves a copy of the source alone; ranks 2..4 pull in its extremes
    assert same(repair_plane(fr[0], fr[0], 1), fr[0]) and not same(repair_plane(fr[0], fr[0], 2), fr[0])


# ---- the kernel's selection ------------------------------------------------------------------------------------------------------

def _bounds_as_the_kernel_takes_them(v, rank):
    """bounds_of() of csrc/sn_repair.hip: three columns sorted in themselves, then the places a[k] can be."""
    cols = [sorted((v[0][c], v[1][c], v[2][c])) for c in range(3)]
    L, M, H = (sorted(c[i] for c in cols) for i in range(3))
    if rank == 1:
        return L[0], H[2]
    if rank == 2:
        return min(L[1], M[0]), max(H[1], M[2])
    q, p = max(L[1], M[0]), min(H[1], M[2])
    if rank == 3:
        return min(q, L[2], H[0]), max(p, H[0], L[2])
    u, w = min(L[2], H[0]), max(L[2], H[0])
    return min(max(u, q), w, M[1]), max(min(w, p), u, M[1])


def test_the_kernels_selection_on_every_zero_one_input():
    """A network of minima and maxima that selects a[k] on every 0-1 input selects it on every input."""
    for word in range(512):
        f = [(word >> i) & 1 for i in range(9)]
        a = sorted(f)
        for rank in RANKS:
            assert _bounds_as_the_kernel_takes_them([f[0:3], f[3:6], f[6:9]], rank) == (a[rank - 1], a[9 - rank]), (word, rank)
    text = open(os.path.join(CSRC, "sn_repair.hip")).read()
    for line in ("a[2] = min(L1, M0)", "a[3] = min(max(L1, M0), L2, H0)", "a[4] = min(max(u, max(L1, M0)), v, M1)", "a[6] = max(min(v, min(H1, M2)), u, M1)"):
        assert line in text


def test_the_float_keys_order_as_less_than_does():
    """The kernel stages float samples as keys (sign-magnitude to two's complement): the order of the keys is the order of <, both
    zeros are one key, key 0 decodes to +0.0 and a NaN lies beyond either infinity."""
    def key(bits):
        m = int(bits) & 0x7FFFFFFF
        return -m if int(bits) >> 31 else m
    def back(k):
        return (0x80000000 - k) & 0xFFFFFFFF if k < 0 else k
    vals = np.array([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], np.float32)
    keys = [key(b) for b in vals.view(np.uint32)]
    assert keys == sorted(keys) and keys[3] == keys[4] == 0 and back(0) == 0
    for b, k in zip(vals.view(np.uint32), keys):
        assert back(k) == int(b) or k == 0
    inf = 0x7F800000
    assert all(abs(key(b)) > inf for b in (0x7F800001, 0x7FC00000, 0xFFC01234, 0xFFFFFFFF)) and abs(keys[0]) == inf == keys[-1]


# ---- the frames of the GPU tests -------------------------------------------------------------------------------------------------

def _tile():
    m = re.search(r"kRepairTileBytes = (\d+), kRepairTileH = (\d+);", open(os.path.join(CSRC, "sn_repair.hip")).read())
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("fmt", ["Y8", "Y10", "Y16", "Y32"])
def test_frame_0_of_every_kernel_launch_holds_every_class(fmt):
    clip = clip_format(fmt, 64, 32)
    tile_bytes, th = _tile()
    assert (tile_bytes, th) == (256, 16)
    for si, (W, H) in enumerate(rc.kernel_shapes(clip.bytes, tile_bytes, th)):
        if W <= 8 or H <= 8:
            continue
        S, R = rc.kernel_patterns(clip, W, H, seed=5000 + si)[0]
        for rank in RANKS:
            below, above, inside = rc.classes(S, R, rank)
            print(f"{fmt} {W}x{H} rank {rank}: below {below:.3f} above {above:.3f} inside {inside:.3f}")
            assert below > 0 and above > 0 and inside > 0


@pytest.mark.parametrize("i", range(len(rc.ROWS)), ids=[f"{c[0]}-{c[1]}x{c[2]}-{i}" for i, c in enumerate(rc.ROWS)])
def test_on_frame_0_of_every_row_every_repaired_plane_is_clamped_to_each_bound(i):
    """Without dh and with dh and a reduction, ranks 1 and 3, every processed plane: at least one sample of the result lies
    below a[rank] and one above a[10 - rank], and the repaired frame differs from the unrepaired one -- alone, and behind the
    sharpening too."""
    case = rc.ROWS[i]
    chroma = rc.chromas_of(case)[-1]  # every plane the GPU tests repair
    for form in rc.forms_of(case):
        frames, _, res = rc.unmasked(case, form, 1, rc.first_of(case))
        repaired = rc.repaired_planes(case, form, chroma)
        assert any(repaired)
        for sharpen in (None, (rc.AMOUNT, True)):
            for rank in rc.RANKS:
                _, _, plain, want = rc.expected(case, form, rank, chroma, sharpen=sharpen, count=1)
                for p, (S, R) in enumerate(zip(frames[0], plain[0])):
                    if not repaired[p]:
                        assert same(want[0][p], plain[0][p])
                        continue
                    below, above, _ = rc.classes(S, R, rank)
                    print(f"{case[0]} {case[1]}x{case[2]} form {form} sharpen {sharpen} rank {rank} plane {p}: below {below:.4f} above {above:.4f}")
                    assert below > 0 and above > 0, f"form {form} sharpen {sharpen} rank {rank} plane {p}: below {below}, above {above}"
                    assert not same(want[0][p], plain[0][p])
        assert same(res[0][0], rc.expected(case, form, 0, False, count=1)[3][0][0])  # rank 0: the unmasked frame


@pytest.mark.parametrize("i", rc.BOTH_ROWS)
def test_the_both_fields_rows_are_clamped_to_each_bound_too(i):
    for rank in rc.RANKS:
        frames, plain, want = rc.expected_both(i, rank, True)
        assert len(frames[0]) == 1 or fc.CASES[i].kw.get("aac")
        for p in range(len(frames[0])):
            assert not same(want[0][p], plain[0][p]), f"row {i} rank {rank} plane {p}: the expected plane is the unrepaired one"
