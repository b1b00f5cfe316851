"""Every wave count and every right-edge lane of the fused sweeps, bit-exact against the CPU oracle.

A fused sweep kernel is a template over its wave count, and the wave count follows from the plane's width alone
(tests/sweep_geometry_cases.py restates the formula and derives the widths below from it; tests/test_sweep_geometry_cpu.py
checks that table).  Each (wave count, mode, arithmetic) is a kernel of its own -- registers, LDS size, seam mailbox -- so
every one of them is launched here at the narrowest and the widest plane it takes:

  a  planes on their own at both ends of every strip count, all three sample types
  b  the last column on every lane it can take in a first, a second and a third wave (16-bit, float, 4:4:4)
  c  the pool-coupled sweeps of 4:2:0 / 4:2:2 clips with 5, 6 and (8-bit) 7 waves; U and V as one sweep with 5, 6, 7
  d  padded sweeps of fresh pools whose lines end 1 .. 3 lanes before the sweep does -- in its last strip or in the one before
  e  row loops that end at every position of the five-row seam block
  f  one, two, ... nine frames in workgroups that hold four or two of them
  g  the SSE2 arithmetic's instances at the narrowest plane of every strip count

Every context is created with mode="fused" (no pool path behind it), and every case asserts that the sweeps served all of
its frames.  One test id is one width or shape; its patterns run inside.
"""
import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2, clip_format
from oracle.oracle import Oracle
from tests import sse2_sweep_cases as sc
from tests import sweep_geometry_cases as gc
from tests.util import describe_diff, oracle_cfg, same, to_host

pytestmark = pytest.mark.gpu

TYPES = ("Y8", "Y16", "Y32")
TIES = {"Y8": "near-flat", "Y16": "near-flat", "Y32": "eighths"}  # the type's tie-heavy pattern
FILL = 0x5C
VIEW = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits as int16


def _served(flt, nframes):
    i = flt.info()
    assert i.fused_eligible == 1 and i.fused_frames == nframes and i.banded_frames == 0, \
        f"the sweeps did not serve these frames: eligible {i.fused_eligible}, fused {i.fused_frames} of {nframes}, banded {i.banded_frames}"
    return i


def _check(fmt, w, h, kw, pattern, nframes=2, **policy):
    """nframes host frames, parities 0, 1, ..., against one oracle instance."""
    clip = clip_format(fmt, w, h)
    ora = Oracle(oracle_cfg(clip, **kw))
    with SangNom2(clip, mode="fused", **policy, **kw) as flt:
        assert flt.info().fused_eligible == 1
        for f, src in enumerate(gc.frames(clip, pattern, nframes)):
            want = ora.process(src, parity=f & 1)
            got = flt.get_frame(src, parity=f & 1)
            for p in range(len(want)):
                assert same(want[p], got[p]), f"{fmt} {w}x{h} {kw} {policy} {pattern} frame {f} plane {p}: " + describe_diff(want[p], got[p])
        return _served(flt, nframes)


def _device_batch(flt, clip, frames, parities, dst_frames=None, dst_pitch=None):
    """The frames of a one-plane clip as one device batch.  The destination is an allocation of FILL bytes that holds dst_frames
    frames (default: as many as the source) of rows dst_pitch samples long (default: the width); returns all of it, on the host,
    as [dst_frames, rows, dst_pitch] samples."""
    import torch
    dev, n = torch.device("cuda:0"), len(frames)
    rows, w = flt.plane_shape_out(0)
    src = torch.from_numpy(np.stack([fr[0] for fr in frames]).view(VIEW[clip.bytes])).pin_memory().to(dev)
    alloc = torch.full((dst_frames or n, rows, (dst_pitch or w) * clip.bytes), FILL, dtype=torch.uint8, device=dev).view(src.dtype)
    torch.cuda.synchronize()
    flt.process_batch([src], [alloc[:n, :, :w]], parities)
    flt.synchronize()
    return to_host(alloc).view(clip.dtype)


def _untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


# ---- a. wave counts --------------------------------------------------------------------------------------------------------

WAVE_CASES = [(t, w) for t in TYPES for w in gc.WAVE_WIDTHS[t]]


@pytest.mark.parametrize("t,w", WAVE_CASES, ids=[f"{t}-{w}" for t, w in WAVE_CASES])
def test_planes_at_both_ends_of_every_strip_count_match_oracle(hip_lib, t, w):
    for pattern in ("noise", "edges", TIES[t]):
        for aa in (48, 128):
            _check(t, w, 26, dict(order=1, aa=aa), pattern)
    if w in gc.WIDEST[t]:
        for order in (0, 2):
            _check(t, w, 26, dict(order=order, aa=48), "noise")
        for order in (0, 1, 2):
            _check(t, w, 14, dict(order=order, aa=48, dh=True), "noise")


# ---- b. the right edge -------------------------------------------------------------------------------------------------------

EDGE_PATTERNS = {"Y16": ("noise", "flat", "near-flat"), "YUV444P16": ("noise", "flat", "near-flat"), "Y32": ("noise", "negzero", "small")}


@pytest.mark.parametrize("w", gc.EDGE_WIDTHS)
@pytest.mark.parametrize("fmt", list(EDGE_PATTERNS))
def test_last_column_on_every_lane_matches_oracle(hip_lib, fmt, w):
    kw = dict(order=1, aa=48, aac=48) if fmt == "YUV444P16" else dict(order=1, aa=48)
    for pattern in EDGE_PATTERNS[fmt]:
        _check(fmt, w, 24, kw, pattern)


# ---- c. coupled sweeps -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,w,h", gc.COUPLED16, ids=[f"{c[0]}-{c[1]}" for c in gc.COUPLED16])
def test_coupled_sweeps_of_five_and_six_waves_match_oracle(hip_lib, fmt, w, h):
    for pattern in ("noise", "edges"):
        _check(fmt, w, h, dict(order=1, aa=48, aac=48), pattern)


@pytest.mark.parametrize("fmt,w,h", gc.COUPLED8, ids=[f"{c[0]}-{c[1]}" for c in gc.COUPLED8])
def test_8_bit_coupled_sweeps_of_five_six_and_seven_waves_match_oracle(hip_lib, record_property, fmt, w, h):
    """Luma, U and V as three sweeps over 9, 11 and 13 strips.  Under the default policy too: U and V as one sweep take at most
    eight strips (the next test)."""
    for pattern in ("noise", "edges"):
        info = _check(fmt, w, h, dict(order=1, aa=48, aac=48), pattern)
        record_property(f"uv_sweeps-{pattern}", info.uv_sweeps)
        info = _check(fmt, w, h, dict(order=1, aa=48, aac=48), pattern, chroma_sweeps=1)
        assert info.uv_sweeps == 0


@pytest.mark.parametrize("fmt,w,h", gc.UV_ONE_SWEEP, ids=[f"{c[0]}-{c[1]}" for c in gc.UV_ONE_SWEEP])
def test_u_and_v_as_one_sweep_of_five_six_and_seven_waves_match_oracle(hip_lib, record_property, fmt, w, h):
    for pattern in ("noise", "edges"):
        info = _check(fmt, w, h, dict(order=1, aa=48, aac=48), pattern)
        record_property(f"uv_sweeps-{pattern}", info.uv_sweeps)
        assert info.uv_sweeps == 1, "U and V did not run as one sweep"


# ---- d. padded sweeps --------------------------------------------------------------------------------------------------------

PADDED_CASES = [(t, w, s) for t in TYPES for w, s in gc.PADDED[t]]


def _fresh_want(clip, frames, parities, **kw):
    return [Oracle(oracle_cfg(clip, **kw)).process(fr, parity=par)[0] for fr, par in zip(frames, parities)]


@pytest.mark.parametrize("t,w,stride", PADDED_CASES, ids=[f"{t}-{w}of{s}" for t, w, s in PADDED_CASES])
def test_padded_sweeps_match_a_new_oracle_per_frame(hip_lib, t, w, stride):
    """fresh_pool planes a multiple of 8 and not of 32 wide, as a device batch whose destination rows are as long as the pool
    stride the sweep covers: whatever lies right of the plane stays as it was."""
    clip, parities = clip_format(t, w, 24), (1, 0, 1)
    for pattern in ("noise", "edges"):
        frames = gc.frames(clip, pattern, 3)
        want = _fresh_want(clip, frames, parities, order=1, aa=48)
        with SangNom2(clip, mode="fused", fresh_pool=True, max_batch=3, order=1, aa=48) as flt:
            assert flt.info().fused_eligible == 1 and flt.info().history_free == 1
            got = _device_batch(flt, clip, frames, parities, dst_pitch=stride)
            _served(flt, 3)
        for f in range(3):
            assert same(want[f], got[f, :, :w]), f"{t} {w} of {stride} {pattern} frame {f}: " + describe_diff(want[f], got[f, :, :w])
        assert _untouched(got[:, :, w:]), f"{t} {w} of {stride} {pattern}: columns right of the plane were written"


# ---- e. row blocks at the seams ------------------------------------------------------------------------------------------------

SEAM_CASES = [(t, w) for t in TYPES for w in gc.SEAM_WIDTHS[t]]


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("t,w", SEAM_CASES, ids=[f"{t}-{w}" for t, w in SEAM_CASES])
def test_row_loops_that_end_anywhere_in_a_seam_block_match_oracle(hip_lib, t, w, order):
    for h in gc.HEIGHTS:
        _check(t, w, h, dict(order=order, aa=48), "noise")


# ---- f. frames per workgroup ---------------------------------------------------------------------------------------------------

GROUP_CASES = [c + (False,) for c in gc.GROUPS] + [c + (True,) for c in gc.GROUPS_PADDED]


@pytest.mark.parametrize("t,w,h,fresh", GROUP_CASES, ids=[f"{c[0]}-{c[1]}" + ("-padded" if c[3] else "") for c in GROUP_CASES])
def test_batches_that_fill_and_do_not_fill_their_workgroups_match_oracle(hip_lib, t, w, h, fresh):
    """Four one-wave planes or two two-wave planes share a workgroup, and a workgroup's frame index past the end repeats the last
    frame: every frame of a batch against its own result, and the frame behind the batch's last one untouched."""
    clip = clip_format(t, w, h)
    for n in gc.GROUP_FRAMES:
        frames = gc.frames(clip, "noise", n)
        parities = [(f + 1) & 1 for f in range(n)]
        if fresh:
            want = _fresh_want(clip, frames, parities, order=1, aa=48)
        else:
            ora = Oracle(oracle_cfg(clip, order=1, aa=48))
            want = [ora.process(fr, parity=par)[0] for fr, par in zip(frames, parities)]
        with SangNom2(clip, mode="fused", fresh_pool=fresh, max_batch=n, order=1, aa=48) as flt:
            got = _device_batch(flt, clip, frames, parities, dst_frames=n + 1)
            _served(flt, n)
        for f in range(n):
            assert same(want[f], got[f]), f"{t} {w}x{h} batch of {n}, frame {f}: " + describe_diff(want[f], got[f])
        assert _untouched(got[n]), f"{t} {w}x{h} batch of {n}: the frame behind the last one was written"


# ---- g. SSE2 arithmetic ----------------------------------------------------------------------------------------------------------

SSE2_CASES = [(t, w) for t in ("Y8", "Y16") for w in gc.NARROWEST[t]]


@pytest.mark.parametrize("t,w", SSE2_CASES, ids=[f"{t}-{w}" for t, w in SSE2_CASES])
def test_sse2_instances_at_the_narrowest_plane_of_every_strip_count_match_the_model(hip_lib, t, w):
    """opt=1 with sse2_sweeps=1 against the numpy model of the reference's SSE2 path; sc.expected asserts first that the default
    arithmetic gives something else on this input."""
    clip, frames, parities, want = sc.expected(t, w, 16, {}, {}, 1, "noise01")
    with SangNom2(clip, mode="fused", opt=1, sse2_sweeps=1) as flt:
        assert flt.info().fused_eligible == 1
        got = flt.get_frame(frames[0], parity=parities[0])
        assert same(want[0][0], got[0]), f"{t} {w}x16: " + describe_diff(want[0][0], got[0])
        _served(flt, 1)
