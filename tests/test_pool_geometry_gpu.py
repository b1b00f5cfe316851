"""Stage 2 of the pool path and its chains at every strip count, right-edge lane, row phase, wave count and workgroup count,
bit-exact against the reference in pools and pixels (float on bit patterns).

The pool path (csrc/sn_pool_kernels.hip) is what every redo and every clip the sweeps do not serve lands on, and the yardstick
of the "fused equals pool" tests.  Its stage 2 is fifteen kernels of a plane behind three schedules and twelve chain kernels,
each written out on its own; tests/pool_geometry_cases.py derives from the dispatch rules a table that launches every one of them
at the ends of its geometry, and tests/test_pool_geometry_cpu.py proves that table without a GPU.

Pixels alone are a blunt check here: stage 3 keeps an arg-min and a threshold, so a slightly wrong smoothed cost can leave the
picture as it is -- most of all in columns w .. stride - 1 and rows 0 and bh, which only the next frame sees.  So every case
compares the pool itself (sn_debug_read_pool: all nine buffers, rows 0 .. bh, columns up to the stride) after every frame or launch.

Every context has mode="pool"; one context per case; no test hook but sn_debug_read_pool, no environment variable.
"""
import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom2
from tests import pool_geometry_cases as gc
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

VIEW = {1: np.uint8, 2: np.int16, 4: np.float32}  # torch has no uint16: same bits as int16


def _context(c, clip):
    kw = dict(opt=1, sse2_sweeps=0) if c.opt else {}  # sse2_sweeps = 0: the pool kernels serve the saturating arithmetic
    return SangNom2(clip, mode="pool", max_batch=max(c.launch, 1), order=c.order, aa=c.aa, chain=c.chain, **kw)


def _pool_diff(want, got):
    idx = np.argwhere(want.view(np.uint32) != got.view(np.uint32)) if want.dtype == np.float32 else np.argwhere(want != got)
    return f"{len(idx)} differing cells, first (buffer, row, column) {idx[:6].tolist()}"


def _launch(flt, clip, frames, parities):
    """One process_batch launch of device-resident frames; the output frames on the host."""
    import torch
    dev = torch.device("cuda:0")
    src = torch.from_numpy(np.stack([fr[0] for fr in frames]).view(VIEW[clip.bytes])).pin_memory().to(dev)
    dst = torch.zeros((len(frames),) + flt.plane_shape_out(0), dtype=src.dtype, device=dev)
    torch.cuda.synchronize()
    flt.process_batch([src], [dst], parity=list(parities))
    flt.synchronize()
    return to_host(dst).view(clip.dtype)


def _geometry(flt, c):
    i = flt.info()
    assert i.pool_stride == gc.stride_of(c) and i.pool_rows == gc.bh(c.h) + 1, (i.pool_stride, i.pool_rows)
    assert i.fused_frames == 0 and i.banded_frames == 0, (i.fused_frames, i.banded_frames)
    return i


def _run_plane_case(c):
    """Frames one by one through get_frame (pool 0 after every frame), or one launch of c.launch frames of a history-free clip: frame
    f of such a launch runs on pool slot f, sn_debug_read_pool serves every slot of the launch, and each is compared -- with one
    reference instance fed in order, whose pool after frame f is what a slot that started from zeros holds (every cell but rows 0
    and bh, which stay zero, is written anew)."""
    clip, cid = gc.clip_of(c), gc.case_id(c)
    ref = gc.reference_of(c)
    frames = gc.frames_of(c)[0]
    want = [gc.reference_frame(ref, c, src, 1) for src in frames]
    with _context(c, clip) as flt:
        _geometry(flt, c)
        if c.launch:
            assert clip.width % 32 == 0 and flt.info().history_free == 1
            got = _launch(flt, clip, frames, c.parities)
            for f, (out, pool) in enumerate(want):
                got_pool = flt.read_pool(f)
                assert same(pool, got_pool), f"{cid} pool of frame {f}: " + _pool_diff(pool, got_pool)
                assert same(out, got[f]), f"{cid} frame {f}: " + describe_diff(out, got[f])
        else:
            for f, (src, (out, pool)) in enumerate(zip(frames, want)):
                got = flt.get_frame(src, parity=1)[0]
                got_pool = flt.read_pool(0)
                assert same(pool, got_pool), f"{cid} pool after frame {f}: " + _pool_diff(pool, got_pool)
                assert same(out, got), f"{cid} frame {f}: " + describe_diff(out, got)
        i = _geometry(flt, c)
        assert i.chained_frames == 0 and i.frames == len(frames)


def _ids(cases):
    return [gc.case_id(c) for c in cases]


@pytest.mark.parametrize("c", gc.STRIPS, ids=_ids(gc.STRIPS))
def test_strips_at_both_ends_of_every_strip_count(hip_lib, c):
    _run_plane_case(c)


@pytest.mark.parametrize("c", gc.EDGE, ids=_ids(gc.EDGE))
def test_last_lane_on_every_position_of_the_second_and_third_strip(hip_lib, c):
    _run_plane_case(c)


@pytest.mark.parametrize("c", gc.ROWS, ids=_ids(gc.ROWS))
def test_row_loops_that_end_at_every_phase(hip_lib, c):
    _run_plane_case(c)


@pytest.mark.parametrize("c", gc.X8, ids=_ids(gc.X8))
def test_x8_with_a_partly_idle_last_wave_and_on_both_sides_of_the_lds_boundary(hip_lib, c):
    _run_plane_case(c)


@pytest.mark.parametrize("c", gc.STRIDED, ids=_ids(gc.STRIDED))
def test_strided_pools_and_planes_around_the_blocks_of_stages_1_and_3(hip_lib, c):
    _run_plane_case(c)


@pytest.mark.parametrize("c", gc.SSE2, ids=_ids(gc.SSE2))
def test_saturating_instances_match_the_model(hip_lib, c):
    _run_plane_case(c)


@pytest.mark.parametrize("c", gc.CHAIN, ids=_ids(gc.CHAIN))
def test_chains_at_every_strip_count_and_workgroup_count(hip_lib, c):
    """Two launches on one context, the second from the first's pool; every frame of both and the final pool against one reference
    instance fed in order.  chained_frames is exact (0 for the strides the chain refuses).  Over several workgroups per buffer
    chain_redone must stay 0: a redone launch has its grouped result replaced, and the case would prove nothing."""
    clip, cid = gc.clip_of(c), gc.case_id(c)
    ref = gc.reference_of(c)
    with _context(c, clip) as flt:
        _geometry(flt, c)
        assert flt.info().history_free == 0 and flt.get_policy().chain == c.chain
        pool = None
        for launch, frames in enumerate(gc.frames_of(c)):
            want = [gc.reference_frame(ref, c, src, par) for src, par in zip(frames, c.parities)]
            got = _launch(flt, clip, frames, c.parities)
            for f, (out, pool) in enumerate(want):
                assert same(out, got[f]), f"{cid} launch {launch} frame {f}: " + describe_diff(out, got[f])
        got_pool = flt.read_pool(0)
        assert same(pool, got_pool), f"{cid} final pool: " + _pool_diff(pool, got_pool)
        i = _geometry(flt, c)
        assert i.chained_frames == gc.chained_frames(c), (i.chained_frames, gc.chained_frames(c))
        assert i.frames == 2 * c.launch
        if c.chain > 1:
            assert i.chain_redone == 0, f"{cid}: {i.chain_redone} launches were redone on one workgroup per buffer"
