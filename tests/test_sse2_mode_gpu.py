"""The SSE2 arithmetic mode (sn_options.arithmetic = SN_ARITH_SSE2; `opt=1` in the Python mirror) on the GPU.

Everything is bit-exact, tolerance zero.  Two references:
* the reference's own opt=1 / opt=0 outputs stored in tests/golden/sse2_*.npz (SSE2_FIXTURES.md);
* tests/sse2_model.py, the numpy model that reproduces those fixtures (tests/test_sse2_fixtures_cpu.py), on wider ground.
Inputs are 2x2 checkers of 0/MAXT, 0/MAXT noise and full-range noise; every 8-bit and 16-bit case also asserts that the
model's output differs from the opt=0 oracle's, so a case on which the mode cannot be told from the default fails.
"""
import ctypes

import numpy as np
import pytest

from avisynth_sangnom2_amd import SangNom, SangNom2, SangNomAA, SangNomAAHost, SangNomError, capi, clip_format, synth
from oracle.sangnom_numpy import NumpySangNom
from tests import sse2_model as sm
from tests.util import describe_diff, same, to_host

pytestmark = pytest.mark.gpu

NAMES = sm.fixture_names()


def _clip(meta):
    return clip_format(meta["fmt"], meta["width"], meta["height"])


def _assert_frames(want, got, what):
    for p, (a, b) in enumerate(zip(want, got)):
        assert same(a, b), f"{what} plane {p}: " + describe_diff(a, b)


# ---- the reference's own outputs -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["auto", "pool"])
@pytest.mark.parametrize("name", NAMES)
def test_fixture_through_process_host(hip_lib, name, mode):
    meta, frames, out1, _ = sm.load_fixture(name)
    with SangNom2(_clip(meta), opt=1, mode=mode, **meta["kw"]) as flt:
        assert hip_lib.sn_get_arithmetic(flt._h) == capi.SN_ARITH_SSE2
        for f, src in enumerate(frames):
            _assert_frames(out1[f], flt.get_frame(src, parity=meta["parity"][f]), f"{name} frame {f}")


@pytest.mark.parametrize("name", NAMES)
def test_fixture_through_process_device_strided(hip_lib, name):
    import torch
    meta, frames, out1, _ = sm.load_fixture(name)
    clip, n, dev = _clip(meta), meta["nframes"], torch.device("cuda:0")
    vt = {1: np.uint8, 2: np.int16, 4: np.float32}[clip.bytes]  # torch has no uint16: same bits
    with SangNom2(clip, opt=1, max_batch=n, **meta["kw"]) as flt:
        src = [torch.from_numpy(np.stack([fr[p] for fr in frames]).view(vt)).pin_memory().to(dev) for p in range(clip.planes)]
        dst = [torch.zeros((n,) + flt.plane_shape_out(p), dtype=src[p].dtype, device=dev) for p in range(clip.planes)]
        torch.cuda.synchronize()
        flt.process_batch(src, dst, meta["parity"])
        flt.synchronize()
        for f in range(n):
            _assert_frames(out1[f], [to_host(dst[p][f]).view(clip.dtype) for p in range(clip.planes)], f"{name} frame {f}")


@pytest.mark.parametrize("name", NAMES)
def test_fixture_through_the_host_ring(hip_lib, name):
    meta, frames, out1, _ = sm.load_fixture(name)
    with SangNom2(_clip(meta), opt=1, host_depth=4, **meta["kw"]) as flt:
        slots = [flt.submit(src, parity=meta["parity"][f]) for f, src in enumerate(frames)]
        for f, s in enumerate(slots):
            _assert_frames(out1[f], flt.collect(s), f"{name} frame {f}")


@pytest.mark.parametrize("opt", [-1, 0])
@pytest.mark.parametrize("name", NAMES)
def test_default_mode_still_gives_the_references_opt0_output(hip_lib, name, opt):
    """opt=-1 and opt=0 are the C++ arithmetic, through the new entry point as well."""
    meta, frames, _, out0 = sm.load_fixture(name)
    with SangNom2(_clip(meta), opt=opt, **meta["kw"]) as flt:
        assert hip_lib.sn_get_arithmetic(flt._h) == capi.SN_ARITH_CXX
        for f, src in enumerate(frames):
            _assert_frames(out0[f], flt.get_frame(src, parity=meta["parity"][f]), f"{name} frame {f}")


# ---- the library against the model on wider ground ---------------------------------------------------------------------

def _frames(clip, pattern, n, seed0):
    return [synth.frame(clip, pattern, seed=seed0 + i) for i in range(n)]


def _model_kw(clip, kw):
    return dict(bytes=clip.bytes, bits=clip.bits, planes=clip.planes, subw=clip.subw, subh=clip.subh,
                order=kw.get("order", 1), aa=kw.get("aa", 48), aac=kw.get("aac", 0), dh=kw.get("dh", False))


def _plane_model(clip, kw, p):
    """The model of plane p filtered as a Y clip of its own (isolated_planes / fresh_pool)."""
    k = _model_kw(clip, kw)
    k.update(planes=1, subw=0, subh=0, aa=k["aa"] if p == 0 else k["aac"])
    return (clip.width >> (clip.subw if p else 0), clip.height >> (clip.subh if p else 0)), k


def _want(clip, kw, frames, parities, arithmetic, isolated=False, fresh=False):
    """Per frame the planes the reference would give: one instance with the shared pool, or (isolated) one instance per
    plane, or (fresh) a new instance per plane and frame."""
    out = []
    if not (isolated or fresh):
        m = sm.model_for(arithmetic, clip.width, clip.height, **_model_kw(clip, kw))
        return [m.get_frame(fr, parity=par) for fr, par in zip(frames, parities)], m
    keep = {}
    for fr, par in zip(frames, parities):
        planes = []
        for p in range(clip.planes):
            (w, h), k = _plane_model(clip, kw, p)
            if fresh or p not in keep:
                keep[p] = sm.model_for(arithmetic, w, h, **k)
            planes.append(keep[p].get_frame([fr[p]], parity=par)[0])
        out.append(planes)
    return out, None


def _differs(a_frames, b_frames):
    return any(not same(a, b) for x, y in zip(a_frames, b_frames) for a, b in zip(x, y))


WIDE = [
    # (format, width, height, filter kwargs, context kwargs, frames, pattern)
    ("Y8", 32, 24, {}, {}, 1, "noise01"),
    ("Y8", 40, 24, dict(order=2), {}, 2, "checker2"),
    ("Y8", 72, 40, dict(order=0), {}, 3, "noise01"),
    ("Y8", 100, 24, dict(aa=128), {}, 3, "noise01"),
    ("Y8", 512, 24, {}, {}, 1, "noise"),
    ("Y8", 512, 24, {}, {}, 1, "checker2"),
    ("Y8", 992, 24, dict(order=2), {}, 2, "noise01"),
    ("Y8", 1920, 32, {}, {}, 1, "noise01"),
    ("Y8", 3840, 24, {}, {}, 1, "checker2"),
    ("Y8", 3840, 24, dict(order=0), {}, 2, "noise"),
    ("Y8", 1000, 32, {}, {}, 3, "noise01"),                       # history-carrying and wide
    ("Y8", 100, 24, {}, dict(fresh_pool=True), 2, "noise01"),
    ("Y8", 256, 20, dict(dh=True), {}, 1, "noise01"),
    ("Y10", 64, 24, {}, {}, 1, "noise01"),
    ("Y10", 1920, 24, {}, {}, 1, "noise01"),
    ("Y16", 64, 24, dict(order=2), {}, 2, "checker2"),
    ("Y16", 1920, 24, {}, {}, 1, "noise01"),
    ("Y16", 600, 24, {}, {}, 1, "noise"),
    ("Y16", 104, 24, {}, {}, 3, "noise01"),                       # history-carrying
    ("YUV420P8", 128, 32, dict(aac=48), {}, 2, "noise01"),
    ("YUV420P8", 128, 32, dict(aac=48), dict(isolated_planes=True), 2, "noise01"),
    ("YUV420P8", 1024, 32, dict(aac=48), {}, 1, "noise01"),
    ("YUV420P8", 200, 32, dict(aac=48, order=0), {}, 3, "noise01"),  # history-carrying, three planes
    ("YUV422P8", 128, 24, dict(aac=48), {}, 1, "noise01"),
    ("YUV422P8", 128, 24, dict(aac=48), dict(isolated_planes=True), 1, "checker2"),
    ("YUV420P16", 128, 32, dict(aac=48), {}, 2, "noise01"),
    ("YUV420P16", 128, 32, dict(aac=48), dict(isolated_planes=True), 1, "noise01"),
    ("YUV422P16", 128, 24, dict(aac=48), {}, 1, "noise01"),
    ("YUV422P16", 128, 24, dict(aac=48), dict(isolated_planes=True), 2, "noise01"),
    ("YUV420P8", 128, 32, dict(aac=48), dict(fresh_pool=True), 2, "noise01"),
    ("YUV444P8", 64, 16, dict(aac=48, dh=True), {}, 1, "noise01"),
]
# the pools at which the pool path's stage 2 changes its kernel (csrc/sn_pool_dispatch.h; tests/test_gpu_parity.py,
# POOL_STAGE2_CASES, has the same shapes in the default arithmetic), and a 520-wide clip whose pool (stride 544) carries
# its stale columns from frame to frame
WIDE += [(fmt, w, h, {}, {}, 3, "noise") for fmt in ("Y8", "Y16")
         for w, h in ((256, 32), (480, 32), (512, 32), (544, 32), (7680, 24), (7712, 24), (8192, 24), (520, 24))]


# how a context is asked to run: whole-plane sweeps wherever the configuration has them (8-bit planes on their own, in this
# arithmetic), the library's own policy for small launches (row bands or the pool kernels), the pool kernels only
PATHS = {"sweep": dict(small_launches=capi.SN_SMALL_SWEEP), "auto": {}, "pool": dict(mode="pool")}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("fmt,w,h,kw,ckw,n,pattern", WIDE,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[6]}-{'-'.join(f'{a}{b}' for a, b in {**c[3], **c[4]}.items())}" for c in WIDE])
def test_library_matches_the_model(hip_lib, fmt, w, h, kw, ckw, n, pattern, path):
    clip = clip_format(fmt, w, h)
    frames = _frames(clip, pattern, n, seed0=300)
    parities = [(f + 1) & 1 for f in range(n)]
    isolated, fresh = bool(ckw.get("isolated_planes")), bool(ckw.get("fresh_pool"))
    want, model = _want(clip, kw, frames, parities, 1, isolated, fresh)
    if clip.bits in (8, 16):  # (9..15 bits: the two paths almost never differ on in-range samples)
        base, _ = _want(clip, kw, frames, parities, 0, isolated, fresh)
        assert _differs(want, base), "this case cannot tell the SSE2 arithmetic from the default"
    with SangNom2(clip, opt=1, **kw, **ckw, **PATHS[path]) as flt:
        for f, src in enumerate(frames):
            _assert_frames(want[f], flt.get_frame(src, parity=parities[f]), f"frame {f}")
        if model is not None and w % 32 != 0:  # the shared pool a history-carrying clip carries along, one plane or three
            assert np.array_equal(model.pool.astype(clip.dtype), flt.read_pool(0)), "pool differs after the last frame"
        i = flt.info()
        assert i.frames == n
        if path == "sweep" and i.fused_eligible:  # the sweeps did run where the context says it has them
            assert i.fused_frames == n
        if path == "pool":
            assert i.fused_frames == 0


# fresh_pool planes whose width is a multiple of 8 but not of 32 are what the PADDED sweep serves (the plane is swept over
# its pool stride with zero costs in the padding): its SN_ARITH_SSE2 instances against a new model instance per plane and frame
PADDED = [("Y8", 104, 24, {}, "noise01"), ("Y8", 104, 24, dict(order=2), "checker2"), ("Y8", 1000, 32, {}, "noise01"),
          ("Y8", 1000, 32, dict(order=0), "checker2"), ("Y8", 3816, 24, {}, "noise"), ("Y8", 72, 20, dict(dh=True), "noise01"),
          ("YUV420P8", 208, 32, dict(aac=48), "noise01"), ("YUV444P8", 104, 24, dict(aac=48), "checker2")]


@pytest.mark.parametrize("mode", ["auto", "fused"])
@pytest.mark.parametrize("fmt,w,h,kw,pattern", PADDED, ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[4]}" for c in PADDED])
def test_padded_sweep_of_fresh_pools_matches_the_model(hip_lib, fmt, w, h, kw, pattern, mode):
    import torch
    clip, n = clip_format(fmt, w, h), 3
    assert all((w >> (clip.subw if p else 0)) % 8 == 0 and (w >> (clip.subw if p else 0)) % 32 != 0 for p in range(clip.planes))
    frames = _frames(clip, pattern, n, seed0=500)
    parities = [1, 0, 1]
    want, _ = _want(clip, kw, frames, parities, 1, fresh=True)
    base, _ = _want(clip, kw, frames, parities, 0, fresh=True)
    assert _differs(want, base), "this case cannot tell the SSE2 arithmetic from the default"
    with SangNom2(clip, opt=1, fresh_pool=True, mode=mode, small_launches=capi.SN_SMALL_SWEEP, **kw) as flt:
        assert flt.info().fused_eligible == 1 and flt.info().history_free == 1
        for f, src in enumerate(frames):  # one frame per launch
            _assert_frames(want[f], flt.get_frame(src, parity=parities[f]), f"frame {f}")
        i = flt.info()
        assert i.frames == n and i.fused_frames == n and i.banded_frames == 0, "the padded sweep did not serve these frames"
    dev = torch.device("cuda:0")
    with SangNom2(clip, opt=1, fresh_pool=True, mode=mode, max_batch=n, small_launches=capi.SN_SMALL_SWEEP, **kw) as flt:  # ... and a batch
        src = [torch.from_numpy(np.stack([fr[p] for fr in frames])).pin_memory().to(dev) for p in range(clip.planes)]
        dst = [torch.zeros((n,) + flt.plane_shape_out(p), dtype=src[p].dtype, device=dev) for p in range(clip.planes)]
        torch.cuda.synchronize()
        flt.process_batch(src, dst, parities)
        flt.synchronize()
        for f in range(n):
            _assert_frames(want[f], [to_host(dst[p][f]) for p in range(clip.planes)], f"batch frame {f}")
        assert flt.info().fused_frames == n


HISTORY = [("Y8", 100, 40, {}), ("Y8", 104, 40, {}), ("Y8", 1000, 32, dict(order=0)), ("Y16", 104, 24, {}),
           ("YUV420P8", 208, 32, dict(aac=48)), ("YUV420P16", 80, 32, dict(aac=48))]


@pytest.mark.parametrize("chain", [0, -1, 1])
@pytest.mark.parametrize("fmt,w,h,kw", HISTORY, ids=[f"{c[0]}-{c[1]}" for c in HISTORY])
def test_history_carrying_batches_run_as_chains_in_the_mode(hip_lib, fmt, w, h, kw, chain):
    """Several frames of a history-carrying clip in one call: the chain kernels (sn_policy.chain) and the pass-by-pass
    form must both give what one reference instance gives frame after frame."""
    import torch
    clip, n, dev = clip_format(fmt, w, h), 5, torch.device("cuda:0")
    frames = _frames(clip, "noise01", n, seed0=700)
    parities = [1, 0, 1, 1, 0]
    want, _ = _want(clip, kw, frames, parities, 1)
    base, _ = _want(clip, kw, frames, parities, 0)
    assert _differs(want, base)
    vt = {1: np.uint8, 2: np.int16}[clip.bytes]
    with SangNom2(clip, opt=1, max_batch=n, chain=chain, **kw) as flt:
        assert flt.info().history_free == 0
        src = [torch.from_numpy(np.stack([fr[p] for fr in frames]).view(vt)).pin_memory().to(dev) for p in range(clip.planes)]
        dst = [torch.zeros((n,) + flt.plane_shape_out(p), dtype=src[p].dtype, device=dev) for p in range(clip.planes)]
        torch.cuda.synchronize()
        flt.process_batch(src, dst, parities)
        flt.synchronize()
        for f in range(n):
            _assert_frames(want[f], [to_host(dst[p][f]).view(clip.dtype) for p in range(clip.planes)], f"frame {f}")
        chained = flt.info().chained_frames
    with SangNom2(clip, opt=0, max_batch=n, chain=chain, **kw) as flt:  # the same scheduling as in the default arithmetic
        dst0 = [torch.zeros_like(d) for d in dst]
        torch.cuda.synchronize()
        flt.process_batch(src, dst0, parities)
        flt.synchronize()
        for f in range(n):
            _assert_frames(base[f], [to_host(dst0[p][f]).view(clip.dtype) for p in range(clip.planes)], f"default frame {f}")
        assert flt.info().chained_frames == chained
    if chain >= 0 and all((w >> (clip.subw if p else 0)) % 8 == 0 for p in range(clip.planes)):  # what the chain kernels take
        assert chained > 0


@pytest.mark.parametrize("fmt", ["Y8", "Y16", "YUV420P8"])
def test_a_chain_launch_that_timed_out_is_redone_in_the_mode(hip_lib, fmt):
    """The guarded redo behind a chain over several workgroups per buffer (sn_debug_raise_chain_fault makes the next launch
    really go wrong): stage 1 again and the chain on one workgroup per buffer, all in the SSE2 arithmetic -- the frames and
    the pool carried into the next launch equal the model's, and sn_info.chain_redone counts the launch."""
    import torch
    clip = clip_format(fmt, 1008 if fmt == "YUV420P8" else 1000, 40)  # (a chain needs planes a multiple of 8 wide: 504-wide chroma)
    n, kw, dev = 12, dict(aac=48), torch.device("cuda:0")
    frames = _frames(clip, "noise01", 3 * n, seed0=800)
    want, model = _want(clip, kw, frames, [1] * (3 * n), 1)
    base, _ = _want(clip, kw, frames, [1] * (3 * n), 0)
    assert _differs(want, base)
    vt = {1: np.uint8, 2: np.int16}[clip.bytes]
    with SangNom2(clip, opt=1, max_batch=n, chain=8, **kw) as flt:
        for launch in range(3):
            part = frames[launch * n:(launch + 1) * n]
            src = [torch.from_numpy(np.stack([fr[p] for fr in part]).view(vt)).pin_memory().to(dev) for p in range(clip.planes)]
            dst = [torch.zeros((n,) + flt.plane_shape_out(p), dtype=src[p].dtype, device=dev) for p in range(clip.planes)]
            torch.cuda.synchronize()
            if launch == 1:
                flt.raise_chain_fault()
            flt.process_batch(src, dst)
            flt.synchronize()
            info = flt.info()
            assert info.chained_frames == (launch + 1) * n
            assert info.chain_redone == (1 if launch >= 1 else 0), (fmt, launch, info.chain_redone)
            for f in range(n):
                _assert_frames(want[launch * n + f], [to_host(dst[p][f]).view(clip.dtype) for p in range(clip.planes)], f"launch {launch} frame {f}")
        extra = synth.frame(clip, "noise01", seed=999)  # a frame on its own carries on from the chain's last pool
        _assert_frames(model.get_frame(extra), flt.get_frame(extra), "single frame after the chains")
        assert np.array_equal(model.pool.astype(clip.dtype), flt.read_pool(0)), "pool differs after the chains"


@pytest.mark.parametrize("fmt,w,h,kw", [("Y8", 1056, 300, {}), ("Y8", 3840, 120, dict(order=2)), ("Y16", 960, 200, {}),
                                        ("YUV420P8", 256, 128, dict(aac=48))], ids=["y8-1056", "y8-3840", "y16-960", "yuv420p8-256"])
def test_forced_bands_and_pool_mode_agree_with_auto(hip_lib, fmt, w, h, kw):
    """SN_MODE_AUTO with the small-launch policy as it ships, with bands forced (sn_debug_set_bands) or switched off, and
    SN_MODE_POOL: one answer, the model's.  8-bit planes on their own are really cut into bands in this arithmetic (a frame
    whose check fails is redone by the pool kernels, in the same arithmetic); the other clips run on the pool kernels."""
    clip = clip_format(fmt, w, h)
    frames = _frames(clip, "noise01", 2, seed0=900)
    want, _ = _want(clip, kw, frames, [1, 1], 1)
    base, _ = _want(clip, kw, frames, [1, 1], 0)
    assert _differs(want, base)
    for mode, bands in (("auto", 0), ("auto", 4), ("auto", -1), ("pool", 0)):
        with SangNom2(clip, opt=1, mode=mode, **kw) as flt:
            if bands:
                flt.set_bands(bands)
            for f, src in enumerate(frames):
                _assert_frames(want[f], flt.get_frame(src), f"{mode} bands {bands} frame {f}")
            i = flt.info()
            if bands > 0 and mode == "auto" and fmt == "Y8":
                assert i.banded_frames == len(frames), "the forced bands did not run"
            if fmt != "Y8":
                assert i.banded_frames == 0 and i.fused_frames == 0


# ---- interface -------------------------------------------------------------------------------------------------------

def _cfg(**kw):
    base = dict(struct_size=ctypes.sizeof(capi.SnConfig), width=64, height=32, bytes_per_sample=1, bits_per_sample=8,
                num_planes=1, sub_w=0, sub_h=0, order=1, aa=48, aac=0, dh=0, luma=1, chroma=1, device=0, max_batch=1, mode=0,
                host_depth=0, isolated_planes=0, fresh_pool=0, stream=None)
    base.update(kw)
    return capi.SnConfig(**base)


def test_create_ex_options(hip_lib):
    h = ctypes.c_void_p()
    cfg = _cfg()
    # NULL options and arithmetic 0: the default
    for opts in (None, ctypes.byref(capi.options(capi.SN_ARITH_CXX))):
        assert hip_lib.sn_create_ex(ctypes.byref(cfg), None, opts, ctypes.byref(h)) == capi.SN_OK
        assert hip_lib.sn_get_arithmetic(h) == capi.SN_ARITH_CXX
        hip_lib.sn_destroy(h)
    assert hip_lib.sn_get_arithmetic(None) == -1
    bad = capi.options(7)
    assert hip_lib.sn_create_ex(ctypes.byref(cfg), None, ctypes.byref(bad), ctypes.byref(h)) == capi.SN_ERR_INVALID_ARG
    assert b"arithmetic" in hip_lib.sn_last_error(None)
    bad = capi.options(1)
    bad.struct_size = 8
    assert hip_lib.sn_create_ex(ctypes.byref(cfg), None, ctypes.byref(bad), ctypes.byref(h)) == capi.SN_ERR_INVALID_ARG
    bad = capi.options(1)
    bad.reserved[3] = 1
    assert hip_lib.sn_create_ex(ctypes.byref(cfg), None, ctypes.byref(bad), ctypes.byref(h)) == capi.SN_ERR_INVALID_ARG
    assert ctypes.sizeof(capi.SnOptions) == 32
    assert hip_lib.sn_abi_version() == 4


def test_the_mode_reports_where_its_planes_run(hip_lib):
    """In this arithmetic the 8-bit sweeps of planes on their own exist (Y8, 4:4:4, isolated planes, fresh pools); 9..16-bit
    clips and subsampled chroma that shares the luma pool run on the pool kernels: fused_eligible is 0 there, SN_MODE_FUSED
    fails with a message that names the mode, and no frame counts as fused.  All of them are eligible by default."""
    sweep = capi.SN_SMALL_SWEEP
    for fmt, w, h, kw, has_sweeps in (("Y8", 256, 64, {}, True), ("YUV444P8", 256, 64, dict(aac=48), True),
                                      ("YUV420P8", 256, 64, dict(aac=48, isolated_planes=True), True),
                                      ("Y8", 104, 64, dict(fresh_pool=True), True),
                                      ("Y16", 256, 64, {}, False), ("Y10", 256, 64, {}, False),
                                      ("YUV420P8", 256, 64, dict(aac=48), False), ("YUV422P8", 256, 64, dict(aac=48), False),
                                      ("YUV420P16", 256, 64, dict(aac=48, isolated_planes=True), False)):
        clip = clip_format(fmt, w, h)
        src = synth.frame(clip, "noise01", seed=1)
        with SangNom2(clip, opt=0, small_launches=sweep, **kw) as flt:
            assert flt.info().fused_eligible == 1
            flt.get_frame(src)
            assert flt.info().fused_frames == 1
        with SangNom2(clip, opt=1, small_launches=sweep, **kw) as flt:
            assert flt.info().fused_eligible == (1 if has_sweeps else 0)
            flt.get_frame(src)
            i = flt.info()
            assert i.frames == 1 and i.fused_frames == (1 if has_sweeps else 0) and i.banded_frames == 0
        if has_sweeps:
            with SangNom2(clip, opt=1, mode="fused", **kw) as flt:
                flt.get_frame(src)
                assert flt.info().fused_frames == 1
        else:
            with pytest.raises(SangNomError, match="SN_ARITH_SSE2") as ei:
                SangNom2(clip, opt=1, mode="fused", **kw)
            assert ei.value.code == capi.SN_ERR_UNSUPPORTED


def test_planes_narrower_than_two_vectors_are_rejected_in_the_mode(hip_lib):
    for fmt, w, h, kw, ok in (("Y8", 24, 16, {}, False), ("Y8", 32, 16, {}, True), ("Y16", 8, 16, {}, False), ("Y16", 16, 16, {}, True),
                              ("Y32", 4, 16, {}, False), ("Y32", 8, 16, {}, True),
                              ("YUV420P8", 48, 32, dict(aac=48), False),               # chroma 24 wide
                              ("YUV420P8", 48, 32, dict(aac=48, chroma=False), True),  # ... but not processed
                              ("YUV420P8", 64, 32, dict(aac=48), True)):
        clip = clip_format(fmt, w, h)
        if ok:
            SangNom2(clip, opt=1, **kw).close()
        else:
            with pytest.raises(SangNomError, match="two vectors") as ei:
                SangNom2(clip, opt=1, **kw)
            assert ei.value.code == capi.SN_ERR_UNSUPPORTED
    with pytest.raises(SangNomError, match="two vectors"):  # the TURNED clip of the anti-aliasing call: 24 samples wide
        SangNomAAHost(clip_format("Y8", 64, 24), opt=1)
    SangNomAAHost(clip_format("Y8", 64, 24), opt=0).close()


@pytest.mark.parametrize("fmt,w,h,kw", [("Y32", 72, 32, {}), ("Y32", 256, 32, {}), ("YUV444PS", 64, 16, dict(aac=48, dh=True)), ("YUV420PS", 128, 32, dict(aac=20))])
def test_float_contexts_are_equal_in_both_modes(hip_lib, fmt, w, h, kw):
    clip = clip_format(fmt, w, h)
    frames = _frames(clip, "noise", 2, seed0=11)
    m = NumpySangNom(w, h, **_model_kw(clip, kw))
    want = [m.get_frame(fr) for fr in frames]
    for opt in (0, 1):
        with SangNom2(clip, opt=opt, **kw) as flt:
            assert hip_lib.sn_get_arithmetic(flt._h) == opt
            assert flt.info().fused_eligible == (1 if w % 32 == 0 else 0)  # float keeps its sweeps (widths that are a multiple of 32)
            for f, src in enumerate(frames):
                _assert_frames(want[f], flt.get_frame(src), f"opt {opt} frame {f}")


def test_legacy_entry_point_passes_opt_on(hip_lib):
    clip = clip_format("Y8", 64, 32)
    src = synth.frame(clip, "checker2", seed=3)
    m1, m0 = sm.Sse2SangNom(64, 32, order=2), NumpySangNom(64, 32, order=2)
    w1, w0 = m1.get_frame(src), m0.get_frame(src)
    assert not same(w1[0], w0[0])
    with SangNom(clip, order=0, opt=1) as flt:  # legacy order 0 = bottom field = SangNom2's 2
        _assert_frames(w1, flt.get_frame(src), "opt=1")
    with SangNom(clip, order=0) as flt:
        _assert_frames(w0, flt.get_frame(src), "opt=-1")


# ---- the anti-aliasing idiom ---------------------------------------------------------------------------------------------

def _aa_want(clip, kw, frames, arithmetic):
    turned = dict(_model_kw(clip, kw), subw=clip.subh, subh=clip.subw)
    first = sm.model_for(arithmetic, clip.height, clip.width, **turned)
    second = sm.model_for(arithmetic, clip.width, clip.height, **_model_kw(clip, kw))
    out = []
    for fr in frames:
        a = first.get_frame([np.ascontiguousarray(np.rot90(pl, k=1)) for pl in fr])
        out.append(second.get_frame([np.ascontiguousarray(np.rot90(pl, k=-1)) for pl in a]))
    return out


@pytest.mark.parametrize("fmt,w,h,kw", [("Y8", 96, 64, {}), ("Y8", 100, 72, dict(order=2)), ("Y16", 64, 48, {}),
                                        ("YUV420P8", 128, 64, dict(aac=48))], ids=["y8", "y8-history", "y16", "yuv420p8"])
def test_anti_aliasing_call_in_the_mode(hip_lib, fmt, w, h, kw):
    import torch
    clip = clip_format(fmt, w, h)
    frames = _frames(clip, "noise01", 2, seed0=40)
    want = _aa_want(clip, kw, frames, 1)
    assert _differs(want, _aa_want(clip, kw, frames, 0))
    with SangNomAAHost(clip, opt=1, **kw) as aa:  # sn_aa_create_ex
        for f, fr in enumerate(frames):
            _assert_frames(want[f], aa.get_frame(fr), f"host frame {f}")
    dev = torch.device("cuda:0")
    vt = {1: np.uint8, 2: np.int16}[clip.bytes]
    with SangNomAA(clip, max_batch=1, opt=1, **kw) as aa:  # two contexts and the turn kernel
        for f, fr in enumerate(frames):
            src = [torch.from_numpy(fr[p][None].view(vt)).pin_memory().to(dev) for p in range(clip.planes)]
            dst = [torch.zeros_like(s) for s in src]
            torch.cuda.synchronize()
            aa.process_batch(src, dst)
            aa.synchronize()
            _assert_frames(want[f], [to_host(dst[p][0]).view(clip.dtype) for p in range(clip.planes)], f"device frame {f}")
