"""Host-side mirror of the reference's filter object for tests and the benchmark.

`SangNom2(clip_format, order, aa, aac, threads, dh, luma, chroma, opt)` keeps the reference's
argument names, defaults and error text (/root/reference/src/SangNom2.cpp:399-435; README.md:20-57)
and `get_frame` plays the role of `SangNom2::GetFrame` (src/SangNom2.cpp:332-397).  All pixel work is
done by libsangnom_hip.so through the C ABI; torch is used only to hold device memory.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import capi


class SangNomError(RuntimeError):
    """Raised where the reference would call env->ThrowError, with the same message."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


@dataclass
class ClipFormat:
    """The part of AviSynth's VideoInfo the filter looks at (planar Y / YUV only)."""
    width: int
    height: int
    bytes: int = 1       # vi.ComponentSize()
    bits: int = 8        # vi.BitsPerComponent()
    planes: int = 1      # vi.NumComponents() clipped to 3
    subw: int = 0        # log2 chroma subsampling
    subh: int = 0

    @property
    def dtype(self):
        return {1: np.uint8, 2: np.uint16, 4: np.float32}[self.bytes]


_FORMATS = {
    "Y8": dict(bytes=1, bits=8, planes=1), "Y10": dict(bytes=2, bits=10, planes=1),
    "Y12": dict(bytes=2, bits=12, planes=1), "Y14": dict(bytes=2, bits=14, planes=1),
    "Y16": dict(bytes=2, bits=16, planes=1), "Y32": dict(bytes=4, bits=32, planes=1),
    "YUV422P16": dict(bytes=2, bits=16, planes=3, subw=1, subh=0),
    "YUV420P8": dict(bytes=1, bits=8, planes=3, subw=1, subh=1),
    "YUV420P10": dict(bytes=2, bits=10, planes=3, subw=1, subh=1),
    "YUV420P12": dict(bytes=2, bits=12, planes=3, subw=1, subh=1),
    "YUV420P16": dict(bytes=2, bits=16, planes=3, subw=1, subh=1),
    "YUV422P8": dict(bytes=1, bits=8, planes=3, subw=1, subh=0),
    "YUV422P10": dict(bytes=2, bits=10, planes=3, subw=1, subh=0), "YUV422P12": dict(bytes=2, bits=12, planes=3, subw=1, subh=0),
    "YUV444P8": dict(bytes=1, bits=8, planes=3), "YUV444P16": dict(bytes=2, bits=16, planes=3),
    "YUV444PS": dict(bytes=4, bits=32, planes=3), "YUV420PS": dict(bytes=4, bits=32, planes=3, subw=1, subh=1),
    "YUV422PS": dict(bytes=4, bits=32, planes=3, subw=1, subh=0),
}


def clip_format(name: str, width: int, height: int) -> ClipFormat:
    """ClipFormat from an AviSynth+ pixel_type name such as "YUV420P8" or "Y16"."""
    return ClipFormat(width=width, height=height, **_FORMATS[name])


def _packed_surface_of(t, shape_of, B, what, packed, msb):
    """sn_surfaces of ONE device tensor that holds a packed 4:2:2 batch: [N, H, 2 W] of the sample type for "yuyv" / "uyvy",
    [N, H, 4 ceil(W / 6)] int32 for "v210"."""
    if (packed, bool(msb)) not in capi.PACKED_LAYOUTS:
        raise ValueError(f"{what}: packed must be 'yuyv', 'uyvy' or 'v210' (v210 has no MSB form)")
    if isinstance(t, (list, tuple)):
        if len(t) != 1:
            raise ValueError(f"{what}: a packed surface is ONE tensor")
        t = t[0]
    H, W = shape_of(0)
    v210 = packed == "v210"
    want, size = ((H, 4 * ((W + 5) // 6)), 4) if v210 else ((H, 2 * W), B)
    if t.dim() != 3 or tuple(t.shape[1:]) != want:
        raise ValueError(f"{what}: shape {tuple(t.shape)}, expected (N,) + {want}")
    if t.element_size() != size or not t.is_cuda or t.stride(-1) != 1:
        raise ValueError(f"{what}: a device-resident tensor of {'int32' if v210 else 'the sample type'} with contiguous rows expected")
    return capi.surfaces(capi.PACKED_LAYOUTS[(packed, bool(msb))], [t.data_ptr()], [t.stride(1) * size], [t.stride(0) * size]), t.shape[0]


def _surfaces_of(planes, shape_of, nplanes, B, what, msb=False, packed=None):
    """sn_surfaces of device tensors: the planar tensors process_batch takes ([N, H_p, W_p] each), or two tensors
    [Y [N, H, W], UV [N, Hc, Wc, 2]] for a semi-planar surface (NV12, P010 / P016, NV16, NV24; UV[..., 0] is U).
    msb: 16-bit words with the sample in the high bits (SN_LAYOUT_*_MSB).  packed: "yuyv", "uyvy" or "v210" -- one tensor."""
    if packed is not None:
        return _packed_surface_of(planes, shape_of, B, what, packed, msb)
    planes = list(planes)
    semi = len(planes) == 2 and planes[1].dim() == 4
    if not semi and len(planes) < nplanes:
        raise ValueError(f"{what}: {nplanes} planar tensors or [Y, UV] expected")
    N = planes[0].shape[0]
    ptr, pitch, fs = [], [], []
    for p, t in enumerate(planes[:2 if semi else nplanes]):
        want = (N,) + tuple(shape_of(1 if p else 0)) + ((2,) if semi and p else ())
        if tuple(t.shape) != want:
            raise ValueError(f"{what} plane {p}: shape {tuple(t.shape)}, expected {want}")
        if t.element_size() != B or not t.is_cuda:
            raise ValueError(f"{what}: device-resident tensors of the clip's sample type expected")
        if t.stride(-1) != 1 or (semi and p and t.stride(2) != 2):
            raise ValueError(f"{what} plane {p}: rows must be contiguous (a UV tensor: stride(2) == 2, last stride 1)")
        ptr.append(t.data_ptr()), pitch.append(t.stride(1) * B), fs.append(t.stride(0) * B)
    layout = (capi.SN_LAYOUT_SEMIPLANAR_MSB if semi else capi.SN_LAYOUT_PLANAR_MSB) if msb else \
        (capi.SN_LAYOUT_SEMIPLANAR if semi else capi.SN_LAYOUT_PLANAR)
    return capi.surfaces(layout, ptr, pitch, fs), N


class SangNom2:
    """One filter instance == one sn_context (its own stream and device pool)."""

    def __init__(self, clip: ClipFormat, order: int = 1, aa: int = 48, aac: int = 0, threads: int = 0,
                 dh: bool = False, luma: bool = True, chroma: bool = True, opt: int = -1,
                 device: int = 0, max_batch: int = 1, mode: str = "auto", stream: int | None = None,
                 host_depth: int = 0, isolated_planes: bool = False, fresh_pool: bool = False,
                 small_launches: int | None = None, chain: int | None = None, copy_threads: int | None = None,
                 scratch_budget_mb: int | None = None, chroma_sweeps: int | None = None, sse2_sweeps: int | None = None,
                 column_parts: int = 0):
        # `threads` is a dummy in the reference (README.md:40-41); `opt` picks its CPU code path, and with it the
        # arithmetic: opt=1 reproduces its SSE2 path (SN_ARITH_SSE2), opt=0 and opt=-1 its C++ path.
        if opt < -1 or opt > 1:
            raise SangNomError(capi.SN_ERR_CONFIG, "SangNom2: opt must be between -1..2.")  # sic, SangNom2.cpp:420
        self.clip = clip
        self._lib = capi.load()
        cfg = capi.SnConfig(
            struct_size=ctypes.sizeof(capi.SnConfig), width=clip.width, height=clip.height,
            bytes_per_sample=clip.bytes, bits_per_sample=clip.bits, num_planes=clip.planes,
            sub_w=clip.subw, sub_h=clip.subh, order=order, aa=aa, aac=aac, dh=int(dh), luma=int(luma),
            chroma=int(chroma), device=device, max_batch=max_batch, mode=capi.MODES[mode], host_depth=host_depth, isolated_planes=int(isolated_planes), fresh_pool=int(fresh_pool),
            stream=stream)
        self._cfg = cfg
        self.max_batch = max_batch
        self.device = device
        self._h = ctypes.c_void_p()
        # scheduling only (sn_policy, sangnom_hip.h); None = capi.POLICY_DEFAULTS.  chain: 0 on, -1 off, 1 / 2 / 4 / 8 = on with
        # at most that many workgroups per cost buffer.  sse2_sweeps (opt=1 only, read at creation): 1 = the sweeps serve every
        # configuration they serve with opt=0, 0 = 9..16-bit and shared-pool 4:2:0 / 4:2:2 clips stay on the pool kernels
        pol = capi.policy(small_launches=small_launches, chain=chain, copy_threads=copy_threads, scratch_budget_mb=scratch_budget_mb,
                          chroma_sweeps=chroma_sweeps, sse2_sweeps=sse2_sweeps)
        self.arithmetic = capi.arithmetic_of_opt(opt)
        # column_parts=1 (sn_options, fixed at creation): 16-bit and float planes wider than 3840 in column parts
        opts = capi.options(self.arithmetic, column_parts=column_parts)
        rc = self._lib.sn_create_ex(ctypes.byref(cfg), ctypes.byref(pol), ctypes.byref(opts), ctypes.byref(self._h))
        if rc != capi.SN_OK:
            self._h = None
            raise SangNomError(rc, self._lib.sn_last_error(None).decode())
        self.out_height = clip.height * 2 if dh else clip.height

    # -- geometry -------------------------------------------------------------------------------
    @property
    def nplanes(self) -> int:
        return min(self.clip.planes, 3)

    def plane_shape_in(self, p: int):
        return (self.clip.height >> (self.clip.subh if p else 0), self.clip.width >> (self.clip.subw if p else 0))

    def plane_shape_out(self, p: int):
        return (self.out_height >> (self.clip.subh if p else 0), self.clip.width >> (self.clip.subw if p else 0))

    # -- life cycle -----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.sn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int):
        if rc != capi.SN_OK:
            raise SangNomError(rc, self._lib.sn_last_error(self._h).decode())

    def info(self) -> capi.SnInfo:
        i = capi.SnInfo(struct_size=ctypes.sizeof(capi.SnInfo))
        self._check(self._lib.sn_get_info(self._h, ctypes.byref(i)))
        return i

    def stream_handle(self) -> int:
        return self._lib.sn_get_stream(self._h)

    def synchronize(self):
        self._check(self._lib.sn_synchronize(self._h))

    def read_pool(self, slot: int = 0) -> np.ndarray:
        i = self.info()
        out = np.empty((9, i.pool_rows, i.pool_stride), dtype=self.clip.dtype)
        self._check(self._lib.sn_debug_read_pool(self._h, slot, out.ctypes.data, out.nbytes))
        return out

    def set_policy(self, **fields) -> None:
        """Change the scheduling policy of the live context (sn_set_policy): small_launches, chain, copy_threads, chroma_sweeps
        (scratch_budget_mb and sse2_sweeps are read at creation only)."""
        cur = capi.SnPolicy(struct_size=ctypes.sizeof(capi.SnPolicy))
        self._check(self._lib.sn_get_policy(self._h, ctypes.byref(cur)))
        for k, v in fields.items():
            setattr(cur, k, int(v))
        self._check(self._lib.sn_set_policy(self._h, ctypes.byref(cur)))

    def get_policy(self) -> capi.SnPolicy:
        cur = capi.SnPolicy(struct_size=ctypes.sizeof(capi.SnPolicy))
        self._check(self._lib.sn_get_policy(self._h, ctypes.byref(cur)))
        return cur

    def raise_chain_fault(self) -> None:
        """Test hook: as if a chain over several workgroups had timed out (sn_debug_raise_chain_fault)."""
        self._check(self._lib.sn_debug_raise_chain_fault(self._h))

    def set_bands(self, bands: int = 0, warm_rows: int = 0) -> None:
        """Test hook: row bands of the small-launch path (sn_debug_set_bands)."""
        self._check(self._lib.sn_debug_set_bands(self._h, bands, warm_rows))

    def parts_info(self) -> capi.SnPartsInfo:
        """The column parts of this context (sn_get_parts_info); synchronises the stream."""
        i = capi.SnPartsInfo(struct_size=ctypes.sizeof(capi.SnPartsInfo))
        self._check(self._lib.sn_get_parts_info(self._h, ctypes.byref(i)))
        return i

    def debug_set_column_parts(self, parts: int = 0, ghost_columns: int = 0) -> None:
        """Test hook: force the number of column parts / the seams' distance from a window's end (sn_debug_set_column_parts)."""
        self._check(self._lib.sn_debug_set_column_parts(self._h, int(parts), int(ghost_columns)))

    def read_coupled_rows(self, which: int) -> np.ndarray:
        """Rows the fused 4:2:0 sweep of plane `which` left for the next plane: [9, rows, width]."""
        rows = self.info().coupled_rows
        out = np.empty((9, rows, self.clip.width), dtype=self.clip.dtype)
        self._check(self._lib.sn_debug_read_coupled_rows(self._h, which, out.ctypes.data, out.nbytes))
        return out

    # -- GetFrame -------------------------------------------------------------------------------
    def get_frame(self, src, parity: int = 1, dst=None):
        """Host planes (numpy 2-D arrays, any row pitch) in, host planes out (synchronous)."""
        n = self.nplanes
        if dst is None:
            dst = [np.zeros(self.plane_shape_out(p), dtype=self.clip.dtype) for p in range(n)]
        sp, dp = (ctypes.c_void_p * 3)(), (ctypes.c_void_p * 3)()
        spi, dpi = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)()
        for p in range(n):
            s, d = src[p], dst[p]
            if s.dtype != self.clip.dtype or d.dtype != self.clip.dtype:
                raise TypeError("plane dtype does not match the clip format")
            if s.shape != self.plane_shape_in(p) or d.shape != self.plane_shape_out(p):
                raise ValueError(f"plane {p}: shape {s.shape}->{d.shape}, expected "
                                 f"{self.plane_shape_in(p)}->{self.plane_shape_out(p)}")
            if s.strides[1] != self.clip.bytes or d.strides[1] != self.clip.bytes:
                raise ValueError("planes must be contiguous along x")
            sp[p], dp[p], spi[p], dpi[p] = s.ctypes.data, d.ctypes.data, s.strides[0], d.strides[0]
        self._check(self._lib.sn_process_host(self._h, sp, spi, dp, dpi, int(parity)))
        return dst

    # -- GetFrame with look-ahead: the host ring ------------------------------------------------------
    def host_slots(self) -> int:
        return self._lib.sn_host_slots(self._h)

    def _plane_args(self, planes, shape_of):
        ptr, pitch = (ctypes.c_void_p * 3)(), (ctypes.c_int32 * 3)()
        for p in range(self.nplanes):
            a = planes[p]
            if a.dtype != self.clip.dtype or a.shape != shape_of(p) or a.strides[1] != self.clip.bytes:
                raise ValueError(f"plane {p}: expected {shape_of(p)} {self.clip.dtype}, x-contiguous")
            ptr[p], pitch[p] = a.ctypes.data, a.strides[0]
        return ptr, pitch

    def submit(self, src, parity: int = 1, dst=None) -> int:
        """Queue one host frame (H2D, sweeps, D2H on a ring slot's own stream); returns the slot.  With `dst` the
        output planes are named now (sn_submit_host_to): pinned ones are written straight from the device."""
        sp, spi = self._plane_args(src, self.plane_shape_in)
        slot = ctypes.c_int32(-1)
        if dst is None:
            self._check(self._lib.sn_submit_host(self._h, sp, spi, int(parity), ctypes.byref(slot)))
        else:
            dp, dpi = self._plane_args(dst, self.plane_shape_out)
            self._check(self._lib.sn_submit_host_to(self._h, sp, spi, dp, dpi, int(parity), ctypes.byref(slot)))
        return slot.value

    def collect(self, slot: int, dst=None, announced: bool = False):
        """Wait for the frame in `slot` and copy it into host planes (announced: they were named at submission)."""
        if announced:
            self._check(self._lib.sn_collect_host(self._h, int(slot), None, None))
            return dst
        if dst is None:
            dst = [np.zeros(self.plane_shape_out(p), dtype=self.clip.dtype) for p in range(self.nplanes)]
        dp, dpi = self._plane_args(dst, self.plane_shape_out)
        self._check(self._lib.sn_collect_host(self._h, int(slot), dp, dpi))
        return dst

    def turn(self, src, dst, direction: int):
        """TurnRight (direction > 0) / TurnLeft (< 0) of device planes: src [N, H, W] -> dst [N, W, H] (torch tensors)."""
        B = self.clip.bytes
        N, H, W = src.shape
        if tuple(dst.shape) != (N, W, H) or src.stride(2) != 1 or dst.stride(2) != 1 or src.element_size() != B or dst.element_size() != B:
            raise ValueError("turn: dst must be [N, W, H] of the clip's sample type, both x-contiguous")
        self._check(self._lib.sn_turn_device(self._h, int(direction), N, src.data_ptr(), src.stride(0) * B, src.stride(1) * B, W, H,
                                             dst.data_ptr(), dst.stride(0) * B, dst.stride(1) * B))
        return dst

    def reduce(self, src, dst, kernel, ox: int, oy: int):
        """sn_reduce_device: src [N, 2 H, 2 W] -> dst [N, H, W] (torch tensors on the device) by kernel "tent" | "halfband",
        centred on src[2y + oy][2x + ox].  Asynchronous on the context's stream."""
        B = self.clip.bytes
        N, H, W = dst.shape
        if tuple(src.shape) != (N, 2 * H, 2 * W) or src.stride(2) != 1 or dst.stride(2) != 1 or src.element_size() != B or dst.element_size() != B:
            raise ValueError("reduce: src must be [N, 2 H, 2 W] for dst [N, H, W], both x-contiguous and of the clip's sample type")
        self._check(self._lib.sn_reduce_device(self._h, capi.REDUCE_KERNELS.get(kernel, kernel), N, src.data_ptr(), src.stride(0) * B, src.stride(1) * B,
                                               W, H, int(ox), int(oy), dst.data_ptr(), dst.stride(0) * B, dst.stride(1) * B))
        return dst

    def mask_merge(self, src, aa, dst, lo: int, hi: int, expand: int = 1):
        """sn_mask_merge_device: the Sobel edge mask of src [N, H, W] (lo, hi in 8-bit scale, expand 0 | 1) merges aa into src:
        dst = src where the mask is 0, aa where it is 256.  aa=None: dst is the mask itself.  dst may be aa.  Torch tensors
        on the device; asynchronous on the context's stream."""
        B = self.clip.bytes
        N, H, W = dst.shape
        for t in (src, dst) + (() if aa is None else (aa,)):
            if tuple(t.shape) != (N, H, W) or t.stride(2) != 1 or t.element_size() != B:
                raise ValueError("mask_merge: src, aa and dst must be [N, H, W], x-contiguous and of the clip's sample type")
        m = capi.aa_mask((lo, hi), expand)
        a_ptr, a_fs, a_p = (None, 0, 0) if aa is None else (aa.data_ptr(), aa.stride(0) * B, aa.stride(1) * B)
        self._check(self._lib.sn_mask_merge_device(self._h, ctypes.byref(m), N, src.data_ptr(), src.stride(0) * B, src.stride(1) * B, a_ptr, a_fs, a_p,
                                                   W, H, dst.data_ptr(), dst.stride(0) * B, dst.stride(1) * B))
        return dst

    def contra_sharpen(self, src, aa, dst, amount: int):
        """sn_contra_sharpen_device: aa [N, H, W] (a filtered plane) is sharpened by amount / 64 (1..255) of an unsharp mask,
        limited by what src - aa allows over 3 x 3, and written to dst (sangnom_hip.h, "Contra-sharpening").  dst must overlap
        neither src nor aa.  Torch tensors on the device; asynchronous on the context's stream."""
        B = self.clip.bytes
        N, H, W = dst.shape
        for t in (src, aa, dst):
            if tuple(t.shape) != (N, H, W) or t.stride(2) != 1 or t.element_size() != B:
                raise ValueError("contra_sharpen: src, aa and dst must be [N, H, W], x-contiguous and of the clip's sample type")
        self._check(self._lib.sn_contra_sharpen_device(self._h, int(amount), N, src.data_ptr(), src.stride(0) * B, src.stride(1) * B, aa.data_ptr(),
                                                       aa.stride(0) * B, aa.stride(1) * B, W, H, dst.data_ptr(), dst.stride(0) * B, dst.stride(1) * B))
        return dst

    def merge(self, a, b, dst):
        """sn_merge_device: dst = avg(a, b), sample by sample (sangnom_hip.h, "Both fields": integers (a + b + 1) >> 1, float
        (a + b) * 0.5f with every NaN as 0x7FC00000).  a, b and dst are [N, H, W]; dst may be a or b itself, any other overlap is
        refused.  Torch tensors on the device; asynchronous on the context's stream."""
        B = self.clip.bytes
        N, H, W = dst.shape
        for t in (a, b, dst):
            if tuple(t.shape) != (N, H, W) or t.stride(2) != 1 or t.element_size() != B:
                raise ValueError("merge: a, b and dst must be [N, H, W], x-contiguous and of the clip's sample type")
        self._check(self._lib.sn_merge_device(self._h, N, a.data_ptr(), a.stride(0) * B, a.stride(1) * B, b.data_ptr(), b.stride(0) * B, b.stride(1) * B,
                                              W, H, dst.data_ptr(), dst.stride(0) * B, dst.stride(1) * B))
        return dst

    def turn_merge(self, a, b, dst, direction: int):
        """sn_turn_merge_device: the quarter turn (direction > 0 clockwise, < 0 anti-clockwise) of avg(a, b) in one kernel.  a and b
        are [N, H, W], dst is [N, W, H] and overlaps neither.  Torch tensors on the device; asynchronous on the context's stream."""
        B = self.clip.bytes
        N, H, W = a.shape
        if tuple(b.shape) != (N, H, W) or any(t.stride(2) != 1 or t.element_size() != B for t in (a, b, dst)) or tuple(dst.shape) != (N, W, H):
            raise ValueError("turn_merge: a and b must be [N, H, W] and dst [N, W, H], x-contiguous and of the clip's sample type")
        self._check(self._lib.sn_turn_merge_device(self._h, int(direction), N, a.data_ptr(), a.stride(0) * B, a.stride(1) * B, b.data_ptr(),
                                                   b.stride(0) * B, b.stride(1) * B, W, H, dst.data_ptr(), dst.stride(0) * B, dst.stride(1) * B))
        return dst

    def repair(self, src, aa, dst, rank: int):
        """sn_repair_device: each sample of aa [N, H, W] (a filtered plane) is clamped into the range of the rank-th smallest
        and rank-th largest (rank 1..4) of the nine samples of src around it and written to dst (sangnom_hip.h, "Rank
        repair").  dst may be aa itself; it must not overlap src.  Torch tensors on the device; asynchronous on the context's stream."""
        B = self.clip.bytes
        N, H, W = dst.shape
        for t in (src, aa, dst):
            if tuple(t.shape) != (N, H, W) or t.stride(2) != 1 or t.element_size() != B:
                raise ValueError("repair: src, aa and dst must be [N, H, W], x-contiguous and of the clip's sample type")
        self._check(self._lib.sn_repair_device(self._h, int(rank), N, src.data_ptr(), src.stride(0) * B, src.stride(1) * B, aa.data_ptr(),
                                               aa.stride(0) * B, aa.stride(1) * B, W, H, dst.data_ptr(), dst.stride(0) * B, dst.stride(1) * B))
        return dst

    def mask_merge_luma(self, luma, src, aa, dst, lo: int, hi: int, expand: int = 1, sub_w: int = 1, sub_h: int = 1):
        """sn_mask_merge_luma_device: the Sobel edge mask of luma [N, H << sub_h, W << sub_w], reduced to chroma's geometry
        by the block mean, merges aa into src.  src, aa and dst are one tensor [N, H, W] or a pair of them (U and V in one
        launch); aa=None: dst is the reduced mask itself.  dst may be aa.  Torch tensors on the device; asynchronous on the
        context's stream."""
        B = self.clip.bytes
        as_pair = lambda t: list(t) if isinstance(t, (list, tuple)) else [t]
        s, d = as_pair(src), as_pair(dst)
        a = None if aa is None else as_pair(aa)
        N, H, W = d[0].shape
        if len(s) not in (1, 2) or len(d) != len(s) or (a is not None and len(a) != len(s)):
            raise ValueError("mask_merge_luma: src, aa and dst must be one tensor each or pairs of the same length")
        for t in s + d + (a or []):
            if tuple(t.shape) != (N, H, W) or t.stride(2) != 1 or t.element_size() != B:
                raise ValueError("mask_merge_luma: src, aa and dst must be [N, H, W], x-contiguous and of the clip's sample type")
        if tuple(luma.shape) != (N, H << sub_h, W << sub_w) or luma.stride(2) != 1 or luma.element_size() != B:
            raise ValueError("mask_merge_luma: luma must be [N, H << sub_h, W << sub_w], x-contiguous and of the clip's sample type")

        def arrays(ts):
            ptr, fs, pitch = (ctypes.c_void_p * 2)(), (ctypes.c_int64 * 2)(), (ctypes.c_int32 * 2)()
            for p, t in enumerate(ts):
                ptr[p], fs[p], pitch[p] = t.data_ptr(), t.stride(0) * B, t.stride(1) * B
            return ptr, fs, pitch
        m = capi.aa_mask((lo, hi), expand)
        sa, da = arrays(s), arrays(d)
        aaa = (None, None, None) if a is None else arrays(a)
        self._check(self._lib.sn_mask_merge_luma_device(self._h, ctypes.byref(m), N, luma.data_ptr(), luma.stride(0) * B, luma.stride(1) * B,
                                                        int(sub_w), int(sub_h), *sa, *aaa, W, H, *da))
        return dst

    def get_frame_device(self, src, dst, parity: int = 1):
        """Device planes: torch tensors [H, W] on this context's GPU.  Asynchronous."""
        return self.process_batch([s.unsqueeze(0) for s in src], [d.unsqueeze(0) for d in dst], [parity])

    def process_batch(self, src, dst, parity=None):
        """src[p] / dst[p]: torch tensors [N, H_p, W_p] (device-resident, x-contiguous).
        Frame f of plane p lives at tensor[f].  Asynchronous on the context's stream."""
        n = self.nplanes
        N = src[0].shape[0]
        sp, dp = (ctypes.c_void_p * 3)(), (ctypes.c_void_p * 3)()
        spi, dpi = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)()
        sfs, dfs = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
        B = self.clip.bytes
        for p in range(n):
            s, d = src[p], dst[p]
            if tuple(s.shape[1:]) != self.plane_shape_in(p) or tuple(d.shape[1:]) != self.plane_shape_out(p):
                raise ValueError(f"plane {p}: bad shape {tuple(s.shape)} -> {tuple(d.shape)}")
            if s.shape[0] != N or d.shape[0] != N:
                raise ValueError("all planes must carry the same number of frames")
            if s.stride(2) != 1 or d.stride(2) != 1 or s.element_size() != B or d.element_size() != B:
                raise ValueError("planes must be x-contiguous tensors of the clip's sample type")
            if not s.is_cuda or not d.is_cuda:
                raise ValueError("process_batch needs device-resident tensors (use get_frame for host planes)")
            sp[p], dp[p] = s.data_ptr(), d.data_ptr()
            spi[p], dpi[p] = s.stride(1) * B, d.stride(1) * B
            sfs[p], dfs[p] = s.stride(0) * B, d.stride(0) * B
        par = None
        if parity is not None:
            par = (ctypes.c_int32 * N)(*[int(x) for x in parity])
        self._check(self._lib.sn_process_device_strided(self._h, N, sp, sfs, spi, dp, dfs, dpi, par))
        return dst

    def process_surfaces(self, src, dst, parity=None, src_msb=False, dst_msb=False, src_packed=None, dst_packed=None):
        """process_batch for decoder and encoder surfaces (sn_process_device_surfaces): each of src and dst is either the
        planar tensors process_batch takes or [Y [N, H, W], UV [N, Hc, Wc, 2]], independently.  src_msb / dst_msb: that
        side's 16-bit words hold the sample in their high bits (P010 on a 10-bit clip, P012 on a 12-bit one); the result is
        the clip's own, aligned as dst_msb says.  src_packed / dst_packed ("yuyv", "uyvy", "v210"; 4:2:2 clips): that side is
        ONE tensor of packed rows -- [N, H, 2 W] of the sample type (YUY2 / UYVY; Y210 / Y212 with the _msb flag), or
        [N, H, 4 ceil(W / 6)] int32 for v210.  Asynchronous on the context's stream (the first call that needs scratch
        allocates it)."""
        s, N = _surfaces_of(src, self.plane_shape_in, self.nplanes, self.clip.bytes, "src", src_msb, src_packed)
        d, Nd = _surfaces_of(dst, self.plane_shape_out, self.nplanes, self.clip.bytes, "dst", dst_msb, dst_packed)
        if N != Nd:
            raise ValueError("src and dst must carry the same number of frames")
        par = None if parity is None else (ctypes.c_int32 * N)(*[int(x) for x in parity])
        self._check(self._lib.sn_process_device_surfaces(self._h, N, ctypes.byref(s), ctypes.byref(d), par))
        return dst

    def surface_info(self) -> capi.SnSurfaceInfo:
        """What the surface calls of this context have done (sn_get_surface_info)."""
        i = capi.SnSurfaceInfo(struct_size=ctypes.sizeof(capi.SnSurfaceInfo))
        self._check(self._lib.sn_get_surface_info(self._h, ctypes.byref(i)))
        return i


def pin_host_array(a: np.ndarray) -> None:
    """sn_pin_host_buffer on a numpy array's memory: frames inside it then move over PCIe without staging copies.
    Keep the array alive and call unpin_host_array before dropping it."""
    rc = capi.load().sn_pin_host_buffer(a.ctypes.data, a.nbytes)
    if rc != capi.SN_OK:
        raise SangNomError(rc, capi.load().sn_last_error(None).decode())


def unpin_host_array(a: np.ndarray) -> None:
    rc = capi.load().sn_unpin_host_buffer(a.ctypes.data)
    if rc != capi.SN_OK:
        raise SangNomError(rc, capi.load().sn_last_error(None).decode())


def SangNom(clip: ClipFormat, order: int = 1, aa: int = 48, opt: int = -1, **kw) -> SangNom2:
    """Legacy entry point (src/SangNom2.cpp:437-472): order 0/1/2 means bottom/top/double-rate and
    is remapped to SangNom2's 2/1/0.  The reference reads args[3] (`opt`) as aac because of an
    out-of-range argument read; that quirk is NOT reproduced: aac is 0 here."""
    if order < 0 or order > 2:
        raise SangNomError(capi.SN_ERR_CONFIG, "SangNom: order must be between 0..2.")
    return SangNom2(clip, order=(2, 1, 0)[order], aa=aa, aac=0, opt=opt, **kw)


class _AAContext:
    """An sn_aa_context: the anti-aliasing idiom TurnLeft().SangNom2(...).TurnRight().SangNom2(...) as one call of the
    library.  Not a function of the reference; the result is what that script gives with it.
    dh=True: both passes with dh=true, enlargement by two in both directions; every plane is processed (luma / chroma are
    ignored, as in the reference) and every destination plane is twice as wide and twice as high as its source plane.
    reduce="tent" | "halfband" (with dh): the enlarged frame is reduced on the device by that kernel, centred on the source
    samples (sangnom_hip.h has the arithmetic), and every destination plane has the source plane's shape again.
    mask=(lo, hi), mask_expand=0 | 1 (without dh, or with dh and reduce): the result is merged into the source through a Sobel
    edge mask of the source (sangnom_hip.h, "Edge mask"): flat areas and texture keep the source's samples.
    mask_chroma="own" | "luma": every processed plane through its own mask (the default), or chroma through the mask of the
    source luma plane reduced to chroma's geometry, as anti-aliasing scripts do.
    sharpen=None | 1..255 (64 = unity), sharpen_chroma=False (without dh, or with dh and reduce): the result is contra-sharpened
    behind the last step and before the mask (sangnom_hip.h, "Contra-sharpening"): an unsharp mask, allowed only as far as the
    filter changed the picture and only towards the source.  Plane 0, or every processed plane with sharpen_chroma.
    fields="one" | "both" (without dh): "both" interpolates both fields in every pass -- two filter instances, order 1 and
    order 2 -- and averages the two results on the device (sangnom_hip.h, "Both fields"); `order` and the per-frame parity
    then have no influence.  Sharpening and mask follow the averaged result.
    repair=None | 1..4, repair_chroma=False (without dh, or with dh and reduce): behind the sharpening and before the mask each
    sample of the result is clamped into the range of the repair-th smallest and repair-th largest of the nine source samples
    around it (sangnom_hip.h, "Rank repair"), in place.  Plane 0, or every processed plane with repair_chroma."""

    def __init__(self, clip: ClipFormat, order: int = 1, aa: int = 48, aac: int = 0, luma: bool = True, chroma: bool = True,
                 device: int = 0, isolated_planes: bool = False, fresh_pool: bool = False, opt: int = -1, max_batch: int = 1,
                 host_depth: int = 0, stream: int | None = None, dh: bool = False, column_parts: int = 0, reduce=0, mask=None, mask_expand: int = 1,
                 mask_chroma="own", sharpen=None, sharpen_chroma: bool = False, fields="one", repair=None,
                 repair_chroma: bool = False, **policy_kw):
        if opt < -1 or opt > 1:
            raise SangNomError(capi.SN_ERR_CONFIG, "SangNom2: opt must be between -1..2.")  # sic, SangNom2.cpp:420
        self.clip = clip
        self.dh = bool(dh)
        aopts = capi.aa_options(reduce)  # reduce="tent" | "halfband" (dh only): the frame comes back at source size
        self.reduce = aopts.reduce
        amask = capi.aa_mask(mask, mask_expand)  # mask=(lo, hi): the result goes into the source through the source's edge mask
        amask_ex = capi.aa_mask_ex(mask_chroma)
        asharpen = capi.aa_sharpen(sharpen, sharpen_chroma)
        afields = capi.aa_fields(fields)
        arepair = capi.aa_repair(repair, repair_chroma)
        self.max_batch = max_batch
        self._lib = capi.load()
        cfg = capi.SnConfig(
            struct_size=ctypes.sizeof(capi.SnConfig), width=clip.width, height=clip.height, bytes_per_sample=clip.bytes,
            bits_per_sample=clip.bits, num_planes=clip.planes, sub_w=clip.subw, sub_h=clip.subh, order=order, aa=aa, aac=aac,
            dh=int(self.dh), luma=int(luma), chroma=int(chroma), device=device, max_batch=max_batch, mode=capi.SN_MODE_AUTO, host_depth=host_depth,
            isolated_planes=int(isolated_planes), fresh_pool=int(fresh_pool), stream=stream)
        self._h = ctypes.c_void_p()
        pol = capi.policy(**{k: policy_kw.get(k) for k in ("small_launches", "chain", "copy_threads", "scratch_budget_mb", "chroma_sweeps", "sse2_sweeps")})
        opts = capi.options(capi.arithmetic_of_opt(opt), column_parts=column_parts)
        rc = self._lib.sn_aa_create_ex7(ctypes.byref(cfg), ctypes.byref(pol), ctypes.byref(opts), ctypes.byref(aopts), ctypes.byref(amask),
                                        ctypes.byref(amask_ex), ctypes.byref(asharpen), ctypes.byref(afields), ctypes.byref(arepair),
                                        ctypes.byref(self._h))
        if rc != capi.SN_OK:
            self._h = None
            raise SangNomError(rc, self._lib.sn_aa_last_error(None).decode())

    @property
    def nplanes(self) -> int:
        return min(self.clip.planes, 3)

    def plane_shape(self, p: int):
        return (self.clip.height >> (self.clip.subh if p else 0), self.clip.width >> (self.clip.subw if p else 0))

    def plane_shape_out(self, p: int):
        h, w = self.plane_shape(p)
        return (2 * h, 2 * w) if self.dh and not self.reduce else (h, w)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sn_aa_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int):
        if rc != capi.SN_OK:
            raise SangNomError(rc, self._lib.sn_aa_last_error(self._h).decode())

    def synchronize(self):
        self._check(self._lib.sn_aa_synchronize(self._h))

    def stream_handle(self) -> int:
        return self._lib.sn_aa_get_stream(self._h)

    def mask(self) -> capi.SnAAMask:
        """sn_aa_get_mask: the edge mask of this context (kind 0 when there is none)."""
        m = capi.SnAAMask(struct_size=ctypes.sizeof(capi.SnAAMask))
        self._check(self._lib.sn_aa_get_mask(self._h, ctypes.byref(m)))
        return m

    @property
    def mask_ex(self) -> capi.SnAAMaskEx:
        """sn_aa_get_mask_ex: which mask merges chroma in this context."""
        m = capi.SnAAMaskEx(struct_size=ctypes.sizeof(capi.SnAAMaskEx))
        self._check(self._lib.sn_aa_get_mask_ex(self._h, ctypes.byref(m)))
        return m

    @property
    def sharpen(self) -> capi.SnAASharpen:
        """sn_aa_get_sharpen: the contra-sharpening of this context (amount 0 when it is off)."""
        m = capi.SnAASharpen(struct_size=ctypes.sizeof(capi.SnAASharpen))
        self._check(self._lib.sn_aa_get_sharpen(self._h, ctypes.byref(m)))
        return m

    @property
    def repair(self) -> capi.SnAARepair:
        """sn_aa_get_repair: the rank repair of this context (rank 0 when it is off)."""
        m = capi.SnAARepair(struct_size=ctypes.sizeof(capi.SnAARepair))
        self._check(self._lib.sn_aa_get_repair(self._h, ctypes.byref(m)))
        return m

    @property
    def fields(self) -> capi.SnAAFields:
        """sn_aa_get_fields: which fields the passes of this context interpolate (mode 0 one, 1 both)."""
        m = capi.SnAAFields(struct_size=ctypes.sizeof(capi.SnAAFields))
        self._check(self._lib.sn_aa_get_fields(self._h, ctypes.byref(m)))
        return m

    def info(self, pass_: int) -> capi.SnInfo:
        """sn_get_info of one of the filter instances: 0 the turned clip's, 1 the clip's; fields="both": 2 and 3 their order-2 twins."""
        i = capi.SnInfo(struct_size=ctypes.sizeof(capi.SnInfo))
        self._check(self._lib.sn_aa_get_info(self._h, int(pass_), ctypes.byref(i)))
        return i

    def parts_info(self, pass_: int) -> capi.SnPartsInfo:
        """sn_get_parts_info of one of the two filter instances (the second pass of dh=True is twice the clip's width)."""
        i = capi.SnPartsInfo(struct_size=ctypes.sizeof(capi.SnPartsInfo))
        self._check(self._lib.sn_aa_get_parts_info(self._h, int(pass_), ctypes.byref(i)))
        return i


class SangNomAA(_AAContext):
    """The idiom on device-resident batches (sn_aa_process_device_strided): the frames stay on the device between the
    two passes."""

    def __init__(self, clip: ClipFormat, max_batch: int = 1, device: int = 0, **kw):
        super().__init__(clip, max_batch=max_batch, device=device, **kw)

    def process_batch(self, src, dst, parity=None):
        """src[p], dst[p]: torch tensors [N, H_p, W_p] on the device (dh: dst[p] is [N, 2 H_p, 2 W_p]).  Asynchronous on
        the call's stream."""
        n, B = self.nplanes, self.clip.bytes
        N = src[0].shape[0]
        sp, dp = (ctypes.c_void_p * 3)(), (ctypes.c_void_p * 3)()
        spi, dpi = (ctypes.c_int32 * 3)(), (ctypes.c_int32 * 3)()
        sfs, dfs = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
        for p in range(n):
            s, d = src[p], dst[p]
            if tuple(s.shape) != (N,) + self.plane_shape(p) or tuple(d.shape) != (N,) + self.plane_shape_out(p):
                raise ValueError(f"plane {p}: bad shape {tuple(s.shape)} -> {tuple(d.shape)}")
            if s.stride(2) != 1 or d.stride(2) != 1 or s.element_size() != B or d.element_size() != B:
                raise ValueError("planes must be x-contiguous tensors of the clip's sample type")
            if not s.is_cuda or not d.is_cuda:
                raise ValueError("process_batch needs device-resident tensors (SangNomAAHost takes host planes)")
            sp[p], dp[p] = s.data_ptr(), d.data_ptr()
            spi[p], dpi[p] = s.stride(1) * B, d.stride(1) * B
            sfs[p], dfs[p] = s.stride(0) * B, d.stride(0) * B
        par = None if parity is None else (ctypes.c_int32 * N)(*[int(x) for x in parity])
        self._check(self._lib.sn_aa_process_device_strided(self._h, N, sp, sfs, spi, dp, dfs, dpi, par))
        return dst

    def process_surfaces(self, src, dst, parity=None, src_msb=False, dst_msb=False, src_packed=None, dst_packed=None):
        """process_batch for decoder and encoder surfaces (sn_aa_process_device_surfaces): each of src and dst is either
        the planar tensors or [Y [N, H, W], UV [N, Hc, Wc, 2]] (dh: dst is [Y [N, 2 H, 2 W], UV [N, 2 Hc, 2 Wc, 2]]).
        src_msb / dst_msb, src_packed / dst_packed: as for SangNom2.process_surfaces (dh: a packed dst has rows for 2 W)."""
        s, N = _surfaces_of(src, self.plane_shape, self.nplanes, self.clip.bytes, "src", src_msb, src_packed)
        d, Nd = _surfaces_of(dst, self.plane_shape_out, self.nplanes, self.clip.bytes, "dst", dst_msb, dst_packed)
        if N != Nd:
            raise ValueError("src and dst must carry the same number of frames")
        par = None if parity is None else (ctypes.c_int32 * N)(*[int(x) for x in parity])
        self._check(self._lib.sn_aa_process_device_surfaces(self._h, N, ctypes.byref(s), ctypes.byref(d), par))
        return dst

    def surface_info(self) -> capi.SnSurfaceInfo:
        """What the surface calls of this context have done (sn_aa_get_surface_info)."""
        i = capi.SnSurfaceInfo(struct_size=ctypes.sizeof(capi.SnSurfaceInfo))
        self._check(self._lib.sn_aa_get_surface_info(self._h, ctypes.byref(i)))
        return i


class SangNomAAHost(_AAContext):
    """The idiom on host planes (sn_aa_process_host; sn_aa_submit_host / sn_aa_collect_host for look-ahead): the frame
    crosses PCIe once each way.  This is what the plugin function SangNomAA (host/sangnom2_avs_plugin.cpp) binds."""

    def _plane_args(self, planes, shape_of=None):
        ptr, pitch = (ctypes.c_void_p * 3)(), (ctypes.c_int32 * 3)()
        for p in range(self.nplanes):
            a = planes[p]
            if a.dtype != self.clip.dtype or a.strides[1] != self.clip.bytes:
                raise ValueError("planes must be x-contiguous arrays of the clip's sample type")
            if shape_of is not None and a.shape != shape_of(p):
                raise ValueError(f"plane {p}: shape {a.shape}, expected {shape_of(p)}")
            ptr[p], pitch[p] = a.ctypes.data, a.strides[0]
        return ptr, pitch

    def get_frame(self, src, parity: int = 1, dst=None):
        sp, spi = self._plane_args(src, self.plane_shape if self.dh else None)
        if dst is None:
            dst = [np.zeros(self.plane_shape_out(p), dtype=self.clip.dtype) if self.dh else np.zeros_like(src[p]) for p in range(self.nplanes)]
        dp, dpi = self._plane_args(dst, self.plane_shape_out if self.dh else None)
        self._check(self._lib.sn_aa_process_host(self._h, sp, spi, dp, dpi, int(parity)))
        return dst

    def slots(self) -> int:
        return self._lib.sn_aa_host_slots(self._h)

    def submit(self, src, parity: int = 1) -> int:
        """Queue one host frame on the ring; returns its slot (SangNomError with code SN_ERR_BUSY when the ring is full)."""
        sp, spi = self._plane_args(src, self.plane_shape if self.dh else None)
        slot = ctypes.c_int32(-1)
        self._check(self._lib.sn_aa_submit_host(self._h, sp, spi, int(parity), ctypes.byref(slot)))
        return slot.value

    def collect(self, slot: int, dst=None):
        """Wait for the frame in `slot`; returns its planes."""
        if dst is None:
            dst = [np.zeros(self.plane_shape_out(p), dtype=self.clip.dtype) for p in range(self.nplanes)]
        dp, dpi = self._plane_args(dst, self.plane_shape_out if self.dh else None)
        self._check(self._lib.sn_aa_collect_host(self._h, int(slot), dp, dpi))
        return dst
