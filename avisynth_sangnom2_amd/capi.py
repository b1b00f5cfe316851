"""ctypes binding of libsangnom_hip.so (include/sangnom_hip.h).

This module is plumbing: it loads the in-tree shared library and declares the C ABI.  It fails
loudly (ImportError at load()) if the library has not been built -- there is no Python or CPU
fallback for the kernels.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsangnom_hip.so")

SN_OK, SN_ERR_INVALID_ARG, SN_ERR_CONFIG, SN_ERR_HIP, SN_ERR_NO_DEVICE, SN_ERR_UNSUPPORTED, SN_ERR_BUSY = range(7)
SN_MODE_AUTO, SN_MODE_POOL, SN_MODE_FUSED = range(3)
MODES = {"auto": SN_MODE_AUTO, "pool": SN_MODE_POOL, "fused": SN_MODE_FUSED}

# every symbol include/sangnom_hip.h declares
EXPORTS = (
    "sn_abi_version", "sn_validate", "sn_create", "sn_destroy", "sn_last_error",
    "sn_process_host", "sn_process_device", "sn_process_device_strided", "sn_synchronize",
    "sn_get_stream", "sn_get_info", "sn_debug_read_pool", "sn_debug_read_coupled_rows",
    "sn_host_slots", "sn_submit_host", "sn_collect_host", "sn_turn_device",
    "sn_aa_create", "sn_aa_process_host", "sn_aa_last_error", "sn_aa_destroy",
    "sn_pin_host_buffer", "sn_unpin_host_buffer", "sn_submit_host_to", "sn_debug_set_bands",
    "sn_create_with_policy", "sn_get_policy", "sn_set_policy", "sn_aa_create_with_policy",
    "sn_debug_raise_chain_fault",
    "sn_create_ex", "sn_aa_create_ex", "sn_get_arithmetic",
    "sn_aa_process_device_strided", "sn_aa_synchronize", "sn_aa_get_stream", "sn_aa_get_info",
    "sn_aa_host_slots", "sn_aa_submit_host", "sn_aa_collect_host",
    "sn_get_parts_info", "sn_aa_get_parts_info", "sn_debug_set_column_parts",
    "sn_process_device_surfaces", "sn_aa_process_device_surfaces", "sn_get_surface_info", "sn_aa_get_surface_info",
    "sn_aa_get_reduce", "sn_reduce_device", "sn_aa_get_mask", "sn_mask_merge_device",
    "sn_aa_get_mask_ex", "sn_mask_merge_luma_device",
    "sn_aa_get_sharpen", "sn_contra_sharpen_device",
    "sn_aa_get_fields", "sn_merge_device", "sn_turn_merge_device",
    "sn_aa_get_repair", "sn_repair_device",
)
# ... and the ones whose names end in a digit
EXPORTS_NUMBERED = ("sn_aa_create_ex2", "sn_aa_create_ex3", "sn_aa_create_ex4", "sn_aa_create_ex5", "sn_aa_create_ex6", "sn_aa_create_ex7")

# sn_aa_options.reduce: the anti-aliasing call with dh returns the frame at source size (sangnom_hip.h has the arithmetic)
SN_AA_REDUCE_NONE, SN_AA_REDUCE_TENT, SN_AA_REDUCE_HALFBAND = 0, 1, 2
REDUCE_KERNELS = {0: SN_AA_REDUCE_NONE, None: SN_AA_REDUCE_NONE, False: SN_AA_REDUCE_NONE, "none": SN_AA_REDUCE_NONE,
                  "tent": SN_AA_REDUCE_TENT, 1: SN_AA_REDUCE_TENT, "halfband": SN_AA_REDUCE_HALFBAND, 2: SN_AA_REDUCE_HALFBAND}

# sn_surfaces.layout: planar Y, U, V or Y plus one plane of U,V pairs (NV12, P010 / P016, NV16, NV24); _MSB: 16-bit words
# with the sample in the high bits (P010 on a 10-bit context, P012 on a 12-bit one)
SN_LAYOUT_PLANAR, SN_LAYOUT_SEMIPLANAR, SN_LAYOUT_PLANAR_MSB, SN_LAYOUT_SEMIPLANAR_MSB = 0, 1, 2, 3
# packed 4:2:2, one plane: YUY2 / Y216, UYVY / v216, their MSB-aligned forms (Y210 on a 10-bit context, Y212 on a 12-bit one), v210
SN_LAYOUT_PACKED_YUYV, SN_LAYOUT_PACKED_UYVY, SN_LAYOUT_PACKED_YUYV_MSB, SN_LAYOUT_PACKED_UYVY_MSB, SN_LAYOUT_PACKED_V210 = 8, 9, 10, 11, 12
PACKED_LAYOUTS = {("yuyv", False): SN_LAYOUT_PACKED_YUYV, ("uyvy", False): SN_LAYOUT_PACKED_UYVY, ("yuyv", True): SN_LAYOUT_PACKED_YUYV_MSB,
                  ("uyvy", True): SN_LAYOUT_PACKED_UYVY_MSB, ("v210", False): SN_LAYOUT_PACKED_V210}

# sn_options.arithmetic: which of the reference's two code paths a context reproduces (sangnom_hip.h)
SN_ARITH_CXX, SN_ARITH_SSE2 = 0, 1

SN_SMALL_AUTO, SN_SMALL_SWEEP = 0, 1
# What a filter object asks for when its caller says nothing (all zeros = the library's defaults).  The test suite
# changes entries here (small clips would otherwise never reach the whole-plane sweeps); the library itself reads no
# environment variable.
POLICY_DEFAULTS = {"small_launches": SN_SMALL_AUTO, "chain": 0, "copy_threads": 0, "scratch_budget_mb": 0, "chroma_sweeps": 0,
                   "sse2_sweeps": 0}


class SnConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "struct_size", "width", "height", "bytes_per_sample", "bits_per_sample", "num_planes",
        "sub_w", "sub_h", "order", "aa", "aac", "dh", "luma", "chroma", "device", "max_batch",
        "mode", "host_depth", "isolated_planes", "fresh_pool")] + [("stream", ctypes.c_void_p)]


class SnPolicy(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("struct_size", "small_launches", "chain", "copy_threads", "scratch_budget_mb", "chroma_sweeps",
                                                 "sse2_sweeps")] + [("reserved", ctypes.c_int32 * 1)]


class SnOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("arithmetic", ctypes.c_int32), ("column_parts", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 5)]


class SnAAOptions(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("reduce", ctypes.c_int32), ("reserved", ctypes.c_int32 * 6)]


def aa_options(reduce=0) -> "SnAAOptions":
    """sn_aa_options: reduce = 0, "tent" (1) or "halfband" (2)."""
    if reduce not in REDUCE_KERNELS:
        raise ValueError("reduce must be 0, 'tent' or 'halfband'")
    return SnAAOptions(struct_size=ctypes.sizeof(SnAAOptions), reduce=REDUCE_KERNELS[reduce])


# sn_aa_mask.kind: the call's result is merged into the source through an edge mask of the source (sangnom_hip.h, "Edge mask")
SN_AA_MASK_NONE, SN_AA_MASK_SOBEL = 0, 1


class SnAAMask(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("kind", ctypes.c_int32), ("lo", ctypes.c_int32), ("hi", ctypes.c_int32),
                ("expand", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


def aa_mask(mask=None, expand=1) -> "SnAAMask":
    """sn_aa_mask: mask = None (no mask) or (lo, hi) in 8-bit scale; expand = 0 or 1.  The library checks the values."""
    if mask is None:
        return SnAAMask(struct_size=ctypes.sizeof(SnAAMask), kind=SN_AA_MASK_NONE)
    lo, hi = mask
    return SnAAMask(struct_size=ctypes.sizeof(SnAAMask), kind=SN_AA_MASK_SOBEL, lo=int(lo), hi=int(hi), expand=int(expand))


# sn_aa_mask_ex.chroma: which mask merges chroma -- the chroma plane's own, or the source luma plane's reduced to chroma's geometry
SN_AA_MASK_CHROMA_OWN, SN_AA_MASK_CHROMA_LUMA = 0, 1
MASK_CHROMA = {"own": SN_AA_MASK_CHROMA_OWN, "luma": SN_AA_MASK_CHROMA_LUMA}


class SnAAMaskEx(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("chroma", ctypes.c_int32), ("reserved", ctypes.c_int32 * 6)]


def aa_mask_ex(chroma="own") -> "SnAAMaskEx":
    """sn_aa_mask_ex: chroma = "own" (every plane through its own mask) or "luma" (chroma through the luma plane's mask)."""
    if not isinstance(chroma, str) or chroma not in MASK_CHROMA:
        raise ValueError("mask_chroma must be 'own' or 'luma'")
    return SnAAMaskEx(struct_size=ctypes.sizeof(SnAAMaskEx), chroma=MASK_CHROMA[chroma])


class SnAASharpen(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("amount", ctypes.c_int32), ("chroma", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5)]


def aa_sharpen(amount=None, chroma=False) -> "SnAASharpen":
    """sn_aa_sharpen: amount = None or 0 (off) or 1..255 (64 = unity); chroma = whether processed chroma planes are sharpened
    too.  The library checks the values."""
    return SnAASharpen(struct_size=ctypes.sizeof(SnAASharpen), amount=int(amount or 0), chroma=int(bool(chroma)))


# sn_aa_fields.mode: which fields a pass interpolates -- the one cfg.order names, or both (order 1 and order 2, averaged)
SN_AA_FIELDS_ONE, SN_AA_FIELDS_BOTH = 0, 1
FIELDS = {"one": SN_AA_FIELDS_ONE, "both": SN_AA_FIELDS_BOTH}


class SnAAFields(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("mode", ctypes.c_int32), ("reserved", ctypes.c_int32 * 6)]


def aa_fields(fields="one") -> "SnAAFields":
    """sn_aa_fields: fields = "one" (a pass keeps one field, as ever) or "both" (sangnom_hip.h, "Both fields")."""
    if not isinstance(fields, str) or fields not in FIELDS:
        raise ValueError("fields must be 'one' or 'both'")
    return SnAAFields(struct_size=ctypes.sizeof(SnAAFields), mode=FIELDS[fields])


class SnAARepair(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("rank", ctypes.c_int32), ("chroma", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5)]


def aa_repair(rank=None, chroma=False) -> "SnAARepair":
    """sn_aa_repair: rank = None or 0 (off) or 1..4 (sangnom_hip.h, "Rank repair"); chroma = whether processed chroma planes
    are repaired too."""
    if rank is not None and (isinstance(rank, bool) or not isinstance(rank, int) or rank < 0 or rank > 4):
        raise ValueError("repair must be None or 0 (off) or 1..4")
    return SnAARepair(struct_size=ctypes.sizeof(SnAARepair), rank=int(rank or 0), chroma=int(bool(chroma)))


class SnPartsInfo(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("parts", ctypes.c_int32 * 3), ("ghost_columns", ctypes.c_int32),
                ("part_frames", ctypes.c_int64), ("part_fallbacks", ctypes.c_int64)]


class SnSurfaces(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("layout", ctypes.c_int32), ("plane", ctypes.c_void_p * 3), ("pitch", ctypes.c_int32 * 3),
                ("reserved", ctypes.c_int32), ("frame_stride", ctypes.c_int64 * 3)]


class SnSurfaceInfo(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("reserved", ctypes.c_int32), ("scratch_bytes", ctypes.c_int64),
                ("split_frames", ctypes.c_int64), ("merged_frames", ctypes.c_int64), ("copied_frames", ctypes.c_int64)]


def surfaces(layout: int, planes, pitches, frame_strides) -> "SnSurfaces":
    """sn_surfaces from device pointers, pitches and frame strides in bytes (two entries for SN_LAYOUT_SEMIPLANAR and
    SN_LAYOUT_SEMIPLANAR_MSB: Y, UV; one for SN_LAYOUT_PACKED_*).  The planes that are not given stay NULL."""
    s = SnSurfaces(struct_size=ctypes.sizeof(SnSurfaces), layout=int(layout))
    for p, (ptr, pitch, fs) in enumerate(zip(planes, pitches, frame_strides)):
        s.plane[p], s.pitch[p], s.frame_stride[p] = ptr, int(pitch), int(fs)
    return s


def options(arithmetic: int = SN_ARITH_CXX, column_parts: int = 0) -> "SnOptions":
    """sn_options: what is fixed at creation.  column_parts=1: 16-bit and float planes wider than one workgroup of the
    sweeps holds (3840 columns) are swept in column parts (sangnom_hip.h)."""
    return SnOptions(struct_size=ctypes.sizeof(SnOptions), arithmetic=int(arithmetic), column_parts=int(column_parts))


def arithmetic_of_opt(opt: int) -> int:
    """The script argument `opt`: 1 asks for the reference's SSE2 arithmetic; 0 and -1 are its C++ arithmetic (this
    library's default -- upstream's own -1 means SSE2 on x86-64)."""
    return SN_ARITH_SSE2 if opt == 1 else SN_ARITH_CXX


def policy(**over) -> "SnPolicy":
    """sn_policy from POLICY_DEFAULTS with the given fields replaced (None = keep the default)."""
    v = dict(POLICY_DEFAULTS)
    v.update({k: x for k, x in over.items() if x is not None})
    return SnPolicy(struct_size=ctypes.sizeof(SnPolicy), **{k: int(x) for k, x in v.items()})


class SnInfo(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("out_height", ctypes.c_int32),
                ("pool_stride", ctypes.c_int32), ("pool_rows", ctypes.c_int32),
                ("fused_eligible", ctypes.c_int32), ("history_free", ctypes.c_int32),
                ("frames", ctypes.c_int64), ("fused_frames", ctypes.c_int64),
                ("coupled_rows", ctypes.c_int32), ("uv_sweeps", ctypes.c_int32),
                ("threshold", ctypes.c_double * 3),
                ("banded_frames", ctypes.c_int64), ("band_fallbacks", ctypes.c_int64),
                ("chained_frames", ctypes.c_int64), ("chain_redone", ctypes.c_int64)]


def build(force: bool = False) -> str:
    """Compile libsangnom_hip.so for gfx950 with hipcc (csrc/Makefile)."""
    args = ["make", "-s", "-C", os.path.join(_HERE, "csrc")]
    if force:
        subprocess.check_call(args + ["clean"])
    subprocess.check_call(args + ["-j4"])
    return LIB_PATH


_lib = None


def _share_torch_hip_runtime():
    """One process must hold ONE HIP runtime.  PyTorch-ROCm wheels bundle their own libamdhip64.so
    (SONAME libamdhip64.so.7, the same SONAME libsangnom_hip.so needs); if the system copy were
    loaded first, a later `import torch` would load a second runtime and find no GPU.  So when torch
    is installed its runtime is loaded first and libsangnom_hip.so binds to it by SONAME.  Without
    torch (a plain C/C++ host such as the AviSynth adapter) the RUNPATH copy under /opt/rocm is used."""
    try:
        import torch  # noqa: F401
    except Exception:
        return
    cand = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)


def load():
    """Load the library and declare prototypes.  Raises ImportError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    _share_torch_hip_runtime()
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    p3v, p3i, p3l = ctypes.POINTER(vp), ctypes.POINTER(i32), ctypes.POINTER(i64)
    L.sn_abi_version.restype = ctypes.c_int
    L.sn_validate.argtypes = [ctypes.POINTER(SnConfig), ctypes.c_char_p, ctypes.c_size_t]
    L.sn_create.argtypes = [ctypes.POINTER(SnConfig), ctypes.POINTER(vp)]
    L.sn_create_with_policy.argtypes = [ctypes.POINTER(SnConfig), ctypes.POINTER(SnPolicy), ctypes.POINTER(vp)]
    L.sn_create_ex.argtypes = [ctypes.POINTER(SnConfig), ctypes.POINTER(SnPolicy), ctypes.POINTER(SnOptions), ctypes.POINTER(vp)]
    L.sn_aa_create_ex.argtypes = [ctypes.POINTER(SnConfig), ctypes.POINTER(SnPolicy), ctypes.POINTER(SnOptions), ctypes.POINTER(vp)]
    L.sn_aa_create_ex2.argtypes = [ctypes.POINTER(SnConfig), ctypes.POINTER(SnPolicy), ctypes.POINTER(SnOptions), ctypes.POINTER(SnAAOptions),
                                   ctypes.POINTER(vp)]
    L.sn_aa_create_ex3.argtypes = [ctypes.POINTER(SnConfig), ctypes.POINTER(SnPolicy), ctypes.POINTER(SnOptions), ctypes.POINTER(SnAAOptions),
                                   ctypes.POINTER(SnAAMask), ctypes.POINTER(vp)]
    L.sn_aa_get_mask.argtypes = [vp, ctypes.POINTER(SnAAMask)]
    L.sn_aa_create_ex4.argtypes = [ctypes.POINTER(SnConfig), ctypes.POINTER(SnPolicy), ctypes.POINTER(SnOptions), ctypes.POINTER(SnAAOptions),
                                   ctypes.POINTER(SnAAMask), ctypes.POINTER(SnAAMaskEx), ctypes.POINTER(vp)]
    L.sn_aa_get_mask_ex.argtypes = [vp, ctypes.POINTER(SnAAMaskEx)]
    L.sn_aa_create_ex5.argtypes = [ctypes.POINTER(SnConfig), ctypes.POINTER(SnPolicy), ctypes.POINTER(SnOptions), ctypes.POINTER(SnAAOptions),
                                   ctypes.POINTER(SnAAMask), ctypes.POINTER(SnAAMaskEx), ctypes.POINTER(SnAASharpen), ctypes.POINTER(vp)]
    L.sn_aa_get_sharpen.argtypes = [vp, ctypes.POINTER(SnAASharpen)]
    L.sn_aa_create_ex6.argtypes = [ctypes.POINTER(SnConfig), ctypes.POINTER(SnPolicy), ctypes.POINTER(SnOptions), ctypes.POINTER(SnAAOptions),
                                   ctypes.POINTER(SnAAMask), ctypes.POINTER(SnAAMaskEx), ctypes.POINTER(SnAASharpen), ctypes.POINTER(SnAAFields),
                                   ctypes.POINTER(vp)]
    L.sn_aa_get_fields.argtypes = [vp, ctypes.POINTER(SnAAFields)]
    L.sn_aa_create_ex7.argtypes = [ctypes.POINTER(SnConfig), ctypes.POINTER(SnPolicy), ctypes.POINTER(SnOptions), ctypes.POINTER(SnAAOptions),
                                   ctypes.POINTER(SnAAMask), ctypes.POINTER(SnAAMaskEx), ctypes.POINTER(SnAASharpen), ctypes.POINTER(SnAAFields),
                                   ctypes.POINTER(SnAARepair), ctypes.POINTER(vp)]
    L.sn_aa_get_repair.argtypes = [vp, ctypes.POINTER(SnAARepair)]
    L.sn_repair_device.argtypes = [vp, i32, i32, vp, i64, i32, vp, i64, i32, i32, i32, vp, i64, i32]
    L.sn_merge_device.argtypes = [vp, i32, vp, i64, i32, vp, i64, i32, i32, i32, vp, i64, i32]
    L.sn_turn_merge_device.argtypes = [vp, i32, i32, vp, i64, i32, vp, i64, i32, i32, i32, vp, i64, i32]
    L.sn_contra_sharpen_device.argtypes = [vp, i32, i32, vp, i64, i32, vp, i64, i32, i32, i32, vp, i64, i32]
    L.sn_mask_merge_luma_device.argtypes = [vp, ctypes.POINTER(SnAAMask), i32, vp, i64, i32, i32, i32, p3v, p3l, p3i, p3v, p3l, p3i, i32, i32,
                                            p3v, p3l, p3i]
    L.sn_mask_merge_device.argtypes = [vp, ctypes.POINTER(SnAAMask), i32, vp, i64, i32, vp, i64, i32, i32, i32, vp, i64, i32]
    L.sn_aa_get_reduce.argtypes = [vp]
    L.sn_reduce_device.argtypes = [vp, i32, i32, vp, i64, i32, i32, i32, i32, i32, vp, i64, i32]
    L.sn_get_arithmetic.argtypes = [vp]
    L.sn_get_policy.argtypes = [vp, ctypes.POINTER(SnPolicy)]
    L.sn_set_policy.argtypes = [vp, ctypes.POINTER(SnPolicy)]
    L.sn_aa_create_with_policy.argtypes = [ctypes.POINTER(SnConfig), ctypes.POINTER(SnPolicy), ctypes.POINTER(vp)]
    L.sn_destroy.argtypes = [vp]
    L.sn_destroy.restype = None
    L.sn_last_error.argtypes = [vp]
    L.sn_last_error.restype = ctypes.c_char_p
    L.sn_process_host.argtypes = [vp, p3v, p3i, p3v, p3i, i32]
    L.sn_process_device.argtypes = [vp, p3v, p3i, p3v, p3i, i32]
    L.sn_host_slots.argtypes = [vp]
    L.sn_turn_device.argtypes = [vp, i32, i32, vp, ctypes.c_int64, i32, i32, i32, vp, ctypes.c_int64, i32]
    L.sn_submit_host.argtypes = [vp, p3v, p3i, i32, ctypes.POINTER(i32)]
    L.sn_collect_host.argtypes = [vp, i32, p3v, p3i]
    L.sn_process_device_strided.argtypes = [vp, i32, p3v, p3l, p3i, p3v, p3l, p3i, p3i]
    L.sn_synchronize.argtypes = [vp]
    L.sn_get_stream.argtypes = [vp]
    L.sn_get_stream.restype = vp
    L.sn_get_info.argtypes = [vp, ctypes.POINTER(SnInfo)]
    L.sn_debug_read_pool.argtypes = [vp, i32, vp, ctypes.c_size_t]
    L.sn_debug_read_coupled_rows.argtypes = [vp, i32, vp, ctypes.c_size_t]
    L.sn_debug_set_bands.argtypes = [vp, i32, i32]
    L.sn_debug_raise_chain_fault.argtypes = [vp]
    L.sn_pin_host_buffer.argtypes = [vp, ctypes.c_size_t]
    L.sn_unpin_host_buffer.argtypes = [vp]
    L.sn_submit_host_to.argtypes = [vp, p3v, p3i, p3v, p3i, i32, ctypes.POINTER(i32)]
    L.sn_aa_create.argtypes = [ctypes.POINTER(SnConfig), ctypes.POINTER(vp)]
    L.sn_aa_process_host.argtypes = [vp, p3v, p3i, p3v, p3i, i32]
    L.sn_aa_last_error.argtypes = [vp]
    L.sn_aa_last_error.restype = ctypes.c_char_p
    L.sn_aa_destroy.argtypes = [vp]
    L.sn_aa_destroy.restype = None
    L.sn_aa_process_device_strided.argtypes = [vp, i32, p3v, p3l, p3i, p3v, p3l, p3i, p3i]
    L.sn_aa_synchronize.argtypes = [vp]
    L.sn_aa_get_stream.argtypes = [vp]
    L.sn_aa_get_stream.restype = vp
    L.sn_aa_get_info.argtypes = [vp, i32, ctypes.POINTER(SnInfo)]
    L.sn_aa_host_slots.argtypes = [vp]
    L.sn_aa_submit_host.argtypes = [vp, p3v, p3i, i32, ctypes.POINTER(i32)]
    L.sn_aa_collect_host.argtypes = [vp, i32, p3v, p3i]
    L.sn_get_parts_info.argtypes = [vp, ctypes.POINTER(SnPartsInfo)]
    L.sn_aa_get_parts_info.argtypes = [vp, i32, ctypes.POINTER(SnPartsInfo)]
    L.sn_debug_set_column_parts.argtypes = [vp, i32, i32]
    L.sn_process_device_surfaces.argtypes = [vp, i32, ctypes.POINTER(SnSurfaces), ctypes.POINTER(SnSurfaces), p3i]
    L.sn_aa_process_device_surfaces.argtypes = [vp, i32, ctypes.POINTER(SnSurfaces), ctypes.POINTER(SnSurfaces), p3i]
    L.sn_get_surface_info.argtypes = [vp, ctypes.POINTER(SnSurfaceInfo)]
    L.sn_aa_get_surface_info.argtypes = [vp, ctypes.POINTER(SnSurfaceInfo)]
    _lib = L
    return L
