"""The surface calls' ABI without a GPU: the symbols, the two new structs as a C compiler lays them out, and every older
struct and the ABI version unchanged (the change is additive)."""
import ctypes
import os
import re
import subprocess

import numpy as np

from avisynth_sangnom2_amd import capi, clip_format
from tests import surface_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sn_process_device_surfaces", "sn_aa_process_device_surfaces", "sn_get_surface_info", "sn_aa_get_surface_info")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "sangnom_hip.h"
#define OFF(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void)
{
    printf("sn_surfaces %zu\n", sizeof(sn_surfaces));
    OFF(sn_surfaces, struct_size); OFF(sn_surfaces, layout); OFF(sn_surfaces, plane); OFF(sn_surfaces, pitch);
    OFF(sn_surfaces, reserved); OFF(sn_surfaces, frame_stride);
    printf("sn_surface_info %zu\n", sizeof(sn_surface_info));
    OFF(sn_surface_info, struct_size); OFF(sn_surface_info, reserved); OFF(sn_surface_info, scratch_bytes);
    OFF(sn_surface_info, split_frames); OFF(sn_surface_info, merged_frames); OFF(sn_surface_info, copied_frames);
    printf("sn_config %zu\nsn_policy %zu\nsn_options %zu\nsn_info %zu\nsn_parts_info %zu\n", sizeof(sn_config), sizeof(sn_policy),
           sizeof(sn_options), sizeof(sn_info), sizeof(sn_parts_info));
    printf("SN_ABI_VERSION %d\nlayouts %d %d\n", SN_ABI_VERSION, SN_LAYOUT_PLANAR, SN_LAYOUT_SEMIPLANAR);
    return 0;
}
"""


def _probe(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=60).stdout
    return {k: [int(x) for x in v.split()] for k, v in (line.split(" ", 1) for line in out.strip().splitlines())}


def test_new_symbols_are_declared_exported_and_mirrored(hip_lib):
    header = open(os.path.join(ROOT, "include", "sangnom_hip.h")).read()
    declared = set(re.findall(r"\b(sn_[a-z_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in capi.EXPORTS and hasattr(hip_lib, name), name
        assert getattr(hip_lib, name).argtypes is not None, f"{name} has no argtypes"
    assert hip_lib.sn_abi_version() == 4


def test_struct_layouts_in_c_and_in_the_mirror(tmp_path):
    c = _probe(tmp_path)
    assert c["sn_surfaces"] == [72] and c["sn_surface_info"] == [40]
    want = dict(struct_size=0, layout=4, plane=8, pitch=32, reserved=44, frame_stride=48)
    for f, off in want.items():
        assert c[f"sn_surfaces.{f}"] == [off] and getattr(capi.SnSurfaces, f).offset == off, f
    want = dict(struct_size=0, reserved=4, scratch_bytes=8, split_frames=16, merged_frames=24, copied_frames=32)
    for f, off in want.items():
        assert c[f"sn_surface_info.{f}"] == [off] and getattr(capi.SnSurfaceInfo, f).offset == off, f
    assert ctypes.sizeof(capi.SnSurfaces) == 72 and ctypes.sizeof(capi.SnSurfaceInfo) == 40
    assert c["SN_ABI_VERSION"] == [4] and c["layouts"] == [capi.SN_LAYOUT_PLANAR, capi.SN_LAYOUT_SEMIPLANAR] == [0, 1]


def test_older_structs_keep_their_sizes(tmp_path):
    """sn_config 88, sn_policy 32, sn_options 32, sn_info 104, sn_parts_info 40: what ABI version 4 had before the surfaces."""
    c = _probe(tmp_path)
    assert (c["sn_config"], c["sn_policy"], c["sn_options"], c["sn_info"], c["sn_parts_info"]) == ([88], [32], [32], [104], [40])
    for name, mirror in (("sn_config", capi.SnConfig), ("sn_policy", capi.SnPolicy), ("sn_options", capi.SnOptions), ("sn_info", capi.SnInfo),
                         ("sn_parts_info", capi.SnPartsInfo)):
        assert ctypes.sizeof(mirror) == c[name][0], name


def test_null_context_is_refused(hip_lib):
    s = capi.surfaces(capi.SN_LAYOUT_PLANAR, [0], [0], [0])
    i = capi.SnSurfaceInfo(struct_size=ctypes.sizeof(capi.SnSurfaceInfo))
    assert hip_lib.sn_process_device_surfaces(None, 1, ctypes.byref(s), ctypes.byref(s), None) == capi.SN_ERR_INVALID_ARG
    assert hip_lib.sn_aa_process_device_surfaces(None, 1, ctypes.byref(s), ctypes.byref(s), None) == capi.SN_ERR_INVALID_ARG
    assert hip_lib.sn_get_surface_info(None, ctypes.byref(i)) == capi.SN_ERR_INVALID_ARG
    assert hip_lib.sn_aa_get_surface_info(None, ctypes.byref(i)) == capi.SN_ERR_INVALID_ARG


def test_the_helpers_of_the_gpu_tests():
    """Interleaving, the odd layout's alignment classes, and the scratch formula the chunking test relies on."""
    u, v = np.arange(6, dtype=np.uint8).reshape(2, 3), 100 + np.arange(6, dtype=np.uint8).reshape(2, 3)
    assert sc.uv_rows(u, v).tolist() == [[0, 100, 1, 101, 2, 102], [3, 103, 4, 104, 5, 105]]
    assert sc.interleave(u, v).shape == (2, 3, 2)
    for B in (1, 2):
        for name in sc.SURFACE_LAYOUTS:
            ly, luv = sc.surface_layouts(name, [(64, 256), (32, 128)], B, 3)
            assert luv.row == 2 * 128 * B and luv.rows == 32 and ly.row == 256 * B
            for L in (ly, luv):
                assert L.base % B == 0 and L.pitch % B == 0 and L.stride % B == 0 and L.pitch >= L.row and L.stride > L.rows * L.pitch
                if name == "odd":
                    assert L.base % (2 * B) and L.pitch % (2 * B), "the odd layout must not be aligned beyond the sample size"
                else:
                    assert L.base % 16 == 0 and L.pitch % 16 == 0 and L.stride % 16 == 0
    clip = clip_format(sc.CHUNKED.fmt, sc.CHUNKED.w, sc.CHUNKED.h)
    assert sc.scratch_frame_bytes(clip) == 2 * (256 * 20 + 256 * 20)
    assert sc.scratch_frames(clip, sc.CHUNKED.n, 1) == 3, "four frames must take two chunks under a budget of 1 MiB"
    assert sc.scratch_frames(clip, 4, 24576) == 4
    assert len({c.id for c in sc.PARITY}) == len(sc.PARITY)
