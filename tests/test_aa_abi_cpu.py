"""The anti-aliasing call's additions to the C ABI, as far as they can be checked without a GPU: declared, exported, and
a NULL context refused before any device is touched."""
import ctypes
import os
import re

from avisynth_sangnom2_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sn_aa_process_device_strided", "sn_aa_synchronize", "sn_aa_get_stream", "sn_aa_get_info", "sn_aa_host_slots",
       "sn_aa_submit_host", "sn_aa_collect_host")


def test_header_declares_and_library_exports_the_new_entry_points(hip_lib):
    header = open(os.path.join(ROOT, "include", "sangnom_hip.h")).read()
    declared = set(re.findall(r"\b(sn_[a-z_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, f"include/sangnom_hip.h does not declare {name}"
        assert name in capi.EXPORTS
        assert hasattr(hip_lib, name), f"libsangnom_hip.so does not export {name}"
    assert hip_lib.sn_abi_version() == 4  # symbols were added, nothing changed


def test_null_context_is_refused_without_touching_a_device(hip_lib):
    L = hip_lib
    p3v, p3i, p3l = (ctypes.c_void_p * 3)(), (ctypes.c_int32 * 3)(), (ctypes.c_int64 * 3)()
    slot = ctypes.c_int32(-1)
    info = capi.SnInfo(struct_size=ctypes.sizeof(capi.SnInfo))
    assert L.sn_aa_process_device_strided(None, 1, p3v, p3l, p3i, p3v, p3l, p3i, None) == capi.SN_ERR_INVALID_ARG
    assert L.sn_aa_synchronize(None) == capi.SN_ERR_INVALID_ARG
    assert L.sn_aa_get_stream(None) is None
    assert L.sn_aa_get_info(None, 0, ctypes.byref(info)) == capi.SN_ERR_INVALID_ARG
    assert L.sn_aa_host_slots(None) <= 0
    assert L.sn_aa_submit_host(None, p3v, p3i, 1, ctypes.byref(slot)) == capi.SN_ERR_INVALID_ARG
    assert L.sn_aa_collect_host(None, 0, p3v, p3i) == capi.SN_ERR_INVALID_ARG
    assert b"NULL" in L.sn_aa_last_error(None)
