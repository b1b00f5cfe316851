// sn_surface_layout.h -- what a value of sn_surfaces.layout means, on the host only (no device code: a host compiler takes this
// header as it is, tests/c/surface_layout_check.cpp checks it against values written out by hand).
//   which planes a surface has and which of plane[0..2] must be NULL,
//   how long a row of each plane is for a width and a sample size, and what base, pitch and frame stride must be multiples of,
//   which context a layout needs.
// The device side of the packed layouts is sn_packed.hip, that of the semi-planar and MSB-aligned ones sn_uv.hip.
#pragma once
#include <stdint.h>

#include "sangnom_hip.h"

namespace sn {

enum Packing { kNotPacked = 0, kPackedYuyv = 1, kPackedUyvy = 2, kPackedV210 = 3 };

struct SurfaceLayout {
    bool valid = false;
    bool semi = false;  // plane[1] is a plane of U,V pairs
    bool msb = false;   // 16-bit words, the sample in the high bits
    int packing = kNotPacked;  // one plane holds Y, U and V
};

inline SurfaceLayout surface_layout(int layout)
{
    SurfaceLayout d;
    d.valid = true;
    switch (layout) {
    case SN_LAYOUT_PLANAR: break;
    case SN_LAYOUT_SEMIPLANAR: d.semi = true; break;
    case SN_LAYOUT_PLANAR_MSB: d.msb = true; break;
    case SN_LAYOUT_SEMIPLANAR_MSB: d.semi = d.msb = true; break;
    case SN_LAYOUT_PACKED_YUYV: d.packing = kPackedYuyv; break;
    case SN_LAYOUT_PACKED_UYVY: d.packing = kPackedUyvy; break;
    case SN_LAYOUT_PACKED_YUYV_MSB: d.packing = kPackedYuyv, d.msb = true; break;
    case SN_LAYOUT_PACKED_UYVY_MSB: d.packing = kPackedUyvy, d.msb = true; break;
    case SN_LAYOUT_PACKED_V210: d.packing = kPackedV210; break;
    default: d.valid = false;  // 4..7 and everything beyond the enum
    }
    return d;
}

// planes a description of this layout carries on a context with `planes` planes; plane[p] for p at or beyond it must be NULL
// where surface_null_planes says so
inline int surface_planes(const SurfaceLayout& d, int planes) { return d.packing ? 1 : d.semi ? 2 : planes; }

// first plane index that must be NULL (3: none): plane[2] of a semi-planar surface, plane[1] and plane[2] of a packed one
inline int surface_null_from(const SurfaceLayout& d) { return d.packing ? 1 : d.semi ? 2 : 3; }

// bytes of a row of plane p: w_luma and w_chroma are the widths in samples of that side, B the bytes per sample
inline int64_t surface_row_bytes(const SurfaceLayout& d, int p, int w_luma, int w_chroma, int B)
{
    if (d.packing == kPackedV210) return 16 * (((int64_t)w_luma + 5) / 6);
    if (d.packing) return 2 * (int64_t)w_luma * B;
    if (p == 0) return (int64_t)w_luma * B;
    return (int64_t)(d.semi ? 2 : 1) * w_chroma * B;
}

// what base, pitch and frame stride must be multiples of: the sample, or v210's 32-bit word
inline int surface_align(const SurfaceLayout& d, int B) { return d.packing == kPackedV210 ? 4 : B; }

// zero bits below every sample of a 16-bit word
inline int surface_shift(const SurfaceLayout& d, int bits) { return d.msb ? 16 - bits : 0; }

// nullptr when a context with these properties takes the layout, otherwise why not (SN_ERR_UNSUPPORTED; every text names layout
// or the property that is in the way)
inline const char* surface_refusal(const SurfaceLayout& d, int planes, int sub_w, int sub_h, int B, int bits)
{
    if (d.msb && B != 2) return "sn_surfaces.layout SN_LAYOUT_*_MSB needs bytes_per_sample == 2 (the sample in the high bits of a 16-bit word)";
    if (d.semi && planes < 3) return "SN_LAYOUT_SEMIPLANAR needs a context with num_planes == 3";
    if (d.semi && B == 4) return "SN_LAYOUT_SEMIPLANAR with bytes_per_sample == 4: no such surface exists";
    if (d.packing) {
        if (planes != 3 || sub_w != 1 || sub_h != 0)
            return "sn_surfaces.layout SN_LAYOUT_PACKED_* needs a 4:2:2 context (num_planes == 3, sub_w == 1, sub_h == 0)";
        if (B != 1 && B != 2) return "sn_surfaces.layout SN_LAYOUT_PACKED_* needs bytes_per_sample 1 or 2";
        if (d.packing == kPackedV210 && bits != 10) return "sn_surfaces.layout SN_LAYOUT_PACKED_V210 needs bits_per_sample == 10";
    }
    return nullptr;
}

}  // namespace sn
