// sn_uv.hip -- semi-planar chroma on the device: a UV plane of U,V sample pairs (NV12, P010 / P016, NV16, NV24: what a
// hardware decoder hands over and an encoder takes) split into a U and a V plane for the passes, and merged back.
//   split:  u[y][x] = uv[y][2x],  v[y][x] = uv[y][2x + 1]
//   merge:  uv[y][2x] = u[y][x],  uv[y][2x + 1] = v[y][x]
// Memory-bound, no reuse, so no LDS: a lane of the vector path moves 16 bytes per access -- two 16-byte loads of UV,
// de-interleaved in registers by v_perm_b32 (byte selectors for 8-bit samples, half-word selectors for 16-bit), one 16-byte
// store each of U and V; the merge is the inverse.  4 x cw x h x B bytes per frame either way (h / 2 lines in the field form).
// The vector path needs every base, pitch and frame stride of the launch to be a multiple of 16 (vec_ok, chosen per launch
// as k_turn's dword_ok); the samples of a row beyond its last whole 16 bytes of U -- and every sample of a launch that is not
// aligned -- move one sample at a time.  Whole waves take the same path up to the last one of a row.
// Field form (line_parity 0 / 1): only the lines of that parity are read and written, the lines the SangNom2 pass that
// follows keeps and the only ones it reads; the other lines of the destination are left as they were.
// Rows are addressed with 64-bit offsets; a store never reaches beyond cw x B bytes of a U or V row, 2 x cw x B of a UV row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sn_internal.h"

namespace sn {

constexpr int kUvLanes = 64;  // lanes along a row: one wave
constexpr int kUvRows = 4;    // rows per workgroup

// One side of a launch: frame f's line y starts at base + f * fs + y * pitch.
struct UvPlane {
    uint8_t* base;
    int64_t fs;
    int32_t pitch;
};

// v_perm_b32 takes bytes 0..3 from its second operand and 4..7 from its first
template <int B>
struct UvSel;
template <>
struct UvSel<1> {  // d0 = U0 V0 U1 V1, d1 = U2 V2 U3 V3
    static constexpr uint32_t even = 0x06040200u, odd = 0x07050301u;  // (d1, d0) -> U0 U1 U2 U3 / V0 V1 V2 V3
    static constexpr uint32_t lo = 0x05010400u, hi = 0x07030602u;     // (v, u)   -> U0 V0 U1 V1 / U2 V2 U3 V3
};
template <>
struct UvSel<2> {  // d0 = U0 V0, d1 = U1 V1
    static constexpr uint32_t even = 0x05040100u, odd = 0x07060302u;  // (d1, d0) -> U0 U1 / V0 V1
    static constexpr uint32_t lo = 0x05040100u, hi = 0x07060302u;     // (v, u)   -> U0 V0 / U1 V1
};

// vec_ok: vectors i < nvec of a row are 16 bytes of U and of V (32 of UV); the lanes behind them take the row's remaining
// samples.  Otherwise every lane walks samples.  Rows and frames beyond what the grid holds are looped over.
template <class T, bool kMerge>
__global__ void __launch_bounds__(kUvLanes* kUvRows) k_uv(UvPlane uv, UvPlane pu, UvPlane pv, int cw, int row0, int rstep, int nrows, int nframes,
                                                          int vec_ok)
{
    constexpr int B = (int)sizeof(T);
    constexpr int per = 16 / B;  // samples per 16 bytes
    const int nvec = vec_ok ? cw / per : 0;
    const int i = blockIdx.x * kUvLanes + threadIdx.x;
    const int lanes = gridDim.x * kUvLanes;
    for (int f = blockIdx.z; f < nframes; f += gridDim.z) {
        for (int r = blockIdx.y * kUvRows + threadIdx.y; r < nrows; r += gridDim.y * kUvRows) {
            const int64_t y = row0 + (int64_t)rstep * r;
            uint8_t* const puv = uv.base + (int64_t)f * uv.fs + y * uv.pitch;
            uint8_t* const pub = pu.base + (int64_t)f * pu.fs + y * pu.pitch;
            uint8_t* const pvb = pv.base + (int64_t)f * pv.fs + y * pv.pitch;
            if (i < nvec) {
                if constexpr (!kMerge) {
                    const uint4 a = reinterpret_cast<const uint4*>(puv)[2 * i], b = reinterpret_cast<const uint4*>(puv)[2 * i + 1];
                    uint4 u, v;
                    u.x = __builtin_amdgcn_perm(a.y, a.x, UvSel<B>::even), v.x = __builtin_amdgcn_perm(a.y, a.x, UvSel<B>::odd);
                    u.y = __builtin_amdgcn_perm(a.w, a.z, UvSel<B>::even), v.y = __builtin_amdgcn_perm(a.w, a.z, UvSel<B>::odd);
                    u.z = __builtin_amdgcn_perm(b.y, b.x, UvSel<B>::even), v.z = __builtin_amdgcn_perm(b.y, b.x, UvSel<B>::odd);
                    u.w = __builtin_amdgcn_perm(b.w, b.z, UvSel<B>::even), v.w = __builtin_amdgcn_perm(b.w, b.z, UvSel<B>::odd);
                    reinterpret_cast<uint4*>(pub)[i] = u;
                    reinterpret_cast<uint4*>(pvb)[i] = v;
                } else {
                    const uint4 u = reinterpret_cast<const uint4*>(pub)[i], v = reinterpret_cast<const uint4*>(pvb)[i];
                    uint4 a, b;
                    a.x = __builtin_amdgcn_perm(v.x, u.x, UvSel<B>::lo), a.y = __builtin_amdgcn_perm(v.x, u.x, UvSel<B>::hi);
                    a.z = __builtin_amdgcn_perm(v.y, u.y, UvSel<B>::lo), a.w = __builtin_amdgcn_perm(v.y, u.y, UvSel<B>::hi);
                    b.x = __builtin_amdgcn_perm(v.z, u.z, UvSel<B>::lo), b.y = __builtin_amdgcn_perm(v.z, u.z, UvSel<B>::hi);
                    b.z = __builtin_amdgcn_perm(v.w, u.w, UvSel<B>::lo), b.w = __builtin_amdgcn_perm(v.w, u.w, UvSel<B>::hi);
                    reinterpret_cast<uint4*>(puv)[2 * i] = a;
                    reinterpret_cast<uint4*>(puv)[2 * i + 1] = b;
                }
            } else {
                // the ragged tail of an aligned row, or the whole row of a launch that is not: one sample per access
                for (int x = nvec * per + (i - nvec); x < cw; x += lanes - nvec) {
                    if constexpr (!kMerge) {
                        reinterpret_cast<T*>(pub)[x] = reinterpret_cast<const T*>(puv)[2 * x];
                        reinterpret_cast<T*>(pvb)[x] = reinterpret_cast<const T*>(puv)[2 * x + 1];
                    } else {
                        reinterpret_cast<T*>(puv)[2 * x] = reinterpret_cast<const T*>(pub)[x];
                        reinterpret_cast<T*>(puv)[2 * x + 1] = reinterpret_cast<const T*>(pvb)[x];
                    }
                }
            }
        }
    }
}

static hipError_t launch_uv(hipStream_t st, bool merge, int bytes, int nframes, const UvPlane& uv, const UvPlane& pu, const UvPlane& pv, int cw, int h,
                            int line_parity)
{
    if (nframes <= 0 || cw <= 0 || h <= 0) return hipSuccess;
    if (bytes != 1 && bytes != 2) return hipErrorInvalidValue;
    const int row0 = line_parity < 0 ? 0 : line_parity & 1, rstep = line_parity < 0 ? 1 : 2;
    const int nrows = (h - row0 + rstep - 1) / rstep;
    if (nrows <= 0) return hipSuccess;
    auto aligned = [](const UvPlane& p) { return (uintptr_t)p.base % 16 == 0 && p.pitch % 16 == 0 && p.fs % 16 == 0; };
    const int vec_ok = aligned(uv) && aligned(pu) && aligned(pv) ? 1 : 0;
    const int per = 16 / bytes;
    // aligned: a lane per vector and one per sample of the tail (fewer than `per`); otherwise up to 16 waves walk a row's samples
    int64_t want = vec_ok ? cw / per + cw % per : (cw < 16 * kUvLanes ? cw : 16 * kUvLanes);
    const unsigned gx = (unsigned)((want + kUvLanes - 1) / kUvLanes);
    const int gy = (nrows + kUvRows - 1) / kUvRows;
    dim3 grid(gx < 1 ? 1 : gx, gy > 65535 ? 65535 : gy, nframes > 65535 ? 65535 : nframes), block(kUvLanes, kUvRows);
    if (bytes == 1) {
        if (merge) hipLaunchKernelGGL((k_uv<uint8_t, true>), grid, block, 0, st, uv, pu, pv, cw, row0, rstep, nrows, nframes, vec_ok);
        else hipLaunchKernelGGL((k_uv<uint8_t, false>), grid, block, 0, st, uv, pu, pv, cw, row0, rstep, nrows, nframes, vec_ok);
    } else {
        if (merge) hipLaunchKernelGGL((k_uv<uint16_t, true>), grid, block, 0, st, uv, pu, pv, cw, row0, rstep, nrows, nframes, vec_ok);
        else hipLaunchKernelGGL((k_uv<uint16_t, false>), grid, block, 0, st, uv, pu, pv, cw, row0, rstep, nrows, nframes, vec_ok);
    }
    return hipGetLastError();
}

hipError_t launch_uv_split(hipStream_t st, int bytes, int nframes, const uint8_t* uv, int64_t uv_fs, int uv_pitch, int cw, int h, uint8_t* u,
                           int64_t u_fs, int u_pitch, uint8_t* v, int64_t v_fs, int v_pitch, int line_parity)
{
    return launch_uv(st, false, bytes, nframes, UvPlane{const_cast<uint8_t*>(uv), uv_fs, uv_pitch}, UvPlane{u, u_fs, u_pitch}, UvPlane{v, v_fs, v_pitch}, cw,
                     h, line_parity);
}

hipError_t launch_uv_merge(hipStream_t st, int bytes, int nframes, const uint8_t* u, int64_t u_fs, int u_pitch, const uint8_t* v, int64_t v_fs,
                           int v_pitch, int cw, int h, uint8_t* uv, int64_t uv_fs, int uv_pitch)
{
    return launch_uv(st, true, bytes, nframes, UvPlane{uv, uv_fs, uv_pitch}, UvPlane{const_cast<uint8_t*>(u), u_fs, u_pitch},
                     UvPlane{const_cast<uint8_t*>(v), v_fs, v_pitch}, cw, h, -1);
}

}  // namespace sn
