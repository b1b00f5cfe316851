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
// MSB-aligned surfaces (SN_LAYOUT_*_MSB: P010 / P012, the sample in the HIGH bits of its 16-bit word): the passes see
// LSB-aligned planes, so a side with shift s = 16 - bits_per_sample is converted where its samples move anyway --
//   (x >> ss) << ds   with ss the source's shift and ds the destination's (0 for an LSB side), wave-uniform arguments.
// The MSB instances of k_uv do it inside the split (ss, 0), the merge (0, ds) or a straight conversion (ss, ds), on each
// dword as two packed 16-bit shifts (v_pk_lshrrev_b16 / v_pk_lshlrev_b16); k_shift16 is the same for ONE plane -- luma, the
// planar chroma of a PLANAR_MSB side, a copied plane (ss == ds != 0: the mask) --, shaped as k_uv is, and safe in place
// (src == dst): a lane reads its 16 bytes, or its sample, before it writes them, and no two lanes share a byte.
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

typedef uint16_t U16x2 __attribute__((ext_vector_type(2)));

// (x >> ss) << ds on both 16-bit halves of a dword
__device__ __forceinline__ uint32_t shift_pk(uint32_t x, int ss, int ds)
{
    U16x2 v = __builtin_bit_cast(U16x2, x);
    v = (v >> (uint16_t)ss) << (uint16_t)ds;
    return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ uint4 shift_pk(uint4 a, int ss, int ds)
{
    return make_uint4(shift_pk(a.x, ss, ds), shift_pk(a.y, ss, ds), shift_pk(a.z, ss, ds), shift_pk(a.w, ss, ds));
}
__device__ __forceinline__ uint16_t shift_one(uint16_t x, int ss, int ds) { return (uint16_t)(((uint32_t)x >> ss) << ds); }

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
// kMsb (uint16_t only): every sample read goes through (x >> ss) << ds; the other instances ignore ss and ds.
template <class T, bool kMerge, bool kMsb = false>
__global__ void __launch_bounds__(kUvLanes* kUvRows) k_uv(UvPlane uv, UvPlane pu, UvPlane pv, int cw, int row0, int rstep, int nrows, int nframes,
                                                          int vec_ok, int ss, int ds)
{
    static_assert(!kMsb || sizeof(T) == 2, "MSB-aligned samples are 16-bit words");
    [[maybe_unused]] auto conv4 = [=](uint4 a) { if constexpr (kMsb) return shift_pk(a, ss, ds); else return a; };
    [[maybe_unused]] auto conv1 = [=](T x) { if constexpr (kMsb) return (T)shift_one(x, ss, ds); else return x; };
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
                    const uint4 a = conv4(reinterpret_cast<const uint4*>(puv)[2 * i]), b = conv4(reinterpret_cast<const uint4*>(puv)[2 * i + 1]);
                    uint4 u, v;
                    u.x = __builtin_amdgcn_perm(a.y, a.x, UvSel<B>::even), v.x = __builtin_amdgcn_perm(a.y, a.x, UvSel<B>::odd);
                    u.y = __builtin_amdgcn_perm(a.w, a.z, UvSel<B>::even), v.y = __builtin_amdgcn_perm(a.w, a.z, UvSel<B>::odd);
                    u.z = __builtin_amdgcn_perm(b.y, b.x, UvSel<B>::even), v.z = __builtin_amdgcn_perm(b.y, b.x, UvSel<B>::odd);
                    u.w = __builtin_amdgcn_perm(b.w, b.z, UvSel<B>::even), v.w = __builtin_amdgcn_perm(b.w, b.z, UvSel<B>::odd);
                    reinterpret_cast<uint4*>(pub)[i] = u;
                    reinterpret_cast<uint4*>(pvb)[i] = v;
                } else {
                    const uint4 u = conv4(reinterpret_cast<const uint4*>(pub)[i]), v = conv4(reinterpret_cast<const uint4*>(pvb)[i]);
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
                        reinterpret_cast<T*>(pub)[x] = conv1(reinterpret_cast<const T*>(puv)[2 * x]);
                        reinterpret_cast<T*>(pvb)[x] = conv1(reinterpret_cast<const T*>(puv)[2 * x + 1]);
                    } else {
                        reinterpret_cast<T*>(puv)[2 * x] = conv1(reinterpret_cast<const T*>(pub)[x]);
                        reinterpret_cast<T*>(puv)[2 * x + 1] = conv1(reinterpret_cast<const T*>(pvb)[x]);
                    }
                }
            }
        }
    }
}

// One plane of 16-bit words: dst[y][x] = (src[y][x] >> ss) << ds for x < w, the rows row0 + rstep r.  The shape of k_uv: vectors
// i < nvec of a row are 16 bytes (vec_ok), the lanes behind them take the row's remaining samples; never a byte beyond 2 w.
__global__ void __launch_bounds__(kUvLanes* kUvRows) k_shift16(UvPlane src, UvPlane dst, int w, int row0, int rstep, int nrows, int nframes, int vec_ok,
                                                               int ss, int ds)
{
    constexpr int per = 8;
    const int nvec = vec_ok ? w / per : 0;
    const int i = blockIdx.x * kUvLanes + threadIdx.x;
    const int lanes = gridDim.x * kUvLanes;
    for (int f = blockIdx.z; f < nframes; f += gridDim.z) {
        for (int r = blockIdx.y * kUvRows + threadIdx.y; r < nrows; r += gridDim.y * kUvRows) {
            const int64_t y = row0 + (int64_t)rstep * r;
            const uint8_t* const ps = src.base + (int64_t)f * src.fs + y * src.pitch;
            uint8_t* const pd = dst.base + (int64_t)f * dst.fs + y * dst.pitch;
            if (i < nvec) {
                const uint4 a = reinterpret_cast<const uint4*>(ps)[i];
                reinterpret_cast<uint4*>(pd)[i] = shift_pk(a, ss, ds);
            } else {
                for (int x = nvec * per + (i - nvec); x < w; x += lanes - nvec) {
                    const uint16_t a = reinterpret_cast<const uint16_t*>(ps)[x];
                    reinterpret_cast<uint16_t*>(pd)[x] = shift_one(a, ss, ds);
                }
            }
        }
    }
}

static bool uv_aligned(const UvPlane& p) { return (uintptr_t)p.base % 16 == 0 && p.pitch % 16 == 0 && p.fs % 16 == 0; }

// aligned: a lane per vector and one per sample of the tail (fewer than `per`); otherwise up to 16 waves walk a row's samples
static dim3 uv_grid(int vec_ok, int w, int per, int nrows, int nframes)
{
    const int64_t want = vec_ok ? w / per + w % per : (w < 16 * kUvLanes ? w : 16 * kUvLanes);
    const unsigned gx = (unsigned)((want + kUvLanes - 1) / kUvLanes);
    const int gy = (nrows + kUvRows - 1) / kUvRows;
    return dim3(gx < 1 ? 1 : gx, gy > 65535 ? 65535 : gy, nframes > 65535 ? 65535 : nframes);
}

static hipError_t launch_uv(hipStream_t st, bool merge, int bytes, int nframes, const UvPlane& uv, const UvPlane& pu, const UvPlane& pv, int cw, int h,
                            int line_parity, int ss, int ds)
{
    if (nframes <= 0 || cw <= 0 || h <= 0) return hipSuccess;
    if (bytes != 1 && bytes != 2) return hipErrorInvalidValue;
    const bool msb = ss != 0 || ds != 0;
    if (msb && (bytes != 2 || ss < 0 || ss > 15 || ds < 0 || ds > 15)) return hipErrorInvalidValue;
    const int row0 = line_parity < 0 ? 0 : line_parity & 1, rstep = line_parity < 0 ? 1 : 2;
    const int nrows = (h - row0 + rstep - 1) / rstep;
    if (nrows <= 0) return hipSuccess;
    const int vec_ok = uv_aligned(uv) && uv_aligned(pu) && uv_aligned(pv) ? 1 : 0;
    const dim3 grid = uv_grid(vec_ok, cw, 16 / bytes, nrows, nframes), block(kUvLanes, kUvRows);
    if (bytes == 1) {
        if (merge) hipLaunchKernelGGL((k_uv<uint8_t, true>), grid, block, 0, st, uv, pu, pv, cw, row0, rstep, nrows, nframes, vec_ok, 0, 0);
        else hipLaunchKernelGGL((k_uv<uint8_t, false>), grid, block, 0, st, uv, pu, pv, cw, row0, rstep, nrows, nframes, vec_ok, 0, 0);
    } else if (!msb) {
        if (merge) hipLaunchKernelGGL((k_uv<uint16_t, true>), grid, block, 0, st, uv, pu, pv, cw, row0, rstep, nrows, nframes, vec_ok, 0, 0);
        else hipLaunchKernelGGL((k_uv<uint16_t, false>), grid, block, 0, st, uv, pu, pv, cw, row0, rstep, nrows, nframes, vec_ok, 0, 0);
    } else {
        if (merge) hipLaunchKernelGGL((k_uv<uint16_t, true, true>), grid, block, 0, st, uv, pu, pv, cw, row0, rstep, nrows, nframes, vec_ok, ss, ds);
        else hipLaunchKernelGGL((k_uv<uint16_t, false, true>), grid, block, 0, st, uv, pu, pv, cw, row0, rstep, nrows, nframes, vec_ok, ss, ds);
    }
    return hipGetLastError();
}

static UvPlane uv_plane(const PlaneView& p) { return UvPlane{const_cast<uint8_t*>(p.base), p.fs, p.pitch}; }

hipError_t launch_uv_split(hipStream_t st, int bytes, int nframes, PlaneView uv, int cw, int h, PlaneViewW u, PlaneViewW v, int line_parity, int ss, int ds)
{
    return launch_uv(st, false, bytes, nframes, uv_plane(uv), uv_plane(u), uv_plane(v), cw, h, line_parity, ss, ds);
}

hipError_t launch_uv_merge(hipStream_t st, int bytes, int nframes, PlaneView u, PlaneView v, int cw, int h, PlaneViewW uv, int ss, int ds)
{
    return launch_uv(st, true, bytes, nframes, uv_plane(uv), uv_plane(u), uv_plane(v), cw, h, -1, ss, ds);
}

hipError_t launch_shift16(hipStream_t st, int nframes, PlaneView src, int w, int h, PlaneViewW dst, int line_parity, int ss, int ds)
{
    if (nframes <= 0 || w <= 0 || h <= 0) return hipSuccess;
    if (ss < 0 || ss > 15 || ds < 0 || ds > 15) return hipErrorInvalidValue;
    const int row0 = line_parity < 0 ? 0 : line_parity & 1, rstep = line_parity < 0 ? 1 : 2;
    const int nrows = (h - row0 + rstep - 1) / rstep;
    if (nrows <= 0) return hipSuccess;
    const UvPlane s = uv_plane(src), d = uv_plane(dst);
    const int vec_ok = uv_aligned(s) && uv_aligned(d) ? 1 : 0;
    hipLaunchKernelGGL(k_shift16, uv_grid(vec_ok, w, 8, nrows, nframes), dim3(kUvLanes, kUvRows), 0, st, s, d, w, row0, rstep, nrows, nframes, vec_ok, ss, ds);
    return hipGetLastError();
}

}  // namespace sn
