// Shared device pieces of the corner kernels (fd_points.hip: k_corner, k_corner_short, k_fast;
// fd_corner_lp.hip: k_corner_lp): workgroup -> tile decoding, frame loads, the prior mask's bits, the exact
// response arithmetic, and the integer kernels' row step -- gradient row sums, stored responses, NMS --
// written once for k_corner's ring walk and k_corner_short's straight-line walk (the candidate lists they
// write: fd_emit.h). Each including translation unit gets its own copy (anonymous namespace).
#pragma once

#include "fd_emit.h"

namespace fdk {
namespace {

constexpr float kInvCnt = 1.0f / 9.0f;                  // 1 / (3*3)  (:71)
constexpr float kInvCnt2 = (1.0f / 9.0f) * (1.0f / 9.0f);  // harris :72
constexpr float kHarrisAlpha = 0.04f;                  // feature_point_harris_detector.h:13

// Workgroup -> (frame, 4 consecutive tiles of that frame); returns false for the idle waves of a
// frame's last workgroup (they still take part in the workgroup barriers).
// The tile coordinates are made visibly wave-uniform (readfirstlane), so row/tile logic stays scalar.
// Logical workgroup id: workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share an L2), so
// the grid is remapped to give each XCD a contiguous range of logical ids -- a band of a frame's tile
// rows, whose halo rows then come from that XCD's own L2 (for speed only: any placement is correct).
// Bijective for any grid size: XCD group x = b % 8 holds q (+1 for x < r) workgroups.
__device__ __forceinline__ int logical_block() {
    const int b = static_cast<int>(blockIdx.x), n = static_cast<int>(gridDim.x);
    const int q = n >> 3, r = n & 7, x = b & 7;
    return x * q + min(x, r) + (b >> 3);
}

__device__ __forceinline__ bool decode_tile(const PointsArgs &a, int &f, int &ty, int &tx) {
    const int lb = logical_block();
    f = lb / a.blocks_per_frame;
    const int t = __builtin_amdgcn_readfirstlane((lb % a.blocks_per_frame) * 4 + (threadIdx.x >> 6));
    tx = t % a.tiles_x;
    ty = t / a.tiles_x;
    return t < a.tiles_x * a.tiles_y;
}

// Dword of frame bytes [off, off+4). `aligned` (cols % 4 == 0) guarantees whole-dword range checks;
// otherwise assemble from byte loads so that a dword straddling the frame end still returns its bytes.
// A compile-time choice: a runtime branch here makes the waitcnt pass drain the prefetch queue.
template <bool ALIGNED>
__device__ __forceinline__ uint32_t load_px4(__amdgpu_buffer_rsrc_t r, int32_t off) {
    if constexpr (ALIGNED) return buf_load_u32(r, off);
    return buf_load_u8(r, off) | (buf_load_u8(r, off + 1) << 8) | (buf_load_u8(r, off + 2) << 16) |
           (buf_load_u8(r, off + 3) << 24);
}
// Two pixels [off, off+2) as the low bytes of a dword (aligned: off is even, cols % 4 == 0 and c0 even).
template <bool ALIGNED>
__device__ __forceinline__ uint32_t load_px2(__amdgpu_buffer_rsrc_t r, int32_t off) {
    if constexpr (ALIGNED) return buf_load_u16(r, off);
    return buf_load_u8(r, off) | (buf_load_u8(r, off + 1) << 8);
}

// Prior-mask bits of the NC columns from c0 (a multiple of NC: they share a word) of one row.
template <int NC>
__device__ __forceinline__ uint32_t mask_bits(const PointsArgs &a, int f, int row, int c0) {
    if (c0 < 0 || c0 >= a.cols) return 0u;
    const uint32_t w = a.mask[(static_cast<int64_t>(f) * a.rows + row) * a.mask_wpr + (c0 >> 5)];
    return (w >> (c0 & 31)) & ((1u << NC) - 1u);
}

// Two pixels' float math at a time: <2 x float> arithmetic compiles to v_pk_mul_f32 / v_pk_add_f32 /
// v_pk_fma_f32, which round each lane exactly like the scalar op (the kernel is VALU-issue bound, and
// a packed op retires two pixels' worth of one reference operation per issue slot).
// sqrt_rn_rsq2 (correctly rounded sqrt on the reciprocal square root) lives in fd_device.h.

// Stored responses of two pixels (responses_ semantics: 0 unless written), from exact integer tensor
// sums. Same operations in the same order as the reference; only the issue is paired.
//
// Integer-to-float without v_cvt: every gradient product carries a bias beta (mod 2^32) chosen so that
// the nine products of a 3x3 sum carry exactly 9*beta == 0x4B000000 (the bit pattern of 2^23), or
// 0x4B400000 (2^23 + 2^22) for the signed cross term. Then for 0 <= S < 2^23 (S <= 9*255^2 here,
// |Sxy| < 2^22) the biased sum read as a float is exactly 2^23 + S, and one exact (packed)
// subtraction recovers float(S). 9 is odd, so beta = target * 9^-1 mod 2^32 exists.
constexpr uint32_t kBiasSq = 0xB3000000u;  // 9 * kBiasSq == 0x4B000000 (mod 2^32)
constexpr uint32_t kBiasXy = 0x41400000u;  // 9 * kBiasXy == 0x4B400000 (mod 2^32)
static_assert(9u * kBiasSq == 0x4B000000u && 9u * kBiasXy == 0x4B400000u, "bias");

// G1 (detect mode with thr >= 0): only the pre-check gates the stored value, so a pixel whose
// response is <= thr keeps its response instead of 0. The NMS that reads these values tests
// x > max(thr, neighbours): with thr >= 0 a kept response <= thr acts exactly like the reference's 0
// there (as a centre it fails x > thr, as a neighbour max(thr, r) == thr == max(thr, 0)), and every
// emitted candidate has x > thr, i.e. the reference's stored value. Saves a compare per pixel.
template <int KIND, bool G1>
__device__ __forceinline__ f2 corner_response2(uint32_t sxx0, uint32_t sxx1, uint32_t syy0, uint32_t syy1,
                                               uint32_t sxy0, uint32_t sxy1, float thr) {
    const f2 bxx = f2{__uint_as_float(sxx0), __uint_as_float(sxx1)};  // 2^23 + Sxx, exactly
    const f2 byy = f2{__uint_as_float(syy0), __uint_as_float(syy1)};
    const f2 fxy = f2{__uint_as_float(sxy0), __uint_as_float(sxy1)} - 12582912.0f;
    f2 res, gate, r;
    if constexpr (KIND == 0) {  // Harris, feature_point_harris_detector.cpp:95-103
        const f2 fxx = bxx - 8388608.0f, fyy = byy - 8388608.0f;
        const f2 trace = fxx + fyy;
        gate = ((trace * trace) * 0.21f) * kInvCnt2;
        r = (((fxx * fyy) - (fxy * fxy)) - ((kHarrisAlpha * trace) * trace)) * kInvCnt2;
    } else {  // Shi-Tomasi, feature_point_shi_tomas_detector.cpp:94-103
        // a = fl(Sxx * k) as one fma on the biased sum: bxx*k - 2^23*k is (bxx - 2^23)*k = Sxx*k
        // exactly before the fma's single rounding (2^23*k is exact: a power-of-two multiple of k).
        const f2 a = __builtin_elementwise_fma(bxx, f2{kInvCnt, kInvCnt}, f2{-8388608.0f * kInvCnt, -8388608.0f * kInvCnt});
        const f2 c = __builtin_elementwise_fma(byy, f2{kInvCnt, kInvCnt}, f2{-8388608.0f * kInvCnt, -8388608.0f * kInvCnt});
        gate = a + c;
        const f2 b = fxy * kInvCnt;
        const f2 d = a - c;
        // (4b)*b = 4*fl(b*b) exactly, so dd + fl(fl(4b)*b) is one fma of b*b with 4
        const f2 common = sqrt_rn_rsq2(__builtin_elementwise_fma(b * b, f2{4.0f, 4.0f}, d * d));
        r = (gate + common) * 0.5f;
    }
    if constexpr (G1) {
        res.x = gate.x > thr ? r.x : 0.0f;
        res.y = gate.y > thr ? r.y : 0.0f;
    } else {
        res.x = (gate.x > thr && r.x > thr) ? r.x : 0.0f;
        res.y = (gate.y > thr && r.y > thr) ? r.y : 0.0f;
    }
    return res;
}

// ---------------------------------------------------------------------------------------------------
// The integer kernels' row step (k_corner, k_corner_short), for a lane of NC columns c0 .. c0+NC-1 in a
// wave whose lanes 0 and 63 only supply halo (tile width 62 NC). Each piece takes its rows as arguments
// and is indifferent to how the caller keeps them (a 3-slot ring, or one slot per row).
// ---------------------------------------------------------------------------------------------------
// Which of the lane's columns count, fixed for the tile.
template <int NC>
struct TileCols {
    int c0;               // the lane's first column: tx * 62 NC + NC (lane - 1)
    bool interior;        // every lane's columns inside [2, cols-3]: only the frame's first/last rows need masking
    bool cval[NC];        // column inside [2, cols-3]
    bool colv[NC];        // ... and owned by an interior lane (emitted)
    uint64_t colv_b[NC];  // ballot of colv
};
template <int NC>
__device__ __forceinline__ TileCols<NC> tile_columns(int tx, int cols) {
    constexpr int TW = 62 * NC;
    const int lane = lane_id();
    const int c0 = tx * TW + NC * (lane - 1);
    TileCols<NC> tc;
    tc.c0 = c0;
    tc.interior = tx * TW - NC >= 2 && tx * TW + NC * 62 + NC - 1 <= cols - 3;
#pragma unroll
    for (int m = 0; m < NC; ++m) {
        tc.cval[m] = c0 + m >= 2 && c0 + m <= cols - 3;
        tc.colv[m] = tc.cval[m] && lane >= 1 && lane <= 62;
        tc.colv_b[m] = ballot(tc.colv[m]);
    }
    return tc;
}

// Biased horizontal 3-tap sums of one row's gradient products (3 products, 3*beta).
template <int NC>
struct HSums {
    uint32_t xx[NC], yy[NC], xy[NC];
};

// Gradients of a centre row at the lane's NC columns (feature_point_harris_detector.cpp:35-62) and their
// horizontal sums. Pc / P_below / P_above: the lane's pixels of the centre row and of the rows below and
// above it; Lc / Rc: the neighbour lanes' pixels of the centre row (its two halo bytes come from them).
// Products carry the float-conversion bias (v_mad_i32_i24 with a constant addend: free).
template <int NC>
__device__ __forceinline__ void grad_row_sums(uint32_t Lc, uint32_t Pc, uint32_t Rc, uint32_t P_below, uint32_t P_above,
                                              HSums<NC> &h) {
    uint32_t qxx[NC + 2], qyy[NC + 2], qxy[NC + 2];  // products at columns c0-1 .. c0+NC (k = m + 1)
    uint32_t bsq = kBiasSq, bxy = kBiasXy;
    asm volatile("" : "+s"(bsq), "+s"(bxy));  // opaque: keeps v_mad (else mul + or)
#pragma unroll
    for (int m = 0; m < NC; ++m) {
        const int ix = win_byte<NC>(Lc, Pc, Rc, m + 1) - win_byte<NC>(Lc, Pc, Rc, m - 1);
        const int iy = win_byte<NC>(0, P_below, 0, m) - win_byte<NC>(0, P_above, 0, m);
        qxx[m + 1] = static_cast<uint32_t>(ix * ix) + bsq;
        qyy[m + 1] = static_cast<uint32_t>(iy * iy) + bsq;
        qxy[m + 1] = static_cast<uint32_t>(ix * iy) + bxy;
    }
    // Halo products from the neighbour lanes' edge columns (exact for lanes 0 / 63's inner columns,
    // whose neighbours are lanes 1 / 62).
    qxx[0] = from_left(qxx[NC]);
    qyy[0] = from_left(qyy[NC]);
    qxy[0] = from_left(qxy[NC]);
    qxx[NC + 1] = from_right(qxx[1]);
    qyy[NC + 1] = from_right(qyy[1]);
    qxy[NC + 1] = from_right(qxy[1]);
#pragma unroll
    for (int m = 0; m < NC; ++m) {
        h.xx[m] = add3u(qxx[m], qxx[m + 1], qxx[m + 2]);
        h.yy[m] = add3u(qyy[m], qyy[m + 1], qyy[m + 2]);
        h.xy[m] = add3u(qxy[m], qxy[m + 1], qxy[m + 2]);
    }
}

// Stored responses of row rr from the horizontal sums of rows rr-1, rr, rr+1 (in any order): the vertical
// 3-row sums are exact integers (< 2^23).
template <int KIND, bool G1, bool MASKED, int NC>
__device__ __forceinline__ void response_row(const PointsArgs &a, int f, int rr, const TileCols<NC> &tc,
                                             const HSums<NC> &h0, const HSums<NC> &h1, const HSums<NC> &h2,
                                             float (&rsp)[NC]) {
    const bool rowv = rr >= 2 && rr <= a.rows - 3;
    uint32_t sxx[NC], syy[NC], sxy[NC];
#pragma unroll
    for (int m = 0; m < NC; ++m) {
        sxx[m] = add3u(h0.xx[m], h1.xx[m], h2.xx[m]);
        syy[m] = add3u(h0.yy[m], h1.yy[m], h2.yy[m]);
        sxy[m] = add3u(h0.xy[m], h1.xy[m], h2.xy[m]);
    }
    float r[NC];
#pragma unroll
    for (int m = 0; m < NC; m += 2) {
        const f2 rp = corner_response2<KIND, G1>(sxx[m], sxx[m + 1], syy[m], syy[m + 1], sxy[m], sxy[m + 1], a.thr);
        r[m] = rp.x;
        r[m + 1] = rp.y;
    }
    if (!MASKED && rowv && tc.interior) {  // wave-uniform: no per-pixel masking needed
#pragma unroll
        for (int m = 0; m < NC; ++m) rsp[m] = r[m];
    } else {
        uint32_t mb = (1u << NC) - 1u;
        if constexpr (MASKED) mb = rowv ? mask_bits<NC>(a, f, rr, tc.c0) : 0u;
        // The halo lanes' inner columns (lane 0's last, lane 63's first) are exact and serve as the NMS
        // neighbours of the tile's edge columns.
#pragma unroll
        for (int m = 0; m < NC; ++m) rsp[m] = (rowv && tc.cval[m] && ((mb >> m) & 1u)) ? r[m] : 0.0f;
    }
}

// NMS of one row (feature_point_harris_detector.cpp:120-137): strict, 4-neighbour. x: the row's stored
// responses, up / dn: those of its two vertical neighbours (in either order).
// x > thr and x > each neighbour  <=>  x > max(thr, neighbours)  (no NaNs; +-0 compare equal): two v_max3.
// b[m] is the wave ballot of fl[m], v[m] the candidate's response (emit_row's arguments).
template <int NC>
__device__ __forceinline__ void nms_row(const float (&x)[NC], const float (&up)[NC], const float (&dn)[NC], float thr,
                                        const TileCols<NC> &tc, uint64_t (&b)[NC], bool (&fl)[NC], float (&v)[NC]) {
    const float lft = from_left_f(x[NC - 1]);
    const float rgt = from_right_f(x[0]);
#pragma unroll
    for (int m = 0; m < NC; ++m) {
        const float xl = m == 0 ? lft : x[m - 1];
        const float xr = m == NC - 1 ? rgt : x[m + 1];
        const float nb = max3f(max3f(xl, xr, thr), up[m], dn[m]);
        const bool hit = x[m] > nb;
        v[m] = x[m];
        fl[m] = tc.colv[m] && hit;
        b[m] = ballot(hit) & tc.colv_b[m];  // the compare's lane mask, no bool round trip
    }
}

}  // namespace
}  // namespace fdk
