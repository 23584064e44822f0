// Image warp by a per-frame homography or camera model (fd_frames_warp: an MI355X extension, the reference
// has no such stage) for gfx950. The arithmetic is the contract of include/fd_hip.h.
//
// k_warp<MODEL, MASK>: a workgroup is 4 waves, one destination row each, and a lane owns the 4 bytes of one
// aligned dword of the row of `out`: the row's first byte may sit at any address, so the lane's pixels are
// x0 .. x0 + 3 with x0 = 4 * (lane's dword) - (row address & 3). A dword that lies inside the row is one packed
// store; the (at most two) dwords that straddle the row's ends are byte stores of the pixels inside. The mask
// has its own base, so its dwords are packed where its address happens to be aligned too, bytes otherwise.
// The frame's parameters are read through a constant-address-space pointer formed from kernel arguments and
// blockIdx only, so they are scalar loads into SGPRs, once per frame. All floating point up to the source
// position is double (the file is built without contraction; f64 division is the correctly rounded default):
// the row terms (h1 * y, ...; the camera model's b) once per lane, the rest per pixel, which gives the bits of
// the per-pixel sequence. The source bytes are plain global gathers: neighbouring destination pixels read
// neighbouring source lines, and the vector cache and L2 do the reuse. No LDS, no workspace.
#include "fd_bilinear.h"
#include "fd_device.h"
#include "fd_hip.h"
#include "fd_kernels.h"

namespace fdk {
namespace {

constexpr int kWarpPx = 4;     // destination pixels per lane: one dword of out
constexpr int kWarpRows = 4;   // destination rows per workgroup, one wave each
constexpr int kWarpThreads = kWave * kWarpRows;
constexpr int kWarpTile = kWave * kWarpPx;  // bytes of a destination row per workgroup

typedef const __attribute__((address_space(4))) double *cparams_t;

// The destination -> source map of one frame on one destination row y.
template <int MODEL>
struct RowMap;

template <>
struct RowMap<FD_WARP_HOMOGRAPHY> {
    static constexpr int kParams = 9;
    double h0, h3, h6, h2, h5, h8, r0, r1, r2;
    __device__ __forceinline__ RowMap(cparams_t h, double y)
        : h0(h[0]), h3(h[3]), h6(h[6]), h2(h[2]), h5(h[5]), h8(h[8]), r0(h[1] * y), r1(h[4] * y), r2(h[7] * y) {}
    __device__ __forceinline__ void at(double x, double &sx, double &sy) const {
        const double X = (h0 * x + r0) + h2, Y = (h3 * x + r1) + h5, W = (h6 * x + r2) + h8;
        sx = X / W;
        sy = Y / W;
    }
};

template <>
struct RowMap<FD_WARP_CAMERA> {
    static constexpr int kParams = 22;
    double fxn, cxn, r0, r3, r6, r2, r5, r8, t0, t1, t2;  // t: r1 * b, r4 * b, r7 * b
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
    __device__ __forceinline__ RowMap(cparams_t p, double y)
        : fxn(p[0]), cxn(p[2]), r0(p[4]), r3(p[7]), r6(p[10]), r2(p[6]), r5(p[9]), r8(p[12]),
          fx(p[13]), fy(p[14]), cx(p[15]), cy(p[16]), k1(p[17]), k2(p[18]), p1(p[19]), p2(p[20]), k3(p[21]) {
        const double b = (y - p[3]) / p[1];
        t0 = p[5] * b;
        t1 = p[8] * b;
        t2 = p[11] * b;
    }
    __device__ __forceinline__ void at(double x, double &sx, double &sy) const {
        const double a = (x - cxn) / fxn;
        const double X = (r0 * a + t0) + r2, Y = (r3 * a + t1) + r5, W = (r6 * a + t2) + r8;
        const double xn = X / W, yn = Y / W;
        const double q2 = xn * xn + yn * yn, q4 = q2 * q2, q6 = q4 * q2;
        const double rad = ((1.0 + k1 * q2) + k2 * q4) + k3 * q6;
        const double m = 2.0 * (xn * yn);
        const double xd = (xn * rad + p1 * m) + p2 * (q2 + 2.0 * (xn * xn));
        const double yd = (yn * rad + p1 * (q2 + 2.0 * (yn * yn))) + p2 * m;
        sx = fx * xd + cx;
        sy = fy * yd + cy;
    }
};

template <int MODEL, bool MASK>
__global__ __launch_bounds__(kWarpThreads) void k_warp(WarpArgs a) {
    const int rb = static_cast<int>(blockIdx.x) / a.tiles, tile = static_cast<int>(blockIdx.x) - rb * a.tiles;
    const int y = rb * kWarpRows + static_cast<int>(threadIdx.y);
    if (y >= a.out_rows) return;
    const float xmax = static_cast<float>(a.cols - 1), ymax = static_cast<float>(a.rows - 1);
    const int64_t frame = static_cast<int64_t>(a.rows) * a.cols;
    const uint32_t fill = static_cast<uint32_t>(a.fill);
    for (int b = blockIdx.y; b < a.batch; b += gridDim.y) {
        const int64_t row = (static_cast<int64_t>(b) * a.out_rows + y) * a.out_cols;  // the row's first byte in out and mask
        const int shift = static_cast<int>((reinterpret_cast<uintptr_t>(a.out) + static_cast<uint64_t>(row)) & 3u);
        const int x0 = (tile * kWave + static_cast<int>(threadIdx.x)) * kWarpPx - shift;  // >= -3
        if (x0 >= a.out_cols) continue;
        const cparams_t params =
            (cparams_t)(a.params + (a.shared ? int64_t(0) : static_cast<int64_t>(b) * RowMap<MODEL>::kParams));
        const RowMap<MODEL> map(params, static_cast<double>(y));
        const uint8_t *img = a.frames + static_cast<int64_t>(b) * frame;
        uint32_t px4 = 0, mk4 = 0;
#pragma unroll
        for (int j = 0; j < kWarpPx; ++j) {
            double sx, sy;
            map.at(static_cast<double>(x0 + j), sx, sy);
            const float px = static_cast<float>(sx), py = static_cast<float>(sy);
            uint32_t v = fill;
            // (false on NaN; a pixel left of the row's start, x0 + j < 0, is computed like any other and not stored)
            if (px >= 0.0f && px <= xmax && py >= 0.0f && py <= ymax) {
                int ix, iy;
                Weights w;
                split_pos(px, py, ix, iy, w);
                ix = min(ix, a.cols - 1);  // (only where (float)(cols - 1) rounds up, past 2^24 columns)
                iy = min(iy, a.rows - 1);
                const int ix1 = min(ix + 1, a.cols - 1), iy1 = min(iy + 1, a.rows - 1);
                const uint8_t *r0 = img + static_cast<int64_t>(iy) * a.cols, *r1 = img + static_cast<int64_t>(iy1) * a.cols;
                const int S = w.w00 * r0[ix] + w.w10 * r0[ix1] + w.w01 * r1[ix] + w.w11 * r1[ix1];
                v = static_cast<uint32_t>((S + (1 << 19)) >> 20);
                mk4 |= 1u << (8 * j);
            }
            px4 |= v << (8 * j);
        }
        uint8_t *o = a.out + row + x0;
        const bool whole = x0 >= 0 && x0 + kWarpPx <= a.out_cols;
        if (whole) {
            *reinterpret_cast<uint32_t *>(o) = px4;  // aligned by the choice of x0
        } else {
#pragma unroll
            for (int j = 0; j < kWarpPx; ++j)
                if (x0 + j >= 0 && x0 + j < a.out_cols) o[j] = static_cast<uint8_t>(px4 >> (8 * j));
        }
        if (MASK) {
            uint8_t *m = a.mask + row + x0;
            if (whole && (reinterpret_cast<uintptr_t>(m) & 3u) == 0) {
                *reinterpret_cast<uint32_t *>(m) = mk4;
            } else {
#pragma unroll
                for (int j = 0; j < kWarpPx; ++j)
                    if (x0 + j >= 0 && x0 + j < a.out_cols) m[j] = static_cast<uint8_t>(mk4 >> (8 * j));
            }
        }
    }
}

template <int MODEL>
void launch_model(const WarpArgs &a, dim3 grid, hipStream_t s) {
    const dim3 block(kWave, kWarpRows);
    if (a.mask)
        hipLaunchKernelGGL((k_warp<MODEL, true>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((k_warp<MODEL, false>), grid, block, 0, s, a);
}

}  // namespace

hipError_t launch_warp(WarpArgs a, hipStream_t s) {
    if (a.out_rows == 0 || a.out_cols == 0) return hipSuccess;
    // a row's dwords start up to 3 bytes before its first pixel
    a.tiles = static_cast<int>((static_cast<int64_t>(a.out_cols) + 3 + kWarpTile - 1) / kWarpTile);
    const int64_t blocks = static_cast<int64_t>(a.tiles) * ((static_cast<int64_t>(a.out_rows) + kWarpRows - 1) / kWarpRows);
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(min(a.batch, 65535)));
    if (a.model == FD_WARP_HOMOGRAPHY)
        launch_model<FD_WARP_HOMOGRAPHY>(a, grid, s);
    else
        launch_model<FD_WARP_CAMERA>(a, grid, s);
    return hipGetLastError();
}

}  // namespace fdk
