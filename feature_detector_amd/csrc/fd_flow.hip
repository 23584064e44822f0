// Image pyramid and pyramidal Lucas-Kanade feature tracking (fd_pyr_build, fd_flow_lk: an MI355X
// extension, the reference has no tracker) for gfx950. The arithmetic is the contract of include/fd_hip.h.
//
// k_pyr_down: one level from the one below it, (a + b + c + d + 2) >> 2 over 2 x 2 boxes. A bandwidth
// kernel: where a level's width is a multiple of 8 a thread turns two 8-byte loads (8 pixels of two rows)
// into one dword store (every row of such a level is 8-byte aligned: levels start 256-aligned); other
// widths take one output pixel per thread from four byte loads.
//
// k_flow_lk: one wave per feature, kFlowWaves features per workgroup; the waves never meet (no
// __syncthreads: each leaves as soon as its feature is decided). Lane i owns window pixels i, i + 64, ...
// (ROUNDS of them, a template parameter so that the template values Iq, Gx, Gy stay in registers across
// the iterations of a level). Every sampling first stages its u8 patch in the wave's LDS rows (lane & 31 =
// column, lane >> 5 = row parity: no division), (2r + 4)^2 bytes for the template with its gradient
// ring, (2r + 2)^2 for a search sample; the bilinear raw sums are formed from LDS bytes with the four
// wave-uniform integer weights. All window sums are integers: a lane sums its own <= 7 products in
// int32, the wave total is taken exactly as two 16-bit halves through the DPP ladder of fd_device.h
// (wave_total_add), so the order of the reduction cannot matter. The only floating point is the
// wave-uniform 2 x 2 solve in double (every lane computes the same values from the same totals; the file
// is built without contraction, f64 division is the correctly rounded default) and the float update of
// d. Every branch of the level / iteration loops is wave-uniform, so all 64 lanes reach every DPP step.
//
// The backward pass of the forward-backward check is the same kernel with the pyramids swapped, started
// from the forward result with the original position as the guess; it reads the forward status as its
// valid flag (valid_is_status). k_flow_finish applies the round-trip test and counts the tracked slots per
// frame, one global atomic per workgroup.
#include "fd_window.h"

namespace fdk {
namespace {

constexpr int kPyrThreads = 256;

// WIDE: cols (of the source level) is a multiple of 8; a thread makes 4 output pixels.
template <bool WIDE>
__global__ __launch_bounds__(kPyrThreads) void k_pyr_down(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                          int64_t frames_rows_out, int rows, int cols) {
    const int ocols = cols >> 1, orows = rows >> 1;
    const int per_row = WIDE ? cols >> 3 : ocols;
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kPyrThreads + threadIdx.x;
    if (t >= frames_rows_out * per_row) return;
    const int64_t fr = t / per_row;  // frame * orows + output row
    const int xi = static_cast<int>(t - fr * per_row);
    const int64_t f = fr / orows;
    const int oy = static_cast<int>(fr - f * orows);
    const uint8_t *r0 = src + (f * rows + 2 * oy) * cols;
    if constexpr (WIDE) {
        const uint2 a = *reinterpret_cast<const uint2 *>(r0 + 8 * xi);
        const uint2 b = *reinterpret_cast<const uint2 *>(r0 + cols + 8 * xi);
        auto box = [](uint32_t p, uint32_t q, int sh) {
            return (((p >> sh) & 0xFFu) + ((p >> (sh + 8)) & 0xFFu) + ((q >> sh) & 0xFFu) + ((q >> (sh + 8)) & 0xFFu) + 2u) >> 2;
        };
        const uint32_t o = box(a.x, b.x, 0) | (box(a.x, b.x, 16) << 8) | (box(a.y, b.y, 0) << 16) | (box(a.y, b.y, 16) << 24);
        *reinterpret_cast<uint32_t *>(dst + fr * ocols + 4 * xi) = o;
    } else {
        const uint8_t *p = r0 + 2 * xi;
        const uint32_t s = static_cast<uint32_t>(p[0]) + p[1] + p[cols] + p[cols + 1] + 2u;
        dst[fr * ocols + xi] = static_cast<uint8_t>(s >> 2);
    }
}

template <int ROUNDS>
__global__ __launch_bounds__(kFlowThreads) void k_flow_lk(FlowArgs a) {
    __shared__ uint8_t patches[kFlowWaves][kFlowPatch];
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int lane = lane_id();
    const int64_t lin = static_cast<int64_t>(blockIdx.x) * kFlowWaves + wave;
    if (lin >= static_cast<int64_t>(a.batch) * a.stride) return;
    const int f = static_cast<int>(lin / a.stride);
    const int slot_in = static_cast<int>(lin - static_cast<int64_t>(f) * a.stride);
    const int nf = frame_count(a.counts, f, a.stride);
    if (slot_in >= nf) return;
    uint8_t *patch = patches[wave];
    const float x = a.xy[2 * lin], y = a.xy[2 * lin + 1];
    // the slot's result: lost tracks (and invalid slots) hand the input position back
    auto finish = [&](int status, float ox, float oy, float err, bool with_err) {
        if (lane == 0) {
            a.out_xy[2 * lin] = ox;
            a.out_xy[2 * lin + 1] = oy;
            a.out_status[lin] = static_cast<uint8_t>(status);
            if (with_err && a.out_err) a.out_err[lin] = err;
        }
    };
    if (a.valid) {
        const uint8_t v = a.valid[lin];
        if (a.valid_is_status ? v != 1 : v == 0) {
            finish(0, x, y, 0.0f, false);
            return;
        }
    }
    const float xmax = static_cast<float>(a.cols - 1), ymax = static_cast<float>(a.rows - 1);
    if (!(finite_f(x) && finite_f(y) && x >= 0.0f && x <= xmax && y >= 0.0f && y <= ymax)) {
        finish(2, x, y, -1.0f, true);
        return;
    }
    const int r = a.r, W = 2 * r + 1, n = W * W;
    // this lane's window pixels: byte offset of (u + r, v + r) in a patch, -1 beyond the window
    int woff[ROUNDS];
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        const int k = lane + kWave * j;
        const int v = k / W, u = k - v * W;
        woff[j] = k < n ? v * kFlowPitch + u : -1;
    }
    const int top = a.levels - 1;
    float dx = 0.0f, dy = 0.0f;
    if (a.guess) {
        const float s = __uint_as_float(static_cast<uint32_t>(127 - top) << 23);
        dx = (a.guess[2 * lin] - x) * s;
        dy = (a.guess[2 * lin + 1] - y) * s;
    }
    int e_last = 0;
    for (int l = top; l >= 0; --l) {
        const int rows_l = a.rows >> l, cols_l = a.cols >> l;
        const int64_t frame_off = a.off[l] + static_cast<int64_t>(f) * rows_l * cols_l;
        const float down = __uint_as_float(static_cast<uint32_t>(127 - l) << 23);
        const float up = __uint_as_float(static_cast<uint32_t>(127 + l) << 23);
        const float px = x * down, py = y * down;
        int ix, iy;
        Weights w;
        split_pos(px, py, ix, iy, w);
        wave_lds_sync();  // the previous patch has been read
        stage_patch(patch, a.tmpl + frame_off, rows_l, cols_l, ix - r - 1, iy - r - 1, 2 * r + 4, lane);
        wave_lds_sync();
        int iq[ROUNDS], gx[ROUNDS], gy[ROUNDS];
        int s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            const uint8_t *c = patch + max(woff[j], 0) + kFlowPitch + 1;  // (u, v) in the ringed patch
            const int sc = raw_sum(c, w);
            const int gxx = (raw_sum(c + 1, w) - raw_sum(c - 1, w) + (1 << 15)) >> 16;
            const int gyy = (raw_sum(c + kFlowPitch, w) - raw_sum(c - kFlowPitch, w) + (1 << 15)) >> 16;
            const bool on = woff[j] >= 0;
            iq[j] = (sc + (1 << 14)) >> 15;
            gx[j] = on ? gxx : 0;
            gy[j] = on ? gyy : 0;
            s11 += gx[j] * gx[j];
            s12 += gx[j] * gy[j];
            s22 += gy[j] * gy[j];
        }
        const double a11 = static_cast<double>(wave_sum_i32(s11)), a12 = static_cast<double>(wave_sum_i32(s12)),
                     a22 = static_cast<double>(wave_sum_i32(s22));
        const double e11 = a11 - a.tau, e22 = a22 - a.tau;
        const double a12sq = a12 * a12;
        const double det = a11 * a22 - a12sq;
        const bool usable = det > 0.0 && e11 > 0.0 && e22 > 0.0 && e11 * e22 - a12sq >= 0.0;
        if (!usable && l == 0) {
            finish(3, x, y, -1.0f, true);
            return;
        }
        if (usable) {
            for (int it = 0; it < a.max_iters; ++it) {
                const float qx = px + dx, qy = py + dy;
                const float q0x = qx * up, q0y = qy * up;
                if (!(q0x >= 0.0f && q0x <= xmax && q0y >= 0.0f && q0y <= ymax)) {
                    finish(2, x, y, -1.0f, true);
                    return;
                }
                int jx, jy;
                Weights wj;
                split_pos(qx, qy, jx, jy, wj);
                wave_lds_sync();
                stage_patch(patch, a.srch + frame_off, rows_l, cols_l, jx - r, jy - r, 2 * r + 2, lane);
                wave_lds_sync();
                int t1 = 0, t2 = 0, te = 0;
#pragma unroll
                for (int j = 0; j < ROUNDS; ++j) {
                    const int jq = (raw_sum(patch + max(woff[j], 0), wj) + (1 << 14)) >> 15;
                    const int d = woff[j] >= 0 ? iq[j] - jq : 0;
                    t1 += d * gx[j];
                    t2 += d * gy[j];
                    te += abs(d);
                }
                const double b1 = static_cast<double>(wave_sum_i32(t1)), b2 = static_cast<double>(wave_sum_i32(t2));
                e_last = static_cast<int>(wave_total_add(static_cast<uint32_t>(te)));  // <= 441 * 8160
                const double sx = (a22 * b1 - a12 * b2) / det;
                const double sy = (a11 * b2 - a12 * b1) / det;
                const float fx = static_cast<float>(sx), fy = static_cast<float>(sy);
                if (!(finite_f(fx) && finite_f(fy))) {
                    finish(4, x, y, -1.0f, true);
                    return;
                }
                dx = dx + fx;
                dy = dy + fy;
                if (fx * fx + fy * fy <= a.eps2) break;
            }
        }
        if (l > 0) {
            dx = dx * 2.0f;
            dy = dy * 2.0f;
        }
    }
    const float err = static_cast<float>(static_cast<double>(e_last) / (32.0 * n));
    finish(a.max_error >= 0.0f && err > a.max_error ? 6 : 1, x + dx, y + dy, err, true);
}

constexpr int kFinishThreads = 256;

__global__ __launch_bounds__(kFinishThreads) void k_flow_finish(FlowFinishArgs a) {
    __shared__ int total;
    const int tiles = (a.stride + kFinishThreads - 1) / kFinishThreads;
    const int f = static_cast<int>(blockIdx.x) / tiles;
    const int i = (static_cast<int>(blockIdx.x) - f * tiles) * kFinishThreads + static_cast<int>(threadIdx.x);
    const int nf = frame_count(a.counts, f, a.stride);
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    bool ok = false;
    if (i < nf) {
        const int64_t s = static_cast<int64_t>(f) * a.stride + i;
        ok = a.status[s] == 1;
        if (ok && a.back_status) {
            const float bx = a.back_xy[2 * s] - a.xy[2 * s], by = a.back_xy[2 * s + 1] - a.xy[2 * s + 1];
            if (a.back_status[s] != 1 || bx * bx + by * by > a.fb2) {
                ok = false;
                a.status[s] = 5;
            }
        }
    }
    const int n_ok = popc64(ballot(ok));
    if (lane_id() == 0 && n_ok) atomicAdd(&total, n_ok);
    __syncthreads();
    if (threadIdx.x == 0 && a.out_counts && total) atomicAdd(a.out_counts + f, total);
}

template <int ROUNDS>
void launch_rounds(const FlowArgs &a, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL((k_flow_lk<ROUNDS>), dim3(blocks), dim3(kFlowThreads), 0, s, a);
}

}  // namespace

hipError_t launch_pyr_down(const uint8_t *src, uint8_t *dst, int batch, int rows, int cols, hipStream_t s) {
    const int64_t frames_rows_out = static_cast<int64_t>(batch) * (rows >> 1);
    const bool wide = (cols & 7) == 0;
    const int64_t threads = frames_rows_out * (wide ? cols >> 3 : cols >> 1);
    const int64_t blocks = (threads + kPyrThreads - 1) / kPyrThreads;
    if (blocks == 0) return hipSuccess;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    if (wide)
        hipLaunchKernelGGL((k_pyr_down<true>), dim3(static_cast<unsigned>(blocks)), dim3(kPyrThreads), 0, s, src, dst,
                           frames_rows_out, rows, cols);
    else
        hipLaunchKernelGGL((k_pyr_down<false>), dim3(static_cast<unsigned>(blocks)), dim3(kPyrThreads), 0, s, src, dst,
                           frames_rows_out, rows, cols);
    return hipGetLastError();
}

hipError_t launch_flow_lk(const FlowArgs &a, hipStream_t s) {
    const int64_t blocks = (static_cast<int64_t>(a.batch) * a.stride + kFlowWaves - 1) / kFlowWaves;
    if (blocks == 0) return hipSuccess;
    if (blocks >= (int64_t(1) << 31) || a.r < 1 || a.r > 10) return hipErrorInvalidValue;
    const int n = (2 * a.r + 1) * (2 * a.r + 1);
    const unsigned g = static_cast<unsigned>(blocks);
    switch ((n + kWave - 1) / kWave) {
        case 1: launch_rounds<1>(a, g, s); break;
        case 2: launch_rounds<2>(a, g, s); break;
        case 3: launch_rounds<3>(a, g, s); break;
        case 4: launch_rounds<4>(a, g, s); break;
        case 5: launch_rounds<5>(a, g, s); break;
        case 6: launch_rounds<6>(a, g, s); break;
        default: launch_rounds<7>(a, g, s); break;
    }
    return hipGetLastError();
}

hipError_t launch_flow_finish(const FlowFinishArgs &a, hipStream_t s) {
    const int64_t blocks = static_cast<int64_t>(a.batch) * ((a.stride + kFinishThreads - 1) / kFinishThreads);
    if (blocks == 0) return hipSuccess;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_flow_finish, dim3(static_cast<unsigned>(blocks)), dim3(kFinishThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace fdk
