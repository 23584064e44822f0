// Sub-pixel corner refinement (fd_points_refine: an MI355X extension, the reference's detectors stop at
// integer pixels) for gfx950. The arithmetic is the contract of include/fd_hip.h.
//
// k_refine has k_flow_lk's shape and shares its window code (fd_window.h): one wave per feature, kFlowWaves
// features per workgroup; the waves never meet. Lane i owns window pixels i, i + 64, ... (ROUNDS of them, a
// template parameter so that the lane's offsets and weights stay in registers across the iterations). Every
// iteration stages the (2r + 4)^2 u8 patch around floor(c) in the wave's LDS rows and forms Gx, Gy from LDS
// bytes with the four wave-uniform integer weights. The five weighted sums are integers: one product
// w Gx^2 fits int32 (121 * 4080^2 < 2^31), its multiple by an offset does not, so a lane accumulates in
// int64 and the wave total is taken exactly as three limbs (16, 16 and the rest) through the DPP ladder
// of fd_device.h: the order of the reduction cannot matter, and there is no floating-point sum. The only
// floating point is the wave-uniform 2 x 2 solve in double (every lane computes the same values from the
// same totals; the file is built without contraction, f64 division is the correctly rounded default) and
// the float update of c. Every branch of the iteration loop is wave-uniform, so all 64 lanes reach every
// DPP step.
#include "fd_window.h"

namespace fdk {
namespace {

// Exact sum over the wave of one int64 per lane with |v| < 2^47: two 16-bit limbs and the signed rest.
__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
    const uint32_t lo = wave_total_add(static_cast<uint32_t>(v) & 0xFFFFu);           // <= 64 * 65535
    const uint32_t mid = wave_total_add(static_cast<uint32_t>(v >> 16) & 0xFFFFu);    // <= 64 * 65535
    const int32_t hi = static_cast<int32_t>(wave_total_add(static_cast<uint32_t>(v >> 32)));  // |.| <= 64 * 2^15
    return static_cast<int64_t>(hi) * (int64_t(1) << 32) + static_cast<int64_t>(mid) * 65536 + static_cast<int64_t>(lo);
}

template <int ROUNDS>
__global__ __launch_bounds__(kFlowThreads) void k_refine(RefineArgs a) {
    __shared__ uint8_t patches[kFlowWaves][kFlowPatch];
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int lane = lane_id();
    const int64_t lin = static_cast<int64_t>(blockIdx.x) * kFlowWaves + wave;
    if (lin >= static_cast<int64_t>(a.batch) * a.stride) return;
    const int f = static_cast<int>(lin / a.stride);
    const int slot_in = static_cast<int>(lin - static_cast<int64_t>(f) * a.stride);
    if (slot_in >= frame_count(a.counts, f, a.stride)) return;
    uint8_t *patch = patches[wave];
    // read once, before the slot's only write: out_xy may be xy
    const float x = a.xy[2 * lin], y = a.xy[2 * lin + 1];
    // the slot's result: everything but a refined corner hands the input position back
    auto finish = [&](int status, float ox, float oy) {
        if (lane == 0) {
            a.out_xy[2 * lin] = ox;
            a.out_xy[2 * lin + 1] = oy;
            a.out_status[lin] = static_cast<uint8_t>(status);
        }
    };
    if (a.valid && a.valid[lin] == 0) {
        finish(0, x, y);
        return;
    }
    const float xmax = static_cast<float>(a.cols - 1), ymax = static_cast<float>(a.rows - 1);
    if (!(finite_f(x) && finite_f(y) && x >= 0.0f && x <= xmax && y >= 0.0f && y <= ymax)) {
        finish(2, x, y);
        return;
    }
    const int r = a.r, W = 2 * r + 1, n = W * W;
    // this lane's window pixels: byte offset of (u + r, v + r) in a patch, the offsets (u, v) and the weight
    // (r + 1 - |u|)(r + 1 - |v|); beyond the window the weight is 0 and the pixel is the window's first
    int woff[ROUNDS], wu[ROUNDS], wv[ROUNDS], ww[ROUNDS];
#pragma unroll
    for (int j = 0; j < ROUNDS; ++j) {
        const int k = lane + kWave * j;
        const bool on = k < n;
        const int vr = on ? k / W : 0, ur = on ? k - vr * W : 0;
        woff[j] = vr * kFlowPitch + ur;
        wu[j] = ur - r;
        wv[j] = vr - r;
        ww[j] = on ? (r + 1 - abs(ur - r)) * (r + 1 - abs(vr - r)) : 0;
    }
    const uint8_t *img = a.frames + static_cast<int64_t>(f) * a.rows * a.cols;
    float cx = x, cy = y;
    for (int it = 0; it < a.max_iters; ++it) {
        if (!(cx >= 0.0f && cx <= xmax && cy >= 0.0f && cy <= ymax)) {
            finish(2, x, y);
            return;
        }
        int ix, iy;
        Weights w;
        split_pos(cx, cy, ix, iy, w);
        wave_lds_sync();  // the previous patch has been read
        stage_patch(patch, img, a.rows, a.cols, ix - r - 1, iy - r - 1, 2 * r + 4, lane);
        wave_lds_sync();
        int64_t s11 = 0, s12 = 0, s22 = 0, t1 = 0, t2 = 0;
#pragma unroll
        for (int j = 0; j < ROUNDS; ++j) {
            const uint8_t *c = patch + woff[j] + kFlowPitch + 1;  // (u, v) in the ringed patch
            const int gx = (raw_sum(c + 1, w) - raw_sum(c - 1, w) + (1 << 15)) >> 16;
            const int gy = (raw_sum(c + kFlowPitch, w) - raw_sum(c - kFlowPitch, w) + (1 << 15)) >> 16;
            const int p11 = ww[j] * gx * gx, p12 = ww[j] * gx * gy, p22 = ww[j] * gy * gy;  // |.| <= 121 * 4080^2 < 2^31
            s11 += p11;
            s12 += p12;
            s22 += p22;
            t1 += static_cast<int64_t>(p11) * wu[j] + static_cast<int64_t>(p12) * wv[j];
            t2 += static_cast<int64_t>(p12) * wu[j] + static_cast<int64_t>(p22) * wv[j];
        }
        const double g11 = static_cast<double>(wave_sum_i64(s11)), g12 = static_cast<double>(wave_sum_i64(s12)),
                     g22 = static_cast<double>(wave_sum_i64(s22));
        const double b1 = static_cast<double>(wave_sum_i64(t1)), b2 = static_cast<double>(wave_sum_i64(t2));
        const double e11 = g11 - a.tau, e22 = g22 - a.tau;
        const double g12sq = g12 * g12;
        const double det = g11 * g22 - g12sq;
        if (!(det > 0.0 && e11 > 0.0 && e22 > 0.0 && e11 * e22 - g12sq >= 0.0)) {
            finish(3, x, y);
            return;
        }
        const double sx = (g22 * b1 - g12 * b2) / det;
        const double sy = (g11 * b2 - g12 * b1) / det;
        const float fx = static_cast<float>(sx), fy = static_cast<float>(sy);
        cx = cx + fx;
        cy = cy + fy;
        if (!(fabsf(cx - x) <= a.max_shift && fabsf(cy - y) <= a.max_shift)) {  // (false on a non-finite step)
            finish(4, x, y);
            return;
        }
        if (fx * fx + fy * fy <= a.eps2) break;
    }
    finish(1, cx, cy);
}

template <int ROUNDS>
void launch_rounds(const RefineArgs &a, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL((k_refine<ROUNDS>), dim3(blocks), dim3(kFlowThreads), 0, s, a);
}

}  // namespace

hipError_t launch_refine(const RefineArgs &a, hipStream_t s) {
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

}  // namespace fdk
