// Line band descriptor (fd_lines_describe: an MI355X extension, the reference's line path stops at the
// rectangles) for gfx950. The arithmetic is the contract of include/fd_hip.h.
//
// k_line_desc: one workgroup of 4 waves per line slot. Thread 0 does the line's set-up in double once and leaves
// it in LDS. Rows j of the support region are dealt to the waves (j = wave, wave + 4, ...); within a row, lanes
// run along the line (sample i = lane, lane + 64, ...), so neighbouring lanes read neighbouring pixels and a
// wave's four byte gathers fall in a few cache lines. A lane's part of a row's four sums fits 32 bits (at most
// 64 samples of less than 2^23), the wave total is taken exactly as two 16-bit limbs through the DPP ladder of
// fd_device.h, and the row's sums are kept in LDS as 64-bit integers: no floating-point sum depends on the
// launch shape. S needs no fifth sum: it is the sum of v0 - v1 over the rows.
//
// Epilogue: lane (k, m) of the first 4 * bands threads forms band k's mean and standard deviation of component
// m, serially over the band's rows in the contract's order. The two group norms are serial sums in index order,
// one lane each (threads 0 and 64, so that they sit in different waves); the final norm is thread 0's; the
// scaled values leave one per thread. Every branch that encloses a DPP step or a barrier is uniform over the
// wave or the workgroup.
#include "fd_device.h"
#include "fd_hip.h"
#include "fd_kernels.h"

namespace fdk {
namespace {

constexpr int kLdThreads = 256;
constexpr int kLdWaves = kLdThreads / kWave;
constexpr int kLdMaxRows = 32 * 16;   // bands * band_width at the option limits
constexpr int kLdMaxDim = 8 * 32;
constexpr int kLdMaxSamples = 4096;

struct LineSetup {
    double cx, cy, dlx, dly;
    int dqx, dqy, n, valid;
};

// Exact sum over the wave of one value per lane, each below 2^31, in every lane.
__device__ __forceinline__ uint64_t wave_sum_u31(uint32_t v) {
    const uint32_t lo = wave_total_add(v & 0xFFFFu);  // <= 64 * 65535
    const uint32_t hi = wave_total_add(v >> 16);      // <= 64 * 32767
    return (static_cast<uint64_t>(hi) << 16) + lo;
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }

__global__ __launch_bounds__(kLdThreads) void k_line_desc(LineDescArgs a) {
    __shared__ uint64_t sums[kLdMaxRows][4];
    __shared__ double vals[kLdMaxDim];
    __shared__ LineSetup setup;
    __shared__ int64_t wave_s[kLdWaves];
    __shared__ double group_q[2], final_q;
    const int tid = threadIdx.x, lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int f = static_cast<int>(blockIdx.x / static_cast<unsigned>(a.stride));
    const int slot = static_cast<int>(blockIdx.x - static_cast<unsigned>(f) * static_cast<unsigned>(a.stride));
    const int count = a.counts ? min(static_cast<int>(static_cast<uint32_t>(a.counts[f]) & kCountMask), a.stride) : a.stride;
    if (slot >= count) return;  // (the whole workgroup)
    const int64_t lin = static_cast<int64_t>(blockIdx.x);
    const int w = a.band_width, H = a.bands * w, dim = 8 * a.bands;
    float *desc = a.out_desc + lin * dim;

    if (tid == 0) {
        const float *p = a.lines + lin * a.line_floats;
        const float fsx = p[0], fsy = p[1], fex = p[2], fey = p[3];
        const bool fin = finite_f(fsx) && finite_f(fsy) && finite_f(fex) && finite_f(fey);
        const double sx = fsx, sy = fsy, ex = fex, ey = fey;
        const double dx = ex - sx, dy = ey - sy;
        const double L = sqrt(dx * dx + dy * dy);
        LineSetup s{};
        s.cx = (sx + ex) * 0.5;
        s.cy = (sy + ey) * 0.5;
        s.valid = fin && L >= 1.0;
        if (s.valid) {
            s.dlx = dx / L;
            s.dly = dy / L;
            s.dqx = static_cast<int>(rint(s.dlx * 16384.0));
            s.dqy = static_cast<int>(rint(s.dly * 16384.0));
            s.n = static_cast<int>(fmin(floor(L), static_cast<double>(kLdMaxSamples)));
        }
        setup = s;
        if (a.out_xy) {
            a.out_xy[2 * lin] = fin ? static_cast<float>(s.cx) : 0.0f;
            a.out_xy[2 * lin + 1] = fin ? static_cast<float>(s.cy) : 0.0f;
        }
    }
    __syncthreads();
    if (!setup.valid) {  // (the whole workgroup)
        for (int i = tid; i < dim; i += kLdThreads) desc[i] = 0.0f;
        if (tid == 0 && a.out_valid) a.out_valid[lin] = 0;
        return;
    }
    const double cx = setup.cx, cy = setup.cy, dlx = setup.dlx, dly = setup.dly;
    const double nx = -dly, ny = dlx;
    const int dqx = setup.dqx, dqy = setup.dqy, nqx = -dqy, nqy = dqx, N = setup.n;
    const uint8_t *img = a.frames + static_cast<int64_t>(f) * a.rows * a.cols;
    const double xmax = static_cast<double>(a.cols - 2), ymax = static_cast<double>(a.rows - 2);
    const double a0 = static_cast<double>(N - 1) * 0.5, b0 = static_cast<double>(H - 1) * 0.5;

    int64_t s_rows = 0;  // this wave's rows' part of S (wave-uniform)
    for (int j = wave; j < H; j += kLdWaves) {
        const double b = static_cast<double>(j) - b0;
        const double bx = b * nx, by = b * ny;
        uint32_t p0 = 0, p1 = 0, p2 = 0, p3 = 0;  // < 64 * 2^23
        for (int i = lane; i < N; i += kWave) {
            const double al = static_cast<double>(i) - a0;
            const double x = cx + (al * dlx + bx), y = cy + (al * dly + by);
            const double fx = floor(x + 0.5), fy = floor(y + 0.5);
            if (fx >= 1.0 && fx <= xmax && fy >= 1.0 && fy <= ymax) {
                const uint8_t *c = img + static_cast<int64_t>(static_cast<int>(fy)) * a.cols + static_cast<int>(fx);
                const int gx = static_cast<int>(c[1]) - static_cast<int>(c[-1]);
                const int gy = static_cast<int>(c[a.cols]) - static_cast<int>(c[-a.cols]);
                const int gp = gx * nqx + gy * nqy, gl = gx * dqx + gy * dqy;
                p0 += static_cast<uint32_t>(max(gp, 0));
                p1 += static_cast<uint32_t>(max(-gp, 0));
                p2 += static_cast<uint32_t>(max(gl, 0));
                p3 += static_cast<uint32_t>(max(-gl, 0));
            }
        }
        const uint64_t t0 = wave_sum_u31(p0), t1 = wave_sum_u31(p1), t2 = wave_sum_u31(p2), t3 = wave_sum_u31(p3);
        s_rows += static_cast<int64_t>(t0) - static_cast<int64_t>(t1);
        if (lane == 0) {
            sums[j][0] = t0;
            sums[j][1] = t1;
            sums[j][2] = t2;
            sums[j][3] = t3;
        }
    }
    if (lane == 0) wave_s[wave] = s_rows;
    __syncthreads();

    const bool flip = wave_s[0] + wave_s[1] + wave_s[2] + wave_s[3] < 0;
    if (tid < 4 * a.bands) {
        const int k = tid >> 2, m = tid & 3, mr = flip ? m ^ 1 : m;
        const int jb = (k - 1) * w;
        int n_rows = 0;
        double sum = 0.0;
        for (int t = 0; t < 3 * w; ++t) {
            const int j = jb + t;
            if (j < 0 || j >= H) continue;
            const int64_t g = H - abs(2 * j - (H - 1)), l = 3 * w - abs(2 * t - (3 * w - 1));
            sum += static_cast<double>(g * l * static_cast<int64_t>(sums[flip ? H - 1 - j : j][mr]));
            ++n_rows;
        }
        const double rows_d = static_cast<double>(n_rows);
        const double mean = sum / rows_d;
        double acc = 0.0;
        for (int t = 0; t < 3 * w; ++t) {
            const int j = jb + t;
            if (j < 0 || j >= H) continue;
            const int64_t g = H - abs(2 * j - (H - 1)), l = 3 * w - abs(2 * t - (3 * w - 1));
            const double d = static_cast<double>(g * l * static_cast<int64_t>(sums[flip ? H - 1 - j : j][mr])) - mean;
            acc += d * d;
        }
        vals[8 * k + m] = mean;
        vals[8 * k + 4 + m] = sqrt(acc / rows_d);
    }
    __syncthreads();
    if (tid == 0 || tid == kWave) {  // the means' group, the stds' group
        const int off = tid == 0 ? 0 : 4;
        double s = 0.0;
        for (int k = 0; k < a.bands; ++k)
            for (int m = 0; m < 4; ++m) {
                const double v = vals[8 * k + off + m];
                s += v * v;
            }
        const double q = sqrt(s);
        if (q > 0.0)
            for (int k = 0; k < a.bands; ++k)
                for (int m = 0; m < 4; ++m) vals[8 * k + off + m] = fmin(vals[8 * k + off + m] / q, 0.4);
        group_q[off >> 2] = q;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < dim; ++i) s += vals[i] * vals[i];
        final_q = sqrt(s);
        if (a.out_valid) a.out_valid[lin] = group_q[0] > 0.0 || group_q[1] > 0.0 ? 1 : 0;
    }
    __syncthreads();
    const double q = final_q;
    for (int i = tid; i < dim; i += kLdThreads) desc[i] = q > 0.0 ? static_cast<float>(vals[i] / q) : 0.0f;
}

}  // namespace

hipError_t launch_line_desc(const LineDescArgs &a, hipStream_t s) {
    const int64_t blocks = static_cast<int64_t>(a.batch) * a.stride;
    if (blocks == 0) return hipSuccess;
    if (blocks >= (int64_t(1) << 31) || a.bands < 1 || a.bands * a.band_width > kLdMaxRows || 8 * a.bands > kLdMaxDim ||
        a.band_width < 1 || a.rows < 3 || a.cols < 3)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_line_desc, dim3(static_cast<unsigned>(blocks)), dim3(kLdThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace fdk
