// RANSAC verification of matches and tracks (fd_ransac, include/fd_hip.h): the fundamental matrix from 8
// correspondences or the homography from 4, a fixed number of hypotheses, all evaluated. Every floating
// point operation is a double one, rounded once (the build passes -ffp-contract=off), in the contract's
// order, so the result is a definite one that tests/ransac_ref.py restates bit for bit.
//
// k_ransac_compact, one workgroup per frame: the ordered list of the frame's correspondences (conditioned
// coordinates, 32 bytes each) by a workgroup prefix over the take flags, and every slot's index in it.
// k_ransac_hyp, one wave per workgroup, a lane per hypothesis: the lane samples, builds its 8 x 9 system
// and eliminates it with complete pivoting. The pivot search indexes rows and columns by data, so the
// system lives in LDS as [element][lane] (36 KiB): the bank of an access depends on the lane alone,
// whatever element each lane picks, and nothing is indexed dynamically in registers. The correspondences
// then pass through an LDS tile that every lane reads at the same address (a broadcast), each lane
// counting its own model's inliers. The wave's best (count, lowest index) goes to the frame's 64-bit slot
// in one atomicMax. k_ransac_finish, one workgroup per frame: classifies every slot with the winner by the
// same device function and writes the outputs.
//
// k_ransac_refit (fd_ransac_refit), one workgroup per frame after k_ransac_compact: every round of the
// least-squares refit on the support set inside one launch. The 9 x 9 normal matrix is summed in the
// contract's order (256 partials in registers, an LDS tree in slices of 9 entries), its smallest eigenvector
// comes from a fixed number of cyclic Jacobi sweeps on one wave with the matrix and V in LDS, F is projected
// to rank 2 by the same routine on F^T F, and every correspondence is classified again.
//
// k_pose_recover (fd_pose_recover), one workgroup per frame: one wave turns the frame's F into the essential
// matrix and its four pose candidates (the same Jacobi on E^T E, the 3 x 3 matrices in LDS), every thread walks
// the slots t, t + 256, ... with four counts in registers, the workgroup picks the winner, and a second walk
// writes the points. k_triangulate (fd_triangulate), one thread per slot, runs the same step for a given pose.
// Neither needs k_ransac_compact: nothing in them depends on a correspondence's number in the list.
//
// The sampler, the elimination, the Jacobi routine and the small products are fd_solve.h's, and the skeleton around
// them (compaction, score and vote, the finish walk, the refit's frame and slice tree) is fd_estimate.h's, both
// shared with fd_pnp.hip: what stands here is the two-view problem's own arithmetic.
#include "fd_estimate.h"

namespace fdk {
namespace {

constexpr int kFundamental = 0;      // FD_RANSAC_FUNDAMENTAL

typedef double d4 __attribute__((ext_vector_type(4)));

// Element (r, c) of a lane's 8 x 9 system: A points at the lane's column of the [element][lane] array.
__device__ __forceinline__ double &el(double *A, int r, int c) { return fdk::el<8, kWave>(A, r, c); }

// The inlier test of a conditioned model h on a conditioned correspondence p = (x, y, u, v): the Sampson
// distance (F) or the forward transfer error (H) against tt = t * t, without a division. A NaN fails.
template <int MODEL>
__device__ __forceinline__ bool inlier(const double (&h)[9], d4 p, double tt) {
    const double x = p.x, y = p.y, u = p.z, v = p.w;
    if (MODEL == kFundamental) {
        const double l0 = h[0] * x + h[1] * y + h[2];
        const double l1 = h[3] * x + h[4] * y + h[5];
        const double l2 = h[6] * x + h[7] * y + h[8];
        const double m0 = h[0] * u + h[3] * v + h[6];
        const double m1 = h[1] * u + h[4] * v + h[7];
        const double e = u * l0 + v * l1 + l2;
        return e * e <= tt * (l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1);
    }
    const double w = h[6] * x + h[7] * y + h[8];
    const double dx = (h[0] * x + h[1] * y + h[2]) - u * w;
    const double dy = (h[3] * x + h[4] * y + h[5]) - v * w;
    return dx * dx + dy * dy <= tt * (w * w);
}

__global__ __launch_bounds__(kRansacThreads) void k_ransac_compact(RansacArgs a) {
    __shared__ uint32_t wsum[kRansacThreads / kWave];
    compact_slots<d4>(a, wsum, [&](int64_t qi, int64_t ti, d4 &p) {
        const float2 q = reinterpret_cast<const float2 *>(a.q_xy)[qi];
        const float2 t = reinterpret_cast<const float2 *>(a.t_xy)[ti];
        p.x = (static_cast<double>(q.x) - a.cx) * a.scale;
        p.y = (static_cast<double>(q.y) - a.cy) * a.scale;
        p.z = (static_cast<double>(t.x) - a.cx) * a.scale;
        p.w = (static_cast<double>(t.y) - a.cy) * a.scale;
        return isfinite(q.x) && isfinite(q.y) && isfinite(t.x) && isfinite(t.y);
    });
}

template <int MODEL>
__global__ __launch_bounds__(kWave) void k_ransac_hyp(RansacArgs a) {
    constexpr int M = MODEL == kFundamental ? 8 : 4;
    __shared__ double mat[72 * kWave];
    __shared__ d4 tile[kTile];
    int f, h;
    hypothesis_index(a.hypotheses, f, h);
    const int n = a.n[f];
    const d4 *corr = reinterpret_cast<const d4 *>(a.corr) + static_cast<int64_t>(f) * a.q_stride;
    int pick[M];
    bool ok = h < a.hypotheses;
    ok = sample<M>(a.seed, f, h, n, pick) && ok;
    double *A = mat + lane_id();
#pragma unroll
    for (int k = 0; k < M; ++k) {
        d4 p = {0.0, 0.0, 0.0, 0.0};
        if (ok) p = corr[pick[k]];  // pick < n <= q_stride
        const double x = p.x, y = p.y, u = p.z, v = p.w;
        if (MODEL == kFundamental) {
            el(A, k, 0) = u * x;
            el(A, k, 1) = u * y;
            el(A, k, 2) = u;
            el(A, k, 3) = v * x;
            el(A, k, 4) = v * y;
            el(A, k, 5) = v;
            el(A, k, 6) = x;
            el(A, k, 7) = y;
            el(A, k, 8) = 1.0;
        } else {
            el(A, 2 * k, 0) = x;
            el(A, 2 * k, 1) = y;
            el(A, 2 * k, 2) = 1.0;
            el(A, 2 * k, 3) = 0.0;
            el(A, 2 * k, 4) = 0.0;
            el(A, 2 * k, 5) = 0.0;
            el(A, 2 * k, 6) = -(u * x);
            el(A, 2 * k, 7) = -(u * y);
            el(A, 2 * k, 8) = -u;
            el(A, 2 * k + 1, 0) = 0.0;
            el(A, 2 * k + 1, 1) = 0.0;
            el(A, 2 * k + 1, 2) = 0.0;
            el(A, 2 * k + 1, 3) = x;
            el(A, 2 * k + 1, 4) = y;
            el(A, 2 * k + 1, 5) = 1.0;
            el(A, 2 * k + 1, 6) = -(v * x);
            el(A, 2 * k + 1, 7) = -(v * y);
            el(A, 2 * k + 1, 8) = -v;
        }
    }
    double x[9];
    ok = null_vector<8, kWave>(A, x) && ok;

    const int count = count_inliers(corr, n, tile, [&](const d4 &p) { return inlier<MODEL>(x, p, a.tt); });
    if (ok) {
        double *dst = model_at<9>(a.models, f, a.hypotheses, h);
#pragma unroll
        for (int c = 0; c < 9; ++c) dst[c] = x[c];
    }
    vote_best(ok, count, h, a.best + f);
}

// The pixel-coordinate model of the conditioned one x, divided by its entry of largest magnitude, into om[9]
// (the "Outputs" paragraph of fd_ransac; fd_ransac_refit writes its accepted model the same way).
template <int MODEL>
__device__ __forceinline__ void write_model(const double (&x)[9], double cx, double cy, double s, double *om) {
    const double T[9] = {s, 0.0, -(s * cx), 0.0, s, -(s * cy), 0.0, 0.0, 1.0};
    double L[9], mt[9], p[9];
    if (MODEL == kFundamental) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) L[3 * i + j] = T[3 * j + i];
    } else {
        const double inv = 1.0 / s;
        const double Ti[9] = {inv, 0.0, cx, 0.0, inv, cy, 0.0, 0.0, 1.0};
#pragma unroll
        for (int c = 0; c < 9; ++c) L[c] = Ti[c];
    }
    matmul3(x, T, mt);
    matmul3(L, mt, p);
    double best = -1.0, pv = p[0];
#pragma unroll
    for (int c = 0; c < 9; ++c)
        if (fabs(p[c]) > best) {
            best = fabs(p[c]);
            pv = p[c];
        }
#pragma unroll
    for (int c = 0; c < 9; ++c) om[c] = p[c] / pv;
}

template <int MODEL>
__global__ __launch_bounds__(kRansacThreads) void k_ransac_finish(RansacArgs a) {
    __shared__ int total;
    const int f = static_cast<int>(blockIdx.x);
    const int nf = frame_count(a.q_counts, f, a.q_stride);
    int h;
    double x[9];
    const bool has = winner(a, f, h, x);
    const int count = classify_slots<d4>(a, f, nf, has, &total, [&](const d4 &p) { return inlier<MODEL>(x, p, a.tt); });
    if (threadIdx.x != 0) return;
    if (a.out_counts) a.out_counts[f] = count;
    if (a.out_best) a.out_best[f] = h;
    double *om = a.out_model + static_cast<int64_t>(f) * 9;
    if (!has) {
#pragma unroll
        for (int c = 0; c < 9; ++c) om[c] = 0.0;
        return;
    }
    write_model<MODEL>(x, a.cx, a.cy, a.scale, om);
}

// ---- fd_ransac_refit: the least-squares refit of a model on its inliers ------------------------------------
constexpr int kSweeps = FD_REFIT_SWEEPS;
constexpr int kNormal = 45;  // entries (a, b), a <= b, of the 9 x 9 normal matrix, row-major (all at once through the tree: 90 KiB)

// acc += row^T row, the 45 entries in order, each one product and one sum.
__device__ __forceinline__ void add_row(double (&acc)[kNormal], const double (&r)[9]) {
    int e = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = i; j < 9; ++j, ++e) acc[e] = acc[e] + r[i] * r[j];
}

// One workgroup per frame, all rounds, in fd_estimate.h's refit frame: a thread's list positions i = t (mod 256)
// are also the contract's partial t of the normal matrix, so its 45 sums stay in registers over the frame.
template <int MODEL>
__global__ __launch_bounds__(kRansacThreads) void k_ransac_refit(RefitArgs g) {
    constexpr int M = MODEL == kFundamental ? 8 : 4;
    __shared__ double red[kSlice * kRansacThreads];
    __shared__ double mat[18 * 9];
    __shared__ double mat3[6 * 3];
    __shared__ double accepted[9];
    __shared__ int total;
    const RansacArgs &a = g.r;
    const int f = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x), lane = lane_id();
    const int nf = frame_count(a.q_counts, f, a.q_stride);
    const int64_t s0 = static_cast<int64_t>(f) * a.q_stride;
    const int n = a.n[f];
    const d4 *corr = reinterpret_cast<const d4 *>(a.corr) + s0;
    Support sup{g.member + 2 * s0, a.q_stride, 0};
    load_members(a, f, nf, g.in_inlier, sup.mem);
    uint32_t mine = 0;
    for (int i = tid; i < n; i += kRansacThreads) mine += sup.mem[i];
    sup.count = wg_count(mine, &total);

    for (int round = 0; round < g.rounds && sup.count >= M; ++round) {  // every exit is uniform over the workgroup
        const uint8_t *S = sup.current();
        double acc[kNormal];
#pragma unroll
        for (int e = 0; e < kNormal; ++e) acc[e] = 0.0;
        for (int i = tid; i < n; i += kRansacThreads) {
            if (!S[i]) continue;
            const d4 p = corr[i];
            const double x = p.x, y = p.y, u = p.z, v = p.w;
            if (MODEL == kFundamental) {
                const double r0[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
                add_row(acc, r0);
            } else {
                const double r0[9] = {x, y, 1.0, 0.0, 0.0, 0.0, -(u * x), -(u * y), -u};
                const double r1[9] = {0.0, 0.0, 0.0, x, y, 1.0, -(v * x), -(v * y), -v};
                add_row(acc, r0);
                add_row(acc, r1);
            }
        }
        reduce_upper<kNormal, 9, true>(acc, red, mat);
        if (tid < 81) mat[81 + tid] = tid / 9 == tid % 9 ? 1.0 : 0.0;
        __syncthreads();
        if (tid < kWave) jacobi<9, kSweeps>(mat, lane);
        __syncthreads();
        double d[9], x[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) d[k] = mat[k * 9 + k];
        const int at = smallest<9>(d);
        double d2 = __builtin_inf(), dmax = d[0];
        bool valid = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (k != at && d[k] < d2) d2 = d[k];
            if (d[k] > dmax) dmax = d[k];
            x[k] = mat[(9 + k) * 9 + at];
            valid = valid && isfinite(x[k]);
        }
        valid = valid && d2 > 1e-12 * dmax;
        if (MODEL == kFundamental) {
            if (tid == 0) gram3_identity<3>(x, mat3);
            __syncthreads();
            if (tid < kWave) jacobi<3, kSweeps>(mat3, lane);
            __syncthreads();
            double d3[3], v[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) d3[k] = mat3[3 * k + k];
            const int at3 = smallest<3>(d3);
#pragma unroll
            for (int k = 0; k < 3; ++k) v[k] = mat3[(3 + k) * 3 + at3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                double w = 0.0;
#pragma unroll
                for (int j = 0; j < 3; ++j) w = w + x[3 * i + j] * v[j];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    x[3 * i + j] = x[3 * i + j] - w * v[j];
                    valid = valid && isfinite(x[3 * i + j]);
                }
            }
        }
        if (!valid) break;
        const int c = reclassify(corr, n, sup.candidate(), &total, [&](const d4 &p) { return inlier<MODEL>(x, p, a.tt); });
        if (!sup.accept(c)) break;
        if (tid == 0) {  // the accepted model: thread 0 writes it out at the end
#pragma unroll
            for (int k = 0; k < 9; ++k) accepted[k] = x[k];
        }
    }

    write_members(a, f, nf, sup.current());
    if (tid != 0) return;
    const int count = sup.count, done = sup.done;
    // What only this epilogue needs is read from the kernel argument segment here (the argument block is the
    // kernel's one parameter): named through `g`, the loads sit at the kernel's entry and their scalar
    // registers stay occupied over the rounds, two of them spilled.
    typedef const __attribute__((address_space(4))) RefitArgs *late_args;
    const late_args e = (late_args)__builtin_amdgcn_kernarg_segment_ptr();
    int32_t *const out_counts = e->r.out_counts, *const out_rounds = e->out_rounds;
    if (out_counts) out_counts[f] = count;
    if (out_rounds) out_rounds[f] = done;
    double *om = e->r.out_model + static_cast<int64_t>(f) * 9;
    if (done == 0) {  // in_model's bits as they are
        copy_bits<9>(e->in_model + static_cast<int64_t>(f) * 9, om);
        return;
    }
    double xa[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) xa[k] = accepted[k];
    write_model<MODEL>(xa, e->r.cx, e->r.cy, e->r.scale, om);
}

// ---- fd_pose_recover, fd_triangulate: the pose of a fundamental matrix and the inliers' 3-D points ----------
constexpr int kPoseSweeps = FD_POSE_SWEEPS;

// Whether slot i of frame f (slots from s0) takes part, by fd_ransac's rules and the in_inlier byte, and its
// normalised rays (ax, ay), (bx, by).
__device__ __forceinline__ bool pose_rays(const PoseArgs &a, int f, int64_t s0, int i, double &ax, double &ay, double &bx,
                                          double &by) {
    bool take = !a.pair_valid || a.pair_valid[s0 + i] == 1;
    take = take && (!a.in_inlier || a.in_inlier[s0 + i] == 1);
    const int j = a.match_idx ? a.match_idx[s0 + i] : i;
    take = take && j >= 0 && j < a.t_stride;
    ax = ay = bx = by = 0.0;
    if (!take) return false;
    const float2 q = reinterpret_cast<const float2 *>(a.q_xy)[s0 + i];
    const float2 t = reinterpret_cast<const float2 *>(a.t_xy)[static_cast<int64_t>(f) * a.t_stride + j];
    ax = (static_cast<double>(q.x) - a.cam[2]) / a.cam[0];
    ay = (static_cast<double>(q.y) - a.cam[3]) / a.cam[1];
    bx = (static_cast<double>(t.x) - a.cam[6]) / a.cam[4];
    by = (static_cast<double>(t.y) - a.cam[7]) / a.cam[5];
    return isfinite(q.x) && isfinite(q.y) && isfinite(t.x) && isfinite(t.y);
}

// The contract's step for the pose (R, t): whether the point is in front, and its depth z1 along (ax, ay, 1).
__device__ __forceinline__ bool pose_step(const double (&R)[9], const double (&t)[3], double ax, double ay, double bx, double by,
                                          double mm, double D, double &z1) {
    const double r0 = R[0] * ax + R[1] * ay + R[2];
    const double r1 = R[3] * ax + R[4] * ay + R[5];
    const double r2 = R[6] * ax + R[7] * ay + R[8];
    const double rr = dot3(r0, r1, r2, r0, r1, r2), pp = dot3(bx, by, 1.0, bx, by, 1.0), rp = dot3(r0, r1, r2, bx, by, 1.0);
    const double rt = dot3(r0, r1, r2, t[0], t[1], t[2]), pt = dot3(bx, by, 1.0, t[0], t[1], t[2]);
    const double det = rr * pp - rp * rp;
    z1 = (rp * pt - pp * rt) / det;
    const double z2 = (rr * pt - rp * rt) / det;
    return det > mm * (rr * pp) && z1 > 0.0 && z2 > 0.0 && z1 <= D && z2 <= D;
}

// A slot's outputs: the byte, and the point (z1 ax, z1 ay, z1) or zeros.
__device__ __forceinline__ void write_point(const PoseArgs &a, int64_t slot, bool in, double ax, double ay, double z1) {
    if (a.out_valid) a.out_valid[slot] = in ? 1 : 0;
    if (a.out_points) {
        a.out_points[3 * slot] = in ? static_cast<float>(z1 * ax) : 0.0f;
        a.out_points[3 * slot + 1] = in ? static_cast<float>(z1 * ay) : 0.0f;
        a.out_points[3 * slot + 2] = in ? static_cast<float>(z1) : 0.0f;
    }
}

__global__ __launch_bounds__(kRansacThreads) void k_triangulate(PoseArgs a, int chunks) {
    const int f = static_cast<int>(blockIdx.x) / chunks;
    const int i = (static_cast<int>(blockIdx.x) - f * chunks) * kRansacThreads + static_cast<int>(threadIdx.x);
    const int nf = frame_count(a.q_counts, f, a.q_stride);
    const int64_t s0 = static_cast<int64_t>(f) * a.q_stride;
    double R[9], t[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) R[c] = a.in_model[static_cast<int64_t>(f) * 12 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = a.in_model[static_cast<int64_t>(f) * 12 + 9 + c];
    bool in = false;
    if (i < nf) {  // nf <= q_stride
        double ax, ay, bx, by, z1 = 0.0;
        in = pose_rays(a, f, s0, i, ax, ay, bx, by);
        in = pose_step(R, t, ax, ay, bx, by, a.mm, a.D, z1) && in;
        write_point(a, s0 + i, in, ax, ay, z1);
    }
    const uint32_t wave_n = wave_total_add(in ? 1u : 0u);
    if (lane_id() == 0 && wave_n && a.out_counts) atomicAdd(a.out_counts + f, static_cast<int>(wave_n));  // zeroed by the launcher
}

__global__ __launch_bounds__(kRansacThreads) void k_pose_recover(PoseArgs a) {
    __shared__ double mat3[6 * 3];  // G, then V
    __shared__ double em[9];        // E
    __shared__ double cand[21];     // Ra, Rb, u3
    __shared__ int has_cand;
    __shared__ int cnt[4];
    const int f = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x), lane = lane_id();
    const int nf = frame_count(a.q_counts, f, a.q_stride);
    const int64_t s0 = static_cast<int64_t>(f) * a.q_stride;

    if (tid < kWave) {  // steps 1-4 on one wave
        if (tid == 0) {
            double F[9], FK[9], E[9];
#pragma unroll
            for (int c = 0; c < 9; ++c) F[c] = a.in_model[static_cast<int64_t>(f) * 9 + c];
            const double Kq[9] = {a.cam[0], 0.0, a.cam[2], 0.0, a.cam[1], a.cam[3], 0.0, 0.0, 1.0};
            const double KtT[9] = {a.cam[4], 0.0, 0.0, 0.0, a.cam[5], 0.0, a.cam[6], a.cam[7], 1.0};
            matmul3(F, Kq, FK);
            matmul3(KtT, FK, E);
#pragma unroll
            for (int c = 0; c < 9; ++c) em[c] = E[c];
            gram3_identity<3>(E, mat3);
        }
        wave_lds_sync();
        jacobi<3, kPoseSweeps>(mat3, lane);
        wave_lds_sync();
        if (tid == 0) {
            double d[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = mat3[3 * k + k];
            const int j = smallest<3>(d);
            const int ia = j == 0 ? 1 : 0, ib = j == 2 ? 1 : 2;
            double dmax = d[0];
#pragma unroll
            for (int k = 1; k < 3; ++k)
                if (d[k] > dmax) dmax = d[k];
            const double da = mat3[3 * ia + ia], db = mat3[3 * ib + ib];
            const double dmin = db < da ? db : da;
            double v1[3], v2[3], w1[3], w2[3], u1[3], u2[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v1[k] = mat3[(3 + k) * 3 + ia];
                v2[k] = mat3[(3 + k) * 3 + ib];
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                w1[i] = dot3(em[3 * i], em[3 * i + 1], em[3 * i + 2], v1[0], v1[1], v1[2]);
                w2[i] = dot3(em[3 * i], em[3 * i + 1], em[3 * i + 2], v2[0], v2[1], v2[2]);
            }
            const double n1 = sqrt(dot3(w1[0], w1[1], w1[2], w1[0], w1[1], w1[2]));
            const double n2 = sqrt(dot3(w2[0], w2[1], w2[2], w2[0], w2[1], w2[2]));
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                u1[i] = w1[i] / n1;
                u2[i] = w2[i] / n2;
            }
            const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
            const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
            bool ok = isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]) && dmin > 1e-12 * dmax;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double ra = (u2[i] * v1[k] - u1[i] * v2[k]) + u3[i] * v3[k];
                    const double rb = (u1[i] * v2[k] - u2[i] * v1[k]) + u3[i] * v3[k];
                    cand[3 * i + k] = ra;
                    cand[9 + 3 * i + k] = rb;
                    ok = ok && isfinite(ra) && isfinite(rb);
                }
                cand[18 + i] = u3[i];
                ok = ok && isfinite(u3[i]) && isfinite(v1[i]) && isfinite(v2[i]);
            }
            has_cand = ok ? 1 : 0;
        }
    }
    if (tid < 4) cnt[tid] = 0;
    __syncthreads();

    const bool has = has_cand != 0;
    double Ra[9], Rb[9], tp[3], tn[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        Ra[c] = cand[c];
        Rb[c] = cand[9 + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        tp[c] = cand[18 + c];
        tn[c] = -tp[c];
    }
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    if (has)
        for (int i = tid; i < nf; i += kRansacThreads) {
            double ax, ay, bx, by, z;
            if (!pose_rays(a, f, s0, i, ax, ay, bx, by)) continue;
            c0 += pose_step(Ra, tp, ax, ay, bx, by, a.mm, a.D, z) ? 1u : 0u;
            c1 += pose_step(Ra, tn, ax, ay, bx, by, a.mm, a.D, z) ? 1u : 0u;
            c2 += pose_step(Rb, tp, ax, ay, bx, by, a.mm, a.D, z) ? 1u : 0u;
            c3 += pose_step(Rb, tn, ax, ay, bx, by, a.mm, a.D, z) ? 1u : 0u;
        }
    const uint32_t w0 = wave_total_add(c0), w1 = wave_total_add(c1), w2 = wave_total_add(c2), w3 = wave_total_add(c3);
    if (lane == 0) {
        if (w0) atomicAdd(&cnt[0], static_cast<int>(w0));
        if (w1) atomicAdd(&cnt[1], static_cast<int>(w1));
        if (w2) atomicAdd(&cnt[2], static_cast<int>(w2));
        if (w3) atomicAdd(&cnt[3], static_cast<int>(w3));
    }
    __syncthreads();
    int best = cnt[0], choice = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (cnt[k] > best) {
            best = cnt[k];
            choice = k;
        }
    const bool pose = has && best > 0;  // uniform over the workgroup
    double R[9], t[3];
#pragma unroll
    for (int c = 0; c < 9; ++c) R[c] = choice < 2 ? Ra[c] : Rb[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = (choice & 1) ? tn[c] : tp[c];
    if (a.out_valid || a.out_points)
        for (int i = tid; i < nf; i += kRansacThreads) {
            double ax = 0.0, ay = 0.0, bx, by, z1 = 0.0;
            bool in = false;
            if (pose) {
                in = pose_rays(a, f, s0, i, ax, ay, bx, by);
                in = pose_step(R, t, ax, ay, bx, by, a.mm, a.D, z1) && in;
            }
            write_point(a, s0 + i, in, ax, ay, z1);
        }
    if (tid != 0) return;
    if (a.out_counts) a.out_counts[f] = pose ? best : 0;
    if (a.out_choice) a.out_choice[f] = pose ? choice : -1;
    if (a.out_pose) {
        double *op = a.out_pose + static_cast<int64_t>(f) * 12;
#pragma unroll
        for (int c = 0; c < 9; ++c) op[c] = pose ? R[c] : 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) op[9 + c] = pose ? t[c] : 0.0;
    }
}

}  // namespace

hipError_t launch_pose_recover(const PoseArgs &a, hipStream_t s) {
    if (a.batch < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pose_recover, dim3(static_cast<unsigned>(a.batch)), dim3(kRansacThreads), 0, s, a);
    return hipGetLastError();
}

// One thread per slot, (chunks, batch) workgroups as one grid dimension (no 65535 limit on the batch).
hipError_t launch_triangulate(const PoseArgs &a, hipStream_t s) {
    const int chunks = (a.q_stride + kRansacThreads - 1) / kRansacThreads;
    const int64_t blocks = static_cast<int64_t>(a.batch) * chunks;
    if (a.batch < 1 || chunks < 1 || blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    if (a.out_counts) {
        const hipError_t e = hipMemsetAsync(a.out_counts, 0, sizeof(int32_t) * a.batch, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_triangulate, dim3(static_cast<unsigned>(blocks)), dim3(kRansacThreads), 0, s, a, chunks);
    return hipGetLastError();
}

hipError_t launch_ransac_refit(const RefitArgs &a, hipStream_t s) {
    if (a.r.batch < 1) return hipErrorInvalidValue;
    const dim3 frames(static_cast<unsigned>(a.r.batch));
    hipLaunchKernelGGL(k_ransac_compact, frames, dim3(kRansacThreads), 0, s, a.r);
    if (a.r.model == kFundamental)
        hipLaunchKernelGGL((k_ransac_refit<0>), frames, dim3(kRansacThreads), 0, s, a);
    else
        hipLaunchKernelGGL((k_ransac_refit<1>), frames, dim3(kRansacThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ransac(const RansacArgs &a, hipStream_t s) {
    const int64_t blocks = static_cast<int64_t>(a.batch) * ((a.hypotheses + kWave - 1) / kWave);
    if (a.batch < 1 || blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    const dim3 frames(static_cast<unsigned>(a.batch)), hyps(static_cast<unsigned>(blocks));
    hipLaunchKernelGGL(k_ransac_compact, frames, dim3(kRansacThreads), 0, s, a);
    if (a.model == kFundamental) {
        hipLaunchKernelGGL((k_ransac_hyp<0>), hyps, dim3(kWave), 0, s, a);
        hipLaunchKernelGGL((k_ransac_finish<0>), frames, dim3(kRansacThreads), 0, s, a);
    } else {
        hipLaunchKernelGGL((k_ransac_hyp<1>), hyps, dim3(kWave), 0, s, a);
        hipLaunchKernelGGL((k_ransac_finish<1>), frames, dim3(kRansacThreads), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace fdk
