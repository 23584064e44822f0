// Absolute camera pose from 3-D - 2-D correspondences (fd_pnp_ransac, fd_pnp_refit of include/fd_hip.h): a fixed
// number of 6-point DLT camera matrices, all evaluated, the winner turned into a pose, and a Gauss-Newton
// refinement of the reprojection error on its inliers. Every floating point operation is a double one, rounded
// once (the build passes -ffp-contract=off), in the contract's order, so the result is a definite one that
// tests/pnp_ref.py restates bit for bit. The sampler, the elimination and the Jacobi routine are fd_ransac's
// (fd_solve.h), and so is the skeleton around them (fd_estimate.h: compaction, score and vote, the finish walk, the
// refit's frame and slice tree): what stands here is the PnP problem's own arithmetic.
//
// k_pnp_compact, one workgroup per frame: the ordered list of the frame's correspondences (conditioned point
// and ray, 40 bytes each) by a workgroup prefix over the take flags, and every slot's index in it.
// k_pnp_hyp, one wave per workgroup, a lane per hypothesis: the lane samples, builds its 11 x 12 system in LDS
// as [element][lane] (66 KiB: two workgroups per CU) and eliminates it with complete pivoting; the
// correspondences then pass through a broadcast tile, each lane counting its own matrix's inliers, and the
// wave's best goes to the frame's 64-bit slot in one atomicMax. k_pnp_finish, one workgroup per frame: one wave
// orthonormalises the winner (the Jacobi on M^T M), then every slot is classified and the outputs written.
//
// k_pnp_refit, one workgroup per frame after k_pnp_compact (centre 0, scale 1): every Gauss-Newton round inside
// one launch. The 27 sums of [J^T J | J^T r] stay in registers per thread (256 partials), an LDS tree combines
// them in slices of 9, thread 0 solves the 6 x 7 system by the same elimination and updates the pose by the
// Cayley transform, and every correspondence is classified again.
#include "fd_estimate.h"

namespace fdk {
namespace {

constexpr int kPnpRows = 11;                         // of the 12 rows of 6 picks
constexpr int kPnpElems = kPnpRows * (kPnpRows + 1);  // 132 doubles per lane
constexpr int kPnpSweeps = FD_POSE_SWEEPS;
constexpr int kGn = 27;  // entries (i, j), i <= j, i < 6, of the 6 x 7 system [J^T J | J^T r], row-major

// A correspondence: the conditioned 3-D point and the normalised ray of its image point.
struct Corr5 {
    double X, Y, Z, bx, by;
};

// The inlier test of a 3 x 4 matrix P on a correspondence: the reprojection error in pixels against tt = t * t,
// without a division; a point behind the camera (w <= 0) and a NaN fail.
__device__ __forceinline__ bool pnp_inlier(const double (&P)[12], const Corr5 &p, double fx, double fy, double tt) {
    const double y0 = P[0] * p.X + P[1] * p.Y + P[2] * p.Z + P[3];
    const double y1 = P[4] * p.X + P[5] * p.Y + P[6] * p.Z + P[7];
    const double w = P[8] * p.X + P[9] * p.Y + P[10] * p.Z + P[11];
    const double dx = fx * (y0 - p.bx * w);
    const double dy = fy * (y1 - p.by * w);
    return w > 0.0 && dx * dx + dy * dy <= tt * (w * w);
}

__global__ __launch_bounds__(kRansacThreads) void k_pnp_compact(PnpArgs a) {
    __shared__ uint32_t wsum[kRansacThreads / kWave];
    compact_slots<Corr5>(a, wsum, [&](int64_t qi, int64_t ti, Corr5 &p) {
        if (a.p_valid && a.p_valid[qi] != 1) return false;
        const float *q = a.p_xyz + 3 * qi;
        const float qx = q[0], qy = q[1], qz = q[2];
        const float2 t = reinterpret_cast<const float2 *>(a.t_xy)[ti];
        p.X = (static_cast<double>(qx) - a.center[0]) * a.scale;
        p.Y = (static_cast<double>(qy) - a.center[1]) * a.scale;
        p.Z = (static_cast<double>(qz) - a.center[2]) * a.scale;
        p.bx = (static_cast<double>(t.x) - a.cam[2]) / a.cam[0];
        p.by = (static_cast<double>(t.y) - a.cam[3]) / a.cam[1];
        return isfinite(qx) && isfinite(qy) && isfinite(qz) && isfinite(t.x) && isfinite(t.y);
    });
}

__global__ __launch_bounds__(kWave) void k_pnp_hyp(PnpArgs a) {
    constexpr int M = 6;
    __shared__ double mat[kPnpElems * kWave];
    __shared__ Corr5 tile[kTile];
    int f, h;
    hypothesis_index(a.hypotheses, f, h);
    const int n = a.n[f];
    const Corr5 *corr = reinterpret_cast<const Corr5 *>(a.corr) + static_cast<int64_t>(f) * a.q_stride;
    int pick[M];
    bool ok = h < a.hypotheses;
    ok = sample<M>(a.seed, f, h, n, pick) && ok;
    double *A = mat + lane_id();
#pragma unroll
    for (int k = 0; k < M; ++k) {
        Corr5 p = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (ok) p = corr[pick[k]];  // pick < n <= q_stride
        const double row[8] = {p.X, p.Y, p.Z, 1.0, -(p.bx * p.X), -(p.bx * p.Y), -(p.bx * p.Z), -p.bx};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            el<kPnpRows, kWave>(A, 2 * k, c) = row[c];
            el<kPnpRows, kWave>(A, 2 * k, 4 + c) = 0.0;
            el<kPnpRows, kWave>(A, 2 * k, 8 + c) = row[4 + c];
        }
        if (2 * k + 1 < kPnpRows) {
            const double tail[4] = {-(p.by * p.X), -(p.by * p.Y), -(p.by * p.Z), -p.by};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                el<kPnpRows, kWave>(A, 2 * k + 1, c) = 0.0;
                el<kPnpRows, kWave>(A, 2 * k + 1, 4 + c) = row[c];
                el<kPnpRows, kWave>(A, 2 * k + 1, 8 + c) = tail[c];
            }
        }
    }
    double x[12];
    ok = null_vector<kPnpRows, kWave>(A, x) && ok;
    // the sign that puts the points of a proper camera in front of it
    const double det = (x[0] * (x[5] * x[10] - x[6] * x[9]) - x[1] * (x[4] * x[10] - x[6] * x[8])) + x[2] * (x[4] * x[9] - x[5] * x[8]);
    ok = ok && det != 0.0 && isfinite(det);
    if (det < 0.0) {
#pragma unroll
        for (int c = 0; c < 12; ++c) x[c] = -x[c];
    }

    const int count =
        count_inliers(corr, n, tile, [&](const Corr5 &p) { return pnp_inlier(x, p, a.cam[0], a.cam[1], a.tt); });
    if (ok) {
        double *dst = model_at<12>(a.models, f, a.hypotheses, h);
#pragma unroll
        for (int c = 0; c < 12; ++c) dst[c] = x[c];
    }
    vote_best(ok, count, h, a.best + f);
}

__global__ __launch_bounds__(kRansacThreads) void k_pnp_finish(PnpArgs a) {
    __shared__ double mat3[6 * 3];  // M^T M, then V
    __shared__ double pose_s[12];
    __shared__ int has_pose;
    __shared__ int total;
    const int f = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x), lane = lane_id();
    const int nf = frame_count(a.q_counts, f, a.q_stride);
    int h;
    double P[12];
    const bool won = winner(a, f, h, P);

    if (tid < kWave) {  // winner to pose, on one wave
        if (tid == 0) gram3_identity<4>(P, mat3);
        wave_lds_sync();
        jacobi<3, kPnpSweeps>(mat3, lane);
        wave_lds_sync();
        if (tid == 0) {
            double d[3], sd[3], V[9], W[9], R[9], t[3];
            const double Mm[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = mat3[3 * k + k];
#pragma unroll
            for (int c = 0; c < 9; ++c) V[c] = mat3[9 + c];
            double dmin = d[0], dmax = d[0];
#pragma unroll
            for (int k = 1; k < 3; ++k) {
                if (d[k] < dmin) dmin = d[k];
                if (d[k] > dmax) dmax = d[k];
            }
            bool ok = won && isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]) && dmin > 1e-12 * dmax;
#pragma unroll
            for (int k = 0; k < 3; ++k) sd[k] = sqrt(d[k]);
            matmul3(Mm, V, W);
            const double ks = ((sd[0] + sd[1]) + sd[2]) / 3.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    double s = 0.0;
#pragma unroll
                    for (int j = 0; j < 3; ++j) s = s + (W[3 * i + j] / sd[j]) * V[3 * k + j];
                    R[3 * i + k] = s;
                    ok = ok && isfinite(s) && isfinite(V[3 * i + k]);
                }
                const double tc = P[4 * i + 3] / ks;
                t[i] = tc / a.scale - dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], a.center[0], a.center[1], a.center[2]);
                ok = ok && isfinite(t[i]);
            }
#pragma unroll
            for (int c = 0; c < 9; ++c) pose_s[c] = ok ? R[c] : 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) pose_s[9 + c] = ok ? t[c] : 0.0;
            has_pose = ok ? 1 : 0;
        }
    }
    __syncthreads();
    const bool has = has_pose != 0;  // without a pose the frame is as one without a valid hypothesis
    const int count = classify_slots<Corr5>(a, f, nf, has, &total,
                                            [&](const Corr5 &p) { return pnp_inlier(P, p, a.cam[0], a.cam[1], a.tt); });
    if (tid != 0) return;
    if (a.out_counts) a.out_counts[f] = count;
    if (a.out_best) a.out_best[f] = has ? h : -1;
    double *op = a.out_model + static_cast<int64_t>(f) * 12;
#pragma unroll
    for (int c = 0; c < 12; ++c) op[c] = pose_s[c];
}

// The 3 x 4 matrix [R | t] of a pose stored R row-major, then t.
__device__ __forceinline__ void pose_matrix(const double *pose, double (&P)[12]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) P[4 * i + j] = pose[3 * i + j];
        P[4 * i + 3] = pose[9 + i];
    }
}

// One workgroup per frame, all rounds, in fd_estimate.h's refit frame: a thread's list positions i = t (mod 256)
// are also the contract's partial t of the sums, so its 27 sums stay in registers over the frame.
__global__ __launch_bounds__(kRansacThreads) void k_pnp_refit(PnpRefitArgs g) {
    __shared__ double red[kSlice * kRansacThreads];
    __shared__ double sys[6 * 7];
    __shared__ double poses[2][12];  // the current pose and the round's candidate, by turns with the support set's halves
    __shared__ int cand_ok;
    __shared__ int total;
    const PnpArgs &a = g.r;
    const int f = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x);
    const int nf = frame_count(a.q_counts, f, a.q_stride);
    const int64_t s0 = static_cast<int64_t>(f) * a.q_stride;
    const int n = a.n[f];
    const double fx = a.cam[0], fy = a.cam[1];
    const Corr5 *corr = reinterpret_cast<const Corr5 *>(a.corr) + s0;
    Support sup{g.member + 2 * s0, a.q_stride, 0};
    if (tid < 12) poses[0][tid] = g.in_model[static_cast<int64_t>(f) * 12 + tid];
    load_members(a, f, nf, g.in_inlier, sup.mem);  // its barrier: the pose too
    double P[12];
    pose_matrix(poses[0], P);
    uint32_t mine = 0, mine0 = 0;
    for (int i = tid; i < n; i += kRansacThreads) {
        mine0 += sup.mem[i];
        mine += pnp_inlier(P, corr[i], fx, fy, a.tt) ? 1u : 0u;
    }
    const int members0 = wg_count(mine0, &total);
    sup.count = wg_count(mine, &total);  // c_0: what in_model classifies, not |S_0|

    for (int round = 0; round < g.rounds; ++round) {  // every exit is uniform over the workgroup
        double pose[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) pose[c] = poses[sup.cur][c];
        double *cand_s = poses[sup.cur ^ 1];
        const uint8_t *S = sup.current();
        double acc[kGn];
#pragma unroll
        for (int e = 0; e < kGn; ++e) acc[e] = 0.0;
        for (int i = tid; i < n; i += kRansacThreads) {
            if (!S[i]) continue;
            const Corr5 p = corr[i];
            const double y0 = pose[0] * p.X + pose[1] * p.Y + pose[2] * p.Z + pose[9];
            const double y1 = pose[3] * p.X + pose[4] * p.Y + pose[5] * p.Z + pose[10];
            const double y2 = pose[6] * p.X + pose[7] * p.Y + pose[8] * p.Z + pose[11];
            const double iz = 1.0 / y2;
            const double u = y0 * iz, v = y1 * iz;
            const double jx[7] = {fx * -(u * v), fx * (1.0 + u * u), fx * -v, fx * iz, 0.0, fx * -(u * iz), fx * (u - p.bx)};
            const double jy[7] = {fy * -(1.0 + v * v), fy * (u * v), fy * u, 0.0, fy * iz, fy * -(v * iz), fy * (v - p.by)};
            int e = 0;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = r; c < 7; ++c, ++e) {
                    acc[e] = acc[e] + jx[r] * jx[c];
                    acc[e] = acc[e] + jy[r] * jy[c];
                }
        }
        reduce_upper<kGn, 7, false>(acc, red, sys);
        if (tid == 0) {  // the step, and the pose it leads to
            double x[7];
            bool valid = null_vector<6, 1>(sys, x);
            const double h[3] = {x[0] / 2.0, x[1] / 2.0, x[2] / 2.0};
            const double hh = h[0] * h[0] + h[1] * h[1] + h[2] * h[2];
            const double fc = 2.0 / (1.0 + hh);
            const double K[9] = {0.0, -h[2], h[1], h[2], 0.0, -h[0], -h[1], h[0], 0.0};
            double C[9], R[9], Rn[9];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    C[3 * i + j] = (i == j ? 1.0 : 0.0) + fc * (K[3 * i + j] + (h[i] * h[j] - (i == j ? hh : 0.0)));
#pragma unroll
            for (int c = 0; c < 9; ++c) R[c] = pose[c];
            matmul3(C, R, Rn);
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                cand_s[c] = Rn[c];
                valid = valid && isfinite(Rn[c]);
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double tn = dot3(C[3 * i], C[3 * i + 1], C[3 * i + 2], pose[9], pose[10], pose[11]) + x[3 + i];
                cand_s[9 + i] = tn;
                valid = valid && isfinite(tn);
            }
            cand_ok = valid ? 1 : 0;
        }
        __syncthreads();
        if (!cand_ok) break;
        pose_matrix(poses[sup.cur ^ 1], P);
        const int c = reclassify(corr, n, sup.candidate(), &total, [&](const Corr5 &p) { return pnp_inlier(P, p, fx, fy, a.tt); });
        if (!sup.accept(c)) break;
    }

    write_members(a, f, nf, sup.current());
    if (tid != 0) return;
    if (a.out_counts) a.out_counts[f] = sup.done ? sup.count : members0;
    if (g.out_rounds) g.out_rounds[f] = sup.done;
    double *op = a.out_model + static_cast<int64_t>(f) * 12;
    if (sup.done)
        copy_bits<12>(poses[sup.cur], op);
    else  // in_model's bits as they are (out_model may be in_model)
        copy_bits<12>(g.in_model + static_cast<int64_t>(f) * 12, op);
}

}  // namespace

hipError_t launch_pnp_ransac(const PnpArgs &a, hipStream_t s) {
    const int64_t blocks = static_cast<int64_t>(a.batch) * ((a.hypotheses + kWave - 1) / kWave);
    if (a.batch < 1 || blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    const dim3 frames(static_cast<unsigned>(a.batch)), hyps(static_cast<unsigned>(blocks));
    hipLaunchKernelGGL(k_pnp_compact, frames, dim3(kRansacThreads), 0, s, a);
    hipLaunchKernelGGL(k_pnp_hyp, hyps, dim3(kWave), 0, s, a);
    hipLaunchKernelGGL(k_pnp_finish, frames, dim3(kRansacThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pnp_refit(const PnpRefitArgs &a, hipStream_t s) {
    if (a.r.batch < 1) return hipErrorInvalidValue;
    const dim3 frames(static_cast<unsigned>(a.r.batch));
    hipLaunchKernelGGL(k_pnp_compact, frames, dim3(kRansacThreads), 0, s, a.r);
    hipLaunchKernelGGL(k_pnp_refit, frames, dim3(kRansacThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace fdk
