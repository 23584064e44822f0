// Alignment of two 3-D point sets with known correspondences (fd_align_ransac, fd_align_refit, fd_align_apply of
// include/fd_hip.h): a fixed number of 3-point similarity (or rigid) transforms Y = s R X + t, all evaluated, and a
// closed-form least-squares refit of the winner on its inliers by Horn's quaternion method. Every floating point
// operation is a double one, rounded once (the build passes -ffp-contract=off), in the contract's order, so the
// result is a definite one that tests/align_ref.py restates bit for bit. The sampler and the Jacobi routine are
// fd_ransac's (fd_solve.h), and so is the skeleton around them (fd_estimate.h: compaction, score and vote, the finish
// walk, the refit's frame and sum tree): what stands here is the alignment problem's own arithmetic.
//
// k_align_compact, one workgroup per frame: the ordered list of the frame's correspondences (source and target point,
// 48 bytes each) by a workgroup prefix over the take flags, and every slot's index in it.
// k_align_hyp, one wave per workgroup, a lane per hypothesis: the lane samples three correspondences and builds its
// model in registers from the two triangles' orthonormal frames (no system, no elimination); the correspondences then
// pass through a broadcast tile, each lane counting its own model's inliers, and the wave's best goes to the frame's
// 64-bit slot in one atomicMax. k_align_finish, one workgroup per frame: every slot classified by the winner.
//
// k_align_refit, one workgroup per frame after k_align_compact: every round inside one launch. Two passes over the
// members (the six sums of the centroids, then the nine cross products and the source's spread about them), each
// through the LDS tree; the first wave runs the 4 x 4 Jacobi, thread 0 turns the quaternion into the model, and every
// correspondence is classified again. k_align_apply: one thread per point slot.
#include "fd_estimate.h"

namespace fdk {
namespace {

constexpr int kAlignModel = 13;  // R row-major, t, s
constexpr int kAlignSweeps = FD_ALIGN_SWEEPS;
constexpr int kAlignSums = 10;   // the second pass: A[3][3] row-major, then Sx (the first pass uses six)

// A correspondence: the source point and its target.
struct Corr6 {
    double X[3], Y[3];
};

// z = s * (R X) + t, the expression of the inlier test and of fd_align_apply.
__device__ __forceinline__ void align_map(const double (&m)[kAlignModel], const double (&X)[3], double (&z)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) z[i] = m[12] * dot3(m[3 * i], m[3 * i + 1], m[3 * i + 2], X[0], X[1], X[2]) + m[9 + i];
}

// The inlier test: the squared distance of the mapped source point from the target against tt = th * th; a NaN fails.
__device__ __forceinline__ bool align_inlier(const double (&m)[kAlignModel], const Corr6 &p, double tt) {
    double z[3];
    align_map(m, p.X, z);
    const double e0 = p.Y[0] - z[0], e1 = p.Y[1] - z[1], e2 = p.Y[2] - z[2];
    return e0 * e0 + e1 * e1 + e2 * e2 <= tt;
}

__device__ __forceinline__ double dot3v(const double (&a)[3], const double (&b)[3]) {
    return dot3(a[0], a[1], a[2], b[0], b[1], b[2]);
}

// The right-handed orthonormal frame (e1, e2, e3) of the triangle sides u, v by Gram-Schmidt; false for a
// zero u or a v (nearly) along it.
__device__ __forceinline__ bool side_frame(const double (&u)[3], const double (&v)[3], double (&e1)[3], double (&e2)[3],
                                           double (&e3)[3]) {
    const double uu = dot3v(u, u);
    const double su = sqrt(uu);
#pragma unroll
    for (int k = 0; k < 3; ++k) e1[k] = u[k] / su;
    const double d = dot3v(v, e1);
    double w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = v[k] - d * e1[k];
    const double ww = dot3v(w, w);
    const double sw = sqrt(ww);
#pragma unroll
    for (int k = 0; k < 3; ++k) e2[k] = w[k] / sw;
    e3[0] = e1[1] * e2[2] - e1[2] * e2[1];
    e3[1] = e1[2] * e2[0] - e1[0] * e2[2];
    e3[2] = e1[0] * e2[1] - e1[1] * e2[0];
    return uu > 0.0 && ww > 1e-12 * dot3v(v, v);
}

// U.U + V.V + (V - U).(V - U): the summed squared side lengths of a triangle.
__device__ __forceinline__ double side_lengths(const double (&u)[3], const double (&v)[3]) {
    const double g[3] = {v[0] - u[0], v[1] - u[1], v[2] - u[2]};
    return dot3v(u, u) + dot3v(v, v) + dot3v(g, g);
}

__device__ __forceinline__ bool all_finite(const double (&m)[kAlignModel]) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < kAlignModel; ++c) ok = ok && isfinite(m[c]);
    return ok;
}

__global__ __launch_bounds__(kRansacThreads) void k_align_compact(AlignArgs a) {
    __shared__ uint32_t wsum[kRansacThreads / kWave];
    compact_slots<Corr6>(a, wsum, [&](int64_t qi, int64_t ti, Corr6 &p) {
        if (a.q_valid && a.q_valid[qi] != 1) return false;
        if (a.t_valid && a.t_valid[ti] != 1) return false;
        const float *q = a.q_xyz + 3 * qi, *t = a.t_xyz + 3 * ti;
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float qv = q[k], tv = t[k];
            p.X[k] = static_cast<double>(qv);
            p.Y[k] = static_cast<double>(tv);
            finite = finite && isfinite(qv) && isfinite(tv);
        }
        return finite;
    });
}

__global__ __launch_bounds__(kWave) void k_align_hyp(AlignArgs a) {
    constexpr int M = 3;
    __shared__ Corr6 tile[kTile];
    int f, h;
    hypothesis_index(a.hypotheses, f, h);
    const int n = a.n[f];
    const Corr6 *corr = reinterpret_cast<const Corr6 *>(a.corr) + static_cast<int64_t>(f) * a.q_stride;
    int pick[M];
    bool ok = h < a.hypotheses;
    ok = sample<M>(a.seed, f, h, n, pick) && ok;
    Corr6 p[M] = {};
    if (ok) {
#pragma unroll
        for (int k = 0; k < M; ++k) p[k] = corr[pick[k]];  // pick < n <= q_stride
    }
    double u[3], v[3], U[3], V[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u[k] = p[1].X[k] - p[0].X[k];
        v[k] = p[2].X[k] - p[0].X[k];
        U[k] = p[1].Y[k] - p[0].Y[k];
        V[k] = p[2].Y[k] - p[0].Y[k];
    }
    double e1[3], e2[3], e3[3], f1[3], f2[3], f3[3];
    ok = side_frame(u, v, e1, e2, e3) && ok;
    ok = side_frame(U, V, f1, f2, f3) && ok;
    double m[kAlignModel];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) m[3 * i + j] = f1[i] * e1[j] + f2[i] * e2[j] + f3[i] * e3[j];
    m[12] = a.kind == FD_ALIGN_RIGID ? 1.0 : sqrt(side_lengths(U, V) / side_lengths(u, v));
    double Xm[3], Ym[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        Xm[k] = p[0].X[k] + (u[k] + v[k]) / 3.0;
        Ym[k] = p[0].Y[k] + (U[k] + V[k]) / 3.0;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) m[9 + i] = Ym[i] - m[12] * dot3(m[3 * i], m[3 * i + 1], m[3 * i + 2], Xm[0], Xm[1], Xm[2]);
    ok = ok && all_finite(m) && m[12] > 0.0;

    const int count = count_inliers(corr, n, tile, [&](const Corr6 &c) { return align_inlier(m, c, a.tt); });
    if (ok) {
        double *dst = model_at<kAlignModel>(a.models, f, a.hypotheses, h);
#pragma unroll
        for (int c = 0; c < kAlignModel; ++c) dst[c] = m[c];
    }
    vote_best(ok, count, h, a.best + f);
}

__global__ __launch_bounds__(kRansacThreads) void k_align_finish(AlignArgs a) {
    __shared__ int total;
    const int f = static_cast<int>(blockIdx.x);
    const int nf = frame_count(a.q_counts, f, a.q_stride);
    int h;
    double m[kAlignModel];
    const bool has = winner(a, f, h, m);
    const int count = classify_slots<Corr6>(a, f, nf, has, &total, [&](const Corr6 &p) { return align_inlier(m, p, a.tt); });
    if (threadIdx.x != 0) return;
    if (a.out_counts) a.out_counts[f] = count;
    if (a.out_best) a.out_best[f] = h;
    double *om = a.out_model + static_cast<int64_t>(f) * kAlignModel;
#pragma unroll
    for (int c = 0; c < kAlignModel; ++c) om[c] = m[c];
}

// Horn's matrix of the cross sums A (row-major, source row and target column) and the identity behind it:
// jacobi<4>'s input, by one thread.
__device__ __forceinline__ void horn_identity(const double *A, double *mat4) {
    const double Sxx = A[0], Sxy = A[1], Sxz = A[2], Syx = A[3], Syy = A[4], Syz = A[5], Szx = A[6], Szy = A[7], Szz = A[8];
    const double N[16] = {Sxx + Syy + Szz, Syz - Szy,       Szx - Sxz,        Sxy - Syx,
                          Syz - Szy,       Sxx - Syy - Szz, Sxy + Syx,        Szx + Sxz,
                          Szx - Sxz,       Sxy + Syx,       -Sxx + Syy - Szz, Syz + Szy,
                          Sxy - Syx,       Szx + Sxz,       Syz + Szy,        -Sxx - Syy + Szz};
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        mat4[c] = N[c];
        mat4[16 + c] = (c >> 2) == (c & 3) ? 1.0 : 0.0;
    }
}

// The model of a round from the Jacobi's result (diagonal and V in mat4), the sums A and Sx and the centroids;
// false for an invalid round.
__device__ __forceinline__ bool horn_model(const double *mat4, const double *sums, const double (&Xb)[3], const double (&Yb)[3],
                                           int kind, double (&m)[kAlignModel]) {
    int at = 0;
    double top = mat4[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (mat4[4 * k + k] > top) {
            top = mat4[4 * k + k];
            at = k;
        }
    const double a = mat4[16 + at], b = mat4[20 + at], c = mat4[24 + at], d = mat4[28 + at];
    const double qq = a * a + b * b + c * c + d * d;
    m[0] = (a * a + b * b - c * c - d * d) / qq;
    m[1] = (2.0 * (b * c - a * d)) / qq;
    m[2] = (2.0 * (b * d + a * c)) / qq;
    m[3] = (2.0 * (b * c + a * d)) / qq;
    m[4] = (a * a - b * b + c * c - d * d) / qq;
    m[5] = (2.0 * (c * d - a * b)) / qq;
    m[6] = (2.0 * (b * d - a * c)) / qq;
    m[7] = (2.0 * (c * d + a * b)) / qq;
    m[8] = (a * a - b * b - c * c + d * d) / qq;
    const double Sx = sums[9];
    double s = 1.0;
    if (kind != FD_ALIGN_RIGID) {
        double tr = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) tr = tr + m[3 * i + j] * sums[3 * j + i];
        s = tr / Sx;
    }
    m[12] = s;
#pragma unroll
    for (int i = 0; i < 3; ++i) m[9 + i] = Yb[i] - s * dot3(m[3 * i], m[3 * i + 1], m[3 * i + 2], Xb[0], Xb[1], Xb[2]);
    return Sx > 0.0 && all_finite(m) && s > 0.0;
}

// One workgroup per frame, all rounds, in fd_estimate.h's refit frame: a thread's list positions i = t (mod 256)
// are also the contract's partial t of the sums, so its sums stay in registers over the frame.
__global__ __launch_bounds__(kRansacThreads) void k_align_refit(AlignRefitArgs g) {
    __shared__ double red[kAlignSums * kRansacThreads];
    __shared__ double sums[kAlignSums];
    __shared__ double mat4[2 * 16];                // Horn's matrix, then V
    __shared__ double models[2][kAlignModel];  // the current model and the round's candidate, by turns with the support set's halves
    __shared__ int cand_ok;
    __shared__ int total;
    const AlignArgs &a = g.r;
    const int f = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x);
    const int nf = frame_count(a.q_counts, f, a.q_stride);
    const int64_t s0 = static_cast<int64_t>(f) * a.q_stride;
    const int n = a.n[f];
    const Corr6 *corr = reinterpret_cast<const Corr6 *>(a.corr) + s0;
    Support sup{g.member + 2 * s0, a.q_stride, 0};
    if (tid < kAlignModel) models[0][tid] = g.in_model[static_cast<int64_t>(f) * kAlignModel + tid];
    load_members(a, f, nf, g.in_inlier, sup.mem);  // its barrier: the model too
    double m[kAlignModel];
#pragma unroll
    for (int c = 0; c < kAlignModel; ++c) m[c] = models[0][c];
    uint32_t mine = 0, mine0 = 0;
    for (int i = tid; i < n; i += kRansacThreads) {
        mine0 += sup.mem[i];
        mine += align_inlier(m, corr[i], a.tt) ? 1u : 0u;
    }
    const int members0 = wg_count(mine0, &total);
    sup.count = wg_count(mine, &total);  // c_0: what in_model classifies, not |S_0|
    int members = members0;

    for (int round = 0; round < g.rounds; ++round) {  // every exit is uniform over the workgroup
        if (members < 3) break;
        double *cand_s = models[sup.cur ^ 1];
        const uint8_t *S = sup.current();
        double c6[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) c6[e] = 0.0;
        for (int i = tid; i < n; i += kRansacThreads) {
            if (!S[i]) continue;
            const Corr6 p = corr[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                c6[k] = c6[k] + p.X[k];
                c6[3 + k] = c6[3 + k] + p.Y[k];
            }
        }
        reduce_sums<6>(c6, red, sums);
        const double dm = static_cast<double>(members);
        const double Xb[3] = {sums[0] / dm, sums[1] / dm, sums[2] / dm};
        const double Yb[3] = {sums[3] / dm, sums[4] / dm, sums[5] / dm};
        double acc[kAlignSums];
#pragma unroll
        for (int e = 0; e < kAlignSums; ++e) acc[e] = 0.0;
        for (int i = tid; i < n; i += kRansacThreads) {
            if (!S[i]) continue;
            const Corr6 p = corr[i];
            const double xc[3] = {p.X[0] - Xb[0], p.X[1] - Xb[1], p.X[2] - Xb[2]};
            const double yc[3] = {p.Y[0] - Yb[0], p.Y[1] - Yb[1], p.Y[2] - Yb[2]};
#pragma unroll
            for (int i2 = 0; i2 < 3; ++i2)
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[3 * i2 + j] = acc[3 * i2 + j] + xc[i2] * yc[j];
            acc[9] = acc[9] + dot3v(xc, xc);
        }
        reduce_sums<kAlignSums>(acc, red, sums);  // every thread has read the centroids: the tree's barriers lie between
        if (tid < kWave) {  // the quaternion, on one wave
            if (tid == 0) horn_identity(sums, mat4);
            wave_lds_sync();
            jacobi<4, kAlignSweeps>(mat4, lane_id());
            wave_lds_sync();
            if (tid == 0) {
                double cand[kAlignModel];
                const bool valid = horn_model(mat4, sums, Xb, Yb, a.kind, cand);
#pragma unroll
                for (int c = 0; c < kAlignModel; ++c) cand_s[c] = cand[c];
                cand_ok = valid ? 1 : 0;
            }
        }
        __syncthreads();
        if (!cand_ok) break;
#pragma unroll
        for (int c = 0; c < kAlignModel; ++c) m[c] = cand_s[c];
        const int c = reclassify(corr, n, sup.candidate(), &total, [&](const Corr6 &p) { return align_inlier(m, p, a.tt); });
        if (!sup.accept(c)) break;
        members = c;
    }

    write_members(a, f, nf, sup.current());
    if (tid != 0) return;
    if (a.out_counts) a.out_counts[f] = sup.done ? sup.count : members0;
    if (g.out_rounds) g.out_rounds[f] = sup.done;
    double *om = a.out_model + static_cast<int64_t>(f) * kAlignModel;
    if (sup.done)
        copy_bits<kAlignModel>(models[sup.cur], om);
    else  // in_model's bits as they are (out_model may be in_model)
        copy_bits<kAlignModel>(g.in_model + static_cast<int64_t>(f) * kAlignModel, om);
}

// One thread per point slot; a slot reads its own point only before it writes it (xyz_out may be xyz_in).
__global__ __launch_bounds__(kRansacThreads) void k_align_apply(AlignApplyArgs a) {
    const int64_t slot = static_cast<int64_t>(blockIdx.x) * kRansacThreads + threadIdx.x;
    if (slot >= static_cast<int64_t>(a.batch) * a.stride) return;
    const int f = static_cast<int>(slot / a.stride), i = static_cast<int>(slot - static_cast<int64_t>(f) * a.stride);
    if (i >= frame_count(a.counts, f, a.stride)) return;
    if (a.valid && a.valid[slot] != 1) return;
    double m[kAlignModel];
#pragma unroll
    for (int c = 0; c < kAlignModel; ++c) m[c] = a.model[static_cast<int64_t>(f) * kAlignModel + c];
    const float *in = a.xyz_in + 3 * slot;
    const double X[3] = {static_cast<double>(in[0]), static_cast<double>(in[1]), static_cast<double>(in[2])};
    double z[3];
    align_map(m, X, z);
    float *out = a.xyz_out + 3 * slot;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = static_cast<float>(z[k]);
}

}  // namespace

hipError_t launch_align_ransac(const AlignArgs &a, hipStream_t s) {
    const int64_t blocks = static_cast<int64_t>(a.batch) * ((a.hypotheses + kWave - 1) / kWave);
    if (a.batch < 1 || blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    const dim3 frames(static_cast<unsigned>(a.batch)), hyps(static_cast<unsigned>(blocks));
    hipLaunchKernelGGL(k_align_compact, frames, dim3(kRansacThreads), 0, s, a);
    hipLaunchKernelGGL(k_align_hyp, hyps, dim3(kWave), 0, s, a);
    hipLaunchKernelGGL(k_align_finish, frames, dim3(kRansacThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_align_refit(const AlignRefitArgs &a, hipStream_t s) {
    if (a.r.batch < 1) return hipErrorInvalidValue;
    const dim3 frames(static_cast<unsigned>(a.r.batch));
    hipLaunchKernelGGL(k_align_compact, frames, dim3(kRansacThreads), 0, s, a.r);
    hipLaunchKernelGGL(k_align_refit, frames, dim3(kRansacThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_align_apply(const AlignApplyArgs &a, hipStream_t s) {
    const int64_t blocks = (static_cast<int64_t>(a.batch) * a.stride + kRansacThreads - 1) / kRansacThreads;
    if (a.batch < 1 || a.stride < 1 || blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_align_apply, dim3(static_cast<unsigned>(blocks)), dim3(kRansacThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace fdk
