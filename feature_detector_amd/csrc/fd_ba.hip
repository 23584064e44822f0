// Windowed bundle adjustment (fd_bundle_adjust of include/fd_hip.h): the poses of up to 8 cameras and the 3-D
// points they share, refined by Levenberg-Marquardt on a truncated reprojection cost, the points eliminated by
// the Schur complement. Every floating point operation is a double one, rounded once (the build passes
// -ffp-contract=off), in the contract's order, so the result is a definite one that tests/ba_ref.py restates bit
// for bit.
//
// k_bundle_adjust, one workgroup of 256 per problem, every trial inside one launch. A trial is five passes with
// workgroup barriers between them:
//   point pass   a thread per point slot t, t + 256, ..., looping over the cameras: the rows of every active
//                observation, V_i, g_i, the inverse of the damped V_i by its adjugate, then W_ci and Y_ci of the
//                free cameras, all into the context workspace (52 doubles per observation, 15 per point).
//   system pass  a thread per entry (a, b), a <= b, of the R x (R + 1) Schur system in LDS, walking the points in
//                ascending order: the order of every sum is the contract's by construction, whatever the launch.
//   elimination  complete pivoting at run-time size R = 6 x (free cameras) <= 48, cooperative: a thread per
//                column and a wave per row residue; every element update is one a - f*b, so the bits are those of
//                a one-lane loop. The pivot is the largest magnitude, the lowest row-major index among equals.
//                Back substitution runs on one wave, a lane per row, the sums taking the columns in descending
//                order (R steps instead of R * R / 2 dependent ones).
//   update       a thread per free camera (Cayley transform) and per point slot (back substitution through V^-1).
//   cost         256 partials over the slots, then the LDS tree.
#include "fd_match_common.h"
#include "fd_solve.h"

namespace fdk {
namespace {

constexpr int kBaThreads = kRansacThreads;
constexpr int kBaWaves = kBaThreads / kWave;
constexpr int kBaRows = 6 * FD_BA_MAX_CAMS;  // 48
constexpr int kBaCols = kBaRows + 1;         // the row pitch of the system in LDS
// an observation's workspace: jx[7], jy[7], W[6][3], Y[6][3], bx, by
constexpr int kObsJx = 0, kObsJy = 7, kObsW = 14, kObsY = 32, kObsRay = 50;
static_assert(kBaObsDoubles == 52 && kBaPointDoubles == 15, "the host sizes the workspace");
// a point's workspace: X of the two states by turns (2 x 3), the inverse's six entries (00 01 02 11 12 22), g[3]
constexpr int kPtInv = 6, kPtG = 12;
// an observation's byte: active in this linearisation, its point eliminated, it exists
constexpr uint8_t kActive = 1, kElim = 2, kExists = 4;

// A workgroup-uniform double kept in a vector register: the trial loop's uniform doubles (the cost, the damping, the
// focal lengths) otherwise take scalar register pairs for its whole length, and the kernel runs at its SGPR limit.
__device__ __forceinline__ double in_vgpr(double x) {
    asm volatile("" : "+v"(x));
    return x;
}

template <typename T>
__device__ __forceinline__ T *in_vgpr(T *p) {
    asm volatile("" : "+v"(p));
    return p;
}

struct Proj {
    double y0, y1, y2;
};

__device__ __forceinline__ Proj project(const double *pose, double X, double Y, double Z) {
    Proj p;
    p.y0 = pose[0] * X + pose[1] * Y + pose[2] * Z + pose[9];
    p.y1 = pose[3] * X + pose[4] * Y + pose[5] * Z + pose[10];
    p.y2 = pose[6] * X + pose[7] * Y + pose[8] * Z + pose[11];
    return p;
}

// The cost term of an observation and whether it is in the active set: e <= tt in front of the camera.
__device__ __forceinline__ double cost_term(const Proj &p, double bx, double by, double fx, double fy, double tt, bool &active) {
    active = false;
    if (!(p.y2 > 0.0)) return tt;
    const double a = p.y0 / p.y2, b = p.y1 / p.y2;
    const double dx = fx * (a - bx), dy = fy * (b - by);
    const double e = dx * dx + dy * dy;
    active = e <= tt;
    return active ? e : tt;
}

// The workgroup's sum of 256 partials by the contract's tree; every thread gets it.
__device__ __forceinline__ double wg_tree(double mine, double *red) {
    const int tid = static_cast<int>(threadIdx.x);
    __syncthreads();
    red[tid] = mine;
    for (int step = kBaThreads / 2; step >= 1; step >>= 1) {
        __syncthreads();
        if (tid < step) red[tid] = red[tid] + red[tid + step];
    }
    __syncthreads();
    return red[0];
}

struct Problem {
    int n, cams;
    const uint8_t *act;   // [cams][p_stride]
    const double *obs;    // [cams][p_stride][52]
    const double *pts;    // [p_stride][15]
    int p_stride;
    double fx, fy, tt;
};

// The cost of state `st` (its poses and its points); FINAL: also the bytes of out_inlier and their number.
template <bool FINAL>
__device__ __forceinline__ double state_cost(const Problem &q, const double (*poses)[12], int st, double *red, uint8_t *out_inlier,
                                             int o_stride, uint32_t &ones) {
    const int tid = static_cast<int>(threadIdx.x);
    double part = 0.0;
    ones = 0;
    for (int i = tid; i < q.n; i += kBaThreads) {
        const double *X = q.pts + static_cast<int64_t>(i) * kBaPointDoubles + 3 * st;
        const double X0 = X[0], X1 = X[1], X2 = X[2];
        for (int c = 0; c < q.cams; ++c) {
            const int64_t oi = static_cast<int64_t>(c) * q.p_stride + i;
            bool active = false;
            if (q.act[oi] & kExists) {
                const double *ray = q.obs + oi * kBaObsDoubles + kObsRay;
                part = part + cost_term(project(poses[c], X0, X1, X2), ray[0], ray[1], q.fx, q.fy, q.tt, active);
            }
            if (FINAL) {
                if (out_inlier) out_inlier[static_cast<int64_t>(c) * o_stride + i] = active ? 1 : 0;  // i < p_stride <= o_stride
                ones += active ? 1u : 0u;
            }
        }
    }
    return wg_tree(part, red);
}

__global__ __launch_bounds__(kBaThreads) void k_bundle_adjust(BaArgs karg) {
    // The argument block is staged in LDS once and read from there where a pass needs a field: kept in scalar
    // registers across the trial loop, its thirty pointers and scalars spilled 60 SGPRs.
    __shared__ BaArgs a;
    __shared__ double A[kBaRows * kBaCols];
    __shared__ double red[kBaThreads];
    __shared__ double poses[2][FD_BA_MAX_CAMS][12];  // the current state's and the trial's, by turns
    __shared__ double fv[kBaRows];                   // a step's row factors
    __shared__ double ys[kBaCols], xs[kBaCols];      // back substitution; the step
    __shared__ unsigned long long wkey[kBaWaves];
    __shared__ int widx[kBaWaves];
    __shared__ int perm[kBaCols];
    __shared__ int fidx[FD_BA_MAX_CAMS];  // a camera's index among the free ones, or -1
    __shared__ int freec[FD_BA_MAX_CAMS];
    __shared__ int nfree, trial_ok, cand_ok, total;

    if (threadIdx.x == 0) a = karg;
    __syncthreads();
    const int b = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x), lane = lane_id(), wv = tid / kWave;
    const int C = a.cams, ps = opaque(a.p_stride);  // opaque: held in vector registers, like in_vgpr's values
    const int n = opaque(frame_count(a.counts, b, ps));
    const double fx = in_vgpr(a.cam[0]), fy = in_vgpr(a.cam[1]);
    uint8_t *act = in_vgpr(a.act + static_cast<int64_t>(b) * C * ps);
    double *obs = in_vgpr(a.obs + static_cast<int64_t>(b) * C * ps * kBaObsDoubles);
    double *pts = in_vgpr(a.pts + static_cast<int64_t>(b) * ps * kBaPointDoubles);

    if (tid < C * 12) poses[0][tid / 12][tid % 12] = a.in_poses[static_cast<int64_t>(b) * C * 12 + tid];
    if (tid == 0) {
        int f = 0;
        for (int c = 0; c < C; ++c) {
            const bool fixed = a.cam_fixed ? a.cam_fixed[static_cast<int64_t>(b) * C + c] != 0 : c == 0;
            fidx[c] = fixed ? -1 : f;
            if (!fixed) freec[f++] = c;
        }
        nfree = f;
    }
    // the observations that exist, their rays, and the points' first state
    for (int i = tid; i < n; i += kBaThreads) {
        const float *pin = a.p_xyz + static_cast<int64_t>(b) * ps * 3;
        const float px = pin[3 * i], py = pin[3 * i + 1], pz = pin[3 * i + 2];
        const bool pok = (!a.p_valid || a.p_valid[static_cast<int64_t>(b) * ps + i] == 1) && isfinite(px) && isfinite(py) && isfinite(pz);
        double *X = pts + static_cast<int64_t>(i) * kBaPointDoubles;
        X[0] = static_cast<double>(px);
        X[1] = static_cast<double>(py);
        X[2] = static_cast<double>(pz);
        for (int c = 0; c < C; ++c) {
            const int64_t si = (static_cast<int64_t>(b) * C + c) * a.o_stride + i;  // i < p_stride <= o_stride
            const int64_t oi = static_cast<int64_t>(c) * ps + i;
            bool ex = pok && (!a.obs_valid || a.obs_valid[si] == 1);
            if (ex) {
                const float u = a.obs_xy[2 * si], v = a.obs_xy[2 * si + 1];
                ex = isfinite(u) && isfinite(v);
                obs[oi * kBaObsDoubles + kObsRay] = (static_cast<double>(u) - a.cam[2]) / fx;
                obs[oi * kBaObsDoubles + kObsRay + 1] = (static_cast<double>(v) - a.cam[3]) / fy;
            }
            act[oi] = ex ? kExists : 0;
        }
    }
    __syncthreads();
    const int F = nfree, R = 6 * F;
    Problem q = {n, C, act, obs, pts, ps, fx, fy, in_vgpr(a.tt)};
    int cur = 0, done = 0;  // the state in force (poses[cur], X at 3 * cur); accepted trials
    uint32_t ones;
    const double cost0 = in_vgpr(state_cost<false>(q, poses[0], 0, red, nullptr, 0, ones));
    double cost = cost0, lam = in_vgpr(a.lambda);

    for (int trial = 0; trial < a.rounds; ++trial) {  // every branch on the trial's state is uniform over the workgroup
        const double damp = in_vgpr(1.0 + lam);
        const double (*P)[12] = poses[cur];
        // ---- point pass
        for (int i = tid; i < n; i += kBaThreads) {
            double *pt = pts + static_cast<int64_t>(i) * kBaPointDoubles;
            const double X0 = pt[3 * cur], X1 = pt[3 * cur + 1], X2 = pt[3 * cur + 2];
            double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
            int nact = 0;
            for (int c = 0; c < C; ++c) {
                const int64_t oi = static_cast<int64_t>(c) * ps + i;
                const uint8_t ex = act[oi] & kExists;
                bool active = false;
                if (ex) {
                    double *o = obs + oi * kBaObsDoubles;
                    const double bx = o[kObsRay], by = o[kObsRay + 1];
                    const double *pose = P[c];
                    const Proj y = project(pose, X0, X1, X2);
                    cost_term(y, bx, by, fx, fy, q.tt, active);
                    if (active) {
                        const double iz = 1.0 / y.y2;
                        const double u = y.y0 * iz, v = y.y1 * iz;
                        const double jx[7] = {fx * -(u * v), fx * (1.0 + u * u), fx * -v, fx * iz, 0.0, fx * -(u * iz), fx * (u - bx)};
                        const double jy[7] = {fy * -(1.0 + v * v), fy * (u * v), fy * u, 0.0, fy * iz, fy * -(v * iz), fy * (v - by)};
                        double px[3], py[3];
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            px[k] = fx * iz * (pose[k] - u * pose[6 + k]);
                            py[k] = fy * iz * (pose[3 + k] - v * pose[6 + k]);
                        }
                        int e = 0;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
#pragma unroll
                            for (int l = k; l < 3; ++l, ++e) {
                                V[e] = V[e] + px[k] * px[l];
                                V[e] = V[e] + py[k] * py[l];
                            }
                            g[k] = g[k] + px[k] * jx[6];
                            g[k] = g[k] + py[k] * jy[6];
                        }
                        ++nact;
                        if (fidx[c] >= 0) {
#pragma unroll
                            for (int r = 0; r < 7; ++r) {
                                o[kObsJx + r] = jx[r];
                                o[kObsJy + r] = jy[r];
                            }
#pragma unroll
                            for (int r = 0; r < 6; ++r)
#pragma unroll
                                for (int k = 0; k < 3; ++k) o[kObsW + 3 * r + k] = jx[r] * px[k] + jy[r] * py[k];
                        }
                    }
                }
                act[oi] = ex | (active ? kActive : 0);
            }
            // the damped V_i and its inverse by the adjugate: 00 01 02 11 12 22 = V[0..5]
            const double d0 = V[0] * damp, d1 = V[3] * damp, d2 = V[5] * damp;
            const double c00 = d1 * d2 - V[4] * V[4], c01 = V[2] * V[4] - V[1] * d2, c02 = V[1] * V[4] - V[2] * d1;
            const double c11 = d0 * d2 - V[2] * V[2], c12 = V[1] * V[2] - d0 * V[4], c22 = d0 * d1 - V[1] * V[1];
            const double det = d0 * c00 + V[1] * c01 + V[2] * c02;
            const bool elim = nact >= 2 && isfinite(det) && det > 1e-12 * (d0 * d1 * d2);
            const double I[6] = {c00 / det, c01 / det, c02 / det, c11 / det, c12 / det, c22 / det};
#pragma unroll
            for (int k = 0; k < 6; ++k) pt[kPtInv + k] = I[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) pt[kPtG + k] = g[k];
            if (elim) {
                const double Im[3][3] = {{I[0], I[1], I[2]}, {I[1], I[3], I[4]}, {I[2], I[4], I[5]}};
                for (int c = 0; c < C; ++c) {
                    const int64_t oi = static_cast<int64_t>(c) * ps + i;
                    if (!(act[oi] & kActive)) continue;
                    act[oi] |= kElim;
                    if (fidx[c] < 0) continue;
                    double *o = obs + oi * kBaObsDoubles;
#pragma unroll
                    for (int r = 0; r < 6; ++r) {
                        const double w0 = o[kObsW + 3 * r], w1 = o[kObsW + 3 * r + 1], w2 = o[kObsW + 3 * r + 2];
#pragma unroll
                        for (int k = 0; k < 3; ++k) o[kObsY + 3 * r + k] = w0 * Im[0][k] + w1 * Im[1][k] + w2 * Im[2][k];
                    }
                }
            }
        }
        __syncthreads();
        // ---- system pass: entry (ra, cb), ra <= cb <= R, of [S | rhs], row-major over the upper part
        const int nent = R * (R + 3) / 2;
        for (int ent = tid; ent < nent; ent += kBaThreads) {
            int ra = 0, rem = ent;
            while (rem >= R + 1 - ra) {
                rem -= R + 1 - ra;
                ++ra;
            }
            const int cb = ra + rem;
            const bool rhs = cb == R;
            const int c = freec[ra / 6], r = ra % 6;
            const int d = rhs ? c : freec[cb / 6], s = rhs ? 6 : cb % 6;
            const uint8_t *ac = act + static_cast<int64_t>(c) * ps, *ad = act + static_cast<int64_t>(d) * ps;
            const double *oc = obs + static_cast<int64_t>(c) * ps * kBaObsDoubles, *od = obs + static_cast<int64_t>(d) * ps * kBaObsDoubles;
            double u = 0.0, e = 0.0;
            for (int i = 0; i < n; ++i) {
                const uint8_t fc = ac[i];
                if (!(fc & kActive)) continue;
                const double *o = oc + static_cast<int64_t>(i) * kBaObsDoubles;
                if (c == d) {
                    u = u + o[kObsJx + r] * o[kObsJx + s];
                    u = u + o[kObsJy + r] * o[kObsJy + s];
                }
                if (!(fc & kElim) || !(ad[i] & kActive)) continue;
                const double *w = rhs ? pts + static_cast<int64_t>(i) * kBaPointDoubles + kPtG
                                      : od + static_cast<int64_t>(i) * kBaObsDoubles + kObsW + 3 * s;
                const double *y = o + kObsY + 3 * r;
                e = e + (y[0] * w[0] + y[1] * w[1] + y[2] * w[2]);
            }
            if (ra == cb) u = u * damp;
            const double v = u - e;
            A[ra * kBaCols + cb] = v;
            if (!rhs) A[cb * kBaCols + ra] = v;
        }
        if (tid <= R) perm[tid] = tid;
        if (tid == 0) {
            trial_ok = 1;  // the solve's verdict
            cand_ok = 1;   // every pose and point of the trial's state is finite
        }
        __syncthreads();
        // ---- elimination with complete pivoting
        bool ok = true;
        double p0 = 0.0;
        for (int k = 0; k < R; ++k) {
            const int w = R + 1 - k;
            double best = -1.0;
            int bi = 0;
            if (lane < w)
                for (int r = k + wv; r < R; r += kBaWaves) {
                    const double m = fabs(A[r * kBaCols + k + lane]);
                    if (m > best) {  // false for a NaN
                        best = m;
                        bi = (r - k) * w + lane;
                    }
                }
            // the largest magnitude, the lowest row-major index among equals: first over the wave, then over the waves
            const unsigned long long key = best >= 0.0 ? static_cast<unsigned long long>(__double_as_longlong(best)) + 1ull : 0ull;
            const uint32_t hi = wave_max_u32(static_cast<uint32_t>(key >> 32));
            const uint32_t lo = wave_max_u32(static_cast<uint32_t>(key >> 32) == hi ? static_cast<uint32_t>(key) : 0u);
            const unsigned long long top = (static_cast<unsigned long long>(hi) << 32) | lo;
            const uint32_t at = wave_min_u32(key == top ? static_cast<uint32_t>(bi) : 0xFFFFFFFFu);
            if (lane == 0) {
                wkey[wv] = top;
                widx[wv] = static_cast<int>(at);
            }
            __syncthreads();
            unsigned long long tk = 0ull;
            int ti = 0;
#pragma unroll
            for (int j = 0; j < kBaWaves; ++j) {
                const unsigned long long kj = wkey[j];
                const int ij = widx[j];
                if (kj > tk || (kj == tk && kj != 0ull && ij < ti)) {
                    tk = kj;
                    ti = ij;
                }
            }
            best = tk ? __longlong_as_double(static_cast<long long>(tk - 1ull)) : -1.0;
            const int pr = tk ? k + ti / w : k, pc = tk ? k + ti % w : k;
            if (k == 0) p0 = in_vgpr(best);
            ok = ok && best > 1e-12 * p0;
            if (tid < w && pr != k) {  // the columns left of k are never read again
                const double t = A[k * kBaCols + k + tid];
                A[k * kBaCols + k + tid] = A[pr * kBaCols + k + tid];
                A[pr * kBaCols + k + tid] = t;
            }
            __syncthreads();
            if (tid < R && pc != k) {
                const double t = A[tid * kBaCols + k];
                A[tid * kBaCols + k] = A[tid * kBaCols + pc];
                A[tid * kBaCols + pc] = t;
            }
            if (tid == 0) {
                const int t = perm[k];
                perm[k] = perm[pc];
                perm[pc] = t;
            }
            __syncthreads();
            if (tid > k && tid < R) fv[tid] = A[tid * kBaCols + k] / A[k * kBaCols + k];
            __syncthreads();
            if (lane < w - 1) {
                const int cc = k + 1 + lane;
                const double top_c = A[k * kBaCols + cc];
                for (int r = k + 1 + wv; r < R; r += kBaWaves) A[r * kBaCols + cc] = A[r * kBaCols + cc] - fv[r] * top_c;
            }
            __syncthreads();
        }
        // ---- back substitution from y[R] = 1 on one wave (R <= 48 lanes), the permutation undone, the step
        if (R > 0 && tid < kWave) {
            double s = 0.0;
            if (lane == 0) ys[R] = 1.0;
            wave_lds_sync();
            for (int cc = R; cc >= 1; --cc) {
                if (lane < cc) s = s + A[lane * kBaCols + cc] * ys[cc];
                if (lane == cc - 1) ys[cc - 1] = (0.0 - s) / A[lane * kBaCols + lane];
                wave_lds_sync();
            }
            if (lane <= R) xs[perm[lane]] = ys[lane];
            wave_lds_sync();
            const double xr = xs[R];
            double st = 0.0;
            bool fin = true;
            if (lane <= R) fin = isfinite(xs[lane]);
            if (lane < R) {
                st = xs[lane] / xr;
                fin = fin && isfinite(st);
            }
            wave_lds_sync();
            if (lane < R) xs[lane] = st;
            if (ballot(!fin) != 0ull || !ok) {
                if (lane == 0) trial_ok = 0;
            }
        }
        __syncthreads();
        // ---- the trial's state
        const int nxt = cur ^ 1;
        if (tid < C) {
            const double *pose = poses[cur][tid];
            double *cand = poses[nxt][tid];
            const int fa = fidx[tid];
            if (fa < 0 || !trial_ok) {
#pragma unroll
                for (int k = 0; k < 12; ++k) cand[k] = pose[k];
            } else {
                const double *x = xs + 6 * fa;
                const double h[3] = {x[0] / 2.0, x[1] / 2.0, x[2] / 2.0};
                const double hh = h[0] * h[0] + h[1] * h[1] + h[2] * h[2];
                const double fc = 2.0 / (1.0 + hh);
                const double K[9] = {0.0, -h[2], h[1], h[2], 0.0, -h[0], -h[1], h[0], 0.0};
                double Cm[9], Rm[9], Rn[9];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        Cm[3 * i + j] = (i == j ? 1.0 : 0.0) + fc * (K[3 * i + j] + (h[i] * h[j] - (i == j ? hh : 0.0)));
#pragma unroll
                for (int k = 0; k < 9; ++k) Rm[k] = pose[k];
                matmul3(Cm, Rm, Rn);
                bool fin = true;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    cand[k] = Rn[k];
                    fin = fin && isfinite(Rn[k]);
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double tn = dot3(Cm[3 * i], Cm[3 * i + 1], Cm[3 * i + 2], pose[9], pose[10], pose[11]) + x[3 + i];
                    cand[9 + i] = tn;
                    fin = fin && isfinite(tn);
                }
                if (!fin) atomicAnd(&cand_ok, 0);
            }
        }
        if (trial_ok) {
            bool fin = true;
            for (int i = tid; i < n; i += kBaThreads) {
                double *pt = pts + static_cast<int64_t>(i) * kBaPointDoubles;
                double X[3] = {pt[3 * cur], pt[3 * cur + 1], pt[3 * cur + 2]};
                bool elim = false;
                for (int c = 0; c < C && !elim; ++c) elim = (act[static_cast<int64_t>(c) * ps + i] & kElim) != 0;
                if (elim) {
                    double v[3] = {pt[kPtG], pt[kPtG + 1], pt[kPtG + 2]};
                    for (int fa = 0; fa < F; ++fa) {
                        const int64_t oi = static_cast<int64_t>(freec[fa]) * ps + i;
                        if (!(act[oi] & kActive)) continue;
                        const double *wm = obs + oi * kBaObsDoubles + kObsW;
#pragma unroll
                        for (int r = 0; r < 6; ++r) {
                            const double xr = xs[6 * fa + r];
#pragma unroll
                            for (int k = 0; k < 3; ++k) v[k] = v[k] + wm[3 * r + k] * xr;
                        }
                    }
                    const double *I = pt + kPtInv;
                    const double n0 = X[0] - (I[0] * v[0] + I[1] * v[1] + I[2] * v[2]);
                    const double n1 = X[1] - (I[1] * v[0] + I[3] * v[1] + I[4] * v[2]);
                    const double n2 = X[2] - (I[2] * v[0] + I[4] * v[1] + I[5] * v[2]);
                    X[0] = n0;
                    X[1] = n1;
                    X[2] = n2;
                    fin = fin && isfinite(n0) && isfinite(n1) && isfinite(n2);
                }
                pt[3 * nxt] = X[0];
                pt[3 * nxt + 1] = X[1];
                pt[3 * nxt + 2] = X[2];
            }
            if (!fin) atomicAnd(&cand_ok, 0);
        }
        __syncthreads();
        bool accept = false;
        if (trial_ok && cand_ok) {
            const double cost_n = state_cost<false>(q, poses[nxt], nxt, red, nullptr, 0, ones);
            accept = cost_n < cost;
            if (accept) cost = in_vgpr(cost_n);
        }
        if (accept) {
            cur = nxt;
            done = opaque(done + 1);
            lam = in_vgpr(lam * a.down);
        } else {
            lam = in_vgpr(lam * a.up);
        }
        __syncthreads();  // the flags and the workspace are rewritten by the next trial
    }

    // ---- the outputs, from the state in force
    uint8_t *oin = a.out_inlier ? a.out_inlier + static_cast<int64_t>(b) * C * a.o_stride : nullptr;
    state_cost<true>(q, poses[cur], cur, red, oin, a.o_stride, ones);
    const int count = wg_count(ones, &total);
    if (a.out_points) {
        const uint32_t *pbits = reinterpret_cast<const uint32_t *>(a.p_xyz) + static_cast<int64_t>(b) * ps * 3;
        uint32_t *obits = reinterpret_cast<uint32_t *>(a.out_points) + static_cast<int64_t>(b) * ps * 3;
        for (int i = tid; i < n; i += kBaThreads) {
            bool part = false;
            for (int c = 0; c < C; ++c) part = part || (act[static_cast<int64_t>(c) * ps + i] & kExists) != 0;
            const double *X = pts + static_cast<int64_t>(i) * kBaPointDoubles + 3 * cur;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint32_t given = pbits[3 * i + k];  // out_points may be p_xyz: read, then written, by this thread only
                obits[3 * i + k] = part ? __float_as_uint(static_cast<float>(X[k])) : given;
            }
        }
    }
    if (tid < C * 12) a.out_poses[static_cast<int64_t>(b) * C * 12 + tid] = poses[cur][tid / 12][tid % 12];
    if (tid != 0) return;
    if (a.out_counts) a.out_counts[b] = count;
    if (a.out_rounds) a.out_rounds[b] = done;
    if (a.out_cost) {
        a.out_cost[2 * b] = cost0;
        a.out_cost[2 * b + 1] = cost;
    }
}

}  // namespace

hipError_t launch_bundle_adjust(const BaArgs &a, hipStream_t s) {
    if (a.batch < 1 || a.cams < 1 || a.cams > FD_BA_MAX_CAMS || a.p_stride < 1 || a.o_stride < a.p_stride) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bundle_adjust, dim3(static_cast<unsigned>(a.batch)), dim3(kBaThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace fdk
