// Device code shared by the geometry stages (fd_ransac.hip: fd_ransac, fd_ransac_refit, fd_pose_recover;
// fd_pnp.hip: fd_pnp_ransac, fd_pnp_refit): the counter-based sampler, the null vector of an R x (R + 1)
// system by Gaussian elimination with complete pivoting, the cyclic Jacobi on one wave, and the small
// products and counts around them. Every floating point operation is a double one, rounded once (the build
// passes -ffp-contract=off), in the order include/fd_hip.h states. This file is the maths; the skeleton of an
// estimator around it (compaction, score and vote, finish walk, refit frame, slice tree) is fd_estimate.h.
#pragma once

#include "fd_hip.h"
#include "fd_window.h"

namespace fdk {

constexpr int kRansacThreads = 256;  // the per-frame kernels of both files
constexpr int kTile = 256;           // correspondences per LDS tile of a scoring loop

__device__ __forceinline__ uint32_t mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// The M distinct picks of hypothesis h of frame f among n correspondences; false when there are fewer
// than M or a pick found no new index in 32 tries.
template <int M>
__device__ __forceinline__ bool sample(uint32_t seed, int f, int h, int n, int (&pick)[M]) {
#pragma unroll
    for (int k = 0; k < M; ++k) pick[k] = 0;
    if (n < M) return false;
    const uint32_t base = mix(mix(seed + 0x9E3779B9u * static_cast<uint32_t>(f)) + static_cast<uint32_t>(h));
    bool ok = true;
#pragma unroll
    for (int k = 0; k < M; ++k) {
        bool found = false;
        for (int a = 0; a < 32 && !found && ok; ++a) {
            const int idx = static_cast<int>(__umulhi(mix(base + 32u * k + a), static_cast<uint32_t>(n)));
            bool dup = false;
#pragma unroll
            for (int j = 0; j < k; ++j) dup |= pick[j] == idx;
            if (!dup) {
                pick[k] = idx;
                found = true;
            }
        }
        ok = ok && found;
    }
    return ok;
}

// Element (r, c) of a ROWS x (ROWS + 1) system whose elements lie STRIDE doubles apart: a lane's column of
// an [element][lane] array (STRIDE = kWave, A pointing at the lane's first element), or a plain row-major
// array (STRIDE = 1).
template <int ROWS, int STRIDE>
__device__ __forceinline__ double &el(double *A, int r, int c) {
    return A[((ROWS + 1) * r + c) * STRIDE];
}

// Null vector of the system by Gaussian elimination with complete pivoting, into x (x[ROWS] = 1 before the
// column permutation is undone); false for a pivot that fails the relative test or a non-finite result.
// Destroys the system. ROWS <= 15: the permutation is held in nibbles.
template <int ROWS, int STRIDE>
__device__ __forceinline__ bool null_vector(double *A, double (&x)[ROWS + 1]) {
    constexpr int COLS = ROWS + 1;
    static_assert(COLS <= 16, "one nibble per column");
    uint64_t perm = 0xFEDCBA9876543210ull & (~0ull >> (4 * (16 - COLS)));  // nibble c: the original column now at position c
    bool ok = true;
    double p0 = 0.0;
#pragma nounroll
    for (int k = 0; k < ROWS; ++k) {
        double best = -1.0;
        int pr = k, pc = k;
        for (int r = k; r < ROWS; ++r)
            for (int c = k; c < COLS; ++c) {
                const double m = fabs(el<ROWS, STRIDE>(A, r, c));
                if (m > best) {  // false for a NaN
                    best = m;
                    pr = r;
                    pc = c;
                }
            }
        if (k == 0) p0 = best;
        ok = ok && best > 1e-12 * p0;
        for (int c = k; c < COLS; ++c) {  // the columns left of k are never read again
            const double t = el<ROWS, STRIDE>(A, k, c);
            el<ROWS, STRIDE>(A, k, c) = el<ROWS, STRIDE>(A, pr, c);
            el<ROWS, STRIDE>(A, pr, c) = t;
        }
        for (int r = 0; r < ROWS; ++r) {
            const double t = el<ROWS, STRIDE>(A, r, k);
            el<ROWS, STRIDE>(A, r, k) = el<ROWS, STRIDE>(A, r, pc);
            el<ROWS, STRIDE>(A, r, pc) = t;
        }
        const uint64_t nk = (perm >> (4 * k)) & 15u, nc = (perm >> (4 * pc)) & 15u;
        perm = (perm & ~(15ull << (4 * k))) | (nc << (4 * k));
        perm = (perm & ~(15ull << (4 * pc))) | (nk << (4 * pc));
        const double piv = el<ROWS, STRIDE>(A, k, k);
        for (int r = k + 1; r < ROWS; ++r) {
            const double f = el<ROWS, STRIDE>(A, r, k) / piv;
            for (int c = k + 1; c < COLS; ++c)
                el<ROWS, STRIDE>(A, r, c) = el<ROWS, STRIDE>(A, r, c) - f * el<ROWS, STRIDE>(A, k, c);
        }
    }
    double y[COLS];
    y[ROWS] = 1.0;
#pragma unroll
    for (int k = ROWS - 1; k >= 0; --k) {
        double s = 0.0;
#pragma unroll
        for (int c = k + 1; c < COLS; ++c) s = s + el<ROWS, STRIDE>(A, k, c) * y[c];
        y[k] = (0.0 - s) / el<ROWS, STRIDE>(A, k, k);
    }
    // undo the column permutation through the (now free) first elements of the system
#pragma unroll
    for (int c = 0; c < COLS; ++c) A[static_cast<int>((perm >> (4 * c)) & 15u) * STRIDE] = y[c];
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
        x[c] = A[c * STRIDE];
        ok = ok && isfinite(x[c]);
    }
    return ok;
}

// out = a * b, 3 x 3 row-major, every sum from 0.0 with the inner index ascending.
__device__ __forceinline__ void matmul3(const double (&a)[9], const double (&b)[9], double (&out)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc = acc + a[3 * i + k] * b[3 * k + j];
            out[3 * i + j] = acc;
        }
}

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
    return a0 * b0 + a1 * b1 + a2 * b2;
}

// The workgroup's sum of one count per thread.
__device__ __forceinline__ int wg_count(uint32_t mine, int *total) {
    __syncthreads();
    if (threadIdx.x == 0) *total = 0;
    __syncthreads();
    const uint32_t wave_n = wave_total_add(mine);
    if (lane_id() == 0 && wave_n) atomicAdd(total, static_cast<int>(wave_n));
    __syncthreads();
    return *total;
}

// Cyclic Jacobi of the contract on one wave. m holds 2 N rows of N doubles in LDS: the symmetric matrix, then
// V. Lane r < 2 N owns row r: every element update of a rotation is an expression of the values before it,
// so the lanes read their two elements, then write them (the matrix rows mirrored into the columns), and the
// result is the serial restatement's bit for bit. The dependent chain of a rotation (two divisions, two square
// roots) is computed by every lane alike; p, q and the skip are wave-uniform.
template <int N, int SWEEPS>
__device__ __forceinline__ void jacobi(double *m, int lane) {
    const bool live = lane < 2 * N, sym = lane < N;
    const int r = live ? lane : 0;
    for (int sweep = 0; sweep < SWEEPS; ++sweep)
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                const double apq = m[p * N + q];
                if (apq == 0.0) continue;
                const double app = m[p * N + p], aqq = m[q * N + q];
                const double xp = m[r * N + p], xq = m[r * N + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0);
                const double s = t * c;
                double np = c * xp - s * xq, nq = s * xp + c * xq;
                if (sym && r == p) {
                    np = app - t * apq;
                    nq = 0.0;
                }
                if (sym && r == q) {
                    np = 0.0;
                    nq = aqq + t * apq;
                }
                wave_lds_sync();
                if (live) {
                    m[r * N + p] = np;
                    m[r * N + q] = nq;
                }
                if (sym) {
                    m[p * N + r] = np;
                    m[q * N + r] = nq;
                }
                wave_lds_sync();
            }
}

// Index of the smallest of d: a strict < from entry 0.
template <int N>
__device__ __forceinline__ int smallest(const double (&d)[N]) {
    int at = 0;
    double best = d[0];
#pragma unroll
    for (int i = 1; i < N; ++i)
        if (d[i] < best) {
            best = d[i];
            at = i;
        }
    return at;
}

}  // namespace fdk
