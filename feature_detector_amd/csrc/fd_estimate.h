// The skeleton around the maths of fd_solve.h that the estimators share (fd_ransac.hip over 32-byte
// correspondences d4, fd_pnp.hip over 40-byte ones Corr5, fd_align.hip over 48-byte ones Corr6): the compaction of a frame's slots into its ordered
// list, the broadcast-tile score of a hypothesis, the vote for the frame's best and its decoding, the finish
// walk, the frame of a refit (members by list position in a double buffer, reclassified every round), the slice
// tree of the refits' sums, and M^T M beside the identity for the 3 x 3 Jacobi. A new estimator supplies its
// correspondence type, how a slot is loaded and conditioned, and its inlier test, as functors.
//
// `A` is a kernel's argument block (RansacArgs, PnpArgs, AlignArgs): the helpers read the fields all have under one
// name (q_counts, match_idx, pair_valid, q_stride, t_stride, corr, cidx, n, best, out_inlier). No helper holds a
// floating point operation of its own but reduce_upper, reduce_sums and gram3_identity, whose sums keep the
// contract's order.
#pragma once

#include "fd_solve.h"

namespace fdk {

constexpr int kSlice = 9;  // entries of a refit's sums through the LDS tree at a time: 9 * 256 * 8 B = 18 KiB

// k_*_compact, one workgroup per frame: the frame's taken slots in slot order into its list, every slot's index
// in it (or -1), the list's length, and the frame's vote word zeroed. A slot is a candidate when its pair_valid
// byte is 1 and its partner j lies in the train array; load(i, j, p) then fills p from slot i and partner j and
// says whether the slot is taken. wsum: LDS [kRansacThreads / kWave].
template <class Corr, class A, class Load>
__device__ __forceinline__ void compact_slots(const A &a, uint32_t *wsum, Load load) {
    const int f = static_cast<int>(blockIdx.x), tid = static_cast<int>(threadIdx.x);
    const int nf = frame_count(a.q_counts, f, a.q_stride);
    const int64_t s0 = static_cast<int64_t>(f) * a.q_stride;
    Corr *corr = reinterpret_cast<Corr *>(a.corr) + s0;
    uint32_t base = 0;
    for (int i0 = 0; i0 < nf; i0 += kRansacThreads) {
        const int i = i0 + tid;
        bool take = false;
        Corr p = {};
        if (i < nf) {
            take = !a.pair_valid || a.pair_valid[s0 + i] == 1;
            const int j = a.match_idx ? a.match_idx[s0 + i] : i;
            take = take && j >= 0 && j < a.t_stride;
            if (take) take = load(s0 + i, static_cast<int64_t>(f) * a.t_stride + j, p);
        }
        uint32_t tot;
        const uint32_t pos = base + wg_excl_add<kRansacThreads>(take ? 1u : 0u, wsum, tot);
        if (take) corr[pos] = p;  // pos < nf <= q_stride
        if (i < nf) a.cidx[s0 + i] = take ? static_cast<int32_t>(pos) : -1;
        base += tot;
    }
    if (tid == 0) {
        a.n[f] = static_cast<int32_t>(base);
        a.best[f] = 0ull;
    }
}

// The hypothesis kernels' frame and hypothesis of this lane: one wave per workgroup, a lane per hypothesis.
__device__ __forceinline__ void hypothesis_index(int hypotheses, int &f, int &h) {
    const int groups = (hypotheses + kWave - 1) / kWave;
    f = static_cast<int>(blockIdx.x) / groups;
    h = (static_cast<int>(blockIdx.x) - f * groups) * kWave + lane_id();
}

// The inliers of this lane's model among the frame's n correspondences: they pass through an LDS tile that every
// lane reads at the same address (a broadcast). n is the frame's: uniform over the one-wave workgroup.
template <class Corr, class Pred>
__device__ __forceinline__ int count_inliers(const Corr *corr, int n, Corr *tile, Pred pred) {
    int count = 0;
    for (int base = 0; base < n; base += kTile) {
        const int m = min(kTile, n - base);
        __syncthreads();
        for (int j = lane_id(); j < m; j += kWave) tile[j] = corr[base + j];
        __syncthreads();
        for (int j = 0; j < m; ++j) count += pred(tile[j]) ? 1 : 0;
    }
    return count;
}

// Hypothesis h of frame f among the frame's models of N doubles each.
template <int N>
__device__ __forceinline__ double *model_at(double *models, int f, int hypotheses, int h) {
    return models + (static_cast<int64_t>(f) * hypotheses + h) * N;
}

// The wave's best (count, lowest index) into the frame's 64-bit word in one atomicMax: count + 1 in the high
// half, so that a valid hypothesis with no inlier still beats "none" (0), and 0xFFFFFFFF - h in the low one.
__device__ __forceinline__ void vote_best(bool ok, int count, int h, unsigned long long *best) {
    const uint32_t hi = ok ? static_cast<uint32_t>(count) + 1u : 0u;
    const uint32_t top = wave_max_u32(hi);
    const uint32_t lo = wave_max_u32(hi == top ? 0xFFFFFFFFu - static_cast<uint32_t>(h) : 0u);
    if (lane_id() == 0 && top) atomicMax(best, (static_cast<unsigned long long>(top) << 32) | lo);
}

// The frame's winner from its word: whether there is one, its index h (-1) and its model x (zeros).
template <int N, class A>
__device__ __forceinline__ bool winner(const A &a, int f, int &h, double (&x)[N]) {
    const unsigned long long key = a.best[f];
    const bool has = key != 0ull;
    h = has ? static_cast<int>(0xFFFFFFFFu - static_cast<uint32_t>(key)) : -1;
#pragma unroll
    for (int c = 0; c < N; ++c) x[c] = has ? model_at<N>(a.models, f, a.hypotheses, h)[c] : 0.0;
    return has;
}

// The finish walk of a frame's nf slots: a slot is an inlier when the frame has a model, the slot is in the list
// and pred says so of its correspondence. Writes out_inlier and returns the frame's count (wg_count's barriers).
template <class Corr, class A, class Pred>
__device__ __forceinline__ int classify_slots(const A &a, int f, int nf, bool has, int *total, Pred pred) {
    const int64_t s0 = static_cast<int64_t>(f) * a.q_stride;
    const Corr *corr = reinterpret_cast<const Corr *>(a.corr) + s0;
    uint32_t mine = 0;
    for (int i = static_cast<int>(threadIdx.x); i < nf; i += kRansacThreads) {
        bool in = false;
        if (has) {
            const int ci = a.cidx[s0 + i];
            if (ci >= 0) in = pred(corr[ci]);
        }
        if (a.out_inlier) a.out_inlier[s0 + i] = in ? 1 : 0;
        mine += in ? 1u : 0u;
    }
    return wg_count(mine, total);
}

// ---- the frame of a refit: one workgroup per frame, every round inside one launch -------------------------------
// The support set lives in global memory by list position, [2][q_stride] bytes per frame: the current one and the
// round's candidate. Thread t reads and writes the positions i = t (mod 256) only.
struct Support {
    uint8_t *mem;
    int stride;
    int count;              // of the current set (the estimator's own start value)
    int cur = 0, done = 0;  // the current half; accepted rounds
    __device__ __forceinline__ const uint8_t *current() const { return mem + cur * stride; }
    __device__ __forceinline__ uint8_t *candidate() const { return mem + (cur ^ 1) * stride; }
    // A round whose candidate has c members: taken unless they are fewer. Uniform over the workgroup.
    __device__ __forceinline__ bool accept(int c) {
        if (c < count) return false;
        count = c;
        cur ^= 1;
        ++done;
        return true;
    }
};

// The given members into half 0 of mem: only an in_inlier byte equal to 1 is one. Ends with a barrier.
template <class A>
__device__ __forceinline__ void load_members(const A &a, int f, int nf, const uint8_t *in_inlier, uint8_t *mem) {
    const int64_t s0 = static_cast<int64_t>(f) * a.q_stride;
    for (int s = static_cast<int>(threadIdx.x); s < nf; s += kRansacThreads) {
        const int ci = a.cidx[s0 + s];
        if (ci >= 0) mem[ci] = in_inlier[s0 + s] == 1 ? 1 : 0;  // ci < n <= q_stride
    }
    __syncthreads();
}

// Every correspondence of the list classified by pred into the candidate set S2; the workgroup's count.
template <class Corr, class Pred>
__device__ __forceinline__ int reclassify(const Corr *corr, int n, uint8_t *S2, int *total, Pred pred) {
    uint32_t mine = 0;
    for (int i = static_cast<int>(threadIdx.x); i < n; i += kRansacThreads) {
        const bool in = pred(corr[i]);
        S2[i] = in ? 1 : 0;
        mine += in ? 1u : 0u;
    }
    return wg_count(mine, total);
}

// out_inlier of the frame's slots from the members S, after a barrier for the members other threads wrote.
template <class A>
__device__ __forceinline__ void write_members(const A &a, int f, int nf, const uint8_t *S) {
    const int64_t s0 = static_cast<int64_t>(f) * a.q_stride;
    __syncthreads();
    if (a.out_inlier)
        for (int s = static_cast<int>(threadIdx.x); s < nf; s += kRansacThreads) {
            const int ci = a.cidx[s0 + s];
            a.out_inlier[s0 + s] = ci >= 0 ? S[ci] : 0;
        }
}

// N doubles' bits as they are, all read before the first is written (dst may be src).
template <int N>
__device__ __forceinline__ void copy_bits(const double *src, double *dst) {
    unsigned long long w[N];
#pragma unroll
    for (int c = 0; c < N; ++c) w[c] = reinterpret_cast<const unsigned long long *>(src)[c];
#pragma unroll
    for (int c = 0; c < N; ++c) reinterpret_cast<unsigned long long *>(dst)[c] = w[c];
}

// The workgroup's sums of ENTRIES register partials per thread (thread t's are the contract's partial t), through
// an LDS tree in slices of kSlice, unpacked as the row-major upper part of a system of rows N long into sys and
// mirrored below the diagonal; MIRROR_LAST: the last column too (a square matrix; without it column N - 1 is a
// right-hand side). red: LDS [kSlice * kRansacThreads]. Ends with a barrier.
template <int ENTRIES, int N, bool MIRROR_LAST>
__device__ __forceinline__ void reduce_upper(const double (&acc)[ENTRIES], double *red, double *sys) {
    static_assert(ENTRIES % kSlice == 0, "whole slices");
    const int tid = static_cast<int>(threadIdx.x);
#pragma unroll
    for (int sl = 0; sl < ENTRIES / kSlice; ++sl) {
#pragma unroll
        for (int j = 0; j < kSlice; ++j) red[j * kRansacThreads + tid] = acc[sl * kSlice + j];
        for (int step = kRansacThreads / 2; step >= 1; step >>= 1) {
            __syncthreads();
            if (tid < step) {
#pragma unroll
                for (int j = 0; j < kSlice; ++j)
                    red[j * kRansacThreads + tid] = red[j * kRansacThreads + tid] + red[j * kRansacThreads + tid + step];
            }
        }
        __syncthreads();
        if (tid < kSlice) {
            int i = 0, rem = sl * kSlice + tid;  // entry (i, j) of the row-major upper part
            while (rem >= N - i) {
                rem -= N - i;
                ++i;
            }
            const int j = i + rem;
            const double v = red[tid * kRansacThreads];
            sys[i * N + j] = v;
            if (MIRROR_LAST || j < N - 1) sys[j * N + i] = v;
        }
        __syncthreads();
    }
}

// The same tree for ENTRIES plain sums at once (ENTRIES <= 10: 20 KiB), left in out[0..ENTRIES) for every thread to
// read. red: LDS [ENTRIES * kRansacThreads]. Ends with a barrier.
template <int ENTRIES>
__device__ __forceinline__ void reduce_sums(const double (&acc)[ENTRIES], double *red, double *out) {
    const int tid = static_cast<int>(threadIdx.x);
#pragma unroll
    for (int j = 0; j < ENTRIES; ++j) red[j * kRansacThreads + tid] = acc[j];
    for (int step = kRansacThreads / 2; step >= 1; step >>= 1) {
        __syncthreads();
        if (tid < step) {
#pragma unroll
            for (int j = 0; j < ENTRIES; ++j)
                red[j * kRansacThreads + tid] = red[j * kRansacThreads + tid] + red[j * kRansacThreads + tid + step];
        }
    }
    __syncthreads();
    if (tid < ENTRIES) out[tid] = red[tid * kRansacThreads];
    __syncthreads();
}

// G = M^T M of the 3 x 3 matrix in the first three columns of M's rows (LD doubles apart), each sum from 0.0
// with the row index ascending, and the identity behind it: jacobi<3>'s input, by one thread.
template <int LD, int N>
__device__ __forceinline__ void gram3_identity(const double (&M)[N], double *mat3) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s = s + M[LD * k + i] * M[LD * k + j];
            mat3[3 * i + j] = s;
            mat3[9 + 3 * i + j] = i == j ? 1.0 : 0.0;
        }
}

}  // namespace fdk
