// Wave-level pieces of libstdc++'s std::sort (GCC 11, bits/stl_algo.h, bits/stl_heap.h) with comp =
// response greater (feature_point_detector.cpp:58-60), for the reference tie order (fd_select_ref.hip,
// fd_select_refw.hip): the median-of-three pivot, the introsort of a range of <= kRefWaveLocal elements
// by one wave, the final insertion sort of its leaves, and the depth-limit heapsort. Device functions on
// pointers (LDS or global memory).
#pragma once

#include "fd_device.h"

namespace fdk {

namespace {

constexpr int kRefMaxRanges = 256;  // unresolved ranges (> 16) in the list; bound: DESIGN.md
constexpr int kRefLeaf = 16;        // libstdc++ _S_threshold
// A range of <= kRefWaveLocal elements is partitioned to the end (its whole subtree) by one wave in LDS,
// with no workgroup barriers, in 12 B per element of the 96 KiB greedy span per wave (elements + stopper
// positions). A/B on the bench tie frames (profiles/r04_ref_wl_ab.txt): off / 64 / 128 / 256 / 512 = headline
// 52.3 / 51.3 / 50.1 / 48.4 / 52.5 us per call, north star 1.48 / 1.54 / 1.53 / 1.52 / 1.53 ms.
constexpr uint32_t kRefWaveLocal = 256;
constexpr int kRefStack = 64;  // pending subranges per wave (depth-first: <= 2 per level)

__device__ __forceinline__ float as_f(uint32_t u) { return __uint_as_float(u); }

// libstdc++ __move_median_to_first(result = lo, a = lo + 1, b = mid, c = hi - 1) with comp = resp
// greater: the position whose element becomes the pivot (swapped into lo).
__device__ __forceinline__ uint32_t median_pos(float ra, float rb, float rc, uint32_t a, uint32_t b, uint32_t c) {
    if (ra > rb) {
        if (rb > rc) return b;
        if (ra > rc) return c;
        return a;
    }
    if (ra > rc) return a;
    if (rb > rc) return c;
    return b;
}

// Position of the k-th set bit (0-based) of m; m must hold more than k bits.
__device__ __forceinline__ uint32_t select_bit(uint64_t m, uint32_t k) {
    uint32_t pos = 0;
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
        const uint32_t c = static_cast<uint32_t>(__popcll(m & ((1ull << step) - 1ull)));
        if (k >= c) {
            k -= c;
            m >>= step;
            pos += static_cast<uint32_t>(step);
        }
    }
    return pos;
}

// ---- std::__partial_sort(first, last, last): the introsort's depth-limit fallback ---------------------
// bits/stl_heap.h with comp = response greater (feature_point_detector.cpp:58-60): __adjust_heap sifts the
// hole down to a leaf along the child that comp does not order first, then __push_heap moves the value up
// while comp(parent, value). f is LDS or global memory (generic pointer).
__device__ __forceinline__ bool ref_gt(uint2 a, uint2 b) { return __uint_as_float(a.x) > __uint_as_float(b.x); }

__device__ void ref_adjust_heap(uint2 *f, int hole, int len, uint2 v) {
    const int top = hole;
    int second = hole;
    while (second < (len - 1) / 2) {
        second = 2 * (second + 1);
        if (ref_gt(f[second], f[second - 1])) --second;
        f[hole] = f[second];
        hole = second;
    }
    if ((len & 1) == 0 && second == (len - 2) / 2) {
        second = 2 * (second + 1);
        f[hole] = f[second - 1];
        hole = second - 1;
    }
    while (hole > top) {  // __push_heap(f, hole, top, v)
        const int parent = (hole - 1) / 2;
        const uint2 pv = f[parent];
        if (!ref_gt(pv, v)) break;
        f[hole] = pv;
        hole = parent;
    }
    f[hole] = v;
}

// One wave: __make_heap then __sort_heap on f[0, len). __make_heap adjusts parents (len - 2) / 2 down to 0;
// the parents of one tree level own disjoint subtrees and the deeper levels come first, so the lanes
// adjust a level's parents at once. __sort_heap's pops depend on each other: lane 0.
__device__ __forceinline__ void ref_heapsort(uint2 *f, int len) {
    if (len < 2) return;
    const int lane = lane_id();
    const int last_parent = (len - 2) / 2;
    for (int k = 31 - __clz(last_parent + 1); k >= 0; --k) {
        const int lo = (1 << k) - 1, hi = min((1 << (k + 1)) - 2, last_parent);
        for (int p = lo + lane; p <= hi; p += kWave) ref_adjust_heap(f, p, len, f[p]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (lane == 0)
        for (int l = len - 1; l >= 1; --l) {
            const uint2 v = f[l];
            f[l] = f[0];
            ref_adjust_heap(f, 0, l, v);
        }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wave, one element per lane: libstdc++'s introsort on a range of 17..64 elements (E[0, len), in
// LDS) to the end, every subrange of a level partitioned at once. Lane p keeps its subrange [sa, sb);
// stopper ranks are popcounts of the subrange's ballot, the k-th stopper's position a bit select, the
// exchanges and the pivot move shuffles. Leaves: stable rank by response, descending, into ordp.
// A subrange at the depth limit (std::__partial_sort) is written back to X (xp: X at E[0]'s position) and
// queued in hq (absolute [lo, hi) pairs, count *hn) for the heapsort step; its lanes take no further part.
__device__ bool ref_wave_small(uint2 *E, uint32_t len, uint32_t dep, uint32_t *ordp, uint2 *xp, uint32_t xlo,
                               uint32_t *hq, int *hn) {
    const uint32_t p = static_cast<uint32_t>(lane_id());
    uint2 v = p < len ? E[p] : make_uint2(0u, 0u);
    uint32_t sa = 0, sb = len, dp = dep;
    bool queued = false;
    for (int it = 0; it < 64; ++it) {
        bool big = p < len && !queued && sb - sa > static_cast<uint32_t>(kRefLeaf);
        if (ballot(big) == 0ull) break;
        if (ballot(big && dp == 0u) != 0ull) {
            const bool hp = big && dp == 0u;
            if (hp) xp[p] = v;
            if (hp && p == sa) {
                const int q = atomicAdd(hn, 1);
                if (q < kRefMaxRanges) {
                    hq[2 * q] = xlo + sa;
                    hq[2 * q + 1] = xlo + sb;
                }
            }
            queued = queued || hp;
            big = big && !hp;
            if (ballot(big) == 0ull) break;
        }
        // pivot: __move_median_to_first(sa, sa + 1, mid, sb - 1)
        const uint32_t mid = sa + (sb - sa) / 2u;
        const uint32_t i1 = min(sa + 1u, 63u), i2 = min(mid, 63u), i3 = sb >= 1u ? min(sb - 1u, 63u) : 0u;
        const float ra = __uint_as_float(static_cast<uint32_t>(__shfl(static_cast<int>(v.x), static_cast<int>(i1))));
        const float rb = __uint_as_float(static_cast<uint32_t>(__shfl(static_cast<int>(v.x), static_cast<int>(i2))));
        const float rc = __uint_as_float(static_cast<uint32_t>(__shfl(static_cast<int>(v.x), static_cast<int>(i3))));
        const uint32_t ch = median_pos(ra, rb, rc, sa + 1u, mid, sb - 1u);
        uint32_t src = p;
        if (big) src = p == sa ? ch : (p == ch ? sa : p);
        v.x = static_cast<uint32_t>(__shfl(static_cast<int>(v.x), static_cast<int>(min(src, 63u))));
        v.y = static_cast<uint32_t>(__shfl(static_cast<int>(v.y), static_cast<int>(min(src, 63u))));
        const float pv = __uint_as_float(static_cast<uint32_t>(__shfl(static_cast<int>(v.x), static_cast<int>(min(sa, 63u)))));
        // stoppers of (sa, sb)
        const bool in = big && p > sa && p < sb;
        const float rv = __uint_as_float(v.x);
        const uint64_t BL = ballot(in && rv <= pv), BR = ballot(in && rv >= pv);
        const uint64_t hiMask = sb >= 64u ? ~0ull : ((1ull << sb) - 1ull);
        const uint64_t seg = hiMask & ~((2ull << min(sa, 62u)) - 1ull);  // bits (sa, sb)
        const uint64_t bl = BL & seg, br = BR & seg;
        const uint32_t nL = static_cast<uint32_t>(__popcll(bl)), nR = static_cast<uint32_t>(__popcll(br));
        // pair k = p - (sa + 1): t_k = l_k < r_k (r_k: the k-th right stopper from the right)
        const uint32_t k = p - (sa + 1u);
        const uint32_t mn = min(nL, nR);
        const bool tk = in && k < mn && select_bit(bl, k) < select_bit(br, nR - 1u - k);
        const uint64_t T = ballot(tk) & seg;
        const uint32_t K = static_cast<uint32_t>(__builtin_ctzll(~(T >> min(sa + 1u, 63u))));
        // exchanges
        const uint64_t below = (1ull << p) - 1ull;
        const uint64_t above = p >= 63u ? 0ull : ~((2ull << p) - 1ull);
        const uint32_t rankL = static_cast<uint32_t>(__popcll(bl & below));
        const uint32_t rankR = static_cast<uint32_t>(__popcll(br & above));
        const bool isL = ((bl >> p) & 1ull) != 0ull, isR = ((br >> p) & 1ull) != 0ull;
        uint32_t s2 = p;
        if (isL && rankL < K) s2 = select_bit(br, nR - 1u - rankL);
        else if (isR && rankR < K) s2 = select_bit(bl, rankR);
        v.x = static_cast<uint32_t>(__shfl(static_cast<int>(v.x), static_cast<int>(s2)));
        v.y = static_cast<uint32_t>(__shfl(static_cast<int>(v.y), static_cast<int>(s2)));
        if (big) {
            uint32_t cut = 0xFFFFFFFFu;
            if (K < nL) cut = select_bit(bl, K);
            if (K >= 1u) cut = min(cut, select_bit(br, nR - K));
            if (p < cut) sb = cut;
            else sa = cut;
            --dp;
        }
    }
    // leaves: stable rank within [sa, sb)
    const float ri = __uint_as_float(v.x);
    uint32_t rk = 0;
#pragma unroll
    for (int j = 0; j < kRefLeaf; ++j) {
        const uint32_t t = sa + static_cast<uint32_t>(j);
        const float rt = __uint_as_float(static_cast<uint32_t>(__shfl(static_cast<int>(v.x), static_cast<int>(min(t, 63u)))));
        rk += (t < sb && (rt > ri || (rt == ri && t < p))) ? 1u : 0u;
    }
    if (p < len && !queued) ordp[sa + rk] = v.y;
    return true;
}

// One wave: libstdc++'s introsort on X[lo, hi) (<= kRefWaveLocal elements, > kRefLeaf) to the end -- the
// same partitions as the workgroup levels (median of (first + 1, mid, last - 1) moved to first, left
// stoppers resp <= pivot from the left paired with right stoppers resp >= pivot from the right while
// l_k < r_k, cut = min(l_K, r_{K-1})), then the final insertion sort of every leaf (stable, response
// descending) -- with the elements in the wave's LDS. Writes the range's visiting order into ord[lo, hi).
// A subrange at the depth limit is queued for the heapsort step (hq, hn). Returns false on a broken invariant.
__device__ __forceinline__ bool ref_wave_resolve(uint2 *X, uint32_t *ord, uint32_t lo, uint32_t hi, uint32_t dep, uint2 *E,
                                 uint16_t *Lp, uint16_t *Rp, uint32_t *stk, uint32_t *hq, int *hn) {
    const int lane = lane_id();
    const uint32_t s = hi - lo;
    for (uint32_t i = lane; i < s; i += kWave) E[i] = X[lo + i];
    // stack entries: a (10 bits) | b (11 bits) << 10 | depth left << 21, positions relative to lo
    int top = 0;
    if (lane == 0) stk[0] = 0u | (s << 10) | (dep << 21);
    top = 1;
    bool ok = true;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    while (top > 0) {
        --top;
        const uint32_t ent = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(stk[top])));
        const uint32_t a = ent & 1023u, b = (ent >> 10) & 2047u, dp = ent >> 21;
        if (b - a <= static_cast<uint32_t>(kWave) && b - a > static_cast<uint32_t>(kRefLeaf)) {
            if (!ref_wave_small(E + a, b - a, dp, ord + lo + a, X + lo + a, lo + a, hq, hn)) {
                ok = false;
                break;
            }
            continue;
        }
        if (b - a <= static_cast<uint32_t>(kRefLeaf)) {
            // leaf: stable rank by response, descending (lanes 0-15)
            const int len = static_cast<int>(b - a);
            const int q = lane & (kRefLeaf - 1);
            const uint2 v = q < len ? E[a + q] : make_uint2(0u, 0u);
            const float ri = __uint_as_float(v.x);
            uint32_t rk = 0;
#pragma unroll
            for (int t = 0; t < kRefLeaf; ++t) {
                const float rt = __uint_as_float(static_cast<uint32_t>(__shfl(static_cast<int>(v.x), t)));
                rk += (t < len && (rt > ri || (rt == ri && t < q))) ? 1u : 0u;
            }
            if (lane < kRefLeaf && q < len) ord[lo + a + rk] = v.y;
            continue;
        }
        if (dp == 0u) {  // std::__partial_sort(a, b, b): back to X and queued for the heapsort step
            for (uint32_t i = lane; i < b - a; i += kWave) X[lo + a + i] = E[a + i];
            if (lane == 0) {
                const int q = atomicAdd(hn, 1);
                if (q < kRefMaxRanges) {
                    hq[2 * q] = lo + a;
                    hq[2 * q + 1] = lo + b;
                }
            }
            continue;
        }
        // pivot: __move_median_to_first(a, a + 1, mid, b - 1)
        const uint32_t mid = a + (b - a) / 2u;
        const uint2 xa = E[a + 1], xb = E[mid], xc = E[b - 1];
        const uint32_t ch = median_pos(__uint_as_float(xa.x), __uint_as_float(xb.x), __uint_as_float(xc.x), a + 1, mid, b - 1);
        const uint2 xp = ch == a + 1 ? xa : (ch == mid ? xb : xc);
        const uint2 x0 = E[a];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane == 0) {
            E[a] = xp;
            E[ch] = x0;
        }
        const float pv = __uint_as_float(xp.x);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // stoppers of [a + 1, b): left ones by rank from the left, right ones by rank from the left (reversed below)
        uint32_t nL = 0, nR = 0;
        for (uint32_t i0 = a + 1; i0 < b; i0 += kWave) {
            const uint32_t i = i0 + lane;
            const bool in = i < b;
            const float rv = in ? __uint_as_float(E[i].x) : 0.0f;
            const bool ls = in && rv <= pv, rs = in && rv >= pv;
            const uint64_t bl = ballot(ls), br = ballot(rs);
            if (ls) Lp[nL + mbcnt64(bl, 0)] = static_cast<uint16_t>(i);
            if (rs) Rp[nR + mbcnt64(br, 0)] = static_cast<uint16_t>(i);
            nL += popc64(bl);
            nR += popc64(br);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // K: pairs k with l_k < r_k (r_k = the k-th right stopper from the right), monotone in k
        const uint32_t mn = min(nL, nR);
        uint32_t K = 0;
        for (uint32_t k0 = 0; k0 < mn; k0 += kWave) {
            const uint32_t k = k0 + lane;
            const bool t = k < mn && Lp[k] < Rp[nR - 1u - min(k, nR - 1u)];
            const uint64_t bt = ballot(t);
            const uint32_t run = bt == ~0ull ? 64u : static_cast<uint32_t>(__builtin_ctzll(~bt));
            K += run;
            if (run < 64u) break;
        }
        // the swaps (pairs are disjoint)
        for (uint32_t k0 = 0; k0 < K; k0 += kWave) {
            const uint32_t k = k0 + lane;
            if (k < K) {
                const uint32_t pl = Lp[k], pr = Rp[nR - 1u - k];
                const uint2 vl = E[pl], vr = E[pr];
                E[pl] = vr;
                E[pr] = vl;
            }
        }
        uint32_t cut = 0xFFFFFFFFu;
        if (K < nL) cut = Lp[K];
        if (K >= 1u) cut = min(cut, static_cast<uint32_t>(Rp[nR - K]));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (cut <= a || cut >= b || top + 2 > kRefStack) {  // (cannot happen: the scans stop inside the range)
            ok = false;
            break;
        }
        // children, left one on top (depth-first; the order of resolution does not matter)
        if (lane == 0) {
            stk[top] = cut | (b << 10) | ((dp - 1u) << 21);
            stk[top + 1] = a | (cut << 10) | ((dp - 1u) << 21);
        }
        top += 2;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    return ok;
}

}  // namespace

}  // namespace fdk
