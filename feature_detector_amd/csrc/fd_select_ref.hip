// K4d k_select_reference: the reference tie order (FD_TIES_REFERENCE) on the GPU, graph-capturable.
//
// SelectGoodFeatures sorts its raster-ordered candidates with an unstable std::sort
// (feature_point_detector.cpp:58-60); among equal responses the visiting order is whatever libstdc++'s
// introsort leaves. k_select visits equal responses by raster index and flags every frame whose scanned
// prefix meets a tie (FD_FRAME_TIES); this kernel re-selects exactly those frames in libstdc++'s order.
//
// libstdc++ (GCC 11, bits/stl_algo.h) std::sort = __introsort_loop(first, last, 2 * __lg(n)) then
// __final_insertion_sort. The loop partitions a range of more than 16 elements around the median of
// (first + 1, mid, last - 1) moved to `first` (__move_median_to_first), by __unguarded_partition over
// [first + 1, last): a left scan stops at elements e with !(e > pivot) ("left stoppers", LS: resp <=
// pivot), a right scan at !(pivot > e) ("right stoppers", RS: resp >= pivot), and the k-th left stopper
// from the left swaps with the k-th right stopper from the right while l_k < r_k. With K such swaps the
// cut is min(l_{K+1}, r_K) (the left scan's last stop: the next original left stopper, or at the latest
// r_K, which now holds a left stopper). Both halves recurse with depth - 1; the loop leaves ranges of <=
// 16 elements, which the final insertion sort orders stably and never crosses (every element right of a
// cut is <= every element left of it). So the final order of any prefix follows from partitions of the
// ranges that overlap it alone: ranks of the stoppers come from prefix counts (ballots), the pairing is
// a scatter of stopper positions by rank, and K per range is where l_k < r_k stops holding (monotone).
//
// One 1024-thread workgroup per flagged frame:
//   1. the frame's candidates in push order: raster order for the built-in detectors (a bitmap of the
//      candidate pixels and its word prefix ranks the unordered list), the list order as given for
//      caller lists (fd_points_select);
//   2. windows of kSelectChunk positions from the front: every range overlapping the window is
//      partitioned, level by level, all of a level's ranges at once (flat index space over their
//      partition spans, one block of it per wave), until only leaves (<= 16) cover the window; leaves
//      are insertion-sorted by 16 lanes each into the visiting order; before the first greedy scan,
//      children of <= kRefWaveLocal elements leave the levels and are sorted to the end by one wave
//      each in LDS (ref_wave_resolve), which saves the last levels' barriers;
//   3. the ordered greedy (ordered_chunk) over the new positions (one wave, occupancy grid); stop at
//      `need`, else the next window (ranges right of the window wait in the range list).
// A range that reaches the depth limit takes libstdc++'s fallback, std::__partial_sort(first, last, last)
// = __make_heap + __sort_heap, emulated exactly by one wave (ref_heapsort: the heap built level by level,
// the subtrees of one level being disjoint, then the pops by one lane), in LDS when the range fits there;
// its visiting order is then final. FD_FRAME_UNRESOLVED is left only for a broken internal invariant
// (range guards), in which case the frame keeps k_select's raster-order features; on host-output calls
// the host then sorts the frame with std::sort itself and k_select_ordered (below) scans that order.
//
// The wave-level sort pieces are in fd_ref_sort.h, the multi-workgroup prelude for large frames in
// fd_select_refw.hip, the greedy in fd_greedy.h.
#include "fd_greedy.h"
#include "fd_ref_sort.h"

namespace fdk {

namespace {

constexpr int kRefThreads = 1024;
constexpr int kRefWaves = kRefThreads / kWave;
constexpr int kRefU = 4;            // 64-element rounds per wave whose global loads are issued together
constexpr uint32_t kRefRidCap = 8192;  // flat elements per level whose range index pass 1 caches for passes 2-3
constexpr uint32_t kNoPos = 0xFFFFFFFFu;

struct alignas(16) RefLds {
    OrderedLds g;  // the greedy; until its grid is initialised, pxy .. grid_lds are the phases' scratch
    // sorted list of the unresolved ranges [lo, hi) (> 16 elements), double-buffered, with depth left
    uint32_t r_lo[2][kRefMaxRanges];
    uint32_t r_hi[2][kRefMaxRanges];
    uint32_t r_dep[2][kRefMaxRanges];
    // the level's active ranges (the list's prefix overlapping the window) j < m_act
    uint32_t o[kRefMaxRanges + 1];  // flat offset of range j's partition span [lo + 1, hi)
    float piv[kRefMaxRanges];
    uint32_t headL[kRefMaxRanges], headR[kRefMaxRanges], headW[kRefMaxRanges];
    uint32_t bL[kRefMaxRanges], nL[kRefMaxRanges], eR[kRefMaxRanges], nR[kRefMaxRanges];
    uint32_t cut[kRefMaxRanges];
    uint32_t waveL[kRefWaves], waveR[kRefWaves];
    // leaves produced by the level
    uint32_t leaf_lo[2 * kRefMaxRanges], leaf_hi[2 * kRefMaxRanges];
    // ranges of <= kRefWaveLocal elements handed to single waves (first window only), and the waves' stacks
    uint32_t wl_lo[kRefMaxRanges], wl_hi[kRefMaxRanges], wl_dep[kRefMaxRanges];
    uint32_t wl_ord[kRefMaxRanges];  // the list by size, largest first
    int wl_next;                     // next entry of wl_ord for a free wave
    uint32_t wstk[kRefWaves][kRefStack];
    uint32_t wsum[kRefWaves];
    uint16_t rid[kRefRidCap];  // levels with T <= kRefRidCap: each element's active range (set by pass 1)
    int cur, m_all, m_act, n_leaf, fail, n_wl, n_heap, n_hq;
    uint32_t heap_j[kRefMaxRanges];      // active ranges at depth 0 (heapsort fallback)
    uint32_t hq[2 * kRefMaxRanges];      // wave-local subranges at depth 0: absolute [lo, hi), heapsorted after the phase
    uint32_t T, fin;
};
// The span the phases reuse before the grid exists (bitmap, element copies, wave-local buffers).
static_assert(offsetof(RefLds, g) == 0 && offsetof(OrderedLds, pxy) == 0 &&
                  offsetof(OrderedLds, pcell) == sizeof(OrderedLds::pxy) &&
                  offsetof(OrderedLds, cmask) == offsetof(OrderedLds, pcell) + sizeof(OrderedLds::pcell) &&
                  offsetof(OrderedLds, grid_lds) == offsetof(OrderedLds, cmask) + sizeof(OrderedLds::cmask),
              "greedy span: pxy .. grid_lds contiguous");
constexpr uint32_t kRefSpanBytes =
    sizeof(OrderedLds::pxy) + sizeof(OrderedLds::pcell) + sizeof(OrderedLds::cmask) + sizeof(OrderedLds::grid_lds);

// Range guard of every data-dependent index (the emulation's invariants keep them in range; a broken
// invariant clamps the access, marks the frame failed and, with RefSortArgs::dbg, records the first
// violation: code, index, bound, level).
#define FD_REF_IDX(idx, bound, code) ref_idx((idx), (bound), (code), L, r, f)
__device__ __forceinline__ uint32_t ref_idx(uint32_t idx, uint32_t bound, uint32_t code, RefLds &L,
                                            const RefSortArgs &r, int f) {
    if (idx < bound) return idx;
    L.fail = 4;
    if (r.dbg && atomicCAS(&r.dbg[static_cast<int64_t>(f) * 8], 0u, code) == 0u) {
        r.dbg[static_cast<int64_t>(f) * 8 + 1] = idx;
        r.dbg[static_cast<int64_t>(f) * 8 + 2] = bound;
        r.dbg[static_cast<int64_t>(f) * 8 + 3] = static_cast<uint32_t>(L.m_act);
        r.dbg[static_cast<int64_t>(f) * 8 + 4] = L.T;
    }
    return bound ? bound - 1u : 0u;
}

// Index of the active range holding flat element e (o[j] <= e < o[j+1]), from a wave-uniform start j0
// at most 5 ranges back (every span has >= 16 elements, a round of 64 lanes meets <= 5 of them).
__device__ __forceinline__ int range_of(const uint32_t *o, int m, int j0, uint32_t e) {
    int j = j0;
    while (j + 1 < m && o[j + 1] <= e) ++j;
    return j;
}

// First active range whose span holds flat element e (binary search, wave-uniform e).
__device__ __forceinline__ int range_search(const uint32_t *o, int m, uint32_t e) {
    int lo = 0, hi = m - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (o[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Wave 0: the active prefix of the current list for window [fin, win_end) and the flat offsets of
// the active ranges' partition spans.
__device__ __forceinline__ void set_active(RefLds &L, uint32_t win_end) {
    const int lane = lane_id();
    const int c = L.cur, m = L.m_all;
    uint32_t carry = 0;
    int act = 0;
    for (int b = 0; b < m; b += kWave) {
        const int j = b + lane;
        const bool in = j < m && L.r_lo[c][j] < win_end;
        const uint64_t bal = ballot(in);
        const uint32_t span = in ? L.r_hi[c][j] - L.r_lo[c][j] - 1u : 0u;
        const uint32_t incl = wave_incl_add(span);
        if (in) L.o[j] = carry + incl - span;
        carry += static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(incl), kWave - 1));
        act += popc64(bal);
        if (bal != ~0ull) break;  // sorted list: the first range past the window ends the prefix
    }
    if (lane == 0) {
        L.m_act = act;
        L.o[act] = carry;
        L.T = carry;
    }
}

// Diagnostic phase clocks (SelectArgs::stamps, FD_SELECT_STAMPS): thread 0 adds the cycles since the
// previous mark to slot k of the frame's stamps (slots 16-23; k_select uses 0-15).
#define FD_REF_MARK(k)                                                                  \
    do {                                                                                \
        if (a.stamps && tid == 0) {                                                     \
            const uint64_t now_ = __builtin_readcyclecounter();                         \
            a.stamps[static_cast<int64_t>(f) * 32 + (k)] += now_ - t_mark;              \
            t_mark = now_;                                                              \
        }                                                                               \
    } while (0)
#define FD_REF_COUNT(k, v)                                                              \
    do {                                                                                \
        if (a.stamps && tid == 0) a.stamps[static_cast<int64_t>(f) * 32 + (k)] += (v);  \
    } while (0)

// Wave 0: the active ranges at the depth limit (L.heap_j) heapsorted one at a time (std::__partial_sort,
// ref_heapsort; in LDS when the range fits the free space: the greedy span before the grid exists, pxy ..
// cmask after), their visiting order written to ord (final), and the range list rebuilt without them.
// (A function of its own: the rare path stays out of k_select_reference's register allocation.)
__device__ __attribute__((noinline)) void ref_heap_step(lds_t<RefLds> *Lp, uint2 *X, uint32_t *ord, uint32_t n, int m,
                                                        bool grid_ready) {
    RefLds &L = *from_lds(Lp);
    const int lane = lane_id();
    const int c = L.cur, nh = L.n_heap;
    const uint32_t cap_lds = static_cast<uint32_t>(
        (grid_ready ? sizeof(L.g.pxy) + sizeof(L.g.pcell) + sizeof(L.g.cmask)
                    : sizeof(L.g.pxy) + sizeof(L.g.pcell) + sizeof(L.g.cmask) + sizeof(L.g.grid_lds)) / sizeof(uint2));
    for (int h = 0; h < nh; ++h) {
        const uint32_t j = L.heap_j[h];
        const uint32_t lo = L.r_lo[c][j], hi = min(L.r_hi[c][j], n);
        const uint32_t len = hi > lo ? hi - lo : 0u;
        uint2 *hbuf = X + lo;
        if (len <= cap_lds) {
            hbuf = reinterpret_cast<uint2 *>(L.g.pxy);
            for (uint32_t i = lane; i < len; i += kWave) hbuf[i] = X[lo + i];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        ref_heapsort(hbuf, static_cast<int>(len));
        for (uint32_t i = lane; i < len; i += kWave) {
            const uint2 e = hbuf[i];
            X[lo + i] = e;
            ord[lo + i] = e.y;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // the list without them (order kept), into the other buffer
    const int nc = c ^ 1;
    uint32_t at = 0;
    for (int b = 0; b < L.m_all; b += kWave) {
        const int j = b + lane;
        const bool keep = j < L.m_all && !(j < m && L.r_dep[c][j] == 0u);
        const uint64_t bk = ballot(keep);
        if (keep) {
            const uint32_t q = at + static_cast<uint32_t>(mbcnt64(bk, 0));
            L.r_lo[nc][q] = L.r_lo[c][j];
            L.r_hi[nc][q] = L.r_hi[c][j];
            L.r_dep[nc][q] = L.r_dep[c][j];
        }
        at += static_cast<uint32_t>(popc64(bk));
    }
    if (lane == 0) {
        L.m_all = static_cast<int>(at);
        L.cur = nc;
    }
    __builtin_amdgcn_s_waitcnt(0);
    set_active(L, L.fin + kSelectChunk);
}

// One flagged frame as the phases of k_select_reference see it (per thread; the phases are inlined into
// the kernel, which keeps the object in registers). A phase runs on every thread of the workgroup and
// keeps its barriers inside.
struct RefFrame {
    static constexpr int NT = kRefThreads;
    RefLds &L;
    const SelectArgs &a;
    const RefSortArgs &r;
    const int f, tid, lane, wv;
    uint64_t t_mark;  // FD_REF_MARK's clock (thread 0)
    uint32_t n, npx;
    const float *lresp;
    const uint32_t *lidx;
    uint2 *X;
    const uint32_t *Xr;  // X[p].x (response bits) = Xr[2p]
    uint32_t *lpos, *rpos, *ord;
    // The grid is initialised just before the first greedy scan: until then its LDS (with pxy .. cmask)
    // holds the partition levels' element copies and stopper positions (LDS mode below).
    bool grid_ready = false;
    bool wrote = false;  // a window's greedy has written features (out_xy no longer k_select's)

    __device__ __forceinline__ RefFrame(RefLds &L_, const SelectArgs &a_, const RefSortArgs &r_, int f_)
        : L(L_), a(a_), r(r_), f(f_), tid(threadIdx.x), lane(lane_id()), wv(threadIdx.x / kWave) {
        t_mark = a.stamps && tid == 0 ? __builtin_readcyclecounter() : 0ull;
        if (a.stamps && tid == 0)
            for (int k = 0; k < 32; ++k) a.stamps[static_cast<int64_t>(f) * 32 + k] = 0;  // (after k_select's printout)
        n = static_cast<uint32_t>(min(static_cast<int64_t>(a.cand_n[f]), a.list_cap));
        npx = static_cast<uint32_t>(a.rows) * static_cast<uint32_t>(a.cols);
        lresp = a.list_resp + static_cast<int64_t>(f) * a.list_cap;
        lidx = a.list_idx + static_cast<int64_t>(f) * a.list_cap;
        X = r.x + static_cast<int64_t>(f) * r.cap;
        Xr = reinterpret_cast<const uint32_t *>(X);
        lpos = r.lpos + static_cast<int64_t>(f) * r.cap;
        rpos = r.rpos + static_cast<int64_t>(f) * r.cap;
        ord = r.ord + static_cast<int64_t>(f) * r.cap;
    }

    // ---- 1. the push order: X = the frame's candidates as std::sort receives them ----------------------
    // (every per-candidate loop loads kRefPush candidates' data before using any: one memory round trip
    // per kRefPush candidates instead of one or two per candidate)
    __device__ __forceinline__ void push_order() {
        constexpr int kRefPush = 8;
        if (r.wide) {
            // (the prelude built X)
        } else if (r.push_order) {
            for (uint32_t i0 = tid; i0 < n; i0 += kRefPush * NT) {
                float rv[kRefPush];
                uint32_t qv[kRefPush];
#pragma unroll
                for (int k = 0; k < kRefPush; ++k) {
                    const uint32_t i = min(i0 + k * NT, n - 1u);
                    rv[k] = lresp[i];
                    qv[k] = lidx[i];
                }
#pragma unroll
                for (int k = 0; k < kRefPush; ++k)
                    if (i0 + k * NT < n) X[i0 + k * NT] = make_uint2(__float_as_uint(rv[k]), qv[k]);
            }
        } else {
            // Raster order of unique pixel indices, a part of the frame at a time: the part's candidate bitmap
            // in LDS (the greedy's arrays, pxy .. grid_lds, are free until the grid is initialised; LDS
            // atomics instead of one global atomic per candidate, which one CU issues slowly), its word prefix
            // (offset by the earlier parts' candidates) in rpos, rank = prefix + set bits below.
            constexpr uint32_t kPartWords = kRefSpanBytes / 4;
            uint32_t *const lbits = L.g.pxy;
            uint32_t *const wpre = rpos;
            const uint32_t words = (npx + 31u) >> 5;
            uint32_t carry = 0;  // candidates in the earlier parts
            for (uint32_t pw0 = 0; pw0 < words; pw0 += kPartWords) {
                const uint32_t pw = min(kPartWords, words - pw0);
                for (uint32_t w = tid; w < pw; w += NT) lbits[w] = 0u;
                __syncthreads();
                for (uint32_t i0 = tid; i0 < n; i0 += kRefPush * NT) {
                    uint32_t qv[kRefPush];
#pragma unroll
                    for (int k = 0; k < kRefPush; ++k) qv[k] = lidx[min(i0 + k * NT, n - 1u)];
#pragma unroll
                    for (int k = 0; k < kRefPush; ++k) {
                        const uint32_t wl = (qv[k] >> 5) - pw0;  // (wraps past the part when below it)
                        if (i0 + k * NT < n && qv[k] < npx && wl < pw) atomicOr(&lbits[wl], 1u << (qv[k] & 31u));
                    }
                }
                __syncthreads();
                // word prefix: a run of consecutive words per thread
                const uint32_t per = (pw + NT - 1) / NT;
                const uint32_t w0 = min(pw, tid * per), w1 = min(pw, w0 + per);
                uint32_t cnt = 0;
                for (uint32_t w = w0; w < w1; ++w) cnt += __popc(lbits[w]);
                uint32_t tot;
                uint32_t base = carry + wg_excl_add<NT>(cnt, L.wsum, tot);
                for (uint32_t w = w0; w < w1; ++w) {
                    wpre[pw0 + w] = base;
                    base += __popc(lbits[w]);
                }
                carry += tot;
                __syncthreads();  // (the prefix stores are read back by other threads: same workgroup, L1-coherent
                                  // through the barrier's release/acquire)
                for (uint32_t i0 = tid; i0 < n; i0 += kRefPush * NT) {
                    uint32_t qv[kRefPush], wp[kRefPush];
                    float rv[kRefPush];
#pragma unroll
                    for (int k = 0; k < kRefPush; ++k) {
                        const uint32_t i = min(i0 + k * NT, n - 1u);
                        qv[k] = lidx[i];
                        rv[k] = lresp[i];
                    }
#pragma unroll
                    for (int k = 0; k < kRefPush; ++k) {
                        const uint32_t wl = min((qv[k] >> 5) - pw0, pw - 1u);
                        wp[k] = wpre[pw0 + wl];
                    }
#pragma unroll
                    for (int k = 0; k < kRefPush; ++k) {
                        const uint32_t q = qv[k], wl = (q >> 5) - pw0;
                        if (i0 + k * NT >= n || q >= npx || wl >= pw) continue;
                        const uint32_t rk = wp[k] + __popc(lbits[wl] & ((1u << (q & 31u)) - 1u));
                        X[FD_REF_IDX(rk, n, 1)] = make_uint2(__float_as_uint(rv[k]), q);
                    }
                }
                __syncthreads();  // lbits reused by the next part (and the grid later)
            }
        }
    }

    // ---- the range list before the first window: __introsort_loop(0, n, 2 * __lg(n)) -------------------
    __device__ __forceinline__ void init_ranges() {
        if (tid == 0) {
            ordered_reset(L.g);
            L.fail = 0;
            L.n_hq = 0;
            L.cur = 0;
            L.n_leaf = 0;
            L.fin = 0;
            L.n_wl = 0;
            // __introsort_loop(0, n, 2 * __lg(n)); n <= 16: the final insertion sort alone (one leaf)
            if (r.wide) {
                // the prelude's state: [0, h) of its last level, then the levels' right children, in position
                // order; ranges of <= 16 elements are leaves
                const RefCtl &C = r.ctl[f];
                const uint32_t nlev = min(C.nlev, static_cast<uint32_t>(kRefWideLevels));
                if (C.n != n || C.bad) L.fail = 6;
                int m = 0, nl = 0;
                auto add = [&](uint32_t lo, uint32_t hi, uint32_t dep) {
                    if (hi > lo + static_cast<uint32_t>(kRefLeaf)) {
                        L.r_lo[0][m] = lo;
                        L.r_hi[0][m] = hi;
                        L.r_dep[0][m] = dep;
                        ++m;
                    } else if (hi > lo) {
                        L.leaf_lo[nl] = lo;
                        L.leaf_hi[nl] = hi;
                        ++nl;
                    }
                };
                add(0u, min(C.h[nlev], n), C.dep[nlev]);
                for (int l = static_cast<int>(nlev) - 1; l >= 0; --l) add(C.sib_lo[l], min(C.sib_hi[l], n), C.dep[l] - 1u);
                L.m_all = m;
                L.n_leaf = nl;
            } else if (n > static_cast<uint32_t>(kRefLeaf)) {
                L.r_lo[0][0] = 0;
                L.r_hi[0][0] = n;
                L.r_dep[0][0] = 2u * (31u - __clz(n));
                L.m_all = 1;
            } else {
                L.m_all = 0;
                if (n > 0) {
                    L.leaf_lo[0] = 0;
                    L.leaf_hi[0] = n;
                    L.n_leaf = 1;
                }
            }
        }
        __syncthreads();
        FD_REF_MARK(16);  // push order (bitmap, ranks, scatter) + grid init
        if (wv == 0) set_active(L, kSelectChunk);
        __syncthreads();
    }

    // ---- active ranges at the depth limit: std::__partial_sort(first, last, last) ----------------------
    // Heapsorted one at a time by wave 0 (in LDS when the range fits the free space: the greedy span
    // before the grid exists, pxy .. cmask after), their visiting order written to ord (final), and
    // dropped from the range list; then the level runs on the rest. True: there were some (the list changed).
    __device__ __forceinline__ bool heap_ranges(int m) {
        if (tid == 0) L.n_heap = 0;
        __syncthreads();
        if (tid < m && L.r_dep[L.cur][tid] == 0u) L.heap_j[atomicAdd(&L.n_heap, 1)] = static_cast<uint32_t>(tid);
        __syncthreads();
        if (L.n_heap == 0) return false;
        if (wv == 0) ref_heap_step(to_lds(&L), X, ord, n, m, grid_ready);
        __syncthreads();
        FD_REF_COUNT(31, 1u);
        return true;
    }

    // ---- one partition level over the m active ranges (list buffer c) ----------------------------------
    // pivots: __move_median_to_first of every active range
    __device__ __forceinline__ void level_pivots(int m, int c) {
        if (tid < m) {
            const uint32_t lo = L.r_lo[c][tid], hi = L.r_hi[c][tid];
            if (L.r_dep[c][tid] == 0u) L.fail = 1;  // invariant: depth-0 ranges were heapsorted above
            const uint32_t mid = lo + (hi - lo) / 2u;
            const uint2 xa = X[FD_REF_IDX(lo + 1, n, 2)], xb = X[FD_REF_IDX(mid, n, 2)], xc = X[FD_REF_IDX(hi - 1, n, 2)];
            const uint32_t ch = median_pos(as_f(xa.x), as_f(xb.x), as_f(xc.x), lo + 1, mid, hi - 1);
            const uint2 xp = ch == lo + 1 ? xa : (ch == mid ? xb : xc);
            const uint2 x0 = X[FD_REF_IDX(lo, n, 3)];
            X[FD_REF_IDX(lo, n, 3)] = xp;
            X[FD_REF_IDX(ch, n, 3)] = x0;
            L.piv[tid] = as_f(xp.x);
            L.cut[tid] = kNoPos;  // (written by the element where l_k < r_k stops holding)
        }
        __syncthreads();
        FD_REF_MARK(24);  // pivots
    }

    // pass 1 over the wave's block [e0, e1) of the flat element space: stopper counts per wave, local
    // prefixes at the range heads. Each wave walks its block kRefU rounds of 64 elements at a time: the
    // rounds' element positions first (LDS), then all their response loads at once, then the ballots in
    // order (one global round trip per kRefU rounds instead of one per round).
    __device__ __forceinline__ void level_pass1(int m, int c, bool cached, bool ldsm, uint32_t e0, uint32_t e1) {
        uint32_t *const RV = L.g.pxy;
        {
            uint32_t cl = 0, cr = 0;
            int jw = e0 < e1 ? range_search(L.o, m, e0) : 0;
            for (uint32_t b0 = e0; b0 < e1; b0 += kRefU * kWave) {
                uint32_t pu[kRefU];
                int ju[kRefU];
                bool vu[kRefU];
                float ru[kRefU];
#pragma unroll
                for (int u = 0; u < kRefU; ++u) {
                    const uint32_t b = b0 + u * kWave, e = b + lane;
                    vu[u] = e < e1;
                    while (jw + 1 < m && L.o[jw + 1] <= b) ++jw;
                    ju[u] = vu[u] ? range_of(L.o, m, jw, e) : jw;
                    pu[u] = L.r_lo[c][ju[u]] + 1u + (e - L.o[ju[u]]);
                }
#pragma unroll
                for (int u = 0; u < kRefU; ++u) ru[u] = vu[u] ? as_f(Xr[2u * FD_REF_IDX(pu[u], n, 5)]) : 0.0f;
                if (cached) {
#pragma unroll
                    for (int u = 0; u < kRefU; ++u)
                        if (vu[u]) {
                            L.rid[b0 + u * kWave + lane] = static_cast<uint16_t>(ju[u]);
                            if (ldsm) RV[b0 + u * kWave + lane] = __float_as_uint(ru[u]);
                        }
                }
#pragma unroll
                for (int u = 0; u < kRefU; ++u) {
                    const uint32_t e = b0 + u * kWave + lane;
                    const int j = ju[u];
                    const float pv = L.piv[j];
                    const bool ls = vu[u] && ru[u] <= pv, rs = vu[u] && ru[u] >= pv;
                    const uint64_t bl = ballot(ls), br = ballot(rs);
                    if (vu[u] && e == L.o[j]) {
                        L.headL[j] = cl + mbcnt64(bl, 0);
                        L.headR[j] = cr + mbcnt64(br, 0);
                        L.headW[j] = wv;
                    }
                    cl += popc64(bl);
                    cr += popc64(br);
                }
            }
            if (lane == 0) {
                L.waveL[wv] = cl;
                L.waveR[wv] = cr;
            }
        }
        __syncthreads();
        FD_REF_MARK(25);  // pass 1
    }

    // per range: global stopper bases and counts. wbL, wbR: exclusive wave prefixes, lane i = wave i
    __device__ __forceinline__ void level_bases(int m, uint32_t &wbL, uint32_t &wbR) {
        {
            const uint32_t vl = lane < kRefWaves ? L.waveL[lane] : 0u, vr = lane < kRefWaves ? L.waveR[lane] : 0u;
            wbL = wave_incl_add(vl) - vl;
            wbR = wave_incl_add(vr) - vr;
        }
        const uint32_t totL = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(wbL), kRefWaves - 1)) +
                              L.waveL[kRefWaves - 1];
        const uint32_t totR = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(wbR), kRefWaves - 1)) +
                              L.waveR[kRefWaves - 1];
        {
            // every wave computes its lanes' ranges (shuffles are per wave); ranges j = tid < m
            const int j = tid < m ? tid : 0;
            const int jn = j + 1;
            const uint32_t hw = L.headW[j], hwn = jn < m ? L.headW[jn] : 0u;
            const uint32_t bLj = static_cast<uint32_t>(__shfl(static_cast<int>(wbL), static_cast<int>(hw))) + L.headL[j];
            const uint32_t bRj = static_cast<uint32_t>(__shfl(static_cast<int>(wbR), static_cast<int>(hw))) + L.headR[j];
            // (shuffles with every lane active: ds_bpermute does not read inactive source lanes)
            const uint32_t sLn = static_cast<uint32_t>(__shfl(static_cast<int>(wbL), static_cast<int>(hwn)));
            const uint32_t sRn = static_cast<uint32_t>(__shfl(static_cast<int>(wbR), static_cast<int>(hwn)));
            const uint32_t bLn = jn < m ? sLn + L.headL[jn] : totL;
            const uint32_t bRn = jn < m ? sRn + L.headR[jn] : totR;
            if (tid < m) {
                L.bL[tid] = bLj;
                L.nL[tid] = bLn - bLj;
                L.eR[tid] = bRn;
                L.nR[tid] = bRn - bRj;
            }
        }
        __syncthreads();
        FD_REF_MARK(26);  // stopper bases
    }

    // passes 2-3, compiled twice: stopper positions in LDS (LM, LDS mode) or in lpos / rpos
    template <bool LM>
    __device__ __forceinline__ void level_passes(int m, int c, bool cached, uint32_t e0, uint32_t e1, uint32_t wbL,
                                                 uint32_t wbR) {
        uint32_t *const RV = L.g.pxy;  // [kRefRidCap] x 3 over pxy .. grid_lds (96 KiB, see the push)
        uint32_t *const LP = RV + kRefRidCap;
        uint32_t *const RP = LP + kRefRidCap;
        auto lp_st = [&](uint32_t i, uint32_t v) {
            if constexpr (LM) LP[i] = v;
            else lpos[i] = v;
        };
        auto rp_st = [&](uint32_t i, uint32_t v) {
            if constexpr (LM) RP[i] = v;
            else rpos[i] = v;
        };
        auto lp_ld = [&](uint32_t i) -> uint32_t {
            if constexpr (LM) return LP[i];
            else return lpos[i];
        };
        auto rp_ld = [&](uint32_t i) -> uint32_t {
            if constexpr (LM) return RP[i];
            else return rpos[i];
        };
        // pass 2: scatter stopper positions by rank (left stoppers from the left, right from the right);
        // the same kRefU-round walk as pass 1
        {
            const uint32_t mywbL = static_cast<uint32_t>(__shfl(static_cast<int>(wbL), wv));
            const uint32_t mywbR = static_cast<uint32_t>(__shfl(static_cast<int>(wbR), wv));
            uint32_t cl = mywbL, cr = mywbR;
            int jw = !cached && e0 < e1 ? range_search(L.o, m, e0) : 0;
            for (uint32_t b0 = e0; b0 < e1; b0 += kRefU * kWave) {
                uint32_t pu[kRefU];
                int ju[kRefU];
                bool vu[kRefU];
                float ru[kRefU];
#pragma unroll
                for (int u = 0; u < kRefU; ++u) {
                    const uint32_t b = b0 + u * kWave, e = b + lane;
                    vu[u] = e < e1;
                    if (cached) {
                        ju[u] = vu[u] ? L.rid[e] : 0;
                    } else {
                        while (jw + 1 < m && L.o[jw + 1] <= b) ++jw;
                        ju[u] = vu[u] ? range_of(L.o, m, jw, e) : jw;
                    }
                    pu[u] = L.r_lo[c][ju[u]] + 1u + (e - L.o[ju[u]]);
                }
#pragma unroll
                for (int u = 0; u < kRefU; ++u)
                    ru[u] = !vu[u] ? 0.0f : (LM ? as_f(RV[b0 + u * kWave + lane]) : as_f(Xr[2u * FD_REF_IDX(pu[u], n, 6)]));
#pragma unroll
                for (int u = 0; u < kRefU; ++u) {
                    const int j = ju[u];
                    const uint32_t oj = L.o[j], p = pu[u];
                    const float pv = L.piv[j];
                    const bool ls = vu[u] && ru[u] <= pv, rs = vu[u] && ru[u] >= pv;
                    const uint64_t bl = ballot(ls), br = ballot(rs);
                    if (ls) {
                        const uint32_t rankL = static_cast<uint32_t>(mbcnt64(bl, 0)) + cl - L.bL[j];  // 0-based
                        lp_st(FD_REF_IDX(oj + rankL, L.T, 7), p);
                    }
                    if (rs) {
                        const uint32_t rankR = L.eR[j] - (static_cast<uint32_t>(mbcnt64(br, 0)) + cr) - 1u;  // from the right
                        rp_st(FD_REF_IDX(oj + rankR, L.T, 8), p);
                    }
                    cl += popc64(bl);
                    cr += popc64(br);
                }
            }
        }
        __syncthreads();
        FD_REF_MARK(27);  // pass 2
        // pass 3 (swaps and cuts in one pass): pair k is exchanged iff t_k = l_k < r_k (monotone in k,
        // so these are exactly the pairs k < K); the element where t stops holding finds K and writes
        // the range's cut -- K = k + 1 at the last true pair (cut = min(l_{K}, r_{K-1})), K = 0 at a
        // false first pair (cut = l_0). The kRefU rounds' stopper positions, then their elements,
        // loaded together.
        {
            int jw = !cached && e0 < e1 ? range_search(L.o, m, e0) : 0;
            for (uint32_t b0 = e0; b0 < e1; b0 += kRefU * kWave) {
                int ju[kRefU];
                bool vu[kRefU];
                uint32_t l0[kRefU], r0[kRefU], l1[kRefU], r1[kRefU];
                uint2 vl[kRefU], vr[kRefU];
#pragma unroll
                for (int u = 0; u < kRefU; ++u) {
                    const uint32_t b = b0 + u * kWave, e = b + lane;
                    vu[u] = e < e1;
                    if (cached) {
                        ju[u] = vu[u] ? L.rid[e] : 0;
                    } else {
                        while (jw + 1 < m && L.o[jw + 1] <= b) ++jw;
                        ju[u] = vu[u] ? range_of(L.o, m, jw, e) : jw;
                    }
                }
#pragma unroll
                for (int u = 0; u < kRefU; ++u) {
                    const uint32_t e = b0 + u * kWave + lane;
                    // (clamped reads: entries past T are never used)
                    l0[u] = lp_ld(FD_REF_IDX(min(e, L.T - 1u), L.T, 9));
                    r0[u] = rp_ld(FD_REF_IDX(min(e, L.T - 1u), L.T, 9));
                    l1[u] = lp_ld(FD_REF_IDX(min(e + 1u, L.T - 1u), L.T, 10));
                    r1[u] = rp_ld(FD_REF_IDX(min(e + 1u, L.T - 1u), L.T, 10));
                }
                bool su[kRefU];
#pragma unroll
                for (int u = 0; u < kRefU; ++u) {
                    const uint32_t e = b0 + u * kWave + lane;
                    const int j = ju[u];
                    const uint32_t k = e - L.o[j];  // 0-based pair index
                    const uint32_t nLj = L.nL[j], mn = min(nLj, L.nR[j]);
                    const bool t = vu[u] && k < mn && l0[u] < r0[u];
                    const bool tn = t && k + 1 < mn && l1[u] < r1[u];
                    su[u] = t;
                    if (t && !tn) {  // K = k + 1
                        uint32_t cut = r0[u];
                        if (k + 1 < nLj) cut = min(cut, l1[u]);
                        L.cut[j] = cut;
                    } else if (vu[u] && k == 0u && !t) {  // K = 0 (nL >= 1: the median leaves a stopper)
                        L.cut[j] = l0[u];
                    }
                    if (t) {
                        l0[u] = FD_REF_IDX(l0[u], n, 12);
                        r0[u] = FD_REF_IDX(r0[u], n, 13);
                    }
                }
#pragma unroll
                for (int u = 0; u < kRefU; ++u) {
                    if (su[u]) {
                        vl[u] = X[l0[u]];
                        vr[u] = X[r0[u]];
                    }
                }
#pragma unroll
                for (int u = 0; u < kRefU; ++u) {
                    if (su[u]) {
                        X[l0[u]] = vr[u];
                        X[r0[u]] = vl[u];
                    }
                }
            }
        }
        __syncthreads();
        FD_REF_MARK(29);  // pass 3 (swaps + cuts)
    }

    // children: ranges > 16 into the next list (in order), the rest are leaves; then the active prefix
    __device__ __forceinline__ void level_children(int m, int c) {
        if (wv == 0) {
            const int nc = c ^ 1;
            uint32_t w_at = 0, l_at = 0;
            // before the first greedy scan, children of <= kRefWaveLocal elements go to the wave-local
            // list (while it has room) instead of the next level
            const bool wl_on = !grid_ready;
            uint32_t v_at = static_cast<uint32_t>(L.n_wl);
            for (int b = 0; b < m; b += kWave) {
                const int j = b + lane;
                const bool in = j < m;
                uint32_t lo = 0, hi = 0, ct = 0, dp = 0;
                if (in) {
                    lo = L.r_lo[c][j];
                    hi = L.r_hi[c][j];
                    ct = L.cut[j];
                    dp = L.r_dep[c][j] - 1u;
                    if (ct <= lo || ct >= hi) {  // (cannot happen: the scans stop inside the range)
                        L.fail = 2;
                        ct = lo + 1;
                    }
                }
                bool bigL = in && ct - lo > static_cast<uint32_t>(kRefLeaf);
                bool bigR = in && hi - ct > static_cast<uint32_t>(kRefLeaf);
                {
                    const bool cL = wl_on && bigL && ct - lo <= kRefWaveLocal;
                    const bool cR = wl_on && bigR && hi - ct <= kRefWaveLocal;
                    const uint32_t nv = (cL ? 1u : 0u) + (cR ? 1u : 0u);
                    const uint32_t iv = wave_incl_add(nv);
                    uint32_t pv = v_at + iv - nv;
                    if (cL && pv < static_cast<uint32_t>(kRefMaxRanges)) {
                        L.wl_lo[pv] = lo;
                        L.wl_hi[pv] = ct;
                        L.wl_dep[pv] = dp;
                        bigL = false;
                    }
                    if (cL) ++pv;
                    if (cR && pv < static_cast<uint32_t>(kRefMaxRanges)) {
                        L.wl_lo[pv] = ct;
                        L.wl_hi[pv] = hi;
                        L.wl_dep[pv] = dp;
                        bigR = false;
                    }
                    v_at += static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(iv), kWave - 1));
                }
                const uint32_t nb = (bigL ? 1u : 0u) + (bigR ? 1u : 0u);
                const bool leafL = in && ct - lo <= static_cast<uint32_t>(kRefLeaf);
                const bool leafR = in && hi - ct <= static_cast<uint32_t>(kRefLeaf);
                const uint32_t nlf = (leafL ? 1u : 0u) + (leafR ? 1u : 0u);
                const uint32_t ib = wave_incl_add(nb), il = wave_incl_add(nlf);
                uint32_t pb = w_at + ib - nb, pl = l_at + il - nlf;
                if (bigL && pb < kRefMaxRanges) {
                    L.r_lo[nc][pb] = lo;
                    L.r_hi[nc][pb] = ct;
                    L.r_dep[nc][pb] = dp;
                }
                if (bigL) ++pb;
                if (bigR && pb < kRefMaxRanges) {
                    L.r_lo[nc][pb] = ct;
                    L.r_hi[nc][pb] = hi;
                    L.r_dep[nc][pb] = dp;
                }
                if (leafL) {
                    L.leaf_lo[pl] = lo;
                    L.leaf_hi[pl] = ct;
                    ++pl;
                }
                if (leafR) {
                    L.leaf_lo[pl] = ct;
                    L.leaf_hi[pl] = hi;
                }
                w_at += static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(ib), kWave - 1));
                l_at += static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(il), kWave - 1));
            }
            // the ranges right of the window follow unchanged
            const int rest = L.m_all - m;
            for (int i = lane; i < rest; i += kWave) {
                const uint32_t q = w_at + static_cast<uint32_t>(i);
                if (q < kRefMaxRanges) {
                    L.r_lo[nc][q] = L.r_lo[c][m + i];
                    L.r_hi[nc][q] = L.r_hi[c][m + i];
                    L.r_dep[nc][q] = L.r_dep[c][m + i];
                }
            }
            if (lane == 0) {
                const uint32_t tot = w_at + static_cast<uint32_t>(rest);
                if (tot > kRefMaxRanges) L.fail = 3;
                L.m_all = static_cast<int>(min(tot, static_cast<uint32_t>(kRefMaxRanges)));
                L.cur = nc;
                L.n_leaf = static_cast<int>(l_at);
                L.n_wl = static_cast<int>(min(v_at, static_cast<uint32_t>(kRefMaxRanges)));
            }
            __builtin_amdgcn_s_waitcnt(0);
            set_active(L, L.fin + kSelectChunk);
        }
        __syncthreads();
        FD_REF_MARK(30);  // children + active prefix
    }

    // The level: every active range partitioned once. False: a broken invariant (L.fail).
    __device__ __forceinline__ bool partition_level(int m) {
        const int c = L.cur;
        const uint64_t t_level = a.stamps && tid == 0 ? __builtin_readcyclecounter() : 0ull;
        level_pivots(m, c);
        if (L.fail) return false;
        const uint32_t T = L.T;
        const bool cached = T <= kRefRidCap;  // passes 2-3 read the range index pass 1 stored
        // LDS mode (small levels before the first greedy scan): pass 1 also keeps each element's
        // response in LDS (RV) and the stopper positions live in LDS (LP, RP) instead of lpos / rpos:
        // pass 2 makes no memory round trip, pass 3 one (the swaps themselves).
        const bool ldsm = cached && !grid_ready;
        const uint32_t blk = ((T + kRefWaves * kWave - 1) / (kRefWaves * kWave)) * kWave;
        const uint32_t e0 = min(T, wv * blk), e1 = min(T, e0 + blk);
        level_pass1(m, c, cached, ldsm, e0, e1);
        uint32_t wbL, wbR;
        level_bases(m, wbL, wbR);
        if (ldsm) level_passes<true>(m, c, cached, e0, e1, wbL, wbR);
        else level_passes<false>(m, c, cached, e0, e1, wbL, wbR);
        level_children(m, c);
        if (a.stamps && tid == 0) {  // per level (slots 0-15): T << 40 | cycles
            const uint64_t lv = a.stamps[static_cast<int64_t>(f) * 32 + 18];
            if (lv < 16u)
                a.stamps[static_cast<int64_t>(f) * 32 + lv] =
                    (static_cast<uint64_t>(T) << 40) | (__builtin_readcyclecounter() - t_level);
        }
        FD_REF_COUNT(18, 1u);
        FD_REF_COUNT(19, T);
        return !L.fail;
    }

    // ---- leaves: the final insertion sort (stable, response descending) into the visiting order --------
    // 16 lanes per leaf: lane q holds element q and counts the elements that precede it
    __device__ __forceinline__ void leaves() {
        for (int lf0 = 0; lf0 < L.n_leaf; lf0 += NT / kRefLeaf) {
            const int lf = lf0 + tid / kRefLeaf, q = tid % kRefLeaf;
            const bool have_leaf = lf < L.n_leaf;
            const uint32_t lo = have_leaf ? L.leaf_lo[lf] : 0u, hi = have_leaf ? L.leaf_hi[lf] : 0u;
            const int len = min(static_cast<int>(hi - lo), kRefLeaf);
            const bool mine = have_leaf && q < len;
            const uint2 v = mine ? X[FD_REF_IDX(lo + q, n, 16)] : make_uint2(0u, 0u);
            const float ri = as_f(v.x);
            uint32_t rk = 0;
#pragma unroll
            for (int t = 0; t < kRefLeaf; ++t) {  // lane group's element t (every lane of the wave takes part)
                const float rt = as_f(static_cast<uint32_t>(__shfl(static_cast<int>(v.x), (lane & ~(kRefLeaf - 1)) + t)));
                rk += (t < len && (rt > ri || (rt == ri && t < q))) ? 1u : 0u;
            }
            if (mine) ord[FD_REF_IDX(lo + rk, n, 17)] = v.y;
        }
        __syncthreads();
        FD_REF_MARK(20);  // leaves
        if (tid == 0) L.n_leaf = 0;
    }

    // ---- wave-local ranges: one wave each, partitioned to the end in LDS (the greedy span) -------------
    // False: a broken invariant (L.fail).
    __device__ __forceinline__ bool wave_local() {
        constexpr uint32_t kWaveBytes = kRefWaveLocal * (8u + 2u + 2u);
        static_assert(kRefWaves * kWaveBytes <= kRefSpanBytes, "wave-local buffers fit the greedy span");
        unsigned char *const wb = reinterpret_cast<unsigned char *>(L.g.pxy) + wv * kWaveBytes;
        uint2 *const E = reinterpret_cast<uint2 *>(wb);
        uint16_t *const Lp = reinterpret_cast<uint16_t *>(wb + kRefWaveLocal * 8u);
        uint16_t *const Rp = Lp + kRefWaveLocal;
        const int nw = L.n_wl;
        // largest ranges first, each to whichever wave is free (longest-processing-time order)
        if (tid < nw) {
            const uint32_t st = L.wl_hi[tid] - L.wl_lo[tid];
            uint32_t rk = 0;
            for (int u = 0; u < nw; ++u) {
                const uint32_t su = L.wl_hi[u] - L.wl_lo[u];
                rk += (su > st || (su == st && u < tid)) ? 1u : 0u;
            }
            L.wl_ord[rk] = static_cast<uint32_t>(tid);
        }
        if (tid == 0) L.wl_next = kRefWaves;
        __syncthreads();
        bool ok = true;
        for (int j = wv; j < nw && ok;) {
            const uint32_t q = L.wl_ord[j];
            ok = ref_wave_resolve(X, ord, L.wl_lo[q], L.wl_hi[q], L.wl_dep[q], E, Lp, Rp, L.wstk[wv], L.hq, &L.n_hq);
            int nj = 0;
            if (lane == 0) nj = atomicAdd(&L.wl_next, 1);
            j = __builtin_amdgcn_readfirstlane(__shfl(nj, 0));
        }
        if (!ok && lane == 0) L.fail = 5;
        __syncthreads();
        if (L.n_hq > 0) {  // queued depth-limit subranges (<= kRefWaveLocal each): one wave each, in its buffer
            const int nq = min(L.n_hq, kRefMaxRanges);
            for (int q = wv; q < nq; q += kRefWaves) {
                const uint32_t qlo = L.hq[2 * q], len = min(L.hq[2 * q + 1] - qlo, kRefWaveLocal);
                for (uint32_t i = lane; i < len; i += kWave) E[i] = X[FD_REF_IDX(qlo + i, n, 19)];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                ref_heapsort(E, static_cast<int>(len));
                for (uint32_t i = lane; i < len; i += kWave) ord[FD_REF_IDX(qlo + i, n, 19)] = E[i].y;
            }
            if (tid == 0 && L.n_hq > kRefMaxRanges) L.fail = 7;
            __syncthreads();
            if (tid == 0) L.n_hq = 0;
        }
        if (tid == 0) L.n_wl = 0;
        FD_REF_MARK(23);  // wave-local ranges
        return !L.fail;
    }

    // ---- 3. window final: greedy over [fin, fin_new), the positions left of the first waiting range ----
    // Returns fin_new.
    __device__ __forceinline__ uint32_t greedy_window(const GreedyFrame &g) {
        const uint32_t fin = L.fin;
        const uint32_t fin_new = L.m_all > 0 ? L.r_lo[L.cur][0] : n;
        if (!grid_ready) {
            ordered_grid_init(a, g, tid, NT);
            grid_ready = true;
            __syncthreads();
        }
        for (uint32_t base = fin; base < fin_new && !r.order_only; base += kSelectChunk) {
            if (L.g.s_done) break;
            wrote = true;
            const int cn = static_cast<int>(min(static_cast<uint32_t>(kSelectChunk), fin_new - base));
            ordered_chunk(a, f, g, L.g, cn, [&](int i) { return ord[FD_REF_IDX(base + i, n, 18)]; }, tid, NT);
        }
        FD_REF_MARK(21);  // greedy over the finished window
        FD_REF_COUNT(22, 1u);
        return fin_new;
    }

    __device__ __forceinline__ void next_window(uint32_t fin_new) {
        if (wv == 0) {
            if (lane == 0) L.fin = fin_new;
            __builtin_amdgcn_s_waitcnt(0);
            set_active(L, fin_new + kSelectChunk);
        }
        __syncthreads();
    }

    // ---- the frame's status and count ------------------------------------------------------------------
    __device__ __forceinline__ void finish(bool finished) {
        __syncthreads();
        if (tid == 0) {
            if (!finished && !L.fail) L.fail = 8;  // the loop bound ran out
            if (L.fail) {
                // Device outputs of a failed frame: k_select's features (raster tie order) while no window
                // has been scanned; else the features the reference order accepted so far -- a prefix of the
                // reference's result, not a mix of the two orders. Host-output calls resolve it on the host.
                if (wrote) a.out_counts[f] = L.g.s_acc;
                atomicOr(&a.status[f], FD_FRAME_UNRESOLVED);
            } else {
                if (!r.order_only) a.out_counts[f] = L.g.s_acc;
                atomicOr(&a.status[f], FD_FRAME_RESOLVED);
            }
        }
    }
};

template <int NT>
__global__ __launch_bounds__(NT) void k_select_reference(SelectArgs a, RefSortArgs r) {
    static_assert(NT == kRefThreads, "k_select_reference runs 1024 threads");
    __shared__ RefLds L;
    const int f = blockIdx.x;
    const uint32_t st0 = a.status[f];
    if (!(st0 & FD_FRAME_TIES) || (st0 & FD_FRAME_GUARD)) return;
    RefFrame F(L, a, r, f);
    // 1. the push order
    F.push_order();
    const GreedyFrame g(a, f, L.g.grid_lds);
    F.init_ranges();
    // 2. windows x levels (bounded: each level halves). A frame whose emulation has not finished when the
    // bound runs out -- LSD seed orders of ~10M entries would need that many -- is failed (code 8), not
    // reported resolved with an unwritten tail of ord. (r.guard_limit: diagnostic override only.)
    const int guard_lim = r.guard_limit > 0 ? r.guard_limit : 1 << 16;
    bool finished = false;  // (uniform: set where every thread leaves the loop together)
    for (int guard = 0; guard < guard_lim; ++guard) {
        const int m = L.m_act;
        if (m > 0) {
            if (F.heap_ranges(m)) continue;
            if (!F.partition_level(m)) break;
        }
        F.leaves();
        if (L.m_act > 0) {  // the window is not all leaves yet: the next level
            __syncthreads();
            continue;
        }
        if (L.n_wl > 0 && !F.wave_local()) break;
        // 3. the greedy over the finished window
        const uint32_t fin_new = F.greedy_window(g);
        if (L.g.s_done || fin_new >= F.n) {
            finished = true;
            break;
        }
        F.next_window(fin_new);
    }
    F.finish(finished);
}

// Greedy selection in a given order: the host-resolved fallback of the reference order. On host-output
// calls the runtime sorts the candidates of a frame that k_select_reference left FD_FRAME_UNRESOLVED
// with std::sort itself (resolve_ties, fd_rt_select.cpp) and passes the raster indices in that order;
// they are visited chunk by chunk by the same ordered greedy. Overwrites the frame's features.
template <int NT>
__global__ __launch_bounds__(NT) void k_select_ordered(SelectArgs a, OrderedArgs o) {
    __shared__ OrderedLds L;
    const int j = blockIdx.x, tid = threadIdx.x;
    const int f = o.frame[j];
    const uint32_t *ord = o.order + o.offset[j];
    const int64_t n = o.count[j];
    const GreedyFrame g(a, f, L.grid_lds);
    ordered_grid_init(a, g, tid, NT);
    if (tid == 0) ordered_reset(L);
    __syncthreads();
    for (int64_t base = 0; base < n; base += kSelectChunk) {
        if (L.s_done) break;
        const int c = static_cast<int>(min(static_cast<int64_t>(kSelectChunk), n - base));
        ordered_chunk(a, f, g, L, c, [&](int i) { return ord[base + i]; }, tid, NT);
    }
    if (tid == 0) {
        a.out_counts[f] = L.s_acc;
        atomicAnd(&a.status[f], ~FD_FRAME_UNRESOLVED);
        atomicOr(&a.status[f], FD_FRAME_RESOLVED);
    }
}

}  // namespace

hipError_t launch_select_reference(const SelectArgs &a, const RefSortArgs &r0, int batch, bool wide, hipStream_t s) {
    if (batch <= 0) return hipSuccess;
    RefSortArgs r = r0;
    r.wide = wide ? 1 : 0;
    if (wide) {
        const hipError_t e = launch_ref_prelude(a, r, batch, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_select_reference<kRefThreads>, dim3(static_cast<unsigned>(batch)), dim3(kRefThreads), 0, s, a, r);
    return hipGetLastError();
}

hipError_t launch_select_ordered(const SelectArgs &a, const OrderedArgs &o, int n_frames, hipStream_t s) {
    if (n_frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_select_ordered<256>, dim3(static_cast<unsigned>(n_frames)), dim3(256), 0, s, a, o);
    return hipGetLastError();
}

}  // namespace fdk
