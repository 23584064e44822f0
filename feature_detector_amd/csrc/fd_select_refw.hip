// Wide prelude of k_select_reference (fd_select_ref.hip) for frames of >= 1 Mpx.
//
// One flagged 1080p frame holds ~10^5-10^6 candidates, and a single workgroup walks its push order and
// its first partition levels (the window's leftmost range [0, h) halves per level) through chains of
// memory round trips on one CU. The prelude spreads exactly that work over kRefWideGroups workgroups per
// frame, one kernel per step (the kernel boundary is the only cross-workgroup hand-off):
//   push: k_refw_init (state; the flagged frames into a compact list) -> k_refw_clear -> k_refw_bits (raster bitmap, global atomics) ->
//         k_refw_wcount (set bits per word slice) -> k_refw_wprefix (word prefix) -> k_refw_place
//         (X[rank] = candidate);
//   per level l while h > kRefWideMin: k_refw_lcount (pivot = median of X[1], X[h/2], X[h-1]; stopper
//         counts per block of [1, h)) -> k_refw_lscatter (stopper positions by rank) -> k_refw_lswap
//         (pairs with l_k < r_k swapped, the cut found where that stops holding, the pivot moved to 0).
// The pivot swap is applied virtually until k_refw_lswap (position ch reads the old X[0]), so no step
// writes what another workgroup of the same kernel reads. k_select_reference then starts from the state
// (RefCtl): range [0, h), the right children of the levels in position order, no push.
#include "fd_hip.h"
#include "fd_kernels.h"
#include "fd_ref_sort.h"

#include <algorithm>

namespace fdk {

namespace {

constexpr int kWT = 256;        // threads per prelude workgroup
constexpr int kWChunk = 8192;   // k_refw_lscatter: responses staged in LDS per chunk
constexpr int kWUnroll = 8;     // loads issued before use
constexpr uint32_t kNone = 0xFFFFFFFFu;

__device__ __forceinline__ bool wide_frame(const SelectArgs &a, int f) {
    const uint32_t st = a.status[f];
    return (st & FD_FRAME_TIES) && !(st & FD_FRAME_GUARD);
}

// [s, e) = workgroup g's share of [0, len) (blocks of ceil(len / G))
__device__ __forceinline__ void wide_share(uint32_t len, int g, uint32_t &s, uint32_t &e) {
    const uint32_t b = (len + kRefWideGroups - 1) / kRefWideGroups;
    s = min(len, static_cast<uint32_t>(g) * b);
    e = min(len, s + b);
}

// one workgroup per frame: the state of a flagged frame, and the frame into the compact list the other
// prelude kernels walk (their grids cover min(batch, kRefWideSlots) frames x kRefWideGroups)
__global__ __launch_bounds__(kWT) void k_refw_init(SelectArgs a, RefSortArgs r) {
    const int f = blockIdx.x;
    if (!wide_frame(a, f) || threadIdx.x != 0) return;
    RefCtl &C = r.ctl[f];
    const uint32_t n = static_cast<uint32_t>(min(static_cast<int64_t>(a.cand_n[f]), a.list_cap));
    C.n = n;
    C.nlev = 0;
    C.bad = 0;
    C.h[0] = n;
    C.dep[0] = n > static_cast<uint32_t>(kRefLeaf) ? 2u * (31u - __clz(n)) : 0u;
    C.act[0] = n > kRefWideMin && C.dep[0] > 0u ? 1u : 0u;
    for (int l = 1; l <= kRefWideLevels; ++l) C.act[l] = 0u;
    const uint32_t j = atomicAdd(&r.wfr[0], 1u);
    r.wfr[1 + j] = static_cast<uint32_t>(f);
}

__device__ __forceinline__ void refw_clear(const SelectArgs &a, const RefSortArgs &r, int f, int g, int) {
    if (r.push_order) return;
    const uint32_t npx = static_cast<uint32_t>(a.rows) * static_cast<uint32_t>(a.cols);
    uint32_t s, e;
    wide_share((npx + 31u) >> 5, g, s, e);
    uint32_t *bits = r.lpos + static_cast<int64_t>(f) * r.cap;
    for (uint32_t w = s + threadIdx.x; w < e; w += kWT) bits[w] = 0u;
}

__device__ __forceinline__ void refw_bits(const SelectArgs &a, const RefSortArgs &r, int f, int g, int) {
    if (!wide_frame(a, f)) return;
    const uint32_t n = r.ctl[f].n;
    const uint32_t npx = static_cast<uint32_t>(a.rows) * static_cast<uint32_t>(a.cols);
    const float *lresp = a.list_resp + static_cast<int64_t>(f) * a.list_cap;
    const uint32_t *lidx = a.list_idx + static_cast<int64_t>(f) * a.list_cap;
    uint2 *X = r.x + static_cast<int64_t>(f) * r.cap;
    uint32_t *bits = r.lpos + static_cast<int64_t>(f) * r.cap;
    uint32_t s, e;
    wide_share(n, g, s, e);
    for (uint32_t i0 = s + threadIdx.x; i0 < e; i0 += kWUnroll * kWT) {
        uint32_t qv[kWUnroll];
        float rv[kWUnroll];
#pragma unroll
        for (int k = 0; k < kWUnroll; ++k) {
            const uint32_t i = min(i0 + k * kWT, e - 1u);
            qv[k] = lidx[i];
            rv[k] = r.push_order ? lresp[i] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < kWUnroll; ++k) {
            if (i0 + k * kWT >= e) continue;
            if (r.push_order) X[i0 + k * kWT] = make_uint2(__float_as_uint(rv[k]), qv[k]);
            else if (qv[k] < npx) atomicOr(&bits[qv[k] >> 5], 1u << (qv[k] & 31u));
        }
    }
}

__device__ __forceinline__ void refw_wcount(const SelectArgs &a, const RefSortArgs &r, int f, int g, int) {
    __shared__ uint32_t ws[kWT / kWave];
    if (!wide_frame(a, f) || r.push_order) return;
    const uint32_t npx = static_cast<uint32_t>(a.rows) * static_cast<uint32_t>(a.cols);
    const uint32_t *bits = r.lpos + static_cast<int64_t>(f) * r.cap;
    uint32_t s, e;
    wide_share((npx + 31u) >> 5, g, s, e);
    uint32_t cnt = 0;
    for (uint32_t w = s + threadIdx.x; w < e; w += kWT) cnt += __popc(bits[w]);
    uint32_t tot;
    wg_excl_add<kWT>(cnt, ws, tot);
    if (threadIdx.x == 0) r.wcnt[(static_cast<int64_t>(f) * kRefWideGroups + g) * 2] = tot;
}

__device__ __forceinline__ void refw_wprefix(const SelectArgs &a, const RefSortArgs &r, int f, int g, int) {
    __shared__ uint32_t ws[kWT / kWave];
    if (!wide_frame(a, f) || r.push_order) return;
    const uint32_t npx = static_cast<uint32_t>(a.rows) * static_cast<uint32_t>(a.cols);
    const uint32_t *bits = r.lpos + static_cast<int64_t>(f) * r.cap;
    uint32_t *wpre = r.rpos + static_cast<int64_t>(f) * r.cap;
    uint32_t base = 0;
    for (int i = 0; i < g; ++i) base += r.wcnt[(static_cast<int64_t>(f) * kRefWideGroups + i) * 2];
    uint32_t s, e;
    wide_share((npx + 31u) >> 5, g, s, e);
    // a run of consecutive words per thread
    const uint32_t per = (e - s + kWT - 1) / kWT;
    const uint32_t w0 = min(e, s + threadIdx.x * per), w1 = min(e, w0 + per);
    uint32_t cnt = 0;
    for (uint32_t w = w0; w < w1; ++w) cnt += __popc(bits[w]);
    uint32_t tot;
    uint32_t at = base + wg_excl_add<kWT>(cnt, ws, tot);
    for (uint32_t w = w0; w < w1; ++w) {
        wpre[w] = at;
        at += __popc(bits[w]);
    }
}

__device__ __forceinline__ void refw_place(const SelectArgs &a, const RefSortArgs &r, int f, int g, int) {
    if (!wide_frame(a, f) || r.push_order) return;
    const uint32_t n = r.ctl[f].n;
    const uint32_t npx = static_cast<uint32_t>(a.rows) * static_cast<uint32_t>(a.cols);
    const float *lresp = a.list_resp + static_cast<int64_t>(f) * a.list_cap;
    const uint32_t *lidx = a.list_idx + static_cast<int64_t>(f) * a.list_cap;
    uint2 *X = r.x + static_cast<int64_t>(f) * r.cap;
    const uint32_t *bits = r.lpos + static_cast<int64_t>(f) * r.cap;
    const uint32_t *wpre = r.rpos + static_cast<int64_t>(f) * r.cap;
    uint32_t s, e;
    wide_share(n, g, s, e);
    for (uint32_t i0 = s + threadIdx.x; i0 < e; i0 += kWUnroll * kWT) {
        uint32_t qv[kWUnroll], wp[kWUnroll], wb[kWUnroll];
        float rv[kWUnroll];
#pragma unroll
        for (int k = 0; k < kWUnroll; ++k) {
            const uint32_t i = min(i0 + k * kWT, e - 1u);
            qv[k] = lidx[i];
            rv[k] = lresp[i];
        }
#pragma unroll
        for (int k = 0; k < kWUnroll; ++k) {
            const uint32_t w = min(qv[k], npx - 1u) >> 5;
            wp[k] = wpre[w];
            wb[k] = bits[w];
        }
#pragma unroll
        for (int k = 0; k < kWUnroll; ++k) {
            const uint32_t q = qv[k];
            if (i0 + k * kWT >= e || q >= npx) continue;
            const uint32_t rk = wp[k] + __popc(wb[k] & ((1u << (q & 31u)) - 1u));
            if (rk < n) X[rk] = make_uint2(__float_as_uint(rv[k]), q);
        }
    }
}

// level l, step 1: the pivot, stopper counts of workgroup g's block of [1, h)
__device__ __forceinline__ void refw_lcount(const SelectArgs &a, const RefSortArgs &r, int f, int g, int l) {
    __shared__ uint32_t ws[kWT / kWave];
    if (!wide_frame(a, f)) return;
    RefCtl &C = r.ctl[f];
    if (!C.act[l]) return;
    const uint32_t h = C.h[l];
    const uint2 *X = r.x + static_cast<int64_t>(f) * r.cap;
    const uint32_t *Xr = reinterpret_cast<const uint32_t *>(X);
    const uint32_t mid = h / 2u;
    const uint2 xa = X[1], xb = X[mid], xc = X[h - 1u], x0 = X[0];
    const uint32_t ch = median_pos(as_f(xa.x), as_f(xb.x), as_f(xc.x), 1u, mid, h - 1u);
    const uint2 xch = ch == 1u ? xa : (ch == mid ? xb : xc);
    const float pv = as_f(xch.x);
    if (g == 0 && threadIdx.x == 0) {
        C.ch = ch;
        C.pv = xch.x;
        C.x0 = x0;
        C.xch = xch;
    }
    uint32_t s, e;
    wide_share(h - 1u, g, s, e);
    s += 1u;
    e += 1u;
    uint32_t cl = 0, cr = 0;
    for (uint32_t p0 = s + threadIdx.x; p0 < e; p0 += kWUnroll * kWT) {
        float rv[kWUnroll];
#pragma unroll
        for (int k = 0; k < kWUnroll; ++k) {
            const uint32_t p = min(p0 + k * kWT, e - 1u);
            rv[k] = p == ch ? as_f(x0.x) : as_f(Xr[2u * p]);
        }
#pragma unroll
        for (int k = 0; k < kWUnroll; ++k)
            if (p0 + k * kWT < e) {
                cl += rv[k] <= pv ? 1u : 0u;
                cr += rv[k] >= pv ? 1u : 0u;
            }
    }
    uint32_t tl, tr;
    wg_excl_add<kWT>(cl, ws, tl);
    wg_excl_add<kWT>(cr, ws, tr);
    if (threadIdx.x == 0) {
        r.wcnt[(static_cast<int64_t>(f) * kRefWideGroups + g) * 2] = tl;
        r.wcnt[(static_cast<int64_t>(f) * kRefWideGroups + g) * 2 + 1] = tr;
    }
}

// level l, step 2: stopper positions by rank (left stoppers from the left into lpos, right stoppers from
// the right into rpos); the block is staged in LDS a chunk at a time and each thread ranks a run of it
__device__ __forceinline__ void refw_lscatter(const SelectArgs &a, const RefSortArgs &r, int f, int g, int l) {
    __shared__ uint32_t ws[kWT / kWave];
    __shared__ uint32_t sres[kWChunk];
    if (!wide_frame(a, f)) return;
    RefCtl &C = r.ctl[f];
    if (!C.act[l]) return;
    const uint32_t h = C.h[l], ch = C.ch, x0r = C.x0.x;
    const float pv = as_f(C.pv);
    const uint32_t *Xr = reinterpret_cast<const uint32_t *>(r.x + static_cast<int64_t>(f) * r.cap);
    uint32_t *lpos = r.lpos + static_cast<int64_t>(f) * r.cap;
    uint32_t *rpos = r.rpos + static_cast<int64_t>(f) * r.cap;
    // bases of this block, totals
    uint32_t bL = 0, bR = 0, nL = 0, nR = 0;
    for (int i = 0; i < kRefWideGroups; ++i) {
        const uint32_t vl = r.wcnt[(static_cast<int64_t>(f) * kRefWideGroups + i) * 2];
        const uint32_t vr = r.wcnt[(static_cast<int64_t>(f) * kRefWideGroups + i) * 2 + 1];
        bL += i < g ? vl : 0u;
        bR += i < g ? vr : 0u;
        nL += vl;
        nR += vr;
    }
    if (g == 0 && threadIdx.x == 0) {
        C.nL = nL;
        C.nR = nR;
    }
    uint32_t s, e;
    wide_share(h - 1u, g, s, e);
    s += 1u;
    e += 1u;
    for (uint32_t cs = s; cs < e; cs += kWChunk) {
        const uint32_t len = min(static_cast<uint32_t>(kWChunk), e - cs);
        for (uint32_t j0 = threadIdx.x; j0 < len; j0 += kWUnroll * kWT) {
            uint32_t v[kWUnroll];
#pragma unroll
            for (int k = 0; k < kWUnroll; ++k) {
                const uint32_t j = min(j0 + k * kWT, len - 1u);
                v[k] = cs + j == ch ? x0r : Xr[2u * (cs + j)];
            }
#pragma unroll
            for (int k = 0; k < kWUnroll; ++k)
                if (j0 + k * kWT < len) sres[j0 + k * kWT] = v[k];
        }
        __syncthreads();
        const uint32_t per = (len + kWT - 1) / kWT;
        const uint32_t j0 = min(len, threadIdx.x * per), j1 = min(len, j0 + per);
        uint32_t cl = 0, cr = 0;
        for (uint32_t j = j0; j < j1; ++j) {
            const float rv = as_f(sres[j]);
            cl += rv <= pv ? 1u : 0u;
            cr += rv >= pv ? 1u : 0u;
        }
        uint32_t tot;
        const uint32_t ex = wg_excl_add<kWT>(cl | (cr << 16), ws, tot);  // (each field < 2^16: len <= 8192)
        uint32_t rl = bL + (ex & 0xFFFFu), rr = bR + (ex >> 16);
        for (uint32_t j = j0; j < j1; ++j) {
            const uint32_t p = cs + j;
            const float rv = as_f(sres[j]);
            const bool ls = rv <= pv, rs = rv >= pv;
            uint32_t kl = kNone, kr = kNone;
            if (ls) {
                kl = rl++;
                lpos[kl] = p;
            }
            if (rs) {
                kr = nR - 1u - rr++;
                rpos[kr] = p;
            }
            if (p == ch) {
                C.chL = kl;
                C.chR = kr;
            }
        }
        bL += tot & 0xFFFFu;
        bR += tot >> 16;
        __syncthreads();  // (sres reused by the next chunk)
    }
}

// level l, step 3: pairs k < K swapped (t_k = l_k < r_k holds exactly for k < K); the item where t
// stops holding gives K, the cut and the next level; workgroup 0 moves the pivot to position 0
__device__ __forceinline__ void refw_lswap(const SelectArgs &a, const RefSortArgs &r, int f, int g, int l) {
    if (!wide_frame(a, f)) return;
    RefCtl &C = r.ctl[f];
    if (!C.act[l]) return;
    const uint32_t h = C.h[l], ch = C.ch, nL = C.nL, nR = C.nR;
    const uint2 x0 = C.x0, xch = C.xch;
    const uint32_t mn = min(nL, nR);
    if (mn == 0u) {  // (cannot happen: the median of three leaves a stopper of each kind in [1, h))
        if (g == 0 && threadIdx.x == 0) C.bad = 1u;
        return;
    }
    uint2 *X = r.x + static_cast<int64_t>(f) * r.cap;
    const uint32_t *lpos = r.lpos + static_cast<int64_t>(f) * r.cap;
    const uint32_t *rpos = r.rpos + static_cast<int64_t>(f) * r.cap;
    uint32_t s, e;
    wide_share(mn + 1u, g, s, e);  // items k in [0, mn]
    for (uint32_t k0 = s + threadIdx.x; k0 < e; k0 += 4 * kWT) {
        uint32_t pl[4], pr[4], ql[4], qr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t k = min(k0 + u * kWT, mn - 1u);
            const uint32_t kp = k0 + u * kWT == 0u ? 0u : min(k0 + u * kWT - 1u, mn - 1u);
            pl[u] = lpos[k];
            pr[u] = rpos[k];
            ql[u] = lpos[kp];
            qr[u] = rpos[kp];
        }
        bool t[4];
        uint2 vl[4], vr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t k = k0 + u * kWT;
            t[u] = k < e && k < mn && pl[u] < pr[u];
            if (t[u]) {
                vl[u] = pl[u] == ch ? x0 : X[pl[u]];
                vr[u] = pr[u] == ch ? x0 : X[pr[u]];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t k = k0 + u * kWT;
            if (t[u]) {
                X[pl[u]] = vr[u];
                X[pr[u]] = vl[u];
            }
            const bool tp = k == 0u || ql[u] < qr[u];
            if (k < e && tp && !t[u]) {  // K = k
                uint32_t cut = k < nL ? lpos[k] : kNone;
                if (k >= 1u) cut = min(cut, qr[u]);
                const uint32_t d1 = C.dep[l] - 1u;
                if (cut == 0u || cut >= h) {  // (cannot happen: the scans stop inside the range)
                    C.bad = 1u;
                    cut = h;
                }
                C.sib_lo[l] = cut;
                C.sib_hi[l] = h;
                C.h[l + 1] = cut;
                C.dep[l + 1] = d1;
                C.act[l + 1] = l + 1 < kRefWideLevels && cut > kRefWideMin && d1 > 0u && !C.bad ? 1u : 0u;
                C.nlev = static_cast<uint32_t>(l + 1);
            }
        }
    }
    if (g == 0 && threadIdx.x == 0) {
        const uint32_t cl = C.chL, cr = C.chR;
        const bool swapped = (cl < mn && lpos[cl] < rpos[cl]) || (cr < mn && lpos[cr] < rpos[cr]);
        X[0] = xch;
        if (!swapped) X[ch] = x0;
    }
}

// the prelude kernels: workgroup (slot, g) takes flagged frames slot, slot + slots, ... of the list
#define FD_REFW_KERNEL(name)                                                                         \
    __global__ __launch_bounds__(kWT) void k_##name(SelectArgs a, RefSortArgs r, int l) {          \
        const int g = static_cast<int>(blockIdx.x % kRefWideGroups);                                \
        const uint32_t slots = gridDim.x / kRefWideGroups, cnt = r.wfr[0];                          \
        for (uint32_t j = blockIdx.x / kRefWideGroups; j < cnt; j += slots)                         \
            name(a, r, static_cast<int>(r.wfr[1 + j]), g, l);                                       \
    }
FD_REFW_KERNEL(refw_clear)
FD_REFW_KERNEL(refw_bits)
FD_REFW_KERNEL(refw_wcount)
FD_REFW_KERNEL(refw_wprefix)
FD_REFW_KERNEL(refw_place)
FD_REFW_KERNEL(refw_lcount)
FD_REFW_KERNEL(refw_lscatter)
FD_REFW_KERNEL(refw_lswap)
#undef FD_REFW_KERNEL

}  // namespace

hipError_t launch_ref_prelude(const SelectArgs &a, const RefSortArgs &r, int batch, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>(std::min(batch, kRefWideSlots)) * kRefWideGroups), blk(kWT);
    hipError_t e = hipMemsetAsync(r.wfr, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_refw_init, dim3(static_cast<unsigned>(batch)), blk, 0, s, a, r);
    if (!r.push_order) hipLaunchKernelGGL(k_refw_clear, grid, blk, 0, s, a, r, 0);
    hipLaunchKernelGGL(k_refw_bits, grid, blk, 0, s, a, r, 0);
    if (!r.push_order) {
        hipLaunchKernelGGL(k_refw_wcount, grid, blk, 0, s, a, r, 0);
        hipLaunchKernelGGL(k_refw_wprefix, grid, blk, 0, s, a, r, 0);
        hipLaunchKernelGGL(k_refw_place, grid, blk, 0, s, a, r, 0);
    }
    for (int l = 0; l < kRefWideLevels; ++l) {
        hipLaunchKernelGGL(k_refw_lcount, grid, blk, 0, s, a, r, l);
        hipLaunchKernelGGL(k_refw_lscatter, grid, blk, 0, s, a, r, l);
        hipLaunchKernelGGL(k_refw_lswap, grid, blk, 0, s, a, r, l);
    }
    return hipSuccess;
}

}  // namespace fdk
