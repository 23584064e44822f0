// Producer side of the selection's list format (fdk::CandList, fd_kernels.h), shared by every kernel that
// emits candidates (k_corner, k_fast, k_corner_lp, k_heat_candidates, k_cand_lists): the key map, the
// workgroup's LDS level-0 histogram, a frame's view of the lists, a wave's append and the sorted-segment
// flush. k_select / k_gather / k_wide_gather / k_select_reference read what these write.
#pragma once

#include "fd_device.h"
#include "fd_kernels.h"

namespace fdk {

// Selection key: the response through the frame's key map (order-preserving, injective on the
// candidates' response range; see CandList::key_base), then ~idx so that equal responses order by
// ascending raster index (tie_idx_desc: idx, descending, SuperPoint's multimap walk order).
__device__ __forceinline__ uint32_t sel_key32(float resp, uint32_t key_base, int key_lz) {
    return (float_key(resp) - key_base) << key_lz;
}
__device__ __forceinline__ uint64_t sel_key64(float resp, uint32_t idx, uint32_t key_base, int key_lz, int tie_desc) {
    return (static_cast<uint64_t>(sel_key32(resp, key_base, key_lz)) << 32) | static_cast<uint64_t>(tie_desc ? idx : ~idx);
}
// Level-0 bin (hist0's index): the key's top 12 bits.
__device__ __forceinline__ uint32_t level0_bin(float resp, uint32_t key_base, int key_lz) {
    return sel_key32(resp, key_base, key_lz) >> 20;
}
// The inverse at a bin's lower edge: float_key of the lowest response that maps to level-0 bin `bin`.
__device__ __forceinline__ uint32_t level0_floor_key(uint32_t bin, uint32_t key_base, int key_lz) {
    return key_base + ((bin << 20) >> key_lz);
}

// Frame f's part of the lists.
struct ListFrame {
    float *resp;
    uint32_t *idx;
    int64_t cap;
};
__device__ __forceinline__ ListFrame list_frame(const CandList &l, int f) {
    return {l.resp + static_cast<int64_t>(f) * l.cap, l.idx + static_cast<int64_t>(f) * l.cap, l.cap};
}

// (the per-pixel kernels run 256-thread workgroups: a constant stride, no blockDim load -- whose wait
// would also hold for every vector-memory operation in flight, e.g. seg_list_flush's returning atomic)
constexpr int kPixWg = 256;
// LDS accesses all issued before any is used (the histogram loops were chains of one LDS round trip,
// and in the flush one exec-masked branch, per bin group); the clear by 16-byte stores (h is 16-byte
// aligned in every LDS layout: DetectLdsT, LpLds, k_heat_candidates, k_cand_lists).
// (WG: the workgroup's threads, for the kernels that run another size than kPixWg)
template <int WG = kPixWg>
__device__ __forceinline__ void hist_clear(uint32_t *h) {
    constexpr int kHistPer = kHistBins / (4 * WG);  // uint4 groups per thread
    uint4 *h4 = reinterpret_cast<uint4 *>(h);
#pragma unroll
    for (int k = 0; k < kHistPer; ++k) h4[threadIdx.x + k * WG] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
}
// The flush keeps one bin per lane per atomic instruction (64 consecutive dwords: a 4-dwords-per-lane
// pattern spreads each wave instruction over 4x the 64-B atomic requests, measured +4.9 us at batch 1).
template <int WG = kPixWg>
__device__ __forceinline__ void hist_flush(const uint32_t *h, uint32_t *g) {
    __syncthreads();
    constexpr int kPer = kHistBins / WG;
    uint32_t v[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) v[k] = h[threadIdx.x + k * WG];
#pragma unroll
    for (int k = 0; k < kPer; ++k)
        if (v[k]) atomicAdd(&g[threadIdx.x + k * WG], v[k]);
}

// Append the n (wave-uniform) candidates a wave staged in LDS to frame f's list: one returning atomic
// by lane 0, then a strided copy (entries past the capacity are dropped; the count keeps growing, the
// selection clamps it). hist (LDS, or null): the level-0 histogram is counted here, once per staged
// candidate, rather than where the candidates are found.
__device__ __forceinline__ void wave_append(const CandList &l, int f, const float *sr, const uint32_t *si, int n,
                                            uint32_t *hist) {
    uint32_t base = 0;
    if (lane_id() == 0) base = atomicAdd(&l.count[f], static_cast<uint32_t>(n));
    base = __builtin_amdgcn_readfirstlane(base);
    const ListFrame d = list_frame(l, f);
    for (int i = lane_id(); i < n; i += kWave) {
        const float r = sr[i];
        if (hist) atomicAdd(&hist[level0_bin(r, l.key_base, l.key_lz)], 1u);
        const int64_t pos = static_cast<int64_t>(base) + i;
        if (pos < d.cap) {
            d.resp[pos] = r;
            d.idx[pos] = si[i];
        }
    }
}

// Sorted-segment flush (PointsArgs::segdesc; small launches whose tiles never overflow the staging):
// the workgroup's candidates, all still staged in LDS, go to the frame's list as one contiguous
// segment ordered by level-0 bin, descending (a counting sort on the workgroup's LDS histogram `hist`),
// and the segment is described in segdesc[f][g] (g: the workgroup's place in its frame). k_select then
// reads only each segment's prefix at or above its first-chunk cut (a few entries per workgroup) instead
// of scanning the whole list. Every thread of the workgroup calls it. Src is where the entries are staged:
//   n             this lane's staged entries (zeroed here)
//   wave_total()  the wave's staged entries (wave-uniform)
//   visit(fn)     fn(response, raster index) for each of this lane's entries
//   counted()     the entries are in `hist` already (counted when they were staged)
//   flush(a, f)   the source's plain append (the wave's entries and their histogram counts)
template <int WG = kPixWg, class Src>
__device__ __forceinline__ void seg_list_flush(Src &src, const PointsArgs &a, int f, int g, bool active, uint32_t *hist,
                                               const uint32_t *ovf, uint32_t (&wtot)[WG / kWave], uint32_t &wg_base) {
    constexpr int kWaves = WG / kWave;
    const int tid = threadIdx.x, lane = lane_id(), wv = tid >> 6;
    if (!active) src.n = 0;
    const uint32_t wn = src.wave_total();
    if (lane == 0) wtot[wv] = wn;
    __syncthreads();
    if (*ovf) {  // part of the workgroup's list is already out unsorted: plain flush (frame marked)
        if (active) src.flush(a, f);
        hist_flush<WG>(hist, a.list.hist0 + static_cast<int64_t>(f) * kHistBins);
        return;
    }
    // The segment's place in the list: one returning atomic, issued before the histogram work so that
    // its round trip overlaps the counting sort's scan (thread 0 waits for it only at its LDS store).
    uint32_t seg_base_early = 0;
    uint32_t seg_total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
#pragma unroll
    for (int q = 4; q < kWaves; ++q) seg_total += wtot[q];
    if (tid == 0 && seg_total) seg_base_early = atomicAdd(&a.list.count[f], seg_total);
    const uint32_t kb = a.list.key_base;
    const int lz = a.list.key_lz;
    if (!src.counted()) src.visit([&](float r, uint32_t) { atomicAdd(&hist[level0_bin(r, kb, lz)], 1u); });
    hist_flush<WG>(hist, a.list.hist0 + static_cast<int64_t>(f) * kHistBins);  // (leads with a barrier)
    __syncthreads();
    // in place: hist[b] = entries of bins above b (exclusive scan in descending bin order)
    constexpr int kPer = kHistBins / WG;
    uint32_t v[kPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) sum += (v[k] = hist[kHistBins - 1 - (tid * kPer + k)]);
    const uint32_t incl = wave_incl_add(sum);
    if (lane == kWave - 1) wtot[wv] = incl;
    __syncthreads();
    uint32_t run = incl - sum, total = 0;
    for (int q = 0; q < kWaves; ++q) {
        run += q < wv ? wtot[q] : 0u;
        total += wtot[q];
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        hist[kHistBins - 1 - (tid * kPer + k)] = run;
        run += v[k];
    }
    const int64_t seg = static_cast<int64_t>(f) * a.blocks_per_frame + g;
    if (tid == 0) {
        wg_base = seg_base_early;
        a.segdesc[seg] = make_uint2(wg_base, total);
    }
    __syncthreads();
    const ListFrame d = list_frame(a.list, f);
    const int64_t base = wg_base;
    uint64_t *head = a.seghead + seg * kSegHead;
    src.visit([&](float r, uint32_t id) {
        const uint32_t lp = atomicAdd(&hist[level0_bin(r, kb, lz)], 1u);
        const int64_t pos = base + lp;
        if (pos < d.cap) {
            d.resp[pos] = r;
            d.idx[pos] = id;
        }
        // the segment's head as selection keys (ascending-index ties): k_select's first read, no list hop
        if (lp < static_cast<uint32_t>(kSegHead)) head[lp] = sel_key64(r, id, kb, lz, 0);
    });
    src.n = 0;
}

}  // namespace fdk
