// Device code shared by the two matchers (fd_match.hip, fd_nn_match.hip): a frame's entry count and the
// epilogue that turns a lane's (best, second) into the outputs.
// The count helpers also serve the other per-keypoint kernels (fd_brief.hip, fd_nn.hip, fd_flow.hip, fd_refine.hip).
#pragma once

#include "fd_device.h"
#include "fd_kernels.h"

namespace fdk {

// A count word without fd_points_detect's guard flags (bits 25..31).
__device__ __forceinline__ int count_word(int32_t w) { return static_cast<int>(static_cast<uint32_t>(w) & kCountMask); }

// Entries of frame f: its count word, at most stride; stride without counts.
__device__ __forceinline__ int frame_count(const int32_t *counts, int f, int stride) {
    return counts ? min(count_word(counts[f]), stride) : stride;
}

// The end of both matchers (Args: MatchArgs with D = int, NnMatchArgs with D = float), per lane: entry q
// of frame f (slot aslot; `live`: it exists) has the raw best index `raw` (-1 without a first distance)
// and the distances d1 / d2 (-1 where has1 / has2 is false). The best is accepted if it passes the
// distance bound, the ratio test (ratio_ok: the kernel's own verdict on d1 against d2, used only with the
// test on and a second distance present) and the cross-check's reverse table. Writes out_idx and out_dist
// of the live lanes and adds the wave's accepted entries to out_counts[f].
template <typename D, typename Args>
__device__ __forceinline__ void match_emit(const Args &a, int f, int q, int64_t aslot, bool live, bool has1, bool has2,
                                           D d1, D d2, int raw, bool ratio_ok) {
    bool ok = has1;
    if (ok && a.max_distance >= D(0) && d1 > a.max_distance) ok = false;
    if (ok && a.max_ratio > 0.0f && has2 && !ratio_ok) ok = false;
    if (ok && a.rev && a.rev[static_cast<int64_t>(f) * a.b_stride + raw] != q) ok = false;
    if (live) {
        a.out_idx[aslot] = ok ? raw : -1;
        if (a.out_dist) {
            a.out_dist[2 * aslot] = d1;
            a.out_dist[2 * aslot + 1] = d2;
        }
    }
    if (a.out_counts) {
        const int n_ok = popc64(ballot(ok));
        if (lane_id() == 0 && n_ok) atomicAdd(a.out_counts + f, n_ok);
    }
}

}  // namespace fdk
