// Nearest-neighbour Hamming matcher for BRIEF descriptors (fd_brief_match, an MI355X extension: the
// reference has no matcher) for gfx950.
//
// One kernel serves both directions. Its "a" side is the set whose entries get an answer, its "b" side
// the set that is searched: the forward pass has a = query, b = train; the cross-check's reverse pass has
// a = train, b = query and writes only the raw best index into a workspace table, which the forward pass
// then reads once per accepted candidate.
//
// Layout: a workgroup of 4 waves covers 64 "a" descriptors of one frame. Every lane owns one of them and
// keeps its words in VGPRs (lane l of each of the 4 waves owns the same descriptor). The frame's "b"
// descriptors go through LDS in tiles of 256; wave w scans entries w, w + 4, w + 8, ... of a tile, so the
// four waves share a tile's work evenly whatever its fill, and every lane of a wave reads the same LDS
// address each step (a broadcast, no bank conflicts). Per pair: NW xor + popcount-accumulate, then the
// update of (best, best index, second). The four partial results are merged exactly by wave 0.
//
// Exactness. Within a wave the scan is in ascending index order with a strict `<`, so equal distances
// keep the lowest index; the merge takes the lexicographic minimum of (distance, index), which is that
// same rule for any partition of the indices. The second distance is a value only (the smallest
// distance to an entry with another index than the best): per update second = min(second, max(d, best)),
// per merge the minimum of both seconds and the losing best.
//
// Validity costs nothing per pair: an invalid "b" entry starts its popcount sum at kInvalidPenalty
// instead of 0 (a word per entry in LDS), so it loses against every valid entry (distance <= 256), and
// a result >= kInvalidPenalty means "absent". Bits above `length` are masked on both sides, once: the
// lane's own words when they are loaded, the "b" words when a tile is filled.
//
// The GATED instances (fd_brief_match_guided) add the search window: a lane keeps its own entry's (x, y)
// in two registers, a tile's 256 "b" positions go to LDS beside the words (2 KiB, read as the same
// broadcast), and a pair outside the window takes the invalid entry's route: its popcount sum starts at
// kInvalidPenalty. Per pair that is two subtractions, two compares and a select; the update and the merge
// do not know of it. |b - a| has the same bits as |a - b|, so the reverse pass decides on the same pairs.
//
// The model instances (fd_brief_match_model; kGateF, kGateHFwd, kGateHRev of fd_match_gate.h) add the
// epipolar band or the transfer disc to the window. k_match_gate_vectors (below) first writes four doubles
// per entry of both sets; a lane keeps its own entry's four in registers, a tile's go to LDS beside the
// positions (8 KiB, the same broadcast read), and a failing pair takes the same route as one outside the
// window. Per pair that is 8 (F) or 7 (H) double operations and a compare.
#include "fd_match_common.h"
#include "fd_match_gate.h"

namespace fdk {
namespace {

constexpr int kMatchWaves = 4;
constexpr int kMatchThreads = kMatchWaves * kWave;
constexpr int kMatchTile = kMatchThreads;  // "b" entries per LDS tile (one valid flag per thread)
constexpr int kInvalidPenalty = 1 << 20;
constexpr int kAbsent = 0x7FFFFFFF;

// NW: descriptor words held per lane and per LDS row (words above ceil(length / 32) are zero).
// GATE (fd_match_gate.h): from kGateWindow on only "b" entries inside the lane's window are candidates
// (a.a_xy, a.b_xy, a.radius_x / _y), from kGateF on only those that pass the model test as well (a.a_gate,
// a.b_gate, a.gate_tt).
template <int NW, int GATE>
__global__ __launch_bounds__(kMatchThreads) void k_brief_match(MatchArgs a) {
    constexpr bool GATED = GATE != kGateNone, MODEL = GATE >= kGateF;
    __shared__ __attribute__((aligned(16))) uint32_t tile[kMatchTile * NW];
    __shared__ uint32_t pen[kMatchTile];
    __shared__ float bxy[GATED ? 2 * kMatchTile : 1];
    __shared__ __attribute__((aligned(16))) double bgv[MODEL ? 4 * kMatchTile : 2];
    __shared__ int32_t part[3][kMatchWaves - 1][kWave];
    const int tiles = (a.a_stride + kWave - 1) / kWave;
    const int f = static_cast<int>(blockIdx.x) / tiles;
    const int q0 = (static_cast<int>(blockIdx.x) - f * tiles) * kWave;
    const int na = frame_count(a.a_counts, f, a.a_stride);
    if (q0 >= na) return;  // (the whole workgroup: nothing of this frame is read or written)
    const int nb = frame_count(a.b_counts, f, a.b_stride);
    const int lane = lane_id();
    const int wave = static_cast<int>(threadIdx.x) >> 6;
    const int nw = (a.length + 31) >> 5;
    const uint32_t tail = (a.length & 31) ? (1u << (a.length & 31)) - 1u : ~0u;
    const int q = q0 + lane;
    const bool live = q < na;
    const int64_t aslot = static_cast<int64_t>(f) * a.a_stride + q;
    uint32_t qw[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        qw[w] = (live && w < nw) ? a.a_bits[aslot * nw + w] : 0u;
        if (w == nw - 1) qw[w] &= tail;
    }
    float ax = 0.0f, ay = 0.0f;
    const float *bp = nullptr;
    if constexpr (GATED) {
        if (live) {
            ax = a.a_xy[2 * aslot];
            ay = a.a_xy[2 * aslot + 1];
        }
        bp = a.b_xy + static_cast<int64_t>(f) * a.b_stride * 2;
    }
    double ag[4] = {0.0, 0.0, 0.0, 0.0};
    const double *bg = nullptr;
    if constexpr (MODEL) {
        if (live) {
#pragma unroll
            for (int k = 0; k < 4; ++k) ag[k] = a.a_gate[4 * aslot + k];
        }
        bg = a.b_gate + static_cast<int64_t>(f) * a.b_stride * 4;
    }
    const uint32_t *bb = a.b_bits + static_cast<int64_t>(f) * a.b_stride * nw;
    const uint8_t *bv = a.b_valid ? a.b_valid + static_cast<int64_t>(f) * a.b_stride : nullptr;
    int best = kAbsent, second = kAbsent, bidx = -1;
    for (int t0 = 0; t0 < nb; t0 += kMatchTile) {
        const int n = min(kMatchTile, nb - t0);
        __syncthreads();  // every wave is done with the previous tile
        for (int i = static_cast<int>(threadIdx.x); i < n * NW; i += kMatchThreads) {
            const int r = i / NW, w = i % NW;
            uint32_t v = w < nw ? bb[static_cast<int64_t>(t0 + r) * nw + w] : 0u;
            if (w == nw - 1) v &= tail;
            tile[i] = v;
        }
        if (static_cast<int>(threadIdx.x) < n)
            pen[threadIdx.x] = (bv && !bv[t0 + threadIdx.x]) ? static_cast<uint32_t>(kInvalidPenalty) : 0u;
        if constexpr (GATED) {
            for (int i = static_cast<int>(threadIdx.x); i < 2 * n; i += kMatchThreads)
                bxy[i] = bp[static_cast<int64_t>(t0) * 2 + i];
        }
        if constexpr (MODEL) {
            for (int i = static_cast<int>(threadIdx.x); i < 4 * n; i += kMatchThreads)
                bgv[i] = bg[static_cast<int64_t>(t0) * 4 + i];
        }
        __syncthreads();
#pragma unroll 2
        for (int j = wave; j < n; j += kMatchWaves) {
            uint32_t d = pen[j];
            if constexpr (GATED) {
                // one subtraction and one inclusive compare per axis; a NaN fails both
                const bool in = fabsf(bxy[2 * j] - ax) <= a.radius_x && fabsf(bxy[2 * j + 1] - ay) <= a.radius_y;
                d = in ? d : static_cast<uint32_t>(kInvalidPenalty);
            }
            if constexpr (MODEL) {
                const double og[4] = {bgv[4 * j], bgv[4 * j + 1], bgv[4 * j + 2], bgv[4 * j + 3]};
                d = model_pass<GATE>(ag, og, a.gate_tt) ? d : static_cast<uint32_t>(kInvalidPenalty);
            }
#pragma unroll
            for (int w = 0; w < NW; ++w) d += static_cast<uint32_t>(__popc(qw[w] ^ tile[j * NW + w]));
            const int di = static_cast<int>(d);
            second = min(second, max(di, best));
            bidx = di < best ? t0 + j : bidx;
            best = min(best, di);
        }
    }
    if (wave) {
        part[0][wave - 1][lane] = best;
        part[1][wave - 1][lane] = bidx;
        part[2][wave - 1][lane] = second;
    }
    __syncthreads();
    if (wave) return;
    for (int w = 0; w < kMatchWaves - 1; ++w) {
        const int ob = part[0][w][lane], oi = part[1][w][lane], os = part[2][w][lane];
        const bool take = ob < best || (ob == best && oi < bidx);
        second = min(min(second, os), take ? best : ob);
        if (take) {
            best = ob;
            bidx = oi;
        }
    }
    const bool avalid = live && (!a.a_valid || a.a_valid[aslot]);
    const int d1 = (avalid && best < kInvalidPenalty) ? best : -1;
    const int d2 = (avalid && second < kInvalidPenalty) ? second : -1;
    // the ratio rule: one float multiply and one compare (the file is built without contraction)
    match_emit(a, f, q, aslot, live, d1 >= 0, d2 >= 0, d1, d2, d1 >= 0 ? bidx : -1,
               static_cast<float>(d1) < a.max_ratio * static_cast<float>(d2));
}

template <int NW>
void launch_nw(const MatchArgs &a, unsigned blocks, hipStream_t s) {
    switch (gate_of(a)) {
        case kGateNone: hipLaunchKernelGGL((k_brief_match<NW, kGateNone>), dim3(blocks), dim3(kMatchThreads), 0, s, a); break;
        case kGateWindow: hipLaunchKernelGGL((k_brief_match<NW, kGateWindow>), dim3(blocks), dim3(kMatchThreads), 0, s, a); break;
        case kGateF: hipLaunchKernelGGL((k_brief_match<NW, kGateF>), dim3(blocks), dim3(kMatchThreads), 0, s, a); break;
        case kGateHFwd: hipLaunchKernelGGL((k_brief_match<NW, kGateHFwd>), dim3(blocks), dim3(kMatchThreads), 0, s, a); break;
        default: hipLaunchKernelGGL((k_brief_match<NW, kGateHRev>), dim3(blocks), dim3(kMatchThreads), 0, s, a); break;
    }
}

// The gate vector of every slot of both sets (side 0: query, side 1: train), one lane per slot. Slots past a
// frame's count get one too (their positions are read, whatever they hold): the matchers never read it.
__global__ __launch_bounds__(256) void k_match_gate_vectors(MatchGateArgs a) {
    const int64_t n0 = static_cast<int64_t>(a.batch) * a.stride[0], n1 = static_cast<int64_t>(a.batch) * a.stride[1];
    int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n0 + n1) return;
    const int side = i >= n0;
    if (side) i -= n0;
    const double *M = a.m + 9 * (i / a.stride[side]);
    const double x = static_cast<double>(a.xy[side][2 * i]), y = static_cast<double>(a.xy[side][2 * i + 1]);
    double v0, v1, v2, v3;
    if (a.model == 0) {
        if (side == 0) {
            v0 = (M[0] * x + M[1] * y) + M[2];
            v1 = (M[3] * x + M[4] * y) + M[5];
            v2 = (M[6] * x + M[7] * y) + M[8];
            v3 = v0 * v0 + v1 * v1;
        } else {
            const double m0 = (M[0] * x + M[3] * y) + M[6];
            const double m1 = (M[1] * x + M[4] * y) + M[7];
            v0 = x;
            v1 = y;
            v2 = 1.0;
            v3 = m0 * m0 + m1 * m1;
        }
    } else if (side == 0) {
        v0 = (M[0] * x + M[1] * y) + M[2];
        v1 = (M[3] * x + M[4] * y) + M[5];
        v2 = (M[6] * x + M[7] * y) + M[8];
        v3 = a.tt * (v2 * v2);
    } else {
        v0 = x;
        v1 = y;
        v2 = 0.0;
        v3 = 0.0;
    }
    double *o = a.out[side] + 4 * i;
    o[0] = v0;
    o[1] = v1;
    o[2] = v2;
    o[3] = v3;
}

}  // namespace

hipError_t launch_brief_match(const MatchArgs &a, hipStream_t s) {
    const int64_t blocks = static_cast<int64_t>(a.batch) * ((a.a_stride + kWave - 1) / kWave);
    if (blocks == 0) return hipSuccess;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    const int nw = (a.length + 31) / 32;
    const unsigned g = static_cast<unsigned>(blocks);
    if (nw <= 1)
        launch_nw<1>(a, g, s);
    else if (nw <= 2)
        launch_nw<2>(a, g, s);
    else if (nw <= 4)
        launch_nw<4>(a, g, s);
    else
        launch_nw<8>(a, g, s);
    return hipGetLastError();
}

hipError_t launch_match_gate_vectors(const MatchGateArgs &a, hipStream_t s) {
    const int64_t total = static_cast<int64_t>(a.batch) * (static_cast<int64_t>(a.stride[0]) + a.stride[1]);
    if (total == 0) return hipSuccess;
    const int64_t blocks = (total + 255) / 256;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_match_gate_vectors, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace fdk
