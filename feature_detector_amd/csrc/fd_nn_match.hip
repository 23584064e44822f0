// Nearest-neighbour squared-L2 matcher for NN float descriptors (fd_nn_match, an MI355X extension: the
// reference has no matcher) for gfx950, on the f32-input MFMA.
//
// The distance is a definite float sequence (include/fd_hip.h): dot(q, t) and the norms are fmaf chains
// with k ascending, d = fmaxf(0, (n(q) + n(t)) - 2 * dot). v_mfma_f32_16x16x4_f32 computes, per output
// element, D = fma(a_k3, b_k3, fma(a_k2, b_k2, fma(a_k1, b_k1, fma(a_k0, b_k0, C)))) with one rounding
// per product, so one accumulator per output pair, fed K steps 0, 1, 2, ... in order, is that chain. K
// is never split across accumulators; the dependent-accumulator latency (40 cycles against a 32-cycle
// issue) is covered by the independent 16-column sub-tiles of an LDS tile.
//
// Two kernels. k_nn_norms: one lane per descriptor, the plain fmaf chain n(x), +inf for a descriptor
// that is flagged invalid. The +inf carries validity through k_nn_match at no cost per pair: an invalid
// "b" entry has distance +inf and loses every `<`, an invalid "a" entry has only +inf distances, and
// +inf is written as "absent" (-1). (A descriptor whose squared norm is not finite is therefore treated
// as invalid; non-finite inputs are unspecified.)
//
// k_nn_match serves both directions like k_brief_match: the "a" side gets answers, the "b" side is
// searched; the cross-check's reverse pass has a = train, b = query and writes only the raw best index.
// A workgroup of 4 waves covers 64 "a" descriptors of one frame, wave w rows 16w .. 16w + 15, whose A
// fragments stay in VGPRs for the whole K (lane l: row l & 15, k = 4s + (l >> 4) of step s: K / 4
// registers). The frame's "b" descriptors go through LDS in tiles of TB rows, filled with 16-byte loads
// and stores; the row pitch K + 4 floats puts the 64 lanes of a B-fragment read (row l & 15, k = 4s +
// (l >> 4)) on the 64 banks 4 (l & 15) + (l >> 4). Every wave scans the whole tile for its own rows, so
// no merge between waves is needed. C/D: lane l holds column l & 15 of rows 4 (l >> 4) + 0..3, so a lane
// keeps (best, index, second) for four rows over the columns congruent to l & 15; columns ascend within
// a lane, and the final merge over the 16 lanes that share the rows is the lexicographic minimum of
// (distance, index), which is the serial scan's rule for any partition of the indices (fd_match.hip).
//
// The GATED instances (fd_nn_match_guided) add the search window of fd_match.hip: a lane keeps the
// positions of its four rows (8 registers), a tile's TB "b" positions go to LDS beside bnorm, and a pair
// outside the window gets d = +inf where an invalid column already does, after the MFMA chain, which the
// gate does not touch.
//
// The model instances (fd_nn_match_model; kGateF, kGateHFwd, kGateHRev of fd_match_gate.h) add the model
// test on the gate vectors of k_match_gate_vectors (fd_match.hip). Four rows of four doubles per lane do not
// fit beside the A fragments (the K = 256 window instance already sits at the 128 registers of 4 waves per
// SIMD), so the workgroup's 64 "a" vectors and positions go to LDS once (2.5 KiB) and a tile's TB "b" vectors
// beside the positions (TB * 32 bytes); a pair reads both from there (lanes that share a row or a column read the same
// address). The test runs per tile ahead of the MFMA chain, one bit per pair into a mask register, and a
// failing pair gets d = +inf like one outside the window.
#include "fd_match_common.h"
#include "fd_match_gate.h"

namespace fdk {
namespace {

constexpr int kNnWaves = 4;
constexpr int kNnThreads = kNnWaves * kWave;
constexpr int kNnRows = 16 * kNnWaves;  // "a" descriptors per workgroup

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4 load4(const float *p, bool vec) {
    if (vec) return *reinterpret_cast<const f4 *>(p);
    return f4{p[0], p[1], p[2], p[3]};
}

// n(x) of every descriptor in slots < counts[f] of both sets (side 0, then side 1); +inf when flagged invalid.
__global__ __launch_bounds__(256) void k_nn_norms(NnNormArgs a) {
    const int64_t n0 = static_cast<int64_t>(a.batch) * a.stride[0], n1 = static_cast<int64_t>(a.batch) * a.stride[1];
    int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n0 + n1) return;
    const int side = i >= n0;
    if (side) i -= n0;
    const int stride = a.stride[side];
    const int f = static_cast<int>(i / stride);
    if (static_cast<int>(i - static_cast<int64_t>(f) * stride) >= frame_count(a.counts[side], f, stride)) return;
    const float *p = a.desc[side] + i * a.dim;
    const bool vec = a.vec[side];
    float acc = 0.0f;
    for (int k = 0; k < a.dim; k += 4) {
        const f4 v = load4(p + k, vec);
        acc = __builtin_fmaf(v.x, v.x, acc);
        acc = __builtin_fmaf(v.y, v.y, acc);
        acc = __builtin_fmaf(v.z, v.z, acc);
        acc = __builtin_fmaf(v.w, v.w, acc);
    }
    const bool valid = !a.valid[side] || a.valid[side][i];
    a.out[side][i] = valid ? acc : __builtin_inff();
}

// K: the instance's descriptor length (dim zero-padded up to it: fmaf(0, 0, acc) leaves acc unchanged);
// TB: "b" rows per LDS tile (TB / 16 independent accumulators per wave); GATE (fd_match_gate.h): from
// kGateWindow on only "b" rows inside a row's window are candidates (a.a_xy, a.b_xy, a.radius_x / _y), from
// kGateF on only those that pass the model test as well (a.a_gate, a.b_gate, a.gate_tt).
// The gated instances ask for the ungated ones' 4 waves per SIMD (the LDS tile's limit): unasked, the
// K = 256 one takes 132 registers and drops to 3. The model instances ask for 3: capped at the 128 registers
// of 4 they spill a few loop-invariant addresses (4 to 14 registers too many), which they must not.
template <int K, int TB, int GATE>
__global__ __launch_bounds__(kNnThreads) __attribute__((amdgpu_waves_per_eu(GATE >= kGateF ? 3 : GATE != kGateNone ? 4 : 1))) void k_nn_match(NnMatchArgs a) {
    constexpr bool GATED = GATE != kGateNone, MODEL = GATE >= kGateF;
    constexpr int P = K + 4, NS = K / 4, NJ = TB / 16, C4 = K / 4;
    __shared__ __attribute__((aligned(16))) float tile[TB * P];
    __shared__ float bnorm[TB];
    __shared__ __attribute__((aligned(8))) float bxy[GATED ? 2 * TB : 2];
    __shared__ __attribute__((aligned(16))) double agv[MODEL ? 4 * kNnRows : 2];
    __shared__ __attribute__((aligned(8))) float axy[MODEL ? 2 * kNnRows : 2];
    __shared__ __attribute__((aligned(16))) double bgv[MODEL ? 4 * TB : 2];
    const int tiles = (a.a_stride + kNnRows - 1) / kNnRows;
    const int f = static_cast<int>(blockIdx.x) / tiles;
    const int q0 = (static_cast<int>(blockIdx.x) - f * tiles) * kNnRows;
    const int na = frame_count(a.a_counts, f, a.a_stride);
    if (q0 >= na) return;  // (the whole workgroup: nothing of this frame is read or written)
    const int nb = frame_count(a.b_counts, f, a.b_stride);
    const int lane = lane_id();
    const int wave = static_cast<int>(threadIdx.x) >> 6;
    const int c = lane & 15, g = lane >> 4;
    const float inf = __builtin_inff();

    // A fragments of the wave's 16 rows, and the norms of the four rows this lane holds results of
    float af[NS];
    {
        const int row = q0 + 16 * wave + c;
        const float *ap = a.a_desc + (static_cast<int64_t>(f) * a.a_stride + min(row, na - 1)) * a.dim;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int k = 4 * s + g;
            af[s] = (row < na && k < a.dim) ? ap[k] : 0.0f;
        }
    }
    float an[4], best[4], second[4];
    int bidx[4];
    float ax[4], ay[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = q0 + 16 * wave + 4 * g + r;
        an[r] = row < na ? a.a_norm[static_cast<int64_t>(f) * a.a_stride + row] : inf;
        if constexpr (GATED && !MODEL) {
            const float *ap = a.a_xy + (static_cast<int64_t>(f) * a.a_stride + min(row, na - 1)) * 2;
            ax[r] = ap[0];
            ay[r] = ap[1];
        }
        best[r] = inf;
        second[r] = inf;
        bidx[r] = -1;
    }

    const float *bf = a.b_desc + static_cast<int64_t>(f) * a.b_stride * a.dim;
    const float *bnf = a.b_norm + static_cast<int64_t>(f) * a.b_stride;
    const float *bpf = GATED ? a.b_xy + static_cast<int64_t>(f) * a.b_stride * 2 : nullptr;
    const double *bgf = MODEL ? a.b_gate + static_cast<int64_t>(f) * a.b_stride * 4 : nullptr;
    if constexpr (MODEL) {  // (the first tile's barriers order these stores before the first read; nb == 0 reads none)
        const int64_t row0 = static_cast<int64_t>(f) * a.a_stride + q0;
        const int rows = min(kNnRows, na - q0);
        if (static_cast<int>(threadIdx.x) < 4 * rows) agv[threadIdx.x] = a.a_gate[4 * row0 + threadIdx.x];
        if (static_cast<int>(threadIdx.x) < 2 * rows) axy[threadIdx.x] = a.a_xy[2 * row0 + threadIdx.x];
    }
    for (int t0 = 0; t0 < nb; t0 += TB) {
        const int n = min(TB, nb - t0);
        __syncthreads();  // every wave is done with the previous tile
        for (int i = static_cast<int>(threadIdx.x); i < n * C4; i += kNnThreads) {
            const int r = i / C4, k = (i % C4) * 4;
            f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (k < a.dim) v = load4(bf + static_cast<int64_t>(t0 + r) * a.dim + k, a.b_vec);
            *reinterpret_cast<f4 *>(&tile[r * P + k]) = v;
        }
        if (static_cast<int>(threadIdx.x) < TB)
            bnorm[threadIdx.x] = static_cast<int>(threadIdx.x) < n ? bnf[t0 + threadIdx.x] : inf;
        if constexpr (GATED) {  // (positions past the fill stay stale: their norm is +inf)
            if (static_cast<int>(threadIdx.x) < 2 * n) bxy[threadIdx.x] = bpf[static_cast<int64_t>(t0) * 2 + threadIdx.x];
        }
        if constexpr (MODEL) {  // (likewise stale past the fill)
            if (static_cast<int>(threadIdx.x) < 4 * n) bgv[threadIdx.x] = bgf[static_cast<int64_t>(t0) * 4 + threadIdx.x];
        }
        __syncthreads();
        // the window and the model test of the lane's 4 x NJ pairs, before the MFMA chain (while no accumulator
        // is live): bit 4j + r for row r against column 16j + c. One row at a time keeps the doubles few.
        uint32_t pass = 0u;
        if constexpr (MODEL) {
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
                const double *ap = agv + 4 * (16 * wave + 4 * g + r);
                const double ag[4] = {ap[0], ap[1], ap[2], ap[3]};
                const float rx = axy[2 * (16 * wave + 4 * g + r)], ry = axy[2 * (16 * wave + 4 * g + r) + 1];
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const double *bp = bgv + 4 * (16 * j + c);
                    const double og[4] = {bp[0], bp[1], bp[2], bp[3]};
                    const bool in = fabsf(bxy[2 * (16 * j + c)] - rx) <= a.radius_x && fabsf(bxy[2 * (16 * j + c) + 1] - ry) <= a.radius_y;
                    pass |= (in && model_pass<GATE>(ag, og, a.gate_tt) ? 1u : 0u) << (4 * j + r);
                }
            }
        }
        f4 acc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        const float *tp = tile + c * P + g;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s], tp[16 * j * P + 4 * s], acc[j], 0, 0, 0);
        }
        // rows of the tile past its fill hold stale words: their norm is +inf and nothing of them is used
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float bn = bnorm[16 * j + c];
            const bool ok = bn < inf;
            const int col = t0 + 16 * j + c;
            float bx = 0.0f, by = 0.0f;
            if constexpr (GATED && !MODEL) {
                bx = bxy[2 * (16 * j + c)];
                by = bxy[2 * (16 * j + c) + 1];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float d = fmaxf(0.0f, (an[r] + bn) - 2.0f * acc[j][r]);
                d = ok ? d : inf;
                if constexpr (GATED && !MODEL) {
                    // one subtraction and one inclusive compare per axis; a NaN fails both
                    const bool in = fabsf(bx - ax[r]) <= a.radius_x && fabsf(by - ay[r]) <= a.radius_y;
                    d = in ? d : inf;
                }
                if constexpr (MODEL) d = ((pass >> (4 * j + r)) & 1u) ? d : inf;
                // the serial scan: a new best moves the old best to second, else d may lower second;
                // a NaN compares false both times
                const bool lt = d < best[r];
                const float s2 = lt ? best[r] : d;
                second[r] = s2 < second[r] ? s2 : second[r];
                bidx[r] = lt ? col : bidx[r];
                best[r] = lt ? d : best[r];
            }
        }
    }

    // merge over the 16 lanes (columns) that hold the same four rows: every lane ends with the result
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float ob = __shfl_xor(best[r], m), os = __shfl_xor(second[r], m);
            const int oi = __shfl_xor(bidx[r], m);
            const bool take = ob < best[r] || (ob == best[r] && oi < bidx[r]);
            const float lose = take ? best[r] : ob;
            float s2 = os < second[r] ? os : second[r];
            s2 = lose < s2 ? lose : s2;
            second[r] = s2;
            best[r] = take ? ob : best[r];
            bidx[r] = take ? oi : bidx[r];
        }
    }
    // lane c < 4 of each group of 16 writes row 4g + c
    float b1 = inf, b2 = inf;
    int bi = -1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (c == r) {
            b1 = best[r];
            b2 = second[r];
            bi = bidx[r];
        }
    }
    const int q = q0 + 16 * wave + 4 * g + c;
    const bool live = c < 4 && q < na;
    const int64_t aslot = static_cast<int64_t>(f) * a.a_stride + q;
    const bool has1 = live && b1 < inf, has2 = live && b2 < inf;
    const float d1 = has1 ? b1 : -1.0f, d2 = has2 ? b2 : -1.0f;
    // the ratio rule: two float multiplies and one compare (the file is built without contraction)
    match_emit(a, f, q, aslot, live, has1, has2, d1, d2, has1 ? bi : -1, d1 < (a.max_ratio * a.max_ratio) * d2);
}

template <int K, int TB>
void launch_k(const NnMatchArgs &a, unsigned blocks, hipStream_t s) {
    switch (gate_of(a)) {
        case kGateNone: hipLaunchKernelGGL((k_nn_match<K, TB, kGateNone>), dim3(blocks), dim3(kNnThreads), 0, s, a); break;
        case kGateWindow: hipLaunchKernelGGL((k_nn_match<K, TB, kGateWindow>), dim3(blocks), dim3(kNnThreads), 0, s, a); break;
        case kGateF: hipLaunchKernelGGL((k_nn_match<K, TB, kGateF>), dim3(blocks), dim3(kNnThreads), 0, s, a); break;
        case kGateHFwd: hipLaunchKernelGGL((k_nn_match<K, TB, kGateHFwd>), dim3(blocks), dim3(kNnThreads), 0, s, a); break;
        default: hipLaunchKernelGGL((k_nn_match<K, TB, kGateHRev>), dim3(blocks), dim3(kNnThreads), 0, s, a); break;
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

hipError_t launch_nn_norms(NnNormArgs a, hipStream_t s) {
    const int64_t total = static_cast<int64_t>(a.batch) * (static_cast<int64_t>(a.stride[0]) + a.stride[1]);
    if (total == 0) return hipSuccess;
    const int64_t blocks = (total + 255) / 256;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    for (int i = 0; i < 2; ++i) a.vec[i] = aligned16(a.desc[i]);
    hipLaunchKernelGGL(k_nn_norms, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_nn_match(NnMatchArgs a, hipStream_t s) {
    const int64_t blocks = static_cast<int64_t>(a.batch) * ((a.a_stride + kNnRows - 1) / kNnRows);
    if (blocks == 0) return hipSuccess;
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    a.b_vec = aligned16(a.b_desc);
    const unsigned g = static_cast<unsigned>(blocks);
    if (a.dim <= 128)
        launch_k<128, 64>(a, g, s);
    else
        launch_k<256, 32>(a, g, s);
    return hipGetLastError();
}

}  // namespace fdk
