// Contrast-limited adaptive histogram equalization (fd_frames_equalize: an MI355X extension, the reference has
// no such stage) for gfx950. The arithmetic, integers only, is the contract of include/fd_hip.h.
//
// k_eq_tab: the interpolation table of the two axes, one thread per column and per row: the *cell* of the pixel
// (cell 0 lies before the first tile centre, cell k between the centres of tiles k - 1 and k, cell `tiles` past
// the last centre; a cell's two tiles are max(k - 1, 0) and min(k, tiles - 1)) and the 1/1024 fraction inside it.
//
// k_eq_lut: one workgroup of 4 waves per (frame, tile). A group of 2^lanes_log2 lanes walks a tile row as the
// aligned dwords that cover it (the tile's left edge is arbitrary: a dword that straddles a row end is read as
// the bytes inside the tile), and counts into the sub-histogram of its wave, 32-bit LDS counters, so that a flat
// region keeps one wave, not the workgroup, on one address; a dword of four equal bytes is one add of 4. Then
// thread v owns bin v: merge, clip, the excess summed over the workgroup, the redistribution, an inclusive scan
// and the rounded division; the LUT leaves as 256 bytes.
//
// k_eq_apply: a workgroup is 4 waves, one destination row each, over 256 columns of one row cell (the rows
// between two tile-row centres), and a lane owns the 4 bytes of one aligned dword of the row of `out`, as in
// k_warp: packed aligned stores, byte stores at a row's ends, any base. The four LUTs of a cell are staged in
// LDS *packed*: entry v of cell (jc, ic) holds lut[j0][i0][v] | lut[j0][i1][v] << 8 | lut[j1][i0][v] << 16 |
// lut[j1][i1][v] << 24, so a pixel costs one ds_read_b32 instead of four byte gathers, and only the column
// cells the workgroup's 259 columns touch are staged (64 lanes transpose one cell from four dword loads each).
// The columns' table entries sit in LDS beside them. Every pixel is then the fixed-point blend of the contract.
#include <algorithm>

#include "fd_device.h"
#include "fd_hip.h"
#include "fd_kernels.h"

namespace fdk {
namespace {

constexpr int kEqThreads = 256;
constexpr int kEqWaves = kEqThreads / kWave;
constexpr int kEqPx = 4;                   // destination pixels per lane: one dword of out
constexpr int kEqTile = kWave * kEqPx;     // bytes of a destination row per workgroup
constexpr int kEqCols = kEqTile + 3;       // columns a workgroup may touch: a row's dwords start up to 3 bytes early
constexpr int kEqColTab = 260;             // LDS words of the columns' table entries (kEqCols, 16-byte multiple)

// Edge i of an axis of n pixels cut into t tiles.
__device__ __forceinline__ int edge(int i, int n, int t) { return static_cast<int>(static_cast<int64_t>(i) * n / t); }
// Twice the centre of tile i.
__device__ __forceinline__ int64_t centre2(int i, int n, int t) { return static_cast<int64_t>(edge(i, n, t)) + edge(i + 1, n, t); }

__global__ __launch_bounds__(kEqThreads) void k_eq_tab(EqualizeArgs a) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kEqThreads + threadIdx.x;
    if (t >= static_cast<int64_t>(a.cols) + a.rows) return;
    const bool col = t < a.cols;
    const int x = static_cast<int>(col ? t : t - a.cols), n = col ? a.cols : a.rows, tiles = col ? a.tiles_x : a.tiles_y;
    const int it = static_cast<int>(((static_cast<int64_t>(x) + 1) * tiles - 1) / n);  // the tile that holds x
    const int64_t p = 2 * static_cast<int64_t>(x) + 1;
    const int i0 = p >= centre2(it, n, tiles) ? it : it - 1;  // the largest i with centre2(i) <= p (-1: none)
    uint32_t cell, f = 0;
    if (i0 < 0) {
        cell = 0;
    } else if (i0 >= tiles - 1) {
        cell = static_cast<uint32_t>(tiles);
    } else {
        const int64_t c0 = centre2(i0, n, tiles), c1 = centre2(i0 + 1, n, tiles);
        f = static_cast<uint32_t>(((p - c0) * 1024) / (c1 - c0));
        cell = static_cast<uint32_t>(i0 + 1);
    }
    a.tab[t] = cell | f << 8;
}

__global__ __launch_bounds__(kEqThreads) void k_eq_lut(EqualizeArgs a) {
    __shared__ uint32_t hist[kEqWaves][256];
    __shared__ uint32_t wsum[kEqWaves];
    const int tid = threadIdx.x;
    const int tj = static_cast<int>(blockIdx.x) / a.tiles_x, ti = static_cast<int>(blockIdx.x) - tj * a.tiles_x;
    const int x0 = edge(ti, a.cols, a.tiles_x), y0 = edge(tj, a.rows, a.tiles_y);
    const int w = edge(ti + 1, a.cols, a.tiles_x) - x0, h = edge(tj + 1, a.rows, a.tiles_y) - y0;
    const uint32_t area = static_cast<uint32_t>(w) * static_cast<uint32_t>(h);  // <= 2^24 (fd_frames_equalize)
    const int group = 1 << a.lanes_log2;  // lanes that share a tile row
    const int l = tid & (group - 1), sub = tid >> a.lanes_log2, nsub = kEqThreads >> a.lanes_log2;
    uint32_t *hw = hist[tid / kWave];
    for (int b = blockIdx.y; b < a.batch; b += gridDim.y) {
#pragma unroll
        for (int i = 0; i < kEqWaves; ++i) hist[i][tid] = 0;
        __syncthreads();
        const uint8_t *img = a.frames + (static_cast<int64_t>(b) * a.rows + y0) * a.cols + x0;
        for (int r = sub; r < h; r += nsub) {
            const uint8_t *rowp = img + static_cast<int64_t>(r) * a.cols;
            const int lead = static_cast<int>(reinterpret_cast<uintptr_t>(rowp) & 3u);
            const int nd = (lead + w + 3) >> 2;  // aligned dwords that cover the tile row
            for (int k = l; k < nd; k += group) {
                const int o = 4 * k - lead;  // the dword's first byte, relative to the tile row: >= -3
                if (o >= 0 && o + 4 <= w) {
                    const uint32_t d = *reinterpret_cast<const uint32_t *>(rowp + o);
                    if (d == (d & 0xFFu) * 0x01010101u) {
                        atomicAdd(&hw[d & 0xFFu], 4u);
                    } else {
#pragma unroll
                        for (int m = 0; m < 4; ++m) atomicAdd(&hw[(d >> (8 * m)) & 0xFFu], 1u);
                    }
                } else {
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        if (o + m >= 0 && o + m < w) atomicAdd(&hw[rowp[o + m]], 1u);
                }
            }
        }
        __syncthreads();
        uint32_t hv = 0;  // bin tid
#pragma unroll
        for (int i = 0; i < kEqWaves; ++i) hv += hist[i][tid];
        if (a.clip_milli > 0) {
            const uint64_t lim64 = static_cast<uint64_t>(a.clip_milli) * area / 256000u;
            const uint32_t lim = lim64 < 1 ? 1u : (lim64 < area ? static_cast<uint32_t>(lim64) : area);  // (no bin exceeds the area)
            const uint32_t over = hv > lim ? hv - lim : 0u;
            hv = min(hv, lim);
            uint32_t excess;
            (void)wg_excl_add<kEqThreads>(over, wsum, excess);
            hv += excess >> 8;
            const uint32_t res = excess & 255u;
            if (res > 0) {
                const uint32_t step = 256u / res, v = static_cast<uint32_t>(tid);
                if (v % step == 0 && v / step < res) ++hv;
            }
        }
        uint32_t total;
        const uint32_t cdf = wg_excl_add<kEqThreads>(hv, wsum, total) + hv;  // (ends with a barrier: hist is free again)
        a.luts[(static_cast<int64_t>(b) * gridDim.x + blockIdx.x) * 256 + tid] = static_cast<uint8_t>((cdf * 255u + area / 2) / area);
    }
}

__global__ __launch_bounds__(kEqThreads) void k_eq_apply(EqualizeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t eq_lds[];
    uint32_t *ctab = eq_lds;             // [kEqColTab] table entries of columns xbase .. xbase + kEqCols - 1 (clamped)
    uint32_t *cells = eq_lds + kEqColTab;  // [column cells touched][256] packed LUT entries
    const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(threadIdx.y), tid = wave * kWave + lane;
    int q = static_cast<int>(blockIdx.x);
    const int chunk = q % a.chunks;
    q /= a.chunks;
    const int jc = q % (a.tiles_y + 1), part = q / (a.tiles_y + 1);
    // rows of row cell jc: 2y + 1 >= centre2(jc - 1) and < centre2(jc)
    const int ys = jc == 0 ? 0 : static_cast<int>(centre2(jc - 1, a.rows, a.tiles_y) >> 1);
    const int ye = jc == a.tiles_y ? a.rows : static_cast<int>(centre2(jc, a.rows, a.tiles_y) >> 1);
    if (ys + kEqWaves * part >= ye) return;  // (the whole workgroup: an empty cell or part)
    const int j0 = max(jc - 1, 0), j1 = min(jc, a.tiles_y - 1);
    const int xbase = chunk * kEqTile - 3;
    const int ic_lo = static_cast<int>(a.tab[max(xbase, 0)] & 0xFFu);
    const int ic_hi = static_cast<int>(a.tab[min(xbase + kEqCols - 1, a.cols - 1)] & 0xFFu);
    for (int i = tid; i < kEqCols; i += kEqThreads) ctab[i] = a.tab[min(max(xbase + i, 0), a.cols - 1)];
    for (int b = blockIdx.y; b < a.batch; b += gridDim.y) {
        const uint8_t *luts = a.luts + static_cast<int64_t>(b) * a.tiles_y * a.tiles_x * 256;
        for (int c = ic_lo + wave; c <= ic_hi; c += kEqWaves) {
            const int i0 = max(c - 1, 0), i1 = min(c, a.tiles_x - 1);
            const uint32_t A = reinterpret_cast<const uint32_t *>(luts + (j0 * a.tiles_x + i0) * 256)[lane];
            const uint32_t B = reinterpret_cast<const uint32_t *>(luts + (j0 * a.tiles_x + i1) * 256)[lane];
            const uint32_t C = reinterpret_cast<const uint32_t *>(luts + (j1 * a.tiles_x + i0) * 256)[lane];
            const uint32_t D = reinterpret_cast<const uint32_t *>(luts + (j1 * a.tiles_x + i1) * 256)[lane];
            uint32_t *dst = cells + (c - ic_lo) * 256 + 4 * lane;
#pragma unroll
            for (int m = 0; m < 4; ++m)
                dst[m] = ((A >> (8 * m)) & 0xFFu) | ((B >> (8 * m)) & 0xFFu) << 8 | ((C >> (8 * m)) & 0xFFu) << 16 |
                         ((D >> (8 * m)) & 0xFFu) << 24;
        }
        __syncthreads();
        for (int y = ys + wave + kEqWaves * part; y < ye; y += kEqWaves * a.row_split) {
            const int64_t row = (static_cast<int64_t>(b) * a.rows + y) * a.cols;  // the row's first byte in frames and out
            const int shift = static_cast<int>((reinterpret_cast<uintptr_t>(a.out) + static_cast<uint64_t>(row)) & 3u);
            const int x0 = chunk * kEqTile + lane * kEqPx - shift;  // >= xbase
            if (x0 >= a.cols) continue;
            const uint32_t fy = a.tab[a.cols + y] >> 8;
            const bool whole = x0 >= 0 && x0 + kEqPx <= a.cols;
            const uint8_t *src = a.frames + row + x0;
            uint32_t in4 = 0;
            if (whole && (reinterpret_cast<uintptr_t>(src) & 3u) == 0) {
                in4 = *reinterpret_cast<const uint32_t *>(src);
            } else {
#pragma unroll
                for (int j = 0; j < kEqPx; ++j)
                    if (x0 + j >= 0 && x0 + j < a.cols) in4 |= static_cast<uint32_t>(src[j]) << (8 * j);
            }
            uint32_t px4 = 0;
#pragma unroll
            for (int j = 0; j < kEqPx; ++j) {  // (a pixel outside the row is computed from the clamped column and not stored)
                const uint32_t ce = ctab[x0 - xbase + j];
                const uint32_t fx = ce >> 8;
                const uint32_t e = cells[(static_cast<int>(ce & 0xFFu) - ic_lo) * 256 + ((in4 >> (8 * j)) & 0xFFu)];
                const uint32_t top = (e & 0xFFu) * (1024u - fx) + ((e >> 8) & 0xFFu) * fx;
                const uint32_t bot = ((e >> 16) & 0xFFu) * (1024u - fx) + (e >> 24) * fx;
                px4 |= ((top * (1024u - fy) + bot * fy + (1u << 19)) >> 20) << (8 * j);
            }
            uint8_t *o = a.out + row + x0;
            if (whole) {
                *reinterpret_cast<uint32_t *>(o) = px4;  // aligned by the choice of x0
            } else {
#pragma unroll
                for (int j = 0; j < kEqPx; ++j)
                    if (x0 + j >= 0 && x0 + j < a.cols) o[j] = static_cast<uint8_t>(px4 >> (8 * j));
            }
        }
        __syncthreads();  // the next frame's cells overwrite these
    }
}

}  // namespace

hipError_t launch_equalize(EqualizeArgs a, hipStream_t s) {
    const int64_t entries = static_cast<int64_t>(a.cols) + a.rows;
    hipLaunchKernelGGL(k_eq_tab, dim3(static_cast<unsigned>((entries + kEqThreads - 1) / kEqThreads)), dim3(kEqThreads), 0, s, a);
    const unsigned frames = static_cast<unsigned>(std::min(a.batch, 65535));
    // lanes per tile row: the power of two that covers the widest row's dwords, so that narrow tiles fill a wave
    const int nd = ((a.cols + a.tiles_x - 1) / a.tiles_x + 6) >> 2;
    for (a.lanes_log2 = 0; (1 << a.lanes_log2) < nd && a.lanes_log2 < 8; ++a.lanes_log2) {}
    hipLaunchKernelGGL(k_eq_lut, dim3(static_cast<unsigned>(a.tiles_x * a.tiles_y), frames), dim3(kEqThreads), 0, s, a);
    // a row's dwords start up to 3 bytes before its first pixel
    a.chunks = static_cast<int>((static_cast<int64_t>(a.cols) + 3 + kEqTile - 1) / kEqTile);
    // small launches: a row cell's rows are dealt to up to row_split workgroups of at least 8 rows
    const int64_t base = static_cast<int64_t>(a.chunks) * (a.tiles_y + 1);
    const int64_t want = (2048 + base * a.batch - 1) / (base * a.batch);
    a.row_split = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(want, a.rows / a.tiles_y / 8)));
    if (base * a.row_split >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    const size_t lds = sizeof(uint32_t) * (kEqColTab + static_cast<size_t>(a.tiles_x + 1) * 256);
    hipLaunchKernelGGL(k_eq_apply, dim3(static_cast<unsigned>(base * a.row_split), frames), dim3(kWave, kEqWaves), lds, s, a);
    return hipGetLastError();
}

}  // namespace fdk
