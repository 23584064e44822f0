// Separable integer smoothing (fd_frames_blur, fd_pyr_build_gauss: an MI355X extension, the reference has no
// such stage) for gfx950. The arithmetic, integers only, is the contract of include/fd_hip.h.
//
// k_blur<R, STEP>: one fused kernel, both passes. A workgroup of 4 waves owns a tile of tile_rows (32, 16 or 8)
// output rows by kBlurTileCols = 128 output columns of one frame, and walks four phases with a barrier between
// them:
//   load        the source rows and columns the tile needs (STEP * (rows - 1) + 1 + 2R by STEP * 131 + 1 + 2 R4,
//               R4 = R rounded up to 4) into LDS as dwords, the reflection resolved here: interior dwords are one
//               aligned load, a dword on a frame edge (or of a row that is not dword aligned) four byte loads.
//   horizontal  a thread makes 4 adjacent values of h for one source row from STEP + R4 / 2 dwords of that row
//               (every byte position is a compile-time constant) and writes them as 4 x 16 bits, one ds_write_b64.
//               With STEP 2 only the even columns are computed.
//   vertical    a thread makes 4 adjacent output pixels of one output row from 2R + 1 ds_read_b64 of the column
//               quad (consecutive lanes read consecutive 8 bytes: no bank conflict), rounds once, and writes the
//               4 bytes as one dword into the tile's output image in LDS (over the dead source rows). With STEP 2
//               only the even rows are computed.
//   store       as k_eq_apply: a lane owns one aligned dword of a row of `out`, takes its 4 bytes from the LDS
//               image at the row's own byte shift (two dwords and a funnel shift), and stores it packed; a row's
//               first and last bytes leave as bytes. That shift is why a tile computes 132 columns: the 128 and
//               the 4 before them.
// The source is read from memory once (plus halo), the output written once, nothing in between leaves the CU.
// The taps are kernel arguments (scalar registers); products are 24-bit multiplies (taps <= 256, h < 2^16).
// R is the loop bound of an instance, the smallest of 2, 3, 5, 8, 11, 15 that holds the call's radius; taps above
// the radius are 0 (launch_blur), which adds 0 to every sum. Nothing here depends on the launch shape: a pixel's
// value is the contract's, whichever tile computes it.
#include <algorithm>

#include "fd_device.h"
#include "fd_hip.h"
#include "fd_kernels.h"

namespace fdk {
namespace {

constexpr int kBlurThreads = 256;
constexpr int kBlurQuads = kBlurTileCols / 4 + 1;  // quads of output columns a tile computes per row: its 128 and the 4 before

template <int R, int STEP>
struct BlurGeom {
    static constexpr int R4 = (R + 3) / 4 * 4;
    static constexpr int kSrcDw = STEP * kBlurQuads + R4 / 2;  // dwords of a source row in LDS
    static constexpr int kQuadDw = STEP + R4 / 2;              // dwords a quad of h reads
    // source rows of a tile of th output rows
    __host__ __device__ static constexpr int src_rows(int th) { return STEP * (th - 1) + 1 + 2 * R; }
    // LDS dwords: h ([rows][2 * kBlurQuads], first: 8-byte aligned), then the source rows
    __host__ __device__ static constexpr int h_dwords(int th) { return src_rows(th) * 2 * kBlurQuads; }
    __host__ __device__ static constexpr int lds_dwords(int th) { return h_dwords(th) + src_rows(th) * kSrcDw; }
};

// include/fd_hip.h's refl(i, n)
__device__ __forceinline__ int reflect(int i, int n) {
    if (static_cast<unsigned>(i) < static_cast<unsigned>(n)) return i;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

// Byte i (compile-time after unrolling) of the dwords d.
template <int N>
__device__ __forceinline__ uint32_t dw_byte(const uint32_t (&d)[N], int i) {
    return (d[i >> 2] >> (8 * (i & 3))) & 0xFFu;
}

template <int R, int STEP>
__global__ __launch_bounds__(kBlurThreads) void k_blur(BlurArgs a) {
    using G = BlurGeom<R, STEP>;
    extern __shared__ __attribute__((aligned(16))) uint32_t blur_lds[];
    uint32_t *hbuf = blur_lds;                           // [source rows][kBlurQuads] x 4 values of 16 bits
    uint32_t *src = blur_lds + G::h_dwords(a.tile_rows);  // [source rows][kSrcDw] source bytes
    uint32_t *otile = src;                               // [output rows][kBlurQuads] output bytes, after the horizontal pass
    const int tid = threadIdx.x;
    const int tile_y = static_cast<int>(blockIdx.x) / a.chunks, chunk = static_cast<int>(blockIdx.x) - tile_y * a.chunks;
    const int y0 = tile_y * a.tile_rows;
    const int th = min(a.tile_rows, a.out_rows - y0);  // >= 1 (launch_blur's grid)
    const int sh = G::src_rows(th);
    const int xb = chunk * kBlurTileCols - 4;  // the first output column computed
    const int xs0 = STEP * xb - G::R4;         // the source column of byte 0 of an LDS row: a multiple of 4
    const int ys0 = STEP * y0 - R;             // the source row of LDS row 0
    for (int b = blockIdx.y; b < a.batch; b += gridDim.y) {
        const uint8_t *img = a.frames + static_cast<int64_t>(b) * a.rows * a.cols;
        for (int i = tid; i < sh * G::kSrcDw; i += kBlurThreads) {
            const int sr = i / G::kSrcDw, x = xs0 + 4 * (i - sr * G::kSrcDw);
            const uint8_t *rowp = img + static_cast<int64_t>(reflect(ys0 + sr, a.rows)) * a.cols;
            uint32_t d = 0;
            if (x >= 0 && x + 4 <= a.cols) {
                if ((reinterpret_cast<uintptr_t>(rowp + x) & 3u) == 0) {
                    d = *reinterpret_cast<const uint32_t *>(rowp + x);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) d |= static_cast<uint32_t>(rowp[x + j]) << (8 * j);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) d |= static_cast<uint32_t>(rowp[reflect(x + j, a.cols)]) << (8 * j);
            }
            src[i] = d;
        }
        __syncthreads();
        for (int i = tid; i < sh * kBlurQuads; i += kBlurThreads) {
            const int sr = i / kBlurQuads, q = i - sr * kBlurQuads;
            const uint32_t *p = src + sr * G::kSrcDw + STEP * q;
            uint32_t d[G::kQuadDw];
#pragma unroll
            for (int t = 0; t < G::kQuadDw; ++t) d[t] = p[t];
            uint32_t h[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = STEP * j + G::R4;  // the byte of d under output column 4q + j
                uint32_t s = __umul24(static_cast<uint32_t>(a.taps[0]), dw_byte(d, c));
#pragma unroll
                for (int k = 1; k <= R; ++k) s += __umul24(static_cast<uint32_t>(a.taps[k]), dw_byte(d, c - k) + dw_byte(d, c + k));
                h[j] = s;  // <= 65280
            }
            reinterpret_cast<uint2 *>(hbuf)[i] = make_uint2(h[0] | h[1] << 16, h[2] | h[3] << 16);
        }
        __syncthreads();
        for (int i = tid; i < th * kBlurQuads; i += kBlurThreads) {
            const int ty = i / kBlurQuads, q = i - ty * kBlurQuads;
            const uint2 *p = reinterpret_cast<const uint2 *>(hbuf) + STEP * ty * kBlurQuads + q;  // source row STEP * (y0 + ty) - R
            uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k <= 2 * R; ++k) {
                const uint2 e = p[k * kBlurQuads];
                const uint32_t w = static_cast<uint32_t>(a.taps[k < R ? R - k : k - R]);
                v[0] += __umul24(w, e.x & 0xFFFFu);
                v[1] += __umul24(w, e.x >> 16);
                v[2] += __umul24(w, e.y & 0xFFFFu);
                v[3] += __umul24(w, e.y >> 16);
            }
            otile[i] = (v[0] + 32768u) >> 16 | ((v[1] + 32768u) >> 16) << 8 | ((v[2] + 32768u) >> 16) << 16 |
                       ((v[3] + 32768u) >> 16) << 24;
        }
        __syncthreads();
        for (int i = tid; i < th * (kBlurTileCols / 4); i += kBlurThreads) {
            const int ty = i / (kBlurTileCols / 4), l = i - ty * (kBlurTileCols / 4);
            const int64_t row = (static_cast<int64_t>(b) * a.out_rows + y0 + ty) * a.out_cols;  // the row's first byte in out
            const int shift = static_cast<int>((reinterpret_cast<uintptr_t>(a.out) + static_cast<uint64_t>(row)) & 3u);
            const int x0 = chunk * kBlurTileCols + 4 * l - shift;  // >= xb + 1
            if (x0 >= a.out_cols) continue;
            const uint32_t *r = otile + ty * kBlurQuads;
            uint32_t px4;
            if (shift == 0) {
                px4 = r[l + 1];
            } else {  // bytes 4 (l + 1) - shift .. of the row
                px4 = r[l] >> (8 * (4 - shift)) | r[l + 1] << (8 * shift);
            }
            uint8_t *o = a.out + row + x0;
            if (x0 >= 0 && x0 + 4 <= a.out_cols) {
                *reinterpret_cast<uint32_t *>(o) = px4;  // aligned by the choice of x0
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x0 + j >= 0 && x0 + j < a.out_cols) o[j] = static_cast<uint8_t>(px4 >> (8 * j));
            }
        }
        __syncthreads();  // the next frame's source rows overwrite the output image
    }
}

template <int R, int STEP>
hipError_t launch_instance(const BlurArgs &a, dim3 grid, hipStream_t s) {
    const size_t lds = sizeof(uint32_t) * BlurGeom<R, STEP>::lds_dwords(a.tile_rows);
    static_assert(sizeof(uint32_t) * BlurGeom<R, STEP>::lds_dwords(kBlurTileRows) <= 64 * 1024, "the tile must fit 64 KiB of LDS");
    hipLaunchKernelGGL((k_blur<R, STEP>), grid, dim3(kBlurThreads), lds, s, a);
    return hipGetLastError();
}

template <int STEP>
hipError_t launch_step(const BlurArgs &a, dim3 grid, hipStream_t s) {
    if (a.radius <= 2) return launch_instance<2, STEP>(a, grid, s);
    if (a.radius <= 3) return launch_instance<3, STEP>(a, grid, s);
    if (a.radius <= 5) return launch_instance<5, STEP>(a, grid, s);
    if (a.radius <= 8) return launch_instance<8, STEP>(a, grid, s);
    if (a.radius <= 11) return launch_instance<11, STEP>(a, grid, s);
    return launch_instance<15, STEP>(a, grid, s);
}

}  // namespace

hipError_t launch_blur(BlurArgs a, hipStream_t s) {
    if (a.radius < 0 || a.radius > 15 || (a.step != 1 && a.step != 2)) return hipErrorInvalidValue;
    if (a.batch < 1 || a.out_rows < 1 || a.out_cols < 1) return hipSuccess;
    for (int k = a.radius + 1; k < 16; ++k) a.taps[k] = 0;
    // a row's dwords start up to 3 bytes before its first pixel: always the same bytes where every row is a
    // whole number of dwords
    const int lead = (a.out_cols & 3) ? 3 : static_cast<int>(reinterpret_cast<uintptr_t>(a.out) & 3u);
    a.chunks = static_cast<int>((static_cast<int64_t>(a.out_cols) + lead + kBlurTileCols - 1) / kBlurTileCols);
    const unsigned frames = static_cast<unsigned>(std::min(a.batch, 65535));
    // small launches: shorter tiles, for more workgroups than compute units
    a.tile_rows = kBlurTileRows;
    while (a.tile_rows > 8 && static_cast<int64_t>(a.chunks) * ((a.out_rows + a.tile_rows - 1) / a.tile_rows) * frames < 512)
        a.tile_rows >>= 1;
    const int64_t blocks = static_cast<int64_t>(a.chunks) * ((a.out_rows + a.tile_rows - 1) / a.tile_rows);
    if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>(blocks), frames);
    return a.step == 1 ? launch_step<1>(a, grid, s) : launch_step<2>(a, grid, s);
}

}  // namespace fdk
