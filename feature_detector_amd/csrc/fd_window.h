// Device code shared by the two window kernels (fd_flow.hip's k_flow_lk, fd_refine.hip's k_refine): one wave
// per feature, the wave's u8 patch staged in its own LDS rows, the bilinear raw sum S of include/fd_hip.h
// from LDS bytes with four wave-uniform integer weights, and the exact wave total of an int32 per lane.
#pragma once

#include "fd_bilinear.h"
#include "fd_match_common.h"

namespace fdk {

constexpr int kFlowWaves = 4;
constexpr int kFlowThreads = kFlowWaves * kWave;
constexpr int kFlowPitch = 24;  // LDS patch row pitch in bytes: 2 * 10 + 4, the widest template patch
constexpr int kFlowPatch = kFlowPitch * kFlowPitch;

// Orders a wave's LDS accesses for the compiler. The hardware needs nothing: one wave's LDS instructions
// execute in order, and the waves of a workgroup share no LDS here.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Exact sum over the wave of one int32 per lane (|sum| may pass 2^31): low and high halves apart.
__device__ __forceinline__ int64_t wave_sum_i32(int32_t v) {
    const uint32_t lo = wave_total_add(static_cast<uint32_t>(v) & 0xFFFFu);            // <= 64 * 65535
    const int32_t hi = static_cast<int32_t>(wave_total_add(static_cast<uint32_t>(v >> 16)));  // |.| <= 64 * 32768
    return static_cast<int64_t>(hi) * 65536 + static_cast<int64_t>(lo);
}

// The P x P pixels from (x0, y0) of a level into the wave's patch, reads clamped to the level's edge.
__device__ __forceinline__ void stage_patch(uint8_t *patch, const uint8_t *img, int rows, int cols, int x0, int y0, int P,
                                            int lane) {
    const int px = lane & 31, par = lane >> 5;
    if (px < P) {
        const int xx = min(max(x0 + px, 0), cols - 1);
        for (int py = par; py < P; py += 2) {
            const int yy = min(max(y0 + py, 0), rows - 1);
            patch[py * kFlowPitch + px] = img[static_cast<int64_t>(yy) * cols + xx];
        }
    }
}

// (split_pos and its four weights: fd_bilinear.h)
__device__ __forceinline__ int raw_sum(const uint8_t *p, const Weights &w) {
    return w.w00 * p[0] + w.w10 * p[1] + w.w01 * p[kFlowPitch] + w.w11 * p[kFlowPitch + 1];
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }

}  // namespace fdk
