// The bilinear sampler's position split, shared by the window kernels (fd_window.h: bytes from an LDS patch)
// and the image warp (fd_warp.hip: bytes from global memory): the raw sum S of include/fd_hip.h is
// w00 I(iy, ix) + w10 I(iy, ix + 1) + w01 I(iy + 1, ix) + w11 I(iy + 1, ix + 1) with these weights.
#pragma once

#include <hip/hip_runtime.h>

namespace fdk {

struct Weights {
    int w00, w10, w01, w11;
};
// ix = floor(x), and the four integer weights of the fraction in 1/1024 steps (truncated)
__device__ __forceinline__ void split_pos(float x, float y, int &ix, int &iy, Weights &w) {
    const float fx = floorf(x), fy = floorf(y);
    ix = static_cast<int>(fx);
    iy = static_cast<int>(fy);
    const int qx = static_cast<int>((x - fx) * 1024.0f), qy = static_cast<int>((y - fy) * 1024.0f);
    w.w00 = (1024 - qx) * (1024 - qy);
    w.w10 = qx * (1024 - qy);
    w.w01 = (1024 - qx) * qy;
    w.w11 = qx * qy;
}

}  // namespace fdk
