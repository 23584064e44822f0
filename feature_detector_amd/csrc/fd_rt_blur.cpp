// Host runtime of libfdhip.so: separable integer smoothing (fd_blur_taps, fd_frames_blur) over k_blur of
// fd_blur.hip. fd_pyr_build_gauss, which launches the same kernel per level, is in fd_rt_flow.cpp.
#include <algorithm>
#include <cmath>

#include "fd_ctx.h"

using namespace fdrt;

extern "C" {

int fd_blur_taps(double sigma, int radius, fd_blur_opts *opts) {
    if (!opts || !std::isfinite(sigma) || !(sigma > 0.0)) return FD_ERR_INVALID;
    int r = radius;
    if (r < 1 || r > FD_BLUR_MAX_RADIUS)
        r = 3.0 * sigma >= FD_BLUR_MAX_RADIUS ? FD_BLUR_MAX_RADIUS : std::max(1, static_cast<int>(std::ceil(3.0 * sigma)));
    double g[FD_BLUR_MAX_RADIUS + 1], sum = 0.0;
    for (int k = 0; k <= r; ++k) g[k] = std::exp(-static_cast<double>(k * k) / (2.0 * sigma * sigma));
    for (int k = 1; k <= r; ++k) sum += g[k];
    sum = g[0] + 2.0 * sum;
    int32_t w[FD_BLUR_MAX_RADIUS + 1] = {};
    int32_t side = 0;
    for (int k = 1; k <= r; ++k) {
        w[k] = static_cast<int32_t>(std::floor(256.0 * g[k] / sum + 0.5));
        side += w[k];
    }
    w[0] = 256 - 2 * side;
    if (w[0] < w[1]) return FD_ERR_INVALID;
    opts->radius = r;
    std::copy(w, w + FD_BLUR_MAX_RADIUS + 1, opts->taps);
    opts->step = 1;
    return FD_OK;
}

int fd_frames_blur(fd_ctx *c, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                   const fd_blur_opts *opts, uint8_t *out, int out_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!opts || !frames || !out) return fail(c, FD_ERR_INVALID, "bad arguments");
    if (batch < 1 || rows < 1 || cols < 1) return fail(c, FD_ERR_INVALID, "batch, rows and cols must be >= 1");
    if (rows > (1 << 30) || cols > (1 << 30)) return fail(c, FD_ERR_INVALID, "rows and cols must be <= 2^30");
    fdk::BlurArgs a{};
    if (int rc = blur_options(c, *opts, a)) return rc;
    if (out == frames && !frames_on_device == !out_on_device)
        return fail(c, FD_ERR_INVALID, "out must not be frames: there is no in-place blur");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    const bool all_dev = frames_on_device && out_on_device;
    int rc = refuse_sync_under_capture(c, all_dev);
    if (rc) return rc;
    if ((rc = stage_frames(c, frames, frames_on_device, batch, rows, cols, a.frames))) return rc;
    a.batch = batch;
    a.rows = rows;
    a.cols = cols;
    a.out_rows = (rows + a.step - 1) / a.step;
    a.out_cols = (cols + a.step - 1) / a.step;
    HostIo io(c, out_on_device);  // (host frames have their own buffer)
    FD_HIP_TRY(c, io.out(out, static_cast<size_t>(batch) * a.out_rows * a.out_cols, a.out));
    FD_HIP_TRY(c, fdk::launch_blur(a, c->stream));
    if ((rc = io.finish(nullptr, batch, 0))) return rc;  // host out: copied back, synchronised
    if (out_on_device && !all_dev) FD_HIP_TRY(c, hipStreamSynchronize(c->stream));  // the caller's host frames have been read
    return FD_OK;
}

}  // extern "C"

// fd_blur_opts as fd_frames_blur checks them, into the kernel's arguments.
int fdrt::blur_options(fd_ctx *c, const fd_blur_opts &o, fdk::BlurArgs &a) {
    if (o.radius < 0 || o.radius > FD_BLUR_MAX_RADIUS) return fail(c, FD_ERR_INVALID, "radius must be in [0, 15]");
    if (o.step != 1 && o.step != 2) return fail(c, FD_ERR_INVALID, "step must be 1 or 2");
    int64_t sum = 0;
    for (int k = 0; k <= o.radius; ++k) {
        if (o.taps[k] < 0) return fail(c, FD_ERR_INVALID, "taps must be >= 0");
        sum += (k ? 2 : 1) * static_cast<int64_t>(o.taps[k]);
    }
    if (sum != 256) return fail(c, FD_ERR_INVALID, "taps must sum to 256: w[0] + 2*(w[1] + ... + w[r])");
    a.radius = o.radius;
    a.step = o.step;
    std::copy(o.taps, o.taps + o.radius + 1, a.taps);
    return FD_OK;
}
