// Host runtime of libfdhip.so: image warp by a homography or a camera model (fd_frames_warp) over k_warp of
// fd_warp.hip.
#include "fd_ctx.h"

using namespace fdrt;

extern "C" {

int fd_frames_warp(fd_ctx *c, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                   const fd_warp_opts *opts, const double *params, int params_on_device, int out_rows, int out_cols,
                   uint8_t *out, uint8_t *out_mask, int out_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!opts || !frames || !params || !out) return fail(c, FD_ERR_INVALID, "bad arguments");
    if (batch < 1 || rows < 1 || cols < 1) return fail(c, FD_ERR_INVALID, "batch, rows and cols must be >= 1");
    if (out_rows < 0 || out_cols < 0) return fail(c, FD_ERR_INVALID, "out_rows and out_cols must be >= 0");
    if (opts->model != FD_WARP_HOMOGRAPHY && opts->model != FD_WARP_CAMERA)
        return fail(c, FD_ERR_INVALID, "model must be FD_WARP_HOMOGRAPHY or FD_WARP_CAMERA");
    if (opts->shared_params != 0 && opts->shared_params != 1) return fail(c, FD_ERR_INVALID, "shared_params must be 0 or 1");
    if (opts->fill < 0 || opts->fill > 255) return fail(c, FD_ERR_INVALID, "fill must be in [0, 255]");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    const bool all_dev = frames_on_device && params_on_device && out_on_device;
    int rc = refuse_sync_under_capture(c, all_dev);
    if (rc) return rc;
    if (out_rows == 0 || out_cols == 0) return FD_OK;  // no destination pixels
    fdk::WarpArgs a{};
    if ((rc = stage_frames(c, frames, frames_on_device, batch, rows, cols, a.frames))) return rc;
    a.batch = batch;
    a.rows = rows;
    a.cols = cols;
    a.out_rows = out_rows;
    a.out_cols = out_cols;
    a.model = opts->model;
    a.shared = opts->shared_params;
    a.fill = opts->fill;
    const size_t per = opts->model == FD_WARP_HOMOGRAPHY ? 9 : 22;
    const size_t n = static_cast<size_t>(batch) * out_rows * out_cols;
    HostIo pin(c, params_on_device);  // staging[0] (host params), then the outputs
    FD_HIP_TRY(c, pin.in(params, per * (opts->shared_params ? 1 : batch), a.params));
    HostIo io(c, out_on_device, 1);
    FD_HIP_TRY(c, io.out(out, n, a.out));
    FD_HIP_TRY(c, io.out(out_mask, n, a.mask));
    FD_HIP_TRY(c, fdk::launch_warp(a, c->stream));
    if ((rc = io.finish(nullptr, batch, 0))) return rc;  // host outputs: copied back, synchronised
    if (out_on_device && !all_dev) FD_HIP_TRY(c, hipStreamSynchronize(c->stream));  // the caller's host arrays have been read
    return FD_OK;
}

}  // extern "C"
