// Host runtime of libfdhip.so: sub-pixel corner refinement (fd_points_refine) over k_refine of
// fd_refine.hip; the per-frame counts are k_flow_finish's (fd_flow.hip) without a backward pass.
#include <algorithm>
#include <cmath>

#include "fd_ctx.h"

using namespace fdrt;

extern "C" {

int fd_points_refine(fd_ctx *c, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                     const fd_refine_opts *opts, const float *xy, const uint8_t *valid, const int32_t *counts, int32_t stride,
                     float *out_xy, uint8_t *out_status, int32_t *out_counts, int io_on_device) {
    int rc = check_shape(c, FD_HARRIS, batch, rows, cols, false);
    if (rc) return rc;
    if (!opts || !frames || !xy || !out_xy || !out_status) return fail(c, FD_ERR_INVALID, "bad arguments");
    if (stride < 0) return fail(c, FD_ERR_INVALID, "stride must be >= 0");
    if (opts->half_window < 1 || opts->half_window > 10) return fail(c, FD_ERR_INVALID, "half_window must be in [1, 10]");
    if (opts->max_iters < 1 || opts->max_iters > 100) return fail(c, FD_ERR_INVALID, "max_iters must be in [1, 100]");
    if (!std::isfinite(opts->epsilon) || !(opts->epsilon > 0.0f)) return fail(c, FD_ERR_INVALID, "epsilon must be finite and > 0");
    if (!std::isfinite(opts->min_eigen) || opts->min_eigen < 0.0f)
        return fail(c, FD_ERR_INVALID, "min_eigen must be finite and >= 0");
    if (!std::isfinite(opts->max_shift) || !(opts->max_shift > 0.0f))
        return fail(c, FD_ERR_INVALID, "max_shift must be finite and > 0");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = refuse_sync_under_capture(c, io_on_device && frames_on_device))) return rc;
    if (stride == 0) return zero_counts(c, out_counts, batch, io_on_device);  // no slots: every frame refines 0 features
    const size_t slots = static_cast<size_t>(batch) * stride;
    const int r1 = opts->half_window + 1;
    fdk::RefineArgs a{};
    if ((rc = stage_frames(c, frames, frames_on_device, batch, rows, cols, a.frames))) return rc;
    a.batch = batch;
    a.rows = rows;
    a.cols = cols;
    a.stride = stride;
    a.r = opts->half_window;
    a.max_iters = opts->max_iters;
    a.eps2 = opts->epsilon * opts->epsilon;
    a.max_shift = opts->max_shift;
    a.tau = static_cast<double>(opts->min_eigen) * 1024.0 * static_cast<double>(r1 * r1 * r1 * r1);
    HostIo io(c, io_on_device);
    FD_HIP_TRY(c, io.in(xy, 2 * slots, a.xy));
    FD_HIP_TRY(c, io.in(valid, slots, a.valid));
    FD_HIP_TRY(c, io.in(counts, batch, a.counts));
    FD_HIP_TRY(c, io.out_slots(out_xy, slots, 2, a.out_xy));  // (its own buffer, also where out_xy == xy)
    FD_HIP_TRY(c, io.out_slots(out_status, slots, 1, a.out_status));
    fdk::FlowFinishArgs fin{};
    FD_HIP_TRY(c, io.out(out_counts, batch, fin.out_counts));
    FD_HIP_TRY(c, fdk::launch_refine(a, c->stream));
    if (fin.out_counts) {
        fin.status = a.out_status;
        fin.counts = a.counts;
        fin.batch = batch;
        fin.stride = stride;
        if ((rc = finish_counts(c, fin))) return rc;
    }
    if ((rc = io.finish(counts, batch, stride))) return rc;
    if (io_on_device && !frames_on_device) FD_HIP_TRY(c, hipStreamSynchronize(c->stream));  // the caller's frames have been read
    return FD_OK;
}

}  // extern "C"
