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
    if (stride == 0) {  // no slots: every frame refines 0 features
        if (out_counts && io_on_device) FD_HIP_TRY(c, hipMemsetAsync(out_counts, 0, sizeof(int32_t) * batch, c->stream));
        if (out_counts && !io_on_device) std::fill(out_counts, out_counts + batch, 0);
        return FD_OK;
    }
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
    int32_t *dcounts_out = out_counts;
    if (io_on_device) {
        a.xy = xy;
        a.valid = valid;
        a.counts = counts;
        a.out_xy = out_xy;
        a.out_status = out_status;
    } else {  // the tracker's staging buffers: the two stages never overlap on one context
        FD_HIP_TRY(c, ensure_as(c, c->f_xy, 2 * slots, a.xy));
        FD_HIP_TRY(c, hipMemcpyAsync(c->f_xy.p, xy, sizeof(float) * 2 * slots, hipMemcpyHostToDevice, c->stream));
        if (valid) {
            FD_HIP_TRY(c, ensure_as(c, c->f_valid, slots, a.valid));
            FD_HIP_TRY(c, hipMemcpyAsync(c->f_valid.p, valid, slots, hipMemcpyHostToDevice, c->stream));
        }
        if (counts) {
            FD_HIP_TRY(c, ensure_as(c, c->f_counts, batch, a.counts));
            FD_HIP_TRY(c, hipMemcpyAsync(c->f_counts.p, counts, sizeof(int32_t) * batch, hipMemcpyHostToDevice, c->stream));
        }
        FD_HIP_TRY(c, ensure_as(c, c->f_oxy, 2 * slots, a.out_xy));
        FD_HIP_TRY(c, ensure_as(c, c->f_ost, slots, a.out_status));
        if (out_counts) FD_HIP_TRY(c, ensure_as(c, c->f_ocnt, batch, dcounts_out));
    }
    FD_HIP_TRY(c, fdk::launch_refine(a, c->stream));
    if (dcounts_out) {
        fdk::FlowFinishArgs fin{};
        fin.status = a.out_status;
        fin.counts = a.counts;
        fin.batch = batch;
        fin.stride = stride;
        fin.out_counts = dcounts_out;
        FD_HIP_TRY(c, hipMemsetAsync(dcounts_out, 0, sizeof(int32_t) * batch, c->stream));
        FD_HIP_TRY(c, fdk::launch_flow_finish(fin, c->stream));
    }
    if (!io_on_device) {
        if (out_counts)
            FD_HIP_TRY(c, hipMemcpyAsync(out_counts, dcounts_out, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, c->stream));
        return copy_back_written(c, counts, batch, stride, {{out_xy, a.out_xy, 2 * sizeof(float)}, {out_status, a.out_status, 1}});
    }
    if (!frames_on_device) FD_HIP_TRY(c, hipStreamSynchronize(c->stream));  // the caller's frames have been read
    return FD_OK;
}

}  // extern "C"
