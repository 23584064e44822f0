// Host runtime of libfdhip.so: the image pyramids (fd_pyr_layout, fd_pyr_build, fd_pyr_build_gauss) and the pyramidal
// Lucas-Kanade tracker (fd_flow_lk) over the kernels of fd_flow.hip (and k_blur of fd_blur.hip: the Gaussian levels).
#include <algorithm>
#include <cmath>

#include "fd_ctx.h"

using namespace fdrt;

namespace {

static_assert(fdk::kPyrMaxLevels == FD_PYR_MAX_LEVELS, "FlowArgs::off holds one offset per level");

// fd_pyr_layout's arithmetic; false for what it rejects.
bool pyr_offsets(int batch, int rows, int cols, int levels, int64_t *off) {
    if (batch < 1 || rows < 1 || cols < 1 || levels < 1 || levels > FD_PYR_MAX_LEVELS) return false;
    if ((rows >> (levels - 1)) < 1 || (cols >> (levels - 1)) < 1) return false;
    off[0] = 0;
    for (int l = 0; l < levels; ++l) {
        const int64_t end = off[l] + static_cast<int64_t>(batch) * (rows >> l) * (cols >> l);
        off[l + 1] = (end + 255) / 256 * 256;
    }
    return true;
}

// One level [batch][rows >> 1][cols >> 1] of fd_pyr_build_gauss from the level [batch][rows][cols] below it: k_blur
// with pyrDown's taps and step 2, storing the floor dimensions.
hipError_t pyr_down_gauss(const uint8_t *src, uint8_t *dst, int batch, int rows, int cols, hipStream_t s) {
    fdk::BlurArgs a{};
    a.frames = src;
    a.out = dst;
    a.batch = batch;
    a.rows = rows;
    a.cols = cols;
    a.out_rows = rows >> 1;
    a.out_cols = cols >> 1;
    a.radius = 2;
    a.step = 2;
    a.taps[0] = 96;
    a.taps[1] = 64;
    a.taps[2] = 16;
    return fdk::launch_blur(a, s);
}

// fd_pyr_build and fd_pyr_build_gauss: the checks, the staging and the level loop; the level kernel differs.
int pyr_build(fd_ctx *c, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols, int levels, uint8_t *pyr,
              int pyr_on_device, bool gauss) {
    int rc = check_shape(c, FD_HARRIS, batch, rows, cols, false);
    if (rc) return rc;
    if (!frames || !pyr) return fail(c, FD_ERR_INVALID, "frames or pyr is NULL");
    int64_t off[FD_PYR_MAX_LEVELS + 1];
    if (!pyr_offsets(batch, rows, cols, levels, off))
        return fail(c, FD_ERR_INVALID, "levels must be in [1, 6] and the top level must keep a pixel");
    if (pyr_on_device && (reinterpret_cast<uintptr_t>(pyr) & 255))
        return fail(c, FD_ERR_INVALID, "a device pyr must be 256-byte aligned");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = refuse_sync_under_capture(c, pyr_on_device && frames_on_device))) return rc;
    uint8_t *dpyr = pyr;
    if (!pyr_on_device) FD_HIP_TRY(c, ensure_as(c, c->staging[0], static_cast<size_t>(off[levels]), dpyr));
    const size_t bytes0 = static_cast<size_t>(batch) * rows * cols;
    FD_HIP_TRY(c, hipMemcpyAsync(dpyr, frames, bytes0, frames_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                 c->stream));
    for (int l = 0; l + 1 < levels; ++l)
        FD_HIP_TRY(c, (gauss ? pyr_down_gauss : fdk::launch_pyr_down)(dpyr + off[l], dpyr + off[l + 1], batch, rows >> l, cols >> l,
                                                                      c->stream));
    if (!pyr_on_device) {
        for (int l = 0; l < levels; ++l)  // the levels only: the caller's padding bytes stay
            FD_HIP_TRY(c, hipMemcpyAsync(pyr + off[l], dpyr + off[l], static_cast<size_t>(batch) * (rows >> l) * (cols >> l),
                                         hipMemcpyDeviceToHost, c->stream));
    }
    if (!pyr_on_device || !frames_on_device) FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FD_OK;
}

}  // namespace

int fdrt::finish_counts(fd_ctx *c, const fdk::FlowFinishArgs &fin) {
    if (fin.out_counts) FD_HIP_TRY(c, hipMemsetAsync(fin.out_counts, 0, sizeof(int32_t) * fin.batch, c->stream));
    FD_HIP_TRY(c, fdk::launch_flow_finish(fin, c->stream));
    return FD_OK;
}

extern "C" {

int fd_pyr_layout(int batch, int rows, int cols, int levels, int64_t *offsets) {
    if (!offsets) return FD_ERR_INVALID;
    int64_t off[FD_PYR_MAX_LEVELS + 1];
    if (!pyr_offsets(batch, rows, cols, levels, off)) return FD_ERR_INVALID;
    std::copy(off, off + levels + 1, offsets);
    return FD_OK;
}

int fd_pyr_build(fd_ctx *c, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols, int levels,
                 uint8_t *pyr, int pyr_on_device) {
    return pyr_build(c, frames, frames_on_device, batch, rows, cols, levels, pyr, pyr_on_device, false);
}

int fd_pyr_build_gauss(fd_ctx *c, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols, int levels,
                       uint8_t *pyr, int pyr_on_device) {
    return pyr_build(c, frames, frames_on_device, batch, rows, cols, levels, pyr, pyr_on_device, true);
}

int fd_flow_lk(fd_ctx *c, int batch, int rows, int cols, int levels, const fd_flow_opts *opts, const uint8_t *prev_pyr,
               const uint8_t *next_pyr, const float *xy, const uint8_t *valid, const int32_t *counts, int32_t stride,
               const float *guess_xy, float *out_xy, uint8_t *out_status, float *out_err, int32_t *out_counts,
               int io_on_device) {
    int rc = check_shape(c, FD_HARRIS, batch, rows, cols, false);
    if (rc) return rc;
    if (!opts || !prev_pyr || !next_pyr || !xy || !out_xy || !out_status) return fail(c, FD_ERR_INVALID, "bad arguments");
    if (stride < 0) return fail(c, FD_ERR_INVALID, "stride must be >= 0");
    int64_t off[FD_PYR_MAX_LEVELS + 1];
    if (!pyr_offsets(batch, rows, cols, levels, off))
        return fail(c, FD_ERR_INVALID, "levels must be in [1, 6] and the top level must keep a pixel");
    fdk::FlowArgs a{};
    std::copy(off, off + levels, a.off);  // (the kernel needs the levels' starts, not the total size)
    if (opts->half_window < 1 || opts->half_window > 10) return fail(c, FD_ERR_INVALID, "half_window must be in [1, 10]");
    if (opts->max_iters < 1 || opts->max_iters > 100) return fail(c, FD_ERR_INVALID, "max_iters must be in [1, 100]");
    if (!std::isfinite(opts->epsilon) || !(opts->epsilon > 0.0f)) return fail(c, FD_ERR_INVALID, "epsilon must be finite and > 0");
    if (!std::isfinite(opts->min_eigen) || opts->min_eigen < 0.0f)
        return fail(c, FD_ERR_INVALID, "min_eigen must be finite and >= 0");
    if (!std::isfinite(opts->fb_max_dist) || !std::isfinite(opts->max_error))
        return fail(c, FD_ERR_INVALID, "fb_max_dist and max_error must be finite");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = refuse_sync_under_capture(c, io_on_device))) return rc;
    if (stride == 0) return zero_counts(c, out_counts, batch, io_on_device);  // no slots: every frame tracks 0 features
    const size_t slots = static_cast<size_t>(batch) * stride;
    const int n = (2 * opts->half_window + 1) * (2 * opts->half_window + 1);
    const bool fb = opts->fb_max_dist >= 0.0f;
    a.tmpl = prev_pyr;
    a.srch = next_pyr;
    a.batch = batch;
    a.rows = rows;
    a.cols = cols;
    a.levels = levels;
    a.stride = stride;
    a.r = opts->half_window;
    a.max_iters = opts->max_iters;
    a.eps2 = opts->epsilon * opts->epsilon;
    a.max_error = opts->max_error;
    a.tau = static_cast<double>(opts->min_eigen) * 1024.0 * n;
    HostIo io(c, io_on_device);
    FD_HIP_TRY(c, io.in(xy, 2 * slots, a.xy));
    FD_HIP_TRY(c, io.in(valid, slots, a.valid));
    FD_HIP_TRY(c, io.in(counts, batch, a.counts));
    FD_HIP_TRY(c, io.in(guess_xy, 2 * slots, a.guess));
    FD_HIP_TRY(c, io.out_slots(out_xy, slots, 2, a.out_xy));
    FD_HIP_TRY(c, io.out_slots(out_status, slots, 1, a.out_status));
    FD_HIP_TRY(c, io.out_slots(out_err, slots, 1, a.out_err, true));  // slots with valid 0 keep the caller's out_err
    fdk::FlowFinishArgs fin{};
    FD_HIP_TRY(c, io.out(out_counts, batch, fin.out_counts));
    FD_HIP_TRY(c, fdk::launch_flow_lk(a, c->stream));
    fin.xy = a.xy;
    fin.status = a.out_status;
    fin.counts = a.counts;
    fin.batch = batch;
    fin.stride = stride;
    if (fb) {
        // the way back: from the forward result in the next frame towards xy in the previous one
        fdk::FlowArgs r = a;
        float *bxy = nullptr;
        uint8_t *bst = nullptr;
        FD_HIP_TRY(c, ensure_as(c, c->f_bxy, 2 * slots, bxy));
        FD_HIP_TRY(c, ensure_as(c, c->f_bst, slots, bst));
        r.tmpl = next_pyr;
        r.srch = prev_pyr;
        r.xy = a.out_xy;
        r.guess = a.xy;
        r.valid = a.out_status;
        r.valid_is_status = 1;
        r.max_error = -1.0f;
        r.out_xy = bxy;
        r.out_status = bst;
        r.out_err = nullptr;
        FD_HIP_TRY(c, fdk::launch_flow_lk(r, c->stream));
        fin.back_xy = bxy;
        fin.back_status = bst;
        fin.fb2 = opts->fb_max_dist * opts->fb_max_dist;
    }
    if ((fb || fin.out_counts) && (rc = finish_counts(c, fin))) return rc;
    return io.finish(counts, batch, stride);
}

}  // extern "C"
