// Host runtime of libfdhip.so: the line band descriptor (fd_lines_describe) over k_line_desc of
// fd_line_desc.hip. No workspace: the kernel keeps a line's sums in LDS.
#include "fd_ctx.h"

using namespace fdrt;

extern "C" {

int fd_lines_describe(fd_ctx *c, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                      const fd_line_desc_opts *opts, const float *lines, int32_t line_floats, const int32_t *counts,
                      int32_t stride, float *out_desc, float *out_xy, uint8_t *out_valid, int io_on_device) {
    int rc = check_shape(c, FD_HARRIS, batch, rows, cols, false);
    if (rc) return rc;
    if (!opts || !frames || !lines || !out_desc) return fail(c, FD_ERR_INVALID, "bad arguments");
    if (rows < 3 || cols < 3) return fail(c, FD_ERR_INVALID, "rows and cols must be >= 3");
    if (stride < 0) return fail(c, FD_ERR_INVALID, "stride must be >= 0");
    if (line_floats != 4 && line_floats != 12) return fail(c, FD_ERR_INVALID, "line_floats must be 4 or 12");
    if (opts->bands < 1 || opts->bands > 32) return fail(c, FD_ERR_INVALID, "bands must be in [1, 32]");
    if (opts->band_width < 1 || opts->band_width > 16) return fail(c, FD_ERR_INVALID, "band_width must be in [1, 16]");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = refuse_sync_under_capture(c, io_on_device && frames_on_device))) return rc;
    if (stride == 0) return FD_OK;  // no slots
    const size_t slots = static_cast<size_t>(batch) * stride;
    fdk::LineDescArgs a{};
    if ((rc = stage_frames(c, frames, frames_on_device, batch, rows, cols, a.frames))) return rc;
    a.batch = batch;
    a.rows = rows;
    a.cols = cols;
    a.stride = stride;
    a.line_floats = line_floats;
    a.bands = opts->bands;
    a.band_width = opts->band_width;
    HostIo io(c, io_on_device);
    FD_HIP_TRY(c, io.in(lines, slots * line_floats, a.lines));
    FD_HIP_TRY(c, io.in(counts, batch, a.counts));
    FD_HIP_TRY(c, io.out_slots(out_desc, slots, 8 * static_cast<size_t>(opts->bands), a.out_desc));
    FD_HIP_TRY(c, io.out_slots(out_xy, slots, 2, a.out_xy));
    FD_HIP_TRY(c, io.out_slots(out_valid, slots, 1, a.out_valid));
    FD_HIP_TRY(c, fdk::launch_line_desc(a, c->stream));
    if ((rc = io.finish(counts, batch, stride))) return rc;
    if (io_on_device && !frames_on_device) FD_HIP_TRY(c, hipStreamSynchronize(c->stream));  // the caller's frames have been read
    return FD_OK;
}

}  // extern "C"
