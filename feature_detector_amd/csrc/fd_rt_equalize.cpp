// Host runtime of libfdhip.so: contrast-limited adaptive histogram equalization (fd_frames_equalize) over
// k_eq_tab, k_eq_lut and k_eq_apply of fd_equalize.hip.
#include <algorithm>

#include "fd_ctx.h"

using namespace fdrt;

extern "C" {

int fd_frames_equalize(fd_ctx *c, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                       const fd_equalize_opts *opts, uint8_t *out, int out_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!opts || !frames || !out) return fail(c, FD_ERR_INVALID, "bad arguments");
    if (batch < 1 || rows < 1 || cols < 1) return fail(c, FD_ERR_INVALID, "batch, rows and cols must be >= 1");
    if (opts->tiles_x < 1 || opts->tiles_x > std::min(32, cols)) return fail(c, FD_ERR_INVALID, "tiles_x must be in [1, min(32, cols)]");
    if (opts->tiles_y < 1 || opts->tiles_y > std::min(32, rows)) return fail(c, FD_ERR_INVALID, "tiles_y must be in [1, min(32, rows)]");
    if (opts->clip_milli < 0) return fail(c, FD_ERR_INVALID, "clip_milli must be >= 0");
    // the largest tile: ceil(cols / tiles_x) x ceil(rows / tiles_y)
    const int64_t area = static_cast<int64_t>((cols + opts->tiles_x - 1) / opts->tiles_x) * ((rows + opts->tiles_y - 1) / opts->tiles_y);
    if (area > (int64_t(1) << 24)) return fail(c, FD_ERR_INVALID, "a tile must not have more than 2^24 pixels");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    const bool all_dev = frames_on_device && out_on_device;
    int rc = refuse_sync_under_capture(c, all_dev);
    if (rc) return rc;
    fdk::EqualizeArgs a{};
    if ((rc = stage_frames(c, frames, frames_on_device, batch, rows, cols, a.frames))) return rc;
    a.batch = batch;
    a.rows = rows;
    a.cols = cols;
    a.tiles_x = opts->tiles_x;
    a.tiles_y = opts->tiles_y;
    a.clip_milli = opts->clip_milli;
    const size_t lut_bytes = static_cast<size_t>(batch) * opts->tiles_y * opts->tiles_x * 256;  // (a multiple of 4: tab is aligned)
    FD_HIP_TRY(c, ensure_as(c, c->e_ws, lut_bytes + sizeof(uint32_t) * (static_cast<size_t>(cols) + rows), a.luts));
    a.tab = reinterpret_cast<uint32_t *>(a.luts + lut_bytes);
    HostIo io(c, out_on_device);  // (host frames have their own buffer: an in-place host call reads that, writes staging[0])
    FD_HIP_TRY(c, io.out(out, static_cast<size_t>(batch) * rows * cols, a.out));
    FD_HIP_TRY(c, fdk::launch_equalize(a, c->stream));
    if ((rc = io.finish(nullptr, batch, 0))) return rc;  // host out: copied back, synchronised
    if (out_on_device && !all_dev) FD_HIP_TRY(c, hipStreamSynchronize(c->stream));  // the caller's host frames have been read
    return FD_OK;
}

}  // extern "C"
