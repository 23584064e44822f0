// Host runtime of libfdhip.so, the C ABI declared in include/fd_hip.h: the context (its stream, its
// grow-only device workspace, the status words) and the staging of host frames and prior features.
// The stages are in fd_rt_points.cpp (point detectors), fd_rt_select.cpp (selection driver),
// fd_rt_lsd.cpp (LSD map and lines), fd_rt_stages.cpp (PNG, BRIEF compute, NN), fd_rt_match.cpp (the two
// descriptor matchers), fd_rt_flow.cpp (pyramid, tracker), fd_rt_refine.cpp (corner refinement) and
// fd_rt_ransac.cpp (RANSAC); fd_ctx.h is their shared header. The keypoint stages' host-pointer calls all
// go through one staging path, HostIo, below.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "fd_ctx.h"

namespace fdrt {

const char *ab_env(const char *name) {
    const char *on = std::getenv("FD_DEBUG_AB");
    if (!on || !*on || std::strcmp(on, "0") == 0) return nullptr;
    return std::getenv(name);
}

int fail(fd_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return code;
}

// Grow-only workspace. Growing while the context stream is being captured into a HIP graph would put
// an allocation into the capture: that fails here with hipErrorStreamCaptureUnsupported (reserve the
// shape first, fd_ctx_reserve, or run the call once before capturing).
hipError_t ensure(fd_ctx *c, DevBuf &b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.n >= bytes) return hipSuccess;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (c && c->stream && hipStreamIsCapturing(c->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        return hipErrorStreamCaptureUnsupported;
    if (b.p) {
        hipError_t e = hipFree(b.p);
        if (e != hipSuccess) return e;
        b.p = nullptr;
        b.n = 0;
    }
    const size_t want = bytes + 256;  // slack: whole-dword loads near the end stay inside the allocation
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) return e;
    b.n = want;
    return hipSuccess;
}

hipError_t ensure_host(HostBuf &b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.n >= bytes) return hipSuccess;
    if (b.p) {
        hipError_t e = hipHostFree(b.p);
        if (e != hipSuccess) return e;
        b.p = nullptr;
        b.n = 0;
    }
    const size_t want = bytes + bytes / 4;  // headroom: batches vary in valid-pixel counts
    hipError_t e = hipHostMalloc(&b.p, want, hipHostMallocDefault);
    if (e != hipSuccess) return e;
    b.n = want;
    return hipSuccess;
}

int check_shape(fd_ctx *c, int kind, int batch, int rows, int cols, bool points) {
    if (!c) return FD_ERR_INVALID;
    if (kind < FD_HARRIS || kind > FD_FAST) return fail(c, FD_ERR_INVALID, "unknown detector kind");
    if (batch < 1 || rows < 1 || cols < 1) return fail(c, FD_ERR_INVALID, "batch, rows and cols must be >= 1");
    // the selection grid packs (x, y) into 16 bits each
    if (points && (rows > 65535 || cols > 65535)) return fail(c, FD_ERR_INVALID, "rows and cols must be <= 65535");
    if (static_cast<int64_t>(rows) * cols >= (int64_t(1) << 31)) return fail(c, FD_ERR_INVALID, "frame too large");
    return FD_OK;
}

int stage_frames(fd_ctx *c, const uint8_t *frames, int on_device, int batch, int rows, int cols,
                 const uint8_t *&dframes) {
    if (frames == nullptr) return fail(c, FD_ERR_INVALID, "frames is NULL");  // feature_point_detector.cpp:9
    const size_t bytes = static_cast<size_t>(batch) * rows * cols;
    if (on_device) {
        dframes = frames;
        return FD_OK;
    }
    FD_HIP_TRY(c, ensure_as(c, c->frames, bytes, dframes));
    FD_HIP_TRY(c, hipMemcpyAsync(c->frames.p, frames, bytes, hipMemcpyHostToDevice, c->stream));
    return FD_OK;
}

int prior_buffers(fd_ctx *c, int batch, int rows, int cols, int64_t total) {
    FD_HIP_TRY(c, ensure(c, c->prior_counts, sizeof(int32_t) * batch));
    if (total <= 0) return FD_OK;
    FD_HIP_TRY(c, ensure(c, c->prior_xy, sizeof(float) * 2 * total));
    FD_HIP_TRY(c, ensure(c, c->prior_frame, sizeof(int32_t) * total));
    FD_HIP_TRY(c, ensure(c, c->mask, sizeof(uint32_t) * static_cast<size_t>(batch) * rows * ((cols + 31) / 32)));
    return FD_OK;
}

int setup_priors(fd_ctx *c, int batch, int rows, int cols, int dist, const float *prior_xy,
                 const int32_t *prior_counts, PriorInfo &pi) {
    pi = PriorInfo{};
    if (prior_counts == nullptr) return FD_OK;
    for (int b = 0; b < batch; ++b) {
        if (prior_counts[b] < 0) return fail(c, FD_ERR_INVALID, "negative prior count");
        pi.total += prior_counts[b];
    }
    if (pi.total > 0 && prior_xy == nullptr)
        return fail(c, FD_ERR_INVALID, "prior_xy is NULL but prior_counts is not zero");
    if (const int rc = prior_buffers(c, batch, rows, cols, pi.total)) return rc;
    FD_HIP_TRY(c, hipMemcpyAsync(c->prior_counts.p, prior_counts, sizeof(int32_t) * batch, hipMemcpyHostToDevice,
                                 c->stream));
    pi.counts_dev = as<int32_t>(c->prior_counts);
    if (pi.total == 0) {
        FD_HIP_TRY(c, hipStreamSynchronize(c->stream));  // prior_counts is caller-owned host memory
        return FD_OK;
    }
    std::vector<int32_t> frame_of;
    frame_of.reserve(static_cast<size_t>(pi.total));
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < prior_counts[b]; ++i) frame_of.push_back(b);
    pi.wpr = (cols + 31) / 32;
    const size_t mbytes = sizeof(uint32_t) * static_cast<size_t>(batch) * rows * pi.wpr;
    FD_HIP_TRY(c, hipMemcpyAsync(c->prior_xy.p, prior_xy, sizeof(float) * 2 * pi.total, hipMemcpyHostToDevice,
                                 c->stream));
    FD_HIP_TRY(c, hipMemcpyAsync(c->prior_frame.p, frame_of.data(), sizeof(int32_t) * pi.total,
                                 hipMemcpyHostToDevice, c->stream));
    FD_HIP_TRY(c, hipMemsetAsync(c->mask.p, 0xFF, mbytes, c->stream));
    FD_HIP_TRY(c, fdk::launch_mask_boxes(as<float>(c->prior_xy), as<int32_t>(c->prior_frame),
                                         static_cast<int>(pi.total), dist, rows, cols, as<uint32_t>(c->mask), pi.wpr,
                                         c->stream));
    // The synchronous copies above read host memory that the caller may free after return.
    FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
    pi.mask = as<uint32_t>(c->mask);
    return FD_OK;
}

int refuse_sync_under_capture(fd_ctx *c, int outputs_on_device) {
    if (outputs_on_device || !c->stream) return FD_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    FD_HIP_TRY(c, hipStreamIsCapturing(c->stream, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return fail(c, FD_ERR_INVALID, "this call synchronises the stream (host outputs): not allowed "
                                       "during stream capture; pass device outputs");
    return FD_OK;
}

int copy_back_written(fd_ctx *c, const int32_t *counts, int batch, int32_t stride, const std::vector<SlotArray> &arrays) {
    for (int b = 0; b < batch; ++b) {
        const int n = counts ? std::min<int64_t>(static_cast<uint32_t>(counts[b]) & fdk::kCountMask, stride) : stride;
        if (n <= 0) continue;
        const size_t s0 = static_cast<size_t>(b) * stride;
        for (const SlotArray &a : arrays)
            if (a.dst)
                FD_HIP_TRY(c, hipMemcpyAsync(static_cast<uint8_t *>(a.dst) + s0 * a.slot_bytes,
                                             static_cast<const uint8_t *>(a.src) + s0 * a.slot_bytes, a.slot_bytes * n,
                                             hipMemcpyDeviceToHost, c->stream));
    }
    FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FD_OK;
}

hipError_t HostIo::stage(const void *p, size_t bytes, bool upload, void *&dev) {
    dev = const_cast<void *>(p);
    if (dev_ || !p) return hipSuccess;
    if (used_ == fd_ctx::kStaging) return hipErrorInvalidValue;  // a call wider than the pool: a programming error
    DevBuf &b = c_->staging[used_++];
    const hipError_t e = ensure(c_, b, bytes);
    if (e != hipSuccess) return e;
    dev = b.p;
    return upload && bytes ? hipMemcpyAsync(dev, p, bytes, hipMemcpyHostToDevice, c_->stream) : hipSuccess;
}

int HostIo::finish(const int32_t *counts, int batch, int32_t stride) {
    if (dev_) return FD_OK;
    for (const SlotArray &a : whole_)
        FD_HIP_TRY(c_, hipMemcpyAsync(a.dst, a.src, a.slot_bytes, hipMemcpyDeviceToHost, c_->stream));
    return copy_back_written(c_, counts, batch, stride, slots_);  // synchronises
}

int set_output(fd_ctx *c, void *out, int byte, size_t bytes, int io_on_device) {
    if (out && io_on_device) FD_HIP_TRY(c, hipMemsetAsync(out, byte, bytes, c->stream));
    if (out && !io_on_device) std::memset(out, byte, bytes);
    return FD_OK;
}

int copy_output(fd_ctx *c, void *out, const void *in, size_t bytes, int io_on_device) {
    if (!out || out == in) return FD_OK;
    if (io_on_device) FD_HIP_TRY(c, hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, c->stream));
    if (!io_on_device) std::memcpy(out, in, bytes);
    return FD_OK;
}

int zero_counts(fd_ctx *c, int32_t *out_counts, int batch, int io_on_device) {
    return set_output(c, out_counts, 0, sizeof(int32_t) * batch, io_on_device);
}

int check_camera(fd_ctx *c, const double *cam, int n, double *out) {
    for (int k = 0; k < n; ++k) {
        if (!std::isfinite(cam[k])) return fail(c, FD_ERR_INVALID, "camera values must be finite");
        out[k] = cam[k];
    }
    for (int k = 0; k < n; k += 4)
        if (cam[k] == 0.0 || cam[k + 1] == 0.0) return fail(c, FD_ERR_INVALID, "fx and fy must be non-zero");
    return FD_OK;
}

int default_line_threads() {
    int t = static_cast<int>(std::thread::hardware_concurrency());
    if (const char *e = std::getenv("OMP_NUM_THREADS"); e && std::atoi(e) > 0) t = std::min(t, std::atoi(e));
    if (const char *e = std::getenv("FD_LINE_THREADS"); e && std::atoi(e) > 0) t = std::atoi(e);
    return std::max(1, t);
}

}  // namespace fdrt

using namespace fdrt;

// The workspace is shared by every call on the context, so a new stream must not start before the
// old one's work: the switch records an event on the old stream and makes the new one wait for it
// (skipped when the new stream is being captured: a capture may not wait on uncaptured work, so the
// caller orders it, e.g. with torch's stream.wait_stream before capturing).
static int switch_stream(fd_ctx *c, hipStream_t s) {
    FD_HIP_TRY(c, hipSetDevice(c->device));
    if (s == c->stream) return FD_OK;
    if (s) {
        int dev = -1;
        FD_HIP_TRY(c, hipStreamGetDevice(s, &dev));
        if (dev != c->device)
            return fail(c, FD_ERR_INVALID, "stream belongs to device " + std::to_string(dev) + ", the context to device " +
                                               std::to_string(c->device));
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    FD_HIP_TRY(c, hipStreamIsCapturing(s, &cs));
    hipStreamCaptureStatus cs_old = hipStreamCaptureStatusNone;
    FD_HIP_TRY(c, hipStreamIsCapturing(c->stream, &cs_old));
    if (cs == hipStreamCaptureStatusNone && cs_old == hipStreamCaptureStatusNone) {
        if (!c->xev) FD_HIP_TRY(c, hipEventCreateWithFlags(&c->xev.p, hipEventDisableTiming));
        FD_HIP_TRY(c, hipEventRecord(c->xev, c->stream));
        FD_HIP_TRY(c, hipStreamWaitEvent(s, c->xev, 0));
    }
    c->stream = s;
    return FD_OK;
}

extern "C" {

const char *fd_build_info(void) {
    return "libfdhip gfx950 (MI355X); kernels: corner response+NMS, FAST-12, greedy select, LSD map; "
           "flags: -O3 -ffp-contract=off";
}

int fd_abi_version(void) { return FD_ABI_VERSION; }

int fd_ctx_create(int device, fd_ctx **out) {
    if (!out) return FD_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return FD_ERR_HIP;
    if (device < 0 || device >= n) return FD_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return FD_ERR_HIP;
    fd_ctx *c = new fd_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->own_stream.p, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return FD_ERR_HIP;
    }
    c->stream = c->own_stream;
    *out = c;
    return FD_OK;
}

void fd_ctx_destroy(fd_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->aux) (void)hipStreamSynchronize(c->aux);
    delete c;  // frees every buffer, then destroys the events, the side stream and the own stream (fd_ctx.h)
}

const char *fd_last_error(const fd_ctx *c) { return c ? c->err.c_str() : "null context"; }

int fd_ctx_set_stream(fd_ctx *c, void *s) {
    if (!c) return FD_ERR_INVALID;
    return switch_stream(c, static_cast<hipStream_t>(s));
}

int fd_ctx_use_own_stream(fd_ctx *c) {
    if (!c) return FD_ERR_INVALID;
    return switch_stream(c, c->own_stream);
}

int fd_ctx_set_tie_order(fd_ctx *c, int order) {
    if (!c) return FD_ERR_INVALID;
    if (order != FD_TIES_RASTER && order != FD_TIES_REFERENCE) return fail(c, FD_ERR_INVALID, "unknown tie order");
    c->tie_order = order;
    return FD_OK;
}

int fd_ctx_frame_status(fd_ctx *c, uint32_t *dst, int batch, int async) {
    if (!c) return FD_ERR_INVALID;
    if (!dst || batch < 0) return fail(c, FD_ERR_INVALID, "bad arguments");
    if (batch > c->status_batch)
        return fail(c, FD_ERR_INVALID, "the last selection call had " + std::to_string(c->status_batch) + " frames");
    if (batch == 0) return FD_OK;
    FD_HIP_TRY(c, hipSetDevice(c->device));
    if (c->h_status_valid && static_cast<size_t>(batch) <= c->h_status.size()) {
        // the last selection call returned host outputs and left its status words here: a host
        // destination is served without a device round trip (device memory still gets a copy)
        hipPointerAttribute_t at{};
        const hipError_t e = hipPointerGetAttributes(&at, dst);
        if (e != hipSuccess) (void)hipGetLastError();  // (unregistered host memory on some runtimes)
        if (e != hipSuccess || at.type == hipMemoryTypeHost || at.type == hipMemoryTypeUnregistered) {
            std::memcpy(dst, c->h_status.data(), sizeof(uint32_t) * batch);
            return FD_OK;
        }
    }
    FD_HIP_TRY(c, hipMemcpyAsync(dst, c->status.p, sizeof(uint32_t) * batch, hipMemcpyDefault, c->stream));
    if (!async) FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FD_OK;
}

void *fd_ctx_get_stream(const fd_ctx *c) { return c ? static_cast<void *>(c->stream) : nullptr; }

int fd_ctx_synchronize(fd_ctx *c) {
    if (!c) return FD_ERR_INVALID;
    FD_HIP_TRY(c, hipSetDevice(c->device));
    FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FD_OK;
}

int fd_ctx_stage(fd_ctx *c, const void *host, int64_t bytes, const uint8_t **device_out) {
    if (!c || !host || bytes < 0 || !device_out) return fail(c, FD_ERR_INVALID, "bad arguments");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    FD_HIP_TRY(c, ensure(c, c->frames, static_cast<size_t>(bytes)));
    FD_HIP_TRY(c, hipMemcpyAsync(c->frames.p, host, static_cast<size_t>(bytes), hipMemcpyHostToDevice, c->stream));
    FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
    *device_out = as<uint8_t>(c->frames);
    return FD_OK;
}

int fd_ctx_reserve(fd_ctx *c, int kind, int batch, int rows, int cols, int64_t max_prior_total) {
    int rc = check_shape(c, kind, batch, rows, cols);
    if (rc) return rc;
    FD_HIP_TRY(c, hipSetDevice(c->device));
    int64_t cap = 0;
    SelectBufs sb{};
    if ((rc = detect_workspace(c, kind, batch, rows, cols, max_prior_total, cap, sb))) return rc;
    if (kind == FD_FAST)  // (the offset table of the shape, at the cached threshold: host work of the first call)
        rc = build_offsets(c, std::max<int64_t>(0, static_cast<int64_t>(rows - 6) * (cols - 6)), c->off_thr);
    return rc;
}

}  // extern "C"
