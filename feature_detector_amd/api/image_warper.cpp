// ImageWarper over libfdhip.so (fd_frames_warp): an MI355X extension, the reference has no such stage. One
// call with host pointers: the frame and the parameters are staged through the context, the destination is
// written by one kernel launch and comes back, complete on return.
#include "feature_detector/image_warper.h"

#include <cstdio>
#include <cstdlib>

#include "fd_hip.h"

namespace feature_detector {

ImageWarper::~ImageWarper() {
    if (ctx_) fd_ctx_destroy(ctx_);
}

void ImageWarper::set_device(int device) {
    if (ctx_ && device != device_) {
        fd_ctx_destroy(ctx_);
        ctx_ = nullptr;
    }
    device_ = device;
}

fd_ctx *ImageWarper::Context() {
    if (!ctx_) {
        int dev = device_;
        if (dev < 0) {
            const char *e = std::getenv("FD_DEVICE");
            dev = e ? std::atoi(e) : 0;
        }
        if (fd_ctx_create(dev, &ctx_) != FD_OK) {
            ctx_ = nullptr;
            Fail("fd_ctx_create failed (no MI355X visible?)");
        }
    }
    return ctx_;
}

bool ImageWarper::Fail(const std::string &what) {
    error_ = what;
    std::fprintf(stderr, "[feature_detector] %s\n", error_.c_str());
    return false;
}

bool ImageWarper::Warp(const GrayImage &src, const double *params, GrayImage &dst, uint8_t *mask) {
    if (!src.data() || src.rows() < 1 || src.cols() < 1) return Fail("Warp: empty source image");
    if (!dst.data() || dst.rows() < 1 || dst.cols() < 1) return Fail("Warp: empty destination image");
    if (!params) return Fail("Warp: no parameters");
    if (dst.data() == src.data()) return Fail("Warp: the destination must not be the source");
    fd_ctx *ctx = Context();
    if (!ctx) return false;
    const fd_warp_opts o{static_cast<int32_t>(options_.kModel), 1, options_.kFill};
    const int rc = fd_frames_warp(ctx, src.data(), 0, 1, src.rows(), src.cols(), &o, params, 0, dst.rows(), dst.cols(),
                                  dst.data(), mask, 0);
    if (rc != FD_OK) return Fail(std::string("fd_frames_warp: ") + fd_last_error(ctx));
    return true;
}

}  // namespace feature_detector
