// ImageWarper over libfdhip.so (fd_frames_warp): an MI355X extension, the reference has no such stage. One
// call with host pointers: the frame and the parameters are staged through the context, the destination is
// written by one kernel launch and comes back, complete on return.
#include "feature_detector/image_warper.h"

#include "fd_hip.h"

namespace feature_detector {

ImageWarper::~ImageWarper() = default;

bool ImageWarper::Warp(const GrayImage &src, const double *params, GrayImage &dst, uint8_t *mask) {
    if (!src.data() || src.rows() < 1 || src.cols() < 1) return context_.Fail("Warp: empty source image");
    if (!dst.data() || dst.rows() < 1 || dst.cols() < 1) return context_.Fail("Warp: empty destination image");
    if (!params) return context_.Fail("Warp: no parameters");
    if (dst.data() == src.data()) return context_.Fail("Warp: the destination must not be the source");
    fd_ctx *ctx = context_.Acquire();
    if (!ctx) return false;
    const fd_warp_opts o{static_cast<int32_t>(options_.kModel), 1, options_.kFill};
    const int rc = fd_frames_warp(ctx, src.data(), 0, 1, src.rows(), src.cols(), &o, params, 0, dst.rows(), dst.cols(),
                                  dst.data(), mask, 0);
    if (rc != FD_OK) return context_.FailCall("fd_frames_warp");
    return true;
}

}  // namespace feature_detector
