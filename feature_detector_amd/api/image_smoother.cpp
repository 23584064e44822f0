// ImageSmoother over libfdhip.so (fd_blur_taps, fd_frames_blur): an MI355X extension, the reference has no such
// stage. One call with host pointers: the frame is staged through the context, the kernel runs, and the
// destination comes back, complete on return.
#include "feature_detector/image_smoother.h"

#include <algorithm>

#include "fd_hip.h"

namespace feature_detector {

ImageSmoother::~ImageSmoother() = default;

bool ImageSmoother::Smooth(const GrayImage &src, GrayImage &dst) {
    if (!src.data() || src.rows() < 1 || src.cols() < 1) return context_.Fail("Smooth: empty source image");
    if (options_.kStep != 1 && options_.kStep != 2) return context_.Fail("Smooth: kStep must be 1 or 2");
    const int rows = (src.rows() + options_.kStep - 1) / options_.kStep, cols = (src.cols() + options_.kStep - 1) / options_.kStep;
    if (!dst.data() || dst.rows() != rows || dst.cols() != cols)
        return context_.Fail("Smooth: the destination must be ceil(rows / kStep) x ceil(cols / kStep)");
    if (dst.data() == src.data()) return context_.Fail("Smooth: the destination must not share the source's buffer");
    fd_blur_opts o{};
    if (options_.kTaps.empty()) {
        if (fd_blur_taps(options_.kSigma, options_.kRadius, &o) != FD_OK)
            return context_.Fail("Smooth: kSigma must be finite and > 0");
    } else {
        if (options_.kTaps.size() > FD_BLUR_MAX_RADIUS + 1) return context_.Fail("Smooth: kTaps must have at most 16 entries");
        o.radius = static_cast<int32_t>(options_.kTaps.size()) - 1;
        std::copy(options_.kTaps.begin(), options_.kTaps.end(), o.taps);
    }
    o.step = options_.kStep;
    fd_ctx *ctx = context_.Acquire();
    if (!ctx) return false;
    const int rc = fd_frames_blur(ctx, src.data(), 0, 1, src.rows(), src.cols(), &o, dst.data(), 0);
    if (rc != FD_OK) return context_.FailCall("fd_frames_blur");
    taps_.assign(o.taps, o.taps + o.radius + 1);
    return true;
}

}  // namespace feature_detector
