// ContrastEqualizer over libfdhip.so (fd_frames_equalize): an MI355X extension, the reference has no such
// stage. One call with host pointers: the frame is staged through the context, the LUT and apply kernels run,
// and the destination comes back, complete on return.
#include "feature_detector/contrast_equalizer.h"

#include <cmath>

#include "fd_hip.h"

namespace feature_detector {

ContrastEqualizer::~ContrastEqualizer() = default;

bool ContrastEqualizer::Equalize(const GrayImage &src, GrayImage &dst) {
    if (!src.data() || src.rows() < 1 || src.cols() < 1) return context_.Fail("Equalize: empty source image");
    if (!dst.data() || dst.rows() != src.rows() || dst.cols() != src.cols())
        return context_.Fail("Equalize: the destination must have the source's shape");
    if (!(options_.kClipLimit >= 0.0f && options_.kClipLimit <= 2.0e6f))  // (false for NaN)
        return context_.Fail("Equalize: kClipLimit must be in [0, 2e6]");
    fd_ctx *ctx = context_.Acquire();
    if (!ctx) return false;
    const fd_equalize_opts o{options_.kTilesX, options_.kTilesY, static_cast<int32_t>(lroundf(options_.kClipLimit * 1000.0f))};
    const int rc = fd_frames_equalize(ctx, src.data(), 0, 1, src.rows(), src.cols(), &o, dst.data(), 0);
    if (rc != FD_OK) return context_.FailCall("fd_frames_equalize");
    return true;
}

}  // namespace feature_detector
