// CornerRefiner over libfdhip.so (fd_points_refine): an MI355X extension, the reference's detectors stop at
// integer pixels. One call with host pointers: the frame and the feature arrays are staged through the
// context, every feature is refined in one kernel launch, the results come back, complete on return.
#include "feature_detector/corner_refiner.h"

#include "fd_hip.h"
#include "vec2_pack.h"

namespace feature_detector {

CornerRefiner::~CornerRefiner() = default;

bool CornerRefiner::Refine(const GrayImage &image, std::vector<Vec2> &uv, std::vector<uint8_t> &status) {
    const size_t n = uv.size();
    status.assign(n, kInvalid);
    if (n == 0) return context_.Fail("Refine: no features");
    if (!image.data() || image.rows() < 1 || image.cols() < 1) return context_.Fail("Refine: empty image");
    fd_ctx *ctx = context_.Acquire();
    if (!ctx) return false;
    std::vector<float> xy = Flatten(uv);
    const fd_refine_opts o{options_.kHalfWindow, options_.kMaxIterations, options_.kEpsilon, options_.kMinEigen,
                           options_.kMaxShift < 0.0f ? static_cast<float>(options_.kHalfWindow) : options_.kMaxShift};
    const int rc = fd_points_refine(ctx, image.data(), 0, 1, image.rows(), image.cols(), &o, xy.data(), nullptr, nullptr,
                                    static_cast<int32_t>(n), xy.data(), status.data(), nullptr, 0);
    if (rc != FD_OK) {
        status.assign(n, kInvalid);
        return context_.FailCall("fd_points_refine");
    }
    uv = Unflatten(xy.data(), n);
    return true;
}

}  // namespace feature_detector
