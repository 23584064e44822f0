// CornerRefiner over libfdhip.so (fd_points_refine): an MI355X extension, the reference's detectors stop at
// integer pixels. One call with host pointers: the frame and the feature arrays are staged through the
// context, every feature is refined in one kernel launch, the results come back, complete on return.
#include "feature_detector/corner_refiner.h"

#include <cstdio>
#include <cstdlib>

#include "fd_hip.h"

namespace feature_detector {

CornerRefiner::~CornerRefiner() {
    if (ctx_) fd_ctx_destroy(ctx_);
}

void CornerRefiner::set_device(int device) {
    if (ctx_ && device != device_) {
        fd_ctx_destroy(ctx_);
        ctx_ = nullptr;
    }
    device_ = device;
}

fd_ctx *CornerRefiner::Context() {
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

bool CornerRefiner::Fail(const std::string &what) {
    error_ = what;
    std::fprintf(stderr, "[feature_detector] %s\n", error_.c_str());
    return false;
}

bool CornerRefiner::Refine(const GrayImage &image, std::vector<Vec2> &uv, std::vector<uint8_t> &status) {
    const size_t n = uv.size();
    status.assign(n, kInvalid);
    if (n == 0) return Fail("Refine: no features");
    if (!image.data() || image.rows() < 1 || image.cols() < 1) return Fail("Refine: empty image");
    fd_ctx *ctx = Context();
    if (!ctx) return false;
    std::vector<float> xy(2 * n);
    for (size_t i = 0; i < n; ++i) {
        xy[2 * i] = uv[i].x();
        xy[2 * i + 1] = uv[i].y();
    }
    const fd_refine_opts o{options_.kHalfWindow, options_.kMaxIterations, options_.kEpsilon, options_.kMinEigen,
                           options_.kMaxShift < 0.0f ? static_cast<float>(options_.kHalfWindow) : options_.kMaxShift};
    const int rc = fd_points_refine(ctx, image.data(), 0, 1, image.rows(), image.cols(), &o, xy.data(), nullptr, nullptr,
                                    static_cast<int32_t>(n), xy.data(), status.data(), nullptr, 0);
    if (rc != FD_OK) {
        status.assign(n, kInvalid);
        return Fail(std::string("fd_points_refine: ") + fd_last_error(ctx));
    }
    for (size_t i = 0; i < n; ++i) uv[i] = Vec2(xy[2 * i], xy[2 * i + 1]);
    return true;
}

}  // namespace feature_detector
