// OpticalFlowLK over libfdhip.so (fd_pyr_build, fd_flow_lk): an MI355X extension, the reference has no
// tracker. The C ABI hands out no device memory but the context's staging buffer, so a call builds both
// frames' pyramids on the GPU with host output (fd_pyr_build: up, k_pyr_down, back), uploads the two packed
// pyramids again in one fd_ctx_stage and tracks every feature in one kernel launch (two with the
// forward-backward check). That is a round trip over PCIe of 4/3 of each frame and three synchronisations
// more than a caller of the C ABI or of the Python API pays, who keeps the pyramids in device memory of its
// own; the class is the convenience form for host images.
#include "feature_detector/optical_flow_lk.h"

#include "fd_hip.h"
#include "vec2_pack.h"

namespace feature_detector {

OpticalFlowLK::~OpticalFlowLK() = default;

bool OpticalFlowLK::Track(const GrayImage &prev, const GrayImage &next, const std::vector<Vec2> &prev_uv,
                          std::vector<Vec2> &next_uv, std::vector<uint8_t> &status, std::vector<float> *error,
                          const std::vector<Vec2> *guess_uv) {
    const size_t n = prev_uv.size();
    next_uv = prev_uv;
    status.assign(n, kInvalid);
    if (error) error->assign(n, -1.0f);
    if (n == 0) return context_.Fail("Track: no features");
    if (guess_uv && guess_uv->size() != n) return context_.Fail("Track: one guess per feature is needed");
    if (!prev.data() || !next.data() || prev.rows() < 1 || prev.cols() < 1) return context_.Fail("Track: empty image");
    if (prev.rows() != next.rows() || prev.cols() != next.cols()) return context_.Fail("Track: the images differ in size");
    const int rows = prev.rows(), cols = prev.cols(), levels = options_.kLevels;
    int64_t off[FD_PYR_MAX_LEVELS + 1];
    if (levels < 1 || levels > FD_PYR_MAX_LEVELS || fd_pyr_layout(1, rows, cols, levels, off) != FD_OK)
        return context_.Fail("Track: kLevels must be in 1..6 and the top level must keep a pixel");
    fd_ctx *ctx = context_.Acquire();
    if (!ctx) return false;
    const size_t total = static_cast<size_t>(off[levels]);
    pyramids_.resize(2 * total);
    if (fd_pyr_build(ctx, prev.data(), 0, 1, rows, cols, levels, pyramids_.data(), 0) != FD_OK ||
        fd_pyr_build(ctx, next.data(), 0, 1, rows, cols, levels, pyramids_.data() + total, 0) != FD_OK)
        return context_.FailCall("fd_pyr_build");
    const uint8_t *device = nullptr;
    if (fd_ctx_stage(ctx, pyramids_.data(), static_cast<int64_t>(2 * total), &device) != FD_OK)
        return context_.FailCall("fd_ctx_stage");
    const std::vector<float> xy = Flatten(prev_uv), guess = guess_uv ? Flatten(*guess_uv) : std::vector<float>();
    std::vector<float> out(2 * n);
    const fd_flow_opts o{options_.kHalfWindow, options_.kMaxIterations, options_.kEpsilon, options_.kMinEigen,
                         options_.kMaxForwardBackward, options_.kMaxError};
    const int rc = fd_flow_lk(ctx, 1, rows, cols, levels, &o, device, device + total, xy.data(), nullptr, nullptr,
                              static_cast<int32_t>(n), guess_uv ? guess.data() : nullptr, out.data(), status.data(),
                              error ? error->data() : nullptr, nullptr, 0);
    if (rc != FD_OK) {
        status.assign(n, kInvalid);
        return context_.FailCall("fd_flow_lk");
    }
    next_uv = Unflatten(out.data(), n);
    return true;
}

}  // namespace feature_detector
