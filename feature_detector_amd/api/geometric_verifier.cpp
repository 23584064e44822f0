// GeometricVerifier over libfdhip.so (fd_ransac): an MI355X extension, the reference has no such stage.
// One host-pointer call per Verify: the positions go up, three kernels run, the mask and the model come back.
#include "feature_detector/geometric_verifier.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "fd_hip.h"

namespace feature_detector {

GeometricVerifier::~GeometricVerifier() {
    if (ctx_) fd_ctx_destroy(ctx_);
}

void GeometricVerifier::set_device(int device) {
    if (ctx_ && device != device_) {
        fd_ctx_destroy(ctx_);
        ctx_ = nullptr;
    }
    device_ = device;
}

fd_ctx *GeometricVerifier::Context() {
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

bool GeometricVerifier::Fail(const std::string &what) {
    error_ = what;
    std::fprintf(stderr, "[feature_detector] %s\n", error_.c_str());
    return false;
}

void GeometricVerifier::SetImageSize(int32_t rows, int32_t cols) {
    options_.kCenterX = static_cast<float>((cols - 1) / 2.0);
    options_.kCenterY = static_cast<float>((rows - 1) / 2.0);
    options_.kScale = static_cast<float>(2.0 / (static_cast<double>(rows) + cols));
}

bool GeometricVerifier::Verify(const std::vector<Vec2> &query_uv, const std::vector<Vec2> &train_uv,
                               std::vector<uint8_t> &inlier, const std::vector<int32_t> *train_index,
                               const std::vector<uint8_t> *valid, std::array<double, 9> *model, int32_t *best_hypothesis) {
    const size_t n = query_uv.size();
    inlier.assign(n, 0);
    if (model) model->fill(0.0);
    if (best_hypothesis) *best_hypothesis = -1;
    if (n == 0) return Fail("Verify: no query points");
    if (train_index && train_index->size() != n) return Fail("Verify: one train index per query point is needed");
    if (valid && valid->size() != n) return Fail("Verify: one valid flag per query point is needed");
    if (!train_index && train_uv.size() < n) return Fail("Verify: without train_index every query point needs its train point");
    fd_ctx *ctx = Context();
    if (!ctx) return false;
    std::vector<float> q(2 * n), t(2 * train_uv.size() + 2);
    for (size_t i = 0; i < n; ++i) {
        q[2 * i] = query_uv[i].x();
        q[2 * i + 1] = query_uv[i].y();
    }
    for (size_t i = 0; i < train_uv.size(); ++i) {
        t[2 * i] = train_uv[i].x();
        t[2 * i + 1] = train_uv[i].y();
    }
    const fd_ransac_opts o{options_.kModel, options_.kHypotheses, options_.kSeed, options_.kThreshold,
                           options_.kCenterX, options_.kCenterY, options_.kScale};
    double m[9];
    int32_t best = -1;
    const int rc = fd_ransac(ctx, 1, &o, q.data(), nullptr, static_cast<int32_t>(n), t.data(),
                             static_cast<int32_t>(train_uv.size()), train_index ? train_index->data() : nullptr,
                             valid ? valid->data() : nullptr, m, inlier.data(), nullptr, &best, 0);
    if (rc != FD_OK) {
        inlier.assign(n, 0);
        return Fail(std::string("fd_ransac: ") + fd_last_error(ctx));
    }
    if (best < 0) return Fail("Verify: no model (too few correspondences, or every sample degenerate)");
    if (model) std::copy(m, m + 9, model->begin());
    if (best_hypothesis) *best_hypothesis = best;
    return true;
}

}  // namespace feature_detector
