// GeometricVerifier over libfdhip.so (fd_ransac): an MI355X extension, the reference has no such stage.
// One host-pointer call per Verify: the positions go up, three kernels run, the mask and the model come back.
// Refit, RecoverPose and Triangulate are one host-pointer call each as well (fd_ransac_refit, fd_pose_recover,
// fd_triangulate), and so are SolvePnP, RefinePnP, BundleAdjust, AlignPoints, RefineAlignment and TransformPoints.
// A method is its size checks, its options struct and its call; what the three RANSAC methods and the three refit
// methods do before and after their call is written once (Begin, NoModel, RansacDone, RefitDone).
#include "feature_detector/geometric_verifier.h"

#include <algorithm>

#include "fd_hip.h"
#include "vec2_pack.h"

namespace feature_detector {

namespace {

// An optional array's data, or nullptr.
template <class T>
const T *Data(const std::vector<T> *v) {
    return v ? v->data() : nullptr;
}

// After a method's size checks (why: what does not fit, or nullptr): the context, or nullptr with the failure reported.
fd_ctx *Begin(DeviceContext &context, const char *method, const char *why) {
    if (why) {
        context.Fail(std::string(method) + ": " + why);
        return nullptr;
    }
    return context.Acquire();
}

// The outputs of Verify, SolvePnP and AlignPoints before their call and after one that failed: no inlier, a zero model,
// no hypothesis.
template <size_t W>
void NoModel(size_t n, std::vector<uint8_t> &inlier, std::array<double, W> *model, int32_t *best_hypothesis) {
    inlier.assign(n, 0);
    if (model) model->fill(0.0);
    if (best_hypothesis) *best_hypothesis = -1;
}

// What those three do with their call's status rc and its winner `best`.
template <size_t W>
bool RansacDone(DeviceContext &context, int rc, const char *call, const char *no_model, int32_t best, std::vector<uint8_t> &inlier,
                std::array<double, W> *model, int32_t *best_hypothesis) {
    if (rc != FD_OK) {
        NoModel(inlier.size(), inlier, model, best_hypothesis);
        return context.FailCall(call);
    }
    if (best < 0) return context.Fail(no_model);
    if (best_hypothesis) *best_hypothesis = best;
    return true;
}

// What Refit, RefinePnP and RefineAlignment do with their call's status rc: a failed call leaves the inliers and the
// model as given; otherwise both are replaced by the call's (out_inlier, m) and the accepted rounds are reported.
template <size_t W>
bool RefitDone(DeviceContext &context, int rc, const char *call, std::vector<uint8_t> &inlier, std::vector<uint8_t> &out_inlier,
               std::array<double, W> &model, const std::array<double, W> &m, int32_t accepted, int32_t *accepted_rounds) {
    if (rc != FD_OK) return context.FailCall(call);
    inlier.swap(out_inlier);
    model = m;
    if (accepted_rounds) *accepted_rounds = accepted;
    return true;
}

// The size checks of the calls on image pairs; nullptr when the arguments fit. inlier: nullptr where the call has none.
const char *PairSizes(size_t n, size_t trains, const std::vector<uint8_t> *inlier, const std::vector<int32_t> *train_index,
                      const std::vector<uint8_t> *valid) {
    if (n == 0) return "no query points";
    if (inlier && inlier->size() != n) return "one inlier flag per query point is needed";
    if (train_index && train_index->size() != n) return "one train index per query point is needed";
    if (valid && valid->size() != n) return "one valid flag per query point is needed";
    if (!train_index && trains < n) return "without train_index every query point needs its train point";
    return nullptr;
}

// The train (or image) positions as floats, with two floats of padding behind them.
std::vector<float> FlattenPadded(const std::vector<Vec2> &uv) {
    std::vector<float> t = Flatten(uv);
    t.resize(t.size() + 2);
    return t;
}

}  // namespace

GeometricVerifier::~GeometricVerifier() = default;

void GeometricVerifier::SetImageSize(int32_t rows, int32_t cols) {
    options_.kCenterX = static_cast<float>((cols - 1) / 2.0);
    options_.kCenterY = static_cast<float>((rows - 1) / 2.0);
    options_.kScale = static_cast<float>(2.0 / (static_cast<double>(rows) + cols));
}

bool GeometricVerifier::Verify(const std::vector<Vec2> &query_uv, const std::vector<Vec2> &train_uv,
                               std::vector<uint8_t> &inlier, const std::vector<int32_t> *train_index,
                               const std::vector<uint8_t> *valid, std::array<double, 9> *model, int32_t *best_hypothesis) {
    const size_t n = query_uv.size();
    NoModel(n, inlier, model, best_hypothesis);
    fd_ctx *ctx = Begin(context_, "Verify", PairSizes(n, train_uv.size(), nullptr, train_index, valid));
    if (!ctx) return false;
    const std::vector<float> q = Flatten(query_uv);
    const std::vector<float> t = FlattenPadded(train_uv);
    const fd_ransac_opts o{options_.kModel, options_.kHypotheses, options_.kSeed, options_.kThreshold,
                           options_.kCenterX, options_.kCenterY, options_.kScale};
    std::array<double, 9> m{};  // the model is optional: a failed call or one without a winner leaves *model zero
    int32_t best = -1;
    const int rc = fd_ransac(ctx, 1, &o, q.data(), nullptr, static_cast<int32_t>(n), t.data(), static_cast<int32_t>(train_uv.size()),
                             Data(train_index), Data(valid), m.data(), inlier.data(), nullptr, &best, 0);
    if (!RansacDone<9>(context_, rc, "fd_ransac", "Verify: no model (too few correspondences, or every sample degenerate)", best,
                       inlier, nullptr, best_hypothesis))
        return false;
    if (model) *model = m;
    return true;
}

bool GeometricVerifier::Refit(const std::vector<Vec2> &query_uv, const std::vector<Vec2> &train_uv, std::vector<uint8_t> &inlier,
                              std::array<double, 9> &model, int32_t rounds, const std::vector<int32_t> *train_index,
                              const std::vector<uint8_t> *valid, int32_t *accepted_rounds) {
    const size_t n = query_uv.size();
    if (accepted_rounds) *accepted_rounds = 0;
    fd_ctx *ctx = Begin(context_, "Refit", PairSizes(n, train_uv.size(), &inlier, train_index, valid));
    if (!ctx) return false;
    const std::vector<float> q = Flatten(query_uv);
    const std::vector<float> t = FlattenPadded(train_uv);
    const fd_refit_opts o{options_.kModel, rounds, options_.kThreshold, options_.kCenterX, options_.kCenterY, options_.kScale};
    std::vector<uint8_t> out_inlier(n);
    std::array<double, 9> m;
    int32_t accepted = 0;
    const int rc = fd_ransac_refit(ctx, 1, &o, q.data(), nullptr, static_cast<int32_t>(n), t.data(),
                                   static_cast<int32_t>(train_uv.size()), Data(train_index), Data(valid), model.data(),
                                   inlier.data(), m.data(), out_inlier.data(), nullptr, &accepted, 0);
    return RefitDone(context_, rc, "fd_ransac_refit", inlier, out_inlier, model, m, accepted, accepted_rounds);
}

namespace {

fd_pose_opts PoseOpts(const GeometricVerifier::Camera &q, const GeometricVerifier::Camera &t, const GeometricVerifier::PoseOptions &o) {
    return fd_pose_opts{q.fx, q.fy, q.cx, q.cy, t.fx, t.fy, t.cx, t.cy, o.kMaxDepth, o.kMinParallax};
}

}  // namespace

bool GeometricVerifier::RecoverPose(const std::vector<Vec2> &query_uv, const std::vector<Vec2> &train_uv,
                                    const std::vector<uint8_t> &inlier, const std::array<double, 9> &model,
                                    const Camera &query_camera, const Camera &train_camera, std::array<double, 12> &pose,
                                    std::vector<std::array<float, 3>> &points, std::vector<uint8_t> &point_valid,
                                    const std::vector<int32_t> *train_index, const std::vector<uint8_t> *valid, int32_t *choice) {
    const size_t n = query_uv.size();
    pose.fill(0.0);
    points.assign(n, std::array<float, 3>{0.0f, 0.0f, 0.0f});
    point_valid.assign(n, 0);
    if (choice) *choice = -1;
    fd_ctx *ctx = Begin(context_, "RecoverPose", PairSizes(n, train_uv.size(), &inlier, train_index, valid));
    if (!ctx) return false;
    const std::vector<float> q = Flatten(query_uv);
    const std::vector<float> t = FlattenPadded(train_uv);
    const fd_pose_opts o = PoseOpts(query_camera, train_camera, pose_options_);
    int32_t won = -1;
    const int rc = fd_pose_recover(ctx, 1, &o, q.data(), nullptr, static_cast<int32_t>(n), t.data(),
                                   static_cast<int32_t>(train_uv.size()), Data(train_index), Data(valid), model.data(),
                                   inlier.data(), pose.data(), &won, points[0].data(), point_valid.data(), nullptr, 0);
    if (rc != FD_OK) {
        pose.fill(0.0);
        points.assign(n, std::array<float, 3>{0.0f, 0.0f, 0.0f});
        point_valid.assign(n, 0);
        return context_.FailCall("fd_pose_recover");
    }
    if (won < 0) return context_.Fail("RecoverPose: no pose (a degenerate model, a pure rotation, or no inlier in front)");
    if (choice) *choice = won;
    return true;
}

bool GeometricVerifier::Triangulate(const std::vector<Vec2> &query_uv, const std::vector<Vec2> &train_uv,
                                    const std::array<double, 12> &pose, const Camera &query_camera, const Camera &train_camera,
                                    std::vector<std::array<float, 3>> &points, std::vector<uint8_t> &point_valid,
                                    const std::vector<uint8_t> *inlier, const std::vector<int32_t> *train_index,
                                    const std::vector<uint8_t> *valid, int32_t *count) {
    const size_t n = query_uv.size();
    points.assign(n, std::array<float, 3>{0.0f, 0.0f, 0.0f});
    point_valid.assign(n, 0);
    if (count) *count = 0;
    fd_ctx *ctx = Begin(context_, "Triangulate", PairSizes(n, train_uv.size(), inlier, train_index, valid));
    if (!ctx) return false;
    const std::vector<float> q = Flatten(query_uv);
    const std::vector<float> t = FlattenPadded(train_uv);
    const fd_pose_opts o = PoseOpts(query_camera, train_camera, pose_options_);
    int32_t found = 0;
    const int rc = fd_triangulate(ctx, 1, &o, q.data(), nullptr, static_cast<int32_t>(n), t.data(),
                                  static_cast<int32_t>(train_uv.size()), Data(train_index), Data(valid), pose.data(), Data(inlier),
                                  points[0].data(), point_valid.data(), &found, 0);
    if (rc != FD_OK) {
        points.assign(n, std::array<float, 3>{0.0f, 0.0f, 0.0f});
        point_valid.assign(n, 0);
        return context_.FailCall("fd_triangulate");
    }
    if (count) *count = found;
    return true;
}

namespace {

// The size checks SolvePnP and RefinePnP share; nullptr when the arguments fit. inlier: nullptr where the call has none.
const char *PnpSizes(size_t n, size_t images, const std::vector<uint8_t> *point_valid, const std::vector<int32_t> *image_index,
                     const std::vector<uint8_t> *valid, const std::vector<uint8_t> *inlier) {
    if (n == 0) return "no points";
    if (point_valid && point_valid->size() != n) return "one point_valid flag per point is needed";
    if (image_index && image_index->size() != n) return "one image index per point is needed";
    if (valid && valid->size() != n) return "one valid flag per point is needed";
    if (!image_index && images < n) return "without image_index every point needs its image position";
    if (inlier && inlier->size() != n) return "one inlier flag per point is needed";
    return nullptr;
}

fd_pnp_opts PnpOpts(const GeometricVerifier::PnpOptions &o, const GeometricVerifier::Camera &c, int32_t rounds) {
    return fd_pnp_opts{o.kHypotheses, o.kSeed, rounds, o.kThreshold, c.fx, c.fy, c.cx, c.cy,
                       {o.kCenter[0], o.kCenter[1], o.kCenter[2]}, o.kScale};
}

}  // namespace

bool GeometricVerifier::SolvePnP(const std::vector<std::array<float, 3>> &points, const std::vector<Vec2> &image_uv,
                                 const Camera &camera, std::array<double, 12> &pose, std::vector<uint8_t> &inlier,
                                 const std::vector<uint8_t> *point_valid, const std::vector<int32_t> *image_index,
                                 const std::vector<uint8_t> *valid, int32_t *best_hypothesis) {
    const size_t n = points.size();
    NoModel(n, inlier, &pose, best_hypothesis);
    fd_ctx *ctx = Begin(context_, "SolvePnP", PnpSizes(n, image_uv.size(), point_valid, image_index, valid, nullptr));
    if (!ctx) return false;
    const std::vector<float> t = FlattenPadded(image_uv);
    const fd_pnp_opts o = PnpOpts(pnp_options_, camera, 1);
    int32_t best = -1;
    const int rc = fd_pnp_ransac(ctx, 1, &o, points[0].data(), Data(point_valid), nullptr, static_cast<int32_t>(n), t.data(),
                                 static_cast<int32_t>(image_uv.size()), Data(image_index), Data(valid), pose.data(), inlier.data(),
                                 nullptr, &best, 0);
    return RansacDone(context_, rc, "fd_pnp_ransac", "SolvePnP: no pose (fewer than 6 correspondences, or every sample degenerate)",
                      best, inlier, &pose, best_hypothesis);
}

bool GeometricVerifier::RefinePnP(const std::vector<std::array<float, 3>> &points, const std::vector<Vec2> &image_uv,
                                  const Camera &camera, std::array<double, 12> &pose, std::vector<uint8_t> &inlier, int32_t rounds,
                                  const std::vector<uint8_t> *point_valid, const std::vector<int32_t> *image_index,
                                  const std::vector<uint8_t> *valid, int32_t *accepted_rounds) {
    const size_t n = points.size();
    if (accepted_rounds) *accepted_rounds = 0;
    fd_ctx *ctx = Begin(context_, "RefinePnP", PnpSizes(n, image_uv.size(), point_valid, image_index, valid, &inlier));
    if (!ctx) return false;
    const std::vector<float> t = FlattenPadded(image_uv);
    const fd_pnp_opts o = PnpOpts(pnp_options_, camera, rounds);
    std::vector<uint8_t> out_inlier(n);
    std::array<double, 12> p;
    int32_t accepted = 0;
    const int rc = fd_pnp_refit(ctx, 1, &o, points[0].data(), Data(point_valid), nullptr, static_cast<int32_t>(n), t.data(),
                                static_cast<int32_t>(image_uv.size()), Data(image_index), Data(valid), pose.data(), inlier.data(),
                                p.data(), out_inlier.data(), nullptr, &accepted, 0);
    return RefitDone(context_, rc, "fd_pnp_refit", inlier, out_inlier, pose, p, accepted, accepted_rounds);
}

bool GeometricVerifier::BundleAdjust(std::vector<std::array<double, 12>> &poses, std::vector<std::array<float, 3>> &points,
                                     const std::vector<std::vector<Vec2>> &observations, const Camera &camera,
                                     std::vector<std::vector<uint8_t>> &inlier,
                                     const std::vector<std::vector<uint8_t>> *observation_valid,
                                     const std::vector<uint8_t> *point_valid, const std::vector<uint8_t> *fixed,
                                     std::array<double, 2> *cost, int32_t *accepted_rounds) {
    const size_t cams = poses.size(), n = points.size();
    if (accepted_rounds) *accepted_rounds = 0;
    inlier.assign(cams, std::vector<uint8_t>(n, 0));
    if (cams < 1 || cams > FD_BA_MAX_CAMS) return context_.Fail("BundleAdjust: 1 to 8 cameras are needed");
    if (n == 0) return context_.Fail("BundleAdjust: no points");
    if (observations.size() != cams) return context_.Fail("BundleAdjust: one observation vector per camera is needed");
    if (observation_valid && observation_valid->size() != cams)
        return context_.Fail("BundleAdjust: one observation_valid vector per camera is needed");
    for (size_t c = 0; c < cams; ++c) {
        if (observations[c].size() != n) return context_.Fail("BundleAdjust: every camera needs one observation per point");
        if (observation_valid && (*observation_valid)[c].size() != n)
            return context_.Fail("BundleAdjust: one observation_valid flag per observation is needed");
    }
    if (point_valid && point_valid->size() != n) return context_.Fail("BundleAdjust: one point_valid flag per point is needed");
    if (fixed && fixed->size() != cams) return context_.Fail("BundleAdjust: one fixed flag per camera is needed");
    fd_ctx *ctx = context_.Acquire();
    if (!ctx) return false;
    std::vector<float> obs;
    std::vector<uint8_t> ov;
    obs.reserve(2 * cams * n);
    for (size_t c = 0; c < cams; ++c) {
        const std::vector<float> row = Flatten(observations[c]);
        obs.insert(obs.end(), row.begin(), row.end());
        if (observation_valid) ov.insert(ov.end(), (*observation_valid)[c].begin(), (*observation_valid)[c].end());
    }
    const BundleOptions &b = bundle_options_;
    const fd_ba_opts o{b.kRounds, b.kThreshold, camera.fx, camera.fy, camera.cx, camera.cy, b.kLambda, b.kUp, b.kDown};
    std::vector<double> out_poses(12 * cams);
    std::vector<float> out_points(3 * n);
    std::vector<uint8_t> out_inlier(cams * n);
    double out_cost[2] = {0.0, 0.0};
    int32_t accepted = 0;
    const int rc = fd_bundle_adjust(ctx, 1, static_cast<int>(cams), &o, poses[0].data(), Data(fixed), points[0].data(),
                                    Data(point_valid), nullptr, static_cast<int32_t>(n), obs.data(),
                                    observation_valid ? ov.data() : nullptr, static_cast<int32_t>(n), out_poses.data(),
                                    out_points.data(), out_inlier.data(), nullptr, out_cost, &accepted, 0);
    if (rc != FD_OK) return context_.FailCall("fd_bundle_adjust");
    for (size_t c = 0; c < cams; ++c) {
        std::copy(out_poses.begin() + 12 * c, out_poses.begin() + 12 * (c + 1), poses[c].begin());
        inlier[c].assign(out_inlier.begin() + c * n, out_inlier.begin() + (c + 1) * n);
    }
    for (size_t i = 0; i < n; ++i) std::copy(out_points.begin() + 3 * i, out_points.begin() + 3 * (i + 1), points[i].begin());
    if (cost) *cost = {out_cost[0], out_cost[1]};
    if (accepted_rounds) *accepted_rounds = accepted;
    return true;
}

namespace {

// The size checks AlignPoints and RefineAlignment share; nullptr when the arguments fit. inlier: nullptr where the call
// has none.
const char *AlignSizes(size_t n, size_t targets, const std::vector<uint8_t> *source_valid, const std::vector<uint8_t> *target_valid,
                       const std::vector<int32_t> *target_index, const std::vector<uint8_t> *valid,
                       const std::vector<uint8_t> *inlier) {
    if (n == 0) return "no source points";
    if (source_valid && source_valid->size() != n) return "one source_valid flag per source point is needed";
    if (target_valid && target_valid->size() != targets) return "one target_valid flag per target point is needed";
    if (target_index && target_index->size() != n) return "one target index per source point is needed";
    if (valid && valid->size() != n) return "one valid flag per source point is needed";
    if (!target_index && targets < n) return "without target_index every source point needs its target point";
    if (inlier && inlier->size() != n) return "one inlier flag per source point is needed";
    return nullptr;
}

// The target points, or one zero point where there are none (an index may still be given: no entry is in range).
const float *TargetData(const std::vector<std::array<float, 3>> &target) {
    static const float none[3] = {0.0f, 0.0f, 0.0f};
    return target.empty() ? none : target[0].data();
}

}  // namespace

bool GeometricVerifier::AlignPoints(const std::vector<std::array<float, 3>> &source, const std::vector<std::array<float, 3>> &target,
                                    std::array<double, 13> &model, std::vector<uint8_t> &inlier,
                                    const std::vector<uint8_t> *source_valid, const std::vector<uint8_t> *target_valid,
                                    const std::vector<int32_t> *target_index, const std::vector<uint8_t> *valid,
                                    int32_t *best_hypothesis) {
    const size_t n = source.size();
    NoModel(n, inlier, &model, best_hypothesis);
    fd_ctx *ctx = Begin(context_, "AlignPoints", AlignSizes(n, target.size(), source_valid, target_valid, target_index, valid, nullptr));
    if (!ctx) return false;
    const fd_align_opts o{align_options_.kKind, align_options_.kHypotheses, align_options_.kSeed, 1, align_options_.kThreshold};
    int32_t best = -1;
    const int rc = fd_align_ransac(ctx, 1, &o, source[0].data(), Data(source_valid), nullptr, static_cast<int32_t>(n),
                                   TargetData(target), Data(target_valid), static_cast<int32_t>(target.size()), Data(target_index),
                                   Data(valid), model.data(), inlier.data(), nullptr, &best, 0);
    return RansacDone(context_, rc, "fd_align_ransac", "AlignPoints: no model (fewer than 3 correspondences, or every sample degenerate)",
                      best, inlier, &model, best_hypothesis);
}

bool GeometricVerifier::RefineAlignment(const std::vector<std::array<float, 3>> &source,
                                        const std::vector<std::array<float, 3>> &target, std::array<double, 13> &model,
                                        std::vector<uint8_t> &inlier, int32_t rounds, const std::vector<uint8_t> *source_valid,
                                        const std::vector<uint8_t> *target_valid, const std::vector<int32_t> *target_index,
                                        const std::vector<uint8_t> *valid, int32_t *accepted_rounds) {
    const size_t n = source.size();
    if (accepted_rounds) *accepted_rounds = 0;
    fd_ctx *ctx = Begin(context_, "RefineAlignment", AlignSizes(n, target.size(), source_valid, target_valid, target_index, valid, &inlier));
    if (!ctx) return false;
    const fd_align_opts o{align_options_.kKind, 1, 0, rounds, align_options_.kThreshold};
    std::vector<uint8_t> out_inlier(n);
    std::array<double, 13> m;
    int32_t accepted = 0;
    const int rc = fd_align_refit(ctx, 1, &o, source[0].data(), Data(source_valid), nullptr, static_cast<int32_t>(n),
                                  TargetData(target), Data(target_valid), static_cast<int32_t>(target.size()), Data(target_index),
                                  Data(valid), model.data(), inlier.data(), m.data(), out_inlier.data(), nullptr, &accepted, 0);
    return RefitDone(context_, rc, "fd_align_refit", inlier, out_inlier, model, m, accepted, accepted_rounds);
}

bool GeometricVerifier::TransformPoints(const std::array<double, 13> &model, std::vector<std::array<float, 3>> &points,
                                        const std::vector<uint8_t> *point_valid) {
    const size_t n = points.size();
    if (n == 0) return context_.Fail("TransformPoints: no points");
    if (point_valid && point_valid->size() != n) return context_.Fail("TransformPoints: one point_valid flag per point is needed");
    fd_ctx *ctx = context_.Acquire();
    if (!ctx) return false;
    std::vector<std::array<float, 3>> out(points);  // the call fails as a whole: points are then left as given
    const int rc = fd_align_apply(ctx, 1, model.data(), points[0].data(), Data(point_valid), nullptr, static_cast<int32_t>(n),
                                  out[0].data(), 0);
    if (rc != FD_OK) return context_.FailCall("fd_align_apply");
    points.swap(out);
    return true;
}

}  // namespace feature_detector
