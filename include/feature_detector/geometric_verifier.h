// GeometricVerifier: RANSAC verification of point correspondences (matches or tracks) against a fundamental
// matrix or a homography over the MI355X kernels of libfdhip.so (fd_ransac).
//
// MI355X extension: the reference has no such stage, although the survivors of a geometric check are what
// a front end hands to DetectGoodFeatures(image, need, features) as the features it already has. The
// semantics, a definite arithmetic sequence (a counter-based sampler, a fixed number of hypotheses that are
// all evaluated, one solve in double each), are those of fd_ransac (include/fd_hip.h): the model is the
// best minimal-sample model, not a refit.
#ifndef FEATURE_DETECTOR_GEOMETRIC_VERIFIER_H_
#define FEATURE_DETECTOR_GEOMETRIC_VERIFIER_H_

#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "device_context.h"
#include "fd_types.h"

namespace feature_detector {

/* Class GeometricVerifier Declaration. */
class GeometricVerifier {
public:
    enum Model : int32_t { kFundamental = 0, kHomography = 1 };  // 8-point and 4-point minimal samples

    struct Options {
        Model kModel = kFundamental;
        int32_t kHypotheses = 256;   // 1..4096, all evaluated
        uint32_t kSeed = 0;
        float kThreshold = 1.0f;     // pixels: Sampson distance (fundamental), forward transfer error (homography)
        // the fixed conditioning transform (x - center) * scale applied to every coordinate; SetImageSize
        // fills the three from an image size
        float kCenterX = 0.0f;
        float kCenterY = 0.0f;
        float kScale = 1.0f / 256.0f;
    };

public:
    GeometricVerifier() = default;
    virtual ~GeometricVerifier();
    GeometricVerifier(const GeometricVerifier &) = delete;
    GeometricVerifier &operator=(const GeometricVerifier &) = delete;

    // center = ((cols - 1) / 2, (rows - 1) / 2), scale = 2 / (rows + cols)
    void SetImageSize(int32_t rows, int32_t cols);

    // Verifies the correspondences query_uv[i] <-> train_uv[train_index[i]] (a matcher's output; -1 and
    // out-of-range entries take no part), or query_uv[i] <-> train_uv[i] without train_index (tracks).
    // valid (optional, one flag per query point): only the points flagged exactly 1 take part, so
    // OpticalFlowLK's status passes as it is. inlier[i]: 1 if correspondence i is an inlier of the best
    // model. model (optional): row-major 3 x 3 in pixel coordinates, its largest entry 1.0. best_hypothesis
    // (optional): the index of the winning sample.
    // False, with inlier all 0 and a zero model, when no model is found (fewer correspondences than a
    // sample needs, or every sample degenerate), for no query points, a train_index or valid of the wrong
    // size, fewer train than query points without train_index, options out of range, or a libfdhip
    // failure (last_error()).
    bool Verify(const std::vector<Vec2> &query_uv, const std::vector<Vec2> &train_uv, std::vector<uint8_t> &inlier,
                const std::vector<int32_t> *train_index = nullptr, const std::vector<uint8_t> *valid = nullptr,
                std::array<double, 9> *model = nullptr, int32_t *best_hypothesis = nullptr);

    // Refits Verify's model on its inliers by least squares (fd_ransac_refit of include/fd_hip.h): up to
    // `rounds` (1..4) times the model is fitted to the inliers and the inliers are classified again, while
    // their number does not fall; a fundamental matrix comes back with rank 2. query_uv, train_uv,
    // train_index and valid are what Verify took; inlier and model are what it returned and receive the
    // result. accepted_rounds (optional): the rounds taken; with 0 (too few or degenerate inliers, or fewer
    // inliers than before) model keeps its bits and inlier its members.
    // False for no query points, an inlier, train_index or valid of the wrong size, fewer train than query
    // points without train_index, options or rounds out of range, or a libfdhip failure (last_error()); inlier
    // and model are then left as given.
    bool Refit(const std::vector<Vec2> &query_uv, const std::vector<Vec2> &train_uv, std::vector<uint8_t> &inlier,
               std::array<double, 9> &model, int32_t rounds = 2, const std::vector<int32_t> *train_index = nullptr,
               const std::vector<uint8_t> *valid = nullptr, int32_t *accepted_rounds = nullptr);

    // Reference for member variables.
    Options &options() { return options_; }
    const Options &options() const { return options_; }

    void set_device(int device) { context_.set_device(device); }
    int device() const { return context_.device(); }
    const std::string &last_error() const { return context_.last_error(); }

private:
    Options options_;
    DeviceContext context_;
};

}  // namespace feature_detector

#endif  // FEATURE_DETECTOR_GEOMETRIC_VERIFIER_H_
