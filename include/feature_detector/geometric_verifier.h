// GeometricVerifier: RANSAC verification of point correspondences (matches or tracks) against a fundamental
// matrix or a homography over the MI355X kernels of libfdhip.so (fd_ransac).
//
// MI355X extension: the reference has no such stage, although the survivors of a geometric check are what
// a front end hands to DetectGoodFeatures(image, need, features) as the features it already has. The
// semantics, a definite arithmetic sequence (a counter-based sampler, a fixed number of hypotheses that are
// all evaluated, one solve in double each), are those of fd_ransac (include/fd_hip.h): the model is the
// best minimal-sample model, not a refit. Refit refits it (fd_ransac_refit); RecoverPose and Triangulate turn a
// fundamental matrix into the relative camera pose and the inliers' 3-D points (fd_pose_recover, fd_triangulate).
// AlignPoints, RefineAlignment and TransformPoints put two such point sets into one frame (fd_align_*).
#ifndef FEATURE_DETECTOR_GEOMETRIC_VERIFIER_H_
#define FEATURE_DETECTOR_GEOMETRIC_VERIFIER_H_

#include <array>
#include <cstdint>
#include <limits>
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

    // A zero-skew pinhole camera, and what a triangulated point must satisfy.
    struct Camera {
        double fx = 1.0, fy = 1.0, cx = 0.0, cy = 0.0;
    };
    struct PoseOptions {
        float kMaxDepth = std::numeric_limits<float>::infinity();  // no limit; the largest depth along either ray, in units of |t|
        float kMinParallax = 1e-3f;              // the sine of the smallest accepted angle between the two rays
    };

    // The relative camera pose of Verify's / Refit's fundamental matrix and the 3-D points of its inliers
    // (fd_pose_recover of include/fd_hip.h). query_uv, train_uv, train_index and valid are what Verify took,
    // inlier and model what it (or Refit) returned. pose: R row-major, then t of unit length, X_train = R X_query
    // + t: of the four poses the matrix allows, the one with the most inliers in front of both cameras.
    // points[i] (query camera frame, in units of |t|) and point_valid[i] = 1 for every inlier in front; zeros
    // elsewhere. choice (optional): the winning candidate 0..3.
    // False, with a zero pose and no valid point, when there is no pose (a zero or rank-1 model, a pure rotation,
    // no inlier in front), for no query points, an inlier, train_index or valid of the wrong size, fewer train
    // than query points without train_index, a camera or option out of range, or a libfdhip failure.
    bool RecoverPose(const std::vector<Vec2> &query_uv, const std::vector<Vec2> &train_uv, const std::vector<uint8_t> &inlier,
                     const std::array<double, 9> &model, const Camera &query_camera, const Camera &train_camera,
                     std::array<double, 12> &pose, std::vector<std::array<float, 3>> &points, std::vector<uint8_t> &point_valid,
                     const std::vector<int32_t> *train_index = nullptr, const std::vector<uint8_t> *valid = nullptr,
                     int32_t *choice = nullptr);

    // The 3-D points of the correspondences under a known pose (fd_triangulate): a calibrated stereo rig behind
    // OpticalFlowLK, or a pose from elsewhere; t of any length sets the unit. inlier (optional): only the points
    // flagged exactly 1 take part. count (optional): the valid points. False for the size and range errors of
    // RecoverPose or a libfdhip failure.
    bool Triangulate(const std::vector<Vec2> &query_uv, const std::vector<Vec2> &train_uv, const std::array<double, 12> &pose,
                     const Camera &query_camera, const Camera &train_camera, std::vector<std::array<float, 3>> &points,
                     std::vector<uint8_t> &point_valid, const std::vector<uint8_t> *inlier = nullptr,
                     const std::vector<int32_t> *train_index = nullptr, const std::vector<uint8_t> *valid = nullptr,
                     int32_t *count = nullptr);

    PoseOptions &pose_options() { return pose_options_; }
    const PoseOptions &pose_options() const { return pose_options_; }

    // Options of SolvePnP and RefinePnP.
    struct PnpOptions {
        int32_t kHypotheses = 256;   // 1..4096, all evaluated
        uint32_t kSeed = 0;
        float kThreshold = 2.0f;     // pixels: the reprojection error
        // the fixed conditioning (X - center) * scale of the 3-D points in SolvePnP: the scene's centroid and
        // the inverse of its spread are a good choice
        std::array<double, 3> kCenter{{0.0, 0.0, 0.0}};
        double kScale = 1.0;
    };

    // The camera pose of an image against known 3-D points (fd_pnp_ransac of include/fd_hip.h): the 6-point DLT
    // camera matrix with the most inliers among kHypotheses samples, made a rotation and a translation. points[i]
    // <-> image_uv[image_index[i]] (or image_uv[i] without image_index); RecoverPose's / Triangulate's points and
    // point_valid pass as they are (point_valid and valid optional: only the points flagged exactly 1 take
    // part). pose: R row-major, then t, X_camera = R X + t in the points' units. inlier[i]: 1 if point i
    // reprojects within kThreshold pixels.
    // False, with a zero pose and inlier all 0, when there is no pose (fewer than 6 correspondences, every sample
    // degenerate: a planar scene has none), for no points, a mask or index of the wrong size, fewer image
    // positions than points without image_index, a camera or option out of range, or a libfdhip failure.
    bool SolvePnP(const std::vector<std::array<float, 3>> &points, const std::vector<Vec2> &image_uv, const Camera &camera,
                  std::array<double, 12> &pose, std::vector<uint8_t> &inlier, const std::vector<uint8_t> *point_valid = nullptr,
                  const std::vector<int32_t> *image_index = nullptr, const std::vector<uint8_t> *valid = nullptr,
                  int32_t *best_hypothesis = nullptr);

    // Refines SolvePnP's pose on its inliers by Gauss-Newton on the reprojection error (fd_pnp_refit): up to
    // `rounds` (1..8) times, the inliers classified again after each, while their number does not fall. The
    // other arguments are what SolvePnP took; pose and inlier are what it returned and receive the result.
    // accepted_rounds (optional): the rounds taken; with 0 pose keeps its bits and inlier its members.
    // False for the size and range errors of SolvePnP, rounds out of range, or a libfdhip failure; pose and
    // inlier are then left as given.
    bool RefinePnP(const std::vector<std::array<float, 3>> &points, const std::vector<Vec2> &image_uv, const Camera &camera,
                   std::array<double, 12> &pose, std::vector<uint8_t> &inlier, int32_t rounds = 4,
                   const std::vector<uint8_t> *point_valid = nullptr, const std::vector<int32_t> *image_index = nullptr,
                   const std::vector<uint8_t> *valid = nullptr, int32_t *accepted_rounds = nullptr);

    PnpOptions &pnp_options() { return pnp_options_; }
    const PnpOptions &pnp_options() const { return pnp_options_; }

    // Options of BundleAdjust.
    struct BundleOptions {
        int32_t kRounds = 8;         // 1..16 Levenberg-Marquardt trials, accepted and rejected
        float kThreshold = 2.0f;     // pixels: truncation of the cost and the inlier gate
        double kLambda = 1e-3;       // the initial damping, > 0
        double kUp = 10.0;           // its factor after a rejected trial, > 1
        double kDown = 0.1;          // its factor after an accepted trial, in (0, 1]
    };

    // Windowed bundle adjustment (fd_bundle_adjust of include/fd_hip.h): refines the poses of 1..8 cameras and the
    // 3-D points they share, by Levenberg-Marquardt on the reprojection cost truncated at kThreshold pixels. poses[c]:
    // R row-major, then t, X_c = R X + t (SolvePnP's / RefinePnP's / RecoverPose's; the first camera of a two-view
    // start is the identity). observations[c][i] is camera c's image position of points[i]: tracks are slot-aligned
    // (gather matched features first); observation_valid (optional, one vector per camera) and point_valid
    // (optional): only the entries flagged exactly 1 take part. fixed (optional, one flag per camera): a non-zero flag
    // holds the camera; without it camera 0 alone is held (hold two to pin the scale). No free camera is
    // structure-only refinement. poses and points receive the result; inlier[c][i]: 1 if the observation is within
    // kThreshold pixels at the final state. cost (optional): the cost before and after. accepted_rounds
    // (optional): the accepted trials; with 0 poses and points keep their bits.
    // False for no cameras or more than 8, no points, a vector of the wrong size, a camera or option out of range,
    // or a libfdhip failure; poses and points are then left as given.
    bool BundleAdjust(std::vector<std::array<double, 12>> &poses, std::vector<std::array<float, 3>> &points,
                      const std::vector<std::vector<Vec2>> &observations, const Camera &camera,
                      std::vector<std::vector<uint8_t>> &inlier, const std::vector<std::vector<uint8_t>> *observation_valid = nullptr,
                      const std::vector<uint8_t> *point_valid = nullptr, const std::vector<uint8_t> *fixed = nullptr,
                      std::array<double, 2> *cost = nullptr, int32_t *accepted_rounds = nullptr);

    BundleOptions &bundle_options() { return bundle_options_; }
    const BundleOptions &bundle_options() const { return bundle_options_; }

    // Options of AlignPoints and RefineAlignment.
    enum AlignKind : int32_t { kSimilarity = 0, kRigid = 1 };  // Y = s R X + t; rigid: s = 1
    struct AlignOptions {
        AlignKind kKind = kSimilarity;
        int32_t kHypotheses = 256;   // 1..4096, all evaluated
        uint32_t kSeed = 0;
        float kThreshold = 0.1f;     // the distance |Y - (s R X + t)| in the target's units, absolute
    };

    // The similarity (or rigid) transform between two sets of 3-D points (fd_align_ransac of include/fd_hip.h): of
    // kHypotheses 3-point samples the one with the most inliers. source[i] <-> target[target_index[i]] (or target[i]
    // without target_index); RecoverPose's / Triangulate's points and point_valid pass as they are on either side
    // (source_valid, target_valid and valid optional: only the entries flagged exactly 1 take part). model: R
    // row-major, then t, then s, target = s R source + t. inlier[i]: 1 if source point i maps within kThreshold of
    // its target. Planar point sets are fine; duplicate and collinear samples are rejected.
    // False, with a zero model and inlier all 0, when there is no model (fewer than 3 correspondences, every sample
    // degenerate), for no source points, a mask or index of the wrong size, fewer target than source points without
    // target_index, an option out of range, or a libfdhip failure.
    bool AlignPoints(const std::vector<std::array<float, 3>> &source, const std::vector<std::array<float, 3>> &target,
                     std::array<double, 13> &model, std::vector<uint8_t> &inlier, const std::vector<uint8_t> *source_valid = nullptr,
                     const std::vector<uint8_t> *target_valid = nullptr, const std::vector<int32_t> *target_index = nullptr,
                     const std::vector<uint8_t> *valid = nullptr, int32_t *best_hypothesis = nullptr);

    // Refits AlignPoints' model on its inliers in closed form (fd_align_refit): up to `rounds` (1..8) times, the
    // inliers classified again after each, while their number does not fall. The other arguments are what AlignPoints
    // took; model and inlier are what it returned and receive the result. accepted_rounds (optional): the rounds taken;
    // with 0 model keeps its bits and inlier its members. Collinear inliers leave the roll about their line arbitrary.
    // False for the size and range errors of AlignPoints, rounds out of range, or a libfdhip failure; model and inlier
    // are then left as given.
    bool RefineAlignment(const std::vector<std::array<float, 3>> &source, const std::vector<std::array<float, 3>> &target,
                         std::array<double, 13> &model, std::vector<uint8_t> &inlier, int32_t rounds = 4,
                         const std::vector<uint8_t> *source_valid = nullptr, const std::vector<uint8_t> *target_valid = nullptr,
                         const std::vector<int32_t> *target_index = nullptr, const std::vector<uint8_t> *valid = nullptr,
                         int32_t *accepted_rounds = nullptr);

    // points[i] = (float)(s R points[i] + t) for every point (fd_align_apply), or with point_valid for those flagged
    // exactly 1 (the others keep their bits). False for no points, a point_valid of the wrong size, or a libfdhip
    // failure; points are then left as given.
    bool TransformPoints(const std::array<double, 13> &model, std::vector<std::array<float, 3>> &points,
                         const std::vector<uint8_t> *point_valid = nullptr);

    AlignOptions &align_options() { return align_options_; }
    const AlignOptions &align_options() const { return align_options_; }

    // Reference for member variables.
    Options &options() { return options_; }
    const Options &options() const { return options_; }

    void set_device(int device) { context_.set_device(device); }
    int device() const { return context_.device(); }
    const std::string &last_error() const { return context_.last_error(); }

private:
    Options options_;
    PoseOptions pose_options_;
    PnpOptions pnp_options_;
    BundleOptions bundle_options_;
    AlignOptions align_options_;
    DeviceContext context_;
};

}  // namespace feature_detector

#endif  // FEATURE_DETECTOR_GEOMETRIC_VERIFIER_H_
