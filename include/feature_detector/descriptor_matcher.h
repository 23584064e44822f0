// BriefMatcher: nearest-neighbour Hamming matching of BriefType descriptors over the MI355X kernel of
// libfdhip.so (fd_brief_match).
//
// MI355X extension: the reference has no matcher (its demos stop at the descriptors). The semantics are
// those of fd_brief_match (include/fd_hip.h): equal distances go to the lowest train index, an invalid
// descriptor is neither matched nor a candidate, and a best match is reported only if it passes the
// enabled tests of Options. MatchGuided adds the tracker's search window (fd_brief_match_guided): a train
// descriptor is a candidate of a query only if its keypoint lies within (radius_x, radius_y) pixels of the
// query's. MatchModel adds a two-view model (fd_brief_match_model): a train descriptor is a candidate only if
// the pair of keypoints passes the fundamental matrix's Sampson test or the homography's transfer test.
#ifndef FEATURE_DETECTOR_DESCRIPTOR_MATCHER_H_
#define FEATURE_DETECTOR_DESCRIPTOR_MATCHER_H_

#include <cstdint>
#include <string>
#include <vector>

#include "descriptor_brief.h"
#include "device_context.h"

namespace feature_detector {

// The model kinds of MatchModel (FD_RANSAC_FUNDAMENTAL / FD_RANSAC_HOMOGRAPHY of include/fd_hip.h).
enum class MatchModelKind : int32_t { kFundamental = 0, kHomography = 1 };
// A window radius that holds every finite position: MatchModel's default, the model gate alone.
constexpr float kOpenMatchRadius = 3.0e38f;

/* Class BriefMatcher Declaration. */
class BriefMatcher {
public:
    struct Options {
        int32_t kMaxDistance = -1;  // reject a best match farther than this; < 0: no bound
        float kMaxRatio = 0.0f;     // accept only if best < kMaxRatio * second best; <= 0: off
        bool kCrossCheck = false;   // accept q -> t only if t's best query is q
    };

public:
    BriefMatcher() = default;
    virtual ~BriefMatcher();
    BriefMatcher(const BriefMatcher &) = delete;
    BriefMatcher &operator=(const BriefMatcher &) = delete;

    // train_index[i]: the train descriptor matched to query[i], or -1. distance (optional): [i] the raw
    // smallest distance of query[i] to a valid train descriptor, accepted or not (-1: none).
    // query_valid / train_valid (optional, one flag per descriptor): BriefDescriptor leaves all-zero
    // descriptors for keypoints it cannot describe; flag them 0 to keep them out of the matching.
    // False for empty inputs, descriptors of unequal length or a length outside 1..256, flag vectors of
    // the wrong size, or a libfdhip failure (last_error()).
    bool Match(const std::vector<BriefType> &query, const std::vector<BriefType> &train, std::vector<int32_t> &train_index,
               std::vector<int32_t> *distance = nullptr, const std::vector<uint8_t> *query_valid = nullptr,
               const std::vector<uint8_t> *train_valid = nullptr);

    // Match within a search window: train[j] is a candidate of query[i] only if
    // |train_uv[j].x - query_uv[i].x| <= radius_x and |train_uv[j].y - query_uv[i].y| <= radius_y (float,
    // inclusive; a NaN position never matches). query_uv / train_uv: one position per descriptor, as
    // the detector returned them or as a motion model predicts them. Outputs and the return value are
    // Match's; also false for position vectors of the wrong size or a radius that is negative or not finite.
    bool MatchGuided(const std::vector<BriefType> &query, const std::vector<BriefType> &train,
                     const std::vector<Vec2> &query_uv, const std::vector<Vec2> &train_uv, float radius_x, float radius_y,
                     std::vector<int32_t> &train_index, std::vector<int32_t> *distance = nullptr,
                     const std::vector<uint8_t> *query_valid = nullptr, const std::vector<uint8_t> *train_valid = nullptr);

    // Match under a two-view model, the second pass after the model is known: train[j] is a candidate of
    // query[i] only if the pair (query_uv[i], train_uv[j]) passes the model test of fd_brief_match_model (the
    // Sampson test of a fundamental matrix, the query -> train transfer test of a homography; `threshold` in
    // pixels) and MatchGuided's window (open by default). model: row-major 3 x 3 in pixel coordinates, as
    // fd_ransac / fd_ransac_refit write it; nine zeros (no model) leave the window alone. Outputs and the
    // return value are MatchGuided's; also false for a null model or a threshold that is not finite and > 0.
    bool MatchModel(const std::vector<BriefType> &query, const std::vector<BriefType> &train,
                    const std::vector<Vec2> &query_uv, const std::vector<Vec2> &train_uv, const double model[9],
                    MatchModelKind kind, float threshold, std::vector<int32_t> &train_index,
                    std::vector<int32_t> *distance = nullptr, const std::vector<uint8_t> *query_valid = nullptr,
                    const std::vector<uint8_t> *train_valid = nullptr, float radius_x = kOpenMatchRadius,
                    float radius_y = kOpenMatchRadius);

    // Reference for member variables.
    Options &options() { return options_; }
    const Options &options() const { return options_; }

    void set_device(int device) { context_.set_device(device); }
    int device() const { return context_.device(); }
    const std::string &last_error() const { return context_.last_error(); }

private:
    // model null: Match / MatchGuided
    bool Run(const std::vector<BriefType> &query, const std::vector<BriefType> &train, const std::vector<Vec2> *query_uv,
             const std::vector<Vec2> *train_uv, float radius_x, float radius_y, std::vector<int32_t> &train_index,
             std::vector<int32_t> *distance, const std::vector<uint8_t> *query_valid, const std::vector<uint8_t> *train_valid,
             const double *model = nullptr, MatchModelKind kind = MatchModelKind::kFundamental, float threshold = 0.0f);

private:
    Options options_;
    DeviceContext context_;
};

/* Class NNDescriptorMatcher Declaration. */
// Nearest-neighbour squared-L2 matching of NN float descriptors (SuperPoint 256, DISK 128 channels) over
// fd_nn_match. Descriptors are contiguous rows of `dim` floats: a std::vector of the reference's
// Eigen::Matrix<float, N, 1> descriptors is such an array (data() of its first element, dim = N), so no
// Eigen type appears here. The semantics, the float sequence of the distance included, are fd_nn_match's
// (include/fd_hip.h).
class NNDescriptorMatcher {
public:
    struct Options {
        float kMaxDistance = -1.0f;  // reject a best match with squared distance above this; < 0: no bound
        float kMaxRatio = 0.0f;      // accept only if best < kMaxRatio^2 * second best (squared distances); <= 0: off
        bool kCrossCheck = false;    // accept q -> t only if t's best query is q
    };

public:
    NNDescriptorMatcher() = default;
    virtual ~NNDescriptorMatcher();
    NNDescriptorMatcher(const NNDescriptorMatcher &) = delete;
    NNDescriptorMatcher &operator=(const NNDescriptorMatcher &) = delete;

    // query: n_query rows, train: n_train rows of dim floats (dim a multiple of 4, 4..256).
    // train_index[i]: the train row matched to query row i, or -1. distance (optional): [i] the raw
    // smallest squared distance of query i to a valid train row, accepted or not (-1: none).
    // query_valid / train_valid (optional, one flag per row): flag 0 the all-zero descriptors of keypoints
    // outside the descriptor map to keep them out of the matching.
    // False for empty inputs, a bad dim, flag vectors of the wrong size, or a libfdhip failure (last_error()).
    bool Match(const float *query, int32_t n_query, const float *train, int32_t n_train, int32_t dim,
               std::vector<int32_t> &train_index, std::vector<float> *distance = nullptr,
               const std::vector<uint8_t> *query_valid = nullptr, const std::vector<uint8_t> *train_valid = nullptr);

    // Match within a search window (fd_nn_match_guided), as BriefMatcher::MatchGuided: query_xy / train_xy
    // are n_query / n_train rows of (x, y) floats, row i the keypoint of descriptor row i.
    bool MatchGuided(const float *query, int32_t n_query, const float *query_xy, const float *train, int32_t n_train,
                     const float *train_xy, int32_t dim, float radius_x, float radius_y, std::vector<int32_t> &train_index,
                     std::vector<float> *distance = nullptr, const std::vector<uint8_t> *query_valid = nullptr,
                     const std::vector<uint8_t> *train_valid = nullptr);

    // Match under a two-view model (fd_nn_match_model), as BriefMatcher::MatchModel.
    bool MatchModel(const float *query, int32_t n_query, const float *query_xy, const float *train, int32_t n_train,
                    const float *train_xy, int32_t dim, const double model[9], MatchModelKind kind, float threshold,
                    std::vector<int32_t> &train_index, std::vector<float> *distance = nullptr,
                    const std::vector<uint8_t> *query_valid = nullptr, const std::vector<uint8_t> *train_valid = nullptr,
                    float radius_x = kOpenMatchRadius, float radius_y = kOpenMatchRadius);

    // Reference for member variables.
    Options &options() { return options_; }
    const Options &options() const { return options_; }

    void set_device(int device) { context_.set_device(device); }
    int device() const { return context_.device(); }
    const std::string &last_error() const { return context_.last_error(); }

private:
    // model null: Match / MatchGuided
    bool Run(const float *query, int32_t n_query, const float *query_xy, const float *train, int32_t n_train,
             const float *train_xy, int32_t dim, bool guided, float radius_x, float radius_y,
             std::vector<int32_t> &train_index, std::vector<float> *distance, const std::vector<uint8_t> *query_valid,
             const std::vector<uint8_t> *train_valid, const double *model = nullptr,
             MatchModelKind kind = MatchModelKind::kFundamental, float threshold = 0.0f);

private:
    Options options_;
    DeviceContext context_;
};

}  // namespace feature_detector

#endif  // FEATURE_DETECTOR_DESCRIPTOR_MATCHER_H_
