// CornerRefiner: sub-pixel refinement of corner positions over the MI355X kernel of libfdhip.so
// (fd_points_refine), the cornerSubPix step between DetectGoodFeatures and OpticalFlowLK::Track.
//
// MI355X extension: the reference's detectors return integer pixel positions. The semantics, a definite
// arithmetic sequence, are those of fd_points_refine (include/fd_hip.h).
#ifndef FEATURE_DETECTOR_CORNER_REFINER_H_
#define FEATURE_DETECTOR_CORNER_REFINER_H_

#include <cstdint>
#include <string>
#include <vector>

#include "device_context.h"
#include "fd_types.h"

namespace feature_detector {

/* Class CornerRefiner Declaration. */
class CornerRefiner {
public:
    // The defaults are the usual conventions of cornerSubPix callers, not tuned values.
    struct Options {
        int32_t kHalfWindow = 5;       // the window is (2 * kHalfWindow + 1)^2 pixels, 1..10
        int32_t kMaxIterations = 20;   // 1..100
        float kEpsilon = 0.01f;        // stop after a step of at most this length
        float kMinEigen = 1e-3f;       // smallest accepted minimum eigenvalue of the weighted mean gradient matrix
        float kMaxShift = -1.0f;       // largest move per axis in pixels; < 0: kHalfWindow
    };

    // status values (fd_refine_status): kRefined is the only success
    enum Status : uint8_t { kInvalid = 0, kRefined = 1, kOutside = 2, kFlat = 3, kDiverged = 4 };

public:
    CornerRefiner() = default;
    virtual ~CornerRefiner();
    CornerRefiner(const CornerRefiner &) = delete;
    CornerRefiner &operator=(const CornerRefiner &) = delete;

    // Refines uv in place: uv[i] moves onto the corner it sits near where status[i] is kRefined and stays
    // as it is otherwise (status[i]: the reason).
    // False for no features, an empty image, options out of range, or a libfdhip failure (last_error());
    // uv is then unchanged.
    bool Refine(const GrayImage &image, std::vector<Vec2> &uv, std::vector<uint8_t> &status);

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

#endif  // FEATURE_DETECTOR_CORNER_REFINER_H_
