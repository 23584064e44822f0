// OpticalFlowLK: pyramidal Lucas-Kanade tracking of feature points from one frame into the next over the
// MI355X kernels of libfdhip.so (fd_pyr_build, fd_flow_lk).
//
// MI355X extension: the reference has no tracker, although DetectGoodFeatures(image, need, features) is
// shaped for one (it masks around the features it is given and only tops up). The semantics, a definite
// arithmetic sequence, are those of fd_flow_lk (include/fd_hip.h).
#ifndef FEATURE_DETECTOR_OPTICAL_FLOW_LK_H_
#define FEATURE_DETECTOR_OPTICAL_FLOW_LK_H_

#include <cstdint>
#include <string>
#include <vector>

#include "device_context.h"
#include "fd_types.h"

namespace feature_detector {

/* Class OpticalFlowLK Declaration. */
class OpticalFlowLK {
public:
    // The defaults are the usual conventions of pyramidal LK front ends, not tuned values.
    struct Options {
        int32_t kLevels = 3;           // pyramid levels, 1..6
        int32_t kHalfWindow = 7;       // the window is (2 * kHalfWindow + 1)^2 pixels, 1..10
        int32_t kMaxIterations = 30;   // per level, 1..100
        float kEpsilon = 0.01f;        // a level stops after a step of at most this length
        float kMinEigen = 1e-3f;       // smallest accepted minimum eigenvalue of the mean gradient matrix
        float kMaxForwardBackward = -1.0f;  // forward-backward check: largest round trip in pixels; < 0: off
        float kMaxError = -1.0f;       // largest mean absolute residual of a track; < 0: off
    };

    // status values (fd_flow_status): kTracked is the only success
    enum Status : uint8_t { kInvalid = 0, kTracked = 1, kOutside = 2, kFlat = 3, kStep = 4, kForwardBackward = 5, kError = 6 };

public:
    OpticalFlowLK() = default;
    virtual ~OpticalFlowLK();
    OpticalFlowLK(const OpticalFlowLK &) = delete;
    OpticalFlowLK &operator=(const OpticalFlowLK &) = delete;

    // next_uv[i]: where prev_uv[i] of `prev` lies in `next`; status[i]: kTracked or the reason it is lost
    // (next_uv[i] is then unspecified). error (optional): [i] the mean absolute residual of the window in
    // intensity units. guess_uv (optional, one per feature): the expected positions in `next`, a motion
    // model's prediction; without it the search starts at prev_uv.
    // False for no features, an empty image, images of different sizes, a guess_uv of the wrong size,
    // options out of range, or a libfdhip failure (last_error()).
    bool Track(const GrayImage &prev, const GrayImage &next, const std::vector<Vec2> &prev_uv, std::vector<Vec2> &next_uv,
               std::vector<uint8_t> &status, std::vector<float> *error = nullptr,
               const std::vector<Vec2> *guess_uv = nullptr);

    // Reference for member variables.
    Options &options() { return options_; }
    const Options &options() const { return options_; }

    void set_device(int device) { context_.set_device(device); }
    int device() const { return context_.device(); }
    const std::string &last_error() const { return context_.last_error(); }

private:
    Options options_;
    DeviceContext context_;
    std::vector<uint8_t> pyramids_;  // both packed pyramids, built on the GPU into host memory, then staged in one upload
};

}  // namespace feature_detector

#endif  // FEATURE_DETECTOR_OPTICAL_FLOW_LK_H_
