// ImageSmoother: Gaussian smoothing of a gray image over the MI355X kernel of libfdhip.so (fd_frames_blur): the
// low-pass ahead of the BRIEF descriptor and, with kStep = 2, one level of a Gaussian pyramid.
//
// MI355X extension: the reference has no such stage. The semantics, exact integer arithmetic with reflected
// borders and one rounding, are those of fd_frames_blur, the taps those of fd_blur_taps (include/fd_hip.h).
#ifndef FEATURE_DETECTOR_IMAGE_SMOOTHER_H_
#define FEATURE_DETECTOR_IMAGE_SMOOTHER_H_

#include <cstdint>
#include <string>
#include <vector>

#include "device_context.h"
#include "fd_types.h"

namespace feature_detector {

/* Class ImageSmoother Declaration. */
class ImageSmoother {
public:
    struct Options {
        float kSigma = 2.0f;          // standard deviation of the Gaussian, > 0 (with kRadius = 3: ORB's 7 x 7 kernel)
        int32_t kRadius = 0;          // 1..15: the kernel is (2 kRadius + 1)^2; 0: min(15, max(1, ceil(3 kSigma)))
        int32_t kStep = 1;            // 1: same size; 2: every second row and column
        std::vector<int32_t> kTaps;   // not empty: w[0..r] used as they are instead of kSigma and kRadius
                                      // (each >= 0, w[0] + 2 (w[1] + ... + w[r]) == 256, r <= 15)
    };

public:
    ImageSmoother() = default;
    virtual ~ImageSmoother();
    ImageSmoother(const ImageSmoother &) = delete;
    ImageSmoother &operator=(const ImageSmoother &) = delete;

    // Fills dst (its buffer is the caller's and must not be src's; its shape must be ceil(rows / kStep) x
    // ceil(cols / kStep)) with the smoothed src. False for an empty image, a shape mismatch, a shared buffer,
    // options out of range, or a libfdhip failure (last_error()); dst is then unchanged.
    bool Smooth(const GrayImage &src, GrayImage &dst);

    // Reference for member variables.
    Options &options() { return options_; }
    const Options &options() const { return options_; }
    // The radius and the taps w[0..radius] of the last successful Smooth (empty before it).
    const std::vector<int32_t> &taps() const { return taps_; }

    void set_device(int device) { context_.set_device(device); }
    int device() const { return context_.device(); }
    const std::string &last_error() const { return context_.last_error(); }

private:
    Options options_;
    std::vector<int32_t> taps_;
    DeviceContext context_;
};

}  // namespace feature_detector

#endif  // FEATURE_DETECTOR_IMAGE_SMOOTHER_H_
