// ContrastEqualizer: contrast-limited adaptive histogram equalization (CLAHE) of a gray image over the MI355X
// kernels of libfdhip.so (fd_frames_equalize): the photometric pre-processing ahead of the detectors and the
// tracker.
//
// MI355X extension: the reference has no such stage. The semantics, exact integer arithmetic, are those of
// fd_frames_equalize (include/fd_hip.h).
#ifndef FEATURE_DETECTOR_CONTRAST_EQUALIZER_H_
#define FEATURE_DETECTOR_CONTRAST_EQUALIZER_H_

#include <cstdint>
#include <string>

#include "device_context.h"
#include "fd_types.h"

namespace feature_detector {

/* Class ContrastEqualizer Declaration. */
class ContrastEqualizer {
public:
    struct Options {
        int32_t kTilesX = 8;       // 1..32, no more than the image's columns
        int32_t kTilesY = 8;       // 1..32, no more than the image's rows
        float kClipLimit = 3.0f;   // OpenCV's clipLimit (clip_milli = lroundf(kClipLimit * 1000)); 0: no clipping
    };

public:
    ContrastEqualizer() = default;
    virtual ~ContrastEqualizer();
    ContrastEqualizer(const ContrastEqualizer &) = delete;
    ContrastEqualizer &operator=(const ContrastEqualizer &) = delete;

    // Fills dst (its buffer is the caller's, its shape must be src's; it may share src's buffer: in place) with
    // the equalized src. False for an empty image, a shape mismatch, options out of range, or a libfdhip failure
    // (last_error()); dst is then unchanged.
    bool Equalize(const GrayImage &src, GrayImage &dst);

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

#endif  // FEATURE_DETECTOR_CONTRAST_EQUALIZER_H_
