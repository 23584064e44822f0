// ImageWarper: a gray image warped by a homography or a camera model over the MI355X kernel of libfdhip.so
// (fd_frames_warp): registration of a frame by GeometricVerifier's homography, lens undistortion and stereo
// rectification ahead of the detectors.
//
// MI355X extension: the reference has no such stage. The semantics, a definite arithmetic sequence, are
// those of fd_frames_warp (include/fd_hip.h).
#ifndef FEATURE_DETECTOR_IMAGE_WARPER_H_
#define FEATURE_DETECTOR_IMAGE_WARPER_H_

#include <cstdint>
#include <string>

#include "device_context.h"
#include "fd_types.h"

namespace feature_detector {

/* Class ImageWarper Declaration. */
class ImageWarper {
public:
    // kHomography: params is double[9], row-major 3 x 3, destination -> source (a homography fitted from the
    // previous frame's features to the next frame's warps the next frame onto the previous one as it is).
    // kCamera: params is double[22]: destination intrinsics fx, fy, cx, cy; a row-major rotation taking a
    // destination ray to a source-camera ray; source intrinsics fx, fy, cx, cy; k1, k2, p1, p2, k3.
    enum Model : int32_t { kHomography = 0, kCamera = 1 };

    struct Options {
        Model kModel = kHomography;
        int32_t kFill = 0;  // 0..255: the value of destination pixels with no source
    };

public:
    ImageWarper() = default;
    virtual ~ImageWarper();
    ImageWarper(const ImageWarper &) = delete;
    ImageWarper &operator=(const ImageWarper &) = delete;

    // Fills dst (its buffer, rows and cols are the caller's: the destination's shape) from src. mask, if not
    // null, has dst.rows() * dst.cols() bytes: 1 where the pixel has a source, 0 where it got kFill.
    // False for an empty image, null params, dst sharing src's buffer, options out of range, or a libfdhip
    // failure (last_error()); dst is then unchanged.
    bool Warp(const GrayImage &src, const double *params, GrayImage &dst, uint8_t *mask = nullptr);

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

#endif  // FEATURE_DETECTOR_IMAGE_WARPER_H_
