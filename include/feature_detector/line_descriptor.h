// LineDescriptor: a band descriptor (LBD style) of the segments FeatureLineDetector finds, over the MI355X
// kernel of libfdhip.so (fd_lines_describe), so that the segments of two frames can be matched with
// DescriptorMatcher's float matcher.
//
// MI355X extension: the reference's line path stops at the segments. The semantics are those of
// fd_lines_describe (include/fd_hip.h).
#ifndef FEATURE_DETECTOR_LINE_DESCRIPTOR_H_
#define FEATURE_DETECTOR_LINE_DESCRIPTOR_H_

#include <cstdint>
#include <string>
#include <vector>

#include "device_context.h"
#include "fd_types.h"

namespace feature_detector {

/* Class LineDescriptor Declaration. */
class LineDescriptor {
public:
    struct Options {
        int32_t kBands = 9;      // 1..32: bands across the line
        int32_t kBandWidth = 7;  // 1..16: rows of one band
    };

public:
    LineDescriptor() = default;
    virtual ~LineDescriptor();
    LineDescriptor(const LineDescriptor &) = delete;
    LineDescriptor &operator=(const LineDescriptor &) = delete;

    // Floats of one descriptor with the current options: 8 * kBands.
    int32_t dim() const { return 8 * options_.kBands; }

    // descriptors = lines.size() x dim() floats, row-major: the unit-norm descriptor of every line
    // (start.x, start.y, end.x, end.y: DetectGoodFeatures' features), all zero for a line that has none
    // (shorter than a pixel, not finite, or on a flat region). midpoints() and valid() are then one entry
    // per line. False for an empty image, one smaller than 3 x 3, options out of range, or a libfdhip
    // failure (last_error()); descriptors is then unchanged. No lines: true, descriptors empty.
    bool Compute(const GrayImage &image, const std::vector<Vec4> &lines, std::vector<float> &descriptors);

    // Of the last successful Compute: every segment's midpoint (DescriptorMatcher's guided positions) and
    // whether it has a descriptor.
    const std::vector<Vec2> &midpoints() const { return midpoints_; }
    const std::vector<uint8_t> &valid() const { return valid_; }

    // Reference for member variables.
    Options &options() { return options_; }
    const Options &options() const { return options_; }

    void set_device(int device) { context_.set_device(device); }
    int device() const { return context_.device(); }
    const std::string &last_error() const { return context_.last_error(); }

private:
    Options options_;
    std::vector<Vec2> midpoints_;
    std::vector<uint8_t> valid_;
    DeviceContext context_;
};

}  // namespace feature_detector

#endif  // FEATURE_DETECTOR_LINE_DESCRIPTOR_H_
