// LineDescriptor over libfdhip.so (fd_lines_describe): an MI355X extension, the reference's line path stops
// at the segments. One call with host pointers: the frame and the lines are staged through the context, the
// kernel runs, and the descriptors, midpoints and flags come back, complete on return.
#include "feature_detector/line_descriptor.h"

#include <limits>

#include "fd_hip.h"
#include "vec2_pack.h"

namespace feature_detector {

LineDescriptor::~LineDescriptor() = default;

bool LineDescriptor::Compute(const GrayImage &image, const std::vector<Vec4> &lines, std::vector<float> &descriptors) {
    if (!image.data() || image.rows() < 3 || image.cols() < 3) return context_.Fail("Compute: the image must be at least 3 x 3");
    if (options_.kBands < 1 || options_.kBands > 32) return context_.Fail("Compute: kBands must be in [1, 32]");
    if (options_.kBandWidth < 1 || options_.kBandWidth > 16) return context_.Fail("Compute: kBandWidth must be in [1, 16]");
    if (lines.size() > static_cast<size_t>(std::numeric_limits<int32_t>::max())) return context_.Fail("Compute: too many lines");
    fd_ctx *ctx = context_.Acquire();
    if (!ctx) return false;
    const size_t n = lines.size();
    if (n == 0) {
        descriptors.clear();
        midpoints_.clear();
        valid_.clear();
        return true;
    }
    std::vector<float> flat(4 * n), desc(n * static_cast<size_t>(dim())), xy(2 * n);
    for (size_t i = 0; i < n; ++i)
        for (int j = 0; j < 4; ++j) flat[4 * i + j] = lines[i][j];
    std::vector<uint8_t> valid(n);
    const fd_line_desc_opts o{options_.kBands, options_.kBandWidth};
    const int rc = fd_lines_describe(ctx, image.data(), 0, 1, image.rows(), image.cols(), &o, flat.data(), 4, nullptr,
                                     static_cast<int32_t>(n), desc.data(), xy.data(), valid.data(), 0);
    if (rc != FD_OK) return context_.FailCall("fd_lines_describe");
    descriptors.swap(desc);
    midpoints_ = Unflatten(xy.data(), n);
    valid_.swap(valid);
    return true;
}

}  // namespace feature_detector
