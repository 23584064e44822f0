// Headless demo of OpticalFlowLK (an MI355X extension; the reference has no tracker): Shi-Tomasi detection
// (kMinFeatureDistance 15, kMinValidResponse 40, need 60) on the first frame, its features tracked into
// the second frame. Prints JSON lines; positions and errors as the hexadecimal bit patterns of their floats.
//   usage: fd_demo_flow <raw u8 gray file> <rows> <cols> <second raw u8 gray file>
//                       [levels] [half_window] [max_forward_backward]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "demo_util.h"
#include "feature_detector/feature_point_detector.h"
#include "feature_detector/optical_flow_lk.h"

using namespace feature_detector;

int main(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s <raw u8 file> <rows> <cols> <second raw u8 file> [levels] [half_window] [max_fb]\n", argv[0]);
        return 2;
    }
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    GrayImage image0(ReadFrame(argv[1], rows, cols), rows, cols, true);
    GrayImage image1(ReadFrame(argv[4], rows, cols), rows, cols, true);

    FeaturePointShiTomasDetector detector;
    detector.options().kMinFeatureDistance = 15;
    detector.options().kMinValidResponse = 40.0f;
    std::vector<Vec2> features;
    const bool ok_d = detector.DetectGoodFeatures(image0, 60, features);
    std::printf("{\"test\": \"detect\", \"ok\": %s, \"features\": [", ok_d ? "true" : "false");
    for (size_t i = 0; i < features.size(); ++i) std::printf("%s[%.1f, %.1f]", i ? ", " : "", features[i].x(), features[i].y());
    std::printf("]}\n");

    OpticalFlowLK flow;
    flow.options().kMinEigen = 1e-4f;
    if (argc > 5) flow.options().kLevels = std::atoi(argv[5]);
    if (argc > 6) flow.options().kHalfWindow = std::atoi(argv[6]);
    if (argc > 7) flow.options().kMaxForwardBackward = static_cast<float>(std::atof(argv[7]));
    std::vector<Vec2> tracked;
    std::vector<uint8_t> status;
    std::vector<float> error;
    const bool ok = flow.Track(image0, image1, features, tracked, status, &error);
    std::printf("{\"test\": \"track\", \"ok\": %s, \"status\": [", ok ? "true" : "false");
    for (size_t i = 0; i < status.size(); ++i) std::printf("%s%d", i ? ", " : "", status[i]);
    std::printf("], \"xy_bits\": [");
    for (size_t i = 0; i < tracked.size(); ++i) std::printf("%s[%u, %u]", i ? ", " : "", Bits(tracked[i].x()), Bits(tracked[i].y()));
    std::printf("], \"err_bits\": [");
    for (size_t i = 0; i < error.size(); ++i) std::printf("%s%u", i ? ", " : "", Bits(error[i]));
    std::printf("]}\n");

    // Track's false cases: no features, images of different sizes
    GrayImage half(image1.data(), rows / 2, cols, false);
    const bool empty = flow.Track(image0, image1, std::vector<Vec2>{}, tracked, status);
    const bool mismatched = flow.Track(image0, half, features, tracked, status);
    std::printf("{\"test\": \"track_false_cases\", \"empty_features\": %s, \"mismatched_size\": %s}\n", empty ? "true" : "false",
                mismatched ? "true" : "false");
    return 0;
}
