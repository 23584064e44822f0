// Headless demo of CornerRefiner (an MI355X extension; the reference's detectors stop at integer pixels):
// Shi-Tomasi detection (kMinFeatureDistance 15, kMinValidResponse 40, need 60), its features refined in
// place. Prints JSON lines; refined positions as the hexadecimal bit patterns of their floats.
//   usage: fd_demo_refine <raw u8 gray file> <rows> <cols> [half_window] [max_shift]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "demo_util.h"
#include "feature_detector/corner_refiner.h"
#include "feature_detector/feature_point_detector.h"

using namespace feature_detector;

int main(int argc, char **argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s <raw u8 file> <rows> <cols> [half_window] [max_shift]\n", argv[0]);
        return 2;
    }
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    GrayImage image(ReadFrame(argv[1], rows, cols), rows, cols, true);

    FeaturePointShiTomasDetector detector;
    detector.options().kMinFeatureDistance = 15;
    detector.options().kMinValidResponse = 40.0f;
    std::vector<Vec2> features;
    const bool ok_d = detector.DetectGoodFeatures(image, 60, features);
    std::printf("{\"test\": \"detect\", \"ok\": %s, \"features\": [", ok_d ? "true" : "false");
    for (size_t i = 0; i < features.size(); ++i) std::printf("%s[%.1f, %.1f]", i ? ", " : "", features[i].x(), features[i].y());
    std::printf("]}\n");

    CornerRefiner refiner;
    if (argc > 4) refiner.options().kHalfWindow = std::atoi(argv[4]);
    if (argc > 5) refiner.options().kMaxShift = static_cast<float>(std::atof(argv[5]));
    std::vector<Vec2> refined = features;
    std::vector<uint8_t> status;
    const bool ok = refiner.Refine(image, refined, status);
    std::printf("{\"test\": \"refine\", \"ok\": %s, \"status\": [", ok ? "true" : "false");
    for (size_t i = 0; i < status.size(); ++i) std::printf("%s%d", i ? ", " : "", status[i]);
    std::printf("], \"xy_bits\": [");
    for (size_t i = 0; i < refined.size(); ++i) std::printf("%s[%u, %u]", i ? ", " : "", Bits(refined[i].x()), Bits(refined[i].y()));
    std::printf("]}\n");

    // a feature that needs no detector (the frame's centre): with no GPU the class says so in last_error()
    std::vector<Vec2> centre{Vec2(static_cast<float>(cols / 2), static_cast<float>(rows / 2))};
    const bool ok_c = refiner.Refine(image, centre, status);
    std::printf("{\"test\": \"centre\", \"ok\": %s, \"status\": %d, \"xy_bits\": [%u, %u], ", ok_c ? "true" : "false",
                status.empty() ? -1 : status[0], Bits(centre[0].x()), Bits(centre[0].y()));
    PrintError(ok_c ? std::string() : refiner.last_error());
    std::printf("}\n");

    // Refine's false cases: no features, an option out of range
    std::vector<Vec2> none;
    const bool empty = refiner.Refine(image, none, status);
    refiner.options().kHalfWindow = 11;
    std::vector<Vec2> again = centre;
    const bool bad_option = refiner.Refine(image, again, status);
    std::printf("{\"test\": \"refine_false_cases\", \"empty_features\": %s, \"bad_option\": %s, ", empty ? "true" : "false",
                bad_option ? "true" : "false");
    PrintError(refiner.last_error());
    std::printf("}\n");
    return 0;
}
