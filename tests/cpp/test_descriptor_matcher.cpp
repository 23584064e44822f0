// Headless demo of BriefMatcher (an MI355X extension; the reference has no matcher): Harris detection
// (kMinFeatureDistance 15, kMinValidResponse 30, need 200) and BriefDescriptor (kLength 256, kHalfPatchSize
// 8) on two frames, then the first frame's descriptors matched against the second's. Prints JSON lines.
//   usage: fd_demo_match <raw u8 gray file> <rows> <cols> <second raw u8 gray file>
//                        [max_distance] [max_ratio] [cross_check: 0 / 1]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "demo_util.h"
#include "feature_detector/descriptor_brief.h"
#include "feature_detector/descriptor_matcher.h"
#include "feature_detector/feature_point_detector.h"

using namespace feature_detector;

static std::vector<BriefType> Describe(const char *name, const GrayImage &image) {
    FeaturePointHarrisDetector detector;
    detector.options().kMinFeatureDistance = 15;
    detector.options().kMinValidResponse = 30.0f;
    std::vector<Vec2> features;
    const bool ok = detector.DetectGoodFeatures(image, 200, features);
    BriefDescriptor descriptor;
    std::vector<BriefType> descriptors;
    const bool ok_d = descriptor.Compute(image, features, descriptors);
    std::printf("{\"test\": \"%s\", \"ok\": %s, \"features\": [", name, ok && ok_d ? "true" : "false");
    for (size_t i = 0; i < features.size(); ++i)
        std::printf("%s[%.1f, %.1f]", i ? ", " : "", features[i].x(), features[i].y());
    std::printf("]}\n");
    return descriptors;
}

// BriefDescriptor leaves an all-zero descriptor where it cannot describe a keypoint: flag those invalid
static std::vector<uint8_t> AnyBitSet(const std::vector<BriefType> &descriptors) {
    std::vector<uint8_t> valid(descriptors.size(), 0);
    for (size_t i = 0; i < descriptors.size(); ++i)
        for (const bool bit : descriptors[i]) valid[i] |= bit ? 1 : 0;
    return valid;
}

static void PrintMatch(const char *name, bool ok, const std::vector<int32_t> &index, const std::vector<int32_t> &distance) {
    std::printf("{\"test\": \"%s\", \"ok\": %s, \"train_index\": [", name, ok ? "true" : "false");
    for (size_t i = 0; i < index.size(); ++i) std::printf("%s%d", i ? ", " : "", index[i]);
    std::printf("], \"distance\": [");
    for (size_t i = 0; i < distance.size(); ++i) std::printf("%s%d", i ? ", " : "", distance[i]);
    std::printf("]}\n");
}

int main(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s <raw u8 file> <rows> <cols> <second raw u8 file> [max_distance] [max_ratio] [cross_check]\n",
                     argv[0]);
        return 2;
    }
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
    GrayImage image0(ReadFrame(argv[1], rows, cols), rows, cols, true);
    GrayImage image1(ReadFrame(argv[4], rows, cols), rows, cols, true);
    const std::vector<BriefType> query = Describe("frame0", image0);
    const std::vector<BriefType> train = Describe("frame1", image1);

    BriefMatcher matcher;
    if (argc > 5) matcher.options().kMaxDistance = std::atoi(argv[5]);
    if (argc > 6) matcher.options().kMaxRatio = static_cast<float>(std::atof(argv[6]));
    if (argc > 7) matcher.options().kCrossCheck = std::atoi(argv[7]) != 0;
    std::vector<int32_t> index, distance;
    bool ok = matcher.Match(query, train, index, &distance);
    PrintMatch("match", ok, index, distance);
    const std::vector<uint8_t> query_valid = AnyBitSet(query), train_valid = AnyBitSet(train);
    ok = matcher.Match(query, train, index, &distance, &query_valid, &train_valid);
    PrintMatch("match_valid", ok, index, distance);

    // Match's false cases: no query descriptors, descriptors of unequal length
    std::vector<BriefType> shorter = train;
    if (!shorter.empty()) shorter[0].resize(128);
    const bool empty_query = matcher.Match(std::vector<BriefType>{}, train, index);
    const bool mismatched = matcher.Match(query, shorter, index);
    std::printf("{\"test\": \"match_false_cases\", \"empty_query\": %s, \"mismatched_length\": %s}\n",
                empty_query ? "true" : "false", mismatched ? "true" : "false");
    return 0;
}
