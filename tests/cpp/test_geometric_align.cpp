// Headless demo of GeometricVerifier::AlignPoints, ::RefineAlignment and ::TransformPoints (MI355X extensions; the
// reference has no such stage): the source and target points of a file (source i with target i) turned into the
// similarity or rigid transform between them and its inliers, refined, and applied to the inliers.
// Prints JSON lines; doubles as the decimal bit patterns of their 64 bits, floats of their 32.
//   usage: fd_demo_align <raw float32 file of n x 6: X Y Z, then its target> <n> <kind> <hypotheses> <seed> <threshold> <rounds>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "demo_util.h"
#include "feature_detector/geometric_verifier.h"

using namespace feature_detector;

static void Print(const char *test, bool ok, int32_t extra, const std::array<double, 13> &model, const std::vector<uint8_t> &inlier) {
    std::printf("{\"test\": \"%s\", \"ok\": %s, \"extra\": %d, \"model_bits\": [", test, ok ? "true" : "false", extra);
    for (size_t i = 0; i < 13; ++i) std::printf("%s%llu", i ? ", " : "", Bits(model[i]));
    std::printf("], \"inlier\": [");
    for (size_t i = 0; i < inlier.size(); ++i) std::printf("%s%d", i ? ", " : "", inlier[i]);
    std::printf("]}\n");
}

int main(int argc, char **argv) {
    if (argc < 8) {
        std::fprintf(stderr, "usage: %s <points.f32> <n> <kind> <hypotheses> <seed> <threshold> <rounds>\n", argv[0]);
        return 2;
    }
    const size_t n = static_cast<size_t>(std::atoi(argv[2]));
    std::vector<float> raw(6 * n);
    FILE *f = std::fopen(argv[1], "rb");
    const bool read = f && std::fread(raw.data(), sizeof(float), raw.size(), f) == raw.size();
    if (f) std::fclose(f);
    if (!read) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::vector<std::array<float, 3>> source(n), target(n);
    for (size_t i = 0; i < n; ++i) {
        source[i] = {raw[6 * i], raw[6 * i + 1], raw[6 * i + 2]};
        target[i] = {raw[6 * i + 3], raw[6 * i + 4], raw[6 * i + 5]};
    }
    GeometricVerifier verifier;
    GeometricVerifier::AlignOptions &o = verifier.align_options();
    o.kKind = static_cast<GeometricVerifier::AlignKind>(std::atoi(argv[3]));
    o.kHypotheses = std::atoi(argv[4]);
    o.kSeed = static_cast<uint32_t>(std::strtoul(argv[5], nullptr, 10));
    o.kThreshold = static_cast<float>(std::atof(argv[6]));
    const int32_t rounds = std::atoi(argv[7]);

    std::array<double, 13> model;
    std::vector<uint8_t> inlier;
    int32_t best = 7, accepted = -1;
    bool ok = verifier.AlignPoints(source, target, model, inlier, nullptr, nullptr, nullptr, nullptr, &best);
    Print("align", ok, best, model, inlier);
    ok = verifier.RefineAlignment(source, target, model, inlier, rounds, nullptr, nullptr, nullptr, nullptr, &accepted);
    Print("refine", ok, accepted, model, inlier);
    std::vector<std::array<float, 3>> moved = source;
    ok = verifier.TransformPoints(model, moved, &inlier);
    std::printf("{\"test\": \"transform\", \"ok\": %s, \"point_bits\": [", ok ? "true" : "false");
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) std::printf("%s%u", i + k ? ", " : "", Bits(moved[i][k]));
    std::printf("]}\n");

    // two points have no model; a wrong size, a bad kind and rounds out of range are refused
    std::vector<std::array<float, 3>> two(source.begin(), source.begin() + (n < 2 ? n : 2));
    std::array<double, 13> none;
    none.fill(1.0);
    std::vector<uint8_t> few;
    const bool no_model = verifier.AlignPoints(two, target, none, few, nullptr, nullptr, nullptr, nullptr, &best);
    bool cleared = best == -1 && few.size() == two.size();
    for (double v : none) cleared = cleared && v == 0.0;
    for (uint8_t v : few) cleared = cleared && v == 0;
    std::vector<uint8_t> short_mask(n ? n - 1 : 0);
    const bool wrong_size = verifier.AlignPoints(source, target, none, few, &short_mask);
    const bool wrong_target = verifier.AlignPoints(source, target, none, few, nullptr, &short_mask);
    std::array<double, 13> kept = model;
    const bool bad_rounds = verifier.RefineAlignment(source, target, kept, inlier, 9);
    std::vector<std::array<float, 3>> same = source;
    const bool bad_mask = verifier.TransformPoints(model, same, &short_mask);
    o.kKind = static_cast<GeometricVerifier::AlignKind>(2);
    const bool bad_kind = verifier.AlignPoints(source, target, none, few);
    std::printf("{\"test\": \"align_false_cases\", \"no_model\": %s, \"cleared\": %s, \"wrong_size\": %s, \"wrong_target\": %s, "
                "\"bad_kind\": %s, \"bad_rounds\": %s, \"bad_mask\": %s, \"kept\": %s}\n",
                no_model ? "true" : "false", cleared ? "true" : "false", wrong_size ? "true" : "false",
                wrong_target ? "true" : "false", bad_kind ? "true" : "false", bad_rounds ? "true" : "false",
                bad_mask ? "true" : "false", (kept == model && same == source) ? "true" : "false");
    return 0;
}
