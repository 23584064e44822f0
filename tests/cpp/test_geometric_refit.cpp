// Headless demo of GeometricVerifier::Refit (an MI355X extension; the reference has no such stage): the
// correspondences of a file verified as tracks (point i with point i), then the model refitted on its inliers.
// Prints JSON lines; the model's doubles as the decimal bit patterns of their 64 bits.
//   usage: fd_demo_refit <raw float32 file of n x 4: qx qy tx ty> <n> <rows> <cols> <model 0|1> <hypotheses> <seed> <rounds>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "demo_util.h"
#include "feature_detector/geometric_verifier.h"

using namespace feature_detector;

static void Print(const char *test, bool ok, const std::vector<uint8_t> &inlier, const std::array<double, 9> &model, int32_t extra) {
    std::printf("{\"test\": \"%s\", \"ok\": %s, \"extra\": %d, \"inlier\": [", test, ok ? "true" : "false", extra);
    for (size_t i = 0; i < inlier.size(); ++i) std::printf("%s%d", i ? ", " : "", inlier[i]);
    std::printf("], \"model_bits\": [");
    for (size_t i = 0; i < 9; ++i) std::printf("%s%llu", i ? ", " : "", Bits(model[i]));
    std::printf("]}\n");
}

int main(int argc, char **argv) {
    if (argc < 9) {
        std::fprintf(stderr, "usage: %s <raw float32 n x 4 file> <n> <rows> <cols> <model> <hypotheses> <seed> <rounds>\n", argv[0]);
        return 2;
    }
    const size_t n = static_cast<size_t>(std::atoi(argv[2]));
    std::vector<float> raw(4 * n);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(raw.data(), sizeof(float), raw.size(), f) != raw.size()) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::fclose(f);
    std::vector<Vec2> query(n), train(n);
    for (size_t i = 0; i < n; ++i) {
        query[i] = Vec2(raw[4 * i], raw[4 * i + 1]);
        train[i] = Vec2(raw[4 * i + 2], raw[4 * i + 3]);
    }

    GeometricVerifier verifier;
    verifier.SetImageSize(std::atoi(argv[3]), std::atoi(argv[4]));
    verifier.options().kModel = static_cast<GeometricVerifier::Model>(std::atoi(argv[5]));
    verifier.options().kHypotheses = std::atoi(argv[6]);
    verifier.options().kSeed = static_cast<uint32_t>(std::strtoul(argv[7], nullptr, 10));
    const int32_t rounds = std::atoi(argv[8]);

    std::vector<uint8_t> inlier;
    std::array<double, 9> model;
    int32_t best = 0, accepted = -1;
    bool ok = verifier.Verify(query, train, inlier, nullptr, nullptr, &model, &best);
    Print("verify", ok, inlier, model, best);
    ok = verifier.Refit(query, train, inlier, model, rounds, nullptr, nullptr, &accepted);
    Print("refit", ok, inlier, model, accepted);

    // Refit's false cases leave the mask and the model as given
    const std::vector<uint8_t> mask = inlier;
    const std::array<double, 9> kept = model;
    std::vector<uint8_t> short_mask(n ? n - 1 : 0);
    const bool wrong_size = verifier.Refit(query, train, short_mask, model);
    const bool bad_rounds = verifier.Refit(query, train, inlier, model, 5);
    const bool empty = verifier.Refit(std::vector<Vec2>{}, train, short_mask, model);
    std::printf("{\"test\": \"refit_false_cases\", \"wrong_size\": %s, \"bad_rounds\": %s, \"empty\": %s, \"untouched\": %s}\n",
                wrong_size ? "true" : "false", bad_rounds ? "true" : "false", empty ? "true" : "false",
                inlier == mask && model == kept ? "true" : "false");
    return 0;
}
