// Headless demo of GeometricVerifier (an MI355X extension; the reference has no such stage): the
// correspondences of a file verified as tracks (point i with point i), then as matches (the train points in
// reverse order behind a train index with a -1 and an out-of-range entry, and valid flags that drop every
// seventh point). Prints JSON lines; the model's doubles as the decimal bit patterns of their 64 bits.
//   usage: fd_demo_geometry <raw float32 file of n x 4: qx qy tx ty> <n> <rows> <cols> [model 0|1] [hypotheses] [seed]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "demo_util.h"
#include "feature_detector/geometric_verifier.h"

using namespace feature_detector;

static void Print(const char *test, bool ok, const std::vector<uint8_t> &inlier, const std::array<double, 9> &model, int32_t best) {
    std::printf("{\"test\": \"%s\", \"ok\": %s, \"best\": %d, \"inlier\": [", test, ok ? "true" : "false", best);
    for (size_t i = 0; i < inlier.size(); ++i) std::printf("%s%d", i ? ", " : "", inlier[i]);
    std::printf("], \"model_bits\": [");
    for (size_t i = 0; i < 9; ++i) std::printf("%s%llu", i ? ", " : "", Bits(model[i]));
    std::printf("]}\n");
}

int main(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s <raw float32 n x 4 file> <n> <rows> <cols> [model] [hypotheses] [seed]\n", argv[0]);
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
    if (argc > 5) verifier.options().kModel = static_cast<GeometricVerifier::Model>(std::atoi(argv[5]));
    if (argc > 6) verifier.options().kHypotheses = std::atoi(argv[6]);
    if (argc > 7) verifier.options().kSeed = static_cast<uint32_t>(std::strtoul(argv[7], nullptr, 10));

    std::vector<uint8_t> inlier;
    std::array<double, 9> model;
    int32_t best = 0;
    bool ok = verifier.Verify(query, train, inlier, nullptr, nullptr, &model, &best);
    Print("tracks", ok, inlier, model, best);

    std::vector<Vec2> reversed(train.rbegin(), train.rend());
    std::vector<int32_t> index(n);
    std::vector<uint8_t> valid(n);
    for (size_t i = 0; i < n; ++i) {
        index[i] = static_cast<int32_t>(n - 1 - i);
        valid[i] = static_cast<uint8_t>(i % 7 == 3 ? 2 : 1);
    }
    if (n > 1) {
        index[0] = -1;
        index[1] = static_cast<int32_t>(n);
    }
    ok = verifier.Verify(query, reversed, inlier, &index, &valid, &model, &best);
    Print("matches", ok, inlier, model, best);

    // Verify's false cases: no points, an index of the wrong size, fewer points than a sample needs
    std::vector<int32_t> short_index(n ? n - 1 : 0);
    const bool empty = verifier.Verify(std::vector<Vec2>{}, train, inlier);
    const bool wrong_size = verifier.Verify(query, train, inlier, &short_index);
    const std::vector<Vec2> few(query.begin(), query.begin() + (n < 3 ? n : 3));
    const bool too_few = verifier.Verify(few, train, inlier, nullptr, nullptr, &model, &best);
    std::printf("{\"test\": \"verify_false_cases\", \"empty\": %s, \"wrong_size\": %s, \"too_few\": %s, \"too_few_best\": %d}\n",
                empty ? "true" : "false", wrong_size ? "true" : "false", too_few ? "true" : "false", best);
    return 0;
}
