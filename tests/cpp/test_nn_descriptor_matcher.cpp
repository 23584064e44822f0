// Headless driver of NNDescriptorMatcher (include/feature_detector/descriptor_matcher.h) for
// tests/test_cpp_nn_match.py.
//   fd_demo_nn_match <fixture> [max_distance max_ratio cross_check]
// fixture: int32 n_query, n_train, dim; float query[n_query][dim]; float train[n_train][dim];
//          uint8 query_valid[n_query]; uint8 train_valid[n_train]
// Prints one JSON line per run: without and with the valid flags, then the false cases. Distances are
// printed as the bit patterns of the floats.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "demo_util.h"
#include "feature_detector/descriptor_matcher.h"

using feature_detector::NNDescriptorMatcher;

namespace {

void PrintRun(const char *name, bool ok, const std::vector<int32_t> &index, const std::vector<float> &distance) {
    std::printf("{\"test\": \"%s\", \"ok\": %s, \"train_index\": [", name, ok ? "true" : "false");
    for (size_t i = 0; i < index.size(); ++i) std::printf("%s%d", i ? ", " : "", index[i]);
    std::printf("], \"distance_bits\": [");
    for (size_t i = 0; i < distance.size(); ++i) std::printf("%s%u", i ? ", " : "", Bits(distance[i]));
    std::printf("]}\n");
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2 && argc != 5) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[3];
    if (std::fread(head, sizeof(int32_t), 3, f) != 3) return 2;
    const int32_t nq = head[0], nt = head[1], dim = head[2];
    std::vector<float> query(static_cast<size_t>(nq) * dim), train(static_cast<size_t>(nt) * dim);
    std::vector<uint8_t> qv(nq), tv(nt);
    if (std::fread(query.data(), sizeof(float), query.size(), f) != query.size() ||
        std::fread(train.data(), sizeof(float), train.size(), f) != train.size() ||
        std::fread(qv.data(), 1, qv.size(), f) != qv.size() || std::fread(tv.data(), 1, tv.size(), f) != tv.size())
        return 2;
    std::fclose(f);

    NNDescriptorMatcher matcher;
    if (argc == 5) {
        matcher.options().kMaxDistance = static_cast<float>(std::atof(argv[2]));
        matcher.options().kMaxRatio = static_cast<float>(std::atof(argv[3]));
        matcher.options().kCrossCheck = std::atoi(argv[4]) != 0;
    }
    std::vector<int32_t> index;
    std::vector<float> distance;
    bool ok = matcher.Match(query.data(), nq, train.data(), nt, dim, index, &distance);
    PrintRun("match", ok, index, distance);
    ok = matcher.Match(query.data(), nq, train.data(), nt, dim, index, &distance, &qv, &tv);
    PrintRun("match_valid", ok, index, distance);

    const bool empty_query = matcher.Match(query.data(), 0, train.data(), nt, dim, index);
    const bool bad_dim = matcher.Match(query.data(), nq, train.data(), nt, 6, index);
    std::vector<uint8_t> short_flags(1, 1);
    const bool bad_flags = nq > 1 && matcher.Match(query.data(), nq, train.data(), nt, dim, index, nullptr, &short_flags);
    std::printf("{\"test\": \"match_false_cases\", \"empty_query\": %s, \"bad_dim\": %s, \"bad_flags\": %s}\n",
                empty_query ? "true" : "false", bad_dim ? "true" : "false", bad_flags ? "true" : "false");
    return 0;
}
