// Headless driver of BriefMatcher::MatchGuided and NNDescriptorMatcher::MatchGuided
// (include/feature_detector/descriptor_matcher.h) for tests/test_cpp_match_guided.py.
//   fd_demo_match_guided <fixture> <radius_x> <radius_y> <max_ratio> <cross_check>
// fixture: int32 n_query, n_train, dim, length; float query[n_query][dim]; float train[n_train][dim];
//          uint32 query_bits[n_query][8]; uint32 train_bits[n_train][8]; float query_xy[n_query][2];
//          float train_xy[n_train][2]; uint8 query_valid[n_query]; uint8 train_valid[n_train]
// Prints one JSON line per run: each class without and with the valid flags, then the false cases. Float
// distances are printed as their bit patterns.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "demo_util.h"
#include "feature_detector/descriptor_matcher.h"

using feature_detector::BriefMatcher;
using feature_detector::BriefType;
using feature_detector::NNDescriptorMatcher;

namespace {

template <typename T>
bool Read(std::FILE *f, std::vector<T> &v) {
    return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

void PrintHead(const char *name, bool ok, const std::vector<int32_t> &index) {
    std::printf("{\"test\": \"%s\", \"ok\": %s, \"train_index\": [", name, ok ? "true" : "false");
    for (size_t i = 0; i < index.size(); ++i) std::printf("%s%d", i ? ", " : "", index[i]);
}

void PrintRun(const char *name, bool ok, const std::vector<int32_t> &index, const std::vector<int32_t> &distance) {
    PrintHead(name, ok, index);
    std::printf("], \"distance\": [");
    for (size_t i = 0; i < distance.size(); ++i) std::printf("%s%d", i ? ", " : "", distance[i]);
    std::printf("]}\n");
}

void PrintRun(const char *name, bool ok, const std::vector<int32_t> &index, const std::vector<float> &distance) {
    PrintHead(name, ok, index);
    std::printf("], \"distance_bits\": [");
    for (size_t i = 0; i < distance.size(); ++i) std::printf("%s%u", i ? ", " : "", Bits(distance[i]));
    std::printf("]}\n");
}

std::vector<BriefType> Unpack(const std::vector<uint32_t> &words, int32_t n, int32_t length) {
    std::vector<BriefType> out(n, BriefType(length, false));
    for (int32_t i = 0; i < n; ++i)
        for (int32_t j = 0; j < length; ++j) out[i][j] = (words[static_cast<size_t>(i) * 8 + (j >> 5)] >> (j & 31)) & 1u;
    return out;
}

std::vector<Vec2> Points(const std::vector<float> &xy) {
    std::vector<Vec2> out(xy.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = Vec2(xy[2 * i], xy[2 * i + 1]);
    return out;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[4];
    if (std::fread(head, sizeof(int32_t), 4, f) != 4) return 2;
    const int32_t nq = head[0], nt = head[1], dim = head[2], length = head[3];
    std::vector<float> query(static_cast<size_t>(nq) * dim), train(static_cast<size_t>(nt) * dim);
    std::vector<uint32_t> qbits(static_cast<size_t>(nq) * 8), tbits(static_cast<size_t>(nt) * 8);
    std::vector<float> qxy(static_cast<size_t>(nq) * 2), txy(static_cast<size_t>(nt) * 2);
    std::vector<uint8_t> qv(nq), tv(nt);
    if (!Read(f, query) || !Read(f, train) || !Read(f, qbits) || !Read(f, tbits) || !Read(f, qxy) || !Read(f, txy) ||
        !Read(f, qv) || !Read(f, tv))
        return 2;
    std::fclose(f);
    const float rx = static_cast<float>(std::atof(argv[2])), ry = static_cast<float>(std::atof(argv[3]));
    const float ratio = static_cast<float>(std::atof(argv[4]));
    const bool cross = std::atoi(argv[5]) != 0;

    BriefMatcher brief;
    brief.options().kMaxRatio = ratio;
    brief.options().kCrossCheck = cross;
    const std::vector<BriefType> q = Unpack(qbits, nq, length), t = Unpack(tbits, nt, length);
    const std::vector<Vec2> quv = Points(qxy), tuv = Points(txy);
    std::vector<int32_t> index, idist;
    bool ok = brief.MatchGuided(q, t, quv, tuv, rx, ry, index, &idist);
    PrintRun("brief", ok, index, idist);
    ok = brief.MatchGuided(q, t, quv, tuv, rx, ry, index, &idist, &qv, &tv);
    PrintRun("brief_valid", ok, index, idist);

    NNDescriptorMatcher nn;
    nn.options().kMaxRatio = ratio;
    nn.options().kCrossCheck = cross;
    std::vector<float> fdist;
    ok = nn.MatchGuided(query.data(), nq, qxy.data(), train.data(), nt, txy.data(), dim, rx, ry, index, &fdist);
    PrintRun("nn", ok, index, fdist);
    ok = nn.MatchGuided(query.data(), nq, qxy.data(), train.data(), nt, txy.data(), dim, rx, ry, index, &fdist, &qv, &tv);
    PrintRun("nn_valid", ok, index, fdist);

    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const std::vector<Vec2> short_uv(1);
    const bool brief_short_uv = nq > 1 && brief.MatchGuided(q, t, short_uv, tuv, rx, ry, index);
    const bool brief_negative = brief.MatchGuided(q, t, quv, tuv, -1.0f, ry, index);
    const bool brief_nan = brief.MatchGuided(q, t, quv, tuv, rx, nan, index);
    const bool nn_null_xy = nn.MatchGuided(query.data(), nq, nullptr, train.data(), nt, txy.data(), dim, rx, ry, index);
    const bool nn_inf = nn.MatchGuided(query.data(), nq, qxy.data(), train.data(), nt, txy.data(), dim, inf, ry, index);
    const bool nn_empty = nn.MatchGuided(query.data(), 0, qxy.data(), train.data(), nt, txy.data(), dim, rx, ry, index);
    std::printf("{\"test\": \"false_cases\", \"brief_short_uv\": %s, \"brief_negative\": %s, \"brief_nan\": %s, "
                "\"nn_null_xy\": %s, \"nn_inf\": %s, \"nn_empty\": %s}\n",
                brief_short_uv ? "true" : "false", brief_negative ? "true" : "false", brief_nan ? "true" : "false",
                nn_null_xy ? "true" : "false", nn_inf ? "true" : "false", nn_empty ? "true" : "false");
    return 0;
}
