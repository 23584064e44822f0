// Headless driver of BriefMatcher::MatchModel and NNDescriptorMatcher::MatchModel
// (include/feature_detector/descriptor_matcher.h) for tests/test_cpp_match_model.py.
//   fd_demo_match_model <fixture> <kind> <threshold> <radius> <max_ratio> <cross_check>
// fixture: int32 n_query, n_train, dim, length; double model[9]; float query[n_query][dim]; float train[n_train][dim];
//          uint32 query_bits[n_query][8]; uint32 train_bits[n_train][8]; float query_xy[n_query][2];
//          float train_xy[n_train][2]; uint8 query_valid[n_query]; uint8 train_valid[n_train]
// radius < 0: the default (open) window. Prints one JSON line per run: each class without and with the valid
// flags, then the false cases. Float distances are printed as their bit patterns.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "demo_util.h"
#include "feature_detector/descriptor_matcher.h"

using feature_detector::BriefMatcher;
using feature_detector::BriefType;
using feature_detector::MatchModelKind;
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

const char *B(bool v) { return v ? "true" : "false"; }

}  // namespace

int main(int argc, char **argv) {
    if (argc != 7) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[4];
    if (std::fread(head, sizeof(int32_t), 4, f) != 4) return 2;
    const int32_t nq = head[0], nt = head[1], dim = head[2], length = head[3];
    std::vector<double> model(9);
    std::vector<float> query(static_cast<size_t>(nq) * dim), train(static_cast<size_t>(nt) * dim);
    std::vector<uint32_t> qbits(static_cast<size_t>(nq) * 8), tbits(static_cast<size_t>(nt) * 8);
    std::vector<float> qxy(static_cast<size_t>(nq) * 2), txy(static_cast<size_t>(nt) * 2);
    std::vector<uint8_t> qv(nq), tv(nt);
    if (!Read(f, model) || !Read(f, query) || !Read(f, train) || !Read(f, qbits) || !Read(f, tbits) || !Read(f, qxy) ||
        !Read(f, txy) || !Read(f, qv) || !Read(f, tv))
        return 2;
    std::fclose(f);
    const MatchModelKind kind = std::atoi(argv[2]) ? MatchModelKind::kHomography : MatchModelKind::kFundamental;
    const float thr = static_cast<float>(std::atof(argv[3])), radius = static_cast<float>(std::atof(argv[4]));
    const float ratio = static_cast<float>(std::atof(argv[5]));
    const bool cross = std::atoi(argv[6]) != 0;
    const double *M = model.data();

    BriefMatcher brief;
    brief.options().kMaxRatio = ratio;
    brief.options().kCrossCheck = cross;
    const std::vector<BriefType> q = Unpack(qbits, nq, length), t = Unpack(tbits, nt, length);
    const std::vector<Vec2> quv = Points(qxy), tuv = Points(txy);
    std::vector<int32_t> index, idist;
    bool ok = radius < 0.0f ? brief.MatchModel(q, t, quv, tuv, M, kind, thr, index, &idist)
                            : brief.MatchModel(q, t, quv, tuv, M, kind, thr, index, &idist, nullptr, nullptr, radius, radius);
    PrintRun("brief", ok, index, idist);
    ok = radius < 0.0f ? brief.MatchModel(q, t, quv, tuv, M, kind, thr, index, &idist, &qv, &tv)
                       : brief.MatchModel(q, t, quv, tuv, M, kind, thr, index, &idist, &qv, &tv, radius, radius);
    PrintRun("brief_valid", ok, index, idist);

    NNDescriptorMatcher nn;
    nn.options().kMaxRatio = ratio;
    nn.options().kCrossCheck = cross;
    std::vector<float> fdist;
    const float *Q = query.data(), *T = train.data(), *QP = qxy.data(), *TP = txy.data();
    ok = radius < 0.0f ? nn.MatchModel(Q, nq, QP, T, nt, TP, dim, M, kind, thr, index, &fdist)
                       : nn.MatchModel(Q, nq, QP, T, nt, TP, dim, M, kind, thr, index, &fdist, nullptr, nullptr, radius, radius);
    PrintRun("nn", ok, index, fdist);
    ok = radius < 0.0f ? nn.MatchModel(Q, nq, QP, T, nt, TP, dim, M, kind, thr, index, &fdist, &qv, &tv)
                       : nn.MatchModel(Q, nq, QP, T, nt, TP, dim, M, kind, thr, index, &fdist, &qv, &tv, radius, radius);
    PrintRun("nn_valid", ok, index, fdist);

    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const std::vector<Vec2> short_uv(1);
    const bool brief_short_uv = nq > 1 && brief.MatchModel(q, t, short_uv, tuv, M, kind, thr, index);
    const bool brief_null_model = brief.MatchModel(q, t, quv, tuv, nullptr, kind, thr, index);
    const bool brief_zero_threshold = brief.MatchModel(q, t, quv, tuv, M, kind, 0.0f, index);
    const bool brief_nan_threshold = brief.MatchModel(q, t, quv, tuv, M, kind, nan, index);
    const bool brief_negative_radius = brief.MatchModel(q, t, quv, tuv, M, kind, thr, index, nullptr, nullptr, nullptr, -1.0f, 1.0f);
    const bool nn_null_xy = nn.MatchModel(Q, nq, nullptr, T, nt, TP, dim, M, kind, thr, index);
    const bool nn_null_model = nn.MatchModel(Q, nq, QP, T, nt, TP, dim, nullptr, kind, thr, index);
    const bool nn_inf_threshold = nn.MatchModel(Q, nq, QP, T, nt, TP, dim, M, kind, inf, index);
    const bool nn_bad_kind = nn.MatchModel(Q, nq, QP, T, nt, TP, dim, M, static_cast<MatchModelKind>(2), thr, index);
    const bool nn_empty = nn.MatchModel(Q, 0, QP, T, nt, TP, dim, M, kind, thr, index);
    std::printf("{\"test\": \"false_cases\", \"brief_short_uv\": %s, \"brief_null_model\": %s, \"brief_zero_threshold\": %s, "
                "\"brief_nan_threshold\": %s, \"brief_negative_radius\": %s, \"nn_null_xy\": %s, \"nn_null_model\": %s, "
                "\"nn_inf_threshold\": %s, \"nn_bad_kind\": %s, \"nn_empty\": %s}\n",
                B(brief_short_uv), B(brief_null_model), B(brief_zero_threshold), B(brief_nan_threshold), B(brief_negative_radius),
                B(nn_null_xy), B(nn_null_model), B(nn_inf_threshold), B(nn_bad_kind), B(nn_empty));
    return 0;
}
