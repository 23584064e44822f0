// BriefMatcher over libfdhip.so (fd_brief_match): an MI355X extension, the reference has no matcher.
// One call matches every query descriptor against every train descriptor in one kernel launch (two with
// the cross-check). NNDescriptorMatcher: the same over fd_nn_match for float descriptors (squared L2).
// MatchGuided of both: the same call through the guided entry points, with the keypoint positions.
// MatchModel of both: the same through the model-gated entry points, with the positions and a 3 x 3 model.
#include "feature_detector/descriptor_matcher.h"

#include <cmath>

#include "fd_hip.h"
#include "vec2_pack.h"

namespace feature_detector {

namespace {

// std::vector<bool> descriptors -> [n][words] uint32, bit i = bit i % 32 of word i / 32 (fd_brief_compute's layout)
bool Pack(const std::vector<BriefType> &descriptors, size_t length, std::vector<uint32_t> &words) {
    const size_t nw = (length + 31) / 32;
    words.assign(descriptors.size() * nw, 0u);
    for (size_t i = 0; i < descriptors.size(); ++i) {
        if (descriptors[i].size() != length) return false;
        for (size_t j = 0; j < length; ++j)
            if (descriptors[i][j]) words[i * nw + (j >> 5)] |= 1u << (j & 31);
    }
    return true;
}

bool BadRadius(float r) { return !std::isfinite(r) || r < 0.0f; }
bool BadThreshold(float t) { return !std::isfinite(t) || t <= 0.0f; }

}  // namespace

BriefMatcher::~BriefMatcher() = default;

bool BriefMatcher::Match(const std::vector<BriefType> &query, const std::vector<BriefType> &train,
                         std::vector<int32_t> &train_index, std::vector<int32_t> *distance,
                         const std::vector<uint8_t> *query_valid, const std::vector<uint8_t> *train_valid) {
    return Run(query, train, nullptr, nullptr, 0.0f, 0.0f, train_index, distance, query_valid, train_valid);
}

bool BriefMatcher::MatchGuided(const std::vector<BriefType> &query, const std::vector<BriefType> &train,
                               const std::vector<Vec2> &query_uv, const std::vector<Vec2> &train_uv, float radius_x,
                               float radius_y, std::vector<int32_t> &train_index, std::vector<int32_t> *distance,
                               const std::vector<uint8_t> *query_valid, const std::vector<uint8_t> *train_valid) {
    return Run(query, train, &query_uv, &train_uv, radius_x, radius_y, train_index, distance, query_valid, train_valid);
}

bool BriefMatcher::MatchModel(const std::vector<BriefType> &query, const std::vector<BriefType> &train,
                              const std::vector<Vec2> &query_uv, const std::vector<Vec2> &train_uv, const double model[9],
                              MatchModelKind kind, float threshold, std::vector<int32_t> &train_index,
                              std::vector<int32_t> *distance, const std::vector<uint8_t> *query_valid,
                              const std::vector<uint8_t> *train_valid, float radius_x, float radius_y) {
    if (!model || BadThreshold(threshold)) {
        train_index.assign(query.size(), -1);
        if (distance) distance->assign(query.size(), -1);
        return context_.Fail("MatchModel: a model and a finite threshold > 0 are needed");
    }
    return Run(query, train, &query_uv, &train_uv, radius_x, radius_y, train_index, distance, query_valid, train_valid, model,
               kind, threshold);
}

// query_uv / train_uv null: Match; else MatchGuided, or with a model MatchModel
bool BriefMatcher::Run(const std::vector<BriefType> &query, const std::vector<BriefType> &train,
                       const std::vector<Vec2> *query_uv, const std::vector<Vec2> *train_uv, float radius_x, float radius_y,
                       std::vector<int32_t> &train_index, std::vector<int32_t> *distance,
                       const std::vector<uint8_t> *query_valid, const std::vector<uint8_t> *train_valid, const double *model,
                       MatchModelKind kind, float threshold) {
    train_index.assign(query.size(), -1);
    if (distance) distance->assign(query.size(), -1);
    if (query.empty() || train.empty()) return context_.Fail("Match: empty input");
    const size_t length = query[0].size();
    if (length < 1 || length > 256) return context_.Fail("Match: descriptor length outside 1..256");
    std::vector<uint32_t> q, t;
    if (!Pack(query, length, q) || !Pack(train, length, t)) return context_.Fail("Match: descriptors of unequal length");
    if ((query_valid && query_valid->size() != query.size()) || (train_valid && train_valid->size() != train.size()))
        return context_.Fail("Match: one valid flag per descriptor is needed");
    if (query_uv && (query_uv->size() != query.size() || train_uv->size() != train.size()))
        return context_.Fail("MatchGuided: one position per descriptor is needed");
    if (query_uv && (BadRadius(radius_x) || BadRadius(radius_y))) return context_.Fail("MatchGuided: a radius must be finite and >= 0");
    fd_ctx *ctx = context_.Acquire();
    if (!ctx) return false;
    fd_match_opts o{static_cast<int32_t>(length), options_.kMaxDistance, options_.kMaxRatio, options_.kCrossCheck ? 1 : 0};
    std::vector<int32_t> dist(2 * query.size(), -1);
    const uint8_t *qv = query_valid ? query_valid->data() : nullptr, *tv = train_valid ? train_valid->data() : nullptr;
    const int32_t nq = static_cast<int32_t>(query.size()), nt = static_cast<int32_t>(train.size());
    int rc;
    if (query_uv) {
        const std::vector<float> qxy = Flatten(*query_uv), txy = Flatten(*train_uv);
        const fd_match_gate gate{radius_x, radius_y};
        const fd_match_model_gate mgate{static_cast<int32_t>(kind), threshold, radius_x, radius_y};
        if (model)
            rc = fd_brief_match_model(ctx, 1, &o, &mgate, model, q.data(), qv, nullptr, nq, qxy.data(), t.data(), tv, nullptr,
                                      nt, txy.data(), train_index.data(), dist.data(), nullptr, 0);
        else
            rc = fd_brief_match_guided(ctx, 1, &o, &gate, q.data(), qv, nullptr, nq, qxy.data(), t.data(), tv, nullptr, nt,
                                       txy.data(), train_index.data(), dist.data(), nullptr, 0);
    } else {
        rc = fd_brief_match(ctx, 1, &o, q.data(), qv, nullptr, nq, t.data(), tv, nullptr, nt, train_index.data(),
                            dist.data(), nullptr, 0);
    }
    if (rc != FD_OK) {
        train_index.assign(query.size(), -1);
        return context_.FailCall("fd_brief_match");
    }
    if (distance)
        for (size_t i = 0; i < query.size(); ++i) (*distance)[i] = dist[2 * i];
    return true;
}

NNDescriptorMatcher::~NNDescriptorMatcher() = default;

bool NNDescriptorMatcher::Match(const float *query, int32_t n_query, const float *train, int32_t n_train, int32_t dim,
                                std::vector<int32_t> &train_index, std::vector<float> *distance,
                                const std::vector<uint8_t> *query_valid, const std::vector<uint8_t> *train_valid) {
    return Run(query, n_query, nullptr, train, n_train, nullptr, dim, false, 0.0f, 0.0f, train_index, distance, query_valid,
               train_valid);
}

bool NNDescriptorMatcher::MatchGuided(const float *query, int32_t n_query, const float *query_xy, const float *train,
                                      int32_t n_train, const float *train_xy, int32_t dim, float radius_x, float radius_y,
                                      std::vector<int32_t> &train_index, std::vector<float> *distance,
                                      const std::vector<uint8_t> *query_valid, const std::vector<uint8_t> *train_valid) {
    return Run(query, n_query, query_xy, train, n_train, train_xy, dim, true, radius_x, radius_y, train_index, distance,
               query_valid, train_valid);
}

bool NNDescriptorMatcher::MatchModel(const float *query, int32_t n_query, const float *query_xy, const float *train,
                                     int32_t n_train, const float *train_xy, int32_t dim, const double model[9],
                                     MatchModelKind kind, float threshold, std::vector<int32_t> &train_index,
                                     std::vector<float> *distance, const std::vector<uint8_t> *query_valid,
                                     const std::vector<uint8_t> *train_valid, float radius_x, float radius_y) {
    if (!model || BadThreshold(threshold)) {
        const size_t nq = n_query > 0 ? static_cast<size_t>(n_query) : 0;
        train_index.assign(nq, -1);
        if (distance) distance->assign(nq, -1.0f);
        return context_.Fail("MatchModel: a model and a finite threshold > 0 are needed");
    }
    return Run(query, n_query, query_xy, train, n_train, train_xy, dim, true, radius_x, radius_y, train_index, distance,
               query_valid, train_valid, model, kind, threshold);
}

bool NNDescriptorMatcher::Run(const float *query, int32_t n_query, const float *query_xy, const float *train,
                              int32_t n_train, const float *train_xy, int32_t dim, bool guided, float radius_x,
                              float radius_y, std::vector<int32_t> &train_index, std::vector<float> *distance,
                              const std::vector<uint8_t> *query_valid, const std::vector<uint8_t> *train_valid,
                              const double *model, MatchModelKind kind, float threshold) {
    const size_t nq = n_query > 0 ? static_cast<size_t>(n_query) : 0;
    train_index.assign(nq, -1);
    if (distance) distance->assign(nq, -1.0f);
    if (!query || !train || n_query < 1 || n_train < 1) return context_.Fail("Match: empty input");
    if (dim < 4 || dim > 256 || (dim & 3)) return context_.Fail("Match: dim must be a multiple of 4 in 4..256");
    if ((query_valid && query_valid->size() != nq) || (train_valid && train_valid->size() != static_cast<size_t>(n_train)))
        return context_.Fail("Match: one valid flag per descriptor is needed");
    if (guided && (!query_xy || !train_xy)) return context_.Fail("MatchGuided: positions are needed");
    if (guided && (BadRadius(radius_x) || BadRadius(radius_y))) return context_.Fail("MatchGuided: a radius must be finite and >= 0");
    fd_ctx *ctx = context_.Acquire();
    if (!ctx) return false;
    fd_nn_match_opts o{dim, options_.kMaxDistance, options_.kMaxRatio, options_.kCrossCheck ? 1 : 0};
    std::vector<float> dist(2 * nq, -1.0f);
    const uint8_t *qv = query_valid ? query_valid->data() : nullptr, *tv = train_valid ? train_valid->data() : nullptr;
    int rc;
    if (guided && model) {
        const fd_match_model_gate mgate{static_cast<int32_t>(kind), threshold, radius_x, radius_y};
        rc = fd_nn_match_model(ctx, 1, &o, &mgate, model, query, qv, nullptr, n_query, query_xy, train, tv, nullptr, n_train,
                               train_xy, train_index.data(), dist.data(), nullptr, 0);
    } else if (guided) {
        const fd_match_gate gate{radius_x, radius_y};
        rc = fd_nn_match_guided(ctx, 1, &o, &gate, query, qv, nullptr, n_query, query_xy, train, tv, nullptr, n_train,
                                train_xy, train_index.data(), dist.data(), nullptr, 0);
    } else {
        rc = fd_nn_match(ctx, 1, &o, query, qv, nullptr, n_query, train, tv, nullptr, n_train, train_index.data(),
                         dist.data(), nullptr, 0);
    }
    if (rc != FD_OK) {
        train_index.assign(nq, -1);
        return context_.FailCall("fd_nn_match");
    }
    if (distance)
        for (size_t i = 0; i < nq; ++i) (*distance)[i] = dist[2 * i];
    return true;
}

}  // namespace feature_detector
