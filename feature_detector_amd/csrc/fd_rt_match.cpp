// Host runtime of libfdhip.so: the descriptor matchers. fd_brief_match (Hamming, fd_match.hip) and
// fd_nn_match (squared L2, fd_nn_match.hip) and their guided and model-gated entries are one driver, run_match; what a
// matcher brings of its own (option checks, bytes per descriptor slot, its argument fields, the NN norms
// pre-pass) is a traits struct, BriefMatch / NnMatch.
#include <algorithm>
#include <cmath>
#include <utility>

#include "fd_ctx.h"

using namespace fdrt;

namespace {

// One set of a call, query or train: the caller's arrays, then (host-pointer calls) their staged copies.
struct Side {
    const void *desc;       // [batch][stride] descriptor slots
    const uint8_t *valid;   // [batch][stride] or null (= all valid)
    const int32_t *counts;  // [batch] or null (= stride each)
    int32_t stride;
    const float *xy;  // [batch][stride][2], guided calls only
};

struct BriefMatch {
    using Opts = fd_match_opts;
    using Args = fdk::MatchArgs;
    static int check(fd_ctx *c, const Opts &o) {
        if (o.length < 1 || o.length > 256) return fail(c, FD_ERR_INVALID, "length must be in [1, 256]");
        if (!std::isfinite(o.max_ratio)) return fail(c, FD_ERR_INVALID, "max_ratio must be finite");
        return FD_OK;
    }
    static size_t slot_bytes(const Opts &o) { return sizeof(uint32_t) * static_cast<size_t>((o.length + 31) / 32); }
    static int bind(fd_ctx *, Args &a, const Opts &o, const Side &q, const Side &t) {
        a.a_bits = static_cast<const uint32_t *>(q.desc);
        a.a_valid = q.valid;
        a.b_bits = static_cast<const uint32_t *>(t.desc);
        a.b_valid = t.valid;
        a.length = o.length;
        a.max_distance = o.max_distance;
        return FD_OK;
    }
    static void swap_sets(Args &a) {
        std::swap(a.a_bits, a.b_bits);
        std::swap(a.a_valid, a.b_valid);
    }
    static hipError_t launch(const Args &a, hipStream_t s) { return fdk::launch_brief_match(a, s); }
};

struct NnMatch {
    using Opts = fd_nn_match_opts;
    using Args = fdk::NnMatchArgs;
    static int check(fd_ctx *c, const Opts &o) {
        if (o.dim < 4 || o.dim > 256 || (o.dim & 3)) return fail(c, FD_ERR_INVALID, "dim must be a multiple of 4 in [4, 256]");
        if (!std::isfinite(o.max_ratio) || !std::isfinite(o.max_distance))
            return fail(c, FD_ERR_INVALID, "max_ratio and max_distance must be finite");
        return FD_OK;
    }
    static size_t slot_bytes(const Opts &o) { return sizeof(float) * static_cast<size_t>(o.dim); }
    // the norms of both sets first: validity rides on them ([batch][q_stride], then [batch][t_stride])
    static int bind(fd_ctx *c, Args &a, const Opts &o, const Side &q, const Side &t) {
        const size_t qslots = static_cast<size_t>(a.batch) * q.stride, tslots = static_cast<size_t>(a.batch) * t.stride;
        float *norms = nullptr;
        FD_HIP_TRY(c, ensure_as(c, c->m_norm, qslots + tslots, norms));
        a.a_desc = static_cast<const float *>(q.desc);
        a.a_norm = norms;
        a.b_desc = static_cast<const float *>(t.desc);
        a.b_norm = norms + qslots;
        a.dim = o.dim;
        a.max_distance = o.max_distance;
        const fdk::NnNormArgs nn{{a.a_desc, a.b_desc}, {q.valid, t.valid}, {q.counts, t.counts}, {norms, norms + qslots},
                                 {q.stride, t.stride}, a.batch, o.dim, {}};
        FD_HIP_TRY(c, fdk::launch_nn_norms(nn, c->stream));
        return FD_OK;
    }
    static void swap_sets(Args &a) {
        std::swap(a.a_desc, a.b_desc);
        std::swap(a.a_norm, a.b_norm);
    }
    static hipError_t launch(const Args &a, hipStream_t s) { return fdk::launch_nn_match(a, s); }
};

// The cross-check's reverse pass of the forward arguments: the sets change roles (the window is symmetric;
// the model gate is told which set is the query), the reverse table is the only output and nothing is tested.
template <class M>
typename M::Args swapped(typename M::Args a, int32_t *rev) {
    std::swap(a.a_counts, a.b_counts);
    std::swap(a.a_stride, a.b_stride);
    std::swap(a.a_xy, a.b_xy);
    std::swap(a.a_gate, a.b_gate);
    a.a_is_query = !a.a_is_query;
    M::swap_sets(a);
    a.out_idx = rev;
    a.out_dist = nullptr;
    a.out_counts = nullptr;
    a.rev = nullptr;
    a.max_distance = -1;
    a.max_ratio = 0.0f;
    return a;
}

// The guided matchers' window arguments (gate null: the unguided entry, nothing to check).
int check_gate(fd_ctx *c, const fd_match_gate *gate, const float *q_xy, const float *t_xy) {
    if (!gate) return FD_OK;
    if (!q_xy || !t_xy) return fail(c, FD_ERR_INVALID, "q_xy / t_xy is NULL");
    if (!std::isfinite(gate->radius_x) || !std::isfinite(gate->radius_y) || gate->radius_x < 0.0f || gate->radius_y < 0.0f)
        return fail(c, FD_ERR_INVALID, "radius_x and radius_y must be finite and >= 0");
    return FD_OK;
}

// The model-gated matchers' arguments (mg null: another entry, nothing to check); its radii are check_gate's.
int check_model_gate(fd_ctx *c, const fd_match_model_gate *mg, const double *model) {
    if (!mg) return FD_OK;
    if (!model) return fail(c, FD_ERR_INVALID, "model is NULL");
    if (mg->model != FD_RANSAC_FUNDAMENTAL && mg->model != FD_RANSAC_HOMOGRAPHY)
        return fail(c, FD_ERR_INVALID, "gate model must be FD_RANSAC_FUNDAMENTAL or FD_RANSAC_HOMOGRAPHY");
    if (!std::isfinite(mg->threshold) || mg->threshold <= 0.0f) return fail(c, FD_ERR_INVALID, "threshold must be finite and > 0");
    return FD_OK;
}

// One set's arrays as the kernels take them: the caller's device pointers, or their staged copies.
hipError_t stage_side(HostIo &io, Side &s, size_t slot_bytes, size_t slots, int batch) {
    const uint8_t *desc = static_cast<const uint8_t *>(s.desc);
    hipError_t e = io.in(desc, slot_bytes * slots, desc);
    s.desc = desc;
    if (e == hipSuccess) e = io.in(s.valid, slots, s.valid);
    if (e == hipSuccess) e = io.in(s.counts, batch, s.counts);
    if (e == hipSuccess) e = io.in(s.xy, 2 * slots, s.xy);
    return e;
}

// A matcher call. With cross_check the kernel runs twice, first with the roles swapped into the reverse
// table (the best query of every train descriptor), then forward, where it applies the tests, the reverse
// table among them; out_counts is zeroed on the stream before it. gate (with q.xy, t.xy) is the guided
// entries' window, null for the unguided ones. mg (with model, [batch][9]) is the model-gated entries' gate,
// whose radii are the window then: k_match_gate_vectors first writes both sets' gate vectors into workspace.
template <class M>
int run_match(fd_ctx *c, int batch, const typename M::Opts *opts, const fd_match_gate *gate, const fd_match_model_gate *mg,
              const double *model, Side q, Side t, int32_t *out_idx, decltype(M::Args::out_dist) out_dist,
              int32_t *out_counts, int io_on_device) {
    const int32_t *host_counts = q.counts;  // (q and t are staged below)
    if (!opts || !q.desc || !t.desc || !out_idx) return fail(c, FD_ERR_INVALID, "bad arguments");
    fd_match_gate window{};
    if (mg) {
        window = {mg->radius_x, mg->radius_y};
        gate = &window;
    }
    int rc = check_gate(c, gate, q.xy, t.xy);
    if (rc) return rc;
    if ((rc = check_model_gate(c, mg, model))) return rc;
    if (batch < 1 || q.stride < 0 || t.stride < 0) return fail(c, FD_ERR_INVALID, "need batch >= 1 and strides >= 0");
    if ((rc = M::check(c, *opts))) return rc;
    FD_HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = refuse_sync_under_capture(c, io_on_device))) return rc;
    if (q.stride == 0) return zero_counts(c, out_counts, batch, io_on_device);  // no query slots: every frame has 0 matches
    const size_t qslots = static_cast<size_t>(batch) * q.stride, tslots = static_cast<size_t>(batch) * t.stride;
    typename M::Args a{};
    HostIo io(c, io_on_device);
    FD_HIP_TRY(c, stage_side(io, q, M::slot_bytes(*opts), qslots, batch));
    FD_HIP_TRY(c, stage_side(io, t, M::slot_bytes(*opts), tslots, batch));
    if (mg) FD_HIP_TRY(c, io.in(model, static_cast<size_t>(batch) * 9, model));
    FD_HIP_TRY(c, io.out_slots(out_idx, qslots, 1, a.out_idx));
    FD_HIP_TRY(c, io.out_slots(out_dist, qslots, 2, a.out_dist));
    FD_HIP_TRY(c, io.out(out_counts, batch, a.out_counts));
    a.a_counts = q.counts;
    a.b_counts = t.counts;
    a.a_stride = q.stride;
    a.b_stride = t.stride;
    a.batch = batch;
    a.max_ratio = opts->max_ratio;
    a.a_is_query = 1;
    if (gate) {
        a.a_xy = q.xy;
        a.b_xy = t.xy;
        a.radius_x = gate->radius_x;
        a.radius_y = gate->radius_y;
    }
    if (mg) {
        double *vec = nullptr;
        FD_HIP_TRY(c, ensure_as(c, c->m_gate, 4 * (qslots + tslots), vec));
        const double th = static_cast<double>(mg->threshold);
        a.a_gate = vec;
        a.b_gate = vec + 4 * qslots;
        a.gate_tt = th * th;
        a.gate_model = mg->model;
        const fdk::MatchGateArgs ga{{q.xy, t.xy}, {vec, vec + 4 * qslots}, {q.stride, t.stride}, batch, mg->model, model, a.gate_tt};
        FD_HIP_TRY(c, fdk::launch_match_gate_vectors(ga, c->stream));
    }
    if ((rc = M::bind(c, a, *opts, q, t))) return rc;
    if (opts->cross_check && t.stride > 0) {
        int32_t *rev = nullptr;
        FD_HIP_TRY(c, ensure_as(c, c->m_rev, tslots, rev));
        FD_HIP_TRY(c, M::launch(swapped<M>(a, rev), c->stream));
        a.rev = rev;
    }
    if (a.out_counts) FD_HIP_TRY(c, hipMemsetAsync(a.out_counts, 0, sizeof(int32_t) * batch, c->stream));
    FD_HIP_TRY(c, M::launch(a, c->stream));
    return io.finish(host_counts, batch, q.stride);
}

}  // namespace

extern "C" {

int fd_brief_match(fd_ctx *c, int batch, const fd_match_opts *opts, const uint32_t *q_bits, const uint8_t *q_valid,
                   const int32_t *q_counts, int32_t q_stride, const uint32_t *t_bits, const uint8_t *t_valid,
                   const int32_t *t_counts, int32_t t_stride, int32_t *out_idx, int32_t *out_dist, int32_t *out_counts,
                   int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    return run_match<BriefMatch>(c, batch, opts, nullptr, nullptr, nullptr, {q_bits, q_valid, q_counts, q_stride, nullptr},
                                 {t_bits, t_valid, t_counts, t_stride, nullptr}, out_idx, out_dist, out_counts, io_on_device);
}

int fd_brief_match_guided(fd_ctx *c, int batch, const fd_match_opts *opts, const fd_match_gate *gate,
                          const uint32_t *q_bits, const uint8_t *q_valid, const int32_t *q_counts, int32_t q_stride,
                          const float *q_xy, const uint32_t *t_bits, const uint8_t *t_valid, const int32_t *t_counts,
                          int32_t t_stride, const float *t_xy, int32_t *out_idx, int32_t *out_dist, int32_t *out_counts,
                          int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!gate) return fail(c, FD_ERR_INVALID, "gate is NULL");
    return run_match<BriefMatch>(c, batch, opts, gate, nullptr, nullptr, {q_bits, q_valid, q_counts, q_stride, q_xy},
                                 {t_bits, t_valid, t_counts, t_stride, t_xy}, out_idx, out_dist, out_counts, io_on_device);
}

int fd_nn_match(fd_ctx *c, int batch, const fd_nn_match_opts *opts, const float *q_desc, const uint8_t *q_valid,
                const int32_t *q_counts, int32_t q_stride, const float *t_desc, const uint8_t *t_valid,
                const int32_t *t_counts, int32_t t_stride, int32_t *out_idx, float *out_dist, int32_t *out_counts,
                int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    return run_match<NnMatch>(c, batch, opts, nullptr, nullptr, nullptr, {q_desc, q_valid, q_counts, q_stride, nullptr},
                              {t_desc, t_valid, t_counts, t_stride, nullptr}, out_idx, out_dist, out_counts, io_on_device);
}

int fd_nn_match_guided(fd_ctx *c, int batch, const fd_nn_match_opts *opts, const fd_match_gate *gate, const float *q_desc,
                       const uint8_t *q_valid, const int32_t *q_counts, int32_t q_stride, const float *q_xy,
                       const float *t_desc, const uint8_t *t_valid, const int32_t *t_counts, int32_t t_stride,
                       const float *t_xy, int32_t *out_idx, float *out_dist, int32_t *out_counts, int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!gate) return fail(c, FD_ERR_INVALID, "gate is NULL");
    return run_match<NnMatch>(c, batch, opts, gate, nullptr, nullptr, {q_desc, q_valid, q_counts, q_stride, q_xy},
                              {t_desc, t_valid, t_counts, t_stride, t_xy}, out_idx, out_dist, out_counts, io_on_device);
}

int fd_brief_match_model(fd_ctx *c, int batch, const fd_match_opts *opts, const fd_match_model_gate *gate,
                         const double *model, const uint32_t *q_bits, const uint8_t *q_valid, const int32_t *q_counts,
                         int32_t q_stride, const float *q_xy, const uint32_t *t_bits, const uint8_t *t_valid,
                         const int32_t *t_counts, int32_t t_stride, const float *t_xy, int32_t *out_idx, int32_t *out_dist,
                         int32_t *out_counts, int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!gate) return fail(c, FD_ERR_INVALID, "gate is NULL");
    return run_match<BriefMatch>(c, batch, opts, nullptr, gate, model, {q_bits, q_valid, q_counts, q_stride, q_xy},
                                 {t_bits, t_valid, t_counts, t_stride, t_xy}, out_idx, out_dist, out_counts, io_on_device);
}

int fd_nn_match_model(fd_ctx *c, int batch, const fd_nn_match_opts *opts, const fd_match_model_gate *gate,
                      const double *model, const float *q_desc, const uint8_t *q_valid, const int32_t *q_counts,
                      int32_t q_stride, const float *q_xy, const float *t_desc, const uint8_t *t_valid,
                      const int32_t *t_counts, int32_t t_stride, const float *t_xy, int32_t *out_idx, float *out_dist,
                      int32_t *out_counts, int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!gate) return fail(c, FD_ERR_INVALID, "gate is NULL");
    return run_match<NnMatch>(c, batch, opts, nullptr, gate, model, {q_desc, q_valid, q_counts, q_stride, q_xy},
                              {t_desc, t_valid, t_counts, t_stride, t_xy}, out_idx, out_dist, out_counts, io_on_device);
}

}  // extern "C"
