// Host runtime of libfdhip.so: the alignment of two 3-D point sets (fd_align_ransac, fd_align_refit) and its
// application (fd_align_apply) over the kernels of fd_align.hip. The two estimator calls keep their checks and hand on
// to the drivers they share with fd_rt_ransac.cpp (fd_rt_estimate.h).
#include <cmath>

#include "fd_rt_estimate.h"

using namespace fdrt;

namespace {

constexpr size_t kModel = 13, kCorr = 6;  // doubles per model (R row-major, t, s) and per correspondence (X, Y)

// What fd_align_ransac and fd_align_refit ask of the arguments they share, and the fields both fill alike.
int align_args(fd_ctx *c, fdk::AlignArgs &a, int batch, const fd_align_opts *o, int32_t q_stride, int32_t t_stride,
               const int32_t *match_idx) {
    const int rc = check_slots(c, batch, q_stride, t_stride, match_idx);
    if (rc) return rc;
    if (o->kind != FD_ALIGN_SIMILARITY && o->kind != FD_ALIGN_RIGID)
        return fail(c, FD_ERR_INVALID, "kind must be FD_ALIGN_SIMILARITY or FD_ALIGN_RIGID");
    if (!std::isfinite(o->threshold) || !(o->threshold > 0.0f)) return fail(c, FD_ERR_INVALID, "threshold must be finite and > 0");
    slot_fields(a, batch, q_stride, t_stride);
    a.kind = o->kind;
    const double t = static_cast<double>(o->threshold);
    a.tt = t * t;
    return FD_OK;
}

// The input arrays of both calls, staged or handed on.
int align_inputs(fd_ctx *c, HostIo &io, fdk::AlignArgs &a, const float *q_xyz, const uint8_t *q_valid, const int32_t *q_counts,
                 const float *t_xyz, const uint8_t *t_valid, const int32_t *match_idx, const uint8_t *pair_valid) {
    const size_t qs = static_cast<size_t>(a.batch) * a.q_stride, ts = static_cast<size_t>(a.batch) * a.t_stride;
    FD_HIP_TRY(c, io.in(q_xyz, 3 * qs, a.q_xyz));
    FD_HIP_TRY(c, io.in(q_valid, qs, a.q_valid));
    FD_HIP_TRY(c, io.in(q_counts, a.batch, a.q_counts));
    FD_HIP_TRY(c, io.in(t_xyz, 3 * ts, a.t_xyz));
    FD_HIP_TRY(c, io.in(t_valid, ts, a.t_valid));
    FD_HIP_TRY(c, io.in(match_idx, qs, a.match_idx));
    FD_HIP_TRY(c, io.in(pair_valid, qs, a.pair_valid));
    return FD_OK;
}

}  // namespace

extern "C" {

int fd_align_ransac(fd_ctx *c, int batch, const fd_align_opts *opts, const float *q_xyz, const uint8_t *q_valid,
                    const int32_t *q_counts, int32_t q_stride, const float *t_xyz, const uint8_t *t_valid, int32_t t_stride,
                    const int32_t *match_idx, const uint8_t *pair_valid, double *out_model, uint8_t *out_inlier,
                    int32_t *out_counts, int32_t *out_best, int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!opts || !q_xyz || !t_xyz || !out_model) return fail(c, FD_ERR_INVALID, "bad arguments");
    fdk::AlignArgs a{};
    const int rc = align_args(c, a, batch, opts, q_stride, t_stride, match_idx);
    if (rc) return rc;
    if (opts->hypotheses < 1 || opts->hypotheses > FD_RANSAC_MAX_HYPOTHESES)
        return fail(c, FD_ERR_INVALID, "hypotheses must be in [1, 4096]");
    a.hypotheses = opts->hypotheses;
    a.seed = opts->seed;
    const auto stage = [&](HostIo &io, fdk::AlignArgs &r) {
        return align_inputs(c, io, r, q_xyz, q_valid, q_counts, t_xyz, t_valid, match_idx, pair_valid);
    };
    return ransac_call(c, a, kModel, kCorr, stage, fdk::launch_align_ransac,
                       {q_counts, nullptr, nullptr, out_model, out_inlier, out_counts, out_best, io_on_device});
}

int fd_align_refit(fd_ctx *c, int batch, const fd_align_opts *opts, const float *q_xyz, const uint8_t *q_valid,
                   const int32_t *q_counts, int32_t q_stride, const float *t_xyz, const uint8_t *t_valid, int32_t t_stride,
                   const int32_t *match_idx, const uint8_t *pair_valid, const double *in_model, const uint8_t *in_inlier,
                   double *out_model, uint8_t *out_inlier, int32_t *out_counts, int32_t *out_rounds, int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!opts || !q_xyz || !t_xyz || !in_model || !in_inlier || !out_model) return fail(c, FD_ERR_INVALID, "bad arguments");
    fdk::AlignRefitArgs g{};
    const int rc = align_args(c, g.r, batch, opts, q_stride, t_stride, match_idx);
    if (rc) return rc;
    if (opts->rounds < 1 || opts->rounds > FD_ALIGN_MAX_ROUNDS) return fail(c, FD_ERR_INVALID, "rounds must be in [1, 8]");
    g.rounds = opts->rounds;
    const auto stage = [&](HostIo &io, fdk::AlignArgs &r) {
        return align_inputs(c, io, r, q_xyz, q_valid, q_counts, t_xyz, t_valid, match_idx, pair_valid);
    };
    // 9 inputs and 4 outputs: the whole staging pool
    return refit_call(c, g, kModel, kCorr, stage, fdk::launch_align_refit,
                      {q_counts, in_model, in_inlier, out_model, out_inlier, out_counts, out_rounds, io_on_device});
}

int fd_align_apply(fd_ctx *c, int batch, const double *model, const float *xyz_in, const uint8_t *valid, const int32_t *counts,
                   int32_t stride, float *xyz_out, int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!model || !xyz_in || !xyz_out) return fail(c, FD_ERR_INVALID, "bad arguments");
    if (batch < 1) return fail(c, FD_ERR_INVALID, "batch must be >= 1");
    if (stride < 0) return fail(c, FD_ERR_INVALID, "stride must be >= 0");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    const int rc = refuse_sync_under_capture(c, io_on_device);
    if (rc) return rc;
    if (stride == 0) return FD_OK;  // no slots: nothing is written
    const size_t slots = static_cast<size_t>(batch) * stride;
    fdk::AlignApplyArgs a{};
    a.batch = batch;
    a.stride = stride;
    HostIo io(c, io_on_device);
    FD_HIP_TRY(c, io.in(model, kModel * batch, a.model));
    FD_HIP_TRY(c, io.in(xyz_in, 3 * slots, a.xyz_in));
    FD_HIP_TRY(c, io.in(valid, slots, a.valid));
    FD_HIP_TRY(c, io.in(counts, batch, a.counts));
    // preloaded: the slots below counts[b] that are not valid keep the caller's bytes through the copy back
    FD_HIP_TRY(c, io.out_slots(xyz_out, slots, 3, a.xyz_out, true));
    FD_HIP_TRY(c, fdk::launch_align_apply(a, c->stream));
    return io.finish(counts, batch, stride);
}

}  // extern "C"
