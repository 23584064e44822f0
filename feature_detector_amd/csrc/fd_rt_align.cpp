// Host runtime of libfdhip.so: the alignment of two 3-D point sets (fd_align_ransac, fd_align_refit) and its
// application (fd_align_apply) over the kernels of fd_align.hip. The slot checks, the workspace of the compaction
// kernel, the staging of host arrays and the outputs of a call without slots are the ones fd_rt_ransac.cpp uses
// (fd_ctx.h).
#include <cmath>

#include "fd_ctx.h"

using namespace fdrt;

namespace {

constexpr size_t kModel = 13;  // R row-major, t, s

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
    int rc = align_args(c, a, batch, opts, q_stride, t_stride, match_idx);
    if (rc) return rc;
    if (opts->hypotheses < 1 || opts->hypotheses > FD_RANSAC_MAX_HYPOTHESES)
        return fail(c, FD_ERR_INVALID, "hypotheses must be in [1, 4096]");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    rc = refuse_sync_under_capture(c, io_on_device);
    if (rc) return rc;
    const size_t models = kModel * batch;
    if (q_stride == 0) {  // no slots: no frame has a model
        rc = set_output(c, out_model, 0, sizeof(double) * models, io_on_device);
        if (!rc) rc = zero_counts(c, out_counts, batch, io_on_device);
        if (!rc) rc = set_output(c, out_best, 0xFF, sizeof(int32_t) * batch, io_on_device);
        return rc;
    }
    const size_t qs = static_cast<size_t>(batch) * q_stride;
    a.hypotheses = opts->hypotheses;
    a.seed = opts->seed;
    rc = list_workspace(c, a, 6);
    if (rc) return rc;
    FD_HIP_TRY(c, ensure_as(c, c->g_models, static_cast<size_t>(batch) * opts->hypotheses * kModel, a.models));
    HostIo io(c, io_on_device);
    rc = align_inputs(c, io, a, q_xyz, q_valid, q_counts, t_xyz, t_valid, match_idx, pair_valid);
    if (rc) return rc;
    FD_HIP_TRY(c, io.out(out_model, models, a.out_model));
    FD_HIP_TRY(c, io.out_slots(out_inlier, qs, 1, a.out_inlier));
    FD_HIP_TRY(c, io.out(out_counts, batch, a.out_counts));
    FD_HIP_TRY(c, io.out(out_best, batch, a.out_best));
    FD_HIP_TRY(c, fdk::launch_align_ransac(a, c->stream));
    return io.finish(q_counts, batch, q_stride);
}

int fd_align_refit(fd_ctx *c, int batch, const fd_align_opts *opts, const float *q_xyz, const uint8_t *q_valid,
                   const int32_t *q_counts, int32_t q_stride, const float *t_xyz, const uint8_t *t_valid, int32_t t_stride,
                   const int32_t *match_idx, const uint8_t *pair_valid, const double *in_model, const uint8_t *in_inlier,
                   double *out_model, uint8_t *out_inlier, int32_t *out_counts, int32_t *out_rounds, int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!opts || !q_xyz || !t_xyz || !in_model || !in_inlier || !out_model) return fail(c, FD_ERR_INVALID, "bad arguments");
    fdk::AlignRefitArgs g{};
    int rc = align_args(c, g.r, batch, opts, q_stride, t_stride, match_idx);
    if (rc) return rc;
    if (opts->rounds < 1 || opts->rounds > FD_ALIGN_MAX_ROUNDS) return fail(c, FD_ERR_INVALID, "rounds must be in [1, 8]");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    rc = refuse_sync_under_capture(c, io_on_device);
    if (rc) return rc;
    const size_t models = kModel * batch;
    if (q_stride == 0) {  // no slots: no round is accepted
        rc = copy_output(c, out_model, in_model, sizeof(double) * models, io_on_device);
        if (!rc) rc = zero_counts(c, out_counts, batch, io_on_device);
        if (!rc) rc = zero_counts(c, out_rounds, batch, io_on_device);
        return rc;
    }
    const size_t qs = static_cast<size_t>(batch) * q_stride;
    g.rounds = opts->rounds;
    rc = list_workspace(c, g.r, 6);
    if (rc) return rc;
    FD_HIP_TRY(c, ensure_as(c, c->g_member, 2 * qs, g.member));
    HostIo io(c, io_on_device);  // 9 inputs and 4 outputs: the whole staging pool
    rc = align_inputs(c, io, g.r, q_xyz, q_valid, q_counts, t_xyz, t_valid, match_idx, pair_valid);
    if (rc) return rc;
    FD_HIP_TRY(c, io.in(in_model, models, g.in_model));
    FD_HIP_TRY(c, io.in(in_inlier, qs, g.in_inlier));
    FD_HIP_TRY(c, io.out(out_model, models, g.r.out_model));
    FD_HIP_TRY(c, io.out_slots(out_inlier, qs, 1, g.r.out_inlier));
    FD_HIP_TRY(c, io.out(out_counts, batch, g.r.out_counts));
    FD_HIP_TRY(c, io.out(out_rounds, batch, g.out_rounds));
    FD_HIP_TRY(c, fdk::launch_align_refit(g, c->stream));
    return io.finish(q_counts, batch, q_stride);
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
