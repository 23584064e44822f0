// Host runtime of libfdhip.so: RANSAC verification of matches and tracks (fd_ransac), the least-squares
// refit of its model (fd_ransac_refit), the pose of a fundamental matrix (fd_pose_recover) and triangulation
// (fd_triangulate) over the kernels of fd_ransac.hip, and the absolute pose from 3-D points (fd_pnp_ransac,
// fd_pnp_refit) over those of fd_pnp.hip. The six calls share the staging of the pair arrays here. The RANSAC and
// refit calls keep their checks and hand on to the drivers they share with fd_rt_align.cpp (fd_rt_estimate.h), with
// their argument block, two widths, their input stager and their launcher.
#include <cmath>

#include "fd_rt_estimate.h"

using namespace fdrt;

namespace {

// doubles per model and per correspondence: F or H and (x, y, u, v); R, t and (Xc, Yc, Zc, bx, by)
constexpr size_t kPairModel = 9, kPairCorr = 4, kPose = 12, kPnpCorr = 5;

// The pair arrays every call has behind its query side's own (q_xy, or p_xyz and p_valid), staged or handed on.
template <class A>
int stage_pairs(fd_ctx *c, HostIo &io, A &a, const float *t_xy, const int32_t *q_counts, const int32_t *match_idx,
                const uint8_t *pair_valid) {
    const size_t qs = static_cast<size_t>(a.batch) * a.q_stride, ts = static_cast<size_t>(a.batch) * a.t_stride;
    FD_HIP_TRY(c, io.in(t_xy, 2 * ts, a.t_xy));
    FD_HIP_TRY(c, io.in(q_counts, a.batch, a.q_counts));
    FD_HIP_TRY(c, io.in(match_idx, qs, a.match_idx));
    FD_HIP_TRY(c, io.in(pair_valid, qs, a.pair_valid));
    return FD_OK;
}

// What fd_ransac and fd_ransac_refit ask of the arguments they share (o: fd_ransac_opts or fd_refit_opts), and the
// fields both fill alike.
template <class O>
int pair_args(fd_ctx *c, fdk::RansacArgs &a, int batch, int32_t q_stride, int32_t t_stride, const int32_t *match_idx,
              const O &o) {
    const int rc = check_slots(c, batch, q_stride, t_stride, match_idx);
    if (rc) return rc;
    if (o.model != FD_RANSAC_FUNDAMENTAL && o.model != FD_RANSAC_HOMOGRAPHY)
        return fail(c, FD_ERR_INVALID, "model must be FD_RANSAC_FUNDAMENTAL or FD_RANSAC_HOMOGRAPHY");
    if (!std::isfinite(o.threshold) || !(o.threshold > 0.0f)) return fail(c, FD_ERR_INVALID, "threshold must be finite and > 0");
    if (!std::isfinite(o.center_x) || !std::isfinite(o.center_y))
        return fail(c, FD_ERR_INVALID, "center_x and center_y must be finite");
    if (!std::isfinite(o.scale) || !(o.scale > 0.0f)) return fail(c, FD_ERR_INVALID, "scale must be finite and > 0");
    slot_fields(a, batch, q_stride, t_stride);
    a.model = o.model;
    a.cx = static_cast<double>(o.center_x);
    a.cy = static_cast<double>(o.center_y);
    a.scale = static_cast<double>(o.scale);
    const double t = static_cast<double>(o.threshold) * a.scale;
    a.tt = t * t;
    return FD_OK;
}

// The pair arrays of the two-view calls (RansacArgs, PoseArgs), staged or handed on.
template <class A>
int pair_inputs(fd_ctx *c, HostIo &io, A &a, const float *q_xy, const int32_t *q_counts, const float *t_xy,
                const int32_t *match_idx, const uint8_t *pair_valid) {
    FD_HIP_TRY(c, io.in(q_xy, 2 * static_cast<size_t>(a.batch) * a.q_stride, a.q_xy));
    return stage_pairs(c, io, a, t_xy, q_counts, match_idx, pair_valid);
}

// What fd_triangulate and fd_pose_recover ask of the arguments they share, and the option fields of the kernels'
// argument block.
int pose_args(fd_ctx *c, fdk::PoseArgs &a, int batch, const fd_pose_opts *o, int32_t q_stride, int32_t t_stride,
              const int32_t *match_idx) {
    int rc = check_slots(c, batch, q_stride, t_stride, match_idx);
    if (rc) return rc;
    const double cam[8] = {o->fx_q, o->fy_q, o->cx_q, o->cy_q, o->fx_t, o->fy_t, o->cx_t, o->cy_t};
    rc = check_camera(c, cam, 8, a.cam);
    if (rc) return rc;
    if (!(o->max_depth > 0.0f)) return fail(c, FD_ERR_INVALID, "max_depth must be > 0");
    if (!(o->min_parallax >= 0.0f && o->min_parallax <= 1.0f)) return fail(c, FD_ERR_INVALID, "min_parallax must be in [0, 1]");
    slot_fields(a, batch, q_stride, t_stride);
    const double m = static_cast<double>(o->min_parallax);
    a.mm = m * m;
    a.D = static_cast<double>(o->max_depth);
    return FD_OK;
}

// What fd_pnp_ransac and fd_pnp_refit ask of the arguments they share, and the fields both fill alike. The
// conditioning is the caller's (fd_pnp_ransac) or none (fd_pnp_refit).
int pnp_args(fd_ctx *c, fdk::PnpArgs &a, int batch, const fd_pnp_opts *o, int32_t q_stride, int32_t t_stride,
             const int32_t *match_idx, bool conditioned) {
    int rc = check_slots(c, batch, q_stride, t_stride, match_idx);
    if (rc) return rc;
    if (!std::isfinite(o->threshold) || !(o->threshold > 0.0f)) return fail(c, FD_ERR_INVALID, "threshold must be finite and > 0");
    const double cam[4] = {o->fx, o->fy, o->cx, o->cy};
    rc = check_camera(c, cam, 4, a.cam);
    if (rc) return rc;
    for (int k = 0; k < 3; ++k) {
        if (conditioned && !std::isfinite(o->center[k])) return fail(c, FD_ERR_INVALID, "center must be finite");
        a.center[k] = conditioned ? o->center[k] : 0.0;
    }
    if (conditioned && (!std::isfinite(o->scale) || !(o->scale > 0.0))) return fail(c, FD_ERR_INVALID, "scale must be finite and > 0");
    a.scale = conditioned ? o->scale : 1.0;
    slot_fields(a, batch, q_stride, t_stride);
    const double t = static_cast<double>(o->threshold);
    a.tt = t * t;
    return FD_OK;
}

// The input arrays of both calls, staged or handed on.
int pnp_inputs(fd_ctx *c, HostIo &io, fdk::PnpArgs &a, const float *p_xyz, const uint8_t *p_valid, const int32_t *q_counts,
               const float *t_xy, const int32_t *match_idx, const uint8_t *pair_valid) {
    const size_t qs = static_cast<size_t>(a.batch) * a.q_stride;
    FD_HIP_TRY(c, io.in(p_xyz, 3 * qs, a.p_xyz));
    FD_HIP_TRY(c, io.in(p_valid, qs, a.p_valid));
    return stage_pairs(c, io, a, t_xy, q_counts, match_idx, pair_valid);
}

}  // namespace

extern "C" {

int fd_pnp_ransac(fd_ctx *c, int batch, const fd_pnp_opts *opts, const float *p_xyz, const uint8_t *p_valid,
                  const int32_t *q_counts, int32_t q_stride, const float *t_xy, int32_t t_stride, const int32_t *match_idx,
                  const uint8_t *pair_valid, double *out_pose, uint8_t *out_inlier, int32_t *out_counts, int32_t *out_best,
                  int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!opts || !p_xyz || !t_xy || !out_pose) return fail(c, FD_ERR_INVALID, "bad arguments");
    fdk::PnpArgs a{};
    const int rc = pnp_args(c, a, batch, opts, q_stride, t_stride, match_idx, true);
    if (rc) return rc;
    if (opts->hypotheses < 1 || opts->hypotheses > FD_RANSAC_MAX_HYPOTHESES)
        return fail(c, FD_ERR_INVALID, "hypotheses must be in [1, 4096]");
    a.hypotheses = opts->hypotheses;
    a.seed = opts->seed;
    const auto stage = [&](HostIo &io, fdk::PnpArgs &r) {
        return pnp_inputs(c, io, r, p_xyz, p_valid, q_counts, t_xy, match_idx, pair_valid);
    };
    return ransac_call(c, a, kPose, kPnpCorr, stage, fdk::launch_pnp_ransac,
                       {q_counts, nullptr, nullptr, out_pose, out_inlier, out_counts, out_best, io_on_device});
}

int fd_pnp_refit(fd_ctx *c, int batch, const fd_pnp_opts *opts, const float *p_xyz, const uint8_t *p_valid,
                 const int32_t *q_counts, int32_t q_stride, const float *t_xy, int32_t t_stride, const int32_t *match_idx,
                 const uint8_t *pair_valid, const double *in_pose, const uint8_t *in_inlier, double *out_pose,
                 uint8_t *out_inlier, int32_t *out_counts, int32_t *out_rounds, int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!opts || !p_xyz || !t_xy || !in_pose || !in_inlier || !out_pose) return fail(c, FD_ERR_INVALID, "bad arguments");
    fdk::PnpRefitArgs g{};
    const int rc = pnp_args(c, g.r, batch, opts, q_stride, t_stride, match_idx, false);
    if (rc) return rc;
    if (opts->rounds < 1 || opts->rounds > FD_PNP_MAX_ROUNDS) return fail(c, FD_ERR_INVALID, "rounds must be in [1, 8]");
    g.rounds = opts->rounds;
    const auto stage = [&](HostIo &io, fdk::PnpArgs &r) {
        return pnp_inputs(c, io, r, p_xyz, p_valid, q_counts, t_xy, match_idx, pair_valid);
    };
    return refit_call(c, g, kPose, kPnpCorr, stage, fdk::launch_pnp_refit,  // 8 inputs and 4 outputs
                      {q_counts, in_pose, in_inlier, out_pose, out_inlier, out_counts, out_rounds, io_on_device});
}

int fd_ransac(fd_ctx *c, int batch, const fd_ransac_opts *opts, const float *q_xy, const int32_t *q_counts,
              int32_t q_stride, const float *t_xy, int32_t t_stride, const int32_t *match_idx, const uint8_t *pair_valid,
              double *out_model, uint8_t *out_inlier, int32_t *out_counts, int32_t *out_best, int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!opts || !q_xy || !t_xy || !out_model) return fail(c, FD_ERR_INVALID, "bad arguments");
    fdk::RansacArgs a{};
    const int rc = pair_args(c, a, batch, q_stride, t_stride, match_idx, *opts);
    if (rc) return rc;
    if (opts->hypotheses < 1 || opts->hypotheses > FD_RANSAC_MAX_HYPOTHESES)
        return fail(c, FD_ERR_INVALID, "hypotheses must be in [1, 4096]");
    a.hypotheses = opts->hypotheses;
    a.seed = opts->seed;
    const auto stage = [&](HostIo &io, fdk::RansacArgs &r) {
        return pair_inputs(c, io, r, q_xy, q_counts, t_xy, match_idx, pair_valid);
    };
    return ransac_call(c, a, kPairModel, kPairCorr, stage, fdk::launch_ransac,
                       {q_counts, nullptr, nullptr, out_model, out_inlier, out_counts, out_best, io_on_device});
}

int fd_ransac_refit(fd_ctx *c, int batch, const fd_refit_opts *opts, const float *q_xy, const int32_t *q_counts,
                    int32_t q_stride, const float *t_xy, int32_t t_stride, const int32_t *match_idx,
                    const uint8_t *pair_valid, const double *in_model, const uint8_t *in_inlier, double *out_model,
                    uint8_t *out_inlier, int32_t *out_counts, int32_t *out_rounds, int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!opts || !q_xy || !t_xy || !in_model || !in_inlier || !out_model) return fail(c, FD_ERR_INVALID, "bad arguments");
    fdk::RefitArgs g{};
    const int rc = pair_args(c, g.r, batch, q_stride, t_stride, match_idx, *opts);
    if (rc) return rc;
    if (opts->rounds < 1 || opts->rounds > FD_REFIT_MAX_ROUNDS) return fail(c, FD_ERR_INVALID, "rounds must be in [1, 4]");
    g.rounds = opts->rounds;
    const auto stage = [&](HostIo &io, fdk::RansacArgs &r) {
        return pair_inputs(c, io, r, q_xy, q_counts, t_xy, match_idx, pair_valid);
    };
    return refit_call(c, g, kPairModel, kPairCorr, stage, fdk::launch_ransac_refit,  // 7 inputs and 4 outputs
                      {q_counts, in_model, in_inlier, out_model, out_inlier, out_counts, out_rounds, io_on_device});
}

int fd_triangulate(fd_ctx *c, int batch, const fd_pose_opts *opts, const float *q_xy, const int32_t *q_counts, int32_t q_stride,
                   const float *t_xy, int32_t t_stride, const int32_t *match_idx, const uint8_t *pair_valid,
                   const double *in_pose, const uint8_t *in_inlier, float *out_points, uint8_t *out_valid, int32_t *out_counts,
                   int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!opts || !q_xy || !t_xy || !in_pose) return fail(c, FD_ERR_INVALID, "bad arguments");
    fdk::PoseArgs a{};
    int rc = pose_args(c, a, batch, opts, q_stride, t_stride, match_idx);
    if (rc) return rc;
    FD_HIP_TRY(c, hipSetDevice(c->device));
    rc = refuse_sync_under_capture(c, io_on_device);
    if (rc) return rc;
    if (q_stride == 0) return zero_counts(c, out_counts, batch, io_on_device);
    const size_t qs = static_cast<size_t>(batch) * q_stride;
    HostIo io(c, io_on_device);
    rc = pair_inputs(c, io, a, q_xy, q_counts, t_xy, match_idx, pair_valid);
    if (rc) return rc;
    FD_HIP_TRY(c, io.in(in_inlier, qs, a.in_inlier));
    FD_HIP_TRY(c, io.in(in_pose, static_cast<size_t>(12) * batch, a.in_model));
    FD_HIP_TRY(c, io.out_slots(out_points, qs, 3, a.out_points));
    FD_HIP_TRY(c, io.out_slots(out_valid, qs, 1, a.out_valid));
    FD_HIP_TRY(c, io.out(out_counts, batch, a.out_counts));
    FD_HIP_TRY(c, fdk::launch_triangulate(a, c->stream));
    return io.finish(q_counts, batch, q_stride);
}

int fd_pose_recover(fd_ctx *c, int batch, const fd_pose_opts *opts, const float *q_xy, const int32_t *q_counts, int32_t q_stride,
                    const float *t_xy, int32_t t_stride, const int32_t *match_idx, const uint8_t *pair_valid,
                    const double *in_model, const uint8_t *in_inlier, double *out_pose, int32_t *out_choice, float *out_points,
                    uint8_t *out_valid, int32_t *out_counts, int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!opts || !q_xy || !t_xy || !in_model || !in_inlier) return fail(c, FD_ERR_INVALID, "bad arguments");
    fdk::PoseArgs a{};
    int rc = pose_args(c, a, batch, opts, q_stride, t_stride, match_idx);
    if (rc) return rc;
    FD_HIP_TRY(c, hipSetDevice(c->device));
    rc = refuse_sync_under_capture(c, io_on_device);
    if (rc) return rc;
    const size_t poses = static_cast<size_t>(12) * batch;
    if (q_stride == 0) {  // no slots: no frame has a pose
        rc = set_output(c, out_pose, 0, sizeof(double) * poses, io_on_device);
        if (!rc) rc = set_output(c, out_choice, 0xFF, sizeof(int32_t) * batch, io_on_device);
        if (!rc) rc = zero_counts(c, out_counts, batch, io_on_device);
        return rc;
    }
    const size_t qs = static_cast<size_t>(batch) * q_stride;
    HostIo io(c, io_on_device);  // 7 inputs and 5 outputs: the whole staging pool
    rc = pair_inputs(c, io, a, q_xy, q_counts, t_xy, match_idx, pair_valid);
    if (rc) return rc;
    FD_HIP_TRY(c, io.in(in_inlier, qs, a.in_inlier));
    FD_HIP_TRY(c, io.in(in_model, static_cast<size_t>(9) * batch, a.in_model));
    FD_HIP_TRY(c, io.out(out_pose, poses, a.out_pose));
    FD_HIP_TRY(c, io.out(out_choice, batch, a.out_choice));
    FD_HIP_TRY(c, io.out_slots(out_points, qs, 3, a.out_points));
    FD_HIP_TRY(c, io.out_slots(out_valid, qs, 1, a.out_valid));
    FD_HIP_TRY(c, io.out(out_counts, batch, a.out_counts));
    FD_HIP_TRY(c, fdk::launch_pose_recover(a, c->stream));
    return io.finish(q_counts, batch, q_stride);
}

}  // extern "C"
