// Host runtime of libfdhip.so: windowed bundle adjustment (fd_bundle_adjust) over the kernel of fd_ba.hip.
#include <algorithm>
#include <cmath>

#include "fd_ctx.h"

using namespace fdrt;

extern "C" {

int fd_bundle_adjust(fd_ctx *c, int batch, int cams, const fd_ba_opts *opts, const double *in_poses, const uint8_t *cam_fixed,
                     const float *p_xyz, const uint8_t *p_valid, const int32_t *counts, int32_t p_stride, const float *obs_xy,
                     const uint8_t *obs_valid, int32_t o_stride, double *out_poses, float *out_points, uint8_t *out_inlier,
                     int32_t *out_counts, double *out_cost, int32_t *out_rounds, int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!opts || !in_poses || !p_xyz || !obs_xy || !out_poses) return fail(c, FD_ERR_INVALID, "bad arguments");
    if (batch < 1) return fail(c, FD_ERR_INVALID, "batch must be >= 1");
    if (cams < 1 || cams > FD_BA_MAX_CAMS) return fail(c, FD_ERR_INVALID, "cams must be in [1, 8]");
    if (p_stride < 0 || o_stride < 0) return fail(c, FD_ERR_INVALID, "strides must be >= 0");
    if (o_stride < p_stride) return fail(c, FD_ERR_INVALID, "slot i of a camera observes point i: o_stride must be >= p_stride");
    if (opts->rounds < 1 || opts->rounds > FD_BA_MAX_ROUNDS) return fail(c, FD_ERR_INVALID, "rounds must be in [1, 16]");
    if (!std::isfinite(opts->threshold) || !(opts->threshold > 0.0f)) return fail(c, FD_ERR_INVALID, "threshold must be finite and > 0");
    fdk::BaArgs a{};
    const double cam[4] = {opts->fx, opts->fy, opts->cx, opts->cy};
    int rc = check_camera(c, cam, 4, a.cam);
    if (rc) return rc;
    if (!std::isfinite(opts->lambda) || !(opts->lambda > 0.0)) return fail(c, FD_ERR_INVALID, "lambda must be finite and > 0");
    if (!std::isfinite(opts->up) || !(opts->up > 1.0)) return fail(c, FD_ERR_INVALID, "up must be finite and > 1");
    if (!(opts->down > 0.0 && opts->down <= 1.0)) return fail(c, FD_ERR_INVALID, "down must be in (0, 1]");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    rc = refuse_sync_under_capture(c, io_on_device);
    if (rc) return rc;
    const size_t poses = static_cast<size_t>(12) * cams * batch;
    if (p_stride == 0) {  // no slots: no trial is accepted
        rc = copy_output(c, out_poses, in_poses, sizeof(double) * poses, io_on_device);
        if (!rc) rc = zero_counts(c, out_counts, batch, io_on_device);
        if (!rc) rc = zero_counts(c, out_rounds, batch, io_on_device);
        if (!rc) rc = set_output(c, out_cost, 0, sizeof(double) * 2 * batch, io_on_device);
        return rc;
    }
    a.batch = batch;
    a.cams = cams;
    a.p_stride = p_stride;
    a.o_stride = o_stride;
    a.rounds = opts->rounds;
    const double t = static_cast<double>(opts->threshold);
    a.tt = t * t;
    a.lambda = opts->lambda;
    a.up = opts->up;
    a.down = opts->down;
    const size_t ps = static_cast<size_t>(batch) * p_stride, os = static_cast<size_t>(batch) * cams * o_stride;
    FD_HIP_TRY(c, ensure_as(c, c->ba_obs, ps * cams * fdk::kBaObsDoubles, a.obs));
    FD_HIP_TRY(c, ensure_as(c, c->ba_pts, ps * fdk::kBaPointDoubles, a.pts));
    FD_HIP_TRY(c, ensure_as(c, c->ba_act, ps * cams, a.act));
    HostIo io(c, io_on_device);  // 7 inputs and 5 outputs here, out_inlier after them: the whole staging pool
    FD_HIP_TRY(c, io.in(in_poses, poses, a.in_poses));
    FD_HIP_TRY(c, io.in(cam_fixed, static_cast<size_t>(batch) * cams, a.cam_fixed));
    FD_HIP_TRY(c, io.in(p_xyz, 3 * ps, a.p_xyz));
    FD_HIP_TRY(c, io.in(p_valid, ps, a.p_valid));
    FD_HIP_TRY(c, io.in(counts, batch, a.counts));
    FD_HIP_TRY(c, io.in(obs_xy, 2 * os, a.obs_xy));
    FD_HIP_TRY(c, io.in(obs_valid, os, a.obs_valid));
    FD_HIP_TRY(c, io.out(out_poses, poses, a.out_poses));
    FD_HIP_TRY(c, io.out_slots(out_points, ps, 3, a.out_points));
    FD_HIP_TRY(c, io.out(out_counts, batch, a.out_counts));
    FD_HIP_TRY(c, io.out(out_cost, static_cast<size_t>(2) * batch, a.out_cost));
    FD_HIP_TRY(c, io.out(out_rounds, batch, a.out_rounds));
    // out_inlier has a row per camera: its written prefixes are those of batch * cams frames of o_stride slots, so it
    // is staged by a second HostIo that starts behind the first one's buffers. `staged` must list every array handed
    // to io.in / io.out above, in any order: a new array goes into both places.
    const void *staged[] = {in_poses, cam_fixed, p_xyz, p_valid, counts, obs_xy, obs_valid, out_poses, out_points, out_counts, out_cost, out_rounds};
    const int used = static_cast<int>(std::count_if(std::begin(staged), std::end(staged), [](const void *p) { return p != nullptr; }));
    static_assert(sizeof(staged) / sizeof(staged[0]) + 1 == fd_ctx::kStaging, "the call's arrays and out_inlier fill the staging pool");
    HostIo rows(c, io_on_device, used);
    FD_HIP_TRY(c, rows.out_slots(out_inlier, os, 1, a.out_inlier));
    FD_HIP_TRY(c, fdk::launch_bundle_adjust(a, c->stream));
    if (io_on_device) return FD_OK;
    std::vector<int32_t> row_counts(static_cast<size_t>(batch) * cams);
    for (int b = 0; b < batch; ++b) {
        const int32_t n = counts ? static_cast<int32_t>(std::min<int64_t>(static_cast<uint32_t>(counts[b]) & fdk::kCountMask, p_stride)) : p_stride;
        std::fill(row_counts.begin() + static_cast<size_t>(b) * cams, row_counts.begin() + static_cast<size_t>(b + 1) * cams, n);
    }
    rc = rows.finish(row_counts.data(), batch * cams, o_stride);
    if (rc) return rc;
    return io.finish(counts, batch, p_stride);
}

}  // extern "C"
