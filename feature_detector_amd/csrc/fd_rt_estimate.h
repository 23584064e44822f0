// Internal header of libfdhip.so's host runtime: what the estimators' entry points share (fd_rt_ransac.cpp: fd_ransac,
// fd_pnp_ransac and their refits; fd_rt_align.cpp: fd_align_ransac, fd_align_refit). The slot checks and fields, the
// workspace of a compaction kernel, and the two drivers that take a RANSAC or a refit call from hipSetDevice to
// HostIo::finish. An entry point keeps its null and option checks and supplies its argument block, two widths, how
// its own input arrays are staged, and its launcher.
#pragma once

#include "fd_ctx.h"

namespace fdrt {

// What the estimators ask of their [batch][q_stride] slots and the partners among [batch][t_stride].
inline int check_slots(fd_ctx *c, int batch, int32_t q_stride, int32_t t_stride, const int32_t *match_idx) {
    if (batch < 1) return fail(c, FD_ERR_INVALID, "batch must be >= 1");
    if (q_stride < 0 || t_stride < 0) return fail(c, FD_ERR_INVALID, "strides must be >= 0");
    if (!match_idx && t_stride < q_stride)
        return fail(c, FD_ERR_INVALID, "without match_idx slot i pairs with slot i: t_stride must be >= q_stride");
    return FD_OK;
}

// The slot fields of an argument block (RansacArgs, PoseArgs, PnpArgs, AlignArgs).
template <class A>
void slot_fields(A &a, int batch, int32_t q_stride, int32_t t_stride) {
    a.batch = batch;
    a.q_stride = q_stride;
    a.t_stride = t_stride;
}

// The workspace of a compaction kernel (RansacArgs, PnpArgs, AlignArgs): the frames' lists of `doubles` per
// correspondence, every slot's index in them, their lengths and the frames' vote words.
template <class A>
int list_workspace(fd_ctx *c, A &a, size_t doubles) {
    const size_t qs = static_cast<size_t>(a.batch) * a.q_stride;
    FD_HIP_TRY(c, ensure_as(c, c->g_corr, doubles * qs, a.corr));
    FD_HIP_TRY(c, ensure_as(c, c->g_cidx, qs, a.cidx));
    FD_HIP_TRY(c, ensure_as(c, c->g_n, a.batch, a.n));
    FD_HIP_TRY(c, ensure_as(c, c->g_best, a.batch, a.best));
    return FD_OK;
}

// An estimator call's arrays as the caller gave them, apart from the estimator's own inputs: the counts that bound
// the written inlier slots, a refit's given model and support, and the four outputs (last: out_best or out_rounds).
struct EstimateIo {
    const int32_t *q_counts;
    const double *in_model;
    const uint8_t *in_inlier;
    double *out_model;
    uint8_t *out_inlier;
    int32_t *out_counts, *out_last;
    int on_device;
};

// The four outputs in their staging order, the launch and the copy back (a: RansacArgs, PnpArgs or AlignArgs).
template <class A, class G, class Launch>
int estimate_finish(fd_ctx *c, HostIo &io, A &a, const G &g, size_t model, int32_t *&last, Launch launch, const EstimateIo &e) {
    const size_t qs = static_cast<size_t>(a.batch) * a.q_stride;
    FD_HIP_TRY(c, io.out(e.out_model, model * a.batch, a.out_model));
    FD_HIP_TRY(c, io.out_slots(e.out_inlier, qs, 1, a.out_inlier));
    FD_HIP_TRY(c, io.out(e.out_counts, a.batch, a.out_counts));
    FD_HIP_TRY(c, io.out(e.out_last, a.batch, last));
    FD_HIP_TRY(c, launch(g, c->stream));
    return io.finish(e.q_counts, a.batch, a.q_stride);
}

// A RANSAC call after its entry point's checks. a: the argument block with its slot, option, hypotheses and seed
// fields set; model, corr: doubles per model and per correspondence; stage(io, a): the estimator's input arrays,
// staged or handed on in their order.
template <class A, class Stage, class Launch>
int ransac_call(fd_ctx *c, A &a, size_t model, size_t corr, Stage stage, Launch launch, const EstimateIo &e) {
    FD_HIP_TRY(c, hipSetDevice(c->device));
    int rc = refuse_sync_under_capture(c, e.on_device);
    if (rc) return rc;
    if (a.q_stride == 0) {  // no slots: no frame has a model
        rc = set_output(c, e.out_model, 0, sizeof(double) * model * a.batch, e.on_device);
        if (!rc) rc = zero_counts(c, e.out_counts, a.batch, e.on_device);
        if (!rc) rc = set_output(c, e.out_last, 0xFF, sizeof(int32_t) * a.batch, e.on_device);
        return rc;
    }
    rc = list_workspace(c, a, corr);
    if (rc) return rc;
    FD_HIP_TRY(c, ensure_as(c, c->g_models, static_cast<size_t>(a.batch) * a.hypotheses * model, a.models));
    HostIo io(c, e.on_device);
    rc = stage(io, a);
    if (rc) return rc;
    return estimate_finish(c, io, a, a, model, a.out_best, launch, e);
}

// A refit call after its entry point's checks. g: RefitArgs, PnpRefitArgs or AlignRefitArgs with g.r's slot and
// option fields and g.rounds set; stage(io, g.r) as for ransac_call. e.in_model may be e.out_model and e.in_inlier
// e.out_inlier: an output never shares its input's staging buffer.
template <class G, class Stage, class Launch>
int refit_call(fd_ctx *c, G &g, size_t model, size_t corr, Stage stage, Launch launch, const EstimateIo &e) {
    FD_HIP_TRY(c, hipSetDevice(c->device));
    int rc = refuse_sync_under_capture(c, e.on_device);
    if (rc) return rc;
    const int batch = g.r.batch;
    if (g.r.q_stride == 0) {  // no slots: no round is accepted
        rc = copy_output(c, e.out_model, e.in_model, sizeof(double) * model * batch, e.on_device);
        if (!rc) rc = zero_counts(c, e.out_counts, batch, e.on_device);
        if (!rc) rc = zero_counts(c, e.out_last, batch, e.on_device);
        return rc;
    }
    const size_t qs = static_cast<size_t>(batch) * g.r.q_stride;
    rc = list_workspace(c, g.r, corr);
    if (rc) return rc;
    FD_HIP_TRY(c, ensure_as(c, c->g_member, 2 * qs, g.member));
    // the estimator's 5 (fd_ransac_refit), 6 (fd_pnp_refit) or 7 (fd_align_refit) inputs, these 2 and 4 outputs: with
    // fd_align_refit's 9 inputs and 4 outputs the whole staging pool
    HostIo io(c, e.on_device);
    rc = stage(io, g.r);
    if (rc) return rc;
    FD_HIP_TRY(c, io.in(e.in_model, model * batch, g.in_model));
    FD_HIP_TRY(c, io.in(e.in_inlier, qs, g.in_inlier));
    return estimate_finish(c, io, g.r, g, model, g.out_rounds, launch, e);
}

}  // namespace fdrt
