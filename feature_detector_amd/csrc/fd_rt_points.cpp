// Host runtime of libfdhip.so: the point detectors. FAST's tables, the launch geometry of the per-pixel
// kernels (fd_points.hip, fd_corner_lp.hip), the detect path's workspace and the entry points
// fd_points_detect / _select / _response / _candidates.
#include <algorithm>
#include <cstdlib>
#include <limits>

#include "fd_ctx.h"

using namespace fdrt;

namespace {

// Tile height: a multiple of `period` (3 for the corner walk, 7 for FAST) that still gives the launch
// enough waves to fill 256 CUs, capped so halo rows stay a small overhead.
int choose_tile_h(int64_t batch, int tiles_x, int out_rows, int period, int max_mult) {
    const int64_t target_waves = 10240;  // ~2 rounds of resident waves at 256 CUs (measured sweep)
    int64_t h = (batch * tiles_x * static_cast<int64_t>(out_rows)) / target_waves;
    if (h < period && period == 6) {
        // small launches: the tile's serial row chain is the latency; 3 rows (9 steps of the 6-row
        // ring, the loop stops early) measured best at 640x480 batch 1 (tile_h 6/4/3/2/1: K1 11.4 /
        // 10.3 / 10.1 / 10.2 / 13.2 us, and k_select grows with the number of segments below 3).
        // Harris / Shi-Tomasi launches of this height in sorted-segment mode with thr >= 0 run
        // k_corner_short (fd_points.hip): the same workgroup footprint and segments, so nothing here or in
        // fd_ctx_reserve depends on it; 8 waves of two columns per lane per workgroup, no row ring
        // (headline step 25.39 -> 24.06 us, profiles/r08_k1_short_tile_ab.txt).
        h = 3;  // (fdk's kShortTileH: launch_corner tests tile_h against it)
    } else {
        h = std::max<int64_t>(h, period);
        h = ((h + period - 1) / period) * period;
    }
    h = std::min<int64_t>(h, static_cast<int64_t>(period) * max_mult);
    return static_cast<int>(h);
}

// FAST score table (FastOffsets::run_lut): for every 16-bit ring mask, the reference's two-pass count
// (feature_point_fast_detector.cpp:55-78) of consecutive set bits, run over the mask twice without a
// reset between the passes (so a run may wrap around), stopping once 16 is reached.
int ensure_run_lut(fd_ctx *c) {
    if (c->run_lut_ready) return FD_OK;
    FD_HIP_TRY(c, ensure(c, c->run_lut, 65536));
    std::vector<uint8_t> table(65536);
    for (uint32_t b = 0; b < 65536; ++b) {
        int run = 0, best = 0;
        for (int pass = 0; pass < 2 && best < 16; ++pass)
            for (int k = 0; k < 16; ++k) {
                run = ((b >> k) & 1u) ? run + 1 : 0;
                best = std::max(best, run);
            }
        table[b] = static_cast<uint8_t>(std::min(best, 16));
    }
    FD_HIP_TRY(c, hipMemcpyAsync(c->run_lut.p, table.data(), 65536, hipMemcpyHostToDevice, c->stream));
    FD_HIP_TRY(c, hipStreamSynchronize(c->stream));  // the host table dies with this call
    c->run_lut_ready = true;
    return FD_OK;
}

// Geometry of the per-pixel launch for a detector kind.
struct PointGeom {
    int border;    // 2 for Harris/Shi-Tomasi, 3 for FAST
    int out_rows;  // rows of the candidate region
    int tiles_x, tiles_y, tile_h;
    int blocks_per_frame;
    bool empty;
};

// Columns per lane of k_corner_lp for a corner launch in list mode (fd_points_detect /
// fd_points_response); 0 = k_corner (FAST, negative thresholds, the raster-ordered candidate stage).
// Large launches take wide lanes (the halo exchanges and loop control shared by more pixels), small
// ones narrow lanes (more waves, shorter serial row chains). FD_PX overrides (A/B).
int corner_px(int kind, int batch, int rows, int cols, float thr) {
    if (kind == FD_FAST || !(thr >= 0.0f)) return 0;
    // k_corner_lp addresses a frame's list through a buffer resource: list_cap * 4 bytes < 2^32
    if (static_cast<int64_t>(rows) * cols >= (int64_t(1) << 30)) return 0;
    if (const char *e = ab_env("FD_PX")) {
        const int v = std::atoi(e);
        if (v == 0 || v == 2 || v == 4 || v == 8) return v;
    }
    // Measured (north-star shape, 1080p x 256): 4 columns per lane 4-5 % faster than k_corner, 8 slower
    // (VGPR-limited to 3 waves per SIMD); at 640x480 x 1 k_corner is faster (11.4 vs 10.0 us).
    const int64_t px = static_cast<int64_t>(batch) * rows * cols;
    return px >= (int64_t(1) << 21) ? 4 : 0;
}

PointGeom point_geom(int kind, int batch, int rows, int cols, int px = 0) {
    PointGeom g{};
    g.border = kind == FD_FAST ? 3 : 2;
    g.out_rows = rows - 2 * g.border;
    const int out_cols = cols - 2 * g.border;
    g.empty = g.out_rows <= 0 || out_cols <= 0;
    const int tw = px ? fdk::lp_tile_w(px) : fdk::kTileW;
    g.tiles_x = std::max(1, (cols - g.border + tw - 1) / tw);
    const int period = kind == FD_FAST ? 7 : 6;  // rows per unrolled loop iteration of the kernel
    g.tile_h = choose_tile_h(batch, g.tiles_x, std::max(g.out_rows, 1), period, kind == FD_FAST ? 9 : 100);
    g.tiles_y = std::max(1, (std::max(g.out_rows, 1) + g.tile_h - 1) / g.tile_h);
    g.blocks_per_frame = (g.tiles_x * g.tiles_y + 3) / 4;
    return g;
}

// Sorted-segment lists (PointsArgs::segdesc): for launches small enough that k_select can give every
// workgroup segment of a frame its own threads (<= kSelectThreads segments per frame) and that would
// otherwise gather their first chunk inside k_select (no k_gather kernel). FD_SEG_LISTS=0: off (A/B).
bool use_seg_lists(const PointGeom &g, int rows, int cols) {
    if (g.empty) return false;
    if (const char *e = ab_env("FD_SEG_LISTS"); e && std::atoi(e) == 0) return false;
    return g.blocks_per_frame <= fdk::kSelectThreads && static_cast<int64_t>(rows) * cols < (1 << 20);
}

// The per-pixel launch of a geometry: frames, tiles and threshold (the callers add the lists or segments).
fdk::PointsArgs points_args(const uint8_t *dframes, int batch, int rows, int cols, const PointGeom &g, int px, float thr) {
    fdk::PointsArgs a{};
    a.px = px;
    a.frames = dframes;
    a.batch = batch;
    a.rows = rows;
    a.cols = cols;
    a.tiles_x = g.tiles_x;
    a.tiles_y = g.tiles_y;
    a.tile_h = g.tile_h;
    a.blocks_per_frame = g.blocks_per_frame;
    a.aligned4 = (cols % 4 == 0) && (reinterpret_cast<uintptr_t>(dframes) % 4 == 0);
    a.thr = thr;
    return a;
}

// The prefix tables of masked FAST's candidate numbering (PointsArgs::row_base / word_pref).
int mask_scan_tables(fd_ctx *c, int batch, int rows, int cols) {
    FD_HIP_TRY(c, ensure(c, c->row_base, sizeof(int32_t) * static_cast<size_t>(batch) * rows));
    FD_HIP_TRY(c, ensure(c, c->word_pref, sizeof(int32_t) * static_cast<size_t>(batch) * rows * ((cols + 31) / 32)));
    return FD_OK;
}

// FAST with prior features: scan the mask into the prefix tables and hand them to the launch.
int fast_mask_scan(fd_ctx *c, const PriorInfo &pi, fdk::PointsArgs &a) {
    if (!pi.mask) return FD_OK;
    if (a.rows > 4096) return fail(c, FD_ERR_INVALID, "FAST with prior features supports rows <= 4096");
    if (const int rc = mask_scan_tables(c, a.batch, a.rows, a.cols)) return rc;
    a.row_base = as<int32_t>(c->row_base);
    a.word_pref = as<int32_t>(c->word_pref);
    FD_HIP_TRY(c, fdk::launch_fast_mask_scan(pi.mask, pi.wpr, a.batch, a.rows, a.cols, as<int32_t>(c->row_base),
                                             as<int32_t>(c->word_pref), c->stream));
    return FD_OK;
}

}  // namespace

namespace fdrt {

// FAST running offset o_0 = 1e-5f, o_{k+1} = fl(o_k + 1e-5f) (feature_point_fast_detector.cpp:85,93)
// as runs of constant increment; verified exact against the recurrence before use.
int build_offsets(fd_ctx *c, int64_t n, float thr) {
    int rc = ensure_run_lut(c);
    if (rc) return rc;
    c->off.run_lut = as<uint8_t>(c->run_lut);
    if (c->off_n == n && c->off_thr == thr) return FD_OK;
    fdk::FastOffsets o{};
    o.nseg = 0;
    o.k0 = std::numeric_limits<int64_t>::max();
    std::vector<float> seq(static_cast<size_t>(std::max<int64_t>(n, 1)));
    float v = 1e-5f;
    double prev_inc = -1.0;
    for (int64_t k = 0; k < n; ++k) {
        seq[static_cast<size_t>(k)] = v;
        const float next = v + 1e-5f;
        const double inc = static_cast<double>(next) - static_cast<double>(v);
        if (k == 0 || inc != prev_inc) {
            if (o.nseg >= fdk::kMaxOffsetSegs) return fail(c, FD_ERR_INVALID, "FAST offset table too large");
            o.k_start[o.nseg] = k;
            o.o_start[o.nseg] = static_cast<double>(v);
            o.inc[o.nseg] = inc;
            ++o.nseg;
            prev_inc = inc;
        }
        if (o.k0 == std::numeric_limits<int64_t>::max() && v > thr) o.k0 = k;
        v = next;
    }
    if (o.nseg == 0) {
        o.nseg = 1;
        o.k_start[0] = 0;
        o.o_start[0] = 1e-5;
        o.inc[0] = 0.0;
    }
    int s = 0;
    for (int64_t k = 0; k < n; ++k) {
        while (s + 1 < o.nseg && o.k_start[s + 1] <= k) ++s;
        const float r = static_cast<float>(o.o_start[s] + static_cast<double>(k - o.k_start[s]) * o.inc[s]);
        if (r != seq[static_cast<size_t>(k)]) return fail(c, FD_ERR_INVALID, "FAST offset table not exact");
    }
    o.run_lut = as<uint8_t>(c->run_lut);
    c->off = o;
    c->off_n = n;
    c->off_thr = thr;
    return FD_OK;
}

int detect_workspace(fd_ctx *c, int kind, int batch, int rows, int cols, int64_t max_prior_total, int64_t &list_cap,
                     SelectBufs &sb) {
    const int64_t px = static_cast<int64_t>(rows) * cols;
    list_cap = (kind == FD_FAST ? px : px / 2) + 64;
    int rc = select_buffers(c, batch, list_cap, sb);
    if (rc) return rc;
    if ((rc = prior_buffers(c, batch, rows, cols, max_prior_total))) return rc;
    if (kind == FD_FAST) {
        if ((rc = ensure_run_lut(c))) return rc;
        if (!c->fast_cut.p) {  // the emission cut's words (zero: no cut, until a selection proposes one)
            FD_HIP_TRY(c, ensure(c, c->fast_cut, 2 * sizeof(uint32_t)));
            FD_HIP_TRY(c, hipMemsetAsync(c->fast_cut.p, 0, c->fast_cut.n, c->stream));
        }
        if (max_prior_total > 0 && (rc = mask_scan_tables(c, batch, rows, cols))) return rc;
    }
    if (c->tie_order == FD_TIES_REFERENCE) {  // k_select_reference's scratch
        fdk::RefSortArgs r{};
        if ((rc = ref_buffers(c, batch, rows, cols, list_cap, r))) return rc;
    }
    // the segment lists of either kernel a corner launch may take (k_corner, k_corner_lp: the threshold decides)
    for (const int lp : {0, corner_px(kind, batch, rows, cols, 0.0f)}) {
        const PointGeom g = point_geom(kind, batch, rows, cols, lp);
        if (!use_seg_lists(g, rows, cols)) continue;
        const size_t nseg = static_cast<size_t>(batch) * g.blocks_per_frame;
        FD_HIP_TRY(c, ensure(c, c->segdesc, sizeof(uint2) * nseg));
        FD_HIP_TRY(c, ensure(c, c->seghead, sizeof(uint64_t) * fdk::kSegHead * nseg));
    }
    return FD_OK;
}

}  // namespace fdrt

extern "C" {

int fd_points_detect(fd_ctx *c, int kind, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                     const fd_point_opts *opts, const float *prior_xy, const int32_t *prior_counts, uint32_t need,
                     float *out_xy, int32_t out_stride, int32_t *out_counts, int outputs_on_device) {
    int rc = check_shape(c, kind, batch, rows, cols);
    if (rc) return rc;
    if (!opts || !out_xy || !out_counts || out_stride < 1) return fail(c, FD_ERR_INVALID, "bad output arguments");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = refuse_sync_under_capture(c, outputs_on_device))) return rc;
    const uint8_t *dframes = nullptr;
    if ((rc = stage_frames(c, frames, frames_on_device, batch, rows, cols, dframes))) return rc;
    PriorInfo pi;
    rc = setup_priors(c, batch, rows, cols, opts->min_feature_distance, prior_xy, prior_counts, pi);
    if (rc) return rc;

    const float thr = opts->min_valid_response;
    const int px = corner_px(kind, batch, rows, cols, thr);
    const PointGeom g = point_geom(kind, batch, rows, cols, px);
    int64_t cap = 0;
    SelectBufs sb{};
    if ((rc = detect_workspace(c, kind, batch, rows, cols, pi.total, cap, sb))) return rc;

    fdk::PointsArgs a = points_args(dframes, batch, rows, cols, g, px, thr);
    list_outputs(c, a.list, cap, sb);
    a.mask = pi.mask;
    a.mask_wpr = pi.wpr;
    if (use_seg_lists(g, rows, cols)) {
        a.segdesc = as<uint2>(c->segdesc);
        a.seg_bad = sb.seg_bad;
        a.seghead = as<uint64_t>(c->seghead);
    }
    const int64_t n_off = static_cast<int64_t>(rows - 6) * (cols - 6);
    if (kind == FD_FAST && !g.empty) {
        if ((rc = build_offsets(c, n_off, thr))) return rc;
    }
    key_map(kind, thr, kind == FD_FAST && !g.empty ? &c->off : nullptr, n_off, a.list.key_base, a.list.key_lz);
    // FAST's emission cut (PointsArgs::emit_cut): only in the raster tie order (the
    // reference order's emulation needs every candidate in push order).
    const bool fast_cut = kind == FD_FAST && !g.empty && c->tie_order == FD_TIES_RASTER;
    c->sel_dirty = true;  // until k_select is enqueued: it resets the control block
    if (!g.empty) {
        if (kind == FD_FAST) {
            if ((rc = fast_mask_scan(c, pi, a))) return rc;
            if (fast_cut) {
                // the emission cut of this call (written by the previous FAST call's selection) and the word
                // this call's selection proposes the next one in: two words, alternating per call
                const int p = c->fast_cut_parity;
                c->fast_cut_parity ^= 1;
                a.emit_cut = as<uint32_t>(c->fast_cut) + p;
                a.emit_cut_next = as<uint32_t>(c->fast_cut) + (p ^ 1);
                a.skipped = sb.skipped;
            }
            FD_HIP_TRY(c, fdk::launch_fast(false, a, c->off, c->stream));
        } else {
            FD_HIP_TRY(c, fdk::launch_corner(kind, false, a, c->stream));
        }
    }

    SelectCall sc(batch, rows, cols, opts->min_feature_distance, need, cap, a.list.key_base, a.list.key_lz);
    sc.segdesc = a.segdesc;
    sc.seghead = a.seghead;
    sc.nseg = g.blocks_per_frame;
    sc.wide_eager = kind == FD_FAST;
    if (fast_cut) {
        sc.redo_points = &a;
        sc.redo_off = &c->off;
        sc.skipped = sb.skipped;
        sc.cut_cur = a.emit_cut;
        sc.cut_next = a.emit_cut_next;
    }
    return run_select(c, sc, pi, sb, out_xy, out_stride, out_counts, outputs_on_device, frames_on_device);
}

// SelectGoodFeatures (feature_point_detector.cpp:54-88) over caller-supplied candidates (the
// ComputeCandidates seam, :20): k_cand_lists puts them into the selection's list format (push order
// kept), then the same k_select as fd_points_detect, with the full float order as key map.
int fd_points_select(fd_ctx *c, int batch, int rows, int cols, const fd_point_opts *opts, const float *cand_resp,
                     const int32_t *cand_x, const int32_t *cand_y, const int64_t *cand_counts, int64_t cand_cap,
                     int cands_on_device, const float *prior_xy, const int32_t *prior_counts, uint32_t need,
                     float *out_xy, int32_t out_stride, int32_t *out_counts, int outputs_on_device) {
    int rc = check_shape(c, FD_HARRIS, batch, rows, cols);
    if (rc) return rc;
    if (!opts || !out_xy || !out_counts || out_stride < 1) return fail(c, FD_ERR_INVALID, "bad output arguments");
    if (!cand_counts || cand_cap < 0 || cand_cap > 0xFFFFFFFFll)
        return fail(c, FD_ERR_INVALID, "cand_counts is NULL or cand_cap out of range");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = refuse_sync_under_capture(c, outputs_on_device))) return rc;
    int64_t max_n = cand_cap;
    if (!cands_on_device) {
        max_n = 0;
        for (int b = 0; b < batch; ++b) {
            if (cand_counts[b] < 0 || cand_counts[b] > cand_cap)
                return fail(c, FD_ERR_INVALID, "frame " + std::to_string(b) + ": candidate count outside [0, cand_cap]");
            max_n = std::max(max_n, cand_counts[b]);
        }
    }
    if (max_n > 0 && (!cand_resp || !cand_x || !cand_y)) return fail(c, FD_ERR_INVALID, "candidate arrays are NULL");
    PriorInfo pi;
    rc = setup_priors(c, batch, rows, cols, opts->min_feature_distance, prior_xy, prior_counts, pi);
    if (rc) return rc;
    const int64_t cap = std::max<int64_t>(max_n, 64);
    SelectBufs sb{};
    if ((rc = select_buffers(c, batch, cap, sb))) return rc;
    fdk::CandInArgs a{};
    a.stride = cands_on_device ? cand_cap : max_n;
    if (cands_on_device) {
        a.resp = cand_resp;
        a.x = cand_x;
        a.y = cand_y;
        a.counts = cand_counts;
    } else {  // pack the frames' lists at stride max_n
        const size_t tot = static_cast<size_t>(batch) * static_cast<size_t>(std::max<int64_t>(max_n, 1));
        FD_HIP_TRY(c, ensure_as(c, c->c_resp, tot, a.resp));
        FD_HIP_TRY(c, ensure_as(c, c->c_x, tot, a.x));
        FD_HIP_TRY(c, ensure_as(c, c->c_y, tot, a.y));
        FD_HIP_TRY(c, ensure_as(c, c->c_counts, batch, a.counts));
        for (int b = 0; b < batch; ++b) {
            const size_t n = static_cast<size_t>(cand_counts[b]);
            if (n == 0) continue;
            const size_t src = static_cast<size_t>(b) * static_cast<size_t>(cand_cap);
            const size_t dst = static_cast<size_t>(b) * static_cast<size_t>(max_n);
            FD_HIP_TRY(c, hipMemcpyAsync(as<float>(c->c_resp) + dst, cand_resp + src, sizeof(float) * n,
                                         hipMemcpyHostToDevice, c->stream));
            FD_HIP_TRY(c, hipMemcpyAsync(as<int32_t>(c->c_x) + dst, cand_x + src, sizeof(int32_t) * n,
                                         hipMemcpyHostToDevice, c->stream));
            FD_HIP_TRY(c, hipMemcpyAsync(as<int32_t>(c->c_y) + dst, cand_y + src, sizeof(int32_t) * n,
                                         hipMemcpyHostToDevice, c->stream));
        }
        FD_HIP_TRY(c, hipMemcpyAsync(c->c_counts.p, cand_counts, sizeof(int64_t) * batch, hipMemcpyHostToDevice,
                                     c->stream));
    }
    a.batch = batch;
    a.rows = rows;
    a.cols = cols;
    list_outputs(c, a.list, cap, sb);
    // any float: keys from float_key(-inf) - 1 (never 0) to float_key(+inf), the whole 32-bit range
    a.list.key_base = host_float_key(-std::numeric_limits<float>::infinity()) - 1u;
    a.list.key_lz = 0;
    a.bad = sb.pre_count;
    a.border = -1;  // list position = push position
    c->sel_dirty = true;  // until k_select is enqueued: it resets the control block
    FD_HIP_TRY(c, fdk::launch_cand_lists(a, max_n, c->stream));
    if (!cands_on_device) FD_HIP_TRY(c, hipStreamSynchronize(c->stream));  // caller's host arrays were the sources
    SelectCall sc(batch, rows, cols, opts->min_feature_distance, need, cap, a.list.key_base, a.list.key_lz);
    sc.value_flag = true;
    sc.push_order = true;
    sc.dup_keys = true;
    sc.value_msg = "a candidate outside the frame, a NaN response or a bad candidate count";
    return run_select(c, sc, pi, sb, out_xy, out_stride, out_counts, outputs_on_device, 1);
}

static int points_response(fd_ctx *c, int kind, const uint8_t *frames, int batch, int rows, int cols,
                           const fd_point_opts *opts, float *out_resp, uint32_t *out_idx, int64_t cand_cap,
                           uint32_t *out_counts, bool reset_counts) {
    int rc = check_shape(c, kind, batch, rows, cols);
    if (rc) return rc;
    if (!opts || !frames || !out_resp || !out_idx || !out_counts || cand_cap < 1)
        return fail(c, FD_ERR_INVALID, "bad arguments");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    // k_corner_lp addresses the caller's list through a buffer resource of cand_cap * 4 bytes and
    // 32-bit byte offsets: larger capacities take k_corner (64-bit positions against the int64 cap).
    const int px = cand_cap < (int64_t(1) << 30) ? corner_px(kind, batch, rows, cols, opts->min_valid_response) : 0;
    const PointGeom g = point_geom(kind, batch, rows, cols, px);
    if (reset_counts) FD_HIP_TRY(c, hipMemsetAsync(out_counts, 0, sizeof(uint32_t) * batch, c->stream));
    if (g.empty) return FD_OK;
    fdk::PointsArgs a = points_args(frames, batch, rows, cols, g, px, opts->min_valid_response);
    list_outputs(a.list, out_resp, out_idx, cand_cap, out_counts, nullptr);  // (no selection: no histogram, no key map)
    if (kind == FD_FAST) {
        rc = build_offsets(c, static_cast<int64_t>(rows - 6) * (cols - 6), opts->min_valid_response);
        if (rc) return rc;
        FD_HIP_TRY(c, fdk::launch_fast(false, a, c->off, c->stream));
    } else {
        FD_HIP_TRY(c, fdk::launch_corner(kind, false, a, c->stream));
    }
    return FD_OK;
}

int fd_points_response(fd_ctx *c, int kind, const uint8_t *frames, int batch, int rows, int cols,
                       const fd_point_opts *opts, float *out_resp, uint32_t *out_idx, int64_t cand_cap,
                       uint32_t *out_counts) {
    return points_response(c, kind, frames, batch, rows, cols, opts, out_resp, out_idx, cand_cap, out_counts, true);
}

int fd_points_response_append(fd_ctx *c, int kind, const uint8_t *frames, int batch, int rows, int cols,
                              const fd_point_opts *opts, float *out_resp, uint32_t *out_idx, int64_t cand_cap,
                              uint32_t *out_counts) {
    return points_response(c, kind, frames, batch, rows, cols, opts, out_resp, out_idx, cand_cap, out_counts, false);
}

int fd_points_candidates(fd_ctx *c, int kind, const uint8_t *frames, int frames_on_device, int batch, int rows,
                         int cols, const fd_point_opts *opts, const float *prior_xy, const int32_t *prior_counts,
                         float *out_resp, int32_t *out_x, int32_t *out_y, int64_t cand_cap, int64_t *out_counts,
                         float *out_response_map, int outputs_on_device) {
    int rc = check_shape(c, kind, batch, rows, cols);
    if (rc) return rc;
    if (!opts || !out_resp || !out_x || !out_y || !out_counts || cand_cap < 0)
        return fail(c, FD_ERR_INVALID, "bad output arguments");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    const uint8_t *dframes = nullptr;
    if ((rc = stage_frames(c, frames, frames_on_device, batch, rows, cols, dframes))) return rc;
    PriorInfo pi;
    rc = setup_priors(c, batch, rows, cols, opts->min_feature_distance, prior_xy, prior_counts, pi);
    if (rc) return rc;

    const PointGeom g = point_geom(kind, batch, rows, cols);
    const int segcap = kind == FD_FAST ? fdk::kSegFast : fdk::kSegCorner;
    const size_t nseg = static_cast<size_t>(batch) * rows * g.tiles_x;
    FD_HIP_TRY(c, ensure(c, c->seg_cnt, sizeof(int32_t) * nseg));
    FD_HIP_TRY(c, ensure(c, c->seg, sizeof(fdk::Cand) * nseg * segcap));
    const size_t npx = static_cast<size_t>(batch) * rows * cols;
    float *dmap = nullptr;
    if (out_response_map) {
        dmap = out_response_map;
        if (!outputs_on_device) FD_HIP_TRY(c, ensure_as(c, c->resp_map, npx, dmap));
        FD_HIP_TRY(c, hipMemsetAsync(dmap, 0, sizeof(float) * npx, c->stream));
    }
    float *dr = out_resp;
    int32_t *dx = out_x, *dy = out_y;
    int64_t *dc = out_counts;
    const size_t ncap = static_cast<size_t>(std::max<int64_t>(cand_cap, 1)) * batch;
    if (!outputs_on_device) {
        FD_HIP_TRY(c, ensure_as(c, c->c_resp, ncap, dr));
        FD_HIP_TRY(c, ensure_as(c, c->c_x, ncap, dx));
        FD_HIP_TRY(c, ensure_as(c, c->c_y, ncap, dy));
        FD_HIP_TRY(c, ensure_as(c, c->c_counts, batch, dc));
    }
    if (g.empty) {
        FD_HIP_TRY(c, hipMemsetAsync(dc, 0, sizeof(int64_t) * batch, c->stream));
    } else {
        fdk::PointsArgs a = points_args(dframes, batch, rows, cols, g, 0, opts->min_valid_response);  // (px 0: k_corner)
        a.mask = pi.mask;
        a.mask_wpr = pi.wpr;
        a.seg_cnt = as<int32_t>(c->seg_cnt);
        a.seg = as<fdk::Cand>(c->seg);
        a.resp_map = dmap;
        if (kind == FD_FAST) {
            rc = build_offsets(c, static_cast<int64_t>(rows - 6) * (cols - 6), opts->min_valid_response);
            if (rc) return rc;
            if ((rc = fast_mask_scan(c, pi, a))) return rc;
            FD_HIP_TRY(c, fdk::launch_fast(true, a, c->off, c->stream));
        } else {
            FD_HIP_TRY(c, fdk::launch_corner(kind, true, a, c->stream));
        }
        fdk::CompactArgs k{};
        k.seg_cnt = a.seg_cnt;
        k.seg = a.seg;
        k.rows = rows;
        k.cols = cols;
        k.tiles_x = g.tiles_x;
        k.seg_cap = segcap;
        k.row_lo = g.border;
        k.row_hi = rows - g.border;
        k.out_resp = dr;
        k.out_x = dx;
        k.out_y = dy;
        k.cap = cand_cap;
        k.out_counts = dc;
        FD_HIP_TRY(c, fdk::launch_compact(k, batch, c->stream));
    }
    if (!outputs_on_device) {
        FD_HIP_TRY(c, hipMemcpyAsync(out_counts, dc, sizeof(int64_t) * batch, hipMemcpyDeviceToHost, c->stream));
        if (cand_cap > 0) {
            FD_HIP_TRY(c, hipMemcpyAsync(out_resp, dr, sizeof(float) * cand_cap * batch, hipMemcpyDeviceToHost, c->stream));
            FD_HIP_TRY(c, hipMemcpyAsync(out_x, dx, sizeof(int32_t) * cand_cap * batch, hipMemcpyDeviceToHost, c->stream));
            FD_HIP_TRY(c, hipMemcpyAsync(out_y, dy, sizeof(int32_t) * cand_cap * batch, hipMemcpyDeviceToHost, c->stream));
        }
        if (out_response_map)
            FD_HIP_TRY(c, hipMemcpyAsync(out_response_map, dmap, sizeof(float) * npx, hipMemcpyDeviceToHost, c->stream));
        FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (int b = 0; b < batch; ++b)
            if (out_counts[b] > cand_cap) return fail(c, FD_ERR_CAPACITY, "cand_cap smaller than the candidates found");
    } else if (!frames_on_device) {
        FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return FD_OK;
}

}  // extern "C"
