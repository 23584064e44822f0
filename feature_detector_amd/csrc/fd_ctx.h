// Internal header of libfdhip.so's host runtime (fd_rt_*.cpp): the context behind the C ABI of
// include/fd_hip.h, its owning workspace buffers, and the helpers the runtime's files share. Everything
// but struct fd_ctx (the C ABI's opaque type) lives in namespace fdrt.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "fd_hip.h"
#include "fd_kernels.h"

namespace fdrt {

// What the context owns, released with it (null until created): a stream, an event, or workspace memory.
template <typename H, hipError_t (*Release)(H)>
struct Owned {
    H p = nullptr;
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() {
        if (p) (void)Release(p);
    }
    operator H() const { return p; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
// Grow-only workspace memory of n bytes, grown by ensure() / ensure_host() only: device memory
// (hipMalloc) and pinned host memory (hipHostMalloc).
template <hipError_t (*Free)(void *)>
struct Buf : Owned<void *, Free> {
    size_t n = 0;
};
using DevBuf = Buf<hipFree>;
using HostBuf = Buf<hipHostFree>;

}  // namespace fdrt

// Members are destroyed in reverse order of declaration: the handles come first so that they outlive
// every buffer (fd_ctx_destroy: buffers freed, then the events, the side stream, the own stream).
struct fd_ctx {
    int device = 0;
    std::string err;
    fdrt::Stream own_stream;
    // fd_lsd_lines' seed order: a side stream (the sort overlaps the lists' copy and the host setup) and its
    // two events (lists ready -> sort; sort copied back)
    fdrt::Stream aux;
    fdrt::Event l_ev1, l_ev0;
    fdrt::Event xev;  // orders a stream switch after the old stream's work (fd_ctx_set_stream)
    hipStream_t stream = nullptr;  // the stream in use: own_stream or the caller's
    // workspace
    fdrt::DevBuf frames, prior_xy, prior_frame, prior_counts, mask, row_base, word_pref;
    fdrt::DevBuf list_resp, list_idx, grid;
    // selection control block: [batch][kHistBins] level-0 histograms, then list_count per frame.
    // Zero between calls: k_select resets what a call used. sel_dirty marks a call whose kernels may
    // not have run to the end (the next call clears the block first).
    fdrt::DevBuf selctl, pre_keys, wide_keys, segdesc, seghead;
    bool sel_dirty = true;
    fdrt::DevBuf seg_cnt, seg, resp_map, c_resp, c_x, c_y, c_counts;
    fdrt::DevBuf l_norm, l_angle, l_valid, l_cnt, l_base, l_idx, l_counts, l_bits;
    // host-pointer calls of the keypoint stages (BRIEF, matchers, tracker, refinement, RANSAC, NN descriptors) and
    // of fd_frames_warp stage their arrays here, in call order (fdrt::HostIo); the widest calls are a model-gated match (9 inputs, 3 outputs), fd_pose_recover (7 and 5), fd_pnp_refit (8 and 4), fd_align_refit (9 and 4) and fd_bundle_adjust (7 and 6)
    static constexpr int kStaging = 13;
    fdrt::DevBuf staging[kStaging];
    // the matchers' cross-check reverse table ([batch][t_stride] best query of every train descriptor) and
    // fd_nn_match's norms of both sets ([batch][q_stride], then [batch][t_stride]); the model-gated matchers' gate
    // vectors of both sets ([batch][q_stride][4] doubles, then [batch][t_stride][4])
    fdrt::DevBuf m_rev, m_norm, m_gate;
    // fd_flow_lk: the backward pass's results ([batch][stride] positions and status)
    fdrt::DevBuf f_bxy, f_bst;
    // fd_ransac: the frames' correspondence lists ([batch][q_stride] conditioned (x, y, u, v) doubles), every
    // slot's index in them, their lengths, the hypotheses' models ([batch][hypotheses][9] doubles) and the
    // per-frame best-hypothesis words; fd_ransac_refit: the support sets by list position ([batch][2][q_stride] bytes).
    // fd_pnp_ransac and fd_pnp_refit use the same buffers with 5 doubles per correspondence and 12 per hypothesis,
    // fd_align_ransac and fd_align_refit with 6 and 13
    fdrt::DevBuf g_corr, g_cidx, g_n, g_models, g_best, g_member;
    // fd_bundle_adjust: a trial's linearisation per observation ([batch][cams][p_stride][52] doubles) and per point
    // ([batch][p_stride][15] doubles), and the observations' state bytes ([batch][cams][p_stride])
    fdrt::DevBuf ba_obs, ba_pts, ba_act;
    // fd_frames_equalize: the tiles' LUTs ([batch][tiles_y][tiles_x][256] bytes), then the columns' and rows'
    // interpolation entries ([cols + rows] words)
    fdrt::DevBuf e_ws;
    fdrt::DevBuf n_heat, n_map, n_xy, n_counts, n_out;
    fdrt::DevBuf dbg;
    // per-frame status of the last selection call: [batch] FD_FRAME_* flags, then [batch] candidate
    // counts (internal); status_batch = its frame count (0: no selection call yet)
    fdrt::DevBuf status;
    int status_batch = 0;
    int tie_order = FD_TIES_RASTER;
    fdrt::DevBuf ord, ord_meta;  // FD_TIES_REFERENCE host path: host-computed visiting orders of flagged frames
    fdrt::DevBuf r_x, r_lpos, r_rpos, r_ord, r_ctl, r_wcnt, r_wfr;  // FD_TIES_REFERENCE on the GPU (k_select_reference scratch)
    fdrt::DevBuf run_lut;   // FAST score per 16-bit ring mask (FastOffsets::run_lut), filled once
    bool run_lut_ready = false;
    fdrt::DevBuf fast_cut;  // FAST emission cut: two float words, read / proposed alternately per call
    int fast_cut_parity = 0;
    // fd_lsd_lines: compact lists (device), their pinned host copies, frame 0's final state
    // (l_lists: one buffer of three sections, map index | norm | angle, copied back in one transfer)
    fdrt::DevBuf l_lists, l_fbase;
    fdrt::HostBuf h_lists;
    std::vector<int32_t> st_idx;
    std::vector<float> st_norm, st_angle;
    std::vector<uint8_t> st_used;
    // fd_lsd_lines' seed order on the GPU: lists in the selection's format, status + counts, the orders'
    // and statuses' pinned host copies
    fdrt::DevBuf l_sresp, l_sidx, l_sst;
    fdrt::HostBuf h_ord, h_sst;
    // fd_png_frames: decoded samples of a batch (pinned) and their device copy (colour input)
    fdrt::HostBuf h_png;
    fdrt::DevBuf d_png;
    // host-output selection calls: status words, counts and features come back in one copy into h_res
    // (pinned); the status words stay cached on the host (h_status) for fd_ctx_frame_status until the
    // next selection call
    fdrt::HostBuf h_res;
    std::vector<uint32_t> h_status;
    bool h_status_valid = false;
    // FAST offset table cache
    int64_t off_n = -1;
    float off_thr = 0.0f;
    fdk::FastOffsets off{};
};

namespace fdrt {

// Test and diagnostic switches (FD_PX, FD_SEG_LISTS, FD_SELECT_STAMPS, ...) take effect only when FD_DEBUG_AB is
// set as well, so a stray variable in a user's environment cannot change the library's code path.
const char *ab_env(const char *name);
int fail(fd_ctx *c, int code, const std::string &msg);

#define FD_HIP_TRY(ctx, expr)                                                                                    \
    do {                                                                                                         \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess)                                                                                    \
            return fdrt::fail((ctx), FD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));             \
    } while (0)

// Grow-only (fd_rt_context.cpp): growing under stream capture fails with hipErrorStreamCaptureUnsupported.
hipError_t ensure(fd_ctx *c, DevBuf &b, size_t bytes);
hipError_t ensure_host(HostBuf &b, size_t bytes);

template <typename T>
T *as(DevBuf &b) {
    return static_cast<T *>(b.p);
}
// ensure() for n elements of T; `out` then points at the buffer.
template <typename T>
hipError_t ensure_as(fd_ctx *c, DevBuf &b, size_t n, T *&out) {
    const hipError_t e = ensure(c, b, sizeof(T) * n);
    if (e == hipSuccess) out = static_cast<T *>(b.p);
    return e;
}

int check_shape(fd_ctx *c, int kind, int batch, int rows, int cols, bool points = true);
// Stage the frames on the device (or use the caller's device pointer).
int stage_frames(fd_ctx *c, const uint8_t *frames, int on_device, int batch, int rows, int cols,
                 const uint8_t *&dframes);

struct PriorInfo {
    int64_t total = 0;
    const uint32_t *mask = nullptr;
    const int32_t *counts_dev = nullptr;
    int wpr = 0;
};

// The prior features' device buffers for up to `total` priors in the batch (setup_priors, fd_ctx_reserve).
int prior_buffers(fd_ctx *c, int batch, int rows, int cols, int64_t total);
// Upload prior features and draw their boxes into the mask bitmap (feature_point_detector.cpp:90-98).
int setup_priors(fd_ctx *c, int batch, int rows, int cols, int dist, const float *prior_xy,
                 const int32_t *prior_counts, PriorInfo &pi);

// Calls that will synchronise the context stream (host outputs) cannot run while that stream is being
// captured into a graph: refused at entry, before any work is enqueued.
int refuse_sync_under_capture(fd_ctx *c, int outputs_on_device);

// Host outputs of the per-keypoint stages: the kernel writes slots [0, counts[b]) of frame b only (all `stride`
// without counts). Copies that prefix of every array back, frame by frame, so that the caller's buffers keep
// their contents past it as the device path does, and synchronises.
struct SlotArray {
    void *dst;
    const void *src;
    size_t slot_bytes;
};
int copy_back_written(fd_ctx *c, const int32_t *counts, int batch, int32_t stride, const std::vector<SlotArray> &arrays);

// The arrays of one keypoint-stage call, host or device (io_on_device). Device-side: in / out / out_slots hand
// the caller's pointer on and finish does nothing, so the call touches no staging buffer and enqueues its
// kernels and memsets only. Host-side: every non-null array takes the next buffer of fd_ctx::staging (so an
// output never shares its input's, even where the host pointers are equal), inputs (and `preload`ed outputs)
// are uploaded on the stream, and finish copies the outputs back (`out` arrays whole, `out_slots` arrays by
// copy_back_written) and synchronises, once. A null pointer stays null; n == 0 stages without a copy.
// That sync is why an entry point calls refuse_sync_under_capture before it builds one.
class HostIo {
  public:
    // first: the staging buffer the call's arrays start at (a call whose inputs and outputs are on different
    // sides builds one HostIo per side, the second past the first's arrays)
    HostIo(fd_ctx *c, int io_on_device, int first = 0) : c_(c), dev_(io_on_device != 0), used_(first) {}
    template <typename T>
    hipError_t in(const T *p, size_t n, const T *&dev) {
        void *d = nullptr;
        const hipError_t e = stage(p, sizeof(T) * n, true, d);
        dev = static_cast<const T *>(d);
        return e;
    }
    template <typename T>
    hipError_t out(T *p, size_t n, T *&dev) {
        return out_array(p, sizeof(T) * n, 0, false, dev);
    }
    // a [batch][stride] output of `per_slot` elements per slot, `slots` = batch * stride
    template <typename T>
    hipError_t out_slots(T *p, size_t slots, size_t per_slot, T *&dev, bool preload = false) {
        return out_array(p, sizeof(T) * per_slot * slots, sizeof(T) * per_slot, preload, dev);
    }
    // counts: the call's host counts (the written prefix of every out_slots array)
    int finish(const int32_t *counts, int batch, int32_t stride);

  private:
    hipError_t stage(const void *p, size_t bytes, bool upload, void *&dev);
    template <typename T>
    hipError_t out_array(T *p, size_t bytes, size_t slot_bytes, bool preload, T *&dev) {
        void *d = nullptr;
        const hipError_t e = stage(p, bytes, preload, d);
        dev = static_cast<T *>(d);
        if (e == hipSuccess && p && !dev_) (slot_bytes ? slots_ : whole_).push_back({p, d, slot_bytes ? slot_bytes : bytes});
        return e;
    }
    fd_ctx *c_;
    bool dev_;
    int used_;
    std::vector<SlotArray> whole_, slots_;  // host-side outputs: {host, staged, bytes (whole_) or bytes per slot (slots_)}
};

// A call without slots (stride 0) launches nothing and writes its per-frame outputs on the side io_on_device
// names: every byte of `out` set (0: zeros of any type; 0xFF: int32 -1), or `in` copied unless it is `out`
// itself. A null `out` is skipped.
int set_output(fd_ctx *c, void *out, int byte, size_t bytes, int io_on_device);
int copy_output(fd_ctx *c, void *out, const void *in, size_t bytes, int io_on_device);
// Every frame's count is 0.
int zero_counts(fd_ctx *c, int32_t *out_counts, int batch, int io_on_device);
// n camera values (fx, fy, cx, cy per camera) into out: all finite, fx and fy non-zero.
int check_camera(fd_ctx *c, const double *cam, int n, double *out);

// k_flow_finish after zeroing its counts (fd_flow_lk, fd_points_refine).
int finish_counts(fd_ctx *c, const fdk::FlowFinishArgs &fin);

// fd_blur_opts as fd_frames_blur checks them, into the kernel's radius, step and taps (fd_rt_blur.cpp).
int blur_options(fd_ctx *c, const fd_blur_opts &o, fdk::BlurArgs &a);

// Host threads of the line stage and the PNG decoder (OMP_NUM_THREADS caps, FD_LINE_THREADS overrides).
int default_line_threads();

struct SelectBufs {
    uint32_t *hist0, *list_count, *pre_count, *seg_bad, *wide_count, *wide_cut, *skipped;
    uint64_t *pre_keys, *wide_keys;
    uint32_t *status, *cand_n;
};

// Candidate lists, the (self-resetting) control block and the status words for `batch` frames.
int select_buffers(fd_ctx *c, int batch, int64_t cap, SelectBufs &sb);
// The list fields of a candidate kernel's argument block (the key map goes into the same object, key_map):
// the caller's arrays (fd_points_response), or the context's lists and the level-0 histogram of `sb`.
inline void list_outputs(fdk::CandList &l, float *resp, uint32_t *idx, int64_t cap, uint32_t *count, uint32_t *hist0) {
    l.resp = resp;
    l.idx = idx;
    l.cap = cap;
    l.count = count;
    l.hist0 = hist0;
}
inline void list_outputs(fd_ctx *c, fdk::CandList &l, int64_t cap, const SelectBufs &sb) {
    list_outputs(l, as<float>(c->list_resp), as<uint32_t>(c->list_idx), cap, sb.list_count, sb.hist0);
}
// Scratch of k_select_reference for `batch` frames of lists of `cap` entries.
int ref_buffers(fd_ctx *c, int batch, int rows, int cols, int64_t cap, fdk::RefSortArgs &r);

uint32_t host_float_key(float f);
// Key map of the selection (SelectArgs::key_base / key_lz): candidates have responses in
// (thr, rmax], rmax = +inf for the corner detectors and 16 + the largest FAST offset (+1) for FAST.
void key_map(int kind, float thr, const fdk::FastOffsets *off, int64_t n_off, uint32_t &base, int &lz);

// Inputs of the selection stage (K4) after a candidate kernel filled the lists of a SelectBufs.
struct SelectCall {
    int batch, rows, cols, dist;
    uint32_t need;
    int64_t cap;
    uint32_t key_base;
    int key_lz;
    int tie_idx_desc = 0;  // equal responses: raster index descending (SuperPoint multimap) instead of ascending
    bool wide_eager = false;  // FAST: the wide pass comes with the first chunk (SelectArgs::wide_eager)
    bool value_flag = false;  // the candidate kernel flags out-of-range values in pre_count (gather kernel off)
    const uint2 *segdesc = nullptr;  // sorted segments of the candidate kernel (PointsArgs::segdesc)
    const uint64_t *seghead = nullptr;
    int nseg = 0;
    bool push_order = false;  // lists hold the caller's push order (fd_points_select), not raster order
    bool dup_keys = false;    // a pixel may be listed twice with one response (caller lists): equal keys
    bool grid_at_d0 = false;  // distance 0 tests the grid too (1-pixel cells; set with push_order)
    // FAST emission cut (PointsArgs::emit_cut): the per-pixel launch of this call (re-run for the frames
    // the selection flags, kFrameRedo), its offsets, the skipped counters and the cut words
    const fdk::PointsArgs *redo_points = nullptr;
    const fdk::FastOffsets *redo_off = nullptr;
    uint32_t *skipped = nullptr;
    const uint32_t *cut_cur = nullptr;
    uint32_t *cut_next = nullptr;
    const char *value_msg = "a value above the declared maximum (fd_nn_opts::max_response)";
    SelectCall(int batch_, int rows_, int cols_, int dist_, uint32_t need_, int64_t cap_, uint32_t key_base_, int key_lz_)
        : batch(batch_), rows(rows_), cols(cols_), dist(dist_), need(need_), cap(cap_), key_base(key_base_),
          key_lz(key_lz_) {}
};

// The error a frame's status word read back on the host stands for: FD_FRAME_VALUE_RANGE (reported with
// `value_msg`; nullptr: not checked) or a tripped consistency guard; FD_OK otherwise.
int frame_status_error(fd_ctx *c, uint32_t status, int frame, const char *value_msg);

// K4 (k_gather + k_select) on the candidate lists, features into out_xy / out_counts (device, or copied
// back to the host and checked when !outputs_on_device).
int run_select(fd_ctx *c, const SelectCall &q, const PriorInfo &pi, const SelectBufs &sb, float *out_xy,
               int32_t out_stride, int32_t *out_counts, int outputs_on_device, int frames_on_device);

// Everything fd_points_detect allocates for a shape, whatever its options: the candidate lists of
// `list_cap` entries per frame and the selection's buffers (`sb`), the segment lists, FAST's run table,
// cut words and (with priors) mask-scan tables, the prior buffers for up to `max_prior_total` priors, and
// the reference tie order's scratch when the context has that order. fd_ctx_reserve calls it ahead of a
// graph capture; fd_points_detect calls it and takes pointers.
int detect_workspace(fd_ctx *c, int kind, int batch, int rows, int cols, int64_t max_prior_total, int64_t &list_cap,
                     SelectBufs &sb);
// Cached FAST offset table of the context (c->off) for n candidates-region pixels and a threshold.
int build_offsets(fd_ctx *c, int64_t n, float thr);

}  // namespace fdrt
