/*
 * fd_hip.h -- C ABI of the MI355X feature-detection hot path (libfdhip.so).
 *
 * Plain C, no HIP/torch types: pointers, sizes and status codes only. A context owns one HIP stream
 * (or borrows the caller's) and all device workspace; calls on different contexts may run
 * concurrently from different host threads (one context per GPU is the multi-GPU model).
 *
 * Each entry point names the reference interface it replaces (paths relative to
 * Horizon1026/Feature_Detector/src/). The reference has no FFI of its own: its seams are the C++
 * virtual FeaturePointDetector::ComputeCandidates (feature_point_detector.h:44, called at
 * feature_point_detector.cpp:20), the whole DetectGoodFeatures (feature_point_detector.h:29), and the
 * private FeatureLineDetector::ComputeLineLevelAngleMap (feature_line_detector.h:66, called at
 * feature_line_detector.cpp:22). The C++ drop-in classes in include/feature_detector/ call these.
 *
 * Conventions: every function returns FD_OK (0) or an FD_ERR_* code; fd_last_error() describes the
 * last failure on that context. Pointers flagged "*_on_device" are HIP device pointers on the
 * context's device, otherwise host pointers. Device-pointer calls are asynchronous on the context
 * stream; host-pointer outputs are complete when the call returns.
 */
#ifndef FD_HIP_H_
#define FD_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FD_OK 0
#define FD_ERR_INVALID 1  /* bad argument */
#define FD_ERR_HIP 2      /* HIP runtime error (allocation, launch, copy) */
#define FD_ERR_CAPACITY 3 /* an output capacity was too small; counts still report true sizes */

typedef struct fd_ctx fd_ctx;

/* Detector kinds: FeaturePointHarrisDetector (feature_point_harris_detector.h:9),
 * FeaturePointShiTomasDetector (feature_point_shi_tomas_detector.h:9),
 * FeaturePointFastDetector (feature_point_fast_detector.h:9). */
enum fd_point_kind { FD_HARRIS = 0, FD_SHI_TOMASI = 1, FD_FAST = 2 };

/* FeaturePointDetector::Options (feature_point_detector.h:15-20) fields used on the hot path.
 * The SubOptions of the reference are private constants and fixed here: Harris kAlpha = 0.04 and
 * kHalfPatchSize = 1 (feature_point_harris_detector.h:12-15), Shi-Tomasi kHalfPatchSize = 1
 * (feature_point_shi_tomas_detector.h:12-14), FAST kN = 12 and kMinPixelDiffValue = 15
 * (feature_point_fast_detector.h:12-15). */
typedef struct fd_point_opts {
    int32_t min_feature_distance; /* kMinFeatureDistance, default 15 */
    float min_valid_response;     /* kMinValidResponse,  default 0.1 */
} fd_point_opts;

/* ---- context ---------------------------------------------------------------------------------- */
int fd_ctx_create(int device, fd_ctx **out);
void fd_ctx_destroy(fd_ctx *ctx);
const char *fd_last_error(const fd_ctx *ctx);
/* Run on the caller's hipStream_t from now on (NULL = the HIP null stream, e.g. PyTorch's default
 * stream). A new context runs on a non-blocking stream of its own; fd_ctx_use_own_stream restores it. */
int fd_ctx_set_stream(fd_ctx *ctx, void *hip_stream);
int fd_ctx_use_own_stream(fd_ctx *ctx);
void *fd_ctx_get_stream(const fd_ctx *ctx);
int fd_ctx_synchronize(fd_ctx *ctx);
/* Pre-size device workspace for a (kind, batch, rows, cols) shape so that later calls of that shape
 * allocate nothing (required before hipGraph capture of fd_points_detect). Not covered: the global
 * occupancy grid of very small min_feature_distance (cells > 16384 per frame, e.g. 640x480 with d <= 4)
 * -- run one call of the shape before capturing. A call that would grow the workspace while its
 * stream is being captured fails (FD_ERR_HIP, "stream capture") instead of allocating. */
int fd_ctx_reserve(fd_ctx *ctx, int kind, int batch, int rows, int cols, int64_t max_prior_total);
/*
 * Order of equal responses in the selection (SelectGoodFeatures, feature_point_detector.cpp:58-60 sorts
 * with an unstable std::sort, so equal responses have no defined order):
 *   FD_TIES_RASTER     (default) response descending, equal responses by raster index ascending: a
 *                      total order, fully asynchronous and graph-capturable.
 *   FD_TIES_REFERENCE  the reference's own permutation: every frame whose greedy scan meets two equal
 *                      responses (FD_FRAME_TIES) is re-selected, on the GPU, in the order libstdc++'s
 *                      (GCC 11) std::sort leaves the raster-ordered candidates in (its introsort is
 *                      emulated over the visited prefix; FD_FRAME_RESOLVED). Frames without such a tie
 *                      are identical in both modes. Asynchronous and graph-capturable (reserve first,
 *                      fd_ctx_reserve after fd_ctx_set_tie_order). The depth limit's heapsort is emulated
 *                      too. A frame that breaks one of the emulation's capacity guards or its loop bound
 *                      gets FD_FRAME_UNRESOLVED instead: host-output calls then resolve it on the host;
 *                      device-output calls return k_select's raster-order features for it (if no window
 *                      of the reference order was scanned) or the features the reference order selected
 *                      before the stop (a prefix of the reference's result), with the flag in
 *                      fd_ctx_frame_status.
 * SuperPoint's fd_nn_select has a defined order (std::multimap) and ignores this setting.
 */
enum fd_tie_order { FD_TIES_RASTER = 0, FD_TIES_REFERENCE = 1 };
int fd_ctx_set_tie_order(fd_ctx *ctx, int order);

/*
 * Per-frame status words of the last selection call on this context (fd_points_detect, fd_nn_select):
 * FD_FRAME_* bits. Copies `batch` words to dst on the context stream (dst: device or host memory);
 * with async = 0 the call waits for the copy. Device-output calls return plain counts and leave their
 * flags here, so a caller can check them without a host round trip per call.
 */
#define FD_FRAME_TIES 0x00000001u       /* equal responses met in the greedy scan (order defined by the mode) */
#define FD_FRAME_RESOLVED 0x00000002u   /* re-selected in the reference's std::sort order (FD_TIES_REFERENCE) */
#define FD_FRAME_UNRESOLVED 0x00000004u /* FD_TIES_REFERENCE: the GPU emulation stopped (see fd_tie_order) */
#define FD_FRAME_REDETECTED 0x00000008u /* FAST, FD_TIES_RASTER: detected and selected a second time in the same call,
                                           without the adaptive emission cut (it was too high for this frame) */
#define FD_FRAME_VALUE_RANGE 0x40000000u /* fd_nn_select: a heatmap value above fd_nn_opts::max_response */
#define FD_FRAME_GUARD 0xBE000000u      /* internal consistency guard tripped (host-output calls fail FD_ERR_HIP) */
int fd_ctx_frame_status(fd_ctx *ctx, uint32_t *dst, int batch, int async);

/* Copy `bytes` of host memory into the context's frame staging buffer; *device_out receives its device
 * address, valid until the next call that stages frames on this context. Lets a caller run several
 * entry points on one upload (frames_on_device = 1). Synchronous. */
int fd_ctx_stage(fd_ctx *ctx, const void *host, int64_t bytes, const uint8_t **device_out);

/* ---- corner / FAST points ----------------------------------------------------------------------- */
/*
 * fd_points_detect -- FeaturePointDetector::DetectGoodFeatures (feature_point_detector.cpp:7-25) on a
 * batch of independent frames: mask from prior features (:12-16, :90-98), candidates
 * (ComputeCandidates: Harris feature_point_harris_detector.cpp:5-137, Shi-Tomasi
 * feature_point_shi_tomas_detector.cpp:5-137, FAST feature_point_fast_detector.cpp:11-98), sort by
 * response and greedy min-distance selection (SelectGoodFeatures :54-88).
 *
 *   frames        batch * rows * cols u8, row-major, frame-contiguous (GrayImage layout)
 *   prior_xy      all frames' incoming `features` (x, y float pairs) concatenated, or NULL
 *   prior_counts  batch entries (number of prior features of each frame), or NULL
 *   need          needed_feature_num (counts the prior features, checked after each append, :67-69)
 *   out_xy        batch * out_stride (x, y) float pairs: the NEW features of each frame, in order
 *   out_counts    batch int32: number of new features per frame (plain counts; per-frame flags are
 *                 in fd_ctx_frame_status)
 * Candidate order: response descending; equal responses as fd_ctx_set_tie_order says (default raster
 * index ascending; FD_TIES_REFERENCE = the reference's std::sort permutation, DESIGN.md "Tie order").
 * out_stride must be >= min(need, candidates) + 1.
 */
int fd_points_detect(fd_ctx *ctx, int kind, const uint8_t *frames, int frames_on_device, int batch, int rows,
                     int cols, const fd_point_opts *opts, const float *prior_xy, const int32_t *prior_counts,
                     uint32_t need, float *out_xy, int32_t out_stride, int32_t *out_counts, int outputs_on_device);

/*
 * fd_points_candidates -- the ComputeCandidates seam (feature_point_detector.h:44): per frame, the
 * candidates in the order the reference pushes them (raster order), as (response, x, y). Mask rules
 * as above. Writes at most cand_cap per frame at [b * cand_cap]; out_counts (int64) gets the true
 * count (FD_ERR_CAPACITY if any exceeds cand_cap). Optionally also returns the response map
 * (batch * rows * cols float, 0 where not stored; NULL to skip) -- Harris/Shi-Tomasi responses_
 * (feature_point_harris_detector.cpp:74-75,100-102); for FAST the map holds score + offset of every
 * candidate pixel and 0 elsewhere.
 */
int fd_points_candidates(fd_ctx *ctx, int kind, const uint8_t *frames, int frames_on_device, int batch, int rows,
                         int cols, const fd_point_opts *opts, const float *prior_xy, const int32_t *prior_counts,
                         float *out_resp, int32_t *out_x, int32_t *out_y, int64_t cand_cap, int64_t *out_counts,
                         float *out_response_map, int outputs_on_device);

/*
 * fd_points_select -- SelectGoodFeatures (feature_point_detector.cpp:54-88) over caller-supplied
 * candidates: the ComputeCandidates seam (feature_point_detector.h:44, called at
 * feature_point_detector.cpp:20) for a FeaturePointDetector subclass whose candidates come from
 * elsewhere. Frame b's candidates are (cand_resp, cand_x, cand_y)[b * cand_cap + i], i < cand_counts[b],
 * in the order ComputeCandidates pushed them; fd_points_candidates' outputs can be passed as they are.
 * Mask from the prior features as fd_points_detect (:12-16, :90-98); then sort by response and greedy
 * min-distance scan (the reference's SelectGoodFeatures does not filter by min_valid_response, and
 * neither does this call). Equal responses as fd_ctx_set_tie_order says: FD_TIES_RASTER orders them
 * by raster index, FD_TIES_REFERENCE by libstdc++'s std::sort of the pushed order. A pixel may be
 * listed more than once. Every candidate must lie in the frame and have a non-NaN response
 * (host outputs: FD_ERR_INVALID; device outputs: FD_FRAME_VALUE_RANGE in fd_ctx_frame_status).
 * cand_* and cand_counts are device pointers when cands_on_device, host pointers otherwise;
 * out_xy / out_counts as fd_points_detect.
 */
int fd_points_select(fd_ctx *ctx, int batch, int rows, int cols, const fd_point_opts *opts, const float *cand_resp,
                     const int32_t *cand_x, const int32_t *cand_y, const int64_t *cand_counts, int64_t cand_cap,
                     int cands_on_device, const float *prior_xy, const int32_t *prior_counts, uint32_t need,
                     float *out_xy, int32_t out_stride, int32_t *out_counts, int outputs_on_device);

/*
 * fd_points_response -- the per-pixel stage alone (response + NMS for Harris/Shi-Tomasi, segment test
 * + offset for FAST), i.e. ComputeCandidates without ordering: per frame, the candidates' responses
 * at out_resp[b * cand_cap] and raster indices (row * cols + col) at out_idx[b * cand_cap], in
 * unspecified order, and their count in out_counts[b]. Device pointers only (frames and outputs).
 * Used to time the hot kernel alone and by callers that select features themselves.
 */
int fd_points_response(fd_ctx *ctx, int kind, const uint8_t *frames, int batch, int rows, int cols,
                       const fd_point_opts *opts, float *out_resp, uint32_t *out_idx, int64_t cand_cap,
                       uint32_t *out_counts);

/*
 * fd_points_response_append -- fd_points_response without resetting out_counts: each frame's
 * candidates are appended after the out_counts[b] entries already there (slots past cand_cap are
 * counted but not written). A launch is then the corner/segment-test kernel alone, so a caller can
 * issue many back to back (or capture them in a HIP graph) to time the kernel by itself.
 */
int fd_points_response_append(fd_ctx *ctx, int kind, const uint8_t *frames, int batch, int rows, int cols,
                              const fd_point_opts *opts, float *out_resp, uint32_t *out_idx, int64_t cand_cap,
                              uint32_t *out_counts);

/* ---- LSD level-line map ------------------------------------------------------------------------ */
/*
 * fd_lsd_map -- FeatureLineDetector::ComputeLineLevelAngleMap (feature_line_detector.cpp:56-97).
 * Maps are (rows-1) x (cols-1) per frame, row-major, computed for row in [1, rows-3] and col in
 * [1, cols-3] and 0 elsewhere:
 *   norm   gradient_norm (:82)          (float, NULL to skip)
 *   angle  line_level_angle (:85)       (float, 0 where not valid; NULL to skip)
 *   valid  is_valid = norm > min_norm   (u8, NULL to skip)
 * valid_idx receives, per frame at [b * idx_cap], the row-major map index (row * (cols-1) + col) of
 * every valid pixel in the reference's scan order (column outer, row inner, :71-72, :86), i.e.
 * sorted_pixels_ before its std::sort (:92). valid_counts (int64) gets the true counts.
 */
int fd_lsd_map(fd_ctx *ctx, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols, float min_norm,
               float *norm, float *angle, uint8_t *valid, int32_t *valid_idx, int64_t idx_cap, int64_t *valid_counts,
               int outputs_on_device);

/*
 * fd_lsd_map_pitched -- fd_lsd_map with dense maps of row pitch map_pitch entries (>= cols-1): row r of
 * frame b's maps starts at entry (b * (rows-1) + r) * map_pitch of norm / angle / valid (entries past
 * cols-2 in a row are left untouched, except that frames too small to scan -- rows or cols < 4 -- get
 * their maps cleared whole). The map indices in valid_idx stay row * (cols-1) + col. With a
 * pitch that is a multiple of 16 entries every map row starts 64-byte (f32) / 16-byte (u8) aligned and
 * the map kernel's row stores are aligned (the faster layout for device outputs; host outputs are
 * always computed that way and copied to the caller's pitch). fd_lsd_map = map_pitch cols-1.
 */
int fd_lsd_map_pitched(fd_ctx *ctx, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                       float min_norm, float *norm, float *angle, uint8_t *valid, int64_t map_pitch, int32_t *valid_idx,
                       int64_t idx_cap, int64_t *valid_counts, int outputs_on_device);

/* ---- LSD line segments (level-line map on the GPU, region growing on host threads) --------------- */
/* FeatureLineDetector::Options (feature_line_detector.h:40-45). */
typedef struct fd_lsd_opts {
    float min_valid_gradient_norm;         /* kMinValidGradientNorm (20) */
    float min_tolerance_angle_residual_rad; /* kMinToleranceAngleResidualInRad (22.5 deg as float) */
    float min_valid_line_length;           /* kMinValidLineLengthInPixel (20) */
    float max_tolerance_inlier_ratio;      /* kMaxToleranceInlierRation (0.6) */
} fd_lsd_opts;

/* FeatureLineDetector::RectangleParam (feature_line_detector.h:29-38) of an accepted segment, as the
 * reference leaves it in rectangles_ (start/end offset by +0.5, feature_line_detector.cpp:43-44). */
typedef struct fd_lsd_rect {
    float start[2], end[2], center[2]; /* (x, y) */
    float length, width, angle;
    float dir[2];
    float inlier_ratio;
} fd_lsd_rect;

/*
 * fd_lsd_lines -- FeatureLineDetector::DetectGoodFeatures (feature_line_detector.cpp:12-54) for a
 * batch of frames. The level-line map runs on the GPU in compact mode (no dense maps: per valid pixel
 * its map index, norm and angle in scan order, bit-exact to fd_lsd_map); the lists come back over PCIe
 * once and region growing + rectangle fitting (:99-228) run per frame on `threads` host threads
 * (<= 0: all hardware threads). Segment k of frame b is out_rects[b * rect_stride + k]; its endpoints
 * are the reference's features[k] = (start.x, start.y, end.x, end.y). out_counts[b] = segments found
 * (may exceed rect_stride: only rect_stride are written; FD_ERR_CAPACITY is not raised for lines).
 * needed == 0 returns FD_OK with counts 0 and no work (:15). frames may be host or device memory.
 * Unpinned semantics of the un-vendored Slam_Utility (CircularBuffer overflow, AngleDiffInRad): DESIGN.md.
 */
int fd_lsd_lines(fd_ctx *ctx, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                 const fd_lsd_opts *opts, uint32_t needed, fd_lsd_rect *out_rects, int32_t rect_stride,
                 int32_t *out_counts, int threads);

/*
 * fd_lsd_lines_state -- the last fd_lsd_lines call's frame 0 as the reference leaves its members
 * (pixels_ / sorted_pixels_, feature_line_detector.h:74-75): the valid pixels in scan order (map index,
 * norm, angle) and each one's final is_used flag. n receives the count; at most cap are written.
 */
int fd_lsd_lines_state(fd_ctx *ctx, int32_t *idx, float *norm, float *angle, uint8_t *used, int64_t cap, int64_t *n);

/* ---- ingest front end: PNG frames ----------------------------------------------------------------- */
/*
 * The reference loads frames with Visualizor2D::LoadImage (test/test_feature_point_detector.cpp:104,
 * un-vendored). PNG files with 8-bit samples, colour type gray / gray+alpha / RGB / RGBA, no interlace.
 * Colour becomes gray as (4899 R + 9617 G + 1868 B + 8192) >> 14 (BT.601; the reference's conversion
 * is parity-unpinned); alpha is dropped. Errors: FD_ERR_INVALID (not a PNG, corrupt or
 * unsupported variant), FD_ERR_CAPACITY (output too small).
 *
 * fd_png_info   -- geometry of one PNG (no context, no GPU).
 * fd_png_decode -- one PNG to a host gray image (host decode; the C++ loader uses it).
 * fd_png_frames -- a batch of same-size PNGs to device gray frames [n][rows][cols] (the layout
 *                  fd_points_detect / fd_lsd_lines take): zlib inflate + PNG row filters on `threads`
 *                  host threads (<= 0: all, capped by OMP_NUM_THREADS) into pinned memory, one H2D copy,
 *                  colour -> gray on the GPU, stream-ordered on the context stream.
 */
int fd_png_info(const uint8_t *png, size_t len, int32_t *rows, int32_t *cols, int32_t *channels);
int fd_png_decode(const uint8_t *png, size_t len, uint8_t *out_gray, size_t cap, int32_t *rows, int32_t *cols);
int fd_png_frames(fd_ctx *ctx, const uint8_t *const *pngs, const size_t *lens, int n, int rows, int cols,
                  uint8_t *frames_device, int threads);

/* ---- steered BRIEF descriptor ------------------------------------------------------------------- */
/* BriefDescriptor::Options (descriptor_brief.h:17-20) plus the float-coordinate sampler of the
 * un-vendored GrayImage (descriptor_brief.cpp:24,42-43; see DESIGN.md: parity unpinned). */
enum fd_sampler { FD_SAMPLE_BILINEAR = 0, FD_SAMPLE_TRUNCATE = 1 };
typedef struct fd_brief_opts {
    int32_t length;          /* kLength, bits per descriptor, 1..256 (default 256) */
    int32_t half_patch_size; /* kHalfPatchSize, moment patch half size, 0..255 (default 8) */
    int32_t sampler;         /* enum fd_sampler */
} fd_brief_opts;

/*
 * fd_brief_compute -- Descriptor<BriefType>::Compute (descriptor.h:27-40) with
 * BriefDescriptor::ComputeForOneFeature (descriptor_brief.cpp:8-50) per keypoint, for a batch of frames.
 * uv: [batch][stride][2] float (x = col, y = row), the layout fd_points_detect writes, so a device-side
 * detect -> describe chain needs no host round trip. counts: keypoints per frame (int32 [batch]; NULL =
 * stride each; bits 25..31 are ignored, so fd_points_detect's device counts can be passed as they are).
 * out_bits: [batch][stride][ceil(length/32)] uint32, descriptor bit i = bit (i % 32) of word i / 32
 * (bit i set <=> I(p1_i) < I(p2_i), descriptor_brief.cpp:44-46); keypoints outside the border
 * (:13-17) or with zero moment (:30) get all-zero words and out_valid 0 (NULL to skip out_valid).
 * Slots k >= counts[b] are not written. uv, counts, out_bits and out_valid are all device pointers
 * when io_on_device, all host pointers otherwise.
 */
int fd_brief_compute(fd_ctx *ctx, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                     const fd_brief_opts *opts, const float *uv, const int32_t *counts, int32_t stride,
                     uint32_t *out_bits, uint8_t *out_valid, int io_on_device);

/* ---- Hamming matcher for BRIEF descriptors (MI355X extension: the reference has no matcher) -------- */
typedef struct fd_match_opts {
    int32_t length;       /* bits per descriptor, 1..256 (fd_brief_opts::length); words = ceil(length/32) */
    int32_t max_distance; /* reject a best match with distance > max_distance; < 0: no bound */
    float   max_ratio;    /* ratio test: accept only if (float)d1 < max_ratio * (float)d2; <= 0: off */
    int32_t cross_check;  /* 1: accept q -> t only if t's best query is q */
} fd_match_opts;

/*
 * fd_brief_match -- nearest neighbour in Hamming distance of every query descriptor among the train
 * descriptors, frame b of the query set against frame b of the train set. Layouts are what
 * fd_brief_compute writes: *_bits [batch][stride][ceil(length/32)] uint32, *_valid [batch][stride]
 * (NULL = all valid), *_counts int32 [batch] (NULL = stride each; bits 25..31 are ignored, so
 * fd_points_detect's device counts can be passed as they are). Matching frame i of one batch against
 * its frame i + 1 is the same call with the train pointers advanced by one frame and batch - 1.
 * Distance: popcount of the xor over bits 0..length-1; the bits above `length` in the last word are
 * masked here, on both sides. An invalid train descriptor is never a candidate; an invalid query gets
 * out_idx -1 and both distances -1 (invalid descriptors are all-zero words and would otherwise match
 * each other at distance 0).
 * out_dist [batch][q_stride][2] (NULL to skip): [0] the smallest distance to a valid train descriptor,
 * [1] the smallest distance to a valid train descriptor with another index than the best one (equal to
 * [0] on a tie); -1 when absent (no valid train descriptor, or only one). Both are raw values, written
 * whether or not the match is accepted. Equal distances go to the lowest train index (what a serial
 * scan with `<` gives).
 * out_idx [batch][q_stride]: the best train index if it passes every enabled test, else -1. Tests:
 * max_distance (rejects d1 > max_distance); the ratio test, one float multiply and one compare
 * ((float)d1 < max_ratio * (float)d2, skipped when d2 is absent); cross_check (the train descriptor's
 * best query -- over the frame's valid queries, smallest distance, lowest query index on ties,
 * independent of the other two tests -- must be this query).
 * out_counts [batch] (NULL to skip): accepted matches among slots < q_counts[b]. Slots >= q_counts[b]
 * of out_idx and out_dist are not written. q_stride 0: nothing but out_counts = 0; t_stride 0: as all
 * train counts 0.
 * All pointers are device pointers when io_on_device: the call is then asynchronous on the context's
 * stream, and graph-capturable once a first call of the shape has sized the workspace (the
 * cross-check's reverse table; growing it under capture fails). Host pointers otherwise: staged
 * through context buffers, complete on return.
 * FD_ERR_INVALID: ctx / opts / q_bits / t_bits / out_idx NULL, length outside 1..256, a negative
 * stride, batch < 1, a non-finite max_ratio.
 */
int fd_brief_match(fd_ctx *ctx, int batch, const fd_match_opts *opts,
                   const uint32_t *q_bits, const uint8_t *q_valid, const int32_t *q_counts, int32_t q_stride,
                   const uint32_t *t_bits, const uint8_t *t_valid, const int32_t *t_counts, int32_t t_stride,
                   int32_t *out_idx, int32_t *out_dist, int32_t *out_counts, int io_on_device);

/* ---- Squared-L2 matcher for NN float descriptors (MI355X extension: the reference has no matcher) --- */
typedef struct fd_nn_match_opts {
    int32_t dim;          /* floats per descriptor: a multiple of 4, 4..256 */
    float   max_distance; /* reject a best match with squared distance > max_distance; < 0: no bound */
    float   max_ratio;    /* accept only if d1 < (max_ratio * max_ratio) * d2 (squared distances); <= 0: off */
    int32_t cross_check;  /* 1: accept q -> t only if t's best query is q */
} fd_nn_match_opts;

/*
 * fd_nn_match -- nearest neighbour in squared L2 distance of every query descriptor among the train
 * descriptors, frame b of the query set against frame b of the train set: fd_brief_match's sibling for
 * the float descriptors of the SuperPoint / DISK path. *_desc is [batch][stride][dim] float, exactly as
 * fd_nn_descriptors and fd_nn_select_list write them (256 channels for SuperPoint, 128 for DISK);
 * *_valid [batch][stride] (NULL = all valid) and *_counts int32 [batch] (NULL = stride each; bits 25..31
 * are ignored) are as in fd_brief_match, and so is matching frame i of one batch against its frame
 * i + 1: the train pointers advanced by one frame, batch - 1.
 * Distance: squared L2 as this float sequence, bit for bit (no contraction, one rounding per step):
 *   dot(q, t): acc = 0; for k = 0 .. dim-1: acc = fmaf(q[k], t[k], acc)
 *   n(x) = dot(x, x), the same chain
 *   d = fmaxf(0.0f, (n(q) + n(t)) - 2.0f * dot(q, t))
 * d(q, t) has the same bits from either side (products and sums commute), so the cross-check below is
 * symmetric: "t's best query is q" is decided on the very distances of the forward search.
 * An invalid train descriptor is never a candidate; an invalid query gets out_idx -1 and both distances
 * -1. An all-zero descriptor is valid unless flagged (fd_nn_descriptors writes zeros for keypoints
 * outside the map: flag those). Equal distances go to the lowest train index (what a serial scan in
 * ascending index order with `<` gives); a NaN distance never wins a `<`. Inputs that are not finite, or
 * whose squared norm is not finite in float, are otherwise unspecified (such a descriptor may be
 * treated as invalid).
 * out_dist [batch][q_stride][2] float (NULL to skip): [0] the smallest distance to a valid train
 * descriptor, [1] the smallest distance to a valid train descriptor with another index than the best one
 * (equal to [0] on a tie); -1.0f when absent. Both are raw values, written whether or not the match is
 * accepted.
 * out_idx [batch][q_stride]: the best train index if it passes every enabled test, else -1. Tests:
 * max_distance (rejects d1 > max_distance); the ratio test, two float multiplies and one compare
 * (d1 < (max_ratio * max_ratio) * d2, skipped when d2 is absent); cross_check (the train descriptor's
 * best query -- over the frame's valid queries, the same distance sequence, lowest query index on ties,
 * independent of the other two tests -- must be this query).
 * out_counts [batch] (NULL to skip): accepted matches among slots < q_counts[b]. Slots >= q_counts[b]
 * of out_idx and out_dist are not written. q_stride 0: nothing but out_counts = 0; t_stride 0: as all
 * train counts 0.
 * All pointers are device pointers when io_on_device: the call is then asynchronous on the context's
 * stream, and graph-capturable once a first call of the shape has sized the workspace (the norms and
 * the cross-check's reverse table; growing them under capture fails). Host pointers otherwise: staged
 * through context buffers, complete on return.
 * FD_ERR_INVALID: ctx / opts / q_desc / t_desc / out_idx NULL, dim outside 4..256 or not a multiple of
 * 4, a negative stride, batch < 1, a non-finite max_ratio or max_distance.
 */
int fd_nn_match(fd_ctx *ctx, int batch, const fd_nn_match_opts *opts,
                const float *q_desc, const uint8_t *q_valid, const int32_t *q_counts, int32_t q_stride,
                const float *t_desc, const uint8_t *t_valid, const int32_t *t_counts, int32_t t_stride,
                int32_t *out_idx, float *out_dist, int32_t *out_counts, int io_on_device);

/* ---- Guided (position-gated) matching: a search window for both matchers (MI355X extension) --------- */
typedef struct fd_match_gate {
    float radius_x; /* half-width of the window in pixels: finite, >= 0 */
    float radius_y; /* half-height */
} fd_match_gate;

/*
 * fd_brief_match_guided / fd_nn_match_guided -- fd_brief_match / fd_nn_match with a search window, the
 * frame-to-frame tracker's form: a train keypoint is a candidate of a query only if it lies within a few
 * pixels of where the query is expected.
 * q_xy / t_xy: positions float [batch][stride][2], stored (x, y): what fd_points_detect / fd_nn_select
 * write, with the stride and slot order of that side's descriptor arrays. Query positions may be
 * predictions (the last position plus a motion model); they need not lie inside the frame or be integers.
 * The gate: train entry j is a candidate of query i iff both
 *   fabsf(t_xy[j].x - q_xy[i].x) <= gate->radius_x
 *   fabsf(t_xy[j].y - q_xy[i].y) <= gate->radius_y
 * hold, each one float subtraction (one rounding) and one inclusive compare. A NaN on either side makes a
 * compare false, so that pair is never a candidate (inf - inf is NaN and fails the same way).
 * fabsf(a - b) has the bits of fabsf(b - a): the gate is symmetric, so the cross-check stays decided on
 * the pairs of the forward search.
 * Everything the unguided entry defines over "valid train descriptors" is defined here over "valid train
 * descriptors inside this query's window", and nothing else changes: the best distance with the lowest
 * train index on ties; the second distance (the smallest distance to another candidate in the window; -1
 * when the window holds fewer than two, and the ratio test is then skipped); an empty window gives
 * out_idx -1 and both distances -1; the cross-check's reverse search takes a train entry's best query
 * over the valid queries whose window contains it, lowest query index on ties. The distance definition,
 * max_distance, the ratio formulas, out_counts, the unwritten slots >= q_counts[b], the ignored bits
 * 25..31 of counts, the zero-stride cases, host staging against device pointers and graph capture (once
 * a first call of the shape has sized the workspace) are those of the unguided entries. With finite
 * positions and both radii 3.0e38f every output equals the unguided call's.
 * FD_ERR_INVALID: whatever the unguided entry rejects; gate, q_xy or t_xy NULL; a radius that is
 * negative, NaN or infinite.
 */
int fd_brief_match_guided(fd_ctx *ctx, int batch, const fd_match_opts *opts, const fd_match_gate *gate,
                          const uint32_t *q_bits, const uint8_t *q_valid, const int32_t *q_counts, int32_t q_stride,
                          const float *q_xy,
                          const uint32_t *t_bits, const uint8_t *t_valid, const int32_t *t_counts, int32_t t_stride,
                          const float *t_xy,
                          int32_t *out_idx, int32_t *out_dist, int32_t *out_counts, int io_on_device);
int fd_nn_match_guided(fd_ctx *ctx, int batch, const fd_nn_match_opts *opts, const fd_match_gate *gate,
                       const float *q_desc, const uint8_t *q_valid, const int32_t *q_counts, int32_t q_stride,
                       const float *q_xy,
                       const float *t_desc, const uint8_t *t_valid, const int32_t *t_counts, int32_t t_stride,
                       const float *t_xy,
                       int32_t *out_idx, float *out_dist, int32_t *out_counts, int io_on_device);

/* ---- Model-gated matching: an epipolar or homography gate for both matchers (MI355X extension) ------- */
typedef struct fd_match_model_gate {
    int32_t model;      /* FD_RANSAC_FUNDAMENTAL (0) or FD_RANSAC_HOMOGRAPHY (1), defined with fd_ransac below */
    float   threshold;  /* pixels, finite, > 0 */
    float   radius_x, radius_y; /* fd_match_gate's window, applied as well; 3.0e38f leaves it open */
} fd_match_model_gate;

/*
 * fd_brief_match_model / fd_nn_match_model -- fd_brief_match_guided / fd_nn_match_guided with a second gate,
 * the two-view model of the frame: the second matching pass of a front end that has estimated F or H
 * (search by epipolar line, guided matching). A train keypoint is a candidate of a query only if the pair
 * agrees with the model, so matches come back that the ratio test and the cross-check rejected while the
 * whole frame competed.
 * model: double [batch][9], row-major 3 x 3 in pixel coordinates, one per frame: out_model of fd_ransac or
 * fd_ransac_refit as it is (a device pointer when io_on_device, so verify -> refit -> rematch needs no
 * synchronisation). q_xy / t_xy and every other argument are the guided entries'.
 *
 * The gate, a definite sequence: all of it double, every operation rounded once, no contraction. With
 * (x, y) = (double)q_xy[i], (u, v) = (double)t_xy[j], M the frame's nine doubles and t = (double)threshold,
 * train entry j is a candidate of query i iff the window test of fd_match_gate holds with radius_x / radius_y
 * (exactly as in the guided entries) and the model test holds:
 *   F:  l0 = (M0*x + M1*y) + M2;  l1 = (M3*x + M4*y) + M5;  l2 = (M6*x + M7*y) + M8
 *       m0 = (M0*u + M3*v) + M6;  m1 = (M1*u + M4*v) + M7
 *       e = (u*l0 + v*l1) + l2
 *       candidate iff e*e <= (t*t) * ((l0*l0 + l1*l1) + (m0*m0 + m1*m1))            (the Sampson test)
 *   H (query -> train, fd_ransac's direction):
 *       px = (M0*x + M1*y) + M2;  py = (M3*x + M4*y) + M5;  w = (M6*x + M7*y) + M8
 *       dx = px - u*w;  dy = py - v*w
 *       candidate iff dx*dx + dy*dy <= (t*t) * (w*w)                                 (the forward transfer test)
 * The grouping (l0*l0 + l1*l1) + (m0*m0 + m1*m1) lets each side's half be computed once per entry. It is
 * not fd_ransac's left-to-right sum, and the gate works on pixel coordinates where fd_ransac works on
 * conditioned ones: the gate is fd_ransac's inlier test mathematically, not bit for bit.
 * A NaN fails the compare, so a position or a model entry that is not finite yields no candidate (a frame
 * whose model holds a NaN matches nothing). A frame whose model is nine zeros ("no model", as fd_ransac
 * writes it) passes every pair of finite positions (0 <= 0): that frame falls back to the window alone, and
 * with both radii 3.0e38f to the unguided call.
 * The cross-check's reverse search evaluates the same expressions on the same operands: a pair is always
 * (query, train), whichever set is searched, so the gate has the same bits in both directions and the
 * cross-check stays decided on the pairs of the forward search. For H the reverse search therefore uses the
 * forward transfer predicate, not the inverse homography.
 * Everything else is the guided entries' contract over "valid train descriptors that pass the gate": the best
 * distance with the lowest train index on ties, the second distance (-1 with fewer than two candidates, and
 * the ratio test is then skipped), no candidate giving out_idx -1 and both distances -1, max_distance, the
 * ratio formulas, out_counts, the unwritten slots >= q_counts[b], the zero-stride cases, host staging against
 * device pointers, and graph capture once a first call of the shape has sized the workspace (the gate
 * vectors of both sets, 32 bytes per slot, beside the guided entries' workspace).
 * FD_ERR_INVALID: whatever the guided entry rejects (gate->radius_x / radius_y are its radii); model NULL;
 * gate->model outside {0, 1}; a threshold that is not finite or is <= 0.
 */
int fd_brief_match_model(fd_ctx *ctx, int batch, const fd_match_opts *opts, const fd_match_model_gate *gate,
                         const double *model,
                         const uint32_t *q_bits, const uint8_t *q_valid, const int32_t *q_counts, int32_t q_stride,
                         const float *q_xy,
                         const uint32_t *t_bits, const uint8_t *t_valid, const int32_t *t_counts, int32_t t_stride,
                         const float *t_xy,
                         int32_t *out_idx, int32_t *out_dist, int32_t *out_counts, int io_on_device);
int fd_nn_match_model(fd_ctx *ctx, int batch, const fd_nn_match_opts *opts, const fd_match_model_gate *gate,
                      const double *model,
                      const float *q_desc, const uint8_t *q_valid, const int32_t *q_counts, int32_t q_stride,
                      const float *q_xy,
                      const float *t_desc, const uint8_t *t_valid, const int32_t *t_counts, int32_t t_stride,
                      const float *t_xy,
                      int32_t *out_idx, float *out_dist, int32_t *out_counts, int io_on_device);

/* ---- Image pyramid and pyramidal Lucas-Kanade tracking (MI355X extension) --------------------------- */
#define FD_PYR_MAX_LEVELS 6

/*
 * fd_pyr_layout -- the packed pyramid of a batch: [level][batch][rows_l][cols_l] uint8 with
 * rows_l = rows >> l, cols_l = cols >> l, every level starting at a multiple of 256 bytes. offsets[l] is
 * the byte offset of level l (offsets[0] = 0) and offsets[levels] the size of the whole (the next multiple
 * of 256 after the last level). A host computation: no context, no GPU.
 * FD_ERR_INVALID: offsets NULL, batch < 1, levels outside 1..6, or a top level with a zero dimension.
 */
int fd_pyr_layout(int batch, int rows, int cols, int levels, int64_t *offsets /* [levels + 1] */);

/*
 * fd_pyr_build -- the box pyramid of a batch of frames [batch][rows][cols] into pyr (fd_pyr_layout).
 * Level 0 is a copy of the frames; pixel (y, x) of level l + 1 is
 *   (I(2y, 2x) + I(2y, 2x + 1) + I(2y + 1, 2x) + I(2y + 1, 2x + 1) + 2) >> 2
 * of level l (an odd last row or column is dropped). Padding bytes between levels are not written.
 * frames / pyr are device pointers when frames_on_device / pyr_on_device (pyr then 256-byte aligned, as
 * device allocations are); with both the call is copies and kernels on the context's stream only
 * (graph-capturable). A host pyr is built in the context's workspace and copied back, complete on return.
 * FD_ERR_INVALID: what fd_pyr_layout rejects; ctx, frames or pyr NULL; a misaligned device pyr.
 */
int fd_pyr_build(fd_ctx *ctx, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols, int levels,
                 uint8_t *pyr, int pyr_on_device);

typedef struct fd_flow_opts {
    int32_t half_window; /* r in 1..10: the window is (2r + 1)^2 = n pixels */
    int32_t max_iters;   /* 1..100 iterations per level */
    float epsilon;       /* > 0: a level stops after a step of length <= epsilon (level pixels) */
    float min_eigen;     /* >= 0: smallest accepted minimum eigenvalue of the window's mean gradient matrix,
                            central-difference gradients in intensity units per pixel (Gx, Gy are 32 times
                            those, hence the 1024 of the level test) */
    float fb_max_dist;   /* forward-backward check: largest round-trip distance in pixels; < 0: off */
    float max_error;     /* largest mean absolute residual (intensity units) of a track; < 0: off */
} fd_flow_opts;

/* out_status values of fd_flow_lk: 1 is the only "tracked" */
enum fd_flow_status {
    FD_FLOW_INVALID = 0,  /* valid flag 0 */
    FD_FLOW_TRACKED = 1,
    FD_FLOW_OUTSIDE = 2,  /* xy not finite or outside the frame, or the track left the frame */
    FD_FLOW_FLAT = 3,     /* the level-0 gradient matrix fails the level test */
    FD_FLOW_STEP = 4,     /* a non-finite step */
    FD_FLOW_FB = 5,       /* failed the forward-backward check */
    FD_FLOW_ERROR = 6     /* out_err above max_error */
};

/*
 * fd_flow_lk -- pyramidal Lucas-Kanade (inverse-compositional: the gradients come from the template
 * frame) for the features xy of every frame of a batch, from the pyramids of the previous and the next
 * frames (fd_pyr_build with the same batch, rows, cols, levels; device pointers always). The reference
 * has no tracker: the contract is this text, a definite arithmetic sequence in which every window sum is
 * an exact integer (any summation order gives it) and only the 2 x 2 solve is floating point.
 *
 * xy: float [batch][stride][2], stored (x, y): what fd_points_detect / fd_nn_select write. counts int32
 * [batch] (NULL: stride each; bits 25..31 ignored), valid uint8 [batch][stride] (NULL: all valid),
 * guess_xy as xy: the expected positions in the next frame (NULL: xy itself).
 *
 * Raw bilinear sum. For a float position (x, y) on a level image I (rows_l x cols_l) and integer offsets
 * (u, v): ix = (int)floorf(x), ax = x - floorf(x) (exact), qx = (int)(ax * 1024.0f) (truncated), y
 * likewise, and
 *   S(u, v) = (1024 - qx)(1024 - qy) I(cy(iy + v), cx(ix + u))     + qx (1024 - qy) I(cy(iy + v), cx(ix + u + 1))
 *           + (1024 - qx) qy         I(cy(iy + v + 1), cx(ix + u)) + qx qy          I(cy(iy + v + 1), cx(ix + u + 1))
 * with cx / cy clamping to [0, cols_l - 1] / [0, rows_l - 1]: no read is undefined. S < 2^28.
 *
 * Per feature slot below counts[b]:
 *   valid 0: status 0, out_xy = xy, out_err not written.
 *   xy not finite or outside [0, cols - 1] x [0, rows - 1]: status 2.
 *   L = levels - 1; in float d = (guess - xy) * 2^-L per axis (0 without a guess). For l = L .. 0:
 *   1. p = xy * 2^-l (exact; the quarter-pixel offset of the box pyramid is ignored, as OpenCV ignores its own).
 *   2. Template from the previous pyramid's level l at p, for u, v in [-r, r] (arithmetic shifts):
 *        Iq = (S(u, v) + 2^14) >> 15   (intensity * 32)
 *        Gx = (S(u + 1, v) - S(u - 1, v) + 2^15) >> 16,  Gy = (S(u, v + 1) - S(u, v - 1) + 2^15) >> 16
 *   3. A11 = sum Gx^2, A12 = sum Gx Gy, A22 = sum Gy^2: exact integers.
 *   4. Level test, in double, every operation rounded once, no contraction:
 *        tau = (double)min_eigen * 1024.0 * n; e11 = a11 - tau; e22 = a22 - tau; det = a11 * a22 - a12 * a12
 *        usable iff det > 0 && e11 > 0 && e22 > 0 && e11 * e22 - a12 * a12 >= 0
 *      (the minimum-eigenvalue test without a square root). An unusable level above 0 is skipped with d
 *      carried down; an unusable level 0 gives status 3.
 *   5. At most max_iters iterations: q = p + d (one float add per axis). In-frame test in level-0 units:
 *      0 <= q.x * 2^l <= (float)(cols - 1) and the same for y (false on NaN); failing it gives status 2 at
 *      any level. Jq = (S_next(u, v at q) + 2^14) >> 15 from the next pyramid's level l; D = Iq - Jq;
 *      b1 = sum D Gx, b2 = sum D Gy, E = sum |D| (exact integers). In double
 *        sx = (a22 * b1 - a12 * b2) / det,  sy = (a11 * b2 - a12 * b1) / det
 *      then in float fx = (float)sx, fy = (float)sy; a non-finite fx or fy gives status 4; d = d + (fx, fy);
 *      the level stops after the update when fx * fx + fy * fy <= epsilon * epsilon (float, every product
 *      rounded).
 *   6. If l > 0: d = d * 2.0f.
 *   out_xy = xy + d; out_err = (float)((double)E / (32.0 * n)) with the E of the last iteration at level 0.
 *   Running out of iterations is not a loss. max_error >= 0 && out_err > max_error: status 6.
 * Forward-backward check (fb_max_dist >= 0), for the slots still at status 1: a second pass tracks out_xy
 * from the next pyramid back into the previous one with the same options (max_error apart: it is not
 * applied to the way back) and xy as the guess. A lost backward track gives status 5, and so does
 * bx * bx + by * by > fb_max_dist * fb_max_dist with bx = back.x - xy.x, by = back.y - xy.y (float).
 *
 * Outputs: out_status uint8 (enum fd_flow_status; 1 = tracked, everything else lost), out_xy, out_err
 * (NULL to skip), out_counts [batch] (NULL to skip): the status-1 slots below counts[b]. A slot lost
 * inside the tracker (status 2, 3, 4) has out_xy = xy and out_err = -1; status 5 and 6 keep the forward
 * track's values. Slots >= counts[b] are not written. stride 0: nothing but out_counts = 0.
 * The feature arrays (xy, valid, counts, guess_xy and the outputs) are device pointers when io_on_device:
 * the call is then asynchronous on the context's stream, and graph-capturable once a first call of the
 * shape has sized the workspace (the backward pass's results; growing them under capture fails). Host
 * pointers otherwise: staged through context buffers, complete on return.
 * FD_ERR_INVALID: ctx, opts, a pyramid, xy, out_xy or out_status NULL; batch < 1; a negative stride; rows,
 * cols, levels that fd_pyr_layout rejects; an option outside its range above or not finite.
 */
int fd_flow_lk(fd_ctx *ctx, int batch, int rows, int cols, int levels, const fd_flow_opts *opts,
               const uint8_t *prev_pyr, const uint8_t *next_pyr,
               const float *xy, const uint8_t *valid, const int32_t *counts, int32_t stride, const float *guess_xy,
               float *out_xy, uint8_t *out_status, float *out_err, int32_t *out_counts, int io_on_device);

/* ---- Sub-pixel corner refinement (MI355X extension: the reference's detectors stop at integer pixels) -- */
typedef struct fd_refine_opts {
    int32_t half_window; /* r in 1..10: the window is (2r + 1)^2 pixels */
    int32_t max_iters;   /* 1..100 */
    float epsilon;       /* > 0: stop after a step of length <= epsilon (pixels) */
    float min_eigen;     /* >= 0: as fd_flow_opts.min_eigen, of the weighted mean gradient matrix */
    float max_shift;     /* > 0, finite: largest |refined - xy| per axis, in pixels */
} fd_refine_opts;

/* out_status values of fd_points_refine: 1 is the only "refined" */
enum fd_refine_status {
    FD_REFINE_INVALID = 0,  /* valid flag 0 */
    FD_REFINE_REFINED = 1,
    FD_REFINE_OUTSIDE = 2,  /* xy not finite or outside the frame, or the iteration left the frame */
    FD_REFINE_FLAT = 3,     /* the window's gradient matrix fails the level test */
    FD_REFINE_DIVERGED = 4  /* moved further than max_shift from xy, or a non-finite step */
};

/*
 * fd_points_refine -- the cornerSubPix step between detection and tracking: for every feature xy of every
 * frame of a batch, the point c whose offsets to the window's pixels are orthogonal to the gradients there
 * (c + G^-1 sum w g g^T p, iterated), on frames [batch][rows][cols] uint8. A device pyramid of fd_pyr_build
 * passes as frames as it is: its level 0 is at offset 0. Like fd_flow_lk the contract is this text, a definite
 * arithmetic sequence in which every window sum is an exact integer (any summation order gives it) and only
 * the 2 x 2 solve is floating point.
 *
 * xy, valid, counts, stride and io_on_device are fd_flow_lk's: xy float [batch][stride][2], stored (x, y);
 * counts int32 [batch] (NULL: stride each; bits 25..31 ignored, so fd_points_detect's counts pass as they
 * are); valid uint8 [batch][stride] (NULL: all valid). out_xy may be xy itself (in place): a slot reads its
 * position once and writes it once. S(u, v) is fd_flow_lk's raw bilinear sum on the frame (floor, the
 * fraction truncated to 1/1024, reads clamped to the frame's edge).
 *
 * Per feature slot below counts[b]:
 *   valid 0: status 0, out_xy = xy.
 *   xy not finite or outside [0, cols - 1] x [0, rows - 1]: status 2, out_xy = xy.
 *   c = xy (float). At most max_iters iterations:
 *   1. In-frame test: 0 <= c.x <= (float)(cols - 1) and 0 <= c.y <= (float)(rows - 1) (false on NaN);
 *      failing it gives status 2.
 *   2. Gradients at c, for integer offsets u, v in [-r, r] (arithmetic shifts):
 *        Gx = (S(u + 1, v) - S(u - 1, v) + 2^15) >> 16,  Gy = (S(u, v + 1) - S(u, v - 1) + 2^15) >> 16
 *      (32 times the central difference in intensity units per pixel; |G| <= 4080).
 *   3. With the integer weight w(u, v) = (r + 1 - |u|)(r + 1 - |v|) (a tent; sum w = (r + 1)^4):
 *        G11 = sum w Gx^2,  G12 = sum w Gx Gy,  G22 = sum w Gy^2
 *        B1 = sum w (Gx^2 u + Gx Gy v),  B2 = sum w (Gx Gy u + Gy^2 v)
 *      exact integers. A single term can pass 2^31 (r = 10: w |u| 2 4080^2 up to 1.1e10); the totals stay
 *      below 2^42, so their conversion to double is exact.
 *   4. Level test, in double, every operation rounded once, no contraction:
 *        tau = (double)min_eigen * 1024.0 * (double)((r + 1)^4)
 *        e11 = g11 - tau; e22 = g22 - tau; det = g11 * g22 - g12 * g12
 *        usable iff det > 0 && e11 > 0 && e22 > 0 && e11 * e22 - g12 * g12 >= 0
 *      (fd_flow_lk's step 4 on the weighted matrix). Not usable: status 3.
 *   5. In double sx = (g22 * b1 - g12 * b2) / det, sy = (g11 * b2 - g12 * b1) / det; in float fx = (float)sx,
 *      fy = (float)sy; c = c + (fx, fy), one float add per axis.
 *      !(fabsf(c.x - xy.x) <= max_shift && fabsf(c.y - xy.y) <= max_shift): status 4 (a non-finite step fails
 *      the test too). The loop stops after the update when fx * fx + fy * fy <= epsilon * epsilon (float,
 *      every product rounded).
 *   Running out of iterations is not a loss: status 1, out_xy = c (the in-frame test is step 1's alone: the
 *   last update is not followed by one, so a refined c may lie up to max_shift outside the frame).
 *   Status 2, 3 and 4 hand xy back, so out_xy is always a usable position array.
 *
 * Outputs: out_status uint8 (enum fd_refine_status), out_xy, out_counts [batch] (NULL to skip): the status-1
 * slots below counts[b]. Slots >= counts[b] are not written. stride 0: nothing but out_counts = 0.
 * frames is a device pointer when frames_on_device, else a host pointer staged through the context as
 * fd_pyr_build stages host frames. The feature arrays (xy, valid, counts and the outputs) are device
 * pointers when io_on_device. With device frames and device feature arrays the call is kernels on the
 * context's stream only: asynchronous and graph-capturable (no workspace is involved). Host feature arrays
 * are staged through context buffers, complete on return; so is a call with host frames.
 * FD_ERR_INVALID: ctx, opts, frames, xy, out_xy or out_status NULL; batch, rows or cols < 1; a negative
 * stride; an option outside its range above or not finite.
 */
int fd_points_refine(fd_ctx *ctx, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                     const fd_refine_opts *opts,
                     const float *xy, const uint8_t *valid, const int32_t *counts, int32_t stride,
                     float *out_xy, uint8_t *out_status, int32_t *out_counts, int io_on_device);

/* ---- RANSAC verification of matches and tracks (MI355X extension) ------------------------------------ */
#define FD_RANSAC_FUNDAMENTAL 0 /* fundamental matrix from m = 8 correspondences */
#define FD_RANSAC_HOMOGRAPHY 1  /* homography from m = 4 correspondences */
#define FD_RANSAC_MAX_HYPOTHESES 4096

typedef struct fd_ransac_opts {
    int32_t model;      /* FD_RANSAC_FUNDAMENTAL or FD_RANSAC_HOMOGRAPHY */
    int32_t hypotheses; /* 1..4096, all evaluated: no early exit */
    uint32_t seed;
    float threshold;    /* pixels, finite, > 0: Sampson distance (F), forward transfer error (H) */
    float center_x, center_y, scale; /* fixed conditioning transform, finite, scale > 0 */
} fd_ransac_opts;

/*
 * fd_ransac -- geometric verification of the correspondences of every frame of a batch: the model (F or H)
 * of the minimal sample with the most inliers among a fixed number of hypotheses, and the inlier mask.
 * The stage is an outlier filter whose mask feeds the next call (fd_flow_lk's valid, the prior features of
 * fd_points_detect); the model is the best minimal-sample model (fd_ransac_refit refits it). The reference has no such
 * stage: the contract is this text, a definite sequence. All floating point is double, every operation
 * rounded once, no contraction, f64 division correctly rounded.
 *
 * q_xy: float [batch][q_stride][2], t_xy: float [batch][t_stride][2], stored (x, y). q_counts int32 [batch]
 * (NULL: q_stride each; bits 25..31 ignored). match_idx int32 [batch][q_stride] as a matcher's out_idx
 * leaves it (NULL: slot i pairs with slot i, the tracker's case). pair_valid uint8 [batch][q_stride]: a
 * slot takes part only where the byte is exactly 1, so fd_flow_lk's out_status passes as it is (NULL: all).
 *
 * Correspondences of frame b: slot i is one when i < q_counts[b], pair_valid is NULL or 1 at the slot,
 * j = match_idx ? match_idx[i] : i satisfies 0 <= j < t_stride, and all four coordinates are finite.
 * They are taken in ascending i and numbered 0..n-1, each with four conditioned coordinates
 *   x = ((double)q.x - (double)center_x) * (double)scale, y likewise with center_y, (u, v) the same of t_xy[j].
 *
 * Sampler (uint32 arithmetic): mix(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16.
 * Hypothesis h of frame b: base = mix(mix(seed + 0x9E3779B9*b) + h). Pick k = 0..m-1 tries a = 0..31:
 * r = mix(base + 32k + a), idx = ((uint64)r * n) >> 32; the first idx not among the earlier picks is taken;
 * 32 failed tries make the hypothesis invalid. n < m: no hypothesis is valid.
 *
 * Rows of the 8 x 9 system. F, per pick: [u*x, u*y, u, v*x, v*y, v, x, y, 1]. H, per pick, two rows, in
 * pick order: [x, y, 1, 0, 0, 0, -(u*x), -(u*y), -u] and [0, 0, 0, x, y, 1, -(v*x), -(v*y), -v].
 *
 * Null vector, Gaussian elimination with complete pivoting. For k = 0..7: the pivot is the entry of largest
 * |A[r][c]| over r = k..7 (outer, ascending), c = k..8 (inner, ascending), compared with a strict > starting
 * from -1 at (k, k) (a NaN never wins); p0 = the pivot magnitude of step 0; the hypothesis is invalid unless
 * best > 1e-12 * p0; rows k <-> r and columns k <-> c are swapped (the column permutation recorded); for
 * r = k+1..7: f = A[r][k] / A[k][k], A[r][c] = A[r][c] - f * A[k][c] for c = k+1..8. Back substitution:
 * x[8] = 1; for k = 7..0: s = 0.0, s = s + A[k][c] * x[c] over c ascending from k+1, x[k] = (0.0 - s) / A[k][k].
 * The column permutation is undone; a non-finite entry makes the hypothesis invalid.
 *
 * Score, on conditioned coordinates with t = (double)threshold * (double)scale. F: l = F (x, y, 1),
 * m0, m1 the first two entries of F^T (u, v, 1), each a left-to-right sum of three products,
 * e = u*l0 + v*l1 + l2; inlier iff e*e <= (t*t) * (l0*l0 + l1*l1 + m0*m0 + m1*m1). H: w = h6*x + h7*y + h8,
 * dx = (h0*x + h1*y + h2) - u*w, dy = (h3*x + h4*y + h5) - v*w; inlier iff dx*dx + dy*dy <= (t*t) * (w*w).
 * A NaN fails the compare. The best hypothesis is the valid one with the most inliers, the lowest index
 * among equals (the matchers' rule). A frame with no valid hypothesis has no model.
 *
 * Outputs. out_model double [batch][9], row-major 3 x 3 in pixel coordinates: with
 * T = [[s, 0, -(s*cx)], [0, s, -(s*cy)], [0, 0, 1]] the F model is T^T (F T) and the H model T^-1 (H T),
 * T^-1 = [[1.0/s, 0, cx], [0, 1.0/s, cy], [0, 0, 1]], every product plain triple loops, each sum from 0.0
 * with the inner index ascending; the result is divided by its entry of largest magnitude (strict > from -1,
 * so the lowest index among equals), which becomes exactly 1.0. A frame with no model gets nine zeros.
 * out_inlier uint8 [batch][q_stride] (NULL to skip): 1 for a correspondence the best model classifies as an
 * inlier by the test above, 0 for every other slot below q_counts[b]; slots >= q_counts[b] are not written.
 * out_counts [batch] (NULL to skip): the number of ones. out_best [batch] (NULL to skip): the winning
 * hypothesis index, or -1. q_stride 0: nothing but out_counts = 0, out_best = -1 and a zero model.
 *
 * The arrays are device pointers when io_on_device: the call is then asynchronous on the context's stream,
 * and graph-capturable once a first call of the shape has sized the workspace. Host pointers otherwise:
 * staged through context buffers, complete on return.
 * FD_ERR_INVALID: ctx, opts, q_xy, t_xy or out_model NULL; batch < 1; a negative stride; match_idx NULL
 * with t_stride < q_stride; an option outside its range above or not finite.
 */
int fd_ransac(fd_ctx *ctx, int batch, const fd_ransac_opts *opts,
              const float *q_xy, const int32_t *q_counts, int32_t q_stride,
              const float *t_xy, int32_t t_stride,
              const int32_t *match_idx, const uint8_t *pair_valid,
              double *out_model, uint8_t *out_inlier, int32_t *out_counts, int32_t *out_best,
              int io_on_device);

#define FD_REFIT_MAX_ROUNDS 4
/* Jacobi sweeps of fd_ransac_refit. Found on the CPU with the restatement (tests/refit_ref.py): over every
 * scene of tests/test_refit_host.py and tests/test_gpu_refit.py the eigenvector of the 9 x 9 normal matrix and
 * the one of F^T F change no bit after 6 sweeps (first-round matrices); the rule adds 2
 * (tests/test_refit_host.py::test_sweep_count_rule). */
#define FD_REFIT_SWEEPS 8

typedef struct fd_refit_opts {
    int32_t model;      /* FD_RANSAC_FUNDAMENTAL or FD_RANSAC_HOMOGRAPHY */
    int32_t rounds;     /* 1..4 */
    float threshold;    /* pixels, finite, > 0: fd_ransac's */
    float center_x, center_y, scale; /* fd_ransac's conditioning transform: pass the same three */
} fd_refit_opts;

/*
 * fd_ransac_refit -- the least-squares refit of fd_ransac's model on its inliers: per frame the model that
 * minimises the algebraic error over the support set, the set classified again, up to `rounds` times while
 * the inlier count does not fall; F is projected to rank 2. The model a consumer such as fd_frames_warp
 * should take. A definite sequence like fd_ransac's, with its conventions: all floating point double, every
 * operation rounded once, no contraction, f64 division and square root correctly rounded.
 *
 * q_xy, q_counts, q_stride, t_xy, t_stride, match_idx, pair_valid: fd_ransac's, and the correspondence list
 * 0..n-1 with its conditioned coordinates (x, y, u, v) is fd_ransac's. in_model double [batch][9] and
 * in_inlier uint8 [batch][q_stride]: fd_ransac's out_model and out_inlier.
 *
 * Support set. S_0 = the correspondences whose in_inlier byte is exactly 1; c_0 = |S_0|.
 *
 * Round r = 1..rounds:
 * 1. Fit from S_(r-1). Invalid when |S| < 4 (H) or 8 (F). Normal matrix N (9 x 9) = sum over the support of
 *    row^T row with fd_ransac's rows, one per correspondence for F, two for H. Only the 45 entries (a, b),
 *    a <= b, are summed, each by acc = acc + row[a] * row[b], then mirrored. Order: partial L = 0..255 starts
 *    from 0.0 and takes the list positions i = L, L + 256, ... in ascending i, skipping those not in S; for H
 *    the first row's product is added, then the second's. The partials are combined by the tree
 *    P[L] = P[L] + P[L + step] for all L < step, with step = 128, 64, ..., 1; N is P[0].
 * 2. Eigenvector by cyclic Jacobi on A = N (n = 9) with V = identity, FD_REFIT_SWEEPS sweeps, each visiting
 *    the pairs (p, q), p < q, in row-major order. A pair with A[p][q] == 0.0 is skipped. Otherwise, with
 *    app, aqq, apq the entries before the rotation:
 *      theta = (aqq - app) / (2.0 * apq);  t = (theta < 0 ? -1.0 : 1.0) / (|theta| + sqrt(theta*theta + 1.0))
 *      c = 1.0 / sqrt(t*t + 1.0);  s = t * c
 *    and every new element is an expression of the elements before the rotation:
 *      for k != p, q:  A[k][p] = A[p][k] = c*A[k][p] - s*A[k][q];   A[k][q] = A[q][k] = s*A[k][p] + c*A[k][q]
 *      A[p][p] = app - t*apq;  A[q][q] = aqq + t*apq;  A[p][q] = A[q][p] = 0.0
 *      for every k:    V[k][p] = c*V[k][p] - s*V[k][q];             V[k][q] = s*V[k][p] + c*V[k][q]
 *    (each product rounded, then the sum or difference). The solution is column j of V, j the index of the
 *    smallest diagonal entry of A (strict < from entry 0: the lowest index among equals). The fit is invalid
 *    for a non-finite entry of that column, and unless d2 > 1e-12 * dmax, d2 the smallest diagonal entry apart
 *    from entry j and dmax the largest (a NaN fails): a support set that leaves more than one direction free
 *    (collinear points for H, a pure translation for F) has no refit.
 * 3. F only, rank 2. G = F^T F, G[i][j] = sum over k ascending from 0.0 of F[k][i] * F[k][j]; the same Jacobi
 *    routine with n = 3 on G; v = the column of V at G's smallest diagonal entry; w[i] = sum over j ascending
 *    from 0.0 of F[i][j] * v[j]; F[i][j] = F[i][j] - w[i] * v[j]. A non-finite entry makes the fit invalid.
 * 4. Classify every correspondence of the list, not only the support, by fd_ransac's inlier test with the new
 *    model and t = (double)threshold * (double)scale: S_r, c_r = |S_r|.
 * 5. Guard: the round is accepted iff the fit is valid and c_r >= c_(r-1). Otherwise the loop stops and the
 *    state of the last accepted round stands.
 *
 * Outputs. out_model double [batch][9]: the model of the last accepted round, denormalised and divided by
 * its entry of largest magnitude exactly as fd_ransac's; with no accepted round the nine doubles of in_model,
 * bit for bit. out_inlier uint8 [batch][q_stride] (NULL to skip): 1 for the members of the last accepted
 * round's S (of S_0 with none: a member's byte becomes exactly 1), 0 for every other slot below q_counts[b];
 * slots >= q_counts[b] are not written. out_counts [batch] (NULL to skip): |S|. out_rounds int32 [batch]
 * (NULL to skip): the accepted rounds, 0..rounds. out_model may be in_model and out_inlier may be in_inlier.
 * q_stride 0: out_model = in_model, out_counts = 0, out_rounds = 0.
 *
 * Device pointers when io_on_device: asynchronous on the context's stream (k_ransac_compact and one more
 * kernel), graph-capturable once a first call of the shape has sized the workspace. Host pointers otherwise:
 * staged through context buffers, complete on return.
 * FD_ERR_INVALID: fd_ransac's conditions; rounds outside 1..4; in_model or in_inlier NULL.
 */
int fd_ransac_refit(fd_ctx *ctx, int batch, const fd_refit_opts *opts,
                    const float *q_xy, const int32_t *q_counts, int32_t q_stride,
                    const float *t_xy, int32_t t_stride,
                    const int32_t *match_idx, const uint8_t *pair_valid,
                    const double *in_model, const uint8_t *in_inlier,
                    double *out_model, uint8_t *out_inlier, int32_t *out_counts, int32_t *out_rounds,
                    int io_on_device);

/* ---- Relative pose from a fundamental matrix, and triangulation (MI355X extension) --------------------- */
/* Jacobi sweeps of fd_pose_recover. Found on the CPU with the restatement (tests/pose_ref.py) by
 * FD_REFIT_SWEEPS's rule: over every scene of tests/test_pose_host.py and tests/test_gpu_pose.py the diagonal and
 * V of E^T E change no bit after 5 sweeps; the rule adds 2 (tests/test_pose_host.py::test_sweep_count_rule). */
#define FD_POSE_SWEEPS 7

typedef struct fd_pose_opts {
    double fx_q, fy_q, cx_q, cy_q; /* zero-skew pinhole camera of the q image: finite, fx and fy non-zero */
    double fx_t, fy_t, cx_t, cy_t; /* the t image's */
    float max_depth;    /* > 0, +inf allowed: the largest accepted depth along either ray, in units of |t| */
    float min_parallax; /* 0..1: the sine of the smallest accepted angle between the two rays */
} fd_pose_opts;

/*
 * fd_triangulate and fd_pose_recover -- what a front end verifies matches or tracks for: the relative camera
 * pose (R, t), X_t = R X_q + t, from the fundamental matrix of fd_ransac / fd_ransac_refit, and the 3-D
 * points of the inliers in the q camera's frame. Definite sequences like fd_ransac's, with its conventions:
 * all floating point double, every operation rounded once, no contraction, f64 division and square root
 * correctly rounded. No lens distortion (undistort or warp first), no five-point solver (PnP: fd_pnp_ransac below).
 *
 * q_xy, q_counts, q_stride, t_xy, t_stride, match_idx, pair_valid: fd_ransac's, with its rules for which
 * slots are correspondences. Coordinates are plain pixels, x = (double)q.x: no conditioning transform.
 * Normalised rays: ax = (x - cx_q) / fx_q, ay = (y - cy_q) / fy_q, and (bx, by) the same of t_xy[j] with the t
 * camera.
 *
 * The step, per correspondence and pose (R row-major, t):
 *   r[i] = R[i][0]*ax + R[i][1]*ay + R[i][2] (left to right);  p' = (bx, by, 1)
 *   rr = r.r, pp = p'.p', rp = r.p', rt = r.t, pt = p'.t, each a left-to-right sum of three products
 *   det = rr*pp - rp*rp;  z1 = (rp*pt - pp*rt) / det;  z2 = (rr*pt - rp*rt) / det
 * (the depths along the two rays that minimise |z1 r - z2 p' + t|). The point is in front iff
 *   det > (m*m) * (rr*pp), m = (double)min_parallax;  z1 > 0;  z2 > 0;  z1 <= D;  z2 <= D, D = (double)max_depth
 * (a NaN fails every compare). The 3-D point is (z1*ax, z1*ay, z1), each component rounded once to float.
 *
 * fd_triangulate, a known pose (a calibrated stereo rig behind fd_flow_lk, or a pose from elsewhere).
 * in_pose double [batch][12]: R row-major, then t, of any scale. in_inlier uint8 [batch][q_stride] (NULL: every
 * correspondence): only the slots whose byte is exactly 1 take part. out_points float [batch][q_stride][3],
 * out_valid uint8 [batch][q_stride]: 1 and the point for a participating correspondence that is in front; 0
 * and a zero point for every other slot below q_counts[b]; slots >= q_counts[b] are not written. out_counts
 * int32 [batch]: the ones. Each of the three may be NULL. q_stride 0: out_counts = 0.
 *
 * fd_pose_recover. in_model double [batch][9]: a fundamental matrix with (u, v, 1) F (x, y, 1)^T = 0, (u, v)
 * from t_xy (fd_ransac's out_model); in_inlier as above, required.
 * 1. E = K_t^T (F K_q), K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]: both products plain triple loops, each sum
 *    from 0.0 with the inner index ascending.
 * 2. G[i][j] = sum over k ascending from 0.0 of E[k][i]*E[k][j]; fd_ransac_refit's cyclic Jacobi on G (n = 3,
 *    V = identity), FD_POSE_SWEEPS sweeps; d = the diagonal; j = the index of its smallest entry (strict < from
 *    entry 0), a < b the other two; v1 = V[:, a], v2 = V[:, b].
 * 3. w1 = E v1, w2 = E v2 (rows summed left to right); u1 = w1 / sqrt(w1.w1), u2 = w2 / sqrt(w2.w2) (the dot
 *    products left to right); u3 = u1 x u2, v3 = v1 x v2, every component a*b - c*d with both products rounded
 *    first: (u1, u2, u3) and (v1, v2, v3) are right-handed, so no determinant needs a sign fix.
 * 4. Ra[i][k] = (u2[i]*v1[k] - u1[i]*v2[k]) + u3[i]*v3[k];  Rb[i][k] = (u1[i]*v2[k] - u2[i]*v1[k]) + u3[i]*v3[k].
 *    Candidates: 0 (Ra, +u3), 1 (Ra, -u3), 2 (Rb, +u3), 3 (Rb, -u3).
 *    There is no pose unless d, v1, v2, u3, Ra and Rb are all finite and min(d[a], d[b]) > 1e-12 * max(d): a zero
 *    model and a model of rank 1 have none.
 * 5. Every correspondence whose in_inlier byte is exactly 1 runs the step for the four candidates; c_k = the
 *    number in front. The winner is the largest c_k, the lowest k among equals; c_k = 0: no pose. A pure
 *    rotation has a rank-2 E but parallel rays: with min_parallax > 0 no candidate has a point.
 * out_pose double [batch][12]: the winner's R, then its t (|t| = 1 to rounding); twelve zeros without a pose.
 * out_choice int32 [batch]: 0..3, or -1. out_points, out_valid, out_counts: fd_triangulate's, for the winner and
 * the in_inlier set; without a pose zeros below q_counts[b]. Every output may be NULL. q_stride 0: out_counts =
 * 0, out_choice = -1, a zero pose.
 *
 * Device pointers when io_on_device: asynchronous on the context's stream (one kernel, no workspace: always
 * graph-capturable). Host pointers otherwise: staged through context buffers, complete on return.
 * FD_ERR_INVALID: ctx, opts, q_xy, t_xy, in_pose (fd_triangulate), in_model or in_inlier (fd_pose_recover)
 * NULL; batch < 1; a negative stride; match_idx NULL with t_stride < q_stride; a camera value not finite, fx
 * or fy zero; max_depth not > 0 (a NaN included); min_parallax outside 0..1.
 */
int fd_triangulate(fd_ctx *ctx, int batch, const fd_pose_opts *opts,
                   const float *q_xy, const int32_t *q_counts, int32_t q_stride,
                   const float *t_xy, int32_t t_stride,
                   const int32_t *match_idx, const uint8_t *pair_valid,
                   const double *in_pose, const uint8_t *in_inlier,
                   float *out_points, uint8_t *out_valid, int32_t *out_counts,
                   int io_on_device);

int fd_pose_recover(fd_ctx *ctx, int batch, const fd_pose_opts *opts,
                    const float *q_xy, const int32_t *q_counts, int32_t q_stride,
                    const float *t_xy, int32_t t_stride,
                    const int32_t *match_idx, const uint8_t *pair_valid,
                    const double *in_model, const uint8_t *in_inlier,
                    double *out_pose, int32_t *out_choice,
                    float *out_points, uint8_t *out_valid, int32_t *out_counts,
                    int io_on_device);

/* ---- Absolute pose from 3-D points: PnP RANSAC and refinement (MI355X extension) ----------------------- */
#define FD_PNP_MAX_ROUNDS 8

typedef struct fd_pnp_opts {
    int32_t hypotheses; /* 1..4096, all evaluated (fd_pnp_ransac; fd_pnp_refit ignores it) */
    uint32_t seed;      /* fd_pnp_ransac */
    int32_t rounds;     /* 1..8 (fd_pnp_refit; fd_pnp_ransac ignores it) */
    float threshold;    /* pixels, finite, > 0: the reprojection error */
    double fx, fy, cx, cy; /* zero-skew pinhole camera of the t image: finite, fx and fy non-zero */
    double center[3], scale; /* fixed conditioning of the 3-D points, finite, scale > 0 (fd_pnp_ransac; fd_pnp_refit
                                works in the camera's units and ignores them) */
} fd_pnp_opts;

/*
 * fd_pnp_ransac and fd_pnp_refit -- the camera pose (R, t), X_t = R X + t, of the t image against known 3-D
 * points: the step that places the next frame against the points fd_pose_recover / fd_triangulate left, at
 * their scale. Definite sequences like fd_ransac's, with its conventions: all floating point double, every
 * operation rounded once, no contraction, f64 division and square root correctly rounded; only + - * / sqrt. An
 * expression written a + b + c is summed left to right; "from 0.0" means the sum starts at 0.0.
 *
 * p_xyz float [batch][q_stride][3]: fd_triangulate's / fd_pose_recover's out_points as it is; p_valid uint8
 * [batch][q_stride]: their out_valid as it is (NULL: all). t_xy float [batch][t_stride][2]. q_counts, match_idx,
 * pair_valid: fd_ransac's (the tracker's out_status passes as pair_valid as it is).
 * Correspondences of frame b: slot i is one when i < q_counts[b], p_valid and pair_valid are each NULL or exactly
 * 1 at the slot, j = match_idx ? match_idx[i] : i satisfies 0 <= j < t_stride, and the three coordinates of the
 * point and the two of t_xy[j] are finite. They are taken in ascending i and numbered 0..n-1, each with
 *   the ray  bx = ((double)u - cx) / fx,  by = ((double)v - cy) / fy,  (u, v) = t_xy[j], and
 *   the point  Xc = ((double)p.x - center[0]) * scale, Yc and Zc likewise (fd_pnp_refit: X = (double)p.x).
 *
 * Inlier test of a 3 x 4 matrix P (row-major) on a correspondence, with t = (double)threshold:
 *   y_i = P[i][0]*Xc + P[i][1]*Yc + P[i][2]*Zc + P[i][3];  w = y_2
 *   dx = fx * (y_0 - bx*w);  dy = fy * (y_1 - by*w);  inlier iff w > 0 and dx*dx + dy*dy <= (t*t) * (w*w)
 * (division-free like fd_ransac's H; a NaN fails).
 *
 * fd_pnp_ransac: fixed-count RANSAC over 6-point DLT camera matrices.
 * Sample: m = 6 picks by fd_ransac's sampler unchanged. System: pick k gives the rows 2k and 2k + 1,
 *   [Xc, Yc, Zc, 1, 0, 0, 0, 0, -(bx*Xc), -(bx*Yc), -(bx*Zc), -bx]
 *   [0, 0, 0, 0, Xc, Yc, Zc, 1, -(by*Xc), -(by*Yc), -(by*Zc), -by]
 * and the first 11 rows form the 11 x 12 system. Null vector: fd_ransac's Gaussian elimination with complete
 * pivoting, with R = 11 rows and R + 1 columns where that text has 8 and 9 (r = k..R-1 outer, c = k..R inner, the
 * same strict >, the same test best > 1e-12 * p0, back substitution from x[R] = 1, the permutation undone, a
 * non-finite entry invalid). The twelve entries are P, row-major.
 * Sign: det = (P0*(P5*P10 - P6*P9) - P1*(P4*P10 - P6*P8)) + P2*(P4*P9 - P5*P8), P0..P11 the entries in order
 * (the determinant of the left 3 x 3 block M); the hypothesis is invalid if det is 0 or not finite; if det < 0
 * all twelve entries are negated. Coplanar points and other degenerate samples fail the pivot test: a planar
 * scene has no DLT pose (points that are coplanar only up to their float rounding pass the test with a matrix that
 * fits them and an arbitrary pose).
 * Score: the inlier test over the frame's correspondences. The best hypothesis is the valid one with the most
 * inliers, the lowest index among equals. n < 6: no hypothesis is valid.
 * Winner to pose: G[i][j] = sum over k ascending from 0.0 of M[k][i]*M[k][j]; fd_ransac_refit's cyclic Jacobi on G
 * (n = 3, V = identity), FD_POSE_SWEEPS sweeps, giving the diagonal d and V; sd[j] = sqrt(d[j]);
 * W[i][j] = sum over k from 0.0 of M[i][k]*V[k][j];  R[i][k] = sum over j from 0.0 of (W[i][j] / sd[j]) * V[k][j];
 * ks = (sd[0] + sd[1] + sd[2]) / 3.0;  tc[i] = P[i][3] / ks;
 * t[i] = tc[i] / scale - (R[i][0]*center[0] + R[i][1]*center[1] + R[i][2]*center[2]).
 * There is no pose unless d, V, R and t are all finite and min(d) > 1e-12 * max(d). A frame whose winner has no
 * pose is treated as one without a valid hypothesis.
 * Outputs. out_pose double [batch][12]: R row-major, then t; twelve zeros without a pose. out_inlier uint8
 * [batch][q_stride] (NULL to skip): 1 for a correspondence the winning P classifies as an inlier, 0 for every
 * other slot below q_counts[b] (all of them without a pose); slots >= q_counts[b] are not written. out_counts
 * [batch] (NULL to skip): the ones. out_best [batch] (NULL to skip): the winning hypothesis, or -1. q_stride 0:
 * nothing but out_counts = 0, out_best = -1 and a zero pose.
 *
 * fd_pnp_refit: Gauss-Newton on the reprojection error over the inliers, unconditioned (center 0, scale 1).
 * in_pose double [batch][12] and in_inlier uint8 [batch][q_stride]: fd_pnp_ransac's out_pose and out_inlier.
 * Start: S_0 = the correspondences whose in_inlier byte is exactly 1; the current pose is in_pose; c_0 = the
 * number of correspondences of the whole list that P = [R | t] of in_pose classifies as inliers. (Not |S_0|:
 * orthonormalising a projective winner usually loses inliers, and this c_0 lets the first round be accepted.)
 * Round r = 1..rounds, for the current (R, t):
 * 1. For each member of S_(r-1): y_i = R[i][0]*X + R[i][1]*Y + R[i][2]*Z + t[i]; iz = 1.0 / y_2; a = y_0*iz;
 *    b = y_1*iz; the two rows of seven
 *      jx = [fx * -(a*b), fx * (1.0 + a*a), fx * -b, fx * iz, 0.0, fx * -(a*iz), fx * (a - bx)]
 *      jy = [fy * -(1.0 + b*b), fy * (a*b), fy * a, 0.0, fy * iz, fy * -(b*iz), fy * (b - by)]
 *    (the Jacobian of the left perturbation y' = y + w x y + delta, then the residual). The 27 entries (i, j),
 *    i = 0..5, j = i..6, row-major, are summed: acc = acc + jx[i]*jx[j], then acc = acc + jy[i]*jy[j]. Order:
 *    fd_ransac_refit's, 256 partials from 0.0 over the list positions L, L + 256, ... ascending (members only),
 *    then the tree P[L] = P[L] + P[L + step], step = 128..1. They fill the 6 x 7 system [N | g], N mirrored.
 * 2. x = the null vector of [N | g] by the elimination above with R = 6 (x[6] = 1): N x + g = 0.
 *    w = x[0..2], delta = x[3..5].
 * 3. Cayley transform: h[i] = w[i] / 2.0; hh = h0*h0 + h1*h1 + h2*h2; f = 2.0 / (1.0 + hh);
 *    K = [[0, -h2, h1], [h2, 0, -h0], [-h1, h0, 0]];
 *    C[i][j] = (i == j ? 1.0 : 0.0) + f * (K[i][j] + (h[i]*h[j] - (i == j ? hh : 0.0)));
 *    R' = C R (sums from 0.0, inner index ascending); t'[i] = C[i][0]*t[0] + C[i][1]*t[1] + C[i][2]*t[2] + delta[i].
 *    The round is invalid unless the solve is valid and R', t' are finite.
 * 4. Classify every correspondence of the list with P = [R' | t']: S_r, c_r = |S_r|.
 * 5. Guard: the round is accepted iff it is valid and c_r >= c_(r-1); (R', t') becomes the current pose.
 *    Otherwise the loop stops and the state of the last accepted round stands.
 * Outputs. out_pose: the pose of the last accepted round; with none the twelve doubles of in_pose, bit for bit.
 * out_inlier (NULL to skip): 1 for the members of the last accepted round's S (of S_0 with none), 0 for every
 * other slot below q_counts[b]; slots >= q_counts[b] are not written. out_counts (NULL to skip): the ones of
 * out_inlier. out_rounds int32 [batch] (NULL to skip): the accepted rounds, 0..rounds. out_pose may be in_pose
 * and out_inlier may be in_inlier. q_stride 0: out_pose = in_pose, out_counts = 0, out_rounds = 0.
 *
 * Device pointers when io_on_device: asynchronous on the context's stream (three kernels; fd_pnp_refit: two),
 * graph-capturable once a first call of the shape has sized the workspace. Host pointers otherwise: staged
 * through context buffers, complete on return.
 * FD_ERR_INVALID: ctx, opts, p_xyz, t_xy or out_pose NULL (fd_pnp_refit: in_pose or in_inlier too); batch < 1; a
 * negative stride; match_idx NULL with t_stride < q_stride; threshold not finite or not > 0; a camera value not
 * finite, fx or fy zero; fd_pnp_ransac: hypotheses outside 1..4096, center or scale not finite, scale not > 0;
 * fd_pnp_refit: rounds outside 1..8.
 */
int fd_pnp_ransac(fd_ctx *ctx, int batch, const fd_pnp_opts *opts,
                  const float *p_xyz, const uint8_t *p_valid, const int32_t *q_counts, int32_t q_stride,
                  const float *t_xy, int32_t t_stride,
                  const int32_t *match_idx, const uint8_t *pair_valid,
                  double *out_pose, uint8_t *out_inlier, int32_t *out_counts, int32_t *out_best,
                  int io_on_device);

int fd_pnp_refit(fd_ctx *ctx, int batch, const fd_pnp_opts *opts,
                 const float *p_xyz, const uint8_t *p_valid, const int32_t *q_counts, int32_t q_stride,
                 const float *t_xy, int32_t t_stride,
                 const int32_t *match_idx, const uint8_t *pair_valid,
                 const double *in_pose, const uint8_t *in_inlier,
                 double *out_pose, uint8_t *out_inlier, int32_t *out_counts, int32_t *out_rounds,
                 int io_on_device);

/* ---- 3-D point-set alignment: similarity / rigid RANSAC, refit and apply (MI355X extension) ------------- */
#define FD_ALIGN_SIMILARITY 0 /* Y = s R X + t, 7 degrees of freedom */
#define FD_ALIGN_RIGID      1 /* s is exactly 1.0 everywhere, 6 degrees of freedom */
#define FD_ALIGN_MAX_ROUNDS 8
/* Jacobi sweeps of fd_align_refit. Found on the CPU with the restatement (tests/align_ref.py) by FD_REFIT_SWEEPS's
 * rule: over every scene of tests/test_align_host.py and tests/test_gpu_align.py the diagonal of Horn's 4 x 4 matrix
 * and the quaternion q change no bit after 5 sweeps; the rule adds 2 (tests/test_align_host.py::test_sweep_count_rule). */
#define FD_ALIGN_SWEEPS 7

typedef struct fd_align_opts {
    int32_t kind;       /* FD_ALIGN_SIMILARITY or FD_ALIGN_RIGID */
    int32_t hypotheses; /* 1..4096, all evaluated (fd_align_ransac; fd_align_refit ignores it) */
    uint32_t seed;      /* fd_align_ransac */
    int32_t rounds;     /* 1..8 (fd_align_refit; fd_align_ransac ignores it) */
    float threshold;    /* finite, > 0: the distance |Y - (s R X + t)| in the target's units */
} fd_align_opts;

/*
 * fd_align_ransac, fd_align_refit and fd_align_apply -- the similarity (or rigid) transform Y = s R X + t between two
 * sets of 3-D points with known correspondences, and its application: what joins a new keyframe window to the map
 * before it, closes a loop whose landmarks were triangulated twice at drifted scales, or registers fd_pose_recover's
 * points (in units of the first baseline) against metric ones. Definite sequences like fd_pnp_ransac's, with its
 * conventions: all floating point double, every operation rounded once, no contraction, f64 division and square root
 * correctly rounded; only + - * / sqrt. An expression written a + b + c is summed left to right; "from 0.0" means the
 * sum starts at 0.0; a.b of two 3-vectors is a0*b0 + a1*b1 + a2*b2; a x b has the components a1*b2 - a2*b1,
 * a2*b0 - a0*b2, a0*b1 - a1*b0, both products rounded first. tests/align_ref.py restates the three calls.
 *
 * q_xyz float [batch][q_stride][3] and t_xyz float [batch][t_stride][3]; q_valid uint8 [batch][q_stride] and t_valid
 * uint8 [batch][t_stride] (each NULL: all): fd_triangulate's / fd_pose_recover's out_points and out_valid as they are.
 * q_counts, match_idx, pair_valid: fd_pnp_ransac's.
 * Correspondences of frame b: slot i is one when i < q_counts[b], q_valid and pair_valid are each NULL or exactly 1
 * at i, j = match_idx ? match_idx[i] : i satisfies 0 <= j < t_stride, t_valid is NULL or exactly 1 at j, and the six
 * coordinates are finite. They are taken in ascending i and numbered 0..n-1, with X = (double)q_xyz[i] and
 * Y = (double)t_xyz[j] (six doubles; no conditioning: every formula below works on differences or centred values).
 *
 * Model: 13 doubles, R row-major, then t, then s. FD_ALIGN_RIGID: s is exactly 1.0 wherever a model is computed.
 * Inlier test of a model on a correspondence, with th = (double)threshold:
 *   z_i = s * (R[i][0]*X0 + R[i][1]*X1 + R[i][2]*X2) + t[i];  e_i = Y_i - z_i
 *   inlier iff e0*e0 + e1*e1 + e2*e2 <= th*th  (a NaN fails).
 *
 * fd_align_ransac: fixed-count RANSAC over 3-point samples, m = 3 picks a, b, c by fd_ransac's sampler unchanged.
 * 1. u = Xb - Xa, v = Xc - Xa, U = Yb - Ya, V = Yc - Ya.
 * 2. Frame of (u, v): uu = u.u; e1 = u / sqrt(uu) (each component divided by the one square root); d = v.e1;
 *    w = v - d*e1; ww = w.w; e2 = w / sqrt(ww); e3 = e1 x e2. The frame is valid iff uu > 0 and ww > 1e-12 * (v.v):
 *    duplicate and collinear picks fail. The same of (U, V) gives f1, f2, f3.
 * 3. R[i][j] = f1[i]*e1[j] + f2[i]*e2[j] + f3[i]*e3[j].
 * 4. FD_ALIGN_SIMILARITY: s = sqrt((U.U + V.V + G.G) / (u.u + v.v + g.g)) with G = V - U and g = v - u (the ratio of
 *    the triangles' summed squared side lengths). FD_ALIGN_RIGID: s = 1.0.
 * 5. Xm = Xa + (u + v) / 3.0, Ym = Ya + (U + V) / 3.0, per component.
 * 6. t[i] = Ym[i] - s * (R[i][0]*Xm0 + R[i][1]*Xm1 + R[i][2]*Xm2).
 * 7. The hypothesis is invalid unless both frames are valid, all 13 values are finite and s > 0.
 * Score: the inlier test over the frame's correspondences. The best hypothesis is the valid one with the most
 * inliers, the lowest index among equals. n < 3: no hypothesis is valid.
 * Outputs. out_model double [batch][13]: the winner's; thirteen zeros without one. out_inlier uint8
 * [batch][q_stride] (NULL to skip): 1 for a correspondence the winner classifies as an inlier, 0 for every other slot
 * below q_counts[b]; slots >= q_counts[b] are not written. out_counts [batch] (NULL to skip): the ones. out_best
 * [batch] (NULL to skip): the winning hypothesis, or -1. q_stride 0: nothing but out_counts = 0, out_best = -1 and a
 * zero model.
 *
 * fd_align_refit: closed-form least squares (Horn's quaternion method) on the members, the list classified again.
 * in_model double [batch][13] and in_inlier uint8 [batch][q_stride]: fd_align_ransac's out_model and out_inlier.
 * Start: S_0 = the correspondences whose in_inlier byte is exactly 1; c_0 = the number of correspondences of the
 * whole list that in_model classifies as inliers. Round r = 1..rounds, on S_(r-1) with m members:
 * 1. The six sums of X and Y over the members, in fd_ransac_refit's order: 256 partials from 0.0 over the list
 *    positions L, L + 256, ... ascending (members only), then the tree P[L] = P[L] + P[L + step], step = 128..1.
 *    Xb = sum / (double)m, Yb likewise. The round is invalid for m < 3.
 * 2. A second pass in the same order, with xc = X - Xb and yc = Y - Yb: the nine A[i][j] = A[i][j] + xc[i]*yc[j]
 *    (i the source row, j the target column, row-major), then Sx = Sx + (xc0*xc0 + xc1*xc1 + xc2*xc2).
 * 3. With Sxx = A[0][0], Sxy = A[0][1], ..., Szz = A[2][2], the symmetric matrix
 *      N = [[ Sxx+Syy+Szz, Syz-Szy,      Szx-Sxz,      Sxy-Syx     ],
 *           [ Syz-Szy,     Sxx-Syy-Szz,  Sxy+Syx,      Szx+Sxz     ],
 *           [ Szx-Sxz,     Sxy+Syx,     -Sxx+Syy-Szz,  Syz+Szy     ],
 *           [ Sxy-Syx,     Szx+Sxz,      Syz+Szy,     -Sxx-Syy+Szz ]]
 *    (a leading -Sxx is the negation, then the two further terms left to right); fd_ransac_refit's cyclic Jacobi on N
 *    (n = 4, V = identity), FD_ALIGN_SWEEPS sweeps; k = the index of the largest diagonal entry (strict > from entry
 *    0); (a, b, c, d) = V[:, k]; qq = a*a + b*b + c*c + d*d;
 *      R00 = (a*a+b*b-c*c-d*d)/qq   R01 = (2.0*(b*c-a*d))/qq     R02 = (2.0*(b*d+a*c))/qq
 *      R10 = (2.0*(b*c+a*d))/qq     R11 = (a*a-b*b+c*c-d*d)/qq   R12 = (2.0*(c*d-a*b))/qq
 *      R20 = (2.0*(b*d-a*c))/qq     R21 = (2.0*(c*d+a*b))/qq     R22 = (a*a-b*b-c*c+d*d)/qq
 *    always a proper rotation, for planar member sets too (collinear members leave the roll about their line free).
 * 4. FD_ALIGN_SIMILARITY: s = (the sum over i, j row-major from 0.0 of R[i][j]*A[j][i]) / Sx. FD_ALIGN_RIGID:
 *    s = 1.0. The round is invalid unless Sx > 0, the 13 values are finite and s > 0.
 * 5. t[i] = Yb[i] - s * (R[i][0]*Xb0 + R[i][1]*Xb1 + R[i][2]*Xb2).
 * 6. Classify every correspondence of the list: S_r, c_r = |S_r|. Guard: the round is accepted iff it is valid and
 *    c_r >= c_(r-1); otherwise the loop stops and the state of the last accepted round stands.
 * Outputs. out_model: the model of the last accepted round; with none the thirteen doubles of in_model, bit for bit.
 * out_inlier (NULL to skip): 1 for the members of the last accepted round's S (of S_0 with none), 0 for every other
 * slot below q_counts[b]; slots >= q_counts[b] are not written. out_counts (NULL to skip): the ones of out_inlier.
 * out_rounds int32 [batch] (NULL to skip): the accepted rounds, 0..rounds. out_model may be in_model and out_inlier
 * may be in_inlier. q_stride 0: out_model = in_model, out_counts = 0, out_rounds = 0.
 *
 * fd_align_apply: a model applied to points, so that the merged set stays on the device. model double [batch][13];
 * xyz_in float [batch][stride][3]; valid uint8 [batch][stride] (NULL: all); counts int32 [batch] (NULL: stride; bits
 * 25..31 ignored, at most stride). For every slot i < counts[b] whose valid byte is NULL or exactly 1:
 * xyz_out[i] = (float)z, z the inlier test's expression with X = (double)xyz_in[i], each component rounded once to
 * float. Every other slot is not written. xyz_out may be xyz_in. stride 0: nothing is written.
 *
 * Device pointers when io_on_device: asynchronous on the context's stream (three kernels; fd_align_refit: two;
 * fd_align_apply: one, no workspace), graph-capturable once a first call of the shape has sized the workspace. Host
 * pointers otherwise: staged through context buffers, complete on return.
 * FD_ERR_INVALID: ctx, opts, q_xyz, t_xyz or out_model NULL (fd_align_refit: in_model or in_inlier too); batch < 1; a
 * negative stride; match_idx NULL with t_stride < q_stride; threshold not finite or not > 0; kind neither constant;
 * fd_align_ransac: hypotheses outside 1..4096; fd_align_refit: rounds outside 1..8. fd_align_apply: ctx, model,
 * xyz_in or xyz_out NULL; batch < 1; a negative stride.
 * The threshold is absolute, in the target's units: a threshold that grows with depth is not in this call.
 */
int fd_align_ransac(fd_ctx *ctx, int batch, const fd_align_opts *opts,
                    const float *q_xyz, const uint8_t *q_valid, const int32_t *q_counts, int32_t q_stride,
                    const float *t_xyz, const uint8_t *t_valid, int32_t t_stride,
                    const int32_t *match_idx, const uint8_t *pair_valid,
                    double *out_model, uint8_t *out_inlier, int32_t *out_counts, int32_t *out_best,
                    int io_on_device);

int fd_align_refit(fd_ctx *ctx, int batch, const fd_align_opts *opts,
                   const float *q_xyz, const uint8_t *q_valid, const int32_t *q_counts, int32_t q_stride,
                   const float *t_xyz, const uint8_t *t_valid, int32_t t_stride,
                   const int32_t *match_idx, const uint8_t *pair_valid,
                   const double *in_model, const uint8_t *in_inlier,
                   double *out_model, uint8_t *out_inlier, int32_t *out_counts, int32_t *out_rounds,
                   int io_on_device);

int fd_align_apply(fd_ctx *ctx, int batch, const double *model,
                   const float *xyz_in, const uint8_t *valid, const int32_t *counts, int32_t stride,
                   float *xyz_out, int io_on_device);

/* ---- Windowed bundle adjustment (MI355X extension) ------------------------------------------------------ */
#define FD_BA_MAX_CAMS 8
#define FD_BA_MAX_ROUNDS 16

typedef struct fd_ba_opts {
    int32_t rounds;        /* 1..16 LM trials (accepted + rejected) */
    float   threshold;     /* pixels, finite, > 0: truncation of the cost and the inlier gate */
    double  fx, fy, cx, cy;/* one zero-skew pinhole camera for all views, as fd_pnp_opts */
    double  lambda, up, down; /* initial damping > 0, factor on reject > 1, factor on accept in (0, 1] */
} fd_ba_opts;

/*
 * fd_bundle_adjust -- the poses of up to 8 cameras and the 3-D points they share, refined together: the local
 * bundle adjustment over the last few keyframes that corrects what fd_pose_recover's two-view points and
 * fd_pnp_refit's motion-only refinement leave. It minimises the truncated reprojection cost by Levenberg-Marquardt,
 * the points eliminated by the Schur complement onto the free cameras. A definite sequence like fd_pnp_refit's, with
 * its conventions: all floating point double, every operation rounded once, no contraction, f64 division correctly
 * rounded; only + - * /. An expression written a + b + c is summed left to right; "from 0.0" means the sum starts at
 * 0.0. tests/ba_ref.py restates it.
 *
 * in_poses double [batch][cams][12]: per camera fd_pnp_ransac's / fd_pnp_refit's out_pose as it is (R row-major,
 * then t; X_c = R X + t); the first camera of a two-view start is the identity (1 0 0 0 1 0 0 0 1 0 0 0) and the
 * second fd_pose_recover's out_pose. cam_fixed uint8 [batch][cams]: a non-zero byte holds the camera; NULL: camera 0
 * alone is held. A problem with no free camera is legal (structure-only refinement), and so is one whose points are
 * all held (below). p_xyz float [batch][p_stride][3] and p_valid uint8 [batch][p_stride] (NULL: all):
 * fd_triangulate's / fd_pose_recover's out_points and out_valid as they are. counts int32 [batch] (NULL: p_stride;
 * bits 25..31 ignored, at most p_stride). obs_xy float [batch][cams][o_stride][2] and obs_valid uint8
 * [batch][cams][o_stride] (NULL: all): row c is the tracker's out_xy and out_status of frame c. Slot i of every
 * camera observes point i: tracks are slot-aligned and there is no match_idx in this call; a caller with matched,
 * not tracked, features gathers them into slot order first.
 *
 * Observation (c, i) of problem b exists iff i < counts[b], p_valid and obs_valid are each NULL or exactly 1 at the
 * slot, and the three floats of the point and the two of obs_xy[c][i] are finite. Its ray is
 *   bx = ((double)u - cx) / fx,  by = ((double)v - cy) / fy,  (u, v) = obs_xy[c][i],
 * and the point starts as X = ((double)p.x, (double)p.y, (double)p.z). A point participates when it has an observation.
 * A state is the poses of all cameras and the points. t = (double)threshold, tt = t*t.
 *
 * Cost of a state. Per observation, with (R, t) its camera's pose and X its point:
 *   y_k = R[k][0]*X_0 + R[k][1]*X_1 + R[k][2]*X_2 + t[k]
 *   if y_2 > 0:  a = y_0 / y_2;  b = y_1 / y_2;  dx = fx * (a - bx);  dy = fy * (b - by);  e = dx*dx + dy*dy;
 *                the term is e if e <= tt, else tt;  otherwise (also for a NaN) the term is tt.
 * The observation is active iff y_2 > 0 and e <= tt. The cost is the sum of the terms: 256 partials from 0.0, partial
 * L over the slots i = L, L + 256, ... ascending and within a slot over the cameras ascending (existing observations
 * only), then the tree P[L] = P[L] + P[L + step], step = 128..1.
 *
 * Trial r = 1..rounds, from the current state, damping lambda (first the option's) and D = 1.0 + lambda:
 * 1. Rows. For each active observation: iz = 1.0 / y_2; a = y_0*iz; b = y_1*iz; fd_pnp_refit's rows of seven
 *      jx = [fx * -(a*b), fx * (1.0 + a*a), fx * -b, fx * iz, 0.0, fx * -(a*iz), fx * (a - bx)]
 *      jy = [fy * -(1.0 + b*b), fy * (a*b), fy * a, 0.0, fy * iz, fy * -(b*iz), fy * (b - by)]
 *    (left perturbation of the camera; entry 6 is the residual) and the point rows, k = 0..2,
 *      px[k] = fx*iz * (R[0][k] - a*R[2][k]);  py[k] = fy*iz * (R[1][k] - b*R[2][k]).
 * 2. Point blocks. Per point, over the cameras ascending (active observations only), from 0.0:
 *      V[k][l] (k <= l):  acc = acc + px[k]*px[l], then acc = acc + py[k]*py[l];
 *      g[k]:              acc = acc + px[k]*jx[6], then acc = acc + py[k]*jy[6].
 *    Damped diagonal d_k = V[k][k] * D. Adjugate and determinant:
 *      c00 = d1*d2 - V12*V12;  c01 = V02*V12 - V01*d2;  c02 = V01*V12 - V02*d1;
 *      c11 = d0*d2 - V02*V02;  c12 = V01*V02 - d0*V12;  c22 = d0*d1 - V01*V01;
 *      det = d0*c00 + V01*c01 + V02*c02;   I[k][l] = ckl / det (symmetric).
 *    The point is held for the trial when it has fewer than 2 active observations, or unless det is finite and
 *    det > 1e-12 * (d0*d1*d2). A held point is not eliminated and does not move; its active observations still enter
 *    U and g of their cameras, exactly as in fd_pnp_refit.
 *    For an eliminated point and each free camera c that observes it actively:
 *      W_c[r][k] = jx[r]*px[k] + jy[r]*py[k]  (r = 0..5);   Y_c[r][k] = W_c[r][0]*I[0][k] + W_c[r][1]*I[1][k] + W_c[r][2]*I[2][k].
 * 3. Schur system. The free cameras in ascending order number 0..F-1; R = 6 F; row 6 f + r is entry r of free camera
 *    f. For rows a = (c, r) <= b = (d, s), and for the right-hand column b = R (d = c, s = 6), two sums over the points
 *    in ascending slot order, each from 0.0:
 *      u: only if c == d, over the active observations (c, i):  u = u + jx[r]*jx[s], then u = u + jy[r]*jy[s];
 *      e: over the eliminated points i with (c, i) and (d, i) active:
 *         e = e + (Y_c[r][0]*W_d[s][0] + Y_c[r][1]*W_d[s][1] + Y_c[r][2]*W_d[s][2]),   for b = R with g[k] for W_d[s][k].
 *    A[a][b] = (a == b ? u * D : u) - e, mirrored into A[b][a] for b < R: the R x (R + 1) system [S | rhs], S x + rhs = 0.
 * 4. Elimination: fd_ransac's Gaussian elimination with complete pivoting at run-time size R (r = k..R-1 outer,
 *    c = k..R inner, the same strict >, so the first of the largest magnitudes in that order wins and a NaN never
 *    does; the same test best > 1e-12 * p0; row factor f = A[r][k] / A[k][k], A[r][c] = A[r][c] - f*A[k][c]). Back
 *    substitution from y[R] = 1: y[k] = (0.0 - s) / A[k][k], s from 0.0 over c = R, R-1, ..., k+1 (descending, the one
 *    difference from fd_ransac's text: row k's sum then takes each y[c] as it appears). The permutation is undone
 *    giving x; the step is x[j] / x[R], j < R. The trial is invalid if a pivot fails the test or an entry of x or of
 *    the step is not finite. R = 0: there is no system and this step is valid.
 * 5. Update. Free camera f with w = step[6f..6f+2], delta = step[6f+3..6f+5]: fd_pnp_refit's Cayley transform
 *    (its step 3) gives (R', t'); a held camera keeps its twelve doubles. Eliminated point:
 *      v[k] = g[k], then over the free cameras ascending that observe it actively, r = 0..5: v[k] = v[k] + W_c[r][k]*step[6f+r];
 *      X'[k] = X[k] - (I[k][0]*v[0] + I[k][1]*v[1] + I[k][2]*v[2]).
 *    The trial is invalid unless every R', t' and X' is finite.
 * 6. Accept rule: the trial is accepted iff it is valid and its state's cost' < cost. On accept the state and cost'
 *    become current and lambda = lambda * down; otherwise lambda = lambda * up and the state of the last accepted
 *    trial stands for the next trial. All `rounds` trials run.
 *
 * Outputs, from the final current state. out_poses double [batch][cams][12]: a held camera's twelve doubles bit for
 * bit; with no accepted trial all of in_poses, bit for bit. out_points float [batch][p_stride][3] (NULL to skip):
 * (float) of the final double for participating points; every other slot below counts[b] keeps the input bits; slots
 * >= counts[b] are not written. out_inlier uint8 [batch][cams][o_stride] (NULL to skip): 1 for the observations active
 * at the final state, 0 for every other slot below counts[b]; slots >= counts[b] are not written. out_counts int32
 * [batch] (NULL to skip): the ones. out_cost double [batch][2] (NULL to skip): the cost of the given and of the
 * final state. out_rounds int32 [batch] (NULL to skip): the accepted trials. out_poses may be in_poses and out_points
 * may be p_xyz. p_stride 0: out_poses = in_poses, out_counts and out_rounds 0, both out_cost entries 0.0.
 *
 * Device pointers when io_on_device: asynchronous on the context's stream (one kernel, a workgroup per problem),
 * graph-capturable once a first call of the shape has sized the workspace (417 bytes per observation slot and 120 per point slot). Host
 * pointers otherwise: staged through context buffers, complete on return.
 * FD_ERR_INVALID: ctx, opts, in_poses, p_xyz, obs_xy or out_poses NULL; batch < 1; cams outside 1..8; a negative
 * stride; o_stride < p_stride; rounds outside 1..16; threshold not finite or not > 0; a camera value not finite, fx
 * or fy zero; lambda not finite or not > 0; up not finite or not > 1; down outside (0, 1].
 * Not in this call, left for later: per-camera intrinsics, lens distortion (warp or undistort first), intrinsics
 * refinement, more than 8 cameras, observation lists with a match index, Huber or other smooth robust losses,
 * marginalisation priors.
 */
int fd_bundle_adjust(fd_ctx *ctx, int batch, int cams, const fd_ba_opts *opts,
                     const double *in_poses, const uint8_t *cam_fixed,
                     const float *p_xyz, const uint8_t *p_valid, const int32_t *counts, int32_t p_stride,
                     const float *obs_xy, const uint8_t *obs_valid, int32_t o_stride,
                     double *out_poses, float *out_points, uint8_t *out_inlier, int32_t *out_counts,
                     double *out_cost, int32_t *out_rounds, int io_on_device);

/* ---- Image warp by a homography or a camera model (MI355X extension) --------------------------------- */
#define FD_WARP_HOMOGRAPHY 0 /* params: double[9], row-major 3 x 3, fd_ransac's out_model layout */
#define FD_WARP_CAMERA 1     /* params: double[22], below */

typedef struct fd_warp_opts {
    int32_t model;         /* FD_WARP_HOMOGRAPHY or FD_WARP_CAMERA */
    int32_t shared_params; /* 1: one parameter set for every frame; 0: params is [batch][P] */
    int32_t fill;          /* 0..255: value of destination pixels with no source */
} fd_warp_opts;

/*
 * fd_frames_warp -- every pixel of out [batch][out_rows][out_cols] uint8 sampled bilinearly from the frame
 * of frames [batch][rows][cols] uint8 with its index, at the source position a small per-frame model gives:
 * registration of a frame by fd_ransac's homography, and lens undistortion / stereo rectification ahead of
 * fd_points_detect. The reference has no such stage: the contract is this text, a definite sequence. All
 * floating point up to the source position is double, every operation rounded once, no contraction, f64
 * division correctly rounded (fd_ransac's conventions). params: double [batch][P], or [P] for every frame
 * when shared_params; P = 9 or 22.
 *
 * Source position (sx, sy) of destination pixel (x, y) of frame b, x and y converted exactly to double.
 * FD_WARP_HOMOGRAPHY, h = the frame's nine parameters: the map is destination -> source (inverse map):
 *   X = (h0*x + h1*y) + h2;  Y = (h3*x + h4*y) + h5;  W = (h6*x + h7*y) + h8;  sx = X / W;  sy = Y / W
 * There is no test on the sign of W: fd_ransac normalises by its largest entry, so a valid model may have
 * W < 0 everywhere. Consequence: call fd_ransac with q = the previous frame's features and t = the next
 * frame's; its H maps previous-frame pixels to next-frame pixels, so passing out_model as it is warps the
 * next frame onto the previous one. No inversion is needed, and with params_on_device no host round trip.
 * FD_WARP_CAMERA, the 22 parameters in order: the destination (ideal pinhole) intrinsics fxn, fyn, cxn, cyn;
 * r0..r8, row-major, the rotation taking a destination ray to a source-camera ray (the identity for plain
 * undistortion, the transposed rectifying rotation for stereo); the source intrinsics fx, fy, cx, cy; the
 * distortion coefficients k1, k2, p1, p2, k3 (OpenCV's order):
 *   a = (x - cxn) / fxn;  b = (y - cyn) / fyn
 *   X = (r0*a + r1*b) + r2;  Y = (r3*a + r4*b) + r5;  W = (r6*a + r7*b) + r8;  xn = X / W;  yn = Y / W
 *   q2 = xn*xn + yn*yn;  q4 = q2*q2;  q6 = q4*q2
 *   rad = ((1.0 + k1*q2) + k2*q4) + k3*q6;  m = 2.0*(xn*yn)
 *   xd = (xn*rad + p1*m) + p2*(q2 + 2.0*(xn*xn));  yd = (yn*rad + p1*(q2 + 2.0*(yn*yn))) + p2*m
 *   sx = fx*xd + cx;  sy = fy*yd + cy
 * (a depends on the column only and b on the row only: computing them once per column or row gives the same
 * bits.)
 *
 * Sampling, both models: px = (float)sx, py = (float)sy, rounded to nearest. The pixel has a source iff
 * 0 <= px <= (float)(cols - 1) and 0 <= py <= (float)(rows - 1); the test is false on NaN, so W = 0,
 * infinities and NaN parameters all land on "no source". With a source: out = (S(0, 0) + 2^19) >> 20 with
 * fd_flow_lk's raw bilinear sum S on the frame at (px, py) (floor, the fraction truncated to 1/1024, reads
 * clamped to the frame's edge), and mask 1. Without: out = fill, mask 0. Consequences: the identity
 * homography with equal shapes copies the frame bit for bit (a zero fraction gives S = 2^20 I), and an
 * integer translation copies the shifted overlap and fills the rest. A warped frame is what fd_flow_lk and
 * fd_points_refine would read at the same float positions, rounded to a byte.
 *
 * out_mask uint8 [batch][out_rows][out_cols] (NULL to skip). out must not overlap frames. No alignment beyond
 * a byte is asked of frames, out or out_mask, and out_cols may be odd. Each of frames, params and the outputs
 * (out and out_mask together) is a device pointer when its *_on_device flag is set. With all three on the
 * device the call is kernels on the context's stream only: asynchronous and graph-capturable (no workspace
 * is involved). Host frames are staged through the context as fd_pyr_build stages them, host params and
 * outputs through context buffers; a call with any host array is complete on return. out_rows or out_cols
 * 0: nothing is written, and the call succeeds.
 * FD_ERR_INVALID: ctx, opts, frames, params or out NULL; batch, rows or cols < 1; a negative out dimension;
 * model or shared_params outside {0, 1}; fill outside 0..255. Parameter values are never rejected: they are
 * device data, and a bad model gives fill.
 */
int fd_frames_warp(fd_ctx *ctx, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                   const fd_warp_opts *opts, const double *params, int params_on_device,
                   int out_rows, int out_cols, uint8_t *out, uint8_t *out_mask /* NULL to skip */, int out_on_device);

/* ---- Contrast-limited adaptive histogram equalization (MI355X extension) ----------------------------- */
typedef struct fd_equalize_opts {
    int32_t tiles_x;    /* 1..32, <= cols */
    int32_t tiles_y;    /* 1..32, <= rows */
    int32_t clip_milli; /* clip limit x 1000 (OpenCV's clipLimit 3.0 -> 3000); 0: no clipping */
} fd_equalize_opts;

/*
 * fd_frames_equalize -- CLAHE of every frame of frames [batch][rows][cols] uint8 into out of the same shape:
 * the photometric pre-processing stage ahead of fd_points_detect (absolute response thresholds, FAST's fixed
 * intensity threshold) and fd_flow_lk (brightness constancy). The reference has no such stage: the contract is
 * this text. Every quantity is an integer; divisions are floor divisions of non-negative values. Frames are
 * independent.
 *
 * Tiles. Column edges ex[i] = (i*cols)/tiles_x, i = 0..tiles_x; row edges ey[j] likewise with rows and tiles_y.
 * Tile (j, i) covers rows ey[j] .. ey[j+1]-1 and columns ex[i] .. ex[i+1]-1; A is its area. Tiles may differ in
 * size by one row or column; there is no padding and no reflection; tiles <= dimension gives A >= 1.
 *
 * LUT of a tile. h[v] = the number of its pixels equal to v. If clip_milli > 0:
 *   lim = max(1, (clip_milli*A)/256000)   (a 64-bit product);   E = sum of max(h[v]-lim, 0)
 *   h[v] = min(h[v], lim), then h[v] += E/256
 *   r = E % 256; if r > 0: step = 256/r, and h[v] += 1 for every v with v % step == 0 and v/step < r
 * (OpenCV's single redistribution pass: bins may end above lim, as intended). The sum of h is A always.
 *   cdf[v] = h[0] + ... + h[v];   lut[v] = (cdf[v]*255 + A/2) / A
 * so lut is non-decreasing and lut[255] = 255. A call in which any tile has A > 2^24 is refused, which keeps
 * cdf*255 + A/2 below 2^32.
 *
 * Interpolation, separable, in fd_flow_lk's 1/1024 fixed point. Column x, from the edges only: c2[i] =
 * ex[i]+ex[i+1] (twice tile i's centre), p = 2x+1.
 *   p < c2[0]:            i0 = i1 = 0, fx = 0
 *   p >= c2[tiles_x-1]:   i0 = i1 = tiles_x-1, fx = 0
 *   otherwise:            i0 = the largest i with c2[i] <= p, i1 = i0+1,
 *                         fx = ((p - c2[i0])*1024) / (c2[i1] - c2[i0]), so 0 <= fx < 1024
 * Rows likewise: j0, j1, fy. For a pixel with value v:
 *   top = lut[j0][i0][v]*(1024-fx) + lut[j0][i1][v]*fx
 *   bot = lut[j1][i0][v]*(1024-fx) + lut[j1][i1][v]*fx
 *   out = (top*(1024-fy) + bot*fy + 2^19) >> 20        (at most 255*2^20 + 2^19 < 2^32)
 * Consequences: tiles_x = tiles_y = 1 with clip_milli = 0 is plain global histogram equalization; clip_milli = 0
 * with more tiles is unclipped AHE; the output depends only on the frame and the three options, never on the
 * launch shape.
 *
 * No alignment beyond a byte is asked of frames or out, and cols may be odd. out may be exactly frames (in
 * place, host or device); any other overlap is the caller's error and is not detected. frames and out are
 * device pointers when their *_on_device flag is set. Host frames are staged through the context as
 * fd_pyr_build stages them, a host out through a context buffer; a call with a host array is complete on
 * return. The tiles' LUTs (batch*tiles_y*tiles_x*256 bytes) and the axes' interpolation entries live in the
 * context's workspace: with both pointers on the device, and once a call of no smaller footprint has run, the
 * call is kernels on the context's stream only: asynchronous and graph-capturable.
 * FD_ERR_INVALID: ctx, opts, frames or out NULL; batch, rows or cols < 1; tiles_x outside 1..min(32, cols);
 * tiles_y outside 1..min(32, rows); clip_milli < 0; a tile area above 2^24.
 */
int fd_frames_equalize(fd_ctx *ctx, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                       const fd_equalize_opts *opts, uint8_t *out, int out_on_device);

/* ---- Gaussian smoothing and the Gaussian pyramid (MI355X extension) ----------------------------------- */
#define FD_BLUR_MAX_RADIUS 15
typedef struct fd_blur_opts {
    int32_t radius;    /* r in 0..15: the kernel is (2r+1) x (2r+1), separable, symmetric */
    int32_t taps[16];  /* w[0..r] >= 0 with w[0] + 2*(w[1]+...+w[r]) == 256; entries above r ignored */
    int32_t step;      /* 1: same size; 2: every second row and column (pyrDown's decimation) */
} fd_blur_opts;

/*
 * fd_blur_taps -- the integer taps of a Gaussian of standard deviation sigma, into *opts. A host function (no
 * context, no GPU), and the only implementation of this rounding: every binding calls it.
 *   r = radius if radius is in 1..15, otherwise r = min(15, max(1, ceil(3*sigma)))
 *   g[k] = exp(-(k*k) / (2*sigma*sigma)) in double, k = 0..r;   S = g[0] + 2*(g[1] + ... + g[r])
 *   w[k] = floor(256*g[k]/S + 0.5) for k = 1..r;   w[0] = 256 - 2*(w[1] + ... + w[r])
 * opts->radius = r, opts->taps[0..r] = w, the taps above r are 0, opts->step = 1.
 * FD_ERR_INVALID: opts NULL; sigma not finite or <= 0; w[0] < w[1] (the rounding left a dip in the middle).
 */
int fd_blur_taps(double sigma, int radius /* 0: choose */, fd_blur_opts *opts);

/*
 * fd_frames_blur -- every frame of frames [batch][rows][cols] uint8 smoothed by a separable symmetric kernel
 * of integer taps into out [batch][out_rows][out_cols] uint8, out_rows = (rows + step - 1)/step and out_cols
 * likewise: the low-pass ahead of fd_brief_compute (ORB smooths before it compares single samples), and with
 * step 2 one level of a Gaussian pyramid. The reference has no such stage: the contract is this text. Every
 * quantity is an integer. Frames are independent.
 *
 * Border: reflect-101, iterated, so that any dimension works with any radius. For a dimension n and an index i
 * (any integer): refl(i, n) = 0 if n == 1; otherwise p = 2(n-1), m = ((i mod p) + p) mod p (so 0 <= m < p), and
 * refl = m if m < n, else p - m. I(Y, X) below stands for frame[refl(Y, rows)][refl(X, cols)]: a read never
 * crosses into a neighbouring frame of the batch.
 *
 * Output pixel (y, x) is centred on source pixel (Y, X) = (step*y, step*x). With w = taps and r = radius:
 *   h(Y', X) = w[0]*I(Y', X) + sum over k = 1..r of w[k]*(I(Y', X-k) + I(Y', X+k))      0 <= h <= 255*256 = 65280
 *   v        = w[0]*h(Y, X)  + sum over k = 1..r of w[k]*(h(Y-k, X) + h(Y+k, X))        0 <= v <= 255*2^16
 *   out(y, x) = (v + 2^15) >> 16
 * One rounding, at the end; none between the passes (h is kept whole, in 16 bits).
 * Consequences: r = 0 with step 1 is a copy. A constant frame is unchanged. taps {96, 64, 16} with step 2 is
 * (S16 + 128) >> 8 with S16 the sum under the 5 x 5 kernel [1 4 6 4 1] x [1 4 6 4 1] (every tap is 16 times its
 * binomial weight, so v = 256*S16): the arithmetic of OpenCV's pyrDown with its default border, an equality
 * with OpenCV that is not verified here. Taps need not decrease ({0, 128} is legal). The output depends only on
 * the frame and the options, never on the launch shape.
 *
 * No alignment beyond a byte is asked of frames or out, and every dimension may be odd. frames and out are
 * device pointers when their *_on_device flag is set. Host frames are staged through the context as
 * fd_pyr_build stages them, a host out through a context buffer; a call with a host array is complete on
 * return. With both pointers on the device the call is one kernel on the context's stream: asynchronous and
 * graph-capturable (no workspace is involved). out == frames on the same side is refused (a workgroup's halo
 * would be overwritten by its neighbour: there is no in-place call); any other overlap is the caller's error
 * and is not detected.
 * FD_ERR_INVALID: ctx, opts, frames or out NULL; batch, rows or cols < 1; rows or cols > 2^30; radius outside 0..15; a negative tap
 * among w[0..r]; w[0] + 2*(w[1]+...+w[r]) != 256; step not 1 or 2; out == frames on the same side.
 */
int fd_frames_blur(fd_ctx *ctx, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                   const fd_blur_opts *opts, uint8_t *out, int out_on_device);

/*
 * fd_pyr_build_gauss -- fd_pyr_build with a Gaussian in place of the 2 x 2 box: the same packed layout
 * (fd_pyr_layout), staging, alignment rule and errors, so that fd_flow_lk takes the pyramid as it is. Level 0
 * is a copy of the frames. Level l+1 is the top-left (rows_l >> 1) x (cols_l >> 1) block of fd_frames_blur of
 * level l (rows_l x cols_l, reflected at that level's own edges) with radius 2, taps {96, 64, 16} and step 2:
 * for an odd dimension the blur's last row or column is dropped. Padding bytes between the levels are not
 * written.
 */
int fd_pyr_build_gauss(fd_ctx *ctx, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                       int levels, uint8_t *pyr, int pyr_on_device);

/* ---- Line band descriptor (MI355X extension) ---------------------------------------------------------- */
typedef struct fd_line_desc_opts {
    int32_t bands;      /* 1..32 (default 9): bands across the line; the descriptor has dim = 8*bands floats */
    int32_t band_width; /* 1..16 (default 7): rows of one band */
} fd_line_desc_opts;

/*
 * fd_lines_describe -- an LBD-style band descriptor (after Zhang & Koch's line band descriptor) of every
 * segment of lines [batch][stride][line_floats] over frames [batch][rows][cols] uint8, so that the segments of
 * fd_lsd_lines can be matched by fd_nn_match / fd_nn_match_guided as they are (dim = 8*bands is a multiple of
 * 4, at most 256). The reference has no such stage: the contract is this text. Per-pixel work is in integers;
 * everything else is in double, IEEE round-to-nearest, no contraction, one rounding per written operation, in
 * the order written. Lines and frames are independent.
 *
 * Floats 0..3 of a line are (sx, sy, ex, ey), each converted to double; line_floats is 4, or 12 so that an
 * array of fd_lsd_rect passes as it is. w = band_width, H = bands*w.
 *
 * Per line.
 *   dx = ex - sx;  dy = ey - sy;  L = sqrt(dx*dx + dy*dy)
 *   c  = ((sx + ex)*0.5, (sy + ey)*0.5)
 *   The line is invalid if one of the four floats is not finite or if L >= 1 is false. Otherwise
 *   dL = (dx/L, dy/L);  n = (-dL.y, dL.x)
 *   dLq = (rint(dL.x*16384), rint(dL.y*16384)) as integers (round half to even);  nq = (-dLq.y, dLq.x)
 *   N = min(floor(L), 4096)   (>= 1) samples along the line, H rows across it.
 *
 * Sample (i, j), 0 <= i < N, 0 <= j < H.
 *   a = i - (N - 1)*0.5;  b = j - (H - 1)*0.5                    (exact)
 *   x = c.x + (a*dL.x + b*n.x);  y = c.y + (a*dL.y + b*n.y)
 *   px = floor(x + 0.5);  py = floor(y + 0.5)
 *   A sample with 1 <= px <= cols - 2 and 1 <= py <= rows - 2 false contributes nothing. Otherwise, with I the frame,
 *   gx = I(py, px+1) - I(py, px-1);  gy = I(py+1, px) - I(py-1, px)
 *   gp = gx*nq.x + gy*nq.y;  gl = gx*dLq.x + gy*dLq.y             (integers, |.| < 2^23)
 * Row sums, exact integers (they pass 2^32): v[j][0] = sum_i max(gp, 0), v[j][1] = sum_i max(-gp, 0), v[j][2]
 * and v[j][3] the same of gl. S = sum_j (v[j][0] - v[j][1]), the sum of every gp.
 *
 * Orientation. If S < 0 the row sums are replaced by those of the reversed segment, r[j][m] = v[H-1-j][m^1]
 * (rows reversed, v0 <-> v1, v2 <-> v3); otherwise r = v. The sample grid is symmetric about c and (-a)*(-dL.x)
 * has the bits of a*dL.x, so r is what the call computes for (ex, ey, sx, sy) whenever S != 0: the descriptor
 * does not depend on the order of the endpoints, bit for bit. (Against the unreversed descriptor, the band
 * order is reversed and the components of each group of four are swapped in pairs.)
 *
 * Bands. Row j has the global weight G[j] = H - |2j - (H - 1)|. Band k, 0 <= k < bands, is formed from the rows
 * of bands k-1, k, k+1 that exist: local index t = 0 .. 3w-1 stands for row j = (k-1)*w + t, skipped unless
 * 0 <= j < H; its local weight is l[t] = 3w - |2t - (3w - 1)|; n_rows = the rows not skipped. For component m
 * of 0..3, over t ascending:
 *   u[t] = (double)(G[j]*l[t]*r[j][m])                             (an exact integer below 2^53)
 *   mean = (sum_t u[t]) / n_rows;   std = sqrt((sum_t (u[t] - mean)*(u[t] - mean)) / n_rows)
 * (sums start at 0.0). The raw descriptor is D[8k + m] = mean, D[8k + 4 + m] = std.
 *
 * Normalisation. For the 4*bands means (indices 8k + m) and then for the 4*bands stds (8k + 4 + m), each group in
 * ascending index order: s = sum of D[i]*D[i]; q = sqrt(s); if q > 0, D[i] = min(D[i] / q, 0.4); a group with
 * q == 0 stays zero. Then over all 8*bands indices ascending: s = sum of D[i]*D[i]; q = sqrt(s); out_desc[i] =
 * (float)(D[i] / q), one rounding. If both groups have q == 0 (a flat or empty support region) the line is invalid.
 *
 * Outputs, for slots < counts[b] only (all `stride` with counts NULL; bits 25..31 of a count are ignored and the
 * count is clamped to stride); other slots are not written. out_desc [batch][stride][8*bands]: the descriptor,
 * all zero for an invalid line. out_xy [batch][stride][2], NULL to skip: ((float)c.x, (float)c.y), the midpoint
 * fd_nn_match_guided takes as q_xy / t_xy, or (0, 0) where an endpoint is not finite. out_valid [batch][stride],
 * NULL to skip: 1, or 0 for an invalid line (it passes as fd_nn_match's q_valid / t_valid).
 *
 * frames are device memory when frames_on_device is set; lines, counts and the outputs are device pointers
 * when io_on_device is set, else host arrays staged through the context, and a call with any host array is
 * complete on return. With everything on the device the call is one kernel on the context's stream, allocates
 * nothing, and is graph-capturable. stride == 0: FD_OK, no work.
 * FD_ERR_INVALID: ctx, opts, frames, lines or out_desc NULL; bands outside 1..32; band_width outside 1..16;
 * line_floats not 4 or 12; batch < 1; stride < 0; rows or cols < 3.
 */
int fd_lines_describe(fd_ctx *ctx, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                      const fd_line_desc_opts *opts, const float *lines, int32_t line_floats, const int32_t *counts /* NULL: stride each */,
                      int32_t stride, float *out_desc, float *out_xy /* NULL to skip */, uint8_t *out_valid /* NULL to skip */,
                      int io_on_device);

/* ---- SuperPoint post-processing (the network runs in PyTorch-ROCm) -------------------------------- */
/* NNFeaturePointDetector::Options (nn_feature_point_detector.h:22-31) fields of the heatmap path. */
typedef struct fd_nn_opts {
    int32_t invalid_boundary;     /* kInvalidBoundary, default 3 */
    int32_t min_feature_distance; /* kMinFeatureDistance, default 15 */
    int32_t max_features;         /* kMaxNumberOfDetectedFeatures, default 240 (counts prior features) */
    float min_response;           /* kMinResponse, default 0.1 */
    float max_response;           /* upper bound of the heatmap values: 1.0 for SuperPoint's softmax
                                     probabilities (finer selection keys); a larger value fails the call
                                     (FD_ERR_INVALID). <= min_response or non-finite: no bound assumed */
} fd_nn_opts;

/*
 * fd_nn_select -- CreateMask + SelectKeypointCandidatesFromHeatMap + SelectGoodFeaturesFromCandidates
 * (nn_feature_point_detector.cpp:59-73, 128-155) for a batch of full-resolution heatmaps
 * [batch][rows][cols] (float). Candidates are heatmap values > min_response outside the invalid
 * boundary and the prior boxes; they are visited in the reference's std::multimap order (response
 * descending, equal responses by raster index descending) and kept greedily with the
 * min_feature_distance box rule until max_features (including the priors) exist. out_xy / out_counts
 * as fd_points_detect (new features only, selection order).
 */
int fd_nn_select(fd_ctx *ctx, const float *heatmap, int heatmap_on_device, int batch, int rows, int cols,
                 const fd_nn_opts *opts, const float *prior_xy, const int32_t *prior_counts, float *out_xy,
                 int32_t out_stride, int32_t *out_counts, int outputs_on_device);

/*
 * fd_nn_select_list -- the keypoint-list models (kSuperpointNms / kDiskNms, whose networks run NMS
 * in-graph): CreateMask + ArgSort + DirectlySelectGoodFeaturesWithDescriptors
 * (nn_feature_point_detector.cpp:59-73, 204-230; nn_feature_point_detector_superpoint.cpp:106-109,
 * nn_feature_point_detector_disk.cpp:106-109). Per frame b, counts[b] keypoints (u = x, v = y as int64
 * pairs, [b * cap + i]) with scores [b * cap + i] and optionally descriptor rows
 * cand_desc [(b * cap + i) * desc_dim ...]. Keypoints are visited by descending score; equal scores
 * by descending raster index, then descending list index (SlamOperation::ArgSort is un-vendored: its
 * order of equal scores is parity-unpinned). Masked ones (border, prior boxes) are skipped,
 * the rest kept until max_features (priors included) with the min_feature_distance box rule.
 * out_xy / out_counts as fd_nn_select; out_desc [b * out_stride + k][desc_dim] = the descriptor row
 * of new feature k (new features only, as the reference's `descriptors`). Inputs (keypoints, scores,
 * counts, cand_desc) are device pointers when inputs_on_device; outputs when outputs_on_device.
 */
int fd_nn_select_list(fd_ctx *ctx, const int64_t *keypoints, const float *scores, const int64_t *counts, int64_t cap,
                      int inputs_on_device, int batch, int rows, int cols, const fd_nn_opts *opts,
                      const float *prior_xy, const int32_t *prior_counts, const float *cand_desc, int desc_dim,
                      float *out_desc, float *out_xy, int32_t out_stride, int32_t *out_counts, int outputs_on_device);

/*
 * fd_nn_descriptors -- ExtractDescriptorsForSelectedFeatures (nn_feature_point_detector.cpp:163-193):
 * per feature (x, y) in xy [batch][stride][2] (counts as fd_brief_compute), bilinear samples at
 * (y / 8, x / 8) of each of the `channels` planes of the descriptor map (zero outside
 * [0, map_rows-1) x [0, map_cols-1)), into out [batch][stride][channels]. map_layout
 * FD_MAP_NCHW: [batch][channels][map_rows][map_cols] (the reference's per-channel matrices);
 * FD_MAP_NHWC: [batch][map_rows][map_cols][channels] (channels-last network output, read in place).
 * xy, counts and out are all device pointers when io_on_device, host pointers otherwise.
 */
enum fd_map_layout { FD_MAP_NCHW = 0, FD_MAP_NHWC = 1 };
int fd_nn_descriptors(fd_ctx *ctx, const float *map, int map_on_device, int map_layout, int batch, int channels,
                      int map_rows, int map_cols, const float *xy, const int32_t *counts, int32_t stride, float *out,
                      int io_on_device);

/*
 * fd_nn_bias_relu -- the NN detectors' bias + ReLU after a bias-free convolution, and with pool = 1 the
 * 2x2 / stride-2 max pool that follows (nn.MaxPool2d(2, 2)), in one pass over an NHWC (channels-last)
 * fp16 activation x [n][h][w][c] on the device: y = relu(x + bias[c]) ([n][h][w][c]; may alias x), or
 * its pooled [n][h/2][w/2][c]. Arithmetic as PyTorch's separate half-precision add / ReLU / max-pool ops
 * (the add in float, rounded to half); a NaN sum becomes 0 (torch.relu would keep it).
 * bias: bias_len fp16 values on the device, bias_len == c (FD_ERR_INVALID otherwise); c a multiple of 8;
 * pool needs even h and w; 16-byte aligned pointers. Runs on the context's stream.
 */
int fd_nn_bias_relu(fd_ctx *ctx, const void *x, const void *bias, int64_t bias_len, void *y, int n, int h, int w,
                    int c, int pool);

/*
 * fd_nn_conv3x3_c1 -- the NN encoders' first layer (one input channel, 3x3 filter, stride 1, zero padding
 * 1; SuperPoint conv1a) with its bias and ReLU, in one pass: y [n][h][w][channels] (channels-last fp16) =
 * relu(conv(x) + bias) for x [n][h][w] fp16 and weight [channels][1][3][3] fp16, all on the device. The
 * convolution sums its 9 products in float (FMA, tap order) and rounds to half; the bias is then added in
 * float and rounded (as a bias-free convolution followed by fd_nn_bias_relu). channels in {8, 16, 32, 64,
 * 128, 256}; w <= 4096; y 16-byte aligned. Runs on the context's stream.
 */
int fd_nn_conv3x3_c1(fd_ctx *ctx, const void *x, const void *weight, const void *bias, int64_t channels, void *y,
                     int n, int h, int w);

/*
 * fd_nn_conv3x3_c64 -- a 3x3 convolution from 64 to 64 channels (stride 1, zero padding 1; SuperPoint
 * conv1b / conv2a / conv2b) with its bias and ReLU and, with pool = 1, the 2x2 / stride-2 max pool, on the
 * matrix cores: x [n][h][w][64] channels-last fp16 -> channels [y_offset, y_offset + 64) of y
 * [n][h][w][y_channels] (or [n][h/2][w/2][y_channels]) fp16, with weight_packed [9 taps (ky, kx)][64 out][64 in]
 * fp16 and bias [64] fp16 (that block of output channels), all on the device; wider outputs (64 -> 128,
 * SuperPoint conv3a) are one call per 64-channel block. fp16 products summed in float; the sum rounded to
 * half, the bias added in float and rounded (as a bias-free convolution followed by fd_nn_bias_relu).
 * x, weight_packed, y 16-byte aligned; y_channels a multiple of 64; pool needs even h, w.
 */
int fd_nn_conv3x3_c64(fd_ctx *ctx, const void *x, const void *weight_packed, const void *bias, void *y, int n, int h,
                      int w, int pool, int y_channels, int y_offset);

/*
 * fd_nn_heat_softmax -- SuperPoint's detector-head output (the network's last stage after convPb:
 * softmax over a cell's 65 channels, the dustbin channel dropped, pixel_shuffle by 8): semi
 * [n][hc][wc][65] channels-last fp16 logits -> heat [n][8 hc][8 wc] float, heat[8i + r][8j + c] =
 * exp(x_{8r+c} - m) / sum_k exp(x_k - m) over the cell's 65 logits x (m their max), in float. bias
 * (optional, 65 fp16): convPb's bias, added to a bias-free convolution's output in half first. All on
 * the device, semi and bias 2-byte, heat 4-byte aligned. Runs on the context's stream.
 */
int fd_nn_heat_softmax(fd_ctx *ctx, const void *semi, const void *bias, float *heat, int n, int hc, int wc);

/*
 * fd_nn_desc_normalize -- SuperPoint's descriptor-head output (after convDb): every cell's c-channel
 * vector divided by max(||x||_2, 1e-12), in float: x [cells][c] fp16 (a channels-last map) -> y
 * [cells][c] float, all on the device; bias (optional, c fp16): convDb's bias, added in half first;
 * c a multiple of 8; x, bias and y 16-byte aligned. Runs on the context's stream.
 */
int fd_nn_desc_normalize(fd_ctx *ctx, const void *x, const void *bias, float *y, int64_t cells, int c);

/* ---- build info --------------------------------------------------------------------------------- */
const char *fd_build_info(void);

/*
 * ABI version of this header: bumped whenever an entry point's parameter list changes or one is removed
 * (5: int64_t bias_len in fd_nn_bias_relu; 6: fd_nn_conv3x3_c1c64 removed -- the fused first layers
 * measured slower than fd_nn_conv3x3_c1 + fd_nn_conv3x3_c64). Bindings compare fd_abi_version() with the FD_ABI_VERSION they were
 * written for and refuse a mismatched library, instead of passing misread arguments.
 */
#define FD_ABI_VERSION 6
int fd_abi_version(void);

/* ---- ingest: pinned, pipelined host frames -> features ------------------------ */
/*
 * A streaming front end for DetectGoodFeatures on host frames (what the reference's callers do per
 * frame after Visualizor2D::LoadImage, test_feature_point_detector.cpp:104-110): `depth` slots, each
 * a pinned host buffer for `batch` frames plus device buffers. fd_ingest_submit copies a slot to the
 * GPU on the ingest's own copy stream and queues detection (fd_points_detect) and the copy-back of
 * the features on the context stream, so the upload of slot i+1 overlaps the detection of slot i.
 * The host fills a slot's frames in place (fd_ingest_frames) and collects its features with
 * fd_ingest_wait; slots are reused round-robin by the caller. One ingest per context at a time (its
 * detections share the context workspace, serialised on the context stream).
 */
typedef struct fd_ingest fd_ingest;
int fd_ingest_create(fd_ctx *ctx, int kind, int batch, int rows, int cols, int depth, uint32_t need,
                     int32_t out_stride, fd_ingest **out);
void fd_ingest_destroy(fd_ingest *ing);
/* pinned host buffer of slot `slot`: batch * rows * cols bytes (GrayImage layout) */
uint8_t *fd_ingest_frames(fd_ingest *ing, int slot);
/* queue slot `slot` (its frames written) with these options; returns without waiting */
int fd_ingest_submit(fd_ingest *ing, int slot, const fd_point_opts *opts);
/* wait for slot `slot`; *xy -> batch * out_stride (x, y) pairs, *counts -> batch new-feature counts
 * (pinned host memory owned by the ingest, valid until the slot is submitted again) */
int fd_ingest_wait(fd_ingest *ing, int slot, const float **xy, const int32_t **counts);

#ifdef __cplusplus
}
#endif

#endif /* FD_HIP_H_ */
