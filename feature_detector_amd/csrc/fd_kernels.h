// Kernel argument blocks and the host-side launchers of every kernel file (fd_*.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace fdk {

// Tile geometry of the per-pixel kernels: one wave owns kTileW output columns (lanes 1..62, 4 px
// each; lanes 0 and 63 only supply halo data) and tile_h output rows, walked top to bottom.
constexpr int kTileW = 248;
constexpr int kSegCorner = kTileW / 2;  // strict 4-neighbour NMS: <= 1 candidate per 2 columns
constexpr int kSegFast = kTileW;        // FAST has no NMS
constexpr int kSelectChunk = 2048;      // candidates sorted per greedy chunk (LDS)
constexpr int kSelectThreads = 1024;    // k_select workgroup size (sorted segments: <= this many per frame)
constexpr int kGridLdsCells = 16384;    // occupancy grid kept in LDS up to this many cells
constexpr int kMaxOffsetSegs = 48;
constexpr int kSegHead = 64;           // selection keys kept per sorted segment head (PointsArgs::seghead)
constexpr int kWideKeys = 8192;        // keys per frame of k_select's wide first pass (SelectArgs::wide_keys)
constexpr int kHistBins = 4096;         // level-0 digit of the selection key: top 12 bits of the mapped response

// k_corner_lp tiles: px columns per lane, halo-only lanes per side so that lane 0 / 63 cover the 3
// columns of reach (NMS + 3x3 sum + central difference): 2 lanes at px = 2, else 1.
constexpr int lp_halo_lanes(int px) { return px == 2 ? 2 : 1; }
constexpr int lp_tile_w(int px) { return (64 - 2 * lp_halo_lanes(px)) * px; }

// A raster-mode segment entry (fd_points_candidates only).
struct Cand {
    float resp;
    uint32_t idx;  // row * cols + col
};

// FAST running offset o_k (feature_point_fast_detector.cpp:85,93) as a piecewise-arithmetic table:
// o_k = o_start[s] + (k - k_start[s]) * inc[s], exact in double.
struct FastOffsets {
    int nseg;
    int64_t k0;  // first k with o_k > threshold (score-0 pixels before it are never candidates)
    int64_t k_start[kMaxOffsetSegs];
    double o_start[kMaxOffsetSegs];
    double inc[kMaxOffsetSegs];
    // FAST score of a 16-bit ring mask (bit k = sample k of kFastIndice): the longest circular run of
    // set bits, i.e. the reference's two-pass count (feature_point_fast_detector.cpp:55-78). 64 KiB,
    // device memory owned by the context (build_offsets fills it once).
    const uint8_t *run_lut;
};

// The selection's list format, as a candidate kernel's outputs: unordered per-frame lists (SoA) and the
// level-0 key histogram. The producers write it through fd_emit.h; k_select, k_gather, k_wide_gather and
// k_select_reference read it (SelectArgs names the same arrays).
// Key map: 32-bit key = (float_key(response) - key_base) << key_lz; all candidates have responses >
// min_valid_response, so key_base = float_key(min_valid_response) and key_lz spreads the possible response
// range over the full 32 bits (finer level-0 bins). Level-0 bin = key >> 20 (fd_emit.h: level0_bin).
struct CandList {
    float *resp;      // [batch][cap]
    uint32_t *idx;    // [batch][cap] raster index, row * cols + col
    int64_t cap;      // entries per frame; candidates past it are counted, not stored
    uint32_t *count;  // [batch]
    uint32_t *hist0;  // [batch][kHistBins] or null
    uint32_t key_base;
    int key_lz;
};
static_assert(sizeof(CandList) == 48, "kernel-argument layout");

struct PointsArgs {
    const uint8_t *frames;
    int batch, rows, cols;
    int tiles_x, tiles_y, tile_h;
    int blocks_per_frame;  // workgroups of 4 waves per frame (a workgroup never straddles frames)
    int px;  // corner detect/response: columns per lane of k_corner_lp (2, 4, 8; tile width lp_tile_w), 0 = k_corner
    int aligned4;  // cols % 4 == 0 and 4-byte aligned frames: whole-dword loads are range-exact
    float thr;
    const uint32_t *mask;  // prior-feature bitmap [batch][rows][mask_wpr], bit = mask true; null = all ones
    int mask_wpr;
    CandList list;  // detect mode
    // raster mode: per (frame, row, tile_x) segments
    int32_t *seg_cnt;
    Cand *seg;
    float *resp_map;  // optional full response map (raster mode)
    // masked FAST: k = row_base[f][r] + word_pref[f][r][w] + popcount within the word
    const int32_t *row_base;
    const int32_t *word_pref;
    // Sorted-segment mode (small launches, detect mode with hist0): [batch][blocks_per_frame] (base,
    // count) of each workgroup's bin-sorted list segment; seg_bad[f] set when a tile overflowed its
    // staging (the frame's list is then unsorted). Null = off.
    uint2 *segdesc;
    uint32_t *seg_bad;
    uint64_t *seghead;  // [batch][blocks_per_frame][kSegHead] the segments' first keys (selection keys)
    // FAST emission cut (detect mode, raster tie order): a candidate whose response is
    // below the float *emit_cut (bits; null: none) is counted in skipped[f] instead of emitted; workgroup 0
    // sets *emit_cut_next to +inf, the identity of the selection's proposals for the next call. redo_status:
    // the second pass, where only the frames whose status word has kFrameRedo run (emitting everything).
    const uint32_t *emit_cut;
    uint32_t *emit_cut_next;
    uint32_t *skipped;
    const uint32_t *redo_status;
};
static_assert(offsetof(PointsArgs, list) == 64 && offsetof(PointsArgs, seg_cnt) == 112 && sizeof(PointsArgs) == 208,
              "kernel-argument layout");

// Internal status bit (SelectArgs::status): the selection ran out of emitted keys of a frame whose
// per-pixel pass skipped some (FAST emission cut); the frame is detected and selected again in the same
// call (redo pass), which clears the bit.
constexpr uint32_t kFrameRedo = 0x00000100u;

// (Its list fields are not a CandList: they sit in another order, and the order is the measured one -- a
// reordered block cost the headline 0.16 us and more SGPR spills, profiles/r07_select_chain_ab.txt.)
struct SelectArgs {
    const float *list_resp;
    const uint32_t *list_idx;
    uint32_t *list_count;  // reset to 0 by the kernel once the frame is done
    uint32_t *hist0;       // [batch][kHistBins], reset likewise
    int64_t list_cap;
    int rows, cols;
    const uint32_t *mask;
    int mask_wpr;
    const int32_t *prior_counts;  // device, per frame (null = none)
    uint32_t need;
    int dist;
    int grid_w, grid_h;
    uint32_t *grid_global;  // [batch][grid_w * grid_h] when the grid does not fit LDS (slow path)
    float *out_xy;
    int out_stride;
    int32_t *out_counts;  // plain feature counts (no flag bits)
    // host-output calls in the raster tie order: out_xy / out_counts are pinned host memory and the final
    // status words are mirrored here by finish_frame, so no copy follows the kernel (nullptr: none)
    uint32_t *status_host;
    // [batch] per-frame status (fd_hip.h FD_FRAME_*: tie in the scanned prefix, guard flags) and
    // [batch] candidate count of the frame (kept for a tie resolution after the list count is reset)
    uint32_t *status;
    uint32_t *cand_n;
    uint32_t key_base;  // the key map (CandList)
    int key_lz;
    int tie_idx_desc;  // equal responses by descending raster index (SuperPoint) instead of ascending
    int value_flag;    // pre_count bit 31 set by the candidate kernel -> guard flag 0x40000000 (out of key range)
    // gather kernel (k_gather, batch x gather_groups workgroups) -> first level-0 chunk per frame;
    // null pre_keys: k_select gathers it itself
    uint64_t *pre_keys;   // [batch][kSelectChunk]
    uint32_t *pre_count;  // [batch], reset by k_select
    int gather_groups;
    const uint2 *segdesc;   // the candidate kernel's sorted segments (PointsArgs::segdesc) or null
    const uint64_t *seghead;  // their first kSegHead selection keys (PointsArgs::seghead)
    uint32_t *seg_bad;      // [batch], reset by k_select
    int nseg;               // segments per frame
    uint64_t *wide_keys;  // [batch][kWideKeys] scratch of the wide pass, or null (one list pass per chunk)
    int wide_eager;       // wide pass with the first chunk (FAST) instead of at the first later list pass
    // k_wide_cut + k_wide_gather (batch x wide_groups workgroups of 256 threads, before k_select): the wide pass of a
    // wide_eager frame spread over the frame's list, keys into wide_keys, their number into wide_count
    // (reset by k_select); null wide_count: k_select makes the pass itself, one workgroup per frame
    uint32_t *wide_count;
    uint32_t *wide_cut;  // [batch] k_wide_cut's level-0 bin cut (kHistBins: none), read by k_wide_gather
    int wide_groups;
    // FAST emission cut (PointsArgs::emit_cut): skipped [batch] (reset here), the cut this call used and the
    // word the frames' proposals for the next call go to (atomicMin of float bits); redo_status: the redo
    // pass, in which only frames flagged kFrameRedo run (k_wide_cut / k_wide_gather / k_select)
    uint32_t *skipped;
    const uint32_t *cut_cur;
    uint32_t *cut_next;
    const uint32_t *redo_status;
    int batch;  // frames of the call (the redo pass's workgroups loop over them)
    int grid_at_d0;    // distance 0 still tests the grid (1-pixel cells): caller lists may name a pixel twice
    int dup_keys;      // equal selection keys possible (caller lists): the orderings rank them stably
    uint64_t *stamps;  // diagnostic only (FD_SELECT_STAMPS): per-frame phase clocks, never read back by kernels
};

// Greedy selection over candidates given in an explicit order (FD_TIES_REFERENCE: the reference's
// std::sort permutation of a frame, computed on the host), one workgroup per listed frame.
struct OrderedArgs {
    const uint32_t *order;  // raster indices (row * cols + col), each frame's run in visiting order
    const int64_t *offset;  // [n_frames] start of frame j's run in `order`
    const uint32_t *count;  // [n_frames] its length
    const int32_t *frame;   // [n_frames] frame index (into SelectArgs' per-frame arrays)
};

// Wide prelude of k_select_reference (large frames, launch_select_reference with wide): the push order
// and the first partition levels of the frame's leftmost range, each spread over kRefWideGroups
// workgroups per flagged frame, while that range has more than kRefWideMin elements.
constexpr int kRefWideLevels = 8;
constexpr int kRefWideGroups = 32;
constexpr int kRefWideSlots = 32;  // flagged frames in flight per prelude kernel (more: each workgroup loops)
constexpr uint32_t kRefWideMin = 8192;
struct RefCtl {  // per frame, written by the prelude, read by k_select_reference
    uint32_t n, nlev, bad;
    uint32_t h[kRefWideLevels + 1], dep[kRefWideLevels + 1], act[kRefWideLevels + 1];  // level l: range [0, h[l])
    uint32_t sib_lo[kRefWideLevels], sib_hi[kRefWideLevels];  // level l's right child [sib_lo, sib_hi), depth dep[l] - 1
    uint32_t ch, pv, nL, nR, chL, chR;  // the current level's pivot position / response bits, stopper counts, ranks of ch
    uint2 x0, xch;                      // its elements at 0 and ch before the pivot swap
};

// k_select_reference (FD_TIES_REFERENCE on the GPU): per-frame scratch of cap entries each (cap >= the
// list capacity and >= rows * cols / 32: the raster-order bitmap and its word prefix live in lpos / rpos).
struct RefSortArgs {
    uint2 *x;        // [batch][cap] (response bits, raster index) in push order, partitioned in place
    uint32_t *lpos;  // [batch][cap] left-stopper positions by rank (per level)
    uint32_t *rpos;  // [batch][cap] right-stopper positions by rank
    uint32_t *ord;   // [batch][cap] the reference's visiting order (raster indices) of the finalised prefix
    int64_t cap;
    int push_order;  // the list is already in push order (fd_points_select); else unique raster indices
    uint32_t *dbg;   // [batch][8] first broken invariant per frame (FD_REF_DEBUG), or null
    RefCtl *ctl;     // [batch] wide prelude state (launch_select_reference with wide), else unused
    uint32_t *wcnt;  // [batch][kRefWideGroups][2] per-workgroup counts of the prelude
    uint32_t *wfr;   // [1 + batch] the prelude's compact list: count, flagged frames
    int wide;        // set by the launcher: the prelude ran (push order and the first levels are done)
    int order_only;  // the visiting order alone (ord, every window; no greedy, no outputs): LSD seed order
    int guard_limit;  // iterations of the window x level loop before the frame is failed (0: 1 << 16); diagnostic override
};

// fd_points_select: caller candidates (response, x, y at [f * stride], counts[f]) -> list format.
struct CandInArgs {
    const float *resp;
    const int32_t *x, *y;
    const int64_t *counts;  // [batch] (device)
    int64_t stride;
    int batch, rows, cols;
    CandList list;
    uint32_t *bad;  // [batch] bit 31: a candidate outside the frame, a NaN response or a bad count
    // keypoint-list models (fd_nn_select_list): (u, v) int64 pairs instead of x / y, and candidates
    // within `border` of the frame edge dropped (CreateMask's zero rows/cols). The list is then
    // appended to (unordered; the selection orders equal scores by raster index, tie_idx_desc).
    const int64_t *kp;
    int border;  // < 0: keep push order at list position i (fd_points_select)
};
static_assert(offsetof(CandInArgs, list) == 56 && offsetof(CandInArgs, bad) == 104 && sizeof(CandInArgs) == 128,
              "kernel-argument layout");

// fd_nn_select_list: descriptor rows of the selected keypoints. Per (frame f, feature k), the
// candidate at that pixel visited first by the selection (highest score, then highest index).
struct NnPickArgs {
    const int64_t *kp;      // [batch][stride_in][2]
    const float *scores;    // [batch][stride_in]
    const int64_t *counts;  // [batch]
    int64_t stride_in;
    const float *desc;      // [batch][stride_in][dim]
    int dim;
    const float *xy;        // [batch][out_stride][2] selected features
    const int32_t *n_sel;   // [batch]
    int out_stride;
    int batch;
    float *out;             // [batch][out_stride][dim]
};

struct CompactArgs {
    const int32_t *seg_cnt;
    const Cand *seg;
    int rows, cols, tiles_x, seg_cap, row_lo, row_hi;  // segment rows [row_lo, row_hi)
    float *out_resp;
    int32_t *out_x, *out_y;
    int64_t cap;
    int64_t *out_counts;
};

struct LsdArgs {
    const uint8_t *frames;
    int batch, rows, cols;
    int strips, chunks, chunk_h;
    int strips4;   // k_lsd_map strips of 256 columns (4 per lane); strips: 64-column strips
    int aligned4;  // cols % 4 == 0 and 4-byte aligned frames: whole-dword row loads
    float min_norm;
    float *norm, *angle;
    uint8_t *valid;
    int pitch;          // dense maps: entries per map row (>= cols-1; a multiple of 4 keeps the row stores aligned)
    uint32_t *rowbits;  // [batch][chunks][cols-1]: valid rows of each (column, chunk), bit r - r0 (chunk_h <= 32;
                        // column fastest: a wave's stores and loads are contiguous)
    int32_t *col_cnt;   // [batch][chunks][cols-1]
    int32_t *col_base;  // same size; only the chunk-0 row is written: per column, the exclusive scan of the
                        // columns' totals (all chunks) in column order, i.e. where the column's run starts in the list
    int32_t *idx;
    int64_t idx_cap;
    int64_t *counts;
    // Compact mode (fd_lsd_lines): no dense maps (norm/angle/valid null); the scatter writes, per valid
    // pixel in scan order, its map index, norm and angle into one list for the whole batch, frame f's
    // run starting at frame_base[f] (exclusive scan of counts, k_lsd_frames). Null = per-frame idx_cap.
    float *lnorm;
    float *langle;
    int64_t *frame_base;
};

struct BriefArgs {
    const uint8_t *frames;
    int batch, rows, cols;
    const float *uv;        // [batch][stride][2] (x, y)
    const int32_t *counts;  // [batch] or null (= stride)
    int stride;
    int length, half, sampler;
    uint32_t *out_bits;  // [batch][stride][ceil(length / 32)]
    uint8_t *out_valid;  // [batch][stride] or null
};

// A frame's count word (detect_points' device counts pass as they are): the count in bits 0..24, the
// guard flags of fd_points_detect above them.
constexpr uint32_t kCountMask = 0x01FFFFFFu;

// What both matchers' kernels take alike: every entry of the "a" set against the "b" set of the same
// frame. Forward pass: a = query, b = train. Cross-check's reverse pass: a = train, b = query, out_idx =
// the reverse table, no other output and no test. Guided matching (fd_*_match_guided): with a_xy / b_xy
// set, a "b" entry is a candidate of an "a" entry only inside the window |dx| <= radius_x, |dy| <= radius_y
// (the reverse pass swaps the two position arrays with the sets; the gate is symmetric). Model-gated
// matching (fd_*_match_model): with a_gate / b_gate set as well, a candidate must also pass the model test
// of fd_match_gate.h on the two entries' gate vectors (the reverse pass swaps them and flips a_is_query).
struct MatchCommon {
    const int32_t *a_counts;  // [batch] or null (= a_stride); bits 25..31 ignored
    const int32_t *b_counts;  // the same of the searched set
    int a_stride, b_stride, batch;
    int32_t *out_idx;     // [batch][a_stride]: best b index that passes the tests, else -1
    int32_t *out_counts;  // [batch] += accepted entries (zeroed by the caller), or null
    const int32_t *rev;   // [batch][b_stride] best a index of every b entry (cross-check), or null
    float max_ratio;      // <= 0: off
    const float *a_xy;    // [batch][a_stride][2] (x, y), or null (both null: no gate)
    const float *b_xy;    // [batch][b_stride][2]
    float radius_x, radius_y;  // the window's half-width / half-height (unused without a gate)
    const double *a_gate;  // [batch][a_stride][4] gate vectors (k_match_gate_vectors), or null (both null: no model)
    const double *b_gate;  // [batch][b_stride][4]
    double gate_tt;        // the model gate's t*t
    int gate_model;        // FD_RANSAC_FUNDAMENTAL (0) or FD_RANSAC_HOMOGRAPHY (1)
    int a_is_query;        // the "a" set is the query set (forward pass)
};

// The model gate's pre-pass: the gate vector (fd_match_gate.h) of every slot of both sets, side 0 the query
// set, side 1 the train set.
struct MatchGateArgs {
    const float *xy[2];   // [batch][stride[i]][2]
    double *out[2];       // [batch][stride[i]][4]
    int stride[2];
    int batch, model;     // FD_RANSAC_FUNDAMENTAL (0) or FD_RANSAC_HOMOGRAPHY (1)
    const double *m;      // [batch][9], row-major 3 x 3
    double tt;            // t*t
};

// Hamming matcher (fd_match.hip).
struct MatchArgs : MatchCommon {
    const uint32_t *a_bits;  // [batch][a_stride][ceil(length / 32)]
    const uint8_t *a_valid;  // [batch][a_stride] or null (= all valid)
    const uint32_t *b_bits;  // the same two arrays of the searched set
    const uint8_t *b_valid;
    int length;
    int32_t *out_dist;  // [batch][a_stride][2] raw best / second distance (-1: absent), or null
    int max_distance;   // < 0: off
};

// Squared-L2 matcher for float descriptors (fd_nn_match.hip). k_nn_norms first writes n(x) of every
// descriptor of both sets (+inf for one flagged invalid, which is how validity reaches k_nn_match);
// k_nn_match then runs as the Hamming matcher does.
struct NnNormArgs {
    const float *desc[2];     // [batch][stride[i]][dim]
    const uint8_t *valid[2];  // [batch][stride[i]] or null (= all valid)
    const int32_t *counts[2];  // [batch] or null (= stride[i]); bits 25..31 ignored
    float *out[2];            // [batch][stride[i]]; slots >= counts are not written
    int stride[2];
    int batch, dim;
    int vec[2];  // desc[i] is 16-byte aligned (set by the launcher)
};
struct NnMatchArgs : MatchCommon {
    const float *a_desc;  // [batch][a_stride][dim]
    const float *a_norm;  // [batch][a_stride] (k_nn_norms)
    const float *b_desc;  // the same two arrays of the searched set
    const float *b_norm;
    int dim;             // a multiple of 4, 4..256
    float *out_dist;     // [batch][a_stride][2] raw best / second distance (-1: absent), or null
    float max_distance;  // < 0: off
    int b_vec;           // b_desc is 16-byte aligned (set by the launcher)
};

// SuperPoint heatmap -> candidate lists (the K1 list format + level-0 histogram), for K4.
struct HeatArgs {
    const float *heat;  // [batch][rows][cols]
    int batch, rows, cols;
    int blocks_per_frame;
    float thr;
    int border;            // kInvalidBoundary: rows/cols within it are masked out
    const uint32_t *mask;  // prior-feature bitmap (null = none)
    int mask_wpr;
    CandList list;
    float vmax;           // values above it set bit 31 of value_flag[f] (the key map assumes <= vmax)
    uint32_t *value_flag;  // [batch], the selection control block's pre_count words (gather disabled)
};
static_assert(offsetof(HeatArgs, list) == 48 && offsetof(HeatArgs, vmax) == 96 && sizeof(HeatArgs) == 112,
              "kernel-argument layout");

// Bilinear descriptor sampling from the 1/8-resolution descriptor map.
struct NnDescArgs {
    const float *map;  // [batch][channels][map_rows][map_cols], or [batch][map_rows][map_cols][channels] (nhwc)
    int batch, channels, map_rows, map_cols;
    int nhwc;
    const float *xy;        // [batch][stride][2]
    const int32_t *counts;  // [batch] or null (= stride)
    int stride;
    float *out;  // [batch][stride][channels]
};

// Pyramidal Lucas-Kanade tracker (fd_flow.hip): the template comes from pyramid `tmpl`, the search runs in
// `srch` (the backward pass swaps them).
constexpr int kPyrMaxLevels = 6;  // FD_PYR_MAX_LEVELS
struct FlowArgs {
    const uint8_t *tmpl, *srch;  // packed pyramids (fd_pyr_layout)
    int64_t off[kPyrMaxLevels];  // byte offset of every level (fd_pyr_layout without its last entry)
    int batch, rows, cols, levels, stride;
    int r, max_iters;            // half window 1..10
    float eps2;                  // epsilon * epsilon (float)
    float max_error;             // < 0: off
    double tau;                  // (double)min_eigen * 1024.0 * n
    const float *xy;             // [batch][stride][2] (x, y)
    const uint8_t *valid;        // [batch][stride] or null (= all valid)
    int valid_is_status;         // valid holds a status array: only slots equal to 1 are tracked
    const int32_t *counts;       // [batch] or null (= stride); bits 25..31 ignored
    const float *guess;          // as xy, or null (= xy)
    float *out_xy;               // [batch][stride][2]
    uint8_t *out_status;         // [batch][stride]
    float *out_err;              // [batch][stride] or null
};

// k_flow_finish: the forward-backward test (back_status non-null) and the per-frame counts.
struct FlowFinishArgs {
    const float *xy;             // the forward pass's input positions
    uint8_t *status;             // forward status, updated in place (5: failed the round trip)
    const float *back_xy;        // backward result, or null with back_status
    const uint8_t *back_status;
    float fb2;                   // fb_max_dist * fb_max_dist (float)
    const int32_t *counts;
    int batch, stride;
    int32_t *out_counts;         // [batch] += tracked slots (zeroed by the caller), or null
};

// Sub-pixel corner refinement (fd_refine.hip) on the frames [batch][rows][cols]; the per-frame counts come
// from k_flow_finish (FlowFinishArgs without a backward pass).
struct RefineArgs {
    const uint8_t *frames;
    int batch, rows, cols, stride;
    int r, max_iters;            // half window 1..10
    float eps2;                  // epsilon * epsilon (float)
    float max_shift;
    double tau;                  // (double)min_eigen * 1024.0 * (r + 1)^4
    const float *xy;             // [batch][stride][2] (x, y); may be out_xy
    const uint8_t *valid;        // [batch][stride] or null (= all valid)
    const int32_t *counts;       // [batch] or null (= stride); bits 25..31 ignored
    float *out_xy;               // [batch][stride][2]
    uint8_t *out_status;         // [batch][stride]
};

// RANSAC verification (fd_ransac.hip): one block for the three kernels. k_ransac_compact fills corr, cidx,
// n and zeroes best; k_ransac_hyp fills models and raises best; k_ransac_finish writes the outputs.
struct RansacArgs {
    const float *q_xy, *t_xy;    // [batch][q_stride][2], [batch][t_stride][2] (x, y)
    const int32_t *q_counts;     // [batch] or null (= q_stride); bits 25..31 ignored
    const int32_t *match_idx;    // [batch][q_stride] or null (slot i pairs with slot i)
    const uint8_t *pair_valid;   // [batch][q_stride] or null; only a byte equal to 1 takes part
    int batch, q_stride, t_stride;
    int model, hypotheses;       // FD_RANSAC_*; 1..4096
    uint32_t seed;
    double cx, cy, scale;        // the conditioning transform, as doubles of the option floats
    double tt;                   // ((double)threshold * scale)^2
    double *corr;                // [batch][q_stride][4] conditioned (x, y, u, v) of the correspondences, in slot order
    int32_t *cidx;               // [batch][q_stride] a slot's index in corr, or -1
    int32_t *n;                  // [batch] correspondences
    double *models;              // [batch][hypotheses][9] conditioned models
    unsigned long long *best;    // [batch] ((count + 1) << 32) | (0xFFFFFFFF - h) of the best valid hypothesis; 0: none
    double *out_model;           // [batch][9]
    uint8_t *out_inlier;         // [batch][q_stride] or null
    int32_t *out_counts, *out_best;  // [batch] or null
};

// Least-squares refit of a RANSAC model on its inliers (fd_ransac.hip; fd_ransac_refit of include/fd_hip.h).
// k_ransac_compact runs on `r` as it does for fd_ransac (hypotheses, seed, models, out_best unused; r.best is
// zeroed); k_ransac_refit reads r's lists and writes r.out_model, r.out_inlier, r.out_counts.
struct RefitArgs {
    RansacArgs r;
    const double *in_model;      // [batch][9]; may be r.out_model
    const uint8_t *in_inlier;    // [batch][q_stride]; only a byte equal to 1 is a member; may be r.out_inlier
    uint8_t *member;             // [batch][2][q_stride] workspace: membership by list position, current and candidate
    int rounds;                  // 1..4
    int32_t *out_rounds;         // [batch] or null
};

// Pose from a fundamental matrix and triangulation (fd_ransac.hip; fd_pose_recover and fd_triangulate of
// include/fd_hip.h). The pair arrays are fd_ransac's.
struct PoseArgs {
    const float *q_xy, *t_xy;
    const int32_t *q_counts;
    const int32_t *match_idx;
    const uint8_t *pair_valid;
    const uint8_t *in_inlier;    // [batch][q_stride]; only a byte equal to 1 takes part; null (fd_triangulate): all
    const double *in_model;      // fd_pose_recover: F [batch][9]; fd_triangulate: the pose [batch][12]
    int batch, q_stride, t_stride;
    double cam[8];               // fx, fy, cx, cy of the q camera, then of the t camera
    double mm, D;                // (double)min_parallax squared; (double)max_depth
    double *out_pose;            // [batch][12] or null (fd_pose_recover)
    int32_t *out_choice;         // [batch] or null (fd_pose_recover)
    float *out_points;           // [batch][q_stride][3] or null
    uint8_t *out_valid;          // [batch][q_stride] or null
    int32_t *out_counts;         // [batch] or null
};

// Absolute pose from 3-D points (fd_pnp.hip; fd_pnp_ransac and fd_pnp_refit of include/fd_hip.h): one block for
// its kernels. k_pnp_compact fills corr, cidx, n and zeroes best; k_pnp_hyp fills models and raises best;
// k_pnp_finish writes the outputs.
struct PnpArgs {
    const float *p_xyz, *t_xy;   // [batch][q_stride][3], [batch][t_stride][2]
    const uint8_t *p_valid;      // [batch][q_stride] or null; only a byte equal to 1 takes part
    const int32_t *q_counts;     // [batch] or null (= q_stride); bits 25..31 ignored
    const int32_t *match_idx;    // [batch][q_stride] or null (slot i pairs with slot i)
    const uint8_t *pair_valid;   // [batch][q_stride] or null; only a byte equal to 1 takes part
    int batch, q_stride, t_stride;
    int hypotheses;              // 1..4096
    uint32_t seed;
    double cam[4];               // fx, fy, cx, cy of the t image
    double center[3], scale;     // the conditioning of the 3-D points (fd_pnp_refit: 0 and 1)
    double tt;                   // (double)threshold squared
    double *corr;                // [batch][q_stride][5] (Xc, Yc, Zc, bx, by) of the correspondences, in slot order
    int32_t *cidx;               // [batch][q_stride] a slot's index in corr, or -1
    int32_t *n;                  // [batch] correspondences
    double *models;              // [batch][hypotheses][12] camera matrices of the conditioned points
    unsigned long long *best;    // [batch] as RansacArgs::best
    double *out_model;           // [batch][12]
    uint8_t *out_inlier;         // [batch][q_stride] or null
    int32_t *out_counts, *out_best;  // [batch] or null
};

// k_pnp_compact runs on `r` (hypotheses, seed, models, out_best unused); k_pnp_refit reads r's lists and writes
// r.out_model, r.out_inlier, r.out_counts.
struct PnpRefitArgs {
    PnpArgs r;
    const double *in_model;      // [batch][12]; may be r.out_model
    const uint8_t *in_inlier;    // [batch][q_stride]; only a byte equal to 1 is a member; may be r.out_inlier
    uint8_t *member;             // [batch][2][q_stride] workspace: membership by list position, current and candidate
    int rounds;                  // 1..8
    int32_t *out_rounds;         // [batch] or null
};

// 3-D point-set alignment (fd_align.hip; fd_align_ransac and fd_align_refit of include/fd_hip.h): one block for its
// kernels. k_align_compact fills corr, cidx, n and zeroes best; k_align_hyp fills models and raises best;
// k_align_finish writes the outputs.
struct AlignArgs {
    const float *q_xyz, *t_xyz;  // [batch][q_stride][3], [batch][t_stride][3]
    const uint8_t *q_valid;      // [batch][q_stride] or null; only a byte equal to 1 takes part
    const uint8_t *t_valid;      // [batch][t_stride] or null; only a byte equal to 1 takes part
    const int32_t *q_counts;     // [batch] or null (= q_stride); bits 25..31 ignored
    const int32_t *match_idx;    // [batch][q_stride] or null (slot i pairs with slot i)
    const uint8_t *pair_valid;   // [batch][q_stride] or null; only a byte equal to 1 takes part
    int batch, q_stride, t_stride;
    int kind, hypotheses;        // FD_ALIGN_*; 1..4096
    uint32_t seed;
    double tt;                   // (double)threshold squared
    double *corr;                // [batch][q_stride][6] (X, Y) of the correspondences, in slot order
    int32_t *cidx;               // [batch][q_stride] a slot's index in corr, or -1
    int32_t *n;                  // [batch] correspondences
    double *models;              // [batch][hypotheses][13] R, t, s
    unsigned long long *best;    // [batch] as RansacArgs::best
    double *out_model;           // [batch][13]
    uint8_t *out_inlier;         // [batch][q_stride] or null
    int32_t *out_counts, *out_best;  // [batch] or null
};

// k_align_compact runs on `r` (hypotheses, seed, models, out_best unused); k_align_refit reads r's lists and writes
// r.out_model, r.out_inlier, r.out_counts.
struct AlignRefitArgs {
    AlignArgs r;
    const double *in_model;      // [batch][13]; may be r.out_model
    const uint8_t *in_inlier;    // [batch][q_stride]; only a byte equal to 1 is a member; may be r.out_inlier
    uint8_t *member;             // [batch][2][q_stride] workspace: membership by list position, current and candidate
    int rounds;                  // 1..8
    int32_t *out_rounds;         // [batch] or null
};

// fd_align_apply: k_align_apply, one thread per point slot.
struct AlignApplyArgs {
    const double *model;         // [batch][13]
    const float *xyz_in;         // [batch][stride][3]; may be xyz_out
    const uint8_t *valid;        // [batch][stride] or null; only a byte equal to 1 is written
    const int32_t *counts;       // [batch] or null (= stride); bits 25..31 ignored
    int batch, stride;
    float *xyz_out;              // [batch][stride][3]
};

// Windowed bundle adjustment (fd_ba.hip; fd_bundle_adjust of include/fd_hip.h): k_bundle_adjust, one workgroup
// per problem. The workspace holds what a trial's linearisation leaves for its system and update passes.
constexpr int kBaObsDoubles = 52;    // per observation: jx[7], jy[7], W[6][3], Y[6][3], bx, by
constexpr int kBaPointDoubles = 15;  // per point: X of the two states by turns, the inverse's six entries, g[3]
struct BaArgs {
    const double *in_poses;      // [batch][cams][12]; may be out_poses
    const uint8_t *cam_fixed;    // [batch][cams] or null (camera 0 alone is held); a non-zero byte holds the camera
    const float *p_xyz;          // [batch][p_stride][3]; may be out_points
    const uint8_t *p_valid;      // [batch][p_stride] or null; only a byte equal to 1 takes part
    const int32_t *counts;       // [batch] or null (= p_stride); bits 25..31 ignored
    const float *obs_xy;         // [batch][cams][o_stride][2]
    const uint8_t *obs_valid;    // [batch][cams][o_stride] or null; only a byte equal to 1 takes part
    int batch, cams, p_stride, o_stride, rounds;
    double cam[4];               // fx, fy, cx, cy
    double tt;                   // (double)threshold squared
    double lambda, up, down;
    double *obs;                 // workspace [batch][cams][p_stride][kBaObsDoubles]
    double *pts;                 // workspace [batch][p_stride][kBaPointDoubles]
    uint8_t *act;                // workspace [batch][cams][p_stride]: an observation's exists / active / eliminated bits
    double *out_poses;           // [batch][cams][12]
    float *out_points;           // [batch][p_stride][3] or null
    uint8_t *out_inlier;         // [batch][cams][o_stride] or null
    int32_t *out_counts;         // [batch] or null
    double *out_cost;            // [batch][2] or null
    int32_t *out_rounds;         // [batch] or null
};

// Image warp (fd_warp.hip): every destination pixel of out [batch][out_rows][out_cols] sampled from the frames
// [batch][rows][cols] at the position a per-frame model gives (fd_frames_warp of include/fd_hip.h).
struct WarpArgs {
    const uint8_t *frames;
    const double *params;        // [batch][9 | 22], or one set for every frame (shared)
    uint8_t *out, *mask;         // [batch][out_rows][out_cols], any byte alignment; mask null: not written
    int batch, rows, cols, out_rows, out_cols;
    int model, shared, fill;     // FD_WARP_*; fill 0..255
    int tiles;                   // launch_warp's: workgroup columns per destination row
};

// Contrast-limited adaptive histogram equalization (fd_equalize.hip; fd_frames_equalize of include/fd_hip.h).
struct EqualizeArgs {
    const uint8_t *frames;       // [batch][rows][cols], any byte alignment
    uint8_t *out;                // [batch][rows][cols], any byte alignment; may be frames
    uint8_t *luts;               // workspace: [batch][tiles_y][tiles_x][256], dword aligned
    uint32_t *tab;               // workspace: [cols] then [rows] interpolation entries, cell | fraction << 8
    int batch, rows, cols, tiles_x, tiles_y, clip_milli;
    int lanes_log2, chunks, row_split;  // launch_equalize's: lanes per tile row, workgroup columns per row, workgroups per row cell
};

// Separable integer smoothing (fd_blur.hip; fd_frames_blur and fd_pyr_build_gauss of include/fd_hip.h).
constexpr int kBlurTileCols = 128;  // output columns of a workgroup's tile
constexpr int kBlurTileRows = 32;   // output rows of a tile (16 or 8 at small launches: launch_blur)
struct BlurArgs {
    const uint8_t *frames;       // [batch][rows][cols], any byte alignment
    uint8_t *out;                // [batch][out_rows][out_cols], any byte alignment; must not be frames
    int batch, rows, cols;
    // the rows and columns stored: ((rows | cols) + step - 1) / step, or fewer (the pyramid's floor dimensions
    // crop the last row and column of an odd level)
    int out_rows, out_cols;
    int radius, step;            // 0..15; 1 or 2
    int taps[16];                // w[0..radius]; launch_blur zeroes the rest (an instance may run a wider loop)
    int tile_rows, chunks;       // launch_blur's: output rows per workgroup, workgroup columns per output row
};

// Line band descriptor (fd_line_desc.hip; fd_lines_describe of include/fd_hip.h).
struct LineDescArgs {
    const uint8_t *frames;   // [batch][rows][cols]
    const float *lines;      // [batch][stride][line_floats], floats 0..3 = (start.x, start.y, end.x, end.y)
    const int32_t *counts;   // [batch] or null (= stride); bits 25..31 ignored
    float *out_desc;         // [batch][stride][8 * bands]
    float *out_xy;           // [batch][stride][2] midpoints, or null
    uint8_t *out_valid;      // [batch][stride], or null
    int batch, rows, cols, stride, line_floats, bands, band_width;
};

// Launchers (stream-ordered, no allocation, no synchronisation: graph-capturable).
// k_line_desc, one workgroup per line slot
hipError_t launch_line_desc(const LineDescArgs &a, hipStream_t s);
// the three kernels of fd_frames_equalize, in order
hipError_t launch_equalize(EqualizeArgs a, hipStream_t s);
// k_blur, one launch (out_rows or out_cols 0: none)
hipError_t launch_blur(BlurArgs a, hipStream_t s);
hipError_t launch_warp(WarpArgs a, hipStream_t s);
// the three kernels of fd_ransac, in order
hipError_t launch_ransac(const RansacArgs &a, hipStream_t s);
// k_ransac_compact, then k_ransac_refit (all rounds in one launch)
hipError_t launch_ransac_refit(const RefitArgs &a, hipStream_t s);
// k_pose_recover, one workgroup per frame
hipError_t launch_pose_recover(const PoseArgs &a, hipStream_t s);
// a memset of out_counts, then k_triangulate (q_stride >= 1)
hipError_t launch_triangulate(const PoseArgs &a, hipStream_t s);
// k_pnp_compact, k_pnp_hyp, k_pnp_finish
hipError_t launch_pnp_ransac(const PnpArgs &a, hipStream_t s);
// k_pnp_compact, then k_pnp_refit (all rounds in one launch)
hipError_t launch_pnp_refit(const PnpRefitArgs &a, hipStream_t s);
// k_align_compact, k_align_hyp, k_align_finish
hipError_t launch_align_ransac(const AlignArgs &a, hipStream_t s);
// k_align_compact, then k_align_refit (all rounds in one launch)
hipError_t launch_align_refit(const AlignRefitArgs &a, hipStream_t s);
// k_align_apply (stride >= 1)
hipError_t launch_align_apply(const AlignApplyArgs &a, hipStream_t s);
// k_bundle_adjust, every trial in one launch (p_stride >= 1)
hipError_t launch_bundle_adjust(const BaArgs &a, hipStream_t s);
// one pyramid level [batch][rows >> 1][cols >> 1] from the level [batch][rows][cols] below it
hipError_t launch_pyr_down(const uint8_t *src, uint8_t *dst, int batch, int rows, int cols, hipStream_t s);
hipError_t launch_flow_lk(const FlowArgs &a, hipStream_t s);
hipError_t launch_flow_finish(const FlowFinishArgs &a, hipStream_t s);
hipError_t launch_refine(const RefineArgs &a, hipStream_t s);
hipError_t launch_mask_boxes(const float *prior_xy, const int32_t *prior_frame, int n_prior, int dist, int rows,
                             int cols, uint32_t *mask, int mask_wpr, hipStream_t s);
hipError_t launch_fast_mask_scan(const uint32_t *mask, int mask_wpr, int batch, int rows, int cols, int32_t *row_base,
                                 int32_t *word_pref, hipStream_t s);
hipError_t launch_corner(int kind, bool raster, const PointsArgs &a, hipStream_t s);
hipError_t launch_corner_lp_any(int kind, const PointsArgs &a, hipStream_t s);  // k_corner_lp (a.px != 0)
hipError_t launch_fast(bool raster, const PointsArgs &a, const FastOffsets &off, hipStream_t s);
hipError_t launch_select(const SelectArgs &a, int batch, hipStream_t s);  // k_gather (a.pre_keys) / k_wide_gather (a.wide_count) + k_select
hipError_t launch_select_ordered(const SelectArgs &a, const OrderedArgs &o, int n_frames, hipStream_t s);
// libstdc++ std::sort order emulated on the GPU for the frames k_select flagged (FD_FRAME_TIES)
// wide: run the multi-workgroup prelude first (r.ctl, r.wcnt set): frames of >= 1 Mpx
hipError_t launch_select_reference(const SelectArgs &a, const RefSortArgs &r, int batch, bool wide, hipStream_t s);
hipError_t launch_ref_prelude(const SelectArgs &a, const RefSortArgs &r, int batch, hipStream_t s);  // (its wide prelude: fd_select_refw.hip)
// fd_lsd_lines: the reference's seed order (std::sort of the scan-ordered valid list by norm, descending,
// feature_line_detector.cpp:88-94) of every frame into r.ord: the compact lists (frame_base, idx, lnorm)
// into the list format of `a` (push order), then k_select_reference with order_only.
hipError_t launch_lsd_seed_order(const int64_t *frame_base, const int32_t *idx, const float *lnorm, const SelectArgs &a,
                                 const RefSortArgs &r, int batch, bool wide, hipStream_t s);
hipError_t launch_cand_lists(const CandInArgs &a, int64_t max_count, hipStream_t s);
hipError_t launch_nn_pick(const NnPickArgs &a, hipStream_t s);
hipError_t launch_compact(const CompactArgs &a, int batch, hipStream_t s);
hipError_t launch_lsd(const LsdArgs &a, hipStream_t s);
hipError_t launch_lsd_count(const LsdArgs &a, hipStream_t s);    // compact mode: map (counts, row bits) + scans
hipError_t launch_lsd_scatter(const LsdArgs &a, hipStream_t s);  // compact mode: the lists
hipError_t launch_brief(const BriefArgs &a, hipStream_t s);
hipError_t launch_brief_match(const MatchArgs &a, hipStream_t s);
hipError_t launch_match_gate_vectors(const MatchGateArgs &a, hipStream_t s);
hipError_t launch_nn_norms(NnNormArgs a, hipStream_t s);
hipError_t launch_nn_match(NnMatchArgs a, hipStream_t s);
hipError_t launch_heat_candidates(const HeatArgs &a, hipStream_t s);
int heat_blocks_per_frame(int64_t npx);
hipError_t launch_nn_desc(const NnDescArgs &a, hipStream_t s);
// SuperPoint heads: softmax + dustbin drop + pixel_shuffle(8) of the fp16 channels-last logits
// [n][hc][wc][65] into heat [n][8hc][8wc] f32; L2 normalisation of fp16 channels-last cells [cells][c]
// into f32 (c a multiple of 8)
// (bias, optional: the preceding convolution's bias added to its half output first, in half)
hipError_t launch_nn_heat_softmax(const void *semi, const void *bias, float *heat, int n, int hc, int wc, hipStream_t s);
hipError_t launch_nn_desc_normalize(const void *x, const void *bias, float *y, int64_t cells, int c, hipStream_t s);
// (w1, b1 non-null: x is the one-channel frame and conv1a -- 1 -> 64, 3x3, bias, ReLU -- is fused in)
hipError_t launch_conv3x3_c64(const void *x, const void *wpk, const void *bias, void *y, int n, int h, int w, int pool,
                              int y_channels, int y_offset, hipStream_t s);
hipError_t launch_conv3x3_c1_bias_relu(const void *x, const void *wt, const void *bias, void *y, int n, int h, int w,
                                       int c, hipStream_t s);
hipError_t launch_bias_relu(const void *x, const void *bias, void *y, int n, int h, int w, int c, int pool,
                            hipStream_t s);
// Interleaved 8-bit samples (channels 1-4) of npx pixels -> gray frames (fd_gray.hip).
hipError_t launch_rgb_gray(const uint8_t *src, int channels, uint8_t *dst, int64_t npx, hipStream_t s);

}  // namespace fdk
