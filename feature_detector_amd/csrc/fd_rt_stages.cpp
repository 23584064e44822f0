// Host runtime of libfdhip.so: PNG ingest (fd_png.cpp decodes, fd_gray.hip converts), BRIEF compute
// (fd_brief.hip), and the NN stages (selection over heatmaps and keypoint lists, descriptor sampling, the
// SuperPoint layers of fd_nn.hip / fd_nn_act.hip). The matchers are in fd_rt_match.cpp.
#include <algorithm>
#include <cmath>
#include <limits>

#include "fd_ctx.h"
#include "fd_png.h"

using namespace fdrt;

extern "C" {

int fd_png_info(const uint8_t *png, size_t len, int32_t *rows, int32_t *cols, int32_t *channels) {
    fdp::PngInfo in;
    if (fdp::png_info(png, len, in) != fdp::kPngOk) return FD_ERR_INVALID;
    if (rows) *rows = in.rows;
    if (cols) *cols = in.cols;
    if (channels) *channels = in.channels;
    return FD_OK;
}

int fd_png_decode(const uint8_t *png, size_t len, uint8_t *out_gray, size_t cap, int32_t *rows, int32_t *cols) {
    fdp::PngInfo in;
    if (fdp::png_info(png, len, in) != fdp::kPngOk) return FD_ERR_INVALID;
    if (rows) *rows = in.rows;
    if (cols) *cols = in.cols;
    const size_t npx = static_cast<size_t>(in.rows) * in.cols;
    if (!out_gray || cap < npx) return FD_ERR_CAPACITY;
    std::vector<uint8_t> samples(npx * in.channels);
    const int rc = fdp::png_decode(png, len, samples.data(), samples.size(), in);
    if (rc == fdp::kPngCapacity) return FD_ERR_CAPACITY;
    if (rc) return FD_ERR_INVALID;
    const int ch = in.channels;
    for (size_t i = 0; i < npx; ++i) {  // the same conversion as k_rgb_gray (fd_gray.hip)
        const uint8_t *p = samples.data() + i * ch;
        out_gray[i] = ch <= 2 ? p[0]
                              : static_cast<uint8_t>((4899u * p[0] + 9617u * p[1] + 1868u * p[2] + 8192u) >> 14);
    }
    return FD_OK;
}

int fd_png_frames(fd_ctx *c, const uint8_t *const *pngs, const size_t *lens, int n, int rows, int cols,
                  uint8_t *frames_device, int threads) {
    if (!c) return FD_ERR_INVALID;
    if (n < 1 || rows < 1 || cols < 1 || !pngs || !lens || !frames_device) return fail(c, FD_ERR_INVALID, "bad arguments");
    // every image must have the batch geometry; its channel count sets the staging layout (all equal)
    int channels = 0;
    for (int i = 0; i < n; ++i) {
        fdp::PngInfo in;
        if (fdp::png_info(pngs[i], lens[i], in) != fdp::kPngOk)
            return fail(c, FD_ERR_INVALID, "image " + std::to_string(i) + ": not a supported PNG");
        if (in.rows != rows || in.cols != cols)
            return fail(c, FD_ERR_INVALID, "image " + std::to_string(i) + ": size differs from the batch");
        if (i > 0 && in.channels != channels)
            return fail(c, FD_ERR_INVALID, "image " + std::to_string(i) + ": channel count differs from the batch");
        channels = in.channels;
    }
    const size_t per = static_cast<size_t>(rows) * cols * channels;
    if (per * n >= (size_t(1) << 32)) return fail(c, FD_ERR_INVALID, "batch too large (samples >= 4 GiB)");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    // the previous call's upload may still read the pinned staging: wait for the stream first
    FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
    FD_HIP_TRY(c, ensure_host(c->h_png, per * n));
    std::vector<fdp::PngInfo> infos(static_cast<size_t>(n));
    const int rc = fdp::png_decode_batch(pngs, lens, n, static_cast<uint8_t *>(c->h_png.p), per, infos.data(),
                                         threads > 0 ? threads : default_line_threads());
    if (rc) return fail(c, rc == fdp::kPngCapacity ? FD_ERR_CAPACITY : FD_ERR_INVALID, "PNG decode failed");
    uint8_t *src = frames_device;  // gray input: straight into the frames
    if (channels != 1) FD_HIP_TRY(c, ensure_as(c, c->d_png, per * n, src));
    FD_HIP_TRY(c, hipMemcpyAsync(src, c->h_png.p, per * n, hipMemcpyHostToDevice, c->stream));
    if (channels != 1)
        FD_HIP_TRY(c, fdk::launch_rgb_gray(src, channels, frames_device, static_cast<int64_t>(rows) * cols * n, c->stream));
    return FD_OK;
}

int fd_brief_compute(fd_ctx *c, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                     const fd_brief_opts *opts, const float *uv, const int32_t *counts, int32_t stride,
                     uint32_t *out_bits, uint8_t *out_valid, int io_on_device) {
    int rc = check_shape(c, FD_HARRIS, batch, rows, cols, false);
    if (rc) return rc;
    if (!opts || !uv || !out_bits || stride < 0) return fail(c, FD_ERR_INVALID, "bad arguments");
    // pattern_idx_ holds 256 pairs (descriptor_brief.h:36): a longer kLength would read past it
    if (opts->length < 1 || opts->length > 256) return fail(c, FD_ERR_INVALID, "length must be in [1, 256]");
    if (opts->half_patch_size < 0 || opts->half_patch_size > 255)
        return fail(c, FD_ERR_INVALID, "half_patch_size must be in [0, 255]");
    if (opts->sampler != FD_SAMPLE_BILINEAR && opts->sampler != FD_SAMPLE_TRUNCATE)
        return fail(c, FD_ERR_INVALID, "unknown sampler");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    if (stride == 0) return FD_OK;
    const uint8_t *dframes = nullptr;
    if ((rc = stage_frames(c, frames, frames_on_device, batch, rows, cols, dframes))) return rc;
    const size_t slots = static_cast<size_t>(batch) * stride;
    const int nw = (opts->length + 31) / 32;
    fdk::BriefArgs a{};
    a.frames = dframes;
    a.batch = batch;
    a.rows = rows;
    a.cols = cols;
    a.stride = stride;
    a.length = opts->length;
    a.half = opts->half_patch_size;
    a.sampler = opts->sampler;
    HostIo io(c, io_on_device);
    FD_HIP_TRY(c, io.in(uv, 2 * slots, a.uv));
    FD_HIP_TRY(c, io.in(counts, batch, a.counts));
    FD_HIP_TRY(c, io.out_slots(out_bits, slots, nw, a.out_bits));
    FD_HIP_TRY(c, io.out_slots(out_valid, slots, 1, a.out_valid));
    FD_HIP_TRY(c, fdk::launch_brief(a, c->stream));
    if ((rc = io.finish(counts, batch, stride))) return rc;
    if (io_on_device && !frames_on_device) FD_HIP_TRY(c, hipStreamSynchronize(c->stream));  // the host frames must stay valid until copied
    return FD_OK;
}

int fd_nn_select(fd_ctx *c, const float *heatmap, int heatmap_on_device, int batch, int rows, int cols,
                 const fd_nn_opts *opts, const float *prior_xy, const int32_t *prior_counts, float *out_xy,
                 int32_t out_stride, int32_t *out_counts, int outputs_on_device) {
    int rc = check_shape(c, FD_HARRIS, batch, rows, cols);
    if (rc) return rc;
    if (!heatmap) return fail(c, FD_ERR_INVALID, "heatmap is NULL");
    if (!opts || !out_xy || !out_counts || out_stride < 1) return fail(c, FD_ERR_INVALID, "bad output arguments");
    if (opts->invalid_boundary < 0) return fail(c, FD_ERR_INVALID, "invalid_boundary must be >= 0");
    if (opts->max_features < 0) return fail(c, FD_ERR_INVALID, "max_features must be >= 0");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = refuse_sync_under_capture(c, outputs_on_device))) return rc;
    const int64_t npx = static_cast<int64_t>(rows) * cols;
    const float *dheat = heatmap;
    if (!heatmap_on_device) {
        FD_HIP_TRY(c, ensure_as(c, c->n_heat, npx * batch, dheat));
        FD_HIP_TRY(c, hipMemcpyAsync(c->n_heat.p, heatmap, sizeof(float) * npx * batch, hipMemcpyHostToDevice, c->stream));
    }
    PriorInfo pi;
    rc = setup_priors(c, batch, rows, cols, opts->min_feature_distance, prior_xy, prior_counts, pi);
    if (rc) return rc;
    const int64_t cap = npx + 64;
    SelectBufs sb{};
    if ((rc = select_buffers(c, batch, cap, sb))) return rc;
    fdk::HeatArgs h{};
    h.heat = dheat;
    h.batch = batch;
    h.rows = rows;
    h.cols = cols;
    h.blocks_per_frame = fdk::heat_blocks_per_frame(npx);
    h.thr = opts->min_response;
    h.border = opts->invalid_boundary;
    h.mask = pi.mask;
    h.mask_wpr = pi.wpr;
    list_outputs(c, h.list, cap, sb);
    // responses in (thr, max_response] (probabilities: max 1) or (thr, +inf]
    key_map(FD_HARRIS, opts->min_response, nullptr, 0, h.list.key_base, h.list.key_lz);
    h.vmax = std::numeric_limits<float>::infinity();
    const bool bounded = std::isfinite(opts->max_response) && opts->max_response > opts->min_response;
    if (bounded) {
        h.vmax = opts->max_response;
        const uint32_t kmax = host_float_key(opts->max_response) + 1u;
        h.list.key_lz = kmax > h.list.key_base ? __builtin_clz(kmax - h.list.key_base) : 0;
    }
    h.value_flag = sb.pre_count;
    c->sel_dirty = true;  // until k_select is enqueued: it resets the control block
    FD_HIP_TRY(c, fdk::launch_heat_candidates(h, c->stream));
    SelectCall sc(batch, rows, cols, opts->min_feature_distance, static_cast<uint32_t>(opts->max_features), cap,
                  h.list.key_base, h.list.key_lz);
    sc.tie_idx_desc = 1;
    sc.value_flag = true;
    return run_select(c, sc, pi, sb, out_xy, out_stride, out_counts, outputs_on_device, heatmap_on_device);
}

// DirectlySelectGoodFeaturesWithDescriptors (nn_feature_point_detector.cpp:204-230) for the
// keypoint-list models (kSuperpointNms / kDiskNms, nn_feature_point_detector_superpoint.cpp:76-112,
// nn_feature_point_detector_disk.cpp:76-112): k_cand_lists (border dropped) + k_select in descending
// (score, raster index) order + k_nn_pick for the descriptor rows.
int fd_nn_select_list(fd_ctx *c, const int64_t *keypoints, const float *scores, const int64_t *counts, int64_t cap,
                      int inputs_on_device, int batch, int rows, int cols, const fd_nn_opts *opts,
                      const float *prior_xy, const int32_t *prior_counts, const float *cand_desc, int desc_dim,
                      float *out_desc, float *out_xy, int32_t out_stride, int32_t *out_counts, int outputs_on_device) {
    int rc = check_shape(c, FD_HARRIS, batch, rows, cols);
    if (rc) return rc;
    if (!opts || !out_xy || !out_counts || out_stride < 1) return fail(c, FD_ERR_INVALID, "bad output arguments");
    if (opts->invalid_boundary < 0) return fail(c, FD_ERR_INVALID, "invalid_boundary must be >= 0");
    if (opts->max_features < 0) return fail(c, FD_ERR_INVALID, "max_features must be >= 0");
    if (!counts || cap < 0 || cap > 0x7FFFFFFFll) return fail(c, FD_ERR_INVALID, "counts is NULL or cap out of range");
    if (cand_desc && (desc_dim < 1 || !out_desc)) return fail(c, FD_ERR_INVALID, "descriptors need desc_dim >= 1 and out_desc");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    if ((rc = refuse_sync_under_capture(c, outputs_on_device))) return rc;
    if (!inputs_on_device)
        for (int b = 0; b < batch; ++b)
            if (counts[b] < 0 || counts[b] > cap)
                return fail(c, FD_ERR_INVALID, "frame " + std::to_string(b) + ": keypoint count outside [0, cap]");
    if (cap > 0 && (!keypoints || !scores)) return fail(c, FD_ERR_INVALID, "keypoints / scores are NULL");
    const int64_t *dkp = keypoints, *dcnt = counts;
    const float *dsc = scores, *ddesc = cand_desc;
    if (!inputs_on_device) {  // one upload of the whole batch
        const size_t nb = static_cast<size_t>(batch) * static_cast<size_t>(cap);
        FD_HIP_TRY(c, ensure_as(c, c->c_x, 2 * std::max<size_t>(nb, 1), dkp));
        FD_HIP_TRY(c, ensure_as(c, c->c_resp, std::max<size_t>(nb, 1), dsc));
        FD_HIP_TRY(c, ensure_as(c, c->c_counts, batch, dcnt));
        if (nb) {
            FD_HIP_TRY(c, hipMemcpyAsync(c->c_x.p, keypoints, sizeof(int64_t) * 2 * nb, hipMemcpyHostToDevice, c->stream));
            FD_HIP_TRY(c, hipMemcpyAsync(c->c_resp.p, scores, sizeof(float) * nb, hipMemcpyHostToDevice, c->stream));
        }
        FD_HIP_TRY(c, hipMemcpyAsync(c->c_counts.p, counts, sizeof(int64_t) * batch, hipMemcpyHostToDevice, c->stream));
        if (cand_desc && nb) {
            FD_HIP_TRY(c, ensure_as(c, c->n_map, nb * desc_dim, ddesc));
            FD_HIP_TRY(c, hipMemcpyAsync(c->n_map.p, cand_desc, sizeof(float) * nb * desc_dim, hipMemcpyHostToDevice,
                                         c->stream));
        }
    }
    PriorInfo pi;
    rc = setup_priors(c, batch, rows, cols, opts->min_feature_distance, prior_xy, prior_counts, pi);
    if (rc) return rc;
    const int64_t lcap = std::max<int64_t>(cap, 64);
    SelectBufs sb{};
    if ((rc = select_buffers(c, batch, lcap, sb))) return rc;
    fdk::CandInArgs a{};
    a.resp = dsc;
    a.kp = dkp;
    a.counts = dcnt;
    a.stride = cap;
    a.batch = batch;
    a.rows = rows;
    a.cols = cols;
    a.border = opts->invalid_boundary;
    list_outputs(c, a.list, lcap, sb);
    a.list.key_base = host_float_key(-std::numeric_limits<float>::infinity()) - 1u;
    a.list.key_lz = 0;
    a.bad = sb.pre_count;
    c->sel_dirty = true;  // until k_select is enqueued: it resets the control block
    FD_HIP_TRY(c, fdk::launch_cand_lists(a, cap, c->stream));
    SelectCall sc(batch, rows, cols, opts->min_feature_distance, static_cast<uint32_t>(opts->max_features), lcap,
                  a.list.key_base, a.list.key_lz);
    sc.tie_idx_desc = 1;  // equal scores: raster index descending (ArgSort walked from the back; unpinned)
    sc.dup_keys = true;
    sc.grid_at_d0 = true;
    sc.value_flag = true;
    sc.value_msg = "a keypoint outside the frame, a NaN score or a bad keypoint count";
    // selection into device buffers first when the descriptor rows are wanted on the device
    float *sel_xy = out_xy;
    int32_t *sel_cnt = out_counts;
    if (cand_desc && !outputs_on_device) {
        FD_HIP_TRY(c, ensure_as(c, c->n_xy, 2 * static_cast<size_t>(out_stride) * batch, sel_xy));
        FD_HIP_TRY(c, ensure_as(c, c->n_counts, batch, sel_cnt));
    }
    rc = run_select(c, sc, pi, sb, sel_xy, out_stride, sel_cnt, cand_desc ? 1 : outputs_on_device, 1);
    if (rc) return rc;
    if (cand_desc) {
        fdk::NnPickArgs k{};
        k.kp = dkp;
        k.scores = dsc;
        k.counts = dcnt;
        k.stride_in = cap;
        k.desc = ddesc;
        k.dim = desc_dim;
        k.xy = sel_xy;
        k.n_sel = sel_cnt;
        k.out_stride = out_stride;
        k.batch = batch;
        float *dout = out_desc;
        if (!outputs_on_device) FD_HIP_TRY(c, ensure_as(c, c->n_out, static_cast<size_t>(out_stride) * batch * desc_dim, dout));
        k.out = dout;
        FD_HIP_TRY(c, fdk::launch_nn_pick(k, c->stream));
        if (!outputs_on_device) {
            std::vector<uint32_t> st(static_cast<size_t>(batch));
            FD_HIP_TRY(c, hipMemcpyAsync(out_xy, sel_xy, sizeof(float) * 2 * static_cast<size_t>(out_stride) * batch,
                                         hipMemcpyDeviceToHost, c->stream));
            FD_HIP_TRY(c, hipMemcpyAsync(out_counts, sel_cnt, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, c->stream));
            FD_HIP_TRY(c, hipMemcpyAsync(out_desc, dout, sizeof(float) * static_cast<size_t>(out_stride) * batch * desc_dim,
                                         hipMemcpyDeviceToHost, c->stream));
            FD_HIP_TRY(c, hipMemcpyAsync(st.data(), sb.status, sizeof(uint32_t) * batch, hipMemcpyDeviceToHost, c->stream));
            FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
            for (int b = 0; b < batch; ++b)
                if ((rc = frame_status_error(c, st[b], b, sc.value_msg))) return rc;
        }
    }
    if (!inputs_on_device) FD_HIP_TRY(c, hipStreamSynchronize(c->stream));  // host inputs were copy sources
    return FD_OK;
}

int fd_nn_bias_relu(fd_ctx *c, const void *x, const void *bias, int64_t bias_len, void *y, int n, int h, int w, int ch,
                    int pool) {
    if (!c) return FD_ERR_INVALID;
    if (!x || !bias || !y) return fail(c, FD_ERR_INVALID, "bad arguments");
    if (bias_len != ch) return fail(c, FD_ERR_INVALID, "bias length must equal the channel count");
    if (n < 0 || h < 0 || w < 0 || ch <= 0 || ch % 8) return fail(c, FD_ERR_INVALID, "need n, h, w >= 0, c a multiple of 8");
    if (pool && ((h | w) & 1)) return fail(c, FD_ERR_INVALID, "pooling needs even h and w");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(y)) & 15)
        return fail(c, FD_ERR_INVALID, "pointers must be 16-byte aligned");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    FD_HIP_TRY(c, fdk::launch_bias_relu(x, bias, y, n, h, w, ch, pool, c->stream));
    return FD_OK;
}

int fd_nn_heat_softmax(fd_ctx *c, const void *semi, const void *bias, float *heat, int n, int hc, int wc) {
    if (!c) return FD_ERR_INVALID;
    if (!semi || !heat) return fail(c, FD_ERR_INVALID, "bad arguments");
    if (n < 0 || hc < 0 || wc < 0) return fail(c, FD_ERR_INVALID, "need n, hc, wc >= 0");
    if (static_cast<int64_t>(hc) * 8 * wc * 8 >= (int64_t(1) << 31) || hc > 65535 || n > 65535)
        return fail(c, FD_ERR_INVALID, "map too large");
    if (((reinterpret_cast<uintptr_t>(semi) | reinterpret_cast<uintptr_t>(bias)) & 1) || (reinterpret_cast<uintptr_t>(heat) & 3))
        return fail(c, FD_ERR_INVALID, "pointers must be 2-byte (semi, bias) / 4-byte (heat) aligned");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    FD_HIP_TRY(c, fdk::launch_nn_heat_softmax(semi, bias, heat, n, hc, wc, c->stream));
    return FD_OK;
}

int fd_nn_desc_normalize(fd_ctx *c, const void *x, const void *bias, float *y, int64_t cells, int ch) {
    if (!c) return FD_ERR_INVALID;
    if (!x || !y) return fail(c, FD_ERR_INVALID, "bad arguments");
    if (cells < 0 || ch <= 0 || ch % 8) return fail(c, FD_ERR_INVALID, "need cells >= 0 and c a multiple of 8");
    if ((cells + 3) / 4 >= (int64_t(1) << 31)) return fail(c, FD_ERR_INVALID, "too many cells");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(y)) & 15)
        return fail(c, FD_ERR_INVALID, "pointers must be 16-byte aligned");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    FD_HIP_TRY(c, fdk::launch_nn_desc_normalize(x, bias, y, cells, ch, c->stream));
    return FD_OK;
}

int fd_nn_conv3x3_c1(fd_ctx *c, const void *x, const void *weight, const void *bias, int64_t channels, void *y, int n,
                     int h, int w) {
    if (!c) return FD_ERR_INVALID;
    if (!x || !weight || !bias || !y) return fail(c, FD_ERR_INVALID, "bad arguments");
    if (channels < 8 || channels > 256 || channels % 8 || 256 % (channels / 8))
        return fail(c, FD_ERR_INVALID, "channels must be 8, 16, 32, 64, 128 or 256");
    if (n < 0 || h < 0 || w < 0) return fail(c, FD_ERR_INVALID, "need n, h, w >= 0");
    if (static_cast<int64_t>(n) * h >= (int64_t(1) << 31)) return fail(c, FD_ERR_INVALID, "n * h must be < 2^31");
    if (w > 4096) return fail(c, FD_ERR_INVALID, "w must be <= 4096");
    if ((reinterpret_cast<uintptr_t>(y) & 15) || (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(weight) |
                                                  reinterpret_cast<uintptr_t>(bias)) & 1)
        return fail(c, FD_ERR_INVALID, "y must be 16-byte aligned, x / weight / bias 2-byte aligned");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    FD_HIP_TRY(c, fdk::launch_conv3x3_c1_bias_relu(x, weight, bias, y, n, h, w, static_cast<int>(channels), c->stream));
    return FD_OK;
}

int fd_nn_conv3x3_c64(fd_ctx *c, const void *x, const void *weight_packed, const void *bias, void *y, int n, int h,
                      int w, int pool, int y_channels, int y_offset) {
    if (!c) return FD_ERR_INVALID;
    if (!x || !weight_packed || !bias || !y) return fail(c, FD_ERR_INVALID, "bad arguments");
    if (n < 0 || h < 0 || w < 0) return fail(c, FD_ERR_INVALID, "need n, h, w >= 0");
    if (pool && ((h | w) & 1)) return fail(c, FD_ERR_INVALID, "pooling needs even h and w");
    if (y_channels < 64 || y_channels % 64 || y_offset < 0 || y_offset % 64 || y_offset + 64 > y_channels)
        return fail(c, FD_ERR_INVALID, "y_channels must be a multiple of 64 holding [y_offset, y_offset + 64)");
    if (static_cast<int64_t>(n) * ((h + 7) / 8) * ((w + 31) / 32) >= (int64_t(1) << 31))  // (K10's 8 x 32 tiles)
        return fail(c, FD_ERR_INVALID, "too many tiles");
    if (static_cast<int64_t>(h) * w * 128 >= (int64_t(1) << 31))  // (one frame's input: 32-bit buffer offsets)
        return fail(c, FD_ERR_INVALID, "frame too large (h * w * 64 channels * 2 B must be < 2^31)");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(weight_packed) | reinterpret_cast<uintptr_t>(y)) & 15 ||
        reinterpret_cast<uintptr_t>(bias) & 1)
        return fail(c, FD_ERR_INVALID, "x, weight, y must be 16-byte aligned");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    FD_HIP_TRY(c, fdk::launch_conv3x3_c64(x, weight_packed, bias, y, n, h, w, pool, y_channels, y_offset, c->stream));
    return FD_OK;
}

int fd_nn_descriptors(fd_ctx *c, const float *map, int map_on_device, int map_layout, int batch, int channels,
                      int map_rows, int map_cols, const float *xy, const int32_t *counts, int32_t stride, float *out,
                      int io_on_device) {
    if (!c) return FD_ERR_INVALID;
    if (!map || !xy || !out) return fail(c, FD_ERR_INVALID, "bad arguments");
    if (batch < 1 || channels < 1 || map_rows < 1 || map_cols < 1 || stride < 0)
        return fail(c, FD_ERR_INVALID, "batch, channels, map_rows, map_cols must be >= 1");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    if (stride == 0) return FD_OK;
    const size_t mapn = static_cast<size_t>(batch) * channels * map_rows * map_cols;
    const size_t slots = static_cast<size_t>(batch) * stride;
    if (map_layout != FD_MAP_NCHW && map_layout != FD_MAP_NHWC) return fail(c, FD_ERR_INVALID, "unknown map layout");
    fdk::NnDescArgs a{};
    a.nhwc = map_layout == FD_MAP_NHWC;
    a.batch = batch;
    a.channels = channels;
    a.map_rows = map_rows;
    a.map_cols = map_cols;
    a.stride = stride;
    a.map = map;
    if (!map_on_device) {
        FD_HIP_TRY(c, ensure_as(c, c->n_map, mapn, a.map));
        FD_HIP_TRY(c, hipMemcpyAsync(c->n_map.p, map, sizeof(float) * mapn, hipMemcpyHostToDevice, c->stream));
    }
    HostIo io(c, io_on_device);
    FD_HIP_TRY(c, io.in(xy, 2 * slots, a.xy));
    FD_HIP_TRY(c, io.in(counts, batch, a.counts));
    FD_HIP_TRY(c, io.out_slots(out, slots, channels, a.out));
    FD_HIP_TRY(c, fdk::launch_nn_desc(a, c->stream));
    if (const int rc = io.finish(counts, batch, stride)) return rc;
    if (io_on_device && !map_on_device) FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FD_OK;
}

}  // extern "C"
