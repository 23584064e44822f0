// Host runtime of libfdhip.so: the LSD stages. fd_lsd_map / fd_lsd_map_pitched (level-line maps,
// fd_lsd.hip) and fd_lsd_lines (compact lists on the GPU, the seed order on a side stream, region growing
// and rectangles on host threads, fd_lines.cpp), with its state read-out.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "fd_ctx.h"
#include "fd_lines.h"

using namespace fdrt;

namespace {

// Shared LSD launch geometry (fd_lsd_map and fd_lsd_lines).
void lsd_geometry(fdk::LsdArgs &a, int batch, int rows, int cols, const uint8_t *dframes) {
    const int work_rows = rows - 3;  // rows [1, rows-3]
    a.frames = dframes;
    a.batch = batch;
    a.rows = rows;
    a.cols = cols;
    a.strips = (cols - 1 + 63) / 64;  // map columns [0, cols-2]
    a.strips4 = (cols - 1 + 255) / 256;
    a.aligned4 = (cols % 4 == 0) && (reinterpret_cast<uintptr_t>(dframes) % 4 == 0);
    a.pitch = cols - 1;  // dense maps: unpitched unless the caller gives a pitch (fd_lsd_map_pitched)
    // k_lsd_map chunks of 32 rows (one row-bit word per (column, chunk)), consecutive waves taking consecutive
    // chunks of a strip: the shortest chunks whose scatter stays on its one-pass path (chunks <= 64 at 1080p);
    // 1080p x256 map + scan + scatter 1.514 -> 1.469 ms against 67-row chunks strip-fastest
    // (profiles/r06_lsd_rows.txt). 16 rows when 32 would leave fewer than 4096 waves (small batches).
    a.chunk_h = static_cast<int64_t>(batch) * a.strips4 * ((work_rows + 31) / 32) < 4096 ? 16 : 32;
    a.chunks = (work_rows + a.chunk_h - 1) / a.chunk_h;
}

// The per-(column, chunk) counts, list bases and row bits of a geometry (LsdArgs::col_cnt / col_base / rowbits).
int lsd_count_buffers(fd_ctx *c, fdk::LsdArgs &a) {
    const size_t ncnt = static_cast<size_t>(a.batch) * (a.cols - 1) * a.chunks;
    FD_HIP_TRY(c, ensure_as(c, c->l_cnt, ncnt, a.col_cnt));
    FD_HIP_TRY(c, ensure_as(c, c->l_base, ncnt, a.col_base));
    FD_HIP_TRY(c, ensure_as(c, c->l_bits, ncnt, a.rowbits));
    return FD_OK;
}

// Row pitch of the library's own (device) dense maps: 16 entries, so every f32 map row starts on a
// 64-byte and every u8 row on a 16-byte boundary and the map kernel's dword / dwordx4 row stores are
// aligned (a 1919-entry row is misaligned on 3 of 4 rows: the vector-memory address unit then splits
// the stores).
int64_t lsd_aligned_pitch(int cols) { return (static_cast<int64_t>(cols) - 1 + 15) / 16 * 16; }

// fd_lsd_lines' seed order (sorted_pixels_, feature_line_detector.cpp:88-94) on a side stream, after
// c->l_ev0 (recorded on the context stream once the compact lists exist): k_select_reference in push
// order over each frame's (norm, map index) list, the orders and statuses copied to c->h_ord / c->h_sst,
// c->l_ev1 recorded after the copies. The context stream does not wait for it: fd_lsd_lines waits on
// l_ev1 before it returns.
int lsd_seed_order(fd_ctx *c, int batch, int map_rows, int map_cols, const std::vector<int64_t> &base,
                   const fdk::LsdArgs &la, int64_t &ord_stride) {
    int64_t cap = 1;
    for (int b = 0; b < batch; ++b) cap = std::max(cap, base[static_cast<size_t>(b) + 1] - base[static_cast<size_t>(b)]);
    if (cap >= (int64_t(1) << 30)) return fail(c, FD_ERR_INVALID, "LSD frame with >= 2^30 valid pixels");
    const size_t nb = static_cast<size_t>(batch);
    fdk::SelectArgs s{};
    FD_HIP_TRY(c, ensure_as(c, c->l_sresp, static_cast<size_t>(cap) * nb, s.list_resp));
    FD_HIP_TRY(c, ensure_as(c, c->l_sidx, static_cast<size_t>(cap) * nb, s.list_idx));
    FD_HIP_TRY(c, ensure_as(c, c->l_sst, 2 * nb, s.status));
    fdk::RefSortArgs r{};
    const int rc = ref_buffers(c, batch, map_rows, map_cols, cap, r);
    if (rc) return rc;
    FD_HIP_TRY(c, ensure_host(c->h_ord, sizeof(uint32_t) * static_cast<size_t>(r.cap) * nb));
    FD_HIP_TRY(c, ensure_host(c->h_sst, sizeof(uint32_t) * nb));
    s.list_cap = cap;
    s.rows = map_rows;
    s.cols = map_cols;
    s.need = 0xFFFFFFFFu;
    s.cand_n = s.status + batch;
    // (no multi-workgroup prelude: every frame is sorted, all workgroups are busy anyway, and the ~30
    // prelude launches cost more than its first levels save: seed orders 0.35-0.6 ms after the lists
    // instead of 0.58-0.87, profiles/r05_lines_seed_order.txt; FD_LSD_WIDE=1: with it, A/B)
    bool wide = false;
    if (const char *e = ab_env("FD_LSD_WIDE")) wide = std::atoi(e) != 0;
    FD_HIP_TRY(c, hipStreamWaitEvent(c->aux, c->l_ev0, 0));
    // order_only never reads ord back: the kernel may write it straight into the pinned host buffer
    // (FD_LSD_ORD_MAPPED=0: a device buffer and a copy, A/B)
    const char *mapped_env = ab_env("FD_LSD_ORD_MAPPED");
    const bool mapped = !mapped_env || std::atoi(mapped_env) != 0;
    if (mapped) {
        void *dp = nullptr;
        FD_HIP_TRY(c, hipHostGetDevicePointer(&dp, c->h_ord.p, 0));
        r.ord = static_cast<uint32_t *>(dp);
    }
    FD_HIP_TRY(c, fdk::launch_lsd_seed_order(la.frame_base, la.idx, la.lnorm, s, r, batch, wide, c->aux));
    if (!mapped)
        FD_HIP_TRY(c, hipMemcpyAsync(c->h_ord.p, r.ord, sizeof(uint32_t) * static_cast<size_t>(r.cap) * nb,
                                     hipMemcpyDeviceToHost, c->aux));
    FD_HIP_TRY(c, hipMemcpyAsync(c->h_sst.p, s.status, sizeof(uint32_t) * nb, hipMemcpyDeviceToHost, c->aux));
    FD_HIP_TRY(c, hipEventRecord(c->l_ev1, c->aux));
    ord_stride = r.cap;
    return FD_OK;
}

}  // namespace

extern "C" {

int fd_lsd_map(fd_ctx *c, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols, float min_norm,
               float *norm, float *angle, uint8_t *valid, int32_t *valid_idx, int64_t idx_cap, int64_t *valid_counts,
               int outputs_on_device) {
    return fd_lsd_map_pitched(c, frames, frames_on_device, batch, rows, cols, min_norm, norm, angle, valid,
                              static_cast<int64_t>(cols) - 1, valid_idx, idx_cap, valid_counts, outputs_on_device);
}

int fd_lsd_map_pitched(fd_ctx *c, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                       float min_norm, float *norm, float *angle, uint8_t *valid, int64_t map_pitch, int32_t *valid_idx,
                       int64_t idx_cap, int64_t *valid_counts, int outputs_on_device) {
    int rc = check_shape(c, FD_HARRIS, batch, rows, cols, false);
    if (rc) return rc;
    if (rows < 2 || cols < 2) return fail(c, FD_ERR_INVALID, "LSD needs rows >= 2 and cols >= 2");  // :14
    const int mc = cols - 1;
    if (map_pitch < mc || map_pitch > (int64_t(1) << 29)) return fail(c, FD_ERR_INVALID, "map_pitch must be >= cols-1");
    // device maps: the caller's pitch; host maps: the library's staging maps use the aligned pitch
    const int64_t dpitch = outputs_on_device ? map_pitch : lsd_aligned_pitch(cols);
    if (static_cast<int64_t>(rows - 1) * dpitch >= (int64_t(1) << 29))  // 32-bit byte offsets into a frame's maps
        return fail(c, FD_ERR_INVALID, "LSD frame too large ((rows-1)*pitch must be < 2^29)");
    if (!valid_counts || idx_cap < 0 || (idx_cap > 0 && !valid_idx))
        return fail(c, FD_ERR_INVALID, "bad output arguments");
    FD_HIP_TRY(c, hipSetDevice(c->device));
    const uint8_t *dframes = nullptr;
    if ((rc = stage_frames(c, frames, frames_on_device, batch, rows, cols, dframes))) return rc;
    const size_t nmap = static_cast<size_t>(batch) * (rows - 1) * static_cast<size_t>(dpitch);
    float *dn = nullptr, *da = nullptr;
    uint8_t *dv = nullptr;
    if (outputs_on_device) {
        dn = norm;
        da = angle;
        dv = valid;
    } else {
        if (norm) FD_HIP_TRY(c, ensure_as(c, c->l_norm, nmap, dn));
        if (angle) FD_HIP_TRY(c, ensure_as(c, c->l_angle, nmap, da));
    }
    // (the valid map is needed internally for the ordered scatter)
    if (dv == nullptr) FD_HIP_TRY(c, ensure_as(c, c->l_valid, nmap, dv));

    int32_t *di = valid_idx;
    int64_t *dc = valid_counts;
    if (!outputs_on_device) {
        FD_HIP_TRY(c, ensure_as(c, c->l_idx, static_cast<size_t>(std::max<int64_t>(idx_cap, 1)) * batch, di));
        FD_HIP_TRY(c, ensure_as(c, c->l_counts, batch, dc));
    }
    const int work_rows = rows - 3;  // rows [1, rows-3]
    const int work_cols = cols - 3;  // cols [1, cols-3]
    if (work_rows <= 0 || work_cols <= 0) {  // nothing scanned: all-zero maps
        if (dn) FD_HIP_TRY(c, hipMemsetAsync(dn, 0, sizeof(float) * nmap, c->stream));
        if (da) FD_HIP_TRY(c, hipMemsetAsync(da, 0, sizeof(float) * nmap, c->stream));
        FD_HIP_TRY(c, hipMemsetAsync(dv, 0, nmap, c->stream));
        FD_HIP_TRY(c, hipMemsetAsync(dc, 0, sizeof(int64_t) * batch, c->stream));
    } else {  // k_lsd_map writes every map entry (zeros outside the scanned rows/columns; pitch padding untouched)
        fdk::LsdArgs a{};
        lsd_geometry(a, batch, rows, cols, dframes);
        a.pitch = static_cast<int>(dpitch);
        a.min_norm = min_norm;
        a.norm = dn;
        a.angle = da;
        a.valid = dv;
        if ((rc = lsd_count_buffers(c, a))) return rc;
        a.idx = di;
        a.idx_cap = idx_cap;
        a.counts = dc;
        FD_HIP_TRY(c, fdk::launch_lsd(a, c->stream));
    }
    if (!outputs_on_device) {
        FD_HIP_TRY(c, hipMemcpyAsync(valid_counts, dc, sizeof(int64_t) * batch, hipMemcpyDeviceToHost, c->stream));
        if (idx_cap > 0)
            FD_HIP_TRY(c, hipMemcpyAsync(valid_idx, di, sizeof(int32_t) * idx_cap * batch, hipMemcpyDeviceToHost, c->stream));
        // pitched device maps -> the host's maps (row pitch map_pitch entries)
        const size_t hrows = static_cast<size_t>(batch) * (rows - 1);
        if (norm)
            FD_HIP_TRY(c, hipMemcpy2DAsync(norm, sizeof(float) * map_pitch, dn, sizeof(float) * dpitch, sizeof(float) * mc,
                                           hrows, hipMemcpyDeviceToHost, c->stream));
        if (angle)
            FD_HIP_TRY(c, hipMemcpy2DAsync(angle, sizeof(float) * map_pitch, da, sizeof(float) * dpitch, sizeof(float) * mc,
                                           hrows, hipMemcpyDeviceToHost, c->stream));
        if (valid)
            FD_HIP_TRY(c, hipMemcpy2DAsync(valid, map_pitch, dv, dpitch, mc, hrows, hipMemcpyDeviceToHost, c->stream));
        FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (int b = 0; b < batch; ++b)
            if (valid_counts[b] > idx_cap) return fail(c, FD_ERR_CAPACITY, "idx_cap smaller than the valid pixels");
    } else if (!frames_on_device) {
        FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return FD_OK;
}

int fd_lsd_lines(fd_ctx *c, const uint8_t *frames, int frames_on_device, int batch, int rows, int cols,
                 const fd_lsd_opts *opts, uint32_t needed, fd_lsd_rect *out_rects, int32_t rect_stride,
                 int32_t *out_counts, int threads) {
    int rc = check_shape(c, FD_HARRIS, batch, rows, cols, false);
    if (rc) return rc;
    if (rows < 2 || cols < 2) return fail(c, FD_ERR_INVALID, "LSD needs rows >= 2 and cols >= 2");  // :14
    if (static_cast<int64_t>(rows - 1) * (cols - 1) >= (int64_t(1) << 29))
        return fail(c, FD_ERR_INVALID, "LSD frame too large ((rows-1)*(cols-1) must be < 2^29)");
    if (!opts || !out_counts || rect_stride < 0 || (rect_stride > 0 && !out_rects))
        return fail(c, FD_ERR_INVALID, "bad output arguments");
    if (frames == nullptr) return fail(c, FD_ERR_INVALID, "frames is NULL");
    c->st_idx.clear();
    c->st_norm.clear();
    c->st_angle.clear();
    c->st_used.clear();
    for (int b = 0; b < batch; ++b) out_counts[b] = 0;
    if (needed == 0) return FD_OK;  // :15
    if (c->aux) FD_HIP_TRY(c, hipStreamSynchronize(c->aux));  // (a failed earlier call's seed sort: drained)
    const bool timing = ab_env("FD_LINES_TIMING") != nullptr;  // diagnostic: phase times to stderr
    // FD_LSD_HOST_SORT=1 (A/B): the seed order by std::sort on the host workers instead of the GPU
    const char *host_sort_env = ab_env("FD_LSD_HOST_SORT");
    const bool host_sort = host_sort_env && std::atoi(host_sort_env) != 0;
    bool gpu_seeds = false;
    int64_t ord_stride = 0;
    // Once the seed sort is launched on the side stream it uses the context's shared scratch (the
    // k_select_reference buffers, h_ord): every return from here on drains it first, so that no later
    // call on the context stream races it (the normal path has waited for it already).
    struct AuxDrain {
        hipStream_t s = nullptr;
        ~AuxDrain() {
            if (s) (void)hipStreamSynchronize(s);
        }
    } drain;
    const auto t_start = std::chrono::steady_clock::now();
    FD_HIP_TRY(c, hipSetDevice(c->device));
    const uint8_t *dframes = nullptr;
    if ((rc = stage_frames(c, frames, frames_on_device, batch, rows, cols, dframes))) return rc;
    std::vector<int64_t> base(static_cast<size_t>(batch) + 1, 0);
    if (rows - 3 > 0 && cols - 3 > 0) {
        // GPU: validity counts + row bits and the scans (pass 1-2), then the compact lists (pass 3)
        fdk::LsdArgs a{};
        lsd_geometry(a, batch, rows, cols, dframes);
        a.min_norm = opts->min_valid_gradient_norm;
        if ((rc = lsd_count_buffers(c, a))) return rc;
        FD_HIP_TRY(c, ensure_as(c, c->l_counts, batch, a.counts));
        FD_HIP_TRY(c, ensure_as(c, c->l_fbase, static_cast<size_t>(batch) + 1, a.frame_base));
        FD_HIP_TRY(c, fdk::launch_lsd_count(a, c->stream));
        FD_HIP_TRY(c, hipMemcpyAsync(base.data(), a.frame_base, sizeof(int64_t) * base.size(), hipMemcpyDeviceToHost,
                                     c->stream));
        FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
        const int64_t total = base[static_cast<size_t>(batch)];
        if (total > 0) {
            const size_t sec = (static_cast<size_t>(total) + 63) & ~size_t(63);  // section length (entries)
            FD_HIP_TRY(c, ensure(c, c->l_lists, sizeof(uint32_t) * 3 * sec));
            FD_HIP_TRY(c, ensure_host(c->h_lists, sizeof(uint32_t) * 3 * sec));
            a.idx = as<int32_t>(c->l_lists);
            a.idx_cap = total;
            a.lnorm = reinterpret_cast<float *>(a.idx + sec);
            a.langle = a.lnorm + sec;
            FD_HIP_TRY(c, fdk::launch_lsd_scatter(a, c->stream));
            if (!host_sort) {
                if (!c->aux) FD_HIP_TRY(c, hipStreamCreateWithFlags(&c->aux.p, hipStreamNonBlocking));
                if (!c->l_ev0) FD_HIP_TRY(c, hipEventCreateWithFlags(&c->l_ev0.p, hipEventDisableTiming));
                if (!c->l_ev1) FD_HIP_TRY(c, hipEventCreateWithFlags(&c->l_ev1.p, hipEventDisableTiming));
                FD_HIP_TRY(c, hipEventRecord(c->l_ev0, c->stream));  // the lists exist (k_lsd_scatter + k_lsd_values)
            }
            // the lists back in one transfer (the PCIe-bound copy is enqueued before the seed sort, which
            // runs beside it on the side stream)
            FD_HIP_TRY(c, hipMemcpyAsync(c->h_lists.p, a.idx, sizeof(uint32_t) * 3 * sec, hipMemcpyDeviceToHost, c->stream));
            if (!host_sort) {
                drain.s = c->aux;
                const int rc2 = lsd_seed_order(c, batch, rows - 1, cols - 1, base, a, ord_stride);
                if (rc2) return rc2;
                gpu_seeds = true;
            }
            FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
    } else if (!frames_on_device) {
        FD_HIP_TRY(c, hipStreamSynchronize(c->stream));  // the staging copy reads the caller's buffer
    }
    const auto t_gpu = std::chrono::steady_clock::now();
    // host: region growing + rectangles, frames over worker threads
    std::vector<fdl::FrameList> fl(static_cast<size_t>(batch));
    const size_t sec = (static_cast<size_t>(base[static_cast<size_t>(batch)]) + 63) & ~size_t(63);
    const int32_t *hidx = static_cast<const int32_t *>(c->h_lists.p);
    const float *hn = reinterpret_cast<const float *>(hidx + sec), *ha = hn + sec;
    for (int b = 0; b < batch; ++b) {
        const int64_t o = base[static_cast<size_t>(b)], n = base[static_cast<size_t>(b) + 1] - o;
        fl[static_cast<size_t>(b)] = fdl::FrameList{n ? hidx + o : nullptr, n ? hn + o : nullptr, n ? ha + o : nullptr, n};
    }
    const int64_t n0 = fl[0].n;
    c->st_used.assign(static_cast<size_t>(n0), 0);
    // the workers wait for the GPU's seed orders after their first frame's setup (once per call)
    std::once_flag seeds_once;
    hipError_t seeds_err = hipSuccess;
    auto t_seeds = t_gpu;
    fdl::SeedOrder so{static_cast<const uint32_t *>(c->h_ord.p), ord_stride, static_cast<const uint32_t *>(c->h_sst.p),
                      [&]() {
                          std::call_once(seeds_once, [&]() {
                              seeds_err = hipEventSynchronize(c->l_ev1);
                              t_seeds = std::chrono::steady_clock::now();
                              if (seeds_err != hipSuccess)  // (reported below; the frames sort on the host)
                                  std::memset(c->h_sst.p, 0, sizeof(uint32_t) * static_cast<size_t>(batch));
                          });
                      }};
    fdl::detect_lines(rows, cols, *opts, fl.data(), batch, out_rects, rect_stride, out_counts, c->st_used.data(),
                      threads > 0 ? threads : default_line_threads(), gpu_seeds ? &so : nullptr);
    if (gpu_seeds) {
        so.wait();  // (every worker waited unless none ran a frame) the side stream's work is done
        FD_HIP_TRY(c, seeds_err);
    }
    if (timing) {
        const auto t_end = std::chrono::steady_clock::now();
        int on_gpu = 0;
        for (int b = 0; gpu_seeds && b < batch; ++b) {
            const uint32_t st = static_cast<const uint32_t *>(c->h_sst.p)[b];
            on_gpu += (st & FD_FRAME_RESOLVED) && !(st & (FD_FRAME_UNRESOLVED | FD_FRAME_GUARD));
        }
        std::fprintf(stderr, "[fd_lsd_lines] batch %d: gpu+d2h %.3f ms, host %.3f ms (seed orders there at %.3f), valid "
                             "%lld, seed orders from the gpu %d\n", batch,
                     std::chrono::duration<double, std::milli>(t_gpu - t_start).count(),
                     std::chrono::duration<double, std::milli>(t_end - t_gpu).count(),
                     std::chrono::duration<double, std::milli>(t_seeds - t_gpu).count(),
                     static_cast<long long>(base[static_cast<size_t>(batch)]), on_gpu);
    }
    if (n0 > 0) {
        c->st_idx.assign(fl[0].idx, fl[0].idx + n0);
        c->st_norm.assign(fl[0].norm, fl[0].norm + n0);
        c->st_angle.assign(fl[0].angle, fl[0].angle + n0);
    }
    return FD_OK;
}

int fd_lsd_lines_state(fd_ctx *c, int32_t *idx, float *norm, float *angle, uint8_t *used, int64_t cap, int64_t *n) {
    if (!c || !n || cap < 0) return FD_ERR_INVALID;
    const int64_t m = static_cast<int64_t>(c->st_idx.size());
    *n = m;
    const int64_t w = std::min(m, cap);
    if (w > 0 && (!idx || !norm || !angle || !used)) return fail(c, FD_ERR_INVALID, "bad output arguments");
    for (int64_t k = 0; k < w; ++k) {
        idx[k] = c->st_idx[static_cast<size_t>(k)];
        norm[k] = c->st_norm[static_cast<size_t>(k)];
        angle[k] = c->st_angle[static_cast<size_t>(k)];
        used[k] = c->st_used[static_cast<size_t>(k)];
    }
    return FD_OK;
}

}  // extern "C"
