// Host runtime of libfdhip.so: the selection driver. Buffers of the selection stage (K4), its key map,
// run_select (k_gather + k_select, the reference tie order's pass, host outputs), the host fallback of the
// reference tie order and the selection's diagnostics. Shared by the point detectors (fd_rt_points.cpp),
// the NN stages (fd_rt_stages.cpp) and fd_lsd_lines' seed order (fd_rt_lsd.cpp).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "fd_ctx.h"

namespace fdrt {

int select_buffers(fd_ctx *c, int batch, int64_t cap, SelectBufs &sb) {
    FD_HIP_TRY(c, ensure(c, c->list_resp, sizeof(float) * cap * batch));
    FD_HIP_TRY(c, ensure(c, c->list_idx, sizeof(uint32_t) * cap * batch));
    FD_HIP_TRY(c, ensure_as(c, c->pre_keys, static_cast<size_t>(fdk::kSelectChunk) * batch, sb.pre_keys));
    FD_HIP_TRY(c, ensure_as(c, c->wide_keys, static_cast<size_t>(fdk::kWideKeys) * batch, sb.wide_keys));
    const size_t ctl = sizeof(uint32_t) * static_cast<size_t>(batch) * (fdk::kHistBins + 6);
    if (c->selctl.n < ctl) {
        FD_HIP_TRY(c, ensure(c, c->selctl, ctl));
        c->sel_dirty = true;
    }
    if (c->sel_dirty) {
        FD_HIP_TRY(c, hipMemsetAsync(c->selctl.p, 0, c->selctl.n, c->stream));
        c->sel_dirty = false;
    }
    uint32_t *base = as<uint32_t>(c->selctl);
    sb.hist0 = base;
    sb.list_count = base + static_cast<size_t>(batch) * fdk::kHistBins;
    sb.pre_count = sb.list_count + batch;
    sb.seg_bad = sb.pre_count + batch;
    sb.wide_count = sb.seg_bad + batch;
    sb.wide_cut = sb.wide_count + batch;
    sb.skipped = sb.wide_cut + batch;
    FD_HIP_TRY(c, ensure_as(c, c->status, 2 * static_cast<size_t>(batch), sb.status));
    sb.cand_n = sb.status + batch;
    return FD_OK;
}

uint32_t host_float_key(float f) {
    uint32_t u;
    std::memcpy(&u, &f, sizeof(u));
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

void key_map(int kind, float thr, const fdk::FastOffsets *off, int64_t n_off, uint32_t &base, int &lz) {
    base = host_float_key(thr);
    uint32_t kmax = host_float_key(std::numeric_limits<float>::infinity());
    if (kind == FD_FAST && off && off->nseg > 0 && n_off > 0) {
        const int s = off->nseg - 1;
        const double omax = off->o_start[s] + static_cast<double>(n_off - 1 - off->k_start[s]) * off->inc[s];
        kmax = std::max(base, host_float_key(static_cast<float>(16.0 + omax + 1.0)));
    }
    lz = kmax > base ? __builtin_clz(kmax - base) : 0;
}

int ref_buffers(fd_ctx *c, int batch, int rows, int cols, int64_t cap, fdk::RefSortArgs &r) {
    const int64_t words = (static_cast<int64_t>(rows) * cols + 31) / 32;
    const int64_t rcap = std::max<int64_t>({cap, words, 1});
    const size_t n = static_cast<size_t>(rcap) * static_cast<size_t>(batch);
    FD_HIP_TRY(c, ensure_as(c, c->r_x, n, r.x));
    FD_HIP_TRY(c, ensure_as(c, c->r_lpos, n, r.lpos));
    FD_HIP_TRY(c, ensure_as(c, c->r_rpos, n, r.rpos));
    FD_HIP_TRY(c, ensure_as(c, c->r_ord, n, r.ord));
    FD_HIP_TRY(c, ensure_as(c, c->r_ctl, static_cast<size_t>(batch), r.ctl));
    FD_HIP_TRY(c, ensure_as(c, c->r_wcnt, 2 * fdk::kRefWideGroups * static_cast<size_t>(batch), r.wcnt));
    FD_HIP_TRY(c, ensure_as(c, c->r_wfr, 1 + static_cast<size_t>(batch), r.wfr));
    r.cap = rcap;
    // diagnostic (FD_DEBUG_AB=1): a low bound on k_select_reference's window x level loop, so that tests
    // reach its failure path (FD_FRAME_UNRESOLVED, host fallback) on small inputs
    if (const char *e = ab_env("FD_REF_GUARD")) r.guard_limit = std::max(0, std::atoi(e));
    return FD_OK;
}

int frame_status_error(fd_ctx *c, uint32_t status, int frame, const char *value_msg) {
    if (value_msg && (status & FD_FRAME_VALUE_RANGE))
        return fail(c, FD_ERR_INVALID, "frame " + std::to_string(frame) + ": " + value_msg);
    if (status & FD_FRAME_GUARD) {
        char hex[16];
        std::snprintf(hex, sizeof hex, "%x", status);
        return fail(c, FD_ERR_HIP, std::string("internal: selection consistency guard tripped (status 0x") + hex +
                                       ", frame " + std::to_string(frame) + ")");
    }
    return FD_OK;
}

namespace {

// FD_TIES_REFERENCE (fd_ctx_set_tie_order): frames whose greedy scan met equal responses
// (FD_FRAME_TIES from k_select) are selected again in the reference's own order. The reference sorts
// its raster-ordered candidates with an unstable std::sort (feature_point_detector.cpp:58-60), whose
// permutation of equal responses is defined only by libstdc++'s introsort run on that exact sequence:
// the frame's candidate list (still in the workspace, unordered) is copied back, put in raster order
// (the order ComputeCandidates pushes them, feature_point_harris_detector.cpp:120-137,
// feature_point_fast_detector.cpp:83-98), sorted here with std::sort and the reference comparator,
// and the resulting visiting order goes back to the GPU for the greedy pass (k_select_ordered).
// `which` selects the frames: FD_FRAME_UNRESOLVED (the frames k_select_reference left to the host).
int resolve_ties(fd_ctx *c, fdk::SelectArgs s, int batch, const SelectBufs &sb, bool push_order, uint32_t which) {
    // The status read below synchronises the stream, which a stream being captured into a graph cannot
    // do (and the host sort could not be replayed): refuse before touching the capture.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    FD_HIP_TRY(c, hipStreamIsCapturing(c->stream, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return fail(c, FD_ERR_INVALID, "FD_TIES_REFERENCE synchronises (status read, host std::sort): not allowed "
                                       "during stream capture; use FD_TIES_RASTER and read FD_FRAME_TIES");
    std::vector<uint32_t> st(2 * static_cast<size_t>(batch));
    FD_HIP_TRY(c, hipMemcpyAsync(st.data(), sb.status, sizeof(uint32_t) * st.size(), hipMemcpyDeviceToHost, c->stream));
    FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<int32_t> frames;
    for (int b = 0; b < batch; ++b) {
        // (the guard is read here anyway: reported for device outputs too)
        if (const int rc = frame_status_error(c, st[b], b, nullptr)) return rc;
        if (st[b] & which) frames.push_back(b);
    }
    if (frames.empty()) return FD_OK;
    struct Cand {
        float resp;
        uint32_t idx;
    };
    std::vector<std::vector<Cand>> lists(frames.size());
    std::vector<std::vector<float>> resp(frames.size());
    std::vector<std::vector<uint32_t>> idx(frames.size());
    for (size_t j = 0; j < frames.size(); ++j) {
        const int f = frames[j];
        const size_t n = std::min<size_t>(st[batch + f], static_cast<size_t>(s.list_cap));
        resp[j].resize(n);
        idx[j].resize(n);
        const size_t o = static_cast<size_t>(f) * static_cast<size_t>(s.list_cap);
        FD_HIP_TRY(c, hipMemcpyAsync(resp[j].data(), s.list_resp + o, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
        FD_HIP_TRY(c, hipMemcpyAsync(idx[j].data(), s.list_idx + o, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
    }
    FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<uint32_t> order;
    std::vector<int64_t> offset(frames.size());
    std::vector<uint32_t> count(frames.size());
    for (size_t j = 0; j < frames.size(); ++j) {
        std::vector<Cand> &v = lists[j];
        v.resize(resp[j].size());
        for (size_t i = 0; i < v.size(); ++i) v[i] = {resp[j][i], idx[j][i]};
        // the order ComputeCandidates pushed them in -- raster order for the built-in detectors (their
        // indices are unique; the lists are unordered), the list order for caller-supplied candidates
        // (fd_points_select keeps it) -- then the reference's sort (:58-60)
        // (raster order of unique indices: any sort gives it; an LSD radix sort, 3 x 11 bits, is ~20x
        // faster than std::sort here and leaves the reference's own std::sort below as the cost)
        if (!push_order) {
            std::vector<Cand> tmp(v.size());
            for (int shift = 0; shift < 33; shift += 11) {
                uint32_t hist[2049] = {};
                for (const Cand &e : v) ++hist[((e.idx >> shift) & 2047u) + 1];
                for (int k = 0; k < 2048; ++k) hist[k + 1] += hist[k];
                for (const Cand &e : v) tmp[hist[(e.idx >> shift) & 2047u]++] = e;
                v.swap(tmp);
            }
        }
        std::sort(v.begin(), v.end(), [](const Cand &a, const Cand &b) { return a.resp > b.resp; });
        offset[j] = static_cast<int64_t>(order.size());
        count[j] = static_cast<uint32_t>(v.size());
        for (const Cand &e : v) order.push_back(e.idx);
    }
    const size_t nf = frames.size();
    const size_t meta = (sizeof(int64_t) + sizeof(uint32_t) + sizeof(int32_t)) * nf;
    FD_HIP_TRY(c, ensure(c, c->ord, sizeof(uint32_t) * std::max<size_t>(order.size(), 1)));
    FD_HIP_TRY(c, ensure(c, c->ord_meta, meta));
    std::vector<uint8_t> mbuf(meta);
    std::memcpy(mbuf.data(), offset.data(), sizeof(int64_t) * nf);
    std::memcpy(mbuf.data() + sizeof(int64_t) * nf, count.data(), sizeof(uint32_t) * nf);
    std::memcpy(mbuf.data() + (sizeof(int64_t) + sizeof(uint32_t)) * nf, frames.data(), sizeof(int32_t) * nf);
    FD_HIP_TRY(c, hipMemcpyAsync(c->ord.p, order.data(), sizeof(uint32_t) * order.size(), hipMemcpyHostToDevice, c->stream));
    FD_HIP_TRY(c, hipMemcpyAsync(c->ord_meta.p, mbuf.data(), meta, hipMemcpyHostToDevice, c->stream));
    fdk::OrderedArgs o{};
    o.order = as<uint32_t>(c->ord);
    o.offset = reinterpret_cast<const int64_t *>(c->ord_meta.p);
    o.count = reinterpret_cast<const uint32_t *>(static_cast<uint8_t *>(c->ord_meta.p) + sizeof(int64_t) * nf);
    o.frame = reinterpret_cast<const int32_t *>(static_cast<uint8_t *>(c->ord_meta.p) +
                                                (sizeof(int64_t) + sizeof(uint32_t)) * nf);
    FD_HIP_TRY(c, fdk::launch_select_ordered(s, o, static_cast<int>(nf), c->stream));
    FD_HIP_TRY(c, hipStreamSynchronize(c->stream));  // the host vectors above are the copies' sources
    return FD_OK;
}

// Diagnostics of the selection (FD_SELECT_STAMPS: phase clocks of k_select and k_select_reference, 32 words
// per frame; FD_REF_DEBUG: k_select_reference's broken invariants, 8 words per frame), both in c->dbg.
int diag_words(fd_ctx *c, size_t bytes) {
    FD_HIP_TRY(c, ensure(c, c->dbg, bytes));
    FD_HIP_TRY(c, hipMemsetAsync(c->dbg.p, 0, bytes, c->stream));
    return FD_OK;
}

enum DiagKind { kDiagSelect, kDiagReference, kDiagRefChecks };

// Copies the diagnostic words back (synchronises) and prints them to stderr.
int print_diag(fd_ctx *c, int batch, DiagKind kind) {
    using ull = unsigned long long;
    if (kind == kDiagRefChecks) {
        std::vector<uint32_t> h(static_cast<size_t>(8) * batch);
        FD_HIP_TRY(c, hipMemcpyAsync(h.data(), c->dbg.p, sizeof(uint32_t) * h.size(), hipMemcpyDeviceToHost, c->stream));
        FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (int b = 0; b < batch; ++b)
            if (h[8 * b])
                std::fprintf(stderr, "k_select_reference frame %d: check %u idx %u bound %u m_act %u T %u\n", b, h[8 * b],
                             h[8 * b + 1], h[8 * b + 2], h[8 * b + 3], h[8 * b + 4]);
        return FD_OK;
    }
    std::vector<uint64_t> all(static_cast<size_t>(batch) * 32);
    FD_HIP_TRY(c, hipMemcpyAsync(all.data(), c->dbg.p, sizeof(uint64_t) * all.size(), hipMemcpyDeviceToHost, c->stream));
    FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (kind == kDiagReference) {  // k_select_reference's phase clocks (slots 16-30) of the flagged frames
        for (int b = 0; b < batch; ++b) {
            const uint64_t *q = all.data() + static_cast<size_t>(b) * 32;
            if (!q[18]) continue;
            std::fprintf(stderr, "k_select_reference frame %d cycles: push %llu | levels %llu sumT %llu: pivots %llu "
                                 "pass1 %llu bases %llu pass2 %llu (K) %llu pass3 %llu children %llu | leaves %llu "
                                 "wave-local %llu greedy %llu windows %llu\n", b, (ull)q[16], (ull)q[18], (ull)q[19],
                         (ull)q[24], (ull)q[25], (ull)q[26], (ull)q[27], (ull)q[28], (ull)q[29], (ull)q[30], (ull)q[20],
                         (ull)q[23], (ull)q[21], (ull)q[22]);
            std::fprintf(stderr, "  levels (T:cycles):");
            for (int l = 0; l < 16 && l < static_cast<int>(q[18]); ++l)
                std::fprintf(stderr, " %llu:%llu", (ull)(q[l] >> 40), (ull)(q[l] & ((1ull << 40) - 1)));
            std::fprintf(stderr, "\n");
        }
        return FD_OK;
    }
    const uint64_t *h = all.data();  // k_select's phase clocks: frame 0, then the spread over the frames
    std::fprintf(stderr, "k_select cycles: init %llu hist0 %llu gather %llu subkeys %llu greedy %llu descent %llu "
                         "control %llu | chunks %llu descents %llu subchunks %llu | extract %llu runsort %llu merges %llu place %llu cmask %llu\n",
                 (ull)h[1], (ull)h[2], (ull)h[3], (ull)h[4], (ull)h[5], (ull)h[6], (ull)h[7], (ull)h[8], (ull)h[9],
                 (ull)h[0], (ull)h[10], (ull)h[11], (ull)h[12], (ull)h[13], (ull)h[14]);
    std::fprintf(stderr, "  fine:");
    for (int i = 16; i < 32; ++i) std::fprintf(stderr, " %llu", (ull)h[i]);
    std::fprintf(stderr, "\n");
    if (batch > 1) {  // the kernel lasts as long as its slowest frame
        uint64_t mn = ~0ull, mx = 0, gmx = 0, grmx = 0;
        int fmx = 0;
        for (int b = 0; b < batch; ++b) {
            const uint64_t *q = all.data() + static_cast<size_t>(b) * 32;
            const uint64_t t = q[1] + q[2] + q[3] + q[4] + q[5] + q[6] + q[7];
            if (t > mx) mx = t, fmx = b;
            mn = std::min(mn, t);
            gmx = std::max(gmx, q[3]);
            grmx = std::max(grmx, q[5]);
        }
        std::fprintf(stderr, "  frames: total cycles min %llu max %llu (frame %d), max gather %llu, max greedy %llu\n",
                     (ull)mn, (ull)mx, fmx, (ull)gmx, (ull)grmx);
    }
    return FD_OK;
}

}  // namespace

int run_select(fd_ctx *c, const SelectCall &q, const PriorInfo &pi, const SelectBufs &sb, float *out_xy,
               int32_t out_stride, int32_t *out_counts, int outputs_on_device, int frames_on_device) {
    fdk::SelectArgs s{};
    const int batch = q.batch, rows = q.rows, cols = q.cols;
    if (q.cap >= (int64_t(1) << 30))  // k_select reads the lists through buffer resources (byte offsets < 2^32)
        return fail(c, FD_ERR_INVALID, "candidate list capacity must be < 2^30 entries per frame");
    s.list_resp = as<float>(c->list_resp);
    s.list_idx = as<uint32_t>(c->list_idx);
    s.list_count = sb.list_count;
    s.hist0 = sb.hist0;
    s.list_cap = q.cap;
    s.rows = rows;
    s.cols = cols;
    s.batch = batch;
    s.tie_idx_desc = q.tie_idx_desc;
    s.value_flag = q.value_flag ? 1 : 0;
    s.mask = pi.mask;
    s.mask_wpr = pi.wpr;
    s.prior_counts = pi.counts_dev;
    s.need = q.need;
    s.dist = q.dist;
    s.grid_at_d0 = (q.push_order || q.grid_at_d0) ? 1 : 0;  // caller lists may name a pixel twice: distance 0 tests it
    s.dup_keys = q.dup_keys ? 1 : 0;
    if (s.dist >= 1 || (s.dist == 0 && s.grid_at_d0)) {
        s.grid_w = (cols + s.dist) / (s.dist + 1);
        s.grid_h = (rows + s.dist) / (s.dist + 1);
        const int64_t cells = static_cast<int64_t>(s.grid_w + 2) * (s.grid_h + 2);  // bordered grid
        if (cells > fdk::kGridLdsCells) FD_HIP_TRY(c, ensure_as(c, c->grid, cells * batch, s.grid_global));
    }
    float *dxy = out_xy;
    int32_t *dcnt = out_counts;
    c->h_status_valid = false;
    // Host outputs: the counts and features are written behind the status words (status | candidate
    // counts | feature counts | features, one buffer), so that all of it returns in one copy into
    // pinned memory and one synchronisation (three pageable copies and a status read cost ~40 us more
    // per 640x480 frame).
    const size_t res_head = (sizeof(uint32_t) * 3 * static_cast<size_t>(batch) + 15) & ~size_t(15);
    const size_t res_bytes = res_head + sizeof(float) * 2 * static_cast<size_t>(out_stride) * batch;
    SelectBufs sbl = sb;
    // In the raster tie order nothing after k_select changes the outputs: the kernel writes the features
    // and counts straight into the pinned result buffer and mirrors the status words there (no copy after
    // the kernel: ~6 us per 640x480 host frame). The reference order's pass rewrites them: copied as before.
    const bool direct = !outputs_on_device && c->tie_order != FD_TIES_REFERENCE;
    if (!outputs_on_device) {
        if (c->status.n < res_bytes) {  // (grow: the selection's status words move with it)
            FD_HIP_TRY(c, ensure(c, c->status, res_bytes));
            sbl.status = as<uint32_t>(c->status);
            sbl.cand_n = sbl.status + batch;
        }
        FD_HIP_TRY(c, ensure_host(c->h_res, res_bytes));
        uint8_t *const res = static_cast<uint8_t *>(direct ? c->h_res.p : c->status.p);
        dcnt = reinterpret_cast<int32_t *>(res + sizeof(uint32_t) * 2 * static_cast<size_t>(batch));
        dxy = reinterpret_cast<float *>(res + res_head);
    }
    s.status_host = direct ? static_cast<uint32_t *>(c->h_res.p) : nullptr;
    s.out_xy = dxy;
    s.out_stride = out_stride;
    s.out_counts = dcnt;
    s.key_base = q.key_base;
    s.key_lz = q.key_lz;
    s.status = sbl.status;
    s.cand_n = sbl.cand_n;
    // Small batches of large frames: spread the first chunk's gather over ~256 workgroups in its own
    // kernel (~9 us of fixed cost: pays off once one workgroup's pass over the list costs more, i.e.
    // from about a megapixel per frame; measured at 640x480: break-even).
    const bool big = static_cast<int64_t>(rows) * cols >= (1 << 20);
    s.gather_groups = big ? std::max(1, std::min(64, 256 / std::max(batch, 1))) : 1;
    if (const char *e = ab_env("FD_GATHER_GROUPS")) s.gather_groups = std::max(1, std::atoi(e));  // A/B
    if (q.value_flag) s.gather_groups = 1;  // pre_count carries the candidate kernel's flag instead
    s.pre_count = sb.pre_count;
    s.pre_keys = s.gather_groups > 1 ? sb.pre_keys : nullptr;
    s.seg_bad = sb.seg_bad;
    s.wide_keys = sb.wide_keys;
    // FAST's top responses are scores plus a slowly growing offset: thousands of candidates share the
    // top bins and the greedy scan runs over several chunks (1280x720 noise: ~5k), so the wide pass
    // comes with the first chunk; the corner detectors usually finish within it (wide pass deferred).
    s.wide_eager = q.wide_eager ? 1 : 0;
    // ... and its list pass is spread over the frame's list by k_wide_gather, ~16k entries per workgroup
    // at FAST's ~30 % candidate density on noise (one workgroup read the whole list before: 1280x720,
    // ~55k of k_select's ~130k cycles per frame).
    // (not under FAST's emission cut: its lists of a few tens of thousands of keys are cheaper to pass once
    // inside k_select -- 85 us vs 73 + 13 + 5 us for k_select, k_wide_gather and k_wide_cut at configs[2])
    if (s.wide_eager && s.wide_keys && !s.pre_keys && !q.value_flag && !q.skipped) {
        const int64_t est = static_cast<int64_t>(rows) * cols * 3 / 10;
        s.wide_groups = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(64, (est + 16383) / 16384)));
        s.wide_count = sb.wide_count;
        s.wide_cut = sb.wide_cut;
    }
    if (q.segdesc && !s.pre_keys) {
        s.segdesc = q.segdesc;
        s.seghead = q.seghead;
        s.nseg = q.nseg;
    }
    static const bool stamps = ab_env("FD_SELECT_STAMPS") != nullptr;
    if (stamps) {  // diagnostic: phase clocks of k_select and k_select_reference
        if (const int rc = diag_words(c, sizeof(uint64_t) * 32 * batch)) return rc;
        s.stamps = as<uint64_t>(c->dbg);
    }
    s.skipped = q.skipped;
    s.cut_cur = q.cut_cur;
    s.cut_next = q.cut_next;
    FD_HIP_TRY(c, fdk::launch_select(s, batch, c->stream));
    if (q.redo_points) {
        // the frames whose selection ran out of emitted keys with candidates left below the cut (kFrameRedo):
        // detected again without the cut and selected again, in stream order; every other workgroup of
        // these launches exits at once (graph-capturable: no host round trip)
        fdk::PointsArgs pr = *q.redo_points;
        pr.emit_cut = nullptr;
        pr.emit_cut_next = nullptr;
        pr.skipped = nullptr;
        pr.redo_status = s.status;
        FD_HIP_TRY(c, fdk::launch_fast(false, pr, *q.redo_off, c->stream));
        fdk::SelectArgs s2 = s;
        s2.skipped = nullptr;
        s2.cut_cur = nullptr;
        s2.cut_next = nullptr;
        s2.redo_status = s.status;
        s2.stamps = nullptr;
        FD_HIP_TRY(c, fdk::launch_select(s2, batch, c->stream));
    }
    c->sel_dirty = false;
    c->status_batch = batch;
    if (stamps)
        if (const int rc = print_diag(c, batch, kDiagSelect)) return rc;
    if (c->tie_order == FD_TIES_REFERENCE && !q.tie_idx_desc) {
        fdk::RefSortArgs r{};
        const int rc = ref_buffers(c, batch, rows, cols, q.cap, r);
        if (rc) return rc;
        r.push_order = q.push_order ? 1 : 0;
        static const bool ref_debug = ab_env("FD_REF_DEBUG") != nullptr;  // diagnostic: broken invariants
        if (ref_debug) {
            if (const int rc2 = diag_words(c, sizeof(uint32_t) * 8 * batch)) return rc2;
            r.dbg = as<uint32_t>(c->dbg);
        }
        // frames of >= 1 Mpx: the multi-workgroup prelude (push order, first levels); FD_REF_WIDE=0/1
        // forces it off / on (tests)
        const char *wide_env = ab_env("FD_REF_WIDE");
        const bool wide = wide_env ? std::atoi(wide_env) != 0
                                   : static_cast<int64_t>(rows) * cols >= (int64_t{1} << 20);
        FD_HIP_TRY(c, fdk::launch_select_reference(s, r, batch, wide, c->stream));
        if (stamps)
            if (const int rc2 = print_diag(c, batch, kDiagReference)) return rc2;
        if (ref_debug)
            if (const int rc2 = print_diag(c, batch, kDiagRefChecks)) return rc2;
        if (!outputs_on_device) {  // the call synchronises anyway: frames left to the host
            // (sbl, not sb: the status words may have moved with the host outputs' result buffer above)
            const int rc2 = resolve_ties(c, s, batch, sbl, q.push_order, FD_FRAME_UNRESOLVED);
            if (rc2) return rc2;
        }
    }
    if (!outputs_on_device) {
        if (!direct) FD_HIP_TRY(c, hipMemcpyAsync(c->h_res.p, c->status.p, res_bytes, hipMemcpyDeviceToHost, c->stream));
        FD_HIP_TRY(c, hipStreamSynchronize(c->stream));
        const uint32_t *st = static_cast<const uint32_t *>(c->h_res.p);
        std::memcpy(out_counts, st + 2 * static_cast<size_t>(batch), sizeof(int32_t) * batch);
        std::memcpy(out_xy, static_cast<const uint8_t *>(c->h_res.p) + res_head,
                    sizeof(float) * 2 * static_cast<size_t>(out_stride) * batch);
        c->h_status.assign(st, st + batch);
        c->h_status_valid = true;
        for (int b = 0; b < batch; ++b) {
            if (const int rc = frame_status_error(c, st[b], b, q.value_msg)) return rc;
            if (out_counts[b] > out_stride) return fail(c, FD_ERR_CAPACITY, "out_stride smaller than the features found");
        }
    } else if (!frames_on_device) {
        FD_HIP_TRY(c, hipStreamSynchronize(c->stream));  // the host frames must stay valid until copied
    }
    return FD_OK;
}

}  // namespace fdrt
