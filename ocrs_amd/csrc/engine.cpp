#include "engine.hpp"

#include <algorithm>
#include <exception>
#include <limits>
#include <map>
#include <thread>

#include "kernels.hpp"

using namespace ocrs;
using namespace ocrs::geom;

// ===========================================================================
// Tiled detection: the plan
// ===========================================================================
TileAxisPlan ocrs::tile_axis_plan(int L, int M, int v) {
    if (L <= 0 || M <= 0 || v < 0 || v > M / 2) fail(OCRS_ERR_INVALID_ARGUMENT, "tile plan: length %d, model length %d, overlap %d", L, M, v);
    TileAxisPlan p;
    if (L <= M) {
        p.origin = {0};
        p.bound = {0, L};
        return p;
    }
    const int n = (L - v + (M - v) - 1) / (M - v);   // the fewest tiles whose neighbours overlap by at least v (n >= 2)
    p.origin.resize(n);
    p.bound.resize(n + 1);
    for (int i = 0; i < n; i++) p.origin[i] = (int32_t)(((int64_t)i * (L - M)) / (n - 1));
    p.bound[0] = 0;
    p.bound[n] = L;
    for (int i = 1; i < n; i++) p.bound[i] = (p.origin[i - 1] + M + p.origin[i]) / 2;   // the middle of the overlap of tiles i - 1 and i
    return p;
}

// ===========================================================================
// Detection — detection.rs:104-200
// ===========================================================================
namespace {

// The reference takes any image per call (detection.rs:131-171) and the model always runs at its own fixed size, so a
// batch may hold pages of SEVERAL sizes (r6; the coalescer merges whatever waits): the model runs once over all of them,
// the size-dependent kernels before and after it (resize in; resize back + threshold, components, contours) run once per
// size, on that size's pages — the same launches with the same arguments as a batch of that size alone, so nobody's bits
// change.  Internally the pages are ordered by size group (`order`); results go back in the caller's order.
struct SizeGroup {
    int h = 0, w = 0, first = 0, count = 0;          // pages [first, first + count) of the grouped order
    int pad_bottom = 0, pad_right = 0, max_comp = 0;
    int64_t px = 0, arena = 0;
    uint8_t* d_mask = nullptr;
    float* d_map = nullptr;                          // page-resolution probabilities: scored requests (and host_map) only
    bool prepared = false;                           // resize_threshold wrote the component stage's initial labels too
    k::CclBuffers b{};
};
struct PageGroups {
    std::vector<SizeGroup> groups;
    std::vector<int> order;      // grouped position -> the caller's page
    std::vector<int> pos_of;     // the caller's page -> grouped position (the inverse of `order`)
    std::vector<int> group_of;   // grouped position -> its size group
};

PageGroups group_pages_by_size(const ocrs_page* const* pages, size_t n) {
    PageGroups pg;
    std::vector<SizeGroup>& groups = pg.groups;
    pg.order.resize(n); pg.pos_of.resize(n); pg.group_of.resize(n);
    std::vector<int> gi(n);
    for (size_t i = 0; i < n; i++) {
        const int h = pages[i]->h, w = pages[i]->w;
        if (h <= 0 || w <= 0 || h > 65535 || w > 65535) fail(OCRS_ERR_INVALID_ARGUMENT, "unsupported page size %dx%d", h, w);
        size_t g = 0;
        while (g < groups.size() && (groups[g].h != h || groups[g].w != w)) g++;
        if (g == groups.size()) { groups.emplace_back(); groups[g].h = h; groups[g].w = w; }
        groups[g].count++;
        gi[i] = (int)g;
    }
    int at = 0;
    for (SizeGroup& g : groups) { g.first = at; at += g.count; g.count = 0; }
    for (size_t i = 0; i < n; i++) {
        SizeGroup& g = groups[gi[i]];
        pg.order[g.first + g.count] = (int)i;
        pg.pos_of[i] = g.first + g.count;
        pg.group_of[g.first + g.count] = gi[i];
        g.count++;
    }
    return pg;
}

// The detector on `n` model-sized inputs d_in [n, in_h, in_w] (the untiled batch, or one chunk of tiles); returns its
// probabilities in the same layout.  A callback model runs once per input, input run_order[k] k-th (null: as they lie),
// and its outputs go to d_cb_out.
const float* run_detector(const ocrs_engine& e, Workspace& ws, const float* d_in, int n, int in_h, int in_w, float* d_cb_out,
                          const int* run_order) {
    if (!e.detection->is_callback()) {
        TensorShape os;
        const float* d_prob =
            static_cast<const HipModel*>(e.detection)->run_device(ws, d_in, n, in_h, in_w, &os, e.tm(), nullptr, nullptr, true, e.debug);
        if (os.n != n || os.h != in_h || os.w != in_w || os.c != 1)
            fail(OCRS_ERR_WRONG_OUTPUT, "model output had unexpected type or shape: detection output [%d,%d,%d,%d]", os.n,
                 os.c, os.h, os.w);
        return d_prob;
    }
    // `trait Model` implemented by the caller: one run per model input, host tensors (detection.rs:184)
    const auto* cb = static_cast<const CallbackModel*>(e.detection);
    const size_t px = (size_t)in_h * in_w;
    for (int k = 0; k < n; k++) {
        const size_t at = (size_t)(run_order ? run_order[k] : k) * px;
        std::vector<float> hin(px), hout;
        ws.download(hin.data(), d_in + at, hin.size() * sizeof(float));
        ws.sync();
        const int64_t ishape[4] = {1, 1, in_h, in_w};
        int64_t oshape[4];
        int ond = 0;
        cb->run(hin.data(), ishape, hout, oshape, &ond);
        if (ond != 4 || oshape[2] != in_h || oshape[3] != in_w || oshape[0] * oshape[1] != 1)
            fail(OCRS_ERR_WRONG_OUTPUT, "model output had unexpected type or shape: detection output is not [1,1,%d,%d]",
                 in_h, in_w);
        OCRS_HIP(hipMemcpyAsync(d_cb_out + at, hout.data(), hout.size() * sizeof(float), hipMemcpyHostToDevice, ws.s()));
        ws.sync();
    }
    return d_cb_out;
}

// Tiled detection: tiles of the whole request in the caller's page order, row-major within a page (a
// caller's model sees them in that order); gather -> model -> stitch per chunk of at most det_tile_batch tiles, so the
// activations of a request are bounded whatever the page size.  Owned rectangles are disjoint: chunks need no ordering
// among themselves.  stitch_threshold fills every group's mask and map.
void run_detector_tiled(const ocrs_engine& e, Workspace& ws, const PageGroups& pg, const std::vector<const float*>& page_ptrs,
                        int in_h, int in_w, int tile_overlap) {
    StageTimers* T = e.tm();
    hipStream_t st = ws.s();
    std::vector<k::TileDesc> tiles;
    for (int i : pg.pos_of) {
        const SizeGroup& g = pg.groups[pg.group_of[i]];
        const TileAxisPlan py = tile_axis_plan(g.h, in_h, tile_overlap), px = tile_axis_plan(g.w, in_w, tile_overlap);
        const size_t at = (size_t)(i - g.first) * g.px;
        for (size_t ty = 0; ty < py.origin.size(); ty++)
            for (size_t tx = 0; tx < px.origin.size(); tx++)
                tiles.push_back(k::TileDesc{page_ptrs[i], g.d_mask + at, g.d_map ? g.d_map + at : nullptr, g.h, g.w, py.origin[ty], px.origin[tx],
                                            py.bound[ty], py.bound[ty + 1], px.bound[tx], px.bound[tx + 1]});
    }
    k::TileDesc* d_tiles = ws.alloc_n<k::TileDesc>(tiles.size());
    ws.upload(d_tiles, tiles.data(), tiles.size() * sizeof(k::TileDesc));
    const size_t chunk = (size_t)std::max(1, option(OPT_DET_TILE_BATCH)), tile_px = (size_t)in_h * in_w;
    float* d_tin = ws.alloc_n<float>(std::min(chunk, tiles.size()) * tile_px);
    float* d_tout = e.detection->is_callback() ? ws.alloc_n<float>(std::min(chunk, tiles.size()) * tile_px) : nullptr;
    const size_t mark = ws.bufs.size();
    for (size_t c0 = 0; c0 < tiles.size(); c0 += chunk) {
        const int nt = (int)std::min(chunk, tiles.size() - c0);
        {
            StageScope sc(T, ST_RESIZE_IN, st);
            k::gather_tiles(d_tiles + c0, nt, d_tin, in_h, in_w, st);
        }
        const float* d_tp = run_detector(e, ws, d_tin, nt, in_h, in_w, d_tout, nullptr);
        {
            StageScope sc(T, ST_RESIZE_THRESH, st);
            k::stitch_threshold(d_tiles + c0, nt, d_tp, in_h, in_w, e.text_threshold, st);
        }
        if (c0 + chunk < tiles.size()) {   // the next chunk reuses this one's activations: drain, then hand them back
            ws.sync();
            while (ws.bufs.size() > mark) ws.bufs.pop_back();
        }
    }
}

// connected components -> rects (detection.rs:41-62)
// Scratch is sized for pages of text: up to 65 536 components and 2 border points per pixel.  The reference
// takes ANY mask (detection.rs:41-62), so a page that does not fit (salt noise, dense halftone) gets its
// component stage re-run on its own with buffers for the worst case — rerun_overflow_page.
k::CclBuffers alloc_ccl(Workspace& ws, int np, int h, int64_t px, int mc, int64_t ar, bool scored, bool zero) {
    k::CclBuffers b{};
    b.labels = ws.alloc_n<int32_t>((size_t)np * px);
    b.row_counts = ws.alloc_n<int32_t>((size_t)np * h);
    b.row_offsets = ws.alloc_n<int32_t>((size_t)np * h);
    b.n_roots = ws.alloc_n<int32_t>(np);
    b.roots = ws.alloc_n<int32_t>((size_t)np * mc);
    b.lengths = ws.alloc_n<int32_t>((size_t)np * mc);
    b.offsets = ws.alloc_n<int32_t>((size_t)np * mc);
    b.overflow = ws.alloc_n<int32_t>(np);
    b.pts = ws.alloc_n<uint32_t>((size_t)np * ar);
    b.tmp = ws.alloc_n<uint32_t>((size_t)np * ar * 4);
    b.keep = ws.alloc_n<uint8_t>((size_t)np * ar);
    b.rects = ws.alloc_n<float>((size_t)np * mc * 6);
    b.valid = ws.alloc_n<uint8_t>((size_t)np * mc);
    if (scored) {
        b.score_pixels = ws.alloc_n<uint32_t>((size_t)np * mc);
        b.score_sums = ws.alloc_n<unsigned long long>((size_t)np * mc);
    }
    if (zero) OCRS_HIP(hipMemsetAsync(b.overflow, 0, np * sizeof(int32_t), ws.s()));
    return b;
}

void run_ccl(const ocrs_engine& e, Workspace& ws, const uint8_t* mask, const float* map, int np, int h, int w, const k::CclBuffers& b,
             int mc, int64_t ar, bool scored, bool prepared) {
    StageTimers* T = e.tm();
    hipStream_t cs = ws.s();
    {
        StageScope sc(T, ST_CCL, cs, prepared ? 3 : 4);
        k::ccl_label(mask, np, h, w, b, mc, cs, prepared);
    }
    if (scored) {   // two fills and one kernel, counted with the component stage
        StageScope sc(T, ST_CCL, cs, 3);
        k::component_scores(mask, map, np, h, w, b, mc, cs);
    }
    {
        StageScope sc(T, ST_CONTOUR_RECTS, cs, prepared ? 1 : 2);
        k::contour_rects(mask, np, h, w, b, mc, ar, /*expand*/ 3.0f, e.min_area, /*eps*/ 2.0f, cs, prepared);
    }
}

struct PageCandidates {   // one page's candidate components on the host; detect_now compacts them by valid[]
    int32_t count = 0;
    std::vector<float> hr;         // [>= count][6] rects
    std::vector<uint8_t> hv;       // valid
    std::vector<uint32_t> hpx;     // scored: the candidates' pixel counts and fixed-point sums
    std::vector<uint64_t> hsum;
};

// queues the download of the `count` candidates of page slot `slot` of `b`, whose slots hold `stride` candidates each
void fetch_candidates(Workspace& ws, const k::CclBuffers& b, size_t slot, size_t stride, int32_t count, bool scored, PageCandidates* pc) {
    const size_t at = slot * stride;
    pc->count = count;
    pc->hr.resize((size_t)count * 6);
    pc->hv.resize(count);
    ws.download(pc->hr.data(), b.rects + at * 6, pc->hr.size() * sizeof(float));
    ws.download(pc->hv.data(), b.valid + at, count);
    if (scored) {
        pc->hpx.resize(count);
        pc->hsum.resize(count);
        ws.download(pc->hpx.data(), b.score_pixels + at, (size_t)count * sizeof(uint32_t));
        ws.download(pc->hsum.data(), b.score_sums + at, (size_t)count * sizeof(uint64_t));
    }
}

// the component stage of page j of `g` (the caller's page `page_no`) again, alone, with buffers for the worst case
void rerun_overflow_page(const ocrs_engine& e, Workspace& ws, const SizeGroup& g, int j, int page_no, bool scored, PageCandidates* pc) {
    // Worst case of an h x w mask: no more than px / 4 + O(h + w) 8-connected components can be pairwise
    // separated, and a border walk enters a pixel at most once per direction (8 px points in total).
    const int64_t mc64 = g.px / 4 + (int64_t)g.h + g.w + 16, ar_big = 8 * g.px + 64;
    if (ar_big >= (int64_t)0x7fffffff)
        fail(OCRS_ERR_CAPACITY, "text mask of page %d: %lld pixels exceed the 32-bit contour arena", page_no, (long long)g.px);
    const int mc = (int)mc64;
    const k::CclBuffers bb = alloc_ccl(ws, 1, g.h, g.px, mc, ar_big, scored, true);
    run_ccl(e, ws, g.d_mask + (size_t)j * g.px, g.d_map ? g.d_map + (size_t)j * g.px : nullptr, 1, g.h, g.w, bb, mc, ar_big, scored, false);
    int32_t cnt = 0, o = 0;
    ws.download(&cnt, bb.n_roots, sizeof cnt);
    ws.download(&o, bb.overflow, sizeof o);
    ws.sync();
    if (o || cnt > mc)
        fail(OCRS_ERR_DEVICE, "internal: component stage of page %d overflowed its worst-case buffers (%d components)", page_no, cnt);
    fetch_candidates(ws, bb, 0, (size_t)mc, cnt, scored, pc);
    ws.sync();
}

// The component stage of every size group and its results on the host, per page in grouped order.
// One round trip in the common case: the counts travel together with the first kSpec candidate rects of every
// page (a page of text has a few hundred to ~1 500 components); only a page with more needs a second one.
std::vector<PageCandidates> component_candidates(const ocrs_engine& e, Workspace& ws, const PageGroups& pg, bool scored) {
    constexpr int kSpec = 2048;
    struct Prefix {   // one size group's counts and speculative candidates
        std::vector<int32_t> counts, ovf;
        PageCandidates all;   // [count pages][spec]
    };
    std::vector<Prefix> prefix(pg.groups.size());
    for (size_t gi = 0; gi < pg.groups.size(); gi++) {
        const SizeGroup& g = pg.groups[gi];
        Prefix& p = prefix[gi];
        run_ccl(e, ws, g.d_mask, g.d_map, g.count, g.h, g.w, g.b, g.max_comp, g.arena, scored, g.prepared);
        const size_t spec = (size_t)std::min(g.max_comp, kSpec);
        p.counts.resize(g.count); p.ovf.resize(g.count);
        p.all.hr.resize(g.count * spec * 6); p.all.hv.resize(g.count * spec);
        ws.download(p.counts.data(), g.b.n_roots, g.count * sizeof(int32_t));
        ws.download(p.ovf.data(), g.b.overflow, g.count * sizeof(int32_t));
        // the first `spec` candidates of every page in ONE strided copy per array (r2: two copies per page — each a blit
        // kernel that waits for CU slots like any other)
        ws.download_2d(p.all.hr.data(), g.b.rects, (size_t)g.max_comp * 6 * sizeof(float), spec * 6 * sizeof(float), g.count);
        ws.download_2d(p.all.hv.data(), g.b.valid, (size_t)g.max_comp, spec, g.count);
        if (scored) {
            p.all.hpx.resize(g.count * spec); p.all.hsum.resize(g.count * spec);
            ws.download_2d(p.all.hpx.data(), g.b.score_pixels, (size_t)g.max_comp * sizeof(uint32_t), spec * sizeof(uint32_t), g.count);
            ws.download_2d(p.all.hsum.data(), g.b.score_sums, (size_t)g.max_comp * sizeof(uint64_t), spec * sizeof(uint64_t), g.count);
        }
    }
    ws.sync();   // one wait for all sizes
    std::vector<PageCandidates> cand(pg.order.size());
    bool more = false;
    std::vector<int> big;   // pages (grouped order) whose component stage did not fit
    for (size_t gi = 0; gi < pg.groups.size(); gi++) {
        const SizeGroup& g = pg.groups[gi];
        const Prefix& p = prefix[gi];
        const size_t spec = (size_t)std::min(g.max_comp, kSpec);
        for (int j = 0; j < g.count; j++) {
            PageCandidates& pc = cand[g.first + j];
            const int32_t cnt = p.counts[j];
            if (p.ovf[j] || cnt > g.max_comp) { big.push_back(g.first + j); continue; }
            if ((size_t)cnt > spec) {   // the second trip
                more = true;
                fetch_candidates(ws, g.b, (size_t)j, (size_t)g.max_comp, cnt, scored, &pc);
                continue;
            }
            pc.count = cnt;
            pc.hr.assign(p.all.hr.begin() + j * spec * 6, p.all.hr.begin() + (j + 1) * spec * 6);
            pc.hv.assign(p.all.hv.begin() + j * spec, p.all.hv.begin() + (j + 1) * spec);
            if (scored) {
                pc.hpx.assign(p.all.hpx.begin() + j * spec, p.all.hpx.begin() + (j + 1) * spec);
                pc.hsum.assign(p.all.hsum.begin() + j * spec, p.all.hsum.begin() + (j + 1) * spec);
            }
        }
    }
    if (more) ws.sync();
    for (int i : big) {
        const SizeGroup& g = pg.groups[pg.group_of[i]];
        rerun_overflow_page(e, ws, g, i - g.first, pg.order[i], scored, &cand[i]);
    }
    return cand;
}

}  // namespace

void ocrs_engine::detect_now(const ocrs_page* const* pages, size_t n, std::vector<std::vector<RotatedRect>>* rects_out,
                             float* host_map, DetScores* scores, int tile_overlap) const {
    if (!detection) fail(OCRS_ERR_MODEL_NOT_LOADED, "Detection model not loaded");
    if (scores && !rects_out) fail(OCRS_ERR_INVALID_ARGUMENT, "detection scores come with the rects");
    if (n == 0) {
        if (rects_out) rects_out->clear();
        if (scores) { scores->score.clear(); scores->pixels.clear(); }
        return;
    }
    const int64_t in_h64 = detection->input_shape[2], in_w64 = detection->input_shape[3];
    if (in_h64 <= 0 || in_w64 <= 0) fail(OCRS_ERR_MODEL_DIMS, "failed to get model dims");  // detection.rs:141-144
    const int in_h = (int)in_h64, in_w = (int)in_w64;
    const int N = (int)n;
    // tiled: the pages are not resized; their model-sized tiles run through the model in chunks and are
    // stitched into the page-resolution mask / map that the code after resize_threshold works on
    const bool tiled = tile_overlap >= 0;
    if (tiled && tile_overlap > std::min(in_h, in_w) / 2)
        fail(OCRS_ERR_INVALID_ARGUMENT, "tile overlap %d: at most half the model input's shorter side (%d)", tile_overlap, std::min(in_h, in_w) / 2);
    PageGroups pg = group_pages_by_size(pages, n);
    std::vector<SizeGroup>& groups = pg.groups;
    if (host_map && groups.size() > 1)
        fail(OCRS_ERR_INVALID_ARGUMENT, "pages whose probability maps are returned in one [n, h, w] array must share a size");

    Workspace ws;
    hipStream_t st = ws.s();
    StageTimers* T = tm();

    // page pointer table, grouped order
    std::vector<const float*> hp(n);
    for (size_t i = 0; i < n; i++) hp[i] = pages[pg.order[i]]->grey.as<float>();

    const float* d_prob = nullptr;   // tiled: the model runs per chunk of tiles, once the pages' masks exist (below)
    if (!tiled) {
        const float** d_ptrs = ws.alloc_n<const float*>(n);
        ws.upload(d_ptrs, hp.data(), n * sizeof(float*));
        float* d_in = ws.alloc_n<float>((size_t)N * in_h * in_w);
        {
            StageScope sc(T, ST_RESIZE_IN, st, groups.size());
            for (SizeGroup& g : groups) {
                g.pad_bottom = std::max(in_h - g.h, 0);   // detection.rs:155-156
                g.pad_right = std::max(in_w - g.w, 0);
                k::resize_pages_to_model(d_ptrs + g.first, g.count, g.h, g.w, g.h + g.pad_bottom, g.w + g.pad_right,
                                         d_in + (size_t)g.first * in_h * in_w, in_h, in_w, st);
            }
        }
        // a callback model runs in the CALLER's page order (a caller's model may count its runs)
        float* d_out = detection->is_callback() ? ws.alloc_n<float>((size_t)N * in_h * in_w) : nullptr;
        d_prob = run_detector(*this, ws, d_in, N, in_h, in_w, d_out, pg.pos_of.data());
    }

    // slice off the padded region, resize back, threshold (detection.rs:187-194,110); r6: where the page width allows, the same
    // launch writes the component stage's initial labels and zeroes its counters (one launch and two fills fewer per size)
    float* d_map = host_map ? ws.alloc_n<float>((size_t)N * groups[0].h * groups[0].w) : nullptr;
    {
        StageScope sc(T, ST_RESIZE_THRESH, st, tiled ? 0 : groups.size());
        for (SizeGroup& g : groups) {
            g.px = (int64_t)g.h * g.w;
            g.d_mask = ws.alloc_n<uint8_t>((size_t)g.count * g.px);
            if (rects_out) {
                g.max_comp = (int)std::min<int64_t>(65536, g.px / 2 + 16);
                g.arena = 2 * g.px + 64;
                g.b = alloc_ccl(ws, g.count, g.h, g.px, g.max_comp, g.arena, scores != nullptr, false);
            }
            // a scored request keeps every size's map (host_map: one size, one array)
            g.d_map = d_map ? d_map : scores ? ws.alloc_n<float>((size_t)g.count * g.px) : nullptr;
            // tiled: stitch_threshold fills the mask and the map; the component stage takes its unprepared path
            if (!tiled)
                g.prepared = k::resize_threshold(d_prob + (size_t)g.first * in_h * in_w, g.count, in_h, in_w, in_h - g.pad_bottom, in_w - g.pad_right,
                                                 text_threshold, g.d_mask, g.d_map, g.h, g.w, st, g.b.labels, g.b.overflow, g.b.offsets);
            if (rects_out && !g.prepared) OCRS_HIP(hipMemsetAsync(g.b.overflow, 0, g.count * sizeof(int32_t), st));
        }
    }
    if (tiled) run_detector_tiled(*this, ws, pg, hp, in_h, in_w, tile_overlap);
    if (host_map)   // (one size group: grouped order = the caller's order)
        ws.download(host_map, d_map, (size_t)N * groups[0].px * sizeof(float));
    if (!rects_out) {
        ws.sync();
        if (T) T->collect();
        return;
    }

    const std::vector<PageCandidates> cand = component_candidates(*this, ws, pg, scores != nullptr);
    rects_out->assign(n, {});
    if (scores) { scores->score.assign(n, {}); scores->pixels.assign(n, {}); }
    for (int i = 0; i < N; i++) {
        const PageCandidates& pc = cand[i];
        auto& out = (*rects_out)[pg.order[i]];
        for (int c = 0; c < pc.count; c++) {
            if (!pc.hv[c]) continue;
            out.push_back(RotatedRect::from_array(&pc.hr[(size_t)c * 6]));
            if (scores) {   // the compaction by valid[] that compacts the rects
                const uint32_t px = pc.hpx[c];
                scores->pixels[pg.order[i]].push_back(px);
                scores->score[pg.order[i]].push_back(px ? (float)((double)pc.hsum[c] / ((double)px * 16777216.0)) : 0.0f);
            }
        }
    }
    if (T) T->collect();
}

// ===========================================================================
// Coalescing front ends (coalesce.hpp): concurrent small requests share one launch sequence
// ===========================================================================
namespace {

// Runs `merged` for the whole batch; if that fails and the batch has several requests, every request is re-run
// on its own so that an error reaches only the caller whose input caused it.
template <class Req, class Merged, class Single>
void run_batch(std::vector<Req*>& batch, Merged&& merged, Single&& single) {
    try {
        merged();
        return;
    } catch (...) {
        if (batch.size() == 1) {
            batch[0]->error = std::current_exception();
            return;
        }
    }
    for (Req* r : batch) {
        try {
            single(*r);
        } catch (...) {
            r->error = std::current_exception();
        }
    }
}

}  // namespace

void ocrs_engine::init_coalescers() {
    det_queue = std::make_unique<Coalescer<DetRequest>>(
        [this](std::vector<DetRequest*>& batch) {
            run_batch(
                batch,
                [&] {
                    if (batch.size() == 1) { detect_now(batch[0]->pages, batch[0]->n, batch[0]->rects, nullptr, batch[0]->scores); return; }
                    std::vector<const ocrs_page*> pages;
                    bool any_scores = false;   // scored if any member asked; the rects are the same either way
                    for (DetRequest* r : batch) {
                        pages.insert(pages.end(), r->pages, r->pages + r->n);
                        any_scores = any_scores || r->scores;
                    }
                    std::vector<std::vector<RotatedRect>> rects;
                    DetScores sc;
                    detect_now(pages.data(), pages.size(), &rects, nullptr, any_scores ? &sc : nullptr);
                    size_t at = 0;
                    for (DetRequest* r : batch) {
                        r->rects->assign(std::make_move_iterator(rects.begin() + at), std::make_move_iterator(rects.begin() + at + r->n));
                        if (r->scores) {
                            r->scores->score.assign(std::make_move_iterator(sc.score.begin() + at), std::make_move_iterator(sc.score.begin() + at + r->n));
                            r->scores->pixels.assign(std::make_move_iterator(sc.pixels.begin() + at), std::make_move_iterator(sc.pixels.begin() + at + r->n));
                        }
                        at += r->n;
                    }
                },
                [&](DetRequest& r) { detect_now(r.pages, r.n, r.rects, nullptr, r.scores); });
        },
        [](const DetRequest&, const DetRequest&) { return true; });   // pages of any sizes share a batch (detect_now groups them by size)
    rec_queue = std::make_unique<Coalescer<RecRequest>>(
        [this](std::vector<RecRequest*>& batch) {
            run_batch(
                batch,
                [&] {
                    if (batch.size() == 1) {
                        RecRequest& r = *batch[0];
                        const std::vector<char> rp(r.rectify ? r.n_pages : 0, 1);
                        recognize_now(r.pages, r.n_pages, *r.lines_per_page, r.results, r.scored, false, r.rectify ? &rp : nullptr);
                        return;
                    }
                    std::vector<const ocrs_page*> pages;
                    std::vector<std::vector<std::vector<RotatedRect>>> lpp;
                    bool any_scores = false;   // scored if any member asked; the steps are the same either way
                    bool any_rectify = false;  // the kind is per request: a merged batch crops each page's lines its caller's way
                    std::vector<char> rp;
                    for (RecRequest* r : batch) {
                        pages.insert(pages.end(), r->pages, r->pages + r->n_pages);
                        lpp.insert(lpp.end(), r->lines_per_page->begin(), r->lines_per_page->end());
                        any_scores = any_scores || r->scored;
                        any_rectify = any_rectify || r->rectify;
                        rp.insert(rp.end(), r->n_pages, r->rectify ? 1 : 0);
                    }
                    std::vector<RecResult> res;
                    recognize_now(pages.data(), pages.size(), lpp, &res, any_scores, false, any_rectify ? &rp : nullptr);
                    size_t line0 = 0, page0 = 0;
                    for (RecRequest* r : batch) {
                        size_t nl = 0;
                        for (const auto& pg : *r->lines_per_page) nl += pg.size();
                        r->results->assign(std::make_move_iterator(res.begin() + line0), std::make_move_iterator(res.begin() + line0 + nl));
                        for (RecResult& l : *r->results) {   // back to the caller's numbering
                            l.line.page -= page0;
                            l.line.index -= line0;
                        }
                        line0 += nl;
                        page0 += r->n_pages;
                    }
                },
                [&](RecRequest& r) {
                    const std::vector<char> rp(r.rectify ? r.n_pages : 0, 1);
                    recognize_now(r.pages, r.n_pages, *r.lines_per_page, r.results, r.scored, false, r.rectify ? &rp : nullptr);
                });
        },
        [](const RecRequest&, const RecRequest&) { return true; });   // lines of any pages share a ragged batch
}

void ocrs_engine::detect(const ocrs_page* const* pages, size_t n, std::vector<std::vector<RotatedRect>>* rects_out,
                         float* host_map, DetScores* scores, int tile_overlap) const {
    const int max_active = option(OPT_COALESCE);   // (r4: 4 / 6 / 12 detection batches in flight instead of 2: 188-193 pages/s from 12 threads either way)
    const size_t max_pages = (size_t)std::max(1, option(OPT_COALESCE_PAGES));
    // merged only where it cannot be observed: HIP executor (a caller's `trait Model` sees every run), rects only
    // (a tiled request is a batch of its own tiles already: never merged, never waits)
    if (max_active <= 0 || !det_queue || !rects_out || host_map || n == 0 || 2 * n >= max_pages || !detection ||
        detection->is_callback() || debug || tile_overlap >= 0) {
        detect_now(pages, n, rects_out, host_map, scores, tile_overlap);
        return;
    }
    DetRequest r;
    r.pages = pages; r.n = n; r.rects = rects_out; r.scores = scores; r.weight = n;
    det_queue->submit(r, max_active, max_pages, option_long(OPT_COALESCE_WINDOW_US));
}

void ocrs_engine::recognize(const ocrs_page* const* pages, size_t n_pages,
                            const std::vector<std::vector<std::vector<RotatedRect>>>& lines_per_page, std::vector<RecResult>* results,
                            bool scored, bool rectify) const {
    const int max_active = option(OPT_COALESCE);
    const size_t max_pages = (size_t)std::max(1, option(OPT_COALESCE_PAGES));
    if (max_active <= 0 || !rec_queue || n_pages == 0 || 2 * n_pages >= max_pages || !recognition || recognition->is_callback()) {
        const std::vector<char> rp(rectify ? n_pages : 0, 1);
        recognize_now(pages, n_pages, lines_per_page, results, scored, false, rectify ? &rp : nullptr);
        return;
    }
    RecRequest r;
    r.pages = pages; r.n_pages = n_pages; r.lines_per_page = &lines_per_page;
    r.results = results; r.scored = scored; r.rectify = rectify; r.weight = n_pages;
    rec_queue->submit(r, max_active, max_pages, option_long(OPT_COALESCE_WINDOW_US));
}

// ===========================================================================
// Recognition — recognition.rs
// ===========================================================================
uint32_t ocrs_engine::rec_input_height() const {  // recognition.rs:332-337
    const int64_t hgt = recognition->input_shape[2];
    return hgt > 0 ? (uint32_t)hgt : 50u;
}

namespace {

// recognition.rs:58-75
uint32_t resized_line_width(int32_t orig_width, int32_t orig_height, int32_t height) {
    const float aspect = (float)orig_width / (float)orig_height;
    float v = (float)height * aspect;
    if (v != v) return 0;  // clamp keeps NaN; `as u32` maps it to 0
    v = v < 10.0f ? 10.0f : v;
    v = v > 2400.0f ? 2400.0f : v;
    return (uint32_t)v;
}

// recognition.rs:29-55
std::vector<PointI> line_polygon(const std::vector<RotatedRect>& words) {
    std::vector<PointI> poly;
    poly.reserve(words.size() * 4);
    auto floor_point = [](PointF p) { return PointI{as_i32(p.x), as_i32(p.y)}; };
    for (const RotatedRect& w : words) {
        LineF left = downwards_line(leftmost_edge(w)), right = downwards_line(rightmost_edge(w));
        poly.push_back(floor_point(left.start));
        poly.push_back(floor_point(right.start));
    }
    for (auto it = words.rbegin(); it != words.rend(); ++it) {
        LineF left = downwards_line(leftmost_edge(*it)), right = downwards_line(rightmost_edge(*it));
        poly.push_back(floor_point(right.end));
        poly.push_back(floor_point(left.end));
    }
    return poly;
}

// recognition.rs:162-193
bool polygon_slice_bounding_rect(const std::vector<PointI>& poly, int32_t min_x, int32_t max_x, Rect* out) {
    bool have = false;
    Rect acc{0, 0, 0, 0};
    const size_t n = poly.size();
    for (size_t k = 0; k < n; k++) {
        PointI s = poly[k], e = poly[(k + 1) % n];
        if (s.x > e.x) std::swap(s, e);  // rightwards()
        if ((s.x < min_x && e.x < min_x) || (s.x > max_x && e.x > max_x)) continue;
        LineF ef{PointF{(float)s.x, (float)s.y}, PointF{(float)e.x, (float)e.y}};
        PointI ts = s, te = e;
        if (auto y = ef.y_for_x((float)min_x)) ts = PointI{min_x, (int32_t)rround(*y)};
        if (auto y = ef.y_for_x((float)max_x)) te = PointI{max_x, (int32_t)rround(*y)};
        Rect br{std::min(ts.y, te.y), std::min(ts.x, te.x), std::max(ts.y, te.y), std::max(ts.x, te.x)};
        acc = have ? acc.unite(br) : br;
        have = true;
    }
    if (have) *out = acc;
    return have;
}

}  // namespace

// DESIGN.md §8.4 (tests/rectify_ref.py restates it): double from the float32 values, every operation as written, sums in
// word order, only + - * / sqrt — and no contraction (the tree is built with -ffp-contract=off), so numpy gives the same bits
LineFrame ocrs::line_frame(const float* w6, size_t n, int32_t H) {
    if (n == 0 || !w6) fail(OCRS_ERR_INVALID_ARGUMENT, "line has no words");
    if (H <= 0) fail(OCRS_ERR_INVALID_ARGUMENT, "line frame: recognition height %d", H);
    LineFrame f;
    f.ranges.resize(4 * n);
    for (size_t i = 0; i < n; i++) { f.ranges[4 * i] = 1; f.ranges[4 * i + 1] = 0; f.ranges[4 * i + 2] = 1; f.ranges[4 * i + 3] = 0; }
    bool finite = true;
    for (size_t i = 0; i < 6 * n; i++) finite = finite && std::isfinite(w6[i]);
    if (!finite) {
        f.rw = resized_line_width(0, 0, H);
        return f;
    }
    auto W = [&](size_t i, int k) { return (double)w6[6 * i + k]; };
    double sx = 0.0, sy = 0.0;
    for (size_t i = 0; i < n; i++) { sx = sx + W(i, 0); sy = sy + W(i, 1); }
    const double mx = sx / (double)n, my = sy / (double)n;
    double Sxx = 0.0, Sxy = 0.0;
    for (size_t i = 0; i < n; i++) {
        Sxx = Sxx + (W(i, 0) - mx) * (W(i, 0) - mx);
        Sxy = Sxy + (W(i, 0) - mx) * (W(i, 1) - my);
    }
    double ax, ay;
    if (n >= 2 && Sxx > 0.0) {
        const double m = Sxy / Sxx, L = std::sqrt(1.0 + m * m);
        ax = 1.0 / L;
        ay = m / L;
    } else {
        ax = -W(0, 3);
        ay = W(0, 2);
        if (ax < 0.0 || (ax == 0.0 && ay < 0.0)) { ax = -ax; ay = -ay; }
    }
    const double nx = -ay, ny = ax;
    std::vector<double> ext(4 * n);   // sa, sb, ta, tb per word
    double s_min = 0.0, s_max = 0.0, t_min = 0.0, t_max = 0.0;
    for (size_t i = 0; i < n; i++) {
        const double cx = W(i, 0), cy = W(i, 1), upx = W(i, 2), upy = W(i, 3), w = W(i, 4), h = W(i, 5);
        const double hx = (w / 2.0) * -upy, hy = (w / 2.0) * upx, vx = (h / 2.0) * upx, vy = (h / 2.0) * upy;
        double sa = 0.0, sb = 0.0, ta = 0.0, tb = 0.0;
        bool first = true;
        for (double sw : {-1.0, 1.0})
            for (double sh : {-1.0, 1.0}) {
                const double px = cx + sw * hx + sh * vx, py = cy + sw * hy + sh * vy;
                const double sv = px * ax + py * ay, tv = px * nx + py * ny;
                if (first) { sa = sb = sv; ta = tb = tv; first = false; }
                sa = std::min(sa, sv); sb = std::max(sb, sv);
                ta = std::min(ta, tv); tb = std::max(tb, tv);
            }
        ext[4 * i] = sa; ext[4 * i + 1] = sb; ext[4 * i + 2] = ta; ext[4 * i + 3] = tb;
        if (i == 0) { s_min = sa; s_max = sb; t_min = ta; t_max = tb; }
        s_min = std::min(s_min, sa); s_max = std::max(s_max, sb);
        t_min = std::min(t_min, ta); t_max = std::max(t_max, tb);
    }
    const double Wl = s_max - s_min, Hl = t_max - t_min;
    auto capped_ceil = [](double v) { return (int32_t)std::min(std::ceil(v), 2147483647.0); };
    const int32_t cw = capped_ceil(Wl), ch = capped_ceil(Hl);
    if (cw <= 0 || ch <= 0) {   // the plain crop's width for a bounding box with a side of zero
        f.rw = resized_line_width(std::max(cw, 0), std::max(ch, 0), H);
        return f;
    }
    const uint32_t rw = resized_line_width(cw, ch, H);
    f.empty = false;
    f.ax = ax; f.ay = ay;
    f.s_min = s_min; f.s_max = s_max; f.t_min = t_min; f.t_max = t_max;
    f.rw = rw;
    const double drw = (double)rw, dH = (double)H;
    f.coef[0] = (float)(s_min * ax + t_min * nx - 0.5);
    f.coef[1] = (float)(ax * Wl / drw);
    f.coef[2] = (float)(nx * Hl / dH);
    f.coef[3] = (float)(s_min * ay + t_min * ny - 0.5);
    f.coef[4] = (float)(ay * Wl / drw);
    f.coef[5] = (float)(ny * Hl / dH);
    for (size_t i = 0; i < n; i++) {
        const double c0 = std::max(std::ceil((ext[4 * i] - s_min) * drw / Wl - 0.5), 0.0);
        const double c1 = std::min(std::floor((ext[4 * i + 1] - s_min) * drw / Wl - 0.5), drw - 1.0);
        const double r0 = std::max(std::ceil((ext[4 * i + 2] - t_min) * dH / Hl - 0.5), 0.0);
        const double r1 = std::min(std::floor((ext[4 * i + 3] - t_min) * dH / Hl - 0.5), dH - 1.0);
        if (c0 > c1 || r0 > r1) continue;   // covers nothing: (1, 0, 1, 0)
        f.ranges[4 * i] = (int32_t)c0; f.ranges[4 * i + 1] = (int32_t)c1;
        f.ranges[4 * i + 2] = (int32_t)r0; f.ranges[4 * i + 3] = (int32_t)r1;
    }
    return f;
}

// the char's slice of the line's frame, mapped to the page in double; a char that starts in the padding is dropped
std::vector<std::pair<size_t, Rect>> ocrs::rectified_char_boxes(const LineFrame& f, uint32_t group_width, uint32_t ctc_input_len,
                                                                const uint32_t* pos, size_t n_steps) {
    std::vector<std::pair<size_t, Rect>> out;
    if (f.empty || n_steps == 0 || ctc_input_len == 0) return out;
    const uint32_t ds = (uint32_t)rround((float)group_width / (float)ctc_input_len), rw = f.rw;
    const double Wl = f.s_max - f.s_min, nx = -f.ay, ny = f.ax, drw = (double)rw;
    auto to_i32 = [](double v) { return (int32_t)std::min(std::max(v, -2147483648.0), 2147483647.0); };
    for (size_t i = 0; i < n_steps; i++) {
        const uint32_t start_x = pos[i] * ds;
        const uint32_t end_x = i + 1 < n_steps ? pos[i + 1] * ds : rw;
        if (start_x >= rw) continue;
        const double sv[2] = {f.s_min + (double)start_x * Wl / drw, f.s_min + (double)end_x * Wl / drw};
        const double tv[2] = {f.t_min, f.t_max};
        double x_lo = 0, x_hi = 0, y_lo = 0, y_hi = 0;
        for (int a = 0; a < 2; a++)
            for (int b = 0; b < 2; b++) {
                const double x = sv[a] * f.ax + tv[b] * nx, y = sv[a] * f.ay + tv[b] * ny;
                if (a == 0 && b == 0) { x_lo = x_hi = x; y_lo = y_hi = y; }
                x_lo = std::min(x_lo, x); x_hi = std::max(x_hi, x);
                y_lo = std::min(y_lo, y); y_hi = std::max(y_hi, y);
            }
        out.emplace_back(i, Rect{to_i32(std::floor(y_lo)), to_i32(std::floor(x_lo)), to_i32(std::ceil(y_hi)), to_i32(std::ceil(x_hi))});
    }
    return out;
}

RecLine ocrs_engine::make_rec_line(const std::vector<RotatedRect>& words, size_t page, size_t index, bool rectify) const {
    if (words.empty()) fail(OCRS_ERR_INVALID_ARGUMENT, "line has no words");  // recognition.rs:433
    if (rectify) {   // the line's own frame stands in for polygon and bounds
        static_assert(sizeof(RotatedRect) == 6 * sizeof(float), "RotatedRect is six packed floats");
        RecLine l;
        l.page = page;
        l.index = index;
        l.rectified = true;
        l.frame = line_frame(&words[0].cx, words.size(), (int32_t)rec_input_height());
        l.resized_width = l.frame.rw;
        l.group_width = (l.resized_width + 49) / 50 * 50;
        return l;
    }
    RectF br = words[0].bounding_rect();
    for (size_t i = 1; i < words.size(); i++) br = br.unite(words[i].bounding_rect());
    const Rect line_rect = br.integral_bounding_rect();
    RecLine l;
    l.page = page;
    l.index = index;
    l.resized_width = resized_line_width(line_rect.width(), line_rect.height(), (int32_t)rec_input_height());
    l.group_width = (l.resized_width + 49) / 50 * 50;  // next_multiple_of(50), recognition.rs:437
    l.polygon = line_polygon(words);
    int32_t t = l.polygon[0].y, bt = t, lf = l.polygon[0].x, rt = lf;
    for (const PointI& p : l.polygon) {
        t = std::min(t, p.y); bt = std::max(bt, p.y);
        lf = std::min(lf, p.x); rt = std::max(rt, p.x);
    }
    l.bounds = Rect{t, lf, bt, rt};
    return l;
}

// ---- crop + resize + pad every line into its place in one tensor (recognition.rs:135-158): one launch for all plain
// lines and one for all rectified ones, whatever their widths
float* ocrs::stage_line_crops(Workspace& ws, StageTimers* T, const ocrs_page* const* pages, size_t n_pages,
                              const std::vector<CropLine>& crops, int rec_h, int64_t total) {
    hipStream_t st = ws.s();
    std::vector<const float*> hp(n_pages);
    std::vector<int32_t> hhw(2 * n_pages);
    for (size_t i = 0; i < n_pages; i++) {
        hp[i] = pages[i]->grey.as<float>();
        hhw[2 * i] = pages[i]->h;
        hhw[2 * i + 1] = pages[i]->w;
    }
    const float** d_pages = ws.alloc_n<const float*>(n_pages);
    int32_t* d_hw = ws.alloc_n<int32_t>(2 * n_pages);
    ws.upload(d_pages, hp.data(), n_pages * sizeof(float*));
    ws.upload(d_hw, hhw.data(), hhw.size() * sizeof(int32_t));

    std::vector<k::LineDesc> descs;
    std::vector<int32_t> poly;
    std::vector<k::RectLineDesc> rdescs;   // the rectified lines: a launch of their own into the same tensor
    std::vector<int32_t> ranges;
    int rect_max_w = 0;
    for (const CropLine& c : crops) {
        const RecLine& ln = *c.line;
        if (ln.rectified) {
            k::RectLineDesc d{};
            d.page = (int32_t)ln.page;
            d.mode = ln.frame.empty ? 1 : 0;
            d.range_off = (int32_t)(ranges.size() / 4);
            d.range_n = ln.frame.empty ? 0 : (int32_t)(ln.frame.ranges.size() / 4);
            d.resized_w = (int32_t)ln.resized_width;
            d.out_w = (int32_t)c.out_w;
            d.out_off = c.out_off;
            d.x0 = ln.frame.coef[0]; d.ax = ln.frame.coef[1]; d.bx = ln.frame.coef[2];
            d.y0 = ln.frame.coef[3]; d.ay = ln.frame.coef[4]; d.by = ln.frame.coef[5];
            rdescs.push_back(d);
            if (!ln.frame.empty) ranges.insert(ranges.end(), ln.frame.ranges.begin(), ln.frame.ranges.end());
            rect_max_w = std::max(rect_max_w, (int)c.out_w);
            continue;
        }
        k::LineDesc d{};
        d.page = (int32_t)ln.page;
        d.poly_off = (int32_t)(poly.size() / 2);
        d.poly_n = (int32_t)ln.polygon.size();
        d.top = ln.bounds.top; d.left = ln.bounds.left;
        d.bh = ln.bounds.height(); d.bw = ln.bounds.width();
        d.resized_w = (int32_t)ln.resized_width;
        d.out_w = (int32_t)c.out_w;
        d.out_off = c.out_off;
        descs.push_back(d);
        for (const PointI& p : ln.polygon) { poly.push_back(p.y); poly.push_back(p.x); }
    }
    if (descs.empty() && rdescs.empty()) return nullptr;
    k::LineDesc* d_descs = descs.empty() ? nullptr : ws.alloc_n<k::LineDesc>(descs.size());
    int32_t* d_poly = descs.empty() ? nullptr : ws.alloc_n<int32_t>(poly.size());
    // host temporaries travel through the workspace's pinned staging: real asynchronous copies, no host wait here
    if (!descs.empty()) {
        ws.upload(d_descs, descs.data(), descs.size() * sizeof(k::LineDesc));
        ws.upload(d_poly, poly.data(), poly.size() * sizeof(int32_t));
    }
    k::RectLineDesc* d_rdescs = nullptr;
    int32_t* d_ranges = nullptr;
    if (!rdescs.empty()) {
        d_rdescs = ws.alloc_n<k::RectLineDesc>(rdescs.size());
        d_ranges = ws.alloc_n<int32_t>(std::max<size_t>(ranges.size(), 4));
        ws.upload(d_rdescs, rdescs.data(), rdescs.size() * sizeof(k::RectLineDesc));
        if (!ranges.empty()) ws.upload(d_ranges, ranges.data(), ranges.size() * sizeof(int32_t));
    }
    float* d_all = ws.alloc_n<float>((size_t)total);
    StageScope sc(T, ST_LINE_CROP, st, (descs.empty() ? 0 : 1) + (rdescs.empty() ? 0 : 1));
    k::crop_lines(d_pages, d_hw, d_descs, d_poly, (int)descs.size(), rec_h, d_all, st);
    k::rectify_lines(d_pages, d_hw, d_rdescs, d_ranges, (int)rdescs.size(), rect_max_w, rec_h, d_all, st);
    return d_all;
}

// Activations of the recognition conv stack scale with the input (~100 B per input pixel of the padded line
// batch).  A request beyond the budget is run as consecutive sub-requests over contiguous runs of its lines
// (lines are independent: recognition.rs:448-503 itself works in chunks of 20), so the caller never has to
// know the limit.  Option "rec_max_pixels" overrides the budget (tests).
static double rec_pixel_budget() {
    const long v = option_long(OPT_REC_MAX_PIXELS);
    return v > 0 ? (double)v : 2.0e9;
}

void ocrs_engine::recognize_now(const ocrs_page* const* pages, size_t n_pages,
                                const std::vector<std::vector<std::vector<RotatedRect>>>& lines_per_page,
                                std::vector<RecResult>* out, bool scored, bool want_logp,
                                const std::vector<char>* rectify_pages) const {
    if (!recognition) fail(OCRS_ERR_MODEL_NOT_LOADED, "Recognition model not loaded");
    const uint32_t rec_h = rec_input_height();
    size_t L = 0;
    for (size_t p = 0; p < n_pages; p++) L += lines_per_page[p].size();
    std::vector<RecResult>& res = *out;
    res.clear();
    res.resize(L);
    L = 0;
    for (size_t p = 0; p < n_pages; p++)
        for (const auto& words : lines_per_page[p]) {
            res[L].line = make_rec_line(words, p, L, rectify_pages && (*rectify_pages)[p]);
            L++;
        }
    const double budget = rec_pixel_budget();
    for (size_t b = 0; b < L;) {   // sub-requests within the budget, each of at least one line
        size_t e = b;
        double px = 0.0;
        while (e < L && (e == b || px + (double)rec_h * res[e].line.group_width <= budget)) px += (double)rec_h * res[e++].line.group_width;
        recognize_lines(pages, n_pages, res.data() + b, e - b, scored, want_logp);
        b = e;
    }
}

void ocrs_engine::recognize_logits(const ocrs_page* page, const std::vector<std::vector<RotatedRect>>& lines_in,
                                   std::vector<std::vector<float>>* logp, int* classes) const {
    if (!recognition) fail(OCRS_ERR_MODEL_NOT_LOADED, "Recognition model not loaded");
    if (recognition->is_callback()) fail(OCRS_ERR_INVALID_ARGUMENT, "recognize_logits needs a model of the fixed-graph executor");
    std::vector<RecResult> res;
    recognize_now(&page, 1, {lines_in}, &res, false, true);
    logp->clear();
    for (RecResult& r : res) logp->push_back(std::move(r.logp));
    *classes = (int)alphabet.size() + 1;
}

void ocrs_engine::run_recognition_ops(const int32_t* widths, size_t n, int first_op, int last_op, bool gx_only, const float* in,
                                      size_t in_len, std::vector<float>* out, std::vector<int32_t>* shapes) const {
    if (!recognition) fail(OCRS_ERR_MODEL_NOT_LOADED, "Recognition model not loaded");
    if (recognition->is_callback()) fail(OCRS_ERR_INVALID_ARGUMENT, "run_recognition_ops needs a model of the fixed-graph executor");
    const auto* hm = static_cast<const HipModel*>(recognition);
    const int ts = hm->packed_split();
    if (ts < 0) fail(OCRS_ERR_INVALID_ARGUMENT, "recognition graph is not <conv stack> TOSEQ GRU* LINEAR LOGSOFTMAX");
    const int nops = (int)hm->ops.size();
    if (n == 0) fail(OCRS_ERR_INVALID_ARGUMENT, "no lines");
    if (first_op < 0 || first_op > last_op || last_op >= nops)
        fail(OCRS_ERR_INVALID_ARGUMENT, "op range [%d, %d] is not inside the model's ops [0, %d]", first_op, last_op, nops - 1);
    if (gx_only && hm->ops[last_op].type != OP_GRU) fail(OCRS_ERR_INVALID_ARGUMENT, "gx_only: op %d is not a GRU", last_op);
    const int h = (int)rec_input_height();
    const int in_slot = hm->ops[first_op].in0, out_slot = hm->ops[last_op].out, seq_slot = hm->ops[ts].out;
    std::vector<std::vector<TensorShape>> shp(n);
    std::vector<int> T(n);
    for (size_t i = 0; i < n; i++) {
        if (widths[i] < 1) fail(OCRS_ERR_INVALID_ARGUMENT, "line %zu: width %d", i, widths[i]);
        hm->infer(1, h, widths[i], &shp[i]);
        T[i] = shp[i][seq_slot].n;
        if (T[i] <= 0) fail(OCRS_ERR_INVALID_ARGUMENT, "line %zu: width %d gives no sequence", i, widths[i]);
    }
    // lines by width (the width groups of the ragged batch), then by sequence length (rows off[t] + m, as recognize_lines)
    std::map<int32_t, std::vector<size_t>> by_w;
    for (size_t i = 0; i < n; i++) by_w[widths[i]].push_back(i);
    std::vector<size_t> order;   // line order of the ragged layout
    for (auto& kv : by_w) order.insert(order.end(), kv.second.begin(), kv.second.end());
    Workspace ws;
    HipModel::PackedPlan plan;
    uint32_t status[8] = {0};
    plan.h_status = status;
    std::vector<int32_t> layout_T;
    for (size_t i : order) layout_T.push_back(T[i]);
    std::vector<size_t> slot_layout;
    const int32_t* d_pos = HipModel::make_packed_plan(ws, layout_T, &plan, &slot_layout);
    std::vector<int32_t> slot_of(n);   // line i's row slot m
    for (int m = 0; m < plan.M; m++) slot_of[order[slot_layout[m]]] = m;
    const std::vector<int32_t>& hoff = plan.h_off;

    // op first_op's input in the layout of the packed path
    const bool seq_in = first_op > ts;
    const int in_c = shp[0][in_slot].c;
    std::vector<float> packed;
    std::vector<size_t> line_at(n);   // offset of each line's input in `in`
    {
        size_t acc = 0;
        for (size_t i = 0; i < n; i++) {
            if (shp[i][in_slot].c != in_c) fail(OCRS_ERR_INVALID_ARGUMENT, "op %d: input channels differ between lines", first_op);
            line_at[i] = acc;
            acc += (size_t)shp[i][in_slot].count();
        }
        if (acc != in_len) fail(OCRS_ERR_INVALID_ARGUMENT, "input has %zu floats, op %d of these lines reads %zu", in_len, first_op, acc);
    }
    if (seq_in) {
        packed.resize((size_t)plan.R * in_c);
        for (size_t i = 0; i < n; i++)
            for (int t = 0; t < T[i]; t++)
                std::copy_n(in + line_at[i] + (size_t)t * in_c, in_c, &packed[((size_t)hoff[t] + slot_of[i]) * in_c]);
    } else {
        for (size_t i : order) packed.insert(packed.end(), in + line_at[i], in + line_at[i] + shp[i][in_slot].count());
    }

    float* d_in = ws.alloc_n<float>(std::max<size_t>(packed.size(), 1));
    ws.upload(d_in, packed.data(), packed.size() * sizeof(float));
    std::vector<HipModel::PackedGroup> pg;
    {
        size_t at = 0, pos = 0;
        for (auto& kv : by_w) {
            const size_t ng = kv.second.size();
            pg.push_back(HipModel::PackedGroup{d_in + (seq_in ? 0 : at), (int)ng, (int)kv.first, d_pos + pos});
            for (size_t i : kv.second) at += (size_t)shp[i][in_slot].count();
            pos += ng;
        }
    }
    int32_t* d_labels = ws.alloc_n<int32_t>((size_t)plan.R);
    HipModel::OpRange r;
    r.first = first_op;
    r.last = last_op;
    r.gx_only = gx_only;
    r.seq_in = seq_in ? d_in : nullptr;
    r.in_c = in_c;
    hm->run_recognition_packed(ws, pg, plan, h, nullptr, nullptr, d_labels, nullptr, nullptr, &r);

    // op last_op's output, back in line order
    const bool seq_out = last_op >= ts;
    const int oc = r.out_c;
    std::vector<float> host;
    if (seq_out) {
        host.resize((size_t)(gx_only ? 2 : 1) * plan.R * oc);
    } else {
        size_t total = 0;
        for (size_t i = 0; i < n; i++) total += (size_t)shp[i][out_slot].count();
        host.resize(total);
    }
    ws.download(host.data(), r.out, host.size() * sizeof(float));
    ws.sync();
    for (uint32_t st8 : status)
        if (st8) fail(OCRS_ERR_DEVICE, "GRU recurrence kernel timed out waiting for a peer workgroup (status 0x%x)", st8);
    out->clear();
    shapes->clear();
    if (seq_out) {
        for (size_t i = 0; i < n; i++) {
            for (int d = 0; d < (gx_only ? 2 : 1); d++)
                for (int t = 0; t < T[i]; t++) {
                    const float* row = &host[((size_t)d * plan.R + hoff[t] + slot_of[i]) * oc];
                    out->insert(out->end(), row, row + oc);
                }
            shapes->insert(shapes->end(), gx_only ? std::initializer_list<int32_t>{2, T[i], oc} : std::initializer_list<int32_t>{T[i], 1, oc});
        }
    } else {
        std::vector<size_t> at(n);
        size_t acc = 0;
        for (size_t i : order) { at[i] = acc; acc += (size_t)shp[i][out_slot].count(); }
        for (size_t i = 0; i < n; i++) {
            const TensorShape& s = shp[i][out_slot];
            if (s.c != oc) fail(OCRS_ERR_RUN_FAILED, "op %d: %d output channels, the model says %d", last_op, oc, s.c);
            out->insert(out->end(), host.begin() + at[i], host.begin() + at[i] + s.count());
            shapes->insert(shapes->end(), {s.h, s.w, s.c});
        }
    }
}

namespace {

struct Chunk { uint32_t gw; std::vector<size_t> members; int64_t off; float* ptr = nullptr; };

// the model output is [T, lines, alphabet + blank] (recognition.rs:487-493)
void check_rec_output(int ndim, int64_t batch, size_t lines, int classes, size_t alphabet_len) {
    if (ndim != 3)
        fail(OCRS_ERR_WRONG_OUTPUT,
             "model output had unexpected type or shape: expected recognition output to have 3 dims but it has %d", ndim);
    if ((size_t)batch != lines)
        fail(OCRS_ERR_WRONG_OUTPUT, "model output had unexpected type or shape: batch size %lld != %zu", (long long)batch, lines);
    if (alphabet_len + 1 != (size_t)classes)
        fail(OCRS_ERR_WRONG_OUTPUT,
             "model output had unexpected type or shape: output column count (%d) does not match alphabet size (%zu)",
             classes, alphabet_len + 1);
}

// The decoded steps of M lines as the CTC kernels leave them: `stride` entries per line, counts[m] of them used.
struct DecodedSteps {
    int stride = 0;
    std::vector<uint32_t> hl, hp;    // labels, positions
    std::vector<int32_t> hc;         // counts
    std::vector<float> hlp;          // scored on the GPU: step log-probs
    std::vector<double> hscore;      // scored on the GPU: [M] line scores
};

// queues their download on `st` through `w` (d_slp / d_score null: not scored on the GPU)
void download_steps(Workspace& w, hipStream_t st, size_t M, int stride, const uint32_t* d_ol, const uint32_t* d_op, const int32_t* d_cnt,
                    const float* d_slp, const double* d_score, DecodedSteps* d) {
    d->stride = stride;
    d->hl.resize(M * stride);
    d->hp.resize(M * stride);
    d->hc.resize(M);
    w.download(d->hl.data(), d_ol, d->hl.size() * 4, st);
    w.download(d->hp.data(), d_op, d->hp.size() * 4, st);
    w.download(d->hc.data(), d_cnt, M * 4, st);
    if (d_slp) {
        d->hlp.resize(M * stride);
        d->hscore.resize(M);
        w.download(d->hlp.data(), d_slp, d->hlp.size() * sizeof(float), st);
        w.download(d->hscore.data(), d_score, M * sizeof(double), st);
    }
}

// line m's slice of them, as the result's steps (and scores, if they came from the GPU)
void take_steps(const DecodedSteps& d, size_t m, uint32_t ctc_len, RecResult* r) {
    const size_t at = m * d.stride;
    r->steps.resize(d.hc[m]);
    for (int q = 0; q < d.hc[m]; q++) r->steps[q] = CtcStep{d.hl[at + q], d.hp[at + q]};
    r->ctc_len = ctc_len;
    if (!d.hscore.empty()) {
        r->step_logp.assign(d.hlp.data() + at, d.hlp.data() + at + d.hc[m]);
        r->line_score = d.hscore[m];
    }
}

// rten decode_beam (recognition.rs:512-514) on the host for one line of T rows, row(t) its t-th row of C log-probs:
// masked as recognition.rs:547-561 does.  seq: scratch.
template <class Row>
void beam_decode_line(const ocrs_engine& e, int T, int C, Row row, std::vector<float>& seq, bool scored, RecResult* r) {
    seq.resize((size_t)T * C);
    for (int t = 0; t < T; t++) {
        const float* src = row(t);
        for (int c = 0; c < C; c++)
            seq[(size_t)t * C + c] = (e.has_excluded && e.excluded[c]) ? -std::numeric_limits<float>::infinity() : src[c];
    }
    double bs = 0.0;
    r->steps = ctc_beam_search(seq.data(), T, C, C, e.beam_width, scored ? &bs : nullptr);
    r->ctc_len = (uint32_t)T;
    if (scored) score_line(seq.data(), T, C, C, nullptr, r->steps, &bs, &r->step_logp, &r->line_score);
}

// ---- `trait Model` implemented by the caller: one run per <=20-line chunk (recognition.rs:485)
void recognize_callback(const ocrs_engine& e, Workspace& ws, const std::vector<Chunk>& chunks, RecResult* res, bool scored) {
    const auto* cb = static_cast<const CallbackModel*>(e.recognition);
    const bool beam = e.decode_method == OCRS_DECODE_BEAM_SEARCH;
    const uint32_t rec_h = e.rec_input_height();
    const uint8_t* d_excl = e.has_excluded ? e.d_excluded.as<uint8_t>() : nullptr;
    hipStream_t st = ws.s();
    std::vector<float> seq;
    for (const Chunk& ch : chunks) {
        const size_t nb = ch.members.size();
        const uint32_t gw = ch.gw;
        std::vector<float> hin(nb * rec_h * gw), hout;
        ws.download(hin.data(), ch.ptr, hin.size() * sizeof(float));
        ws.sync();
        const int64_t ishape[4] = {(int64_t)nb, 1, rec_h, gw};
        int64_t oshape[4] = {0, 0, 0, 0};
        int ond = 0;
        cb->run(hin.data(), ishape, hout, oshape, &ond);
        check_rec_output(ond, oshape[1], nb, (int)oshape[2], e.alphabet.size());
        const int Tn = (int)oshape[0], C = (int)oshape[2];
        if (beam) {  // decode_beam on the model output: line j's row t is hout[(t * nb + j) * C]
            for (size_t j = 0; j < nb; j++)
                beam_decode_line(e, Tn, C, [&](int t) { return &hout[((size_t)t * nb + j) * C]; }, seq, scored, &res[ch.members[j]]);
            continue;
        }
        float* d_logp = ws.alloc_n<float>(hout.size());
        OCRS_HIP(hipMemcpyAsync(d_logp, hout.data(), hout.size() * sizeof(float), hipMemcpyHostToDevice, st));
        int32_t* d_labels = ws.alloc_n<int32_t>((size_t)Tn * nb);
        uint32_t* d_ol = ws.alloc_n<uint32_t>((size_t)nb * Tn);
        uint32_t* d_op = ws.alloc_n<uint32_t>((size_t)nb * Tn);
        int32_t* d_cnt = ws.alloc_n<int32_t>(nb);
        {
            StageScope sc(e.tm(), ST_CTC, st, 2);
            k::argmax_rows(d_logp, (int64_t)Tn * nb, C, d_excl, d_labels, st);
            k::ctc_collapse(d_labels, Tn, (int)nb, d_ol, d_op, d_cnt, st);  // recognition.rs:511
        }
        DecodedSteps dec;
        download_steps(ws, st, nb, Tn, d_ol, d_op, d_cnt, nullptr, nullptr, &dec);
        ws.sync();
        for (size_t j = 0; j < nb; j++) {
            RecResult& r = res[ch.members[j]];
            take_steps(dec, j, (uint32_t)Tn, &r);
            if (scored)   // the model output is on the host already: line j's row t is hout[(t * nb + j) * C]
                score_line(&hout[j * C], Tn, C, nb * (size_t)C, e.has_excluded ? e.excluded.data() : nullptr, r.steps, nullptr,
                           &r.step_logp, &r.line_score);
        }
    }
}

// ---- fixed-graph HIP executor: all width groups in ONE ragged batch.  Each line keeps the
// padded width (hence sequence length) the reference gives it (recognition.rs:437), lines are
// sorted by length so that step t of the recurrence works on a dense prefix of rows.
struct Slot { int T; size_t line; };
struct PackedDecode {   // what the decode stage of one ragged batch leaves for the host
    DecodedSteps dec;              // greedy, or beam search done on the GPU
    bool gpu_beam = false;         // beam search already done on the GPU: dec holds its steps
    std::vector<float> logp;       // beam search on the host / logits wanted: packed [R][C]
    std::vector<int32_t> off;      // with logp
};
struct Sub : PackedDecode {   // one ragged batch of a request: what its launches leave for the host
    std::vector<Slot> slots;
    uint32_t gru_status[8] = {0};  // time-out words of the persistent GRU kernels (0 = fine)
};
struct PackedRequest {   // what the sub-batches of one request share
    const ocrs_engine& e;
    const HipModel* hm;
    const std::vector<Chunk>& chunks;
    std::vector<int> chunk_T;   // each chunk's sequence length
    int C;                      // classes
    bool scored, want_logp;
    RecResult* res;
};

// The decode stage of a packed batch, after the head: the labels / log-probs / row maxima log_softmax_argmax left on the
// device (d_logp: beam search or want_logp; d_maxlp: scored greedy) become the steps of the M lines — the CTC launch on
// `w`'s stream and the queued downloads of what the host needs.  The engine's launch_packed and the test hook
// ctc_decode_packed both end in it.
void decode_packed(Workspace& w, const HipModel::PackedPlan& plan, int C, bool beam, uint32_t beam_width, bool scored,
                   bool want_logp, const uint8_t* d_excl, const int32_t* d_labels, const float* d_logp, const float* d_maxlp,
                   StageTimers* T, PackedDecode& sub) {
    hipStream_t sst = w.s();
    const int M = plan.M, Tmax = plan.Tmax;
    sub.gpu_beam = beam && option(OPT_BEAM_GPU) && k::ctc_beam_supported(C, (int)beam_width);
    if (want_logp || (beam && !sub.gpu_beam)) {   // the host needs the log-probs: the caller, or its beam search
        sub.logp.resize((size_t)plan.R * C);
        sub.off = plan.h_off;
        w.download(sub.logp.data(), d_logp, sub.logp.size() * sizeof(float), sst);
    }
    if (beam && !sub.gpu_beam) return;
    // where the steps land: [M][Tmax] labels and positions, [M] counts; scored: step log-probs and line scores as well
    int2* d_nodes = nullptr;
    int2* d_posn = nullptr;
    if (sub.gpu_beam) {
        const size_t arena = k::ctc_beam_arena_entries(Tmax, (int)beam_width);
        d_nodes = w.alloc_n<int2>((size_t)M * arena);
        d_posn = w.alloc_n<int2>((size_t)M * arena);
    }
    uint32_t* d_ol = w.alloc_n<uint32_t>((size_t)M * Tmax);
    uint32_t* d_op = w.alloc_n<uint32_t>((size_t)M * Tmax);
    int32_t* d_cnt = w.alloc_n<int32_t>(M);
    float* d_slp = scored ? w.alloc_n<float>((size_t)M * Tmax) : nullptr;
    double* d_score = scored ? w.alloc_n<double>(M) : nullptr;
    {
        StageScope sc(T, ST_CTC, sst);
        if (sub.gpu_beam)   // rten decode_beam (recognition.rs:512-514) on the GPU, one workgroup per line (kernels_beam.hip)
            k::ctc_beam_packed(d_logp, plan.d_Tm, plan.d_off, M, Tmax, C, (int)beam_width, d_excl, d_nodes, d_posn, d_ol, d_op, d_cnt,
                               sst, d_score, d_slp);
        else if (scored)   // greedy CTC with each step's log-prob and the greedy path's score, in one pass
            k::ctc_collapse_scored_packed(d_labels, d_maxlp, plan.d_Tm, plan.d_off, M, Tmax, d_ol, d_op, d_slp, d_cnt, d_score, sst);
        else   // greedy CTC (recognition.rs:511)
            k::ctc_collapse_packed(d_labels, plan.d_Tm, plan.d_off, M, Tmax, d_ol, d_op, d_cnt, sst);
    }
    download_steps(w, sst, (size_t)M, Tmax, d_ol, d_op, d_cnt, d_slp, d_score, &sub.dec);
}

// launches chunks [c0, c1) as one ragged batch on `w` and queues the downloads of what unpack_packed needs
void launch_packed(const PackedRequest& rq, size_t c0, size_t c1, Workspace& w, Sub& sub) {
    const ocrs_engine& e = rq.e;
    const bool beam = e.decode_method == OCRS_DECODE_BEAM_SEARCH;
    const uint8_t* d_excl = e.has_excluded ? e.d_excluded.as<uint8_t>() : nullptr;
    StageTimers* T = e.tm();
    const int C = rq.C;
    std::vector<int32_t> lineT;                      // the lines of chunks c0 .. c1 in chunk order
    std::vector<size_t> line_of;                     // and which line of the request each is
    std::vector<size_t> pos_at(c1 - c0);             // index of each chunk's first line
    for (size_t c = c0; c < c1; c++) {
        pos_at[c - c0] = lineT.size();
        for (size_t li : rq.chunks[c].members) {
            lineT.push_back(rq.chunk_T[c]);
            line_of.push_back(li);
        }
    }
    HipModel::PackedPlan plan;
    plan.h_status = sub.gru_status;
    std::vector<size_t> order;
    const int32_t* d_pos = HipModel::make_packed_plan(w, lineT, &plan, &order);
    if (!d_pos) return;
    for (size_t i : order) sub.slots.push_back(Slot{lineT[i], line_of[i]});
    std::vector<HipModel::PackedGroup> pg;
    for (size_t c = c0; c < c1; c++)
        if (rq.chunk_T[c] > 0)
            pg.push_back(HipModel::PackedGroup{rq.chunks[c].ptr, (int)rq.chunks[c].members.size(), (int)rq.chunks[c].gw,
                                               d_pos + pos_at[c - c0]});
    int32_t* d_labels = w.alloc_n<int32_t>((size_t)plan.R);
    float* d_logp = nullptr;
    float* d_maxlp = (rq.scored && !beam) ? w.alloc_n<float>((size_t)plan.R) : nullptr;
    rq.hm->run_recognition_packed(w, pg, plan, (int)e.rec_input_height(), T, d_excl, d_labels, (beam || rq.want_logp) ? &d_logp : nullptr,
                                  d_maxlp);
    decode_packed(w, plan, C, beam, e.beam_width, rq.scored, rq.want_logp, d_excl, d_labels, d_logp, d_maxlp, T, sub);
}

// after the sync: the request's results from what launch_packed downloaded
void unpack_packed(const PackedRequest& rq, const Sub& sub) {
    const ocrs_engine& e = rq.e;
    const int C = rq.C;
    const size_t M = sub.slots.size();
    for (uint32_t st8 : sub.gru_status)
        if (st8) fail(OCRS_ERR_DEVICE, "GRU recurrence kernel timed out waiting for a peer workgroup (status 0x%x)", st8);
    auto row = [&](size_t m, int t) { return &sub.logp[((size_t)sub.off[t] + m) * C]; };
    if (rq.want_logp)
        for (size_t m = 0; m < M; m++) {
            auto& dst = rq.res[sub.slots[m].line].logp;
            dst.resize((size_t)sub.slots[m].T * C);
            for (int t = 0; t < sub.slots[m].T; t++) memcpy(&dst[(size_t)t * C], row(m, t), (size_t)C * sizeof(float));
        }
    if (e.decode_method == OCRS_DECODE_BEAM_SEARCH && !sub.gpu_beam) {  // host side, one thread per slice of lines
        const unsigned nth = (unsigned)std::max<size_t>(1, std::min<size_t>({(size_t)std::thread::hardware_concurrency(), (size_t)32, M}));
        std::vector<std::thread> th;
        for (unsigned w0 = 0; w0 < nth; w0++)
            th.emplace_back([&, w0] {
                std::vector<float> seq;
                for (size_t m = w0; m < M; m += nth)
                    beam_decode_line(e, sub.slots[m].T, C, [&](int t) { return row(m, t); }, seq, rq.scored, &rq.res[sub.slots[m].line]);
            });
        for (auto& t : th) t.join();
        return;
    }
    for (size_t m = 0; m < M; m++) take_steps(sub.dec, m, (uint32_t)sub.slots[m].T, &rq.res[sub.slots[m].line]);
}

void recognize_packed(const ocrs_engine& e, Workspace& ws, const std::vector<Chunk>& chunks, RecResult* res, bool scored, bool want_logp) {
    const auto* hm = static_cast<const HipModel*>(e.recognition);
    PackedRequest rq{e, hm, chunks, std::vector<int>(chunks.size()), 0, scored, want_logp, res};
    int ndim = hm->packed_split() < 0 ? 4 : 3;
    for (size_t c = 0; c < chunks.size() && ndim == 3; c++) {
        TensorShape os = hm->infer(1, (int)e.rec_input_height(), (int)chunks[c].gw);
        if (!os.seq) ndim = 4;
        rq.chunk_T[c] = os.n;
        rq.C = os.c;
    }
    check_rec_output(ndim, 0, 0, rq.C, e.alphabet.size());
    // Two ragged batches when the request mixes long and short lines: the recurrence is a chain
    // of up to 600 dependent, latency-bound steps whose tail only involves the few longest lines.
    // The long groups run first, on a light lane other than this call's own (a stream of their own at stream budget 0),
    // taken only when the request does split; their recurrence then overlaps the conv stack of the short groups (the
    // bulk of the FLOPs) on this call's main stream.
    const int T_SPLIT = 160;
    size_t first_long = chunks.size();
    for (size_t c = 0; c < chunks.size(); c++)
        if (rq.chunk_T[c] > T_SPLIT) { first_long = c; break; }
    size_t n_long_lines = 0, n_short_lines = 0;
    for (size_t c = 0; c < chunks.size(); c++) (c >= first_long ? n_long_lines : n_short_lines) += chunks[c].members.size();
    const bool split = n_long_lines > 0 && n_short_lines >= 64;
    Sub sub_long, sub_short;
    if (split) {
        Workspace ws_long(true, ws.stream.lane());
        if (ws_long.s() != ws.s()) {   // the crops were produced on ws's stream: the long lines' stream starts after them
            hipEvent_t crops = ws.make_event();   // (light-lane work, runnable as queued: a lane may wait for it)
            OCRS_HIP(hipEventRecord(crops, ws.s()));
            OCRS_HIP(hipStreamWaitEvent(ws_long.s(), crops, 0));
        }
        if (ws.stream.may_park_waits()) {
            launch_packed(rq, first_long, chunks.size(), ws_long, sub_long);
            launch_packed(rq, 0, first_long, ws, sub_short);
            ws_long.sync();
            ws.sync();
        } else {
            // On shared lanes a batch's host thread waits for its conv stack and its recurrences (stream_plan.hpp): the
            // long lines get a host thread of their own for the length of this call, or nothing would overlap.
            std::exception_ptr long_error;
            const Tuning* tuning = current_tuning();
            const int device = ctx().device;
            std::thread long_thread([&] {
                try {
                    DeviceScope bind(device);
                    TuningScope tune(tuning);
                    launch_packed(rq, first_long, chunks.size(), ws_long, sub_long);
                    ws_long.sync();
                    if (StageTimers* T = e.tm()) T->collect();
                } catch (...) {
                    long_error = std::current_exception();
                }
                StageTimers::release_thread_events();
            });
            struct Join { std::thread& t; ~Join() { if (t.joinable()) t.join(); } } join{long_thread};
            launch_packed(rq, 0, first_long, ws, sub_short);
            ws.sync();
            long_thread.join();
            if (long_error) std::rethrow_exception(long_error);
        }
        unpack_packed(rq, sub_long);
        unpack_packed(rq, sub_short);
    } else {
        launch_packed(rq, 0, chunks.size(), ws, sub_short);
        ws.sync();
        unpack_packed(rq, sub_short);
    }
}

}  // namespace

void ocrs::ctc_decode_packed(const float* logits, const int32_t* T, size_t n, int C, const uint8_t* excluded, int method,
                             uint32_t width, bool want_logp, std::vector<RecResult>* res) {
    const bool beam = method >= 2, scored = (method & 1) != 0;
    if (beam && !k::ctc_beam_supported(C, (int)width))
        fail(OCRS_ERR_CAPACITY, "beam search on the GPU supports up to 128 classes and width 128");
    res->assign(n, RecResult{});
    DeviceScope bind(-1);
    Workspace w;
    const std::vector<int32_t> lineT(T, T + n);
    HipModel::PackedPlan plan;
    std::vector<size_t> order;
    if (!HipModel::make_packed_plan(w, lineT, &plan, &order)) return;   // no line has a row
    const int M = plan.M;
    std::vector<size_t> at(n + 1, 0);   // offset of each line's rows in `logits`
    for (size_t i = 0; i < n; i++) at[i + 1] = at[i] + (size_t)lineT[i] * C;
    std::vector<float> packed((size_t)plan.R * C);   // line order[m]'s row t at packed row off[t] + m
    for (int m = 0; m < M; m++)
        for (int t = 0; t < plan.h_Tm[m]; t++)
            std::copy_n(logits + at[order[m]] + (size_t)t * C, C, &packed[((size_t)plan.h_off[t] + m) * C]);
    float* d_logits = w.alloc_n<float>(packed.size());
    w.upload(d_logits, packed.data(), packed.size() * sizeof(float));
    uint8_t* d_excl = nullptr;
    if (excluded) {
        d_excl = w.alloc_n<uint8_t>(C);
        w.upload(d_excl, excluded, C);
    }
    // what run_recognition_packed's LOGSOFTMAX step and launch_packed do after the head GEMM
    int32_t* d_labels = w.alloc_n<int32_t>((size_t)plan.R);
    float* d_logp = (beam || want_logp) ? w.alloc_n<float>((size_t)plan.R * C) : nullptr;
    float* d_maxlp = (scored && !beam) ? w.alloc_n<float>((size_t)plan.R) : nullptr;
    if (!k::log_softmax_argmax(d_logits, plan.R, C, d_excl, d_logp, d_labels, w.s(), d_maxlp))
        fail(OCRS_ERR_CAPACITY, "LogSoftmax over %d classes exceeds the kernel's LDS staging (max ~630)", C);
    PackedDecode out;
    decode_packed(w, plan, C, beam, width, scored, want_logp, d_excl, d_labels, d_logp, d_maxlp, nullptr, out);
    w.sync();
    OCRS_HIP(hipGetLastError());
    if (beam && !out.gpu_beam) fail(OCRS_ERR_RUN_FAILED, "option beam_gpu is off: the beam kernel did not run");
    for (int m = 0; m < M; m++) {
        RecResult& r = (*res)[order[m]];
        const int Tm = plan.h_Tm[m];
        if (want_logp) r.logp.resize((size_t)Tm * C);
        for (int t = 0; t < Tm && want_logp; t++) std::copy_n(&out.logp[((size_t)out.off[t] + m) * C], C, &r.logp[(size_t)t * C]);
        take_steps(out.dec, (size_t)m, (uint32_t)Tm, &r);
    }
}

void ocrs::mask_component_rects(const uint8_t* masks, int n, int h, int w, float expand, float min_area, int max_comp, int64_t arena,
                                int32_t* n_roots, int32_t* overflow, float* rects, uint8_t* valid) {
    DeviceScope bind(-1);
    Workspace ws;
    const int64_t px = (int64_t)h * w;
    uint8_t* d_mask = ws.alloc_n<uint8_t>((size_t)n * px);
    ws.upload(d_mask, masks, (size_t)n * px);
    const k::CclBuffers b = alloc_ccl(ws, n, h, px, max_comp, arena, false, true);
    // slots the contour kernel leaves unwritten are recognisable: valid 0xEE (the kernel writes 0 or 1), rects all-ones words
    OCRS_HIP(hipMemsetAsync(b.valid, 0xEE, (size_t)n * max_comp, ws.s()));
    OCRS_HIP(hipMemsetAsync(b.rects, 0xFF, (size_t)n * max_comp * 6 * sizeof(float), ws.s()));
    // what run_ccl does for an unscored, unprepared size group
    k::ccl_label(d_mask, n, h, w, b, max_comp, ws.s(), false);
    k::contour_rects(d_mask, n, h, w, b, max_comp, arena, expand, min_area, /*eps*/ 2.0f, ws.s(), false);
    ws.download(n_roots, b.n_roots, (size_t)n * sizeof(int32_t));
    ws.download(overflow, b.overflow, (size_t)n * sizeof(int32_t));
    ws.download(rects, b.rects, (size_t)n * max_comp * 6 * sizeof(float));
    ws.download(valid, b.valid, (size_t)n * max_comp);
    ws.sync();
    OCRS_HIP(hipGetLastError());
}

void ocrs_engine::recognize_lines(const ocrs_page* const* pages, size_t n_pages, RecResult* res, size_t L, bool scored,
                                  bool want_logp) const {
    if (L == 0) return;
    const uint32_t rec_h = rec_input_height();
    const bool callback = recognition->is_callback();

    // group by padded width (recognition.rs:430-446); std::map gives a deterministic order
    std::map<uint32_t, std::vector<size_t>> groups;
    for (size_t i = 0; i < L; i++) groups[res[i].line.group_width].push_back(i);

    Workspace ws;
    std::vector<Chunk> chunks;
    std::vector<CropLine> crops;
    int64_t off = 0;
    for (auto& kv : groups) {
        const uint32_t gw = kv.first;
        if (gw == 0) continue;  // zero-width lines produce no input and no text
        // reference: chunks of 20 (recognition.rs:450); rows are independent, so the HIP
        // executor takes bigger chunks, bounded by activation memory (~8 KB per input pixel column).
        const size_t max_chunk = callback ? 20 : std::max<size_t>(1, 2457600 / gw);
        for (size_t c0 = 0; c0 < kv.second.size(); c0 += max_chunk) {
            Chunk ch;
            ch.gw = gw;
            ch.members.assign(kv.second.begin() + c0, kv.second.begin() + std::min(kv.second.size(), c0 + max_chunk));
            ch.off = off;
            for (size_t li : ch.members) {
                crops.push_back(CropLine{&res[li].line, gw, off});
                off += (int64_t)rec_h * gw;
            }
            chunks.push_back(std::move(ch));
        }
    }
    // (ocrs_engine::recognize_now keeps a request within the activation budget; a single line beyond it is refused)
    if ((double)off > std::max(rec_pixel_budget(), 2.0e9))
        fail(OCRS_ERR_CAPACITY, "text line too large for the recognition model (%lld input pixels)", (long long)off);
    float* d_all = stage_line_crops(ws, tm(), pages, n_pages, crops, (int)rec_h, off);
    if (!d_all) return;
    for (Chunk& ch : chunks) ch.ptr = d_all + ch.off;
    if (callback) {
        ws.sync();   // the callback path reads the crops back right away
        recognize_callback(*this, ws, chunks, res, scored);
    } else {
        recognize_packed(*this, ws, chunks, res, scored, want_logp);
    }
    if (StageTimers* T = tm()) T->collect();
}

// recognition.rs:241-311 for one line
std::vector<TextChar> ocrs_engine::text_line_from_result(const RecResult& res, std::vector<float>* char_logp) const {
    const RecLine& line = res.line;
    const uint32_t ctc_input_len = res.ctc_len;
    const std::vector<CtcStep>& steps = res.steps;
    std::vector<TextChar> out;
    if (char_logp) char_logp->clear();
    if (steps.empty() || ctc_input_len == 0) return out;
    if (line.rectified) {
        std::vector<uint32_t> pos(steps.size());
        for (size_t i = 0; i < steps.size(); i++) pos[i] = steps[i].pos;
        for (const auto& kv : rectified_char_boxes(line.frame, line.group_width, ctc_input_len, pos.data(), pos.size())) {
            const uint32_t idx = steps[kv.first].label - 1;
            out.push_back(TextChar{idx < alphabet.size() ? (uint32_t)alphabet[idx] : (uint32_t)'?', kv.second});
            if (char_logp) char_logp->push_back(res.step_logp[kv.first]);
        }
        return out;
    }
    const Rect line_rect = line.bounds;
    const float x_scale = (float)line_rect.width() / (float)line.resized_width;
    const uint32_t downsample = (uint32_t)rround((float)line.group_width / (float)ctc_input_len);
    for (size_t i = 0; i < steps.size(); i++) {
        const uint32_t start_x = steps[i].pos * downsample;
        const uint32_t end_x = i + 1 < steps.size() ? steps[i + 1].pos * downsample : line.resized_width;
        const int32_t sx = line_rect.left + as_i32((float)start_x * x_scale);
        const int32_t ex = line_rect.left + as_i32((float)end_x * x_scale);
        if (sx >= line_rect.right) continue;  // character starts in the padding
        const uint32_t idx = steps[i].label - 1;
        const uint32_t ch = idx < alphabet.size() ? (uint32_t)alphabet[idx] : (uint32_t)'?';
        Rect r;
        if (!polygon_slice_bounding_rect(line.polygon, sx, ex, &r))
            fail(OCRS_ERR_RUN_FAILED, "invalid X coords");  // recognition.rs:299
        out.push_back(TextChar{ch, r});
        if (char_logp) char_logp->push_back(res.step_logp[i]);   // padding steps are skipped with their chars
    }
    return out;
}
