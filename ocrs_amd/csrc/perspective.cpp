// Perspective correction (include/ocrs_amd.h "Perspective correction"): the edge peaks of resident pages,
// the outline chosen among them, the projective page warp that straightens the sheet, and the host maps that bring results
// of the projected page back to the photo's frame.  The kernels are in kernels_perspective.hip, the host arithmetic in
// perspective_math.hpp; tests/perspective_ref.py is the definition.
#include <algorithm>
#include <cmath>
#include <limits>

#include "abi_util.hpp"
#include "engine.hpp"
#include "kernels.hpp"
#include "page_ops.hpp"
#include "perspective_math.hpp"

using namespace ocrs;
using namespace ocrs::abi;

namespace {

constexpr size_t EDGE_MAX_ANGLES = 65535;
constexpr size_t CHOOSE_MAX_ANGLES = 4095;   // what persp::plan() allows: 2 K + 1

void check_table(const int32_t* sc_table, size_t n_angles) {
    if (n_angles < 1 || n_angles > EDGE_MAX_ANGLES) fail(OCRS_ERR_INVALID_ARGUMENT, "edge peaks: %zu angles: 1 .. %zu", n_angles, EDGE_MAX_ANGLES);
    for (size_t i = 0; i < 2 * n_angles; i++)
        if (sc_table[i] > persp::Q16 || sc_table[i] < -persp::Q16)
            fail(OCRS_ERR_INVALID_ARGUMENT, "edge peaks: table entry %zu is %d: Q16 sines and cosines lie within +-%d", i, sc_table[i], persp::Q16);
}

void check_min_step(int min_step) {
    if (min_step < 1 || min_step > 256) fail(OCRS_ERR_INVALID_ARGUMENT, "edge peaks: min_step %d: 1 .. 256", min_step);
}

// peaks[n][2][2][A][16] of the pages, every page and angle in two launches on `ws`'s stream; waits for them
void edge_peaks(Workspace& ws, const ocrs_page* const* pages, size_t n, const int32_t* sc_table, size_t n_angles, int min_step, uint64_t* out_peaks) {
    if (n == 0) return;
    if (n > 65535) fail(OCRS_ERR_CAPACITY, "edge peaks: %zu pages in one call: at most 65535", n);
    std::vector<k::EdgeDesc> descs(n);
    int64_t blocks = 0;
    size_t dwords = 0;
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        if (p->h > persp::MAX_SIDE || p->w > persp::MAX_SIDE)
            fail(OCRS_ERR_INVALID_ARGUMENT, "edge peaks: a page of %d x %d: a side is at most %d (find the outline on a work copy)", p->h, p->w, persp::MAX_SIDE);
        k::EdgeDesc& d = descs[i];
        d.src = p->grey.as<float>();
        d.h = p->h;
        d.w = p->w;
        d.nb = p->h + p->w;
        d.block0 = (int32_t)blocks;
        blocks += k::edge_tiles(p->h, p->w);
        dwords += 4 * n_angles * (size_t)d.nb;
        if (blocks > std::numeric_limits<int32_t>::max() || dwords > ((size_t)1 << 29))
            fail(OCRS_ERR_CAPACITY, "edge peaks: the profiles of one call take more than 2 GiB");
    }
    const size_t per_page = 4 * n_angles * (size_t)persp::BANDS;
    uint32_t* d_prof = ws.alloc_n<uint32_t>(dwords);
    unsigned long long* d_peaks = ws.alloc_n<unsigned long long>(n * per_page);
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        descs[i].prof = d_prof + at;
        descs[i].peaks = d_peaks + i * per_page;
        at += 4 * n_angles * (size_t)descs[i].nb;
    }
    k::EdgeDesc* d_descs = ws.alloc_n<k::EdgeDesc>(n);
    int32_t* d_table = ws.alloc_n<int32_t>(2 * n_angles);
    ws.upload(d_descs, descs.data(), n * sizeof(k::EdgeDesc));
    ws.upload(d_table, sc_table, 2 * n_angles * sizeof(int32_t));
    OCRS_HIP(hipMemsetAsync(d_prof, 0, dwords * sizeof(uint32_t), ws.s()));
    k::edge_peaks(d_descs, (int)n, (int)blocks, d_table, (int)n_angles, min_step, ws.s());
    OCRS_HIP(hipGetLastError());
    ws.download(out_peaks, d_peaks, n * per_page * sizeof(uint64_t));
    ws.sync();
}

persp::Params to_params(const ocrs_outline_params& p) {
    return {p.max_deg, p.step_deg, p.min_cover, p.min_span, p.min_area, p.work_max_side, p.min_step};
}

long check_outline_params(const ocrs_outline_params& p) {
    const long K = persp::plan(to_params(p));
    if (K < 1)
        fail(OCRS_ERR_INVALID_ARGUMENT,
             "outline: work_max_side 1 .. %d, min_step 1 .. 256, max_deg in (0, 45], a finite positive step_deg that max_deg holds 1 .. 2047 of, "
             "min_cover and min_span in (0, 1], min_area in [0, 1]", persp::MAX_SIDE);
    return K;
}

void fill_info(const persp::Outline& o, int wh, int ww, ocrs_outline_info* out) {
    out->found = o.found;
    out->polarity = o.polarity;
    for (int i = 0; i < 8; i++) out->corners[i] = o.corners[i];
    for (int i = 0; i < 4; i++) {
        out->counts[i] = o.counts[i];
        out->angles[i] = o.angles[i];
    }
    out->work_h = wh;
    out->work_w = ww;
}

void check_map8(const float* m) {
    for (int i = 0; i < 8; i++)
        if (!std::isfinite(m[i])) fail(OCRS_ERR_INVALID_ARGUMENT, "a map coefficient that is not finite");
}

// every page projected into a new page of its own, all in one launch on `ws`'s stream; waits for it
PageBatch<k::ProjDesc> project_pages(Workspace& ws, const ocrs_page* const* pages, size_t n, const int* out_hw, const float* m, const float* fill) {
    PageBatch<k::ProjDesc> batch{"project"};
    for (size_t i = 0; i < n; i++) {
        const int oh = out_hw[2 * i], ow = out_hw[2 * i + 1];
        if (oh < 1 || oh > MAX_PAGE_SIDE || ow < 1 || ow > MAX_PAGE_SIDE)
            fail(OCRS_ERR_INVALID_ARGUMENT, "project: %d x %d: a side is 1 .. %d", oh, ow, MAX_PAGE_SIDE);
        check_page_side("project", pages[i]);
        check_map8(m + 8 * i);
    }
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        k::ProjDesc& d = batch.add(out_hw[2 * i], out_hw[2 * i + 1], k::project_blocks(out_hw[2 * i], out_hw[2 * i + 1]));
        d.src = p->grey.as<float>();
        d.dst = batch.made.back()->grey.as<float>();
        d.sh = p->h;
        d.sw = p->w;
        d.dh = out_hw[2 * i];
        d.dw = out_hw[2 * i + 1];
        d.vec = vec16_ok(d.dw, d.dst, d.dst) ? 1 : 0;
        for (int q = 0; q < 8; q++) d.m[q] = m[8 * i + q];
        d.fill = fill[i];
    }
    batch.run(ws, [&](const k::ProjDesc* d_descs, int n_pages, int blocks) { k::project_pages(d_descs, n_pages, blocks, ws.s()); });
    return batch;
}

}  // namespace

extern "C" {

ocrs_status ocrs_outline_params_default(ocrs_outline_params* out) {
    return guarded([&] {
        if (!out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        const persp::Params p = persp::default_params();
        out->max_deg = p.max_deg;
        out->step_deg = p.step_deg;
        out->min_cover = p.min_cover;
        out->min_span = p.min_span;
        out->min_area = p.min_area;
        out->work_max_side = p.work_max_side;
        out->min_step = p.min_step;
    });
}

ocrs_status ocrs_outline_params_check(const ocrs_outline_params* params) {
    return guarded([&] {
        if (!params) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        (void)check_outline_params(*params);
    });
}

ocrs_status ocrs_engine_edge_peaks(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const int32_t* sc_table, size_t n_angles,
                                   int min_step, uint64_t* out_peaks) {
    return guarded_engine(e, [&] {
        if (!e || !sc_table || (n > 0 && (!pages || !out_peaks))) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_table(sc_table, n_angles);
        check_min_step(min_step);
        check_pages_on(e, pages, n);
        Workspace ws;
        edge_peaks(ws, pages, n, sc_table, n_angles, min_step, out_peaks);
    });
}

ocrs_status ocrs_outline_choose(const uint64_t* peaks, const int32_t* sc_table, size_t n_angles, int work_h, int work_w, int page_h, int page_w,
                                const ocrs_outline_params* params, ocrs_outline_info* out) {
    return guarded([&] {
        if (!peaks || !sc_table || !out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        // the pair search is quadratic in the candidates, 16 per angle and sign: the limit of the search's own tables
        if (n_angles > CHOOSE_MAX_ANGLES) fail(OCRS_ERR_INVALID_ARGUMENT, "outline: %zu angles: the choice takes at most %zu", n_angles, CHOOSE_MAX_ANGLES);
        ocrs_outline_params p;
        if (params) p = *params;
        else ocrs_outline_params_default(&p);
        (void)check_outline_params(p);
        check_table(sc_table, n_angles);
        if (work_h < 1 || work_w < 1 || work_h > persp::MAX_SIDE || work_w > persp::MAX_SIDE || page_h < 1 || page_w < 1)
            fail(OCRS_ERR_INVALID_ARGUMENT, "outline: a work page of %d x %d from a page of %d x %d", work_h, work_w, page_h, page_w);
        fill_info(persp::choose(peaks, sc_table, n_angles, work_h, work_w, page_h, page_w, to_params(p)), work_h, work_w, out);
    });
}

ocrs_status ocrs_engine_find_outline(const ocrs_engine* e, const ocrs_page* page, const ocrs_outline_params* params, ocrs_outline_info* out) {
    return guarded_engine(e, [&] {
        if (!e || !page || !out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        ocrs_outline_params p;
        if (params) p = *params;
        else ocrs_outline_params_default(&p);
        const long K = check_outline_params(p);
        check_pages_on(e, &page, 1);
        // 1. the work copy: the area average, when the page is larger than work_max_side
        std::unique_ptr<ocrs_page> work;
        const ocrs_page* wp = page;
        if (std::max(page->h, page->w) > p.work_max_side) {
            int wh = 0, ww = 0;
            ocrs_page* made = nullptr;
            ocrs_status s = ocrs_work_size(page->h, page->w, (double)p.work_max_side / (double)std::max(page->h, page->w), &wh, &ww);
            if (s == OCRS_OK) s = ocrs_engine_resize_page(e, page, wh, ww, OCRS_RESAMPLE_AREA, &made);
            if (s != OCRS_OK) fail(s, "outline: %s", ocrs_last_error());
            work.reset(made);
            wp = made;
        }
        // 2. the peaks at the angles -K .. K steps
        const size_t A = (size_t)(2 * K + 1);
        std::vector<int32_t> table(2 * A);
        const ocrs_status ts = ocrs_skew_table((int)-K, A, p.step_deg, table.data());
        if (ts != OCRS_OK) fail(ts, "outline: %s", ocrs_last_error());
        std::vector<uint64_t> peaks(4 * A * (size_t)persp::BANDS);
        {
            Workspace ws;
            edge_peaks(ws, &wp, 1, table.data(), A, p.min_step, peaks.data());
        }
        // 3. the choice, on the host
        fill_info(persp::choose(peaks.data(), table.data(), A, wp->h, wp->w, page->h, page->w, to_params(p)), wp->h, wp->w, out);
    });
}

ocrs_status ocrs_quad_map(const float corners8[8], int out_hw[2], float m[8]) {
    return guarded([&] {
        if (!corners8 || !out_hw || !m) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        int hw[2];
        float mm[8];
        if (!persp::quad_map(corners8, hw, mm)) fail(OCRS_ERR_INVALID_ARGUMENT, "quad map: a corner that is not finite, or a quad without area");
        out_hw[0] = hw[0];
        out_hw[1] = hw[1];
        for (int i = 0; i < 8; i++) m[i] = mm[i];
    });
}

ocrs_status ocrs_engine_project_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const int* out_hw, const float* m,
                                      const float* fill, ocrs_page** out) {
    return guarded_engine(e, [&] {
        if (!e || (n > 0 && (!pages || !out_hw || !m || !fill || !out))) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_pages_on(e, pages, n);
        Workspace ws;
        project_pages(ws, pages, n, out_hw, m, fill).release_into(out);
    });
}

ocrs_status ocrs_engine_project_page(const ocrs_engine* e, const ocrs_page* page, int out_h, int out_w, const float m[8], float fill,
                                     ocrs_page** out) {
    const int hw[2] = {out_h, out_w};
    return ocrs_engine_project_pages(e, &page, 1, hw, m, &fill, out);
}

ocrs_status ocrs_unproject_rects(float* rects6, size_t n, const float m[8]) {
    return guarded([&] {
        if (!m || (n > 0 && !rects6)) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_map8(m);
        for (size_t i = 0; i < n; i++) persp::unproject_rect(rects6 + 6 * i, m);
    });
}

ocrs_status ocrs_unproject_chars(ocrs_text_char* chars, size_t n, const float m[8]) {
    return guarded([&] {
        if (!m || (n > 0 && !chars)) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_map8(m);
        for (size_t i = 0; i < n; i++) {
            int32_t b[4] = {chars[i].top, chars[i].left, chars[i].bottom, chars[i].right};
            persp::unproject_box(b, m);
            chars[i].top = b[0];
            chars[i].left = b[1];
            chars[i].bottom = b[2];
            chars[i].right = b[3];
        }
    });
}

}  // extern "C"
