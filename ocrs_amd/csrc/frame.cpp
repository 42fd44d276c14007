// Page framing (include/ocrs_amd.h "Page framing"): the ink connected to the page frame taken out of
// resident pages on the device, a page's ink profiles, the choice of the content box and the gutter from them, rectangles
// cut out of resident pages, and the maps back.  The kernels are in kernels_frame.hip, the choice in frame_choose.hpp;
// tests/frame_ref.py is the definition.
#include <cmath>
#include <cstddef>
#include <cstring>

#include "abi_util.hpp"
#include "engine.hpp"
#include "frame_choose.hpp"
#include "kernels.hpp"
#include "page_ops.hpp"

using namespace ocrs;
using namespace ocrs::abi;

static_assert(sizeof(ocrs_frame_info) == sizeof(k::FrameInfo), "ocrs_frame_info is what the kernels write");
static_assert(offsetof(ocrs_frame_info, paper_fill) == offsetof(k::FrameInfo, paper_fill) &&
                  offsetof(ocrs_frame_info, ink) == offsetof(k::FrameInfo, ink) &&
                  offsetof(ocrs_frame_info, ring_ink) == offsetof(k::FrameInfo, ring_ink) &&
                  offsetof(ocrs_frame_info, removed_pixels) == offsetof(k::FrameInfo, removed_pixels) &&
                  offsetof(ocrs_frame_info, kept_pixels) == offsetof(k::FrameInfo, kept_pixels),
              "ocrs_frame_info is what the kernels write");
static_assert(sizeof(ocrs_frame_choice_params) == sizeof(frame::ChoiceParams) && sizeof(ocrs_frame_choice) == sizeof(frame::Choice) &&
                  offsetof(ocrs_frame_choice_params, gutter_max_ink) == offsetof(frame::ChoiceParams, gutter_max_ink) &&
                  offsetof(ocrs_frame_choice, gutter_x) == offsetof(frame::Choice, gutter_x),
              "frame_choose.hpp restates the public structs");

namespace {

void check_params(const ocrs_frame_params& p) {
    if (!std::isfinite(p.threshold)) fail(OCRS_ERR_INVALID_ARGUMENT, "clean_frame: the threshold is a finite number");
    if (p.depth < 0 || p.depth > MAX_PAGE_SIDE) fail(OCRS_ERR_INVALID_ARGUMENT, "clean_frame: a depth of %d: 0 .. %d", p.depth, MAX_PAGE_SIDE);
    if (p.sides < 1 || p.sides > 15) fail(OCRS_ERR_INVALID_ARGUMENT, "clean_frame: sides of %d: 1 .. 15", p.sides);
    if (p.min_area < 0) fail(OCRS_ERR_INVALID_ARGUMENT, "clean_frame: a min_area of %d: at least 0", p.min_area);
    if (std::isinf(p.paper)) fail(OCRS_ERR_INVALID_ARGUMENT, "clean_frame: paper is a finite number, or NaN to measure it");
}

void check_choice_params(const ocrs_frame_choice_params& p) {
    frame::ChoiceParams q;
    memcpy(&q, &p, sizeof q);
    if (!frame::choice_params_ok(q))
        fail(OCRS_ERR_INVALID_ARGUMENT, "frame_choose: min_count %d (>= 1), pad %d (0 .. 65535), gutter_min_width %d (>= 1), gutter_max_ink %d (>= 0)",
             p.min_count, p.pad, p.gutter_min_width, p.gutter_max_ink);
}

// every page's frame cleaned as a new page of its own, all passes for all pages on `ws`'s stream; waits for them
PageBatch<k::FrameDesc> clean_frame(Workspace& ws, const ocrs_page* const* pages, size_t n, const ocrs_frame_params* params,
                                    uint8_t** out_masks, ocrs_frame_info* out_infos) {
    PageBatch<k::FrameDesc> batch{"clean_frame"};
    if (n == 0) return batch;
    check_pages_in("clean_frame", pages, n, true);   // the labels are int32 pixel indices
    size_t mask_words = 0;
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        k::FrameDesc& d = batch.add_like(p, k::frame_tiles(p->h, p->w));
        d.ww = (p->w + 63) / 64;
        d.hw = (p->h + 63) / 64;
        d.depth = params[i].depth;
        d.sides = params[i].sides;
        d.min_area = params[i].min_area;
        d.threshold = params[i].threshold;
        d.paper = params[i].paper;
        mask_words += (size_t)p->h * d.ww;
    }
    // per page: its bit mask, its forest, areas and flags, its histogram, its blocks' counts and its info; the byte mask when
    // it is asked for
    unsigned long long* d_masks = ws.alloc_n<unsigned long long>(mask_words);
    unsigned long long* d_hist = ws.alloc_n<unsigned long long>(n * 256);
    batch.carve_outputs(ws, k::FRAME_COUNTS, out_masks != nullptr);
    mask_words = 0;
    for (size_t i = 0; i < n; i++) {
        k::FrameDesc& d = batch.descs[i];
        const size_t px = (size_t)d.h * d.w;
        d.rmask = d_masks + mask_words;
        mask_words += (size_t)d.h * d.ww;
        d.labels = ws.alloc_n<int32_t>(px);
        d.area = ws.alloc_n<uint32_t>(px);
        d.seed_flag = ws.alloc_n<uint8_t>(px);
        d.hist = d_hist + i * 256;
        d.vec = vec16_ok(d.w, d.src, d.dst) && vec16_ok(d.w, d.mask_out, d.mask_out) ? 1 : 0;
    }
    batch.run_outputs(ws, out_infos, out_masks, [&](const k::FrameDesc* d_descs, int n_pages, int blocks) {
        OCRS_HIP(hipMemsetAsync(d_hist, 0, n * 256 * sizeof(unsigned long long), ws.s()));
        k::clean_frame_pages(d_descs, n_pages, blocks, ws.s());
    });
    return batch;
}

// rectangle i of page i as a new page of its own, all in one launch on `ws`'s stream; waits for it
PageBatch<k::CropDesc> crop(Workspace& ws, const ocrs_page* const* pages, size_t n, const ocrs_crop_rect* rects, const float* fill) {
    PageBatch<k::CropDesc> batch{"crop"};
    for (size_t i = 0; i < n; i++) {
        const int64_t ow = (int64_t)rects[i].x1 - rects[i].x0, oh = (int64_t)rects[i].y1 - rects[i].y0;
        if (ow < 1 || ow > MAX_PAGE_SIDE || oh < 1 || oh > MAX_PAGE_SIDE)
            fail(OCRS_ERR_INVALID_ARGUMENT, "crop: a rectangle of %lld x %lld: a side is 1 .. %d", (long long)oh, (long long)ow, MAX_PAGE_SIDE);
    }
    check_pages_in("crop", pages, n, false);
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        const int ow = (int)((int64_t)rects[i].x1 - rects[i].x0), oh = (int)((int64_t)rects[i].y1 - rects[i].y0);
        k::CropDesc& d = batch.add(oh, ow, k::frame_tiles(oh, ow));
        d.src = p->grey.as<uint32_t>();
        d.dst = batch.made.back()->grey.as<uint32_t>();
        d.h = p->h;
        d.w = p->w;
        d.oh = oh;
        d.ow = ow;
        d.x0 = rects[i].x0;
        d.y0 = rects[i].y0;
        memcpy(&d.fill, &fill[i], sizeof d.fill);   // the word, whatever its bits
        d.vec = vec16_ok(ow, d.dst, d.dst) ? 1 : 0;
    }
    batch.run(ws, [&](const k::CropDesc* d_descs, int n_pages, int tiles) { k::crop_pages(d_descs, n_pages, tiles, ws.s()); });
    return batch;
}

}  // namespace

extern "C" {

ocrs_status ocrs_frame_params_default(ocrs_frame_params* out) {
    return guarded([&] {
        if (!out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        out->threshold = 0.0f;
        out->depth = 128;
        out->sides = 15;
        out->min_area = 0;
        out->paper = std::nanf("");
    });
}

ocrs_status ocrs_frame_params_check(const ocrs_frame_params* params) {
    return params_check(params, check_params);
}

ocrs_status ocrs_engine_clean_frame_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const ocrs_frame_params* params,
                                          ocrs_page** out_pages, uint8_t** out_masks, ocrs_frame_info* out_infos) {
    return pages_call(e, pages, n, params, check_params, out_pages,
                      [&](Workspace& ws) { return clean_frame(ws, pages, n, params, out_masks, out_infos); });
}

ocrs_status ocrs_engine_clean_frame_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_frame_params* params, ocrs_page** out_page,
                                         uint8_t** out_mask, ocrs_frame_info* out_info) {
    return page_call(params, ocrs_frame_params_default, [&](const ocrs_frame_params* q) {
        return ocrs_engine_clean_frame_pages(e, &page, 1, q, out_page, out_mask, out_info);
    });
}

ocrs_status ocrs_engine_ink_profiles(const ocrs_engine* e, const ocrs_page* page, float threshold, uint32_t* out_cols, uint32_t* out_rows) {
    return guarded_engine(e, [&] {
        if (!e || !page) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        if (!std::isfinite(threshold)) fail(OCRS_ERR_INVALID_ARGUMENT, "ink_profiles: the threshold is a finite number");
        check_pages_on(e, &page, 1);
        check_page_side("ink_profiles", page);
        if (!out_cols && !out_rows) return;
        Workspace ws;
        const size_t nc = out_cols ? (size_t)page->w : 0, nr = out_rows ? (size_t)page->h : 0;
        uint32_t* d_sums = ws.alloc_n<uint32_t>(nc + nr);   // the columns' sums, then the rows'
        OCRS_HIP(hipMemsetAsync(d_sums, 0, (nc + nr) * sizeof(uint32_t), ws.s()));
        k::ink_profiles(page->grey.as<float>(), page->h, page->w, threshold, out_cols ? d_sums : nullptr, out_rows ? d_sums + nc : nullptr, ws.s());
        OCRS_HIP(hipGetLastError());
        if (out_cols) ws.download(out_cols, d_sums, nc * sizeof(uint32_t));
        if (out_rows) ws.download(out_rows, d_sums + nc, nr * sizeof(uint32_t));
        ws.sync();
    });
}

ocrs_status ocrs_frame_choice_params_default(ocrs_frame_choice_params* out) {
    return guarded([&] {
        if (!out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        out->min_count = 1;
        out->pad = 16;
        out->gutter_min_width = 8;
        out->gutter_max_ink = 0;
    });
}

ocrs_status ocrs_frame_choice_params_check(const ocrs_frame_choice_params* params) {
    return params_check(params, check_choice_params);
}

ocrs_status ocrs_frame_choose(int h, int w, const uint32_t* col_ink, const uint32_t* row_ink, const ocrs_frame_choice_params* params,
                              ocrs_frame_choice* out) {
    return guarded([&] {
        if (!col_ink || !row_ink || !out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        if (h < 1 || h > MAX_PAGE_SIDE || w < 1 || w > MAX_PAGE_SIDE)
            fail(OCRS_ERR_INVALID_ARGUMENT, "frame_choose: a page of %d x %d: a side is 1 .. %d", h, w, MAX_PAGE_SIDE);
        ocrs_frame_choice_params p;
        if (params) p = *params;
        else ocrs_frame_choice_params_default(&p);
        check_choice_params(p);
        frame::ChoiceParams q;
        memcpy(&q, &p, sizeof q);
        const frame::Choice c = frame::choose(h, w, col_ink, row_ink, q);
        memcpy(out, &c, sizeof c);
    });
}

ocrs_status ocrs_engine_crop_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const ocrs_crop_rect* rects, const float* fill,
                                   ocrs_page** out_pages) {
    return guarded_engine(e, [&] {
        if (!e || (n > 0 && (!pages || !rects || !fill || !out_pages))) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_pages_on(e, pages, n);
        Workspace ws;
        crop(ws, pages, n, rects, fill).release_into(out_pages);
    });
}

ocrs_status ocrs_engine_crop_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_crop_rect* rect, float fill, ocrs_page** out_page) {
    return ocrs_engine_crop_pages(e, &page, 1, rect, &fill, out_page);
}

ocrs_status ocrs_uncrop_rects(float* rects6, size_t n, int x0, int y0) {
    return guarded([&] {
        if (n > 0 && !rects6) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        const float fx = (float)x0, fy = (float)y0;
        for (size_t i = 0; i < n; i++) {
            rects6[6 * i] = rects6[6 * i] + fx;
            rects6[6 * i + 1] = rects6[6 * i + 1] + fy;
        }
    });
}

ocrs_status ocrs_uncrop_chars(ocrs_text_char* chars, size_t n, int x0, int y0) {
    return guarded([&] {
        if (n > 0 && !chars) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        // two's-complement arithmetic (a box far outside the page wraps instead of overflowing)
        const uint32_t dx = (uint32_t)x0, dy = (uint32_t)y0;
        for (size_t i = 0; i < n; i++) {
            ocrs_text_char& c = chars[i];
            c.left = (int32_t)((uint32_t)c.left + dx);
            c.right = (int32_t)((uint32_t)c.right + dx);
            c.top = (int32_t)((uint32_t)c.top + dy);
            c.bottom = (int32_t)((uint32_t)c.bottom + dy);
        }
    });
}

}  // extern "C"
