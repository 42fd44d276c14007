// Working-resolution detection (include/ocrs_amd.h "Working resolution"): resampling resident pages on
// the device, the host maps between a page and its work page, and detection at a work size the caller chooses.
#include <cmath>
#include <numeric>

#include "abi_util.hpp"
#include "engine.hpp"
#include "kernels.hpp"
#include "page_ops.hpp"

using namespace ocrs;
using namespace ocrs::geom;
using namespace ocrs::abi;

namespace {

struct ResizeJob {
    const ocrs_page* page;
    int h, w;     // of the result
    bool area;
};

void check_filter(const char* what, int filter) {
    if (filter != OCRS_RESAMPLE_AUTO && filter != OCRS_RESAMPLE_BILINEAR && filter != OCRS_RESAMPLE_AREA)
        fail(OCRS_ERR_INVALID_ARGUMENT, "%s: unknown filter %d", what, filter);
}

// AUTO resolved, sizes and the filter's own limits checked
ResizeJob resize_job(const ocrs_page* p, int out_h, int out_w, int filter) {
    if (out_h < 1 || out_h > MAX_PAGE_SIDE || out_w < 1 || out_w > MAX_PAGE_SIDE)
        fail(OCRS_ERR_INVALID_ARGUMENT, "resize: %d x %d: a side is 1 .. %d", out_h, out_w, MAX_PAGE_SIDE);
    check_page_side("resize", p);
    const bool shrinks = out_h <= p->h && out_w <= p->w;
    check_filter("resize", filter);
    if (filter == OCRS_RESAMPLE_AREA && !shrinks)
        fail(OCRS_ERR_INVALID_ARGUMENT, "resize: the area filter only shrinks (%d x %d -> %d x %d)", p->h, p->w, out_h, out_w);
    return {p, out_h, out_w, filter == OCRS_RESAMPLE_AREA || (filter == OCRS_RESAMPLE_AUTO && shrinks)};
}

// every job's page resampled into a new page of its own, all in one launch on `ws`'s stream; waits for it
PageBatch<k::ResampleDesc> resize_pages(Workspace& ws, const std::vector<ResizeJob>& jobs) {
    PageBatch<k::ResampleDesc> batch{"resize"};
    for (const ResizeJob& j : jobs) {
        k::ResampleDesc& d = batch.add(j.h, j.w, k::resample_blocks(j.h, j.w));
        d.src = j.page->grey.as<float>();
        d.dst = batch.made.back()->grey.as<float>();
        d.sh = j.page->h;
        d.sw = j.page->w;
        d.dh = j.h;
        d.dw = j.w;
        d.area = j.area ? 1 : 0;
        const int gy = std::gcd(d.sh, d.dh), gx = std::gcd(d.sw, d.dw);
        d.py = (uint32_t)(d.sh / gy);
        d.qy = (uint32_t)(d.dh / gy);
        d.px = (uint32_t)(d.sw / gx);
        d.qx = (uint32_t)(d.dw / gx);
    }
    batch.run(ws, [&](const k::ResampleDesc* d_descs, int n_pages, int blocks) { k::resample_pages(d_descs, n_pages, blocks, ws.s()); });
    return batch;
}

int work_side(int side, double scale) {
    const double v = std::floor((double)side * scale + 0.5);
    return v < 1.0 ? 1 : v > (double)MAX_PAGE_SIDE ? MAX_PAGE_SIDE : (int)v;
}

// rects of a from_h x from_w frame -> the to_h x to_w frame of the same picture; points of the pixel-index frame
void rescale_rects(float* rects6, size_t n, int from_h, int from_w, int to_h, int to_w) {
    if (from_h == to_h && from_w == to_w) return;
    const double sx = (double)to_w / (double)from_w, sy = (double)to_h / (double)from_h;
    for (size_t i = 0; i < n; i++) {
        float* a = rects6 + 6 * i;
        const double cx = a[0], cy = a[1], upx = a[2], upy = a[3], w = a[4], h = a[5];
        a[0] = (float)((cx + 0.5) * sx - 0.5);
        a[1] = (float)((cy + 0.5) * sy - 0.5);
        const double vx = upx * sx, vy = upy * sy, lv = std::sqrt(vx * vx + vy * vy);
        const double ax = -upy * sx, ay = upx * sy, la = std::sqrt(ax * ax + ay * ay);
        if (std::isfinite(lv) && lv > 0.0) {
            a[2] = (float)(vx / lv);
            a[3] = (float)(vy / lv);
            a[4] = (float)(w * la);
            a[5] = (float)(h * lv);
        } else {
            a[4] = (float)(w * sx);
            a[5] = (float)(h * sy);
        }
    }
}

void check_frame(int h, int w, const char* what) {
    if (h < 1 || w < 1) fail(OCRS_ERR_INVALID_ARGUMENT, "%s: a frame of %d x %d", what, h, w);
}

}  // namespace

extern "C" {

ocrs_status ocrs_engine_resize_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const int* out_hw, const int* filters,
                                     ocrs_page** out) {
    return guarded_engine(e, [&] {
        if (!e || (n > 0 && (!pages || !out_hw || !filters || !out))) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_pages_on(e, pages, n);
        std::vector<ResizeJob> jobs;
        for (size_t i = 0; i < n; i++) jobs.push_back(resize_job(pages[i], out_hw[2 * i], out_hw[2 * i + 1], filters[i]));
        Workspace ws;
        resize_pages(ws, jobs).release_into(out);
    });
}

ocrs_status ocrs_engine_resize_page(const ocrs_engine* e, const ocrs_page* page, int out_h, int out_w, int filter, ocrs_page** out) {
    const int hw[2] = {out_h, out_w};
    return ocrs_engine_resize_pages(e, &page, 1, hw, &filter, out);
}

ocrs_status ocrs_work_size(int page_h, int page_w, double scale, int* h, int* w) {
    return guarded([&] {
        if (!h || !w) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_frame(page_h, page_w, "work size");
        if (!std::isfinite(scale) || !(scale > 0.0)) fail(OCRS_ERR_INVALID_ARGUMENT, "work size: the scale is finite and positive");
        *h = work_side(page_h, scale);
        *w = work_side(page_w, scale);
    });
}

ocrs_status ocrs_rescale_rects(float* rects6, size_t n, int from_h, int from_w, int to_h, int to_w) {
    return guarded([&] {
        if (n > 0 && !rects6) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_frame(from_h, from_w, "rescale");
        check_frame(to_h, to_w, "rescale");
        rescale_rects(rects6, n, from_h, from_w, to_h, to_w);
    });
}

ocrs_status ocrs_engine_detect_words_batch_at(const ocrs_engine* e, const ocrs_page* const* pages, size_t n_pages, const int* work_hw,
                                              int filter, int tiled, int overlap, float** rects, size_t* offsets, float** score,
                                              uint32_t** pixels) {
    return guarded_engine(e, [&] {
        if (!e || !rects || !offsets || (n_pages > 0 && (!pages || !work_hw))) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        if (!score != !pixels) fail(OCRS_ERR_INVALID_ARGUMENT, "score and pixels come together");
        check_filter("detect at", filter);
        check_pages_on(e, pages, n_pages);
        // 1. the pages whose work size is not their own, resampled in one launch
        std::vector<ResizeJob> jobs;
        std::vector<size_t> job_of(n_pages, (size_t)-1);
        for (size_t i = 0; i < n_pages; i++) {
            int wh = work_hw[2 * i], ww = work_hw[2 * i + 1];
            if (wh == 0 && ww == 0) { wh = pages[i]->h; ww = pages[i]->w; }
            if (wh == pages[i]->h && ww == pages[i]->w) continue;
            job_of[i] = jobs.size();
            jobs.push_back(resize_job(pages[i], wh, ww, filter));
        }
        std::vector<std::unique_ptr<ocrs_page>> made;
        if (!jobs.empty()) {
            Workspace ws;
            made = std::move(resize_pages(ws, jobs).made);
        }
        std::vector<const ocrs_page*> work(n_pages);
        for (size_t i = 0; i < n_pages; i++) work[i] = job_of[i] == (size_t)-1 ? pages[i] : made[job_of[i]].get();
        // 2. detection, as any request
        const bool scored = score != nullptr;
        std::vector<std::vector<RotatedRect>> rr;
        DetScores sc;
        e->detect(work.data(), n_pages, &rr, nullptr, scored ? &sc : nullptr, tiled ? tile_overlap_arg(overlap) : -1);
        // 3. the rects back in each page's own frame
        pack_words(rr, scored ? &sc : nullptr, rects, offsets, score, pixels, [&](size_t i, float* rects6, size_t n) {
            rescale_rects(rects6, n, work[i]->h, work[i]->w, pages[i]->h, pages[i]->w);
        });
    });
}

ocrs_status ocrs_engine_detect_words_at(const ocrs_engine* e, const ocrs_page* page, int work_h, int work_w, int filter, int tiled,
                                        int overlap, float** rects, size_t* n, float** score, uint32_t** pixels) {
    size_t offs[2] = {0, 0};
    const int hw[2] = {work_h, work_w};
    ocrs_status s = ocrs_engine_detect_words_batch_at(e, &page, page ? 1 : 0, hw, filter, tiled, overlap, rects, offs, score, pixels);
    if (s == OCRS_OK && n) *n = offs[1];
    return s;
}

}  // extern "C"
