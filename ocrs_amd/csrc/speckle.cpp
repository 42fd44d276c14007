// Despeckling (include/ocrs_amd.h "Despeckling"): the isolated specks and pinholes of resident pages taken
// out on the device by the size of their connected components.  The kernels are in kernels_speckle.hip;
// tests/despeckle_ref.py is the definition.
#include <cmath>
#include <cstddef>

#include "abi_util.hpp"
#include "engine.hpp"
#include "kernels.hpp"
#include "page_ops.hpp"

using namespace ocrs;
using namespace ocrs::abi;

static_assert(sizeof(ocrs_speckle_info) == sizeof(k::SpeckleInfo), "ocrs_speckle_info is what the kernels write");
static_assert(offsetof(ocrs_speckle_info, paper_fill) == offsetof(k::SpeckleInfo, paper_fill) &&
                  offsetof(ocrs_speckle_info, ink) == offsetof(k::SpeckleInfo, ink) &&
                  offsetof(ocrs_speckle_info, kept_pixels) == offsetof(k::SpeckleInfo, kept_pixels) &&
                  offsetof(ocrs_speckle_info, hole_pixels) == offsetof(k::SpeckleInfo, hole_pixels),
              "ocrs_speckle_info is what the kernels write");

namespace {

void check_params(const ocrs_speckle_params& p) {
    if (!std::isfinite(p.threshold)) fail(OCRS_ERR_INVALID_ARGUMENT, "despeckle: the threshold is a finite number");
    if (p.max_area < 0 || p.max_area > k::SPECKLE_MAX_AREA)
        fail(OCRS_ERR_INVALID_ARGUMENT, "despeckle: a max_area of %d: 0 .. %d", p.max_area, k::SPECKLE_MAX_AREA);
    if (p.max_hole < 0 || p.max_hole > k::SPECKLE_MAX_AREA)
        fail(OCRS_ERR_INVALID_ARGUMENT, "despeckle: a max_hole of %d: 0 .. %d", p.max_hole, k::SPECKLE_MAX_AREA);
    if (p.keep_near < 0 || p.keep_near > k::SPECKLE_MAX_NEAR)
        fail(OCRS_ERR_INVALID_ARGUMENT, "despeckle: a keep_near of %d: 0 .. %d", p.keep_near, k::SPECKLE_MAX_NEAR);
    if (std::isinf(p.paper)) fail(OCRS_ERR_INVALID_ARGUMENT, "despeckle: paper is a finite number, or NaN to measure it");
    if (std::isinf(p.ink_level)) fail(OCRS_ERR_INVALID_ARGUMENT, "despeckle: ink_level is a finite number, or NaN to measure it");
}

// every page despeckled as a new page of its own, all passes for all pages on `ws`'s stream; waits for them
PageBatch<k::SpeckleDesc> despeckle(Workspace& ws, const ocrs_page* const* pages, size_t n, const ocrs_speckle_params* params,
                                    uint8_t** out_masks, ocrs_speckle_info* out_infos) {
    PageBatch<k::SpeckleDesc> batch{"despeckle"};
    if (n == 0) return batch;
    check_pages_in("despeckle", pages, n, true);   // the labels are int32 pixel indices
    size_t mask_words = 0;
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        k::SpeckleDesc& d = batch.add_like(p, k::speckle_tiles(p->h, p->w));
        d.ww = (p->w + 63) / 64;
        d.hw = (p->h + 63) / 64;
        d.max_area = params[i].max_area;
        d.max_hole = params[i].max_hole;
        d.keep_near = params[i].keep_near;
        d.threshold = params[i].threshold;
        d.paper = params[i].paper;
        d.ink_level = params[i].ink_level;
        mask_words += k::speckle_mask_words(p->h, p->w);
    }
    // per page: its bit masks, its forest, areas and flags, its two histograms, its blocks' counts and its info; the byte
    // mask when it is asked for
    unsigned long long* d_masks = ws.alloc_n<unsigned long long>(mask_words);
    unsigned long long* d_hist = ws.alloc_n<unsigned long long>(n * 512);
    batch.carve_outputs(ws, k::SPECKLE_COUNTS, out_masks != nullptr);
    mask_words = 0;
    for (size_t i = 0; i < n; i++) {
        k::SpeckleDesc& d = batch.descs[i];
        const size_t px = (size_t)d.h * d.w;
        d.masks = d_masks + mask_words;
        mask_words += k::speckle_mask_words(d.h, d.w);
        d.labels = ws.alloc_n<int32_t>(px);
        d.area = ws.alloc_n<uint32_t>(px);
        d.near_flag = ws.alloc_n<uint8_t>(px);
        d.hist = d_hist + i * 512;
        d.vec = vec16_ok(d.w, d.src, d.dst) && vec16_ok(d.w, d.labels, d.mask_out) ? 1 : 0;
    }
    batch.run_outputs(ws, out_infos, out_masks, [&](const k::SpeckleDesc* d_descs, int n_pages, int blocks) {
        OCRS_HIP(hipMemsetAsync(d_hist, 0, n * 512 * sizeof(unsigned long long), ws.s()));
        k::despeckle_pages(d_descs, n_pages, blocks, ws.s());
    });
    return batch;
}

}  // namespace

extern "C" {

ocrs_status ocrs_speckle_params_default(ocrs_speckle_params* out) {
    return guarded([&] {
        if (!out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        out->threshold = 0.0f;
        out->max_area = 4;
        out->max_hole = 0;
        out->keep_near = 0;
        out->paper = std::nanf("");
        out->ink_level = std::nanf("");
    });
}

ocrs_status ocrs_speckle_params_check(const ocrs_speckle_params* params) {
    return params_check(params, check_params);
}

ocrs_status ocrs_engine_despeckle_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const ocrs_speckle_params* params,
                                        ocrs_page** out_pages, uint8_t** out_masks, ocrs_speckle_info* out_infos) {
    return pages_call(e, pages, n, params, check_params, out_pages,
                      [&](Workspace& ws) { return despeckle(ws, pages, n, params, out_masks, out_infos); });
}

ocrs_status ocrs_engine_despeckle_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_speckle_params* params, ocrs_page** out_page,
                                       uint8_t** out_mask, ocrs_speckle_info* out_info) {
    return page_call(params, ocrs_speckle_params_default, [&](const ocrs_speckle_params* q) {
        return ocrs_engine_despeckle_pages(e, &page, 1, q, out_page, out_mask, out_info);
    });
}

}  // extern "C"
