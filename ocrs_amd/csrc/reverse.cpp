// Reverse-video repair (include/ocrs_amd.h "Reverse-video repair"): the solid dark panels of resident pages
// that enclose light marks, and what they enclose, inverted on the device by flipping the sign bit.  The kernels are in
// kernels_reverse.hip; tests/reverse_ref.py is the definition.
#include <cmath>
#include <cstddef>
#include <limits>

#include "abi_util.hpp"
#include "engine.hpp"
#include "kernels.hpp"
#include "page_ops.hpp"

using namespace ocrs;
using namespace ocrs::abi;

static_assert(sizeof(ocrs_reverse_info) == sizeof(k::ReverseInfo), "ocrs_reverse_info is what the kernels write");
static_assert(offsetof(ocrs_reverse_info, ink) == offsetof(k::ReverseInfo, ink) &&
                  offsetof(ocrs_reverse_info, components) == offsetof(k::ReverseInfo, components) &&
                  offsetof(ocrs_reverse_info, candidates) == offsetof(k::ReverseInfo, candidates) &&
                  offsetof(ocrs_reverse_info, panels) == offsetof(k::ReverseInfo, panels) &&
                  offsetof(ocrs_reverse_info, panel_pixels) == offsetof(k::ReverseInfo, panel_pixels) &&
                  offsetof(ocrs_reverse_info, holes) == offsetof(k::ReverseInfo, holes) &&
                  offsetof(ocrs_reverse_info, hole_pixels) == offsetof(k::ReverseInfo, hole_pixels) &&
                  offsetof(ocrs_reverse_info, skipped_holes) == offsetof(k::ReverseInfo, skipped_holes) &&
                  offsetof(ocrs_reverse_info, inverted) == offsetof(k::ReverseInfo, inverted),
              "ocrs_reverse_info is what the kernels write");

namespace {

void check_params(const ocrs_reverse_params& p) {
    if (!std::isfinite(p.threshold)) fail(OCRS_ERR_INVALID_ARGUMENT, "unreverse: the threshold is a finite number");
    if (p.min_height < 1 || p.min_height > k::REVERSE_MAX_SIDE)
        fail(OCRS_ERR_INVALID_ARGUMENT, "unreverse: a min_height of %d: 1 .. %d", p.min_height, k::REVERSE_MAX_SIDE);
    if (p.min_width < 1 || p.min_width > k::REVERSE_MAX_SIDE)
        fail(OCRS_ERR_INVALID_ARGUMENT, "unreverse: a min_width of %d: 1 .. %d", p.min_width, k::REVERSE_MAX_SIDE);
    if (!(p.min_fill >= 0.0f && p.min_fill <= 1.0f)) fail(OCRS_ERR_INVALID_ARGUMENT, "unreverse: a min_fill of %g: 0 .. 1", (double)p.min_fill);
    if (p.min_holes < 0) fail(OCRS_ERR_INVALID_ARGUMENT, "unreverse: a min_holes of %d: at least 0", p.min_holes);
    if (p.max_hole < 0) fail(OCRS_ERR_INVALID_ARGUMENT, "unreverse: a max_hole of %d: at least 0 (0: no limit)", p.max_hole);
}

// every page repaired as a new page of its own, all passes for all pages on `ws`'s stream; waits for them
PageBatch<k::ReverseDesc> unreverse(Workspace& ws, const ocrs_page* const* pages, size_t n, const ocrs_reverse_params* params,
                                    uint8_t** out_masks, ocrs_reverse_info* out_infos) {
    PageBatch<k::ReverseDesc> batch{"unreverse"};
    if (n == 0) return batch;
    check_pages_in("unreverse", pages, n, true);   // the labels are int32 pixel indices
    // before anything is allocated or launched: what does not fit in one launch or in the device's memory is refused as such
    int64_t tiles = 0;
    size_t mask_words = 0, pixels = 0;
    for (size_t i = 0; i < n; i++) {
        tiles += k::reverse_tiles(pages[i]->h, pages[i]->w);
        if (tiles > std::numeric_limits<int32_t>::max()) fail(OCRS_ERR_CAPACITY, "unreverse: the pages of one call take more than 2^31 blocks");
        mask_words += k::reverse_mask_words(pages[i]->h, pages[i]->w);
        pixels += (size_t)pages[i]->h * (size_t)pages[i]->w;
    }
    size_t free_bytes = 0, total_bytes = 0;
    OCRS_HIP(hipMemGetInfo(&free_bytes, &total_bytes));
    // per pixel: the new page, the forest, the area and three box words, the byte mask when asked for; per tile its counts
    const size_t need = pixels * (sizeof(float) + k::REVERSE_WORKSPACE_PER_PIXEL + (out_masks ? 1 : 0)) + mask_words * 8 +
                        (size_t)tiles * k::REVERSE_COUNTS * 8 + n * (sizeof(k::ReverseInfo) + sizeof(k::ReverseDesc));
    if (need > total_bytes)
        fail(OCRS_ERR_CAPACITY, "unreverse: the pages of one call take %zu bytes on the device, which has %zu", need, total_bytes);
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        k::ReverseDesc& d = batch.add_like(p, k::reverse_tiles(p->h, p->w));
        d.ww = (p->w + 63) / 64;
        d.hw = (p->h + 63) / 64;
        d.min_height = params[i].min_height;
        d.min_width = params[i].min_width;
        d.fill_q8 = k::reverse_fill_q8(params[i].min_fill);
        d.min_holes = params[i].min_holes;
        d.max_hole = params[i].max_hole;
        d.threshold = params[i].threshold;
    }
    unsigned long long* d_masks = ws.alloc_n<unsigned long long>(mask_words);
    batch.carve_outputs(ws, k::REVERSE_COUNTS, out_masks != nullptr);
    mask_words = 0;
    for (size_t i = 0; i < n; i++) {
        k::ReverseDesc& d = batch.descs[i];
        const size_t px = (size_t)d.h * d.w;
        d.masks = d_masks + mask_words;
        mask_words += k::reverse_mask_words(d.h, d.w);
        d.labels = ws.alloc_n<int32_t>(px);
        d.area = ws.alloc_n<uint32_t>(px);
        d.x0 = ws.alloc_n<uint32_t>(px);
        d.x1 = ws.alloc_n<uint32_t>(px);
        d.y1 = ws.alloc_n<uint32_t>(px);
        d.vec = vec16_ok(d.w, d.src, d.dst) && vec16_ok(d.w, d.dst, d.mask_out) ? 1 : 0;
    }
    batch.run_outputs(ws, out_infos, out_masks, [&](const k::ReverseDesc* d_descs, int n_pages, int blocks) {
        k::unreverse_pages(d_descs, n_pages, blocks, ws.s());
    });
    return batch;
}

}  // namespace

extern "C" {

ocrs_status ocrs_reverse_params_default(ocrs_reverse_params* out) {
    return guarded([&] {
        if (!out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        out->threshold = 0.0f;   // the five below are uncalibrated: DESIGN.md §7.15
        out->min_height = 32;
        out->min_width = 64;
        out->min_fill = 0.4f;
        out->min_holes = 3;
        out->max_hole = 0;
    });
}

ocrs_status ocrs_reverse_params_check(const ocrs_reverse_params* params) {
    return params_check(params, check_params);
}

ocrs_status ocrs_engine_unreverse_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const ocrs_reverse_params* params,
                                        ocrs_page** out_pages, uint8_t** out_masks, ocrs_reverse_info* out_infos) {
    return pages_call(e, pages, n, params, check_params, out_pages,
                      [&](Workspace& ws) { return unreverse(ws, pages, n, params, out_masks, out_infos); });
}

ocrs_status ocrs_engine_unreverse_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_reverse_params* params, ocrs_page** out_page,
                                       uint8_t** out_mask, ocrs_reverse_info* out_info) {
    return page_call(params, ocrs_reverse_params_default, [&](const ocrs_reverse_params* q) {
        return ocrs_engine_unreverse_pages(e, &page, 1, q, out_page, out_mask, out_info);
    });
}

}  // extern "C"
