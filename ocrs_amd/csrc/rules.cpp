// Ruled-line removal (include/ocrs_amd.h "Ruled-line removal"): the rules of forms, tables and underlines
// taken out of resident pages on the device.  The kernels are in kernels_rules.hip; tests/rules_ref.py is the definition.
#include <cmath>
#include <cstddef>

#include "abi_util.hpp"
#include "engine.hpp"
#include "kernels.hpp"
#include "page_ops.hpp"

using namespace ocrs;
using namespace ocrs::abi;

static_assert(sizeof(ocrs_rules_info) == sizeof(k::RulesInfo), "ocrs_rules_info is what the kernels write");
static_assert(offsetof(ocrs_rules_info, fill) == offsetof(k::RulesInfo, fill) && offsetof(ocrs_rules_info, ink) == offsetof(k::RulesInfo, ink) &&
                  offsetof(ocrs_rules_info, kept) == offsetof(k::RulesInfo, kept),
              "ocrs_rules_info is what the kernels write");

namespace {

void check_params(const ocrs_rules_params& p) {
    if (!std::isfinite(p.threshold)) fail(OCRS_ERR_INVALID_ARGUMENT, "rules: the threshold is a finite number");
    if (p.min_length < 2 || p.min_length > 65535) fail(OCRS_ERR_INVALID_ARGUMENT, "rules: a min_length of %d: 2 .. 65535", p.min_length);
    if (p.max_thickness < 1 || p.max_thickness > 64) fail(OCRS_ERR_INVALID_ARGUMENT, "rules: a max_thickness of %d: 1 .. 64", p.max_thickness);
    if (p.margin < 0 || p.margin > 8) fail(OCRS_ERR_INVALID_ARGUMENT, "rules: a margin of %d: 0 .. 8", p.margin);
    if (std::isinf(p.paper)) fail(OCRS_ERR_INVALID_ARGUMENT, "rules: paper is a finite number, or NaN to measure it");
}

// every page with its rules removed as a new page of its own, all passes for all pages on `ws`'s stream; waits for them
PageBatch<k::RulesDesc> remove_rules(Workspace& ws, const ocrs_page* const* pages, size_t n, const ocrs_rules_params* params,
                                     uint8_t** out_masks, ocrs_rules_info* out_infos) {
    PageBatch<k::RulesDesc> batch{"rules"};
    if (n == 0) return batch;
    check_pages_in("rules", pages, n, false);
    size_t mask_words = 0;
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        k::RulesDesc& d = batch.add_like(p, k::rules_tiles(p->h, p->w));
        d.ww = (p->w + 63) / 64;
        d.hw = (p->h + 63) / 64;
        d.min_length = params[i].min_length;
        d.max_thickness = params[i].max_thickness;
        d.margin = params[i].margin;
        d.threshold = params[i].threshold;
        d.paper = params[i].paper;
        d.vec = vec16_ok(p->w, d.src, d.dst) ? 1 : 0;
        mask_words += k::rules_mask_words(p->h, p->w);
    }
    // per page: its bit masks, its histogram, its blocks' counts and its info; the byte mask when it is asked for
    unsigned long long* d_masks = ws.alloc_n<unsigned long long>(mask_words);
    unsigned long long* d_hist = ws.alloc_n<unsigned long long>(n * 256);
    batch.carve_outputs(ws, k::RULES_COUNTS, out_masks != nullptr);
    mask_words = 0;
    for (size_t i = 0; i < n; i++) {
        k::RulesDesc& d = batch.descs[i];
        d.masks = d_masks + mask_words;
        mask_words += k::rules_mask_words(d.h, d.w);
        d.hist = d_hist + i * 256;
    }
    batch.run_outputs(ws, out_infos, out_masks, [&](const k::RulesDesc* d_descs, int n_pages, int blocks) {
        OCRS_HIP(hipMemsetAsync(d_hist, 0, n * 256 * sizeof(unsigned long long), ws.s()));
        k::remove_rules_pages(d_descs, n_pages, blocks, ws.s());
    });
    return batch;
}

}  // namespace

extern "C" {

ocrs_status ocrs_rules_params_default(ocrs_rules_params* out) {
    return guarded([&] {
        if (!out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        out->threshold = 0.0f;
        out->min_length = 96;
        out->max_thickness = 8;
        out->margin = 1;
        out->paper = std::nanf("");
    });
}

ocrs_status ocrs_rules_params_check(const ocrs_rules_params* params) {
    return params_check(params, check_params);
}

ocrs_status ocrs_engine_remove_rules_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const ocrs_rules_params* params,
                                           ocrs_page** out_pages, uint8_t** out_masks, ocrs_rules_info* out_infos) {
    return pages_call(e, pages, n, params, check_params, out_pages,
                      [&](Workspace& ws) { return remove_rules(ws, pages, n, params, out_masks, out_infos); });
}

ocrs_status ocrs_engine_remove_rules_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_rules_params* params, ocrs_page** out_page,
                                          uint8_t** out_mask, ocrs_rules_info* out_info) {
    return page_call(params, ocrs_rules_params_default, [&](const ocrs_rules_params* q) {
        return ocrs_engine_remove_rules_pages(e, &page, 1, q, out_page, out_mask, out_info);
    });
}

}  // extern "C"
