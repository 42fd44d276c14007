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

struct FreeHost {
    void operator()(uint8_t* p) const { free(p); }
};

// every page with its rules removed as a new page of its own, all passes for all pages on `ws`'s stream; waits for them
PageBatch<k::RulesDesc> remove_rules(Workspace& ws, const ocrs_page* const* pages, size_t n, const ocrs_rules_params* params,
                                     uint8_t** out_masks, ocrs_rules_info* out_infos) {
    PageBatch<k::RulesDesc> batch{"rules"};
    if (n == 0) return batch;
    for (size_t i = 0; i < n; i++) check_page_side("rules", pages[i]);
    size_t mask_words = 0;
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        k::RulesDesc& d = batch.add(p->h, p->w, k::rules_tiles(p->h, p->w));
        d.src = p->grey.as<float>();
        d.dst = batch.made.back()->grey.as<float>();
        d.h = p->h;
        d.w = p->w;
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
    unsigned long long* d_counts = ws.alloc_n<unsigned long long>((size_t)batch.blocks * k::RULES_COUNTS);
    k::RulesInfo* d_info = ws.alloc_n<k::RulesInfo>(n);
    std::vector<std::unique_ptr<uint8_t, FreeHost>> host_masks;
    mask_words = 0;
    for (size_t i = 0; i < n; i++) {
        k::RulesDesc& d = batch.descs[i];
        d.masks = d_masks + mask_words;
        mask_words += k::rules_mask_words(d.h, d.w);
        d.hist = d_hist + i * 256;
        d.counts = d_counts + (size_t)d.block0 * k::RULES_COUNTS;
        d.info = d_info + i;
        if (out_masks) {
            d.mask_out = ws.alloc_n<uint8_t>((size_t)d.h * d.w);
            host_masks.emplace_back(static_cast<uint8_t*>(malloc((size_t)d.h * d.w)));
            if (!host_masks.back()) throw std::bad_alloc();
        }
    }
    batch.run(ws, [&](const k::RulesDesc* d_descs, int n_pages, int blocks) {
        OCRS_HIP(hipMemsetAsync(d_hist, 0, n * 256 * sizeof(unsigned long long), ws.s()));
        k::remove_rules_pages(d_descs, n_pages, blocks, ws.s());
        OCRS_HIP(hipGetLastError());   // of the launches, before the downloads are queued
        if (out_infos) ws.download(out_infos, d_info, n * sizeof(k::RulesInfo));
        for (size_t i = 0; i < host_masks.size(); i++)
            ws.download(host_masks[i].get(), batch.descs[i].mask_out, (size_t)batch.descs[i].h * batch.descs[i].w);
    });
    for (size_t i = 0; i < host_masks.size(); i++) out_masks[i] = host_masks[i].release();
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
    return guarded([&] {
        if (!params) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_params(*params);
    });
}

ocrs_status ocrs_engine_remove_rules_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const ocrs_rules_params* params,
                                           ocrs_page** out_pages, uint8_t** out_masks, ocrs_rules_info* out_infos) {
    return guarded_engine(e, [&] {
        if (!e || (n > 0 && (!pages || !params || !out_pages))) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_pages_on(e, pages, n);
        for (size_t i = 0; i < n; i++) check_params(params[i]);
        Workspace ws;
        remove_rules(ws, pages, n, params, out_masks, out_infos).release_into(out_pages);
    });
}

ocrs_status ocrs_engine_remove_rules_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_rules_params* params, ocrs_page** out_page,
                                          uint8_t** out_mask, ocrs_rules_info* out_info) {
    ocrs_rules_params def;
    if (!params) {
        ocrs_rules_params_default(&def);
        params = &def;
    }
    return ocrs_engine_remove_rules_pages(e, &page, 1, params, out_page, out_mask, out_info);
}

}  // extern "C"
