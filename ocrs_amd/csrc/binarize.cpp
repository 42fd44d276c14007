// Adaptive binarisation (include/ocrs_amd.h "Adaptive binarisation"): resident pages cut into ink and paper
// on the device by Sauvola's local threshold, in exact integers.  The kernels are in kernels_binarize.hip;
// tests/binarize_ref.py is the definition.
#include <cmath>
#include <cstddef>
#include <cstring>

#include "abi_util.hpp"
#include "engine.hpp"
#include "kernels.hpp"
#include "page_ops.hpp"

using namespace ocrs;
using namespace ocrs::abi;

static_assert(sizeof(ocrs_binarize_info) == sizeof(k::BinInfo), "ocrs_binarize_info is what the kernels write");
static_assert(offsetof(ocrs_binarize_info, counted) == offsetof(k::BinInfo, counted) &&
                  offsetof(ocrs_binarize_info, ink) == offsetof(k::BinInfo, ink) &&
                  offsetof(ocrs_binarize_info, ink_fill) == offsetof(k::BinInfo, ink_fill) &&
                  offsetof(ocrs_binarize_info, paper_fill) == offsetof(k::BinInfo, paper_fill),
              "ocrs_binarize_info is what the kernels write");

namespace {

void check_params(const ocrs_binarize_params& p) {
    if (p.radius < 1 || p.radius > k::BIN_MAX_RADIUS)
        fail(OCRS_ERR_INVALID_ARGUMENT, "binarize: a radius of %d: 1 .. %d", p.radius, k::BIN_MAX_RADIUS);
    if (p.k_q8 < 0 || p.k_q8 > k::BIN_MAX_KQ) fail(OCRS_ERR_INVALID_ARGUMENT, "binarize: a k_q8 of %d: 0 .. %d", p.k_q8, k::BIN_MAX_KQ);
    if (p.keep_ink != 0 && p.keep_ink != 1) fail(OCRS_ERR_INVALID_ARGUMENT, "binarize: a keep_ink of %d: 0 or 1", p.keep_ink);
    if (std::isinf(p.ink_level)) fail(OCRS_ERR_INVALID_ARGUMENT, "binarize: ink_level is a finite number, or NaN for -0.5");
    if (std::isinf(p.paper)) fail(OCRS_ERR_INVALID_ARGUMENT, "binarize: paper is a finite number, or NaN for +0.5");
}

uint32_t fill_bits(float given, float otherwise) {
    const float f = given != given ? otherwise : given;
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}

// every page binarised as a new page of its own, all passes for all pages on `ws`'s stream; waits for them
PageBatch<k::BinDesc> binarize(Workspace& ws, const ocrs_page* const* pages, size_t n, const ocrs_binarize_params* params,
                               uint8_t** out_masks, ocrs_binarize_info* out_infos) {
    PageBatch<k::BinDesc> batch{"binarize"};
    if (n == 0) return batch;
    check_pages_in("binarize", pages, n, true);
    int64_t row_blocks = 0;
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        const ocrs_binarize_params& q = params[i];
        k::BinDesc& d = batch.add_like(p, k::bin_col_blocks(p->h, p->w, q.radius));
        d.row_block0 = (int32_t)row_blocks;
        row_blocks += k::bin_row_blocks(p->h);
        if (row_blocks > std::numeric_limits<int32_t>::max()) fail(OCRS_ERR_CAPACITY, "binarize: the pages of one call take more than 2^31 blocks");
        d.seg_rows = k::bin_seg_rows(p->h, p->w, q.radius);
        d.strips = (p->w + k::BIN_STRIP - 1) / k::BIN_STRIP;
        d.segs = (p->h + d.seg_rows - 1) / d.seg_rows;
        d.radius = q.radius;
        d.kq = q.k_q8;
        d.keep_ink = q.keep_ink;
        d.ink_bits = fill_bits(q.ink_level, -0.5f);
        d.paper_bits = fill_bits(q.paper, 0.5f);
    }
    // per page: the row sums of its pixels, its blocks' counts and its info; the byte mask when it is asked for
    batch.carve_outputs(ws, k::BIN_COUNTS, out_masks != nullptr);
    for (k::BinDesc& d : batch.descs) d.sums = ws.alloc_n<uint32_t>(2 * (size_t)d.h * d.w);
    batch.run_outputs(ws, out_infos, out_masks, [&](const k::BinDesc* d_descs, int n_pages, int blocks) {
        k::binarize_pages(d_descs, n_pages, (int)row_blocks, blocks, ws.s());
    });
    return batch;
}

}  // namespace

extern "C" {

ocrs_status ocrs_binarize_params_default(ocrs_binarize_params* out) {
    return guarded([&] {
        if (!out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        out->radius = 15;
        out->k_q8 = 87;
        out->keep_ink = 0;
        out->ink_level = std::nanf("");
        out->paper = std::nanf("");
    });
}

ocrs_status ocrs_binarize_params_check(const ocrs_binarize_params* params) {
    return params_check(params, check_params);
}

ocrs_status ocrs_engine_binarize_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const ocrs_binarize_params* params,
                                       ocrs_page** out_pages, uint8_t** out_masks, ocrs_binarize_info* out_infos) {
    return pages_call(e, pages, n, params, check_params, out_pages,
                      [&](Workspace& ws) { return binarize(ws, pages, n, params, out_masks, out_infos); });
}

ocrs_status ocrs_engine_binarize_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_binarize_params* params, ocrs_page** out_page,
                                      uint8_t** out_mask, ocrs_binarize_info* out_info) {
    return page_call(params, ocrs_binarize_params_default, [&](const ocrs_binarize_params* q) {
        return ocrs_engine_binarize_pages(e, &page, 1, q, out_page, out_mask, out_info);
    });
}

}  // extern "C"
