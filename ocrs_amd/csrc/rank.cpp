// Grain removal (include/ocrs_amd.h "Grain removal"): resident pages filtered on the device by a rank
// filter over a rectangle (a median, a percentile, either on outliers only), every result pixel the 32-bit word of a source
// pixel.  The kernels are in kernels_rank.hip; tests/rank_ref.py is the definition.
#include <cstddef>

#include "abi_util.hpp"
#include "engine.hpp"
#include "kernels.hpp"
#include "page_ops.hpp"

using namespace ocrs;
using namespace ocrs::abi;

static_assert(sizeof(ocrs_rank_info) == sizeof(k::RankInfo), "ocrs_rank_info is what the kernels write");
static_assert(offsetof(ocrs_rank_info, counted) == offsetof(k::RankInfo, counted) &&
                  offsetof(ocrs_rank_info, changed) == offsetof(k::RankInfo, changed) &&
                  offsetof(ocrs_rank_info, ink_before) == offsetof(k::RankInfo, ink_before) &&
                  offsetof(ocrs_rank_info, ink_after) == offsetof(k::RankInfo, ink_after) &&
                  offsetof(ocrs_rank_info, spared) == offsetof(k::RankInfo, spared),
              "ocrs_rank_info is what the kernels write");

namespace {

void check_params(const ocrs_rank_params& p) {
    if (p.rx < 0 || p.rx > k::RANK_MAX_RADIUS) fail(OCRS_ERR_INVALID_ARGUMENT, "rank: an rx of %d: 0 .. %d", p.rx, k::RANK_MAX_RADIUS);
    if (p.ry < 0 || p.ry > k::RANK_MAX_RADIUS) fail(OCRS_ERR_INVALID_ARGUMENT, "rank: an ry of %d: 0 .. %d", p.ry, k::RANK_MAX_RADIUS);
    if (p.rx == 0 && p.ry == 0) fail(OCRS_ERR_INVALID_ARGUMENT, "rank: rx and ry are both 0: the window is the pixel");
    if (p.percent < 0 || p.percent > 100) fail(OCRS_ERR_INVALID_ARGUMENT, "rank: a percent of %d: 0 .. 100", p.percent);
    if (p.tail < 0 || p.tail > 50) fail(OCRS_ERR_INVALID_ARGUMENT, "rank: a tail of %d: 0 .. 50", p.tail);
}

// every page filtered as a new page of its own, all launches for all pages on `ws`'s stream; waits for them
PageBatch<k::RankDesc> rank(Workspace& ws, const ocrs_page* const* pages, size_t n, const ocrs_rank_params* params, uint8_t** out_masks,
                            ocrs_rank_info* out_infos) {
    PageBatch<k::RankDesc> batch{"rank"};
    if (n == 0) return batch;
    check_pages_in("rank", pages, n, true);
    int64_t reg_blocks = 0, lds_blocks = 0;   // each at most the batch's blocks, which add() holds under 2^31
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        const ocrs_rank_params& q = params[i];
        k::RankDesc& d = batch.add_like(p, k::rank_blocks(p->h, p->w));
        d.tiles_x = (p->w + k::RANK_TILE_W - 1) / k::RANK_TILE_W;
        d.tiles_y = (p->h + k::RANK_TILE_H - 1) / k::RANK_TILE_H;
        d.rx = q.rx;
        d.ry = q.ry;
        d.percent = q.percent;
        d.tail = q.tail;
        d.cls = k::rank_class(q.rx, q.ry);
        d.reg_block0 = (int32_t)reg_blocks;
        d.lds_block0 = (int32_t)lds_blocks;
        (d.cls == 2 ? lds_blocks : reg_blocks) += k::rank_blocks(p->h, p->w);
    }
    batch.carve_outputs(ws, k::RANK_COUNTS, out_masks != nullptr);
    batch.run_outputs(ws, out_infos, out_masks, [&](const k::RankDesc* d_descs, int n_pages, int) {
        k::rank_pages(d_descs, n_pages, (int)reg_blocks, (int)lds_blocks, ws.s());
    });
    return batch;
}

}  // namespace

extern "C" {

ocrs_status ocrs_rank_params_default(ocrs_rank_params* out) {
    return guarded([&] {
        if (!out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        out->rx = 1;
        out->ry = 1;
        out->percent = 50;
        out->tail = 20;
    });
}

ocrs_status ocrs_rank_params_check(const ocrs_rank_params* params) {
    return params_check(params, check_params);
}

ocrs_status ocrs_engine_rank_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const ocrs_rank_params* params,
                                   ocrs_page** out_pages, uint8_t** out_masks, ocrs_rank_info* out_infos) {
    return pages_call(e, pages, n, params, check_params, out_pages,
                      [&](Workspace& ws) { return rank(ws, pages, n, params, out_masks, out_infos); });
}

ocrs_status ocrs_engine_rank_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_rank_params* params, ocrs_page** out_page,
                                  uint8_t** out_mask, ocrs_rank_info* out_info) {
    return page_call(params, ocrs_rank_params_default, [&](const ocrs_rank_params* q) {
        return ocrs_engine_rank_pages(e, &page, 1, q, out_page, out_mask, out_info);
    });
}

}  // extern "C"
