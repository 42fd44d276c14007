// Stroke repair (include/ocrs_amd.h "Stroke repair"): resident pages whose ink is thickened, thinned,
// closed or opened on the device by running minima and maxima over a rectangle, every result pixel the 32-bit word of a
// source pixel.  The kernels are in kernels_morph.hip; tests/morph_ref.py is the definition.
#include <cstddef>

#include "abi_util.hpp"
#include "engine.hpp"
#include "kernels.hpp"
#include "page_ops.hpp"

using namespace ocrs;
using namespace ocrs::abi;

static_assert(sizeof(ocrs_morph_info) == sizeof(k::MorphInfo), "ocrs_morph_info is what the kernels write");
static_assert(offsetof(ocrs_morph_info, counted) == offsetof(k::MorphInfo, counted) &&
                  offsetof(ocrs_morph_info, changed) == offsetof(k::MorphInfo, changed) &&
                  offsetof(ocrs_morph_info, ink_before) == offsetof(k::MorphInfo, ink_before) &&
                  offsetof(ocrs_morph_info, ink_after) == offsetof(k::MorphInfo, ink_after),
              "ocrs_morph_info is what the kernels write");
static_assert(OCRS_MORPH_THICKEN == 0 && OCRS_MORPH_THIN == 1 && OCRS_MORPH_CLOSE == 2 && OCRS_MORPH_OPEN == 3 && k::MORPH_OPS == 4,
              "the ops index the stage table");

namespace {

void check_params(const ocrs_morph_params& p) {
    if (p.op < 0 || p.op >= k::MORPH_OPS) fail(OCRS_ERR_INVALID_ARGUMENT, "morph: an op of %d: 0 .. %d", p.op, k::MORPH_OPS - 1);
    if (p.rx < 0 || p.rx > k::MORPH_MAX_RADIUS) fail(OCRS_ERR_INVALID_ARGUMENT, "morph: an rx of %d: 0 .. %d", p.rx, k::MORPH_MAX_RADIUS);
    if (p.ry < 0 || p.ry > k::MORPH_MAX_RADIUS) fail(OCRS_ERR_INVALID_ARGUMENT, "morph: an ry of %d: 0 .. %d", p.ry, k::MORPH_MAX_RADIUS);
    if (p.rx == 0 && p.ry == 0) fail(OCRS_ERR_INVALID_ARGUMENT, "morph: rx and ry are both 0: the window is the pixel");
}

// every page repaired as a new page of its own, all passes for all pages on `ws`'s stream; waits for them
PageBatch<k::MorphDesc> morph(Workspace& ws, const ocrs_page* const* pages, size_t n, const ocrs_morph_params* params, uint8_t** out_masks,
                              ocrs_morph_info* out_infos) {
    PageBatch<k::MorphDesc> batch{"morph"};
    if (n == 0) return batch;
    check_pages_in("morph", pages, n, true);
    // the stages of an op: lo takes the least key, hi the greatest, which is the least of the flipped keys
    constexpr uint32_t LO = 0u, HI = 0xffffffffu;
    static const uint32_t flips[k::MORPH_OPS][2] = {{LO, LO}, {HI, HI}, {LO, HI}, {HI, LO}};
    int64_t row_blocks[2] = {0, 0}, col_blocks2 = 0;
    int max_ry = 0;
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        const ocrs_morph_params& q = params[i];
        const int64_t cols = k::morph_col_blocks(p->h, p->w, q.ry), rows = k::morph_row_blocks(p->h, p->w);
        k::MorphDesc& d = batch.add_like(p, cols);
        d.stages = q.op == OCRS_MORPH_CLOSE || q.op == OCRS_MORPH_OPEN ? 2 : 1;
        d.row_block0 = (int32_t)row_blocks[0];
        d.row_block0_2 = (int32_t)row_blocks[1];
        d.block0_2 = (int32_t)col_blocks2;
        row_blocks[0] += rows;
        if (d.stages == 2) {
            row_blocks[1] += rows;
            col_blocks2 += cols;
        }
        if (row_blocks[0] > std::numeric_limits<int32_t>::max()) fail(OCRS_ERR_CAPACITY, "morph: the pages of one call take more than 2^31 blocks");
        d.seg_rows = k::morph_seg_rows(p->h, p->w, q.ry);
        d.strips = (p->w + k::MORPH_STRIP - 1) / k::MORPH_STRIP;
        d.segs = (p->h + d.seg_rows - 1) / d.seg_rows;
        d.row_segs = (p->w + k::MORPH_SEG - 1) / k::MORPH_SEG;
        d.rx = q.rx;
        d.ry = q.ry;
        if (q.ry > max_ry) max_ry = q.ry;
        d.flip[0] = flips[q.op][0];
        d.flip[1] = flips[q.op][1];
    }
    // per page: the row extrema of the stage at hand, the page between two stages, its blocks' counts and its info; the
    // byte mask when it is asked for
    batch.carve_outputs(ws, k::MORPH_COUNTS, out_masks != nullptr);
    for (k::MorphDesc& d : batch.descs) {
        const size_t px = (size_t)d.h * d.w;
        d.keys = ws.alloc_n<uint32_t>(px);
        d.mid = d.stages == 2 ? ws.alloc_n<float>(px) : nullptr;
    }
    batch.run_outputs(ws, out_infos, out_masks, [&](const k::MorphDesc* d_descs, int n_pages, int blocks) {
        const int rows[2] = {(int)row_blocks[0], (int)row_blocks[1]}, cols[2] = {blocks, (int)col_blocks2};
        k::morph_pages(d_descs, n_pages, rows, cols, max_ry, ws.s());
    });
    return batch;
}

}  // namespace

extern "C" {

ocrs_status ocrs_morph_params_default(ocrs_morph_params* out) {
    return guarded([&] {
        if (!out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        out->op = OCRS_MORPH_CLOSE;
        out->rx = 1;
        out->ry = 1;
    });
}

ocrs_status ocrs_morph_params_check(const ocrs_morph_params* params) {
    return params_check(params, check_params);
}

ocrs_status ocrs_engine_morph_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const ocrs_morph_params* params,
                                    ocrs_page** out_pages, uint8_t** out_masks, ocrs_morph_info* out_infos) {
    return pages_call(e, pages, n, params, check_params, out_pages,
                      [&](Workspace& ws) { return morph(ws, pages, n, params, out_masks, out_infos); });
}

ocrs_status ocrs_engine_morph_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_morph_params* params, ocrs_page** out_page,
                                   uint8_t** out_mask, ocrs_morph_info* out_info) {
    return page_call(params, ocrs_morph_params_default, [&](const ocrs_morph_params* q) {
        return ocrs_engine_morph_pages(e, &page, 1, q, out_page, out_mask, out_info);
    });
}

}  // extern "C"
