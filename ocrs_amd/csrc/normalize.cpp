// Page normalisation (include/ocrs_amd.h "Page normalisation"): background flattening, levels and
// polarity of resident pages on the device.  The kernels are in kernels_normalize.hip; tests/normalize_ref.py is the
// definition.
#include <cstddef>

#include "abi_util.hpp"
#include "engine.hpp"
#include "kernels.hpp"
#include "page_ops.hpp"

using namespace ocrs;
using namespace ocrs::abi;

static_assert(sizeof(ocrs_normalize_info) == sizeof(k::NormInfo), "ocrs_normalize_info is what the kernels write");
static_assert(offsetof(ocrs_normalize_info, vote) == offsetof(k::NormInfo, vote) && offsetof(ocrs_normalize_info, counted) == offsetof(k::NormInfo, counted),
              "ocrs_normalize_info is what the kernels write");

namespace {

int tile_shift(const ocrs_normalize_params& p) {
    for (int s = 4; s <= 8; s++)
        if (p.tile == (1 << s)) return s;
    fail(OCRS_ERR_INVALID_ARGUMENT, "normalize: a tile of %d: a power of two, 16 .. 256", p.tile);
}

void check_params(const ocrs_normalize_params& p) {
    (void)tile_shift(p);
    if (p.polarity != OCRS_POLARITY_AUTO && p.polarity != OCRS_POLARITY_KEEP && p.polarity != OCRS_POLARITY_INVERT)
        fail(OCRS_ERR_INVALID_ARGUMENT, "normalize: unknown polarity %d", p.polarity);
}

// every page normalised into a new page of its own, all passes for all pages on `ws`'s stream; waits for them
PageBatch<k::NormDesc> normalize_pages(Workspace& ws, const ocrs_page* const* pages, size_t n, const ocrs_normalize_params* params,
                                       ocrs_normalize_info* out_info) {
    PageBatch<k::NormDesc> batch{"normalize"};
    if (n == 0) return batch;
    check_pages_in("normalize", pages, n, false);
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        const int tshift = tile_shift(params[i]);
        const int th = (p->h + (1 << tshift) - 1) >> tshift, tw = (p->w + (1 << tshift) - 1) >> tshift;
        k::NormDesc& d = batch.add_like(p, (int64_t)th * tw);
        d.tshift = tshift;
        d.th = th;
        d.tw = tw;
        d.polarity = params[i].polarity;
        d.flatten = params[i].flatten ? 1 : 0;
        d.levels = params[i].levels ? 1 : 0;
        d.vec = vec16_ok(p->w, d.src, d.dst) ? 1 : 0;
    }
    // per page: its state; per tile (= block): its record and its level bin
    k::NormState* d_states = ws.alloc_n<k::NormState>(n);
    uint32_t* d_tiles = ws.alloc_n<uint32_t>((size_t)batch.blocks);
    uint8_t* d_grid = ws.alloc_n<uint8_t>((size_t)batch.blocks);
    k::NormInfo* d_info = ws.alloc_n<k::NormInfo>(n);
    for (size_t i = 0; i < n; i++) {
        k::NormDesc& d = batch.descs[i];
        d.state = d_states + i;
        d.tiles = d_tiles + d.block0;
        d.grid = d_grid + d.block0;
    }
    batch.run(ws, [&](const k::NormDesc* d_descs, int n_pages, int blocks) {
        OCRS_HIP(hipMemsetAsync(d_states, 0, n * sizeof(k::NormState), ws.s()));
        k::normalize_pages(d_descs, n_pages, blocks, d_info, ws.s());
        OCRS_HIP(hipGetLastError());   // of the launches, before the download is queued
        if (out_info) ws.download(out_info, d_info, n * sizeof(k::NormInfo));
    });
    return batch;
}

}  // namespace

extern "C" {

ocrs_status ocrs_normalize_params_default(ocrs_normalize_params* out) {
    return guarded([&] {
        if (!out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        out->tile = 64;
        out->polarity = OCRS_POLARITY_AUTO;
        out->flatten = 1;
        out->levels = 1;
    });
}

ocrs_status ocrs_normalize_params_check(const ocrs_normalize_params* params) {
    return params_check(params, check_params);
}

ocrs_status ocrs_engine_normalize_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const ocrs_normalize_params* params,
                                        ocrs_page** out_pages, ocrs_normalize_info* out_info) {
    return pages_call(e, pages, n, params, check_params, out_pages,
                      [&](Workspace& ws) { return normalize_pages(ws, pages, n, params, out_info); });
}

ocrs_status ocrs_engine_normalize_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_normalize_params* params, ocrs_page** out_page,
                                       ocrs_normalize_info* out_info) {
    return page_call(params, ocrs_normalize_params_default, [&](const ocrs_normalize_params* q) {
        return ocrs_engine_normalize_pages(e, &page, 1, q, out_page, out_info);
    });
}

}  // extern "C"
