// Page normalisation (include/ocrs_amd.h "Page normalisation"): background flattening, levels and
// polarity of resident pages on the device.  The kernels are in kernels_normalize.hip; tests/normalize_ref.py is the
// definition.
#include <cstddef>
#include <limits>

#include "abi_util.hpp"
#include "engine.hpp"
#include "kernels.hpp"

using namespace ocrs;
using namespace ocrs::abi;

static_assert(sizeof(ocrs_normalize_info) == sizeof(k::NormInfo), "ocrs_normalize_info is what the kernels write");
static_assert(offsetof(ocrs_normalize_info, vote) == offsetof(k::NormInfo, vote) && offsetof(ocrs_normalize_info, counted) == offsetof(k::NormInfo, counted),
              "ocrs_normalize_info is what the kernels write");

namespace {

constexpr int MAX_SIDE = 65535;

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
std::vector<std::unique_ptr<ocrs_page>> normalize_pages(Workspace& ws, const ocrs_page* const* pages, size_t n,
                                                        const ocrs_normalize_params* params, ocrs_normalize_info* out_info) {
    std::vector<std::unique_ptr<ocrs_page>> made;
    if (n == 0) return made;
    std::vector<k::NormDesc> descs(n);
    int64_t blocks = 0;
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        if (p->h > MAX_SIDE || p->w > MAX_SIDE) fail(OCRS_ERR_INVALID_ARGUMENT, "normalize: a page of %d x %d: a side is at most %d", p->h, p->w, MAX_SIDE);
        k::NormDesc& d = descs[i];
        d.tshift = tile_shift(params[i]);
        d.h = p->h;
        d.w = p->w;
        d.th = (p->h + (1 << d.tshift) - 1) >> d.tshift;
        d.tw = (p->w + (1 << d.tshift) - 1) >> d.tshift;
        d.block0 = (int32_t)blocks;
        blocks += (int64_t)d.th * d.tw;
        if (blocks > std::numeric_limits<int32_t>::max()) fail(OCRS_ERR_CAPACITY, "normalize: the pages of one call take more than 2^31 tiles");
        d.polarity = params[i].polarity;
        d.flatten = params[i].flatten ? 1 : 0;
        d.levels = params[i].levels ? 1 : 0;
    }
    k::NormState* d_states = ws.alloc_n<k::NormState>(n);
    uint32_t* d_tiles = ws.alloc_n<uint32_t>((size_t)blocks);
    uint8_t* d_grid = ws.alloc_n<uint8_t>((size_t)blocks);
    k::NormInfo* d_info = ws.alloc_n<k::NormInfo>(n);
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        auto out = std::make_unique<ocrs_page>();
        out->h = p->h;
        out->w = p->w;
        out->grey = DevBuf((size_t)p->h * p->w * sizeof(float));
        k::NormDesc& d = descs[i];
        d.src = p->grey.as<float>();
        d.dst = out->grey.as<float>();
        d.state = d_states + i;
        d.tiles = d_tiles + d.block0;
        d.grid = d_grid + d.block0;
        d.vec = (p->w % 4 == 0 && (((uintptr_t)d.src | (uintptr_t)d.dst) & 15) == 0) ? 1 : 0;
        made.push_back(std::move(out));
    }
    k::NormDesc* d_descs = ws.alloc_n<k::NormDesc>(n);
    ws.upload(d_descs, descs.data(), n * sizeof(k::NormDesc));
    OCRS_HIP(hipMemsetAsync(d_states, 0, n * sizeof(k::NormState), ws.s()));
    k::normalize_pages(d_descs, (int)n, (int)blocks, d_info, ws.s());
    OCRS_HIP(hipGetLastError());
    if (out_info) ws.download(out_info, d_info, n * sizeof(k::NormInfo));
    ws.sync();
    return made;
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
    return guarded([&] {
        if (!params) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_params(*params);
    });
}

ocrs_status ocrs_engine_normalize_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const ocrs_normalize_params* params,
                                        ocrs_page** out_pages, ocrs_normalize_info* out_info) {
    return guarded_engine(e, [&] {
        if (!e || (n > 0 && (!pages || !params || !out_pages))) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_pages_on(e, pages, n);
        for (size_t i = 0; i < n; i++) check_params(params[i]);
        Workspace ws;
        auto made = normalize_pages(ws, pages, n, params, out_info);
        for (size_t i = 0; i < n; i++) out_pages[i] = made[i].release();
    });
}

ocrs_status ocrs_engine_normalize_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_normalize_params* params, ocrs_page** out_page,
                                       ocrs_normalize_info* out_info) {
    ocrs_normalize_params def;
    if (!params) {
        ocrs_normalize_params_default(&def);
        params = &def;
    }
    return ocrs_engine_normalize_pages(e, &page, 1, params, out_page, out_info);
}

}  // extern "C"
