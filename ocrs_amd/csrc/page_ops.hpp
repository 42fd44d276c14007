// Page operations: what the calls that make new resident pages out of resident pages share: quarter
// turns (orient.cpp), resampling (resample.cpp), normalisation (normalize.cpp), the deskew warp (deskew.cpp), rule removal
// (rules.cpp), despeckling (speckle.cpp), adaptive binarisation (binarize.cpp), stroke repair
// (morph.cpp), page framing (frame.cpp), grain removal (rank.cpp), reverse-video repair (reverse.cpp).  Not part of the
// public header.
#pragma once
#include <cstdlib>
#include <limits>
#include <memory>
#include <type_traits>
#include <vector>

#include "abi_util.hpp"
#include "engine.hpp"

namespace ocrs {
namespace abi {

constexpr int MAX_PAGE_SIDE = 65535;   // of a page a batched operation reads or makes: its kernels index a side in 16 bits

inline std::unique_ptr<ocrs_page> new_page(int h, int w) {   // grey allocated on the bound device, not written
    auto page = std::make_unique<ocrs_page>();
    page->h = h;
    page->w = w;
    page->grey = DevBuf((size_t)h * w * sizeof(float));
    return page;
}

inline void check_page_side(const char* what, const ocrs_page* p) {
    if (p->h > MAX_PAGE_SIDE || p->w > MAX_PAGE_SIDE)
        fail(OCRS_ERR_INVALID_ARGUMENT, "%s: a page of %d x %d: a side is at most %d", what, p->h, p->w, MAX_PAGE_SIDE);
}

// the input pages of a batched operation, all of them before anything is allocated; int32_pixels: the operation indexes the
// pixels of a page in 32 bits
inline void check_pages_in(const char* what, const ocrs_page* const* pages, size_t n, bool int32_pixels) {
    for (size_t i = 0; i < n; i++) {
        check_page_side(what, pages[i]);
        if (int32_pixels && (int64_t)pages[i]->h * pages[i]->w > (int64_t)std::numeric_limits<int32_t>::max())
            fail(OCRS_ERR_INVALID_ARGUMENT, "%s: a page of %d x %d: at most 2^31 - 1 pixels", what, pages[i]->h, pages[i]->w);
    }
}

struct FreeHost {   // of what malloc gave: the buffers a caller releases with ocrs_free
    void operator()(void* p) const { free(p); }
};

// rows of width w in both buffers start 16-byte aligned: a kernel may use 16-byte accesses (a descriptor's `vec`)
inline bool vec16_ok(int w, const void* src, const void* dst) { return w % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0; }

// One launch for a batch of pages: a descriptor per page, whose block0 is the sum of the blocks of the pages before it;
// a block finds its page with find_desc (find_desc.hpp).  The batch owns the pages it makes until release_into.
//
// A masked operation (rules.cpp, speckle.cpp, binarize.cpp, morph.cpp, frame.cpp's cleanup, rank.cpp, reverse.cpp) makes a page of its input's size and, per page, an
// info record and, if asked for, a byte mask; its descriptor has src, dst, h, w, counts, info and mask_out.  It calls
// add_like for every page, then carve_outputs, fills in what is its own, and run_outputs.
template <class Desc>
struct PageBatch {
    const char* what;   // the operation, in messages
    std::vector<std::unique_ptr<ocrs_page>> made;
    std::vector<Desc> descs;
    int64_t blocks = 0;
    std::vector<std::unique_ptr<uint8_t, FreeHost>> host_masks;   // of a masked operation, until run_outputs hands them over

    // a new out_h x out_w page (made.back()) that takes `n` blocks -> its descriptor: zeroed, block0 set
    Desc& add(int out_h, int out_w, int64_t n) {
        made.push_back(new_page(out_h, out_w));
        descs.emplace_back();
        descs.back().block0 = (int32_t)blocks;
        blocks += n;
        if (blocks > std::numeric_limits<int32_t>::max()) fail(OCRS_ERR_CAPACITY, "%s: the pages of one call take more than 2^31 blocks", what);
        return descs.back();
    }
    // a new page of p's size that takes `n` blocks -> its descriptor with src, dst, h and w set
    Desc& add_like(const ocrs_page* p, int64_t n) {
        Desc& d = add(p->h, p->w, n);
        d.src = p->grey.as<float>();
        d.dst = made.back()->grey.as<float>();
        d.h = p->h;
        d.w = p->w;
        return d;
    }
    // after the last add_like: every page's info, its blocks' counts (`per_block` words a block, one allocation) and, with
    // `masks`, its mask_out with a host buffer to receive it
    void carve_outputs(Workspace& ws, size_t per_block, bool masks) {
        auto* d_counts = ws.alloc_n<unsigned long long>((size_t)blocks * per_block);
        auto* d_info = ws.alloc_n<std::remove_pointer_t<decltype(Desc::info)>>(descs.size());
        for (size_t i = 0; i < descs.size(); i++) {
            Desc& d = descs[i];
            d.counts = d_counts + (size_t)d.block0 * per_block;
            d.info = d_info + i;
            if (!masks) continue;
            const size_t px = (size_t)d.h * d.w;
            d.mask_out = ws.alloc_n<uint8_t>(px);
            host_masks.emplace_back(static_cast<uint8_t*>(malloc(px)));
            if (!host_masks.back()) throw std::bad_alloc();
        }
    }
    // descriptors to the device, launch(d_descs, n_pages, total_blocks) on ws's stream, and the wait; nothing for no pages
    template <class Launch>
    void run(Workspace& ws, Launch&& launch) {
        if (descs.empty()) return;
        Desc* d_descs = ws.alloc_n<Desc>(descs.size());
        ws.upload(d_descs, descs.data(), descs.size() * sizeof(Desc));
        launch(d_descs, (int)descs.size(), (int)blocks);
        OCRS_HIP(hipGetLastError());
        ws.sync();
    }
    // run, with the infos (if out_infos) and the masks (if carved) downloaded behind the launches; the masks are the
    // caller's only once all of it has succeeded.  Nothing for no pages.
    template <class Info, class Launch>
    void run_outputs(Workspace& ws, Info* out_infos, uint8_t** out_masks, Launch&& launch) {
        static_assert(sizeof(Info) == sizeof(*Desc::info), "the public info record is what the kernels write");
        run(ws, [&](const Desc* d_descs, int n_pages, int n_blocks) {
            launch(d_descs, n_pages, n_blocks);
            OCRS_HIP(hipGetLastError());   // of the launches, before the downloads are queued
            if (out_infos) ws.download(out_infos, descs[0].info, descs.size() * sizeof(Info));
            for (size_t i = 0; i < host_masks.size(); i++)
                ws.download(host_masks[i].get(), descs[i].mask_out, (size_t)descs[i].h * descs[i].w);
        });
        for (size_t i = 0; i < host_masks.size(); i++) out_masks[i] = host_masks[i].release();
    }
    void release_into(ocrs_page** out) {
        for (size_t i = 0; i < made.size(); i++) out[i] = made[i].release();
    }
};

// ---- the extern "C" tail of an operation with per-page parameters: ocrs_X_params_check, ocrs_engine_X_pages, ocrs_engine_X_page

template <class Params>
ocrs_status params_check(const Params* params, void (*check)(const Params&)) {
    return guarded([&] {
        if (!params) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check(*params);
    });
}

// make(ws) -> the PageBatch of the new pages, run
template <class Params, class Make>
ocrs_status pages_call(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const Params* params, void (*check)(const Params&),
                       ocrs_page** out_pages, Make&& make) {
    return guarded_engine(e, [&] {
        if (!e || (n > 0 && (!pages || !params || !out_pages))) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_pages_on(e, pages, n);
        for (size_t i = 0; i < n; i++) check(params[i]);
        Workspace ws;
        make(ws).release_into(out_pages);
    });
}

// one page: NULL params are the defaults; pages_of(params) is the _pages call on it
template <class Params, class PagesOf>
ocrs_status page_call(const Params* params, ocrs_status (*defaults)(Params*), PagesOf&& pages_of) {
    Params def;
    if (!params) {
        defaults(&def);
        params = &def;
    }
    return pages_of(params);
}

}  // namespace abi
}  // namespace ocrs
