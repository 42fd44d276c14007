// Page operations: what the calls that make new resident pages out of resident pages share: quarter
// turns (orient.cpp), resampling (resample.cpp), normalisation (normalize.cpp), the deskew warp (deskew.cpp), rule removal
// (rules.cpp), despeckling (speckle.cpp), adaptive binarisation (binarize.cpp), stroke repair
// (morph.cpp).  Not part of the public header.
#pragma once
#include <limits>
#include <memory>
#include <vector>

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

// rows of width w in both buffers start 16-byte aligned: a kernel may use 16-byte accesses (a descriptor's `vec`)
inline bool vec16_ok(int w, const void* src, const void* dst) { return w % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0; }

// One launch for a batch of pages: a descriptor per page, whose block0 is the sum of the blocks of the pages before it;
// a block finds its page with find_desc (find_desc.hpp).  The batch owns the pages it makes until release_into.
template <class Desc>
struct PageBatch {
    const char* what;   // the operation, in messages
    std::vector<std::unique_ptr<ocrs_page>> made;
    std::vector<Desc> descs;
    int64_t blocks = 0;

    // a new out_h x out_w page (made.back()) that takes `n` blocks -> its descriptor: zeroed, block0 set
    Desc& add(int out_h, int out_w, int64_t n) {
        made.push_back(new_page(out_h, out_w));
        descs.emplace_back();
        descs.back().block0 = (int32_t)blocks;
        blocks += n;
        if (blocks > std::numeric_limits<int32_t>::max()) fail(OCRS_ERR_CAPACITY, "%s: the pages of one call take more than 2^31 blocks", what);
        return descs.back();
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
    void release_into(ocrs_page** out) {
        for (size_t i = 0; i < made.size(); i++) out[i] = made[i].release();
    }
};

}  // namespace abi
}  // namespace ocrs
