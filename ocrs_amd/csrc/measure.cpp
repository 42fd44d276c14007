// Page measurement (include/ocrs_amd.h "Page measurement"): the stroke width and the text height of
// resident pages as exact integer histograms taken on the device, the host's choice of a scale from them and the work scale
// that follows.  The kernels are in kernels_measure.hip, the choice in measure_choose.hpp; tests/measure_ref.py is the
// definition.  The call makes no page: it has a descriptor of its own and shares find_desc with the page-making operations.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>
#include <vector>

#include "abi_util.hpp"
#include "engine.hpp"
#include "kernels.hpp"
#include "measure_choose.hpp"
#include "page_ops.hpp"

using namespace ocrs;
using namespace ocrs::abi;

static_assert(sizeof(ocrs_measure_info) == sizeof(k::MeasureInfo) && sizeof(ocrs_measure_info) == sizeof(measure::Info),
              "ocrs_measure_info is what the kernels write and what measure_choose.hpp reads");
static_assert(offsetof(ocrs_measure_info, components) == offsetof(k::MeasureInfo, components) &&
                  offsetof(ocrs_measure_info, counted) == offsetof(k::MeasureInfo, counted) &&
                  offsetof(ocrs_measure_info, run_h) == offsetof(k::MeasureInfo, run_h) &&
                  offsetof(ocrs_measure_info, run_v) == offsetof(k::MeasureInfo, run_v) &&
                  offsetof(ocrs_measure_info, comp_h) == offsetof(k::MeasureInfo, comp_h) &&
                  offsetof(ocrs_measure_info, comp_w) == offsetof(k::MeasureInfo, comp_w) &&
                  offsetof(ocrs_measure_info, area_by_h) == offsetof(k::MeasureInfo, area_by_h),
              "ocrs_measure_info is what the kernels write");
static_assert(offsetof(ocrs_measure_info, run_v) == offsetof(measure::Info, run_v) && offsetof(ocrs_measure_info, comp_w) == offsetof(measure::Info, comp_w) &&
                  offsetof(ocrs_measure_info, area_by_h) == offsetof(measure::Info, area_by_h) &&
                  sizeof(ocrs_measure_choice_params) == sizeof(measure::ChoiceParams) && sizeof(ocrs_text_scale) == sizeof(measure::TextScale) &&
                  offsetof(ocrs_text_scale, support) == offsetof(measure::TextScale, support) &&
                  offsetof(ocrs_text_scale, blank) == offsetof(measure::TextScale, blank),
              "measure_choose.hpp restates the public structs");
static_assert(k::MEASURE_BINS == OCRS_MEASURE_BINS && measure::BINS == OCRS_MEASURE_BINS, "one number of bins");

namespace {

void check_params(const ocrs_measure_params& p) {
    if (!std::isfinite(p.threshold)) fail(OCRS_ERR_INVALID_ARGUMENT, "measure: the threshold is a finite number");
    if (p.min_area < 0 || p.min_area > k::MEASURE_MAX_MIN_AREA)
        fail(OCRS_ERR_INVALID_ARGUMENT, "measure: a min_area of %d: 0 .. %d", p.min_area, k::MEASURE_MAX_MIN_AREA);
}

void check_choice_params(const ocrs_measure_choice_params& p) {
    if (!measure::choice_params_ok({p.min_height_strokes}))
        fail(OCRS_ERR_INVALID_ARGUMENT, "measure_choose: min_height_strokes of %g: 0 .. 255", p.min_height_strokes);
}

// every page's record, all passes for all pages on `ws`'s stream; waits for them.  Per pixel of a page the workspace holds
// its label, its area and three box words (20 bytes) and one bit of the mask.
void measure_pages(Workspace& ws, const ocrs_page* const* pages, size_t n, const ocrs_measure_params* params, ocrs_measure_info* out_infos) {
    if (n == 0) return;
    check_pages_in("measure", pages, n, true);   // the labels are int32 pixel indices
    std::vector<k::MeasureDesc> descs(n);
    int64_t blocks = 0;
    size_t mask_words = 0, pixels = 0;
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        k::MeasureDesc& d = descs[i];
        memset(&d, 0, sizeof d);
        d.src = p->grey.as<float>();
        d.h = p->h;
        d.w = p->w;
        d.ww = (p->w + 63) / 64;
        d.min_area = params[i].min_area;
        d.threshold = params[i].threshold;
        d.block0 = (int32_t)blocks;
        blocks += k::measure_tiles(p->h, p->w);
        if (blocks > std::numeric_limits<int32_t>::max()) fail(OCRS_ERR_CAPACITY, "measure: the pages of one call take more than 2^31 blocks");
        mask_words += k::measure_mask_words(p->h, p->w);
        pixels += (size_t)p->h * (size_t)p->w;
    }
    // before anything is allocated or launched: what does not fit in the device's memory is refused as such
    size_t free_bytes = 0, total_bytes = 0;
    OCRS_HIP(hipMemGetInfo(&free_bytes, &total_bytes));
    const size_t need = pixels * 20 + mask_words * 8 + n * (sizeof(k::MeasureInfo) + sizeof(k::MeasureDesc));
    if (need > total_bytes)
        fail(OCRS_ERR_CAPACITY, "measure: the pages of one call take a workspace of %zu bytes, the device has %zu", need, total_bytes);
    unsigned long long* d_mask = ws.alloc_n<unsigned long long>(mask_words);
    int32_t* d_labels = ws.alloc_n<int32_t>(pixels);
    uint32_t* d_words = ws.alloc_n<uint32_t>(4 * pixels);   // area, x0, x1, y1 of every page, page after page
    k::MeasureInfo* d_infos = ws.alloc_n<k::MeasureInfo>(n);
    size_t at_word = 0, at_px = 0;
    for (size_t i = 0; i < n; i++) {
        k::MeasureDesc& d = descs[i];
        const size_t px = (size_t)d.h * d.w;
        d.mask = d_mask + at_word;
        d.labels = d_labels + at_px;
        d.area = d_words + 4 * at_px;
        d.x0 = d.area + px;
        d.x1 = d.x0 + px;
        d.y1 = d.x1 + px;
        d.info = d_infos + i;
        at_word += k::measure_mask_words(d.h, d.w);
        at_px += px;
    }
    k::MeasureDesc* d_descs = ws.alloc_n<k::MeasureDesc>(n);
    ws.upload(d_descs, descs.data(), n * sizeof(k::MeasureDesc));
    OCRS_HIP(hipMemsetAsync(d_infos, 0, n * sizeof(k::MeasureInfo), ws.s()));
    k::measure_pages(d_descs, (int)n, (int)blocks, ws.s());
    OCRS_HIP(hipGetLastError());
    ws.download(out_infos, d_infos, n * sizeof(k::MeasureInfo));   // handed to the caller by the sync, not before
    ws.sync();
}

}  // namespace

extern "C" {

ocrs_status ocrs_measure_params_default(ocrs_measure_params* out) {
    return guarded([&] {
        if (!out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        out->threshold = 0.0f;
        out->min_area = 4;
    });
}

ocrs_status ocrs_measure_params_check(const ocrs_measure_params* params) {
    return params_check(params, check_params);
}

ocrs_status ocrs_engine_measure_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const ocrs_measure_params* params,
                                      ocrs_measure_info* out_infos) {
    return guarded_engine(e, [&] {
        if (!e || (n > 0 && (!pages || !params || !out_infos))) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        for (size_t i = 0; i < n; i++)
            if (!pages[i]) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_pages_on(e, pages, n);
        for (size_t i = 0; i < n; i++) check_params(params[i]);
        Workspace ws;
        measure_pages(ws, pages, n, params, out_infos);
    });
}

ocrs_status ocrs_engine_measure_page(const ocrs_engine* e, const ocrs_page* page, const ocrs_measure_params* params, ocrs_measure_info* out_info) {
    return page_call(params, ocrs_measure_params_default,
                     [&](const ocrs_measure_params* q) { return ocrs_engine_measure_pages(e, &page, 1, q, out_info); });
}

ocrs_status ocrs_measure_choice_params_default(ocrs_measure_choice_params* out) {
    return guarded([&] {
        if (!out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        out->min_height_strokes = 0.5;
    });
}

ocrs_status ocrs_measure_choice_params_check(const ocrs_measure_choice_params* params) {
    return params_check(params, check_choice_params);
}

ocrs_status ocrs_measure_choose(const ocrs_measure_info* info, const ocrs_measure_choice_params* params, ocrs_text_scale* out) {
    return guarded([&] {
        if (!info || !out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        ocrs_measure_choice_params p;
        if (params) p = *params;
        else ocrs_measure_choice_params_default(&p);
        check_choice_params(p);
        measure::Info in;
        memcpy(&in, info, sizeof in);
        const measure::TextScale t = measure::choose(in, {p.min_height_strokes});
        memcpy(out, &t, sizeof t);
    });
}

ocrs_status ocrs_work_scale_for_text(int text_height, double target_height, double min_scale, double max_scale, double* scale) {
    return guarded([&] {
        if (!scale) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        if (!measure::work_scale_args_ok(target_height, min_scale, max_scale))
            fail(OCRS_ERR_INVALID_ARGUMENT, "work scale: a target of %g within [%g, %g]: a positive target and 0 < min_scale <= max_scale", target_height,
                 min_scale, max_scale);
        *scale = measure::work_scale_for_text(text_height, target_height, min_scale, max_scale);
    });
}

}  // extern "C"
