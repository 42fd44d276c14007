// Page deskew (include/ocrs_amd.h "Page deskew"): the skew estimate of resident pages, the affine page
// warp that straightens them, and the host maps that bring results of the warped page back to the scan's frame.  The
// kernels are in kernels_deskew.hip; tests/deskew_ref.py is the definition.
#include <algorithm>
#include <cmath>
#include <limits>

#include "abi_util.hpp"
#include "engine.hpp"
#include "kernels.hpp"
#include "page_ops.hpp"

using namespace ocrs;
using namespace ocrs::abi;

namespace {

constexpr int SKEW_MAX_SIDE = 4096;      // x S + y C - t0 stays inside int32
constexpr int SKEW_Q16 = 65536;
constexpr size_t SKEW_MAX_ANGLES = 65535;
constexpr double PI = 3.14159265358979323846;

void check_table(const int32_t* sc_table, size_t n_angles) {
    if (n_angles < 1 || n_angles > SKEW_MAX_ANGLES) fail(OCRS_ERR_INVALID_ARGUMENT, "skew scores: %zu angles: 1 .. %zu", n_angles, SKEW_MAX_ANGLES);
    for (size_t i = 0; i < 2 * n_angles; i++)
        if (sc_table[i] > SKEW_Q16 || sc_table[i] < -SKEW_Q16)
            fail(OCRS_ERR_INVALID_ARGUMENT, "skew scores: table entry %zu is %d: Q16 sines and cosines lie within +-%d", i, sc_table[i], SKEW_Q16);
}

// scores[n, A] of the pages, every page and angle in two launches on `ws`'s stream; waits for them
void skew_scores(Workspace& ws, const ocrs_page* const* pages, size_t n, const int32_t* sc_table, size_t n_angles, uint64_t* out_scores) {
    if (n == 0) return;
    if (n > 65535) fail(OCRS_ERR_CAPACITY, "skew scores: %zu pages in one call: at most 65535", n);
    std::vector<k::SkewDesc> descs(n);
    int64_t blocks = 0;
    size_t dwords = 0;
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        if (p->h > SKEW_MAX_SIDE || p->w > SKEW_MAX_SIDE)
            fail(OCRS_ERR_INVALID_ARGUMENT, "skew scores: a page of %d x %d: a side is at most %d (estimate on a work copy)", p->h, p->w, SKEW_MAX_SIDE);
        k::SkewDesc& d = descs[i];
        d.src = p->grey.as<float>();
        d.h = p->h;
        d.w = p->w;
        d.nb = p->h + p->w;
        d.block0 = (int32_t)blocks;
        blocks += k::skew_tiles(p->h, p->w);
        dwords += n_angles * (size_t)d.nb;
        if (blocks > std::numeric_limits<int32_t>::max() || dwords > ((size_t)1 << 29))
            fail(OCRS_ERR_CAPACITY, "skew scores: the profiles of one call take more than 2 GiB");
    }
    uint32_t* d_prof = ws.alloc_n<uint32_t>(dwords);
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        descs[i].prof = d_prof + at;
        at += n_angles * (size_t)descs[i].nb;
    }
    k::SkewDesc* d_descs = ws.alloc_n<k::SkewDesc>(n);
    int32_t* d_table = ws.alloc_n<int32_t>(2 * n_angles);
    unsigned long long* d_scores = ws.alloc_n<unsigned long long>(n * n_angles);
    ws.upload(d_descs, descs.data(), n * sizeof(k::SkewDesc));
    ws.upload(d_table, sc_table, 2 * n_angles * sizeof(int32_t));
    OCRS_HIP(hipMemsetAsync(d_prof, 0, dwords * sizeof(uint32_t), ws.s()));
    k::skew_scores(d_descs, (int)n, (int)blocks, d_table, (int)n_angles, d_scores, ws.s());
    OCRS_HIP(hipGetLastError());
    ws.download(out_scores, d_scores, n * n_angles * sizeof(uint64_t));
    ws.sync();
}

void skew_table(long first, size_t n, double step_deg, int32_t* sc_table) {
    for (size_t i = 0; i < n; i++) {
        const double deg = (double)(first + (long)i) * step_deg, th = deg * (PI / 180.0);
        if (!std::isfinite(th)) fail(OCRS_ERR_INVALID_ARGUMENT, "skew table: an angle that is not finite");
        sc_table[2 * i] = (int32_t)std::nearbyint(std::sin(th) * (double)SKEW_Q16);   // to nearest, ties to even (numpy's rint)
        sc_table[2 * i + 1] = (int32_t)std::nearbyint(std::cos(th) * (double)SKEW_Q16);
    }
}

// the coarse angles are the multiples -K r .. K r of the fine step, r fine steps apart
struct SkewPlan { long r, K; };

SkewPlan check_skew_params(const ocrs_skew_params& p) {
    if (p.work_max_side < 1 || p.work_max_side > SKEW_MAX_SIDE)
        fail(OCRS_ERR_INVALID_ARGUMENT, "skew: work_max_side %d: 1 .. %d", p.work_max_side, SKEW_MAX_SIDE);
    if (!(p.fine_step_deg > 0.0) || !std::isfinite(p.fine_step_deg)) fail(OCRS_ERR_INVALID_ARGUMENT, "skew: the fine step is finite and positive");
    if (!(p.max_deg > 0.0) || !(p.max_deg <= 45.0)) fail(OCRS_ERR_INVALID_ARGUMENT, "skew: max_deg %g: above 0, at most 45 (quarter turns are another call's)", p.max_deg);
    const double ratio = p.coarse_step_deg / p.fine_step_deg, r = std::floor(ratio + 0.5);
    if (!std::isfinite(ratio) || r < 1.0 || r > 1e6 || std::fabs(ratio - r) > 1e-6 * r)
        fail(OCRS_ERR_INVALID_ARGUMENT, "skew: the coarse step is a whole multiple of the fine step");
    const double K = std::floor(p.max_deg / p.coarse_step_deg + 1e-9);
    if (K < 1.0 || 2.0 * K + 1.0 > (double)SKEW_MAX_ANGLES || 2.0 * r + 1.0 > (double)SKEW_MAX_ANGLES)
        fail(OCRS_ERR_INVALID_ARGUMENT, "skew: max_deg holds 1 .. %zu coarse steps either way", (SKEW_MAX_ANGLES - 1) / 2);
    return {(long)r, (long)K};
}

// arg max over scores of the angles first, first + stride, ...: ties to the smaller |angle|, then to the negative one
size_t best_angle(const std::vector<uint64_t>& scores, long first, long stride) {
    size_t best = 0;
    for (size_t i = 1; i < scores.size(); i++) {
        const long a = first + (long)i * stride, b = first + (long)best * stride;
        if (scores[i] > scores[best] || (scores[i] == scores[best] && (std::labs(a) < std::labs(b) || (std::labs(a) == std::labs(b) && a < b)))) best = i;
    }
    return best;
}

void check_map(const float* m) {
    for (int i = 0; i < 6; i++)
        if (!std::isfinite(m[i])) fail(OCRS_ERR_INVALID_ARGUMENT, "a map coefficient that is not finite");
}

// every page warped into a new page of its own, all in one launch on `ws`'s stream; waits for it
PageBatch<k::WarpDesc> warp_pages(Workspace& ws, const ocrs_page* const* pages, size_t n, const int* out_hw, const float* m, const float* fill) {
    PageBatch<k::WarpDesc> batch{"warp"};
    for (size_t i = 0; i < n; i++) {
        const int oh = out_hw[2 * i], ow = out_hw[2 * i + 1];
        if (oh < 1 || oh > MAX_PAGE_SIDE || ow < 1 || ow > MAX_PAGE_SIDE)
            fail(OCRS_ERR_INVALID_ARGUMENT, "warp: %d x %d: a side is 1 .. %d", oh, ow, MAX_PAGE_SIDE);
        check_page_side("warp", pages[i]);
        check_map(m + 6 * i);
    }
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        k::WarpDesc& d = batch.add(out_hw[2 * i], out_hw[2 * i + 1], k::warp_blocks(out_hw[2 * i], out_hw[2 * i + 1]));
        d.src = p->grey.as<float>();
        d.dst = batch.made.back()->grey.as<float>();
        d.sh = p->h;
        d.sw = p->w;
        d.dh = out_hw[2 * i];
        d.dw = out_hw[2 * i + 1];
        d.vec = vec16_ok(d.dw, d.dst, d.dst) ? 1 : 0;
        for (int q = 0; q < 6; q++) d.m[q] = m[6 * i + q];
        d.fill = fill[i];
    }
    batch.run(ws, [&](const k::WarpDesc* d_descs, int n_pages, int blocks) { k::warp_pages(d_descs, n_pages, blocks, ws.s()); });
    return batch;
}

inline float round_once(double v) { return (float)v; }

int32_t to_i32(double v) {   // of a floor or a ceil; saturating
    if (!(v > -2147483648.0)) return std::numeric_limits<int32_t>::min();
    if (!(v < 2147483647.0)) return std::numeric_limits<int32_t>::max();
    return (int32_t)v;
}

}  // namespace

extern "C" {

ocrs_status ocrs_skew_params_default(ocrs_skew_params* out) {
    return guarded([&] {
        if (!out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        out->max_deg = 15.0;
        out->coarse_step_deg = 0.5;
        out->fine_step_deg = 0.1;
        out->work_max_side = 1024;
        out->reserved = 0;
    });
}

ocrs_status ocrs_skew_params_check(const ocrs_skew_params* params) {
    return guarded([&] {
        if (!params) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        (void)check_skew_params(*params);
    });
}

ocrs_status ocrs_skew_table(int first, size_t n, double step_deg, int32_t* sc_table) {
    return guarded([&] {
        if (n > 0 && !sc_table) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        if (!std::isfinite(step_deg)) fail(OCRS_ERR_INVALID_ARGUMENT, "skew table: a step that is not finite");
        skew_table(first, n, step_deg, sc_table);
    });
}

ocrs_status ocrs_engine_skew_scores(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const int32_t* sc_table, size_t n_angles,
                                    uint64_t* out_scores) {
    return guarded_engine(e, [&] {
        if (!e || !sc_table || (n > 0 && (!pages || !out_scores))) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_table(sc_table, n_angles);
        check_pages_on(e, pages, n);
        Workspace ws;
        skew_scores(ws, pages, n, sc_table, n_angles, out_scores);
    });
}

ocrs_status ocrs_engine_estimate_skew(const ocrs_engine* e, const ocrs_page* page, const ocrs_skew_params* params, ocrs_skew_info* out) {
    return guarded_engine(e, [&] {
        if (!e || !page || !out) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        ocrs_skew_params p;
        if (params) p = *params;
        else ocrs_skew_params_default(&p);
        const SkewPlan plan = check_skew_params(p);
        check_pages_on(e, &page, 1);
        // 1. the work copy: the area average, when the page is larger than work_max_side
        std::unique_ptr<ocrs_page> work;
        const ocrs_page* wp = page;
        if (std::max(page->h, page->w) > p.work_max_side) {
            int wh = 0, ww = 0;
            ocrs_page* made = nullptr;
            ocrs_status s = ocrs_work_size(page->h, page->w, (double)p.work_max_side / (double)std::max(page->h, page->w), &wh, &ww);
            if (s == OCRS_OK) s = ocrs_engine_resize_page(e, page, wh, ww, OCRS_RESAMPLE_AREA, &made);
            if (s != OCRS_OK) fail(s, "skew: %s", ocrs_last_error());
            work.reset(made);
            wp = made;
        }
        Workspace ws;
        // 2. the coarse angles
        std::vector<int32_t> table(2 * (size_t)(2 * plan.K + 1));
        std::vector<uint64_t> coarse((size_t)(2 * plan.K + 1));
        for (long i = 0; i <= 2 * plan.K; i++) skew_table((i - plan.K) * plan.r, 1, p.fine_step_deg, table.data() + 2 * i);
        skew_scores(ws, &wp, 1, table.data(), coarse.size(), coarse.data());
        const size_t cb = best_angle(coarse, -plan.K * plan.r, plan.r);
        const long ck = ((long)cb - plan.K) * plan.r;
        uint64_t second = 0;
        for (size_t i = 0; i < coarse.size(); i++)
            if (i != cb) second = std::max(second, coarse[i]);
        // 3. the fine angles around the best coarse one
        std::vector<uint64_t> fine((size_t)(2 * plan.r + 1));
        table.resize(2 * fine.size());
        skew_table(ck - plan.r, fine.size(), p.fine_step_deg, table.data());
        skew_scores(ws, &wp, 1, table.data(), fine.size(), fine.data());
        // 4. arg max
        const long fk = ck - plan.r + (long)best_angle(fine, ck - plan.r, 1);
        out->angle_deg = (double)fk * p.fine_step_deg;
        out->best_score = coarse[cb];
        out->second_score = second;
        out->fine_score = fine[(size_t)(fk - (ck - plan.r))];
        out->work_h = wp->h;
        out->work_w = wp->w;
        out->coarse_index = (int32_t)ck;
        out->fine_index = (int32_t)fk;
    });
}

ocrs_status ocrs_engine_warp_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const int* out_hw, const float* m,
                                   const float* fill, ocrs_page** out) {
    return guarded_engine(e, [&] {
        if (!e || (n > 0 && (!pages || !out_hw || !m || !fill || !out))) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_pages_on(e, pages, n);
        Workspace ws;
        warp_pages(ws, pages, n, out_hw, m, fill).release_into(out);
    });
}

ocrs_status ocrs_engine_warp_page(const ocrs_engine* e, const ocrs_page* page, int out_h, int out_w, const float m[6], float fill,
                                  ocrs_page** out) {
    const int hw[2] = {out_h, out_w};
    return ocrs_engine_warp_pages(e, &page, 1, hw, m, &fill, out);
}

ocrs_status ocrs_deskew_map(int h, int w, double angle_deg, int expand, int out_hw[2], float m[6]) {
    return guarded([&] {
        if (!out_hw || !m) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        if (h < 1 || w < 1 || h > MAX_PAGE_SIDE || w > MAX_PAGE_SIDE) fail(OCRS_ERR_INVALID_ARGUMENT, "deskew map: a page of %d x %d", h, w);
        if (!(std::fabs(angle_deg) <= 45.0)) fail(OCRS_ERR_INVALID_ARGUMENT, "deskew map: %g degrees: at most 45 either way (quarter turns are another call's)", angle_deg);
        const double th = angle_deg * (PI / 180.0), c = std::cos(th), s = std::sin(th);
        double ow = (double)w, oh = (double)h;
        if (expand) {
            ow = std::ceil((double)w * std::fabs(c) + (double)h * std::fabs(s));
            oh = std::ceil((double)w * std::fabs(s) + (double)h * std::fabs(c));
        }
        if (ow > (double)MAX_PAGE_SIDE || oh > (double)MAX_PAGE_SIDE) fail(OCRS_ERR_INVALID_ARGUMENT, "deskew map: the upright page would have a side over %d", MAX_PAGE_SIDE);
        out_hw[0] = (int)oh;
        out_hw[1] = (int)ow;
        m[0] = round_once((((double)w / 2.0 - 0.5) - c * ow / 2.0) - s * oh / 2.0);
        m[1] = round_once(c);
        m[2] = round_once(s);
        m[3] = round_once((((double)h / 2.0 - 0.5) + s * ow / 2.0) - c * oh / 2.0);
        m[4] = round_once(-s);
        m[5] = round_once(c);
    });
}

ocrs_status ocrs_unwarp_rects(float* rects6, size_t n, const float m[6]) {
    return guarded([&] {
        if (!m || (n > 0 && !rects6)) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_map(m);
        const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
        const double lw = std::sqrt(m1 * m1 + m4 * m4), lh = std::sqrt(m2 * m2 + m5 * m5);
        for (size_t i = 0; i < n; i++) {
            float* a = rects6 + 6 * i;
            bool finite = true;
            for (int q = 0; q < 6; q++) finite = finite && std::isfinite(a[q]);
            if (!finite) continue;   // passes through as it is
            const double fx = (double)a[0] + 0.5, fy = (double)a[1] + 0.5, ux = a[2], uy = a[3];
            a[0] = (float)((m0 + m1 * fx) + m2 * fy);
            a[1] = (float)((m3 + m4 * fx) + m5 * fy);
            const double vx = m1 * ux + m2 * uy, vy = m4 * ux + m5 * uy, lv = std::sqrt(vx * vx + vy * vy);
            if (lv > 0.0 && std::isfinite(lv)) {
                a[2] = (float)(vx / lv);
                a[3] = (float)(vy / lv);
            }
            a[4] = (float)((double)a[4] * lw);
            a[5] = (float)((double)a[5] * lh);
        }
    });
}

ocrs_status ocrs_unwarp_chars(ocrs_text_char* chars, size_t n, const float m[6]) {
    return guarded([&] {
        if (!m || (n > 0 && !chars)) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_map(m);
        const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
        for (size_t i = 0; i < n; i++) {
            ocrs_text_char& c = chars[i];
            const double xs[2] = {(double)c.left + 0.5, (double)c.right + 0.5}, ys[2] = {(double)c.top + 0.5, (double)c.bottom + 0.5};
            double x0 = 0, x1 = 0, y0 = 0, y1 = 0;
            for (int q = 0; q < 4; q++) {
                const double fx = xs[q & 1], fy = ys[q >> 1];
                const double X = (m0 + m1 * fx) + m2 * fy, Y = (m3 + m4 * fx) + m5 * fy;
                x0 = q ? std::min(x0, X) : X; x1 = q ? std::max(x1, X) : X;
                y0 = q ? std::min(y0, Y) : Y; y1 = q ? std::max(y1, Y) : Y;
            }
            c.left = to_i32(std::floor(x0));
            c.right = to_i32(std::ceil(x1));
            c.top = to_i32(std::floor(y0));
            c.bottom = to_i32(std::ceil(y1));
        }
    });
}

}  // extern "C"
