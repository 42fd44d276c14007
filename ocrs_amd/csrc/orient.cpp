// Quarter turns and auto-orientation (include/ocrs_amd.h "Quarter turns"): turning resident pages on the
// device, mapping results of a turned page back to the scan's frame, and the probe that decides which way is up.
#include <cmath>
#include <limits>
#include <numeric>

#include "abi_util.hpp"
#include "engine.hpp"
#include "kernels.hpp"
#include "page_ops.hpp"

using namespace ocrs;
using namespace ocrs::geom;
using namespace ocrs::abi;

namespace {

inline int reduce_turns(int k) { return ((k % 4) + 4) % 4; }

// np.rot90(page, k) of every page as a new page of its own, all in one launch on `ws`'s stream; waits for it.
PageBatch<k::RotateDesc> rotate_pages(Workspace& ws, const ocrs_page* const* pages, size_t n, const int* turns) {
    PageBatch<k::RotateDesc> batch{"rotate"};
    for (size_t i = 0; i < n; i++) {
        const ocrs_page* p = pages[i];
        const int k = reduce_turns(turns[i]);
        k::RotateDesc& d = batch.add((k & 1) ? p->w : p->h, (k & 1) ? p->h : p->w, k::rotate_tiles(p->h, p->w));
        d.src = p->grey.as<uint32_t>();
        d.dst = batch.made.back()->grey.as<uint32_t>();
        d.h = p->h;
        d.w = p->w;
        d.k = k;
        d.vec = vec16_ok(p->w, d.src, d.dst) ? 1 : 0;
    }
    batch.run(ws, [&](const k::RotateDesc* d_descs, int n_pages, int tiles) { k::rotate_pages(d_descs, n_pages, tiles, ws.s()); });
    return batch;
}

// the word-shape vote: out[0] = summed widths of the words that are wider than tall, out[1] = summed heights of the others
void orientation_vote(const float* rects6, size_t n, double out[2]) {
    out[0] = out[1] = 0.0;
    for (size_t i = 0; i < n; i++) {
        const float* a = rects6 + 6 * i;
        bool finite = true;
        for (int q = 0; q < 6; q++) finite = finite && std::isfinite(a[q]);
        if (!finite) continue;
        const auto c = RotatedRect::from_array(a).corners();
        float x0 = c[0].x, x1 = c[0].x, y0 = c[0].y, y1 = c[0].y;
        for (int q = 0; q < 4; q++) finite = finite && std::isfinite(c[q].x) && std::isfinite(c[q].y);
        if (!finite) continue;
        for (int q = 1; q < 4; q++) {
            x0 = std::min(x0, c[q].x); x1 = std::max(x1, c[q].x);
            y0 = std::min(y0, c[q].y); y1 = std::max(y1, c[q].y);
        }
        const float bw = x1 - x0, bh = y1 - y0;
        if (!std::isfinite(bw) || !std::isfinite(bh)) continue;
        if (bw >= bh) out[0] += (double)bw;
        else out[1] += (double)bh;
    }
}

// up to max_lines (0: all) lines, those of the most words first, ties to the lower index; returned in ascending index
std::vector<size_t> sample_lines(const std::vector<std::vector<RotatedRect>>& lines, size_t max_lines) {
    std::vector<size_t> order(lines.size());
    std::iota(order.begin(), order.end(), (size_t)0);
    if (max_lines == 0 || max_lines >= lines.size()) return order;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return lines[a].size() > lines[b].size(); });
    order.resize(max_lines);
    std::sort(order.begin(), order.end());
    return order;
}

}  // namespace

extern "C" {

ocrs_status ocrs_engine_rotate_pages(const ocrs_engine* e, const ocrs_page* const* pages, size_t n, const int* quarter_turns,
                                     ocrs_page** out) {
    return guarded_engine(e, [&] {
        if (!e || (n > 0 && (!pages || !quarter_turns || !out))) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_pages_on(e, pages, n);
        Workspace ws;
        rotate_pages(ws, pages, n, quarter_turns).release_into(out);
    });
}

ocrs_status ocrs_engine_rotate_page(const ocrs_engine* e, const ocrs_page* page, int quarter_turns, ocrs_page** out) {
    return ocrs_engine_rotate_pages(e, &page, 1, &quarter_turns, out);
}

ocrs_status ocrs_unrotate_rects(float* rects6, size_t n, int page_h, int page_w, int k) {
    return guarded([&] {
        if (n > 0 && !rects6) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        const float xm = (float)(page_w - 1), ym = (float)(page_h - 1);
        k = reduce_turns(k);
        for (size_t i = 0; i < n && k != 0; i++) {
            float* a = rects6 + 6 * i;
            const float x = a[0], y = a[1], ux = a[2], uy = a[3];
            if (k == 1) { a[0] = xm - y; a[1] = x; a[2] = -uy; a[3] = ux; }
            else if (k == 2) { a[0] = xm - x; a[1] = ym - y; a[2] = -ux; a[3] = -uy; }
            else { a[0] = y; a[1] = ym - x; a[2] = uy; a[3] = -ux; }
        }
    });
}

ocrs_status ocrs_unrotate_chars(ocrs_text_char* chars, size_t n, int page_h, int page_w, int k) {
    return guarded([&] {
        if (n > 0 && !chars) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        // two's-complement arithmetic (a box far outside the page wraps instead of overflowing)
        const uint32_t xm = (uint32_t)page_w - 1u, ym = (uint32_t)page_h - 1u;
        k = reduce_turns(k);
        for (size_t i = 0; i < n && k != 0; i++) {
            ocrs_text_char& c = chars[i];
            const uint32_t t = (uint32_t)c.top, l = (uint32_t)c.left, b = (uint32_t)c.bottom, r = (uint32_t)c.right;
            if (k == 1) { c.left = (int32_t)(xm - b); c.right = (int32_t)(xm - t); c.top = (int32_t)l; c.bottom = (int32_t)r; }
            else if (k == 2) { c.left = (int32_t)(xm - r); c.right = (int32_t)(xm - l); c.top = (int32_t)(ym - b); c.bottom = (int32_t)(ym - t); }
            else { c.left = (int32_t)t; c.right = (int32_t)b; c.top = (int32_t)(ym - r); c.bottom = (int32_t)(ym - l); }
        }
    });
}

ocrs_status ocrs_orientation_vote(const float* rects6, size_t n, double out[2]) {
    return guarded([&] {
        if (!out || (n > 0 && !rects6)) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        orientation_vote(rects6, n, out);
    });
}

ocrs_status ocrs_engine_detect_orientation(const ocrs_engine* e, const ocrs_page* page, size_t max_lines, int* quarter_turns,
                                           double vote[2], double score[4], uint32_t n_chars[4]) {
    return guarded_engine(e, [&] {
        if (!e || !page || !quarter_turns) fail(OCRS_ERR_INVALID_ARGUMENT, "null argument");
        check_pages_on(e, &page, 1);
        // (a) the words of the page as given, and which way they read
        std::vector<std::vector<RotatedRect>> words0;
        e->detect(&page, 1, &words0, nullptr);
        std::vector<float> flat;
        append_rects(flat, words0[0]);
        double v[2];
        orientation_vote(flat.data(), words0[0].size(), v);
        const int cand[2] = {v[0] >= v[1] ? 0 : 1, v[0] >= v[1] ? 2 : 3};
        // (b) the candidates other than 0: turned in one launch, detected as one batch
        std::vector<int> turns;
        for (int c : cand)
            if (c != 0) turns.push_back(c);
        std::vector<const ocrs_page*> src(turns.size(), page);
        std::vector<std::unique_ptr<ocrs_page>> turned;
        {
            Workspace ws;
            turned = std::move(rotate_pages(ws, src.data(), src.size(), turns.data()).made);
        }
        std::vector<const ocrs_page*> tp;
        for (const auto& p : turned) tp.push_back(p.get());
        std::vector<std::vector<RotatedRect>> wordsT;
        e->detect(tp.data(), tp.size(), &wordsT, nullptr);
        // (c) lines per candidate, sampled
        const ocrs_page* cpages[2];
        std::vector<std::vector<std::vector<RotatedRect>>> lpp(2);
        for (int q = 0, t = 0; q < 2; q++) {
            const bool as_given = cand[q] == 0;
            cpages[q] = as_given ? page : tp[t];
            const auto lines = find_text_lines(as_given ? words0[0] : wordsT[t]);
            if (!as_given) t++;
            for (size_t li : sample_lines(lines, max_lines)) lpp[q].push_back(lines[li]);
        }
        // (d) one scored recognition batch over both candidates' lines
        std::vector<RecResult> res;
        e->recognize(cpages, 2, lpp, &res, true, false);
        // (e) the mean char log-prob per candidate
        double sc[4];
        uint32_t nc[4] = {0, 0, 0, 0};
        for (int q = 0; q < 4; q++) sc[q] = std::numeric_limits<double>::quiet_NaN();
        size_t at = 0;
        std::vector<float> lp;
        for (int q = 0; q < 2; q++) {
            double sum = 0.0;
            uint32_t cnt = 0;
            for (size_t li = 0; li < lpp[q].size(); li++, at++) {
                e->text_line_from_result(res[at], &lp);
                for (float x : lp) sum += (double)x;
                cnt += (uint32_t)lp.size();
            }
            sc[cand[q]] = cnt ? sum / (double)cnt : -std::numeric_limits<double>::infinity();
            nc[cand[q]] = cnt;
        }
        // (f) the larger score; a tie, and nothing read either way, goes to the smaller turn
        *quarter_turns = sc[cand[1]] > sc[cand[0]] ? cand[1] : cand[0];
        if (vote) { vote[0] = v[0]; vote[1] = v[1]; }
        for (int q = 0; q < 4; q++) {
            if (score) score[q] = sc[q];
            if (n_chars) n_chars[q] = nc[q];
        }
    });
}

}  // extern "C"
