// Perspective correction, the host half: choosing a page's outline among the edge peaks, the projective
// map of a quad, and the maps that bring results of the projected page back.  No HIP and no library dependencies, in the
// way of spec_math.hpp and beam_math.hpp: perspective.cpp and tests/sanitize/perspective_harness.cpp run the same code.
// Every result is a fixed sequence of double operations (+ - * / sqrt floor ceil, no libm trigonometry; build with
// -ffp-contract=off), which tests/perspective_ref.py restates in the same order: the two agree bit for bit.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

namespace ocrs {
namespace persp {

constexpr int BANDS = 16;           // peaks kept per profile row
constexpr int MAX_SIDE = 4096;      // of a page the peaks are taken on: x S + y C - t0 stays inside int32
constexpr int Q16 = 65536;
constexpr int MAX_OUT_SIDE = 65535;

struct Params {
    double max_deg, step_deg, min_cover, min_span, min_area;
    int32_t work_max_side, min_step;
};

inline Params default_params() { return {15.0, 0.5, 0.25, 0.25, 0.1, 512, 8}; }

// the angles are the multiples -K .. K of step_deg; 0 when a value is out of range
inline long plan(const Params& p) {
    if (p.work_max_side < 1 || p.work_max_side > MAX_SIDE) return 0;
    if (p.min_step < 1 || p.min_step > 256) return 0;
    if (!(p.step_deg > 0.0) || !std::isfinite(p.step_deg)) return 0;
    if (!(p.max_deg > 0.0) || !(p.max_deg <= 45.0)) return 0;
    if (!(p.min_cover > 0.0) || !(p.min_cover <= 1.0)) return 0;
    if (!(p.min_span > 0.0) || !(p.min_span <= 1.0)) return 0;
    if (!(p.min_area >= 0.0) || !(p.min_area <= 1.0)) return 0;
    const double K = std::floor(p.max_deg / p.step_deg + 1e-9);
    if (K < 1.0 || 2.0 * K + 1.0 > 4095.0) return 0;
    return (long)K;
}

struct Outline {
    int32_t found = 0;
    float corners[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // TL, TR, BR, BL as (x, y), the source page's pixel-index frame
    int32_t polarity = 0;                          // 0: `+` first (the sheet is lighter than the desk), 1: `-` first
    uint32_t counts[4] = {0, 0, 0, 0};             // top, bottom, left, right
    int32_t angles[4] = {0, 0, 0, 0};              // their indices into the table
};

struct Line {
    double a, b, d;   // a x + b y = d in the work page's pixel-index frame
    double pos;
    uint32_t count;
    int32_t angle;
};

// the candidates of one (family, sign), in ascending (angle index, bin)
inline void candidates(const uint64_t* peaks, const int32_t* sc_table, size_t n_angles, int family, int sign, int wh, int ww, double min_cover,
                       std::vector<Line>* out) {
    out->clear();
    const double L = family == 0 ? (double)ww : (double)wh;
    const double need = std::ceil(min_cover * L);
    // the family's own page: the work page (H) or its transpose (V)
    const int fw = family == 0 ? ww : wh, fh = family == 0 ? wh : ww;
    for (size_t a = 0; a < n_angles; a++) {
        const int64_t S = sc_table[2 * a], C = sc_table[2 * a + 1];
        const int64_t t0 = std::min<int64_t>(0, (int64_t)(fw - 1) * S) + std::min<int64_t>(0, (int64_t)(fh - 1) * C);
        const double s = (double)S / 65536.0, c = (double)C / 65536.0;
        for (int k = 0; k < BANDS; k++) {
            const uint64_t e = peaks[(((size_t)family * 2 + (size_t)sign) * n_angles + a) * BANDS + (size_t)k];
            if (e == 0) continue;
            const uint32_t count = (uint32_t)(e >> 32);
            const int64_t bin = (int64_t)(0xFFFFFFFFu - (uint32_t)(e & 0xFFFFFFFFu));
            if (!((double)count >= need)) continue;
            const double rho = (double)(bin * 65536 + 32768 + t0) / 65536.0;
            const double d = rho + 0.5 * c;
            Line ln;
            // along the family's page the line is s x' + c y' = d; for family V x' = y and y' = x
            ln.a = family == 0 ? s : c;
            ln.b = family == 0 ? c : s;
            ln.d = d;
            const double mid = ((double)fw - 1.0) / 2.0;
            ln.pos = (d - s * mid) / c;
            ln.count = count;
            ln.angle = (int32_t)a;
            if (std::isfinite(ln.pos)) out->push_back(ln);
        }
    }
}

// the pair (first, second) of largest count sum whose positions lie at least `span` apart; ties to the earlier first, then
// to the earlier second.  false: no pair
inline bool best_pair(const std::vector<Line>& first, const std::vector<Line>& second, double span, size_t* bi, size_t* bj) {
    bool any = false;
    uint64_t best = 0;
    for (size_t i = 0; i < first.size(); i++)
        for (size_t j = 0; j < second.size(); j++) {
            if (!(second[j].pos - first[i].pos >= span)) continue;
            const uint64_t sum = (uint64_t)first[i].count + (uint64_t)second[j].count;
            if (!any || sum > best) {
                any = true;
                best = sum;
                *bi = i;
                *bj = j;
            }
        }
    return any;
}

inline void intersect(const Line& p, const Line& q, double* x, double* y) {
    const double det = p.a * q.b - q.a * p.b;
    *x = (p.d * q.b - q.d * p.b) / det;
    *y = (p.a * q.d - q.a * p.d) / det;
}

// peaks: uint64 [2 families][2 signs][n_angles][16] of a work page of wh x ww taken from a page of ph x pw
inline Outline choose(const uint64_t* peaks, const int32_t* sc_table, size_t n_angles, int wh, int ww, int ph, int pw, const Params& p) {
    Outline none;
    std::vector<Line> cand[2][2];
    for (int f = 0; f < 2; f++)
        for (int s = 0; s < 2; s++) candidates(peaks, sc_table, n_angles, f, s, wh, ww, p.min_cover, &cand[f][s]);
    const double span[2] = {p.min_span * ((double)wh - 1.0), p.min_span * ((double)ww - 1.0)};
    int best_sigma = -1;
    uint64_t best_sum = 0;
    size_t pick[2][2][2] = {};   // [sigma][family][first | second]
    for (int sigma = 0; sigma < 2; sigma++) {
        bool ok = true;
        uint64_t sum = 0;
        for (int f = 0; f < 2 && ok; f++) {
            const std::vector<Line>&a = cand[f][sigma], &b = cand[f][1 - sigma];
            ok = best_pair(a, b, span[f], &pick[sigma][f][0], &pick[sigma][f][1]);
            if (ok) sum += (uint64_t)a[pick[sigma][f][0]].count + (uint64_t)b[pick[sigma][f][1]].count;
        }
        if (ok && (best_sigma < 0 || sum > best_sum)) {
            best_sigma = sigma;
            best_sum = sum;
        }
    }
    if (best_sigma < 0) return none;
    const int sg = best_sigma;
    const Line& top = cand[0][sg][pick[sg][0][0]];
    const Line& bottom = cand[0][1 - sg][pick[sg][0][1]];
    const Line& left = cand[1][sg][pick[sg][1][0]];
    const Line& right = cand[1][1 - sg][pick[sg][1][1]];
    const Line* hs[4] = {&top, &top, &bottom, &bottom};
    const Line* vs[4] = {&left, &right, &right, &left};
    const double kx = (double)pw / (double)ww, ky = (double)ph / (double)wh;
    Outline o;
    double c[8];
    for (int q = 0; q < 4; q++) {
        double x, y;
        intersect(*hs[q], *vs[q], &x, &y);
        o.corners[2 * q] = (float)((x + 0.5) * kx - 0.5);
        o.corners[2 * q + 1] = (float)((y + 0.5) * ky - 0.5);
        if (!std::isfinite(o.corners[2 * q]) || !std::isfinite(o.corners[2 * q + 1])) return none;
        c[2 * q] = (double)o.corners[2 * q];
        c[2 * q + 1] = (double)o.corners[2 * q + 1];
    }
    double area2 = 0.0;
    for (int q = 0; q < 4; q++) {
        const int r = (q + 1) & 3, t = (q + 2) & 3;
        const double e1x = c[2 * r] - c[2 * q], e1y = c[2 * r + 1] - c[2 * q + 1];
        const double e2x = c[2 * t] - c[2 * r], e2y = c[2 * t + 1] - c[2 * r + 1];
        if (!(e1x * e2y - e1y * e2x > 0.0)) return none;
        area2 += c[2 * q] * c[2 * r + 1] - c[2 * r] * c[2 * q + 1];
    }
    if (!(0.5 * area2 >= p.min_area * (double)ph * (double)pw)) return none;
    o.found = 1;
    o.polarity = sg;
    const Line* four[4] = {&top, &bottom, &left, &right};
    for (int q = 0; q < 4; q++) {
        o.counts[q] = four[q]->count;
        o.angles[q] = four[q]->angle;
    }
    return o;
}

inline double side_len(double ax, double ay, double bx, double by) {
    const double dx = bx - ax, dy = by - ay;
    return std::sqrt(dx * dx + dy * dy);
}

inline int out_side(double l1, double l2) {
    const double v = std::floor((l1 > l2 ? l1 : l2) + 0.5);
    if (!(v >= 1.0)) return 1;
    if (v > (double)MAX_OUT_SIDE) return MAX_OUT_SIDE;
    return (int)v;
}

// corners: TL, TR, BR, BL as (x, y) -> out_hw = {H', W'} and m[8]: Heckbert's square-to-quad map with u = fx / W',
// v = fy / H'.  false: a value that is not finite or a degenerate quad
inline bool quad_map(const float* corners8, int out_hw[2], float m[8]) {
    for (int i = 0; i < 8; i++)
        if (!std::isfinite(corners8[i])) return false;
    const double x0 = corners8[0], y0 = corners8[1], x1 = corners8[2], y1 = corners8[3], x2 = corners8[4], y2 = corners8[5], x3 = corners8[6],
                 y3 = corners8[7];
    const int ow = out_side(side_len(x0, y0, x1, y1), side_len(x3, y3, x2, y2));
    const int oh = out_side(side_len(x0, y0, x3, y3), side_len(x1, y1, x2, y2));
    const double dx1 = x1 - x2, dx2 = x3 - x2, sx = ((x0 - x1) + x2) - x3;
    const double dy1 = y1 - y2, dy2 = y3 - y2, sy = ((y0 - y1) + y2) - y3;
    const double det = dx1 * dy2 - dy1 * dx2;
    if (det == 0.0 || !std::isfinite(det)) return false;
    const double g = (sx * dy2 - sy * dx2) / det;
    const double h = (dx1 * sy - dy1 * sx) / det;
    const double a = (x1 - x0) + g * x1, b = (x3 - x0) + h * x3;
    const double d = (y1 - y0) + g * y1, e = (y3 - y0) + h * y3;
    const double W = (double)ow, H = (double)oh;
    const double v[8] = {x0, a / W, b / H, y0, d / W, e / H, g / W, h / H};
    for (int i = 0; i < 8; i++) {
        m[i] = (float)v[i];
        if (!std::isfinite(m[i])) return false;
    }
    out_hw[0] = oh;
    out_hw[1] = ow;
    return true;
}

// the point (fx, fy) of the projected page -> its position on the source; false: dn is not finite or not positive
inline bool map_point(const float* m, double fx, double fy, double* X, double* Y, double* dn_out) {
    const double nx = ((double)m[0] + (double)m[1] * fx) + (double)m[2] * fy;
    const double ny = ((double)m[3] + (double)m[4] * fx) + (double)m[5] * fy;
    const double dn = (1.0 + (double)m[6] * fx) + (double)m[7] * fy;
    if (!(dn > 0.0) || !std::isfinite(dn)) return false;
    *X = nx / dn;
    *Y = ny / dn;
    *dn_out = dn;
    return true;
}

// one rect (cx, cy, up.x, up.y, w, h), in place
inline void unproject_rect(float* a, const float* m) {
    for (int q = 0; q < 6; q++)
        if (!std::isfinite(a[q])) return;   // passes through as it is
    double X, Y, dn;
    if (!map_point(m, (double)a[0] + 0.5, (double)a[1] + 0.5, &X, &Y, &dn)) return;
    const double j00 = ((double)m[1] - (double)m[6] * X) / dn, j01 = ((double)m[2] - (double)m[7] * X) / dn;
    const double j10 = ((double)m[4] - (double)m[6] * Y) / dn, j11 = ((double)m[5] - (double)m[7] * Y) / dn;
    const double ux = a[2], uy = a[3];
    const double vx = j00 * ux + j01 * uy, vy = j10 * ux + j11 * uy, lv = std::sqrt(vx * vx + vy * vy);
    const double px = j00 * (-uy) + j01 * ux, py = j10 * (-uy) + j11 * ux, lp = std::sqrt(px * px + py * py);
    a[0] = (float)X;
    a[1] = (float)Y;
    if (lv > 0.0 && std::isfinite(lv)) {
        a[2] = (float)(vx / lv);
        a[3] = (float)(vy / lv);
    }
    a[4] = (float)((double)a[4] * lp);
    a[5] = (float)((double)a[5] * lv);
}

inline int32_t to_i32(double v) {   // of a floor or a ceil; saturating
    if (!(v > -2147483648.0)) return std::numeric_limits<int32_t>::min();
    if (!(v < 2147483647.0)) return std::numeric_limits<int32_t>::max();
    return (int32_t)v;
}

// one box (top, left, bottom, right), in place: the four corners through the map, floor of the minimum, ceil of the
// maximum; a box with a corner the map does not reach (dn <= 0) passes through as it is
inline void unproject_box(int32_t* tlbr, const float* m) {
    const double xs[2] = {(double)tlbr[1] + 0.5, (double)tlbr[3] + 0.5}, ys[2] = {(double)tlbr[0] + 0.5, (double)tlbr[2] + 0.5};
    double x0 = 0, x1 = 0, y0 = 0, y1 = 0;
    for (int q = 0; q < 4; q++) {
        double X, Y, dn;
        if (!map_point(m, xs[q & 1], ys[q >> 1], &X, &Y, &dn)) return;
        x0 = q ? (X < x0 ? X : x0) : X; x1 = q ? (X > x1 ? X : x1) : X;
        y0 = q ? (Y < y0 ? Y : y0) : Y; y1 = q ? (Y > y1 ? Y : y1) : Y;
    }
    tlbr[0] = to_i32(std::floor(y0));
    tlbr[1] = to_i32(std::floor(x0));
    tlbr[2] = to_i32(std::ceil(y1));
    tlbr[3] = to_i32(std::ceil(x1));
}

}  // namespace persp
}  // namespace ocrs
