// The choice of page measurement (include/ocrs_amd.h "Page measurement"): the stroke width and the text
// height of a page from its run-length and component histograms, and the work scale that follows from a text height.  Host
// only, nothing but this header: measure.cpp exports it as ocrs_measure_choose and ocrs_work_scale_for_text,
// tests/sanitize/measure_harness.cpp runs it under the sanitizers.  tests/measure_ref.py restates it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace ocrs {
namespace measure {

constexpr int BINS = 256;   // a length, height or width L is counted at min(L, 255)

struct Info {            // the layout of ocrs_measure_info and of the kernels' record
    uint64_t ink;
    uint32_t components, counted;
    uint32_t run_h[BINS], run_v[BINS];
    uint32_t comp_h[BINS], comp_w[BINS];
    uint64_t area_by_h[BINS];
};
struct ChoiceParams {    // the layout of ocrs_measure_choice_params
    double min_height_strokes;   // 0 .. 255, taken in 1/256
};
struct TextScale {       // the layout of ocrs_text_scale
    int32_t stroke;
    int32_t text_height;
    uint32_t support;
    int32_t blank;
};

// min_height_strokes in 1/256, or -1 when it is refused
inline int64_t height_q8(double m) {
    if (!std::isfinite(m) || m < 0.0 || m > 255.0) return -1;
    return (int64_t)std::floor(m * 256.0 + 0.5);
}
inline bool choice_params_ok(const ChoiceParams& p) { return height_q8(p.min_height_strokes) >= 0; }

struct Sum128 {   // an unsigned sum that cannot wrap
    uint64_t hi = 0, lo = 0;
    void add(uint64_t v) {
        const uint64_t s = lo + v;
        hi += s < lo ? 1u : 0u;
        lo = s;
    }
    bool zero() const { return hi == 0 && lo == 0; }
    Sum128 half_up() const {   // (this + 1) / 2; this is at most 254 * 2^64
        Sum128 r = *this;
        r.add(1);
        r.lo = (r.lo >> 1) | (r.hi << 63);
        r.hi >>= 1;
        return r;
    }
    bool at_least(const Sum128& o) const { return hi > o.hi || (hi == o.hi && lo >= o.lo); }
};

// p checked
inline TextScale choose(const Info& info, const ChoiceParams& p) {
    const int64_t q = height_q8(p.min_height_strokes);
    TextScale t = {0, 0, 0u, 1};
    uint64_t best = 0;
    for (int L = 1; L < BINS - 1; L++) {
        const uint64_t px = (uint64_t)L * ((uint64_t)info.run_h[L] + (uint64_t)info.run_v[L]);   // at most 254 * 2^33
        if (px > best) {   // strictly: the smallest L stays on a tie
            best = px;
            t.stroke = L;
        }
    }
    // the lower median of the qualifying heights by ink: 254 areas of 64 bits are added in 128
    uint64_t support = 0;
    Sum128 total;
    for (int H = 1; H < BINS - 1; H++)
        if (256 * (int64_t)H >= q * (int64_t)t.stroke) {
            support += info.comp_h[H];
            total.add(info.area_by_h[H]);
        }
    if (support == 0) return t;
    const Sum128 half = total.half_up();
    Sum128 cum;
    for (int H = 1; H < BINS - 1 && !total.zero(); H++) {
        if (256 * (int64_t)H < q * (int64_t)t.stroke) continue;
        cum.add(info.area_by_h[H]);
        if (cum.at_least(half)) {
            t.text_height = H;
            break;
        }
    }
    t.support = support > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)support;   // 254 bins of uint32: saturates, never wraps
    t.blank = 0;
    return t;
}

inline bool work_scale_args_ok(double target_height, double min_scale, double max_scale) {
    return std::isfinite(target_height) && target_height > 0.0 && std::isfinite(min_scale) && std::isfinite(max_scale) && min_scale > 0.0 &&
           min_scale <= max_scale;
}

// arguments checked; a blank page (text_height <= 0) keeps its size
inline double work_scale_for_text(int text_height, double target_height, double min_scale, double max_scale) {
    if (text_height <= 0) return 1.0;
    const double s = target_height / (double)text_height;
    return s < min_scale ? min_scale : (s > max_scale ? max_scale : s);
}

}  // namespace measure
}  // namespace ocrs
