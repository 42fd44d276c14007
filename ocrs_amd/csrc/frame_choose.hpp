// The choice of page framing (include/ocrs_amd.h "Page framing"): the content box of a page and the gutter
// of a spread from the page's two ink profiles.  Host only, integers only, nothing but this header: frame.cpp exports it as
// ocrs_frame_choose, tests/sanitize/frame_harness.cpp runs it under the sanitizers.  tests/frame_ref.py restates it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ocrs {
namespace frame {

struct ChoiceParams {   // the layout of ocrs_frame_choice_params
    int32_t min_count;          // >= 1: a column or row with at least this much ink is content
    int32_t pad;                // 0 .. 65535: the margin kept around the content
    int32_t gutter_min_width;   // >= 1: the shortest run of quiet columns that is a gutter
    int32_t gutter_max_ink;     // >= 0: a column with at most this much ink is quiet
};
struct Choice {         // the layout of ocrs_frame_choice
    int32_t found;      // 1: some column and some row hold content
    int32_t x0, y0, x1, y1;   // the box, half open; the whole page when nothing was found
    int32_t gutter_x;   // the first column of the right page, or -1
};

inline bool choice_params_ok(const ChoiceParams& p) {
    return p.min_count >= 1 && p.pad >= 0 && p.pad <= 65535 && p.gutter_min_width >= 1 && p.gutter_max_ink >= 0;
}

// [first index with v >= min_count, last such index + 1), or first = n when there is none
inline void extent(const uint32_t* v, int n, uint32_t min_count, int* first, int* past) {
    *first = n;
    *past = 0;
    for (int i = 0; i < n; i++)
        if (v[i] >= min_count) {
            if (*first == n) *first = i;
            *past = i + 1;
        }
}

// h, w >= 1; cols[w], rows[h]; p checked
inline Choice choose(int h, int w, const uint32_t* cols, const uint32_t* rows, const ChoiceParams& p) {
    Choice c = {0, 0, 0, w, h, -1};
    int cx0, cx1, cy0, cy1;
    extent(cols, w, (uint32_t)p.min_count, &cx0, &cx1);
    extent(rows, h, (uint32_t)p.min_count, &cy0, &cy1);
    if (cx0 == w || cy0 == h) return c;
    c.found = 1;
    const int64_t pad = p.pad;   // sides and pad are at most 65535 each: no overflow either way
    c.x0 = (int32_t)(cx0 - pad < 0 ? 0 : cx0 - pad);
    c.y0 = (int32_t)(cy0 - pad < 0 ? 0 : cy0 - pad);
    c.x1 = (int32_t)(cx1 + pad > w ? w : cx1 + pad);
    c.y1 = (int32_t)(cy1 + pad > h ? h : cy1 + pad);
    // the gutter: the longest run of quiet columns inside the middle quarter of the content, the most central on a tie, then
    // the leftmost
    const int64_t span = cx1 - cx0;
    const int b0 = (int)(cx0 + 3 * span / 8), b1 = (int)(cx0 + 5 * span / 8);
    int best_len = 0, best_start = 0;
    int64_t best_off = 0;
    for (int i = b0; i < b1;) {
        if (cols[i] > (uint32_t)p.gutter_max_ink) {
            i++;
            continue;
        }
        int j = i;
        while (j < b1 && cols[j] <= (uint32_t)p.gutter_max_ink) j++;
        const int len = j - i;
        const int64_t mid = i + len / 2, d = 2 * mid - ((int64_t)cx0 + cx1), off = d < 0 ? -d : d;
        if (len > best_len || (len == best_len && off < best_off)) {   // runs come in ascending order: the leftmost stays on a full tie
            best_len = len;
            best_start = i;
            best_off = off;
        }
        i = j;
    }
    if (best_len >= p.gutter_min_width) c.gutter_x = best_start + best_len / 2;
    return c;
}

}  // namespace frame
}  // namespace ocrs
