// Internals shared by the translation units that export C entry points (abi.cpp, group.cpp): exception -> status
// conversion, device binding, marshalling helpers.  Not part of the public header.
#pragma once
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "engine.hpp"

namespace ocrs {
namespace abi {

template <class F>
ocrs_status guarded(F&& f) {   // host-only entry points: no device is touched
    try {
        f();
        set_last_error("");
        return OCRS_OK;
    } catch (const Error& e) {
        set_last_error(e.what());
        return e.status;
    } catch (const std::bad_alloc&) {
        set_last_error("out of host memory");
        return OCRS_ERR_DEVICE;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return OCRS_ERR_RUN_FAILED;
    }
}

// Entry points that do device work: the calling thread is bound to the handle's device for the call
// (device < 0: the process default, ocrs_set_device).
template <class F>
ocrs_status guarded_on(int device, F&& f) {
    return guarded([&] {
        DeviceScope bind(device);
        f();
    });
}

// Entry points of an engine: bound to the engine's device, with the engine's own options installed for the call.
template <class F>
ocrs_status guarded_engine(const ocrs_engine* e, F&& f) {
    return guarded([&] {
        DeviceScope bind(e ? e->device : -1);
        TuningScope tune(e ? &e->tuning : nullptr);
        f();
    });
}

template <class T>
T* dup_buffer(const std::vector<T>& v) {
    T* p = static_cast<T*>(malloc(std::max<size_t>(v.size(), 1) * sizeof(T)));
    if (!p) throw std::bad_alloc();
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

// ---- word rects across the ABI: six floats per rect (RotatedRect::to_array), pages told apart by offsets
inline void append_rects(std::vector<float>& flat, const std::vector<geom::RotatedRect>& rects) {
    for (const geom::RotatedRect& r : rects) {
        float a[6];
        r.to_array(a);
        flat.insert(flat.end(), a, a + 6);
    }
}

inline std::vector<geom::RotatedRect> unpack_words(const float* rects6, size_t n) {
    std::vector<geom::RotatedRect> words(n);
    for (size_t i = 0; i < n; i++) words[i] = geom::RotatedRect::from_array(rects6 + 6 * i);
    return words;
}

// The outputs of a detect_words_batch call from what detection found: rects / offsets[n + 1], and score / pixels when `sc` is
// given.  per_page(i, rects6, n), if any, may rewrite page i's freshly appended rects in place.
template <class PerPage>
void pack_words(const std::vector<std::vector<geom::RotatedRect>>& rr, const DetScores* sc, float** rects, size_t* offsets,
                float** score, uint32_t** pixels, PerPage&& per_page) {
    std::vector<float> flat, fscore;
    std::vector<uint32_t> fpixels;
    offsets[0] = 0;
    for (size_t i = 0; i < rr.size(); i++) {
        const size_t first = flat.size();
        append_rects(flat, rr[i]);
        per_page(i, flat.data() + first, rr[i].size());
        if (sc) {
            fscore.insert(fscore.end(), sc->score[i].begin(), sc->score[i].end());
            fpixels.insert(fpixels.end(), sc->pixels[i].begin(), sc->pixels[i].end());
        }
        offsets[i + 1] = flat.size() / 6;
    }
    if (sc) {
        *score = dup_buffer(fscore);
        *pixels = dup_buffer(fpixels);
    }
    *rects = dup_buffer(flat);
}
inline void pack_words(const std::vector<std::vector<geom::RotatedRect>>& rr, const DetScores* sc, float** rects, size_t* offsets,
                       float** score, uint32_t** pixels) {
    pack_words(rr, sc, rects, offsets, score, pixels, [](size_t, float*, size_t) {});
}

// the overlap argument of the _tiled entry points: negative = the default
inline int tile_overlap_arg(int overlap) { return overlap < 0 ? OCRS_TILE_OVERLAP_DEFAULT : overlap; }

void check_pages_on(const ocrs_engine* e, const ocrs_page* const* pages, size_t n);
std::u32string decode_utf8(const char* s);
void append_utf8(std::string& s, uint32_t c);
std::vector<std::vector<geom::RotatedRect>> unpack_lines(const float* rects, const size_t* offsets, size_t first, size_t last);
// OcrEngine::prepare_input on pixels that are already on the bound device (launch only, no sync)
ocrs_page* make_page(const void* d_pixels, ocrs_pixel_type type, ocrs_dim_order order, int height, int width, int channels,
                     hipStream_t st, StageTimers* T);
// the same for the n pages of one call (one size, one format) in one launch (k::prepare_image_batch); same bits
std::vector<std::unique_ptr<ocrs_page>> make_pages(const void* const* d_pixels, size_t n, ocrs_pixel_type type, ocrs_dim_order order,
                                                   int height, int width, int channels, hipStream_t st, StageTimers* T);
void check_image_args(const void* pixels, int height, int width, int channels);
// OcrEngine::new (lib.rs:132-180)
std::unique_ptr<ocrs_engine> make_engine(const ocrs_engine_params& params);
// flatten per-line characters into the ABI's (chars, char_offsets) form
void flatten_chars(const ocrs_engine* e, const std::vector<RecResult>& res, std::vector<ocrs_text_char>* flat, std::vector<size_t>* offs);

}  // namespace abi
}  // namespace ocrs
