// Memory-safety evidence for the host half of perspective correction.  TEST INFRASTRUCTURE.
// tests/test_perspective_cpu.py builds this stand-alone program with -fsanitize=address,undefined from the product's own
// perspective_math.hpp (no HIP, no library) and runs it on a file of the CPU test's cases: it prints an FNV-1a hash per
// group of results, which the test compares with the hashes of what libocrs_amd.so returns for the same cases.  After the
// file it drives the same functions over hostile inputs (NaN, infinities, huge values, zero-area quads, peaks of random
// bits) whose results are not compared: any sanitizer report fails the test.
//
// File: u32 n_choose, then per case { u32 A; i32 wh, ww, ph, pw; f64 max_deg, step_deg, min_cover, min_span, min_area;
// i32 work_max_side, min_step; i32 table[2 A]; u64 peaks[64 A] }; u32 n_quads, f32 quads[8 n]; u32 n_maps, f32 maps[8 n];
// u32 n_rects, f32 rects[6 n]; u32 n_boxes, i32 boxes[4 n].  Every map is applied to every rect and every box.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../ocrs_amd/csrc/perspective_math.hpp"

using namespace ocrs::persp;

namespace {

struct Fnv {
    uint64_t h = 14695981039346656037ull;
    void add(const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    }
};

template <class T>
bool take(FILE* f, T* out, size_t n) { return n == 0 || fread(out, sizeof(T), n, f) == n; }

void hash_outline(Fnv& h, const Outline& o) {
    h.add(&o.found, 4);
    h.add(&o.polarity, 4);
    h.add(o.corners, sizeof o.corners);
    h.add(o.counts, sizeof o.counts);
    h.add(o.angles, sizeof o.angles);
}

void hash_quad(Fnv& h, const float* q) {
    int hw[2] = {0, 0};
    float m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int32_t ok = quad_map(q, hw, m) ? 1 : 0;
    if (!ok) {
        hw[0] = hw[1] = 0;
        memset(m, 0, sizeof m);
    }
    h.add(&ok, 4);
    h.add(hw, sizeof hw);
    h.add(m, sizeof m);
}

int from_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    uint32_t n = 0;
    Fnv hc, hq, hr, hb;
    if (!take(f, &n, 1)) return 3;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t A = 0;
        int32_t dims[4], ints[2];
        double dbl[5];
        if (!take(f, &A, 1) || !take(f, dims, 4) || !take(f, dbl, 5) || !take(f, ints, 2) || A < 1 || A > 4096) return 3;
        std::vector<int32_t> table(2 * (size_t)A);
        std::vector<uint64_t> peaks(64 * (size_t)A);
        if (!take(f, table.data(), table.size()) || !take(f, peaks.data(), peaks.size())) return 3;
        const Params p = {dbl[0], dbl[1], dbl[2], dbl[3], dbl[4], ints[0], ints[1]};
        hash_outline(hc, choose(peaks.data(), table.data(), A, dims[0], dims[1], dims[2], dims[3], p));
    }
    if (!take(f, &n, 1)) return 3;
    std::vector<float> quads(8 * (size_t)n);
    if (!take(f, quads.data(), quads.size())) return 3;
    for (uint32_t i = 0; i < n; i++) hash_quad(hq, quads.data() + 8 * (size_t)i);
    uint32_t nm = 0, nr = 0, nb = 0;
    if (!take(f, &nm, 1)) return 3;
    std::vector<float> maps(8 * (size_t)nm);
    if (!take(f, maps.data(), maps.size()) || !take(f, &nr, 1)) return 3;
    std::vector<float> rects(6 * (size_t)nr);
    if (!take(f, rects.data(), rects.size()) || !take(f, &nb, 1)) return 3;
    std::vector<int32_t> boxes(4 * (size_t)nb);
    if (!take(f, boxes.data(), boxes.size())) return 3;
    fclose(f);
    for (uint32_t k = 0; k < nm; k++) {
        std::vector<float> r = rects;
        for (uint32_t i = 0; i < nr; i++) unproject_rect(r.data() + 6 * (size_t)i, maps.data() + 8 * (size_t)k);
        hr.add(r.data(), r.size() * sizeof(float));
        std::vector<int32_t> b = boxes;
        for (uint32_t i = 0; i < nb; i++) unproject_box(b.data() + 4 * (size_t)i, maps.data() + 8 * (size_t)k);
        hb.add(b.data(), b.size() * sizeof(int32_t));
    }
    printf("choose: %016llx\nquad: %016llx\nrects: %016llx\nboxes: %016llx\n", (unsigned long long)hc.h, (unsigned long long)hq.h,
           (unsigned long long)hr.h, (unsigned long long)hb.h);
    return 0;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 2685821237522263789ull;
}

float hostile_float(uint64_t r) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float pool[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, 3e38f, -3e38f, 1e-38f, 1e-45f, inf, -inf, nan, 65535.0f, 100.0f, 1e20f, -1e20f};
    if ((r & 3) == 0) {   // any bit pattern
        const uint32_t bits = (uint32_t)(r >> 16);
        float v;
        memcpy(&v, &bits, 4);
        return v;
    }
    return pool[(r >> 8) % (sizeof pool / sizeof pool[0])];
}

void hostile() {
    unsigned long long seen = 0;
    // quads and maps of hostile floats; zero-area quads (all corners equal, three in a row, a bow tie)
    const float flat_quads[][8] = {{5, 5, 5, 5, 5, 5, 5, 5}, {0, 0, 10, 0, 20, 0, 30, 0}, {0, 0, 10, 10, 10, 0, 0, 10}, {0, 0, 0, 0, 10, 10, 10, 10},
                                   {3e38f, 3e38f, -3e38f, 3e38f, -3e38f, -3e38f, 3e38f, -3e38f}};
    for (const auto& q : flat_quads) {
        int hw[2];
        float m[8];
        seen += quad_map(q, hw, m) ? 1 : 0;
    }
    for (int it = 0; it < 20000; it++) {
        float q[8], m[8], rect[6];
        int32_t box[4];
        for (float& v : q) v = hostile_float(rnd());
        for (float& v : m) v = hostile_float(rnd());
        for (float& v : rect) v = hostile_float(rnd());
        for (int32_t& v : box) v = (rnd() & 1) ? (int32_t)rnd() : (int32_t)(rnd() % 5000) - 100;
        int hw[2];
        float mm[8];
        if (quad_map(q, hw, mm)) {
            seen++;
            unproject_rect(rect, mm);
            unproject_box(box, mm);
        }
        bool finite = true;
        for (float v : m) finite = finite && std::isfinite(v);
        if (finite) {   // what the library lets through
            unproject_rect(rect, m);
            unproject_box(box, m);
        }
        seen += (unsigned long long)(box[0] & 1);
    }
    // peaks of random bits, of saturated counts, of bins far outside the page; tables at the limits; tiny and huge pages
    const int sizes[][4] = {{1, 1, 1, 1}, {400, 480, 400, 480}, {4096, 4096, 65535, 65535}, {3, 4096, 1, 65535}, {512, 384, 3000, 2200}};
    for (int it = 0; it < 300; it++) {
        const size_t A = 1 + (size_t)(rnd() % 9);
        std::vector<int32_t> table(2 * A);
        for (int32_t& v : table) v = (rnd() & 3) == 0 ? ((rnd() & 1) ? 65536 : -65536) : (int32_t)(rnd() % 131073) - 65536;
        if (it % 7 == 0) table[1] = 0;   // a cosine of zero: positions that are not finite are dropped
        std::vector<uint64_t> peaks(64 * A);
        for (uint64_t& e : peaks) {
            const uint64_t r = rnd();
            e = (r & 7) == 0 ? 0 : (r & 7) == 1 ? ~0ull : (r & 7) == 2 ? r : ((r >> 8) % 5000) << 32 | (0xFFFFFFFFull - ((r >> 40) % 9000));
        }
        const int* s = sizes[it % 5];
        Params p = default_params();
        if (it % 3 == 1) p.min_cover = 1e-9, p.min_span = 1e-9, p.min_area = 0.0;
        if (it % 3 == 2) p.min_cover = std::numeric_limits<double>::quiet_NaN();
        seen += (unsigned long long)choose(peaks.data(), table.data(), A, s[0], s[1], s[2], s[3], p).found;
    }
    Params bad = default_params();
    bad.step_deg = 0.0;
    seen += (unsigned long long)plan(bad);
    bad.step_deg = std::numeric_limits<double>::quiet_NaN();
    seen += (unsigned long long)plan(bad);
    bad.step_deg = 1e-300;
    seen += (unsigned long long)plan(bad);
    printf("hostile: ok %llu\n", seen);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1) {
        const int r = from_file(argv[1]);
        if (r != 0) {
            fprintf(stderr, "perspective_harness: cannot read %s (%d)\n", argv[1], r);
            return r;
        }
    }
    hostile();
    return 0;
}
