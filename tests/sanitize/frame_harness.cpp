// Memory-safety evidence for the host half of page framing.  TEST INFRASTRUCTURE.
// tests/test_frame_cpu.py builds this stand-alone program with -fsanitize=address,undefined from the product's own
// frame_choose.hpp (no HIP, no library) and runs it on a file of the CPU test's cases: it prints the choice of every case,
// which the test compares with tests/frame_ref.py.  After the file it drives the same function over profiles of extreme
// counts and sizes whose results are not compared: any sanitizer report fails the test.
//
// File: u32 n, then per case { i32 h, w, min_count, pad, gutter_min_width, gutter_max_ink; u32 cols[w]; u32 rows[h] }.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../ocrs_amd/csrc/frame_choose.hpp"

using ocrs::frame::Choice;
using ocrs::frame::ChoiceParams;

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: frame_harness cases.bin\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t n = 0;
    if (!read_all(f, &n, sizeof n)) return 2;
    for (uint32_t i = 0; i < n; i++) {
        int32_t head[6];
        if (!read_all(f, head, sizeof head) || head[0] < 1 || head[1] < 1) return 2;
        std::vector<uint32_t> cols((size_t)head[1]), rows((size_t)head[0]);   // exact sizes: a read past either is reported
        if (!read_all(f, cols.data(), cols.size() * 4) || !read_all(f, rows.data(), rows.size() * 4)) return 2;
        const ChoiceParams p = {head[2], head[3], head[4], head[5]};
        if (!ocrs::frame::choice_params_ok(p)) {
            printf("refused\n");
            continue;
        }
        const Choice c = ocrs::frame::choose(head[0], head[1], cols.data(), rows.data(), p);
        printf("%d %d %d %d %d %d\n", c.found, c.x0, c.y0, c.x1, c.y1, c.gutter_x);
    }
    fclose(f);
    // extremes: the largest page, the largest counts and parameters, one-pixel pages
    uint64_t sink = 0;
    const int sizes[] = {1, 2, 3, 7, 8, 9, 64, 65535};
    const uint32_t levels[] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    const ChoiceParams params[] = {{1, 0, 1, 0}, {1, 65535, 1, 0x7FFFFFFF}, {0x7FFFFFFF, 16, 0x7FFFFFFF, 0}, {1, 16, 8, 0}};
    for (int h : sizes)
        for (int w : sizes)
            for (uint32_t lv : levels)
                for (const ChoiceParams& p : params) {
                    std::vector<uint32_t> cols((size_t)w, lv), rows((size_t)h, lv);
                    for (int variant = 0; variant < 3; variant++) {
                        if (variant == 1) cols[(size_t)w / 2] = 0u;                   // a one-column gutter
                        if (variant == 2) cols[0] = cols[(size_t)w - 1] = 0xFFFFFFFFu;   // content at both ends
                        const Choice c = ocrs::frame::choose(h, w, cols.data(), rows.data(), p);
                        sink += (uint64_t)(uint32_t)c.found + (uint32_t)c.x0 + (uint32_t)c.y0 + (uint32_t)c.x1 + (uint32_t)c.y1 + (uint32_t)c.gutter_x;
                    }
                }
    printf("extremes %llu\n", (unsigned long long)sink);
    return 0;
}
