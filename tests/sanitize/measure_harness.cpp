// Memory-safety evidence for the host half of page measurement.  TEST INFRASTRUCTURE.
// tests/test_measure_cpu.py builds this stand-alone program with -fsanitize=address,undefined from the product's own
// measure_choose.hpp (no HIP, no library) and runs it on a file of the CPU test's cases: it prints the choice and the work
// scale of every case, which the test compares with tests/measure_ref.py.  After the file it drives the same functions over
// records of extreme counts whose results are not compared: any sanitizer report fails the test.
//
// File: u32 n, then per case { f64 min_height_strokes, target_height, min_scale, max_scale; the 6160 bytes of an info record }.
#include <cstdint>
#include <cstdio>
#include <memory>

#include "../../ocrs_amd/csrc/measure_choose.hpp"

using ocrs::measure::ChoiceParams;
using ocrs::measure::Info;
using ocrs::measure::TextScale;

static_assert(sizeof(Info) == 6160, "the record of include/ocrs_amd.h");

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: measure_harness cases.bin\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t n = 0;
    if (!read_all(f, &n, sizeof n)) return 2;
    for (uint32_t i = 0; i < n; i++) {
        double head[4];
        std::unique_ptr<Info> info(new Info);   // its exact size on the heap: a read past it is reported
        if (!read_all(f, head, sizeof head) || !read_all(f, info.get(), sizeof(Info))) return 2;
        const ChoiceParams p = {head[0]};
        if (!ocrs::measure::choice_params_ok(p)) {
            printf("refused\n");
            continue;
        }
        const TextScale t = ocrs::measure::choose(*info, p);
        printf("%d %d %u %d ", t.stroke, t.text_height, t.support, t.blank);
        if (ocrs::measure::work_scale_args_ok(head[1], head[2], head[3]))
            printf("%a\n", ocrs::measure::work_scale_for_text(t.text_height, head[1], head[2], head[3]));
        else
            printf("refused\n");
    }
    fclose(f);
    // extremes: every bin at the largest counts, single bins, the largest and smallest parameters
    uint64_t sink = 0;
    const uint32_t levels[] = {0u, 1u, 0x7FFFFFFFu, 0xFFFFFFFFu};
    const uint64_t areas[] = {0ull, 1ull, 0x7FFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFFull};
    const double strokes[] = {0.0, 0.001953125, 0.5, 1.5, 255.0};
    std::unique_ptr<Info> info(new Info);
    for (uint32_t lv : levels)
        for (uint64_t ar : areas)
            for (int only = -1; only < ocrs::measure::BINS; only += 51)
                for (double m : strokes) {
                    info->ink = ar;
                    info->components = info->counted = lv;
                    for (int b = 0; b < ocrs::measure::BINS; b++) {
                        const bool on = only < 0 || b == only;
                        info->run_h[b] = info->run_v[b] = info->comp_h[b] = info->comp_w[b] = on ? lv : 0u;
                        info->area_by_h[b] = on ? ar : 0ull;
                    }
                    const TextScale t = ocrs::measure::choose(*info, {m});
                    sink += (uint64_t)(uint32_t)t.stroke + (uint32_t)t.text_height + t.support + (uint32_t)t.blank;
                    sink += (uint64_t)(1000.0 * ocrs::measure::work_scale_for_text(t.text_height, 1e300, 1e-300, 4.0));   // at most 4000
                }
    printf("extremes %llu\n", (unsigned long long)sink);
    return 0;
}
