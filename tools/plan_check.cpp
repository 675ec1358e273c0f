// plan_check: CPU check of the forward path's launch plan (hdr2yuv_amd/csrc/h2y_plan.h), the header the shim compiles.
//   plan_check          checks the plan's properties over grids of configurations; prints "... 0 bad" when all hold
//   plan_check --plans  prints the complete plans of the pinned configurations, one JSON object per line, which
//                       tests/test_walk.py compares value for value with tests/golden/forward_plan.json
// Build: g++ -O2 -std=c++17 -I hdr2yuv_amd/csrc tools/plan_check.cpp -o plan_check
#include <cmath>
#include <cstdio>
#include <cstring>

#include "h2y_plan.h"

using namespace h2y;

static long n_bad = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (n_bad++ < 20) {                            \
                printf("BAD %s: ", #cond);                 \
                printf(__VA_ARGS__);                       \
                printf("\n");                              \
            }                                              \
        }                                                  \
    } while (0)

// the speeds a plan may be cut by: uniform, alternating, measured-looking, and fixed-mode masks with a ratio up to 100
static const double kSpeeds[6][8] = {{1, 1, 1, 1, 1, 1, 1, 1},         {1.25, .75, 1.25, .75, 1.25, .75, 1.25, .75}, {1.2, 1, 1.2, 1, 1.2, 1, 1.2, 1},
                                     {100, 1, 1, 1, 1, 1, 1, 1},       {1, 1, 1, 1, 100, 100, 100, 100},             {.75, .75, .75, .75, 1.25, 1.25, 1.25, .75}};

// per-block speeds in [0.75, 1.25], the same for a given grid
static std::vector<double> block_speeds_for(int grid)
{
    std::vector<double> s((size_t)grid);
    uint32_t x = 12345u + (uint32_t)grid;
    for (double &v : s) {
        x = x * 1664525u + 1013904223u;
        v = 0.75 + 0.5 * (double)(x >> 8) / (double)(1u << 24);
    }
    return s;
}

static loop_shape shape_of(int tiles_w, int tiles_h, int threads, int bpc, bool grouped, int cu, int og, bool scratch)
{
    // a picture of tiles_w x tiles_h thread tiles: width 4 * tiles_w, height 2 * tiles_h
    return loop_shape{bpc, grouped, cu, og, scratch, make_geom(4 * tiles_w, 2 * tiles_h, threads)};
}

// ---- the launch split -----------------------------------------------------------------------------------------------------------
static long check_split()
{
    long n_cfg = 0;
    const int tile_dims[6][2] = {{4, 4}, {16, 32}, {64, 64}, {480, 540}, {960, 1080}, {1920, 2160}}; // 16 tiles ... an 8K frame's
    for (int n : {1, 2, 31, 32, 33, 127, 128, 129, 255, 256, 257, 330, 512, 1000, 1025})
        for (const auto &td : tile_dims)
            for (int threads : {256, 1024})
                for (int bpc : {1, 2, 4})
                    for (int cu : {8, 60, 256})
                        for (int og : {0, 1, 2, 4, 8, 16, 64})
                            for (int grouped = 0; grouped < 2; grouped++)
                                for (int scratch = 0; scratch < 2; scratch++) {
                                    const loop_shape s = shape_of(td[0], td[1], threads, bpc, grouped != 0, cu, og, scratch != 0);
                                    int covered = 0;
                                    launch_plan l;
                                    for (int f0 = 0; f0 < n; f0 += l.frames) {
                                        const bool ok = next_launch(s, n - f0, &l);
                                        CHECK(ok && l.frames / l.groups <= 128, "n %d tiles %u og %d: %d frames in %d groups", n, s.g.tiles, og, l.frames, l.groups);
                                        CHECK(l.frames >= 1 && l.frames <= n - f0, "n %d: launch of %d frames, %d left", n, l.frames, n - f0);
                                        if (l.frames < 1) break;
                                        CHECK(l.groups >= 1 && l.frames % l.groups == 0 && l.grid % l.groups == 0, "n %d: %d frames, grid %d, %d groups", n, l.frames, l.grid, l.groups);
                                        CHECK(!scratch || l.frames <= 32, "n %d: %d frames with scratch", n, l.frames);
                                        CHECK(l.grid >= 1 && (uint64_t)l.grid <= (uint64_t)cu * bpc, "grid %d", l.grid);
                                        CHECK(l.xcd_layout == (grouped && l.grid % (8 * l.groups) == 0), "xcd_layout");
                                        covered += l.frames; // in order: each launch starts where the last one ended
                                    }
                                    CHECK(covered == n, "n %d: %d frames covered", n, covered);
                                    n_cfg++;
                                }
    return n_cfg;
}

// ---- k_fir_fused: units and their rows ------------------------------------------------------------------------------------------
static long check_fir()
{
    long n_cfg = 0;
    std::vector<uint32_t> rows;
    for (const auto &sp : kSpeeds)
        for (int n : {1, 2, 3, 5, 16, 31, 32, 64, 128})
            for (int w : {8, 64, 240, 244, 256, 1920, 3840, 7680, 16384})
                for (int h : {2, 4, 16, 64, 126, 128, 130, 256, 1080, 2160, 4320, 16384})
                    for (int cu : {8, 64, 256})
                        for (int wg = 0; wg < 2; wg++) {
                            const fir_plan p = make_fir_plan(n, w, h, cu, 2);
                            const balance bal{wg ? 0 : 1, 0xFFu, 1.0};
                            const bool weigh = fir_weigh(p, bal, true);
                            CHECK(p.take, "opt_fir 2 always takes k_fir_fused");
                            CHECK(p.units == (uint64_t)n * p.strips * p.segments && p.segments >= 1 && p.strips >= 1, "units");
                            CHECK(p.grid >= 1 && p.grid <= cu && (uint64_t)p.grid * 16u >= (p.units < (uint64_t)cu * 16u ? p.units : (uint64_t)cu * 16u), "grid %d", p.grid);
                            CHECK(!weigh || (p.full && p.segments >= 2), "weighted rows on a grid that is not full");
                            double work[8], speed[8];
                            for (int x = 0; x < 8; x++) speed[x] = bal.speed(x, sp);
                            fir_unit_rows(p, n, weigh, speed, rows, work);
                            CHECK(rows.size() == p.units, "rows of %zu units, %llu planned", rows.size(), (unsigned long long)p.units);
                            double steps = 0.0;
                            bool ok = true;
                            for (uint32_t f = 0; f < (uint32_t)n && ok; f++)
                                for (uint32_t st = 0; st < p.strips && ok; st++) {
                                    uint32_t at = 0;
                                    for (uint32_t i = 0; i < p.segments; i++) {
                                        const uint32_t r = rows[(f * p.segments + i) * p.strips + st], j0 = r & 0xFFFFu, j1 = r >> 16;
                                        // a partition of [0, h2): contiguous, none empty (j1 fits 16 bits or j1 << 16 would have lost it)
                                        if (j0 != at || j1 <= j0 || j1 > p.h2 || p.h2 > 65535u) ok = false;
                                        steps += (double)(j1 - j0) + 3.0 + (j0 < 3u ? (double)j0 : 3.0);
                                        at = j1;
                                    }
                                    if (at != p.h2) ok = false;
                                }
                            CHECK(ok, "n %d %dx%d cu %d weigh %d: segments %u are no partition of %u rows", n, w, h, cu, (int)weigh, p.segments, p.h2);
                            double sum = 0.0;
                            for (int x = 0; x < 8; x++) sum += work[x] * (double)((uint32_t)p.grid * 16u / 8u);
                            CHECK(std::fabs(sum - steps) <= 1e-9 * steps, "n %d %dx%d cu %d: per-XCD work %.17g, the rows say %.17g", n, w, h, cu, sum, steps);
                            n_cfg++;
                        }
    // auto keeps batches that cannot half fill the chip on the two-pass form; two-pass and fused are the option's to force
    CHECK(!make_fir_plan(1, 256, 64, 256, 0).take && make_fir_plan(1, 256, 64, 256, 2).take, "take");
    CHECK(make_fir_plan(64, 3840, 2160, 256, 0).take, "take");
    const fir_plan full = make_fir_plan(64, 3840, 2160, 256, 0);
    CHECK(full.full && !fir_weigh(full, balance{0, 0xFFu, 1.0}, false) && fir_weigh(full, balance{0, 0xFFu, 1.0}, true) &&
              !fir_weigh(full, balance{1, 0xFFu, 1.0}, true) && fir_weigh(full, balance{2, 0x55u, 1.2}, false), "fir_weigh");
    return n_cfg;
}

// ---- slice ranges of a loop-form launch -----------------------------------------------------------------------------------------
static long check_slices()
{
    long n_cfg = 0;
    const int tile_dims[6][2] = {{4, 4}, {16, 32}, {64, 64}, {480, 540}, {960, 1080}, {1920, 2160}};
    for (int n : {1, 2, 8, 32, 128, 330})
        for (const auto &td : tile_dims)
            for (int bpc : {1, 2, 4})
                for (int cu : {8, 60, 256})
                    for (int og : {0, 1, 2, 8}) {
                        const loop_shape s = shape_of(td[0], td[1], 1024, bpc, true, cu, og, false);
                        launch_plan l;
                        if (!next_launch(s, n, &l) || !l.xcd_layout) continue;
                        const uint32_t G = (uint32_t)l.grid / (uint32_t)l.groups, nslices = (s.g.tiles + 63u) / 64u;
                        const std::vector<double> bspeed = block_speeds_for(l.grid);
                        for (int kind = 0; kind < 7; kind++) // the six XCD speeds, then per block
                            for (int tail = 0; tail < 3; tail++)
                                for (int t1 = 0; t1 < 2; t1++) {
                                    const block_speeds bs{kind == 6, l.grid, l.groups, &bspeed};
                                    slice_plan sl;
                                    make_slice_plan(sl, l, s.g.tiles, kSpeeds[kind % 6], bs, t1 != 0, tail);
                                    const bool per_block = sl.range_stride != 0;
                                    CHECK(per_block == (kind == 6 && (size_t)l.groups * (G + 1u) <= kRangeWords), "per block");
                                    CHECK(sl.r.size() == (per_block ? (size_t)l.groups * (G + 1u) : (size_t)G + 1u) && sl.slices == nslices, "table size");
                                    for (uint32_t g = 0; g < (uint32_t)l.groups; g++) { // every group's table is a partition of the slices
                                        const uint32_t *r = sl.r.data() + (size_t)g * sl.range_stride;
                                        bool ok = r[0] == 0 && r[G] == nslices;
                                        double mean = 0.0;
                                        for (uint32_t i = 0; i < G; i++) {
                                            ok = ok && r[i] <= r[i + 1];
                                            mean += sl.bwork[walk_block_of(g, i, (uint32_t)l.groups)] / G;
                                        }
                                        CHECK(ok, "grid %d groups %d slices %u: group %u's table is no partition", l.grid, l.groups, nslices, g);
                                        CHECK(std::fabs(mean - 1.0) < 1e-9, "grid %d groups %d: bwork has mean %.17g over group %u", l.grid, l.groups, mean, g);
                                    }
                                    double wmean = 0.0;
                                    for (int x = 0; x < 8; x++) wmean += sl.work[x] / 8.0;
                                    CHECK(std::fabs(wmean - 1.0) < 1e-9, "work has mean %.17g", wmean);
                                    // a block's queue holds 64 chunks of H2Y_TAIL_CHUNK slices: the group's blocks must hold twice the frame and 96 chunks to spare
                                    const bool fits = ((uint64_t)nslices / H2Y_TAIL_CHUNK + 96u) * 2u <= 64ull * G && G >= 8u;
                                    CHECK(!sl.tail_on || fits, "tail_on with %u slices on %u blocks", nslices, G);
                                    CHECK(!sl.tail_on || (t1 && tail != 2 && l.groups <= 16 && l.frames / l.groups >= (tail == 1 ? 2 : kTailMinFrames)), "tail_on");
                                    n_cfg++;
                                }
                    }
    return n_cfg;
}

// ---- speeds from measured times -------------------------------------------------------------------------------------------------
static long check_speed_update()
{
    long n_cfg = 0;
    CHECK(1.0 - 0.35 == 0.65 && 1.0 - 0.5 == 0.5, "the blend weights' complements are the constants the shim had");
    for (int n : {8, 256})
        for (double weight : {0.5, 0.35})
            for (int kind = 0; kind < 6; kind++) {
                std::vector<double> work((size_t)n), state((size_t)n, 1.0), first, before;
                std::vector<float> time((size_t)n);
                for (int i = 0; i < n; i++) {
                    work[(size_t)i] = 1.0 + 0.01 * (i % 7);
                    time[(size_t)i] = (float)(work[(size_t)i] / kSpeeds[kind][i % 8] * 100.0);
                }
                CHECK(speed_update(state.data(), false, work.data(), time.data(), n, weight), "update");
                first = state;
                double mean = 0.0;
                for (int i = 0; i < n; i++) mean += work[(size_t)i] / (double)time[(size_t)i] / n;
                for (int i = 0; i < n; i++) { // the first sample is taken as it is
                    double v = work[(size_t)i] / (double)time[(size_t)i] / mean;
                    v = v < 0.75 ? 0.75 : v > 1.25 ? 1.25 : v;
                    CHECK(state[(size_t)i] == v && v >= 0.75 && v <= 1.25, "first sample %d: %.17g, %.17g expected", i, state[(size_t)i], v);
                }
                for (int i = 0; i < n; i++) time[(size_t)i] = (float)(work[(size_t)i] / kSpeeds[(kind + 1) % 6][i % 8] * 50.0);
                CHECK(speed_update(state.data(), true, work.data(), time.data(), n, weight), "update");
                mean = 0.0;
                for (int i = 0; i < n; i++) mean += work[(size_t)i] / (double)time[(size_t)i] / n;
                for (int i = 0; i < n; i++) { // later ones are blended with the given weight
                    double v = work[(size_t)i] / (double)time[(size_t)i] / mean;
                    v = v < 0.75 ? 0.75 : v > 1.25 ? 1.25 : v;
                    CHECK(state[(size_t)i] == (1.0 - weight) * first[(size_t)i] + weight * v, "blend %d", i);
                    CHECK(state[(size_t)i] >= 0.75 && state[(size_t)i] <= 1.25, "speed %d out of range: %.17g", i, state[(size_t)i]);
                }
                before = state; // a time or a work that is not positive leaves the state untouched
                for (float bad_t : {0.f, -1.f, NAN}) {
                    const float keep = time[(size_t)n - 1];
                    time[(size_t)n - 1] = bad_t;
                    CHECK(!speed_update(state.data(), true, work.data(), time.data(), n, weight) && state == before, "time %g updated the speeds", bad_t);
                    time[(size_t)n - 1] = keep;
                }
                work[(size_t)n / 2] = 0.0;
                CHECK(!speed_update(state.data(), true, work.data(), time.data(), n, weight) && state == before, "work 0 updated the speeds");
                n_cfg++;
            }
    return n_cfg;
}

// ---- the pinned plans (tests/golden/forward_plan.json) --------------------------------------------------------------------------
// balance kinds of a pinned configuration: 0 adaptive, nothing measured; 1 off; 2 fixed 0x55,1.2; 3 adaptive, XCD speeds measured;
// 4 adaptive, block speeds measured for the first launch's grid shape (loop form only)
static const double kMeasured[8] = {1.07, 0.93, 1.05, 0.95, 1.11, 0.89, 1.02, 0.98};

// ---- table begin
struct loop_cfg {
    const char *name;
    int n, width, height, threads, bpc, grouped, cu, og, scratch, cols, bal, t1, tail;
};
static const loop_cfg kLoopCfgs[] = {
    // the benchmark's shapes: 128 x 4K box (k_fused_t1), 8K half (k_fused_lut16, 8-column tiles), the two-pass FIR form
    {"c2_box_128x4k", 128, 3840, 2160, 1024, 1, 1, 256, 0, 0, 4, 0, 1, 2},
    {"c2_box_128x4k_measured", 128, 3840, 2160, 1024, 1, 1, 256, 0, 0, 4, 3, 1, 2},
    {"c2_box_128x4k_blocks", 128, 3840, 2160, 1024, 1, 1, 256, 0, 0, 4, 4, 1, 2},
    {"c2_box_128x4k_fixed", 128, 3840, 2160, 1024, 1, 1, 256, 0, 0, 4, 2, 1, 2},
    {"c2_box_128x4k_off", 128, 3840, 2160, 1024, 1, 1, 256, 0, 0, 4, 1, 1, 2},
    {"c2_box_64x4k_tail_auto", 64, 3840, 2160, 1024, 1, 1, 256, 0, 0, 4, 3, 1, 0},
    {"c2_box_64x4k_tail_on_groups8", 64, 3840, 2160, 1024, 1, 1, 256, 8, 0, 4, 0, 1, 1},
    {"c4_8k_half_16", 16, 7680, 4320, 1024, 1, 1, 256, 0, 0, 8, 0, 0, 2},
    {"c4_8k_half_16_blocks", 16, 7680, 4320, 1024, 1, 1, 256, 0, 0, 8, 4, 0, 2},
    {"fir_twopass_64x4k", 64, 3840, 2160, 1024, 1, 1, 256, 0, 1, 4, 0, 1, 2},
    {"fir_twopass_16x4k_measured", 16, 3840, 2160, 1024, 1, 1, 256, 0, 1, 4, 3, 1, 2},
    {"fir_twopass_33x1080p", 33, 1920, 1080, 1024, 2, 1, 256, 0, 1, 4, 0, 0, 2},
    // long batches of small pictures: the split into launches
    {"small_330_groups0", 330, 256, 64, 1024, 1, 1, 256, 0, 0, 4, 0, 1, 2},
    {"small_330_groups1", 330, 256, 64, 1024, 1, 1, 256, 1, 0, 4, 0, 1, 2},
    {"small_330_groups2", 330, 256, 64, 1024, 1, 1, 256, 2, 0, 4, 0, 1, 2},
    {"small_330_groups2_tail_on", 330, 256, 64, 1024, 1, 1, 256, 2, 0, 4, 3, 1, 1},
    {"small_8_512x128", 8, 512, 128, 1024, 1, 1, 256, 0, 0, 4, 0, 1, 2},
    {"small_8_512x128_groups2_tail_on", 8, 512, 128, 1024, 1, 1, 256, 2, 0, 4, 2, 1, 1},
    {"hd_1000", 1000, 1920, 1080, 1024, 1, 1, 256, 0, 0, 4, 3, 1, 0},
    {"hd_1025_groups16", 1025, 1920, 1080, 1024, 2, 1, 256, 16, 0, 4, 0, 0, 0},
    {"hd_257_groups64", 257, 1920, 1080, 256, 4, 1, 60, 64, 0, 4, 0, 0, 2},
    {"hd_129_not_grouped", 129, 1920, 1080, 256, 4, 0, 256, 0, 0, 4, 0, 0, 2},
    {"hd_512_blocks", 512, 1920, 1080, 1024, 1, 1, 256, 0, 0, 4, 4, 1, 1},
    {"tiny_1", 1, 16, 8, 1024, 1, 1, 256, 0, 0, 4, 0, 0, 2},
    {"narrow_2", 2, 250, 128, 256, 4, 0, 256, 0, 0, 4, 0, 0, 2},
    {"cu8_255x4k", 255, 3840, 2160, 1024, 1, 1, 8, 0, 0, 4, 3, 1, 1},
    {"cu60_256x1080p_fixed", 256, 1920, 1080, 1024, 2, 1, 60, 0, 0, 4, 2, 1, 0},
    {"cu64_31x4k_groups4", 31, 3840, 2160, 1024, 1, 1, 64, 4, 0, 4, 3, 1, 0},
};
struct fir_cfg {
    const char *name;
    int n, width, height, cu, opt_fir, bal, clocks;
};
static const fir_cfg kFirCfgs[] = {
    // the benchmark's shapes: 64 and 16 x 4K FIR
    {"fir_64x4k", 64, 3840, 2160, 256, 0, 0, 1},
    {"fir_64x4k_measured", 64, 3840, 2160, 256, 0, 3, 1},
    {"fir_64x4k_fixed", 64, 3840, 2160, 256, 0, 2, 0},
    {"fir_64x4k_off", 64, 3840, 2160, 256, 0, 1, 1},
    {"fir_16x4k", 16, 3840, 2160, 256, 0, 0, 1},
    {"fir_16x4k_measured", 16, 3840, 2160, 256, 0, 3, 1},
    {"fir_1x4k_auto", 1, 3840, 2160, 256, 0, 3, 1},
    {"fir_1x4k_fused", 1, 3840, 2160, 256, 2, 3, 1},
    {"fir_8x8k_measured", 8, 7680, 4320, 256, 0, 3, 0},
    {"fir_5x1080p_fixed", 5, 1920, 1080, 256, 0, 2, 1},
    {"fir_64x1080p_measured", 64, 1920, 1080, 256, 0, 3, 1},
    {"fir_8_512x128_fused", 8, 512, 128, 256, 2, 0, 1},
    {"fir_8_512x128_fused_fixed", 8, 512, 128, 256, 2, 2, 1},
    {"fir_8_256x64_auto", 8, 256, 64, 256, 0, 0, 1},
    {"fir_128_244x130_measured", 128, 244, 130, 64, 0, 3, 1},
    {"fir_31_240x126_cu8", 31, 240, 126, 8, 0, 3, 1},
    {"fir_2_16384x16384_cu64", 2, 16384, 16384, 64, 0, 3, 1},
    {"fir_128_256x128_fixed", 128, 256, 128, 256, 0, 2, 0},
    {"fir_16_8x2_fused", 16, 8, 2, 8, 2, 3, 1},
    {"fir_64_3840x256_cu64", 64, 3840, 256, 64, 0, 3, 0},
    {"fir_2_7680x4320_fused", 2, 7680, 4320, 256, 2, 2, 1},
    {"fir_32_1920x1080_cu64_measured", 32, 1920, 1080, 64, 0, 3, 1},
};

static uint32_t fnv(const void *p, size_t bytes)
{
    uint32_t hsh = 2166136261u;
    for (size_t i = 0; i < bytes; i++) hsh = (hsh ^ static_cast<const unsigned char *>(p)[i]) * 16777619u;
    return hsh;
}
static void print_u32s(const char *key, const uint32_t *v, size_t n)
{
    printf("\"%s\": [", key);
    for (size_t i = 0; i < n; i++) printf("%s%u", i ? ", " : "", v[i]);
    printf("]");
}
static void print_f64s(const char *key, const double *v, size_t n)
{
    printf("\"%s\": [", key);
    for (size_t i = 0; i < n; i++) printf("%s%.17g", i ? ", " : "", v[i]);
    printf("]");
}
static void print_loop_cfg(const loop_cfg &c)
{
    printf("{\"name\": \"%s\", \"kind\": \"loop\", \"cfg\": [%d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d], ", c.name, c.n, c.width, c.height, c.threads, c.bpc, c.grouped,
           c.cu, c.og, c.scratch, c.cols, c.bal, c.t1, c.tail);
}
static void print_fir_cfg(const fir_cfg &c)
{
    printf("{\"name\": \"%s\", \"kind\": \"fir\", \"cfg\": [%d, %d, %d, %d, %d, %d, %d], ", c.name, c.n, c.width, c.height, c.cu, c.opt_fir, c.bal, c.clocks);
}
// one launch of a loop-form plan; r empty: no slice ranges (no XCD layout, or balance off)
static void print_launch(bool first, int frames, int grid, int groups, bool xcd_layout, const std::vector<uint32_t> &r, uint32_t range_stride, bool tail_on,
                         const double work[8], const std::vector<double> &bwork)
{
    printf("%s{\"frames\": %d, \"grid\": %d, \"groups\": %d, \"xcd_layout\": %d, \"range_stride\": %u, \"tail_on\": %d, ", first ? "" : ", ", frames, grid, groups,
           xcd_layout ? 1 : 0, range_stride, tail_on ? 1 : 0);
    print_u32s("ranges", r.data(), r.size());
    printf(", ");
    print_f64s("work", work, 8);
    printf(", \"bwork_n\": %zu, \"bwork_fnv\": %u}", bwork.size(), fnv(bwork.data(), bwork.size() * sizeof(double)));
}
static void print_fir(uint32_t strips, uint32_t want, uint32_t segments, uint32_t seg_rows, uint64_t units, uint32_t gw, bool take, int grid, bool full, uint32_t mix_xcds,
                      bool weigh, const std::vector<uint32_t> &rows, const double work[8], int n)
{
    printf("\"strips\": %u, \"want\": %u, \"segments\": %u, \"seg_rows\": %u, \"units\": %llu, \"gw\": %u, \"take\": %d, \"grid\": %d, \"full\": %d, \"mix_xcds\": %u, \"weigh\": %d, ",
           strips, want, segments, seg_rows, (unsigned long long)units, gw, take ? 1 : 0, grid, full ? 1 : 0, mix_xcds, weigh ? 1 : 0);
    std::vector<uint32_t> first_strip, last_strip; // frame 0 strip 0, and the last frame's last strip: their segments' rows in full
    if (!rows.empty())
        for (uint32_t i = 0; i < segments; i++) {
            first_strip.push_back(rows[(size_t)i * strips]);
            last_strip.push_back(rows[((size_t)(n - 1) * segments + i) * strips + strips - 1u]);
        }
    printf("\"rows_n\": %zu, \"rows_fnv\": %u, ", rows.size(), fnv(rows.data(), rows.size() * sizeof(uint32_t)));
    print_u32s("first_strip", first_strip.data(), first_strip.size());
    printf(", ");
    print_u32s("last_strip", last_strip.data(), last_strip.size());
    printf(", ");
    print_f64s("work", work, 8);
    printf("}\n");
}
// ---- table end

static void plan_loop(const loop_cfg &c)
{
    print_loop_cfg(c);
    printf("\"launches\": [");
    const loop_shape s{c.bpc, c.grouped != 0, c.cu, c.og, c.scratch != 0, make_geom(c.width, c.height, c.threads, c.cols)};
    const balance bal{c.bal == 1 ? 1 : c.bal == 2 ? 2 : 0, 0x55u, 1.2};
    std::vector<double> bspeed;
    int bgrid = 0, bgroups = 0;
    launch_plan l;
    for (int f0 = 0; f0 < c.n; f0 += l.frames) {
        if (!next_launch(s, c.n - f0, &l)) {
            printf("\"per-group bound\"");
            break;
        }
        if (c.bal == 4 && f0 == 0) bgrid = l.grid, bgroups = l.groups, bspeed = block_speeds_for(l.grid);
        slice_plan sl;
        for (int x = 0; x < 8; x++) sl.work[x] = 1;
        if (l.xcd_layout && bal.mode != 1) {
            double sp[8];
            for (int x = 0; x < 8; x++) sp[x] = bal.speed(x, c.bal >= 3 ? kMeasured : nullptr);
            const block_speeds bs{c.bal == 4, bgrid, bgroups, &bspeed};
            make_slice_plan(sl, l, s.g.tiles, sp, bs, c.t1 != 0, c.tail);
        }
        print_launch(f0 == 0, l.frames, l.grid, l.groups, l.xcd_layout, sl.r, sl.range_stride, sl.tail_on, sl.work, sl.bwork);
    }
    printf("]}\n");
}

static void plan_fir(const fir_cfg &c)
{
    print_fir_cfg(c);
    const fir_plan p = make_fir_plan(c.n, c.width, c.height, c.cu, c.opt_fir);
    const balance bal{c.bal == 1 ? 1 : c.bal == 2 ? 2 : 0, 0x55u, 1.2};
    const bool weigh = fir_weigh(p, bal, c.bal == 3), clocks = p.full && c.clocks;
    std::vector<uint32_t> rows;
    double work[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (p.take && (weigh || clocks)) {
        double sp[8];
        const double ones[8] = {1, 1, 1, 1, 1, 1, 1, 1};
        for (int x = 0; x < 8; x++) sp[x] = bal.speed(x, c.bal == 3 ? kMeasured : ones);
        fir_unit_rows(p, c.n, weigh, sp, rows, work);
    }
    print_fir(p.strips, p.want, p.segments, p.seg_rows, p.units, p.gw, p.take, p.grid, p.full, p.mix_xcds, weigh, rows, work, c.n);
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--plans")) {
        for (const loop_cfg &c : kLoopCfgs) plan_loop(c);
        for (const fir_cfg &c : kFirCfgs) plan_fir(c);
        return 0;
    }
    const long n_split = check_split(), n_fir = check_fir(), n_slices = check_slices(), n_speed = check_speed_update();
    printf("%ld launch splits, %ld k_fir_fused plans, %ld slice plans, %ld speed updates: %ld bad\n", n_split, n_fir, n_slices, n_speed, n_bad);
    return n_bad ? 1 : 0;
}
