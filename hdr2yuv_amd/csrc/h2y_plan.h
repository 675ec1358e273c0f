/* h2y_plan.h -- the forward path's launch plan: how a batch is cut into launches, a launch into frame groups, a k_fir_fused
 * launch into units and their rows, a loop-form launch into slice ranges, and how measured times become the speeds the next
 * plan is cut by.  Host only and pure arithmetic: what the kernels and the card contribute comes in as plain numbers, so
 * tools/plan_check.cpp (run by tests/test_walk.py) checks every rule on the CPU and pins the plans of
 * tests/golden/forward_plan.json.  h2y_forward.hip turns a plan into stream operations. */
#ifndef H2Y_PLAN_H
#define H2Y_PLAN_H
#include <cstddef>
#include <cstdint>
#include <vector>

#include "h2y_math.h"
#include "h2y_walk.h"

namespace h2y {

/* one launch covers at most kMaxFramesPerLaunch frames: k_fused_t1's waves draw their tiles from one LDS counter per frame of
 * their group (H2Y_CLAIM_FRAMES of them); with frame groups the bound is per GROUP: a launch of g groups takes up to g x 128 */
constexpr int kMaxFramesPerLaunch = 128;
constexpr int kFirSubBatch = 32; /* frames per fused launch on the FIR path: every launch pays its table staging and its last redo pass */
constexpr int kTailMinFrames = 8; /* frames per group from which its last one is drawn dynamically (h2y_walk.h): the plain loop that takes it is
                                     slower than the prefetching one, and a frame is 1/8 of the group's work at most */
constexpr size_t kRangeWords = 1025; /* a table of slice ranges: up to 1024 blocks of a group + 1 */

struct geom {
    bool narrow;
    uint32_t wq, wq_magic, tiles, chunks;
};
inline geom make_geom(int width, int height, int threads, int cols = 4 /* columns of a thread tile (8: k_fused_lut16 on wide-aligned pictures) */)
{
    geom g;
    g.narrow = (width % 4) != 0;
    g.wq = g.narrow ? (uint32_t)width : (uint32_t)width / (uint32_t)cols;
    g.wq_magic = (uint32_t)(0x100000000ull / g.wq);
    if (g.wq == 1) g.wq_magic = 0xFFFFFFFFu;
    g.tiles = g.wq * (uint32_t)((height + 1) / 2);
    g.chunks = (g.tiles + threads - 1) / threads;
    return g;
}

/* Frame groups of a launch (frame_walk in h2y_walk.h), unless the caller set a number: as few as leave every block
 * kMinSlicesPerBlock 64-tile slices of a frame -- a 4K frame on 256 blocks: two groups, 1080p: eight, 8K: one.  Few, because
 * with g groups g frames are read and written at equal offsets at any moment, and whether those streams meet in the same DRAM
 * banks depends on where the frames happen to lie: eight groups ran the same 64 x 4K launch in 1.42 ... 1.72 ms from one set of
 * buffers to the next, two in 1.42 ... 1.51, one in 1.44 ... 1.49 (tools/layoutbench.py).  Not fewer, because a block pays for
 * every frame it visits (its waves' tickets, statistics records, the run-in of its prefetch): 1080p at one group runs at 0.47 of
 * the bandwidth it reaches at eight (0.61). */
constexpr int kMinSlicesPerBlock = 100;
inline int groups_cap(int opt_groups, uint32_t tiles_per_frame, int grid)
{
    if (opt_groups) return opt_groups;
    const uint64_t slices = (tiles_per_frame + 63u) / 64u;
    int ng = 1;
    while (ng < 8 && slices * (uint64_t)ng < (uint64_t)kMinSlicesPerBlock * (uint64_t)grid) ng *= 2;
    return ng;
}

/* what a loop-form kernel, the card and the batch contribute to the launch split */
struct loop_shape {
    int blocks_per_cu; /* of the kernel (its threads per block are in g.chunks) */
    bool grouped;      /* the kernel honours fused_args.groups */
    int n_cu;
    int opt_groups;    /* the "groups" option */
    bool scratch;      /* a second pass reads what the launch leaves in scratch: kFirSubBatch frames at most */
    geom g;
};

/* persistent grid: exactly the blocks the chip holds at once */
inline int grid_for(int n_cu, int blocks_per_cu, uint64_t total_chunks)
{
    uint64_t g = (uint64_t)n_cu * blocks_per_cu;
    if (g > total_chunks) g = total_chunks;
    if (g < 1) g = 1;
    return (int)g;
}

/* the frames of the next launch, `left` of the batch still to go */
inline int launch_frames(const loop_shape &s, int left)
{
    if (s.scratch) return left < kFirSubBatch ? left : kFirSubBatch;
    if (left <= kMaxFramesPerLaunch || !s.grouped) return left < kMaxFramesPerLaunch ? left : kMaxFramesPerLaunch;
    const int gridf = grid_for(s.n_cu, s.blocks_per_cu, (uint64_t)s.g.chunks * left);
    for (int ng = groups_cap(s.opt_groups, s.g.tiles, gridf); ng > 1; ng >>= 1)
        if (gridf % ng == 0) {
            int cand = left < kMaxFramesPerLaunch * ng ? left : kMaxFramesPerLaunch * ng;
            cand -= cand % ng; /* whole groups; what is left over goes into the next launch */
            return cand > kMaxFramesPerLaunch ? cand : kMaxFramesPerLaunch;
        }
    return kMaxFramesPerLaunch;
}

struct launch_plan {
    int frames, grid;
    int groups;      /* as many as divide both the launch's frames and the grid, up to groups_cap() */
    bool xcd_layout; /* XCD-aware rounds (h2y_walk.h) */
};
/* the next launch of a batch; false: its frames per group exceed kMaxFramesPerLaunch (a bug in the rules above) */
inline bool next_launch(const loop_shape &s, int left, launch_plan *l)
{
    l->frames = launch_frames(s, left);
    l->grid = grid_for(s.n_cu, s.blocks_per_cu, (uint64_t)s.g.chunks * l->frames);
    l->groups = 1;
    if (s.grouped)
        for (int ng = groups_cap(s.opt_groups, s.g.tiles, l->grid); ng > 1; ng >>= 1)
            if (l->frames % ng == 0 && l->grid % ng == 0) {
                l->groups = ng;
                break;
            }
    l->xcd_layout = s.grouped && l->grid % (8 * l->groups) == 0;
    return l->frames / l->groups <= kMaxFramesPerLaunch;
}

/* The "balance" option and what has been measured: the speed of XCD x that a plan is cut by.  measured: null = nothing yet. */
struct balance {
    int mode; /* 0 adaptive, 1 off, 2 fixed */
    uint32_t mask;
    double rho;
    double speed(int x, const double *measured) const { return mode == 2 ? (((mask >> x) & 1u) ? rho : 1.0) : (measured ? measured[x] : 1.0); }
};

/* The FIR resampler in one pass (k_fir_fused): a wave's unit of work is (frame, segment of chroma rows, strip of 240 columns).
 * Segments: as few as give every wave of the chip a unit, never shorter than 64 rows (each cut costs six recomputed row
 * pairs).  "auto" (opt_fir 0) keeps short batches, which cannot fill the chip that way, on the two-pass form. */
struct fir_plan {
    uint32_t wq, h2;          /* width / 4, height / 2 */
    uint32_t strips, gw;      /* strips of a frame, waves the chip holds */
    uint32_t want, segments;  /* segments wanted and had */
    uint32_t seg_rows;        /* chroma rows of a segment in the even cut */
    uint64_t units;           /* n * strips * segments */
    int grid;
    bool full;                /* the grid fills the card in whole rounds of the XCDs: rows by XCD speed and block clocks apply */
    uint32_t mix_xcds;
    bool take;                /* k_fir_fused rather than the two-pass form */
};
inline fir_plan make_fir_plan(int n, int width, int height, int n_cu, int opt_fir)
{
    fir_plan p;
    p.wq = (uint32_t)width / 4u, p.h2 = (uint32_t)height / 2u;
    p.strips = (p.wq + H2Y_FF_OWN_LANES - 1u) / H2Y_FF_OWN_LANES, p.gw = (uint32_t)n_cu * 16u;
    const uint32_t max_seg = p.h2 / 64u > 0u ? p.h2 / 64u : 1u;
    p.want = (p.gw + (uint32_t)n * p.strips - 1u) / ((uint32_t)n * p.strips);
    if (p.want > max_seg) p.want = max_seg;
    if (p.want < 1u) p.want = 1u;
    p.seg_rows = (p.h2 + p.want - 1u) / p.want, p.segments = (p.h2 + p.seg_rows - 1u) / p.seg_rows;
    p.units = (uint64_t)n * p.strips * p.segments;
    p.take = opt_fir == 2 || 2u * p.units >= p.gw;
    const uint32_t blocks_needed = (uint32_t)((p.units + 15u) / 16u);
    p.grid = (int)(blocks_needed < (uint32_t)n_cu ? blocks_needed : (uint32_t)n_cu);
    p.full = p.grid == n_cu && p.grid % 8 == 0;
    p.mix_xcds = p.grid % 8 == 0 ? 1u : 0u;
    return p;
}
/* are the rows cut by XCD speed?  (have: k_fir_fused's speeds were measured) */
inline bool fir_weigh(const fir_plan &p, const balance &b, bool have) { return p.full && p.segments >= 2 && b.mode != 1 && (b.mode == 2 || have); }

/* Rows by XCD speed.  The XCDs of a card are not equally fast on k_fir_fused (measured: the odd ones finish 11 % later on
 * equal shares), a wave's units are fixed, and a launch ends with its slowest wave.  Strips are independent, so every
 * (frame, strip) column is cut into its segments in proportion to the speeds sp[] of the XCDs its units will run on (unit u ->
 * wave u % GW -> block / 16 -> XCD block % 8), lead-in steps included; !weigh: the even cut.  rows[u] = j0 | j1 << 16, the
 * chroma rows [j0, j1) of unit u; work[x] = steps per wave of XCD x. */
inline void fir_unit_rows(const fir_plan &p, int n, bool weigh, const double sp[8], std::vector<uint32_t> &rows, double work[8])
{
    const uint32_t ns = p.strips, nseg = p.segments, h2 = p.h2, seg_rows = p.seg_rows;
    const uint32_t gwaves = (uint32_t)p.grid * 16u;
    for (int x = 0; x < 8; x++) work[x] = 0;
    rows.resize((size_t)p.units);
    std::vector<int> xs;
    for (uint32_t f = 0; f < (uint32_t)n; f++)
        for (uint32_t st = 0; st < ns; st++) {
            double ssum = 0.0, csum = 0.0;
            xs.resize(nseg);
            for (uint32_t i = 0; i < nseg; i++) {
                const uint32_t u = (f * nseg + i) * ns + st;
                xs[i] = (int)(h2y_firf_vblock((u % gwaves) / 16u) % 8u); /* the block that works as virtual block (u % GW) / 16 */
                ssum += weigh ? sp[xs[i]] : 1.0;
                csum += i == 0 ? 3.0 : 6.0;
            }
            const double T = ((double)h2 + csum) / ssum;
            uint32_t j0 = 0;
            for (uint32_t i = 0; i < nseg; i++) {
                const uint32_t u = (f * nseg + i) * ns + st;
                uint32_t j1;
                if (!weigh) j1 = (i + 1u) * seg_rows < h2 ? (i + 1u) * seg_rows : h2;
                else if (i + 1u == nseg) j1 = h2;
                else {
                    double r = (weigh ? sp[xs[i]] : 1.0) * T - (i == 0 ? 3.0 : 6.0);
                    const uint32_t left = nseg - 1u - i; /* segments after this one: eight rows each at least */
                    if (r < 8.0) r = 8.0;
                    j1 = j0 + (uint32_t)(r + 0.5);
                    if (j1 + 8u * left > h2) j1 = h2 - 8u * left;
                    if (j1 <= j0) j1 = j0 + 1u;
                }
                rows[u] = j0 | (j1 << 16);
                work[xs[i]] += (double)(j1 - j0) + 3.0 + (j0 < 3u ? (double)j0 : 3.0);
                j0 = j1;
            }
        }
    for (int x = 0; x < 8; x++) work[x] /= (double)(gwaves / 8u); /* steps per wave of that XCD */
}

/* Slices by XCD speed, for a launch under the XCD layout: block i of a group takes one contiguous run of every frame's 64-tile
 * slices, as long as the measured speed of its XCD says (block i of a group runs on XCD i % 8) -- or, once this grid shape has
 * been measured in adaptive mode, as its own speed says. */
struct slice_plan {
    std::vector<uint32_t> r; /* per XCD: one table [G + 1] for every group (range_stride 0); per block: [groups][G + 1] */
    uint32_t range_stride = 0;
    uint32_t slices = 0;     /* 64-tile slices of a frame */
    bool tail_on = false;    /* the dynamic last frame (h2y_walk.h) */
    double work[8];          /* relative work a block of XCD x has */
    std::vector<double> bwork; /* relative work of every block of the grid */
};
/* what has been measured per block, and the grid shape it is for */
struct block_speeds {
    bool use; /* adaptive mode, by block */
    int grid, groups;
    const std::vector<double> *speed;
};
/* The dynamic last frame's condition.  A block holds 64 chunks of H2Y_TAIL_CHUNK slices at most (H2Y_TAIL_QLEN): the group's G
 * blocks must be able to take the whole frame with room to spare, however unevenly they draw (any block may end up in the
 * common pool) */
inline bool tail_queue_fits(uint32_t nslices, uint32_t G) { return (uint64_t)(nslices / H2Y_TAIL_CHUNK + 96u) * 2u <= 64ull * G && G >= 8u; }
inline void make_slice_plan(slice_plan &s, const launch_plan &l, uint32_t tiles, const double sp[8], const block_speeds &bs, bool t1, int opt_tail)
{
    const int grid = l.grid, groups = l.groups, nf = l.frames;
    const uint32_t G = (uint32_t)grid / (uint32_t)groups, nslices = (tiles + 63u) / 64u;
    double mean = 0.0;
    for (int x = 0; x < 8; x++) mean += sp[x] / 8.0;
    for (int x = 0; x < 8; x++) s.work[x] = sp[x] / mean;
    /* per block when this grid shape has been measured (adaptive mode), else per XCD: one table for every group */
    const bool per_block = bs.use && bs.grid == grid && bs.groups == groups && (int)bs.speed->size() == grid && (size_t)groups * (G + 1u) <= kRangeWords;
    s.r.assign(per_block ? (size_t)groups * (G + 1u) : (size_t)G + 1u, 0u);
    s.bwork.assign((size_t)grid, 1.0);
    s.range_stride = 0;
    if (per_block) {
        std::vector<double> w(G);
        for (uint32_t gi = 0; gi < (uint32_t)groups; gi++) {
            for (uint32_t i = 0; i < G; i++) w[i] = (*bs.speed)[walk_block_of(gi, i, (uint32_t)groups)];
            slice_ranges_w(w.data(), G, nslices, s.r.data() + (size_t)gi * (G + 1u)); /* h2y_walk.h */
        }
        s.range_stride = G + 1u;
    } else slice_ranges(sp, G, nslices, s.r.data());
    const int per_group = nf / groups;
    s.tail_on = t1 && opt_tail != 2 && nf % groups == 0 && per_group >= (opt_tail == 1 ? 2 : kTailMinFrames) && groups <= 16 && tail_queue_fits(nslices, G);
    s.slices = nslices;
    for (uint32_t gi = 0; gi < (uint32_t)groups; gi++) {
        const uint32_t *rg = s.r.data() + (size_t)(per_block ? gi : 0u) * (G + 1u);
        for (uint32_t i = 0; i < G; i++) s.bwork[walk_block_of(gi, i, (uint32_t)groups)] = (double)(rg[i + 1] - rg[i]) * (double)G / (double)nslices;
    }
}

/* After a launch whose clocks came back: speed of each of n parts (XCDs, blocks) = the work it had / the time it took,
 * normalised by the mean and clamped to 0.75 ... 1.25; the first sample is taken as it is (!have), later ones are blended in
 * with `weight`.  No update at all (false) when a time or a work is not positive: a grid smaller than a round of XCDs, or
 * nothing measured. */
inline bool speed_update(double *speed, bool have, const double *work, const float *time, int n, double weight)
{
    double mean = 0.0;
    for (int i = 0; i < n; i++) {
        const double t = time[i];
        if (!(t > 0.0) || !(work[i] > 0.0)) return false;
        mean += work[i] / t / n;
    }
    for (int i = 0; i < n; i++) {
        double v = work[i] / (double)time[i] / mean;
        if (v < 0.75) v = 0.75;
        if (v > 1.25) v = 1.25;
        speed[i] = have ? (1.0 - weight) * speed[i] + weight * v : v;
    }
    return true;
}

} // namespace h2y
#endif
