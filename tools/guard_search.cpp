/*
 * tools/guard_search.cpp -- TEST TOOL (host build of h2y_math.h), run by tests/golden/make_guard_pixels.py.
 * Finds input pixels (G, B, R as binary32 bit patterns) that sit on the edges of the two guards that act on a PIXEL:
 *   the chroma division's fma(d, 1/c, 0.5) shortcut, trusted unless the fraction of the quotient is below 2^-30 or
 *   above 1 - 2^-21 (H2Y_GUARD_LO / H2Y_GUARD_HI), and the window in which a pixel with an unsure first-tier sample is
 *   redone (t1_bounds).
 * Categories (one line each: "config category G B R", bits in hex):
 *   0 lo_in    no unsure sample, a chroma fraction below 2^-30            1 lo_out   ... in [2^-30, 5 x 2^-30), pixel not redone
 *   2 hi_in    no unsure sample, a chroma fraction of 1 - 2^-21 or more   3 hi_out   ... in [1 - 5 x 2^-21, 1 - 2^-21), not redone
 *   4 t1_moves an unsure sample whose one-ulp move changes an output integer
 *   5 t1_near  an unsure sample, pixel NOT redone, but redone if t1_bounds' window were twice as wide
 * The search is deterministic: 8 workers whatever the machine, each over its own fixed share of (G, R) pairs, every B of a
 * fixed table inside; results are merged in worker order.  The header only LOCATES pixels: expected codes are the reference's.
 * usage: guard_search LOG2_PAIRS
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>
#include <vector>
#include "../hdr2yuv_amd/csrc/h2y_math.h"
using namespace h2y;

struct cfg { const char *name; int depth, full, mode, m709; };
static void make_params(const cfg &c, pix_params *pp)
{
    memset(pp, 0, sizeof *pp);
    unsigned maxCV = (1u << c.depth) - 1, D = 1u << (c.depth - 8);
    unsigned minVR = c.full ? 0 : 16 * D, maxVR = c.full ? maxCV : 235 * D, maxVRC = c.full ? maxCV : 240 * D;
    pp->convert_transfer = 1; pp->norm_identity = 1; pp->src_tf = H2Y_TF_LINEAR; pp->dst_tf = H2Y_TF_PQ;
    if (c.full) pp->mulY = pp->mulC = (float)maxCV;
    else { pp->mulY = (float)maxVR; pp->addY = (float)minVR; pp->mulC = (float)maxVRC; pp->addC = (float)minVR; }
    pp->mode = c.mode;
    if (c.mode == H2Y_MODE_YCBCR) {
        if (c.m709) { pp->kr = 0.2126; pp->kg = 0.7152; pp->kb = 0.0722; pp->dcb = 1.8556; pp->dcr = 1.5748; }
        else { pp->kr = 0.2627; pp->kg = 0.6780; pp->kb = 0.0593; pp->dcb = 1.8814; pp->dcr = 1.4746; }
        pp->inv_dcb = 1.0 / pp->dcb; pp->inv_dcr = 1.0 / pp->dcr;
    }
    pp->half_m1 = (1u << (c.depth - 1)) - 1; pp->maxCV = maxCV;
}
struct sample { uint32_t x; float v, vdown, ys, cs; bool unsure; };
struct hit { int cat; uint32_t g, b, r; };
static inline double frac_of(uint32_t hw) { return bits2d((uint64_t)hw << 32); }

template <int MODE>
static void exact(const pix_params &pp, float vg, float vb, float vr, uint32_t o[3])
{
    bool dummy;
    pix_matrix<MODE, true>(pp, pix_scale(vg, pp.mulY, pp.addY), pix_scale(vb, pp.mulC, pp.addC), pix_scale(vr, pp.mulC, pp.addC), o[0], o[1], o[2], &dummy);
}
template <int MODE>
static void search(const cfg &c, int ci, const pix_params &pp, const t1_sens &sn, bool t1, const std::vector<sample> &S, long pairs, std::vector<hit> *out)
{
    const int T = 8;
    const uint32_t lo4 = hiword_of(5.0 * 0x1p-30), hi4 = hiword_of(1.0 - 5.0 * 0x1p-21);
    std::vector<std::vector<hit>> per(T);
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++) th.emplace_back([&, t]() {
        std::mt19937_64 rng(7001 + 131 * ci + t);
        int n[6] = {0, 0, 0, 0, 0, 0};
        const int cap[6] = {64, 64, 64, 64, 64, 64};
        for (long p = t; p < pairs; p += T) {
            const sample &sg = S[rng() % S.size()], &sr = S[rng() % S.size()];
            for (size_t k = 0; k < S.size(); k++) {
                const sample &sb = S[k];
                const bool vunc = sg.unsure | sb.unsure | sr.unsure;
                if (vunc && (!t1 || (n[4] >= cap[4] && n[5] >= cap[5]))) continue;
                uint32_t Y, Cb, Cr;
                bool ra, rb;
                pix_matrix_t1<MODE>(pp, sn, sg.ys, sb.cs, sr.cs, vunc, Y, Cb, Cr, &ra, &rb);
                const bool redo = ra | rb;
                if (!vunc) {
                    if (MODE != H2Y_MODE_YCBCR) continue; /* YDzDx has no division */
                    const double yd = ((pp.kr * (double)sr.cs + pp.kg * (double)sg.ys) + pp.kb * (double)sb.cs) + 0.5;
                    const float tmpF = (float)yd;
                    const double qb = __builtin_fma((double)(sb.cs - tmpF), pp.inv_dcb, 0.5), qr = __builtin_fma((double)(sr.cs - tmpF), pp.inv_dcr, 0.5);
                    const uint32_t fb = (uint32_t)(d2bits(fract_f64(qb)) >> 32), fr = (uint32_t)(d2bits(fract_f64(qr)) >> 32);
                    const uint32_t mn = fb < fr ? fb : fr, mx = fb < fr ? fr : fb;
                    int cat = -1;
                    if (mn < H2Y_GUARD_LO) cat = 0;
                    else if (mx >= H2Y_GUARD_HI) cat = 2;
                    else if (!redo && mn < lo4) cat = 1;
                    else if (!redo && mx >= hi4) cat = 3;
                    if (cat >= 0 && n[cat] < cap[cat]) { n[cat]++; per[t].push_back({cat, sg.x, sb.x, sr.x}); }
                    continue;
                }
                /* an unsure sample: does its one-ulp move change an integer? */
                uint32_t a[3], b[3];
                exact<MODE>(pp, sg.v, sb.v, sr.v, a);
                bool moves = false;
                for (int w = 0; w < 3 && !moves; w++) {
                    const sample &s = w == 0 ? sg : w == 1 ? sb : sr;
                    if (!s.unsure) continue;
                    exact<MODE>(pp, w == 0 ? s.vdown : sg.v, w == 1 ? s.vdown : sb.v, w == 2 ? s.vdown : sr.v, b);
                    moves = a[0] != b[0] || a[1] != b[1] || a[2] != b[2];
                }
                if (moves) { if (n[4] < cap[4]) { n[4]++; per[t].push_back({4, sg.x, sb.x, sr.x}); } continue; }
                if (redo || n[5] >= cap[5]) continue;
                t1_sens wide = sn; /* the window twice as wide */
                if (MODE == H2Y_MODE_YCBCR) {
                    wide.a_lo = hiword_of(2.0 * frac_of(sn.a_lo));
                    wide.a_hi = hiword_of(1.0 - 2.0 * (1.0 - frac_of(sn.a_hi)));
                } else {
                    wide.ty = sn.ty - (0.5f - sn.ty);
                    const double l = frac_of(sn.cb_lo), h = frac_of(sn.cb_lo + sn.cb_span), l2 = frac_of(sn.cr_lo), h2 = frac_of(sn.cr_lo + sn.cr_span);
                    wide.cb_lo = hiword_of(2.0 * l); wide.cb_span = hiword_of(1.0 - 2.0 * (1.0 - h)) - wide.cb_lo;
                    wide.cr_lo = hiword_of(2.0 * l2); wide.cr_span = hiword_of(1.0 - 2.0 * (1.0 - h2)) - wide.cr_lo;
                }
                bool wa, wb;
                pix_matrix_t1<MODE>(pp, wide, sg.ys, sb.cs, sr.cs, true, Y, Cb, Cr, &wa, &wb);
                if (wa | wb) { n[5]++; per[t].push_back({5, sg.x, sb.x, sr.x}); }
            }
        }
    });
    for (auto &x : th) x.join();
    for (int t = 0; t < T; t++) out->insert(out->end(), per[t].begin(), per[t].end());
}

int main(int argc, char **argv)
{
    const long pairs = 1L << (argc > 1 ? atoi(argv[1]) : 14);
    std::vector<pq_recA> A(H2Y_PQ_NREC); std::vector<pq_recB> B(H2Y_PQ_NREC); std::vector<pq_rec1> T1(H2Y_T1_NREC);
    pq_build_table(A.data(), B.data()); pq_build_table1(T1.data());
    const cfg cfgs[] = {{"2020_12b_video", 12, 0, H2Y_MODE_YCBCR, 0}, {"709_10b_video", 10, 0, H2Y_MODE_YCBCR, 1},
                        {"2020_16b_full", 16, 1, H2Y_MODE_YCBCR, 0}, {"ydzdx_12b_video", 12, 0, H2Y_MODE_YDZDX, 0}};
    int ci = 0;
    for (const cfg &c : cfgs) {
        pix_params pp; make_params(c, &pp);
        t1_sens sn; const bool t1 = t1_bounds(pp, &sn);
        std::mt19937_64 rng(4242 + ci);
        std::vector<sample> S(1 << 16);
        for (sample &s : S) {
            const uint64_t q = rng();
            const float x = (q & 1) ? (float)(q >> 40) * (1.0f / 16777216.0f) : bits2f(0x38800000u + (uint32_t)((q >> 8) % (0x3F800000u - 0x38800000u)));
            bool slow, unsure;
            float v = pq_fast(x, A.data(), B.data(), &slow);
            if (slow) v = pq_slow(x);
            (void)pq_t1(x, T1.data(), &unsure);
            s.x = f2bits(x); s.v = v; s.vdown = bits2f(f2bits(v) - 1u); s.unsure = unsure;
            s.ys = pix_scale(v, pp.mulY, pp.addY); s.cs = pix_scale(v, pp.mulC, pp.addC);
        }
        std::vector<hit> hits;
        if (c.mode == H2Y_MODE_YCBCR) search<H2Y_MODE_YCBCR>(c, ci, pp, sn, t1, S, pairs, &hits);
        else search<H2Y_MODE_YDZDX>(c, ci, pp, sn, t1, S, pairs, &hits);
        for (const hit &h : hits) printf("%s %d %08x %08x %08x\n", c.name, h.cat, h.g, h.b, h.r);
        fprintf(stderr, "%s: t1 admitted %d, %ld pairs x %zu = %.3g pixels searched, %zu found\n", c.name, (int)t1, pairs, S.size(), (double)pairs * S.size(), hits.size());
        ci++;
    }
    return 0;
}
