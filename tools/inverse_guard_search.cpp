// Locates, over the whole 12-bit (Y, Cb, Cr) cube, the triples whose BT.709 green quotient of matrix_inverse
//     q = (Y - 0.07222 Bp - 0.2126 Rp) / 0.7152 + 0.5        (binary64; Bp, Rp binary32, clamped at 4095)
// lies within WINDOW ulp(double) of a binary32 rounding tie AND whose tie sits on an integer: the two floats either side of
// it truncate to different integers, so the OUTPUT CODE depends on which way (float)q rounds.  Everywhere else a quotient
// that is a few ulp(double) off gives the same code.  2^36 triples, a minute or two on eight threads.
//
// Used by tests/golden/make_inverse_guard_triples.py, which checks every triple printed here again in numpy.  The
// expression is the reference's; nothing of hdr2yuv_amd is included.  Build: g++ -O2 -ffp-contract=off -pthread.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

static const int64_t WINDOW = 4096, TIE = 1ll << 28, LOW29 = (1ll << 29) - 1;

static int code_of(double q)
{
    float t = (float)q;
    if (t > 4095.0f) t = 4095.0f;
    return (int)t;
}

struct hit { int y, cb, cr; };

static void work(int first, int step, std::vector<hit> *out)
{
    std::vector<float> Bp(4096), Rp(4096);
    for (int y = first; y < 4096; y += step) {
        for (int c = 0; c < 4096; c++) {
            float t = (float)(((double)(float)c - 2047.5) * 1.8556 + (double)(float)y);
            Bp[c] = t > 4095.0f ? 4095.0f : t;
            t = (float)(((double)(float)c - 2047.5) * 1.5748 + (double)(float)y);
            Rp[c] = t > 4095.0f ? 4095.0f : t;
        }
        for (int cr = 0; cr < 4096; cr++) {
            const double r = 0.2126 * (double)Rp[cr];
            for (int cb = 0; cb < 4096; cb++) {
                const double q = (((double)(float)y - 0.07222 * (double)Bp[cb]) - r) / 0.7152 + 0.5;
                if (!(q > 0.0)) continue;
                int64_t b;
                memcpy(&b, &q, 8);
                const int64_t d = (b & LOW29) - TIE;
                if (d < -WINDOW || d > WINDOW) continue;
                const int64_t lo = b - 2 * WINDOW, hi = b + 2 * WINDOW; // either side of the tie, wherever in the window q is
                double ql, qh;
                memcpy(&ql, &lo, 8);
                memcpy(&qh, &hi, 8);
                if (code_of(ql) != code_of(qh)) out->push_back(hit{y, cb, cr});
            }
        }
    }
}

int main()
{
    const int NT = 8; // whatever the machine: the output is sorted by the caller, the work split does not show
    std::vector<std::vector<hit>> found(NT);
    std::vector<std::thread> th;
    for (int t = 0; t < NT; t++) th.emplace_back(work, t, NT, &found[t]);
    for (auto &t : th) t.join();
    for (auto &v : found)
        for (const hit &h : v) printf("%d %d %d\n", h.y, h.cb, h.cr);
    return 0;
}
