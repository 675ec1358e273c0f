/*
 * h2y_measure.hip -- the measurements and passes of the C-ABI shim, in four families.  A frame against a reference (cmp_frame
 * entries): the comparison, SSIM, flat and busy areas.  Light and code planes (codelight_plan): content light, the light
 * distribution, the light of PQ code planes, scene signatures and cuts, Delta E ITP, the three linearisers, and further down the
 * HLG and SDR inverses' host twins.  Whole u16 frames: histograms and the scaler, and at the end dither and the sample packings.
 * Passes in place over float planes (gamut_frame entries): the conversion between colour primaries, the tone map, the 3D LUT, HLG,
 * ICtCp.  Each has its checks and geometry, its batch entry, its ring stage (ring_stage, h2y_shim.h), and its arm, result and
 * *_stream_open entries; what they share is in h2y_entry.h and at the head of each family.
 */
#include "h2y_shim.h"

#include "h2y_lut3d1.h"
#include "h2y_hlg1.h"
#include "h2y_gamut1.h"
#include "h2y_gamutcheck1.h"
#include "h2y_dither1.h"
#include "h2y_pack1.h"

/* ---- comparison with a reference (--ref_filename, hdr2yuv.cpp:91-100, :827-833) ---------------------------------------- */

/* k_compare's geometry: planes of n[p] samples (4:2:0: Y, then two chroma planes of (width >> 1) x (height >> 1)) starting at
 * a_off / b_off samples from the two frames' bases */
static cmp_geom cmp_geom_of(int width, int height, int chroma, int sigma, const uint32_t a_off[3], const uint32_t b_off[3])
{
    cmp_geom g{};
    for (int p = 0; p < 3; p++) {
        const plane_dim d = plane_dims(width, height, chroma, p);
        g.n[p] = d.w * d.h;
        g.width[p] = d.w;
        g.a_off[p] = a_off[p];
        g.b_off[p] = b_off[p];
        const bool vec = (a_off[p] & 7u) == (b_off[p] & 7u);
        g.shift[p] = vec ? a_off[p] & 7u : 0u;
        g.vec |= vec ? 1u << p : 0u;
        g.chunks[p] = h2y_compare_chunks(g.n[p], g.shift[p]);
    }
    g.sigma = (uint32_t)sigma;
    return g;
}

static int cmp_check(h2y_ctx *ctx, int width, int height, int chroma, int sigma)
{
    const int rc = picture_size_check(ctx, width, height);
    if (rc) return rc;
    if (chroma != H2Y_CHROMA_420 && chroma != H2Y_CHROMA_444) return fail(ctx, H2Y_EINVAL, "chroma_format_idc must be 1 or 3");
    if (sigma < 0) return fail(ctx, H2Y_EINVAL, "sigma must be >= 0");
    return H2Y_OK;
}

/* k_compare's partials for n_frames frames of g */
static int cmp_partials(h2y_ctx *ctx, const cmp_geom &g, int n_frames)
{
    return ensure(ctx, ctx->cmp_part, std::max<size_t>(1, (size_t)n_frames * (g.chunks[0] + g.chunks[1] + g.chunks[2])) * sizeof(cmp_partial));
}

static int cmp_grid(const h2y_ctx *ctx, const cmp_geom &g, int n_frames)
{
    return unit_grid(ctx, (uint64_t)n_frames * (g.chunks[0] + g.chunks[1] + g.chunks[2]));
}

int h2y_compare_batch(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int sigma, int n_frames, const uint16_t *const *d_a,
                      const uint16_t *const *d_b, h2y_compare_stats *out)
{
    int rc = batch_enter(ctx);
    if (!rc) rc = cmp_check(ctx, width, height, chroma_format_idc, sigma);
    if (rc) return rc;
    uint32_t off[3];
    contiguous_planes(width, height, chroma_format_idc, off);
    const cmp_geom g = cmp_geom_of(width, height, chroma_format_idc, sigma, off, off);
    rc = pair_batch(ctx, n_frames, d_a, d_b, out, ctx->cmp_stats, H2Y_COMPARE_FRAMES_PER_LAUNCH, "k_compare",
                    [&](int nf) { return cmp_partials(ctx, g, nf); },
                    [&](const cmp_frame *frames, int f0, int nf) {
                        return h2y_launch_compare(cmp_grid(ctx, g, nf), ctx->stream, g, frames, nf, ctx->cmp_part.p, ctx->cmp_stats.p + f0);
                    });
    if (rc) return rc;
    ctx->last_variant = std::string("k_compare<") + (chroma_format_idc == H2Y_CHROMA_420 ? "420" : "444") + ">";
    return H2Y_OK;
}

/* The comparison's ring stage.  Per slot a pinned reference (the planes one after the other), its device twin laid out as the
 * ring's frame (so both sides share each plane's alignment and k_compare keeps its 16-byte loads) with the frame's stats behind
 * it (256-byte aligned), pinned stats, and the slot's k_compare table entry (A: the ring's frame, B: the device reference) */
struct cmp_stage : ring_stage {
    struct slot {
        char *h_ref = nullptr, *d_ref = nullptr;
        h2y_compare_stats *h_stats = nullptr;
        bool ref_lent = false;
    };
    std::vector<slot> ss;
    cmp_geom g{};
    cmp_frame *tab = nullptr;
    size_t ref_bytes = 0, stats_off = 0; /* the pinned reference's bytes; where the stats lie in its device twin */
    /* a compare-only ring armed with h2y_stream_unpack: the lent reference holds a packed frame of packed_bytes, which goes up as it
     * is into packed_to[slot]; the unpack stage's k_unpack writes the device twin from there */
    size_t packed_bytes = 0;
    std::vector<char *> packed_to;
    h2y_compare_stats *dev_stats(int k) const { return reinterpret_cast<h2y_compare_stats *>(ss[k].d_ref + stats_off); }
    int ready(h2y_ctx *ctx, int k) override
    {
        if (!ss[k].ref_lent) return fail(ctx, H2Y_EINVAL, "the ring is armed: h2y_stream_reference before each submit");
        return H2Y_OK;
    }
    int upload(h2y_ctx *ctx, int k) override
    {
        slot &s = ss[k];
        if (packed_bytes) HIP_TRY(ctx, hipMemcpyAsync(packed_to[k], s.h_ref, packed_bytes, hipMemcpyHostToDevice, ctx->s_h2d));
        else if (g.b_off[1] == g.n[0] && g.b_off[2] == g.n[0] + g.n[1]) /* the device twin is contiguous too: one copy */
            HIP_TRY(ctx, hipMemcpyAsync(s.d_ref, s.h_ref, ref_bytes, hipMemcpyHostToDevice, ctx->s_h2d));
        else /* padded apart as the inverse ring's output planes */
            for (size_t c = 0, h_off = 0; c < 3; h_off += g.n[c] * sizeof(uint16_t), c++)
                HIP_TRY(ctx, hipMemcpyAsync(s.d_ref + g.b_off[c] * sizeof(uint16_t), s.h_ref + h_off, g.n[c] * sizeof(uint16_t),
                                            hipMemcpyHostToDevice, ctx->s_h2d));
        s.ref_lent = false;
        return H2Y_OK;
    }
    int run(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, h2y_launch_compare(cmp_grid(ctx, g, 1), ctx->stream, g, tab + k, 1, ctx->cmp_part.p, dev_stats(k)));
        return H2Y_OK;
    }
    int download(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, hipMemcpyAsync(ss[k].h_stats, dev_stats(k), sizeof(h2y_compare_stats), hipMemcpyDeviceToHost, ctx->s_d2h));
        return H2Y_OK;
    }
};

/* arm the open ring's frame; keep_output 0: the frame stays on the device */
static int cmp_arm(h2y_ctx *ctx, int sigma, int keep_output)
{
    const ring_frame &f = ctx->s_frame;
    int rc = cmp_check(ctx, f.width, f.height, f.chroma, sigma);
    if (rc) return rc;
    auto st = std::make_unique<cmp_stage>();
    const cmp_geom &g = st->g = cmp_geom_of(f.width, f.height, f.chroma, sigma, f.off, f.off);
    const int depth = (int)ctx->ss.size();
    st->ref_bytes = ((size_t)g.n[0] + g.n[1] + g.n[2]) * sizeof(uint16_t);
    st->stats_off = (((size_t)f.off[2] + g.n[2]) * sizeof(uint16_t) + 255) & ~(size_t)255;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = cmp_partials(ctx, g, 1);
    if (rc) return rc;
    std::vector<cmp_frame> tab(depth);
    st->ss.resize(depth);
    for (int k = 0; k < depth; k++) {
        cmp_stage::slot &s = st->ss[k];
        st->pin_alloc(s.h_ref, st->ref_bytes);
        st->pin_alloc(s.h_stats, sizeof(h2y_compare_stats));
        st->dev_alloc(s.d_ref, st->stats_off + sizeof(h2y_compare_stats));
        tab[k] = cmp_frame{frame_base(ctx, k), reinterpret_cast<const uint16_t *>(s.d_ref)};
    }
    st->table(st->tab, tab);
    rc = stage_arm(ctx, STAGE_COMPARE, std::move(st), "compare");
    if (!rc && !keep_output) ring_frame_stays(ctx);
    return rc;
}

int h2y_stream_compare(h2y_ctx *ctx, int sigma, int keep_output)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    if (ctx->s_stage[STAGE_COMPARE]) return fail(ctx, H2Y_EINVAL, "the ring is armed already");
    if (ctx->s_stage[STAGE_CODELIGHT]) return fail(ctx, H2Y_EINVAL, "a light-only ring takes no other stage");
    if (ctx->s_stage[STAGE_SCALE]) return fail(ctx, H2Y_EUNSUPPORTED, "a ring that scales is not compared: compare the written file instead");
    if (ctx->s_stage[STAGE_DITHER]) return fail(ctx, H2Y_EUNSUPPORTED, "a ring that dithers is not compared: compare the written file instead");
    if (ctx->s_stage[STAGE_PACK]) return fail(ctx, H2Y_EUNSUPPORTED, "a ring that packs is not compared: compare the written file instead");
    if (ctx->s_stage[STAGE_UNPACK] && ctx->s_kind == h2y_ctx::RING_PLANES)
        return fail(ctx, H2Y_EINVAL, "the ring unpacks already: arm the comparison before unpack, so that its reference is unpacked too");
    rc = arm_unstarted(ctx);
    if (rc) return rc;
    if (keep_output != 0 && keep_output != 1) return fail(ctx, H2Y_EINVAL, "keep_output must be 0 or 1");
    return cmp_arm(ctx, sigma, keep_output);
}

int h2y_stream_reference(h2y_ctx *ctx, void **ref)
{
    if (!ctx || !ref) return fail(ctx, H2Y_EINVAL, "null argument");
    if (!ctx->streaming) return fail(ctx, H2Y_EINVAL, "no stream open");
    cmp_stage *st = stage_of<cmp_stage>(ctx, STAGE_COMPARE);
    if (!st) return fail(ctx, H2Y_EINVAL, "the ring is not armed: h2y_stream_compare first");
    const int state = ctx->ss[ctx->s_tail].state;
    if (state != 0 && state != 1) return fail(ctx, H2Y_EINVAL, "all %d slots are in flight: take an output first", (int)ctx->ss.size());
    st->ss[ctx->s_tail].ref_lent = true;
    *ref = st->ss[ctx->s_tail].h_ref;
    return H2Y_OK;
}

int h2y_stream_compare_result(h2y_ctx *ctx, h2y_compare_stats *out)
{
    return stream_result<cmp_stage>(ctx, out, STAGE_COMPARE, "no armed stream open", [&](const cmp_stage &st, int k) { *out = *st.ss[k].h_stats; });
}

/* A ring that only compares: the slot's input is A's three planes, the device output unused */
int h2y_compare_stream_open(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int sigma, int depth)
{
    int rc = ring_may_open(ctx);
    if (!rc) rc = cmp_check(ctx, width, height, chroma_format_idc, sigma);
    if (!rc) rc = open_planes_ring(ctx, width, height, chroma_format_idc, 0, 0, 0, 0, depth);
    if (rc) return rc;
    rc = cmp_arm(ctx, sigma, 0);
    if (rc) stream_free(ctx);
    return rc;
}

/* ---- SSIM beside the comparison (hdr2yuv.cpp:826) ------------------------------------------------------------------------ */

/* k_ssim's geometry: the comparison's planes (4:2:0: Y, then two chroma planes of (width >> 1) x (height >> 1)) starting at a_off /
 * b_off samples from the two frames' bases, and the constants of bit_depth, computed once here in binary64, left to right */
static ssim_geom ssim_geom_of(int width, int height, int chroma, int bit_depth, const uint32_t a_off[3], const uint32_t b_off[3])
{
    ssim_geom g{};
    for (int p = 0; p < 3; p++) {
        const plane_dim d = plane_dims(width, height, chroma, p);
        g.pw[p] = d.w;
        g.ph[p] = d.h;
        g.a_off[p] = a_off[p];
        g.b_off[p] = b_off[p];
        g.strips[p] = h2y_ssim_strips(g.pw[p]);
        g.units[p] = g.strips[p] * h2y_ssim_segments(g.ph[p]);
    }
    g.wide = bit_depth > 12;
    const double M = (double)((1u << bit_depth) - 1u);
    g.c1 = ((0.01 * 0.01) * M) * M * 64.0;
    g.c2 = (((0.03 * 0.03) * M) * M * 64.0) * 63.0;
    return g;
}

static int ssim_check(h2y_ctx *ctx, int width, int height, int chroma, int bit_depth)
{
    const int rc = picture_size_check(ctx, width, height);
    if (rc) return rc;
    if (chroma == 2) return fail(ctx, H2Y_EUNSUPPORTED, "chroma_format_idc 2 (4:2:2) has no SSIM on this path");
    if (chroma != H2Y_CHROMA_420 && chroma != H2Y_CHROMA_444) return fail(ctx, H2Y_EINVAL, "chroma_format_idc must be 1 or 3");
    if (bit_depth < 8 || bit_depth > 16) return fail(ctx, H2Y_EINVAL, "bit_depth must be 8..16");
    const int sub = chroma == H2Y_CHROMA_420;
    if ((width >> sub) < 8 || (height >> sub) < 8)
        return fail(ctx, H2Y_EINVAL, "SSIM needs every plane at least 8x8 (one window): %dx%d %s", width, height, sub ? "4:2:0" : "4:4:4");
    return H2Y_OK;
}

/* k_ssim's partials for n_frames frames of g */
static int ssim_partials(h2y_ctx *ctx, const ssim_geom &g, int n_frames)
{
    return ensure(ctx, ctx->ssim_part, (size_t)n_frames * (g.units[0] + g.units[1] + g.units[2]) * sizeof(int64_t));
}

int h2y_ssim_batch(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int bit_depth, int n_frames, const uint16_t *const *d_a,
                   const uint16_t *const *d_b, h2y_ssim_stats *out)
{
    int rc = batch_enter(ctx);
    if (!rc) rc = ssim_check(ctx, width, height, chroma_format_idc, bit_depth);
    if (rc) return rc;
    uint32_t off[3];
    contiguous_planes(width, height, chroma_format_idc, off);
    const ssim_geom g = ssim_geom_of(width, height, chroma_format_idc, bit_depth, off, off);
    rc = pair_batch(ctx, n_frames, d_a, d_b, out, ctx->ssim_stats, H2Y_SSIM_FRAMES_PER_LAUNCH, "k_ssim",
                    [&](int nf) { return ssim_partials(ctx, g, nf); },
                    [&](const cmp_frame *frames, int f0, int nf) {
                        return h2y_launch_ssim(h2y_ssim_grid(ctx->n_cu, g, nf), ctx->stream, g, frames, nf, ctx->ssim_part.p, ctx->ssim_stats.p + f0);
                    });
    if (rc) return rc;
    ctx->last_variant = std::string("k_ssim<") + (chroma_format_idc == H2Y_CHROMA_420 ? "420" : "444") + "," + (g.wide ? "U64" : "U32") + ">";
    return H2Y_OK;
}

/* SSIM's ring stage: k_ssim after k_compare, on the comparison's table entry of the slot, the frame's SSIM on the device and
 * pinned */
struct ssim_stage : result_stage<h2y_ssim_stats> {
    ssim_geom g{};
    const cmp_frame *tab = nullptr; /* the comparison's stage's */
    int run(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, h2y_launch_ssim(h2y_ssim_grid(ctx->n_cu, g, 1), ctx->stream, g, tab + k, 1, ctx->ssim_part.p, ss[k].d));
        return H2Y_OK;
    }
};

int h2y_stream_ssim(h2y_ctx *ctx, int bit_depth)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    if (ctx->s_stage[STAGE_SCALE]) return fail(ctx, H2Y_EUNSUPPORTED, "a ring that scales computes no SSIM: compare the written file instead");
    if (ctx->s_stage[STAGE_DITHER]) return fail(ctx, H2Y_EUNSUPPORTED, "a ring that dithers computes no SSIM: compare the written file instead");
    if (ctx->s_stage[STAGE_PACK]) return fail(ctx, H2Y_EUNSUPPORTED, "a ring that packs computes no SSIM: compare the written file instead");
    const cmp_stage *cmp = stage_of<cmp_stage>(ctx, STAGE_COMPARE);
    if (!cmp) return fail(ctx, H2Y_EINVAL, "the ring is not armed for comparison: h2y_stream_compare first");
    rc = arm_free(ctx, STAGE_SSIM, "the ring computes SSIM already");
    if (rc) return rc;
    const ring_frame &f = ctx->s_frame;
    if (bit_depth < 0) {
        if (!f.depth) return fail(ctx, H2Y_EINVAL, "a compare-only ring does not know its frames' bit depth: give it to h2y_stream_ssim");
        bit_depth = f.depth;
    }
    rc = ssim_check(ctx, f.width, f.height, f.chroma, bit_depth);
    if (rc) return rc;
    auto st = std::make_unique<ssim_stage>();
    st->g = ssim_geom_of(f.width, f.height, f.chroma, bit_depth, f.off, f.off);
    st->tab = cmp->tab;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = ssim_partials(ctx, st->g, 1);
    if (rc) return rc;
    st->slots(ctx->ss.size());
    return stage_arm(ctx, STAGE_SSIM, std::move(st), "SSIM");
}

int h2y_stream_ssim_result(h2y_ctx *ctx, h2y_ssim_stats *out)
{
    return stream_result<ssim_stage>(ctx, out, STAGE_SSIM, "no stream open that computes SSIM", [&](const ssim_stage &st, int k) { *out = *st.ss[k].h; });
}

/* ---- PSNR of flat and of busy areas, over- and undershoot, beside the comparison ------------------------------------------------ */

/* k_regions' geometry: the comparison's planes starting at a_off / b_off samples from the two frames' bases */
static regions_geom regions_geom_of(int width, int height, int chroma, uint32_t flat_var, int radius, const uint32_t a_off[3], const uint32_t b_off[3])
{
    regions_geom g{};
    for (int p = 0; p < 3; p++) {
        const plane_dim d = plane_dims(width, height, chroma, p);
        g.pw[p] = d.w;
        g.ph[p] = d.h;
        g.a_off[p] = a_off[p];
        g.b_off[p] = b_off[p];
        g.strips[p] = h2y_regions_strips(g.pw[p]);
        g.units[p] = g.strips[p] * h2y_regions_segments(g.ph[p]);
    }
    g.flat_var = flat_var;
    g.radius = (uint32_t)radius;
    return g;
}

static int regions_check(h2y_ctx *ctx, int width, int height, int chroma, int radius)
{
    const int rc = picture_size_check(ctx, width, height);
    if (rc) return rc;
    if (chroma == 2) return fail(ctx, H2Y_EUNSUPPORTED, "chroma_format_idc 2 (4:2:2) has no flat and busy areas on this path");
    if (chroma != H2Y_CHROMA_420 && chroma != H2Y_CHROMA_444) return fail(ctx, H2Y_EINVAL, "chroma_format_idc must be 1 or 3");
    if (radius < 1 || radius > 4) return fail(ctx, H2Y_EINVAL, "radius must be 1..4");
    return H2Y_OK;
}

/* k_regions' partials for n_frames frames of g */
static int regions_partials(h2y_ctx *ctx, const regions_geom &g, int n_frames)
{
    return ensure(ctx, ctx->regions_part, std::max<size_t>(1, (size_t)n_frames * (g.units[0] + g.units[1] + g.units[2])) * sizeof(regions_partial));
}

/* The definition of h2y_regions_stats, step by step, on one plane of pw x ph samples */
static void regions_host_plane(const uint16_t *a, const uint16_t *b, int pw, int ph, uint32_t flat_var, int r, int p, h2y_regions_stats *o)
{
    for (int ty = 0; ty < ph; ty += 8)
        for (int tx = 0; tx < pw; tx += 8) {
            const int tw = std::min(8, pw - tx), th = std::min(8, ph - ty);
            uint64_t s = 0, ss = 0, sse = 0, sad = 0;
            for (int y = ty; y < ty + th; y++)
                for (int x = tx; x < tx + tw; x++) {
                    const uint64_t bv = b[(size_t)y * pw + x], av = a[(size_t)y * pw + x], d = av > bv ? av - bv : bv - av;
                    s += bv, ss += bv * bv, sse += d * d, sad += d;
                }
            const uint64_t n = (uint64_t)tw * th, act = n * ss - s * s;
            const int c = act <= (uint64_t)flat_var * n * n ? 0 : 1;
            o->tiles[p][c] += 1, o->samples[p][c] += n, o->sse[p][c] += sse, o->sad[p][c] += sad;
        }
    for (int y = 0; y < ph; y++)
        for (int x = 0; x < pw; x++) {
            uint32_t m = 65535u, M = 0u;
            for (int yy = std::max(0, y - r); yy <= std::min(ph - 1, y + r); yy++)
                for (int xx = std::max(0, x - r); xx <= std::min(pw - 1, x + r); xx++) {
                    const uint32_t bv = b[(size_t)yy * pw + xx];
                    m = std::min(m, bv), M = std::max(M, bv);
                }
            const uint32_t av = a[(size_t)y * pw + x];
            if (av > M) o->over[p] += 1, o->over_sum[p] += av - M, o->over_max[p] = std::max(o->over_max[p], av - M);
            if (av < m) o->under[p] += 1, o->under_sum[p] += m - av, o->under_max[p] = std::max(o->under_max[p], m - av);
        }
}

int h2y_regions_host(int width, int height, int chroma_format_idc, uint32_t flat_var, int radius, const uint16_t *a, const uint16_t *b,
                     h2y_regions_stats *out)
{
    const int rc = regions_check(nullptr, width, height, chroma_format_idc, radius);
    if (rc) return rc;
    if (!a || !b || !out) return fail(nullptr, H2Y_EINVAL, "null pointer");
    uint32_t off[3];
    contiguous_planes(width, height, chroma_format_idc, off);
    *out = h2y_regions_stats{};
    out->flat_var = flat_var;
    out->radius = (uint32_t)radius;
    for (int p = 0; p < 3; p++) {
        const plane_dim d = plane_dims(width, height, chroma_format_idc, p);
        regions_host_plane(a + off[p], b + off[p], (int)d.w, (int)d.h, flat_var, radius, p, out);
    }
    return H2Y_OK;
}

int h2y_regions_batch(h2y_ctx *ctx, int width, int height, int chroma_format_idc, uint32_t flat_var, int radius, int n_frames,
                      const uint16_t *const *d_a, const uint16_t *const *d_b, h2y_regions_stats *out)
{
    int rc = batch_enter(ctx);
    if (!rc) rc = regions_check(ctx, width, height, chroma_format_idc, radius);
    if (rc) return rc;
    uint32_t off[3];
    contiguous_planes(width, height, chroma_format_idc, off);
    const regions_geom g = regions_geom_of(width, height, chroma_format_idc, flat_var, radius, off, off);
    rc = pair_batch(ctx, n_frames, d_a, d_b, out, ctx->regions_stats, H2Y_REGIONS_FRAMES_PER_LAUNCH, "k_regions",
                    [&](int nf) { return regions_partials(ctx, g, nf); },
                    [&](const cmp_frame *frames, int f0, int nf) {
                        return h2y_launch_regions(h2y_regions_grid(ctx->n_cu, g, nf), ctx->stream, g, frames, nf, ctx->regions_part.p,
                                                  ctx->regions_stats.p + f0);
                    });
    if (rc) return rc;
    ctx->last_variant = std::string("k_regions<") + (chroma_format_idc == H2Y_CHROMA_420 ? "420" : "444") + ",R" + std::to_string(radius) + ">";
    return H2Y_OK;
}

/* The regions' ring stage: k_regions after k_compare (and k_ssim, k_deltae), on the comparison's table entry of the slot, the
 * frame's figures on the device and pinned */
struct regions_stage : result_stage<h2y_regions_stats> {
    regions_geom g{};
    const cmp_frame *tab = nullptr; /* the comparison's stage's */
    int run(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, h2y_launch_regions(h2y_regions_grid(ctx->n_cu, g, 1), ctx->stream, g, tab + k, 1, ctx->regions_part.p, ss[k].d));
        return H2Y_OK;
    }
};

int h2y_stream_regions(h2y_ctx *ctx, uint32_t flat_var, int radius)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    const cmp_stage *cmp = stage_of<cmp_stage>(ctx, STAGE_COMPARE);
    if (!cmp) return fail(ctx, H2Y_EINVAL, "the ring is not armed for comparison: h2y_stream_compare first");
    rc = arm_free(ctx, STAGE_REGIONS, "the ring measures flat and busy areas already");
    if (rc) return rc;
    const ring_frame &f = ctx->s_frame;
    rc = regions_check(ctx, f.width, f.height, f.chroma, radius);
    if (rc) return rc;
    auto st = std::make_unique<regions_stage>();
    st->g = regions_geom_of(f.width, f.height, f.chroma, flat_var, radius, f.off, f.off);
    st->tab = cmp->tab;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = regions_partials(ctx, st->g, 1);
    if (rc) return rc;
    st->slots(ctx->ss.size());
    return stage_arm(ctx, STAGE_REGIONS, std::move(st), "regions");
}

int h2y_stream_regions_result(h2y_ctx *ctx, h2y_regions_stats *out)
{
    return stream_result<regions_stage>(ctx, out, STAGE_REGIONS, "no stream open that measures flat and busy areas",
                                        [&](const regions_stage &st, int k) { *out = *st.ss[k].h; });
}

/* ---- content light level (MaxCLL / MaxFALL) of a forward conversion to PQ ------------------------------------------------------ */

/* the descriptors whose light is measured: conversions to PQ from another transfer, of a G, B, R source */
static int light_check(h2y_ctx *ctx, const h2y_desc *d)
{
    const char *why;
    int rc = h2y_desc_check(d, &why);
    if (rc) return fail(ctx, rc, "descriptor: %s", why);
    if (d->dst_transfer != 16)
        return fail(ctx, H2Y_EUNSUPPORTED, "content light is measured on conversions to PQ (dst_transfer 16), not dst_transfer %d", d->dst_transfer);
    if (d->src_transfer == 16)
        return fail(ctx, H2Y_EUNSUPPORTED, "a PQ source goes to PQ without linear light: there is no light to measure");
    if (d->src_matrix != H2Y_MATRIX_GBR)
        return fail(ctx, H2Y_EUNSUPPORTED, "content light needs a G,B,R source (src_matrix 0), not src_matrix %d", d->src_matrix);
    return H2Y_OK;
}

/* k_light's arguments for d: the conversion's parameters and, for a source transfer other than LINEAR, its stage's tables */
static int light_args_of(h2y_ctx *ctx, const h2y_desc *d, light_args &a)
{
    a = light_args{};
    derive_params(d, &a.pp, false);
    a.npix = (uint32_t)d->width * (uint32_t)d->height;
    a.n4 = a.npix / 4u;
    a.table = nullptr;
    if (a.pp.src_tf != H2Y_TF_LINEAR) {
        const int sf = kSrcFn[a.pp.src_tf]; /* h2y_shim.h */
        const int rc = ensure_tfn(ctx, sf);
        if (rc) return rc;
        a.pp.src_fn = sf;
        a.table = ctx->d_tfn[sf];
        a.pp.tf_ext[0] = ctx->d_tfn_ext[sf];
    }
    return H2Y_OK;
}

static std::string light_variant(const h2y_desc *d, const light_args &a)
{
    static const char *const kIn[] = {"F32", "F16", "U16"}, *const kTf[] = {"LINEAR", "PQ", "RHO_GAMMA", "BT1886"};
    return std::string("k_light<") + kIn[in_kind_of(d)] + "," + kTf[a.pp.src_tf] + ">";
}

/* the stats of one frame of npix pixels, width wide, from its accumulator */
static void light_finish(const light_acc &acc, uint32_t width, uint32_t npix, h2y_light_stats *o)
{
    *o = h2y_light_stats{};
    o->max_bits = (uint32_t)(acc.key >> 32);
    const uint32_t i = ~(uint32_t)acc.key;
    o->x = i % width;
    o->y = i / width;
    o->sum_q = acc.sum;
    o->pixels = npix;
    o->cll = 10000.0 * (double)bits2f(o->max_bits);
    o->fall = ((10000.0 * (double)acc.sum) * 0x1p-32) / (double)npix;
}

/* What h2y_light_batch and h2y_lightdist_batch share: the checks, k_light's arguments, every frame's floor and ceiling on the device
 * (light_as: the descriptor's override, or pic_stats of each frame) and the frame table h */
static int light_batch_prepare(h2y_ctx *ctx, const h2y_desc *d, int n_frames, const void *const *d_planes, const void *out, light_args &a,
                               light_frame *&h)
{
    int rc = batch_enter(ctx);
    if (!rc) rc = light_check(ctx, d);
    if (rc) return rc;
    if (n_frames < 1) return fail(ctx, H2Y_EINVAL, "n_frames must be >= 1");
    if (!d_planes || !out) return fail(ctx, H2Y_EINVAL, "null pointer arrays");
    for (int f = 0; f < n_frames; f++)
        for (int c = 0; c < 3; c++)
            if (!d_planes[3 * f + c] || ((uintptr_t)d_planes[3 * f + c] & 15u))
                return fail(ctx, H2Y_EINVAL, "input plane %d of frame %d is null or not 16-byte aligned", c, f);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = light_args_of(ctx, d, a);
    if (!rc) rc = frame_table(ctx, n_frames, h);
    if (!rc) rc = ensure(ctx, ctx->light_as, (size_t)n_frames * sizeof(assumed_stats));
    if (rc) return rc;
    assumed_stats *d_as = ctx->light_as.p;
    if (d->stats_override) { /* the same six integers for every frame */
        std::vector<assumed_stats> as(n_frames);
        for (auto &x : as)
            for (int c = 0; c < 3; c++) x.floor_[c] = d->floor[c], x.ceil_[c] = d->ceiling[c];
        HIP_TRY(ctx, hipMemcpyAsync(d_as, as.data(), (size_t)n_frames * sizeof(assumed_stats), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    } else /* pic_stats of every frame, as h2y_convert_batch ends up taking it */
        for (int f = 0; f < n_frames; f++) {
            rc = run_stats(ctx, d, d_planes + 3 * f, (int)ctx->b->frames_cap, d_as + f);
            if (rc) return rc;
        }
    ctx->b->dev_assumed_ok = false; /* run_stats used the batch state's scratch slot */
    for (int f = 0; f < n_frames; f++)
        h[f] = light_frame{{d_planes[3 * f], d_planes[3 * f + 1], d_planes[3 * f + 2]}, d_as + f};
    return H2Y_OK;
}

int h2y_light_batch(h2y_ctx *ctx, const h2y_desc *d, int n_frames, const void *const *d_planes, h2y_light_stats *out)
{
    light_args a;
    light_frame *h;
    int rc = light_batch_prepare(ctx, d, n_frames, d_planes, out, a, h);
    if (!rc) rc = ensure(ctx, ctx->light_accs, (size_t)n_frames * sizeof(light_acc));
    if (rc) return rc;
    light_acc *d_acc = ctx->light_accs.p;
    HIP_TRY(ctx, hipMemsetAsync(d_acc, 0, (size_t)n_frames * sizeof(light_acc), ctx->stream));
    const int in_kind = in_kind_of(d);
    rc = timed_launches(ctx, h, n_frames, H2Y_LIGHT_FRAMES_PER_LAUNCH, "k_light", [&](const light_frame *frames, int f0, int nf) {
        return h2y_launch_light(in_kind, h2y_light_grid(a.npix, nf), ctx->stream, a, frames, nf, d_acc + f0);
    });
    if (rc) return rc;
    std::vector<light_acc> acc(n_frames);
    HIP_TRY(ctx, hipMemcpy(acc.data(), d_acc, (size_t)n_frames * sizeof(light_acc), hipMemcpyDeviceToHost));
    for (int f = 0; f < n_frames; f++) light_finish(acc[f], (uint32_t)d->width, a.npix, out + f);
    ctx->last_variant = light_variant(d, a);
    return H2Y_OK;
}

/* Content light's ring stage, on the forward ring's decoded planes with the floor and ceiling the conversion just used
 * (d_assumed): k_light's arguments, its table entry per slot, and the frame's accumulator on the device and pinned */
struct light_stage : result_stage<light_acc> {
    light_args a{};
    light_frame *tab = nullptr;
    int run(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, hipMemsetAsync(ss[k].d, 0, sizeof(light_acc), ctx->stream));
        HIP_TRY(ctx, h2y_launch_light(in_kind_of(&ctx->s_desc), h2y_light_grid(a.npix, 1), ctx->stream, a, tab + k, 1, ss[k].d));
        return H2Y_OK;
    }
};

int h2y_stream_light(h2y_ctx *ctx)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    if (ctx->s_kind != h2y_ctx::RING_FORWARD) return fail(ctx, H2Y_EINVAL, "content light is measured on the forward rings only");
    rc = arm_free(ctx, STAGE_LIGHT, "the ring measures content light already");
    if (rc) return rc;
    const h2y_desc *d = &ctx->s_desc;
    rc = light_check(ctx, d);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto st = std::make_unique<light_stage>();
    rc = light_args_of(ctx, d, st->a);
    if (rc) return rc;
    st->slots(ctx->ss.size());
    st->table(st->tab, light_ring_table(ctx));
    return stage_arm(ctx, STAGE_LIGHT, std::move(st), "content light");
}

/* ---- light distribution (ST 2094-40 dynamic metadata) of a forward conversion to PQ ------------------------------------------- */

/* A workspace of nf frames: k_lightdist's accumulators, then the bins (both zeroed before a launch) */
struct lightdist_layout {
    size_t bins, total;
};
static lightdist_layout lightdist_layout_of(int nf)
{
    lightdist_layout L;
    L.bins = ((size_t)nf * sizeof(lightdist_acc) + 255) & ~(size_t)255;
    L.total = L.bins + (size_t)nf * H2Y_LIGHTDIST_BINS * sizeof(uint32_t);
    return L;
}

/* the stats of one frame of npix pixels from its accumulator and its bins: the finishing step runs here, on the host */
static void lightdist_finish(const lightdist_acc &acc, const uint32_t *bins, uint32_t npix, h2y_lightdist_stats *o)
{
    static const uint32_t kPct[H2Y_LIGHTDIST_PERCENTILES] = H2Y_LIGHTDIST_PCT;
    *o = h2y_lightdist_stats{};
    for (int c = 0; c < 3; c++) o->maxscl_bits[c] = acc.maxscl[c];
    o->max_bits = std::max(acc.maxscl[0], std::max(acc.maxscl[1], acc.maxscl[2]));
    o->sum_q = acc.sum;
    o->pixels = npix;
    o->below_100 = acc.below;
    uint64_t cum = 0;
    int i = 0;
    for (uint32_t k = 0; k < H2Y_LIGHTDIST_BINS && i < H2Y_LIGHTDIST_PERCENTILES; k++) {
        cum += bins[k];
        for (; i < H2Y_LIGHTDIST_PERCENTILES && cum * 10000u >= (uint64_t)kPct[i] * npix; i++)
            o->pct_bits[i] = k ? H2Y_LIGHTDIST_FIRST_BITS + ((k - 1u) << 14) : 0u;
    }
}

static std::string lightdist_variant(const h2y_desc *d, const light_args &a)
{
    return "k_lightdist" + light_variant(d, a).substr(strlen("k_light"));
}

int h2y_lightdist_batch(h2y_ctx *ctx, const h2y_desc *d, int n_frames, const void *const *d_planes, h2y_lightdist_stats *out,
                        uint32_t *bins_out)
{
    light_args a;
    light_frame *h;
    int rc = light_batch_prepare(ctx, d, n_frames, d_planes, out, a, h);
    const lightdist_layout L = lightdist_layout_of(n_frames > 0 ? n_frames : 1);
    if (!rc) rc = ensure(ctx, ctx->lightdist, L.total);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->lightdist.p, 0, L.total, ctx->stream));
    lightdist_acc *d_acc = reinterpret_cast<lightdist_acc *>(ctx->lightdist.p);
    uint32_t *d_bins = reinterpret_cast<uint32_t *>(ctx->lightdist.p + L.bins);
    const int in_kind = in_kind_of(d);
    rc = timed_launches(ctx, h, n_frames, H2Y_LIGHTDIST_FRAMES_PER_LAUNCH, "k_lightdist", [&](const light_frame *frames, int f0, int nf) {
        return h2y_launch_lightdist(in_kind, h2y_lightdist_grid(a.npix, nf), ctx->stream, a, frames, nf, d_acc + f0,
                                    d_bins + (size_t)f0 * H2Y_LIGHTDIST_BINS);
    });
    if (rc) return rc;
    std::vector<lightdist_acc> acc(n_frames);
    std::vector<uint32_t> own(bins_out ? 0 : (size_t)n_frames * H2Y_LIGHTDIST_BINS);
    uint32_t *bins = bins_out ? bins_out : own.data();
    HIP_TRY(ctx, hipMemcpy(acc.data(), d_acc, (size_t)n_frames * sizeof(lightdist_acc), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(bins, d_bins, (size_t)n_frames * H2Y_LIGHTDIST_BINS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int f = 0; f < n_frames; f++) lightdist_finish(acc[f], bins + (size_t)f * H2Y_LIGHTDIST_BINS, a.npix, out + f);
    ctx->last_variant = lightdist_variant(d, a);
    return H2Y_OK;
}

/* The light distribution's ring stage, on what content light's stage sees: k_light's arguments and table entry per slot, and the
 * frame's workspace (lightdist_layout of one frame) on the device and pinned */
struct lightdist_stage : ring_stage {
    struct slot {
        char *d = nullptr, *h = nullptr;
    };
    std::vector<slot> ss;
    light_args a{};
    light_frame *tab = nullptr;
    int run(h2y_ctx *ctx, int k) override
    {
        const lightdist_layout L = lightdist_layout_of(1);
        HIP_TRY(ctx, hipMemsetAsync(ss[k].d, 0, L.total, ctx->stream));
        HIP_TRY(ctx, h2y_launch_lightdist(in_kind_of(&ctx->s_desc), h2y_lightdist_grid(a.npix, 1), ctx->stream, a, tab + k, 1,
                                          reinterpret_cast<lightdist_acc *>(ss[k].d), reinterpret_cast<uint32_t *>(ss[k].d + L.bins)));
        return H2Y_OK;
    }
    int download(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, hipMemcpyAsync(ss[k].h, ss[k].d, lightdist_layout_of(1).total, hipMemcpyDeviceToHost, ctx->s_d2h));
        return H2Y_OK;
    }
};

int h2y_stream_lightdist(h2y_ctx *ctx)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    if (ctx->s_kind != h2y_ctx::RING_FORWARD) return fail(ctx, H2Y_EINVAL, "the light distribution is measured on the forward rings only");
    rc = arm_free(ctx, STAGE_LIGHTDIST, "the ring measures the light distribution already");
    if (rc) return rc;
    const h2y_desc *d = &ctx->s_desc;
    rc = light_check(ctx, d);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto st = std::make_unique<lightdist_stage>();
    rc = light_args_of(ctx, d, st->a);
    if (rc) return rc;
    const lightdist_layout L = lightdist_layout_of(1);
    st->ss.resize(ctx->ss.size());
    for (auto &s : st->ss) {
        st->dev_alloc(s.d, L.total);
        st->pin_alloc(s.h, L.total);
    }
    st->table(st->tab, light_ring_table(ctx));
    return stage_arm(ctx, STAGE_LIGHTDIST, std::move(st), "light distribution");
}

/* 0.1 cd/m2 of a light L in [0, 1] given as bits: rint(100000 x (double)L), half to even */
static long lightdist_units(uint32_t bits) { return lrint(100000.0 * (double)bits2f(bits)); }

size_t h2y_lightdist_json(const h2y_lightdist_stats *stats, int n_frames, long first_frame_index, char *buf, size_t cap)
{
    if (!stats || n_frames < 1 || first_frame_index < 0) return 0;
    for (int k = 0; k < n_frames; k++)
        if (!stats[k].pixels) return 0;
    std::string s = "{\"JSONInfo\": {\"HDR10plusProfile\": \"A\", \"Version\": \"1.0\"},\n\"SceneInfo\": [\n";
    char line[1024];
    for (int k = 0; k < n_frames; k++) {
        const h2y_lightdist_stats &t = stats[k];
        const long avg = lrint(((100000.0 * (double)t.sum_q) * 0x1p-32) / (double)t.pixels);
        const long share = (long)(100u * t.below_100 / t.pixels);
        const uint32_t *p = t.pct_bits; /* 1, 5, 10, 25, 50, 75, 90, 95, 99, 99.98 % */
        snprintf(line, sizeof line,
                 "{\"LuminanceParameters\": {\"AverageRGB\": %ld, \"LuminanceDistributions\": {\"DistributionIndex\": [1, 5, 10, 25, 50, 75, 90, "
                 "95, 99], \"DistributionValues\": [%ld, %ld, %ld, %ld, %ld, %ld, %ld, %ld, %ld]}, \"MaxScl\": [%ld, %ld, %ld]}, "
                 "\"NumberOfWindows\": 1, \"TargetedSystemDisplayMaximumLuminance\": 400, \"SceneFrameIndex\": %d, \"SceneId\": 0, "
                 "\"SequenceFrameIndex\": %ld}%s\n",
                 avg, lightdist_units(p[0]), lightdist_units(p[9]), share, lightdist_units(p[3]), lightdist_units(p[4]), lightdist_units(p[5]),
                 lightdist_units(p[6]), lightdist_units(p[7]), lightdist_units(p[8]), lightdist_units(t.maxscl_bits[2]),
                 lightdist_units(t.maxscl_bits[0]), lightdist_units(t.maxscl_bits[1]), k, first_frame_index + k, k + 1 < n_frames ? "," : "");
        s += line;
    }
    snprintf(line, sizeof line, "],\n\"SceneInfoSummary\": {\"SceneFirstFrameIndex\": [%ld], \"SceneFrameNumbers\": [%d]},\n"
             "\"ToolInfo\": {\"Tool\": \"hdr2yuv\", \"Version\": \"1.0\"}}\n", first_frame_index, n_frames);
    s += line;
    if (buf && cap) {
        const size_t n = std::min(s.size(), cap - 1);
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return s.size();
}

/* ---- light of PQ code planes (h2y_codelight_batch, h2y_codelight_stream_open): include/hdr2yuv_hip.h states the definition ------ */

/* what codelight_check refuses of the descriptor alone, without a context: the host twin of k_code_signal refuses the same */
static int codelight_desc_check(h2y_ctx *ctx, const h2y_codelight_desc *d)
{
    if (!d) return fail(ctx, H2Y_EINVAL, "null h2y_codelight_desc");
    if (d->chroma_format_idc == 2) return fail(ctx, H2Y_EUNSUPPORTED, "chroma_format_idc 2 (4:2:2) has no light on this path");
    if (d->chroma_format_idc != H2Y_CHROMA_420 && d->chroma_format_idc != H2Y_CHROMA_444)
        return fail(ctx, H2Y_EINVAL, "chroma_format_idc must be 1 or 3");
    if (d->matrix_coeffs != H2Y_MATRIX_GBR && d->matrix_coeffs != H2Y_MATRIX_BT709 && d->matrix_coeffs != H2Y_MATRIX_BT2020NC &&
        d->matrix_coeffs != H2Y_MATRIX_ICTCP)
        return fail(ctx, H2Y_EUNSUPPORTED, "light of code planes: matrix_coeffs must be 0 (G,B,R), 1 (BT.709), 9 (BT.2020nc) or 14 (ICtCp), not %d", d->matrix_coeffs);
    int rc = picture_size_check(ctx, d->width, d->height);
    if (rc) return rc;
    if (d->bit_depth < 8 || d->bit_depth > 16) return fail(ctx, H2Y_EINVAL, "bit_depth must be 8..16");
    if (d->full_range != 0 && d->full_range != 1) return fail(ctx, H2Y_EINVAL, "full_range must be 0 or 1");
    if (d->chroma_format_idc == H2Y_CHROMA_420) {
        if (d->matrix_coeffs == H2Y_MATRIX_GBR) return fail(ctx, H2Y_EINVAL, "G,B,R planes (matrix_coeffs 0) are 4:4:4");
        if ((d->width & 1) || (d->height & 1) || d->width > 32766 || d->height > 32766)
            return fail(ctx, H2Y_EINVAL, "4:2:0: width and height must be even, up to 32766");
    }
    return H2Y_OK;
}

/* step 2's constants: what a code of plane 0 (G, B, R planes: of every plane) and of planes 1 and 2 is taken from and divided by */
static void codelight_norm(const h2y_codelight_desc *d, codelight_args &a)
{
    const float s = (float)(1u << (d->bit_depth - 8)), top = (float)((1u << d->bit_depth) - 1u);
    a.sub[0] = d->full_range ? 0.0f : 16.0f * s;
    a.div[0] = d->full_range ? top : 219.0f * s;
    a.sub[1] = d->full_range ? (float)(1u << (d->bit_depth - 1)) : 128.0f * s;
    a.div[1] = d->full_range ? top : 224.0f * s;
}

int codelight_check(h2y_ctx *ctx, const h2y_codelight_desc *d, codelight_plan &p)
{
    int rc = codelight_desc_check(ctx, d);
    if (rc) return rc;
    p.sub = d->chroma_format_idc == H2Y_CHROMA_420;
    rc = inverse_form(ctx, d->chroma_format_idc, d->algorithm, &p.form); /* siting 2 with replication: the inverse entries' refusal */
    if (rc) return rc;
    p.matrix = d->matrix_coeffs;
    codelight_args &a = p.a;
    a.npix = (uint32_t)d->width * (uint32_t)d->height;
    a.n8 = a.npix / 8u;
    codelight_norm(d, a);
    contiguous_planes(d->width, d->height, d->chroma_format_idc, p.off);
    p.width = d->width, p.height = d->height, p.bit_depth = d->bit_depth;
    p.samples = p.off[2] + (p.off[2] - p.off[1]); /* the last plane is as long as the second */
    /* the frames' bases are 16-byte aligned, and so is the scratch: a plane takes 16-byte loads where its start is */
    a.vec = 1u;
    for (int c = 1; c < 3; c++) a.vec |= (p.sub || ((size_t)p.off[c] * sizeof(uint16_t) & 15u) == 0) ? 1u << c : 0u;
    if (p.sub) {
        inv420_args ia;
        inverse420_setup(ia, d->width, d->height, d->bit_depth, d->full_range, d->matrix_coeffs, d->bit_depth, p.form);
        p.up = ia.up;
        p.plane_al = ((size_t)a.npix * sizeof(uint16_t) + 255) & ~(size_t)255;
    }
    return H2Y_OK;
}

/* PQ10000_f's tables into the plan: what light1<true> reads of pix_params */
int codelight_tables(h2y_ctx *ctx, codelight_plan &p)
{
    const int rc = ensure_tfn(ctx, H2Y_TFN_PQ_F);
    if (rc) return rc;
    pix_params &pp = p.a.pp;
    pp = pix_params{};
    pp.convert_transfer = 2;
    pp.src_tf = H2Y_TF_PQ;
    pp.src_fn = H2Y_TFN_PQ_F;
    pp.norm_identity = 1; /* the kernel normalises the codes itself */
    for (int c = 0; c < 3; c++) pp.range[c] = 1.0f;
    pp.tf_ext[0] = ctx->d_tfn_ext[H2Y_TFN_PQ_F];
    p.a.table = ctx->d_tfn[H2Y_TFN_PQ_F];
    return H2Y_OK;
}

static const char *matrix_name(int matrix)
{
    return matrix == H2Y_MATRIX_GBR ? "GBR" : matrix == H2Y_MATRIX_BT709 ? "BT709" : matrix == H2Y_MATRIX_ICTCP ? "ICTCP" : "BT2020NC";
}

static std::string codelight_variant(const codelight_plan &p, bool dist)
{
    return std::string("k_codelight<") + matrix_name(p.matrix) +
           (dist ? ",DIST," : ",LIGHT,") + (!p.sub ? "444" : p.form == UP_FIR_TL ? "FIR_TL" : p.form == UP_FIR ? "FIR" : "REPLICATE") + ">";
}

/* one 4:2:0 frame's chroma (planes at p.off[1], p.off[2] of base) upsampled into the two planes at up */
static hipError_t codelight_upsample(const h2y_ctx *ctx, const codelight_plan &p, const uint16_t *base, char *up)
{
    up_args u = p.up;
    u.src0 = base + p.off[1];
    u.src1 = base + p.off[2];
    u.dst0 = reinterpret_cast<uint16_t *>(up);
    u.dst1 = reinterpret_cast<uint16_t *>(up + p.plane_al);
    return h2y_launch_up444(ctx->stream, u);
}

/* the frame's table entry: its own planes, or its luma and the upsampled chroma at up */
static codelight_frame codelight_entry(const codelight_plan &p, const uint16_t *base, const char *up)
{
    if (!p.sub) return codelight_frame{{base, base + p.off[1], base + p.off[2]}};
    return codelight_frame{{base, reinterpret_cast<const uint16_t *>(up), reinterpret_cast<const uint16_t *>(up + p.plane_al)}};
}

/* A workspace of nf frames: light_acc, then lightdist_layout (all zeroed before a launch) */
static size_t codelight_dist_off(int nf) { return ((size_t)nf * sizeof(light_acc) + 255) & ~(size_t)255; }

int h2y_codelight_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, int n_frames, const uint16_t *const *d_frames, h2y_light_stats *out,
                        h2y_lightdist_stats *dist_out, uint32_t *bins_out)
{
    codelight_plan p;
    int rc = batch_enter(ctx);
    if (!rc) rc = codelight_check(ctx, d, p);
    if (!rc) rc = frames_check(ctx, n_frames, d_frames, out != nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool dist = dist_out || bins_out;
    const int per_launch = std::min(n_frames, H2Y_CODELIGHT_FRAMES_PER_LAUNCH);
    const lightdist_layout L = lightdist_layout_of(n_frames);
    const size_t dist_off = codelight_dist_off(n_frames), ws = dist_off + (dist ? L.total : 0);
    codelight_frame *h;
    rc = codelight_tables(ctx, p);
    if (!rc) rc = frame_table(ctx, n_frames, h);
    if (!rc) rc = ensure(ctx, ctx->codelight, ws);
    if (!rc && p.sub) rc = ensure(ctx, ctx->codelight_up, (size_t)per_launch * 2u * p.plane_al);
    if (rc) return rc;
    char *d_ws = ctx->codelight.p, *d_up = ctx->codelight_up.p;
    /* frame f's upsampled chroma lies in the scratch of its place in its launch; the launches follow one another on one stream */
    for (int f = 0; f < n_frames; f++) h[f] = codelight_entry(p, d_frames[f], p.sub ? d_up + (size_t)(f % per_launch) * 2u * p.plane_al : nullptr);
    HIP_TRY(ctx, hipMemsetAsync(d_ws, 0, ws, ctx->stream));
    light_acc *d_acc = reinterpret_cast<light_acc *>(d_ws);
    lightdist_acc *d_dacc = dist ? reinterpret_cast<lightdist_acc *>(d_ws + dist_off) : nullptr;
    uint32_t *d_bins = dist ? reinterpret_cast<uint32_t *>(d_ws + dist_off + L.bins) : nullptr;
    rc = timed_launches(ctx, h, n_frames, H2Y_CODELIGHT_FRAMES_PER_LAUNCH, "k_codelight", [&](const codelight_frame *frames, int f0, int nf) {
        for (int f = 0; p.sub && f < nf; f++) {
            const hipError_t e = codelight_upsample(ctx, p, d_frames[f0 + f], d_up + (size_t)f * 2u * p.plane_al);
            if (e != hipSuccess) return e;
        }
        return h2y_launch_codelight(p.matrix, h2y_codelight_grid(p.a.npix, nf), ctx->stream, p.a, frames, nf, d_acc + f0,
                                    dist ? d_dacc + f0 : nullptr, dist ? d_bins + (size_t)f0 * H2Y_LIGHTDIST_BINS : nullptr);
    });
    if (rc) return rc;
    std::vector<light_acc> acc(n_frames);
    HIP_TRY(ctx, hipMemcpy(acc.data(), d_acc, (size_t)n_frames * sizeof(light_acc), hipMemcpyDeviceToHost));
    for (int f = 0; f < n_frames; f++) light_finish(acc[f], (uint32_t)d->width, p.a.npix, out + f);
    if (dist) {
        std::vector<lightdist_acc> dacc(n_frames);
        std::vector<uint32_t> own(bins_out ? 0 : (size_t)n_frames * H2Y_LIGHTDIST_BINS);
        uint32_t *bins = bins_out ? bins_out : own.data();
        HIP_TRY(ctx, hipMemcpy(dacc.data(), d_dacc, (size_t)n_frames * sizeof(lightdist_acc), hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(bins, d_bins, (size_t)n_frames * H2Y_LIGHTDIST_BINS * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (int f = 0; dist_out && f < n_frames; f++) lightdist_finish(dacc[f], bins + (size_t)f * H2Y_LIGHTDIST_BINS, p.a.npix, dist_out + f);
    }
    ctx->last_variant = codelight_variant(p, dist);
    return H2Y_OK;
}

/* The light-only ring's stage, on the planes the ring's input holds: per slot the upsampled chroma (4:2:0), the workspace of one
 * frame on the device and pinned, and the slot's k_codelight table entry */
struct codelight_stage : ring_stage {
    struct slot {
        char *up = nullptr, *d = nullptr, *h = nullptr;
    };
    std::vector<slot> ss;
    codelight_plan p;
    bool dist = false;
    size_t ws = 0;
    codelight_frame *tab = nullptr;
    int run(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, hipMemsetAsync(ss[k].d, 0, ws, ctx->stream));
        if (p.sub) HIP_TRY(ctx, codelight_upsample(ctx, p, frame_base(ctx, k), ss[k].up));
        const size_t off = codelight_dist_off(1);
        HIP_TRY(ctx, h2y_launch_codelight(p.matrix, h2y_codelight_grid(p.a.npix, 1), ctx->stream, p.a, tab + k, 1,
                                          reinterpret_cast<light_acc *>(ss[k].d), dist ? reinterpret_cast<lightdist_acc *>(ss[k].d + off) : nullptr,
                                          dist ? reinterpret_cast<uint32_t *>(ss[k].d + off + lightdist_layout_of(1).bins) : nullptr));
        return H2Y_OK;
    }
    int download(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, hipMemcpyAsync(ss[k].h, ss[k].d, ws, hipMemcpyDeviceToHost, ctx->s_d2h));
        return H2Y_OK;
    }
};

/* The light and the distribution of the frame handed out last: a forward ring's stages', or the light-only ring's */
int h2y_stream_light_result(h2y_ctx *ctx, h2y_light_stats *out)
{
    if (!ctx || !out) return fail(ctx, H2Y_EINVAL, "null argument");
    const light_stage *st = ctx->streaming ? stage_of<light_stage>(ctx, STAGE_LIGHT) : nullptr;
    const codelight_stage *cl = ctx->streaming ? stage_of<codelight_stage>(ctx, STAGE_CODELIGHT) : nullptr;
    if (!st && !cl) return fail(ctx, H2Y_EINVAL, "no stream open that measures content light");
    const int rc = output_taken(ctx);
    if (rc) return rc;
    if (cl) light_finish(*reinterpret_cast<const light_acc *>(cl->ss[ctx->s_lent].h), (uint32_t)ctx->s_frame.width, cl->p.a.npix, out);
    else light_finish(*st->ss[ctx->s_lent].h, (uint32_t)ctx->s_desc.width, st->a.npix, out);
    return H2Y_OK;
}

int h2y_stream_lightdist_result(h2y_ctx *ctx, h2y_lightdist_stats *out)
{
    if (!ctx || !out) return fail(ctx, H2Y_EINVAL, "null argument");
    const codelight_stage *cl = ctx->streaming ? stage_of<codelight_stage>(ctx, STAGE_CODELIGHT) : nullptr;
    const lightdist_stage *st = ctx->streaming ? stage_of<lightdist_stage>(ctx, STAGE_LIGHTDIST) : nullptr;
    if (cl && !cl->dist) return fail(ctx, H2Y_EINVAL, "the light-only ring was opened without want_dist");
    if (!cl && !st) return fail(ctx, H2Y_EINVAL, "no stream open that measures the light distribution");
    const int rc = output_taken(ctx);
    if (rc) return rc;
    const char *h = cl ? cl->ss[ctx->s_lent].h + codelight_dist_off(1) : st->ss[ctx->s_lent].h;
    lightdist_finish(*reinterpret_cast<const lightdist_acc *>(h), reinterpret_cast<const uint32_t *>(h + lightdist_layout_of(1).bins),
                     cl ? cl->p.a.npix : st->a.npix, out);
    return H2Y_OK;
}

int h2y_codelight_stream_open(h2y_ctx *ctx, const h2y_codelight_desc *d, int want_dist, int depth)
{
    int rc = ring_may_open(ctx);
    if (rc) return rc;
    auto st = std::make_unique<codelight_stage>();
    rc = codelight_check(ctx, d, st->p); /* the inverse chroma siting is read here */
    if (rc) return rc;
    if (want_dist != 0 && want_dist != 1) return fail(ctx, H2Y_EINVAL, "want_dist must be 0 or 1");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = codelight_tables(ctx, st->p);
    if (!rc) rc = open_planes_ring(ctx, d->width, d->height, d->chroma_format_idc, d->bit_depth, d->full_range, d->matrix_coeffs == H2Y_MATRIX_GBR, 0, depth);
    if (rc) return rc;
    st->dist = want_dist != 0;
    st->ws = codelight_dist_off(1) + (st->dist ? lightdist_layout_of(1).total : 0);
    std::vector<codelight_frame> tab(depth);
    st->ss.resize(depth);
    for (int k = 0; k < depth; k++) {
        codelight_stage::slot &s = st->ss[k];
        if (st->p.sub) st->dev_alloc(s.up, 2u * st->p.plane_al);
        st->dev_alloc(s.d, st->ws);
        st->pin_alloc(s.h, st->ws);
        tab[k] = codelight_entry(st->p, frame_base(ctx, k), s.up);
    }
    st->table(st->tab, tab);
    rc = stage_arm(ctx, STAGE_CODELIGHT, std::move(st), "code light");
    if (rc) stream_free(ctx);
    return rc;
}

/* ---- gamut containment of PQ code planes (h2y_gamutcheck_planes, h2y_gamutcheck_batch, h2y_stream_gamutcheck): include/hdr2yuv_hip.h
 * states the definition --------------------------------------------------------------------------------------------------------------- */

/* a checked request: the sets as given, their matrices, t and a */
struct gamutcheck_plan {
    int n_sets = 0;
    int sets[H2Y_GAMUTCHECK_MAX_SETS] = {0, 0};
    float m[H2Y_GAMUTCHECK_MAX_SETS][9] = {};
    float t = 0.0f, a = 0.0f;
};

/* the refusals of the check's own arguments, in the order every entry reports them */
static int gamutcheck_check(h2y_ctx *ctx, int file_primaries, int n_sets, const int *sets, double ratio, double floor, gamutcheck_plan &g)
{
    if (n_sets < 1 || n_sets > H2Y_GAMUTCHECK_MAX_SETS) return fail(ctx, H2Y_EINVAL, "gamut check: n_sets must be 1..%d, not %d", H2Y_GAMUTCHECK_MAX_SETS, n_sets);
    if (!sets) return fail(ctx, H2Y_EINVAL, "gamut check: null sets");
    if (!(ratio >= 0.0 && ratio <= 1.0)) return fail(ctx, H2Y_EINVAL, "gamut check: ratio must be 0..1, not %g", ratio);
    if (!(floor >= 0.0) || !std::isfinite(floor)) return fail(ctx, H2Y_EINVAL, "gamut check: floor must be a finite number of cd/m2, 0 or more, not %g", floor);
    auto same = [](int a, int b) { return (a == 8 ? 9 : a) == (b == 8 ? 9 : b); };
    for (int s = 0; s < n_sets; s++) {
        if (file_primaries == 10 || sets[s] == 10)
            return fail(ctx, H2Y_EUNSUPPORTED, "gamut check %d against %d: XYZ (colour primaries 10) has no gamut to be contained in", file_primaries, sets[s]);
        const char *why;
        const int rc = h2y_gamut_matrix(file_primaries, sets[s], g.m[s], &why);
        if (rc) return fail(ctx, rc, "gamut check %d against %d: %s", file_primaries, sets[s], why);
        for (int u = 0; u < s; u++)
            if (same(sets[u], sets[s])) return fail(ctx, H2Y_EINVAL, "gamut check: set %d is listed twice", sets[s]);
        g.sets[s] = sets[s];
    }
    g.n_sets = n_sets;
    g.t = (float)ratio;
    g.a = (float)(floor / 10000.0);
    return H2Y_OK;
}

/* a frame's accumulators into the caller's struct: the doubles of step 5 */
static void gamutcheck_finish(const gamutcheck_plan &g, const gamutcheck_frame_acc &acc, uint32_t width, uint32_t npix, h2y_gamutcheck_stats *out)
{
    memset(out, 0, sizeof *out);
    out->pixels = npix;
    out->n_sets = g.n_sets;
    for (int s = 0; s < g.n_sets; s++) {
        const gamutcheck_acc &a = acc.set[s];
        h2y_gamutcheck_set &o = out->set[s];
        o.primaries = g.sets[s];
        o.max_bits = (uint32_t)(a.key >> 32);
        const uint32_t index = ~(uint32_t)a.key;
        o.max_x = a.outside ? (int32_t)(index % width) : -1;
        o.max_y = a.outside ? (int32_t)(index / width) : -1;
        o.outside = a.outside, o.beyond = a.beyond, o.sum_q = a.sum;
        float e;
        memcpy(&e, &o.max_bits, sizeof e);
        o.max_cdm2 = 10000.0 * (double)e;
        o.mean_cdm2 = ((10000.0 * (double)a.sum) * 0x1p-32) / (double)npix;
        o.beyond_share = (double)a.beyond / (double)npix;
    }
}

int h2y_gamutcheck_planes(int file_primaries, int n_sets, const int *sets, double ratio, double floor, int width, int height,
                          const float *const lights[3], h2y_gamutcheck_stats *out)
{
    gamutcheck_plan g;
    int rc = gamutcheck_check(nullptr, file_primaries, n_sets, sets, ratio, floor, g);
    if (!rc) rc = picture_size_check(nullptr, width, height);
    if (rc) return rc;
    if (!lights || !lights[0] || !lights[1] || !lights[2] || !out) return fail(nullptr, H2Y_EINVAL, "null argument");
    const uint32_t npix = (uint32_t)width * (uint32_t)height;
    gamutcheck_regs k[H2Y_GAMUTCHECK_MAX_SETS] = {};
    for (uint32_t i = 0; i < npix; i++) {
        const float lg = lights[0][i], lb = lights[1][i], lr = lights[2][i], mx = fmaxf(fmaxf(lg, lb), lr);
        if (!(lg >= 0.0f && lg <= 1.0f && lb >= 0.0f && lb <= 1.0f && lr >= 0.0f && lr <= 1.0f)) /* a NaN too: e < 1 rests on it */
            return fail(nullptr, H2Y_EINVAL, "gamut check: pixel %u holds a light outside [0, 1]", i);
        for (int s = 0; s < g.n_sets; s++) gamutcheck_keep(g.m[s], g.t, g.a, lg, lb, lr, mx, i, k[s]);
    }
    gamutcheck_frame_acc acc{};
    for (int s = 0; s < g.n_sets; s++) acc.set[s] = gamutcheck_acc{k[s].key, k[s].sum, k[s].outside, k[s].beyond};
    gamutcheck_finish(g, acc, (uint32_t)width, npix, out);
    return H2Y_OK;
}

/* k_gamutcheck's arguments: the plan's codelight_args (tables set) and the check's */
static gamutcheck_args gamutcheck_args_of(const codelight_plan &p, const gamutcheck_plan &g)
{
    gamutcheck_args a{};
    a.c = p.a;
    a.n_sets = (uint32_t)g.n_sets;
    memcpy(a.m, g.m, sizeof a.m);
    a.t = g.t, a.a = g.a;
    return a;
}

int h2y_gamutcheck_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, int file_primaries, int n_sets, const int *sets, double ratio,
                         double floor, int n_frames, const uint16_t *const *d_frames, h2y_gamutcheck_stats *out)
{
    codelight_plan p;
    gamutcheck_plan g;
    int rc = batch_enter(ctx);
    if (!rc) rc = codelight_check(ctx, d, p);
    if (!rc) rc = gamutcheck_check(ctx, file_primaries, n_sets, sets, ratio, floor, g);
    if (!rc) rc = frames_check(ctx, n_frames, d_frames, out != nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int per_launch = std::min(n_frames, H2Y_CODELIGHT_FRAMES_PER_LAUNCH);
    codelight_frame *h;
    rc = codelight_tables(ctx, p);
    if (!rc) rc = frame_table(ctx, n_frames, h);
    if (!rc) rc = ensure(ctx, ctx->gamutcheck, (size_t)n_frames * sizeof(gamutcheck_frame_acc));
    if (!rc && p.sub) rc = ensure(ctx, ctx->codelight_up, (size_t)per_launch * 2u * p.plane_al);
    if (rc) return rc;
    gamutcheck_frame_acc *d_acc = ctx->gamutcheck.p;
    char *d_up = ctx->codelight_up.p;
    for (int f = 0; f < n_frames; f++) /* as h2y_codelight_batch: the upsampled chroma in the scratch of the frame's place in its launch */
        h[f] = codelight_entry(p, d_frames[f], p.sub ? d_up + (size_t)(f % per_launch) * 2u * p.plane_al : nullptr);
    HIP_TRY(ctx, hipMemsetAsync(d_acc, 0, (size_t)n_frames * sizeof(gamutcheck_frame_acc), ctx->stream));
    const gamutcheck_args a = gamutcheck_args_of(p, g);
    rc = timed_launches(ctx, h, n_frames, H2Y_CODELIGHT_FRAMES_PER_LAUNCH, "k_gamutcheck", [&](const codelight_frame *frames, int f0, int nf) {
        for (int f = 0; p.sub && f < nf; f++) {
            const hipError_t e = codelight_upsample(ctx, p, d_frames[f0 + f], d_up + (size_t)f * 2u * p.plane_al);
            if (e != hipSuccess) return e;
        }
        return h2y_launch_gamutcheck(p.matrix, h2y_codelight_grid(p.a.npix, nf), ctx->stream, a, frames, nf, d_acc + f0);
    });
    if (rc) return rc;
    std::vector<gamutcheck_frame_acc> acc(n_frames);
    HIP_TRY(ctx, hipMemcpy(acc.data(), d_acc, (size_t)n_frames * sizeof(gamutcheck_frame_acc), hipMemcpyDeviceToHost));
    for (int f = 0; f < n_frames; f++) gamutcheck_finish(g, acc[f], (uint32_t)d->width, p.a.npix, out + f);
    ctx->last_variant = std::string("k_gamutcheck<") + matrix_name(p.matrix) + "," + std::to_string(g.n_sets) + "," +
                        (!p.sub ? "444" : p.form == UP_FIR_TL ? "FIR_TL" : p.form == UP_FIR ? "FIR" : "REPLICATE") + ">";
    return H2Y_OK;
}

/* The check's stage on the light-only ring: k_gamutcheck on the planes of the ring's codelight_stage, which ran before it (stage_id
 * order) and left the slot's upsampled chroma where its table entry points.  Per slot the frame's accumulators on the device and
 * pinned. */
struct gamutcheck_stage : result_stage<gamutcheck_frame_acc> {
    gamutcheck_plan g;
    gamutcheck_args a{};
    int run(h2y_ctx *ctx, int k) override
    {
        const codelight_stage *cl = stage_of<codelight_stage>(ctx, STAGE_CODELIGHT);
        HIP_TRY(ctx, hipMemsetAsync(ss[k].d, 0, sizeof(gamutcheck_frame_acc), ctx->stream));
        HIP_TRY(ctx, h2y_launch_gamutcheck(cl->p.matrix, h2y_codelight_grid(a.c.npix, 1), ctx->stream, a, cl->tab + k, 1, ss[k].d));
        return H2Y_OK;
    }
};

int h2y_stream_gamutcheck(h2y_ctx *ctx, int file_primaries, int n_sets, const int *sets, double ratio, double floor)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    const codelight_stage *cl = stage_of<codelight_stage>(ctx, STAGE_CODELIGHT);
    if (!cl) return fail(ctx, H2Y_EINVAL, "gamut containment is checked on the light-only ring only");
    rc = arm_free(ctx, STAGE_GAMUTCHECK, "the ring checks gamut containment already");
    if (rc) return rc;
    auto st = std::make_unique<gamutcheck_stage>();
    rc = gamutcheck_check(ctx, file_primaries, n_sets, sets, ratio, floor, st->g);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    st->a = gamutcheck_args_of(cl->p, st->g);
    st->slots(ctx->ss.size());
    return stage_arm(ctx, STAGE_GAMUTCHECK, std::move(st), "gamut check");
}

int h2y_stream_gamutcheck_result(h2y_ctx *ctx, h2y_gamutcheck_stats *out)
{
    return stream_result<gamutcheck_stage>(ctx, out, STAGE_GAMUTCHECK, "no stream open that checks gamut containment",
                                           [&](const gamutcheck_stage &st, int k) {
                                               gamutcheck_finish(st.g, *st.ss[k].h, (uint32_t)ctx->s_frame.width, st.a.c.npix, out);
                                           });
}

/* ---- scene signature and scene cuts (h2y_scenesig_batch, h2y_codescenesig_batch, h2y_stream_scenesig, and the host-only merge and
 * JSON): include/hdr2yuv_hip.h states the definition ---------------------------------------------------------------------------- */

constexpr size_t kSigCells = H2Y_SCENESIG_COLS * H2Y_SCENESIG_ROWS, kSigBytes = kSigCells * sizeof(unsigned long long);

/* n_frames frames' cells from the device into out, each with its pixel count */
static int scenesig_finish(h2y_ctx *ctx, const unsigned long long *d_sig, int n_frames, uint32_t npix, h2y_scenesig *out)
{
    std::vector<unsigned long long> cells((size_t)n_frames * kSigCells);
    HIP_TRY(ctx, hipMemcpy(cells.data(), d_sig, cells.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int f = 0; f < n_frames; f++) {
        for (size_t c = 0; c < kSigCells; c++) out[f].cell[c] = cells[(size_t)f * kSigCells + c];
        out[f].pixels = npix;
    }
    return H2Y_OK;
}

int h2y_scenesig_batch(h2y_ctx *ctx, const h2y_desc *d, int n_frames, const void *const *d_planes, h2y_scenesig *out)
{
    light_args a;
    light_frame *h;
    int rc = light_batch_prepare(ctx, d, n_frames, d_planes, out, a, h);
    if (!rc) rc = ensure(ctx, ctx->scenesig, (size_t)n_frames * kSigBytes);
    if (rc) return rc;
    unsigned long long *d_sig = ctx->scenesig.p;
    HIP_TRY(ctx, hipMemsetAsync(d_sig, 0, (size_t)n_frames * kSigBytes, ctx->stream));
    const int in_kind = in_kind_of(d);
    rc = timed_launches(ctx, h, n_frames, H2Y_SCENESIG_FRAMES_PER_LAUNCH, "k_scenesig", [&](const light_frame *frames, int f0, int nf) {
        return h2y_launch_scenesig(in_kind, ctx->stream, a, h2y_scenesig_geom((uint32_t)d->width, (uint32_t)d->height, 4u, nf), frames, nf,
                                   d_sig + (size_t)f0 * kSigCells);
    });
    if (!rc) rc = scenesig_finish(ctx, d_sig, n_frames, a.npix, out);
    if (rc) return rc;
    ctx->last_variant = "k_scenesig" + light_variant(d, a).substr(strlen("k_light"));
    return H2Y_OK;
}

int h2y_codescenesig_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, int n_frames, const uint16_t *const *d_frames, h2y_scenesig *out)
{
    codelight_plan p;
    int rc = batch_enter(ctx);
    if (!rc) rc = codelight_check(ctx, d, p);
    if (!rc) rc = frames_check(ctx, n_frames, d_frames, out != nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int per_launch = std::min(n_frames, H2Y_CODELIGHT_FRAMES_PER_LAUNCH);
    codelight_frame *h;
    rc = codelight_tables(ctx, p);
    if (!rc) rc = frame_table(ctx, n_frames, h);
    if (!rc) rc = ensure(ctx, ctx->scenesig, (size_t)n_frames * kSigBytes);
    if (!rc && p.sub) rc = ensure(ctx, ctx->codelight_up, (size_t)per_launch * 2u * p.plane_al);
    if (rc) return rc;
    unsigned long long *d_sig = ctx->scenesig.p;
    char *d_up = ctx->codelight_up.p;
    for (int f = 0; f < n_frames; f++) /* as h2y_codelight_batch: the upsampled chroma in the scratch of the frame's place in its launch */
        h[f] = codelight_entry(p, d_frames[f], p.sub ? d_up + (size_t)(f % per_launch) * 2u * p.plane_al : nullptr);
    HIP_TRY(ctx, hipMemsetAsync(d_sig, 0, (size_t)n_frames * kSigBytes, ctx->stream));
    rc = timed_launches(ctx, h, n_frames, H2Y_CODELIGHT_FRAMES_PER_LAUNCH, "k_codescenesig", [&](const codelight_frame *frames, int f0, int nf) {
        for (int f = 0; p.sub && f < nf; f++) {
            const hipError_t e = codelight_upsample(ctx, p, d_frames[f0 + f], d_up + (size_t)f * 2u * p.plane_al);
            if (e != hipSuccess) return e;
        }
        return h2y_launch_codescenesig(p.matrix, ctx->stream, p.a, h2y_scenesig_geom((uint32_t)p.width, (uint32_t)p.height, 8u, nf), frames, nf,
                                       d_sig + (size_t)f0 * kSigCells);
    });
    if (!rc) rc = scenesig_finish(ctx, d_sig, n_frames, p.a.npix, out);
    if (rc) return rc;
    ctx->last_variant = std::string("k_codescenesig<") + matrix_name(p.matrix) + "," +
                        (!p.sub ? "444" : p.form == UP_FIR_TL ? "FIR_TL" : p.form == UP_FIR ? "FIR" : "REPLICATE") + ">";
    return H2Y_OK;
}

/* The signature's ring stage.  On a forward ring: k_scenesig on what the light distribution's stage sees, with k_light's arguments
 * and table entry per slot.  On the light-only ring: k_codescenesig on the planes of the ring's codelight_stage, which ran before it
 * (stage_id order) and left the slot's upsampled chroma where its table entry points.  Per slot the frame's cells on the device and
 * pinned. */
struct scenesig_stage : ring_stage {
    struct slot {
        unsigned long long *d = nullptr, *h = nullptr;
    };
    std::vector<slot> ss;
    bool code = false;
    uint32_t npix = 0;
    scenesig_geom g{};
    light_args a{};
    light_frame *tab = nullptr;
    int run(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, hipMemsetAsync(ss[k].d, 0, kSigBytes, ctx->stream));
        if (code) {
            const codelight_stage *cl = stage_of<codelight_stage>(ctx, STAGE_CODELIGHT);
            HIP_TRY(ctx, h2y_launch_codescenesig(cl->p.matrix, ctx->stream, cl->p.a, g, cl->tab + k, 1, ss[k].d));
        } else HIP_TRY(ctx, h2y_launch_scenesig(in_kind_of(&ctx->s_desc), ctx->stream, a, g, tab + k, 1, ss[k].d));
        return H2Y_OK;
    }
    int download(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, hipMemcpyAsync(ss[k].h, ss[k].d, kSigBytes, hipMemcpyDeviceToHost, ctx->s_d2h));
        return H2Y_OK;
    }
};

int h2y_stream_scenesig(h2y_ctx *ctx)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    const codelight_stage *cl = stage_of<codelight_stage>(ctx, STAGE_CODELIGHT);
    if (!cl && ctx->s_kind != h2y_ctx::RING_FORWARD)
        return fail(ctx, H2Y_EINVAL, "the scene signature is measured on the forward rings and the light-only ring only");
    rc = arm_free(ctx, STAGE_SCENESIG, "the ring measures the scene signature already");
    if (rc) return rc;
    auto st = std::make_unique<scenesig_stage>();
    const int depth = (int)ctx->ss.size();
    if (cl) {
        st->code = true;
        st->npix = cl->p.a.npix;
        st->g = h2y_scenesig_geom((uint32_t)cl->p.width, (uint32_t)cl->p.height, 8u, 1);
        HIP_TRY(ctx, hipSetDevice(ctx->device));
    } else {
        const h2y_desc *d = &ctx->s_desc;
        rc = light_check(ctx, d);
        if (rc) return rc;
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        rc = light_args_of(ctx, d, st->a);
        if (rc) return rc;
        st->npix = st->a.npix;
        st->g = h2y_scenesig_geom((uint32_t)d->width, (uint32_t)d->height, 4u, 1);
    }
    st->ss.resize(depth);
    for (int k = 0; k < depth; k++) {
        st->dev_alloc(st->ss[k].d, kSigBytes);
        st->pin_alloc(st->ss[k].h, kSigBytes);
    }
    if (!cl) st->table(st->tab, light_ring_table(ctx));
    return stage_arm(ctx, STAGE_SCENESIG, std::move(st), "scene signature");
}

int h2y_stream_scenesig_result(h2y_ctx *ctx, h2y_scenesig *out)
{
    return stream_result<scenesig_stage>(ctx, out, STAGE_SCENESIG, "no stream open that measures the scene signature",
                                         [&](const scenesig_stage &st, int k) {
                                             for (size_t c = 0; c < kSigCells; c++) out->cell[c] = st.ss[k].h[c];
                                             out->pixels = st.npix;
                                         });
}

int h2y_stream_lightdist_bins(h2y_ctx *ctx, uint32_t *bins)
{
    if (!ctx || !bins) return fail(ctx, H2Y_EINVAL, "null argument");
    const codelight_stage *cl = ctx->streaming ? stage_of<codelight_stage>(ctx, STAGE_CODELIGHT) : nullptr;
    const lightdist_stage *st = ctx->streaming ? stage_of<lightdist_stage>(ctx, STAGE_LIGHTDIST) : nullptr;
    if (!(cl && cl->dist) && !st) return fail(ctx, H2Y_EINVAL, "no stream open that measures the light distribution");
    const int rc = output_taken(ctx);
    if (rc) return rc;
    const char *h = cl ? cl->ss[ctx->s_lent].h + codelight_dist_off(1) : st->ss[ctx->s_lent].h;
    memcpy(bins, h + lightdist_layout_of(1).bins, H2Y_LIGHTDIST_BINS * sizeof(uint32_t));
    return H2Y_OK;
}

double h2y_scene_distance(const h2y_scenesig *a, const h2y_scenesig *b)
{
    if (!a || !b || !a->pixels || a->pixels != b->pixels) return -1.0;
    uint64_t s = 0;
    for (size_t c = 0; c < kSigCells; c++) s += a->cell[c] > b->cell[c] ? a->cell[c] - b->cell[c] : b->cell[c] - a->cell[c];
    return (double)s / (512.0 * (double)a->pixels);
}

int h2y_scene_cuts(const h2y_scenesig *sig, int n, double threshold, int32_t *scene_id)
{
    if (!sig || !scene_id || n < 1 || !(threshold >= 0.0) || !std::isfinite(threshold)) return 0;
    int32_t s = 0;
    scene_id[0] = 0;
    for (int f = 1; f < n; f++) {
        if (h2y_scene_distance(&sig[f - 1], &sig[f]) > threshold) s++;
        scene_id[f] = s;
    }
    return s + 1;
}

int h2y_scene_merge(const h2y_lightdist_stats *stats, const uint32_t *bins, const int32_t *scene_id, int n_frames, h2y_scene_stats *out, int cap)
{
    static const uint32_t kPct[H2Y_LIGHTDIST_PERCENTILES] = H2Y_LIGHTDIST_PCT;
    if (!stats || !bins || !scene_id || n_frames < 1 || cap < 0 || (cap > 0 && !out) || scene_id[0] != 0) return 0;
    for (int f = 0; f < n_frames; f++)
        if (!stats[f].pixels || (f > 0 && scene_id[f] != scene_id[f - 1] && scene_id[f] != scene_id[f - 1] + 1)) return 0;
    std::vector<uint64_t> sum(H2Y_LIGHTDIST_BINS);
    int scenes = 0;
    for (int f0 = 0; f0 < n_frames; scenes++) {
        int f1 = f0 + 1;
        while (f1 < n_frames && scene_id[f1] == scene_id[f0]) f1++;
        if (scenes < cap) {
            h2y_scene_stats &o = out[scenes];
            o = h2y_scene_stats{};
            o.first_frame = f0, o.n_frames = f1 - f0;
            unsigned __int128 q = 0;
            std::fill(sum.begin(), sum.end(), 0u);
            for (int f = f0; f < f1; f++) {
                for (int c = 0; c < 3; c++) o.maxscl_bits[c] = std::max(o.maxscl_bits[c], stats[f].maxscl_bits[c]);
                o.max_bits = std::max(o.max_bits, stats[f].max_bits);
                q += stats[f].sum_q;
                o.pixels += stats[f].pixels, o.below_100 += stats[f].below_100;
                const uint32_t *b = bins + (size_t)f * H2Y_LIGHTDIST_BINS;
                for (uint32_t k = 0; k < H2Y_LIGHTDIST_BINS; k++) sum[k] += b[k];
            }
            o.sum_q_hi = (uint64_t)(q >> 64), o.sum_q_lo = (uint64_t)q;
            uint64_t cum = 0;
            int i = 0;
            for (uint32_t k = 0; k < H2Y_LIGHTDIST_BINS && i < H2Y_LIGHTDIST_PERCENTILES; k++) { /* lightdist_finish's rule */
                cum += sum[k];
                for (; i < H2Y_LIGHTDIST_PERCENTILES && cum * 10000u >= (uint64_t)kPct[i] * o.pixels; i++)
                    o.pct_bits[i] = k ? H2Y_LIGHTDIST_FIRST_BITS + ((k - 1u) << 14) : 0u;
            }
        }
        f0 = f1;
    }
    return scenes;
}

size_t h2y_lightdist_json_scenes(const h2y_scene_stats *scenes, int n_scenes, long first_frame_index, char *buf, size_t cap)
{
    if (!scenes || n_scenes < 1 || first_frame_index < 0) return 0;
    int64_t at = 0;
    for (int s = 0; s < n_scenes; s++) {
        if (!scenes[s].pixels || scenes[s].n_frames < 1 || scenes[s].first_frame != at) return 0;
        at += scenes[s].n_frames;
    }
    std::string text = "{\"JSONInfo\": {\"HDR10plusProfile\": \"A\", \"Version\": \"1.0\"},\n\"SceneInfo\": [\n";
    std::string firsts, counts;
    char line[1024];
    for (int s = 0; s < n_scenes; s++) {
        const h2y_scene_stats &t = scenes[s];
        const unsigned __int128 q = ((unsigned __int128)t.sum_q_hi << 64) | t.sum_q_lo;
        const long avg = lrint(((100000.0 * (double)q) * 0x1p-32) / (double)t.pixels); /* h2y_lightdist_json's order of operations */
        const long share = (long)((unsigned __int128)100u * t.below_100 / t.pixels);
        const uint32_t *p = t.pct_bits;
        for (int64_t k = 0; k < t.n_frames; k++) {
            const bool last = s + 1 == n_scenes && k + 1 == t.n_frames;
            snprintf(line, sizeof line,
                     "{\"LuminanceParameters\": {\"AverageRGB\": %ld, \"LuminanceDistributions\": {\"DistributionIndex\": [1, 5, 10, 25, 50, 75, 90, "
                     "95, 99], \"DistributionValues\": [%ld, %ld, %ld, %ld, %ld, %ld, %ld, %ld, %ld]}, \"MaxScl\": [%ld, %ld, %ld]}, "
                     "\"NumberOfWindows\": 1, \"TargetedSystemDisplayMaximumLuminance\": 400, \"SceneFrameIndex\": %lld, \"SceneId\": %d, "
                     "\"SequenceFrameIndex\": %lld}%s\n",
                     avg, lightdist_units(p[0]), lightdist_units(p[9]), share, lightdist_units(p[3]), lightdist_units(p[4]), lightdist_units(p[5]),
                     lightdist_units(p[6]), lightdist_units(p[7]), lightdist_units(p[8]), lightdist_units(t.maxscl_bits[2]),
                     lightdist_units(t.maxscl_bits[0]), lightdist_units(t.maxscl_bits[1]), (long long)k, s,
                     (long long)(first_frame_index + t.first_frame + k), last ? "" : ",");
            text += line;
        }
        firsts += (s ? ", " : "") + std::to_string(first_frame_index + t.first_frame);
        counts += (s ? ", " : "") + std::to_string(t.n_frames);
    }
    text += "],\n\"SceneInfoSummary\": {\"SceneFirstFrameIndex\": [" + firsts + "], \"SceneFrameNumbers\": [" + counts +
            "]},\n\"ToolInfo\": {\"Tool\": \"hdr2yuv\", \"Version\": \"1.0\"}}\n";
    if (buf && cap) {
        const size_t n = std::min(text.size(), cap - 1);
        memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return text.size();
}

/* ---- Delta E ITP of PQ code planes (h2y_deltae_batch, h2y_stream_deltae): include/hdr2yuv_hip.h states the definition ------------- */

/* k_deltae's arguments from a checked plan: k_codelight's, and PQ10000_r's tables, what code1 reads of pix_params */
static int deltae_args_of(h2y_ctx *ctx, codelight_plan &p, float threshold, deltae_args &a)
{
    if (!(threshold >= 0.0f)) return fail(ctx, H2Y_EINVAL, "the Delta E threshold must be a number >= 0");
    int rc = codelight_tables(ctx, p);
    if (!rc) rc = ensure_tfn(ctx, H2Y_TFN_PQ_R);
    if (rc) return rc;
    a.c = p.a;
    a.c.pp.dst_tf = H2Y_TF_PQ;
    a.c.pp.dst_fn = H2Y_TFN_PQ_R;
    a.c.pp.tf_ext[1] = ctx->d_tfn_ext[H2Y_TFN_PQ_R];
    a.table_r = ctx->d_tfn[H2Y_TFN_PQ_R];
    a.threshold = threshold;
    return H2Y_OK;
}

static std::string deltae_variant(const codelight_plan &p)
{
    return std::string("k_deltae<") + matrix_name(p.matrix) + "," +
           (!p.sub ? "444" : p.form == UP_FIR_TL ? "FIR_TL" : p.form == UP_FIR ? "FIR" : "REPLICATE") + ">";
}

/* one 4:2:0 pair's chroma (A's planes a1, a2, B's b1, b2) upsampled into the four planes at up */
static hipError_t deltae_upsample(const h2y_ctx *ctx, const codelight_plan &p, const uint16_t *a1, const uint16_t *a2, const uint16_t *b1,
                                  const uint16_t *b2, char *up)
{
    up_args u = p.up;
    u.src0 = a1, u.src1 = a2;
    u.dst0 = reinterpret_cast<uint16_t *>(up);
    u.dst1 = reinterpret_cast<uint16_t *>(up + p.plane_al);
    const hipError_t e = h2y_launch_up444(ctx->stream, u);
    if (e != hipSuccess) return e;
    u.src0 = b1, u.src1 = b2;
    u.dst0 = reinterpret_cast<uint16_t *>(up + 2u * p.plane_al);
    u.dst1 = reinterpret_cast<uint16_t *>(up + 3u * p.plane_al);
    return h2y_launch_up444(ctx->stream, u);
}

/* the pair's table entry: the two frames' own planes (off[] samples from their bases), or their lumas and the upsampled chroma at up */
static deltae_frame deltae_entry(const codelight_plan &p, const uint32_t off[3], const uint16_t *a, const uint16_t *b, const char *up)
{
    if (!p.sub) return deltae_frame{{a, a + off[1], a + off[2]}, {b, b + off[1], b + off[2]}};
    const uint16_t *u = reinterpret_cast<const uint16_t *>(up);
    const size_t n = p.plane_al / sizeof(uint16_t);
    return deltae_frame{{a, u, u + n}, {b, u + 2u * n, u + 3u * n}};
}

/* the stats of one frame of npix pixels, width wide, from its accumulator */
static void deltae_finish(const deltae_acc &acc, uint32_t width, uint32_t npix, float threshold, h2y_deltae_stats *o)
{
    *o = h2y_deltae_stats{};
    o->max_bits = (uint32_t)(acc.key >> 32);
    const uint32_t i = ~(uint32_t)acc.key;
    o->max_x = i % width;
    o->max_y = i / width;
    o->threshold = threshold;
    o->sum_q = acc.sum;
    o->pixels = npix;
    o->over = acc.over;
    o->mean = ((double)acc.sum * 0x1p-20) / (double)npix;
    o->max = (double)bits2f(o->max_bits);
}

int h2y_deltae_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, float threshold, int n_frames, const uint16_t *const *d_a,
                     const uint16_t *const *d_b, h2y_deltae_stats *out)
{
    codelight_plan p;
    int rc = batch_enter(ctx);
    if (!rc) rc = codelight_check(ctx, d, p);
    if (!rc) rc = pairs_check(ctx, n_frames, d_a, d_b, out != nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int per_launch = std::min(n_frames, H2Y_DELTAE_FRAMES_PER_LAUNCH);
    deltae_args a;
    deltae_frame *h;
    rc = deltae_args_of(ctx, p, threshold, a);
    if (!rc) rc = frame_table(ctx, n_frames, h);
    if (!rc) rc = ensure(ctx, ctx->deltae, (size_t)n_frames * sizeof(deltae_acc));
    if (!rc && p.sub) rc = ensure(ctx, ctx->codelight_up, (size_t)per_launch * 4u * p.plane_al);
    if (rc) return rc;
    deltae_acc *d_acc = ctx->deltae.p;
    char *d_up = ctx->codelight_up.p;
    /* pair f's upsampled chroma lies in the scratch of its place in its launch; the launches follow one another on one stream */
    for (int f = 0; f < n_frames; f++)
        h[f] = deltae_entry(p, p.off, d_a[f], d_b[f], p.sub ? d_up + (size_t)(f % per_launch) * 4u * p.plane_al : nullptr);
    HIP_TRY(ctx, hipMemsetAsync(d_acc, 0, (size_t)n_frames * sizeof(deltae_acc), ctx->stream));
    rc = timed_launches(ctx, h, n_frames, H2Y_DELTAE_FRAMES_PER_LAUNCH, "k_deltae", [&](const deltae_frame *frames, int f0, int nf) {
        for (int f = 0; p.sub && f < nf; f++) {
            const uint16_t *xa = d_a[f0 + f], *xb = d_b[f0 + f];
            const hipError_t e = deltae_upsample(ctx, p, xa + p.off[1], xa + p.off[2], xb + p.off[1], xb + p.off[2], d_up + (size_t)f * 4u * p.plane_al);
            if (e != hipSuccess) return e;
        }
        return h2y_launch_deltae(p.matrix, h2y_deltae_grid(a.c.npix, nf), ctx->stream, a, frames, nf, d_acc + f0);
    });
    if (rc) return rc;
    std::vector<deltae_acc> acc(n_frames);
    HIP_TRY(ctx, hipMemcpy(acc.data(), d_acc, (size_t)n_frames * sizeof(deltae_acc), hipMemcpyDeviceToHost));
    for (int f = 0; f < n_frames; f++) deltae_finish(acc[f], (uint32_t)d->width, a.c.npix, threshold, out + f);
    ctx->last_variant = deltae_variant(p);
    return H2Y_OK;
}

/* Delta E's ring stage: k_deltae after k_compare and k_ssim, on the slot's frame and its reference twin (the comparison's table
 * entry).  One scratch serves every slot's four upsampled planes: the frames follow one another on the context's stream.  Per slot
 * the pair's accumulator on the device and pinned, and its k_deltae table entry */
struct deltae_stage : ring_stage {
    struct slot {
        deltae_acc *d = nullptr, *h = nullptr;
        const uint16_t *a = nullptr, *b = nullptr;
    };
    std::vector<slot> ss;
    codelight_plan p;
    deltae_args a{};
    uint32_t off[3] = {0, 0, 0}; /* the ring frame's planes */
    char *up = nullptr;
    deltae_frame *tab = nullptr;
    int run(h2y_ctx *ctx, int k) override
    {
        const slot &s = ss[k];
        HIP_TRY(ctx, hipMemsetAsync(s.d, 0, sizeof(deltae_acc), ctx->stream));
        if (p.sub) HIP_TRY(ctx, deltae_upsample(ctx, p, s.a + off[1], s.a + off[2], s.b + off[1], s.b + off[2], up));
        HIP_TRY(ctx, h2y_launch_deltae(p.matrix, h2y_deltae_grid(a.c.npix, 1), ctx->stream, a, tab + k, 1, s.d));
        return H2Y_OK;
    }
    int download(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, hipMemcpyAsync(ss[k].h, ss[k].d, sizeof(deltae_acc), hipMemcpyDeviceToHost, ctx->s_d2h));
        return H2Y_OK;
    }
};

int h2y_stream_deltae(h2y_ctx *ctx, const h2y_codelight_desc *d, float threshold)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    if (ctx->s_stage[STAGE_CODELIGHT]) return fail(ctx, H2Y_EINVAL, "a light-only ring takes no other stage");
    if (ctx->s_stage[STAGE_DITHER]) return fail(ctx, H2Y_EUNSUPPORTED, "a ring that dithers computes no Delta E: compare the written file instead");
    if (ctx->s_stage[STAGE_PACK]) return fail(ctx, H2Y_EUNSUPPORTED, "a ring that packs computes no Delta E: compare the written file instead");
    const cmp_stage *cmp = stage_of<cmp_stage>(ctx, STAGE_COMPARE);
    if (!cmp) return fail(ctx, H2Y_EINVAL, "the ring is not armed for comparison: h2y_stream_compare first");
    rc = arm_free(ctx, STAGE_DELTAE, "the ring computes Delta E already");
    if (rc) return rc;
    auto st = std::make_unique<deltae_stage>();
    rc = codelight_check(ctx, d, st->p); /* the inverse chroma siting is read here */
    if (rc) return rc;
    const ring_frame &f = ctx->s_frame;
    if (d->width != f.width || d->height != f.height || d->chroma_format_idc != f.chroma)
        return fail(ctx, H2Y_EINVAL, "Delta E: the descriptor is %dx%d chroma_format_idc %d, the ring's frame %dx%d chroma_format_idc %d", d->width,
                    d->height, d->chroma_format_idc, f.width, f.height, f.chroma);
    /* a forward ring's planes are G, B, R where its conversion's matrix is the identity */
    const bool gbr = ctx->s_kind == h2y_ctx::RING_FORWARD ? ctx->s_desc.dst_matrix == H2Y_MATRIX_GBR : f.gbr;
    if (f.depth && (d->bit_depth != f.depth || d->full_range != f.full_range || (d->matrix_coeffs == H2Y_MATRIX_GBR) != gbr))
        return fail(ctx, H2Y_EINVAL, "Delta E: the descriptor (bit_depth %d, full_range %d, matrix_coeffs %d) is not the ring's frame (bit_depth %d, full_range %d, %s)",
                    d->bit_depth, d->full_range, d->matrix_coeffs, f.depth, f.full_range, gbr ? "G,B,R" : "Y,Cb,Cr");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = deltae_args_of(ctx, st->p, threshold, st->a);
    if (rc) return rc;
    /* the ring's planes, not the contiguous ones of the plan: a plane takes 16-byte loads where it starts 16-byte aligned in both frames */
    st->a.c.vec = 1u;
    for (int c = 0; c < 3; c++) {
        st->off[c] = f.off[c];
        if (c) st->a.c.vec |= (st->p.sub || (((size_t)f.off[c] * sizeof(uint16_t)) & 15u) == 0) ? 1u << c : 0u;
    }
    const int depth = (int)ctx->ss.size();
    if (st->p.sub) st->dev_alloc(st->up, 4u * st->p.plane_al);
    std::vector<deltae_frame> tab(depth);
    st->ss.resize(depth);
    for (int k = 0; k < depth; k++) {
        deltae_stage::slot &s = st->ss[k];
        st->dev_alloc(s.d, sizeof(deltae_acc));
        st->pin_alloc(s.h, sizeof(deltae_acc));
        s.a = frame_base(ctx, k);
        s.b = reinterpret_cast<const uint16_t *>(cmp->ss[k].d_ref);
        tab[k] = deltae_entry(st->p, st->off, s.a, s.b, st->up);
    }
    st->table(st->tab, tab);
    return stage_arm(ctx, STAGE_DELTAE, std::move(st), "Delta E");
}

int h2y_stream_deltae_result(h2y_ctx *ctx, h2y_deltae_stats *out)
{
    return stream_result<deltae_stage>(ctx, out, STAGE_DELTAE, "no stream open that computes Delta E", [&](const deltae_stage &st, int k) {
        deltae_finish(*st.ss[k].h, (uint32_t)ctx->s_frame.width, st.a.c.npix, st.a.threshold, out);
    });
}

/* ---- linearised PQ code planes (h2y_linearize_batch, h2y_pqcode_stream_open): include/hdr2yuv_hip.h states the definition ------ */

static const char *linearize_kernel(code_tf tf)
{
    return tf.kind == code_tf::HLG ? "k_hlg_linearize" : tf.kind == code_tf::SDR ? "k_sdr_linearize" : tf.kind == code_tf::SIGNAL ? "k_code_signal" : "k_linearize";
}

static std::string linearize_variant(const codelight_plan &p, code_tf tf)
{
    return std::string(linearize_kernel(tf)) + "<" + matrix_name(p.matrix) + "," +
           (!p.sub ? "444" : p.form == UP_FIR_TL ? "FIR_TL" : p.form == UP_FIR ? "FIR" : "REPLICATE") + ">";
}

/* the frame's table entry: codelight_entry's planes, and the three output planes */
static linearize_frame linearize_entry(const codelight_plan &p, const uint16_t *base, const char *up, void *const out[3])
{
    const codelight_frame c = codelight_entry(p, base, up);
    return linearize_frame{{c.p[0], c.p[1], c.p[2]}, {static_cast<float *>(out[0]), static_cast<float *>(out[1]), static_cast<float *>(out[2])}};
}

/* the four batch entries: the codes are PQ's (k_linearize), HLG's at a display peak (k_hlg_linearize), SDR's at a reference
 * white (k_sdr_linearize), or stay signal whatever they are (k_code_signal) */
static int linearize_frames(h2y_ctx *ctx, const h2y_codelight_desc *d, code_tf tf, int n_frames, const uint16_t *const *d_frames,
                            void *const *d_planes_out)
{
    codelight_plan p;
    int rc = batch_enter(ctx);
    if (!rc) rc = codelight_check(ctx, d, p);
    if (!rc)
        rc = frames_check(ctx, n_frames, d_frames, d_planes_out != nullptr, [&](int f) {
            for (int c = 0; c < 3; c++) {
                if (!d_planes_out[3 * f + c]) return fail(ctx, H2Y_EINVAL, "frame %d: output plane %d is null", f, c);
                if ((uintptr_t)d_planes_out[3 * f + c] & 15u) return fail(ctx, H2Y_EINVAL, "frame %d: output plane %d is not 16-byte aligned", f, c);
            }
            return (int)H2Y_OK;
        });
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int per_launch = std::min(n_frames, H2Y_LINEARIZE_FRAMES_PER_LAUNCH);
    linearize_frame *h;
    hlgsrc_args ha{};
    sdrsrc_args sa{};
    rc = tf.kind == code_tf::HLG ? hlgsrc_args_of(ctx, p, tf.param, ha) : tf.kind == code_tf::SDR ? sdrsrc_tables(ctx, p, tf.param, sa.kappa) :
         tf.kind == code_tf::SIGNAL ? sigsrc_check(ctx, p) : codelight_tables(ctx, p);
    sa.c = p.a;
    if (!rc) rc = frame_table(ctx, n_frames, h);
    if (!rc && p.sub) rc = ensure(ctx, ctx->codelight_up, (size_t)per_launch * 2u * p.plane_al);
    if (rc) return rc;
    char *d_up = ctx->codelight_up.p;
    /* frame f's upsampled chroma lies in the scratch of its place in its launch; the launches follow one another on one stream */
    for (int f = 0; f < n_frames; f++)
        h[f] = linearize_entry(p, d_frames[f], p.sub ? d_up + (size_t)(f % per_launch) * 2u * p.plane_al : nullptr, d_planes_out + 3 * f);
    rc = timed_launches(ctx, h, n_frames, H2Y_LINEARIZE_FRAMES_PER_LAUNCH, linearize_kernel(tf), [&](const linearize_frame *frames, int f0, int nf) {
        for (int f = 0; p.sub && f < nf; f++) {
            const hipError_t e = codelight_upsample(ctx, p, d_frames[f0 + f], d_up + (size_t)f * 2u * p.plane_al);
            if (e != hipSuccess) return e;
        }
        if (tf.kind == code_tf::HLG) return h2y_launch_hlg_linearize(p.matrix, h2y_hlg_linearize_grid(ctx->n_cu, p.a.npix, nf), ctx->stream, ha, frames, nf);
        if (tf.kind == code_tf::SDR) return h2y_launch_sdr_linearize(p.matrix, h2y_sdr_linearize_grid(p.a.npix, nf), ctx->stream, sa, frames, nf);
        if (tf.kind == code_tf::SIGNAL) return h2y_launch_code_signal(p.matrix, h2y_code_signal_grid(p.a.npix, nf), ctx->stream, p.a, frames, nf);
        return h2y_launch_linearize(p.matrix, h2y_linearize_grid(p.a.npix, nf), ctx->stream, p.a, frames, nf);
    });
    if (rc) return rc;
    ctx->last_variant = linearize_variant(p, tf);
    return H2Y_OK;
}

int h2y_linearize_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, int n_frames, const uint16_t *const *d_frames, void *const *d_planes_out)
{
    return linearize_frames(ctx, d, code_tf{}, n_frames, d_frames, d_planes_out);
}

int h2y_hlg_linearize_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, int peak, int n_frames, const uint16_t *const *d_frames,
                            void *const *d_planes_out)
{
    return linearize_frames(ctx, d, code_tf{code_tf::HLG, peak}, n_frames, d_frames, d_planes_out);
}

int h2y_sdr_linearize_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, int white, int n_frames, const uint16_t *const *d_frames,
                            void *const *d_planes_out)
{
    return linearize_frames(ctx, d, code_tf{code_tf::SDR, white}, n_frames, d_frames, d_planes_out);
}

int h2y_code_signal_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, int n_frames, const uint16_t *const *d_frames, void *const *d_planes_out)
{
    return linearize_frames(ctx, d, code_tf{code_tf::SIGNAL, 0}, n_frames, d_frames, d_planes_out);
}

/* The forward ring's PQCODE decode.  One scratch of the context serves every slot: the frames follow one another on its stream. */
int pqcode_scratch(h2y_ctx *ctx, const codelight_plan &p)
{
    return p.sub ? ensure(ctx, ctx->codelight_up, 2u * p.plane_al) : H2Y_OK;
}

linearize_frame pqcode_entry(const h2y_ctx *ctx, const codelight_plan &p, const char *payload, char *const planes[3])
{
    void *const out[3] = {planes[0], planes[1], planes[2]};
    return linearize_entry(p, reinterpret_cast<const uint16_t *>(payload), ctx->codelight_up.p, out);
}

int pqcode_decode(h2y_ctx *ctx, int slot)
{
    const codelight_plan &p = ctx->s_src.code;
    if (p.sub)
        HIP_TRY(ctx, codelight_upsample(ctx, p, reinterpret_cast<const uint16_t *>(ctx->ss[slot].d_in + ctx->s_pay_off), ctx->codelight_up.p));
    const linearize_frame *fr = static_cast<const linearize_frame *>(ctx->s_tab) + slot;
    if (ctx->s_src.hlg) HIP_TRY(ctx, h2y_launch_hlg_linearize(p.matrix, h2y_hlg_linearize_grid(ctx->n_cu, p.a.npix, 1), ctx->stream, ctx->s_src.hlgsrc, fr, 1));
    else if (ctx->s_src.sdr) HIP_TRY(ctx, h2y_launch_sdr_linearize(p.matrix, h2y_sdr_linearize_grid(p.a.npix, 1), ctx->stream, sdrsrc_args{p.a, ctx->s_src.sdr_kappa}, fr, 1));
    else if (ctx->s_src.signal) HIP_TRY(ctx, h2y_launch_code_signal(p.matrix, h2y_code_signal_grid(p.a.npix, 1), ctx->stream, p.a, fr, 1));
    else HIP_TRY(ctx, h2y_launch_linearize(p.matrix, h2y_linearize_grid(p.a.npix, 1), ctx->stream, p.a, fr, 1));
    return H2Y_OK;
}

/* ---- code-value histograms and the legal-range check (hdr2yuv.cpp:658, :797) ---------------------------------------------- */

/* k_histogram's geometry: planes of the comparison's geometry starting at off samples from the frame's base, the legal range of
 * set_pic_clip() at bit_depth (planes 1 and 2 of a YCbCr frame: minVRC..maxVRC; plane 0 and every G, B, R plane: minVR..maxVR) */
static hist_geom hist_geom_of(int width, int height, int chroma, int bit_depth, int full_range, int gbr, int bits, const uint32_t off[3])
{
    hist_geom g{};
    const clip_limits c = make_clip(bit_depth, full_range);
    for (int p = 0; p < 3; p++) {
        const plane_dim d = plane_dims(width, height, chroma, p);
        g.n[p] = d.w * d.h;
        g.off[p] = off[p];
        g.shift[p] = off[p] & 7u;
        g.vec |= 1u << p; /* one side: the groups can always follow the plane's start */
        g.units[p] = h2y_histogram_units(g.n[p], g.shift[p]);
        const bool luma_like = p == 0 || gbr;
        g.lo[p] = luma_like ? c.minVR : c.minVRC;
        g.hi[p] = luma_like ? c.maxVR : c.maxVRC;
    }
    g.nbins = 1u << bits;
    g.down = (uint32_t)(bit_depth - bits);
    return g;
}

static int hist_check(h2y_ctx *ctx, int width, int height, int chroma, int bit_depth, int full_range, int gbr, int bits)
{
    const int rc = picture_size_check(ctx, width, height);
    if (rc) return rc;
    if (chroma == 2) return fail(ctx, H2Y_EUNSUPPORTED, "chroma_format_idc 2 (4:2:2) is not counted on this path");
    if (chroma != H2Y_CHROMA_420 && chroma != H2Y_CHROMA_444) return fail(ctx, H2Y_EINVAL, "chroma_format_idc must be 1 or 3");
    if (bit_depth < 8 || bit_depth > 16) return fail(ctx, H2Y_EINVAL, "bit_depth must be 8..16");
    if (bits < 1 || bits > bit_depth) return fail(ctx, H2Y_EINVAL, "bits must be 1..bit_depth (%d)", bit_depth);
    if ((full_range != 0 && full_range != 1) || (gbr != 0 && gbr != 1)) return fail(ctx, H2Y_EINVAL, "full_range and gbr must be 0 or 1");
    return H2Y_OK;
}

/* A workspace of nf frames: the counts (zeroed), the bins (zeroed), then the stats k_histogram_finish writes */
struct hist_layout {
    size_t bins, stats, total;
};
static hist_layout hist_layout_of(uint32_t nbins, int nf)
{
    hist_layout L;
    L.bins = ((size_t)nf * 3u * sizeof(hist_acc) + 255) & ~(size_t)255;
    L.stats = (L.bins + (size_t)nf * 3u * nbins * sizeof(uint32_t) + 255) & ~(size_t)255;
    L.total = L.stats + (size_t)nf * sizeof(h2y_histogram_stats);
    return L;
}

/* the zeroing and both kernels of nf frames on the context's stream, into the workspace ws */
static int hist_enqueue(h2y_ctx *ctx, const hist_geom &g, const hist_frame *frames, int nf, char *ws)
{
    const hist_layout L = hist_layout_of(g.nbins, nf);
    HIP_TRY(ctx, hipMemsetAsync(ws, 0, L.stats, ctx->stream));
    HIP_TRY(ctx, h2y_launch_histogram(h2y_histogram_grid(ctx->n_cu, g, nf), ctx->stream, g, frames, nf, reinterpret_cast<hist_acc *>(ws),
                                      reinterpret_cast<uint32_t *>(ws + L.bins), reinterpret_cast<h2y_histogram_stats *>(ws + L.stats)));
    return H2Y_OK;
}

int h2y_histogram_batch(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int bit_depth, int full_range, int gbr, int bits,
                        int n_frames, const uint16_t *const *d_frames, h2y_histogram_stats *out_stats, uint32_t *out_bins)
{
    int rc = batch_enter(ctx);
    if (!rc) rc = hist_check(ctx, width, height, chroma_format_idc, bit_depth, full_range, gbr, bits);
    if (!rc) rc = frames_check(ctx, n_frames, d_frames, out_stats != nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t off[3];
    contiguous_planes(width, height, chroma_format_idc, off);
    const hist_geom g = hist_geom_of(width, height, chroma_format_idc, bit_depth, full_range, gbr, bits, off);
    const int per_launch = std::min(n_frames, H2Y_HISTOGRAM_FRAMES_PER_LAUNCH);
    const hist_layout L = hist_layout_of(g.nbins, per_launch);
    hist_frame *h;
    rc = frame_table(ctx, n_frames, h);
    if (!rc) rc = ensure(ctx, ctx->hist, L.total);
    if (rc) return rc;
    char *d_hist = ctx->hist.p;
    for (int f = 0; f < n_frames; f++) h[f].base = d_frames[f];
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_tab, h, (size_t)n_frames * sizeof(hist_frame), hipMemcpyHostToDevice, ctx->stream));
    const hist_frame *frames = static_cast<const hist_frame *>(ctx->d_tab);
    /* one launch at a time: its stats and bins come down before the next one reuses the workspace */
    float ms = 0.f;
    int launches = 0;
    hipEvent_t *ev = ctx->b->ev[0];
    for (int f0 = 0; f0 < n_frames; f0 += per_launch, launches++) {
        const int nf = std::min(per_launch, n_frames - f0);
        const hist_layout Ln = hist_layout_of(g.nbins, nf);
        HIP_TRY(ctx, hipEventRecord(ev[0], ctx->stream));
        rc = hist_enqueue(ctx, g, frames + f0, nf, d_hist);
        if (rc) return rc;
        HIP_TRY(ctx, hipEventRecord(ev[1], ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(out_stats + f0, d_hist + Ln.stats, (size_t)nf * sizeof(h2y_histogram_stats), hipMemcpyDeviceToHost,
                                    ctx->stream));
        if (out_bins)
            HIP_TRY(ctx, hipMemcpyAsync(out_bins + (size_t)f0 * 3u * g.nbins, d_hist + Ln.bins, (size_t)nf * 3u * g.nbins * sizeof(uint32_t),
                                        hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        float t = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&t, ev[0], ev[1]));
        ms += t;
    }
    ctx->b->n_ev = 1;
    ctx->last_ms = ms;
    ctx->last_launches = launches;
    ctx->last_name = "k_histogram";
    ctx->last_variant = std::string("k_histogram<") + (chroma_format_idc == H2Y_CHROMA_420 ? "420" : "444") + "," +
                        (h2y_histogram_lds(g.nbins) < (size_t)g.nbins * sizeof(uint32_t) ? "U16X2" : "U32") + ",bins=" +
                        std::to_string(g.nbins) + ">";
    return H2Y_OK;
}

/* The histogram's ring stage: per slot a device workspace of one frame (hist_layout), pinned stats and bins, and the slot's
 * k_histogram table entry (the ring's frame) */
struct hist_stage : ring_stage {
    struct slot {
        char *d = nullptr;
        h2y_histogram_stats *h_stats = nullptr;
        uint32_t *h_bins = nullptr;
    };
    std::vector<slot> ss;
    hist_geom g{};
    hist_frame *tab = nullptr;
    int run(h2y_ctx *ctx, int k) override { return hist_enqueue(ctx, g, tab + k, 1, ss[k].d); }
    int download(h2y_ctx *ctx, int k) override
    {
        const hist_layout L = hist_layout_of(g.nbins, 1);
        HIP_TRY(ctx, hipMemcpyAsync(ss[k].h_stats, ss[k].d + L.stats, sizeof(h2y_histogram_stats), hipMemcpyDeviceToHost, ctx->s_d2h));
        HIP_TRY(ctx, hipMemcpyAsync(ss[k].h_bins, ss[k].d + L.bins, (size_t)3u * g.nbins * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->s_d2h));
        return H2Y_OK;
    }
};

/* arm the open ring's frame, counted as bit_depth, full_range and gbr say */
static int hist_arm(h2y_ctx *ctx, int bit_depth, int full_range, int gbr, int bits)
{
    const ring_frame &f = ctx->s_frame;
    int rc = hist_check(ctx, f.width, f.height, f.chroma, bit_depth, full_range, gbr, bits);
    if (rc) return rc;
    auto st = std::make_unique<hist_stage>();
    st->g = hist_geom_of(f.width, f.height, f.chroma, bit_depth, full_range, gbr, bits, f.off);
    const hist_layout L = hist_layout_of(st->g.nbins, 1);
    const int depth = (int)ctx->ss.size();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<hist_frame> tab(depth);
    st->ss.resize(depth);
    for (int k = 0; k < depth; k++) {
        hist_stage::slot &s = st->ss[k];
        st->dev_alloc(s.d, L.total);
        st->pin_alloc(s.h_stats, sizeof(h2y_histogram_stats));
        st->pin_alloc(s.h_bins, (size_t)3u * st->g.nbins * sizeof(uint32_t));
        tab[k].base = frame_base(ctx, k);
    }
    st->table(st->tab, tab);
    return stage_arm(ctx, STAGE_HISTOGRAM, std::move(st), "histogram");
}

int h2y_stream_histogram_ex(h2y_ctx *ctx, int bits, int bit_depth, int full_range, int gbr)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    if (ctx->s_stage[STAGE_HISTOGRAM]) return fail(ctx, H2Y_EINVAL, "the ring counts histograms already");
    if (ctx->s_stage[STAGE_CODELIGHT]) return fail(ctx, H2Y_EINVAL, "a light-only ring takes no other stage");
    if (ctx->s_stage[STAGE_SCALE]) return fail(ctx, H2Y_EUNSUPPORTED, "a ring that scales counts no histograms: count the written file instead");
    if (ctx->s_stage[STAGE_DITHER]) return fail(ctx, H2Y_EUNSUPPORTED, "a ring that dithers counts no histograms: count the written file instead");
    if (ctx->s_stage[STAGE_PACK]) return fail(ctx, H2Y_EUNSUPPORTED, "a ring that packs counts no histograms: count the written file instead");
    rc = arm_unstarted(ctx);
    if (rc) return rc;
    const ring_frame &f = ctx->s_frame;
    if (!f.depth && (bit_depth < 0 || full_range < 0 || gbr < 0))
        return fail(ctx, H2Y_EINVAL, "a compare-only ring does not know its frames' bit depth and range: h2y_stream_histogram_ex");
    const int depth = bit_depth >= 0 ? bit_depth : f.depth;
    if (depth < 8 || depth > 16) return fail(ctx, H2Y_EINVAL, "bit_depth must be 8..16");
    return hist_arm(ctx, depth, full_range >= 0 ? full_range : f.full_range, gbr >= 0 ? gbr : (int)f.gbr, bits ? bits : depth);
}

int h2y_stream_histogram(h2y_ctx *ctx, int bits) { return h2y_stream_histogram_ex(ctx, bits, -1, -1, -1); }

int h2y_stream_histogram_result(h2y_ctx *ctx, h2y_histogram_stats *out_stats, uint32_t *out_bins)
{
    return stream_result<hist_stage>(ctx, out_stats, STAGE_HISTOGRAM, "no stream open that counts histograms", [&](const hist_stage &st, int k) {
        *out_stats = *st.ss[k].h_stats;
        if (out_bins) memcpy(out_bins, st.ss[k].h_bins, (size_t)3u * st.g.nbins * sizeof(uint32_t));
    });
}

/* A ring that only counts: the slot's input is the frame's three planes, the device output unused */
int h2y_histogram_stream_open(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int bit_depth, int full_range, int gbr, int bits,
                              int depth)
{
    int rc = ring_may_open(ctx);
    if (!rc) rc = hist_check(ctx, width, height, chroma_format_idc, bit_depth, full_range, gbr, bits);
    if (!rc) rc = open_planes_ring(ctx, width, height, chroma_format_idc, bit_depth, full_range, gbr, 0, depth);
    if (rc) return rc;
    rc = hist_arm(ctx, bit_depth, full_range, gbr, bits);
    if (rc) stream_free(ctx);
    return rc;
}

/* ---- scaling: the Lanczos resampler of include/hdr2yuv_hip.h ----------------------------------------------------------------- */

static double scale_sinc(double x) { return x == 0.0 ? 1.0 : sin(M_PI * x) / (M_PI * x); }

/* one axis' table as the header defines it, in binary64; rc H2Y_EUNSUPPORTED for a row of sum |q| > 32767 */
static int scale_axis_table(int s, int d, int a, int32_t *first, int32_t *count, int16_t *coef, int *max_taps)
{
    const double f = s > d ? (double)s / (double)d : 1.0, r = (double)a * f;
    int most = 0;
    for (int o = 0; o < d; o++) {
        const double c = (((double)o + 0.5) * (double)s) / (double)d - 0.5;
        int idx[H2Y_SCALE_TAPS + 2];
        double w[H2Y_SCALE_TAPS + 2], S = 0.0;
        int n = 0;
        for (int i = (int)ceil(c - r), hi = (int)floor(c + r); i <= hi; i++) {
            if (!(fabs((double)i - c) < r)) continue;
            if (n == H2Y_SCALE_TAPS) return H2Y_EUNSUPPORTED;
            const double t = ((double)i - c) / f;
            idx[n] = i;
            w[n] = scale_sinc(t) * scale_sinc(t / (double)a);
            S += w[n];
            n++;
        }
        if (n == 0) return H2Y_EUNSUPPORTED;
        int q[H2Y_SCALE_TAPS], sum = 0, big = 0;
        for (int k = 0; k < n; k++) {
            q[k] = (int)rint(w[k] * 16384.0 / S);
            sum += q[k];
            if (q[k] > q[big]) big = k;
        }
        q[big] += 16384 - sum;
        const int lo = idx[0] < 0 ? 0 : idx[0] > s - 1 ? s - 1 : idx[0];
        int folded[H2Y_SCALE_TAPS] = {0}, m = 0, mag = 0;
        for (int k = 0; k < n; k++) {
            const int i = idx[k] < 0 ? 0 : idx[k] > s - 1 ? s - 1 : idx[k];
            folded[i - lo] += q[k];
            m = i - lo + 1;
        }
        for (int k = 0; k < m; k++) mag += folded[k] < 0 ? -folded[k] : folded[k];
        if (mag > 32767) return H2Y_EUNSUPPORTED;
        first[o] = lo;
        count[o] = m;
        for (int k = 0; k < H2Y_SCALE_TAPS; k++) coef[(size_t)o * H2Y_SCALE_TAPS + k] = (int16_t)(k < m ? folded[k] : 0);
        most = m > most ? m : most;
    }
    if (max_taps) *max_taps = most;
    return H2Y_OK;
}

static bool scale_axis_ok(int s, int d) { return s >= 1 && d >= 1 && s <= 10000 && d <= 10000 && s <= 4 * d && d <= 4 * s; }

int h2y_scale_taps(int src, int dst, int a, int32_t *first, int32_t *count, int16_t *coef, int *max_taps)
{
    if (!first || !count || !coef) return fail(nullptr, H2Y_EINVAL, "null table");
    if (a < 2 || a > 4) return fail(nullptr, H2Y_EINVAL, "a (lobes) must be 2, 3 or 4");
    if (!scale_axis_ok(src, dst)) return fail(nullptr, H2Y_EINVAL, "sizes must be 1..10000 with a ratio in [1/4, 4]");
    const int rc = scale_axis_table(src, dst, a, first, count, coef, max_taps);
    if (rc) return fail(nullptr, rc, "a table row's coefficients do not fit (sum |q| > 32767)");
    return H2Y_OK;
}

size_t h2y_scale_frame_bytes(int width, int height, int chroma_format_idc)
{
    if (width < 1 || height < 1 || width > 10000 || height > 10000) return 0;
    if (chroma_format_idc == H2Y_CHROMA_444) return (size_t)width * height * 3u * sizeof(uint16_t);
    if (chroma_format_idc != H2Y_CHROMA_420) return 0;
    return ((size_t)width * height + 2u * (size_t)(width >> 1) * (height >> 1)) * sizeof(uint16_t);
}

static int scale_check(h2y_ctx *ctx, int sw, int sh, int dw, int dh, int chroma, int bit_depth, int full_range, int gbr, int a)
{
    if (chroma == 2) return fail(ctx, H2Y_EUNSUPPORTED, "chroma_format_idc 2 (4:2:2) is not scaled");
    if (chroma != H2Y_CHROMA_420 && chroma != H2Y_CHROMA_444) return fail(ctx, H2Y_EINVAL, "chroma_format_idc must be 1 or 3");
    if (sw < 2 || sh < 2 || dw < 2 || dh < 2 || sw > 10000 || sh > 10000 || dw > 10000 || dh > 10000)
        return fail(ctx, H2Y_EINVAL, "scaling: widths and heights must be 2..10000");
    if (chroma == H2Y_CHROMA_420 && ((sw | sh | dw | dh) & 1)) return fail(ctx, H2Y_EINVAL, "scaling 4:2:0: widths and heights must be even");
    if (!scale_axis_ok(sw, dw) || !scale_axis_ok(sh, dh)) return fail(ctx, H2Y_EINVAL, "scaling: each axis ratio must be in [1/4, 4]");
    if (bit_depth < 8 || bit_depth > 16) return fail(ctx, H2Y_EINVAL, "bit_depth must be 8..16");
    if ((full_range != 0 && full_range != 1) || (gbr != 0 && gbr != 1)) return fail(ctx, H2Y_EINVAL, "full_range and gbr must be 0 or 1");
    if (a < 2 || a > 4) return fail(ctx, H2Y_EINVAL, "a (lobes) must be 2, 3 or 4");
    return H2Y_OK;
}

/* k_scale's geometry with its tables still on the host: blob is what goes to the device, at[p][axis][0..2] where plane p's
 * first, count and coef of that axis lie in it (4:4:4: one pair of tables serves the three planes) */
struct scale_host {
    scale_geom g{};
    std::vector<char> blob;
    size_t at[3][2][3]{};
};

static int scale_build(h2y_ctx *ctx, int sw, int sh, int dw, int dh, int chroma, int bit_depth, int full_range, int gbr, int a,
                       const uint32_t src_off[3], const uint32_t dst_off[3], scale_host &H)
{
    const bool sub = chroma == H2Y_CHROMA_420;
    const clip_limits c = make_clip(bit_depth, full_range);
    size_t kind_at[2][2][3];
    for (int kind = 0; kind < (sub ? 2 : 1); kind++)
        for (int axis = 0; axis < 2; axis++) {
            const int s = (axis ? sh : sw) >> kind, d = (axis ? dh : dw) >> kind;
            const size_t ib = ((size_t)d * sizeof(int32_t) + 15) & ~(size_t)15, cb = (size_t)d * H2Y_SCALE_TAPS * sizeof(int16_t);
            const size_t base = H.blob.size();
            H.blob.resize(base + 2 * ib + cb);
            kind_at[kind][axis][0] = base, kind_at[kind][axis][1] = base + ib, kind_at[kind][axis][2] = base + 2 * ib;
            const int rc = scale_axis_table(s, d, a, reinterpret_cast<int32_t *>(&H.blob[base]), reinterpret_cast<int32_t *>(&H.blob[base + ib]),
                                            reinterpret_cast<int16_t *>(&H.blob[base + 2 * ib]), nullptr);
            if (rc) return fail(ctx, rc, "scaling %d -> %d: a table row's coefficients do not fit (sum |q| > 32767)", s, d);
        }
    uint32_t h_rows = 1, seg_max = 1;
    for (int p = 0; p < 3; p++) {
        const int kind = p && sub ? 1 : 0;
        scale_plane &P = H.g.p[p];
        P.sw = (uint32_t)(sw >> kind), P.sh = (uint32_t)(sh >> kind), P.dw = (uint32_t)(dw >> kind), P.dh = (uint32_t)(dh >> kind);
        P.src_off = src_off[p], P.dst_off = dst_off[p];
        P.tiles_x = (P.dw + H2Y_SCALE_TILE_W - 1) / H2Y_SCALE_TILE_W;
        P.tiles = P.tiles_x * ((P.dh + H2Y_SCALE_TILE_H - 1) / H2Y_SCALE_TILE_H);
        const bool luma_like = p == 0 || gbr;
        P.lo = (int32_t)(luma_like ? c.minVR : c.minVRC);
        P.hi = (int32_t)(luma_like ? c.maxVR : c.maxVRC);
        for (int axis = 0; axis < 2; axis++)
            for (int k = 0; k < 3; k++) H.at[p][axis][k] = kind_at[kind][axis][k];
        /* the most source columns and rows one tile reads: what the kernel's LDS must hold */
        for (int axis = 0; axis < 2; axis++) {
            const int32_t *first = reinterpret_cast<const int32_t *>(&H.blob[H.at[p][axis][0]]);
            const int32_t *count = reinterpret_cast<const int32_t *>(&H.blob[H.at[p][axis][1]]);
            const uint32_t d = axis ? P.dh : P.dw, step = axis ? H2Y_SCALE_TILE_H : H2Y_SCALE_TILE_W;
            for (uint32_t o0 = 0; o0 < d; o0 += step) {
                const uint32_t o1 = std::min(d, o0 + step) - 1;
                const uint32_t span = (uint32_t)(first[o1] + count[o1] - first[o0]);
                if (axis) h_rows = std::max(h_rows, span);
                else seg_max = std::max(seg_max, span);
            }
        }
    }
    H.g.h_rows = h_rows;
    H.g.src_cols = (seg_max + 7u + 7u) & ~7u;
    if (h2y_scale_lds(H.g) > 64u * 1024u) return fail(ctx, H2Y_EUNSUPPORTED, "scaling: a tile needs %zu bytes of LDS", h2y_scale_lds(H.g));
    return H2Y_OK;
}

/* the tables' addresses once the blob lies at d_base */
static void scale_bind(scale_host &H, const char *d_base)
{
    for (int p = 0; p < 3; p++) {
        scale_axis *ax[2] = {&H.g.p[p].h, &H.g.p[p].v};
        for (int axis = 0; axis < 2; axis++) {
            ax[axis]->first = reinterpret_cast<const int32_t *>(d_base + H.at[p][axis][0]);
            ax[axis]->count = reinterpret_cast<const int32_t *>(d_base + H.at[p][axis][1]);
            ax[axis]->coef = reinterpret_cast<const int16_t *>(d_base + H.at[p][axis][2]);
        }
    }
}

static int scale_grid(const h2y_ctx *ctx, const scale_geom &g, int n_frames)
{
    return unit_grid(ctx, (uint64_t)n_frames * (g.p[0].tiles + g.p[1].tiles + g.p[2].tiles));
}

static std::string scale_variant(int chroma, int a)
{
    return std::string("k_scale<") + (chroma == H2Y_CHROMA_420 ? "420" : "444") + ",lanczos" + std::to_string(a) + ">";
}

int h2y_scale_batch(h2y_ctx *ctx, int src_w, int src_h, int dst_w, int dst_h, int chroma_format_idc, int bit_depth, int full_range,
                    int gbr, int a, int n_frames, const uint16_t *const *d_src, uint16_t *const *d_dst)
{
    int rc = batch_enter(ctx);
    if (!rc) rc = scale_check(ctx, src_w, src_h, dst_w, dst_h, chroma_format_idc, bit_depth, full_range, gbr, a);
    if (!rc) rc = pairs_check(ctx, n_frames, d_src, d_dst);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t src_off[3], dst_off[3];
    contiguous_planes(src_w, src_h, chroma_format_idc, src_off);
    contiguous_planes(dst_w, dst_h, chroma_format_idc, dst_off);
    scale_host H;
    rc = scale_build(ctx, src_w, src_h, dst_w, dst_h, chroma_format_idc, bit_depth, full_range, gbr, a, src_off, dst_off, H);
    if (rc) return rc;
    scale_frame *h;
    rc = frame_table(ctx, n_frames, h);
    if (!rc) rc = ensure(ctx, ctx->scale_tabs, H.blob.size());
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->scale_tabs.p, H.blob.data(), H.blob.size(), hipMemcpyHostToDevice));
    scale_bind(H, ctx->scale_tabs.p);
    for (int f = 0; f < n_frames; f++) h[f] = scale_frame{d_src[f], d_dst[f]};
    rc = timed_launches(ctx, h, n_frames, H2Y_SCALE_FRAMES_PER_LAUNCH, "k_scale", [&](const scale_frame *frames, int, int nf) {
        return h2y_launch_scale(scale_grid(ctx, H.g, nf), ctx->stream, H.g, frames, nf);
    });
    if (rc) return rc;
    ctx->last_variant = scale_variant(chroma_format_idc, a);
    return H2Y_OK;
}

/* Scaling's ring stage: k_scale's geometry, its tables on the device and each slot's table entry.  On a ring that produces its
 * frame the stage scales it into a frame of its own, on the device and pinned, which goes down and is handed out in the
 * produced frame's place; on a ring without a producer it scales the slot's input into its output. */
struct scale_stage : ring_stage {
    struct slot {
        uint16_t *d = nullptr, *h = nullptr;
    };
    std::vector<slot> ss;
    scale_geom g{};
    char *tabs = nullptr;
    scale_frame *tab = nullptr;
    size_t bytes = 0; /* of the scaled frame */
    bool down = true; /* false: a dither or pack stage armed behind this one sends its own frame down instead */
    int run(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, h2y_launch_scale(scale_grid(ctx, g, 1), ctx->stream, g, tab + k, 1));
        return H2Y_OK;
    }
    int download(h2y_ctx *ctx, int k) override
    {
        if (ss[k].d && down) HIP_TRY(ctx, hipMemcpyAsync(ss[k].h, ss[k].d, bytes, hipMemcpyDeviceToHost, ctx->s_d2h));
        return H2Y_OK;
    }
};

/* arm the open ring's frame, scaled to dw x dh */
static int scale_arm(h2y_ctx *ctx, int dw, int dh, int a)
{
    const ring_frame &f = ctx->s_frame;
    uint32_t dst_off[3];
    contiguous_planes(dw, dh, f.chroma, dst_off);
    scale_host H;
    int rc = scale_build(ctx, f.width, f.height, dw, dh, f.chroma, f.depth, f.full_range, f.gbr, a, f.off, dst_off, H);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto st = std::make_unique<scale_stage>();
    scale_stage *sc = st.get();
    sc->bytes = h2y_scale_frame_bytes(dw, dh, f.chroma);
    const int depth = (int)ctx->ss.size();
    std::vector<scale_frame> tab(depth);
    sc->ss.resize(depth);
    sc->dev_alloc(sc->tabs, H.blob.size());
    for (int k = 0; k < depth; k++) {
        if (!f.in_input) {
            sc->dev_alloc(sc->ss[k].d, sc->bytes);
            sc->pin_alloc(sc->ss[k].h, sc->bytes);
        }
        tab[k] = scale_frame{frame_base(ctx, k), f.in_input ? ctx->ss[k].d_out : sc->ss[k].d};
    }
    if (sc->err == hipSuccess) sc->err = hipMemcpy(sc->tabs, H.blob.data(), H.blob.size(), hipMemcpyHostToDevice);
    sc->table(sc->tab, tab);
    scale_bind(H, sc->tabs);
    sc->g = H.g;
    rc = stage_arm(ctx, STAGE_SCALE, std::move(st), "scaling");
    if (rc || f.in_input) return rc;
    ring_frame_stays(ctx);
    for (int k = 0; k < depth; k++) ctx->ss[k].result = sc->ss[k].h;
    return H2Y_OK;
}

int h2y_stream_scale(h2y_ctx *ctx, int dst_w, int dst_h, int a)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    if (ctx->s_kind != h2y_ctx::RING_FORWARD) return fail(ctx, H2Y_EINVAL, "only a forward ring is armed for scaling");
    if (ctx->s_stage[STAGE_SCALE]) return fail(ctx, H2Y_EINVAL, "the ring scales already");
    if (ctx->s_stage[STAGE_DITHER]) return fail(ctx, H2Y_EINVAL, "the ring dithers already: arm scaling before dither");
    if (ctx->s_stage[STAGE_PACK]) return fail(ctx, H2Y_EINVAL, "the ring packs already: arm scaling before pack");
    if (ctx->s_stage[STAGE_COMPARE] || ctx->s_stage[STAGE_HISTOGRAM] || ctx->s_stage[STAGE_SSIM])
        return fail(ctx, H2Y_EUNSUPPORTED, "a ring armed for comparison, histograms or SSIM is not scaled: compare or count the written file instead");
    rc = arm_unstarted(ctx);
    if (rc) return rc;
    const ring_frame &f = ctx->s_frame;
    /* k_scale aligns sample centres: it would move a top-left sited chroma plane again (the setting cannot change while the ring is open) */
    if (ctx->opt_siting == 2 && f.chroma == H2Y_CHROMA_420)
        return fail(ctx, H2Y_EUNSUPPORTED, "a ring with chroma siting 2 (top-left) is not scaled: the resampler aligns sample centres");
    rc = scale_check(ctx, f.width, f.height, dst_w, dst_h, f.chroma, f.depth, f.full_range, f.gbr, a);
    if (rc) return rc;
    return scale_arm(ctx, dst_w, dst_h, a);
}

/* A ring that only scales: the slot's input is the frame's three planes, its output the scaled frame */
int h2y_scale_stream_open(h2y_ctx *ctx, int src_w, int src_h, int chroma_format_idc, int bit_depth, int full_range, int gbr, int dst_w,
                          int dst_h, int a, int depth)
{
    int rc = ring_may_open(ctx);
    if (!rc) rc = scale_check(ctx, src_w, src_h, dst_w, dst_h, chroma_format_idc, bit_depth, full_range, gbr, a);
    if (!rc) rc = open_planes_ring(ctx, src_w, src_h, chroma_format_idc, bit_depth, full_range, gbr,
                                   h2y_scale_frame_bytes(dst_w, dst_h, chroma_format_idc), depth);
    if (rc) return rc;
    rc = scale_arm(ctx, dst_w, dst_h, a);
    if (rc) stream_free(ctx);
    return rc;
}

/* ---- conversion between colour primaries (--gamut_convert; the reference's matrix_to_primaries() is empty, convert.cpp:1991) ------ */

namespace {

typedef __int128 i128;

/* One set of primaries in exact integers: its normalised primary matrix is A diag(u) / (det k).  RGB: A's columns are the primaries'
 * (x, y, z) in units of 1e-4, u = adj(A) (xw, yw, zw), det = |A|, k = yw; XYZ: the identity. */
struct gamut_set {
    i128 A[3][3], u[3], det, k;
};

void gamut_adj(const i128 A[3][3], i128 adj[3][3])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { /* adj[i][j] = the cofactor of A[j][i] */
            const int r0 = (j + 1) % 3, r1 = (j + 2) % 3, c0 = (i + 1) % 3, c1 = (i + 2) % 3;
            adj[i][j] = A[r0][c0] * A[r1][c1] - A[r0][c1] * A[r1][c0];
        }
}

/* 0: not a set this conversion knows; otherwise a number that is equal for equal chromaticities */
int gamut_set_of(int code, gamut_set &s)
{
    static const int kXy[3][6] = {{6400, 3300, 3000, 6000, 1500, 600},   /* BT.709 */
                                  {7080, 2920, 1700, 7970, 1310, 460},   /* BT.2020 */
                                  {6800, 3200, 2650, 6900, 1500, 600}};  /* P3-D65 */
    static const int kWhite[3] = {3127, 3290, 10000 - 3127 - 3290};      /* D65 */
    const int which = code == 1 ? 0 : code == 8 || code == 9 ? 1 : code == 12 ? 2 : code == 10 ? 3 : -1;
    if (which < 0) return 0;
    if (which == 3) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) s.A[i][j] = i == j;
        s.u[0] = s.u[1] = s.u[2] = s.det = s.k = 1;
        return 4;
    }
    for (int j = 0; j < 3; j++) {
        s.A[0][j] = kXy[which][2 * j];
        s.A[1][j] = kXy[which][2 * j + 1];
        s.A[2][j] = 10000 - kXy[which][2 * j] - kXy[which][2 * j + 1];
    }
    i128 adj[3][3];
    gamut_adj(s.A, adj);
    s.det = 0;
    for (int j = 0; j < 3; j++) s.det += s.A[0][j] * adj[j][0];
    for (int i = 0; i < 3; i++) s.u[i] = adj[i][0] * kWhite[0] + adj[i][1] * kWhite[1] + adj[i][2] * kWhite[2];
    s.k = kWhite[1];
    return which + 1;
}

/* num / den (den != 0, both below 2^100) rounded to nearest binary32, ties to even; false where the result is no normal number */
bool gamut_round(i128 num, i128 den, float *out)
{
    if (num == 0) { *out = 0.0f; return true; }
    const bool neg = (num < 0) != (den < 0);
    i128 n = num < 0 ? -num : num, d = den < 0 ? -den : den;
    int e = 0;
    const i128 lim = (i128)1 << 124;
    while (n >= 2 * d) {
        if (d >= lim) return false;
        d <<= 1, e++;
    }
    while (n < d) {
        if (n >= lim) return false;
        n <<= 1, e--;
    }
    uint32_t q = 1; /* d <= n < 2 d */
    i128 r = n - d;
    for (int b = 0; b < 23; b++) {
        r <<= 1;
        q <<= 1;
        if (r >= d) r -= d, q |= 1u;
    }
    r <<= 1;
    if (r > d || (r == d && (q & 1u))) q++;
    if (q == (1u << 24)) q >>= 1, e++;
    if (e < -126 || e > 127) return false;
    const float v = ldexpf((float)q, e - 23);
    *out = neg ? -v : v;
    return true;
}

} // namespace

int h2y_gamut_matrix(int src_primaries, int dst_primaries, float m[9], const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!m) { *why = "null matrix"; return H2Y_EINVAL; }
    gamut_set s, d;
    const int ks = gamut_set_of(src_primaries, s), kd = gamut_set_of(dst_primaries, d);
    if (!ks || !kd) {
        *why = "colour primaries other than 1 (BT.709), 8 / 9 (BT.2020), 12 (P3-D65) and 10 (XYZ) are not converted";
        return H2Y_EUNSUPPORTED;
    }
    if (ks == kd) { *why = "source and destination primaries have the same chromaticities: there is nothing to convert"; return H2Y_EINVAL; }
    /* M = NPM(d)^-1 NPM(s) = k_d diag(1 / u_d) adj(A_d) A_s diag(u_s) / (det_s k_s)   (det_d cancels) */
    i128 adj[3][3];
    gamut_adj(d.A, adj);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            i128 p = 0;
            for (int t = 0; t < 3; t++) p += adj[i][t] * s.A[t][j];
            if (!gamut_round(d.k * p * s.u[j], d.u[i] * s.det * s.k, &m[3 * i + j])) { *why = "matrix entry out of range"; return H2Y_EINVAL; }
        }
    return H2Y_OK;
}

/* k_gamut's arguments for frames of width x height and a pair of primaries; the checks of both entries */
static int gamut_args_of(h2y_ctx *ctx, int width, int height, int sample_type, int src_primaries, int dst_primaries, int clip, gamut_args &a)
{
    if (sample_type == H2Y_SAMPLE_U16)
        return fail(ctx, H2Y_EUNSUPPORTED, "primaries are converted in linear light on float or half planes, not on U16 samples");
    if (sample_type != H2Y_SAMPLE_F32 && sample_type != H2Y_SAMPLE_F16) return fail(ctx, H2Y_EINVAL, "bad sample type %d", sample_type);
    int rc = picture_size_check(ctx, width, height);
    if (rc) return rc;
    if (clip != 0 && clip != 1) return fail(ctx, H2Y_EINVAL, "clip must be 0 or 1");
    const char *why;
    rc = h2y_gamut_matrix(src_primaries, dst_primaries, a.m, &why);
    if (rc) return fail(ctx, rc, "primaries %d -> %d: %s", src_primaries, dst_primaries, why);
    a.npix = (uint32_t)width * (uint32_t)height;
    a.clip = (uint32_t)clip;
    return H2Y_OK;
}

static std::string gamut_variant(int in_kind, const gamut_args &a)
{
    return std::string("k_gamut<") + (in_kind == H2Y_IN_F16 ? "F16" : "F32") + (a.clip ? ",CLIP>" : ",NOCLIP>");
}

int h2y_gamut_batch(h2y_ctx *ctx, int width, int height, int sample_type, int src_primaries, int dst_primaries, int clip, int n_frames,
                    const void *const *d_src, void *const *d_dst)
{
    gamut_args a{};
    gamut_frame *h;
    int rc = batch_enter(ctx);
    if (!rc) rc = gamut_args_of(ctx, width, height, sample_type, src_primaries, dst_primaries, clip, a);
    if (!rc) rc = pass_frames(ctx, n_frames, d_src, d_dst, false, h);
    if (rc) return rc;
    const int in_kind = sample_type == H2Y_SAMPLE_F16 ? H2Y_IN_F16 : H2Y_IN_F32;
    const uint64_t per_frame = h2y_gamut_chunks(in_kind, a.npix);
    rc = timed_launches(ctx, h, n_frames, H2Y_GAMUT_FRAMES_PER_LAUNCH, "k_gamut", [&](const gamut_frame *frames, int, int nf) {
        return h2y_launch_gamut(in_kind, unit_grid(ctx, per_frame * nf), ctx->stream, a, frames, nf);
    });
    if (rc) return rc;
    ctx->last_variant = gamut_variant(in_kind, a);
    return H2Y_OK;
}

/* The conversion's ring stage: the first pass, k_gamut on the decoded planes */
int h2y_stream_gamut(h2y_ctx *ctx, int src_primaries, int dst_primaries, int clip)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    if (ctx->s_kind != h2y_ctx::RING_FORWARD) return fail(ctx, H2Y_EINVAL, "primaries are converted on the forward rings only");
    if (ring_holds_signal(ctx)) return fail(ctx, H2Y_EINVAL, "the ring's planes hold signal, not light: primaries are converted in linear light");
    rc = arm_free(ctx, STAGE_GAMUT, "the ring converts primaries already");
    if (rc) return rc;
    const h2y_desc *d = &ctx->s_desc;
    auto st = std::make_unique<pass_stage<gamut_args>>();
    st->launch = h2y_launch_gamut;
    rc = gamut_args_of(ctx, d->width, d->height, d->in_sample_type, src_primaries, dst_primaries, clip, st->a);
    if (rc) return rc;
    if (d->src_transfer != H2Y_TRANSFER_LINEAR)
        return fail(ctx, H2Y_EUNSUPPORTED, "primaries are converted in linear light (src_transfer 8), not src_transfer %d", d->src_transfer);
    if (d->src_matrix != H2Y_MATRIX_GBR)
        return fail(ctx, H2Y_EUNSUPPORTED, "converting primaries needs a G,B,R source (src_matrix 0), not src_matrix %d", d->src_matrix);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    st->in_kind = in_kind_of(d);
    st->grid = unit_grid(ctx, h2y_gamut_chunks(st->in_kind, st->a.npix));
    st->table(st->tab, ring_planes_table(ctx));
    return stage_arm(ctx, STAGE_GAMUT, std::move(st), "gamut");
}

/* ---- gamut compression (--gamut_compress; the reference has no such step): include/hdr2yuv_hip.h states the definition --------------- */

int h2y_gamut_compress_curve(int src_primaries, int dst_primaries, float threshold, float power, h2y_gamut_compress_tables *out,
                             const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!out) { *why = "null tables"; return H2Y_EINVAL; }
    if (!(threshold >= 0.5f && threshold <= 0.95f)) { *why = "threshold outside 0.5 <= threshold <= 0.95"; return H2Y_EINVAL; }
    if (!(power >= 1.0f && power <= 4.0f)) { *why = "power outside 1 <= power <= 4"; return H2Y_EINVAL; }
    if (src_primaries == 10 || dst_primaries == 10) {
        *why = "XYZ (colour primaries 10) has no gamut to take limits from: convert it with the clip";
        return H2Y_EUNSUPPORTED;
    }
    memset(out, 0, sizeof *out);
    const int rc = h2y_gamut_matrix(src_primaries, dst_primaries, out->m, why);
    if (rc) return rc;
    out->threshold = threshold, out->power = power;
    static const double kCorner[6][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 1, 1}, {1, 0, 1}, {1, 1, 0}};
    double lim[3] = {0.0, 0.0, 0.0};
    for (const double *x : kCorner) {
        double o[3];
        for (int i = 0; i < 3; i++) o[i] = ((double)out->m[3 * i] * x[0] + (double)out->m[3 * i + 1] * x[1]) + (double)out->m[3 * i + 2] * x[2];
        const double a = std::max(std::max(o[0], o[1]), o[2]);
        for (int i = 0; i < 3; i++) lim[i] = std::max(lim[i], (a - o[i]) / a);
    }
    const double t = threshold, p = power;
    for (int i = 0; i < 3; i++) {
        out->limit[i] = (float)lim[i];
        if (!(out->limit[i] > 1.0f)) continue;
        const double w = (double)out->limit[i] - t, s = w / pow(pow((1.0 - t) / w, -p) - 1.0, 1.0 / p);
        out->scale[i] = (float)(1024.0 / w);
        float *T = out->table[i];
        for (int k = 1; k < H2Y_GAMUT_COMPRESS_NODES - 1; k++) {
            const double u = (w * k) / 1024.0;
            T[k] = (float)(t + u / pow(1.0 + pow(u / s, p), 1.0 / p));
        }
        T[0] = threshold, T[H2Y_GAMUT_COMPRESS_NODES - 1] = 1.0f;
    }
    return H2Y_OK;
}

/* the pixel's constants of a curve */
static void gamut_compress_consts_of(const h2y_gamut_compress_tables &c, gamut_compress_consts &k)
{
    memcpy(k.m, c.m, sizeof k.m);
    k.t = c.threshold;
    const double q = 1.0 - (double)c.threshold * (1.0 - 0x1p-20);
    k.q = (float)q;
    if ((double)k.q < q) k.q = nextafterf(k.q, 2.0f);
    for (int i = 0; i < 3; i++) k.l[i] = c.limit[i], k.k[i] = c.scale[i];
}

int h2y_gamut_compress_planes(int src_primaries, int dst_primaries, float threshold, float power, int sample_type, size_t npix,
                              const void *const src[3], void *const dst[3])
{
    if (sample_type != H2Y_SAMPLE_F32 && sample_type != H2Y_SAMPLE_F16)
        return fail(nullptr, H2Y_EUNSUPPORTED, "gamut compression reads float or half planes, not sample type %d", sample_type);
    if (!src || !dst || !src[0] || !src[1] || !src[2] || !dst[0] || !dst[1] || !dst[2]) return fail(nullptr, H2Y_EINVAL, "null planes");
    auto c = std::make_unique<h2y_gamut_compress_tables>();
    const char *why;
    const int rc = h2y_gamut_compress_curve(src_primaries, dst_primaries, threshold, power, c.get(), &why);
    if (rc) return fail(nullptr, rc, "gamut compression %d -> %d: %s", src_primaries, dst_primaries, why);
    gamut_compress_consts k{};
    gamut_compress_consts_of(*c, k);
    const float *T = &c->table[0][0];
    for (size_t i = 0; i < npix; i++) {
        float v[3], o[3]; /* v: G, B, R; o: R, G, B */
        for (int p = 0; p < 3; p++) {
            if (sample_type == H2Y_SAMPLE_F32) v[p] = static_cast<const float *>(src[p])[i];
            else v[p] = (float)static_cast<const _Float16 *>(src[p])[i]; /* exact */
        }
        gamut_compress_pixel(k, T, v[2], v[0], v[1], o);
        const float w[3] = {o[1], o[2], o[0]};
        for (int p = 0; p < 3; p++) {
            if (sample_type == H2Y_SAMPLE_F32) static_cast<float *>(dst[p])[i] = w[p];
            else static_cast<_Float16 *>(dst[p])[i] = (_Float16)w[p]; /* to nearest even */
        }
    }
    return H2Y_OK;
}

/* k_gamut_compress' arguments for frames of width x height, but for the device tables; the checks of both entries */
static int gamut_compress_args_of(h2y_ctx *ctx, int width, int height, int sample_type, int src_primaries, int dst_primaries,
                                  float threshold, float power, gamut_compress_args &a, std::vector<float> &tables)
{
    if (sample_type == H2Y_SAMPLE_U16)
        return fail(ctx, H2Y_EUNSUPPORTED, "gamut compression works in linear light on float or half planes, not on U16 samples");
    if (sample_type != H2Y_SAMPLE_F32 && sample_type != H2Y_SAMPLE_F16) return fail(ctx, H2Y_EINVAL, "bad sample type %d", sample_type);
    int rc = picture_size_check(ctx, width, height);
    if (rc) return rc;
    auto c = std::make_unique<h2y_gamut_compress_tables>();
    const char *why;
    rc = h2y_gamut_compress_curve(src_primaries, dst_primaries, threshold, power, c.get(), &why);
    if (rc) return fail(ctx, rc, "gamut compression %d -> %d, threshold %g, power %g: %s", src_primaries, dst_primaries, threshold, power, why);
    gamut_compress_consts_of(*c, a.c);
    tables.assign(&c->table[0][0], &c->table[0][0] + 3 * H2Y_GAMUT_COMPRESS_NODES);
    a.npix = (uint32_t)width * (uint32_t)height;
    return H2Y_OK;
}

int h2y_gamut_compress_batch(h2y_ctx *ctx, int width, int height, int sample_type, int src_primaries, int dst_primaries, float threshold,
                             float power, int n_frames, const void *const *d_src, void *const *d_dst)
{
    gamut_compress_args a{};
    std::vector<float> tables;
    gamut_frame *h;
    int rc = batch_enter(ctx);
    if (!rc) rc = gamut_compress_args_of(ctx, width, height, sample_type, src_primaries, dst_primaries, threshold, power, a, tables);
    if (!rc) rc = pass_frames(ctx, n_frames, d_src, d_dst, false, h);
    if (!rc) rc = ensure(ctx, ctx->gamut_compress_tables, tables.size() * sizeof(float));
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->gamut_compress_tables.p, tables.data(), tables.size() * sizeof(float), hipMemcpyHostToDevice));
    a.tables = ctx->gamut_compress_tables.p;
    const int in_kind = sample_type == H2Y_SAMPLE_F16 ? H2Y_IN_F16 : H2Y_IN_F32;
    const uint64_t per_frame = h2y_gamut_chunks(in_kind, a.npix);
    rc = timed_launches(ctx, h, n_frames, H2Y_GAMUT_COMPRESS_FRAMES_PER_LAUNCH, "k_gamut_compress", [&](const gamut_frame *frames, int, int nf) {
        return h2y_launch_gamut_compress(in_kind, unit_grid(ctx, per_frame * nf), ctx->stream, a, frames, nf);
    });
    if (rc) return rc;
    ctx->last_variant = std::string("k_gamut_compress<") + (in_kind == H2Y_IN_F16 ? "F16>" : "F32>");
    return H2Y_OK;
}

/* The compression's ring stage: the gamut stage's place, k_gamut_compress on the decoded planes with the tables of its own */
int h2y_stream_gamut_compress(h2y_ctx *ctx, int src_primaries, int dst_primaries, float threshold, float power)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    if (ctx->s_kind != h2y_ctx::RING_FORWARD) return fail(ctx, H2Y_EINVAL, "primaries are converted on the forward rings only");
    if (ring_holds_signal(ctx)) return fail(ctx, H2Y_EINVAL, "the ring's planes hold signal, not light: primaries are converted in linear light");
    rc = arm_free(ctx, STAGE_GAMUT, "the ring converts primaries already");
    if (rc) return rc;
    const h2y_desc *d = &ctx->s_desc;
    auto st = std::make_unique<pass_stage<gamut_compress_args>>();
    st->launch = h2y_launch_gamut_compress;
    std::vector<float> tables;
    rc = gamut_compress_args_of(ctx, d->width, d->height, d->in_sample_type, src_primaries, dst_primaries, threshold, power, st->a, tables);
    if (rc) return rc;
    if (d->src_transfer != H2Y_TRANSFER_LINEAR)
        return fail(ctx, H2Y_EUNSUPPORTED, "primaries are converted in linear light (src_transfer 8), not src_transfer %d", d->src_transfer);
    if (d->src_matrix != H2Y_MATRIX_GBR)
        return fail(ctx, H2Y_EUNSUPPORTED, "converting primaries needs a G,B,R source (src_matrix 0), not src_matrix %d", d->src_matrix);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    st->in_kind = in_kind_of(d);
    st->grid = unit_grid(ctx, h2y_gamut_chunks(st->in_kind, st->a.npix));
    float *d_tables = nullptr;
    st->table(d_tables, tables);
    st->a.tables = d_tables;
    st->table(st->tab, ring_planes_table(ctx));
    return stage_arm(ctx, STAGE_GAMUT, std::move(st), "gamut");
}

/* ---- tone mapping (--tone_map; the reference has no tone mapper) ------------------------------------------------------------------ */

namespace {

/* ST 2084's inverse EOTF and its inverse, in binary64 */
const double kPqM1 = 2610.0 / 16384.0, kPqM2 = 2523.0 / 4096.0 * 128.0, kPqC1 = 3424.0 / 4096.0, kPqC2 = 2413.0 / 4096.0 * 32.0,
             kPqC3 = 2392.0 / 4096.0 * 32.0;
double pq_n(double l)
{
    const double p = pow(l, kPqM1);
    return pow((kPqC1 + kPqC2 * p) / (1.0 + kPqC3 * p), kPqM2);
}
double pq_n_inv(double v)
{
    const double p = pow(v, 1.0 / kPqM2), num = p - kPqC1;
    return pow((num > 0.0 ? num : 0.0) / (kPqC2 - kPqC3 * p), 1.0 / kPqM1);
}

const char *tonemap_params_why(int src_peak, int dst_peak, int relative)
{
    if (dst_peak < 100 || dst_peak >= src_peak || src_peak > 10000) return "peaks outside 100 <= dst_peak < src_peak <= 10000 cd/m2";
    if (relative != 0 && relative != 1) return "relative must be 0 or 1";
    return nullptr;
}

} // namespace

int h2y_tonemap_curve(int src_peak, int dst_peak, int relative, float gain[H2Y_LIGHTDIST_BINS], float *cap, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!gain || !cap) { *why = "null gain table or cap"; return H2Y_EINVAL; }
    if (const char *w = tonemap_params_why(src_peak, dst_peak, relative)) { *why = w; return H2Y_EINVAL; }
    const double W = pq_n(src_peak / 10000.0), max_lum = pq_n(dst_peak / 10000.0) / W, ks = 1.5 * max_lum - 0.5;
    const double u = relative ? dst_peak / 10000.0 : 1.0, inv_u = relative ? 10000.0 / dst_peak : 1.0;
    gain[0] = (float)inv_u;
    for (uint32_t k = 1; k < H2Y_LIGHTDIST_BINS; k++) {
        const uint32_t bits = H2Y_LIGHTDIST_FIRST_BITS + ((k - 1u) << 14);
        float ef;
        memcpy(&ef, &bits, sizeof ef);
        const double e = ef, n = pq_n(e) / W, e1 = n < 1.0 ? n : 1.0;
        if (e1 < ks) { gain[k] = (float)inv_u; continue; }
        const double t = (e1 - ks) / (1.0 - ks), t2 = t * t, t3 = t2 * t;
        const double e2 = (2.0 * t3 - 3.0 * t2 + 1.0) * ks + (t3 - 2.0 * t2 + t) * (1.0 - ks) + (-2.0 * t3 + 3.0 * t2) * max_lum;
        gain[k] = (float)(pq_n_inv(e2 * W) / (e * u));
    }
    *cap = relative ? 1.0f : (float)(dst_peak / 10000.0);
    return H2Y_OK;
}

/* k_tonemap's arguments for frames of width x height and a pair of peaks, but for the device table; the checks of both entries */
static int tonemap_args_of(h2y_ctx *ctx, int width, int height, int sample_type, int src_peak, int dst_peak, int relative,
                           tonemap_args &a, std::vector<float> &gain)
{
    if (sample_type == H2Y_SAMPLE_U16)
        return fail(ctx, H2Y_EUNSUPPORTED, "tone mapping works in linear light on float or half planes, not on U16 samples");
    if (sample_type != H2Y_SAMPLE_F32 && sample_type != H2Y_SAMPLE_F16) return fail(ctx, H2Y_EINVAL, "bad sample type %d", sample_type);
    int rc = picture_size_check(ctx, width, height);
    if (rc) return rc;
    gain.resize(H2Y_LIGHTDIST_BINS);
    const char *why;
    rc = h2y_tonemap_curve(src_peak, dst_peak, relative, gain.data(), &a.cap, &why);
    if (rc) return fail(ctx, rc, "tone map %d -> %d cd/m2, relative %d: %s", src_peak, dst_peak, relative, why);
    a.npix = (uint32_t)width * (uint32_t)height;
    return H2Y_OK;
}

int h2y_tonemap_batch(h2y_ctx *ctx, int width, int height, int sample_type, int src_peak, int dst_peak, int relative, int n_frames,
                      const void *const *d_src, void *const *d_dst)
{
    tonemap_args a{};
    std::vector<float> gain;
    gamut_frame *h;
    int rc = batch_enter(ctx);
    if (!rc) rc = tonemap_args_of(ctx, width, height, sample_type, src_peak, dst_peak, relative, a, gain);
    if (!rc) rc = pass_frames(ctx, n_frames, d_src, d_dst, false, h);
    if (!rc) rc = ensure(ctx, ctx->tonemap_gain, gain.size() * sizeof(float));
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->tonemap_gain.p, gain.data(), gain.size() * sizeof(float), hipMemcpyHostToDevice));
    a.gain = ctx->tonemap_gain.p;
    const int in_kind = sample_type == H2Y_SAMPLE_F16 ? H2Y_IN_F16 : H2Y_IN_F32;
    const uint64_t per_frame = h2y_gamut_chunks(in_kind, a.npix);
    rc = timed_launches(ctx, h, n_frames, H2Y_TONEMAP_FRAMES_PER_LAUNCH, "k_tonemap", [&](const gamut_frame *frames, int, int nf) {
        return h2y_launch_tonemap(in_kind, h2y_tonemap_grid(ctx->n_cu, per_frame * nf), ctx->stream, a, frames, nf);
    });
    if (rc) return rc;
    ctx->last_variant = std::string("k_tonemap<") + (in_kind == H2Y_IN_F16 ? "F16" : "F32") + (relative ? ",RELATIVE>" : ",ABSOLUTE>");
    return H2Y_OK;
}

/* The curve's ring stage: k_tonemap after the gamut stage's pass, with the gain table of its own */
int h2y_stream_tonemap(h2y_ctx *ctx, int src_peak, int dst_peak, int relative)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    if (ctx->s_kind != h2y_ctx::RING_FORWARD) return fail(ctx, H2Y_EINVAL, "tone mapping works on the forward rings only");
    if (ring_holds_signal(ctx)) return fail(ctx, H2Y_EINVAL, "the ring's planes hold signal, not light: tone mapping works in linear light");
    rc = arm_free(ctx, STAGE_TONEMAP, "the ring maps tones already");
    if (rc) return rc;
    const h2y_desc *d = &ctx->s_desc;
    auto st = std::make_unique<pass_stage<tonemap_args>>();
    st->launch = h2y_launch_tonemap;
    std::vector<float> gain;
    rc = tonemap_args_of(ctx, d->width, d->height, d->in_sample_type, src_peak, dst_peak, relative, st->a, gain);
    if (rc) return rc;
    if (d->src_transfer != H2Y_TRANSFER_LINEAR)
        return fail(ctx, H2Y_EUNSUPPORTED, "tone mapping works in linear light (src_transfer 8), not src_transfer %d", d->src_transfer);
    if (d->src_matrix != H2Y_MATRIX_GBR)
        return fail(ctx, H2Y_EUNSUPPORTED, "tone mapping needs a G,B,R source (src_matrix 0), not src_matrix %d", d->src_matrix);
    rc = unit_range_check(ctx, d, "tone-mapped planes are referred to their target");
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    st->in_kind = in_kind_of(d);
    st->grid = h2y_tonemap_grid(ctx->n_cu, h2y_gamut_chunks(st->in_kind, st->a.npix));
    float *d_gain = nullptr;
    st->table(d_gain, gain);
    st->a.gain = d_gain;
    st->table(st->tab, ring_planes_table(ctx));
    return stage_arm(ctx, STAGE_TONEMAP, std::move(st), "tone map");
}

/* ---- 3D LUT (--lut3d; the reference has no LUT step): include/hdr2yuv_hip.h states the definition ------------------------------------- */

/* a parsed .cube table: the nodes as the kernel reads them */
struct h2y_lut3d {
    int n = 0;
    float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {1.0f, 1.0f, 1.0f}, s[3] = {0.0f, 0.0f, 0.0f};
    std::string title;
    std::vector<lut3d_node> nodes;
};

namespace {

thread_local std::string lut3d_why; /* h2y_lut3d_parse's reason, until the thread's next call */

int lut3d_refuse(const char **why, int code, int line, const char *fmt, ...)
{
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    lut3d_why = line > 0 ? "line " + std::to_string(line) + ": " + buf : std::string(buf);
    *why = lut3d_why.c_str();
    return code;
}

/* the whole token as one binary32 number (strtof: decimal, scientific; "nan" and "inf" too, which the caller refuses) */
bool lut3d_number(const std::string &t, float *v)
{
    if (t.empty()) return false;
    char *e = nullptr;
    *v = strtof(t.c_str(), &e);
    return e == t.c_str() + t.size();
}

/* k numbers, all finite, in tok[1..k] */
bool lut3d_numbers(const std::vector<std::string> &tok, size_t k, float *v)
{
    if (tok.size() != k + 1) return false;
    for (size_t i = 0; i < k; i++)
        if (!lut3d_number(tok[i + 1], v + i) || !std::isfinite(v[i])) return false;
    return true;
}

} // namespace

int h2y_lut3d_parse(const char *text, size_t len, h2y_lut3d **out, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!text || !out) return lut3d_refuse(why, H2Y_EINVAL, 0, "null text or lut");
    *out = nullptr;
    auto lut = std::make_unique<h2y_lut3d>();
    size_t rows = 0, total = 0, pos = 0;
    int line = 0;
    const char *blank = " \t\r\f\v";
    while (pos < len) {
        size_t end = pos;
        while (end < len && text[end] != '\n') end++;
        std::string ln(text + pos, end - pos);
        pos = end + 1;
        line++;
        const size_t b = ln.find_first_not_of(blank);
        if (b == std::string::npos || ln[b] == '#') continue;
        ln = ln.substr(b, ln.find_last_not_of(blank) - b + 1);
        std::vector<std::string> tok;
        for (size_t p = 0; p < ln.size();) {
            const size_t q = ln.find_first_of(blank, p);
            tok.push_back(ln.substr(p, q == std::string::npos ? q : q - p));
            p = q == std::string::npos ? ln.size() : ln.find_first_not_of(blank, q);
        }
        float v[3];
        if (lut3d_number(tok[0], v)) { /* a table row */
            if (!lut->n) return lut3d_refuse(why, H2Y_EINVAL, line, "a table row before LUT_3D_SIZE");
            if (tok.size() != 3) return lut3d_refuse(why, H2Y_EINVAL, line, "a table row of %zu numbers, not three", tok.size());
            for (int c = 0; c < 3; c++) {
                if (!lut3d_number(tok[c], v + c)) return lut3d_refuse(why, H2Y_EINVAL, line, "'%.40s' is not a number", tok[c].c_str());
                if (!std::isfinite(v[c])) return lut3d_refuse(why, H2Y_EINVAL, line, "a value that is not finite");
            }
            if (rows == total) return lut3d_refuse(why, H2Y_EINVAL, line, "too many table rows: more than %d^3 = %zu", lut->n, total);
            lut->nodes[rows++] = lut3d_node{v[0], v[1], v[2], 0.0f};
            continue;
        }
        const std::string &key = tok[0];
        if (key == "LUT_1D_SIZE" || key == "LUT_1D_INPUT_RANGE")
            return lut3d_refuse(why, H2Y_EUNSUPPORTED, line, "%s: 1D LUTs and shaper + 3D files are not read", key.c_str());
        if (rows) return lut3d_refuse(why, H2Y_EINVAL, line, "'%.40s' after the first table row", key.c_str());
        if (key == "TITLE") {
            const size_t q0 = ln.find('"'), q1 = ln.rfind('"');
            if (q0 != std::string::npos && q1 > q0) lut->title = ln.substr(q0 + 1, q1 - q0 - 1);
            else {
                const size_t t = ln.find_first_not_of(blank, 5);
                lut->title = t == std::string::npos ? "" : ln.substr(t);
            }
        } else if (key == "LUT_3D_SIZE") {
            if (lut->n) return lut3d_refuse(why, H2Y_EINVAL, line, "LUT_3D_SIZE given twice");
            char *e = nullptr;
            const long n = tok.size() == 2 ? strtol(tok[1].c_str(), &e, 10) : 0;
            if (tok.size() != 2 || tok[1].empty() || e != tok[1].c_str() + tok[1].size())
                return lut3d_refuse(why, H2Y_EINVAL, line, "LUT_3D_SIZE takes one integer");
            if (n < 2 || n > 128) return lut3d_refuse(why, H2Y_EINVAL, line, "LUT_3D_SIZE %ld outside 2..128", n);
            lut->n = (int)n;
            total = (size_t)n * (size_t)n * (size_t)n;
            lut->nodes.resize(total);
        } else if (key == "DOMAIN_MIN" || key == "DOMAIN_MAX") {
            if (!lut3d_numbers(tok, 3, v)) return lut3d_refuse(why, H2Y_EINVAL, line, "%s takes three finite numbers", key.c_str());
            for (int c = 0; c < 3; c++) (key == "DOMAIN_MIN" ? lut->lo : lut->hi)[c] = v[c];
        } else if (key == "LUT_3D_INPUT_RANGE") {
            if (!lut3d_numbers(tok, 2, v)) return lut3d_refuse(why, H2Y_EINVAL, line, "LUT_3D_INPUT_RANGE takes two finite numbers");
            for (int c = 0; c < 3; c++) lut->lo[c] = v[0], lut->hi[c] = v[1];
        } else
            return lut3d_refuse(why, H2Y_EINVAL, line, "unknown keyword '%.40s'", key.c_str());
    }
    if (!lut->n) return lut3d_refuse(why, H2Y_EINVAL, 0, "no LUT_3D_SIZE");
    if (rows != total) return lut3d_refuse(why, H2Y_EINVAL, 0, "too few table rows: %zu, not %d^3 = %zu", rows, lut->n, total);
    for (int c = 0; c < 3; c++) {
        if (!(lut->hi[c] > lut->lo[c]))
            return lut3d_refuse(why, H2Y_EINVAL, 0, "the domain's maximum %.9g is not above its minimum %.9g (channel %c)", lut->hi[c], lut->lo[c], "rgb"[c]);
        lut->s[c] = (float)((double)(lut->n - 1) / ((double)lut->hi[c] - (double)lut->lo[c]));
        if (!std::isfinite(lut->s[c])) return lut3d_refuse(why, H2Y_EINVAL, 0, "the domain of channel %c is too narrow", "rgb"[c]);
    }
    *out = lut.release();
    return H2Y_OK;
}

void h2y_lut3d_free(h2y_lut3d *lut) { delete lut; }

int h2y_lut3d_info(const h2y_lut3d *lut, int *n, float domain[6], const char **title)
{
    if (!lut) return fail(nullptr, H2Y_EINVAL, "null lut");
    if (n) *n = lut->n;
    if (domain)
        for (int c = 0; c < 3; c++) domain[c] = lut->lo[c], domain[3 + c] = lut->hi[c];
    if (title) *title = lut->title.c_str();
    return H2Y_OK;
}

int h2y_lut3d_nodes(const h2y_lut3d *lut, float *rgb)
{
    if (!lut || !rgb) return fail(nullptr, H2Y_EINVAL, "null lut or nodes");
    for (size_t i = 0; i < lut->nodes.size(); i++) rgb[3 * i] = lut->nodes[i].r, rgb[3 * i + 1] = lut->nodes[i].g, rgb[3 * i + 2] = lut->nodes[i].b;
    return H2Y_OK;
}

/* the pass's constants: the table's, and in signal mode the scale step of (dst_bit_depth, dst_full_range, dst_matrix) as hlg_setup
 * derives it; the checks every entry shares */
static int lut3d_setup(h2y_ctx *ctx, const h2y_lut3d *lut, int interp, int signal, int dst_bit_depth, int dst_full_range, int dst_matrix,
                       lut3d_consts &c)
{
    if (!lut) return fail(ctx, H2Y_EINVAL, "null lut");
    if (interp != 0 && interp != 1) return fail(ctx, H2Y_EINVAL, "interp must be 0 (trilinear) or 1 (tetrahedral)");
    if (signal != 0 && signal != 1) return fail(ctx, H2Y_EINVAL, "signal must be 0 (planes) or 1 (signal)");
    c = lut3d_consts{};
    c.n = (uint32_t)lut->n;
    c.last = (float)(lut->n - 1);
    for (int k = 0; k < 3; k++) c.lo[k] = lut->lo[k], c.s[k] = lut->s[k];
    if (!signal) return H2Y_OK;
    if (dst_matrix != H2Y_MATRIX_GBR && dst_matrix != H2Y_MATRIX_BT2020NC)
        return fail(ctx, H2Y_EUNSUPPORTED, "a LUT's signal is scaled as G,B,R or BT.2020nc (dst_matrix 0 or 9), not dst_matrix %d", dst_matrix);
    if (dst_bit_depth < 8 || dst_bit_depth > 16) return fail(ctx, H2Y_EINVAL, "dst_bit_depth %d outside 8..16", dst_bit_depth);
    if (dst_full_range != 0 && dst_full_range != 1) return fail(ctx, H2Y_EINVAL, "dst_full_range must be 0 or 1");
    h2y_desc d{};
    d.in_sample_type = H2Y_SAMPLE_F32;
    d.src_bit_depth = 32;
    d.dst_bit_depth = dst_bit_depth;
    d.dst_full_range = dst_full_range;
    d.src_matrix = H2Y_MATRIX_GBR;
    d.dst_matrix = dst_matrix;
    d.src_transfer = d.dst_transfer = H2Y_TRANSFER_LINEAR;
    pix_params pp;
    derive_params(&d, &pp, false);
    c.mulY = pp.mulY, c.addY = pp.addY, c.mulC = pp.mulC, c.addC = pp.addC;
    return H2Y_OK;
}

template <int INTERP, int SIGNAL>
static void lut3d_host(const h2y_lut3d *lut, const lut3d_consts &c, int sample_type, size_t npix, const void *const src[3], void *const dst[3])
{
    for (size_t i = 0; i < npix; i++) {
        float v[3];
        for (int p = 0; p < 3; p++) {
            if (sample_type == H2Y_SAMPLE_F32) v[p] = static_cast<const float *>(src[p])[i];
            else v[p] = (float)static_cast<const _Float16 *>(src[p])[i]; /* exact */
        }
        lut3d_pixel<INTERP, SIGNAL>(lut3d_nodes16{lut->nodes.data()}, c, v[0], v[1], v[2]);
        for (int p = 0; p < 3; p++) {
            if (SIGNAL || sample_type == H2Y_SAMPLE_F32) static_cast<float *>(dst[p])[i] = v[p];
            else static_cast<_Float16 *>(dst[p])[i] = (_Float16)v[p]; /* to nearest even */
        }
    }
}

int h2y_lut3d_planes(const h2y_lut3d *lut, int interp, int signal, int dst_bit_depth, int dst_full_range, int dst_matrix, int sample_type,
                     size_t npix, const void *const src[3], void *const dst[3])
{
    if (sample_type != H2Y_SAMPLE_F32 && sample_type != H2Y_SAMPLE_F16)
        return fail(nullptr, H2Y_EUNSUPPORTED, "the LUT pass reads float or half planes, not sample type %d", sample_type);
    if (!src || !dst || !src[0] || !src[1] || !src[2] || !dst[0] || !dst[1] || !dst[2]) return fail(nullptr, H2Y_EINVAL, "null planes");
    lut3d_consts c{};
    const int rc = lut3d_setup(nullptr, lut, interp, signal, dst_bit_depth, dst_full_range, dst_matrix, c);
    if (rc) return rc;
    if (interp && signal) lut3d_host<1, 1>(lut, c, sample_type, npix, src, dst);
    else if (interp) lut3d_host<1, 0>(lut, c, sample_type, npix, src, dst);
    else if (signal) lut3d_host<0, 1>(lut, c, sample_type, npix, src, dst);
    else lut3d_host<0, 0>(lut, c, sample_type, npix, src, dst);
    return H2Y_OK;
}

/* k_lut3d's arguments for frames of width x height, but for the device table; the checks of both entries */
static int lut3d_args_of(h2y_ctx *ctx, int width, int height, int sample_type, const h2y_lut3d *lut, int interp, int signal,
                         int dst_bit_depth, int dst_full_range, int dst_matrix, lut3d_args &a)
{
    if (sample_type == H2Y_SAMPLE_U16)
        return fail(ctx, H2Y_EUNSUPPORTED, "the LUT pass works on float or half planes, not on U16 samples");
    if (sample_type != H2Y_SAMPLE_F32 && sample_type != H2Y_SAMPLE_F16) return fail(ctx, H2Y_EINVAL, "bad sample type %d", sample_type);
    int rc = picture_size_check(ctx, width, height);
    if (!rc) rc = lut3d_setup(ctx, lut, interp, signal, dst_bit_depth, dst_full_range, dst_matrix, a.c);
    if (rc) return rc;
    a.npix = (uint32_t)width * (uint32_t)height;
    return H2Y_OK;
}

static std::string lut3d_variant(int in_kind, int interp, int signal, int lds)
{
    return std::string(lds ? "k_lut3d_lds<" : "k_lut3d<") + (in_kind == H2Y_IN_F16 ? "F16" : "F32") + (interp ? ",TETRA" : ",TRILINEAR") +
           (signal ? ",SIGNAL>" : ",PLANES>");
}

/* does the pass read this table from LDS? (the context's "lut3d_lds" option, for tables small enough) */
static int lut3d_in_lds(const h2y_ctx *ctx, const h2y_lut3d *lut) { return ctx->opt_lut3d_lds && lut->n <= H2Y_LUT3D_LDS_MAX_N; }

int h2y_lut3d_batch(h2y_ctx *ctx, int width, int height, int sample_type, const h2y_lut3d *lut, int interp, int signal, int dst_bit_depth,
                    int dst_full_range, int dst_matrix, int n_frames, const void *const *d_src, void *const *d_dst)
{
    lut3d_args a{};
    gamut_frame *h;
    int rc = batch_enter(ctx);
    if (!rc) rc = lut3d_args_of(ctx, width, height, sample_type, lut, interp, signal, dst_bit_depth, dst_full_range, dst_matrix, a);
    if (!rc) rc = pass_frames(ctx, n_frames, d_src, d_dst, signal && sample_type == H2Y_SAMPLE_F16, h);
    if (rc) return rc;
    const size_t table_bytes = lut->nodes.size() * sizeof(lut3d_node);
    rc = ensure(ctx, ctx->lut3d, table_bytes);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->lut3d.p, lut->nodes.data(), table_bytes, hipMemcpyHostToDevice));
    a.nodes = ctx->lut3d.p;
    const int in_kind = sample_type == H2Y_SAMPLE_F16 ? H2Y_IN_F16 : H2Y_IN_F32;
    const int lds = lut3d_in_lds(ctx, lut);
    const uint64_t per_frame = h2y_lut3d_chunks(lds, in_kind, a.npix);
    rc = timed_launches(ctx, h, n_frames, H2Y_LUT3D_FRAMES_PER_LAUNCH, "k_lut3d", [&](const gamut_frame *frames, int, int nf) {
        return h2y_launch_lut3d(in_kind, interp, signal, lds, h2y_lut3d_grid(ctx->n_cu, lds, per_frame * nf), ctx->stream, a, frames, nf);
    });
    if (rc) return rc;
    ctx->last_variant = lut3d_variant(in_kind, interp, signal, lds);
    return H2Y_OK;
}

/* The LUT's ring stage, after the gamut and tone-map stages' passes and before the HLG and ICtCp stages': as pass_stage, with
 * k_lut3d's three more launch parameters and the table of its own (its launch wrapper takes them, so it is a stage of its own) */
struct lut3d_stage : ring_stage {
    lut3d_args a{};
    gamut_frame *tab = nullptr;
    int in_kind = H2Y_IN_F32, interp = 1, signal = 0, lds = 0;
    int grid = 1;
    int decoded(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, h2y_launch_lut3d(in_kind, interp, signal, lds, grid, ctx->stream, a, tab + k, 1));
        return H2Y_OK;
    }
    int run(h2y_ctx *, int) override { return H2Y_OK; }
};

/* does the open ring's LUT leave code values? (h2y_stream_hlg and h2y_stream_ictcp refuse such a ring) */
static bool lut3d_leaves_codes(const h2y_ctx *ctx)
{
    const lut3d_stage *st = stage_of<lut3d_stage>(ctx, STAGE_LUT3D);
    return st && st->signal;
}

int h2y_stream_lut3d(h2y_ctx *ctx, const h2y_lut3d *lut, int interp, int signal)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    if (ctx->s_kind != h2y_ctx::RING_FORWARD) return fail(ctx, H2Y_EINVAL, "a LUT is applied on the forward rings only");
    rc = arm_free(ctx, STAGE_LUT3D, "the ring applies a LUT already");
    if (rc) return rc;
    const h2y_desc *d = &ctx->s_desc;
    auto st = std::make_unique<lut3d_stage>();
    rc = lut3d_args_of(ctx, d->width, d->height, d->in_sample_type, lut, interp, signal, d->dst_bit_depth, d->dst_full_range, d->dst_matrix,
                           st->a);
    if (rc) return rc;
    if (d->src_matrix != H2Y_MATRIX_GBR)
        return fail(ctx, H2Y_EUNSUPPORTED, "a LUT needs a G,B,R source (src_matrix 0), not src_matrix %d", d->src_matrix);
    rc = unit_range_check(ctx, d, "a LUT's planes are referred to its own range");
    if (rc) return rc;
    if (signal) {
        if (ctx->s_stage[STAGE_HLG] || ctx->s_stage[STAGE_ICTCP])
            return fail(ctx, H2Y_EINVAL, "the ring writes %s: a LUT in signal mode leaves code values too", ctx->s_stage[STAGE_HLG] ? "HLG" : "ICtCp");
        if (d->in_sample_type != H2Y_SAMPLE_F32)
            return fail(ctx, H2Y_EUNSUPPORTED, "a LUT in signal mode leaves code-valued samples in the ring's decoded planes: they must be "
                                               "F32, not F16 (a half cannot hold them)");
        if (d->src_transfer != d->dst_transfer)
            return fail(ctx, H2Y_EUNSUPPORTED, "a LUT in signal mode is the ring's transfer: open it with equal transfers, not %d and %d",
                        d->src_transfer, d->dst_transfer);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    st->in_kind = in_kind_of(d);
    st->interp = interp, st->signal = signal;
    st->lds = lut3d_in_lds(ctx, lut);
    st->grid = h2y_lut3d_grid(ctx->n_cu, st->lds, h2y_lut3d_chunks(st->lds, st->in_kind, st->a.npix));
    lut3d_node *d_nodes = nullptr;
    st->table(d_nodes, lut->nodes);
    st->a.nodes = d_nodes;
    st->table(st->tab, ring_planes_table(ctx));
    return stage_arm(ctx, STAGE_LUT3D, std::move(st), "3D LUT");
}

/* ---- HLG (--hlg; the reference has no HLG transfer): include/hdr2yuv_hip.h states the definition ------------------------------------- */

int h2y_hlg_tables(int peak, int relative, float gain[H2Y_LIGHTDIST_BINS], float oetf[H2Y_LIGHTDIST_BINS], float *k, double *gamma,
                   const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!gain || !oetf || !k || !gamma) { *why = "null table, k or gamma"; return H2Y_EINVAL; }
    if (peak < H2Y_HLG_PEAK_MIN || peak > H2Y_HLG_PEAK_MAX) { *why = "peak outside 400 <= peak <= 2000 cd/m2"; return H2Y_EINVAL; }
    if (relative != 0 && relative != 1) { *why = "relative must be 0 or 1"; return H2Y_EINVAL; }
    const double g = 1.2 + 0.42 * log10(peak / 1000.0), p = (1.0 - g) / g;
    const double a = 0.17883277, b = 1.0 - 4.0 * a, c = 0.5 - a * log(4.0 * a);
    for (uint32_t j = 1; j < H2Y_LIGHTDIST_BINS; j++) {
        const uint32_t bits = H2Y_LIGHTDIST_FIRST_BITS + ((j - 1u) << 14);
        float nf;
        memcpy(&nf, &bits, sizeof nf);
        const double node = nf;
        gain[j] = (float)pow(node, p);
        oetf[j] = j >= (uint32_t)H2Y_HLG_OETF_FIRST ? (float)(a * log(12.0 * node - b) + c) : 0.0f;
    }
    gain[0] = (float)pow(256.0, -p); /* the factor of the reads below the first node: Y^p = (256 Y)^p 256^-p */
    oetf[0] = 0.0f;
    *k = relative ? 1.0f : (float)(10000.0 / peak);
    *gamma = g;
    return H2Y_OK;
}

/* the pass's constants and tables for a peak and the scale step of (dst_bit_depth, dst_full_range, dst_matrix), which is
 * derive_params' for a float source; the checks every entry shares */
static int hlg_setup(h2y_ctx *ctx, int peak, int relative, int dst_bit_depth, int dst_full_range, int dst_matrix, hlg_consts &c,
                     std::vector<float> &tables)
{
    if (dst_matrix != H2Y_MATRIX_GBR && dst_matrix != H2Y_MATRIX_BT2020NC)
        return fail(ctx, H2Y_EUNSUPPORTED, "an HLG signal is G,B,R or BT.2020nc (dst_matrix 0 or 9), not dst_matrix %d", dst_matrix);
    if (dst_bit_depth < 8 || dst_bit_depth > 16) return fail(ctx, H2Y_EINVAL, "dst_bit_depth %d outside 8..16", dst_bit_depth);
    if (dst_full_range != 0 && dst_full_range != 1) return fail(ctx, H2Y_EINVAL, "dst_full_range must be 0 or 1");
    tables.resize(2u * H2Y_LIGHTDIST_BINS);
    const char *why;
    double gamma;
    const int rc = h2y_hlg_tables(peak, relative, tables.data(), tables.data() + H2Y_LIGHTDIST_BINS, &c.k, &gamma, &why);
    if (rc) return fail(ctx, rc, "HLG at %d cd/m2, relative %d: %s", peak, relative, why);
    h2y_desc d{};
    d.in_sample_type = H2Y_SAMPLE_F32;
    d.src_bit_depth = 32;
    d.dst_bit_depth = dst_bit_depth;
    d.dst_full_range = dst_full_range;
    d.src_matrix = H2Y_MATRIX_GBR;
    d.dst_matrix = dst_matrix;
    d.src_transfer = d.dst_transfer = H2Y_TRANSFER_LINEAR;
    pix_params pp;
    derive_params(&d, &pp, false);
    c.mulY = pp.mulY, c.addY = pp.addY, c.mulC = pp.mulC, c.addC = pp.addC;
    return H2Y_OK;
}

int h2y_hlg_planes(int peak, int relative, int dst_bit_depth, int dst_full_range, int dst_matrix, int sample_type, size_t npix,
                   const void *const src[3], float *const dst[3])
{
    if (sample_type != H2Y_SAMPLE_F32 && sample_type != H2Y_SAMPLE_F16)
        return fail(nullptr, H2Y_EUNSUPPORTED, "the HLG pass reads float or half planes, not sample type %d", sample_type);
    if (!src || !dst || !src[0] || !src[1] || !src[2] || !dst[0] || !dst[1] || !dst[2]) return fail(nullptr, H2Y_EINVAL, "null planes");
    hlg_consts c{};
    std::vector<float> tables;
    const int rc = hlg_setup(nullptr, peak, relative, dst_bit_depth, dst_full_range, dst_matrix, c, tables);
    if (rc) return rc;
    const float *gain = tables.data(), *oetf_hi = tables.data() + H2Y_LIGHTDIST_BINS + H2Y_HLG_OETF_FIRST;
    for (size_t i = 0; i < npix; i++) {
        float v[3];
        for (int p = 0; p < 3; p++) {
            if (sample_type == H2Y_SAMPLE_F32) v[p] = static_cast<const float *>(src[p])[i];
            else v[p] = (float)static_cast<const _Float16 *>(src[p])[i]; /* exact */
        }
        hlg_pixel(gain, oetf_hi, c, v[0], v[1], v[2]);
        for (int p = 0; p < 3; p++) dst[p][i] = v[p];
    }
    return H2Y_OK;
}

/* k_hlg's arguments for frames of width x height, but for the device tables */
static int hlg_args_of(h2y_ctx *ctx, int width, int height, int sample_type, int peak, int relative, int dst_bit_depth,
                       int dst_full_range, int dst_matrix, hlg_args &a, std::vector<float> &tables)
{
    if (sample_type == H2Y_SAMPLE_U16)
        return fail(ctx, H2Y_EUNSUPPORTED, "the HLG pass works on display light in float or half planes, not on U16 samples");
    if (sample_type != H2Y_SAMPLE_F32 && sample_type != H2Y_SAMPLE_F16) return fail(ctx, H2Y_EINVAL, "bad sample type %d", sample_type);
    int rc = picture_size_check(ctx, width, height);
    if (!rc) rc = hlg_setup(ctx, peak, relative, dst_bit_depth, dst_full_range, dst_matrix, a.c, tables);
    if (rc) return rc;
    a.npix = (uint32_t)width * (uint32_t)height;
    return H2Y_OK;
}

int h2y_hlg_batch(h2y_ctx *ctx, int width, int height, int sample_type, int peak, int relative, int dst_bit_depth, int dst_full_range,
                  int dst_matrix, int n_frames, const void *const *d_src, void *const *d_dst)
{
    hlg_args a{};
    std::vector<float> tables;
    gamut_frame *h;
    int rc = batch_enter(ctx);
    if (!rc) rc = hlg_args_of(ctx, width, height, sample_type, peak, relative, dst_bit_depth, dst_full_range, dst_matrix, a, tables);
    if (!rc) rc = pass_frames(ctx, n_frames, d_src, d_dst, sample_type == H2Y_SAMPLE_F16, h);
    if (!rc) rc = ensure(ctx, ctx->hlg_tables, tables.size() * sizeof(float));
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->hlg_tables.p, tables.data(), tables.size() * sizeof(float), hipMemcpyHostToDevice));
    a.gain = ctx->hlg_tables.p;
    a.oetf = ctx->hlg_tables.p + H2Y_LIGHTDIST_BINS;
    const int in_kind = sample_type == H2Y_SAMPLE_F16 ? H2Y_IN_F16 : H2Y_IN_F32;
    const uint64_t per_frame = h2y_hlg_chunks(in_kind, a.npix);
    rc = timed_launches(ctx, h, n_frames, H2Y_HLG_FRAMES_PER_LAUNCH, "k_hlg", [&](const gamut_frame *frames, int, int nf) {
        return h2y_launch_hlg(in_kind, h2y_hlg_grid(ctx->n_cu, per_frame * nf), ctx->stream, a, frames, nf);
    });
    if (rc) return rc;
    ctx->last_variant = std::string("k_hlg<") + (in_kind == H2Y_IN_F16 ? "F16" : "F32") + (relative ? ",RELATIVE>" : ",ABSOLUTE>");
    return H2Y_OK;
}

/* The HLG pass's ring stage: k_hlg on F32 planes (pass_stage's in_kind as it stands) after the gamut, tone-map and LUT stages' passes,
 * with the two tables of its own */
int h2y_stream_hlg(h2y_ctx *ctx, int peak, int relative)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    if (ctx->s_kind != h2y_ctx::RING_FORWARD) return fail(ctx, H2Y_EINVAL, "the HLG pass works on the forward rings only");
    if (ctx->s_stage[STAGE_HLG]) return fail(ctx, H2Y_EINVAL, "the ring writes HLG already");
    if (ctx->s_stage[STAGE_ICTCP]) return fail(ctx, H2Y_EINVAL, "the ring writes ICtCp: its planes hold code values, not light");
    if (lut3d_leaves_codes(ctx)) return fail(ctx, H2Y_EINVAL, "the ring's LUT works in signal mode: its planes hold code values, not light");
    rc = arm_unstarted(ctx);
    if (rc) return rc;
    const h2y_desc *d = &ctx->s_desc;
    if (d->in_sample_type != H2Y_SAMPLE_F32)
        return fail(ctx, H2Y_EUNSUPPORTED, "the HLG pass leaves code-valued samples in the ring's decoded planes: they must be F32, not %s",
                    d->in_sample_type == H2Y_SAMPLE_F16 ? "F16 (a half cannot hold them)" : "U16");
    if (d->src_transfer != H2Y_TRANSFER_LINEAR || d->dst_transfer != H2Y_TRANSFER_LINEAR)
        return fail(ctx, H2Y_EUNSUPPORTED, "the HLG pass is the ring's transfer: open it with src_transfer 8 and dst_transfer 8, not %d and %d",
                    d->src_transfer, d->dst_transfer);
    if (d->src_matrix != H2Y_MATRIX_GBR)
        return fail(ctx, H2Y_EUNSUPPORTED, "the HLG pass needs a G,B,R source (src_matrix 0), not src_matrix %d", d->src_matrix);
    auto st = std::make_unique<pass_stage<hlg_args>>();
    st->launch = h2y_launch_hlg;
    std::vector<float> tables;
    rc = hlg_args_of(ctx, d->width, d->height, d->in_sample_type, peak, relative, d->dst_bit_depth, d->dst_full_range, d->dst_matrix, st->a, tables);
    if (!rc) rc = unit_range_check(ctx, d, "the HLG pass is the passthrough flow's");
    if (rc) return rc;
    pix_params pp;
    derive_params(d, &pp, false); /* the ring's own scale step, whatever else its descriptor says */
    st->a.c.mulY = pp.mulY, st->a.c.addY = pp.addY, st->a.c.mulC = pp.mulC, st->a.c.addC = pp.addC;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    st->grid = h2y_hlg_grid(ctx->n_cu, h2y_hlg_chunks(H2Y_IN_F32, st->a.npix));
    float *d_tables = nullptr;
    st->table(d_tables, tables);
    st->a.gain = d_tables;
    st->a.oetf = d_tables + H2Y_LIGHTDIST_BINS;
    st->table(st->tab, ring_planes_table(ctx));
    return stage_arm(ctx, STAGE_HLG, std::move(st), "HLG");
}

/* ---- ICtCp (--ictcp; the reference's matrix 14 is its unbuilt Y'u'v' variant): include/hdr2yuv_hip.h states the definition ------------ */

/* k_ictcp's arguments for frames of width x height: H.273's scale of the depth and range, PQ10000_r's tables (what code1 reads of
 * pix_params); the checks both entries share */
static int ictcp_args_of(h2y_ctx *ctx, int width, int height, int sample_type, int dst_bit_depth, int dst_full_range, ictcp_args &a)
{
    if (sample_type == H2Y_SAMPLE_U16)
        return fail(ctx, H2Y_EUNSUPPORTED, "the ICtCp pass works on display light in float or half planes, not on U16 samples");
    if (sample_type != H2Y_SAMPLE_F32 && sample_type != H2Y_SAMPLE_F16) return fail(ctx, H2Y_EINVAL, "bad sample type %d", sample_type);
    const int rc = picture_size_check(ctx, width, height);
    if (rc) return rc;
    if (dst_bit_depth < 8 || dst_bit_depth > 16) return fail(ctx, H2Y_EINVAL, "dst_bit_depth %d outside 8..16", dst_bit_depth);
    if (dst_full_range != 0 && dst_full_range != 1) return fail(ctx, H2Y_EINVAL, "dst_full_range must be 0 or 1");
    a = ictcp_args{};
    a.npix = (uint32_t)width * (uint32_t)height;
    const float s = (float)(1u << (dst_bit_depth - 8)), top = (float)((1u << dst_bit_depth) - 1u);
    a.oY = dst_full_range ? top : 219.0f * s;
    a.aY = dst_full_range ? 0.0f : 16.0f * s;
    a.oC = dst_full_range ? top : 224.0f * s;
    a.aC = dst_full_range ? (float)(1u << (dst_bit_depth - 1)) : 128.0f * s;
    a.top = top;
    return H2Y_OK;
}

/* PQ10000_r's tables into the arguments, on the context's device */
static int ictcp_tables(h2y_ctx *ctx, ictcp_args &a)
{
    const int rc = ensure_tfn(ctx, H2Y_TFN_PQ_R);
    if (rc) return rc;
    a.pp = pix_params{};
    a.pp.dst_tf = H2Y_TF_PQ;
    a.pp.dst_fn = H2Y_TFN_PQ_R;
    a.pp.tf_ext[1] = ctx->d_tfn_ext[H2Y_TFN_PQ_R];
    a.table_r = ctx->d_tfn[H2Y_TFN_PQ_R];
    return H2Y_OK;
}

int h2y_ictcp_batch(h2y_ctx *ctx, int width, int height, int sample_type, int dst_bit_depth, int dst_full_range, int n_frames,
                    const void *const *d_src, void *const *d_dst)
{
    ictcp_args a{};
    gamut_frame *h;
    int rc = batch_enter(ctx);
    if (!rc) rc = ictcp_args_of(ctx, width, height, sample_type, dst_bit_depth, dst_full_range, a);
    if (!rc) rc = pass_frames(ctx, n_frames, d_src, d_dst, sample_type == H2Y_SAMPLE_F16, h);
    if (!rc) rc = ictcp_tables(ctx, a);
    if (rc) return rc;
    const int in_kind = sample_type == H2Y_SAMPLE_F16 ? H2Y_IN_F16 : H2Y_IN_F32;
    const uint64_t per_frame = h2y_ictcp_chunks(in_kind, a.npix);
    rc = timed_launches(ctx, h, n_frames, H2Y_ICTCP_FRAMES_PER_LAUNCH, "k_ictcp", [&](const gamut_frame *frames, int, int nf) {
        return h2y_launch_ictcp(in_kind, h2y_ictcp_grid(ctx->n_cu, per_frame * nf), ctx->stream, a, frames, nf);
    });
    if (rc) return rc;
    ctx->last_variant = in_kind == H2Y_IN_F16 ? "k_ictcp<F16>" : "k_ictcp<F32>";
    return H2Y_OK;
}

/* The ICtCp pass's ring stage: k_ictcp on F32 planes (pass_stage's in_kind as it stands) after the gamut, tone-map and LUT stages'
 * passes; the table is the context's */
int h2y_stream_ictcp(h2y_ctx *ctx)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    if (ctx->s_kind != h2y_ctx::RING_FORWARD) return fail(ctx, H2Y_EINVAL, "the ICtCp pass works on the forward rings only");
    if (ctx->s_stage[STAGE_ICTCP]) return fail(ctx, H2Y_EINVAL, "the ring writes ICtCp already");
    if (ctx->s_stage[STAGE_HLG]) return fail(ctx, H2Y_EINVAL, "the ring writes HLG: its planes hold code values, not light");
    if (lut3d_leaves_codes(ctx)) return fail(ctx, H2Y_EINVAL, "the ring's LUT works in signal mode: its planes hold code values, not light");
    rc = arm_unstarted(ctx);
    if (rc) return rc;
    const h2y_desc *d = &ctx->s_desc;
    if (d->in_sample_type != H2Y_SAMPLE_F32)
        return fail(ctx, H2Y_EUNSUPPORTED, "the ICtCp pass leaves code-valued samples in the ring's decoded planes: they must be F32, not %s",
                    d->in_sample_type == H2Y_SAMPLE_F16 ? "F16 (a half cannot hold them)" : "U16");
    if (d->src_transfer != H2Y_TRANSFER_LINEAR || d->dst_transfer != H2Y_TRANSFER_LINEAR)
        return fail(ctx, H2Y_EUNSUPPORTED, "the ICtCp pass is the ring's transfer: open it with src_transfer 8 and dst_transfer 8, not %d and %d",
                    d->src_transfer, d->dst_transfer);
    if (d->src_matrix != H2Y_MATRIX_GBR)
        return fail(ctx, H2Y_EUNSUPPORTED, "the ICtCp pass needs a G,B,R source (src_matrix 0), not src_matrix %d", d->src_matrix);
    if (d->dst_matrix != H2Y_MATRIX_GBR)
        return fail(ctx, H2Y_EUNSUPPORTED, "the ICtCp pass is the ring's matrix: open it with dst_matrix 0, not dst_matrix %d", d->dst_matrix);
    auto st = std::make_unique<pass_stage<ictcp_args>>();
    st->launch = h2y_launch_ictcp;
    rc = ictcp_args_of(ctx, d->width, d->height, d->in_sample_type, d->dst_bit_depth, d->dst_full_range, st->a);
    if (!rc) rc = unit_range_check(ctx, d, "the ICtCp pass is the passthrough flow's");
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = ictcp_tables(ctx, st->a);
    if (rc) return rc;
    st->grid = h2y_ictcp_grid(ctx->n_cu, h2y_ictcp_chunks(H2Y_IN_F32, st->a.npix));
    st->table(st->tab, ring_planes_table(ctx));
    return stage_arm(ctx, STAGE_ICTCP, std::move(st), "ICtCp");
}

/* ---- light of HLG code planes (--linearize 1 --src_hlg 1): include/hdr2yuv_hip.h states the definition ----------------------------- */

int h2y_hlg_inverse_tables(int peak, float ootf[H2Y_LIGHTDIST_BINS], float inv[H2Y_LIGHTDIST_BINS], float *kappa, double *gamma,
                           const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!ootf || !inv || !kappa || !gamma) { *why = "null table, kappa or gamma"; return H2Y_EINVAL; }
    if (peak < H2Y_HLG_PEAK_MIN || peak > H2Y_HLG_PEAK_MAX) { *why = "peak outside 400 <= peak <= 2000 cd/m2"; return H2Y_EINVAL; }
    const double g = 1.2 + 0.42 * log10(peak / 1000.0), q = g - 1.0;
    const double a = 0.17883277, b = 1.0 - 4.0 * a, c = 0.5 - a * log(4.0 * a);
    for (uint32_t j = 1; j < H2Y_LIGHTDIST_BINS; j++) {
        const uint32_t bits = H2Y_LIGHTDIST_FIRST_BITS + ((j - 1u) << 14);
        float nf;
        memcpy(&nf, &bits, sizeof nf);
        const double node = nf;
        ootf[j] = (float)pow(node, q);
        inv[j] = j >= (uint32_t)H2Y_HLG_INV_FIRST ? (float)((exp((node - c) / a) + b) / 12.0) : 0.0f;
    }
    ootf[0] = (float)pow(256.0, -q); /* the factor of the reads below the first node: Y^q = (256 Y)^q 256^-q */
    inv[0] = 0.0f;
    *kappa = (float)(peak / 10000.0);
    *gamma = g;
    return H2Y_OK;
}

int h2y_hlg_inverse_planes(int peak, size_t npix, const float *const src[3], float *const dst[3])
{
    if (!src || !dst || !src[0] || !src[1] || !src[2] || !dst[0] || !dst[1] || !dst[2]) return fail(nullptr, H2Y_EINVAL, "null planes");
    std::vector<float> tables(2u * H2Y_LIGHTDIST_BINS);
    float kappa;
    double gamma;
    const char *why;
    const int rc = h2y_hlg_inverse_tables(peak, tables.data(), tables.data() + H2Y_LIGHTDIST_BINS, &kappa, &gamma, &why);
    if (rc) return fail(nullptr, rc, "HLG source at %d cd/m2: %s", peak, why);
    const float *ootf = tables.data(), *inv_hi = tables.data() + H2Y_LIGHTDIST_BINS + H2Y_HLG_INV_FIRST;
    for (size_t i = 0; i < npix; i++) {
        float g = src[0][i], b = src[1][i], r = src[2][i];
        hlg_inverse_pixel(ootf, inv_hi, kappa, g, b, r);
        dst[0][i] = g, dst[1][i] = b, dst[2][i] = r;
    }
    return H2Y_OK;
}

int hlgsrc_args_of(h2y_ctx *ctx, const codelight_plan &p, int peak, hlgsrc_args &a)
{
    if (p.matrix == H2Y_MATRIX_ICTCP)
        return fail(ctx, H2Y_EUNSUPPORTED, "matrix_coeffs 14 (ICtCp) is PQ's here: BT.2100's HLG form of ICtCp has other coefficients and is not built");
    std::vector<float> tables(2u * H2Y_LIGHTDIST_BINS);
    double gamma;
    const char *why;
    int rc = h2y_hlg_inverse_tables(peak, tables.data(), tables.data() + H2Y_LIGHTDIST_BINS, &a.kappa, &gamma, &why);
    if (rc) return fail(ctx, rc, "HLG source at %d cd/m2: %s", peak, why);
    rc = ensure(ctx, ctx->hlgsrc_tables, tables.size() * sizeof(float));
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->hlgsrc_tables.p, tables.data(), tables.size() * sizeof(float), hipMemcpyHostToDevice));
    a.c = p.a;
    a.ootf = ctx->hlgsrc_tables.p;
    a.inv = ctx->hlgsrc_tables.p + H2Y_LIGHTDIST_BINS;
    return H2Y_OK;
}

/* ---- light of SDR code planes (--linearize 1 --src_sdr 1): include/hdr2yuv_hip.h states the definition ------------------------------ */

static bool sdr_white_ok(int white) { return white >= H2Y_SDR_WHITE_MIN && white <= H2Y_SDR_WHITE_MAX; }

int h2y_sdr_inverse_planes(int white, size_t npix, const float *const src[3], float *const dst[3])
{
    if (!src || !dst || !src[0] || !src[1] || !src[2] || !dst[0] || !dst[1] || !dst[2]) return fail(nullptr, H2Y_EINVAL, "null planes");
    if (!sdr_white_ok(white)) return fail(nullptr, H2Y_EINVAL, "SDR source: white(%d) outside %d <= white <= %d cd/m2", white, H2Y_SDR_WHITE_MIN, H2Y_SDR_WHITE_MAX);
    const float kappa = (float)(white / 10000.0);
    for (int c = 0; c < 3; c++)
        for (size_t i = 0; i < npix; i++) {
            const float v = src[c][i], vc = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f; /* step 4s */
            dst[c][i] = tf_to_linear(H2Y_TF_BT1886, vc) * kappa; /* steps 5s (the careful tier's function), 6s: one product, one rounding */
        }
    return H2Y_OK;
}

/* bt1886_f's tables into the plan: what light1<true> reads of pix_params (codelight_tables with the BT.1886 stage) */
int sdrsrc_tables(h2y_ctx *ctx, codelight_plan &p, int white, float &kappa)
{
    if (p.matrix == H2Y_MATRIX_ICTCP)
        return fail(ctx, H2Y_EUNSUPPORTED, "matrix_coeffs 14 (ICtCp) is PQ's here: an SDR source is G,B,R (0), BT.709 (1) or BT.2020nc (9)");
    if (!sdr_white_ok(white)) return fail(ctx, H2Y_EINVAL, "SDR source: white(%d) outside %d <= white <= %d cd/m2", white, H2Y_SDR_WHITE_MIN, H2Y_SDR_WHITE_MAX);
    const int rc = ensure_tfn(ctx, H2Y_TFN_G24);
    if (rc) return rc;
    pix_params &pp = p.a.pp;
    pp = pix_params{};
    pp.convert_transfer = 2;
    pp.src_tf = H2Y_TF_BT1886;
    pp.src_fn = H2Y_TFN_G24;
    pp.norm_identity = 1; /* the kernel normalises the codes itself */
    for (int c = 0; c < 3; c++) pp.range[c] = 1.0f;
    pp.tf_ext[0] = ctx->d_tfn_ext[H2Y_TFN_G24];
    p.a.table = ctx->d_tfn[H2Y_TFN_G24];
    kappa = (float)(white / 10000.0);
    return H2Y_OK;
}

/* ---- signal of code planes (--linearize 1 --src_signal 1): include/hdr2yuv_hip.h states the definition ------------------------------- */

static const char *const kSignalIctcp = "matrix_coeffs 14 (ICtCp) gives L'M'S', not R'G'B': the signal of code planes is G,B,R (0), BT.709 (1) or BT.2020nc (9)";

int sigsrc_check(h2y_ctx *ctx, const codelight_plan &p)
{
    if (p.matrix == H2Y_MATRIX_ICTCP) return fail(ctx, H2Y_EUNSUPPORTED, "%s", kSignalIctcp);
    return H2Y_OK;
}

bool ring_holds_signal(const h2y_ctx *ctx) { return ctx->s_kind == h2y_ctx::RING_FORWARD && ctx->s_src.kind == decode_src::PQCODE && ctx->s_src.signal; }

int h2y_code_signal_planes(const h2y_codelight_desc *d, size_t npix, const uint16_t *const src[3], float *const dst[3])
{
    int rc = codelight_desc_check(nullptr, d);
    if (rc) return rc;
    if (d->matrix_coeffs == H2Y_MATRIX_ICTCP) return fail(nullptr, H2Y_EUNSUPPORTED, "%s", kSignalIctcp);
    if (!src || !dst || !src[0] || !src[1] || !src[2] || !dst[0] || !dst[1] || !dst[2]) return fail(nullptr, H2Y_EINVAL, "null planes");
    codelight_args a{};
    codelight_norm(d, a);
    h2y_code_signal_host(d->matrix_coeffs, a, npix, src, dst);
    return H2Y_OK;
}

/* ---- dither: the reduction to the output bit depth (--dither; the reference's to-do list names it): include/hdr2yuv_hip.h states
 * the definition ------------------------------------------------------------------------------------------------------------------ */

static const char *const kDitherMode[3] = {"cut", "ordered", "noise"};

template <int MODE>
static void dither_offsets_of(uint32_t kp, uint32_t s, int width, int height, uint16_t *t)
{
    for (int y = 0; y < height; y++) {
        const uint32_t row = dither_row<MODE>(kp, (uint32_t)y);
        for (int x = 0; x < width; x++) t[(size_t)y * width + x] = (uint16_t)dither_t<MODE>(kp, row, (uint32_t)x, s);
    }
}

int h2y_dither_offsets(int mode, int shift, int temporal, uint32_t seed, uint32_t frame, int plane, int width, int height, uint16_t *t)
{
    if (!t) return fail(nullptr, H2Y_EINVAL, "null table");
    if (mode < 0 || mode > 2) return fail(nullptr, H2Y_EINVAL, "mode must be 0 (cut), 1 (ordered) or 2 (noise)");
    if (shift < 1 || shift > 8) return fail(nullptr, H2Y_EINVAL, "shift must be 1..8");
    if (temporal != 0 && temporal != 1) return fail(nullptr, H2Y_EINVAL, "temporal must be 0 or 1");
    if (plane < 0 || plane > 2) return fail(nullptr, H2Y_EINVAL, "plane must be 0..2");
    if (width < 1 || height < 1) return fail(nullptr, H2Y_EINVAL, "width and height must be >= 1");
    const uint32_t kp = dither_plane_key(seed ^ 0x9E3779B9u, (uint32_t)temporal, frame, (uint32_t)plane);
    if (mode == H2Y_DITHER_ORDERED) dither_offsets_of<H2Y_DITHER_ORDERED>(kp, (uint32_t)shift, width, height, t);
    else if (mode == H2Y_DITHER_NOISE) dither_offsets_of<H2Y_DITHER_NOISE>(kp, (uint32_t)shift, width, height, t);
    else dither_offsets_of<H2Y_DITHER_CUT>(kp, (uint32_t)shift, width, height, t);
    return H2Y_OK;
}

static int dither_check(h2y_ctx *ctx, int width, int height, int chroma, int src_depth, int dst_depth, int full_range, int gbr, int mode,
                        int temporal)
{
    if (chroma == 2) return fail(ctx, H2Y_EUNSUPPORTED, "chroma_format_idc 2 (4:2:2) is not dithered");
    if (chroma != H2Y_CHROMA_420 && chroma != H2Y_CHROMA_444) return fail(ctx, H2Y_EINVAL, "chroma_format_idc must be 1 or 3");
    if (width < 1 || height < 1 || (uint64_t)width * (uint64_t)height >= (1ull << 28)) return fail(ctx, H2Y_EINVAL, "dither: bad picture size");
    if (chroma == H2Y_CHROMA_420 && ((width | height) & 1)) return fail(ctx, H2Y_EINVAL, "dither 4:2:0: width and height must be even");
    if (dst_depth < 8 || src_depth > 16 || dst_depth >= src_depth || src_depth - dst_depth > 8)
        return fail(ctx, H2Y_EINVAL, "dither: depths must be 8 <= dst < src <= 16, at most 8 bits apart (src %d, dst %d)", src_depth, dst_depth);
    if ((full_range != 0 && full_range != 1) || (gbr != 0 && gbr != 1)) return fail(ctx, H2Y_EINVAL, "full_range and gbr must be 0 or 1");
    if (mode < 0 || mode > 2) return fail(ctx, H2Y_EINVAL, "dither mode must be 0 (cut), 1 (ordered) or 2 (noise)");
    if (temporal != 0 && temporal != 1) return fail(ctx, H2Y_EINVAL, "dither: temporal must be 0 or 1");
    return H2Y_OK;
}

/* k_dither's arguments for checked parameters: planes one after the other, the clamp write_yuv's at the destination depth */
static dither_args dither_args_of(int width, int height, int chroma, int src_depth, int dst_depth, int full_range, int gbr, int temporal,
                                  uint32_t seed)
{
    dither_args a{};
    uint32_t off[3];
    contiguous_planes(width, height, chroma, off);
    const clip_limits c = make_clip(dst_depth, full_range);
    for (int p = 0; p < 3; p++) {
        const bool luma_like = p == 0 || gbr;
        const plane_dim d = plane_dims(width, height, chroma, p);
        a.p[p] = h2y_dither_plane(d.w, d.h, off[p], luma_like ? c.minVR : c.minVRC, luma_like ? c.maxVR : c.maxVRC);
    }
    a.shift = (uint32_t)(src_depth - dst_depth);
    a.key = seed ^ 0x9E3779B9u;
    a.temporal = (uint32_t)temporal;
    return a;
}

static size_t dither_frame_bytes(const dither_args &a) { return ((size_t)a.p[2].off + a.p[2].n) * sizeof(uint16_t); }

static int dither_grid(const h2y_ctx *ctx, const dither_args &a, int n_frames)
{
    return unit_grid(ctx, (uint64_t)n_frames * (a.p[0].chunks + a.p[1].chunks + a.p[2].chunks));
}

int h2y_dither_batch(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int src_depth, int dst_depth, int full_range, int gbr,
                     int mode, int temporal, uint32_t seed, uint32_t first_frame, int n_frames, const uint16_t *const *d_src,
                     uint16_t *const *d_dst)
{
    int rc = batch_enter(ctx);
    if (!rc) rc = dither_check(ctx, width, height, chroma_format_idc, src_depth, dst_depth, full_range, gbr, mode, temporal);
    if (!rc) rc = pairs_check(ctx, n_frames, d_src, d_dst);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const dither_args a = dither_args_of(width, height, chroma_format_idc, src_depth, dst_depth, full_range, gbr, temporal, seed);
    dither_frame *h;
    rc = frame_table(ctx, n_frames, h);
    if (rc) return rc;
    for (int f = 0; f < n_frames; f++) h[f] = dither_frame{d_src[f], d_dst[f]};
    rc = timed_launches(ctx, h, n_frames, H2Y_DITHER_FRAMES_PER_LAUNCH, "k_dither", [&](const dither_frame *frames, int f0, int nf) {
        dither_args b = a;
        b.first = first_frame + (uint32_t)f0;
        return h2y_launch_dither(mode, dither_grid(ctx, b, nf), ctx->stream, b, frames, nf);
    });
    if (rc) return rc;
    ctx->last_variant = std::string("k_dither<") + kDitherMode[mode] + ">";
    return H2Y_OK;
}

/* Dither's ring stage, the last of a slot's: on a ring that produces its frame it reduces the frame that would go down -- the
 * conversion's, or the scale stage's -- into a frame of its own, on the device and pinned, which goes down and is handed out in
 * that frame's place; on a ring without a producer it reduces the slot's input into its output.  The k-th submitted frame has
 * number first + k. */
struct dither_stage : ring_stage {
    struct slot {
        uint16_t *d = nullptr, *h = nullptr;
    };
    std::vector<slot> ss;
    dither_args a{};
    dither_frame *tab = nullptr;
    size_t bytes = 0; /* of the frame */
    int mode = 0;
    uint32_t submitted = 0;
    bool down = true; /* false: a pack stage armed behind this one sends its own frame down instead */
    int run(h2y_ctx *ctx, int k) override
    {
        dither_args b = a;
        b.first = a.first + submitted++;
        HIP_TRY(ctx, h2y_launch_dither(mode, dither_grid(ctx, b, 1), ctx->stream, b, tab + k, 1));
        return H2Y_OK;
    }
    int download(h2y_ctx *ctx, int k) override
    {
        if (ss[k].d && down) HIP_TRY(ctx, hipMemcpyAsync(ss[k].h, ss[k].d, bytes, hipMemcpyDeviceToHost, ctx->s_d2h));
        return H2Y_OK;
    }
};

/* arm the open ring's frame (a scale stage's where one is armed), reduced to dst_depth */
static int dither_arm(h2y_ctx *ctx, int dst_depth, int gbr, int mode, int temporal, uint32_t seed, uint32_t first_frame)
{
    const ring_frame &f = ctx->s_frame;
    scale_stage *sc = stage_of<scale_stage>(ctx, STAGE_SCALE);
    const int width = sc ? (int)sc->g.p[0].dw : f.width, height = sc ? (int)sc->g.p[0].dh : f.height;
    int rc = dither_check(ctx, width, height, f.chroma, f.depth, dst_depth, f.full_range, gbr, mode, temporal);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto st = std::make_unique<dither_stage>();
    dither_stage *di = st.get();
    di->a = dither_args_of(width, height, f.chroma, f.depth, dst_depth, f.full_range, gbr, temporal, seed);
    di->a.first = first_frame;
    di->mode = mode;
    di->bytes = dither_frame_bytes(di->a);
    const int depth = (int)ctx->ss.size();
    std::vector<dither_frame> tab(depth);
    di->ss.resize(depth);
    for (int k = 0; k < depth; k++) {
        if (!f.in_input) {
            di->dev_alloc(di->ss[k].d, std::max<size_t>(di->bytes, 16));
            di->pin_alloc(di->ss[k].h, std::max<size_t>(di->bytes, 16));
        }
        const uint16_t *src = sc && !f.in_input ? sc->ss[k].d : frame_base(ctx, k);
        tab[k] = dither_frame{src, f.in_input ? ctx->ss[k].d_out : di->ss[k].d};
    }
    di->table(di->tab, tab);
    rc = stage_arm(ctx, STAGE_DITHER, std::move(st), "dither");
    if (rc || f.in_input) return rc;
    if (sc) sc->down = false; /* the scaled frame stays on the device: its reduction goes down */
    ring_frame_stays(ctx);
    for (int k = 0; k < depth; k++) ctx->ss[k].result = di->ss[k].h;
    return H2Y_OK;
}

int h2y_stream_dither(h2y_ctx *ctx, int dst_depth, int mode, int temporal, uint32_t seed, uint32_t first_frame)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    if (ctx->s_kind != h2y_ctx::RING_FORWARD) return fail(ctx, H2Y_EINVAL, "only a forward ring is armed for dither");
    if (ctx->s_stage[STAGE_DITHER]) return fail(ctx, H2Y_EINVAL, "the ring dithers already");
    if (ctx->s_stage[STAGE_PACK]) return fail(ctx, H2Y_EINVAL, "the ring packs already: arm dither before pack");
    if (ctx->s_stage[STAGE_COMPARE] || ctx->s_stage[STAGE_HISTOGRAM] || ctx->s_stage[STAGE_SSIM] || ctx->s_stage[STAGE_DELTAE])
        return fail(ctx, H2Y_EUNSUPPORTED, "a ring armed for comparison, histograms, SSIM or Delta E is not dithered: compare or count the written file instead");
    if (ctx->s_desc.dst_matrix == H2Y_MATRIX_YUVPRIME2) return fail(ctx, H2Y_EUNSUPPORTED, "a Y'u'v' ring (dst_matrix_coeffs 15) is not dithered");
    rc = arm_unstarted(ctx);
    if (rc) return rc;
    return dither_arm(ctx, dst_depth, 0, mode, temporal, seed, first_frame);
}

/* A ring that only dithers: the slot's input is the frame's three planes, its output the reduced frame */
int h2y_dither_stream_open(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int src_depth, int dst_depth, int full_range, int gbr,
                           int mode, int temporal, uint32_t seed, uint32_t first_frame, int depth)
{
    int rc = ring_may_open(ctx);
    if (!rc) rc = dither_check(ctx, width, height, chroma_format_idc, src_depth, dst_depth, full_range, gbr, mode, temporal);
    if (!rc) rc = open_planes_ring(ctx, width, height, chroma_format_idc, src_depth, full_range, gbr,
                                   dither_frame_bytes(dither_args_of(width, height, chroma_format_idc, src_depth, dst_depth, full_range, gbr, temporal, seed)),
                                   depth);
    if (rc) return rc;
    rc = dither_arm(ctx, dst_depth, gbr, mode, temporal, seed, first_frame);
    if (rc) stream_free(ctx);
    return rc;
}

/* ---- sample packings: byte and semi-planar frames (--dst_pack, --src_pack): include/hdr2yuv_hip.h states the definition ------------ */

static const char *const kPackName[4] = {"PLANAR16", "PLANAR8", "NV12", "P010"};

size_t h2y_pack_frame_bytes(int width, int height, int chroma_format_idc, int packing)
{
    if (width < 1 || height < 1 || !pack_legal(chroma_format_idc, 0, packing)) return 0;
    const size_t n = (size_t)width * (size_t)height;
    const size_t nc = (size_t)pack_cw((uint32_t)width, chroma_format_idc) * (size_t)pack_ch((uint32_t)height, chroma_format_idc);
    return (n + 2 * nc) * pack_elem_bytes(packing);
}

static int pack_check(h2y_ctx *ctx, int width, int height, int chroma, int bit_depth, int packing)
{
    if (chroma == 2) return fail(ctx, H2Y_EUNSUPPORTED, "chroma_format_idc 2 (4:2:2) is not packed");
    if (chroma != H2Y_CHROMA_420 && chroma != H2Y_CHROMA_444) return fail(ctx, H2Y_EINVAL, "chroma_format_idc must be 1 or 3");
    if (width < 1 || height < 1 || (uint64_t)width * (uint64_t)height >= (1ull << 28)) return fail(ctx, H2Y_EINVAL, "pack: bad picture size");
    if (packing == H2Y_PACK_PLANAR16) return fail(ctx, H2Y_EINVAL, "packing 0 (planar16) is the frame as it is: nothing to pack or unpack");
    if (packing < 0 || packing > H2Y_PACK_P010) return fail(ctx, H2Y_EINVAL, "packing must be 1 (planar8), 2 (nv12) or 3 (p010)");
    if (!pack_legal(chroma, bit_depth, packing))
        return fail(ctx, H2Y_EINVAL, "packing %s does not take bit depth %d with chroma_format_idc %d (planar8: 8 bits; nv12: 8 bits, 4:2:0; p010: 10..16 bits, 4:2:0)",
                    kPackName[packing], bit_depth, chroma);
    return H2Y_OK;
}

int h2y_pack_frame(int width, int height, int chroma_format_idc, int bit_depth, int packing, const uint16_t *src, void *dst)
{
    if (!src || !dst) return fail(nullptr, H2Y_EINVAL, "null frame");
    const int rc = pack_check(nullptr, width, height, chroma_format_idc, bit_depth, packing);
    if (rc) return rc;
    const size_t n = (size_t)width * height, nc = (size_t)pack_cw((uint32_t)width, chroma_format_idc) * pack_ch((uint32_t)height, chroma_format_idc);
    const uint32_t M = (1u << bit_depth) - 1u, s = packing == H2Y_PACK_P010 ? 16u - (uint32_t)bit_depth : 0u;
    uint8_t *b = static_cast<uint8_t *>(dst);
    uint16_t *w = static_cast<uint16_t *>(dst);
    const size_t planar = packing == H2Y_PACK_PLANAR8 ? n + 2 * nc : n; /* these go over element for element */
    for (size_t i = 0; i < planar; i++) {
        if (packing == H2Y_PACK_P010) w[i] = (uint16_t)pack_code(src[i], M, s);
        else b[i] = (uint8_t)pack_code(src[i], M, s);
    }
    if (packing != H2Y_PACK_PLANAR8)
        for (size_t i = 0; i < nc; i++)
            for (size_t c = 0; c < 2; c++) {
                const uint32_t e = pack_code(src[n + c * nc + i], M, s);
                if (packing == H2Y_PACK_P010) w[n + 2 * i + c] = (uint16_t)e;
                else b[n + 2 * i + c] = (uint8_t)e;
            }
    return H2Y_OK;
}

int h2y_unpack_frame(int width, int height, int chroma_format_idc, int bit_depth, int packing, const void *src, uint16_t *dst)
{
    if (!src || !dst) return fail(nullptr, H2Y_EINVAL, "null frame");
    const int rc = pack_check(nullptr, width, height, chroma_format_idc, bit_depth, packing);
    if (rc) return rc;
    const size_t n = (size_t)width * height, nc = (size_t)pack_cw((uint32_t)width, chroma_format_idc) * pack_ch((uint32_t)height, chroma_format_idc);
    const uint32_t s = packing == H2Y_PACK_P010 ? 16u - (uint32_t)bit_depth : 0u;
    const uint8_t *b = static_cast<const uint8_t *>(src);
    const uint16_t *w = static_cast<const uint16_t *>(src);
    const size_t planar = packing == H2Y_PACK_PLANAR8 ? n + 2 * nc : n;
    for (size_t i = 0; i < planar; i++) dst[i] = (uint16_t)unpack_code(packing == H2Y_PACK_P010 ? (uint32_t)w[i] : (uint32_t)b[i], s);
    if (packing != H2Y_PACK_PLANAR8)
        for (size_t i = 0; i < nc; i++)
            for (size_t c = 0; c < 2; c++)
                dst[n + c * nc + i] = (uint16_t)unpack_code(packing == H2Y_PACK_P010 ? (uint32_t)w[n + 2 * i + c] : (uint32_t)b[n + 2 * i + c], s);
    return H2Y_OK;
}

static int pack_grid(const h2y_ctx *ctx, const pack_args &a, int n_frames)
{
    return unit_grid(ctx, (uint64_t)n_frames * (a.j[0].chunks + a.j[1].chunks + a.j[2].chunks));
}

/* both batches: planar[f] and packed[f] are the frames' two sides, whichever is written */
static int pack_batch(h2y_ctx *ctx, bool unpack, int width, int height, int chroma, int bit_depth, int packing, int n_frames,
                      const void *const *planar, const void *const *packed)
{
    int rc = batch_enter(ctx);
    if (!rc) rc = pack_check(ctx, width, height, chroma, bit_depth, packing);
    if (!rc) rc = pairs_check(ctx, n_frames, planar, packed);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t off[3];
    contiguous_planes(width, height, chroma, off);
    const pack_args a = h2y_pack_args((uint32_t)width, (uint32_t)height, chroma, bit_depth, packing, off);
    pack_frame *h;
    rc = frame_table(ctx, n_frames, h);
    if (rc) return rc;
    for (int f = 0; f < n_frames; f++) h[f] = pack_frame{planar[f], packed[f]};
    rc = timed_launches(ctx, h, n_frames, H2Y_PACK_FRAMES_PER_LAUNCH, unpack ? "k_unpack" : "k_pack", [&](const pack_frame *frames, int, int nf) {
        return h2y_launch_pack(packing, unpack, pack_grid(ctx, a, nf), ctx->stream, a, frames, nf);
    });
    if (rc) return rc;
    ctx->last_variant = std::string(unpack ? "k_unpack<" : "k_pack<") + kPackName[packing] + ">";
    return H2Y_OK;
}

int h2y_pack_batch(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int bit_depth, int packing, int n_frames,
                   const uint16_t *const *d_src, void *const *d_dst)
{
    return pack_batch(ctx, false, width, height, chroma_format_idc, bit_depth, packing, n_frames, reinterpret_cast<const void *const *>(d_src), d_dst);
}

int h2y_unpack_batch(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int bit_depth, int packing, int n_frames,
                     const void *const *d_src, uint16_t *const *d_dst)
{
    return pack_batch(ctx, true, width, height, chroma_format_idc, bit_depth, packing, n_frames, reinterpret_cast<const void *const *>(d_dst), d_src);
}

/* Packing's ring stage, the last of a slot's: k_pack packs the frame that would go down -- the ring's, the scale stage's or the
 * dither stage's -- into a frame of its own, on the device and pinned, which goes down and is handed out in that frame's place */
struct pack_stage : ring_stage {
    struct slot {
        char *d = nullptr, *h = nullptr;
    };
    std::vector<slot> ss;
    pack_args a{};
    pack_frame *tab = nullptr;
    size_t bytes = 0; /* of the packed frame */
    int packing = 0;
    int run(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, h2y_launch_pack(packing, false, pack_grid(ctx, a, 1), ctx->stream, a, tab + k, 1));
        return H2Y_OK;
    }
    int download(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, hipMemcpyAsync(ss[k].h, ss[k].d, bytes, hipMemcpyDeviceToHost, ctx->s_d2h));
        return H2Y_OK;
    }
};

int h2y_stream_pack(h2y_ctx *ctx, int packing)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    const ring_frame &f = ctx->s_frame;
    scale_stage *sc = stage_of<scale_stage>(ctx, STAGE_SCALE);
    dither_stage *di = stage_of<dither_stage>(ctx, STAGE_DITHER);
    /* a .yuv frame comes out of a forward ring, and out of a ring without a producer that scales or dithers its input */
    if (ctx->s_kind != h2y_ctx::RING_FORWARD && !(ctx->s_kind == h2y_ctx::RING_PLANES && (sc || di)))
        return fail(ctx, H2Y_EUNSUPPORTED, "the ring's output is no .yuv frame: only a forward, scale-only or dither-only ring packs");
    if (ctx->s_stage[STAGE_PACK]) return fail(ctx, H2Y_EINVAL, "the ring packs already");
    if (ctx->s_stage[STAGE_COMPARE] || ctx->s_stage[STAGE_HISTOGRAM] || ctx->s_stage[STAGE_SSIM] || ctx->s_stage[STAGE_DELTAE])
        return fail(ctx, H2Y_EUNSUPPORTED, "a ring armed for comparison, histograms, SSIM or Delta E is not packed: compare or count the written file instead");
    if (ctx->s_kind == h2y_ctx::RING_FORWARD && ctx->s_desc.dst_matrix == H2Y_MATRIX_YUVPRIME2)
        return fail(ctx, H2Y_EUNSUPPORTED, "a Y'u'v' ring (dst_matrix_coeffs 15) is not packed");
    rc = arm_unstarted(ctx);
    if (rc) return rc;
    const int width = sc ? (int)sc->g.p[0].dw : f.width, height = sc ? (int)sc->g.p[0].dh : f.height;
    const int bit_depth = f.depth - (di ? (int)di->a.shift : 0);
    rc = pack_check(ctx, width, height, f.chroma, bit_depth, packing);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto st = std::make_unique<pack_stage>();
    pack_stage *pk = st.get();
    uint32_t off[3];
    contiguous_planes(width, height, f.chroma, off);
    pk->a = h2y_pack_args((uint32_t)width, (uint32_t)height, f.chroma, bit_depth, packing, off);
    pk->packing = packing;
    pk->bytes = h2y_pack_frame_bytes(width, height, f.chroma, packing);
    const int depth = (int)ctx->ss.size();
    std::vector<pack_frame> tab(depth);
    pk->ss.resize(depth);
    for (int k = 0; k < depth; k++) {
        pk->dev_alloc(pk->ss[k].d, std::max<size_t>(pk->bytes, 16));
        pk->pin_alloc(pk->ss[k].h, std::max<size_t>(pk->bytes, 16));
        /* where the frame that would go down lies: a ring without a producer has its stage write the slot's output */
        const uint16_t *src = f.in_input ? ctx->ss[k].d_out : di ? di->ss[k].d : sc ? sc->ss[k].d : ctx->ss[k].d_out;
        tab[k] = pack_frame{src, pk->ss[k].d};
    }
    pk->table(pk->tab, tab);
    rc = stage_arm(ctx, STAGE_PACK, std::move(st), "pack");
    if (rc) return rc;
    if (sc) sc->down = false; /* the frames in front stay on the device: the packed one goes down */
    if (di) di->down = false;
    ring_frame_stays(ctx);
    for (int k = 0; k < depth; k++) ctx->ss[k].result = reinterpret_cast<const uint16_t *>(pk->ss[k].h);
    return H2Y_OK;
}

/* Unpacking's ring stage, the first of a slot's: it lends its pinned packed frame as the slot's input, takes it up in the place of
 * ring_upload's copy, and k_unpack writes the planes where that copy would have put them, before the ring's producer.  On the
 * compare-only ring the comparison's reference goes the same way (cmp_stage::packed_to). */
struct unpack_stage : ring_stage {
    struct slot {
        char *d = nullptr, *h = nullptr, *d_ref = nullptr;
    };
    std::vector<slot> ss;
    pack_args a{}, a_ref{};
    pack_frame *tab = nullptr, *tab_ref = nullptr;
    size_t bytes = 0; /* of the packed frame */
    int packing = 0;
    void *lend(h2y_ctx *, int k) override { return ss[k].h; }
    int upload(h2y_ctx *ctx, int k) override
    {
        if (bytes) HIP_TRY(ctx, hipMemcpyAsync(ss[k].d, ss[k].h, bytes, hipMemcpyHostToDevice, ctx->s_h2d));
        return H2Y_OK;
    }
    int unpack(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, h2y_launch_pack(packing, true, pack_grid(ctx, a, 1), ctx->stream, a, tab + k, 1));
        if (tab_ref) HIP_TRY(ctx, h2y_launch_pack(packing, true, pack_grid(ctx, a_ref, 1), ctx->stream, a_ref, tab_ref + k, 1));
        return H2Y_OK;
    }
    int run(h2y_ctx *, int) override { return H2Y_OK; }
};

int h2y_stream_unpack(h2y_ctx *ctx, int packing) { return h2y_stream_unpack_ex(ctx, packing, 0); }

int h2y_stream_unpack_ex(h2y_ctx *ctx, int packing, int depth_given)
{
    int rc = arm_enter(ctx);
    if (rc) return rc;
    if (ctx->s_stage[STAGE_UNPACK]) return fail(ctx, H2Y_EINVAL, "the ring unpacks already");
    /* where the planes the upload brings lie in the slot's device input, which frame they are, and its depth */
    const ring_frame &f = ctx->s_frame;
    int width, height, chroma, bit_depth;
    uint32_t off[3];
    size_t base = 0;
    if (ctx->s_kind == h2y_ctx::RING_FORWARD) {
        if (ctx->s_src.kind == decode_src::NONE && ctx->s_desc.in_sample_type == H2Y_SAMPLE_U16)
            return fail(ctx, H2Y_EUNSUPPORTED, "a forward ring on U16 planes (the integer .yuv -> .yuv flow) takes its planes as the reference does: not unpacked");
        if (ctx->s_src.kind != decode_src::PQCODE)
            return fail(ctx, H2Y_EINVAL, "the ring's input is not u16 code planes: only an inverse, planes or code ring unpacks");
        const codelight_plan &p = ctx->s_src.code;
        width = p.width, height = p.height, chroma = p.sub ? H2Y_CHROMA_420 : H2Y_CHROMA_444, bit_depth = p.bit_depth;
        for (int c = 0; c < 3; c++) off[c] = p.off[c];
        base = ctx->s_pay_off;
    } else if (ctx->s_kind == h2y_ctx::RING_INVERSE) {
        const inv_params &p = ctx->s_inv;
        width = p.width, height = p.height, chroma = p.chroma, bit_depth = p.in_depth;
        for (int c = 0; c < 3; c++) off[c] = (uint32_t)(ctx->s_in_off[c] / sizeof(uint16_t));
    } else {
        width = f.width, height = f.height, chroma = f.chroma, bit_depth = f.depth;
        for (int c = 0; c < 3; c++) off[c] = f.off[c];
    }
    rc = arm_unstarted(ctx);
    if (rc) return rc;
    if (depth_given < 0) return fail(ctx, H2Y_EINVAL, "unpack: bit_depth must be 0 (the ring's own) or the frames' depth");
    if (depth_given > 0 && bit_depth > 0 && depth_given != bit_depth)
        return fail(ctx, H2Y_EINVAL, "unpack: bit_depth %d given, but the ring's input depth is %d", depth_given, bit_depth);
    if (depth_given > 0) bit_depth = depth_given; /* a compare-only ring learns its frames' depth here */
    if (packing == H2Y_PACK_P010 && bit_depth == 0)
        return fail(ctx, H2Y_EINVAL, "packing P010 needs the bit depth, which a compare-only ring does not know: give it to h2y_stream_unpack_ex");
    rc = pack_check(ctx, width, height, chroma, bit_depth, packing);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto st = std::make_unique<unpack_stage>();
    unpack_stage *un = st.get();
    const int depth_bits = bit_depth ? bit_depth : 8; /* unknown: a byte packing, whose codes are the bytes */
    un->a = h2y_pack_args((uint32_t)width, (uint32_t)height, chroma, depth_bits, packing, off);
    un->packing = packing;
    un->bytes = h2y_pack_frame_bytes(width, height, chroma, packing);
    cmp_stage *cmp = ctx->s_kind == h2y_ctx::RING_PLANES ? stage_of<cmp_stage>(ctx, STAGE_COMPARE) : nullptr; /* the compare-only ring */
    const int depth = (int)ctx->ss.size();
    std::vector<pack_frame> tab(depth), tab_ref(depth);
    un->ss.resize(depth);
    for (int k = 0; k < depth; k++) {
        un->dev_alloc(un->ss[k].d, std::max<size_t>(un->bytes, 16));
        un->pin_alloc(un->ss[k].h, std::max<size_t>(un->bytes, 16));
        tab[k] = pack_frame{ctx->ss[k].d_in + base, un->ss[k].d};
        if (cmp) {
            un->dev_alloc(un->ss[k].d_ref, std::max<size_t>(un->bytes, 16));
            tab_ref[k] = pack_frame{cmp->ss[k].d_ref, un->ss[k].d_ref};
        }
    }
    un->table(un->tab, tab);
    if (cmp) {
        un->a_ref = h2y_pack_args((uint32_t)width, (uint32_t)height, chroma, depth_bits, packing, cmp->g.b_off);
        un->table(un->tab_ref, tab_ref);
    }
    rc = stage_arm(ctx, STAGE_UNPACK, std::move(st), "unpack");
    if (rc) return rc;
    if (cmp) { /* the lent reference holds a packed frame: it goes up as it is, into the stage's frame */
        cmp->packed_bytes = un->bytes;
        cmp->packed_to.resize(depth);
        for (int k = 0; k < depth; k++) cmp->packed_to[k] = un->ss[k].d_ref;
    }
    return H2Y_OK;
}
