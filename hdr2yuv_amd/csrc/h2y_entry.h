/*
 * h2y_entry.h -- what the measurements' entries share (h2y_measure.hip, and the batch entries of h2y_api.hip): the refusals every
 * batch, arm and result entry begins with, each written once with its one text, the two ring stages that several measurements are
 * (a result per slot; a pass in place), and what the entries of one family share.  Included by h2y_shim.h, after the context and the
 * ring's declarations.  An entry calls these in the order in which it reports its refusals: the order is part of the ABI's behaviour.
 */
#pragma once

/* ---- batch entries ------------------------------------------------------------------------------------------------------------------ */

/* a synchronous batch entry runs beside no queued batch and no ring */
inline int batch_enter(h2y_ctx *ctx)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0) || ctx->streaming) return fail(ctx, H2Y_EINVAL, "a batch is pending or a stream is open");
    return H2Y_OK;
}

/* a picture whose planes' sample offsets fit 32 bits with room to spare */
inline int picture_size_check(h2y_ctx *ctx, int width, int height)
{
    if (width < 1 || height < 1 || (uint64_t)width * (uint64_t)height >= (1ull << 28)) return fail(ctx, H2Y_EINVAL, "bad picture size");
    return H2Y_OK;
}

/* the width and height of plane p: 4:2:0 halves both for planes 1 and 2 */
struct plane_dim {
    uint32_t w, h;
};
inline plane_dim plane_dims(int width, int height, int chroma, int p)
{
    const int sub = p && chroma == H2Y_CHROMA_420 ? 1 : 0;
    return plane_dim{(uint32_t)(width >> sub), (uint32_t)(height >> sub)};
}

/* n_frames whole frames, each at a 16-byte aligned base (arrays_ok: the entry's other pointer arrays are there too); each(f): what
 * else the entry checks of frame f, before frame f + 1 is looked at */
template <typename A, typename F> int frames_check(h2y_ctx *ctx, int n_frames, A *const *d_frames, bool arrays_ok, F each)
{
    if (n_frames < 1) return fail(ctx, H2Y_EINVAL, "n_frames must be >= 1");
    if (!d_frames || !arrays_ok) return fail(ctx, H2Y_EINVAL, "null pointer arrays");
    for (int f = 0; f < n_frames; f++) {
        if (!d_frames[f]) return fail(ctx, H2Y_EINVAL, "frame %d is null", f);
        if ((uintptr_t)d_frames[f] & 15u) return fail(ctx, H2Y_EINVAL, "frame %d is not 16-byte aligned", f);
        const int rc = each(f);
        if (rc) return rc;
    }
    return H2Y_OK;
}
template <typename A> int frames_check(h2y_ctx *ctx, int n_frames, A *const *d_frames, bool arrays_ok)
{
    return frames_check(ctx, n_frames, d_frames, arrays_ok, [](int) { return H2Y_OK; });
}

/* n_frames pairs of whole frames (a frame and its reference, a source and its destination), each at a 16-byte aligned base */
template <typename A, typename B> int pairs_check(h2y_ctx *ctx, int n_frames, A *const *d_a, B *const *d_b, bool arrays_ok = true)
{
    if (n_frames < 1) return fail(ctx, H2Y_EINVAL, "n_frames must be >= 1");
    if (!d_a || !d_b || !arrays_ok) return fail(ctx, H2Y_EINVAL, "null pointer arrays");
    for (int f = 0; f < n_frames; f++) {
        if (!d_a[f] || !d_b[f]) return fail(ctx, H2Y_EINVAL, "frame %d: a frame is null", f);
        if (((uintptr_t)d_a[f] | (uintptr_t)d_b[f]) & 15u) return fail(ctx, H2Y_EINVAL, "frame %d: a frame is not 16-byte aligned", f);
    }
    return H2Y_OK;
}

/* ---- arm entries (h2y_stream_<stage>) ------------------------------------------------------------------------------------------------ */

/* The refusals of an arm entry come in three steps, because most entries have refusals of their own between them: arm_enter, then
 * (what the ring must be), then the stage is not armed yet, then (what must not be armed beside it), then arm_unstarted.  arm_free is
 * the last two where nothing stands between them. */
inline int arm_enter(h2y_ctx *ctx)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if (!ctx->streaming) return fail(ctx, H2Y_EINVAL, "no stream open");
    return H2Y_OK;
}

inline int arm_unstarted(h2y_ctx *ctx)
{
    if (ctx->s_started) return fail(ctx, H2Y_EINVAL, "arm the ring before its first input");
    return H2Y_OK;
}

inline int arm_free(h2y_ctx *ctx, int id, const char *already)
{
    if (ctx->s_stage[id]) return fail(ctx, H2Y_EINVAL, "%s", already);
    return arm_unstarted(ctx);
}

/* ---- result entries (h2y_stream_<stage>_result) -------------------------------------------------------------------------------------- */

inline int output_taken(h2y_ctx *ctx)
{
    if (ctx->s_lent < 0) return fail(ctx, H2Y_EINVAL, "no output taken yet: h2y_stream_output first");
    return H2Y_OK;
}

/* The result of the open ring's stage `id`, armed as an S, for the frame h2y_stream_output handed out last: finish(stage, slot)
 * writes it to the caller.  none: the entry's own sentence for a ring without the stage. */
template <typename S, typename F> int stream_result(h2y_ctx *ctx, const void *out, int id, const char *none, F finish)
{
    if (!ctx || !out) return fail(ctx, H2Y_EINVAL, "null argument");
    const S *st = ctx->streaming ? stage_of<S>(ctx, id) : nullptr;
    if (!st) return fail(ctx, H2Y_EINVAL, "%s", none);
    const int rc = output_taken(ctx);
    if (rc) return rc;
    finish(*st, ctx->s_lent);
    return H2Y_OK;
}

/* ---- ring stages --------------------------------------------------------------------------------------------------------------------- */

/* A stage whose result is one R per slot, on the device and pinned: slots() allocates them while arming, download() brings the
 * slot's down.  The stage adds its geometry or arguments, its table and run(). */
template <typename R> struct result_stage : ring_stage {
    struct slot {
        R *d = nullptr, *h = nullptr;
    };
    std::vector<slot> ss;
    void slots(size_t depth)
    {
        ss.resize(depth);
        for (auto &s : ss) {
            dev_alloc(s.d, sizeof(R));
            pin_alloc(s.h, sizeof(R));
        }
    }
    int download(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, hipMemcpyAsync(ss[k].h, ss[k].d, sizeof(R), hipMemcpyDeviceToHost, ctx->s_d2h));
        return H2Y_OK;
    }
};

/* A pass's stage (gamut, tone map, HLG, ICtCp): in place on a forward ring's decoded planes, in the order of stage_id (gamut, tone map, LUT,
 * then HLG or ICtCp), before pic_stats and the conversion.  It holds the kernel's arguments A, its table entry per slot, the launch's
 * shape and the launch wrapper itself, and leaves nothing of its own behind: what follows reads the planes it left. */
template <typename A> struct pass_stage : ring_stage {
    A a{};
    gamut_frame *tab = nullptr;
    int in_kind = H2Y_IN_F32;
    int grid = 1;
    hipError_t (*launch)(int in_kind, int grid, hipStream_t st, const A &a, const gamut_frame *frames, int n_frames) = nullptr;
    int decoded(h2y_ctx *ctx, int k) override
    {
        HIP_TRY(ctx, launch(in_kind, grid, ctx->stream, a, tab + k, 1));
        return H2Y_OK;
    }
    int run(h2y_ctx *, int) override { return H2Y_OK; }
};

/* ---- what the entries of one family share: frame pairs (compare, SSIM, regions), passes over float planes, the light stages ---------- */

/* What the three batch entries do once their own check has passed and their geometry stands: the checks of the frame pairs, the
 * cmp_frame table, the launches' partials (partials(frames per launch)) and the batch's device stats, the timed launches
 * (launch(frames, f0, nf), timed_launches') and the stats' download into out */
template <typename S, typename P, typename L>
int pair_batch(h2y_ctx *ctx, int n_frames, const uint16_t *const *d_a, const uint16_t *const *d_b, S *out, dev_buf<S> &stats,
                      int per_launch, const char *name, P partials, L launch)
{
    int rc = pairs_check(ctx, n_frames, d_a, d_b, out != nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    cmp_frame *h;
    rc = frame_table(ctx, n_frames, h);
    if (!rc) rc = partials(std::min(n_frames, per_launch));
    if (!rc) rc = ensure(ctx, stats, (size_t)n_frames * sizeof(S));
    if (rc) return rc;
    for (int f = 0; f < n_frames; f++) h[f] = cmp_frame{d_a[f], d_b[f]};
    rc = timed_launches(ctx, h, n_frames, per_launch, name, launch);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(out, stats.p, (size_t)n_frames * sizeof(S), hipMemcpyDeviceToHost));
    return H2Y_OK;
}

/* What a pass's batch entry does once its own arguments are checked: n_frames, the two arrays and every plane of every frame, in
 * their order (widens: the pass writes float planes whatever it reads, so half planes cannot be converted in place); then the device,
 * and the frame table h, filled */
inline int pass_frames(h2y_ctx *ctx, int n_frames, const void *const *d_src, void *const *d_dst, bool widens, gamut_frame *&h)
{
    if (n_frames < 1) return fail(ctx, H2Y_EINVAL, "n_frames must be >= 1");
    if (!d_src || !d_dst) return fail(ctx, H2Y_EINVAL, "null pointer arrays");
    for (int f = 0; f < n_frames; f++)
        for (int c = 0; c < 3; c++) {
            const void *i = d_src[3 * f + c], *o = d_dst[3 * f + c];
            if (!i || !o) return fail(ctx, H2Y_EINVAL, "frame %d: plane %d is null", f, c);
            if (((uintptr_t)i | (uintptr_t)o) & 15u) return fail(ctx, H2Y_EINVAL, "frame %d: plane %d is not 16-byte aligned", f, c);
            if (i == o && widens)
                return fail(ctx, H2Y_EINVAL, "frame %d: plane %d in place: half planes are widened, the float planes need room of their own", f, c);
        }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = frame_table(ctx, n_frames, h);
    if (rc) return rc;
    for (int f = 0; f < n_frames; f++)
        for (int c = 0; c < 3; c++) h[f].src[c] = d_src[3 * f + c], h[f].dst[c] = d_dst[3 * f + c];
    return H2Y_OK;
}

/* the open forward ring's decoded planes, slot by slot, as a pass in place takes them */
inline std::vector<gamut_frame> ring_planes_table(const h2y_ctx *ctx)
{
    std::vector<gamut_frame> tab(ctx->ss.size());
    for (size_t k = 0; k < tab.size(); k++)
        for (int c = 0; c < 3; c++) tab[k].src[c] = tab[k].dst[c] = ctx->ss[k].d_in + c * ctx->s_plane_al;
    return tab;
}

/* a pass whose planes are referred to a range of their own runs on a ring opened with the 0 / 1 statistics override; why: the
 * entry's sentence up to the colon */
inline int unit_range_check(h2y_ctx *ctx, const h2y_desc *d, const char *why)
{
    bool unit = d->stats_override == 1;
    for (int c = 0; c < 3; c++) unit = unit && d->floor[c] == 0 && d->ceiling[c] == 1;
    if (!unit) return fail(ctx, H2Y_EINVAL, "%s: open the ring with stats_override 1, floor 0 and ceiling 1 on all three planes", why);
    return H2Y_OK;
}

/* what the light stages of a forward ring read, slot by slot: the decoded planes, and the floor and ceiling the conversion just
 * used (d_assumed) */
inline std::vector<light_frame> light_ring_table(const h2y_ctx *ctx)
{
    std::vector<light_frame> tab(ctx->ss.size());
    for (size_t k = 0; k < tab.size(); k++) {
        for (int c = 0; c < 3; c++) tab[k].in[c] = ctx->ss[k].d_in + c * ctx->s_plane_al;
        tab[k].assumed = ctx->b->d_assumed;
    }
    return tab;
}
