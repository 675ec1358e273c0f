/*
 * h2y_forward.hip -- the forward conversion of the C-ABI shim (include/hdr2yuv_hip.h): the scalar setup the reference does in
 * init_pic()/set_pic_clip() (common.cpp:172-327), the choice of the kernel, and run_frames(), which every converted frame passes
 * through -- the batch entries, the single-frame entry, the single-step entries here, the forward ring in h2y_ring.hip.
 *
 * How a batch is cut into launches and a launch's work dealt to blocks is arithmetic in h2y_plan.h, checked on the CPU;
 * this file asks the plan and turns it into stream operations.
 */
#include "h2y_shim.h"
#include "h2y_plan.h"

namespace {

/* Share of a batch's pixels (counted in tiles of eight) the first tier passed on, above which the next batches go to the binary64
 * tier's kernels.  Both first-tier kernels now take that tier inside their loops, a wave at a time: with 0.1-0.2 % of the pixels
 * passed on they are 11-16 % ahead of the binary64 tier's kernels, with 1.3-1.5 % 8-19 % behind (tools/densebench.sh: u^2 and u^3
 * of the uniform picture); the lines cross near 0.7 %.  (Rounds 1-2: 8 % -- of tiles, one unsettled pixel making a tile.) */
const double kT1DenseShare = 0.007;
const double kFirSyncMaxFlagged = 0.004; /* k_fir_fused: tiles-of-eight share of unsettled pixels above which its waves are left out of step */
/* A probe of the first tier on dense content is dear (letterboxed 4K, a quarter of the tiles flagged: 8.6 ms per 64-frame launch
 * against k_fused2's 1.6), staying on the binary64 tier too long is cheap (2-10 % slower than the first tier on content that
 * suits it): probe rarely -- after 32 batches, then 64, ... 1024. */
const int kT1SkipBatches = 32;
const int kT1SkipBatchesMax = 1024;

/* hdr2yuv.cpp:803-808: the matrix_convert() target takes the input's depth
 * when both pictures are U16, else the output's */
int tmp_depth_of(const h2y_desc *d) { return d->in_sample_type == H2Y_SAMPLE_U16 ? d->src_bit_depth : d->dst_bit_depth; }

} // namespace

/* Scalar setup for the kernels: everything matrix_convert()/convert()/
 * write_yuv() derive from the picture attributes before their pixel loops. */
void derive_params(const h2y_desc *d, pix_params *pp, bool stage_matrix_only)
{
    memset(pp, 0, sizeof *pp);
    const int tmp_depth = tmp_depth_of(d);
    const clip_limits tc = make_clip(tmp_depth, d->dst_full_range);
    const clip_limits oc = make_clip(d->dst_bit_depth, d->dst_full_range);
    pp->src_tf = tf_class(d->src_transfer);
    pp->dst_tf = tf_class(d->dst_transfer);
    if (d->src_transfer == d->dst_transfer) pp->convert_transfer = 0; /* convert.cpp:930 */
    else pp->convert_transfer = (pp->src_tf == H2Y_TF_LINEAR && pp->dst_tf == H2Y_TF_PQ) ? 1 : 2;
    /* the two stages of a generic pair (tables in h2y_math.h); -1 until run_frames() has the tables on the device */
    pp->src_fn = pp->dst_fn = -1;
    /* convert.cpp:1123-1145 (full range: multiply only; add stays 0.0f) */
    if (d->dst_full_range) {
        pp->mulY = pp->mulC = (float)tc.maxCV;
    } else if (d->dst_matrix == H2Y_MATRIX_GBR) {
        pp->mulY = pp->mulC = (float)(int)tc.maxVR;
        pp->addY = pp->addC = (float)(int)tc.minVR;
    } else {
        pp->mulY = (float)(int)tc.maxVR;
        pp->addY = (float)(int)tc.minVR;
        pp->mulC = (float)(int)tc.maxVRC;
        pp->addC = (float)(int)tc.minVRC;
    }
    /* convert.cpp:1159-1198 */
    if (d->dst_matrix == d->src_matrix && d->dst_primaries == d->src_primaries) pp->mode = H2Y_MODE_IDENTITY;
    else if (d->dst_matrix == H2Y_MATRIX_YDZDX) pp->mode = H2Y_MODE_YDZDX;
    else if (d->dst_matrix == H2Y_MATRIX_YUVPRIME2) pp->mode = H2Y_MODE_YUVP2; /* convert.cpp:1191-1194 */
    else if (d->dst_matrix == H2Y_MATRIX_BT2020NC) {
        pp->mode = H2Y_MODE_YCBCR;
        pp->kr = 0.2627; pp->kg = 0.6780; pp->kb = 0.0593; pp->dcb = 1.8814; pp->dcr = 1.4746;
    } else if (d->dst_matrix == H2Y_MATRIX_BT709) {
        pp->mode = H2Y_MODE_YCBCR;
        pp->kr = 0.2126; pp->kg = 0.7152; pp->kb = 0.0722; pp->dcb = 1.8556; pp->dcr = 1.5748;
    } else {
        pp->mode = H2Y_MODE_YPQRS; /* convert.cpp:913-925 */
        if (d->dst_matrix == H2Y_MATRIX_YDZDX_Y100) { pp->P = -0.5f; pp->Q = 0.491722f; pp->RR = 0.5f; pp->S = -0.49495f; }
        else { pp->P = -0.5f; pp->Q = 0.493393f; pp->RR = 0.5f; pp->S = -0.49602f; }
    }
    if (pp->mode == H2Y_MODE_YCBCR) {
        pp->inv_dcb = 1.0 / pp->dcb;
        pp->inv_dcr = 1.0 / pp->dcr;
    }
    pp->half_m1 = tc.Half - 1;
    pp->maxCV = tc.maxCV;
    pp->fir_max = (float)tc.maxCV;
    if (stage_matrix_only) { /* identity clamp: values are already <= maxCV <= 65535 */
        pp->down_shift = 0;
        pp->ylo = pp->clo = 0;
        pp->yhi = pp->chi = 0xFFFFu;
    } else {
        pp->down_shift = tmp_depth - d->dst_bit_depth; /* tiff.cpp:394 */
        if (d->dst_full_range) { /* tiff.cpp:476: only "> maxCV" */
            pp->ylo = pp->clo = 0;
            pp->yhi = pp->chi = oc.maxCV;
        } else {
            pp->ylo = oc.minVR; pp->yhi = oc.maxVR; pp->clo = oc.minVRC; pp->chi = oc.maxVRC;
        }
    }
    pix_limits_finish(pp);
}

namespace {

/* start of a batch: is the first tier to be skipped this time? */
void t1_begin_batch(h2y_ctx *ctx)
{
    ctx->cur_skip_t1 = ctx->t1_skip > 0;
    if (ctx->cur_skip_t1) ctx->t1_skip--;
}
/* end of a batch that ran k_fused_t1: how many of its tiles had to be redone */
void t1_end_batch(h2y_ctx *ctx, const h2y_desc *d, const frame_stats *fs, int n)
{
    if (!ctx->b->was_t1 || n < 1) return;
    uint64_t redone = 0;
    for (int f = 0; f < n; f++) redone += fs[f].redone;
    const uint64_t tiles = (uint64_t)n * make_geom(d->width, d->height, 1024).tiles;
    if (!strcmp(ctx->last_name, "k_fir_fused")) ctx->fir_flag_share = tiles ? (double)redone / (double)tiles : 0.0;
    { /* for whoever asks h2y_last_kernel_variant(): the share of tiles the first tier passed on */
        const size_t at = ctx->last_variant.find(" flagged=");
        if (at != std::string::npos) ctx->last_variant.erase(at);
        char note[48];
        snprintf(note, sizeof note, " flagged=%.5f", tiles ? (double)redone / (double)tiles : 0.0);
        ctx->last_variant += note;
    }
    if (ctx->opt_t1_steer && (double)redone > kT1DenseShare * (double)tiles) {
        /* still dense at the next probe: stay away twice as long */
        ctx->t1_skip_len = ctx->t1_skip_len ? (ctx->t1_skip_len < kT1SkipBatchesMax ? 2 * ctx->t1_skip_len : kT1SkipBatchesMax) : kT1SkipBatches;
        ctx->t1_skip = ctx->t1_skip_len;
    } else ctx->t1_skip_len = 0;
}

/* known: the floor/ceiling the kernels will assume, when the HOST knows them (hint or
 * override); NULL when they only exist in device memory (stats pre-pass). */
fused_variant pick_variant(const h2y_ctx *ctx, const h2y_desc *d, const pix_params &pp, int out_kind, const assumed_stats *known, t1_sens *sn)
{
    memset(sn, 0, sizeof *sn);
    fused_variant v;
    v.in_kind = in_kind_of(d);
    v.out_kind = out_kind;
    v.mode = pp.mode;
    v.narrow = (d->width % 4) != 0;
    v.even_h = (d->height & 1) == 0;
    v.pipe = 0;
    /* equal transfers (the 16-bit .tiff / .yuv flows): samples straight into the matrix */
    /* k_fused2 has YUVP2 compiled in for 4:4:4 output, which is all that mode ever writes (the 4:2:0 form too: tmp_pic first) */
    const bool loop_mode = pp.mode == H2Y_MODE_YCBCR || pp.mode == H2Y_MODE_YDZDX || (pp.mode == H2Y_MODE_YUVP2 && out_kind == H2Y_OUT_444);
    if (!pp.convert_transfer && !v.narrow && v.even_h && loop_mode) v.pipe = 6;
    if (pp.convert_transfer && !v.narrow) {
        bool ident = known != nullptr;
        for (int c = 0; c < 3 && ident; c++) ident = known->floor_[c] == 0 && known->ceil_[c] == 1;
        v.pipe = ident ? 1 : 2; /* 2 is always valid: (x - 0) / 1 == x exactly */
        if (pp.convert_transfer == 2) /* generic transfer pair: its two stages' tables, in the loop form where that exists */
            v.pipe = (v.even_h && loop_mode) ? 7 /* H2Y_PIPE_TFN */ : 0;
        /* binary32 first tier where few pixels would fall through it (moderate bit depths); t1_bounds() holds for YCbCr and
         * Y'DzDx only, so the other modes never reach k_fused_t1 or k_fir_fused */
        if ((v.pipe == 1 || v.pipe == 2) && v.in_kind != H2Y_IN_U16 && (d->height & 1) == 0 && ctx->opt_t1 && t1_bounds(pp, sn)) {
            v.pipe += 3;
            v.t1_ok = true;
        }
        /* half input with the identity normalisation: the whole transfer is a 64 KB table */
        if (pp.convert_transfer == 1 && ident && v.in_kind == H2Y_IN_F16 && v.even_h && (pp.mode == H2Y_MODE_YCBCR || pp.mode == H2Y_MODE_YDZDX)) v.pipe = 3;
    }
    return v;
}

int out_kind_of(const h2y_desc *d)
{
    if (d->dst_chroma_format_idc == H2Y_CHROMA_444) return H2Y_OUT_444;
    return d->chroma_resampler_type == 0 ? H2Y_OUT_420BOX : H2Y_OUT_444TMP;
}


const float *xcd_times(const batch_state *b) { return reinterpret_cast<const float *>(b->h_fstats + b->bal_slot); }

/* after a launch whose block clocks came back: speed of each XCD = the share its blocks had / the time they took, and the
 * same for every block by itself (speed_update, h2y_plan.h); the next launch's slice ranges follow the speeds */
void balance_update(h2y_ctx *ctx)
{
    batch_state *b = ctx->b;
    if (!b->bal_pending) return;
    b->bal_pending = false;
    if (!speed_update(ctx->bal_speed, ctx->bal_have, b->bal_work, xcd_times(b), 8, 0.5)) return;
    ctx->bal_have = true;
    /* per block: a launch ends with its slowest BLOCK, and blocks of one XCD differ too (+-0.5 % of a launch, half of it the
     * same blocks from launch to launch).  Lighter smoothing than for the XCDs: one block's time is noisier than the mean of 32 */
    const int grid = b->bal_grid;
    if (grid > 0 && grid <= 1024 && b->h_btime && (int)b->bal_bwork.size() == grid) {
        const bool have = ctx->bal_bgrid == grid && ctx->bal_bgroups == b->bal_groups && (int)ctx->bal_bspeed.size() == grid;
        std::vector<double> fresh(have ? 0 : (size_t)grid, 1.0); /* another grid shape: its speeds stay until this one's are known */
        if (!speed_update(have ? ctx->bal_bspeed.data() : fresh.data(), have, b->bal_bwork.data(), b->h_btime, grid, 0.35)) return;
        if (!have) ctx->bal_bspeed.swap(fresh);
        ctx->bal_bgrid = grid;
        ctx->bal_bgroups = b->bal_groups;
    }
}

/* after a k_fir_fused launch whose block clocks came back: speed of each XCD = steps a wave of it had / time it took */
void ffb_update(h2y_ctx *ctx)
{
    batch_state *b = ctx->b;
    if (!b->ffb_pending) return;
    b->ffb_pending = false;
    if (speed_update(ctx->ffb_speed, ctx->ffb_have, b->ffb_work, xcd_times(b), 8, 0.5)) ctx->ffb_have = true;
}

} // namespace

/* the table of transfer function fn on the device (built on the host the first time it is asked for) */
int ensure_tfn(h2y_ctx *ctx, int fn)
{
    if (fn <= H2Y_TFN_NONE || fn >= H2Y_TFN_COUNT || ctx->d_tfn[fn]) return 0;
    std::vector<pq_recA> A(H2Y_PQ_NREC);
    std::vector<pq_recB> B(H2Y_PQ_NREC);
    (void)tfn_build_table(fn, A.data(), B.data());
    char *t = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)&t, H2Y_PQ_TABLE_BYTES));
    ctx->d_tfn[fn] = t;
    HIP_TRY(ctx, hipMemcpy(t, A.data(), H2Y_PQ_NREC * 16, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(t + H2Y_PQ_NREC * 16, B.data(), H2Y_PQ_NREC * 16, hipMemcpyHostToDevice));
    if (fn == H2Y_TFN_PQ_R) ctx->d_tfn_ext[fn] = ctx->d_table_ext; /* the same function, the same layout */
    else {
        std::vector<pq_ext_rec> X(H2Y_PQX_NSEG);
        (void)tfn_build_ext(fn, X.data());
        void *x = nullptr;
        HIP_TRY(ctx, hipMalloc(&x, H2Y_PQX_TABLE_BYTES));
        ctx->d_tfn_ext[fn] = x;
        HIP_TRY(ctx, hipMemcpy(x, X.data(), H2Y_PQX_TABLE_BYTES, hipMemcpyHostToDevice));
    }
    return 0;
}

namespace {

/* k_yuvp2_420's table, once per context */
int ensure_lin(h2y_ctx *ctx)
{
    if (ctx->d_lin) return 0;
    std::vector<uint16_t> lin(65536);
    h2y_yuvp2_lin_table(lin.data());
    uint16_t *t = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)&t, lin.size() * sizeof(uint16_t)));
    ctx->d_lin = t;
    HIP_TRY(ctx, hipMemcpy(t, lin.data(), lin.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return 0;
}


/* what run_frames() was asked and what it derived: the two launch forms work from this */
struct frames_run {
    const h2y_desc *d;
    const frame_io *frames;
    int n;
    const assumed_stats *d_assumed;
    bool check;
    int fstats_offset;
    bool time_it;
    pix_params pp;
    t1_sens sn;
    fused_variant var;
    bool top_left = false; /* the context's chroma siting 2 applies: the second pass is k_fir420_tl */
};

balance balance_of(const h2y_ctx *ctx) { return balance{ctx->opt_bal_mode, ctx->opt_bal_mask, ctx->opt_bal_rho}; }

/* Frame descriptors [f0, f0 + nf) of the batch, as h_frames holds them: host -> device (tiny) -- unless the device already
 * holds exactly these (a caller cycling through the same buffers): one stream operation less in front of the kernel */
int stage_frames(h2y_ctx *ctx, int f0, int nf)
{
    batch_state *b = ctx->b;
    const size_t at = (size_t)ctx->slot_base + f0;
    bool on_device = b->dev_frames.size() == b->frames_cap;
    if (!on_device) b->dev_frames.assign(b->frames_cap, frame_io{});
    on_device = on_device && memcmp(&b->dev_frames[at], b->h_frames + at, nf * sizeof(frame_io)) == 0;
    if (!on_device) {
        HIP_TRY(ctx, hipMemcpyAsync(b->d_frames + at, b->h_frames + at, nf * sizeof(frame_io), hipMemcpyHostToDevice, ctx->stream));
        std::copy(b->h_frames + at, b->h_frames + at + nf, b->dev_frames.begin() + at);
    }
    return 0;
}

/* p holds `need` bytes; zeroed when it had to grow (the kernels that use it keep it zero from there on) */
template <typename T> int ensure_zeroed(h2y_ctx *ctx, T *&p, size_t &cap, size_t need)
{
    if (cap >= need) return 0;
    const int rc = ensure(ctx, p, cap, need);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(p, 0, need, ctx->stream));
    return 0;
}
/* the per-frame "a sample <= -1 was seen" flags of a launch of n frames */
int ensure_low(h2y_ctx *ctx, int n) { return ensure_zeroed(ctx, ctx->b->d_low, ctx->b->low_cap, (size_t)(n > 64 ? n : 64) * sizeof(uint32_t)); }
/* the block clocks of a timed launch (k_stats_final clears the finish entries from here on) */
int ensure_clock(h2y_ctx *ctx, int grid) { return ensure_zeroed(ctx, ctx->b->d_clock, ctx->b->clock_cap, (size_t)2 * grid * sizeof(unsigned long long)); }

/* the event pair around a timed launch; what ran is what h2y_last_kernel_name() / _variant() report */
int timer_start(h2y_ctx *ctx, const char *name, const char *variant)
{
    HIP_TRY(ctx, hipEventRecord(ctx->b->ev[ctx->b->n_ev][0], ctx->stream));
    ctx->last_name = name;
    ctx->last_variant = variant;
    return 0;
}
int timer_stop(h2y_ctx *ctx)
{
    HIP_TRY(ctx, hipEventRecord(ctx->b->ev[ctx->b->n_ev][1], ctx->stream));
    ctx->b->n_ev++;
    return 0;
}

/* k_stats_final's arguments for pic_stats alone: nblk partials per frame in d_partial, nothing of a conversion's launch */
final_args stats_final(const h2y_ctx *ctx, const h2y_desc *d, int nblk, frame_stats *out)
{
    final_args fa;
    fa.partial = ctx->b->d_partial;
    fa.nblk = nblk;
    fa.out = out;
    fa.is_u16 = d->in_sample_type == H2Y_SAMPLE_U16;
    fa.src_bit_depth = d->src_bit_depth;
    fa.redo_count = nullptr;
    fa.low_flag = nullptr;
    fa.check = 0;
    fa.assumed = nullptr;
    fa.publish = nullptr;
    fa.block_clock = nullptr;
    fa.grid = 0;
    fa.xcd_time = nullptr;
    return fa;
}
/* ... and behind a conversion's launch of `grid` blocks on the frames from f0 on: what the launch left beside the partials */
final_args launch_final(const h2y_ctx *ctx, const frames_run &r, int f0, int nblk, bool redo, bool low, bool clocks, int grid)
{
    final_args fa = stats_final(ctx, r.d, nblk, ctx->b->fs_out + r.fstats_offset + f0);
    fa.redo_count = redo ? ctx->b->d_redo : nullptr;
    fa.low_flag = low ? ctx->b->d_low : nullptr;
    fa.check = r.check ? 1 : 0;
    fa.assumed = r.d_assumed;
    fa.block_clock = clocks ? ctx->b->d_clock : nullptr;
    fa.grid = grid;
    static_assert(sizeof(frame_stats) >= 8 * sizeof(float), "the XCD run times ride in one frame_stats entry");
    fa.xcd_time = reinterpret_cast<float *>(ctx->b->fs_out + r.fstats_offset + r.n); /* the caller's copy of the statistics takes one entry more */
    return fa;
}

/* k_fir_fused's unit rows on the device: room for `units`, and the copy only when the device holds other rows */
int stage_unit_rows(h2y_ctx *ctx, const std::vector<uint32_t> &rows)
{
    batch_state *b = ctx->b;
    const size_t units = rows.size();
    if (b->unit_rows_cap < units) {
        if (b->d_unit_rows) HIP_TRY(ctx, hipFree(b->d_unit_rows));
        if (b->h_unit_rows) HIP_TRY(ctx, hipHostFree(b->h_unit_rows));
        b->d_unit_rows = b->h_unit_rows = nullptr;
        b->unit_rows_cap = 0;
        b->dev_unit_rows.clear();
        HIP_TRY(ctx, hipMalloc((void **)&b->d_unit_rows, units * sizeof(uint32_t)));
        HIP_TRY(ctx, hipHostMalloc((void **)&b->h_unit_rows, units * sizeof(uint32_t), hipHostMallocDefault));
        b->unit_rows_cap = units;
    }
    if (b->dev_unit_rows != rows) {
        memcpy(b->h_unit_rows, rows.data(), units * sizeof(uint32_t));
        HIP_TRY(ctx, hipMemcpyAsync(b->d_unit_rows, b->h_unit_rows, units * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        b->dev_unit_rows = rows;
    }
    return 0;
}

/* The FIR resampler in one pass: one k_fir_fused launch over all n frames, cut as plan p says (h2y_plan.h) */
int launch_fir_fused(h2y_ctx *ctx, const frames_run &r, const fir_plan &p)
{
    batch_state *b = ctx->b;
    const h2y_desc *d = r.d;
    const int n = r.n, grid = p.grid;
    const fused_variant &var = r.var;
    const bool ident = var.pipe == 4 || var.pipe == 3; /* assumed floor 0 / ceiling 1 (pipe 3: half input, the table kernel's case) */
    const uint32_t upf = p.strips * p.segments;
    b->was_t1 = true;
    for (int i = 0; i < n; i++) b->h_frames[(size_t)ctx->slot_base + i] = r.frames[i];
    int rc = stage_frames(ctx, 0, n);
    if (rc) return rc;
    rc = ensure(ctx, b->d_partial, b->partial_cap, (size_t)n * upf * 6 * sizeof(float));
    if (rc) return rc;
    rc = ensure(ctx, b->d_redo, b->redo_cap, (size_t)n * upf * sizeof(uint32_t));
    if (rc) return rc;
    if (ident && (rc = ensure_low(ctx, n))) return rc;
    if (r.check) b->approx_min = ident;
    firf_args fa;
    fa.frames = b->d_frames + ctx->slot_base;
    fa.n_frames = n;
    fa.width = (uint32_t)d->width;
    fa.height = (uint32_t)d->height;
    fa.wq = p.wq;
    fa.n_strips = p.strips;
    fa.n_seg = p.segments;
    fa.seg_rows = p.seg_rows;
    fa.units_per_frame = upf;
    fa.total_units = (uint32_t)p.units;
    /* In step (k_fir_fused, "In step"): every step (round 2's kernel: every second; with a fifth of the step's instructions
     * gone since, meeting every step is 0.4-1.7 % ahead, tools/firsyncbench.sh) -- unless the pictures keep sending pixels
     * to the exact tiers (each such pixel holds its wave for a microsecond, and in step all sixteen wait with it: a
     * picture with 0.02 % of its samples below the tables ran in 2.75 ms in step, 2.37 out of step; the usual picture
     * 1.74 and 1.93) */
    const int fsync = ctx->opt_fir_sync >= 0 ? ctx->opt_fir_sync : (ctx->fir_flag_share > kFirSyncMaxFlagged ? 0 : 1);
    fa.sync_mask = fsync > 0 ? (uint32_t)fsync - 1u : ~0u;
    fa.table = ctx->d_table;
    fa.table1 = ctx->d_table1;
    fa.lut16 = ctx->d_lut16;
    fa.sn = r.sn;
    fa.partial = b->d_partial;
    fa.redo_count = b->d_redo;
    fa.low_flag = ident ? b->d_low : nullptr;
    fa.assumed = r.d_assumed;
    fa.pp = r.pp;
    /* rows by XCD speed (fir_unit_rows, h2y_plan.h); the speeds come from the block clocks of earlier launches (ffb_update()) */
    fa.unit_rows = nullptr;
    fa.block_clock = nullptr;
    fa.mix_xcds = p.mix_xcds;
    const bool clocks = p.full && r.time_it;
    const balance bal = balance_of(ctx);
    const bool weigh = fir_weigh(p, bal, ctx->ffb_have);
    double work[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (weigh || clocks) {
        double sp[8];
        for (int x = 0; x < 8; x++) sp[x] = bal.speed(x, ctx->ffb_speed);
        std::vector<uint32_t> rows;
        fir_unit_rows(p, n, weigh, sp, rows, work);
        if (weigh) {
            if ((rc = stage_unit_rows(ctx, rows))) return rc;
            fa.unit_rows = b->d_unit_rows;
        }
    }
    if (clocks) {
        if ((rc = ensure_clock(ctx, grid))) return rc;
        fa.block_clock = b->d_clock;
    }
    const bool ev = r.time_it && b->n_ev < kMaxEvents;
    if (ev) {
        char buf[192];
        snprintf(buf, sizeof buf, "k_fir_fused<%s,420FIR,%s,%s%s> strips=%u segments=%u rows=%u", var.in_kind == H2Y_IN_F16 ? "F16" : "F32",
                 var.mode == H2Y_MODE_YCBCR ? "YCBCR" : "YDZDX", ident ? "PQ_IDENT" : "PQ_NORM", var.pipe == 3 ? ",LUT16" : "", p.strips, p.segments, p.seg_rows);
        if ((rc = timer_start(ctx, "k_fir_fused", buf))) return rc;
    }
    HIP_TRY(ctx, h2y_launch_fir_fused(var.in_kind, var.mode, ident, var.pipe == 3 /* the 16 384-entry table applies */, grid, ctx->stream, fa));
    if (ev && (rc = timer_stop(ctx))) return rc;
    /* (no frame of this path is U16; tail_ctr, tail_n and block_time stay at their defaults) */
    HIP_TRY(ctx, h2y_launch_stats_final(n, ctx->stream, launch_final(ctx, r, 0, (int)upf, true, ident, clocks, grid)));
    if (clocks) {
        b->bal_slot = r.fstats_offset + n;
        b->ffb_pending = true;
        for (int x = 0; x < 8; x++) b->ffb_work[x] = work[x];
    }
    return 0;
}

/* The slice ranges r of a launch where its kernel reads them: one of the batch's two tables in mapped pinned memory.  The kernels
 * read these tables IN PLACE: a slot may only be rewritten once every launch that reads it has finished.  A batch_state is handed
 * out again only after its batch was finished (enqueue / finish, h2y_convert_frame), so both slots are free at a batch's first
 * launch -- except on the stream pipeline, which calls run_frames() back to back on one state without synchronising: there the
 * slots stay busy until the third-table path below has waited for the stream. */
int publish_ranges(h2y_ctx *ctx, const std::vector<uint32_t> &r, bool first_launch, const uint32_t **d_ranges)
{
    batch_state *b = ctx->b;
    if (!b->h_ranges) {
        HIP_TRY(ctx, hipHostMalloc((void **)&b->h_ranges, 2 * kRangeWords * sizeof(uint32_t), hipHostMallocMapped));
        HIP_TRY(ctx, hipHostGetDevicePointer((void **)&b->hd_ranges, b->h_ranges, 0));
        HIP_TRY(ctx, hipHostMalloc((void **)&b->h_btime, 1024 * sizeof(float), hipHostMallocMapped));
        HIP_TRY(ctx, hipHostGetDevicePointer((void **)&b->hd_btime, b->h_btime, 0));
    }
    if (r.size() > kRangeWords) return fail(ctx, H2Y_EINVAL, "internal: %zu slice ranges", r.size());
    if (first_launch && !ctx->streaming) b->slot_busy[0] = b->slot_busy[1] = false;
    int slot = -1;
    for (int k = 0; k < 2 && slot < 0; k++)
        if (b->range_slot[k] == r) slot = k;
    if (slot < 0) {
        for (int k = 0; k < 2 && slot < 0; k++)
            if (!b->slot_busy[k]) slot = k;
        if (slot < 0) { /* a third table within one batch: wait for the launches that read the other two */
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            b->slot_busy[0] = b->slot_busy[1] = false;
            slot = 0;
        }
        memcpy(b->h_ranges + (size_t)slot * kRangeWords, r.data(), r.size() * sizeof(uint32_t));
        b->range_slot[slot] = r;
    }
    b->slot_busy[slot] = true;
    *d_ranges = b->hd_ranges + (size_t)slot * kRangeWords;
    return 0;
}

/* a generic transfer pair through the table tier: source function, then destination function */
int set_tfn_tables(h2y_ctx *ctx, fused_args &a)
{
    const int sf = kSrcFn[a.pp.src_tf], df = kDstFn[a.pp.dst_tf];
    int rc = ensure_tfn(ctx, sf);
    if (!rc) rc = ensure_tfn(ctx, df);
    if (rc) return rc;
    a.pp.src_fn = sf;
    a.pp.dst_fn = df;
    a.table_src = sf ? ctx->d_tfn[sf] : nullptr;
    a.table_dst = df ? ctx->d_tfn[df] : nullptr;
    a.pp.tf_ext[0] = sf ? ctx->d_tfn_ext[sf] : nullptr;
    a.pp.tf_ext[1] = df ? ctx->d_tfn_ext[df] : nullptr;
    return 0;
}

/* One launch of a loop-form kernel (k_fused2, k_fused_t1, k_fused_lut16) on the staged frames [f0, f0 + l.frames) of the batch,
 * and k_stats_final behind it */
int launch_fused(h2y_ctx *ctx, const frames_run &r, const geom &g, const launch_plan &l, int f0, bool first_launch, bool yuvp2)
{
    batch_state *b = ctx->b;
    const h2y_desc *d = r.d;
    const fused_variant &var = r.var;
    const int nf = l.frames, grid = l.grid, groups = l.groups;
    const int waves = h2y_fused_threads(var) / 64; /* the fused kernels leave one min/max record per wave */
    int rc = ensure(ctx, b->d_partial, b->partial_cap, (size_t)nf * grid * waves * 6 * sizeof(float));
    if (rc) return rc;
    const bool t1 = var.pipe == 4 || var.pipe == 5;
    if (t1 && (rc = ensure(ctx, b->d_redo, b->redo_cap, (size_t)nf * grid * waves * sizeof(uint32_t)))) return rc;
    const bool approx = var.pipe == 4; /* first tier, assumed floor 0 / ceiling 1: subsampled minimum */
    if (approx && (rc = ensure_low(ctx, nf))) return rc;
    if (r.check) b->approx_min = approx;
    /* slices by XCD or block speed (make_slice_plan, h2y_plan.h); "off": the even round-robin dealing of frame_walk.  The block
     * clocks of timed launches feed balance_update() */
    const uint32_t *d_slice_ranges = nullptr;
    slice_plan sl;
    for (int x = 0; x < 8; x++) sl.work[x] = 1;
    if (l.xcd_layout && ctx->opt_bal_mode != 1) {
        const balance bal = balance_of(ctx);
        double sp[8];
        for (int x = 0; x < 8; x++) sp[x] = bal.speed(x, ctx->bal_have ? ctx->bal_speed : nullptr);
        const block_speeds bs{ctx->opt_bal_mode == 0 && ctx->opt_bal_blocks, ctx->bal_bgrid, ctx->bal_bgroups, &ctx->bal_bspeed};
        make_slice_plan(sl, l, g.tiles, sp, bs, t1, ctx->opt_tail);
        if ((rc = publish_ranges(ctx, sl.r, first_launch, &d_slice_ranges))) return rc;
    }
    const bool clocks = l.xcd_layout && r.time_it;
    if (clocks && (rc = ensure_clock(ctx, grid))) return rc;
    fused_args a;
    a.xcd_layout = l.xcd_layout ? 1u : 0u;
    a.block_clock = clocks ? b->d_clock : nullptr;
    a.slice_ranges = d_slice_ranges;
    a.range_stride = sl.range_stride;
    a.tail_ctr = nullptr;
    a.tail_slices = 0;
    if (sl.tail_on && d_slice_ranges) { /* the dynamic last frame (k_fused_t1) */
        if (!b->d_tail) {
            HIP_TRY(ctx, hipMalloc((void **)&b->d_tail, 16 * H2Y_TAIL_WORDS * sizeof(uint32_t)));
            HIP_TRY(ctx, hipMemsetAsync(b->d_tail, 0, 16 * H2Y_TAIL_WORDS * sizeof(uint32_t), ctx->stream)); /* k_stats_final clears it from here on */
        }
        a.tail_ctr = b->d_tail;
        a.tail_slices = sl.slices;
    }
    a.redo_count = t1 ? b->d_redo : nullptr;
    a.low_flag = approx ? b->d_low : nullptr;
    a.frames = b->d_frames + ctx->slot_base + f0;
    a.n_frames = nf;
    a.width = d->width;
    a.height = d->height;
    a.wq = g.wq;
    a.wq_magic = g.wq_magic;
    a.tiles_per_frame = g.tiles;
    a.chunks_per_frame = g.chunks;
    a.groups = (uint32_t)groups;
    a.table = ctx->d_table;
    a.table_src = a.table_dst = nullptr;
    a.lut16 = ctx->d_lut16;
    a.table1 = ctx->d_table1;
    a.sn = r.sn;
    a.partial = b->d_partial;
    a.assumed = r.d_assumed;
    a.pp = r.pp;
    if (r.pp.convert_transfer == 2 && !var.narrow && (var.pipe == 0 || var.pipe == 7) && (rc = set_tfn_tables(ctx, a))) return rc;
    a.tiles_magic = g.tiles > 1 ? (uint32_t)(0x100000000ull / g.tiles) : 0xFFFFFFFFu;
    const bool ev = r.time_it && b->n_ev < kMaxEvents;
    if (ev) {
        static const char *const kIn[] = {"F32", "F16", "U16"}, *const kOut[] = {"420BOX", "444", "444TMP"};
        static const char *const kPipe[] = {"RUNTIME", "PQ_IDENT", "PQ_NORM", "LUT16", "PQ_IDENT", "PQ_NORM", "NONE", "TFN"};
        const char *mode = var.mode == H2Y_MODE_YCBCR ? "YCBCR" : var.mode == H2Y_MODE_YDZDX ? "YDZDX" : var.mode == H2Y_MODE_IDENTITY ? "IDENTITY"
                         : var.mode == H2Y_MODE_YUVP2 ? "YUVP2" : "YPQRS";
        char buf[192];
        snprintf(buf, sizeof buf, "%s<%s,%s,%s,%s%s>%s groups=%d xcd=%d%s", h2y_fused_name(var), kIn[var.in_kind], kOut[var.out_kind], mode,
                 kPipe[var.pipe], var.cols8 ? ",COLS8" : "", var.out_kind == H2Y_OUT_444TMP ? (r.top_left ? "+k_fir420_tl" : "+k_fir420") : yuvp2 ? (d->chroma_resampler_type ? "+k_yuvp2_420<FIR>" : "+k_yuvp2_420<BOX>") : "", groups, l.xcd_layout ? 1 : 0,
                 a.tail_ctr ? " tail=1" : "");
        if ((rc = timer_start(ctx, h2y_fused_name(var), buf))) return rc;
    }
    HIP_TRY(ctx, h2y_launch_fused(var, grid, ctx->stream, a));
    if (ev && (rc = timer_stop(ctx))) return rc;
    final_args fa = launch_final(ctx, r, f0, grid / groups * waves, t1, approx, clocks, grid);
    fa.tail_ctr = a.tail_ctr;
    fa.tail_n = groups * (int)H2Y_TAIL_WORDS;
    fa.block_time = clocks && d_slice_ranges && b->fs_out == b->m_fstats ? b->hd_btime : nullptr; /* (enqueued batches: what the host reads in h2y_batch_finish) */
    HIP_TRY(ctx, h2y_launch_stats_final(nf, ctx->stream, fa));
    if (clocks) {
        b->bal_slot = r.fstats_offset + r.n;
        b->bal_pending = true;
        for (int x = 0; x < 8; x++) b->bal_work[x] = sl.work[x];
        b->bal_grid = fa.block_time ? grid : 0;
        b->bal_groups = groups;
        b->bal_bwork = sl.bwork;
    }
    return 0;
}

/* The second pass of the staged frames [f0, f0 + nf), whose fused launch wrote scratch half `half`: k_yuvp2_420, k_fir420 or
 * (chroma siting 2) k_fir420_tl on fir_stream behind that launch, so that it overlaps the next launch on the main stream */
int second_pass(h2y_ctx *ctx, const frames_run &r, bool yuvp2, int f0, int nf, int half)
{
    const h2y_desc *d = r.d;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_fused[half], ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->fir_stream, ctx->ev_fused[half], 0));
    if (yuvp2) {
        yuvp2_args ya;
        ya.frames = ctx->b->d_frames + ctx->slot_base + f0;
        ya.n_frames = nf;
        ya.width = d->width;
        ya.height = d->height;
        ya.lin = ctx->d_lin;
        ya.fir_max = r.pp.fir_max;
        derive_params(d, &ya.pp, false); /* the output picture's write_yuv step */
        HIP_TRY(ctx, h2y_launch_yuvp2_420(d->chroma_resampler_type == 1, ctx->fir_stream, ya));
    } else {
        fir_args fr;
        fr.frames = ctx->b->d_frames + ctx->slot_base + f0;
        fr.n_frames = nf;
        fr.src_cb = fr.src_cr = nullptr;
        fr.dst_cb = fr.dst_cr = nullptr;
        fr.width = d->width;
        fr.height = d->height;
        fr.fir_max = r.pp.fir_max;
        fr.apply_yuv_clamp = 1;
        fr.pp = r.pp;
        HIP_TRY(ctx, r.top_left ? h2y_launch_fir420_tl(ctx->fir_stream, fr) : h2y_launch_fir420(ctx->fir_stream, fr));
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev_fir[half], ctx->fir_stream));
    ctx->fir_used[half] = true;
    return 0;
}

/* The loop-form launches of a batch, as next_launch() cuts it (h2y_plan.h); with scratch (the two-pass FIR form, Y'u'v' 4:2:0)
 * each launch hands its frames to a second pass */
int launch_loop_form(h2y_ctx *ctx, const frames_run &r, bool yuvp2)
{
    const h2y_desc *d = r.d;
    const int n = r.n, out_kind = r.var.out_kind;
    const bool scratch = out_kind == H2Y_OUT_444TMP || yuvp2; /* a second pass reads what the fused kernel leaves in d_tmp */
    const loop_shape s{h2y_fused_blocks_per_cu(r.var), h2y_fused_grouped(r.var), ctx->n_cu, ctx->opt_groups, scratch,
                       make_geom(d->width, d->height, h2y_fused_threads(r.var), r.var.cols8 ? 8 : 4)};
    const size_t npix = (size_t)d->width * d->height;
    /* the 4:4:4 chroma scratch of the two-pass FIR form: as many frames as a sub-batch holds, twice over when the batch
     * has more than one sub-batch (sub-batch i writes half i % 2 while the FIR pass still reads the other).  A single
     * frame (h2y_convert_frame, the CLI's ring) takes 33 MB at 4K, not the 2.1 GB of a full double sub-batch. */
    const int fir_sub = n < kFirSubBatch ? n : kFirSubBatch;
    /* a frame's scratch: Cb and Cr (the FIR), or all of tmp_pic in 256-byte aligned frames (Y'u'v') */
    const size_t tmp_stride = yuvp2 ? (3 * npix + 127) & ~(size_t)127 : 2 * npix;
    if (scratch) {
        /* earlier calls may have laid their halves out differently: nothing of theirs may still be reading */
        for (int hlf = 0; hlf < 2; hlf++)
            if (ctx->fir_used[hlf]) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_fir[hlf], 0));
        int rc = ensure(ctx, ctx->d_tmp, ctx->tmp_cap, (size_t)(n > kFirSubBatch ? 2 : 1) * fir_sub * tmp_stride * sizeof(uint16_t));
        if (rc) return rc;
    }
    launch_plan l;
    for (int f0 = 0, sub = 0; f0 < n; f0 += l.frames, sub++) {
        if (!next_launch(s, n - f0, &l)) return fail(ctx, H2Y_EINVAL, "internal: %d frames in %d groups exceed the per-group bound", l.frames, l.groups);
        const int nf = l.frames, half = sub & 1;
        if (scratch && ctx->fir_used[half]) /* scratch half still being read by an earlier FIR pass? */
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_fir[half], 0));
        for (int i = 0; i < nf; i++) {
            frame_io io = r.frames[f0 + i];
            if (out_kind == H2Y_OUT_444TMP) {
                io.tmp_cb = ctx->d_tmp + ((size_t)half * fir_sub + i) * tmp_stride;
                io.tmp_cr = io.tmp_cb + npix;
            } else if (yuvp2) { /* the fused kernel writes tmp_pic where the .yuv frame would go; k_yuvp2_420 reads it */
                io.yuv = io.out;
                io.out = ctx->d_tmp + ((size_t)half * fir_sub + i) * tmp_stride;
                io.tmp_cr = nullptr;
            }
            ctx->b->h_frames[(size_t)ctx->slot_base + f0 + i] = io;
        }
        int rc = stage_frames(ctx, f0, nf);
        if (!rc) rc = launch_fused(ctx, r, s.g, l, f0, sub == 0, yuvp2);
        if (!rc && scratch) rc = second_pass(ctx, r, yuvp2, f0, nf, half);
        if (rc) return rc;
    }
    if (scratch) /* everything queued after this call on the main stream sees finished chroma */
        for (int hlf = 0; hlf < 2; hlf++)
            if (ctx->fir_used[hlf]) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_fir[hlf], 0));
    return 0;
}

} // namespace

/* What the context's chroma siting (h2y_ctx_set_chroma_siting) makes of descriptor d: *top_left says whether the top-left form
 * applies (not with siting 0, nor with 4:4:4 output, which has no siting); the status is the refusal of what siting 2 cannot site:
 * the box is centre sited by construction, and Y'u'v' 4:2:0 has its own resamplers (k_yuvp2_420). */
int siting_of(h2y_ctx *ctx, const h2y_desc *d, bool *top_left)
{
    *top_left = false;
    if (ctx->opt_siting != 2 || d->dst_chroma_format_idc != H2Y_CHROMA_420) return H2Y_OK;
    if (d->dst_matrix == H2Y_MATRIX_YUVPRIME2)
        return fail(ctx, H2Y_EUNSUPPORTED, "chroma siting 2 (top-left) is not defined for dst_matrix_coeffs 15 with 4:2:0 output");
    if (d->chroma_resampler_type == 0)
        return fail(ctx, H2Y_EUNSUPPORTED, "chroma siting 2 (top-left) needs the FIR resampler: the 2x2 box (chroma_resampler_type 0) is centre sited by construction");
    *top_left = true;
    return H2Y_OK;
}

/* launch fused (+FIR) over frames [0,n) whose frame_io entries are in `frames`: derive the parameters, pick the variant, ask the
 * plan, and queue either one k_fir_fused launch or the loop-form launches of the batch */
int run_frames(h2y_ctx *ctx, const h2y_desc *d, const frame_io *frames, int n, const assumed_stats *d_assumed,
               const assumed_stats *known, bool check, int fstats_offset, bool time_it)
{
    /* Y'u'v' 4:2:0 (dst_matrix_coeffs 15): the fused kernel writes tmp_pic as it is -- 4:4:4, neither shifted nor clamped to the
     * output's range -- into scratch, and k_yuvp2_420 makes the .yuv frame of it (h2y_yuvp2.hip) */
    const bool yuvp2 = d->dst_matrix == H2Y_MATRIX_YUVPRIME2 && d->dst_chroma_format_idc == H2Y_CHROMA_420;
    frames_run r{d, frames, n, d_assumed, check, fstats_offset, time_it};
    int rc = siting_of(ctx, d, &r.top_left); /* read once per call: the whole batch takes one path */
    if (rc) return rc;
    derive_params(d, &r.pp, yuvp2);
    r.pp.pq_ext = ctx->d_table_ext;
    const int out_kind = yuvp2 ? H2Y_OUT_444 : out_kind_of(d);
    if (yuvp2 && (rc = ensure_lin(ctx))) return rc;
    fused_variant &var = r.var;
    var = pick_variant(ctx, d, r.pp, out_kind, known, &r.sn);
    /* k_fused_t1's redo list numbers tiles as frame * tiles + tile in 32 bits */
    if ((var.pipe == 4 || var.pipe == 5) && (uint64_t)n * make_geom(d->width, d->height, h2y_fused_threads(var)).tiles >= 0xFFFFFFFFull) var.pipe -= 3;
    if ((var.pipe == 4 || var.pipe == 5) && ctx->cur_skip_t1) var.pipe -= 3; /* dense zeros lately: binary64 tier for now */
    ctx->b->was_t1 = var.pipe == 4 || var.pipe == 5;
    if (var.pipe == 3 && d->width % 8 == 0) { /* half input through the table: 8-column tiles when every plane allows 16-byte accesses */
        bool ok = ctx->opt_cols8;
        for (int i = 0; i < n && ok; i++) {
            for (int c = 0; c < 3; c++) ok = ok && (reinterpret_cast<uintptr_t>(frames[i].in[c]) & 15u) == 0;
            ok = ok && (reinterpret_cast<uintptr_t>(frames[i].out) & 15u) == 0;
        }
        var.cols8 = ok;
    }
    /* (top-left siting has no one-pass form: decided here, before the plan is asked) */
    if (out_kind == H2Y_OUT_444TMP && !r.top_left && ctx->opt_fir != 1 && var.t1_ok && !ctx->cur_skip_t1 && tmp_depth_of(d) <= H2Y_FIR_INT_MAX_DEPTH) {
        const fir_plan p = make_fir_plan(n, d->width, d->height, ctx->n_cu, ctx->opt_fir);
        if (p.take) return launch_fir_fused(ctx, r, p); /* the FIR resampler in one pass */
    }
    return launch_loop_form(ctx, r, yuvp2);
}


int reserve_batch(h2y_ctx *ctx, int n)
{
    if ((size_t)n > ctx->b->frames_cap) {
        if (ctx->b->d_frames) HIP_TRY(ctx, hipFree(ctx->b->d_frames));
        if (ctx->b->h_frames) HIP_TRY(ctx, hipHostFree(ctx->b->h_frames));
        if (ctx->b->d_fstats) HIP_TRY(ctx, hipFree(ctx->b->d_fstats));
        if (ctx->b->h_fstats) HIP_TRY(ctx, hipHostFree(ctx->b->h_fstats));
        ctx->b->d_frames = nullptr; ctx->b->h_frames = nullptr; ctx->b->d_fstats = nullptr; ctx->b->h_fstats = nullptr;
        ctx->b->frames_cap = 0;
        ctx->b->dev_frames.clear();
        size_t cap = (size_t)n < 64 ? 64 : (size_t)n;
        HIP_TRY(ctx, hipMalloc((void **)&ctx->b->d_frames, cap * sizeof(frame_io)));
        HIP_TRY(ctx, hipHostMalloc((void **)&ctx->b->h_frames, cap * sizeof(frame_io), hipHostMallocDefault));
        /* +1: slot for the stats pre-pass / redo */
        HIP_TRY(ctx, hipMalloc((void **)&ctx->b->d_fstats, (cap + 1) * sizeof(frame_stats)));
        HIP_TRY(ctx, hipHostMalloc((void **)&ctx->b->h_fstats, (cap + 1) * sizeof(frame_stats), hipHostMallocDefault));
        HIP_TRY(ctx, hipHostGetDevicePointer((void **)&ctx->b->m_fstats, ctx->b->h_fstats, 0));
        ctx->b->fs_out = ctx->b->d_fstats;
        ctx->b->frames_cap = cap;
    }
    return 0;
}

/* pic_stats() of one frame on the device; result lands in d_fstats[slot] and,
 * when publish != NULL, as the assumption for later kernels -- no host sync. */
int run_stats(h2y_ctx *ctx, const h2y_desc *d, const void *const in[3], int slot, assumed_stats *publish)
{
    const size_t npix = (size_t)d->width * d->height;
    int grid = ctx->n_cu * 4;
    size_t need_blocks = (npix / 4 + H2Y_FUSED_THREADS - 1) / H2Y_FUSED_THREADS;
    if ((size_t)grid > need_blocks) grid = need_blocks ? (int)need_blocks : 1;
    int rc = ensure(ctx, ctx->b->d_partial, ctx->b->partial_cap, (size_t)grid * 6 * sizeof(float));
    if (rc) return rc;
    stats_args sa;
    bool aligned = true;
    for (int c = 0; c < 3; c++) {
        sa.in[c] = in[c];
        if (((uintptr_t)in[c]) & 15) aligned = false;
    }
    sa.npix = npix;
    sa.vec_ok = aligned ? 1 : 0;
    sa.partial = ctx->b->d_partial;
    HIP_TRY(ctx, h2y_launch_stats(in_kind_of(d), grid, ctx->stream, sa));
    final_args fa = stats_final(ctx, d, grid, ctx->b->d_fstats + slot);
    fa.publish = publish;
    HIP_TRY(ctx, h2y_launch_stats_final(1, ctx->stream, fa));
    return 0;
}

int h2y_convert_batch_enqueue(h2y_ctx *ctx, const h2y_desc *d, int n_frames, const void *const *d_in, uint16_t *const *d_out)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if (ctx->q_count >= 2) return fail(ctx, H2Y_EINVAL, "two batches are already in flight: call h2y_batch_finish first");
    if (ctx->streaming) return fail(ctx, H2Y_EINVAL, "a stream is open: close it first");
    const char *why;
    int rc = h2y_desc_check(d, &why);
    if (rc) return fail(ctx, rc, "descriptor: %s", why);
    if (n_frames < 1 || !d_in || !d_out) return fail(ctx, H2Y_EINVAL, "n_frames < 1 or null pointer arrays");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->b = &ctx->bs[(ctx->q_head + ctx->q_count) & 1]; /* the free slot: its last batch was finished */
    rc = reserve_batch(ctx, n_frames);
    if (rc) return rc;
    ctx->b->p_frames.resize(n_frames);
    for (int f = 0; f < n_frames; f++) {
        frame_io io;
        for (int c = 0; c < 3; c++) {
            io.in[c] = d_in[f * 3 + c];
            if (!io.in[c] || ((uintptr_t)io.in[c] & 15)) return fail(ctx, H2Y_EINVAL, "input plane %d of frame %d is null or not 16-byte aligned", c, f);
        }
        io.out = d_out[f];
        if (!io.out || ((uintptr_t)io.out & 15)) return fail(ctx, H2Y_EINVAL, "output of frame %d is null or not 16-byte aligned", f);
        io.tmp_cb = io.tmp_cr = nullptr;
        ctx->b->p_frames[f] = io;
    }
    ctx->b->n_ev = 0;
    const bool needs_stats = d->src_transfer != d->dst_transfer; /* convert.cpp:930-940: stats are only read then */
    bool check = false;
    bool host_knows = true;
    assumed_stats *as = ctx->b->h_assumed;
    const bool hinted = needs_stats && !d->stats_override && ctx->have_hint && ctx->hint_kind == d->in_sample_type;
    if (!needs_stats || d->stats_override || hinted) {
        /* hinted: assume this batch looks like the last frame we saw; verified below */
        assumed_stats want;
        for (int c = 0; c < 3; c++) {
            want.floor_[c] = hinted ? ctx->hint_floor[c] : d->stats_override ? d->floor[c] : 0;
            want.ceil_[c] = hinted ? ctx->hint_ceil[c] : d->stats_override ? d->ceiling[c] : 1;
        }
        *as = want; /* (the host copy is what pick_variant() reads) */
        if (!ctx->b->dev_assumed_ok || memcmp(&want, &ctx->b->dev_assumed, sizeof want) != 0) {
            HIP_TRY(ctx, hipMemcpyAsync(ctx->b->d_assumed, as, sizeof *as, hipMemcpyHostToDevice, ctx->stream));
            ctx->b->dev_assumed = want;
            ctx->b->dev_assumed_ok = true;
        }
        check = hinted;
    } else {
        /* no history: measure frame 0 (pic_stats pre-pass) and assume the rest match it */
        ctx->b->dev_assumed_ok = false;
        rc = run_stats(ctx, d, ctx->b->p_frames[0].in, (int)ctx->b->frames_cap, ctx->b->d_assumed);
        if (rc) return rc;
        check = true;
        host_knows = false; /* the values exist only in device memory */
    }
    t1_begin_batch(ctx);
    ctx->b->fs_out = ctx->b->m_fstats; /* the statistics (+ the XCD run times) go straight to pinned host memory */
    rc = run_frames(ctx, d, ctx->b->p_frames.data(), n_frames, ctx->b->d_assumed, host_knows ? ctx->b->h_assumed : nullptr, check, 0, true);
    ctx->b->fs_out = ctx->b->d_fstats;
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->b->ev_done, ctx->stream));
    ctx->b->p_desc = *d;
    ctx->b->p_n = n_frames;
    ctx->b->p_check = check;
    ctx->q_count++;
    return H2Y_OK;
}

int h2y_batch_finish(h2y_ctx *ctx, int *n_redone)
{
    if (n_redone) *n_redone = 0;
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if (ctx->q_count == 0) return H2Y_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->b = &ctx->bs[ctx->q_head]; /* the oldest batch in flight; a younger one may still be running behind it */
    ctx->q_head ^= 1;
    ctx->q_count--;
    HIP_TRY(ctx, hipEventSynchronize(ctx->b->ev_done));
    HIP_TRY(ctx, event_ms(ctx->b, &ctx->last_ms));
    ctx->last_launches = ctx->b->n_ev;
#ifdef H2Y_BLOCK_TIMES
    if (const char *e = getenv("H2Y_BLOCK_TIMES_FILE")) { /* one file per finished batch: <name>.<n> */
        static int n_dump = 0;
        char fn[512];
        snprintf(fn, sizeof fn, "%s.%d", e, n_dump++);
        if (!strcmp(ctx->last_name, "k_fir_fused")) h2y_dump_ff_block_times(fn);
        else h2y_dump_block_times(fn);
    }
#endif
    int redone = 0;
    const h2y_desc *d = &ctx->b->p_desc;
    t1_end_batch(ctx, d, ctx->b->h_fstats, ctx->b->p_n);
    balance_update(ctx);
    ffb_update(ctx);
    if (ctx->b->p_check) {
        for (int f = 0; f < ctx->b->p_n; f++) {
            if (!ctx->b->h_fstats[f].mismatch) continue;
            if (ctx->b->approx_min) {
                /* the kernel kept only a subsample of the minimum: what it measured is exact where it matched the
                 * assumption, not here -- take pic_stats() of this frame first, then the pixels, as
                 * h2y_convert_frame() does */
                int rc = run_stats(ctx, d, ctx->b->p_frames[f].in, (int)ctx->b->frames_cap, ctx->b->d_assumed + 1);
                if (rc) return rc;
                HIP_TRY(ctx, hipMemcpyAsync(ctx->b->h_fstats + f, ctx->b->d_fstats + ctx->b->frames_cap, sizeof(frame_stats), hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); /* before run_frames() reuses the slot */
                rc = run_frames(ctx, d, &ctx->b->p_frames[f], 1, ctx->b->d_assumed + 1, nullptr, false, (int)ctx->b->frames_cap, false);
                if (rc) return rc;
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                redone++;
                continue;
            }
            /* the assumption was wrong for this frame: its true floor/ceiling are now
             * known (the fused kernel measured them), so run it again with those */
            assumed_stats *as = ctx->b->h_assumed + 1;
            for (int c = 0; c < 3; c++) {
                as->floor_[c] = ctx->b->h_fstats[f].floor_[c];
                as->ceil_[c] = ctx->b->h_fstats[f].ceil_[c];
            }
            HIP_TRY(ctx, hipMemcpyAsync(ctx->b->d_assumed + 1, as, sizeof *as, hipMemcpyHostToDevice, ctx->stream));
            int rc = run_frames(ctx, d, &ctx->b->p_frames[f], 1, ctx->b->d_assumed + 1, as, false, (int)ctx->b->frames_cap, false);
            if (rc) return rc;
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            redone++;
        }
    }
    if (d->src_transfer != d->dst_transfer && !d->stats_override) {
        const frame_stats &last = ctx->b->h_fstats[ctx->b->p_n - 1];
        for (int c = 0; c < 3; c++) {
            ctx->hint_floor[c] = last.floor_[c];
            ctx->hint_ceil[c] = last.ceil_[c];
        }
        ctx->have_hint = true;
        ctx->hint_kind = d->in_sample_type;
    }
    if (n_redone) *n_redone = redone;
    return H2Y_OK;
}

int h2y_convert_batch(h2y_ctx *ctx, const h2y_desc *d, int n_frames, const void *const *d_in, uint16_t *const *d_out)
{
    int rc = h2y_convert_batch_enqueue(ctx, d, n_frames, d_in, d_out);
    if (rc) return rc;
    while (ctx->q_count > 0) { /* this batch and any enqueued before it */
        rc = h2y_batch_finish(ctx, nullptr);
        if (rc) return rc;
    }
    return H2Y_OK;
}

int h2y_convert_frame(h2y_ctx *ctx, const h2y_desc *d, const void *const in_planes[3], uint16_t *out_yuv)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0)) return fail(ctx, H2Y_EINVAL, "a batch is pending: call h2y_batch_finish first");
    if (ctx->streaming) return fail(ctx, H2Y_EINVAL, "a stream is open: close it first");
    const char *why;
    int rc = h2y_desc_check(d, &why);
    if (rc) return fail(ctx, rc, "descriptor: %s", why);
    if (!in_planes || !in_planes[0] || !in_planes[1] || !in_planes[2] || !out_yuv) return fail(ctx, H2Y_EINVAL, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t pb = h2y_plane_bytes(d), pb_al = (pb + 255) & ~(size_t)255, ob = h2y_frame_bytes(d);
    rc = ensure(ctx, ctx->d_in, ctx->in_cap, 3 * pb_al);
    if (rc) return rc;
    rc = ensure(ctx, ctx->d_out, ctx->out_cap, ob);
    if (rc) return rc;
    frame_io io;
    for (int c = 0; c < 3; c++) {
        io.in[c] = (char *)ctx->d_in + c * pb_al;
        HIP_TRY(ctx, hipMemcpyAsync((void *)io.in[c], in_planes[c], pb, hipMemcpyHostToDevice, ctx->stream));
    }
    io.out = ctx->d_out;
    io.tmp_cb = io.tmp_cr = nullptr;
    /* the reference's order: pic_stats first, then the pixel loops with its result */
    const bool needs_stats = d->src_transfer != d->dst_transfer;
    bool host_knows = true;
    if (needs_stats && !d->stats_override) {
        rc = run_stats(ctx, d, io.in, (int)ctx->b->frames_cap, ctx->b->d_assumed);
        ctx->b->dev_assumed_ok = false; /* d_assumed[0] no longer holds what the last enqueued batch left there */
        if (rc) return rc;
        host_knows = false;
    } else {
        assumed_stats *as = ctx->b->h_assumed;
        for (int c = 0; c < 3; c++) {
            as->floor_[c] = d->stats_override ? d->floor[c] : 0;
            as->ceil_[c] = d->stats_override ? d->ceiling[c] : 1;
        }
        HIP_TRY(ctx, hipMemcpyAsync(ctx->b->d_assumed, as, sizeof *as, hipMemcpyHostToDevice, ctx->stream));
        ctx->b->dev_assumed_ok = false; /* d_assumed[0] no longer holds what the last enqueued batch left there */
    }
    ctx->b->n_ev = 0;
    t1_begin_batch(ctx);
    rc = run_frames(ctx, d, &io, 1, ctx->b->d_assumed, host_knows ? ctx->b->h_assumed : nullptr, false, 0, true);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->b->h_fstats, ctx->b->d_fstats, 2 * sizeof(frame_stats), hipMemcpyDeviceToHost, ctx->stream)); /* + the XCD run times */
    HIP_TRY(ctx, hipMemcpyAsync(out_yuv, ctx->d_out, ob, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    t1_end_batch(ctx, d, ctx->b->h_fstats, 1);
    balance_update(ctx);
    HIP_TRY(ctx, event_ms(ctx->b, &ctx->last_ms));
    ctx->last_launches = ctx->b->n_ev;
    return H2Y_OK;
}

int h2y_pic_stats(h2y_ctx *ctx, const h2y_desc *d, const void *const d_in[3], float fminmax[6], int32_t floor_ceiling[6])
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0)) return fail(ctx, H2Y_EINVAL, "a batch is pending");
    if (ctx->streaming) return fail(ctx, H2Y_EINVAL, "a stream is open: close it first");
    const char *why;
    int rc = h2y_desc_check(d, &why);
    if (rc) return fail(ctx, rc, "descriptor: %s", why);
    if (!d_in || !fminmax || !floor_ceiling) return fail(ctx, H2Y_EINVAL, "null argument");
    for (int c = 0; c < 3; c++) /* run_stats() takes the scalar-load path for planes that are not 16-byte aligned */
        if (!d_in[c] || ((uintptr_t)d_in[c] & (sample_bytes(d) - 1))) return fail(ctx, H2Y_EINVAL, "input plane %d is null or not aligned to its sample size", c);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = run_stats(ctx, d, d_in, (int)ctx->b->frames_cap, nullptr);
    if (rc) return rc;
    frame_stats *hs = ctx->b->h_fstats + ctx->b->frames_cap;
    HIP_TRY(ctx, hipMemcpyAsync(hs, ctx->b->d_fstats + ctx->b->frames_cap, sizeof(frame_stats), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 6; i++) fminmax[i] = hs->mm[i];
    for (int c = 0; c < 3; c++) {
        floor_ceiling[2 * c] = hs->floor_[c];
        floor_ceiling[2 * c + 1] = hs->ceil_[c];
    }
    return H2Y_OK;
}

int h2y_matrix_convert(h2y_ctx *ctx, const h2y_desc *d, const void *const d_in[3], uint16_t *const d_out444[3])
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0)) return fail(ctx, H2Y_EINVAL, "a batch is pending");
    if (ctx->streaming) return fail(ctx, H2Y_EINVAL, "a stream is open: close it first");
    const char *why;
    int rc = h2y_desc_check(d, &why);
    if (rc) return fail(ctx, rc, "descriptor: %s", why);
    if (!d_in || !d_out444) return fail(ctx, H2Y_EINVAL, "null pointer arrays");
    for (int c = 0; c < 3; c++) { /* the kernels issue 16-byte loads and 8-byte stores */
        if (!d_in[c] || ((uintptr_t)d_in[c] & 15)) return fail(ctx, H2Y_EINVAL, "input plane %d is null or not 16-byte aligned", c);
        if (!d_out444[c] || ((uintptr_t)d_out444[c] & 15)) return fail(ctx, H2Y_EINVAL, "output plane %d is null or not 16-byte aligned", c);
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    assumed_stats *as = ctx->b->h_assumed;
    for (int c = 0; c < 3; c++) {
        as->floor_[c] = d->floor[c];
        as->ceil_[c] = d->ceiling[c];
    }
    if (d->src_transfer != d->dst_transfer)
        for (int c = 0; c < 3; c++)
            if (d->floor[c] == d->ceiling[c]) return fail(ctx, H2Y_EINVAL, "floor == ceiling for plane %d", c);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->b->d_assumed, as, sizeof *as, hipMemcpyHostToDevice, ctx->stream));
    ctx->b->dev_assumed_ok = false; /* d_assumed[0] no longer holds what the last enqueued batch left there */
    pix_params pp;
    derive_params(d, &pp, true);
    pp.pq_ext = ctx->d_table_ext;
    fused_variant var;
    var.in_kind = in_kind_of(d);
    var.out_kind = H2Y_OUT_444TMP;
    var.mode = pp.mode;
    var.narrow = (d->width % 4) != 0;
    var.even_h = (d->height & 1) == 0;
    var.pipe = (pp.convert_transfer == 1 && !var.narrow) ? 2 : 0;
    const geom g = make_geom(d->width, d->height, h2y_fused_threads(var));
    frame_io io;
    for (int c = 0; c < 3; c++) io.in[c] = d_in[c];
    io.out = d_out444[0];
    io.tmp_cb = d_out444[1];
    io.tmp_cr = d_out444[2];
    ctx->b->h_frames[0] = io;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->b->d_frames, ctx->b->h_frames, sizeof(frame_io), hipMemcpyHostToDevice, ctx->stream));
    ctx->b->dev_frames.clear(); /* run_frames()'s record of what d_frames holds */
    const int grid = grid_for(ctx->n_cu, h2y_fused_blocks_per_cu(var), g.chunks);
    rc = ensure(ctx, ctx->b->d_partial, ctx->b->partial_cap, (size_t)grid * (h2y_fused_threads(var) / 64) * 6 * sizeof(float));
    if (rc) return rc;
    fused_args a;
    a.frames = ctx->b->d_frames;
    a.n_frames = 1;
    a.width = d->width;
    a.height = d->height;
    a.wq = g.wq;
    a.wq_magic = g.wq_magic;
    a.tiles_per_frame = g.tiles;
    a.chunks_per_frame = g.chunks;
    a.groups = 1;
    a.xcd_layout = 0;
    a.block_clock = nullptr;
    a.slice_ranges = nullptr;
    a.table = ctx->d_table;
    a.table_src = a.table_dst = nullptr; /* (a generic transfer pair takes the careful tier in this stage entry) */
    a.lut16 = ctx->d_lut16;
    a.table1 = ctx->d_table1;
    memset(&a.sn, 0, sizeof a.sn);
    a.tiles_magic = 0;
    a.redo_count = nullptr;
    a.low_flag = nullptr;
    a.partial = ctx->b->d_partial;
    a.assumed = ctx->b->d_assumed;
    a.pp = pp;
    HIP_TRY(ctx, h2y_launch_fused(var, grid, ctx->stream, a));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return H2Y_OK;
}

/* the stage entries' FIR: one u16 plane, no write_yuv clamp */
static hipError_t launch_plane_fir(h2y_ctx *ctx, bool top_left, int width, int height, int bit_depth, const uint16_t *d_src, uint16_t *d_dst)
{
    fir_args fr;
    memset(&fr, 0, sizeof fr);
    fr.frames = nullptr;
    fr.src_cb = d_src;
    fr.src_cr = nullptr;
    fr.dst_cb = d_dst;
    fr.dst_cr = nullptr;
    fr.width = width;
    fr.height = height;
    fr.fir_max = (float)((1u << bit_depth) - 1);
    fr.apply_yuv_clamp = 0;
    return top_left ? h2y_launch_fir420_tl(ctx->stream, fr) : h2y_launch_fir420(ctx->stream, fr);
}

int h2y_subsample_420(h2y_ctx *ctx, int width, int height, int bit_depth, int chroma_resampler_type, const uint16_t *d_src,
                      uint16_t *d_dst)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0)) return fail(ctx, H2Y_EINVAL, "a batch is pending");
    if (ctx->streaming) return fail(ctx, H2Y_EINVAL, "a stream is open: close it first");
    if (width < 2 || height < 2 || (width & 1) || (height & 1) || bit_depth < 8 || bit_depth > 16 || !d_src || !d_dst)
        return fail(ctx, H2Y_EINVAL, "bad subsample arguments");
    if (chroma_resampler_type == 0 && ((width & 3) || (height & 3))) return fail(ctx, H2Y_EINVAL, "box needs multiples of 4");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (chroma_resampler_type == 0) HIP_TRY(ctx, h2y_launch_box420(ctx->stream, d_src, d_dst, width, height));
    else HIP_TRY(ctx, launch_plane_fir(ctx, false, width, height, bit_depth, d_src, d_dst));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return H2Y_OK;
}

int h2y_subsample_420_sited(h2y_ctx *ctx, int width, int height, int bit_depth, int chroma_sample_loc_type, const uint16_t *d_src,
                            uint16_t *d_dst)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0)) return fail(ctx, H2Y_EINVAL, "a batch is pending");
    if (ctx->streaming) return fail(ctx, H2Y_EINVAL, "a stream is open: close it first");
    if (width < 2 || height < 2 || (width & 1) || (height & 1) || bit_depth < 8 || bit_depth > 16 || !d_src || !d_dst)
        return fail(ctx, H2Y_EINVAL, "bad subsample arguments");
    if (chroma_sample_loc_type != 0 && chroma_sample_loc_type != 2)
        return fail(ctx, H2Y_EINVAL, "chroma_sample_loc_type %d: want 0 (the reference's FIR) or 2 (top-left)", chroma_sample_loc_type);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    /* timed like a batch entry's launch (h2y_last_kernel_ms / _name): tools/streambench.py holds the two kernels side by side */
    HIP_TRY(ctx, hipEventRecord(ctx->b->ev[0][0], ctx->stream));
    HIP_TRY(ctx, launch_plane_fir(ctx, chroma_sample_loc_type == 2, width, height, bit_depth, d_src, d_dst));
    HIP_TRY(ctx, hipEventRecord(ctx->b->ev[0][1], ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->b->n_ev = 1;
    HIP_TRY(ctx, event_ms(ctx->b, &ctx->last_ms));
    ctx->last_launches = 1;
    ctx->last_name = chroma_sample_loc_type == 2 ? "k_fir420_tl" : "k_fir420";
    ctx->last_variant = ctx->last_name;
    return H2Y_OK;
}

int h2y_ctx_set_chroma_siting(h2y_ctx *ctx, int chroma_sample_loc_type)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0) || ctx->streaming) return fail(ctx, H2Y_EINVAL, "a batch is pending or a stream is open: set the chroma siting before");
    if (chroma_sample_loc_type != 0 && chroma_sample_loc_type != 2)
        return fail(ctx, H2Y_EINVAL, "chroma_sample_loc_type %d: want 0 (as the resampler sites it) or 2 (top-left)", chroma_sample_loc_type);
    ctx->opt_siting = chroma_sample_loc_type;
    return H2Y_OK;
}
