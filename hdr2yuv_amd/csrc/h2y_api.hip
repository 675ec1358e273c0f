/*
 * h2y_api.hip -- the C-ABI shim declared in include/hdr2yuv_hip.h: the context, the forward conversion and its batches, the
 * single-step entries, the inverse and decode batch entries and the file parsers.  The streaming ring lies in h2y_ring.hip, the
 * measurements (comparison, SSIM, content light, histograms, scaling) in h2y_measure.hip; h2y_shim.h is what the three share.
 *
 * Host side of the drop-in boundary: descriptor validation, the scalar setup
 * the reference does in init_pic()/set_pic_clip() (common.cpp:172-327), device
 * buffer ownership, and kernel launches.  No pixel is ever computed on the
 * host: without a HIP device h2y_ctx_create() fails and nothing else works.
 */
#include "h2y_shim.h"
#include "h2y_walk.h"

#include <zlib.h>

namespace {

thread_local std::string g_err;

const size_t kRangeWords = 1025; /* a table of slice ranges: up to 1024 blocks of a group + 1 */
/* Share of a batch's pixels (counted in tiles of eight) the first tier passed on, above which the next batches go to the binary64
 * tier's kernels.  Both first-tier kernels now take that tier inside their loops, a wave at a time: with 0.1-0.2 % of the pixels
 * passed on they are 11-16 % ahead of the binary64 tier's kernels, with 1.3-1.5 % 8-19 % behind (tools/densebench.sh: u^2 and u^3
 * of the uniform picture); the lines cross near 0.7 %.  (Rounds 1-2: 8 % -- of tiles, one unsettled pixel making a tile.) */
const double kT1DenseShare = 0.007;
/* A probe of the first tier on dense content is dear (letterboxed 4K, a quarter of the tiles flagged: 8.6 ms per 64-frame launch
 * against k_fused2's 1.6), staying on the binary64 tier too long is cheap (2-10 % slower than the first tier on content that
 * suits it): probe rarely -- after 32 batches, then 64, ... 1024. */
const double kFirSyncMaxFlagged = 0.004; /* k_fir_fused: tiles-of-eight share of unsettled pixels above which its waves are left out of step */
const int kTailMinFrames = 8; /* frames per group from which its last one is drawn dynamically (h2y_walk.h): the plain loop that takes it is
                                 slower than the prefetching one, and a frame is 1/8 of the group's work at most */
const int kT1SkipBatches = 32;
const int kT1SkipBatchesMax = 1024;
const int kFirSubBatch = 32; /* frames per fused launch on the FIR path: every launch pays its table staging and its last redo pass */

} // namespace

int fail(h2y_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    if (ctx) ctx->err = buf;
    return code;
}

namespace {

/* transfer_characteristics code -> what matrix_convert() does with it (convert.cpp:1024-1109);
 * -1: the reference only prints a warning for every pixel */
int tf_class(int t)
{
    switch (t) {
    case 8: return H2Y_TF_LINEAR;
    case 16: return H2Y_TF_PQ;
    case 18: return H2Y_TF_RHO_GAMMA;
    case 1: case 6: case 14: case 15: return H2Y_TF_BT1886; /* BT709, BT601, BT2020_10bit, BT2020_12bit */
    default: return -1;
    }
}

size_t sample_bytes(const h2y_desc *d) { return d->in_sample_type == H2Y_SAMPLE_F32 ? 4 : 2; }

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

struct geom {
    bool narrow;
    uint32_t wq, wq_magic, tiles, chunks;
};
geom make_geom(const h2y_desc *d, int threads, int cols = 4 /* columns of a thread tile (8: k_fused_lut16 on wide-aligned pictures) */)
{
    geom g;
    g.narrow = (d->width % 4) != 0;
    g.wq = g.narrow ? (uint32_t)d->width : (uint32_t)d->width / (uint32_t)cols;
    g.wq_magic = (uint32_t)(0x100000000ull / g.wq);
    if (g.wq == 1) g.wq_magic = 0xFFFFFFFFu;
    g.tiles = g.wq * (uint32_t)((d->height + 1) / 2);
    g.chunks = (g.tiles + threads - 1) / threads;
    return g;
}

/* Frame groups of a launch (frame_walk in h2y_kernels.hip), unless the caller set a number: as few as leave every block
 * kMinSlicesPerBlock 64-tile slices of a frame -- a 4K frame on 256 blocks: two groups, 1080p: eight, 8K: one.  Few, because
 * with g groups g frames are read and written at equal offsets at any moment, and whether those streams meet in the same DRAM
 * banks depends on where the frames happen to lie: eight groups ran the same 64 x 4K launch in 1.42 ... 1.72 ms from one set of
 * buffers to the next, two in 1.42 ... 1.51, one in 1.44 ... 1.49 (tools/layoutbench.py).  Not fewer, because a block pays for
 * every frame it visits (its waves' tickets, statistics records, the run-in of its prefetch): 1080p at one group runs at 0.47 of
 * the bandwidth it reaches at eight (0.61). */
const int kMinSlicesPerBlock = 100;
int groups_cap(const h2y_ctx *ctx, uint32_t tiles_per_frame, int grid)
{
    if (ctx->opt_groups) return ctx->opt_groups;
    const uint64_t slices = (tiles_per_frame + 63u) / 64u;
    int ng = 1;
    while (ng < 8 && slices * (uint64_t)ng < (uint64_t)kMinSlicesPerBlock * (uint64_t)grid) ng *= 2;
    return ng;
}

int grid_for(const h2y_ctx *ctx, const fused_variant &v, uint64_t total_chunks)
{
    /* persistent grid: exactly the blocks the chip holds at once */
    uint64_t g = (uint64_t)ctx->n_cu * h2y_fused_blocks_per_cu(v);
    if (g > total_chunks) g = total_chunks;
    if (g < 1) g = 1;
    return (int)g;
}

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
    const uint64_t tiles = (uint64_t)n * make_geom(d, 1024).tiles;
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

constexpr int kMaxFramesPerLaunch = 128;

int out_kind_of(const h2y_desc *d)
{
    if (d->dst_chroma_format_idc == H2Y_CHROMA_444) return H2Y_OUT_444;
    return d->chroma_resampler_type == 0 ? H2Y_OUT_420BOX : H2Y_OUT_444TMP;
}

/* after a launch whose block clocks came back: speed of each XCD = the share its blocks had / the time they took, and the
 * same for every block by itself; the next launch's slice ranges follow the speeds (run_frames()) */
void balance_update(h2y_ctx *ctx)
{
    if (!ctx->b->bal_pending) return;
    ctx->b->bal_pending = false;
    double sp[8], mean = 0.0;
    for (int x = 0; x < 8; x++) {
        const double t = reinterpret_cast<const float *>(ctx->b->h_fstats + ctx->b->bal_slot)[x];
        if (!(t > 0.0)) return; /* grid smaller than a round of XCDs, or nothing measured */
        sp[x] = ctx->b->bal_work[x] / t;
        mean += sp[x] / 8.0;
    }
    for (int x = 0; x < 8; x++) {
        double v = sp[x] / mean;
        if (v < 0.75) v = 0.75;
        if (v > 1.25) v = 1.25;
        ctx->bal_speed[x] = ctx->bal_have ? 0.5 * ctx->bal_speed[x] + 0.5 * v : v;
    }
    ctx->bal_have = true;
    /* per block: a launch ends with its slowest BLOCK, and blocks of one XCD differ too (+-0.5 % of a launch, half of it the
     * same blocks from launch to launch).  Lighter smoothing than for the XCDs: one block's time is noisier than the mean of 32 */
    const int grid = ctx->b->bal_grid;
    if (grid > 0 && grid <= 1024 && ctx->b->h_btime && (int)ctx->b->bal_bwork.size() == grid) {
        std::vector<double> bs((size_t)grid);
        double bmean = 0.0;
        for (int b = 0; b < grid; b++) {
            const double t = ctx->b->h_btime[b];
            if (!(t > 0.0)) return;
            bs[(size_t)b] = ctx->b->bal_bwork[(size_t)b] / t;
            bmean += bs[(size_t)b] / grid;
        }
        const bool have = ctx->bal_bgrid == grid && ctx->bal_bgroups == ctx->b->bal_groups && (int)ctx->bal_bspeed.size() == grid;
        if (!have) ctx->bal_bspeed.assign((size_t)grid, 1.0);
        for (int b = 0; b < grid; b++) {
            double v = bs[(size_t)b] / bmean;
            if (v < 0.75) v = 0.75;
            if (v > 1.25) v = 1.25;
            ctx->bal_bspeed[(size_t)b] = have ? 0.65 * ctx->bal_bspeed[(size_t)b] + 0.35 * v : v;
        }
        ctx->bal_bgrid = grid;
        ctx->bal_bgroups = ctx->b->bal_groups;
    }
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

/* after a k_fir_fused launch whose block clocks came back: speed of each XCD = steps a wave of it had / time it took */
void ffb_update(h2y_ctx *ctx)
{
    if (!ctx->b->ffb_pending) return;
    ctx->b->ffb_pending = false;
    double sp[8], mean = 0.0;
    for (int x = 0; x < 8; x++) {
        const double t = reinterpret_cast<const float *>(ctx->b->h_fstats + ctx->b->bal_slot)[x];
        if (!(t > 0.0) || !(ctx->b->ffb_work[x] > 0.0)) return;
        sp[x] = ctx->b->ffb_work[x] / t;
        mean += sp[x] / 8.0;
    }
    for (int x = 0; x < 8; x++) {
        double v = sp[x] / mean;
        if (v < 0.75) v = 0.75;
        if (v > 1.25) v = 1.25;
        ctx->ffb_speed[x] = ctx->ffb_have ? 0.5 * ctx->ffb_speed[x] + 0.5 * v : v;
    }
    ctx->ffb_have = true;
}

} // namespace

/* launch fused (+FIR) over frames [0,n) whose frame_io entries are in h_frames */
int run_frames(h2y_ctx *ctx, const h2y_desc *d, const frame_io *frames, int n, const assumed_stats *d_assumed,
               const assumed_stats *known, bool check, int fstats_offset, bool time_it)
{
    /* Y'u'v' 4:2:0 (dst_matrix_coeffs 15): the fused kernel writes tmp_pic as it is -- 4:4:4, neither shifted nor clamped to the
     * output's range -- into scratch, and k_yuvp2_420 makes the .yuv frame of it (h2y_yuvp2.hip) */
    const bool yuvp2 = d->dst_matrix == H2Y_MATRIX_YUVPRIME2 && d->dst_chroma_format_idc == H2Y_CHROMA_420;
    pix_params pp;
    derive_params(d, &pp, yuvp2);
    pp.pq_ext = ctx->d_table_ext;
    const int out_kind = yuvp2 ? H2Y_OUT_444 : out_kind_of(d);
    const bool scratch = out_kind == H2Y_OUT_444TMP || yuvp2; /* a second pass reads what the fused kernel leaves in d_tmp */
    if (yuvp2) {
        const int rc = ensure_lin(ctx);
        if (rc) return rc;
    }
    t1_sens sn;
    fused_variant var = pick_variant(ctx, d, pp, out_kind, known, &sn);
    /* k_fused_t1's redo list numbers tiles as frame * tiles + tile in 32 bits */
    if ((var.pipe == 4 || var.pipe == 5) && (uint64_t)n * make_geom(d, h2y_fused_threads(var)).tiles >= 0xFFFFFFFFull) var.pipe -= 3;
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
    if (out_kind == H2Y_OUT_444TMP && ctx->opt_fir != 1 && var.t1_ok && !ctx->cur_skip_t1 && tmp_depth_of(d) <= H2Y_FIR_INT_MAX_DEPTH) {
        /* The FIR resampler in one pass (k_fir_fused): a wave's unit of work is (frame, segment of chroma rows, strip of
         * 240 columns).  Segments: as few as give every wave of the chip a unit, never shorter than 64 rows (each cut
         * costs six recomputed row pairs).  "auto" keeps short batches, which cannot fill the chip that way, on the
         * two-pass form. */
        const uint32_t wq = (uint32_t)d->width / 4u, h2 = (uint32_t)d->height / 2u;
        const uint32_t ns = (wq + H2Y_FF_OWN_LANES - 1u) / H2Y_FF_OWN_LANES, gw = (uint32_t)ctx->n_cu * 16u;
        const uint32_t max_seg = h2 / 64u > 0u ? h2 / 64u : 1u;
        uint32_t want = (gw + (uint32_t)n * ns - 1u) / ((uint32_t)n * ns);
        if (want > max_seg) want = max_seg;
        if (want < 1u) want = 1u;
        const uint32_t seg_rows = (h2 + want - 1u) / want, nseg = (h2 + seg_rows - 1u) / seg_rows;
        const uint64_t units = (uint64_t)n * ns * nseg;
        if (ctx->opt_fir == 2 || 2u * units >= gw) {
            const bool ident = var.pipe == 4 || var.pipe == 3; /* assumed floor 0 / ceiling 1 (pipe 3: half input, the table kernel's case) */
            const uint32_t upf = ns * nseg;
            ctx->b->was_t1 = true;
            bool on_device = ctx->b->dev_frames.size() == ctx->b->frames_cap;
            if (!on_device) ctx->b->dev_frames.assign(ctx->b->frames_cap, frame_io{});
            for (int i = 0; i < n; i++) {
                const size_t idx = (size_t)ctx->slot_base + i;
                on_device = on_device && memcmp(&ctx->b->dev_frames[idx], &frames[i], sizeof(frame_io)) == 0;
                ctx->b->h_frames[idx] = frames[i];
            }
            if (!on_device) {
                HIP_TRY(ctx, hipMemcpyAsync(ctx->b->d_frames + ctx->slot_base, ctx->b->h_frames + ctx->slot_base, n * sizeof(frame_io), hipMemcpyHostToDevice, ctx->stream));
                for (int i = 0; i < n; i++) ctx->b->dev_frames[(size_t)ctx->slot_base + i] = ctx->b->h_frames[(size_t)ctx->slot_base + i];
            }
            int rc = ensure(ctx, ctx->b->d_partial, ctx->b->partial_cap, (size_t)n * upf * 6 * sizeof(float));
            if (rc) return rc;
            rc = ensure(ctx, ctx->b->d_redo, ctx->b->redo_cap, (size_t)n * upf * sizeof(uint32_t));
            if (rc) return rc;
            if (ident) {
                const size_t need = (size_t)(n > 64 ? n : 64) * sizeof(uint32_t);
                if (ctx->b->low_cap < need) {
                    rc = ensure(ctx, ctx->b->d_low, ctx->b->low_cap, need);
                    if (rc) return rc;
                    HIP_TRY(ctx, hipMemsetAsync(ctx->b->d_low, 0, need, ctx->stream));
                }
            }
            if (check) ctx->b->approx_min = ident;
            firf_args fa;
            fa.frames = ctx->b->d_frames + ctx->slot_base;
            fa.n_frames = n;
            fa.width = (uint32_t)d->width;
            fa.height = (uint32_t)d->height;
            fa.wq = wq;
            fa.n_strips = ns;
            fa.n_seg = nseg;
            fa.seg_rows = seg_rows;
            fa.units_per_frame = upf;
            fa.total_units = (uint32_t)units;
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
            fa.sn = sn;
            fa.partial = ctx->b->d_partial;
            fa.redo_count = ctx->b->d_redo;
            fa.low_flag = ident ? ctx->b->d_low : nullptr;
            fa.assumed = d_assumed;
            fa.pp = pp;
            const uint32_t blocks_needed = (uint32_t)((units + 15u) / 16u);
            const int grid = (int)(blocks_needed < (uint32_t)ctx->n_cu ? blocks_needed : (uint32_t)ctx->n_cu);
            /* Rows by XCD speed.  The XCDs of a card are not equally fast on this kernel (measured: the odd ones finish
             * 11 % later on equal shares), a wave's units are fixed, and a launch ends with its slowest wave.  Strips are
             * independent, so every (frame, strip) column is cut into its segments in proportion to the speeds of the XCDs
             * its units will run on (unit u -> wave u % GW -> block / 16 -> XCD block % 8), lead-in steps included.  The
             * speeds come from the block clocks of earlier launches (ffb_update()). */
            fa.unit_rows = nullptr;
            fa.block_clock = nullptr;
            const bool full = grid == ctx->n_cu && grid % 8 == 0;
            fa.mix_xcds = grid % 8 == 0 ? 1u : 0u;
            const bool clocks = full && time_it;
            double sp[8];
            bool weigh = full && nseg >= 2 && ctx->opt_bal_mode != 1 && (ctx->opt_bal_mode == 2 || ctx->ffb_have);
            for (int x = 0; x < 8; x++)
                sp[x] = ctx->opt_bal_mode == 2 ? (((ctx->opt_bal_mask >> x) & 1u) ? ctx->opt_bal_rho : 1.0) : ctx->ffb_speed[x];
            double work[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (weigh || clocks) {
                const uint32_t gwaves = (uint32_t)grid * 16u;
                if (weigh) {
                    if (ctx->b->unit_rows_cap < units) {
                        if (ctx->b->d_unit_rows) HIP_TRY(ctx, hipFree(ctx->b->d_unit_rows));
                        if (ctx->b->h_unit_rows) HIP_TRY(ctx, hipHostFree(ctx->b->h_unit_rows));
                        ctx->b->d_unit_rows = ctx->b->h_unit_rows = nullptr;
                        ctx->b->unit_rows_cap = 0;
                        ctx->b->dev_unit_rows.clear();
                        HIP_TRY(ctx, hipMalloc((void **)&ctx->b->d_unit_rows, units * sizeof(uint32_t)));
                        HIP_TRY(ctx, hipHostMalloc((void **)&ctx->b->h_unit_rows, units * sizeof(uint32_t), hipHostMallocDefault));
                        ctx->b->unit_rows_cap = units;
                    }
                }
                std::vector<uint32_t> rows((size_t)units);
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
                if (weigh) {
                    if (ctx->b->dev_unit_rows != rows) {
                        memcpy(ctx->b->h_unit_rows, rows.data(), units * sizeof(uint32_t));
                        HIP_TRY(ctx, hipMemcpyAsync(ctx->b->d_unit_rows, ctx->b->h_unit_rows, units * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
                        ctx->b->dev_unit_rows = rows;
                    }
                    fa.unit_rows = ctx->b->d_unit_rows;
                }
            }
            if (clocks) {
                const size_t need = (size_t)2 * grid * sizeof(unsigned long long);
                if (ctx->b->clock_cap < need) {
                    rc = ensure(ctx, ctx->b->d_clock, ctx->b->clock_cap, need);
                    if (rc) return rc;
                    HIP_TRY(ctx, hipMemsetAsync(ctx->b->d_clock, 0, need, ctx->stream)); /* k_stats_final clears the finish entries from here on */
                }
                fa.block_clock = ctx->b->d_clock;
            }
            const bool ev = time_it && ctx->b->n_ev < kMaxEvents;
            if (ev) {
                HIP_TRY(ctx, hipEventRecord(ctx->b->ev[ctx->b->n_ev][0], ctx->stream));
                ctx->last_name = "k_fir_fused";
                char buf[192];
                snprintf(buf, sizeof buf, "k_fir_fused<%s,420FIR,%s,%s%s> strips=%u segments=%u rows=%u", var.in_kind == H2Y_IN_F16 ? "F16" : "F32",
                         var.mode == H2Y_MODE_YCBCR ? "YCBCR" : "YDZDX", ident ? "PQ_IDENT" : "PQ_NORM", var.pipe == 3 ? ",LUT16" : "", ns, nseg, seg_rows);
                ctx->last_variant = buf;
            }
            HIP_TRY(ctx, h2y_launch_fir_fused(var.in_kind, var.mode, ident, var.pipe == 3 /* the 16 384-entry table applies */, grid, ctx->stream, fa));
            if (ev) {
                HIP_TRY(ctx, hipEventRecord(ctx->b->ev[ctx->b->n_ev][1], ctx->stream));
                ctx->b->n_ev++;
            }
            final_args fin;
            fin.partial = ctx->b->d_partial;
            fin.nblk = (int)upf;
            fin.redo_count = ctx->b->d_redo;
            fin.low_flag = ident ? ctx->b->d_low : nullptr;
            fin.out = ctx->b->fs_out + fstats_offset;
            fin.is_u16 = 0;
            fin.src_bit_depth = d->src_bit_depth;
            fin.check = check ? 1 : 0;
            fin.assumed = d_assumed;
            fin.publish = nullptr;
            fin.block_clock = clocks ? ctx->b->d_clock : nullptr;
            fin.grid = grid;
            fin.xcd_time = reinterpret_cast<float *>(ctx->b->fs_out + fstats_offset + n); /* the caller's copy of the statistics takes one entry more */
            HIP_TRY(ctx, h2y_launch_stats_final(n, ctx->stream, fin));
            if (clocks) {
                ctx->b->bal_slot = fstats_offset + n;
                ctx->b->ffb_pending = true;
                for (int x = 0; x < 8; x++) ctx->b->ffb_work[x] = work[x];
            }
            return 0;
        }
    }
    const geom g = make_geom(d, h2y_fused_threads(var), var.cols8 ? 8 : 4);
    const size_t npix = (size_t)d->width * d->height;
    /* one launch covers at most kMaxFramesPerLaunch frames: k_fused_t1's waves draw their tiles from one LDS counter
     * per frame of their group (H2Y_CLAIM_FRAMES of them) */
    /* (with frame groups the bound is per GROUP: a launch of g groups takes up to g x 128 frames -- sub_batch() below) */
    auto sub_batch = [&](int left) -> int {
        if (scratch) return left < kFirSubBatch ? left : kFirSubBatch;
        if (left <= kMaxFramesPerLaunch || !h2y_fused_grouped(var)) return left < kMaxFramesPerLaunch ? left : kMaxFramesPerLaunch;
        const int gridf = grid_for(ctx, var, (uint64_t)g.chunks * left);
        for (int ng = groups_cap(ctx, g.tiles, gridf); ng > 1; ng >>= 1)
            if (gridf % ng == 0) {
                int cand = left < kMaxFramesPerLaunch * ng ? left : kMaxFramesPerLaunch * ng;
                cand -= cand % ng; /* whole groups; what is left over goes into the next launch */
                return cand > kMaxFramesPerLaunch ? cand : kMaxFramesPerLaunch;
            }
        return kMaxFramesPerLaunch;
    };
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
    int sub = 0;
    for (int f0 = 0, nf = 0; f0 < n; f0 += nf, sub++) {
        nf = sub_batch(n - f0);
        const int half = sub & 1;
        if (scratch && ctx->fir_used[half]) /* scratch half still being read by an earlier FIR pass? */
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_fir[half], 0));
        /* frame descriptors: host -> device (tiny) -- unless the device already holds exactly these (a caller
         * cycling through the same buffers): one stream operation less in front of the kernel */
        bool on_device = ctx->b->dev_frames.size() == ctx->b->frames_cap;
        if (!on_device) ctx->b->dev_frames.assign(ctx->b->frames_cap, frame_io{});
        for (int i = 0; i < nf; i++) {
            frame_io io = frames[f0 + i];
            if (out_kind == H2Y_OUT_444TMP) {
                io.tmp_cb = ctx->d_tmp + ((size_t)half * fir_sub + i) * tmp_stride;
                io.tmp_cr = io.tmp_cb + npix;
            } else if (yuvp2) { /* the fused kernel writes tmp_pic where the .yuv frame would go; k_yuvp2_420 reads it */
                io.yuv = io.out;
                io.out = ctx->d_tmp + ((size_t)half * fir_sub + i) * tmp_stride;
                io.tmp_cr = nullptr;
            }
            const size_t idx = (size_t)ctx->slot_base + f0 + i;
            on_device = on_device && memcmp(&ctx->b->dev_frames[idx], &io, sizeof io) == 0;
            ctx->b->h_frames[idx] = io;
        }
        if (!on_device) {
            HIP_TRY(ctx, hipMemcpyAsync(ctx->b->d_frames + ctx->slot_base + f0, ctx->b->h_frames + ctx->slot_base + f0, nf * sizeof(frame_io), hipMemcpyHostToDevice,
                                        ctx->stream));
            for (int i = 0; i < nf; i++) ctx->b->dev_frames[(size_t)ctx->slot_base + f0 + i] = ctx->b->h_frames[(size_t)ctx->slot_base + f0 + i];
        }
        const int grid = grid_for(ctx, var, (uint64_t)g.chunks * nf);
        const int waves = h2y_fused_threads(var) / 64; /* the fused kernels leave one min/max record per wave */
        /* frame groups (frame_walk in h2y_kernels.hip): as many as divide both the batch and the grid, up to groups_cap() */
        int groups = 1;
        if (h2y_fused_grouped(var))
            for (int ng = groups_cap(ctx, g.tiles, grid); ng > 1; ng >>= 1)
                if (nf % ng == 0 && grid % ng == 0) {
                    groups = ng;
                    break;
                }
        if (nf / groups > kMaxFramesPerLaunch) return fail(ctx, H2Y_EINVAL, "internal: %d frames in %d groups exceed the per-group bound", nf, groups);
        int rc = ensure(ctx, ctx->b->d_partial, ctx->b->partial_cap, (size_t)nf * grid * waves * 6 * sizeof(float));
        if (rc) return rc;
        const bool t1 = var.pipe == 4 || var.pipe == 5;
        if (t1) {
            rc = ensure(ctx, ctx->b->d_redo, ctx->b->redo_cap, (size_t)nf * grid * waves * sizeof(uint32_t));
            if (rc) return rc;
        }
        const bool approx = var.pipe == 4; /* first tier, assumed floor 0 / ceiling 1: subsampled minimum */
        if (approx) {
            const size_t need = (size_t)(nf > 64 ? nf : 64) * sizeof(uint32_t);
            if (ctx->b->low_cap < need) {
                rc = ensure(ctx, ctx->b->d_low, ctx->b->low_cap, need);
                if (rc) return rc;
                HIP_TRY(ctx, hipMemsetAsync(ctx->b->d_low, 0, need, ctx->stream)); /* the kernels keep it zero from here on */
            }
        }
        if (check) ctx->b->approx_min = approx;
        /* XCD-aware rounds and their weights; the block clocks of timed launches feed balance_update() */
        const bool xcd_layout = h2y_fused_grouped(var) && grid % (8 * groups) == 0;
        /* Slices by XCD speed: block i of a group takes one contiguous run of every frame's 64-tile slices, as long as
         * the measured speed of its XCD says (block i of a group runs on XCD i % 8 under xcd_layout).  "off": the even
         * round-robin dealing of frame_walk. */
        const uint32_t *d_slice_ranges = nullptr;
        uint32_t range_stride = 0;
        bool tail_on = false;
        uint32_t tail_slices = 0;
        std::vector<double> bwork;
        double work[8] = {1, 1, 1, 1, 1, 1, 1, 1};
        if (xcd_layout && ctx->opt_bal_mode != 1) {
            const uint32_t G = (uint32_t)grid / (uint32_t)groups, nslices = (g.tiles + 63u) / 64u;
            double sp[8], mean = 0.0;
            for (int x = 0; x < 8; x++) {
                sp[x] = ctx->opt_bal_mode == 2 ? (((ctx->opt_bal_mask >> x) & 1u) ? ctx->opt_bal_rho : 1.0) : (ctx->bal_have ? ctx->bal_speed[x] : 1.0);
                mean += sp[x] / 8.0;
            }
            for (int x = 0; x < 8; x++) work[x] = sp[x] / mean;
            /* per block when this grid shape has been measured (adaptive mode), else per XCD: one table for every group */
            const bool per_block = ctx->opt_bal_mode == 0 && ctx->opt_bal_blocks && ctx->bal_bgrid == grid && ctx->bal_bgroups == groups &&
                                   (int)ctx->bal_bspeed.size() == grid && (size_t)groups * (G + 1u) <= kRangeWords;
            std::vector<uint32_t> r(per_block ? (size_t)groups * (G + 1u) : (size_t)G + 1u);
            bwork.assign((size_t)grid, 1.0);
            if (per_block) {
                std::vector<double> w(G);
                for (uint32_t gi = 0; gi < (uint32_t)groups; gi++) {
                    for (uint32_t i = 0; i < G; i++) w[i] = ctx->bal_bspeed[walk_block_of(gi, i, (uint32_t)groups)];
                    slice_ranges_w(w.data(), G, nslices, r.data() + (size_t)gi * (G + 1u)); /* h2y_walk.h */
                }
                range_stride = G + 1u;
            } else slice_ranges(sp, G, nslices, r.data());
            /* the dynamic last frame (k_fused_t1): its eight shards' boundaries ride behind the ranges */
            const int per_group = nf / groups;
            tail_on = t1 && ctx->opt_tail != 2 && nf % groups == 0 && per_group >= (ctx->opt_tail == 1 ? 2 : kTailMinFrames) && groups <= 16 &&

                      /* a block holds 64 chunks of H2Y_TAIL_CHUNK slices at most (H2Y_TAIL_QLEN): the group's G blocks must be able to take the
                       * whole frame with room to spare, however unevenly they draw (any block may end up in the common pool) */
                      (uint64_t)(nslices / H2Y_TAIL_CHUNK + 96u) * 2u <= 64ull * G && G >= 8u;
            tail_slices = nslices;
            for (uint32_t gi = 0; gi < (uint32_t)groups; gi++) {
                const uint32_t *rg = r.data() + (size_t)(per_block ? gi : 0u) * (G + 1u);
                for (uint32_t i = 0; i < G; i++) bwork[walk_block_of(gi, i, (uint32_t)groups)] = (double)(rg[i + 1] - rg[i]) * (double)G / (double)nslices;
            }
            if (!ctx->b->h_ranges) {
                HIP_TRY(ctx, hipHostMalloc((void **)&ctx->b->h_ranges, 2 * kRangeWords * sizeof(uint32_t), hipHostMallocMapped));
                HIP_TRY(ctx, hipHostGetDevicePointer((void **)&ctx->b->hd_ranges, ctx->b->h_ranges, 0));
                HIP_TRY(ctx, hipHostMalloc((void **)&ctx->b->h_btime, 1024 * sizeof(float), hipHostMallocMapped));
                HIP_TRY(ctx, hipHostGetDevicePointer((void **)&ctx->b->hd_btime, ctx->b->h_btime, 0));
            }
            if (r.size() > kRangeWords) return fail(ctx, H2Y_EINVAL, "internal: %zu slice ranges", r.size());
            /* The kernels read these tables IN PLACE from mapped pinned memory: a slot may only be rewritten once every launch that
             * reads it has finished.  A batch_state is handed out again only after its batch was finished (enqueue / finish,
             * h2y_convert_frame), so both slots are free at a batch's first launch -- except on the stream pipeline, which calls
             * run_frames() back to back on one state without synchronising: there the slots stay busy until the third-table
             * path below has waited for the stream. */
            if (sub == 0 && !ctx->streaming) ctx->b->slot_busy[0] = ctx->b->slot_busy[1] = false;
            int slot = -1;
            for (int k = 0; k < 2 && slot < 0; k++)
                if (ctx->b->range_slot[k] == r) slot = k;
            if (slot < 0) {
                for (int k = 0; k < 2 && slot < 0; k++)
                    if (!ctx->b->slot_busy[k]) slot = k;
                if (slot < 0) { /* a third table within one batch: wait for the launches that read the other two */
                    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                    ctx->b->slot_busy[0] = ctx->b->slot_busy[1] = false;
                    slot = 0;
                }
                memcpy(ctx->b->h_ranges + (size_t)slot * kRangeWords, r.data(), r.size() * sizeof(uint32_t));
                ctx->b->range_slot[slot] = r;
            }
            ctx->b->slot_busy[slot] = true;
            d_slice_ranges = ctx->b->hd_ranges + (size_t)slot * kRangeWords;
        }
        const bool clocks = xcd_layout && time_it;
        if (clocks) {
            const size_t need = (size_t)2 * grid * sizeof(unsigned long long);
            if (ctx->b->clock_cap < need) {
                rc = ensure(ctx, ctx->b->d_clock, ctx->b->clock_cap, need);
                if (rc) return rc;
                HIP_TRY(ctx, hipMemsetAsync(ctx->b->d_clock, 0, need, ctx->stream)); /* k_stats_final clears the finish entries from here on */
            }
        }
        fused_args a;
        a.xcd_layout = xcd_layout ? 1u : 0u;
        a.block_clock = clocks ? ctx->b->d_clock : nullptr;
        a.slice_ranges = d_slice_ranges;
        a.range_stride = range_stride;
        a.tail_ctr = nullptr;
        a.tail_slices = 0;
        if (tail_on && d_slice_ranges) {
            if (!ctx->b->d_tail) {
                HIP_TRY(ctx, hipMalloc((void **)&ctx->b->d_tail, 16 * H2Y_TAIL_WORDS * sizeof(uint32_t)));
                HIP_TRY(ctx, hipMemsetAsync(ctx->b->d_tail, 0, 16 * H2Y_TAIL_WORDS * sizeof(uint32_t), ctx->stream)); /* k_stats_final clears it from here on */
            }
            a.tail_ctr = ctx->b->d_tail;
            a.tail_slices = tail_slices;
        }
        a.redo_count = t1 ? ctx->b->d_redo : nullptr;
        a.low_flag = approx ? ctx->b->d_low : nullptr;
        a.frames = ctx->b->d_frames + ctx->slot_base + f0;
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
        a.sn = sn;
        a.partial = ctx->b->d_partial;
        a.assumed = d_assumed;
        a.pp = pp;
        if (pp.convert_transfer == 2 && !var.narrow && (var.pipe == 0 || var.pipe == 7)) {
            /* generic transfer pair through the table tier: source function, then destination function */
            static const int kSrcFn[4] = {H2Y_TFN_NONE, H2Y_TFN_PQ_F, H2Y_TFN_RHO_H, H2Y_TFN_G24};    /* by H2Y_TF_* class */
            static const int kDstFn[4] = {H2Y_TFN_NONE, H2Y_TFN_PQ_R, H2Y_TFN_RHO_R, H2Y_TFN_G24INV};
            const int sf = kSrcFn[pp.src_tf], df = kDstFn[pp.dst_tf];
            int rc2 = ensure_tfn(ctx, sf);
            if (!rc2) rc2 = ensure_tfn(ctx, df);
            if (rc2) return rc2;
            a.pp.src_fn = sf;
            a.pp.dst_fn = df;
            a.table_src = sf ? ctx->d_tfn[sf] : nullptr;
            a.table_dst = df ? ctx->d_tfn[df] : nullptr;
            a.pp.tf_ext[0] = sf ? ctx->d_tfn_ext[sf] : nullptr;
            a.pp.tf_ext[1] = df ? ctx->d_tfn_ext[df] : nullptr;
        }
        a.tiles_magic = g.tiles > 1 ? (uint32_t)(0x100000000ull / g.tiles) : 0xFFFFFFFFu;
        const bool ev = time_it && ctx->b->n_ev < kMaxEvents;
        if (ev) {
            HIP_TRY(ctx, hipEventRecord(ctx->b->ev[ctx->b->n_ev][0], ctx->stream));
            ctx->last_name = h2y_fused_name(var);
            static const char *const kIn[] = {"F32", "F16", "U16"}, *const kOut[] = {"420BOX", "444", "444TMP"};
            static const char *const kPipe[] = {"RUNTIME", "PQ_IDENT", "PQ_NORM", "LUT16", "PQ_IDENT", "PQ_NORM", "NONE", "TFN"};
            const char *mode = var.mode == H2Y_MODE_YCBCR ? "YCBCR" : var.mode == H2Y_MODE_YDZDX ? "YDZDX" : var.mode == H2Y_MODE_IDENTITY ? "IDENTITY"
                             : var.mode == H2Y_MODE_YUVP2 ? "YUVP2" : "YPQRS";
            char buf[192];
            snprintf(buf, sizeof buf, "%s<%s,%s,%s,%s%s>%s groups=%d xcd=%d%s", ctx->last_name, kIn[var.in_kind], kOut[var.out_kind], mode,
                     kPipe[var.pipe], var.cols8 ? ",COLS8" : "", out_kind == H2Y_OUT_444TMP ? "+k_fir420" : yuvp2 ? (d->chroma_resampler_type ? "+k_yuvp2_420<FIR>" : "+k_yuvp2_420<BOX>") : "", groups, xcd_layout ? 1 : 0,
                     a.tail_ctr ? " tail=1" : "");
            ctx->last_variant = buf;
        }
        HIP_TRY(ctx, h2y_launch_fused(var, grid, ctx->stream, a));
        if (ev) {
            HIP_TRY(ctx, hipEventRecord(ctx->b->ev[ctx->b->n_ev][1], ctx->stream));
            ctx->b->n_ev++;
        }
        final_args fa;
        fa.partial = ctx->b->d_partial;
        fa.nblk = grid / groups * waves;
        fa.redo_count = t1 ? ctx->b->d_redo : nullptr;
        fa.low_flag = approx ? ctx->b->d_low : nullptr;
        fa.out = ctx->b->fs_out + fstats_offset + f0;
        fa.is_u16 = d->in_sample_type == H2Y_SAMPLE_U16;
        fa.src_bit_depth = d->src_bit_depth;
        fa.check = check ? 1 : 0;
        fa.assumed = d_assumed;
        fa.publish = nullptr;
        fa.block_clock = clocks ? ctx->b->d_clock : nullptr;
        fa.grid = grid;
        static_assert(sizeof(frame_stats) >= 8 * sizeof(float), "the XCD run times ride in one frame_stats entry");
        fa.xcd_time = reinterpret_cast<float *>(ctx->b->fs_out + fstats_offset + n); /* the caller's copy of the statistics takes one entry more */
        fa.tail_ctr = a.tail_ctr;
        fa.tail_n = groups * (int)H2Y_TAIL_WORDS;
        fa.block_time = clocks && d_slice_ranges && ctx->b->fs_out == ctx->b->m_fstats ? ctx->b->hd_btime : nullptr; /* (enqueued batches: what the host reads in h2y_batch_finish) */
        HIP_TRY(ctx, h2y_launch_stats_final(nf, ctx->stream, fa));
        if (clocks) {
            ctx->b->bal_slot = fstats_offset + n;
            ctx->b->bal_pending = true;
            for (int x = 0; x < 8; x++) ctx->b->bal_work[x] = work[x];
            ctx->b->bal_grid = fa.block_time ? grid : 0;
            ctx->b->bal_groups = groups;
            ctx->b->bal_bwork = bwork;
        }
        if (yuvp2) {
            HIP_TRY(ctx, hipEventRecord(ctx->ev_fused[half], ctx->stream));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->fir_stream, ctx->ev_fused[half], 0));
            yuvp2_args ya;
            ya.frames = ctx->b->d_frames + ctx->slot_base + f0;
            ya.n_frames = nf;
            ya.width = d->width;
            ya.height = d->height;
            ya.lin = ctx->d_lin;
            ya.fir_max = pp.fir_max;
            derive_params(d, &ya.pp, false); /* the output picture's write_yuv step */
            HIP_TRY(ctx, h2y_launch_yuvp2_420(d->chroma_resampler_type == 1, ctx->fir_stream, ya));
            HIP_TRY(ctx, hipEventRecord(ctx->ev_fir[half], ctx->fir_stream));
            ctx->fir_used[half] = true;
        }
        if (out_kind == H2Y_OUT_444TMP) {
            HIP_TRY(ctx, hipEventRecord(ctx->ev_fused[half], ctx->stream));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->fir_stream, ctx->ev_fused[half], 0));
            fir_args fr;
            fr.frames = ctx->b->d_frames + ctx->slot_base + f0;
            fr.n_frames = nf;
            fr.src_cb = fr.src_cr = nullptr;
            fr.dst_cb = fr.dst_cr = nullptr;
            fr.width = d->width;
            fr.height = d->height;
            fr.fir_max = pp.fir_max;
            fr.apply_yuv_clamp = 1;
            fr.pp = pp;
            HIP_TRY(ctx, h2y_launch_fir420(ctx->fir_stream, fr));
            HIP_TRY(ctx, hipEventRecord(ctx->ev_fir[half], ctx->fir_stream));
            ctx->fir_used[half] = true;
        }
    }
    if (scratch) /* everything queued after this call on the main stream sees finished chroma */
        for (int hlf = 0; hlf < 2; hlf++)
            if (ctx->fir_used[hlf]) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_fir[hlf], 0));
    return 0;
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
    final_args fa;
    fa.partial = ctx->b->d_partial;
    fa.nblk = grid;
    fa.out = ctx->b->d_fstats + slot;
    fa.is_u16 = d->in_sample_type == H2Y_SAMPLE_U16;
    fa.src_bit_depth = d->src_bit_depth;
    fa.redo_count = nullptr;
    fa.low_flag = nullptr;
    fa.check = 0;
    fa.assumed = nullptr;
    fa.publish = publish;
    fa.block_clock = nullptr;
    fa.grid = 0;
    fa.xcd_time = nullptr;
    HIP_TRY(ctx, h2y_launch_stats_final(1, ctx->stream, fa));
    return 0;
}

int h2y_abi_version(void)
{
#ifdef H2Y_EXPERIMENT
    return H2Y_ABI_VERSION | H2Y_ABI_EXPERIMENT;
#else
    return H2Y_ABI_VERSION;
#endif
}

int h2y_desc_check(const h2y_desc *d, const char **why)
{
    const char *w = nullptr;
    int rc = H2Y_OK;
#define BAD(code, msg) do { rc = (code); w = (msg); goto done; } while (0)
    if (!d) BAD(H2Y_EINVAL, "null descriptor");
    if (d->width < 1 || d->width > 16384 || d->height < 1 || d->height > 16384) BAD(H2Y_EINVAL, "picture dimensions out of bounds");
    if (d->in_sample_type != H2Y_SAMPLE_F32 && d->in_sample_type != H2Y_SAMPLE_F16 && d->in_sample_type != H2Y_SAMPLE_U16)
        BAD(H2Y_EINVAL, "in_sample_type not recognized"); /* common.cpp:229-233 */
    if (d->dst_bit_depth < 8 || d->dst_bit_depth > 16) BAD(H2Y_EINVAL, "dst_bit_depth must be 8..16");
    if (d->in_sample_type == H2Y_SAMPLE_U16) {
        if (d->src_bit_depth < 8 || d->src_bit_depth > 16) BAD(H2Y_EINVAL, "src_bit_depth must be 8..16 for U16 input");
        if (d->dst_bit_depth > d->src_bit_depth) BAD(H2Y_EINVAL, "dst bitdepth > src bitdepth"); /* tiff.cpp:396-401 */
    }
    if (d->dst_chroma_format_idc != H2Y_CHROMA_420 && d->dst_chroma_format_idc != H2Y_CHROMA_444)
        BAD(H2Y_EUNSUPPORTED, "dst_chroma_format_idc must be 1 (4:2:0) or 3 (4:4:4)");
    if (d->dst_chroma_format_idc == H2Y_CHROMA_420) {
        if ((d->width & 1) || (d->height & 1)) BAD(H2Y_EINVAL, "4:2:0 needs even width and height");
        if (d->chroma_resampler_type == 0 && ((d->width & 3) || (d->height & 3)))
            BAD(H2Y_EINVAL, "box resampler reads 4x4 tiles: width and height must be multiples of 4"); /* convert.cpp:100-140 */
    }
    if (d->src_transfer != d->dst_transfer) {
        if (tf_class(d->src_transfer) < 0) BAD(H2Y_EUNSUPPORTED, "src_transfer_characteristics not supported (yet)");  /* convert.cpp:1061 */
        if (tf_class(d->dst_transfer) < 0) BAD(H2Y_EUNSUPPORTED, "dst_transfer_characteristics not supported (yet)");  /* convert.cpp:1107 */
    }
    if (!(d->dst_matrix == d->src_matrix && d->dst_primaries == d->src_primaries)) {
        switch (d->dst_matrix) {
        case H2Y_MATRIX_YDZDX: case H2Y_MATRIX_BT2020NC: case H2Y_MATRIX_BT709:
        case H2Y_MATRIX_YDZDX_Y100: case H2Y_MATRIX_YDZDX_Y500: case H2Y_MATRIX_YUVPRIME2: break;
        default: BAD(H2Y_EUNSUPPORTED, "can't determine color difference to use"); /* convert.cpp:1195-1197 */
        }
    }
    /* convert.cpp:600-630: the Y'u'v' branch subsamples only for resampler 1 (FIR) or 0 (box); any other value leaves
     * its planes uninitialised */
    if (d->dst_matrix == H2Y_MATRIX_YUVPRIME2 && d->dst_chroma_format_idc == H2Y_CHROMA_420 && d->chroma_resampler_type != 0 &&
        d->chroma_resampler_type != 1)
        BAD(H2Y_EUNSUPPORTED, "dst_matrix_coeffs 15 with 4:2:0 takes chroma_resampler_type 0 or 1 only");
    if (d->stats_override)
        for (int c = 0; c < 3; c++)
            if (d->src_transfer != d->dst_transfer && d->ceiling[c] == d->floor[c])
                BAD(H2Y_EINVAL, "stats override with ceiling == floor (division by zero range)");
done:
#undef BAD
    if (why) *why = w ? w : "ok";
    return rc;
}

size_t h2y_frame_bytes(const h2y_desc *d)
{
    if (!d || d->width < 1 || d->height < 1) return 0;
    size_t n = (size_t)d->width * d->height;
    size_t nc = d->dst_chroma_format_idc == H2Y_CHROMA_420 ? (size_t)(d->width >> 1) * (d->height >> 1) : n;
    return (n + 2 * nc) * sizeof(uint16_t);
}

size_t h2y_plane_bytes(const h2y_desc *d)
{
    if (!d || d->width < 1 || d->height < 1) return 0;
    return (size_t)d->width * d->height * sample_bytes(d);
}

const char *h2y_last_error(const h2y_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

/* everything h2y_ctx_create() allocates; on a failure the caller destroys the half-built context */
static int ctx_init(h2y_ctx *ctx, int device)
{
    ctx->device = device;
    for (batch_state &b : ctx->bs)
        for (int i = 0; i < kMaxEvents; i++) b.ev[i][0] = b.ev[i][1] = nullptr;
    HIP_TRY(ctx, hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(ctx, hipGetDeviceProperties(&prop, device));
    ctx->n_cu = prop.multiProcessorCount;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->fir_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) {
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_fused[i], hipEventDisableTiming));
        HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_fir[i], hipEventDisableTiming));
    }
    for (batch_state &b : ctx->bs) {
        for (int i = 0; i < kMaxEvents; i++) {
            HIP_TRY(ctx, hipEventCreate(&b.ev[i][0]));
            HIP_TRY(ctx, hipEventCreate(&b.ev[i][1]));
        }
        HIP_TRY(ctx, hipEventCreateWithFlags(&b.ev_done, hipEventDisableTiming));
    }
    /* PQ fast-tier table: built on the host once, lives in HBM, staged to LDS per block */
    {
        std::vector<pq_recA> A(H2Y_PQ_NREC);
        std::vector<pq_recB> B(H2Y_PQ_NREC);
        pq_build_table(A.data(), B.data());
        HIP_TRY(ctx, hipMalloc(&ctx->d_table, H2Y_PQ_TABLE_BYTES));
        char *t = static_cast<char *>(ctx->d_table);
        HIP_TRY(ctx, hipMemcpy(t, A.data(), H2Y_PQ_NREC * 16, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(t + H2Y_PQ_NREC * 16, B.data(), H2Y_PQ_NREC * 16, hipMemcpyHostToDevice));
        {
            std::vector<pq_ext_rec> X(H2Y_PQX_NSEG);
            pq_build_table_ext(X.data());
            HIP_TRY(ctx, hipMalloc(&ctx->d_table_ext, H2Y_PQX_TABLE_BYTES));
            HIP_TRY(ctx, hipMemcpy(ctx->d_table_ext, X.data(), H2Y_PQX_TABLE_BYTES, hipMemcpyHostToDevice));
        }
        std::vector<pq_rec1> T1(H2Y_T1_NREC);
        pq_build_table1(T1.data());
        HIP_TRY(ctx, hipMalloc(&ctx->d_table1, H2Y_T1_NREC * sizeof(pq_rec1)));
        HIP_TRY(ctx, hipMemcpy(ctx->d_table1, T1.data(), H2Y_T1_NREC * sizeof(pq_rec1), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMalloc((void **)&ctx->d_lut16, H2Y_LUT16_N * sizeof(float)));
        HIP_TRY(ctx, h2y_launch_build_lut16(ctx->stream, ctx->d_table, ctx->d_lut16));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (batch_state &b : ctx->bs) {
        HIP_TRY(ctx, hipMalloc((void **)&b.d_assumed, 2 * sizeof(assumed_stats)));
        HIP_TRY(ctx, hipHostMalloc((void **)&b.h_assumed, 2 * sizeof(assumed_stats), hipHostMallocDefault));
        ctx->b = &b;
        const int rc = reserve_batch(ctx, 64);
        if (rc) return rc;
    }
    ctx->b = &ctx->bs[0];
    return H2Y_OK;
}

int h2y_ctx_create(int device, h2y_ctx **out)
{
    if (!out) return fail(nullptr, H2Y_EINVAL, "null out pointer");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail(nullptr, H2Y_EHIP, "no HIP device (%s): this library has no CPU path", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return fail(nullptr, H2Y_EINVAL, "device %d out of range (have %d)", device, ndev);
    h2y_ctx *ctx = new (std::nothrow) h2y_ctx();
    if (!ctx) return fail(nullptr, H2Y_ENOMEM, "out of host memory");
    const int rc = ctx_init(ctx, device);
    if (rc) { /* g_err holds the reason (h2y_last_error(NULL)); nothing of the half-built context survives */
        h2y_ctx_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return H2Y_OK;
}

/* Tuning and test knobs, per context.  Nothing in this library reads the environment.
 *   "t1"      "0" | "1"                 binary32 first tier off / on (default on)
 *   "groups"  "0" | "1" .. "64"         at most this many frame groups (rounded down to a power of two; 1 = off); "0": by the frame's size (default)
 *   "cols8"   "0" | "1"                 8-column thread tiles for half input (default on)
 *   "balance" "adaptive" | "xcd" | "off" | "<xcd mask>,<ratio>"   slices by measured block speed / XCD speed only / even / fixed XCD weights (default adaptive)
 *   "tail"    "off" | "auto" | "on"     k_fused_t1: the last frame of every frame group drawn dynamically by the blocks that finish first
 *                                       (auto: groups of eight frames or more; on: two suffice; default off: measured neutral)
 *   "fir"     "auto" | "twopass" | "fused"   how the FIR resampler runs (default auto)
 *   "firsync" "0" | "1" .. "1024"       k_fir_fused: the waves of a block meet at a barrier every so many steps (power of two; 0 = never; default "auto": 1, or 0 while many pixels go to the exact tiers) */
int h2y_ctx_set_option(h2y_ctx *ctx, const char *name, const char *value)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if (!name || !value) return fail(ctx, H2Y_EINVAL, "null option name or value");
    if ((ctx->q_count > 0) || ctx->streaming) return fail(ctx, H2Y_EINVAL, "a batch is pending or a stream is open");
    if (!strcmp(name, "t1")) {
        ctx->opt_t1 = value[0] != '0';
        ctx->opt_t1_steer = strcmp(value, "always") != 0; /* "always": stay on the first tier however many pixels it passes on (timing) */
    }
    else if (!strcmp(name, "cols8")) ctx->opt_cols8 = value[0] != '0';
    else if (!strcmp(name, "firsync")) {
        int v = atoi(value), p = 1;
        if (!strcmp(value, "auto")) v = -1;
        else if (v < 0) return fail(ctx, H2Y_EINVAL, "firsync must be >= 0 or \"auto\"");
        while (2 * p <= v && p < 1024) p *= 2;
        ctx->opt_fir_sync = v > 0 ? p : v;
    } else if (!strcmp(name, "groups")) {
        int v = atoi(value), p = 1;
        if (v < 0) return fail(ctx, H2Y_EINVAL, "groups must be >= 0");
        while (2 * p <= v && p < 64) p *= 2;
        ctx->opt_groups = v ? p : 0;
    } else if (!strcmp(name, "balance")) {
        if (!strcmp(value, "adaptive")) { ctx->opt_bal_mode = 0; ctx->opt_bal_blocks = true; }
        else if (!strcmp(value, "xcd")) { ctx->opt_bal_mode = 0; ctx->opt_bal_blocks = false; } /* round 2's form: A/B timing */
        else if (!strcmp(value, "off")) ctx->opt_bal_mode = 1;
        else {
            char *end = nullptr;
            const unsigned long mm = strtoul(value, &end, 0);
            const double r = (end && *end == ',') ? atof(end + 1) : 0.0;
            if (!(mm & 0xFFu) || (mm & 0xFFu) == 0xFFu || !(r > 1.0)) return fail(ctx, H2Y_EINVAL, "balance: want adaptive, xcd, off or <mask>,<ratio > 1>");
            ctx->opt_bal_mode = 2;
            ctx->opt_bal_mask = (uint32_t)(mm & 0xFFu);
            ctx->opt_bal_rho = r;
        }
    } else if (!strcmp(name, "tail")) {
        if (!strcmp(value, "auto")) ctx->opt_tail = 0;
        else if (!strcmp(value, "on")) ctx->opt_tail = 1;
        else if (!strcmp(value, "off")) ctx->opt_tail = 2;
        else return fail(ctx, H2Y_EINVAL, "tail: want auto, on or off");
    } else if (!strcmp(name, "fir")) {
        if (!strcmp(value, "auto")) ctx->opt_fir = 0;
        else if (!strcmp(value, "twopass")) ctx->opt_fir = 1;
        else if (!strcmp(value, "fused")) ctx->opt_fir = 2;
        else return fail(ctx, H2Y_EINVAL, "fir: want auto, twopass or fused");
    } else return fail(ctx, H2Y_EINVAL, "unknown option '%s'", name);
    return H2Y_OK;
}

void h2y_ctx_destroy(h2y_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->streaming) (void)h2y_stream_close(ctx);
    for (batch_state &b : ctx->bs) {
        for (int i = 0; i < kMaxEvents; i++) {
            if (b.ev[i][0]) (void)hipEventDestroy(b.ev[i][0]);
            if (b.ev[i][1]) (void)hipEventDestroy(b.ev[i][1]);
        }
        if (b.ev_done) (void)hipEventDestroy(b.ev_done);
        (void)hipFree(b.d_frames);
        (void)hipHostFree(b.h_frames);
        (void)hipFree(b.d_partial);
        (void)hipFree(b.d_redo);
        (void)hipFree(b.d_low);
        (void)hipFree(b.d_clock);
        (void)hipHostFree(b.h_ranges);
        (void)hipHostFree(b.h_btime);
        (void)hipFree(b.d_tail);
        (void)hipFree(b.d_unit_rows);
        (void)hipHostFree(b.h_unit_rows);
        (void)hipFree(b.d_fstats);
        (void)hipHostFree(b.h_fstats);
        (void)hipFree(b.d_assumed);
        (void)hipHostFree(b.h_assumed);
    }
    (void)hipFree(ctx->d_table);
    for (void *t : ctx->d_tfn) (void)hipFree(t);
    for (int fn = 0; fn < H2Y_TFN_COUNT; fn++)
        if (ctx->d_tfn_ext[fn] && ctx->d_tfn_ext[fn] != ctx->d_table_ext) (void)hipFree(ctx->d_tfn_ext[fn]);
    (void)hipFree(ctx->d_lut16);
    (void)hipFree(ctx->d_table1);
    (void)hipFree(ctx->d_table_ext);
    (void)hipFree(ctx->d_tmp);
    (void)hipFree(ctx->d_lin);
    (void)hipFree(ctx->d_tab);
    (void)hipHostFree(ctx->h_tab);
    (void)hipFree(ctx->d_cmp_part);
    (void)hipFree(ctx->d_cmp_stats);
    (void)hipFree(ctx->d_hist);
    (void)hipFree(ctx->d_ssim_part);
    (void)hipFree(ctx->d_ssim_stats);
    (void)hipFree(ctx->d_light_as);
    (void)hipFree(ctx->d_light_acc);
    (void)hipFree(ctx->d_scale_tabs);
    (void)hipFree(ctx->d_in);
    (void)hipFree(ctx->d_out);
    if (ctx->fir_stream) {
        (void)hipStreamSynchronize(ctx->fir_stream);
        (void)hipStreamDestroy(ctx->fir_stream);
    }
    for (int i = 0; i < 2; i++) {
        if (ctx->ev_fused[i]) (void)hipEventDestroy(ctx->ev_fused[i]);
        if (ctx->ev_fir[i]) (void)hipEventDestroy(ctx->ev_fir[i]);
    }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

int h2y_ctx_set_stream(h2y_ctx *ctx, void *hip_stream)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0)) return fail(ctx, H2Y_EINVAL, "a batch is pending: call h2y_batch_finish first");
    if (ctx->streaming) return fail(ctx, H2Y_EINVAL, "a stream is open: close it first");
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return H2Y_OK;
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
    if (!needs_stats || d->stats_override) {
        assumed_stats want;
        for (int c = 0; c < 3; c++) {
            want.floor_[c] = d->stats_override ? d->floor[c] : 0;
            want.ceil_[c] = d->stats_override ? d->ceiling[c] : 1;
        }
        if (!ctx->b->dev_assumed_ok || memcmp(&want, &ctx->b->dev_assumed, sizeof want) != 0) {
            *as = want;
            HIP_TRY(ctx, hipMemcpyAsync(ctx->b->d_assumed, as, sizeof *as, hipMemcpyHostToDevice, ctx->stream));
            ctx->b->dev_assumed = want;
            ctx->b->dev_assumed_ok = true;
        } else *as = want;
    } else if (ctx->have_hint && ctx->hint_kind == d->in_sample_type) {
        /* assume this batch looks like the last frame we saw; verified below */
        assumed_stats want;
        for (int c = 0; c < 3; c++) {
            want.floor_[c] = ctx->hint_floor[c];
            want.ceil_[c] = ctx->hint_ceil[c];
        }
        if (!ctx->b->dev_assumed_ok || memcmp(&want, &ctx->b->dev_assumed, sizeof want) != 0) {
            *as = want;
            HIP_TRY(ctx, hipMemcpyAsync(ctx->b->d_assumed, as, sizeof *as, hipMemcpyHostToDevice, ctx->stream));
            ctx->b->dev_assumed = want;
            ctx->b->dev_assumed_ok = true;
        } else *as = want; /* (the host copy is what pick_variant() reads) */
        check = true;
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
    float ms = 0.f;
    for (int i = 0; i < ctx->b->n_ev; i++) {
        float t = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&t, ctx->b->ev[i][0], ctx->b->ev[i][1]));
        ms += t;
    }
    ctx->last_ms = ms;
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
    float ms = 0.f;
    for (int i = 0; i < ctx->b->n_ev; i++) {
        float t = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&t, ctx->b->ev[i][0], ctx->b->ev[i][1]));
        ms += t;
    }
    ctx->last_ms = ms;
    ctx->last_launches = ctx->b->n_ev;
    return H2Y_OK;
}

/* matrix_inverse()'s scalars (convert.cpp:1320-1867): everything of inverse_args but the plane pointers */
static void inverse_setup(inverse_args &a, int width, int height, int in_bit_depth, int in_full_range, int in_matrix_coeffs, int out_bit_depth)
{
    const clip_limits ic = make_clip(in_bit_depth, in_full_range);
    a.npix = (uint32_t)width * (uint32_t)height;
    a.d709 = in_matrix_coeffs == H2Y_MATRIX_BT709;
    a.minVR = ic.minVR;
    a.maxVR = ic.maxVR;
    a.shift_right = in_bit_depth > out_bit_depth;
    a.shift = a.shift_right ? in_bit_depth - out_bit_depth : out_bit_depth - in_bit_depth;
}

/* ... and those of the 4:2:0 flow (yuv2tiff.cpp:92-93,142-154: minCV 0, maxCV 2^depth - 1 for the upsampling) */
void inverse420_setup(inv420_args &a, int width, int height, int in_bit_depth, int in_full_range, int in_matrix_coeffs,
                             int out_bit_depth, int algorithm)
{
    a.up.src0 = a.up.src1 = nullptr;
    a.up.dst0 = a.up.dst1 = nullptr;
    a.up.width = width; a.up.height = height;
    a.up.algorithm = algorithm;
    a.up.fmin = 0.0f; a.up.fmax = (float)((1u << in_bit_depth) - 1u);
    for (int c = 0; c < 3; c++) {
        a.inv.in[c] = nullptr;
        a.inv.out[c] = nullptr;
    }
    inverse_setup(a.inv, width, height, in_bit_depth, in_full_range, in_matrix_coeffs, out_bit_depth);
}

int h2y_matrix_inverse(h2y_ctx *ctx, int width, int height, int in_bit_depth, int in_full_range, int in_matrix_coeffs,
                       int out_bit_depth, const uint16_t *const d_in[3], uint16_t *const d_out[3])
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0) || ctx->streaming) return fail(ctx, H2Y_EINVAL, "a batch is pending or a stream is open");
    if (width < 1 || height < 1 || (uint64_t)width * height >= (1ull << 28)) return fail(ctx, H2Y_EINVAL, "bad picture size");
    if (in_bit_depth < 8 || in_bit_depth > 16 || out_bit_depth < 8 || out_bit_depth > 16) return fail(ctx, H2Y_EINVAL, "bit depths must be 8..16");
    if (in_matrix_coeffs == H2Y_MATRIX_GBR) /* convert.cpp:1733-1736: "Can't determine color difference to use?" and exit(0) */
        return fail(ctx, H2Y_EUNSUPPORTED, "matrix_coeffs 0 (GBR) has no inverse in the reference (it exits)");
    if (!d_in || !d_out) return fail(ctx, H2Y_EINVAL, "null pointer arrays");
    inverse_args a;
    for (int c = 0; c < 3; c++) {
        if (!d_in[c] || !d_out[c] || ((uintptr_t)d_in[c] & 7) || ((uintptr_t)d_out[c] & 7))
            return fail(ctx, H2Y_EINVAL, "plane %d is null or not 8-byte aligned", c);
        a.in[c] = d_in[c];
        a.out[c] = d_out[c];
    }
    inverse_setup(a, width, height, in_bit_depth, in_full_range, in_matrix_coeffs, out_bit_depth);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t blocks = (a.npix / 4 + 255) / 256;
    if (blocks > (uint32_t)ctx->n_cu * 16u) blocks = (uint32_t)ctx->n_cu * 16u;
    if (blocks < 1) blocks = 1;
    ctx->b->n_ev = 0;
    HIP_TRY(ctx, hipEventRecord(ctx->b->ev[0][0], ctx->stream));
    HIP_TRY(ctx, h2y_launch_inverse((int)blocks, ctx->stream, a));
    HIP_TRY(ctx, hipEventRecord(ctx->b->ev[0][1], ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->b->ev[0][0], ctx->b->ev[0][1]));
    ctx->last_ms = ms;
    ctx->last_launches = 1;
    ctx->last_name = "k_inverse";
    ctx->last_variant = "k_inverse";
    return H2Y_OK;
}

/* Subsample420to444(), convert.cpp:1869-1986 */
static int upsample_launch(h2y_ctx *ctx, int width, int height, int algorithm, unsigned min_cv, unsigned max_cv, const uint16_t *s0,
                           const uint16_t *s1, uint16_t *d0, uint16_t *d1)
{
    up_args a;
    a.src0 = s0; a.src1 = s1; a.dst0 = d0; a.dst1 = d1;
    a.width = width; a.height = height;
    a.algorithm = algorithm;
    a.fmin = (float)min_cv; a.fmax = (float)max_cv;
    HIP_TRY(ctx, h2y_launch_up444(ctx->stream, a));
    return H2Y_OK;
}

int h2y_upsample_444(h2y_ctx *ctx, int width, int height, int algorithm, unsigned min_cv, unsigned max_cv, const uint16_t *d_src,
                     uint16_t *d_dst)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0) || ctx->streaming) return fail(ctx, H2Y_EINVAL, "a batch is pending or a stream is open");
    /* odd sizes: the reference's FIR branch reads rows of its intermediate it never wrote (convert.cpp:1949 walks
     * j < height over 2 * (height / 2) written rows): no defined bytes */
    if (width < 2 || height < 2 || (width & 1) || (height & 1) || width > 32766 || height > 32766)
        return fail(ctx, H2Y_EINVAL, "upsample: width and height must be even, 2..32766 (the reference takes them as short)");
    if (min_cv > max_cv || max_cv > 65535u) return fail(ctx, H2Y_EINVAL, "upsample: need minCV <= maxCV <= 65535");
    if (!d_src || !d_dst || ((uintptr_t)d_src & 1) || ((uintptr_t)d_dst & 3)) return fail(ctx, H2Y_EINVAL, "upsample: null pointer, or the result plane is not 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = upsample_launch(ctx, width, height, algorithm, min_cv, max_cv, d_src, nullptr, d_dst, nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return H2Y_OK;
}

int h2y_inverse_420(h2y_ctx *ctx, int width, int height, int in_bit_depth, int in_full_range, int in_matrix_coeffs, int out_bit_depth,
                    int algorithm, const uint16_t *const d_in[3], uint16_t *const d_out[3])
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0) || ctx->streaming) return fail(ctx, H2Y_EINVAL, "a batch is pending or a stream is open");
    if (width < 2 || height < 2 || (width & 3) || (height & 1) || width > 32766 || height > 32766)
        return fail(ctx, H2Y_EINVAL, "4:2:0 inverse: width a multiple of 4 and height even, up to 32766"); /* the upsampled planes feed 8-byte loads */
    if (in_bit_depth < 8 || in_bit_depth > 16) return fail(ctx, H2Y_EINVAL, "bit depths must be 8..16");
    if (!d_in || !d_in[0] || !d_in[1] || !d_in[2]) return fail(ctx, H2Y_EINVAL, "null pointer arrays");
    if (out_bit_depth < 8 || out_bit_depth > 16) return fail(ctx, H2Y_EINVAL, "bit depths must be 8..16");
    if (in_matrix_coeffs == H2Y_MATRIX_GBR) return fail(ctx, H2Y_EUNSUPPORTED, "matrix_coeffs 0 (GBR) has no inverse in the reference (it exits)");
    if (!d_out || !d_out[0] || !d_out[1] || !d_out[2]) return fail(ctx, H2Y_EINVAL, "null pointer arrays");
    for (int c = 0; c < 3; c++)
        if (((uintptr_t)d_in[c] & 3) || ((uintptr_t)d_out[c] & 3)) return fail(ctx, H2Y_EINVAL, "plane %d is not 4-byte aligned", c);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    /* one pass: both chroma planes upsampled inside the blocks (yuv2tiff.cpp:92-93,142-154: minCV 0, maxCV 2^depth - 1), then
     * matrix_inverse's pixel; the 4:4:4 chroma never reaches memory (k_inverse420, h2y_resample.hip) */
    inv420_args a;
    inverse420_setup(a, width, height, in_bit_depth, in_full_range, in_matrix_coeffs, out_bit_depth, algorithm);
    a.up.src0 = d_in[1]; a.up.src1 = d_in[2];
    a.inv.in[0] = d_in[0];
    for (int c = 0; c < 3; c++) a.inv.out[c] = d_out[c];
    ctx->b->n_ev = 0;
    HIP_TRY(ctx, hipEventRecord(ctx->b->ev[0][0], ctx->stream));
    HIP_TRY(ctx, h2y_launch_inverse420(ctx->stream, a));
    HIP_TRY(ctx, hipEventRecord(ctx->b->ev[0][1], ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->b->ev[0][0], ctx->b->ev[0][1]));
    ctx->last_ms = ms;
    ctx->last_launches = 1;
    ctx->last_name = "k_inverse420";
    ctx->last_variant = algorithm ? "k_inverse420<FIR>" : "k_inverse420<REPLICATE>";
    return H2Y_OK;
}

int h2y_inverse_frame(h2y_ctx *ctx, int width, int height, int in_chroma_format_idc, int in_bit_depth, int in_full_range,
                      int in_matrix_coeffs, int out_bit_depth, int algorithm, const uint16_t *const in_planes[3], uint16_t *const out_planes[3])
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0) || ctx->streaming) return fail(ctx, H2Y_EINVAL, "a batch is pending or a stream is open");
    if (in_chroma_format_idc != H2Y_CHROMA_444 && in_chroma_format_idc != H2Y_CHROMA_420)
        return fail(ctx, H2Y_EUNSUPPORTED, "inverse flow: input chroma_format_idc must be 3 (4:4:4) or 1 (4:2:0)");
    if (width < 1 || height < 1 || (uint64_t)width * height >= (1ull << 28)) return fail(ctx, H2Y_EINVAL, "bad picture size");
    if (!in_planes || !out_planes) return fail(ctx, H2Y_EINVAL, "null pointer arrays");
    for (int c = 0; c < 3; c++)
        if (!in_planes[c] || !out_planes[c]) return fail(ctx, H2Y_EINVAL, "plane %d is null", c);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool sub = in_chroma_format_idc == H2Y_CHROMA_420;
    const size_t pb = (size_t)width * height * sizeof(uint16_t), pb_al = (pb + 255) & ~(size_t)255;
    const size_t cb = sub ? (size_t)(width >> 1) * (height >> 1) * sizeof(uint16_t) : pb;
    int rc = ensure(ctx, ctx->d_in, ctx->in_cap, 3 * pb_al);
    if (rc) return rc;
    rc = ensure(ctx, ctx->d_out, ctx->out_cap, 3 * pb_al);
    if (rc) return rc;
    const uint16_t *din[3];
    uint16_t *dout[3];
    for (int c = 0; c < 3; c++) {
        din[c] = reinterpret_cast<const uint16_t *>((char *)ctx->d_in + c * pb_al);
        dout[c] = reinterpret_cast<uint16_t *>((char *)ctx->d_out + c * pb_al);
        HIP_TRY(ctx, hipMemcpyAsync((void *)din[c], in_planes[c], c ? cb : pb, hipMemcpyHostToDevice, ctx->stream));
    }
    rc = sub ? h2y_inverse_420(ctx, width, height, in_bit_depth, in_full_range, in_matrix_coeffs, out_bit_depth, algorithm, din, dout)
             : h2y_matrix_inverse(ctx, width, height, in_bit_depth, in_full_range, in_matrix_coeffs, out_bit_depth, din, dout);
    if (rc) return rc;
    for (int c = 0; c < 3; c++) HIP_TRY(ctx, hipMemcpyAsync(out_planes[c], dout[c], pb, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return H2Y_OK;
}

/* What h2y_inverse_batch and h2y_inverse_stream_open accept: the checks of h2y_inverse_420 (4:2:0) or h2y_matrix_inverse (4:4:4) */
int inverse_check(h2y_ctx *ctx, const inv_params &p)
{
    if (p.chroma != H2Y_CHROMA_444 && p.chroma != H2Y_CHROMA_420)
        return fail(ctx, H2Y_EUNSUPPORTED, "inverse flow: input chroma_format_idc must be 3 (4:4:4) or 1 (4:2:0)");
    if (p.chroma == H2Y_CHROMA_420) {
        if (p.width < 2 || p.height < 2 || (p.width & 3) || (p.height & 1) || p.width > 32766 || p.height > 32766)
            return fail(ctx, H2Y_EINVAL, "4:2:0 inverse: width a multiple of 4 and height even, up to 32766");
    } else if (p.width < 1 || p.height < 1 || (uint64_t)p.width * p.height >= (1ull << 28))
        return fail(ctx, H2Y_EINVAL, "bad picture size");
    if (p.in_depth < 8 || p.in_depth > 16 || p.out_depth < 8 || p.out_depth > 16) return fail(ctx, H2Y_EINVAL, "bit depths must be 8..16");
    if (p.matrix == H2Y_MATRIX_GBR) return fail(ctx, H2Y_EUNSUPPORTED, "matrix_coeffs 0 (GBR) has no inverse in the reference (it exits)");
    return H2Y_OK;
}

/* h2y_dpx_decode_batch, h2y_tiff_decode_batch, h2y_exr_decode_batch: src's decode of n_frames payloads into their planes */
template <typename P>
static int decode_batch(h2y_ctx *ctx, const decode_src &src, int per_launch, int n_frames, const void *const *d_payload, P *const *d_planes)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0) || ctx->streaming) return fail(ctx, H2Y_EINVAL, "a batch is pending or a stream is open");
    int rc = src.check(ctx);
    if (rc) return rc;
    if (n_frames < 1) return fail(ctx, H2Y_EINVAL, "n_frames must be >= 1");
    if (!d_payload || !d_planes) return fail(ctx, H2Y_EINVAL, "null pointer arrays");
    const uintptr_t al = src.align();
    for (int f = 0; f < n_frames; f++) {
        if (!d_payload[f]) return fail(ctx, H2Y_EINVAL, "frame %d: payload is null", f);
        if ((uintptr_t)d_payload[f] & (al - 1)) return fail(ctx, H2Y_EINVAL, "frame %d: payload is not %d-byte aligned", f, (int)al);
        for (int c = 0; c < 3; c++) {
            const P *p = d_planes[3 * f + c];
            if (!p) return fail(ctx, H2Y_EINVAL, "frame %d: plane %d is null", f, c);
            if ((uintptr_t)p & (al - 1)) return fail(ctx, H2Y_EINVAL, "frame %d: plane %d is not %d-byte aligned", f, c, (int)al);
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    payload_frame *h;
    rc = frame_table(ctx, n_frames, h);
    if (rc) return rc;
    for (int f = 0; f < n_frames; f++) {
        h[f].payload = d_payload[f];
        for (int c = 0; c < 3; c++) h[f].plane[c] = d_planes[3 * f + c];
    }
    rc = timed_launches(ctx, h, n_frames, per_launch, src.kernel(),
                        [&](const payload_frame *frames, int, int nf) { return src.launch(ctx, frames, nf); });
    if (rc) return rc;
    ctx->last_variant = src.variant();
    return H2Y_OK;
}

int h2y_inverse_batch(h2y_ctx *ctx, int width, int height, int in_chroma_format_idc, int in_bit_depth, int in_full_range,
                      int in_matrix_coeffs, int out_bit_depth, int algorithm, int n_frames, const uint16_t *const *d_in,
                      uint16_t *const *d_out)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0) || ctx->streaming) return fail(ctx, H2Y_EINVAL, "a batch is pending or a stream is open");
    const inv_params p{width, height, in_chroma_format_idc, in_bit_depth, in_full_range, in_matrix_coeffs, out_bit_depth, algorithm};
    int rc = inverse_check(ctx, p);
    if (rc) return rc;
    if (n_frames < 1) return fail(ctx, H2Y_EINVAL, "n_frames must be >= 1");
    if (!d_in || !d_out) return fail(ctx, H2Y_EINVAL, "null pointer arrays");
    const bool sub = in_chroma_format_idc == H2Y_CHROMA_420;
    const uintptr_t align = sub ? 4 : 8; /* k_inverse420_batch: 4-byte accesses at least; k_inverse_batch: 8-byte ones */
    for (int f = 0; f < n_frames; f++)
        for (int c = 0; c < 3; c++) {
            const uint16_t *i = d_in[3 * f + c], *o = d_out[3 * f + c];
            if (!i || !o) return fail(ctx, H2Y_EINVAL, "frame %d: plane %d is null", f, c);
            if (((uintptr_t)i | (uintptr_t)o) & (align - 1)) return fail(ctx, H2Y_EINVAL, "frame %d: plane %d is not %d-byte aligned", f, c, (int)align);
        }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    inv_frame *h;
    rc = frame_table(ctx, n_frames, h);
    if (rc) return rc;
    for (int f = 0; f < n_frames; f++)
        for (int c = 0; c < 3; c++) {
            h[f].in[c] = d_in[3 * f + c];
            h[f].out[c] = d_out[3 * f + c];
        }
    inv420_args a;
    inverse420_setup(a, width, height, in_bit_depth, in_full_range, in_matrix_coeffs, out_bit_depth, algorithm);
    /* units of one frame: k_inverse420's tiles, or k_inverse's chunks of 256 quads (+ the npix % 4 single samples) */
    const uint32_t n4 = a.inv.npix >> 2;
    const uint32_t per_frame = sub ? (uint32_t)h2y_inverse420_tiles(width, height) : (n4 + (a.inv.npix & 3u) + 255) / 256;
    const uint32_t max_grid = (uint32_t)ctx->n_cu * (sub ? 8u : 16u); /* as k_inverse420 (eight blocks of 256 per CU) and k_inverse */
    rc = timed_launches(ctx, h, n_frames, H2Y_INVERSE_FRAMES_PER_LAUNCH, sub ? "k_inverse420_batch" : "k_inverse_batch",
                        [&](const inv_frame *frames, int, int nf) {
                            const uint64_t units = (uint64_t)nf * per_frame;
                            const int grid = (int)(units < max_grid ? units : max_grid);
                            return sub ? h2y_launch_inverse420_batch(grid, ctx->stream, a, frames, nf)
                                       : h2y_launch_inverse_batch(grid, ctx->stream, a.inv, frames, nf);
                        });
    if (rc) return rc;
    ctx->last_variant = sub ? (algorithm ? "k_inverse420_batch<FIR>" : "k_inverse420_batch<REPLICATE>") : "k_inverse_batch";
    return H2Y_OK;
}

/* ---- DPX input (dpx_read(), dpx.cpp:209-520; muxed_dpx_to_planar_float_buf(), common.cpp:14-27) -------------------- */

static int dpx_fmt_of(int bit_size) { return bit_size == 10 ? H2Y_DPX_10 : bit_size == 16 ? H2Y_DPX_16 : H2Y_DPX_F32; }
static uint64_t dpx_pixel_bytes(int bit_size) { return bit_size == 10 ? 4 : bit_size == 16 ? 6 : 12; }

/* what h2y_dpx_parse can return, and nothing else */
static int dpx_info_check(h2y_ctx *ctx, const h2y_dpx_info *di)
{
    if (!di) return fail(ctx, H2Y_EINVAL, "null h2y_dpx_info");
    if (di->bit_size != 10 && di->bit_size != 16 && di->bit_size != 32) return fail(ctx, H2Y_EINVAL, "DPX bit_size must be 10, 16 or 32");
    if (di->width < 1 || di->width > 32767 || di->height < 1 || di->height > 32767) return fail(ctx, H2Y_EINVAL, "DPX width and height must be 1..32767");
    if (di->swap != 0 && di->swap != 1) return fail(ctx, H2Y_EINVAL, "DPX swap must be 0 or 1");
    if (di->payload_bytes != (uint64_t)di->width * (uint64_t)di->height * dpx_pixel_bytes(di->bit_size))
        return fail(ctx, H2Y_EINVAL, "DPX payload_bytes is not width x height x bytes per pixel");
    return H2Y_OK;
}

static uint32_t dpx_u32(const unsigned char *p, bool swap) /* the reference's native (little-endian) read, INT_SW when swapping */
{
    const uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    return swap ? __builtin_bswap32(v) : v;
}

int h2y_dpx_parse(const void *header, size_t n, uint64_t file_bytes, h2y_dpx_info *out, const char **why)
{
    const char *w = nullptr;
    const unsigned char *h = static_cast<const unsigned char *>(header);
    h2y_dpx_info di{};
    if (!header || !out) w = "null argument";
    else if (n < 2048) w = "DPX header shorter than 2048 bytes"; /* dpx.cpp:283 reads 2048 and never checks how many came */
    else {
        const uint32_t magic = dpx_u32(h, false);
        if (magic != 0x53445058u && magic != 0x58504453u) w = "bad magic number in dpx header"; /* dpx.cpp:285-298 */
        else {
            di.swap = magic == 0x58504453u;
            di.width = (int16_t)(uint16_t)dpx_u32(h + 772, di.swap); /* `wide = tmp;` uint to short, dpx.cpp:300-310 */
            di.height = (int16_t)(uint16_t)dpx_u32(h + 776, di.swap);
            di.bit_size = (signed char)h[803];
            di.data_offset = dpx_u32(h + 4, di.swap); /* dpx.cpp:343-347 */
            if (di.bit_size == 12) w = "dpx packing is 12-bit, which is not supported"; /* dpx.cpp:330-333 */
            else if (di.bit_size != 10 && di.bit_size != 16 && di.bit_size != 32) w = "dpx element bit size is not 10, 16 or 32";
            else if (di.width < 1 || di.height < 1) w = "dpx width or height (narrowed to short) is outside 1..32767";
            else {
                di.payload_bytes = (uint64_t)di.width * (uint64_t)di.height * dpx_pixel_bytes(di.bit_size);
                if (di.data_offset + di.payload_bytes > file_bytes) w = "dpx payload runs past the end of the file";
            }
        }
    }
    if (why) *why = w ? w : "";
    if (w) return fail(nullptr, H2Y_EINVAL, "%s", w);
    *out = di;
    return H2Y_OK;
}

/* decode_src's DPX launch and variant: k_dpx_decode on n frames of a table */
static hipError_t dpx_decode(const h2y_ctx *ctx, const h2y_dpx_info &di, const payload_frame *frames, int n)
{
    const int fmt = dpx_fmt_of(di.bit_size);
    const uint32_t npix = (uint32_t)di.width * (uint32_t)di.height;
    return h2y_launch_dpx_decode(fmt, di.swap != 0, unit_grid(ctx, (uint64_t)n * h2y_dpx_chunks(fmt, npix)), ctx->stream, npix, frames, n);
}

static std::string dpx_variant(const h2y_dpx_info &di)
{
    const int fmt = dpx_fmt_of(di.bit_size);
    return std::string("k_dpx_decode<") + (fmt == H2Y_DPX_10 ? "10" : fmt == H2Y_DPX_16 ? "16" : "F32") + (di.swap ? ",SWAP>" : ",NOSWAP>");
}

int h2y_dpx_decode_batch(h2y_ctx *ctx, const h2y_dpx_info *info, int n_frames, const void *const *d_payload, float *const *d_planes)
{
    return decode_batch(ctx, decode_src(info), H2Y_DPX_FRAMES_PER_LAUNCH, n_frames, d_payload, d_planes);
}

/* ---- 16-bit RGB TIFF (read_tiff(), tiff.cpp:54-362; write_tiff(), tiff.cpp:559-652) ------------------------------------- */

namespace {

struct tiff_reader { /* a classic TIFF in memory, in its byte order */
    const unsigned char *p;
    size_t n;
    bool mm;
    uint32_t u16(size_t at) const { return mm ? (uint32_t)p[at] << 8 | p[at + 1] : (uint32_t)p[at + 1] << 8 | p[at]; }
    uint32_t u32(size_t at) const
    {
        return mm ? (uint32_t)p[at] << 24 | (uint32_t)p[at + 1] << 16 | (uint32_t)p[at + 2] << 8 | p[at + 3]
                  : (uint32_t)p[at + 3] << 24 | (uint32_t)p[at + 2] << 16 | (uint32_t)p[at + 1] << 8 | p[at];
    }
};

struct tiff_field { /* one IFD entry the decoder reads: SHORT or LONG values, inline or at `at` */
    bool present = false;
    uint32_t type = 0, count = 0;
    size_t at = 0;
    uint32_t get(const tiff_reader &r, uint32_t k) const { return type == 3 ? r.u16(at + 2 * (size_t)k) : r.u32(at + 4 * (size_t)k); }
};

} // namespace

int h2y_tiff_parse(const void *file, size_t file_bytes, int cutout, h2y_tiff_info *out, uint64_t *row_offsets, int row_capacity,
                   const char **why)
{
    const char *w = nullptr;
    h2y_tiff_info ti{};
    tiff_reader r{static_cast<const unsigned char *>(file), file_bytes, false};
    tiff_field fw, fh, fbps, fcomp, fso, fspp, frps, fsbc, fplanar, ffmt;
    auto parse = [&]() -> const char * {
        if (!file || !out) return "null argument";
        if (cutout & ~(H2Y_TIFF_CUTOUT_HD | H2Y_TIFF_CUTOUT_QHD)) return "cutout must be a combination of H2Y_TIFF_CUTOUT_HD and _QHD";
        if (file_bytes < 8) return "not a TIFF: shorter than its 8-byte header";
        if (r.p[0] == 'I' && r.p[1] == 'I') r.mm = false;
        else if (r.p[0] == 'M' && r.p[1] == 'M') r.mm = true;
        else return "not a TIFF: the byte order mark is neither II nor MM";
        const uint32_t version = r.u16(2);
        if (version == 43) return "BigTIFF is not supported (classic TIFF only)";
        if (version != 42) return "not a TIFF: version is not 42";
        const uint64_t ifd = r.u32(4);
        if (ifd < 8 || ifd + 2 > file_bytes) return "truncated IFD: its offset is past the end of the file";
        const uint32_t entries = r.u16((size_t)ifd);
        if (ifd + 2 + 12ull * entries > file_bytes) return "truncated IFD: its entries run past the end of the file";
        for (uint32_t e = 0; e < entries; e++) {
            const size_t at = (size_t)ifd + 2 + 12 * (size_t)e;
            tiff_field *f = nullptr;
            switch (r.u16(at)) {
            case 256: f = &fw; break;
            case 257: f = &fh; break;
            case 258: f = &fbps; break;
            case 259: f = &fcomp; break;
            case 273: f = &fso; break;
            case 277: f = &fspp; break;
            case 278: f = &frps; break;
            case 279: f = &fsbc; break;
            case 284: f = &fplanar; break;
            case 339: f = &ffmt; break;
            default: continue; /* tags read_tiff does not look at */
            }
            f->present = true;
            f->type = r.u16(at + 2);
            f->count = r.u32(at + 4);
            if (f->type != 3 && f->type != 4) return "a tag the decoder reads is neither SHORT nor LONG";
            if (f->count < 1) return "a tag the decoder reads has no value";
            const uint64_t bytes = (uint64_t)f->count * (f->type == 3 ? 2 : 4);
            f->at = bytes <= 4 ? at + 8 : (size_t)r.u32(at + 8);
            if (bytes > 4 && (uint64_t)f->at + bytes > file_bytes) return "an array runs past the end of the file";
        }
        if (!fw.present || !fh.present || !fso.present || !fsbc.present)
            return "ImageWidth, ImageLength, StripOffsets or StripByteCounts is missing";
        if (fcomp.present && fcomp.get(r, 0) != 1) return "Compression is not 1 (uncompressed strips only)";
        const uint32_t spp = fspp.present ? fspp.get(r, 0) : 1;
        if (spp != 3) return "SamplesPerPixel is not 3 (R, G, B)";
        if (!fbps.present) return "BitsPerSample is not 16";
        for (uint32_t k = 0; k < spp; k++)
            if (fbps.get(r, fbps.count < spp ? 0 : k) != 16) return "BitsPerSample is not 16";
        const uint32_t planar = fplanar.present ? fplanar.get(r, 0) : 1;
        if (planar == 2) return "PlanarConfig 2 (separate planes) is not supported";
        if (planar != 1) return "PlanarConfig is not 1";
        if (ffmt.present)
            for (uint32_t k = 0; k < spp; k++)
                if (ffmt.get(r, ffmt.count < spp ? 0 : k) != 1) return "SampleFormat is not 1 (unsigned integer)";
        const uint32_t W = fw.get(r, 0), H = fh.get(r, 0);
        if (W < 1 || H < 1 || W > (1u << 20) || H > (1u << 20)) return "ImageWidth or ImageLength is outside 1..1048576";
        uint32_t rps = frps.present ? frps.get(r, 0) : H;
        if (rps < 1) return "RowsPerStrip is 0";
        if (rps > H) rps = H;
        const uint32_t strips = (H + rps - 1) / rps;
        if (fso.count != strips || fsbc.count != strips) return "StripOffsets or StripByteCounts does not have one entry per strip";
        const uint64_t rb = 6ull * W;
        for (uint32_t s = 0; s < strips; s++) {
            const uint64_t rows = s + 1 < strips ? rps : H - (uint64_t)s * rps, bc = fsbc.get(r, s), off = fso.get(r, s);
            if (rows == 1 && bc != rb) return "a one-row strip's byte count is not 6 x ImageWidth";
            if (bc < rows * rb) return "a strip's byte count is less than its rows x 6 x ImageWidth";
            if (off + bc > file_bytes) return "a strip runs past the end of the file";
        }
        /* read_tiff's geometry, in its uint32 arithmetic (stripsize = bc[0] = 6 W here) */
        const uint32_t stripsize = (uint32_t)rb;
        uint32_t start = 0;
        if (stripsize > 960u * 6u) {
            start = (stripsize - 3840u * 6u) / 2u;
            if (start >= stripsize) start = 0; /* the reference's "bug fix" */
            if (cutout & H2Y_TIFF_CUTOUT_HD) start = (stripsize - 1920u * 6u) / 2u;
            if (cutout & H2Y_TIFF_CUTOUT_QHD) start = (stripsize - 960u * 6u) / 2u;
        }
        if (2ull * start >= stripsize) return "the cutout is wider than the picture (the reference's uint32 arithmetic wraps)";
        if (start % 6u) return "the horizontal crop starts inside a pixel (odd ImageWidth): the reference misaligns the channels";
        int strip_start = 0;
        if (cutout & H2Y_TIFF_CUTOUT_HD) strip_start = ((int)H - 1080) / 2;
        if (cutout & H2Y_TIFF_CUTOUT_QHD) strip_start = ((int)H - 540) / 2;
        if (strip_start < 0) return "the cutout is taller than the picture";
        ti.file_width = (int32_t)W;
        ti.file_height = (int32_t)H;
        ti.rows_per_strip = (int32_t)rps;
        ti.swap = r.mm;
        ti.x0 = (int32_t)(start / 6u);
        ti.y0 = strip_start;
        ti.width = (int32_t)((stripsize - start) / 6u - start / 6u);
        ti.height = (int32_t)H - 2 * strip_start;
        if (ti.width < 1 || ti.height < 1) return "the decoded picture is empty";
        if ((uint64_t)ti.width * (uint64_t)ti.height >= (1ull << 28)) return "the decoded picture has 2^28 pixels or more";
        ti.row_bytes = rb;
        ti.payload_bytes = (uint64_t)ti.height * rb;
        if (row_offsets && row_capacity < ti.height) return "row_capacity is less than the decoded height";
        ti.contiguous = 1;
        for (int32_t k = 0; k < ti.height; k++) {
            const uint32_t y = (uint32_t)(ti.y0 + k);
            const uint64_t off = (uint64_t)fso.get(r, y / rps) + (uint64_t)(y % rps) * rb;
            if (!k) ti.data_offset = off;
            else if (off != ti.data_offset + (uint64_t)k * rb) ti.contiguous = 0;
            if (row_offsets) row_offsets[k] = off;
        }
        return nullptr;
    };
    w = parse();
    if (why) *why = w ? w : "";
    if (w) return fail(nullptr, H2Y_EINVAL, "%s", w);
    *out = ti;
    return H2Y_OK;
}

int h2y_tiff_layout(int width, int height, uint8_t head[8], uint8_t *tail, size_t *tail_bytes)
{
    if (!head || !tail_bytes) return fail(nullptr, H2Y_EINVAL, "null argument");
    if (width < 1 || height < 1) return fail(nullptr, H2Y_EINVAL, "width and height must be >= 1");
    const uint64_t W = (uint64_t)width, H = (uint64_t)height, rb = 6 * W, ifd = 8 + rb * H;
    /* libtiff 4.3's choices for write_tiff's tags: sizes SHORT up to 65535; StripByteCounts LONG for one strip, else SHORT
     * while a row fits in 16 bits; StripOffsets LONG; arrays of more than 4 bytes out of line, after the IFD, in the order
     * BitsPerSample, StripByteCounts, StripOffsets */
    const int sbc_type = H == 1 || rb > 65535 ? 4 : 3;
    const uint64_t sbc_bytes = H * (sbc_type == 3 ? 2 : 4), so_bytes = 4 * H;
    const uint64_t bps_at = ifd + 2 + 10 * 12 + 4, sbc_at = bps_at + 6, so_at = sbc_at + (sbc_bytes > 4 ? sbc_bytes : 0);
    const uint64_t end = so_at + (so_bytes > 4 ? so_bytes : 0);
    if (end > 0xFFFFFFFFull) return fail(nullptr, H2Y_EINVAL, "a %dx%d TIFF needs 4 GiB or more (BigTIFF)", width, height);
    const size_t need = (size_t)(end - ifd);
    head[0] = head[1] = 'I';
    head[2] = 42;
    head[3] = 0;
    for (int k = 0; k < 4; k++) head[4 + k] = (uint8_t)(ifd >> (8 * k));
    if (!tail) {
        *tail_bytes = need;
        return H2Y_OK;
    }
    if (*tail_bytes < need) return fail(nullptr, H2Y_EINVAL, "tail needs %zu bytes, has %zu", need, *tail_bytes);
    *tail_bytes = need;
    memset(tail, 0, need);
    auto put = [&](uint64_t at, uint64_t v, int bytes) {
        for (int k = 0; k < bytes; k++) tail[at - ifd + k] = (uint8_t)(v >> (8 * k));
    };
    put(ifd, 10, 2);
    uint64_t e = ifd + 2;
    auto entry = [&](int tag, int type, uint64_t count, uint64_t value_or_offset) {
        put(e, tag, 2);
        put(e + 2, type, 2);
        put(e + 4, count, 4);
        put(e + 8, value_or_offset, type == 3 && count == 1 ? 2 : 4);
        e += 12;
    };
    entry(256, W > 65535 ? 4 : 3, 1, W);
    entry(257, H > 65535 ? 4 : 3, 1, H);
    entry(258, 3, 3, bps_at);
    entry(259, 3, 1, 1);
    entry(262, 3, 1, 2);
    entry(273, 4, H, H == 1 ? 8 : so_at);
    entry(277, 3, 1, 3);
    entry(278, 3, 1, 1);
    if (sbc_bytes <= 4) { /* one LONG, or two SHORTs, inline */
        put(e, 279, 2);
        put(e + 2, sbc_type, 2);
        put(e + 4, H, 4);
        for (uint64_t k = 0; k < H; k++) put(e + 8 + k * (sbc_type == 3 ? 2 : 4), rb, sbc_type == 3 ? 2 : 4);
        e += 12;
    } else entry(279, sbc_type, H, sbc_at);
    entry(284, 3, 1, 1);
    put(e, 0, 4); /* no next IFD */
    for (int k = 0; k < 3; k++) put(bps_at + 2 * k, 16, 2);
    if (sbc_bytes > 4)
        for (uint64_t k = 0; k < H; k++) put(sbc_at + k * (sbc_type == 3 ? 2 : 4), rb, sbc_type == 3 ? 2 : 4);
    if (so_bytes > 4)
        for (uint64_t k = 0; k < H; k++) put(so_at + 4 * k, 8 + k * rb, 4);
    return H2Y_OK;
}

/* what h2y_tiff_parse can return, and nothing else; and the decode's clamp_video_range */
static int tiff_info_check(h2y_ctx *ctx, const h2y_tiff_info *ti, int clamp)
{
    if (!ti) return fail(ctx, H2Y_EINVAL, "null h2y_tiff_info");
    if (ti->file_width < 1 || ti->file_width > (1 << 20) || ti->file_height < 1 || ti->file_height > (1 << 20))
        return fail(ctx, H2Y_EINVAL, "TIFF file_width and file_height must be 1..1048576");
    if (ti->width < 1 || ti->height < 1 || ti->x0 < 0 || ti->y0 < 0 || ti->x0 + ti->width > ti->file_width ||
        ti->y0 + ti->height > ti->file_height)
        return fail(ctx, H2Y_EINVAL, "TIFF decoded picture (x0, y0, width, height) lies outside the file's");
    if ((uint64_t)ti->width * (uint64_t)ti->height >= (1ull << 28)) return fail(ctx, H2Y_EINVAL, "TIFF decoded picture has 2^28 pixels or more");
    if (ti->swap != 0 && ti->swap != 1) return fail(ctx, H2Y_EINVAL, "TIFF swap must be 0 or 1");
    if (ti->row_bytes != 6ull * (uint64_t)ti->file_width) return fail(ctx, H2Y_EINVAL, "TIFF row_bytes is not 6 x file_width");
    if (ti->payload_bytes != (uint64_t)ti->height * ti->row_bytes) return fail(ctx, H2Y_EINVAL, "TIFF payload_bytes is not height x row_bytes");
    if (clamp != 0 && clamp != 1) return fail(ctx, H2Y_EINVAL, "clamp_video_range must be 0 or 1");
    return H2Y_OK;
}

/* decode_src's TIFF launch and variant: k_tiff_decode on n frames of a table */
static hipError_t tiff_decode(const h2y_ctx *ctx, const h2y_tiff_info &ti, bool clamp, const payload_frame *frames, int n)
{
    const tiff_geom g{(uint32_t)ti.width, (uint32_t)ti.height, (uint32_t)ti.x0, (uint32_t)ti.row_bytes};
    return h2y_launch_tiff_decode(ti.swap != 0, clamp, unit_grid(ctx, (uint64_t)h2y_tiff_chunks(g.width, g.height) * n), ctx->stream, g,
                                  frames, n);
}

static std::string tiff_variant(const h2y_tiff_info &ti, bool clamp)
{
    return std::string("k_tiff_decode<") + (ti.swap ? "SWAP" : "NOSWAP") + (clamp ? ",CLAMP>" : ",NOCLAMP>");
}

int h2y_tiff_decode_batch(h2y_ctx *ctx, const h2y_tiff_info *info, int clamp_video_range, int n_frames, const void *const *d_payload,
                          uint16_t *const *d_planes)
{
    return decode_batch(ctx, decode_src(info, clamp_video_range), H2Y_TIFF_FRAMES_PER_LAUNCH, n_frames, d_payload, d_planes);
}

static int rgb_size_check(h2y_ctx *ctx, int width, int height)
{
    if (width < 1 || height < 1 || (uint64_t)width * (uint64_t)height >= (1ull << 28)) return fail(ctx, H2Y_EINVAL, "bad picture size");
    return H2Y_OK;
}

int h2y_rgb_interleave_batch(h2y_ctx *ctx, int width, int height, int n_frames, const uint16_t *const *d_planes, uint16_t *const *d_rgb)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0) || ctx->streaming) return fail(ctx, H2Y_EINVAL, "a batch is pending or a stream is open");
    int rc = rgb_size_check(ctx, width, height);
    if (rc) return rc;
    if (n_frames < 1) return fail(ctx, H2Y_EINVAL, "n_frames must be >= 1");
    if (!d_planes || !d_rgb) return fail(ctx, H2Y_EINVAL, "null pointer arrays");
    for (int f = 0; f < n_frames; f++) {
        if (!d_rgb[f]) return fail(ctx, H2Y_EINVAL, "frame %d: output is null", f);
        if ((uintptr_t)d_rgb[f] & 1u) return fail(ctx, H2Y_EINVAL, "frame %d: output is not 2-byte aligned", f);
        for (int c = 0; c < 3; c++) {
            const uint16_t *p = d_planes[3 * f + c];
            if (!p) return fail(ctx, H2Y_EINVAL, "frame %d: plane %d is null", f, c);
            if ((uintptr_t)p & 1u) return fail(ctx, H2Y_EINVAL, "frame %d: plane %d is not 2-byte aligned", f, c);
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rgb_frame *h;
    rc = frame_table(ctx, n_frames, h);
    if (rc) return rc;
    for (int f = 0; f < n_frames; f++) {
        for (int c = 0; c < 3; c++) h[f].plane[c] = d_planes[3 * f + c];
        h[f].rgb = d_rgb[f];
    }
    const uint32_t npix = (uint32_t)width * (uint32_t)height;
    const uint64_t per_frame = h2y_rgb_chunks(npix);
    rc = timed_launches(ctx, h, n_frames, H2Y_TIFF_FRAMES_PER_LAUNCH, "k_rgb_interleave", [&](const rgb_frame *frames, int, int nf) {
        return h2y_launch_rgb_interleave(unit_grid(ctx, per_frame * nf), ctx->stream, npix, frames, nf);
    });
    if (rc) return rc;
    ctx->last_variant = "k_rgb_interleave";
    return H2Y_OK;
}

/* ---- scanline OpenEXR (read_exr(), exr.cpp:138-255) -------------------------------------------------------------------- */

namespace {

struct exr_reader { /* a little-endian file in memory */
    const unsigned char *p;
    size_t n;
    uint32_t u32(size_t at) const { return (uint32_t)p[at] | (uint32_t)p[at + 1] << 8 | (uint32_t)p[at + 2] << 16 | (uint32_t)p[at + 3] << 24; }
    int32_t i32(size_t at) const { return (int32_t)u32(at); }
    uint64_t u64(size_t at) const { return (uint64_t)u32(at) | (uint64_t)u32(at + 4) << 32; }
    /* the NUL-terminated string at `at`: its length, or -1 when it runs past the end */
    long str(size_t at) const
    {
        for (size_t k = at; k < n; k++)
            if (!p[k]) return (long)(k - at);
        return -1;
    }
};

struct exr_channel {
    std::string name;
    int32_t type;
    size_t size;
};

} // namespace

int h2y_exr_parse(const void *file, size_t file_bytes, h2y_exr_info *out, h2y_exr_chunk *chunks, int capacity, const char **why)
{
    h2y_exr_info xi{};
    const exr_reader r{static_cast<const unsigned char *>(file), file_bytes};
    auto parse = [&]() -> const char * {
        if (!file || !out) return "null argument";
        if (file_bytes < 8 || r.u32(0) != 20000630u) return "not an OpenEXR file: the magic number 20000630 is missing";
        const uint32_t version = r.u32(4);
        if (version & 0x200u) return "tiled OpenEXR files are not supported (scanline only)";
        if (version & 0x1000u) return "multi-part OpenEXR files are not supported (single part only)";
        if (version & 0x800u) return "deep OpenEXR files are not supported";
        if ((version & 0xFFu) != 2u) return "OpenEXR format version is not 2";
        if (version & ~0x4FFu) return "unknown OpenEXR version flags";
        /* the header: attributes name\0 type\0 int32 size, value; a NUL ends it */
        std::vector<exr_channel> ch;
        bool have_ch = false, have_comp = false, have_dw = false, have_lo = false;
        int32_t dw[4] = {0, 0, 0, 0};
        size_t at = 8;
        for (;;) {
            if (at >= file_bytes) return "truncated header";
            if (!r.p[at]) {
                at++;
                break;
            }
            const long nl = r.str(at);
            if (nl < 0) return "truncated header";
            const std::string name(reinterpret_cast<const char *>(r.p + at), (size_t)nl);
            at += (size_t)nl + 1;
            const long tl = at < file_bytes ? r.str(at) : -1;
            if (tl < 0) return "truncated header";
            const std::string type(reinterpret_cast<const char *>(r.p + at), (size_t)tl);
            at += (size_t)tl + 1;
            if (at + 4 > file_bytes) return "truncated header";
            const int32_t size = r.i32(at);
            at += 4;
            if (size < 0 || (uint64_t)at + (uint64_t)size > file_bytes) return "truncated header: an attribute runs past the end of the file";
            const size_t end = at + (size_t)size;
            if (name == "channels") {
                if (type != "chlist") return "the channels attribute is not a chlist";
                have_ch = true;
                size_t q = at;
                for (;;) { /* name\0 int32 pixel_type, uint8 pLinear, 3 reserved, int32 xSampling, int32 ySampling; a NUL ends it */
                    if (q >= end) return "truncated channel list";
                    if (!r.p[q]) break;
                    const long cl = r.str(q);
                    if (cl < 0 || q + (size_t)cl + 1 + 16 > end) return "truncated channel list";
                    exr_channel c{std::string(reinterpret_cast<const char *>(r.p + q), (size_t)cl), r.i32(q + (size_t)cl + 1), 0};
                    const int32_t xs = r.i32(q + (size_t)cl + 9), ys = r.i32(q + (size_t)cl + 13);
                    q += (size_t)cl + 17;
                    if (c.type < 0 || c.type > 2) return "a channel's pixel type is not UINT, HALF or FLOAT";
                    if (xs != 1 || ys != 1) return "a channel has x or y sampling other than 1 (subsampled channels are not supported)";
                    if (c.name == "Y" || c.name == "RY" || c.name == "BY")
                        return "luminance/chroma channels (Y, RY, BY) are not supported: RgbaInputFile would convert them through the "
                               "chromaticities";
                    c.size = c.type == H2Y_EXR_HALF ? 2 : 4;
                    ch.push_back(c);
                }
            } else if (name == "compression") {
                if (type != "compression" || size != 1) return "the compression attribute is malformed";
                have_comp = true;
                xi.compression = r.p[at];
            } else if (name == "dataWindow") {
                if (type != "box2i" || size != 16) return "the dataWindow attribute is malformed";
                have_dw = true;
                for (int k = 0; k < 4; k++) dw[k] = r.i32(at + 4 * (size_t)k);
            } else if (name == "lineOrder") {
                if (type != "lineOrder" || size != 1) return "the lineOrder attribute is malformed";
                have_lo = true;
                xi.line_order = r.p[at];
            }
            at = end;
        }
        if (!have_ch || !have_comp || !have_dw || !have_lo) return "a required attribute (channels, compression, dataWindow, lineOrder) is missing";
        static const char *const kCodec[] = {"NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB"};
        if (xi.compression > H2Y_EXR_ZIP) {
            static char msg[10][64];
            if (xi.compression > 9) return "unknown compression";
            snprintf(msg[xi.compression], sizeof msg[0], "%s compression is not supported (NONE, RLE, ZIPS, ZIP only)", kCodec[xi.compression]);
            return msg[xi.compression];
        }
        if (xi.line_order != 0 && xi.line_order != 1) return "lineOrder is neither INCREASING_Y nor DECREASING_Y";
        if (ch.empty()) return "the file has no channels";
        /* OpenEXR keeps the channel list in a map: a line holds the channels in the order of their names */
        std::sort(ch.begin(), ch.end(), [](const exr_channel &a, const exr_channel &b) { return a.name < b.name; });
        for (size_t k = 1; k < ch.size(); k++)
            if (ch[k].name == ch[k - 1].name) return "a channel name appears twice";
        const int64_t w = (int64_t)dw[2] - dw[0] + 1, h = (int64_t)dw[3] - dw[1] + 1;
        if (w < 1 || h < 1 || w > (1 << 20) || h > (1 << 20)) return "the data window's width or height is outside 1..1048576";
        if (w * h >= (1ll << 28)) return "the data window has 2^28 pixels or more";
        xi.width = (int32_t)w;
        xi.height = (int32_t)h;
        xi.x_min = dw[0];
        xi.y_min = dw[1];
        xi.lines_per_chunk = xi.compression == H2Y_EXR_ZIP ? 16 : 1;
        xi.n_chunks = (int32_t)((h + xi.lines_per_chunk - 1) / xi.lines_per_chunk);
        xi.n_channels = (int32_t)ch.size();
        xi.all_half = 1;
        for (int c = 0; c < 3; c++) xi.channel_type[c] = H2Y_EXR_MISSING, xi.channel_offset[c] = -1;
        uint64_t lb = 0;
        for (const exr_channel &c : ch) {
            const int plane = c.name == "G" ? 0 : c.name == "B" ? 1 : c.name == "R" ? 2 : -1; /* "A" and the rest: skipped */
            if (plane >= 0) xi.channel_type[plane] = c.type, xi.channel_offset[plane] = (int32_t)lb;
            if (c.type != H2Y_EXR_HALF) xi.all_half = 0;
            lb += (uint64_t)w * c.size;
            if (lb * (uint64_t)xi.lines_per_chunk >= (1ull << 31)) return "a chunk would hold 2 GiB or more";
        }
        xi.line_bytes = (int32_t)lb;
        xi.flags_bytes = ((uint64_t)xi.n_chunks + 255) & ~(uint64_t)255;
        xi.payload_bytes = xi.flags_bytes + (uint64_t)h * lb;
        if (chunks && capacity < xi.n_chunks) return "capacity is less than the number of chunks";
        /* the offset table: n_chunks uint64, indexed by increasing y whatever the line order */
        if ((uint64_t)at + 8ull * (uint64_t)xi.n_chunks > file_bytes) return "truncated offset table";
        const uint64_t table_end = (uint64_t)at + 8ull * (uint64_t)xi.n_chunks;
        for (int32_t k = 0; k < xi.n_chunks; k++) {
            const uint64_t off = r.u64(at + 8 * (size_t)k);
            if (off < table_end || off + 8 > file_bytes)
                return "broken offset table: an entry points outside the chunk area (OpenEXR would rebuild the table by scanning; "
                       "refused here)";
            const int32_t row = k * xi.lines_per_chunk;
            if ((int64_t)r.i32((size_t)off) != (int64_t)xi.y_min + row) return "broken offset table: a chunk's y is not that of its table slot";
            const int32_t size = r.i32((size_t)off + 4);
            const uint64_t lines = (uint64_t)(xi.height - row < xi.lines_per_chunk ? xi.height - row : xi.lines_per_chunk);
            if (size < 1 || off + 8 + (uint64_t)size > file_bytes) return "a chunk runs past the end of the file";
            if ((uint64_t)size > lines * lb) return "a chunk's packed size exceeds its uncompressed size (corrupt file)";
            if (xi.compression == H2Y_EXR_NONE && (uint64_t)size != lines * lb) return "an uncompressed chunk's size is not its lines' bytes";
            if (chunks) chunks[k] = h2y_exr_chunk{off, (uint32_t)size, row};
        }
        return nullptr;
    };
    const char *w = parse();
    if (why) *why = w ? w : "";
    if (w) return fail(nullptr, H2Y_EINVAL, "%s", w);
    *out = xi;
    return H2Y_OK;
}

/* what h2y_exr_parse can return, and nothing else */
static const char *exr_info_check(const h2y_exr_info *xi)
{
    if (!xi) return "null h2y_exr_info";
    if (xi->width < 1 || xi->width > (1 << 20) || xi->height < 1 || xi->height > (1 << 20) ||
        (uint64_t)xi->width * (uint64_t)xi->height >= (1ull << 28))
        return "EXR width and height must be 1..1048576, below 2^28 pixels";
    if (xi->compression < H2Y_EXR_NONE || xi->compression > H2Y_EXR_ZIP) return "EXR compression must be NONE, RLE, ZIPS or ZIP";
    if (xi->lines_per_chunk != (xi->compression == H2Y_EXR_ZIP ? 16 : 1)) return "EXR lines_per_chunk does not match the compression";
    if (xi->n_chunks != (xi->height + xi->lines_per_chunk - 1) / xi->lines_per_chunk) return "EXR n_chunks is not ceil(height / lines_per_chunk)";
    if (xi->n_channels < 1 || xi->line_bytes < 2 * xi->width || xi->line_bytes % 2 ||
        (uint64_t)xi->line_bytes * (uint64_t)xi->lines_per_chunk >= (1ull << 31))
        return "EXR line_bytes is out of range";
    bool half_only = true;
    for (int c = 0; c < 3; c++) {
        const int t = xi->channel_type[c];
        if (t == H2Y_EXR_MISSING) {
            if (xi->channel_offset[c] != -1) return "EXR channel_offset of a missing channel must be -1";
            continue;
        }
        if (t < H2Y_EXR_UINT || t > H2Y_EXR_FLOAT) return "EXR channel_type must be UINT, HALF, FLOAT or MISSING";
        const int64_t size = t == H2Y_EXR_HALF ? 2 : 4;
        if (t != H2Y_EXR_HALF) half_only = false;
        if (xi->channel_offset[c] < 0 || xi->channel_offset[c] + size * xi->width > xi->line_bytes || xi->channel_offset[c] % 2)
            return "EXR channel_offset lies outside the line";
        if (xi->all_half && xi->channel_offset[c] % (2 * xi->width)) return "EXR channel_offset of an all-half file is not a channel's";
    }
    if (xi->all_half != 0 && xi->all_half != 1) return "EXR all_half must be 0 or 1";
    if (xi->all_half && (!half_only || xi->line_bytes != 2 * xi->width * xi->n_channels)) return "EXR all_half does not match the channels";
    if (xi->flags_bytes != (((uint64_t)xi->n_chunks + 255) & ~(uint64_t)255)) return "EXR flags_bytes is not n_chunks rounded up to 256";
    if (xi->payload_bytes != xi->flags_bytes + (uint64_t)xi->height * (uint64_t)xi->line_bytes)
        return "EXR payload_bytes is not flags_bytes + height x line_bytes";
    return nullptr;
}

/* OpenEXR's rleUncompress: a count byte c < 0 copies the next -c bytes, c >= 0 repeats the next byte c + 1 times.  Whether
 * it filled `out` exactly. */
static bool exr_rle_expand(const unsigned char *in, size_t in_bytes, unsigned char *out, size_t out_bytes)
{
    size_t i = 0, o = 0;
    while (i < in_bytes) {
        const int c = (signed char)in[i++];
        if (c < 0) {
            const size_t k = (size_t)-c;
            if (i + k > in_bytes || o + k > out_bytes) return false;
            memcpy(out + o, in + i, k);
            i += k;
            o += k;
        } else {
            const size_t k = (size_t)c + 1;
            if (i >= in_bytes || o + k > out_bytes) return false;
            memset(out + o, in[i++], k);
            o += k;
        }
    }
    return o == out_bytes;
}

int h2y_exr_unpack(const h2y_exr_info *info, const h2y_exr_chunk *chunks, const void *file, int first_chunk, int n_chunks,
                   void *payload, const char **why)
{
    const char *w = exr_info_check(info);
    if (!w && (!chunks || !file || !payload)) w = "null argument";
    if (!w && (first_chunk < 0 || n_chunks < 0 || first_chunk > info->n_chunks - n_chunks)) w = "chunk range outside the file's chunks";
    static thread_local char msg[160];
    if (!w) {
        unsigned char *pay = static_cast<unsigned char *>(payload);
        const unsigned char *src = static_cast<const unsigned char *>(file);
        const uint64_t lb = (uint64_t)info->line_bytes;
        if (first_chunk == 0) memset(pay + info->n_chunks, 0, (size_t)(info->flags_bytes - (uint64_t)info->n_chunks));
        for (int c = first_chunk; c < first_chunk + n_chunks && !w; c++) {
            const h2y_exr_chunk &k = chunks[c];
            if (k.row != c * info->lines_per_chunk) {
                w = "a chunk record's row is not that of its slot";
                break;
            }
            const uint64_t lines = (uint64_t)(info->height - k.row < info->lines_per_chunk ? info->height - k.row : info->lines_per_chunk);
            const size_t raw = (size_t)(lines * lb);
            unsigned char *dst = pay + info->flags_bytes + (uint64_t)k.row * lb;
            const unsigned char *in = src + k.offset + 8;
            if (k.packed_bytes > raw || (info->compression == H2Y_EXR_NONE && k.packed_bytes != raw)) {
                w = "a chunk's packed size exceeds its uncompressed size (corrupt file)";
                break;
            }
            if (k.packed_bytes == raw) { /* NONE, or stored raw because compression did not help */
                memcpy(dst, in, raw);
                pay[c] = H2Y_EXR_CHUNK_RAW;
                continue;
            }
            if (info->compression == H2Y_EXR_RLE) {
                if (!exr_rle_expand(in, k.packed_bytes, dst, raw)) {
                    snprintf(msg, sizeof msg, "chunk %d (y %d): RLE data does not expand to its %zu bytes", c, info->y_min + k.row, raw);
                    w = msg;
                }
            } else {
                uLongf got = (uLongf)raw;
                const int zr = uncompress(dst, &got, in, (uLong)k.packed_bytes);
                if (zr != Z_OK || got != raw) {
                    snprintf(msg, sizeof msg, "chunk %d (y %d): zlib data does not inflate to its %zu bytes (zlib %d, %lu bytes)", c,
                             info->y_min + k.row, raw, zr, (unsigned long)got);
                    w = msg;
                }
            }
            pay[c] = H2Y_EXR_CHUNK_ENCODED;
        }
    }
    if (why) *why = w ? w : "";
    if (w) return fail(nullptr, H2Y_EINVAL, "%s", w);
    return H2Y_OK;
}

static exr_geom exr_geom_of(const h2y_exr_info &xi)
{
    exr_geom g{};
    g.width = (uint32_t)xi.width;
    g.height = (uint32_t)xi.height;
    g.lines_per_chunk = (uint32_t)xi.lines_per_chunk;
    g.n_chunks = (uint32_t)xi.n_chunks;
    g.n_channels = (uint32_t)xi.n_channels;
    g.line_bytes = (uint32_t)xi.line_bytes;
    g.flags_bytes = (uint32_t)xi.flags_bytes;
    g.all_half = (uint32_t)xi.all_half;
    for (int c = 0; c < 3; c++) g.type[c] = xi.channel_type[c], g.offset[c] = xi.channel_offset[c];
    return g;
}

/* decode_src's EXR launch and variant: k_exr_decode on n frames of a table */
static hipError_t exr_decode(const h2y_ctx *ctx, const h2y_exr_info &xi, const payload_frame *frames, int n)
{
    return h2y_launch_exr_decode(unit_grid(ctx, (uint64_t)xi.n_chunks * n), ctx->stream, exr_geom_of(xi), frames, n);
}

static std::string exr_variant(const h2y_exr_info &xi)
{
    static const char *const kComp[] = {"NONE", "RLE", "ZIPS", "ZIP"};
    return std::string("k_exr_decode<") + kComp[xi.compression] + (xi.all_half ? ",ALL_HALF>" : ",GENERAL>");
}

int h2y_exr_decode_batch(h2y_ctx *ctx, const h2y_exr_info *info, int n_frames, const void *const *d_payload, uint16_t *const *d_planes)
{
    return decode_batch(ctx, decode_src(info), H2Y_EXR_FRAMES_PER_LAUNCH, n_frames, d_payload, d_planes);
}

/* ---- decode_src: each format's facts, for the decode batches and the forward rings ------------------------------------- */

int decode_src::check(h2y_ctx *ctx) const
{
    switch (kind) {
    case DPX: return dpx_info_check(ctx, has_info ? &dpx : nullptr);
    case TIFF: return tiff_info_check(ctx, has_info ? &tiff : nullptr, clamp);
    case EXR:
        if (const char *w = exr_info_check(has_info ? &exr : nullptr)) return fail(ctx, H2Y_EINVAL, "%s", w);
        return H2Y_OK;
    default: return H2Y_OK;
    }
}

int decode_src::planes_check(h2y_ctx *ctx, const h2y_desc *d) const
{
    const char *what;
    int w, h;
    switch (kind) {
    case DPX:
        if (d->in_sample_type != H2Y_SAMPLE_F32) return fail(ctx, H2Y_EINVAL, "a DPX stream decodes to F32 planes: in_sample_type must be H2Y_SAMPLE_F32");
        what = "DPX picture", w = dpx.width, h = dpx.height;
        break;
    case TIFF:
        if (d->in_sample_type != H2Y_SAMPLE_U16 || d->src_bit_depth != 16)
            return fail(ctx, H2Y_EINVAL, "a TIFF stream decodes to 16-bit planes: in_sample_type must be H2Y_SAMPLE_U16, src_bit_depth 16");
        what = "TIFF picture", w = tiff.width, h = tiff.height;
        break;
    case EXR:
        if (d->in_sample_type != H2Y_SAMPLE_F16) return fail(ctx, H2Y_EINVAL, "an EXR stream decodes to half planes: in_sample_type must be H2Y_SAMPLE_F16");
        what = "EXR data window", w = exr.width, h = exr.height;
        break;
    default: return H2Y_OK;
    }
    if (d->width != w || d->height != h)
        return fail(ctx, H2Y_EINVAL, "%s is %dx%d, the descriptor %dx%d (resizing is not part of convert())", what, w, h, d->width, d->height);
    return H2Y_OK;
}

uint64_t decode_src::payload_bytes() const
{
    return kind == DPX ? dpx.payload_bytes : kind == TIFF ? tiff.payload_bytes : kind == EXR ? exr.payload_bytes : 0;
}

uintptr_t decode_src::align() const { return kind == DPX ? 4 : 2; } /* DPX: 32-bit words and float planes; u16 / half elsewhere */

hipError_t decode_src::launch(const h2y_ctx *ctx, const payload_frame *frames, int n) const
{
    switch (kind) {
    case DPX: return dpx_decode(ctx, dpx, frames, n);
    case TIFF: return tiff_decode(ctx, tiff, clamp != 0, frames, n);
    case EXR: return exr_decode(ctx, exr, frames, n);
    default: return hipErrorInvalidValue;
    }
}

const char *decode_src::kernel() const { return kind == DPX ? "k_dpx_decode" : kind == TIFF ? "k_tiff_decode" : kind == EXR ? "k_exr_decode" : ""; }

std::string decode_src::variant() const
{
    return kind == DPX ? dpx_variant(dpx) : kind == TIFF ? tiff_variant(tiff, clamp != 0) : kind == EXR ? exr_variant(exr) : std::string();
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
    const geom g = make_geom(d, h2y_fused_threads(var));
    frame_io io;
    for (int c = 0; c < 3; c++) io.in[c] = d_in[c];
    io.out = d_out444[0];
    io.tmp_cb = d_out444[1];
    io.tmp_cr = d_out444[2];
    ctx->b->h_frames[0] = io;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->b->d_frames, ctx->b->h_frames, sizeof(frame_io), hipMemcpyHostToDevice, ctx->stream));
    ctx->b->dev_frames.clear(); /* run_frames()'s record of what d_frames holds */
    const int grid = grid_for(ctx, var, g.chunks);
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
    else {
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
        HIP_TRY(ctx, h2y_launch_fir420(ctx->stream, fr));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return H2Y_OK;
}

const char *h2y_last_kernel_name(const h2y_ctx *ctx) { return ctx ? ctx->last_name : ""; }
const char *h2y_last_kernel_variant(const h2y_ctx *ctx) { return ctx ? ctx->last_variant.c_str() : ""; }

int h2y_last_kernel_ms(const h2y_ctx *ctx, float *ms, int *launches)
{
    if (!ctx) return H2Y_EINVAL;
    if (ms) *ms = ctx->last_ms;
    if (launches) *launches = ctx->last_launches;
    return H2Y_OK;
}
