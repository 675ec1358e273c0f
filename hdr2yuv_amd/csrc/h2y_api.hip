/*
 * h2y_api.hip -- the C-ABI shim declared in include/hdr2yuv_hip.h: the context and its options, the descriptor check, the
 * inverse and decode batch entries and the file parsers.  The forward conversion (its batches, the single-frame and single-step
 * entries) lies in h2y_forward.hip, the streaming ring in h2y_ring.hip, the measurements (comparison, SSIM, content light,
 * histograms, scaling) in h2y_measure.hip; h2y_shim.h is what the four share.
 *
 * Host side of the drop-in boundary: descriptor validation, device buffer ownership, and kernel launches.  No pixel is ever
 * computed on the host: without a HIP device h2y_ctx_create() fails and nothing else works.
 */
#include "h2y_shim.h"

#include <zlib.h>

static thread_local std::string g_err;

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
 *   "lut3d_lds" "0" | "1"               a 3D LUT of up to 17 nodes per axis is read from LDS, k_lut3d_lds (default on); same bytes either way
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
    else if (!strcmp(name, "lut3d_lds")) ctx->opt_lut3d_lds = value[0] != '0';
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
    delete ctx; /* and with it the measurements' workspaces (dev_buf) */
}

int h2y_ctx_set_stream(h2y_ctx *ctx, void *hip_stream)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0)) return fail(ctx, H2Y_EINVAL, "a batch is pending: call h2y_batch_finish first");
    if (ctx->streaming) return fail(ctx, H2Y_EINVAL, "a stream is open: close it first");
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
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
                             int out_bit_depth, int form)
{
    a.up.src0 = a.up.src1 = nullptr;
    a.up.dst0 = a.up.dst1 = nullptr;
    a.up.width = width; a.up.height = height;
    a.up.algorithm = form;
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
    if (const int rc = batch_enter(ctx)) return rc;
    if (const int rc = picture_size_check(ctx, width, height)) return rc;
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

static int upsample_444(h2y_ctx *ctx, int width, int height, int algorithm /* UP_* */, unsigned min_cv, unsigned max_cv,
                        const uint16_t *d_src, uint16_t *d_dst)
{
    if (const int rc = batch_enter(ctx)) return rc;
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

int h2y_upsample_444(h2y_ctx *ctx, int width, int height, int algorithm, unsigned min_cv, unsigned max_cv, const uint16_t *d_src,
                     uint16_t *d_dst)
{
    return upsample_444(ctx, width, height, algorithm ? UP_FIR : UP_REPLICATE, min_cv, max_cv, d_src, d_dst);
}

int h2y_upsample_444_sited(h2y_ctx *ctx, int width, int height, int chroma_sample_loc_type, unsigned min_cv, unsigned max_cv,
                           const uint16_t *d_src, uint16_t *d_dst)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if (chroma_sample_loc_type != 0 && chroma_sample_loc_type != 2)
        return fail(ctx, H2Y_EINVAL, "chroma_sample_loc_type %d: want 0 (the reference's upsampler) or 2 (top-left)", chroma_sample_loc_type);
    return upsample_444(ctx, width, height, chroma_sample_loc_type == 2 ? UP_FIR_TL : UP_FIR, min_cv, max_cv, d_src, d_dst);
}

int h2y_ctx_set_inverse_chroma_siting(h2y_ctx *ctx, int chroma_sample_loc_type)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0) || ctx->streaming)
        return fail(ctx, H2Y_EINVAL, "a batch is pending or a stream is open: set the inverse chroma siting before");
    if (chroma_sample_loc_type != 0 && chroma_sample_loc_type != 2)
        return fail(ctx, H2Y_EINVAL, "chroma_sample_loc_type %d: want 0 (as the reference's upsampler sites it) or 2 (top-left)", chroma_sample_loc_type);
    ctx->opt_inv_siting = chroma_sample_loc_type;
    return H2Y_OK;
}

/* What `algorithm` means on this context: replication, the reference's FIR pair, or under inverse chroma siting 2 the top-left
 * form.  4:4:4 input has nothing to upsample; replication is centre sited by construction and is refused under siting 2. */
int inverse_form(h2y_ctx *ctx, int chroma, int algorithm, int *form)
{
    *form = algorithm ? UP_FIR : UP_REPLICATE;
    if (ctx->opt_inv_siting != 2 || chroma != H2Y_CHROMA_420) return H2Y_OK;
    if (!algorithm)
        return fail(ctx, H2Y_EUNSUPPORTED, "inverse chroma siting 2 (top-left) with algorithm 0: replication is centre sited by construction");
    *form = UP_FIR_TL;
    return H2Y_OK;
}

int h2y_inverse_420(h2y_ctx *ctx, int width, int height, int in_bit_depth, int in_full_range, int in_matrix_coeffs, int out_bit_depth,
                    int algorithm, const uint16_t *const d_in[3], uint16_t *const d_out[3])
{
    if (const int rc = batch_enter(ctx)) return rc;
    if (width < 2 || height < 2 || (width & 3) || (height & 1) || width > 32766 || height > 32766)
        return fail(ctx, H2Y_EINVAL, "4:2:0 inverse: width a multiple of 4 and height even, up to 32766"); /* the upsampled planes feed 8-byte loads */
    if (in_bit_depth < 8 || in_bit_depth > 16) return fail(ctx, H2Y_EINVAL, "bit depths must be 8..16");
    if (!d_in || !d_in[0] || !d_in[1] || !d_in[2]) return fail(ctx, H2Y_EINVAL, "null pointer arrays");
    if (out_bit_depth < 8 || out_bit_depth > 16) return fail(ctx, H2Y_EINVAL, "bit depths must be 8..16");
    if (in_matrix_coeffs == H2Y_MATRIX_GBR) return fail(ctx, H2Y_EUNSUPPORTED, "matrix_coeffs 0 (GBR) has no inverse in the reference (it exits)");
    if (!d_out || !d_out[0] || !d_out[1] || !d_out[2]) return fail(ctx, H2Y_EINVAL, "null pointer arrays");
    for (int c = 0; c < 3; c++)
        if (((uintptr_t)d_in[c] & 3) || ((uintptr_t)d_out[c] & 3)) return fail(ctx, H2Y_EINVAL, "plane %d is not 4-byte aligned", c);
    int form;
    const int frc = inverse_form(ctx, H2Y_CHROMA_420, algorithm, &form);
    if (frc) return frc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    /* one pass: both chroma planes upsampled inside the blocks (yuv2tiff.cpp:92-93,142-154: minCV 0, maxCV 2^depth - 1), then
     * matrix_inverse's pixel; the 4:4:4 chroma never reaches memory (k_inverse420, h2y_resample.hip) */
    inv420_args a;
    inverse420_setup(a, width, height, in_bit_depth, in_full_range, in_matrix_coeffs, out_bit_depth, form);
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
    ctx->last_variant = form == UP_FIR_TL ? "k_inverse420<FIR_TL>" : form == UP_FIR ? "k_inverse420<FIR>" : "k_inverse420<REPLICATE>";
    return H2Y_OK;
}

int h2y_inverse_frame(h2y_ctx *ctx, int width, int height, int in_chroma_format_idc, int in_bit_depth, int in_full_range,
                      int in_matrix_coeffs, int out_bit_depth, int algorithm, const uint16_t *const in_planes[3], uint16_t *const out_planes[3])
{
    if (const int rc = batch_enter(ctx)) return rc;
    if (in_chroma_format_idc != H2Y_CHROMA_444 && in_chroma_format_idc != H2Y_CHROMA_420)
        return fail(ctx, H2Y_EUNSUPPORTED, "inverse flow: input chroma_format_idc must be 3 (4:4:4) or 1 (4:2:0)");
    if (const int rc = picture_size_check(ctx, width, height)) return rc;
    if (!in_planes || !out_planes) return fail(ctx, H2Y_EINVAL, "null pointer arrays");
    for (int c = 0; c < 3; c++)
        if (!in_planes[c] || !out_planes[c]) return fail(ctx, H2Y_EINVAL, "plane %d is null", c);
    int form;
    const int frc = inverse_form(ctx, in_chroma_format_idc, algorithm, &form); /* the refusal, before anything is copied or launched */
    if (frc) return frc;
    (void)form; /* h2y_inverse_420 below takes it again */
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
    } else if (const int rc = picture_size_check(ctx, p.width, p.height))
        return rc;
    if (p.in_depth < 8 || p.in_depth > 16 || p.out_depth < 8 || p.out_depth > 16) return fail(ctx, H2Y_EINVAL, "bit depths must be 8..16");
    if (p.matrix == H2Y_MATRIX_GBR) return fail(ctx, H2Y_EUNSUPPORTED, "matrix_coeffs 0 (GBR) has no inverse in the reference (it exits)");
    return H2Y_OK;
}

/* h2y_dpx_decode_batch, h2y_tiff_decode_batch, h2y_exr_decode_batch: src's decode of n_frames payloads into their planes */
template <typename P>
static int decode_batch(h2y_ctx *ctx, const decode_src &src, int per_launch, int n_frames, const void *const *d_payload, P *const *d_planes)
{
    if (const int rc = batch_enter(ctx)) return rc;
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
    if (const int rc = batch_enter(ctx)) return rc;
    const inv_params p{width, height, in_chroma_format_idc, in_bit_depth, in_full_range, in_matrix_coeffs, out_bit_depth, algorithm};
    int rc = inverse_check(ctx, p);
    if (rc) return rc;
    int form;
    rc = inverse_form(ctx, in_chroma_format_idc, algorithm, &form);
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
    inverse420_setup(a, width, height, in_bit_depth, in_full_range, in_matrix_coeffs, out_bit_depth, form);
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
    ctx->last_variant = !sub ? "k_inverse_batch"
                        : form == UP_FIR_TL ? "k_inverse420_batch<FIR_TL>" : form == UP_FIR ? "k_inverse420_batch<FIR>" : "k_inverse420_batch<REPLICATE>";
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

int h2y_rgb_interleave_batch(h2y_ctx *ctx, int width, int height, int n_frames, const uint16_t *const *d_planes, uint16_t *const *d_rgb)
{
    int rc = batch_enter(ctx);
    if (!rc) rc = picture_size_check(ctx, width, height);
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
    case PQCODE: /* the linearised planes: F32 LINEAR G,B,R in [+0, 1], floor 0 and ceiling 1 whatever the frame holds (signal: G', B', R' for
                    the ring's signal-mode LUT, under the same descriptor) */
        if (d->in_sample_type != H2Y_SAMPLE_F32 || d->src_transfer != 8 || d->src_matrix != H2Y_MATRIX_GBR)
            return fail(ctx, H2Y_EINVAL, "%s code stream linearises to F32 G,B,R planes: in_sample_type H2Y_SAMPLE_F32, src_transfer 8, src_matrix 0",
                        hlg ? "an HLG" : sdr ? "an SDR" : signal ? "a signal" : "a PQ");
        if (d->stats_override != 1) return fail(ctx, H2Y_EINVAL, "%s code stream needs stats_override 1 with floor 0 and ceiling 1", hlg ? "an HLG" : sdr ? "an SDR" : signal ? "a signal" : "a PQ");
        for (int c = 0; c < 3; c++)
            if (d->floor[c] != 0 || d->ceiling[c] != 1)
                return fail(ctx, H2Y_EINVAL, "%s code stream needs stats_override 1 with floor 0 and ceiling 1", hlg ? "an HLG" : sdr ? "an SDR" : signal ? "a signal" : "a PQ");
        what = hlg ? "HLG code frame" : sdr ? "SDR code frame" : signal ? "signal code frame" : "PQ code frame", w = code.width, h = code.height;
        break;
    default: return H2Y_OK;
    }
    if (d->width != w || d->height != h)
        return fail(ctx, H2Y_EINVAL, "%s is %dx%d, the descriptor %dx%d (resizing is not part of convert())", what, w, h, d->width, d->height);
    return H2Y_OK;
}

uint64_t decode_src::payload_bytes() const
{
    if (kind == PQCODE) return (uint64_t)code.samples * sizeof(uint16_t);
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

const char *h2y_last_kernel_name(const h2y_ctx *ctx) { return ctx ? ctx->last_name : ""; }
const char *h2y_last_kernel_variant(const h2y_ctx *ctx) { return ctx ? ctx->last_variant.c_str() : ""; }

int h2y_last_kernel_ms(const h2y_ctx *ctx, float *ms, int *launches)
{
    if (!ctx) return H2Y_EINVAL;
    if (ms) *ms = ctx->last_ms;
    if (launches) *launches = ctx->last_launches;
    return H2Y_OK;
}
