/*
 * h2y_ring.hip -- the streaming ring of the C-ABI shim (h2y_stream_*): slot allocation and release, the forward and inverse
 * openers and the decoding openers that call them, and the one path a frame takes through an open ring.  What arming adds to a
 * ring (ring_stage, h2y_shim.h) lies with its measurement in h2y_measure.hip.
 */
#include "h2y_shim.h"

/* ---- streaming pipeline ------------------------------------------------------
 * H2D of frame k+1, conversion of frame k and D2H of frame k-1 overlap: three streams, a ring of
 * pinned host slots the caller fills and drains in place.  Every frame is converted in the
 * reference's order (pic_stats pre-pass on the device, then the pixel kernel with its result in
 * device memory): no speculation, nothing to redo, no host round trip between the stages. */
void stream_free(h2y_ctx *ctx)
{
    for (auto &st : ctx->s_stage) st.reset();
    for (auto &s : ctx->ss) {
        if (s.h_in) (void)hipHostFree(s.h_in);
        if (s.h_out) (void)hipHostFree(s.h_out);
        if (s.d_in) (void)hipFree(s.d_in);
        if (s.d_out) (void)hipFree(s.d_out);
        if (s.ev_h2d) (void)hipEventDestroy(s.ev_h2d);
        if (s.ev_conv) (void)hipEventDestroy(s.ev_conv);
        if (s.ev_done) (void)hipEventDestroy(s.ev_done);
    }
    ctx->ss.clear();
    if (ctx->s_h2d) (void)hipStreamDestroy(ctx->s_h2d);
    if (ctx->s_d2h) (void)hipStreamDestroy(ctx->s_d2h);
    ctx->s_h2d = ctx->s_d2h = nullptr;
    if (ctx->s_tab) (void)hipFree(ctx->s_tab);
    ctx->s_tab = nullptr;
    ctx->streaming = false;
    ctx->s_kind = h2y_ctx::RING_FORWARD;
    ctx->s_src = decode_src();
    ctx->s_interleave = false;
    ctx->s_started = false;
    ctx->s_frame = ring_frame();
    ctx->s_down = true;
    ctx->s_head = ctx->s_tail = 0;
    ctx->s_lent = -1;
}

/* every opener's first checks */
int ring_may_open(h2y_ctx *ctx)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if ((ctx->q_count > 0) || ctx->streaming) return fail(ctx, H2Y_EINVAL, "a batch is pending or a stream is already open");
    return H2Y_OK;
}

/* the ring's streams and `depth` slots: pinned input / output and their device twins */
static int stream_alloc(h2y_ctx *ctx, int depth, size_t h_in_bytes, size_t d_in_bytes, size_t h_out_bytes, size_t d_out_bytes)
{
    ctx->ss.assign(depth, h2y_ctx::stream_slot());
    ctx->streaming = true;
    hipError_t e = hipStreamCreateWithFlags(&ctx->s_h2d, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->s_d2h, hipStreamNonBlocking);
    for (auto &s : ctx->ss) {
        if (e == hipSuccess) e = hipHostMalloc((void **)&s.h_in, h_in_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void **)&s.h_out, h_out_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc((void **)&s.d_in, d_in_bytes);
        if (e == hipSuccess) e = hipMalloc((void **)&s.d_out, d_out_bytes);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev_h2d, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev_conv, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming);
        s.result = s.h_out;
    }
    if (e != hipSuccess) {
        stream_free(ctx);
        return fail(ctx, H2Y_ENOMEM, "stream buffers: %s", hipGetErrorString(e));
    }
    return H2Y_OK;
}

/* The end of every arm entry: st, with all it allocated, joins the open ring as its stage `id`; if an allocation or copy of
 * its arming failed it is released instead, and the ring stays open, armed with whatever it was armed with before */
int stage_arm(h2y_ctx *ctx, int id, std::unique_ptr<ring_stage> st, const char *what)
{
    if (st->err != hipSuccess) return fail(ctx, H2Y_ENOMEM, "%s buffers: %s", what, hipGetErrorString(st->err));
    ctx->s_stage[id] = std::move(st);
    return H2Y_OK;
}

/* What a stage or an opener decides when arming: the produced frame stays on the device, and h2y_stream_output hands out
 * nothing (until a stage sets its own frame as the slots' result) */
void ring_frame_stays(h2y_ctx *ctx)
{
    ctx->s_down = false;
    for (auto &s : ctx->ss) s.result = nullptr;
}

/* the open ring's s_tab: the decode's or the interleave's entry of every slot, uploaded once (the ring closes if it fails) */
template <typename T> static int slot_table(h2y_ctx *ctx, const std::vector<T> &tab, const char *what)
{
    const size_t tb = tab.size() * sizeof(T);
    hipError_t e = hipMalloc(&ctx->s_tab, tb);
    if (e != hipSuccess) {
        stream_free(ctx);
        return fail(ctx, H2Y_ENOMEM, "hipMalloc(%zu): %s", tb, hipGetErrorString(e));
    }
    e = hipMemcpy(ctx->s_tab, tab.data(), tb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        stream_free(ctx);
        return fail(ctx, H2Y_EHIP, "hipMemcpy of the %s slot table: %s", what, hipGetErrorString(e));
    }
    return H2Y_OK;
}

/* The forward ring (h2y_stream_open and the decoding openers).  Without a decode (src null) a slot holds the three planes, each
 * 256-byte aligned, on the host and on the device.  With one the pinned slot holds the payload, its device twin the three planes
 * the decode writes and then the payload; each slot's decode table entry is uploaded here once.  The stages see the .yuv frame
 * in the slot's device output. */
static int open_forward_ring(h2y_ctx *ctx, const h2y_desc *d, const decode_src *src, int depth)
{
    int rc = ring_may_open(ctx);
    if (rc) return rc;
    const decode_src &dec = src ? *src : decode_src();
    rc = dec.check(ctx);
    if (rc) return rc;
    const char *why;
    rc = h2y_desc_check(d, &why);
    if (rc) return fail(ctx, rc, "descriptor: %s", why);
    bool top_left;
    rc = siting_of(ctx, d, &top_left); /* what run_frames() would refuse for every frame */
    if (rc) return rc;
    rc = dec.planes_check(ctx, d);
    if (rc) return rc;
    if (depth < 2 || depth > 16) return fail(ctx, H2Y_EINVAL, "depth must be 2..16");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = reserve_batch(ctx, 64);
    if (rc) return rc;
    const size_t pb = h2y_plane_bytes(d), ob = h2y_frame_bytes(d);
    ctx->s_plane_al = (pb + 255) & ~(size_t)255;
    ctx->s_desc = *d;
    for (int c = 0; c < 3; c++) ctx->s_in_off[c] = c * ctx->s_plane_al;
    ctx->s_pay_off = 3 * ctx->s_plane_al;
    const bool decode = dec.kind != decode_src::NONE;
    const size_t h_in = decode ? dec.payload_bytes() : 3 * ctx->s_plane_al;
    rc = stream_alloc(ctx, depth, h_in, decode ? ctx->s_pay_off + h_in : h_in, ob, ob);
    if (rc) return rc;
    if (dec.kind == decode_src::PQCODE) { /* the linearisation's entries: the code planes in the payload, the slot's three planes */
        std::vector<linearize_frame> tab(depth);
        for (int k = 0; k < depth; k++) {
            char *const planes[3] = {ctx->ss[k].d_in + ctx->s_in_off[0], ctx->ss[k].d_in + ctx->s_in_off[1], ctx->ss[k].d_in + ctx->s_in_off[2]};
            tab[k] = pqcode_entry(ctx, dec.code, ctx->ss[k].d_in + ctx->s_pay_off, planes);
        }
        rc = slot_table(ctx, tab, "PQ code");
        if (rc) return rc;
    } else if (decode) {
        std::vector<payload_frame> tab(depth);
        for (int k = 0; k < depth; k++) {
            tab[k].payload = ctx->ss[k].d_in + ctx->s_pay_off;
            for (int c = 0; c < 3; c++) tab[k].plane[c] = ctx->ss[k].d_in + ctx->s_in_off[c];
        }
        rc = slot_table(ctx, tab, dec.kind == decode_src::DPX ? "DPX" : dec.kind == decode_src::TIFF ? "TIFF" : "EXR");
        if (rc) return rc;
    }
    ctx->s_kind = h2y_ctx::RING_FORWARD;
    ctx->s_src = dec;
    ctx->s_out_bytes = ob;
    ring_frame &f = ctx->s_frame;
    f.width = d->width, f.height = d->height, f.chroma = d->dst_chroma_format_idc;
    contiguous_planes(f.width, f.height, f.chroma, f.off);
    f.depth = d->dst_bit_depth, f.full_range = d->dst_full_range;
    return H2Y_OK;
}

/* The same ring for the .yuv -> G,B,R flow: a slot's input is Y, Cb/Dz, Cr/Dx one after the other (each 256-byte aligned; one
 * H2D copy), its output G | B | R, width x height each, contiguous on the host (one D2H copy where the device planes are too).
 * With interleave (write_tiff's), the slot's device output holds after the planes, 256-byte aligned, the interleaved samples,
 * and only those go down; each slot's k_rgb_interleave table entry is uploaded here once.  The stages see the G, B, R planes the
 * inverse kernel writes, s_out_stride bytes apart (before any interleave). */
static int open_inverse_ring(h2y_ctx *ctx, const inv_params &p, bool interleave, int depth)
{
    int rc = ring_may_open(ctx);
    if (!rc) rc = inverse_check(ctx, p);
    int form = 0;
    if (!rc) rc = inverse_form(ctx, p.chroma, p.algorithm, &form); /* the context's inverse chroma siting, read as the ring opens */
    if (rc) return rc;
    if (depth < 2 || depth > 16) return fail(ctx, H2Y_EINVAL, "depth must be 2..16");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t pb = (size_t)p.width * p.height * sizeof(uint16_t), pb_al = (pb + 255) & ~(size_t)255;
    const size_t cb = p.chroma == H2Y_CHROMA_420 ? (size_t)(p.width >> 1) * (p.height >> 1) * sizeof(uint16_t) : pb;
    const size_t cb_al = (cb + 255) & ~(size_t)255;
    ctx->s_in_off[0] = 0;
    ctx->s_in_off[1] = pb_al;
    ctx->s_in_off[2] = pb_al + cb_al;
    ctx->s_in_bytes = pb_al + cb_al + cb;
    ctx->s_out_stride = (pb & 15) ? pb_al : pb; /* 4:2:0 planes are always a multiple of 16 bytes */
    ctx->s_pay_off = (2 * ctx->s_out_stride + pb + 255) & ~(size_t)255;
    ctx->s_inv = p;
    ctx->s_inv.algorithm = form; /* inverse_produce's UP_* form */
    rc = stream_alloc(ctx, depth, ctx->s_in_bytes, ctx->s_in_bytes, 3 * pb, interleave ? ctx->s_pay_off + 3 * pb : 2 * ctx->s_out_stride + pb);
    if (rc) return rc;
    if (interleave) {
        std::vector<rgb_frame> tab(depth);
        for (int k = 0; k < depth; k++) {
            char *o = reinterpret_cast<char *>(ctx->ss[k].d_out);
            for (int c = 0; c < 3; c++) tab[k].plane[c] = reinterpret_cast<const uint16_t *>(o + c * ctx->s_out_stride);
            tab[k].rgb = reinterpret_cast<uint16_t *>(o + ctx->s_pay_off);
        }
        rc = slot_table(ctx, tab, "TIFF inverse");
        if (rc) return rc;
    }
    ctx->s_kind = h2y_ctx::RING_INVERSE;
    ctx->s_interleave = interleave;
    ring_frame &f = ctx->s_frame;
    f.width = p.width, f.height = p.height, f.chroma = H2Y_CHROMA_444;
    for (int c = 0; c < 3; c++) f.off[c] = (uint32_t)(c * ctx->s_out_stride / sizeof(uint16_t));
    f.depth = p.out_depth, f.full_range = p.in_full_range, f.gbr = true;
    return H2Y_OK;
}

/* A ring without a producer, for the stage its opener arms it with (the caller has made its own checks): the slot's input is the
 * frame's three planes one after the other (one H2D copy), which the stages see there; its output holds out_bytes, which go down
 * if a stage writes them (0: nothing does) */
int open_planes_ring(h2y_ctx *ctx, int width, int height, int chroma, int bit_depth, int full_range, int gbr, size_t out_bytes,
                            int depth)
{
    if (depth < 2 || depth > 16) return fail(ctx, H2Y_EINVAL, "depth must be 2..16");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ring_frame f;
    f.width = width, f.height = height, f.chroma = chroma;
    contiguous_planes(width, height, chroma, f.off);
    f.depth = bit_depth, f.full_range = full_range, f.gbr = gbr != 0, f.in_input = true;
    for (int c = 0; c < 3; c++) ctx->s_in_off[c] = f.off[c] * sizeof(uint16_t);
    ctx->s_in_bytes = ((size_t)f.off[2] + (f.off[2] - f.off[1])) * sizeof(uint16_t); /* the last plane is as long as the second */
    const size_t in = std::max<size_t>(ctx->s_in_bytes, 16), out = std::max<size_t>(out_bytes, 16);
    const int rc = stream_alloc(ctx, depth, in, in, out, out);
    if (rc) return rc;
    ctx->s_kind = h2y_ctx::RING_PLANES;
    ctx->s_frame = f;
    ctx->s_out_bytes = out_bytes;
    if (!out_bytes) ring_frame_stays(ctx);
    return H2Y_OK;
}

int h2y_stream_open(h2y_ctx *ctx, const h2y_desc *d, int depth) { return open_forward_ring(ctx, d, nullptr, depth); }

int h2y_inverse_stream_open(h2y_ctx *ctx, int width, int height, int in_chroma_format_idc, int in_bit_depth, int in_full_range,
                            int in_matrix_coeffs, int out_bit_depth, int algorithm, int depth)
{
    const inv_params p{width, height, in_chroma_format_idc, in_bit_depth, in_full_range, in_matrix_coeffs, out_bit_depth, algorithm};
    return open_inverse_ring(ctx, p, false, depth);
}

int h2y_dpx_stream_open(h2y_ctx *ctx, const h2y_desc *d, const h2y_dpx_info *info, int depth)
{
    const decode_src src(info);
    return open_forward_ring(ctx, d, &src, depth);
}

int h2y_tiff_stream_open(h2y_ctx *ctx, const h2y_desc *d, const h2y_tiff_info *info, int clamp_video_range, int depth)
{
    const decode_src src(info, clamp_video_range);
    return open_forward_ring(ctx, d, &src, depth);
}

int h2y_tiff_inverse_stream_open(h2y_ctx *ctx, int width, int height, int in_chroma_format_idc, int in_bit_depth, int in_full_range,
                                 int in_matrix_coeffs, int out_bit_depth, int algorithm, int depth)
{
    const inv_params p{width, height, in_chroma_format_idc, in_bit_depth, in_full_range, in_matrix_coeffs, out_bit_depth, algorithm};
    return open_inverse_ring(ctx, p, true, depth);
}

int h2y_exr_stream_open(h2y_ctx *ctx, const h2y_desc *d, const h2y_exr_info *info, int depth)
{
    const decode_src src(info);
    return open_forward_ring(ctx, d, &src, depth);
}

/* the four code rings: the codes are PQ's, HLG's at a display peak, SDR's at a reference white, or stay signal (no transfer) */
static int open_code_ring(h2y_ctx *ctx, const h2y_desc *d, const h2y_codelight_desc *code, code_tf tf, int depth)
{
    int rc = ring_may_open(ctx);
    if (rc) return rc;
    codelight_plan p;
    rc = codelight_check(ctx, code, p); /* the inverse chroma siting is read here */
    if (rc) return rc;
    if (!d) return fail(ctx, H2Y_EINVAL, "null h2y_desc");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hlgsrc_args ha{};
    float kappa = 0.0f;
    rc = tf.kind == code_tf::HLG ? hlgsrc_args_of(ctx, p, tf.param, ha) : tf.kind == code_tf::SDR ? sdrsrc_tables(ctx, p, tf.param, kappa) :
         tf.kind == code_tf::SIGNAL ? sigsrc_check(ctx, p) : codelight_tables(ctx, p);
    if (!rc) rc = pqcode_scratch(ctx, p);
    if (rc) return rc;
    const decode_src src = tf.kind == code_tf::HLG ? decode_src(p, ha) : tf.kind == code_tf::SDR ? decode_src(p, kappa) :
                           tf.kind == code_tf::SIGNAL ? decode_src(p, decode_src::signal_tag{}) : decode_src(p);
    return open_forward_ring(ctx, d, &src, depth);
}

int h2y_pqcode_stream_open(h2y_ctx *ctx, const h2y_desc *d, const h2y_codelight_desc *code, int depth)
{
    return open_code_ring(ctx, d, code, code_tf{}, depth);
}

int h2y_hlgcode_stream_open(h2y_ctx *ctx, const h2y_desc *d, const h2y_codelight_desc *code, int peak, int depth)
{
    return open_code_ring(ctx, d, code, code_tf{code_tf::HLG, peak}, depth);
}

int h2y_sdrcode_stream_open(h2y_ctx *ctx, const h2y_desc *d, const h2y_codelight_desc *code, int white, int depth)
{
    return open_code_ring(ctx, d, code, code_tf{code_tf::SDR, white}, depth);
}

/* The code ring whose planes stay signal, and the signal-mode LUT that reads them, in one call: without the LUT's scale step the
 * passthrough conversion would scale nothing, so the ring never exists unarmed.  What h2y_pqcode_stream_open refuses of d and code
 * it refuses, then what h2y_stream_lut3d(signal 1) refuses of d and the table; the ring is closed again if the arming fails. */
int h2y_sigcode_stream_open(h2y_ctx *ctx, const h2y_desc *d, const h2y_codelight_desc *code, const h2y_lut3d *lut, int interp, int depth)
{
    int rc = open_code_ring(ctx, d, code, code_tf{code_tf::SIGNAL, 0}, depth);
    if (rc) return rc;
    rc = h2y_stream_lut3d(ctx, lut, interp, 1);
    if (rc) stream_free(ctx); /* nothing has run on it; the context keeps the arming's message */
    return rc;
}

/* ---- the ring's frame by frame entries ------------------------------------------------------------------------------------------ */

/* the slot's input goes up on s_h2d */
static int ring_upload(h2y_ctx *ctx, h2y_ctx::stream_slot &s)
{
    if (ctx->s_stage[STAGE_UNPACK]) return H2Y_OK; /* the stage's own upload brings the packed frame instead */
    if (ctx->s_kind != h2y_ctx::RING_FORWARD) { /* the planes as the slot holds them: one copy (none of an empty frame) */
        if (ctx->s_in_bytes) HIP_TRY(ctx, hipMemcpyAsync(s.d_in, s.h_in, ctx->s_in_bytes, hipMemcpyHostToDevice, ctx->s_h2d));
    } else if (ctx->s_src.kind != decode_src::NONE) /* the payload goes up; the decode writes the three planes below it */
        HIP_TRY(ctx, hipMemcpyAsync(s.d_in + ctx->s_pay_off, s.h_in, ctx->s_src.payload_bytes(), hipMemcpyHostToDevice, ctx->s_h2d));
    else /* the slot's three planes lie one after the other (each padded to 256 bytes): one copy command, not three */
        HIP_TRY(ctx, hipMemcpyAsync(s.d_in, s.h_in, 2 * ctx->s_plane_al + h2y_plane_bytes(&ctx->s_desc), hipMemcpyHostToDevice, ctx->s_h2d));
    return H2Y_OK;
}

/* a forward ring's frame on the context's stream: the decode, pic_stats, the conversion */
static int forward_produce(h2y_ctx *ctx, int slot)
{
    h2y_ctx::stream_slot &s = ctx->ss[slot];
    const h2y_desc *d = &ctx->s_desc;
    const decode_src &src = ctx->s_src;
    frame_io io;
    for (int c = 0; c < 3; c++) io.in[c] = s.d_in + c * ctx->s_plane_al;
    io.out = s.d_out;
    io.tmp_cb = io.tmp_cr = nullptr;
    int rc = H2Y_OK;
    if (src.kind == decode_src::PQCODE) rc = pqcode_decode(ctx, slot);
    else if (src.kind != decode_src::NONE) HIP_TRY(ctx, src.launch(ctx, static_cast<const payload_frame *>(ctx->s_tab) + slot, 1));
    if (rc) return rc;
    for (auto &st : ctx->s_stage) /* what works on the decoded planes: pic_stats and all that follows see its result */
        if (!rc && st) rc = st->decoded(ctx, slot);
    if (rc) return rc;
    const bool needs_stats = d->src_transfer != d->dst_transfer;
    if (needs_stats && !d->stats_override) {
        rc = run_stats(ctx, d, io.in, (int)ctx->b->frames_cap, ctx->b->d_assumed); /* published in device memory, read by the next kernel */
        ctx->b->dev_assumed_ok = false; /* d_assumed[0] no longer holds what the last enqueued batch left there */
        if (rc) return rc;
    } else {
        /* the same six integers for every frame of the stream: staged once per slot, so an earlier copy still in flight reads its own */
        assumed_stats *as = reinterpret_cast<assumed_stats *>(s.h_out); /* the slot's pinned output is idle until its D2H */
        for (int c = 0; c < 3; c++) {
            as->floor_[c] = d->stats_override ? d->floor[c] : 0;
            as->ceil_[c] = d->stats_override ? d->ceiling[c] : 1;
        }
        HIP_TRY(ctx, hipMemcpyAsync(ctx->b->d_assumed, as, sizeof *as, hipMemcpyHostToDevice, ctx->stream));
        ctx->b->dev_assumed_ok = false; /* d_assumed[0] no longer holds what the last enqueued batch left there */
    }
    ctx->slot_base = slot;
    ctx->b->n_ev = 0;
    ctx->cur_skip_t1 = false; /* PCIe-bound here: no steering between the tiers */
    rc = run_frames(ctx, d, &io, 1, ctx->b->d_assumed, nullptr, false, slot, false);
    ctx->slot_base = 0;
    return rc;
}

/* an inverse ring's frame: k_inverse420 / k_inverse and, where the frame goes down interleaved, k_rgb_interleave */
static int inverse_produce(h2y_ctx *ctx, int slot)
{
    h2y_ctx::stream_slot &s = ctx->ss[slot];
    const inv_params &p = ctx->s_inv;
    /* every plane starts on a 16-byte boundary here: the single-frame kernels' wide accesses are safe */
    inv420_args a;
    inverse420_setup(a, p.width, p.height, p.in_depth, p.in_full_range, p.matrix, p.out_depth, p.algorithm);
    for (int c = 0; c < 3; c++) {
        a.inv.in[c] = s.d_in + ctx->s_in_off[c];
        a.inv.out[c] = reinterpret_cast<char *>(s.d_out) + c * ctx->s_out_stride;
    }
    if (p.chroma == H2Y_CHROMA_420) {
        a.up.src0 = static_cast<const uint16_t *>(a.inv.in[1]);
        a.up.src1 = static_cast<const uint16_t *>(a.inv.in[2]);
        a.inv.in[1] = a.inv.in[2] = nullptr;
        HIP_TRY(ctx, h2y_launch_inverse420(ctx->stream, a));
    } else {
        uint32_t blocks = (a.inv.npix / 4 + 255) / 256; /* as h2y_matrix_inverse */
        if (blocks > (uint32_t)ctx->n_cu * 16u) blocks = (uint32_t)ctx->n_cu * 16u;
        if (blocks < 1) blocks = 1;
        HIP_TRY(ctx, h2y_launch_inverse((int)blocks, ctx->stream, a.inv));
    }
    if (ctx->s_interleave && ctx->s_down) { /* write_tiff's interleave into the slot's device output behind the planes */
        const uint32_t npix = (uint32_t)p.width * (uint32_t)p.height;
        HIP_TRY(ctx, h2y_launch_rgb_interleave(unit_grid(ctx, h2y_rgb_chunks(npix)), ctx->stream, npix,
                                               static_cast<const rgb_frame *>(ctx->s_tab) + slot, 1));
    }
    return H2Y_OK;
}

/* the produced frame goes down on s_d2h (s_down) */
static int ring_download(h2y_ctx *ctx, h2y_ctx::stream_slot &s)
{
    if (ctx->s_kind != h2y_ctx::RING_INVERSE) { /* the .yuv frame, or what a stage wrote into the output of a ring without a producer */
        HIP_TRY(ctx, hipMemcpyAsync(s.h_out, s.d_out, ctx->s_out_bytes, hipMemcpyDeviceToHost, ctx->s_d2h));
        return H2Y_OK;
    }
    const size_t pb = (size_t)ctx->s_inv.width * ctx->s_inv.height * sizeof(uint16_t), so = ctx->s_out_stride;
    if (ctx->s_interleave)
        HIP_TRY(ctx, hipMemcpyAsync(s.h_out, reinterpret_cast<char *>(s.d_out) + ctx->s_pay_off, 3 * pb, hipMemcpyDeviceToHost, ctx->s_d2h));
    else if (so == pb) HIP_TRY(ctx, hipMemcpyAsync(s.h_out, s.d_out, 3 * pb, hipMemcpyDeviceToHost, ctx->s_d2h));
    else
        for (int c = 0; c < 3; c++)
            HIP_TRY(ctx, hipMemcpyAsync(reinterpret_cast<char *>(s.h_out) + c * pb, reinterpret_cast<char *>(s.d_out) + c * so, pb,
                                        hipMemcpyDeviceToHost, ctx->s_d2h));
    return H2Y_OK;
}

int h2y_stream_input(h2y_ctx *ctx, void *planes[3])
{
    if (!ctx || !planes) return fail(ctx, H2Y_EINVAL, "null argument");
    if (!ctx->streaming) return fail(ctx, H2Y_EINVAL, "no stream open");
    h2y_ctx::stream_slot &s = ctx->ss[ctx->s_tail];
    if (s.state == 1) { /* asked twice without a submit: same buffers again */
    } else if (s.state != 0) return fail(ctx, H2Y_EINVAL, "all %d slots are in flight: take an output first", (int)ctx->ss.size());
    s.state = 1;
    ctx->s_started = true;
    if (ring_stage *un = ctx->s_stage[STAGE_UNPACK].get()) { /* the packed frame, as the file holds it */
        planes[0] = un->lend(ctx, ctx->s_tail);
        planes[1] = planes[2] = nullptr;
        return H2Y_OK;
    }
    if (ctx->s_src.kind != decode_src::NONE) { /* the payload, as the file holds it (TIFF: the decoded rows, packed; EXR: unpacked) */
        planes[0] = s.h_in;
        planes[1] = planes[2] = nullptr;
        return H2Y_OK;
    }
    for (int c = 0; c < 3; c++) planes[c] = s.h_in + ctx->s_in_off[c];
    return H2Y_OK;
}

/* One frame through the ring: its upload and the armed stages' on s_h2d; on the context's stream the ring's producer, then the
 * stages in their order (an unpack stage's k_unpack in front of the producer); on s_d2h the frame (where it goes down) and the stages' results */
int h2y_stream_submit(h2y_ctx *ctx)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if (!ctx->streaming) return fail(ctx, H2Y_EINVAL, "no stream open");
    const int slot = ctx->s_tail;
    h2y_ctx::stream_slot &s = ctx->ss[slot];
    if (s.state != 1) return fail(ctx, H2Y_EINVAL, "nothing to submit: call h2y_stream_input first");
    int rc = H2Y_OK;
    for (auto &st : ctx->s_stage)
        if (!rc && st) rc = st->ready(ctx, slot);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = ring_upload(ctx, s);
    for (auto &st : ctx->s_stage)
        if (!rc && st) rc = st->upload(ctx, slot);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(s.ev_h2d, ctx->s_h2d));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, s.ev_h2d, 0));
    for (auto &st : ctx->s_stage) /* the planes of a packed input, before anything reads them */
        if (!rc && st) rc = st->unpack(ctx, slot);
    if (rc) return rc;
    if (ctx->s_kind == h2y_ctx::RING_FORWARD) rc = forward_produce(ctx, slot);
    else if (ctx->s_kind == h2y_ctx::RING_INVERSE) rc = inverse_produce(ctx, slot);
    for (auto &st : ctx->s_stage)
        if (!rc && st) rc = st->run(ctx, slot);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(s.ev_conv, ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_d2h, s.ev_conv, 0));
    if (ctx->s_down) rc = ring_download(ctx, s);
    for (auto &st : ctx->s_stage)
        if (!rc && st) rc = st->download(ctx, slot);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(s.ev_done, ctx->s_d2h));
    s.state = 2;
    ctx->s_tail = (slot + 1) % (int)ctx->ss.size();
    return H2Y_OK;
}

int h2y_stream_output(h2y_ctx *ctx, const uint16_t **yuv)
{
    if (!ctx || !yuv) return fail(ctx, H2Y_EINVAL, "null argument");
    if (!ctx->streaming) return fail(ctx, H2Y_EINVAL, "no stream open");
    if (ctx->s_lent >= 0) { /* the frame handed out last time goes back into the ring */
        ctx->ss[ctx->s_lent].state = 0;
        ctx->s_lent = -1;
    }
    h2y_ctx::stream_slot &s = ctx->ss[ctx->s_head];
    if (s.state != 2) return fail(ctx, H2Y_EINVAL, "no submitted frame is waiting");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(s.ev_done));
    *yuv = s.result;
    s.state = 3;
    ctx->s_lent = ctx->s_head;
    ctx->s_head = (ctx->s_head + 1) % (int)ctx->ss.size();
    return H2Y_OK;
}

int h2y_stream_close(h2y_ctx *ctx)
{
    if (!ctx) return fail(nullptr, H2Y_EINVAL, "null ctx");
    if (!ctx->streaming) return H2Y_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    (void)hipStreamSynchronize(ctx->s_h2d);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamSynchronize(ctx->s_d2h);
    stream_free(ctx);
    return H2Y_OK;
}
