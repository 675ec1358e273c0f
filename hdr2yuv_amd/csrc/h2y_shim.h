/*
 * h2y_shim.h -- what the shim's translation units share (h2y_api.hip, h2y_forward.hip, h2y_ring.hip, h2y_measure.hip): the context,
 * the streaming ring's stage interface, and the helpers every entry uses (those of the entries' refusals and the shared stages in
 * h2y_entry.h, included at the end).  Internal: not installed, no part of the ABI.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"
#include "h2y_math.h"

using namespace h2y;

#pragma GCC visibility push(hidden)

struct clip_limits { /* clip_limits_t, hdr.h:345-356 */
    uint32_t minCV, maxCV, minVR, maxVR, minVRC, maxVRC, Half;
};

/* set_pic_clip(), common.cpp:300-327 */
inline clip_limits make_clip(int bit_depth, int full_range)
{
    clip_limits c;
    c.minCV = 0;
    c.maxCV = (1u << bit_depth) - 1;
    c.Half = 1u << (bit_depth - 1);
    if (!full_range) {
        uint32_t D = 1u << (bit_depth - 8);
        c.minVR = 16 * D;
        c.maxVR = 219 * D + c.minVR; /* = 235*D, kept as the reference has it */
        c.minVRC = c.minVR;
        c.maxVRC = 224 * D + c.minVRC;
    } else {
        c.minVR = 0;
        c.maxVR = c.maxCV;
        c.minVRC = 0;
        c.maxVRC = c.maxCV;
    }
    return c;
}

const int kMaxEvents = 64;

/* A grow-only device workspace of the context: ensure() grows it, and it is freed when h2y_ctx_destroy deletes the context, on the
 * context's device, after the last work on its streams was waited for.  No workspace depends on another, so their order (the reverse
 * of their declaration) does not matter.  One declaration in h2y_ctx is all a new one needs. */
template <typename T> struct dev_buf {
    T *p = nullptr;
    size_t cap = 0; /* bytes */
    dev_buf() = default;
    dev_buf(const dev_buf &) = delete;
    dev_buf &operator=(const dev_buf &) = delete;
    ~dev_buf()
    {
        if (p) (void)hipFree(p);
    }
};

/* The parameters of one .yuv -> G,B,R flow (h2y_inverse_batch, h2y_inverse_stream_open) */
struct inv_params {
    int width, height, chroma, in_depth, in_full_range, matrix, out_depth, algorithm;
};

/* what a checked h2y_codelight_desc comes to (codelight_check, h2y_measure.hip) */
struct codelight_plan {
    codelight_args a{};
    int width = 0, height = 0, bit_depth = 0;
    int matrix = 0, form = UP_REPLICATE;
    bool sub = false;      /* 4:2:0: planes 1 and 2 come from the scratch */
    size_t plane_al = 0;   /* 4:2:0: the bytes from one upsampled plane to the next (256-byte aligned) */
    up_args up{};          /* 4:2:0: k_up444's arguments but the planes */
    uint32_t off[3] = {0, 0, 0}; /* the planes' starts in the frame, in samples */
    uint32_t samples = 0;  /* the frame's samples, all three planes */
};

/* What a decode batch entry or a forward ring decodes: nothing (a ring's caller fills the planes), or one format's payload
 * described by the info its parser returned.  Each format's launch and variant lie beside its parser.  PQCODE (h2y_pqcode_stream_open):
 * the payload is a PQ code frame, the decode its linearisation (pqcode_decode, h2y_measure.hip) by the plan checked at the opening.
 * The same kind with hlg set (h2y_hlgcode_stream_open): the codes are HLG's, the decode k_hlg_linearize at hlg.kappa's peak; with sdr
 * set (h2y_sdrcode_stream_open): the codes are BT.1886's, the decode k_sdr_linearize at sdr_kappa's reference white; with signal set
 * (h2y_sigcode_stream_open): no transfer is applied, the decode is k_code_signal and the planes hold G', B', R' for the signal-mode
 * LUT that opener arms. */
struct decode_src {
    enum kind_t { NONE, DPX, TIFF, EXR, PQCODE } kind = NONE;
    bool has_info = true; /* false: the caller passed a null info, which check() refuses */
    int clamp = 0;        /* TIFF: clamp_video_range */
    h2y_dpx_info dpx{};
    h2y_tiff_info tiff{};
    h2y_exr_info exr{};
    codelight_plan code{};
    bool hlg = false;     /* PQCODE: the frame holds HLG codes; hlgsrc: k_hlg_linearize's arguments, the tables in the context's hlgsrc_tables */
    hlgsrc_args hlgsrc{};
    bool sdr = false;     /* PQCODE: the frame holds SDR (BT.1886) codes; code.a carries that stage's tables (sdrsrc_tables), sdr_kappa W / 10000 */
    float sdr_kappa = 0.0f;
    bool signal = false;  /* PQCODE: the planes are the codes' signal, no transfer applied (k_code_signal; code.a's table and pp stay unset) */
    struct signal_tag {};
    decode_src() = default;
    explicit decode_src(const codelight_plan &p) : kind(PQCODE), code(p) {}
    decode_src(const codelight_plan &p, const hlgsrc_args &h) : kind(PQCODE), code(p), hlg(true), hlgsrc(h) {}
    decode_src(const codelight_plan &p, float kappa) : kind(PQCODE), code(p), sdr(true), sdr_kappa(kappa) {}
    decode_src(const codelight_plan &p, signal_tag) : kind(PQCODE), code(p), signal(true) {}
    explicit decode_src(const h2y_dpx_info *i) : kind(DPX), has_info(i != nullptr) { if (i) dpx = *i; }
    decode_src(const h2y_tiff_info *i, int clamp_video_range) : kind(TIFF), has_info(i != nullptr), clamp(clamp_video_range) { if (i) tiff = *i; }
    explicit decode_src(const h2y_exr_info *i) : kind(EXR), has_info(i != nullptr) { if (i) exr = *i; }
    int check(h2y_ctx *ctx) const;                           /* the info is one the parser can return (TIFF: and clamp is 0 or 1) */
    int planes_check(h2y_ctx *ctx, const h2y_desc *d) const; /* d's input planes are the decode's: its sample type, the picture's size */
    uint64_t payload_bytes() const;
    uintptr_t align() const; /* what the payload and the planes must be aligned to, in bytes */
    hipError_t launch(const h2y_ctx *ctx, const payload_frame *frames, int n) const; /* the decode of n frames of a table */
    const char *kernel() const;
    std::string variant() const;
};

/* Everything one batch in flight owns: two of them let h2y_convert_batch_enqueue() queue batch k+1 behind batch k
 * before h2y_batch_finish() has looked at k (the 35 us between two launches -- the statistics kernel, one copy, the
 * host's turn-around -- disappear behind the running kernel). */
struct batch_state {
    /* per-batch device arrays */
    frame_io *d_frames = nullptr, *h_frames = nullptr;
    size_t frames_cap = 0;
    std::vector<frame_io> dev_frames; /* what d_frames holds (size frames_cap once anything was copied; cleared when d_frames is reallocated) */
    float *d_partial = nullptr;
    size_t partial_cap = 0;
    uint32_t *d_redo = nullptr; /* k_fused_t1: per-wave counts of redone tiles */
    size_t redo_cap = 0;
    uint32_t *d_low = nullptr;  /* k_fused_t1: per-frame flag "a sample <= -1 was seen" (zero between launches) */
    size_t low_cap = 0;
    bool approx_min = false;    /* the batch's statistics hold a subsampled minimum (exact only where they match) */
    unsigned long long *d_clock = nullptr;
    size_t clock_cap = 0;
    int bal_slot = 0;                         /* the eight run times travel in the frame_stats entry after the batch's last */
    bool bal_pending = false;                 /* h_fstats[bal_slot] will hold the times of a launch dealt with bal_work */
    double bal_work[8] = {1, 1, 1, 1, 1, 1, 1, 1}; /* relative work a block of XCD x had in that launch */
    /* fused_args.slice_ranges ([blocks of a group + 1]): two tables in pinned host memory that the kernels read in place (a
     * block reads two words of it, once) -- no copy command between two launches.  Two, because the launches of one batch may
     * need different tables (the last one, when it holds fewer frames) while the earlier ones have not run yet. */
    uint32_t *h_ranges = nullptr, *hd_ranges = nullptr; /* host and device address of the same 2 x kRangeWords words (h2y_plan.h) */
    uint32_t *d_tail = nullptr; /* the dynamic last frame's counters: [16 groups][H2Y_TAIL_WORDS]: counters and exhausted bits, zero between launches (k_stats_final) */
    float *h_btime = nullptr, *hd_btime = nullptr; /* every block's run time of a timed launch (pinned, written by k_stats_final) */
    int bal_grid = 0, bal_groups = 0;              /* the launch those times (and bal_bwork) belong to; 0: none */
    std::vector<double> bal_bwork;                 /* relative work each block of the grid had in that launch */
    std::vector<uint32_t> range_slot[2];      /* what the two tables hold */
    bool slot_busy[2] = {false, false};       /* a launch of the batch being queued reads it */
    /* k_fir_fused: the rows of every unit (frame, segment, strip), cut by XCD speed */
    uint32_t *d_unit_rows = nullptr, *h_unit_rows = nullptr;
    size_t unit_rows_cap = 0;                 /* in units */
    std::vector<uint32_t> dev_unit_rows;      /* what d_unit_rows holds */
    bool ffb_pending = false;                 /* h_fstats[bal_slot] will hold the XCD run times of a k_fir_fused launch ... */
    double ffb_work[8] = {0, 0, 0, 0, 0, 0, 0, 0}; /* ... in which a block of XCD x had this much work (steps, mean) */
    frame_stats *d_fstats = nullptr, *h_fstats = nullptr;
    frame_stats *m_fstats = nullptr; /* h_fstats as the device sees it (pinned host memory): k_stats_final of a batch writes there, no copy command */
    frame_stats *fs_out = nullptr;   /* where run_frames() has the statistics written: d_fstats, or m_fstats for an enqueued batch */
    assumed_stats *d_assumed = nullptr, *h_assumed = nullptr; /* [2]: [0] batch, [1] redo */
    assumed_stats dev_assumed;       /* what d_assumed[0] holds when dev_assumed_ok (one small copy command less per batch) */
    bool dev_assumed_ok = false;
    /* the batch itself, between enqueue and finish */
    h2y_desc p_desc;
    int p_n = 0;
    bool p_check = false;
    bool was_t1 = false;
    std::vector<frame_io> p_frames;
    hipEvent_t ev_done = nullptr; /* after the batch's last operation on the stream (the copy of its statistics) */
    /* timing of the main kernels */
    hipEvent_t ev[kMaxEvents][2];
    int n_ev = 0;
};

/* The frame an open ring's measurements see, recorded once by the ring's opener: its planes start off[] samples from the slot's
 * device output, or from its device input on a ring without a producer (in_input) */
struct ring_frame {
    int width = 0, height = 0, chroma = 0;
    uint32_t off[3] = {0, 0, 0};
    int depth = 0; /* bit depth; 0: unknown (a compare-only ring) */
    int full_range = 0;
    bool gbr = false; /* the planes are G, B, R */
    bool in_input = false;
};

/* What arming a ring adds to it.  A stage owns its per-slot device and pinned buffers, its device table of per-slot entries and
 * its geometry: whatever it allocates is released by its destructor, whether the arming failed half-way (the ring stays as it
 * was) or the ring closes.  h2y_stream_submit calls the armed stages in the fixed order of stage_id. */
struct ring_stage {
    std::vector<void *> dev, pinned; /* what the stage owns */
    hipError_t err = hipSuccess;     /* the first allocation or copy that failed while arming; the later ones are skipped */
    virtual ~ring_stage()
    {
        for (void *p : dev) (void)hipFree(p);
        for (void *p : pinned) (void)hipHostFree(p);
    }
    template <typename T> void dev_alloc(T *&p, size_t bytes)
    {
        void *q = nullptr;
        if (err == hipSuccess && (err = hipMalloc(&q, bytes)) == hipSuccess) dev.push_back(q);
        p = static_cast<T *>(q);
    }
    template <typename T> void pin_alloc(T *&p, size_t bytes)
    {
        void *q = nullptr;
        if (err == hipSuccess && (err = hipHostMalloc(&q, bytes, hipHostMallocDefault)) == hipSuccess) pinned.push_back(q);
        p = static_cast<T *>(q);
    }
    /* the stage's device table: one entry per slot, uploaded once */
    template <typename T> void table(T *&d, const std::vector<T> &h)
    {
        dev_alloc(d, h.size() * sizeof(T));
        if (err == hipSuccess) err = hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    }
    virtual int ready(h2y_ctx *, int) { return H2Y_OK; }  /* may the slot be submitted? */
    virtual int upload(h2y_ctx *, int) { return H2Y_OK; } /* on s_h2d, before the slot's ev_h2d */
    /* STAGE_UNPACK only: what h2y_stream_input lends in the place of the slot's planes (its upload() then stands for ring_upload's
     * copy), and, on the context's stream before the ring's producer, the planes written where that copy would have put them */
    virtual void *lend(h2y_ctx *, int) { return nullptr; }
    virtual int unpack(h2y_ctx *, int) { return H2Y_OK; }
    /* on the context's stream, on a forward ring's decoded planes: after the decode, before pic_stats and the conversion */
    virtual int decoded(h2y_ctx *, int) { return H2Y_OK; }
    virtual int run(h2y_ctx *ctx, int slot) = 0;          /* on the context's stream, after the frame was produced */
    virtual int download(h2y_ctx *, int) { return H2Y_OK; } /* the result, on s_d2h after the slot's ev_conv */
};
enum stage_id { STAGE_UNPACK, STAGE_GAMUT, STAGE_TONEMAP, STAGE_LUT3D, STAGE_HLG, STAGE_ICTCP, STAGE_LIGHT, STAGE_LIGHTDIST, STAGE_CODELIGHT, STAGE_GAMUTCHECK, STAGE_SCENESIG, STAGE_COMPARE, STAGE_SSIM, STAGE_DELTAE, STAGE_REGIONS, STAGE_HISTOGRAM, STAGE_SCALE, STAGE_DITHER, STAGE_PACK, STAGE_COUNT };

struct h2y_ctx {
    int device = 0;
    batch_state bs[2];
    batch_state *b = &bs[0]; /* the batch the shim is working on (enqueue: the newest; finish: the oldest) */
    int q_head = 0, q_count = 0; /* batches in flight: bs[q_head] is the oldest */
    int n_cu = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    /* FIR pass runs on its own stream so that it overlaps the next sub-batch's fused kernel */
    hipStream_t fir_stream = nullptr;
    hipEvent_t ev_fused[2] = {nullptr, nullptr}, ev_fir[2] = {nullptr, nullptr};
    bool fir_used[2] = {false, false};
    void *d_table = nullptr;
    void *d_table1 = nullptr; /* binary32 first-tier records */
    void *d_table_ext = nullptr; /* pq_build_table_ext(): the binary64 table below 2^-24, read from global memory by pq_slow() */
    void *d_tfn[H2Y_TFN_COUNT] = {}; /* the other transfer functions' tables (tfn_build_table), built when first needed */
    void *d_tfn_ext[H2Y_TFN_COUNT] = {}; /* and their full-range tables in global memory (tfn_build_ext; PQ10000_r's is d_table_ext) */
    float *d_lut16 = nullptr; /* PQ10000_r of every half in [0,2), built on the device at creation */
    /* The first tier is slow on pictures with many exactly-zero samples (black bars: every such tile is done twice).
     * The kernel counts the tiles it had to redo; when their share in a batch exceeds kT1DenseShare the next
     * kT1SkipBatches batches go to k_fused2 (the binary64 tier answers zero by itself), then the first tier is
     * tried again. */
    /* Balancing across XCDs (frame_walk in h2y_kernels.hip): the loop-form kernels leave the mean run time of the blocks
     * of each XCD; the shares of the next launch follow the speeds seen (balance_update()). */
    bool bal_have = false;
    double bal_speed[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    std::vector<double> bal_bspeed; /* per block of the grid (round 3): what is left between blocks once their XCDs are level */
    int bal_bgrid = 0, bal_bgroups = 0; /* the grid shape bal_bspeed is for */
    bool ffb_have = false;                    /* k_fir_fused has its own speeds: it is vector-issue bound, the XCDs differ more on it */
    double ffb_speed[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    int t1_skip = 0, t1_skip_len = 0;
    bool cur_skip_t1 = false;
    /* h2y_ctx_set_option(): tuning / test knobs, per context (nothing is read from the environment) */
    bool opt_t1 = true;        /* "t1": binary32 first tier on */
    bool opt_t1_steer = true;  /* ... and left for the binary64 tier's kernels while the pictures keep it busy passing pixels on */
    int opt_groups = 0;        /* "groups": at most this many frame groups (power of two; 1 = off); 0 = by the frame's size (groups_cap()) */
    bool opt_cols8 = true;     /* "cols8": 8-column tiles for half input where the planes allow */
    bool opt_lut3d_lds = true; /* "lut3d_lds": a 3D LUT of up to 17 nodes per axis is read from the blocks' copies in LDS (k_lut3d_lds) */
    int opt_bal_mode = 0;      /* "balance": 0 adaptive, 1 off, 2 fixed */
    int opt_tail = 2;           /* "tail": 0 auto (groups of at least kTailMinFrames frames), 1 on (two frames suffice), 2 off (the default: measured
                                   neutral on 64 x 4K -- the blocks' finish times close up from +-30 us to +-15 us of a 1.5 ms launch, and the
                                   frame's own dealing costs what that saves) */
    bool opt_bal_blocks = true; /* adaptive: by the speed of every block ("adaptive"), or of the XCDs only ("xcd") */
    uint32_t opt_bal_mask = 0xFFu;
    double opt_bal_rho = 1.0;
    int opt_fir = 0;           /* "fir": 0 auto, 1 two-pass (4:4:4 scratch + k_fir420), 2 fused single pass where it applies */
    int opt_siting = 0;        /* h2y_ctx_set_chroma_siting(): 0 as the resampler sites the chroma, 2 top-left (k_fir420_tl as the second pass) */
    int opt_inv_siting = 0;    /* h2y_ctx_set_inverse_chroma_siting(): 0 the 4:2:0 chroma sited as the reference's upsampler takes it, 2 top-left
                                  (k_up444 / k_inverse420(_batch) in their UP_FIR_TL form) */
    int opt_fir_sync = -1;     /* "firsync": k_fir_fused's blocks meet at a barrier every so many steps (power of two; 0 = never);
                                  -1 = by the pictures: every step, never while the first tier passes many pixels on */
    double fir_flag_share = 0.0; /* share of the last k_fir_fused batch's pixels (in tiles of eight) the first tier could not settle */
    uint16_t *d_tmp = nullptr;
    size_t tmp_cap = 0;
    uint16_t *d_lin = nullptr; /* k_yuvp2_420: lin(Y') of every u16 code (h2y_yuvp2_lin_table), built when first needed */
    /* the frame table of whichever synchronous batch entry runs (h2y_inverse_batch, the decode and compare batches; none runs
     * beside another batch or a stream): pinned on the host, and its device copy the kernels read (frame_table) */
    void *d_tab = nullptr, *h_tab = nullptr;
    size_t d_tab_cap = 0, h_tab_cap = 0; /* bytes */
    /* The grow-only device workspaces of the batch entries and of the armed stages that share one: each is named here, grown by its
     * user (ensure) and released with the context */
    dev_buf<cmp_partial> cmp_part;             /* k_compare's partials (h2y_compare_batch and an armed ring) */
    dev_buf<h2y_compare_stats> cmp_stats;      /* h2y_compare_batch's stats */
    dev_buf<char> hist;                        /* h2y_histogram_batch: per launch the counts, the bins and the stats (hist_layout) */
    dev_buf<int64_t> ssim_part;                /* k_ssim's partials (h2y_ssim_batch and an armed ring) */
    dev_buf<h2y_ssim_stats> ssim_stats;        /* h2y_ssim_batch's stats */
    dev_buf<regions_partial> regions_part;     /* k_regions' partials (h2y_regions_batch and an armed ring) */
    dev_buf<h2y_regions_stats> regions_stats;  /* h2y_regions_batch's stats */
    dev_buf<assumed_stats> light_as;           /* h2y_light_batch's floor / ceiling per frame */
    dev_buf<light_acc> light_accs;             /* h2y_light_batch's accumulators */
    dev_buf<char> lightdist;                   /* h2y_lightdist_batch: per launch k_lightdist's accumulators, then the bins (lightdist_layout) */
    dev_buf<char> codelight;                   /* h2y_codelight_batch: light_acc, then lightdist_layout */
    dev_buf<char> codelight_up;                /* the code-plane launches' upsampled 4:2:0 chroma (code light, the linearisers, Delta E, the code rings) */
    dev_buf<gamutcheck_frame_acc> gamutcheck;  /* h2y_gamutcheck_batch's accumulators */
    dev_buf<unsigned long long> scenesig;      /* h2y_scenesig_batch's and h2y_codescenesig_batch's cells: 144 uint64 a frame */
    dev_buf<deltae_acc> deltae;                /* h2y_deltae_batch's accumulators */
    dev_buf<char> scale_tabs;                  /* h2y_scale_batch's tap tables */
    dev_buf<float> gamut_compress_tables;      /* h2y_gamut_compress_batch's three tables */
    dev_buf<float> tonemap_gain;               /* h2y_tonemap_batch's gain table */
    dev_buf<lut3d_node> lut3d;                 /* h2y_lut3d_batch's table */
    dev_buf<float> hlg_tables;                 /* h2y_hlg_batch's two tables: the gains, then the OETF's */
    dev_buf<float> hlgsrc_tables;              /* h2y_hlg_linearize_batch's and the HLG code ring's: the OOTF's gains, then the OETF's inverse */

    /* staging for the host-buffer entry */
    void *d_in = nullptr;
    size_t in_cap = 0;
    uint16_t *d_out = nullptr;
    size_t out_cap = 0;
    /* floor/ceiling of the last frame seen: the assumption for the next batch */
    bool have_hint = false;
    int hint_kind = -1;
    int32_t hint_floor[3] = {0, 0, 0}, hint_ceil[3] = {0, 0, 0};
    /* streaming pipeline (h2y_stream_*): a ring of pinned host slots with device twins */
    struct stream_slot {
        char *h_in = nullptr;      /* pinned: three planes, at s_in_off[0..2] */
        uint16_t *h_out = nullptr; /* pinned: one .yuv frame (an inverse stream: G | B | R) */
        char *d_in = nullptr;
        uint16_t *d_out = nullptr;
        hipEvent_t ev_h2d = nullptr, ev_conv = nullptr, ev_done = nullptr;
        int state = 0; /* 0 free, 1 handed out for filling, 2 submitted, 3 output lent to the caller */
        const uint16_t *result = nullptr; /* what h2y_stream_output hands out: h_out, a stage's frame, or null */
    };
    std::vector<stream_slot> ss;
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    h2y_desc s_desc;
    size_t s_plane_al = 0;
    int s_head = 0, s_tail = 0, s_lent = -1;
    bool streaming = false;
    /* what the ring does with a frame: the forward conversion (open_forward_ring), the .yuv -> G,B,R flow (open_inverse_ring),
     * or nothing, its stages alone working on the uploaded planes (open_planes_ring) */
    enum ring_kind { RING_FORWARD, RING_INVERSE, RING_PLANES } s_kind = RING_FORWARD;
    /* a forward ring's decode: with one, the pinned slot holds the payload, its device twin the three planes (at s_in_off[0..2])
     * and then the payload at s_pay_off */
    decode_src s_src;
    /* an inverse ring: the flow's parameters, where the slot's input planes lie, the bytes of one H2D copy, and the distance
     * between the G, B, R planes in the slot's device output (one plane's bytes, or 256-byte aligned when that would leave a plane
     * misaligned for the kernel); with s_interleave (h2y_tiff_inverse_stream_open) the device output holds, at s_pay_off after
     * the planes, write_tiff's interleaved R,G,B samples, and only they go down */
    inv_params s_inv{};
    bool s_interleave = false;
    size_t s_pay_off = 0;
    size_t s_in_off[3] = {0, 0, 0}, s_in_bytes = 0, s_out_stride = 0;
    /* one entry per slot, uploaded when the ring is opened: the decode's or the interleave's (payload_frame, rgb_frame) */
    void *s_tab = nullptr;
    bool s_started = false; /* an input was handed out: too late to arm */
    ring_frame s_frame;     /* the frame the stages see */
    std::unique_ptr<ring_stage> s_stage[STAGE_COUNT]; /* the armed stages */
    bool s_down = true;     /* the produced frame goes down into the slot's h_out */
    size_t s_out_bytes = 0; /* a forward or planes ring: the bytes of that copy */
    int slot_base = 0; /* run_frames(): first entry of d_frames/h_frames to use (one per stream slot) */
    float last_ms = 0.f;
    const char *last_name = "";
    std::string last_variant; /* last_name with its template arguments and launch shape, e.g. "k_fused_t1<F32,420BOX,YCBCR,PQ_IDENT> groups=8 xcd=1" */
    int last_launches = 0;
    std::string err;
};

int fail(h2y_ctx *ctx, int code, const char *fmt, ...);

#define HIP_TRY(ctx, call)                                                                                  \
    do {                                                                                                    \
        hipError_t e_ = (call);                                                                             \
        if (e_ != hipSuccess) return fail(ctx, H2Y_EHIP, "%s: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

template <typename T> int ensure(h2y_ctx *ctx, T *&p, size_t &cap, size_t need_bytes)
{
    if (cap >= need_bytes) return 0;
    if (p) HIP_TRY(ctx, hipFree(p));
    p = nullptr;
    cap = 0;
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, need_bytes);
    if (e != hipSuccess) return fail(ctx, H2Y_ENOMEM, "hipMalloc(%zu): %s", need_bytes, hipGetErrorString(e));
    p = static_cast<T *>(q);
    cap = need_bytes;
    return 0;
}
template <typename T> int ensure(h2y_ctx *ctx, dev_buf<T> &b, size_t need_bytes) { return ensure(ctx, b.p, b.cap, need_bytes); }

/* the offsets, in samples, of three planes one after the other (4:2:0: two chroma planes of (width >> 1) x (height >> 1)) */
inline void contiguous_planes(int width, int height, int chroma, uint32_t off[3])
{
    const uint32_t n = (uint32_t)width * (uint32_t)height, nc = chroma == H2Y_CHROMA_420 ? (uint32_t)(width >> 1) * (uint32_t)(height >> 1) : n;
    off[0] = 0, off[1] = n, off[2] = n + nc;
}

/* the open ring's stage `id` as the type its measurement armed it with (null: not armed) */
template <typename S> S *stage_of(const h2y_ctx *ctx, int id) { return static_cast<S *>(ctx->s_stage[id].get()); }

/* where the frame the stages see (ring_frame) lies in slot k */
inline const uint16_t *frame_base(const h2y_ctx *ctx, int k)
{
    return ctx->s_frame.in_input ? reinterpret_cast<const uint16_t *>(ctx->ss[k].d_in) : ctx->ss[k].d_out;
}

/* transfer_characteristics code -> what matrix_convert() does with it (convert.cpp:1024-1109);
 * -1: the reference only prints a warning for every pixel */
inline int tf_class(int t)
{
    switch (t) {
    case 8: return H2Y_TF_LINEAR;
    case 16: return H2Y_TF_PQ;
    case 18: return H2Y_TF_RHO_GAMMA;
    case 1: case 6: case 14: case 15: return H2Y_TF_BT1886; /* BT709, BT601, BT2020_10bit, BT2020_12bit */
    default: return -1;
    }
}
/* a generic transfer pair through the table tier: the source stage's and the destination stage's function, by H2Y_TF_* class */
const int kSrcFn[4] = {H2Y_TFN_NONE, H2Y_TFN_PQ_F, H2Y_TFN_RHO_H, H2Y_TFN_G24};
const int kDstFn[4] = {H2Y_TFN_NONE, H2Y_TFN_PQ_R, H2Y_TFN_RHO_R, H2Y_TFN_G24INV};

inline size_t sample_bytes(const h2y_desc *d) { return d->in_sample_type == H2Y_SAMPLE_F32 ? 4 : 2; }

inline int in_kind_of(const h2y_desc *d)
{
    return d->in_sample_type == H2Y_SAMPLE_F32 ? H2Y_IN_F32 : d->in_sample_type == H2Y_SAMPLE_F16 ? H2Y_IN_F16 : H2Y_IN_U16;
}

/* a grid of one block per unit of 256 threads, eight blocks of 256 per CU at most */
inline int unit_grid(const h2y_ctx *ctx, uint64_t units)
{
    const uint64_t max_grid = (uint64_t)ctx->n_cu * 8u;
    return (int)(units < max_grid ? (units ? units : 1) : max_grid);
}

/* A synchronous batch entry's frame table of n entries of T: the context's pinned host table h, and its device copy, grown as
 * needed.  One pair serves every entry: none runs beside another batch or a stream. */
template <typename T> int frame_table(h2y_ctx *ctx, int n, T *&h)
{
    const size_t tb = (size_t)n * sizeof(T);
    int rc = ensure(ctx, ctx->d_tab, ctx->d_tab_cap, tb);
    if (rc) return rc;
    if (ctx->h_tab_cap < tb) {
        if (ctx->h_tab) HIP_TRY(ctx, hipHostFree(ctx->h_tab));
        ctx->h_tab = nullptr;
        ctx->h_tab_cap = 0;
        hipError_t e = hipHostMalloc(&ctx->h_tab, tb, hipHostMallocDefault);
        if (e != hipSuccess) return fail(ctx, H2Y_ENOMEM, "hipHostMalloc(%zu): %s", tb, hipGetErrorString(e));
        ctx->h_tab_cap = tb;
    }
    h = static_cast<T *>(ctx->h_tab);
    return H2Y_OK;
}

/* the time between the two events of each of the batch's n_ev pairs, summed, in milliseconds */
inline hipError_t event_ms(const batch_state *b, float *ms)
{
    *ms = 0.f;
    for (int i = 0; i < b->n_ev; i++) {
        float t = 0.f;
        const hipError_t e = hipEventElapsedTime(&t, b->ev[i][0], b->ev[i][1]);
        if (e != hipSuccess) return e;
        *ms += t;
    }
    return hipSuccess;
}

/* The table h of n_frames entries (frame_table's) goes up once, then launch(frames, f0, nf) enqueues one launch on the device
 * entries [f0, f0 + nf), in launches of up to per_launch frames, each timed with an event pair (launches past the last pair are
 * timed by it); then a synchronisation, and last_ms, last_launches and last_name are the batch's */
template <typename T, typename F>
int timed_launches(h2y_ctx *ctx, const T *h, int n_frames, int per_launch, const char *name, F launch)
{
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_tab, h, (size_t)n_frames * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    const T *frames = static_cast<const T *>(ctx->d_tab);
    int launches = 0;
    for (int f0 = 0; f0 < n_frames; f0 += per_launch, launches++) {
        const int nf = n_frames - f0 < per_launch ? n_frames - f0 : per_launch;
        const int e = launches < kMaxEvents ? launches : kMaxEvents - 1;
        if (launches < kMaxEvents) HIP_TRY(ctx, hipEventRecord(ctx->b->ev[e][0], ctx->stream));
        HIP_TRY(ctx, launch(frames + f0, f0, nf));
        HIP_TRY(ctx, hipEventRecord(ctx->b->ev[e][1], ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->b->n_ev = launches < kMaxEvents ? launches : kMaxEvents;
    HIP_TRY(ctx, event_ms(ctx->b, &ctx->last_ms));
    ctx->last_launches = launches;
    ctx->last_name = name;
    return H2Y_OK;
}

/* ---- h2y_forward.hip: the forward path, as the ring and the measurements use it ---------------------------------------------------- */

void derive_params(const h2y_desc *d, pix_params *pp, bool stage_matrix_only);
int ensure_tfn(h2y_ctx *ctx, int fn);
int run_frames(h2y_ctx *ctx, const h2y_desc *d, const frame_io *frames, int n, const assumed_stats *d_assumed, const assumed_stats *known,
               bool check, int fstats_offset, bool time_it);
int siting_of(h2y_ctx *ctx, const h2y_desc *d, bool *top_left); /* the context's chroma siting on d: applies, does not, or the refusal */
int reserve_batch(h2y_ctx *ctx, int n);
int run_stats(h2y_ctx *ctx, const h2y_desc *d, const void *const in[3], int slot, assumed_stats *publish);

/* ---- h2y_api.hip: the inverse set-up ------------------------------------------------------------------------------------------------ */

int inverse_check(h2y_ctx *ctx, const inv_params &p);
int inverse_form(h2y_ctx *ctx, int chroma, int algorithm, int *form); /* the UP_* form of `algorithm` under the context's inverse chroma siting, or the refusal */
void inverse420_setup(inv420_args &a, int width, int height, int in_bit_depth, int in_full_range, int in_matrix_coeffs, int out_bit_depth,
                      int form);

/* ---- h2y_measure.hip: PQ code planes, for h2y_pqcode_stream_open and the forward ring's PQCODE decode ------------------------------ */

int codelight_check(h2y_ctx *ctx, const h2y_codelight_desc *d, codelight_plan &p); /* reads the context's inverse chroma siting */
int codelight_tables(h2y_ctx *ctx, codelight_plan &p);
int pqcode_scratch(h2y_ctx *ctx, const codelight_plan &p);                    /* the context's scratch for one frame's upsampled chroma */
linearize_frame pqcode_entry(const h2y_ctx *ctx, const codelight_plan &p, const char *payload, char *const planes[3]);
int pqcode_decode(h2y_ctx *ctx, int slot);                                    /* k_up444 (4:2:0) and k_linearize (k_hlg_linearize, k_sdr_linearize, k_code_signal) on the slot's payload */
int hlgsrc_args_of(h2y_ctx *ctx, const codelight_plan &p, int peak, hlgsrc_args &a); /* the peak's tables into the context's, k_hlg_linearize's arguments */
int sdrsrc_tables(h2y_ctx *ctx, codelight_plan &p, int white, float &kappa); /* bt1886_f's tables into the plan, as codelight_tables puts PQ10000_f's; kappa of the white */
int sigsrc_check(h2y_ctx *ctx, const codelight_plan &p);                     /* the signal of code planes needs no tables: its one refusal, matrix_coeffs 14 */
bool ring_holds_signal(const h2y_ctx *ctx);                                  /* the open ring is h2y_sigcode_stream_open's: its planes hold signal, not light */

/* what the codes of a code-plane source are (linearize_frames in h2y_measure.hip, open_code_ring in h2y_ring.hip): PQ's, HLG's at a
 * display peak of param cd/m2, SDR (BT.1886) with its reference white at param cd/m2, or SIGNAL: whatever they are, they stay signal
 * (no transfer applied, no param) */
struct code_tf {
    enum kind_t { PQ, HLG, SDR, SIGNAL } kind = PQ;
    int param = 0;
};

/* ---- h2y_ring.hip: what a measurement's arm and *_stream_open entries use ----------------------------------------------------------- */

void stream_free(h2y_ctx *ctx);
int ring_may_open(h2y_ctx *ctx);
int open_planes_ring(h2y_ctx *ctx, int width, int height, int chroma, int bit_depth, int full_range, int gbr, size_t out_bytes, int depth);
int stage_arm(h2y_ctx *ctx, int id, std::unique_ptr<ring_stage> st, const char *what);
void ring_frame_stays(h2y_ctx *ctx);
#include "h2y_entry.h"

#pragma GCC visibility pop
