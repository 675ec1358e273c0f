/*
 * hdr2yuv (MI355X build) -- host program with the reference's command-line surface (hdr2yuv.cpp:73-263) and its
 * resolution of unset attributes (h2y_cli_args.h) for the in-memory convert path.  It reads raw planar input, hands the
 * planes to the C-ABI (include/hdr2yuv_hip.h) and writes the .yuv frames where write_yuv() would append them
 * (tiff.cpp:440: the file is opened in append mode; planes Y, Cb, Cr, little-endian 16-bit).
 *
 * Input formats:
 *   .yuv / .rgb  16-bit planar integer (hdr2yuv.cpp:582-656; .rgb is R,G,B in the file, planes 2,0,1 in memory)
 *   .f32 / .f16  raw planar float / half in G,B,R plane order -- what dpx_read() or read_exr() (exr.cpp:233-235) leave in
 *                memory; the attributes those readers force on the input picture are forced here too
 *   .dpx         10-bit, 16-bit or float DPX (dpx_read(), dpx.cpp:209-520): the header is parsed here (h2y_dpx_parse), the
 *                payload read straight into the pinned slot of the DPX ring and decoded on the device; one file is one
 *                frame, and a name with one integer conversion (shot.%06d.dpx) numbers the files of a sequence
 *   .tiff        16-bit R,G,B TIFF (read_tiff(), tiff.cpp:54-362): the file is mapped and its IFD parsed here
 *                (h2y_tiff_parse), the decoded rows read into the pinned slot of the TIFF ring and de-interleaved on the
 *                device; numbered like .dpx
 *   .exr         scanline OpenEXR (read_exr(), exr.cpp:138-255; NONE, RLE, ZIPS or ZIP): the file is mapped, its header and
 *                offset table parsed here (h2y_exr_parse), its chunks inflated or copied straight into the pinned slot of the
 *                EXR ring by a pool of unpack threads (at most 16 across all GPU threads), the predictor, reorder and
 *                scanline-to-plane work done on the device; numbered like .dpx.  Its size is checked against the command
 *                line before anything else, also under --dry_run, as read_exr() takes it from the file
 *   --synthetic N  the seeded test frame of SURVEY 8c (no input file), treated as an .exr-like float input
 * and, from .yuv input, the .yuv -> .tiff flow (hdr2yuv.cpp:818-819, matrix_inverse): .tiff output (write_tiff(),
 * tiff.cpp:559-652; the samples interleaved on the device, the file bytes libtiff would write around them, one truncated
 * file per frame, numbered through a name like shot.%06d.tiff) or the same samples as planes R, G, B in one .rgb.
 *
 * Several GPUs (--gpus N, an addition: the reference converts one frame per process): one host thread per GPU, each with
 * its own context and pinned ring; thread r takes a contiguous block of the frame indices (the split of
 * hdr2yuv_amd/shard.py), reads frame k at its offset in the source (hdr2yuv.cpp:624) and writes it at
 * `size of the file at start + k x frame bytes` -- the bytes N appending runs in frame order would have left (tiff.cpp:440).
 *
 * Comparison (--ref_filename R [--sigma_compare S], or --compare_only 1; h2y_cli_args.h): each GPU thread arms its ring
 * (h2y_stream_compare; with no destination the frames stay on the device) or opens a compare-only ring, reads frame k of R into
 * the reference slot beside the input, and keeps the stats of frame k by its index; the report is printed once every thread is
 * done, so it is the same for any --gpus.  Report on stdout, planes Y Cb Cr for .yuv and G B R for .rgb / .tiff, maxv =
 * 2^bit_depth - 1 of the compared frames (the destination's, or the source's under --compare_only), PSNR of n samples with a sum
 * of squared differences sse printed "%.4f" of 10 * log10((double)maxv * maxv * n / sse) in double arithmetic, or "inf" for
 * sse 0:
 *   frame <k> psnr <P0> <psnr> <P1> <psnr> <P2> <psnr> max_abs <m0> <m1> <m2> over <o0> <o1> <o2>     one line per frame, in order
 *   summary frames <N> mean_psnr <P0> <m> <P1> <m> <P2> <m> global_psnr <P0> <g> <P1> <g> <P2> <g> max_abs <m0> <m1> <m2> over <o0> <o1> <o2>
 *   first_over frame <k> plane <P> x <x> y <y> a <a> b <b>       (or "first_over none")
 * mean_psnr: the mean over frames of the per-frame value, a frame with sse 0 counting 99.99; global_psnr: from the summed sse
 * and samples; max_abs the largest |a - b|, over the count of |a - b| > S (S 0 by default); first_over the first such sample in
 * frame, plane and raster order, a the output's (the source's) sample, b R's.  Exit status 3 when S was given and over > 0.
 *
 * SSIM (--ssim 1 beside a comparison; h2y_cli_args.h): each GPU thread arms its ring for SSIM too (h2y_stream_ssim) and keeps
 * the figures of frame k by its index; the report follows the compare report, so it is the same for any --gpus.  Planes as there,
 * values "%.6f", dB = -10 * log10(1 - x) "%.4f" or "inf" for x = 1:
 *   ssim frame <k> <P0> <v> <P1> <v> <P2> <v> all <v> db <P0> <d> <P1> <d> <P2> <d> all <d>      one line per frame, in order
 *   ssim summary frames <N> <P0> <m> <P1> <m> <P2> <m> all <m> db ...     the means over frames (summed in frame order), dB of them
 *   ssim worst frame <k> all <v>                                          the lowest all, the first such frame on ties
 *
 * Histogram (--histogram FILE [--histogram_bits B] [--check_range 1], or --histogram_only 1; h2y_cli_args.h): each GPU thread arms
 * its ring (h2y_stream_histogram; h2y_stream_histogram_ex on a compare-only ring) or opens a histogram-only ring, keeps the stats
 * of frame k by its index and sums its frames' bins; the report is printed once every thread is done, so it, and FILE, are the
 * same for any --gpus.  Planes P0 P1 P2 are Y Cb Cr, or G B R for .rgb / .tiff; occupied counts the non-zero bins of 2^B:
 *   histogram frame <k> <P0> min <m> max <M> below <b> above <a> at_low <l> at_high <h> occupied <o> <P1> ... <P2> ...
 *   histogram summary frames <N> <P0> min .. occupied <o> <P1> ... <P2> ...   (sums, and bins occupied in the totals)
 *   histogram legal <P0> <lo>..<hi> <P1> <lo>..<hi> <P2> <lo>..<hi> outside <below + above over all planes and frames>
 * FILE (text): "bin,code_lo,code_hi,<P0>,<P1>,<P2>", then one line per bin, code_lo = bin << (depth - B), code_hi = code_lo +
 * 2^(depth - B) - 1, the counts summed over the frames (a code above 2^depth - 1 counts in the last bin).  Exit status 4 under
 * --check_range 1 when outside > 0 (3 before it, when the comparison's status is 3).
 *
 * Content light (--content_light 1 on the forward flow; h2y_cli_args.h): each GPU thread arms its ring (h2y_stream_light) and keeps
 * the figures of frame k by its index; the report is printed once every thread is done, so it is the same for any --gpus.  cd/m2
 * "%.4f"; MaxCLL and MaxFALL rounded to the nearest integer (halves away from zero):
 *   light frame <k> peak <cll> at <x> <y> average <fall>              one line per frame, in order (the first pixel holding the peak)
 *   light summary frames <N> maxcll <CLL> frame <k> maxfall <FALL> frame <k>    the largest of each, the first such frame on ties
 *   light x265 --max-cll "<CLL>,<FALL>"
 *   light svt-av1 --content-light <CLL>,<FALL>
 *
 * Scaling (--scale 1 [--scale_taps A] with --dst_pic_width / --dst_pic_height on the forward flow; h2y_cli_args.h): each GPU thread
 * arms its ring (h2y_stream_scale), so the frame that comes down is the converted frame resampled on the device to the destination
 * size (include/hdr2yuv_hip.h states the filter); frame k is written at `size of the file at start + k x scaled frame bytes`.
 * --scale_only 1 resamples a .yuv or .rgb source through a scale-only ring (h2y_scale_stream_open) into a file of the same layout.
 *
 * Primaries (--gamut_convert 1 [--gamut_clip 0|1] on the forward flow from .f32, .f16, .exr and .dpx; h2y_cli_args.h): each GPU thread
 * arms its ring (h2y_stream_gamut) with --src_colour_primaries and --dst_colour_primaries, so every slot's decoded planes are
 * converted in place on the device before pic_stats and the conversion: the run writes the bytes it would write had the source
 * held the converted planes, and --content_light beside it measures the converted light.  The banner carries gamut_convert:,
 * gamut_clip: and the nine entries of gamut_matrix: as "%.9g".
 */
#include <algorithm>
#include <array>
#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <fcntl.h>
#include <memory>
#include <mutex>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>

#include "h2y_cli_args.h"

static uint16_t f32_to_f16(float f)
{
    uint32_t x;
    memcpy(&x, &f, 4);
    uint32_t sign = (x >> 16) & 0x8000u;
    int32_t e = (int32_t)((x >> 23) & 0xFF) - 127 + 15;
    uint32_t m = x & 0x7FFFFFu;
    if (e >= 31) return (uint16_t)(sign | 0x7C00u);
    if (e <= 0) {
        if (e < -10) return (uint16_t)sign;
        m |= 0x800000u;
        int shift = 14 - e;
        uint32_t r = m >> shift, rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
        if (rem > half || (rem == half && (r & 1))) r++;
        return (uint16_t)(sign | r);
    }
    uint32_t r = ((uint32_t)e << 10) | (m >> 13), rem = m & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1))) r++;
    return (uint16_t)(sign | r);
}

/* the seeded frame of SURVEY 8c: frame k of a run uses seed 12345 + k */
static void synth_fill(const h2y_desc &d, void *const planes[3], uint32_t seed)
{
    const size_t n = (size_t)d.width * d.height;
    uint32_t s = seed;
    for (int c = 0; c < 3; c++) {
        for (size_t i = 0; i < n; i++) {
            s = s * 1664525u + 1013904223u;
            float v = (float)(s >> 8) * (1.0f / 16777216.0f);
            if (i == 0) v = 0.0f;
            if (i == 1) v = 1.0f;
            if (d.in_sample_type == H2Y_SAMPLE_F16) ((uint16_t *)planes[c])[i] = f32_to_f16(v);
            else ((float *)planes[c])[i] = v;
        }
    }
}

static bool write_at(int fd, const void *buf, size_t n, off_t at)
{
    const char *p = (const char *)buf;
    while (n) {
        ssize_t w = pwrite(fd, p, n, at);
        if (w < 0) {
            if (errno == EINTR) continue;
            return false;
        }
        p += w;
        at += w;
        n -= (size_t)w;
    }
    return true;
}

/* one .dpx file of the run: its name and where its payload starts */
struct dpx_src {
    std::string path;
    uint64_t offset;
};

/* The .dpx files of the run -- --src_filename itself, or the files numbered --src_start_frame .. + want - 1 of a sequence (as
 * many of them as exist in a row) -- parsed, checked against the command line's size and against the first file's geometry
 * and format.  Returns 0 and fills info and files, or prints the first problem and returns 1. */
static int dpx_scan(const cli_args &a, long want, h2y_dpx_info &info, std::vector<dpx_src> &files)
{
    const bool seq = cli_frame_pattern(a.src) == 1;
    for (long k = 0; k < (seq ? want : 1); k++) {
        const std::string path = cli_frame_name(a.src, a.start_frame + k);
        struct stat st;
        if (stat(path.c_str(), &st)) {
            if (k) break; /* the sequence ends here */
            printf("ERROR: unable to open file %s\n", path.c_str());
            return 1;
        }
        unsigned char hdr[2048];
        FILE *f = fopen(path.c_str(), "rb");
        if (!f) { printf("ERROR: unable to open file %s\n", path.c_str()); return 1; }
        const size_t got = fread(hdr, 1, sizeof hdr, f);
        fclose(f);
        h2y_dpx_info di;
        const char *why = nullptr;
        if (h2y_dpx_parse(hdr, got, (uint64_t)st.st_size, &di, &why)) { printf("ERROR: %s: %s\n", path.c_str(), why); return 1; }
        if (di.width != a.in.width || di.height != a.in.height) {
            printf("ERROR: %s is %dx%d, --src_pic_width/--src_pic_height say %dx%d: resizing is not part of convert() (cv.cpp is "
                   "compiled out in the reference)\n", path.c_str(), di.width, di.height, a.in.width, a.in.height);
            return 1;
        }
        if (k && (di.width != info.width || di.height != info.height || di.bit_size != info.bit_size || di.swap != info.swap)) {
            printf("ERROR: %s is %dx%d %d-bit %s-endian, %s %dx%d %d-bit %s-endian: every file of a sequence must have the same\n",
                   path.c_str(), di.width, di.height, di.bit_size, di.swap ? "big" : "little", files[0].path.c_str(), info.width,
                   info.height, info.bit_size, info.swap ? "big" : "little");
            return 1;
        }
        /* fields dpx_read() ignores: the image element's descriptor (byte 800) and packing (u16 at 804) */
        const unsigned descriptor = hdr[800], packing = di.swap ? (unsigned)hdr[804] << 8 | hdr[805] : (unsigned)hdr[805] << 8 | hdr[804];
        if (descriptor != 50) printf("WARNING: %s: descriptor %u is not 50 (RGB); decoded as R,G,B, as dpx_read() does\n", path.c_str(), descriptor);
        if (di.bit_size == 10 && packing != 1)
            printf("WARNING: %s: 10-bit packing %u is not 1 (filled to 32-bit words, method A); decoded as packing 1, as dpx_read() does\n",
                   path.c_str(), packing);
        if (!k) info = di;
        files.push_back({path, di.data_offset});
    }
    return 0;
}

/* one .tiff file of the run: its name and where its decoded rows lie */
struct tiff_src {
    std::string path;
    std::vector<uint64_t> rows; /* file offset of each decoded row */
    bool contiguous;
};

/* The .tiff files of the run, as dpx_scan: each mapped, its IFD parsed for read_tiff's geometry with the command line's
 * cutouts, checked against the command line's size and against the first file's geometry and byte order. */
static int tiff_scan(const cli_args &a, long want, h2y_tiff_info &info, std::vector<tiff_src> &files)
{
    const bool seq = cli_frame_pattern(a.src) == 1;
    for (long k = 0; k < (seq ? want : 1); k++) {
        const std::string path = cli_frame_name(a.src, a.start_frame + k);
        const int fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) {
            if (k) break; /* the sequence ends here */
            printf("ERROR: unable to open file %s\n", path.c_str());
            return 1;
        }
        struct stat st;
        void *map = MAP_FAILED;
        if (!fstat(fd, &st) && st.st_size > 0) map = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (map == MAP_FAILED) { printf("ERROR: unable to map file %s\n", path.c_str()); return 1; }
        h2y_tiff_info ti;
        const char *why = nullptr;
        int rc = h2y_tiff_parse(map, (size_t)st.st_size, a.cutout, &ti, nullptr, 0, &why);
        tiff_src src{path, {}, false};
        if (!rc) {
            src.rows.resize((size_t)ti.height);
            rc = h2y_tiff_parse(map, (size_t)st.st_size, a.cutout, &ti, src.rows.data(), ti.height, &why);
        }
        munmap(map, (size_t)st.st_size);
        if (rc) { printf("ERROR: %s: %s\n", path.c_str(), why); return 1; }
        if (ti.width != a.in.width || ti.height != a.in.height) {
            printf("ERROR: %s decodes to %dx%d, --src_pic_width/--src_pic_height say %dx%d: resizing is not part of convert() (cv.cpp "
                   "is compiled out in the reference)\n", path.c_str(), ti.width, ti.height, a.in.width, a.in.height);
            return 1;
        }
        if (k && (ti.file_width != info.file_width || ti.file_height != info.file_height || ti.swap != info.swap)) {
            printf("ERROR: %s is %dx%d %s-endian, %s %dx%d %s-endian: every file of a sequence must have the same\n", path.c_str(),
                   ti.file_width, ti.file_height, ti.swap ? "big" : "little", files[0].path.c_str(), info.file_width, info.file_height,
                   info.swap ? "big" : "little");
            return 1;
        }
        if (!k && ti.swap)
            printf("WARNING: %s is big-endian (MM): decoded with the bytes of each sample exchanged; the reference reads them unswapped\n",
                   path.c_str());
        src.contiguous = ti.contiguous != 0;
        if (!k) info = ti;
        files.push_back(std::move(src));
    }
    return 0;
}

/* a whole file mapped read-only */
struct mapped_file {
    void *p = MAP_FAILED;
    size_t n = 0;
    bool open(const std::string &path)
    {
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (!fstat(fd, &st) && st.st_size > 0) {
            n = (size_t)st.st_size;
            p = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
        }
        close(fd);
        return p != MAP_FAILED;
    }
    ~mapped_file()
    {
        if (p != MAP_FAILED) munmap(p, n);
    }
};

/* The .exr files of the run, as dpx_scan: each mapped and parsed, its data window checked against the command line and its
 * header against the first file's (every file of a sequence has one h2y_exr_info).  Messages cite read_exr(). */
static int exr_scan(const cli_args &a, long want, h2y_exr_info &info, std::vector<std::string> &files)
{
    const bool seq = cli_frame_pattern(a.src) == 1;
    for (long k = 0; k < (seq ? want : 1); k++) {
        const std::string path = cli_frame_name(a.src, a.start_frame + k);
        mapped_file m;
        if (!m.open(path)) {
            if (k) break; /* the sequence ends here */
            printf("ERROR: read_exr() (exr.cpp:146): unable to open or read file %s\n", path.c_str());
            return 1;
        }
        h2y_exr_info xi;
        const char *why = nullptr;
        if (h2y_exr_parse(m.p, m.n, &xi, nullptr, 0, &why)) {
            printf("ERROR: read_exr() (exr.cpp): %s: %s\n", path.c_str(), why);
            return 1;
        }
        if (xi.width != a.in.width || xi.height != a.in.height) {
            printf("ERROR: read_exr() (exr.cpp:149-153): %s has a %dx%d data window, --src_pic_width/--src_pic_height say %dx%d: "
                   "resizing is not part of convert() (cv.cpp is compiled out in the reference)\n", path.c_str(), xi.width, xi.height,
                   a.in.width, a.in.height);
            return 1;
        }
        if (k && memcmp(&xi, &info, sizeof xi)) {
            printf("ERROR: read_exr() (exr.cpp): %s differs from %s in its data window, compression or channels: every file of a "
                   "sequence must have the same\n", path.c_str(), files[0].c_str());
            return 1;
        }
        if (!k) info = xi;
        files.push_back(path);
    }
    return 0;
}

/* The unpack threads of one GPU thread: h2y_exr_unpack of one frame's chunks, in ranges taken by the pool's threads and the
 * caller alike.  n counts the caller. */
class unpack_pool {
  public:
    explicit unpack_pool(int n)
    {
        for (int i = 1; i < n; i++) th_.emplace_back([this] { work(); });
    }
    ~unpack_pool()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            quit_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    int threads() const { return (int)th_.size() + 1; }
    /* the whole frame into payload: "" or the first error */
    std::string run(const h2y_exr_info &xi, const h2y_exr_chunk *chunks, const void *file, void *payload)
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            xi_ = &xi, chunks_ = chunks, file_ = file, payload_ = payload;
            step_ = std::max(1, xi.n_chunks / (4 * threads()));
            next_ = 0;
            err_.clear();
            busy_ = (int)th_.size();
            gen_++;
        }
        cv_.notify_all();
        take();
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [&] { return busy_ == 0; });
        return err_;
    }

  private:
    void take()
    {
        for (;;) {
            const int c0 = next_.fetch_add(step_);
            if (c0 >= xi_->n_chunks) return;
            const char *why = nullptr;
            if (h2y_exr_unpack(xi_, chunks_, file_, c0, std::min(step_, xi_->n_chunks - c0), payload_, &why)) {
                std::lock_guard<std::mutex> lk(m_);
                if (err_.empty()) err_ = why;
            }
        }
    }
    void work()
    {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return quit_ || gen_ != seen; });
                if (quit_) return;
                seen = gen_;
            }
            take();
            std::lock_guard<std::mutex> lk(m_);
            if (--busy_ == 0) done_.notify_one();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    bool quit_ = false;
    uint64_t gen_ = 0;
    int busy_ = 0, step_ = 1;
    std::atomic<int> next_{0};
    const h2y_exr_info *xi_ = nullptr;
    const h2y_exr_chunk *chunks_ = nullptr;
    const void *file_ = nullptr;
    void *payload_ = nullptr;
    std::string err_;
};

/* at most this many unpack threads in the whole process, the GPU threads that unpack included */
static constexpr int kUnpackThreads = 16;

/* n bytes at `at` of the open file fd into buf */
static bool read_at(int fd, void *buf, size_t n, off_t at)
{
    char *p = (char *)buf;
    while (n) {
        ssize_t r = pread(fd, p, n, at);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return false;
        p += r;
        at += r;
        n -= (size_t)r;
    }
    return true;
}

struct block { /* one thread's share: frames [first, first + count) of the run, on `device` */
    int device = 0;
    long first = 0, count = 0;
    std::string err;
    long done = 0;
};

/* frame k of the reference file into a ring's reference slot: the whole frame as the file holds it, or, for a .rgb (planes
 * R, G, B in the file), into the slot's G | B | R order */
static bool read_ref(FILE *f, bool rgb, size_t plane_bytes, size_t frame_bytes, void *ref)
{
    if (!rgb) return fread(ref, 1, frame_bytes, f) == frame_bytes;
    if (frame_bytes != 3 * plane_bytes) return false; /* a .rgb frame is three full planes: nothing else fits the slot */
    char *p = static_cast<char *>(ref);
    return fread(p + 2 * plane_bytes, 1, plane_bytes, f) == plane_bytes && fread(p, 1, 2 * plane_bytes, f) == 2 * plane_bytes;
}

/* the comparison side of one GPU thread: R opened at its frame `first`, the stats kept by frame index */
struct compare_io {
    std::vector<h2y_compare_stats> *stats = nullptr;
    FILE *ref = nullptr;
    bool rgb = false;
    size_t plane_bytes = 0, frame_bytes = 0;
    bool open(const cli_args &a, long first, size_t plane_b, size_t frame_b, std::vector<h2y_compare_stats> *st)
    {
        stats = st;
        if (!a.ref) return true;
        rgb = !strcasecmp(cli_ext_of(a.ref), "rgb");
        plane_bytes = plane_b, frame_bytes = frame_b;
        ref = fopen(a.ref, "rb");
        return ref && !fseeko(ref, (off_t)frame_b * (off_t)first, SEEK_SET);
    }
    ~compare_io()
    {
        if (ref) fclose(ref);
    }
};

/* the histogram side of one GPU thread: the stats and occupied bins of frame k kept by its index, the bins summed over its frames */
struct histogram_io {
    bool on = false;
    std::vector<h2y_histogram_stats> *stats = nullptr;
    std::vector<std::array<uint32_t, 3>> *occupied = nullptr;
    std::vector<uint32_t> bins;  /* one frame's 3 x nbins */
    std::vector<uint64_t> total; /* this thread's sums */
    size_t nbins = 0;
    void open(const cli_args &a, std::vector<h2y_histogram_stats> *st, std::vector<std::array<uint32_t, 3>> *occ)
    {
        on = a.hist != nullptr;
        if (!on) return;
        stats = st, occupied = occ;
        nbins = (size_t)1 << a.hist_bits;
        bins.assign(3 * nbins, 0u);
        total.assign(3 * nbins, 0u);
    }
    /* after h2y_stream_output: frame k's result */
    bool take(h2y_ctx *ctx, long k)
    {
        if (!on) return true;
        if (h2y_stream_histogram_result(ctx, &(*stats)[k], bins.data())) return false;
        for (int p = 0; p < 3; p++) {
            uint32_t occ = 0;
            for (size_t i = 0; i < nbins; i++) {
                const uint32_t c = bins[p * nbins + i];
                occ += c != 0u;
                total[p * nbins + i] += c;
            }
            (*occupied)[k][p] = occ;
        }
        return true;
    }
};

/* forward path: frames [first, first+count) through one context's pinned ring (dpx: frame k is file dpx[k], decoded on the
 * device -- the ring of h2y_dpx_stream_open; tiff likewise, file tiff[k] through h2y_tiff_stream_open) */
static void run_block(const cli_args &a, const h2y_desc &d, const std::vector<dpx_src> &dpx, const h2y_dpx_info &di,
                      const std::vector<tiff_src> &tiff, const h2y_tiff_info &ti, const std::vector<std::string> &exr,
                      const h2y_exr_info &xi, int fd_out, off_t base, std::vector<h2y_compare_stats> *stats,
                      std::vector<h2y_ssim_stats> *ssim, std::vector<h2y_light_stats> *light, histogram_io *hist, block *b)
{
    h2y_ctx *ctx = nullptr;
    FILE *fin = nullptr;
    auto fail = [&](const std::string &m) {
        b->err = m;
        if (ctx) { h2y_stream_close(ctx); h2y_ctx_destroy(ctx); }
        if (fin) fclose(fin);
    };
    if (b->count < 1) return;
    if (h2y_ctx_create(b->device, &ctx)) return fail(h2y_last_error(nullptr));
    const size_t pb = h2y_plane_bytes(&d), ob = h2y_frame_bytes(&d);
    if (a.in_type != CLI_IN_SYNTH && a.in_type != CLI_IN_DPX && a.in_type != CLI_IN_TIFF && a.in_type != CLI_IN_EXR) {
        fin = fopen(a.src, "rb");
        if (!fin) return fail(std::string("unable to open file ") + a.src);
        if (fseeko(fin, (off_t)(3 * pb) * (off_t)(a.start_frame + b->first), SEEK_SET)) return fail("seek failed"); /* hdr2yuv.cpp:624 */
    }
    /* The reader fills the pinned slot of the pipeline directly, the writer drains what comes out of it two frames
     * later: upload, conversion and download of neighbouring frames overlap. */
    const int depth = 3;
    const int open_rc = a.in_type == CLI_IN_DPX    ? h2y_dpx_stream_open(ctx, &d, &di, depth)
                        : a.in_type == CLI_IN_TIFF ? h2y_tiff_stream_open(ctx, &d, &ti, a.in.video_full_range_flag == 0, depth)
                        : a.in_type == CLI_IN_EXR  ? h2y_exr_stream_open(ctx, &d, &xi, depth)
                                                   : h2y_stream_open(ctx, &d, depth);
    if (open_rc) return fail(h2y_last_error(ctx));
    compare_io cmp;
    if (!cmp.open(a, b->first, 0, ob, stats)) return fail(std::string("unable to read ") + a.ref);
    if (cmp.ref && h2y_stream_compare(ctx, a.sigma, a.dst ? 1 : 0)) return fail(h2y_last_error(ctx));
    if (a.ssim && h2y_stream_ssim(ctx, -1)) return fail(h2y_last_error(ctx));
    if (hist->on && h2y_stream_histogram(ctx, a.hist_bits)) return fail(h2y_last_error(ctx));
    if (a.light && h2y_stream_light(ctx)) return fail(h2y_last_error(ctx));
    if (a.gamut && h2y_stream_gamut(ctx, a.in.colour_primaries, a.out.colour_primaries, a.gamut_clip)) return fail(h2y_last_error(ctx));
    if (a.scale && h2y_stream_scale(ctx, a.out.width, a.out.height, a.scale_taps)) return fail(h2y_last_error(ctx));
    const size_t wb = a.scale ? h2y_scale_frame_bytes(a.out.width, a.out.height, a.out.chroma_format_idc) : ob; /* what comes down */
    std::unique_ptr<unpack_pool> pool;
    std::vector<h2y_exr_chunk> chunks;
    if (a.in_type == CLI_IN_EXR) {
        pool.reset(new unpack_pool(std::max(1, kUnpackThreads / std::max(1, a.gpus))));
        chunks.resize((size_t)xi.n_chunks);
    }
    long in_flight = 0;
    auto drain_one = [&]() -> bool {
        const uint16_t *yuv = nullptr;
        if (h2y_stream_output(ctx, &yuv)) { fail(h2y_last_error(ctx)); return false; }
        const long k = b->first + b->done;
        if (cmp.ref && h2y_stream_compare_result(ctx, &(*cmp.stats)[k])) { fail(h2y_last_error(ctx)); return false; }
        if (a.ssim && h2y_stream_ssim_result(ctx, &(*ssim)[k])) { fail(h2y_last_error(ctx)); return false; }
        if (!hist->take(ctx, k)) { fail(h2y_last_error(ctx)); return false; }
        if (a.light && h2y_stream_light_result(ctx, &(*light)[k])) { fail(h2y_last_error(ctx)); return false; }
        if (a.dst && !write_at(fd_out, yuv, wb, base + (off_t)k * (off_t)wb)) { fail(std::string("short write to ") + a.dst); return false; }
        if (a.verbose > 0 && a.dst) printf("frame %ld: %zu bytes written to %s (device %d)\n", k, wb, a.dst, b->device);
        b->done++;
        in_flight--;
        return true;
    };
    for (long f = 0; f < b->count; f++) {
        void *planes[3];
        if (h2y_stream_input(ctx, planes)) return fail(h2y_last_error(ctx));
        if (a.in_type == CLI_IN_DPX) { /* the payload as the file holds it, straight into the pinned slot */
            const dpx_src &src = dpx[b->first + f];
            FILE *fd = fopen(src.path.c_str(), "rb");
            if (!fd) return fail("unable to open file " + src.path);
            size_t got = 0;
            if (!fseeko(fd, (off_t)src.offset, SEEK_SET)) got = fread(planes[0], 1, di.payload_bytes, fd);
            fclose(fd);
            if (got != di.payload_bytes) return fail("only " + std::to_string(got) + " payload bytes read from " + src.path);
        } else if (a.in_type == CLI_IN_TIFF) { /* the decoded rows, whole: one read when they lie back to back, else one per row */
            const tiff_src &src = tiff[b->first + f];
            const int fd = open(src.path.c_str(), O_RDONLY);
            if (fd < 0) return fail("unable to open file " + src.path);
            bool ok = true;
            char *dst = static_cast<char *>(planes[0]);
            if (src.contiguous) ok = read_at(fd, dst, ti.payload_bytes, (off_t)src.rows[0]);
            else
                for (size_t r = 0; ok && r < src.rows.size(); r++) ok = read_at(fd, dst + r * ti.row_bytes, ti.row_bytes, (off_t)src.rows[r]);
            close(fd);
            if (!ok) return fail("short read from " + src.path);
        } else if (a.in_type == CLI_IN_EXR) { /* parsed again (the file may have changed since the scan), unpacked into the slot */
            const std::string &path = exr[b->first + f];
            mapped_file m;
            if (!m.open(path)) return fail("read_exr() (exr.cpp:146): unable to open or read file " + path);
            h2y_exr_info x2;
            const char *why = nullptr;
            if (h2y_exr_parse(m.p, m.n, &x2, chunks.data(), xi.n_chunks, &why)) return fail("read_exr() (exr.cpp): " + path + ": " + why);
            if (memcmp(&x2, &xi, sizeof xi)) return fail("read_exr() (exr.cpp): " + path + " no longer has the header the run started with");
            const std::string err = pool->run(xi, chunks.data(), m.p, planes[0]);
            if (!err.empty()) return fail("read_exr() (exr.cpp): " + path + ": " + err);
        } else if (fin) {
            /* file plane order -> memory planes (0=G/Y, 1=B/Cb, 2=R/Cr); .rgb holds R,G,B (hdr2yuv.cpp:635-637) */
            const int order_rgb[3] = {2, 0, 1}, order_nat[3] = {0, 1, 2};
            const int *ord = a.in_type == CLI_IN_RGB ? order_rgb : order_nat;
            size_t got = 0;
            for (int k = 0; k < 3; k++) got += fread(planes[ord[k]], 1, pb, fin);
            if (got != 3 * pb) return fail("only " + std::to_string(got) + " bytes read from " + a.src + ", expecting " + std::to_string(3 * pb));
        } else synth_fill(d, planes, 12345u + (uint32_t)(a.synthetic + a.start_frame + b->first + f));
        if (cmp.ref) {
            void *ref = nullptr;
            if (h2y_stream_reference(ctx, &ref)) return fail(h2y_last_error(ctx));
            if (!read_ref(cmp.ref, false, 0, ob, ref)) return fail(std::string("short read from ") + a.ref);
        }
        if (h2y_stream_submit(ctx)) return fail(h2y_last_error(ctx));
        in_flight++;
        if (in_flight == depth - 1 && !drain_one()) return;
    }
    while (in_flight > 0)
        if (!drain_one()) return;
    h2y_stream_close(ctx);
    if (fin) fclose(fin);
    h2y_ctx_destroy(ctx);
}

/* the bytes libtiff writes around write_tiff()'s samples (h2y_tiff_layout) */
struct tiff_wrap {
    uint8_t head[8];
    std::vector<uint8_t> tail;
};

/* .yuv -> RGB (matrix_inverse): frames [first, first+count) through one context's pinned inverse ring, as run_block; .tiff
 * output: the ring with the interleave (h2y_tiff_inverse_stream_open), frame k into its own file, head + samples + tail */
static void run_block_inverse(const cli_args &a, const tiff_wrap &tw, int fd_out, off_t base, std::vector<h2y_compare_stats> *stats,
                              std::vector<h2y_ssim_stats> *ssim, histogram_io *hist, block *b)
{
    h2y_ctx *ctx = nullptr;
    FILE *fin = nullptr;
    auto fail = [&](const std::string &m) {
        b->err = m;
        if (ctx) { h2y_stream_close(ctx); h2y_ctx_destroy(ctx); }
        if (fin) fclose(fin);
    };
    if (b->count < 1) return;
    if (h2y_ctx_create(b->device, &ctx)) return fail(h2y_last_error(nullptr));
    const size_t n = (size_t)a.in.width * a.in.height;
    const bool sub = a.in.chroma_format_idc == H2Y_CHROMA_420;
    const size_t nc = sub ? (size_t)(a.in.width / 2) * (a.in.height / 2) : n, in_frame = (n + 2 * nc) * 2, out_frame = 3 * n * 2;
    fin = fopen(a.src, "rb");
    if (!fin) return fail(std::string("unable to open file ") + a.src);
    if (fseeko(fin, (off_t)in_frame * (off_t)(a.start_frame + b->first), SEEK_SET)) return fail("seek failed");
    const int depth = 3;
    const bool tiff = a.out_type == CLI_OUT_TIFF;
    if ((tiff ? h2y_tiff_inverse_stream_open : h2y_inverse_stream_open)(ctx, a.in.width, a.in.height, a.in.chroma_format_idc,
                                                                       a.in.bit_depth, a.in.video_full_range_flag, a.in.matrix_coeffs,
                                                                       a.out.bit_depth, a.resampler, depth))
        return fail(h2y_last_error(ctx));
    compare_io cmp;
    if (!cmp.open(a, b->first, 2 * n, out_frame, stats)) return fail(std::string("unable to read ") + a.ref);
    if (cmp.ref && h2y_stream_compare(ctx, a.sigma, a.dst ? 1 : 0)) return fail(h2y_last_error(ctx));
    if (a.ssim && h2y_stream_ssim(ctx, -1)) return fail(h2y_last_error(ctx));
    if (hist->on && h2y_stream_histogram(ctx, a.hist_bits)) return fail(h2y_last_error(ctx));
    long in_flight = 0;
    auto drain_one = [&]() -> bool {
        const uint16_t *gbr = nullptr;
        if (h2y_stream_output(ctx, &gbr)) { fail(h2y_last_error(ctx)); return false; }
        const long k = b->first + b->done;
        if (cmp.ref && h2y_stream_compare_result(ctx, &(*cmp.stats)[k])) { fail(h2y_last_error(ctx)); return false; }
        if (a.ssim && h2y_stream_ssim_result(ctx, &(*ssim)[k])) { fail(h2y_last_error(ctx)); return false; }
        if (!hist->take(ctx, k)) { fail(h2y_last_error(ctx)); return false; }
        if (!a.dst) {
            b->done++;
            in_flight--;
            return true;
        }
        if (tiff) { /* TIFFOpen(filename, "w"): a new file */
            const std::string path = cli_frame_name(a.dst, a.start_frame + k);
            const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
            const bool ok = fd >= 0 && write_at(fd, tw.head, sizeof tw.head, 0) && write_at(fd, gbr, out_frame, sizeof tw.head) &&
                            write_at(fd, tw.tail.data(), tw.tail.size(), (off_t)(sizeof tw.head + out_frame));
            if (fd >= 0) close(fd);
            if (!ok) { fail("unable to write " + path); return false; }
            b->done++;
            in_flight--;
            return true;
        }
        const off_t at = base + (off_t)k * (off_t)out_frame;
        /* planes G, B, R -> file order R, G, B (write_tiff: R, G, B per pixel) */
        if (!write_at(fd_out, gbr + 2 * n, 2 * n, at) || !write_at(fd_out, gbr, 4 * n, at + (off_t)(2 * n))) {
            fail(std::string("short write to ") + a.dst);
            return false;
        }
        b->done++;
        in_flight--;
        return true;
    };
    for (long f = 0; f < b->count; f++) {
        void *planes[3];
        if (h2y_stream_input(ctx, planes)) return fail(h2y_last_error(ctx));
        size_t got = fread(planes[0], 1, 2 * n, fin);
        got += fread(planes[1], 1, 2 * nc, fin);
        got += fread(planes[2], 1, 2 * nc, fin);
        if (got != in_frame) return fail(std::string("short read from ") + a.src);
        if (cmp.ref) {
            void *ref = nullptr;
            if (h2y_stream_reference(ctx, &ref)) return fail(h2y_last_error(ctx));
            if (!read_ref(cmp.ref, true, 2 * n, out_frame, ref)) return fail(std::string("short read from ") + a.ref);
        }
        if (h2y_stream_submit(ctx)) return fail(h2y_last_error(ctx));
        in_flight++;
        if (in_flight == depth - 1 && !drain_one()) return;
    }
    while (in_flight > 0)
        if (!drain_one()) return;
    h2y_stream_close(ctx);
    fclose(fin);
    h2y_ctx_destroy(ctx);
}

/* --compare_only: frames [first, first+count) of the source against the same frames of R through one compare-only ring */
static void run_block_compare(const cli_args &a, size_t plane_bytes, size_t frame_bytes, std::vector<h2y_compare_stats> *stats,
                              std::vector<h2y_ssim_stats> *ssim, histogram_io *hist, block *b)
{
    h2y_ctx *ctx = nullptr;
    FILE *fin = nullptr;
    auto fail = [&](const std::string &m) {
        b->err = m;
        if (ctx) { h2y_stream_close(ctx); h2y_ctx_destroy(ctx); }
        if (fin) fclose(fin);
    };
    if (b->count < 1) return;
    if (h2y_ctx_create(b->device, &ctx)) return fail(h2y_last_error(nullptr));
    fin = fopen(a.src, "rb");
    if (!fin) return fail(std::string("unable to open file ") + a.src);
    if (fseeko(fin, (off_t)frame_bytes * (off_t)(a.start_frame + b->first), SEEK_SET)) return fail("seek failed");
    compare_io cmp;
    if (!cmp.open(a, b->first, plane_bytes, frame_bytes, stats)) return fail(std::string("unable to read ") + a.ref);
    const int depth = 3;
    if (h2y_compare_stream_open(ctx, a.in.width, a.in.height, a.in.chroma_format_idc, a.sigma, depth)) return fail(h2y_last_error(ctx));
    if (a.ssim && h2y_stream_ssim(ctx, a.in.bit_depth)) return fail(h2y_last_error(ctx));
    if (hist->on && h2y_stream_histogram_ex(ctx, a.hist_bits, a.hist_depth, a.hist_full, a.hist_gbr)) return fail(h2y_last_error(ctx));
    long in_flight = 0;
    auto drain_one = [&]() -> bool {
        const uint16_t *none = nullptr;
        const long k = b->first + b->done;
        if (h2y_stream_output(ctx, &none) || h2y_stream_compare_result(ctx, &(*stats)[k]) ||
            (a.ssim && h2y_stream_ssim_result(ctx, &(*ssim)[k])) || !hist->take(ctx, k)) {
            fail(h2y_last_error(ctx));
            return false;
        }
        b->done++;
        in_flight--;
        return true;
    };
    for (long f = 0; f < b->count; f++) {
        void *planes[3], *ref = nullptr;
        if (h2y_stream_input(ctx, planes) || h2y_stream_reference(ctx, &ref)) return fail(h2y_last_error(ctx));
        /* the slot's planes lie one after the other: a frame is one read, a .rgb one with its planes put in G, B, R order */
        if (!read_ref(fin, cmp.rgb, plane_bytes, frame_bytes, planes[0])) return fail(std::string("short read from ") + a.src);
        if (!read_ref(cmp.ref, cmp.rgb, plane_bytes, frame_bytes, ref)) return fail(std::string("short read from ") + a.ref);
        if (h2y_stream_submit(ctx)) return fail(h2y_last_error(ctx));
        in_flight++;
        if (in_flight == depth - 1 && !drain_one()) return;
    }
    while (in_flight > 0)
        if (!drain_one()) return;
    h2y_stream_close(ctx);
    fclose(fin);
    h2y_ctx_destroy(ctx);
}

/* --histogram_only: frames [first, first+count) of the source through one histogram-only ring */
static void run_block_histogram(const cli_args &a, size_t plane_bytes, size_t frame_bytes, histogram_io *hist, block *b)
{
    h2y_ctx *ctx = nullptr;
    FILE *fin = nullptr;
    auto fail = [&](const std::string &m) {
        b->err = m;
        if (ctx) { h2y_stream_close(ctx); h2y_ctx_destroy(ctx); }
        if (fin) fclose(fin);
    };
    if (b->count < 1) return;
    if (h2y_ctx_create(b->device, &ctx)) return fail(h2y_last_error(nullptr));
    fin = fopen(a.src, "rb");
    if (!fin) return fail(std::string("unable to open file ") + a.src);
    if (fseeko(fin, (off_t)frame_bytes * (off_t)(a.start_frame + b->first), SEEK_SET)) return fail("seek failed");
    const int depth = 3;
    if (h2y_histogram_stream_open(ctx, a.in.width, a.in.height, a.in.chroma_format_idc, a.hist_depth, a.hist_full, a.hist_gbr, a.hist_bits,
                                  depth))
        return fail(h2y_last_error(ctx));
    const bool rgb = a.in_type == CLI_IN_RGB;
    long in_flight = 0;
    auto drain_one = [&]() -> bool {
        const uint16_t *none = nullptr;
        const long k = b->first + b->done;
        if (h2y_stream_output(ctx, &none) || !hist->take(ctx, k)) { fail(h2y_last_error(ctx)); return false; }
        b->done++;
        in_flight--;
        return true;
    };
    for (long f = 0; f < b->count; f++) {
        void *planes[3];
        if (h2y_stream_input(ctx, planes)) return fail(h2y_last_error(ctx));
        /* the slot's planes lie one after the other: a frame is one read, a .rgb one with its planes put in G, B, R order */
        if (!read_ref(fin, rgb, plane_bytes, frame_bytes, planes[0])) return fail(std::string("short read from ") + a.src);
        if (h2y_stream_submit(ctx)) return fail(h2y_last_error(ctx));
        in_flight++;
        if (in_flight == depth - 1 && !drain_one()) return;
    }
    while (in_flight > 0)
        if (!drain_one()) return;
    h2y_stream_close(ctx);
    fclose(fin);
    h2y_ctx_destroy(ctx);
}

/* --scale_only: frames [first, first+count) of the source through one scale-only ring into the destination */
static void run_block_scale(const cli_args &a, size_t plane_bytes, size_t frame_bytes, size_t out_bytes, int fd_out, off_t base, block *b)
{
    h2y_ctx *ctx = nullptr;
    FILE *fin = nullptr;
    auto fail = [&](const std::string &m) {
        b->err = m;
        if (ctx) { h2y_stream_close(ctx); h2y_ctx_destroy(ctx); }
        if (fin) fclose(fin);
    };
    if (b->count < 1) return;
    if (h2y_ctx_create(b->device, &ctx)) return fail(h2y_last_error(nullptr));
    fin = fopen(a.src, "rb");
    if (!fin) return fail(std::string("unable to open file ") + a.src);
    if (fseeko(fin, (off_t)frame_bytes * (off_t)(a.start_frame + b->first), SEEK_SET)) return fail("seek failed");
    const int depth = 3;
    const bool rgb = a.in_type == CLI_IN_RGB;
    if (h2y_scale_stream_open(ctx, a.in.width, a.in.height, a.in.chroma_format_idc, a.in.bit_depth, a.in.video_full_range_flag, rgb ? 1 : 0,
                              a.out.width, a.out.height, a.scale_taps, depth))
        return fail(h2y_last_error(ctx));
    const size_t on = (size_t)a.out.width * a.out.height * 2; /* bytes of one full output plane */
    long in_flight = 0;
    auto drain_one = [&]() -> bool {
        const uint16_t *out = nullptr;
        if (h2y_stream_output(ctx, &out)) { fail(h2y_last_error(ctx)); return false; }
        const long k = b->first + b->done;
        const off_t at = base + (off_t)k * (off_t)out_bytes;
        const char *p = reinterpret_cast<const char *>(out);
        /* a .rgb: planes G, B, R -> file order R, G, B */
        const bool ok = rgb ? write_at(fd_out, p + 2 * on, on, at) && write_at(fd_out, p, 2 * on, at + (off_t)on) : write_at(fd_out, p, out_bytes, at);
        if (!ok) { fail(std::string("short write to ") + a.dst); return false; }
        if (a.verbose > 0) printf("frame %ld: %zu bytes written to %s (device %d)\n", k, out_bytes, a.dst, b->device);
        b->done++;
        in_flight--;
        return true;
    };
    for (long f = 0; f < b->count; f++) {
        void *planes[3];
        if (h2y_stream_input(ctx, planes)) return fail(h2y_last_error(ctx));
        /* the slot's planes lie one after the other: a frame is one read, a .rgb one with its planes put in G, B, R order */
        if (!read_ref(fin, rgb, plane_bytes, frame_bytes, planes[0])) return fail(std::string("short read from ") + a.src);
        if (h2y_stream_submit(ctx)) return fail(h2y_last_error(ctx));
        in_flight++;
        if (in_flight == depth - 1 && !drain_one()) return;
    }
    while (in_flight > 0)
        if (!drain_one()) return;
    h2y_stream_close(ctx);
    fclose(fin);
    h2y_ctx_destroy(ctx);
}

/* the histogram report of the header comment and FILE; returns the exit status (4: --check_range 1 and samples outside) */
static int histogram_report(const cli_args &a, const std::vector<h2y_histogram_stats> &st, const std::vector<std::array<uint32_t, 3>> &occ,
                            const std::vector<uint64_t> &total)
{
    static const char *const kYuv[3] = {"Y", "Cb", "Cr"}, *const kRgb[3] = {"G", "B", "R"};
    const char *const *name = a.hist_gbr ? kRgb : kYuv;
    const size_t nbins = (size_t)1 << a.hist_bits;
    uint64_t below[3] = {0, 0, 0}, above[3] = {0, 0, 0}, at_low[3] = {0, 0, 0}, at_high[3] = {0, 0, 0};
    uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0, 0, 0};
    auto plane = [&](int p, uint32_t lo, uint32_t hi, uint64_t b, uint64_t ab, uint64_t l, uint64_t h, uint32_t o) {
        printf(" %s min %u max %u below %llu above %llu at_low %llu at_high %llu occupied %u", name[p], lo, hi, (unsigned long long)b,
               (unsigned long long)ab, (unsigned long long)l, (unsigned long long)h, o);
    };
    for (size_t k = 0; k < st.size(); k++) {
        const h2y_histogram_stats &s = st[k];
        printf("histogram frame %zu", k);
        for (int p = 0; p < 3; p++) {
            plane(p, s.min[p], s.max[p], s.below[p], s.above[p], s.at_low[p], s.at_high[p], occ[k][p]);
            below[p] += s.below[p], above[p] += s.above[p], at_low[p] += s.at_low[p], at_high[p] += s.at_high[p];
            if (s.samples[p]) mn[p] = std::min(mn[p], s.min[p]), mx[p] = std::max(mx[p], s.max[p]);
        }
        printf("\n");
    }
    printf("histogram summary frames %zu", st.size());
    uint64_t outside = 0;
    for (int p = 0; p < 3; p++) {
        uint32_t o = 0;
        for (size_t i = 0; i < nbins; i++) o += total[p * nbins + i] != 0u;
        plane(p, mn[p] == 0xFFFFFFFFu ? 0u : mn[p], mx[p], below[p], above[p], at_low[p], at_high[p], o);
        outside += below[p] + above[p];
    }
    printf("\nhistogram legal");
    for (int p = 0; p < 3; p++) printf(" %s %u..%u", name[p], st.empty() ? 0u : st[0].lo[p], st.empty() ? 0u : st[0].hi[p]);
    printf(" outside %llu\n", (unsigned long long)outside);
    FILE *f = fopen(a.hist, "w");
    if (!f) {
        printf("ERROR: unable to write %s\n", a.hist);
        return 1;
    }
    const uint32_t shift = (uint32_t)(a.hist_depth - a.hist_bits);
    fprintf(f, "bin,code_lo,code_hi,%s,%s,%s\n", name[0], name[1], name[2]);
    for (size_t i = 0; i < nbins; i++)
        fprintf(f, "%zu,%zu,%zu,%llu,%llu,%llu\n", i, i << shift, ((i + 1) << shift) - 1, (unsigned long long)total[i],
                (unsigned long long)total[nbins + i], (unsigned long long)total[2 * nbins + i]);
    if (fclose(f)) {
        printf("ERROR: unable to write %s\n", a.hist);
        return 1;
    }
    return a.check_range && outside ? 4 : 0;
}

static std::string psnr_str(uint64_t maxv, uint64_t n, uint64_t sse)
{
    if (sse == 0) return "inf";
    char buf[64];
    snprintf(buf, sizeof buf, "%.4f", 10.0 * log10((double)maxv * maxv * n / sse));
    return buf;
}

/* the report of the header comment; returns the exit status (3: over-sigma samples with --sigma_compare given) */
static int compare_report(const cli_args &a, bool yuv, int bit_depth, const std::vector<h2y_compare_stats> &st)
{
    static const char *const kYuv[3] = {"Y", "Cb", "Cr"}, *const kRgb[3] = {"G", "B", "R"};
    const char *const *name = yuv ? kYuv : kRgb;
    const uint64_t maxv = (1ull << bit_depth) - 1;
    uint64_t n[3] = {0, 0, 0}, sse[3] = {0, 0, 0}, over[3] = {0, 0, 0};
    uint32_t mx[3] = {0, 0, 0};
    double mean[3] = {0, 0, 0};
    long first_f = -1;
    int first_p = -1;
    for (size_t k = 0; k < st.size(); k++) {
        const h2y_compare_stats &s = st[k];
        printf("frame %zu psnr", k);
        for (int p = 0; p < 3; p++) printf(" %s %s", name[p], psnr_str(maxv, s.samples[p], s.sse[p]).c_str());
        printf(" max_abs %u %u %u over %llu %llu %llu\n", s.max_abs[0], s.max_abs[1], s.max_abs[2], (unsigned long long)s.over[0],
               (unsigned long long)s.over[1], (unsigned long long)s.over[2]);
        for (int p = 0; p < 3; p++) {
            n[p] += s.samples[p], sse[p] += s.sse[p], over[p] += s.over[p];
            mx[p] = std::max(mx[p], s.max_abs[p]);
            mean[p] += s.sse[p] ? 10.0 * log10((double)maxv * maxv * s.samples[p] / s.sse[p]) : 99.99;
            if (first_f < 0 && s.over[p]) first_f = (long)k, first_p = p;
        }
    }
    printf("summary frames %zu mean_psnr", st.size());
    for (int p = 0; p < 3; p++) printf(" %s %.4f", name[p], st.empty() ? 0.0 : mean[p] / (double)st.size());
    printf(" global_psnr");
    for (int p = 0; p < 3; p++) printf(" %s %s", name[p], psnr_str(maxv, n[p], sse[p]).c_str());
    printf(" max_abs %u %u %u over %llu %llu %llu\n", mx[0], mx[1], mx[2], (unsigned long long)over[0], (unsigned long long)over[1],
           (unsigned long long)over[2]);
    if (first_f < 0) printf("first_over none\n");
    else {
        const h2y_compare_stats &s = st[(size_t)first_f];
        const bool sub = yuv && a.out.chroma_format_idc == H2Y_CHROMA_420 && first_p > 0;
        const uint64_t w = sub ? (uint64_t)(a.out.width >> 1) : (uint64_t)a.out.width, i = (uint64_t)s.first_over[first_p];
        printf("first_over frame %ld plane %s x %llu y %llu a %u b %u\n", first_f, name[first_p], (unsigned long long)(i % w),
               (unsigned long long)(i / w), s.first_a[first_p], s.first_b[first_p]);
    }
    return a.sigma_given && first_f >= 0 ? 3 : 0;
}

static std::string ssim_db(double x)
{
    if (x >= 1.0) return "inf";
    char s[32];
    snprintf(s, sizeof s, "%.4f", -10.0 * log10(1.0 - x));
    return s;
}

/* the SSIM report of the header comment */
static void ssim_report(bool yuv, const std::vector<h2y_ssim_stats> &st)
{
    static const char *const kYuv[3] = {"Y", "Cb", "Cr"}, *const kRgb[3] = {"G", "B", "R"};
    const char *const *name = yuv ? kYuv : kRgb;
    auto line = [&](const double (&v)[3], double all) {
        for (int p = 0; p < 3; p++) printf(" %s %.6f", name[p], v[p]);
        printf(" all %.6f db", all);
        for (int p = 0; p < 3; p++) printf(" %s %s", name[p], ssim_db(v[p]).c_str());
        printf(" all %s\n", ssim_db(all).c_str());
    };
    double mean[3] = {0, 0, 0}, mean_all = 0;
    size_t worst = 0;
    for (size_t k = 0; k < st.size(); k++) {
        printf("ssim frame %zu", k);
        line(st[k].ssim, st[k].all);
        for (int p = 0; p < 3; p++) mean[p] += st[k].ssim[p];
        mean_all += st[k].all;
        if (st[k].all < st[worst].all) worst = k;
    }
    if (st.empty()) return;
    for (int p = 0; p < 3; p++) mean[p] /= (double)st.size();
    printf("ssim summary frames %zu", st.size());
    line(mean, mean_all / (double)st.size());
    printf("ssim worst frame %zu all %.6f\n", worst, st[worst].all);
}

/* the content light report of the header comment */
static void light_report(const std::vector<h2y_light_stats> &st)
{
    size_t kc = 0, kf = 0;
    for (size_t k = 0; k < st.size(); k++) {
        printf("light frame %zu peak %.4f at %u %u average %.4f\n", k, st[k].cll, st[k].x, st[k].y, st[k].fall);
        if (st[k].cll > st[kc].cll) kc = k;
        if (st[k].fall > st[kf].fall) kf = k;
    }
    if (st.empty()) return;
    const long long cll = llround(st[kc].cll), fall = llround(st[kf].fall);
    printf("light summary frames %zu maxcll %lld frame %zu maxfall %lld frame %zu\n", st.size(), cll, kc, fall, kf);
    printf("light x265 --max-cll \"%lld,%lld\"\n", cll, fall);
    printf("light svt-av1 --content-light %lld,%lld\n", cll, fall);
}

int main(int argc, char **argv)
{
    cli_args a;
    cli_parse(a, argc, argv);
    if ((!a.dst && !a.ref && !a.hist && !a.hist_only && !a.light && !a.scale_only) || (!a.src && a.synthetic < 0)) {
        if (!a.help) cli_help();
        return a.help ? 0 : 1;
    }
    if (cli_resolve(a)) {
        printf("TOO MANY ARGUMENT ERRORS. ABORTING PROGRAM. --help to show options\n\n"); /* hdr2yuv.cpp:567-572 (which exits 0) */
        return 1;
    }
    /* read_exr() runs before anything else is checked and takes the size from the file: a dry run reads the .exr too */
    std::vector<std::string> exr;
    h2y_exr_info xi{};
    if (a.in_type == CLI_IN_EXR) {
        if (exr_scan(a, a.n_frames > 0 ? a.n_frames : 1, xi, exr)) return 1;
        static const char *const kComp[] = {"NONE", "RLE", "ZIPS", "ZIP"};
        printf("exr: %dx%d data window at (%d, %d), %s, %s y, %d channels, %d unpack threads per GPU\n", xi.width, xi.height, xi.x_min,
               xi.y_min, kComp[xi.compression], xi.line_order ? "decreasing" : "increasing", xi.n_channels,
               std::max(1, kUnpackThreads / std::max(1, a.gpus)));
        printf("src_picture: matrix_coeffs %d chroma_format_idc %d bit_depth %d video_full_range_flag %d\n", a.in.matrix_coeffs,
               a.in.chroma_format_idc, a.in.bit_depth, a.in.video_full_range_flag);
    }
    const bool scaling = a.scale == 1 || a.scale_only == 1;
    if (!scaling && (a.out.width != a.in.width || a.out.height != a.in.height)) {
        printf("ERROR: resizing is not part of convert() (cv.cpp is compiled out in the reference); --scale 1 resamples the .yuv frames on "
               "the GPU\n");
        return 1;
    }
    h2y_desc d;
    cli_make_desc(a, &d);
    size_t in_frame_bytes, out_frame_bytes;
    if (a.compare_only || a.hist_only || a.scale_only) { /* two files of one layout, or one */
        const size_t n = (size_t)a.in.width * a.in.height;
        const size_t nc = a.in.chroma_format_idc == H2Y_CHROMA_420 ? (size_t)(a.in.width / 2) * (a.in.height / 2) : n;
        in_frame_bytes = out_frame_bytes = (n + 2 * nc) * 2;
    } else if (a.inverse) {
        if (a.out.bit_depth > 16 || a.in.bit_depth > 16) { printf("ERROR: bit depths must be 8..16 on the inverse flow\n"); return 1; }
        if (a.out.bit_depth < a.in.bit_depth) { /* tiff.cpp:564: SR = dst - src depth, then `R << SR` */
            printf("ERROR: dst bit_depth(%d) < src bit_depth(%d): write_tiff() would shift by a negative count (undefined in the reference)\n", a.out.bit_depth, a.in.bit_depth);
            return 1;
        }
        const size_t n = (size_t)a.in.width * a.in.height;
        const size_t nc = a.in.chroma_format_idc == H2Y_CHROMA_420 ? (size_t)(a.in.width / 2) * (a.in.height / 2) : n;
        in_frame_bytes = (n + 2 * nc) * 2;
        out_frame_bytes = 3 * n * 2;
    } else {
        const char *why = nullptr;
        if (h2y_desc_check(&d, &why)) { printf("ERROR: %s\n", why); return 1; }
        in_frame_bytes = 3 * h2y_plane_bytes(&d);
        out_frame_bytes = h2y_frame_bytes(&d);
    }
    if (scaling) out_frame_bytes = h2y_scale_frame_bytes(a.out.width, a.out.height, a.out.chroma_format_idc); /* the scaled frame's */

    /* how many frames there are to do: --n_frames, or what the file holds from --src_start_frame on if that is fewer */
    long frames = a.n_frames > 0 ? a.n_frames : 1;
    struct stat st;
    std::vector<dpx_src> dpx;
    h2y_dpx_info di{};
    std::vector<tiff_src> tiff;
    h2y_tiff_info ti{};
    if (a.in_type == CLI_IN_EXR) frames = (long)exr.size();
    else if (a.in_type == CLI_IN_TIFF) { /* as .dpx */
        if (!(a.dry_run && stat(cli_frame_name(a.src, a.start_frame).c_str(), &st))) {
            if (tiff_scan(a, frames, ti, tiff)) return 1;
            frames = (long)tiff.size();
            printf("tiff: %dx%d %s-endian, %d rows per strip, decoded %dx%d from (%d, %d), rows %s\n", ti.file_width, ti.file_height,
                   ti.swap ? "big" : "little", ti.rows_per_strip, ti.width, ti.height, ti.x0, ti.y0,
                   ti.contiguous ? "contiguous" : "scattered");
        }
        printf("src_picture: matrix_coeffs %d chroma_format_idc %d bit_depth %d video_full_range_flag %d\n", a.in.matrix_coeffs,
               a.in.chroma_format_idc, a.in.bit_depth, a.in.video_full_range_flag);
    } else if (a.in_type == CLI_IN_DPX) { /* one file per frame; a dry run may name a file that is not there */
        if (!(a.dry_run && stat(cli_frame_name(a.src, a.start_frame).c_str(), &st))) {
            if (dpx_scan(a, frames, di, dpx)) return 1;
            frames = (long)dpx.size();
            printf("dpx: %dx%d %d-bit %s-endian, payload %llu bytes\n", di.width, di.height, di.bit_size, di.swap ? "big" : "little",
                   (unsigned long long)di.payload_bytes);
        }
        printf("src_picture: matrix_coeffs %d chroma_format_idc %d bit_depth %d video_full_range_flag %d\n", a.in.matrix_coeffs,
               a.in.chroma_format_idc, a.in.bit_depth, a.in.video_full_range_flag);
    } else if (a.in_type != CLI_IN_SYNTH && !(a.dry_run && stat(a.src, &st))) { /* (a dry run may name a file that is not there) */
        if (stat(a.src, &st)) { printf("ERROR: unable to open file %s\n", a.src); return 1; }
        const long have = (long)((st.st_size - (off_t)in_frame_bytes * a.start_frame) / (off_t)in_frame_bytes);
        if (st.st_size < (off_t)in_frame_bytes * (a.start_frame + 1)) {
            printf("ERROR: only %lld bytes in %s, expecting %zu from frame %d on\n", (long long)st.st_size, a.src, in_frame_bytes, a.start_frame);
            return 1;
        }
        if (frames > have) frames = have;
    }
    if (a.gpus < 1) a.gpus = 1;
    if (a.devices.empty()) {
        if (a.gpus == 1) a.devices.push_back(a.device);
        else for (int r = 0; r < a.gpus; r++) a.devices.push_back(r);
    }
    if ((int)a.devices.size() != a.gpus) { printf("ERROR: --devices names %zu devices, --gpus %d\n", a.devices.size(), a.gpus); return 1; }
    printf("gpus: %d (devices", a.gpus);
    for (int dv : a.devices) printf(" %d", dv);
    printf(")\nframes: %ld\nframe_bytes: %zu\n", frames, out_frame_bytes);
    /* R in the layout of what the run produces: a whole number of frames, at least as many as the run has */
    const bool cmp_yuv = a.compare_only ? a.in_type == CLI_IN_YUV : a.out_type == CLI_OUT_YUV;
    if (a.ref) {
        if (!stat(a.ref, &st)) {
            if (st.st_size % (off_t)out_frame_bytes) {
                printf("WARNING: reference file (%s): %lld bytes is not a whole number of %zu-byte frames\n", a.ref, (long long)st.st_size,
                       out_frame_bytes);
                return 1;
            }
            if (st.st_size / (off_t)out_frame_bytes < frames) {
                printf("WARNING: reference file (%s) holds %lld frames, the run produces %ld\n", a.ref,
                       (long long)(st.st_size / (off_t)out_frame_bytes), frames);
                return 1;
            }
        } else if (!a.dry_run) { printf("ERROR: unable to open file %s\n", a.ref); return 1; }
        printf("compare: %s %dx%d chroma_format_idc %d bit_depth %d planes %s, %ld frames against %s, sigma %d, output %s\n",
               cmp_yuv ? "yuv" : "rgb", a.out.width, a.out.height, cmp_yuv ? a.out.chroma_format_idc : H2Y_CHROMA_444, a.out.bit_depth,
               cmp_yuv ? "Y,Cb,Cr" : "G,B,R", frames, a.ref, a.sigma, a.compare_only ? "none (compare only)" : a.dst ? "kept" : "none (not written)");
    }
    tiff_wrap tw;
    if (a.out_type == CLI_OUT_TIFF) {
        if (frames > 1 && cli_frame_pattern(a.dst) != 1) {
            printf("ERROR: %ld frames into one .tiff: a .tiff holds one frame; name them with one integer conversion (shot.%%06d.tiff)\n",
                   frames);
            return 1;
        }
        size_t tb = 0;
        if (h2y_tiff_layout(a.in.width, a.in.height, tw.head, nullptr, &tb)) { printf("ERROR: %s\n", h2y_last_error(nullptr)); return 1; }
        tw.tail.resize(tb);
        if (h2y_tiff_layout(a.in.width, a.in.height, tw.head, tw.tail.data(), &tb)) { printf("ERROR: %s\n", h2y_last_error(nullptr)); return 1; }
        printf("tiff_file_bytes: %zu\n", sizeof tw.head + out_frame_bytes + tb);
    }
    if (a.dry_run) return 0;

    /* tiff.cpp:440 opens ios::ate | ios::app: what is in the file stays, frames go behind it (.tiff: one file per frame, below) */
    int fd = -1;
    off_t base = 0;
    if (a.dst && a.out_type != CLI_OUT_TIFF) {
        fd = open(a.dst, O_WRONLY | O_CREAT, 0644);
        if (fd < 0) { printf("ERROR: unable to open %s\n", a.dst); return 1; }
        base = lseek(fd, 0, SEEK_END);
    }

    /* contiguous blocks of frame indices, the first `frames % gpus` one longer (hdr2yuv_amd/shard.py) */
    std::vector<block> blocks(a.gpus);
    long at = 0;
    for (int r = 0; r < a.gpus; r++) {
        blocks[r].device = a.devices[r];
        blocks[r].first = at;
        blocks[r].count = frames / a.gpus + (r < frames % a.gpus ? 1 : 0);
        at += blocks[r].count;
    }
    std::vector<h2y_compare_stats> stats(a.ref ? (size_t)frames : 0);
    std::vector<h2y_ssim_stats> sstats(a.ssim ? (size_t)frames : 0);
    std::vector<h2y_light_stats> lstats(a.light ? (size_t)frames : 0);
    std::vector<h2y_histogram_stats> hstats(a.hist ? (size_t)frames : 0);
    std::vector<std::array<uint32_t, 3>> hocc(a.hist ? (size_t)frames : 0);
    std::vector<histogram_io> hist(a.gpus);
    for (auto &x : hist) x.open(a, &hstats, &hocc);
    auto work = [&](block *b) {
        histogram_io *hi = &hist[b - blocks.data()];
        if (a.hist_only) run_block_histogram(a, (size_t)a.in.width * a.in.height * 2, in_frame_bytes, hi, b);
        else if (a.scale_only) run_block_scale(a, (size_t)a.in.width * a.in.height * 2, in_frame_bytes, out_frame_bytes, fd, base, b);
        else if (a.compare_only) run_block_compare(a, (size_t)a.in.width * a.in.height * 2, in_frame_bytes, &stats, &sstats, hi, b);
        else if (a.inverse) run_block_inverse(a, tw, fd, base, &stats, &sstats, hi, b);
        else run_block(a, d, dpx, di, tiff, ti, exr, xi, fd, base, &stats, &sstats, &lstats, hi, b);
    };
    if (a.gpus == 1) work(&blocks[0]);
    else {
        std::vector<std::thread> th;
        for (int r = 0; r < a.gpus; r++) th.emplace_back(work, &blocks[r]);
        for (auto &t : th) t.join();
    }
    if (fd >= 0) close(fd);
    int rc = 0;
    for (int r = 0; r < a.gpus; r++)
        if (!blocks[r].err.empty()) {
            printf("ERROR (device %d, frames %ld..%ld): %s\n", blocks[r].device, blocks[r].first, blocks[r].first + blocks[r].count - 1, blocks[r].err.c_str());
            rc = 1;
        }
    const bool ran = !rc;
    const bool compared = !rc && a.ref;
    if (compared) rc = compare_report(a, cmp_yuv, a.out.bit_depth, stats);
    if (compared && a.ssim) ssim_report(cmp_yuv, sstats);
    if ((!rc || rc == 3) && a.hist) { /* the bins of every thread, summed (the same totals for any split) */
        std::vector<uint64_t> total(hist[0].total.size(), 0u);
        for (const auto &x : hist)
            for (size_t i = 0; i < total.size(); i++) total[i] += x.total[i];
        const int hrc = histogram_report(a, hstats, hocc, total);
        if (hrc == 1 || !rc) rc = hrc;
    }
    if (ran && a.light) light_report(lstats);
    return rc;
}
