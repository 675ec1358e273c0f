/*
 * h2y_cli_sources.h -- where hdr2yuv's frames come from: the scan of a .dpx, .tiff or .exr sequence before the run (one walk,
 * scan_sequence, with one step per format), the pool of threads that unpacks .exr chunks into a pinned slot, the seeded synthetic
 * frame, and the small file helpers they share.  No HIP here: the scans run under --dry_run too.
 */
#ifndef H2Y_CLI_SOURCES_H
#define H2Y_CLI_SOURCES_H

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <fcntl.h>
#include <functional>
#include <mutex>
#include <sys/mman.h>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>

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

/* a whole file mapped read-only */
struct mapped_file {
    void *p = MAP_FAILED;
    size_t n = 0;
    bool found = false; /* the file could be opened (it may still be empty or refuse the mapping) */
    bool open(const std::string &path)
    {
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        found = true;
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

/* what a format's step says of file k of the run: kept, not there, or refused with the problem already printed */
enum scan_step { SCAN_KEPT, SCAN_ABSENT, SCAN_ERROR };

/* The files of the run -- --src_filename itself, or the files numbered --src_start_frame .. + want - 1 of a sequence (as many of
 * them as exist in a row) -- each handed to the format's step.  A file that is not there ends a sequence; the first file has to
 * be there ("ERROR: <absent> <name>").  Returns 0, or 1 with the first problem printed. */
static int scan_sequence(const cli_args &a, long want, const char *absent, const std::function<scan_step(long, const std::string &)> &step)
{
    const bool seq = cli_frame_pattern(a.src) == 1;
    for (long k = 0; k < (seq ? want : 1); k++) {
        const std::string path = cli_frame_name(a.src, a.start_frame + k);
        const scan_step s = step(k, path);
        if (s == SCAN_ABSENT && k) break; /* the sequence ends here */
        if (s == SCAN_ABSENT) printf("ERROR: %s %s\n", absent, path.c_str());
        if (s != SCAN_KEPT) return 1;
    }
    return 0;
}

/* one .dpx file of the run: its name and where its payload starts */
struct dpx_src {
    std::string path;
    uint64_t offset;
};

/* The .dpx files of the run (scan_sequence; a file is there when stat finds it), parsed, checked against the command line's size
 * and against the first file's geometry and format.  Returns 0 and fills info and files, or prints the first problem and returns 1. */
static int dpx_scan(const cli_args &a, long want, h2y_dpx_info &info, std::vector<dpx_src> &files)
{
    return scan_sequence(a, want, "unable to open file", [&](long k, const std::string &path) {
        struct stat st;
        if (stat(path.c_str(), &st)) return SCAN_ABSENT;
        unsigned char hdr[2048];
        FILE *f = fopen(path.c_str(), "rb");
        if (!f) { printf("ERROR: unable to open file %s\n", path.c_str()); return SCAN_ERROR; }
        const size_t got = fread(hdr, 1, sizeof hdr, f);
        fclose(f);
        h2y_dpx_info di;
        const char *why = nullptr;
        if (h2y_dpx_parse(hdr, got, (uint64_t)st.st_size, &di, &why)) { printf("ERROR: %s: %s\n", path.c_str(), why); return SCAN_ERROR; }
        if (di.width != a.in.width || di.height != a.in.height) {
            printf("ERROR: %s is %dx%d, --src_pic_width/--src_pic_height say %dx%d: resizing is not part of convert() (cv.cpp is "
                   "compiled out in the reference)\n", path.c_str(), di.width, di.height, a.in.width, a.in.height);
            return SCAN_ERROR;
        }
        if (k && (di.width != info.width || di.height != info.height || di.bit_size != info.bit_size || di.swap != info.swap)) {
            printf("ERROR: %s is %dx%d %d-bit %s-endian, %s %dx%d %d-bit %s-endian: every file of a sequence must have the same\n",
                   path.c_str(), di.width, di.height, di.bit_size, di.swap ? "big" : "little", files[0].path.c_str(), info.width,
                   info.height, info.bit_size, info.swap ? "big" : "little");
            return SCAN_ERROR;
        }
        /* fields dpx_read() ignores: the image element's descriptor (byte 800) and packing (u16 at 804) */
        const unsigned descriptor = hdr[800], packing = di.swap ? (unsigned)hdr[804] << 8 | hdr[805] : (unsigned)hdr[805] << 8 | hdr[804];
        if (descriptor != 50) printf("WARNING: %s: descriptor %u is not 50 (RGB); decoded as R,G,B, as dpx_read() does\n", path.c_str(), descriptor);
        if (di.bit_size == 10 && packing != 1)
            printf("WARNING: %s: 10-bit packing %u is not 1 (filled to 32-bit words, method A); decoded as packing 1, as dpx_read() does\n",
                   path.c_str(), packing);
        if (!k) info = di;
        files.push_back({path, di.data_offset});
        return SCAN_KEPT;
    });
}

/* one .tiff file of the run: its name and where its decoded rows lie */
struct tiff_src {
    std::string path;
    std::vector<uint64_t> rows; /* file offset of each decoded row */
    bool contiguous;
};

/* The .tiff files of the run, as dpx_scan (a file is there when it can be opened): each mapped, its IFD parsed for read_tiff's
 * geometry with the command line's cutouts, checked against the command line's size and against the first file's geometry and
 * byte order. */
static int tiff_scan(const cli_args &a, long want, h2y_tiff_info &info, std::vector<tiff_src> &files)
{
    return scan_sequence(a, want, "unable to open file", [&](long k, const std::string &path) {
        h2y_tiff_info ti;
        const char *why = nullptr;
        tiff_src src{path, {}, false};
        {
            mapped_file m;
            if (!m.open(path)) {
                if (!m.found) return SCAN_ABSENT;
                printf("ERROR: unable to map file %s\n", path.c_str());
                return SCAN_ERROR;
            }
            int rc = h2y_tiff_parse(m.p, m.n, a.cutout, &ti, nullptr, 0, &why);
            if (!rc) {
                src.rows.resize((size_t)ti.height);
                rc = h2y_tiff_parse(m.p, m.n, a.cutout, &ti, src.rows.data(), ti.height, &why);
            }
            if (rc) { printf("ERROR: %s: %s\n", path.c_str(), why); return SCAN_ERROR; }
        }
        if (ti.width != a.in.width || ti.height != a.in.height) {
            printf("ERROR: %s decodes to %dx%d, --src_pic_width/--src_pic_height say %dx%d: resizing is not part of convert() (cv.cpp "
                   "is compiled out in the reference)\n", path.c_str(), ti.width, ti.height, a.in.width, a.in.height);
            return SCAN_ERROR;
        }
        if (k && (ti.file_width != info.file_width || ti.file_height != info.file_height || ti.swap != info.swap)) {
            printf("ERROR: %s is %dx%d %s-endian, %s %dx%d %s-endian: every file of a sequence must have the same\n", path.c_str(),
                   ti.file_width, ti.file_height, ti.swap ? "big" : "little", files[0].path.c_str(), info.file_width, info.file_height,
                   info.swap ? "big" : "little");
            return SCAN_ERROR;
        }
        if (!k && ti.swap)
            printf("WARNING: %s is big-endian (MM): decoded with the bytes of each sample exchanged; the reference reads them unswapped\n",
                   path.c_str());
        src.contiguous = ti.contiguous != 0;
        if (!k) info = ti;
        files.push_back(std::move(src));
        return SCAN_KEPT;
    });
}

/* The .exr files of the run, as dpx_scan (a file is there when it can be opened and mapped: an empty one is not): each mapped and
 * parsed, its data window checked against the command line and its header against the first file's (every file of a sequence has
 * one h2y_exr_info).  Messages cite read_exr(). */
static int exr_scan(const cli_args &a, long want, h2y_exr_info &info, std::vector<std::string> &files)
{
    return scan_sequence(a, want, "read_exr() (exr.cpp:146): unable to open or read file", [&](long k, const std::string &path) {
        mapped_file m;
        if (!m.open(path)) return SCAN_ABSENT;
        h2y_exr_info xi;
        const char *why = nullptr;
        if (h2y_exr_parse(m.p, m.n, &xi, nullptr, 0, &why)) {
            printf("ERROR: read_exr() (exr.cpp): %s: %s\n", path.c_str(), why);
            return SCAN_ERROR;
        }
        if (xi.width != a.in.width || xi.height != a.in.height) {
            printf("ERROR: read_exr() (exr.cpp:149-153): %s has a %dx%d data window, --src_pic_width/--src_pic_height say %dx%d: "
                   "resizing is not part of convert() (cv.cpp is compiled out in the reference)\n", path.c_str(), xi.width, xi.height,
                   a.in.width, a.in.height);
            return SCAN_ERROR;
        }
        if (k && memcmp(&xi, &info, sizeof xi)) {
            printf("ERROR: read_exr() (exr.cpp): %s differs from %s in its data window, compression or channels: every file of a "
                   "sequence must have the same\n", path.c_str(), files[0].c_str());
            return SCAN_ERROR;
        }
        if (!k) info = xi;
        files.push_back(path);
        return SCAN_KEPT;
    });
}

/* what the scans found: the files of the run and the header every one of them shares (only the source's format is filled) */
struct scanned {
    std::vector<dpx_src> dpx;
    h2y_dpx_info di{};
    std::vector<tiff_src> tiff;
    h2y_tiff_info ti{};
    std::vector<std::string> exr;
    h2y_exr_info xi{};
};

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

#endif /* H2Y_CLI_SOURCES_H */
