/* blosc1.c — host-side chunk codec of the ingestion path.
 *
 * Zarr stores in the wild are compressed with Blosc-1 (numcodecs' default compressor is
 * Blosc(cname="lz4", shuffle=SHUFFLE)); the reference decodes them through numcodecs inside its
 * dask graph (aggfly/dataset/dataset.py:697-728), GIL-limited to ~2 cores
 * (benchmarks/bench_read_scheduler.py:4-8).  This file decodes Blosc-1 chunks natively, one
 * chunk per host thread, straight into the time-major staging buffer that is then copied to HBM.
 *
 * Blosc-1 container (c-blosc 1.x, format version 2), restated from the published format:
 *   header  [0] version  [1] versionlz  [2] flags  [3] typesize  [4:8] nbytes  [8:12] blocksize
 *           [12:16] cbytes (all little-endian)
 *   flags   0x01 byte shuffle | 0x02 stored uncompressed ("memcpyed") | 0x04 bit shuffle |
 *           0x10 blocks are not split into per-byte streams | bits 5-7: codec (0 blosclz, 1 lz4 /
 *           lz4hc, 2 snappy, 3 zlib, 4 zstd)
 *   then    int32 bstarts[nblocks]: offset of every block's data from the start of the chunk
 *   block   nsplits streams (typesize streams when split, else 1), each: int32 csize, data;
 *           csize == stream length means the stream is stored raw
 *   the (un)shuffle acts per block; the last, shorter block is never split.
 * Pinned against chunks produced by the real c-blosc 1.21 (tests/golden/blosc_fixtures.json).
 *
 * LZ4 / Zstandard come from the system's liblz4.so.1 / libzstd.so.1 (dlopen, stable C ABIs:
 * LZ4_decompress_safe, LZ4_compress_default, ZSTD_decompress, ZSTD_isError), zlib is linked.
 */
#include <dlfcn.h>
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>
#include <zlib.h>
#include <emmintrin.h>

/* AFCODEC_NT_COPY=0 switches the non-temporal stores of the reader and of the byte unshuffle off (A/B knob) */
static int nt_store_default(void) {
    static int v = -1;
    if (v < 0) { const char* e = getenv("AFCODEC_NT_COPY"); v = e ? atoi(e) != 0 : 1; }
    return v;
}

#define AFCODEC_OK 0
#define AFCODEC_E_FORMAT (-1)
#define AFCODEC_E_UNSUPPORTED (-2)
#define AFCODEC_E_SIZE (-3)
#define AFCODEC_E_CODEC (-4)

static __thread char g_err[256];
static int fail(int code, const char* msg) {
    snprintf(g_err, sizeof g_err, "%s", msg);
    return code;
}
const char* afcodec_last_error(void) { return g_err; }

/* ---- lazily bound system codecs ---- */
typedef int (*lz4_dec_fn)(const char*, char*, int, int);
typedef int (*lz4_enc_fn)(const char*, char*, int, int);
typedef int (*lz4_bound_fn)(int);
typedef size_t (*zstd_dec_fn)(void*, size_t, const void*, size_t);
typedef unsigned (*zstd_iserr_fn)(size_t);
typedef size_t (*zstd_enc_fn)(void*, size_t, const void*, size_t, int);
typedef size_t (*zstd_bound_fn)(size_t);
static lz4_dec_fn p_lz4_dec;
static lz4_enc_fn p_lz4_enc;
static lz4_bound_fn p_lz4_bound;
static zstd_dec_fn p_zstd_dec;
static zstd_iserr_fn p_zstd_iserr;
static zstd_enc_fn p_zstd_enc;
static zstd_bound_fn p_zstd_bound;
static int g_lz4_tried, g_zstd_tried;

static int need_lz4(void) {
    if (!g_lz4_tried) {
        void* h = dlopen("liblz4.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (h) {
            p_lz4_dec = (lz4_dec_fn)dlsym(h, "LZ4_decompress_safe");
            p_lz4_enc = (lz4_enc_fn)dlsym(h, "LZ4_compress_default");
            p_lz4_bound = (lz4_bound_fn)dlsym(h, "LZ4_compressBound");
        }
        g_lz4_tried = 1;
    }
    return (p_lz4_dec && p_lz4_enc && p_lz4_bound) ? 0 : fail(AFCODEC_E_UNSUPPORTED, "liblz4.so.1 not available");
}
static int need_zstd(void) {
    if (!g_zstd_tried) {
        void* h = dlopen("libzstd.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (h) {
            p_zstd_dec = (zstd_dec_fn)dlsym(h, "ZSTD_decompress");
            p_zstd_iserr = (zstd_iserr_fn)dlsym(h, "ZSTD_isError");
            p_zstd_enc = (zstd_enc_fn)dlsym(h, "ZSTD_compress");
            p_zstd_bound = (zstd_bound_fn)dlsym(h, "ZSTD_compressBound");
        }
        g_zstd_tried = 1;
    }
    return (p_zstd_dec && p_zstd_iserr) ? 0 : fail(AFCODEC_E_UNSUPPORTED, "libzstd.so.1 not available");
}
int afcodec_have(int codec) { /* 1 lz4, 3 zlib, 4 zstd, 0 blosclz */
    if (codec == 1) return need_lz4() == 0;
    if (codec == 4) return need_zstd() == 0;
    return codec == 0 || codec == 3;
}

static uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static void put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

/* ---- BloscLZ (the FastLZ-derived codec shipped inside c-blosc 1.x) ---- */
static int blosclz_decode(const uint8_t* ip, int length, uint8_t* out, int maxout) {
    const uint8_t* ip_limit = ip + length;
    uint8_t* op = out;
    uint8_t* op_limit = out + maxout;
    if (length == 0) return 0;
    uint32_t ctrl = (*ip++) & 31u;
    for (;;) {
        if (ctrl >= 32) {                                   /* match: length in the top 3 bits, distance below */
            int32_t len = (int32_t)(ctrl >> 5) - 1;
            int32_t ofs = (int32_t)((ctrl & 31u) << 8);
            const uint8_t* ref = op - ofs;
            uint8_t code;
            if (len == 7 - 1) {
                do {
                    if (ip + 1 >= ip_limit) return -1;
                    code = *ip++;
                    len += code;
                } while (code == 255);
            } else if (ip + 1 >= ip_limit) {
                return -1;
            }
            code = *ip++;
            len += 3;
            ref -= code;
            if (code == 255 && ofs == (31 << 8)) {          /* far match: 16-bit distance beyond 8191 */
                if (ip + 1 >= ip_limit) return -1;
                ofs = (*ip++) << 8;
                ofs += *ip++;
                ref = op - ofs - 8191;
            }
            if (op + len > op_limit) return -1;
            if (ref - 1 < out) return -1;
            const int last = ip >= ip_limit;
            if (!last) ctrl = *ip++;
            ref--;
            for (int32_t i = 0; i < len; ++i) op[i] = ref[i];      /* byte-wise: overlapping runs repeat */
            op += len;
            if (last) break;
        } else {                                            /* literal run of ctrl + 1 bytes */
            ctrl++;
            if (op + ctrl > op_limit || ip + ctrl > ip_limit) return -1;
            memcpy(op, ip, ctrl);
            op += ctrl;
            ip += ctrl;
            if (ip >= ip_limit) break;
            ctrl = *ip++;
        }
    }
    return (int)(op - out);
}

/* ---- shuffle filters, per block ---- */
/* 4- and 8-byte elements: 16 elements a step with SSE2 byte / word / dword interleaves (every x86-64 CPU has them).  The planes
 * come out of a cache-resident scratch block and the elements go to a destination nobody reads back soon (page-locked staging
 * the GPU fetches by DMA): with a 16-byte-aligned destination the stores are non-temporal, so the destination lines are not
 * read first. */
static void unshuffle_bytes(int ts, int64_t bsize, const uint8_t* src, uint8_t* dst) {
    const int64_t n = bsize / ts, rem = bsize % ts;
    if (ts == 4) {
        const uint8_t *s0 = src, *s1 = src + n, *s2 = src + 2 * n, *s3 = src + 3 * n;
        const int nt = (((uintptr_t)dst) & 15) == 0 && nt_store_default();
        int64_t i = 0;
        for (; i + 16 <= n; i += 16) {
            const __m128i a = _mm_loadu_si128((const __m128i*)(s0 + i)), b = _mm_loadu_si128((const __m128i*)(s1 + i));
            const __m128i c = _mm_loadu_si128((const __m128i*)(s2 + i)), d = _mm_loadu_si128((const __m128i*)(s3 + i));
            const __m128i ab0 = _mm_unpacklo_epi8(a, b), ab1 = _mm_unpackhi_epi8(a, b), cd0 = _mm_unpacklo_epi8(c, d), cd1 = _mm_unpackhi_epi8(c, d);
            const __m128i o0 = _mm_unpacklo_epi16(ab0, cd0), o1 = _mm_unpackhi_epi16(ab0, cd0), o2 = _mm_unpacklo_epi16(ab1, cd1), o3 = _mm_unpackhi_epi16(ab1, cd1);
            __m128i* out = (__m128i*)(dst + 4 * i);
            if (nt) { _mm_stream_si128(out, o0); _mm_stream_si128(out + 1, o1); _mm_stream_si128(out + 2, o2); _mm_stream_si128(out + 3, o3); }
            else { _mm_storeu_si128(out, o0); _mm_storeu_si128(out + 1, o1); _mm_storeu_si128(out + 2, o2); _mm_storeu_si128(out + 3, o3); }
        }
        for (; i < n; ++i) { dst[4 * i] = s0[i]; dst[4 * i + 1] = s1[i]; dst[4 * i + 2] = s2[i]; dst[4 * i + 3] = s3[i]; }
        if (nt) _mm_sfence();
    } else if (ts == 8) {
        const int nt = (((uintptr_t)dst) & 15) == 0 && nt_store_default();
        int64_t i = 0;
        for (; i + 16 <= n; i += 16) {
            __m128i p[8], t[8], u[8];
            for (int j = 0; j < 8; ++j) p[j] = _mm_loadu_si128((const __m128i*)(src + (int64_t)j * n + i));
            for (int j = 0; j < 4; ++j) { t[2 * j] = _mm_unpacklo_epi8(p[2 * j], p[2 * j + 1]); t[2 * j + 1] = _mm_unpackhi_epi8(p[2 * j], p[2 * j + 1]); }
            /* t[0], t[1]: bytes 0-1 of elements 0-7 / 8-15;  t[2], t[3]: bytes 2-3;  t[4], t[5]: bytes 4-5;  t[6], t[7]: bytes 6-7 */
            u[0] = _mm_unpacklo_epi16(t[0], t[2]); u[1] = _mm_unpackhi_epi16(t[0], t[2]);      /* bytes 0-3 of elements 0-3 / 4-7 */
            u[2] = _mm_unpacklo_epi16(t[1], t[3]); u[3] = _mm_unpackhi_epi16(t[1], t[3]);      /*              elements 8-11 / 12-15 */
            u[4] = _mm_unpacklo_epi16(t[4], t[6]); u[5] = _mm_unpackhi_epi16(t[4], t[6]);      /* bytes 4-7 */
            u[6] = _mm_unpacklo_epi16(t[5], t[7]); u[7] = _mm_unpackhi_epi16(t[5], t[7]);
            __m128i* out = (__m128i*)(dst + 8 * i);
            for (int q = 0; q < 4; ++q) {
                const __m128i lo = _mm_unpacklo_epi32(u[q], u[q + 4]), hi = _mm_unpackhi_epi32(u[q], u[q + 4]);   /* elements 4q, 4q+1 / 4q+2, 4q+3 */
                if (nt) { _mm_stream_si128(out + 2 * q, lo); _mm_stream_si128(out + 2 * q + 1, hi); }
                else { _mm_storeu_si128(out + 2 * q, lo); _mm_storeu_si128(out + 2 * q + 1, hi); }
            }
        }
        for (; i < n; ++i)
            for (int j = 0; j < 8; ++j) dst[8 * i + j] = src[(int64_t)j * n + i];
        if (nt) _mm_sfence();
    } else {
        for (int64_t i = 0; i < n; ++i)
            for (int j = 0; j < ts; ++j) dst[i * ts + j] = src[(int64_t)j * n + i];
    }
    if (rem) memcpy(dst + bsize - rem, src + bsize - rem, (size_t)rem);
}
static void shuffle_bytes(int ts, int64_t bsize, const uint8_t* src, uint8_t* dst) {
    const int64_t n = bsize / ts, rem = bsize % ts;
    for (int j = 0; j < ts; ++j)
        for (int64_t i = 0; i < n; ++i) dst[(int64_t)j * n + i] = src[i * ts + j];
    if (rem) memcpy(dst + bsize - rem, src + bsize - rem, (size_t)rem);
}
/* Bit shuffle: bit b (byte j = b / 8, LSB-first) of element e is stored in bit row b at bit e.
 * c-blosc 1.x bit-shuffles a block only when it holds a multiple of 8 elements; any other block
 * (typically the short last one) is stored unshuffled (pinned by the 1.21 fixtures). */
static void unshuffle_bits(int ts, int64_t bsize, const uint8_t* src, uint8_t* dst) {
    const int64_t n = bsize / ts;
    if (n % 8 != 0) { memcpy(dst, src, (size_t)bsize); return; }
    const int64_t nrow = n / 8;
    for (int64_t g = 0; g < nrow; ++g) {                    /* 8 elements at a time */
        for (int j = 0; j < ts; ++j) {
            uint64_t x = 0;                                 /* byte k of x = bit row (8j + k), byte g */
            for (int k = 0; k < 8; ++k) x |= (uint64_t)src[((int64_t)j * 8 + k) * nrow + g] << (8 * k);
            /* 8x8 bit-matrix transpose (Hacker's Delight 7-3) */
            uint64_t t;
            t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAULL;  x = x ^ t ^ (t << 7);
            t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCULL; x = x ^ t ^ (t << 14);
            t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ULL; x = x ^ t ^ (t << 28);
            for (int m = 0; m < 8; ++m) dst[(g * 8 + m) * ts + j] = (uint8_t)(x >> (8 * m));
        }
    }
    const int64_t off = n * ts;
    if (bsize > off) memcpy(dst + off, src + off, (size_t)(bsize - off));
}

/* the inverse (writer side): the same rule for blocks that do not hold a multiple of 8 elements */
static void shuffle_bits(int ts, int64_t bsize, const uint8_t* src, uint8_t* dst) {
    const int64_t n = bsize / ts;
    if (n % 8 != 0) { memcpy(dst, src, (size_t)bsize); return; }
    const int64_t nrow = n / 8;
    for (int64_t g = 0; g < nrow; ++g) {
        for (int j = 0; j < ts; ++j) {
            uint64_t x = 0, t;                              /* byte m of x = byte j of element 8g + m */
            for (int m = 0; m < 8; ++m) x |= (uint64_t)src[(g * 8 + m) * ts + j] << (8 * m);
            t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAULL;  x = x ^ t ^ (t << 7);
            t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCULL; x = x ^ t ^ (t << 14);
            t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ULL; x = x ^ t ^ (t << 28);
            for (int k2 = 0; k2 < 8; ++k2) dst[((int64_t)j * 8 + k2) * nrow + g] = (uint8_t)(x >> (8 * k2));
        }
    }
    const int64_t off = n * ts;
    if (bsize > off) memcpy(dst + off, src + off, (size_t)(bsize - off));
}

int64_t afcodec_zstd_decode(const void* src, int64_t n, void* dst, int64_t cap);
int64_t afcodec_blosc_decode(const void* chunk, int64_t csize, void* dstv, int64_t dstsize);

/* ---- chunk header ---- */
int afcodec_blosc_info(const void* chunk, int64_t size, int64_t* nbytes, int64_t* blocksize, int32_t* typesize, int32_t* flags) {
    const uint8_t* c = (const uint8_t*)chunk;
    if (!c || size < 16) return fail(AFCODEC_E_FORMAT, "blosc chunk shorter than its 16-byte header");
    if (c[0] != 2) return fail(AFCODEC_E_UNSUPPORTED, "blosc format version is not 2 (Blosc-1)");
    if (nbytes) *nbytes = le32(c + 4);
    if (blocksize) *blocksize = le32(c + 8);
    if (typesize) *typesize = c[3];
    if (flags) *flags = c[2];
    if ((int64_t)le32(c + 12) > size) return fail(AFCODEC_E_SIZE, "blosc chunk is truncated (cbytes > size)");
    return AFCODEC_OK;
}

/* liblz4 1.9.3's LZ4_decompress_safe does not refuse a match offset of 0: it "copies" the destination onto itself, so a damaged
 * stream decodes, to its recorded size, into whatever the destination held (the GPU decoder counts such a stream as an error;
 * tests/lz4_streams.py: off0_window, off0_generic).  One walk over the sequence headers finds it; anything else that is wrong
 * with the stream ends the walk and is left to liblz4. */
static int lz4_has_zero_offset(const uint8_t* s, int64_t n) {
    int64_t p = 0;
    while (p < n) {
        const unsigned t = s[p++];
        int64_t L = t >> 4;
        if (L == 15) {
            unsigned b;
            do { if (p >= n) return 0; b = s[p++]; L += b; } while (b == 255);
        }
        p += L;
        if (p + 2 > n) return 0;                            /* the final literals (or a cut stream) */
        if ((s[p] | s[p + 1]) == 0) return 1;
        p += 2;
        if ((t & 15) == 15) {
            unsigned b;
            do { if (p >= n) return 0; b = s[p++]; } while (b == 255);
        }
    }
    return 0;
}

static int decode_stream(int codec, const uint8_t* src, int32_t csize, uint8_t* dst, int32_t want) {
    int got = -1;
    switch (codec) {
        case 0: got = blosclz_decode(src, csize, dst, want); break;
        case 1: got = lz4_has_zero_offset(src, csize) ? -1 : p_lz4_dec((const char*)src, (char*)dst, csize, want); break;
        case 3: { uLongf n = (uLongf)want; got = uncompress(dst, &n, src, (uLong)csize) == Z_OK ? (int)n : -1; break; }
        case 4: { size_t n = p_zstd_dec(dst, (size_t)want, src, (size_t)csize); got = p_zstd_iserr(n) ? -1 : (int)n; break; }
        default: break;
    }
    return got == want ? 0 : -1;
}

static __thread uint8_t* t_scratch;
static __thread int64_t t_scratch_cap;

typedef struct {
    const uint8_t* c;
    uint8_t* dst;
    int64_t nbytes, blocksize, cbytes, nblocks, leftover;
    int ts, flags, codec, dont_split, want_shuffle, stored;
} blosc_ctx;

/* Parses and validates the header; > 0 = nothing left to do (empty chunk), < 0 = error. */
static int blosc_open(blosc_ctx* x, const void* chunk, int64_t csize, void* dstv, int64_t dstsize) {
    int32_t ts, flags;
    x->c = (const uint8_t*)chunk;
    x->dst = (uint8_t*)dstv;
    int rc = afcodec_blosc_info(chunk, csize, &x->nbytes, &x->blocksize, &ts, &flags);
    if (rc) return rc;
    x->ts = ts; x->flags = flags;
    if (x->nbytes > dstsize) return fail(AFCODEC_E_SIZE, "destination smaller than the chunk's nbytes");
    if (x->nbytes == 0) return 1;
    x->cbytes = le32(x->c + 12);
    x->stored = (flags & 0x02) != 0;
    if (x->stored) {
        if (x->cbytes < 16 + x->nbytes) return fail(AFCODEC_E_FORMAT, "stored chunk shorter than nbytes");
        return AFCODEC_OK;
    }
    x->codec = (flags >> 5) & 7;
    if (x->codec == 1) { if ((rc = need_lz4())) return rc; }
    else if (x->codec == 4) { if ((rc = need_zstd())) return rc; }
    else if (x->codec != 0 && x->codec != 3) return fail(AFCODEC_E_UNSUPPORTED, "blosc codec not supported (snappy)");
    if (x->blocksize <= 0 || ts <= 0 || x->blocksize > x->nbytes) return fail(AFCODEC_E_FORMAT, "bad blocksize / typesize");
    x->nblocks = (x->nbytes + x->blocksize - 1) / x->blocksize;
    x->leftover = x->nbytes % x->blocksize;
    if (16 + 4 * x->nblocks > x->cbytes) return fail(AFCODEC_E_FORMAT, "block table beyond the chunk");
    x->dont_split = (flags >> 4) & 1;
    x->want_shuffle = (flags & 0x01) && ts > 1;
    return AFCODEC_OK;
}

/* One block of an opened chunk; blocks are independent, so a big chunk decodes on many threads. */
static int blosc_block(const blosc_ctx* x, int64_t b) {
    const uint8_t* c = x->c;
    const int ts = x->ts;
    uint8_t* tmp = NULL;
    if (x->want_shuffle || (x->flags & 0x04)) {
        /* per-thread scratch, kept between calls: a fresh malloc of a block (>= 128 KiB -> mmap/munmap)
         * per chunk page-faults every time and serialises the threads on the process's mmap lock */
        if (t_scratch_cap < x->blocksize) {
            free(t_scratch);
            t_scratch = (uint8_t*)malloc((size_t)x->blocksize);
            t_scratch_cap = t_scratch ? x->blocksize : 0;
        }
        tmp = t_scratch;
        if (!tmp) return fail(AFCODEC_E_SIZE, "out of memory");
    }
    const int last_short = (b == x->nblocks - 1) && x->leftover > 0;
    const int64_t bsize = last_short ? x->leftover : x->blocksize;
    const int do_shuf = x->want_shuffle;
    const int do_bits = !do_shuf && (x->flags & 0x04) && bsize >= ts;
    uint8_t* out = x->dst + b * x->blocksize;
    uint8_t* into = (do_shuf || do_bits) ? tmp : out;
    int nsplits = 1;
    if (!x->dont_split && ts <= 16 && x->blocksize / ts >= 128 && !last_short) nsplits = ts;
    const int64_t neblock = bsize / nsplits;
    const int64_t start = (int64_t)(int32_t)le32(c + 16 + 4 * b);
    if (start < 16 + 4 * x->nblocks || start >= x->cbytes) return fail(AFCODEC_E_FORMAT, "block offset out of range");
    const uint8_t* src = c + start;
    for (int j = 0; j < nsplits; ++j) {
        if (src + 4 > c + x->cbytes) return fail(AFCODEC_E_FORMAT, "stream header beyond the chunk");
        const int32_t sz = (int32_t)le32(src);
        src += 4;
        if (sz < 0 || src + sz > c + x->cbytes) return fail(AFCODEC_E_FORMAT, "stream beyond the chunk");
        if (sz == neblock) memcpy(into + j * neblock, src, (size_t)neblock);
        else if (decode_stream(x->codec, src, sz, into + j * neblock, (int32_t)neblock))
            return fail(AFCODEC_E_CODEC, "block failed to decompress to its recorded size");
        src += sz;
    }
    if (do_shuf) unshuffle_bytes(ts, bsize, tmp, out);
    else if (do_bits) unshuffle_bits(ts, bsize, tmp, out);
    return AFCODEC_OK;
}

#include "zstd_passes.h"
typedef struct { afz_frame* frames; int64_t cap_frames, nf; afz_block* blocks; int64_t cap_blocks, nb, lit, nsq, dec; } zstd_lists;
static int zstd_plan_frames(zstd_lists* z, const void* base, int64_t n, const int64_t* comp_off, const int64_t* comp_size, const int64_t* out_off,
                            const int64_t* out_size, int64_t* results);

/* ---- plan of a GPU-side Blosc decode (include/aggfly_codec.h: afcodec_blosc_plan, afcodec_blosc_lz4_plan) ----
 * ONE walk of the containers of n chunks lists, for the kernels of libaggfly_hip, every LZ4 stream and every plain copy
 * (afhip_lz4_decode_streams), every Zstandard frame with its blocks (afhip_zstd_decode, through zstd_plan_frames below) and every
 * block whose byte shuffle (afhip_unshuffle_blocks) or bit shuffle (afhip_bitunshuffle_blocks) has to be undone.  Layout: every
 * Zstandard frame and every stream of a shuffled block decodes into the shuffle scratch (tmp), and the block then moves tmp ->
 * out through one of the two unshuffle lists — an unshuffled Zstandard block as a byte-shuffle record of typesize 1, which is a
 * copy — so that one afhip_zstd_decode call with out = tmp serves a batch of any mix of flavours.  Unshuffled LZ4 streams go
 * straight to the output, as they always have.  Nothing is decoded here.
 * z == NULL is afcodec_blosc_lz4_plan's filter: Zstandard and bit-shuffled chunks are then E_UNSUPPORTED like the other codecs. */
typedef struct { int64_t src_off, dst_off; int32_t csize, dsize, to_out, pad; } lz4_stream_t;
typedef struct { int64_t tmp_off, out_off; int32_t bsize, typesize; } shuf_block_t;
#define GPU_STREAM_MAX 65536

static int blosc_walk(const void* base, int64_t n, const int64_t* comp_off, const int64_t* comp_size, const int64_t* out_off,
                      const int64_t* out_size, lz4_stream_t* streams, int64_t cap_streams, int64_t* n_streams, shuf_block_t* blocks,
                      int64_t cap_blocks, int64_t* n_blocks, shuf_block_t* bits, int64_t cap_bits, int64_t* n_bits, zstd_lists* z,
                      int64_t* tmp_bytes, int32_t* max_dsize, int64_t* results) {
    int64_t ns = 0, nb = 0, nbit = 0, tmp = 0;
    int32_t maxd = 0;
    int rc_all = AFCODEC_OK;
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t* c = (const uint8_t*)base + comp_off[i];
        const int64_t csz = comp_size[i];
        results[i] = 0;
        int64_t nbytes, blocksize; int32_t ts, flags;
        int rc = afcodec_blosc_info(c, csz, &nbytes, &blocksize, &ts, &flags);
        if (rc) { results[i] = rc; rc_all = rc; continue; }
        if (nbytes > out_size[i]) { results[i] = rc_all = fail(AFCODEC_E_SIZE, "destination smaller than the chunk's nbytes"); continue; }
        results[i] = nbytes;
        if (nbytes == 0) continue;
        const int64_t cbytes = le32(c + 12);
        if (flags & 0x02) {                                             /* stored chunk: plain copies, 64 KiB per wave */
            if (cbytes < 16 + nbytes) { results[i] = rc_all = fail(AFCODEC_E_FORMAT, "stored chunk shorter than nbytes"); continue; }
            for (int64_t o = 0; o < nbytes; o += GPU_STREAM_MAX) {
                const int32_t len = (int32_t)((nbytes - o) < GPU_STREAM_MAX ? (nbytes - o) : GPU_STREAM_MAX);
                if (ns >= cap_streams) return fail(AFCODEC_E_SIZE, "stream list too small");
                streams[ns++] = (lz4_stream_t){comp_off[i] + 16 + o, out_off[i] + o, len, len, 1, 0};
            }
            continue;
        }
        const int codec = (flags >> 5) & 7;
        if (!z && (codec != 1 || (flags & 0x04))) { results[i] = AFCODEC_E_UNSUPPORTED; rc_all = fail(AFCODEC_E_UNSUPPORTED, "not an LZ4 chunk with byte shuffle or none: decode on the host"); continue; }
        if (codec != 1 && codec != 4) { results[i] = AFCODEC_E_UNSUPPORTED; rc_all = fail(AFCODEC_E_UNSUPPORTED, "inner codec is neither LZ4 nor Zstandard: decode on the host"); continue; }
        if (blocksize <= 0 || ts <= 0 || blocksize > nbytes) { results[i] = rc_all = fail(AFCODEC_E_FORMAT, "bad blocksize / typesize"); continue; }
        const int64_t nblocks = (nbytes + blocksize - 1) / blocksize, leftover = nbytes % blocksize;
        if (16 + 4 * nblocks > cbytes) { results[i] = rc_all = fail(AFCODEC_E_FORMAT, "block table beyond the chunk"); continue; }
        const int dont_split = (flags >> 4) & 1, want_shuffle = (flags & 0x01) && ts > 1;
        const int64_t ns0 = ns, nb0 = nb, nbit0 = nbit, tmp0 = tmp;
        zstd_lists z0;
        if (z) z0 = *z;
        int bad = 0;
        const char* why = "malformed block table or stream header";
        for (int64_t b = 0; b < nblocks && !bad; ++b) {
            const int last_short = (b == nblocks - 1) && leftover > 0;
            const int64_t bsize = last_short ? leftover : blocksize;
            const int want_bits = !want_shuffle && (flags & 0x04) && bsize >= ts;
            int nsplits = 1;
            if (!dont_split && ts <= 16 && blocksize / ts >= 128 && !last_short) nsplits = ts;
            const int64_t neblock = bsize / nsplits;
            const int64_t start = (int64_t)(int32_t)le32(c + 16 + 4 * b);
            if (start < 16 + 4 * nblocks || start >= cbytes) { bad = AFCODEC_E_FORMAT; break; }
            int64_t dst_base;
            const int via_tmp = want_shuffle || want_bits || codec == 4;
            if (want_bits) {
                if (nbit >= cap_bits) return fail(AFCODEC_E_SIZE, "bit-shuffle block list too small");
                bits[nbit++] = (shuf_block_t){tmp, out_off[i] + b * blocksize, (int32_t)bsize, ts};
            } else if (via_tmp) {
                if (nb >= cap_blocks) return fail(AFCODEC_E_SIZE, "block list too small");
                blocks[nb++] = (shuf_block_t){tmp, out_off[i] + b * blocksize, (int32_t)bsize, want_shuffle ? ts : 1};
            }
            if (via_tmp) {
                dst_base = tmp;
                tmp += (bsize + 15) & ~(int64_t)15;
            } else {
                dst_base = out_off[i] + b * blocksize;
            }
            const uint8_t* src = c + start;
            for (int j = 0; j < nsplits; ++j) {
                if (src + 4 > c + cbytes) { bad = AFCODEC_E_FORMAT; break; }
                const int32_t sz = (int32_t)le32(src);
                src += 4;
                if (sz < 0 || src + sz > c + cbytes) { bad = AFCODEC_E_FORMAT; break; }
                if (codec == 1) {
                    if (sz > neblock + neblock / 255 + 16) { bad = AFCODEC_E_FORMAT; break; }
                    if (ns >= cap_streams) return fail(AFCODEC_E_SIZE, "stream list too small");
                    streams[ns++] = (lz4_stream_t){comp_off[i] + (src - c), dst_base + j * neblock, sz, (int32_t)neblock, via_tmp ? 0 : 1, 0};
                    if (neblock > maxd) maxd = (int32_t)neblock;
                } else if (sz == neblock) {                             /* stored stream of a Zstandard chunk (blocks of up to 1 MiB): 64 KiB per wave */
                    for (int64_t o = 0; o < neblock; o += GPU_STREAM_MAX) {
                        const int32_t len = (int32_t)((neblock - o) < GPU_STREAM_MAX ? (neblock - o) : GPU_STREAM_MAX);
                        if (ns >= cap_streams) return fail(AFCODEC_E_SIZE, "stream list too small");
                        streams[ns++] = (lz4_stream_t){comp_off[i] + (src - c) + o, dst_base + j * neblock + o, len, len, 0, 0};
                    }
                } else {
                    const int64_t f_off = comp_off[i] + (src - c), f_size = sz, f_dst = dst_base + j * neblock;
                    int64_t f_res = 0;
                    const int zrc = zstd_plan_frames(z, base, 1, &f_off, &f_size, &f_dst, &neblock, &f_res);
                    if (zrc == AFCODEC_E_SIZE) return zrc;                          /* a list is full: the caller's capacity, not the chunk */
                    if (zrc) { bad = zrc; why = NULL; break; }                      /* (the frame walk has left its own message) */
                }
                src += sz;
            }
        }
        if (bad) {
            ns = ns0; nb = nb0; nbit = nbit0; tmp = tmp0;
            if (z) *z = z0;
            results[i] = bad;
            rc_all = why ? fail(bad, why) : bad;
        }
    }
    *n_streams = ns; *n_blocks = nb; *tmp_bytes = tmp; *max_dsize = maxd;
    if (n_bits) *n_bits = nbit;
    return rc_all;
}

int afcodec_blosc_lz4_plan(const void* base, int64_t n, const int64_t* comp_off, const int64_t* comp_size, const int64_t* out_off,
                           const int64_t* out_size, void* streams_v, int64_t cap_streams, int64_t* n_streams, void* blocks_v,
                           int64_t cap_blocks, int64_t* n_blocks, int64_t* tmp_bytes, int32_t* max_dsize, int64_t* results) {
    return blosc_walk(base, n, comp_off, comp_size, out_off, out_size, (lz4_stream_t*)streams_v, cap_streams, n_streams,
                      (shuf_block_t*)blocks_v, cap_blocks, n_blocks, NULL, 0, NULL, NULL, tmp_bytes, max_dsize, results);
}

int afcodec_blosc_plan(const void* base, int64_t n, const int64_t* comp_off, const int64_t* comp_size, const int64_t* out_off,
                       const int64_t* out_size, void* streams_v, int64_t cap_streams, int64_t* n_streams, void* blocks_v,
                       int64_t cap_blocks, int64_t* n_blocks, void* bits_v, int64_t cap_bits, int64_t* n_bits, void* frames_v,
                       int64_t cap_frames, int64_t* n_frames, void* zblocks_v, int64_t cap_zblocks, int64_t* n_zblocks, int64_t* lit_bytes,
                       int64_t* n_seqs, int64_t* dec_bytes, int64_t* tmp_bytes, int32_t* max_dsize, int64_t* results) {
    zstd_lists z = {(afz_frame*)frames_v, cap_frames, 0, (afz_block*)zblocks_v, cap_zblocks, 0, 0, 0, 0};
    *n_frames = *n_zblocks = *lit_bytes = *n_seqs = *dec_bytes = 0;
    const int rc = blosc_walk(base, n, comp_off, comp_size, out_off, out_size, (lz4_stream_t*)streams_v, cap_streams, n_streams,
                              (shuf_block_t*)blocks_v, cap_blocks, n_blocks, (shuf_block_t*)bits_v, cap_bits, n_bits, &z, tmp_bytes,
                              max_dsize, results);
    *n_frames = z.nf; *n_zblocks = z.nb; *lit_bytes = z.lit; *n_seqs = z.nsq; *dec_bytes = z.dec;
    return rc;
}

/* Decodes one chunk into dst (capacity dstsize); returns the number of bytes written or < 0. */
int64_t afcodec_blosc_decode(const void* chunk, int64_t csize, void* dstv, int64_t dstsize) {
    blosc_ctx x;
    int rc = blosc_open(&x, chunk, csize, dstv, dstsize);
    if (rc < 0) return rc;
    if (rc > 0) return 0;
    if (x.stored) { memcpy(x.dst, x.c + 16, (size_t)x.nbytes); return x.nbytes; }
    for (int64_t b = 0; b < x.nblocks; ++b)
        if ((rc = blosc_block(&x, b))) return rc;
    return x.nbytes;
}

/* The same with the blocks of the chunk spread over an OpenMP team: for chunks that are few and large
 * (the reference's own converter writes ~256 MB chunks — one per thread would leave most threads idle). */
int64_t afcodec_blosc_decode_mt(const void* chunk, int64_t csize, void* dstv, int64_t dstsize, int nthreads) {
    blosc_ctx x;
    int rc = blosc_open(&x, chunk, csize, dstv, dstsize);
    if (rc < 0) return rc;
    if (rc > 0) return 0;
    if (x.stored) { memcpy(x.dst, x.c + 16, (size_t)x.nbytes); return x.nbytes; }
    if (nthreads < 2 || x.nblocks < 2) {
        for (int64_t b = 0; b < x.nblocks; ++b)
            if ((rc = blosc_block(&x, b))) return rc;
        return x.nbytes;
    }
    int bad = 0;
#pragma omp parallel for schedule(dynamic, 4) num_threads(nthreads) reduction(+ : bad)
    for (int64_t b = 0; b < x.nblocks; ++b)
        if (blosc_block(&x, b)) bad += 1;
    return bad ? fail(AFCODEC_E_CODEC, "one or more blocks of the chunk failed to decode") : x.nbytes;
}

/* Many chunks at once, one per OpenMP thread (ctypes releases the GIL around this call). */
int afcodec_blosc_decode_many(int64_t n, const void* const* chunks, const int64_t* csizes, void* const* dsts,
                              const int64_t* dstsizes, int nthreads, int64_t* results) {
    int bad = 0;
    if (nthreads < 1) nthreads = 1;
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads) reduction(+ : bad)
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r = afcodec_blosc_decode(chunks[i], csizes[i], dsts[i], dstsizes[i]);
        results[i] = r;
        if (r < 0) bad += 1;
    }
    return bad ? fail(AFCODEC_E_CODEC, "one or more chunks failed to decode (see results[])") : AFCODEC_OK;
}

/* zlib / gzip streams through zlib's inflate (wbits 15 + 32: header auto-detected). */
static int64_t inflate_any(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap) {
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, 15 + 32) != Z_OK) return fail(AFCODEC_E_CODEC, "inflateInit2 failed");
    zs.next_in = (Bytef*)src; zs.avail_in = (uInt)n;
    zs.next_out = dst; zs.avail_out = (uInt)cap;
    const int rc = inflate(&zs, Z_FINISH);
    const int64_t got = (int64_t)zs.total_out;
    inflateEnd(&zs);
    if (rc != Z_STREAM_END) return fail(AFCODEC_E_CODEC, "zlib / gzip stream failed to inflate into the chunk size");
    return got;
}

/* numcodecs' LZ4 codec (Zarr v2 compressor id "lz4"): int32 decoded size, then one raw LZ4 block. */
int64_t afcodec_lz4_decode(const void* srcv, int64_t n, void* dst, int64_t cap) {
    const uint8_t* src = (const uint8_t*)srcv;
    int rc = need_lz4();
    if (rc) return rc;
    if (n < 4) return fail(AFCODEC_E_FORMAT, "lz4 chunk shorter than its size header");
    const int64_t want = (int64_t)(int32_t)le32(src);
    if (want < 0 || want > cap) return fail(AFCODEC_E_SIZE, "lz4 chunk decodes to more than its destination");
    const int got = lz4_has_zero_offset(src + 4, n - 4) ? -1 : p_lz4_dec((const char*)src + 4, (char*)dst, (int)(n - 4), (int)want);
    if (got != want) return fail(AFCODEC_E_CODEC, "lz4 block failed to decode to its recorded size");
    return want;
}

/* One chunk file -> dst, by codec kind: 0 raw bytes, 1 Blosc-1, 2 Zstandard frame, 3 zlib or gzip, 4 numcodecs LZ4.
 * kind >> 4 = element size of a byte-unshuffle stage applied AFTER the codec (HDF5's shuffle + deflate filter
 * pair, numcodecs' Shuffle filter): the codec then decodes into per-thread scratch and the planes are woven
 * into dst. */
static int64_t decode_kind_plain(int kind, const uint8_t* buf, int64_t sz, void* dst, int64_t cap);
static __thread uint8_t* t_plane;
static __thread int64_t t_plane_cap;
static int64_t decode_kind(int kind, const uint8_t* buf, int64_t sz, void* dst, int64_t cap) {
    const int es = kind >> 4;
    if (es <= 1) return decode_kind_plain(kind & 15, buf, sz, dst, cap);
    if (t_plane_cap < cap) {
        free(t_plane);
        t_plane = (uint8_t*)malloc((size_t)cap);
        t_plane_cap = t_plane ? cap : 0;
    }
    if (!t_plane) return fail(AFCODEC_E_SIZE, "out of memory");
    const int64_t got = decode_kind_plain(kind & 15, buf, sz, t_plane, cap);
    if (got < 0) return got;
    unshuffle_bytes(es, got, t_plane, (uint8_t*)dst);
    return got;
}
static int64_t decode_kind_plain(int kind, const uint8_t* buf, int64_t sz, void* dst, int64_t cap) {
    switch (kind) {
        case 0:
            if (sz > cap) return fail(AFCODEC_E_SIZE, "raw chunk larger than its destination");
            memcpy(dst, buf, (size_t)sz);
            return sz;
        case 1: return afcodec_blosc_decode(buf, sz, dst, cap);
        case 2: return afcodec_zstd_decode(buf, sz, dst, cap);
        case 3: return inflate_any(buf, sz, (uint8_t*)dst, cap);
        case 4: return afcodec_lz4_decode(buf, sz, dst, cap);
        default: return fail(AFCODEC_E_UNSUPPORTED, "unknown codec kind");
    }
}

/* dst <- src with non-temporal 16-byte stores (SSE2: every x86-64 CPU); head and tail up to alignment by memcpy */
static void nt_memcpy(uint8_t* dst, const uint8_t* src, size_t n) {
    size_t head = (16 - ((uintptr_t)dst & 15)) & 15;
    if (head > n) head = n;
    memcpy(dst, src, head);
    dst += head; src += head; n -= head;
    const size_t body = n & ~(size_t)63;
    for (size_t i = 0; i < body; i += 64) {
        const __m128i a = _mm_loadu_si128((const __m128i*)(src + i)), b = _mm_loadu_si128((const __m128i*)(src + i + 16));
        const __m128i c = _mm_loadu_si128((const __m128i*)(src + i + 32)), d = _mm_loadu_si128((const __m128i*)(src + i + 48));
        _mm_stream_si128((__m128i*)(dst + i), a); _mm_stream_si128((__m128i*)(dst + i + 16), b);
        _mm_stream_si128((__m128i*)(dst + i + 32), c); _mm_stream_si128((__m128i*)(dst + i + 48), d);
    }
    memcpy(dst + body, src + body, n - body);
    _mm_sfence();
}

/* len bytes of fd at file offset off -> dst; -> bytes read.  nt: through a cache-resident bounce buffer, then non-temporal
 * stores — the destination lines are not read first (a third less DRAM traffic than the kernel's copy into the destination),
 * which leaves an upload reading the same page-locked memory more of the host's bandwidth: store -> HBM 59 -> 67 GB/s on a
 * 3.4 GB store, 43 -> 47 on 0.86 GB (profiles/r02_nt_copy_ab.txt).  AFCODEC_NT_COPY=0: the kernel copies straight into dst. */
enum { BOUNCE = 128 << 10 };
static int nt_copy_default(void) { return nt_store_default(); }
static int64_t read_piece(int fd, uint8_t* dst, int64_t len, int64_t off, int nt) {
    int64_t done = 0;
    if (nt) {
        static __thread uint8_t bounce[BOUNCE] __attribute__((aligned(64)));
        while (done < len) {
            const int64_t want = len - done < BOUNCE ? len - done : BOUNCE;
            const ssize_t got = pread(fd, bounce, (size_t)want, (off_t)(off + done));
            if (got <= 0) break;
            nt_memcpy(dst + done, bounce, (size_t)got);
            done += got;
        }
    } else {
        while (done < len) {
            const ssize_t got = pread(fd, dst + done, (size_t)(len - done), (off_t)(off + done));
            if (got <= 0) break;
            done += got;
        }
    }
    return done;
}

/* Is a failed open / stat an ABSENT chunk?  Only "no such file" is (a Zarr chunk that was never written reads as the fill
 * value); EMFILE, EACCES, EIO ... are failures of this process or the medium and must never be mistaken for one: a batch
 * larger than RLIMIT_NOFILE used to report existing chunks as absent, and the caller silently filled them with NaN. */
static int errno_means_absent(int e) { return e == ENOENT || e == ENOTDIR; }

/* The byte range of request i: offset and size checked against the file, WITHOUT keeping a descriptor (batches hold thousands
 * of files; descriptors are opened per 1 MiB piece below, so at most one per thread is open at a time).
 * -> size >= 0, -100 for an absent file (or an empty path), AFCODEC_E_FORMAT for an unreadable file or a range beyond its end. */
static int64_t stat_range(const char* path, const int64_t* offsets, const int64_t* lengths, int64_t i, int64_t* off_out) {
    *off_out = 0;
    if (!path || !path[0]) return -100;
    int64_t off = 0, sz = -1;
    if (offsets && lengths && lengths[i] >= 0) { off = offsets[i]; sz = lengths[i]; }
    struct stat stt;
    if (stat(path, &stt) != 0) return errno_means_absent(errno) ? -100 : AFCODEC_E_FORMAT;
    if (off < 0 || off > (int64_t)stt.st_size) return AFCODEC_E_FORMAT;
    if (sz < 0) sz = (int64_t)stt.st_size - off;
    if (off + sz > (int64_t)stt.st_size) return AFCODEC_E_FORMAT;
    *off_out = off;
    return sz;
}

/* One piece of a file through the calling thread's one-entry descriptor cache: consecutive pieces of a file (the dynamic schedule
 * hands a thread runs of them) share ONE open — at most one descriptor per thread is ever held, so a batch of any size stays
 * under the descriptor limit (every file held open at once ran into EMFILE on large batches and reported existing chunks as
 * absent), without an open / close per MiB.  After the open the file is fstat'ed again: one that shrank since the sizes were
 * taken (replaced while the batch was being read) is reported as such (-2), not as a short read.
 * -> bytes read; -1: could not be opened / read, -2: the file changed. */
typedef struct { int64_t file; int fd; } fd_cache;
static int64_t read_piece_of(fd_cache* fc, int64_t file, const char* path, uint8_t* dst, int64_t len, int64_t off, int nt_copy) {
    if (fc->file != file) {
        if (fc->fd >= 0) close(fc->fd);
        fc->file = file;
        fc->fd = open(path, O_RDONLY);
    }
    if (fc->fd < 0) return -1;
    struct stat stt;
    if (fstat(fc->fd, &stt) != 0) return -1;
    if (off + len > (int64_t)stt.st_size) return -2;
    return read_piece(fc->fd, dst, len, off, nt_copy);
}

/* Reads and decodes byte ranges of chunk files -> dsts[i] on an OpenMP team (no Python between chunks):
 * [offsets[i], offsets[i] + lengths[i]) of paths[i]; lengths[i] < 0 (or offsets == NULL) = the whole file.
 * Ranges serve the inner chunks of Zarr v3 shards.  A missing file leaves results[i] = -100 (the caller
 * fills the Zarr fill value). */
int afcodec_decode_ranges(int kind, int64_t n, const char* const* paths, const int64_t* offsets, const int64_t* lengths,
                          void* const* dsts, const int64_t* dstsizes, int nthreads, int64_t* results) {
    int bad = 0;
    if (nthreads < 1) nthreads = 1;
    if ((kind & 15) == 2 && need_zstd()) return AFCODEC_E_UNSUPPORTED;
    if (kind == 0 && n > 0) {
        /* raw bytes (stores without a compressor; the compressed chunk files of the decode-in-HBM route): the files are
         * cut into 1 MiB pieces and the PIECES are spread over the team — a batch of 14 files of 12.5 MB read one file
         * per thread moved 22 GB/s out of the page cache, 227 files of 1.6 MB 60 GB/s */
        enum { PIECE = 1 << 20 };
        int64_t* first = (int64_t*)malloc((size_t)(n + 1) * sizeof(int64_t));   /* first piece of file i */
        int64_t* offs = (int64_t*)malloc((size_t)n * sizeof(int64_t));
        if (!first || !offs) { free(first); free(offs); return fail(AFCODEC_E_SIZE, "out of memory"); }
#pragma omp parallel for num_threads(nthreads) schedule(dynamic, 8)
        for (int64_t i = 0; i < n; ++i) {
            int64_t sz = stat_range(paths[i], offsets, lengths, i, &offs[i]);
            if (sz >= 0 && sz > dstsizes[i]) sz = AFCODEC_E_SIZE;
            results[i] = sz;
        }
        first[0] = 0;
        for (int64_t i = 0; i < n; ++i) first[i + 1] = first[i] + (results[i] > 0 ? (results[i] + PIECE - 1) / PIECE : 0);
        const int64_t npieces = first[n];
        int changed = 0;
#pragma omp parallel num_threads(nthreads)
        {
            fd_cache fc = {-1, -1};
#pragma omp for schedule(dynamic, 1)
            for (int64_t q = 0; q < npieces; ++q) {
                int64_t lo = 0, hi = n;                               /* the file of piece q: first[lo] <= q < first[lo + 1] */
                while (hi - lo > 1) { const int64_t mid = (lo + hi) / 2; if (first[mid] <= q) lo = mid; else hi = mid; }
                while (first[lo + 1] <= q) ++lo;                      /* (files without pieces share a boundary) */
                const int64_t at = (q - first[lo]) * PIECE, len = results[lo] - at < PIECE ? results[lo] - at : PIECE;
                int64_t o;
#pragma omp atomic read
                o = offs[lo];
                if (o < 0) continue;                                  /* an earlier piece of this file failed */
                const int64_t done = read_piece_of(&fc, lo, paths[lo], (uint8_t*)dsts[lo] + at, len, o + at, nt_copy_default());
                if (done != len) {
#pragma omp atomic write
                    offs[lo] = done == -2 ? -2 : -1;                  /* marks the file as failed (-2: it changed under the read) */
                }
            }
            if (fc.fd >= 0) close(fc.fd);
        }
        for (int64_t i = 0; i < n; ++i) {
            if (results[i] >= 0 && offs[i] < 0) { changed += offs[i] == -2; results[i] = AFCODEC_E_FORMAT; }
            if (results[i] < 0 && results[i] != -100) bad += 1;
        }
        free(first); free(offs);
        if (bad) {
            for (int64_t i = 0; i < n; ++i)
                if (results[i] == AFCODEC_E_SIZE) return fail(AFCODEC_E_CODEC, "raw chunk larger than its destination (see results[])");
            if (changed) return fail(AFCODEC_E_CODEC, "a chunk file shrank between stat and read: the store is being rewritten (see results[])");
            return fail(AFCODEC_E_CODEC, "one or more chunk files could not be read (see results[])");
        }
        return AFCODEC_OK;
    }
    if (kind == 1 && n * 2 <= nthreads) {
        /* fewer Blosc chunks than half the team: one chunk at a time, its blocks over the whole team, decoded
         * straight out of the page cache (mmap: no read() copy of a ~200 MB file in front of the decode) */
        const long page = sysconf(_SC_PAGESIZE);
        for (int64_t i = 0; i < n; ++i) {
            const int fd = open(paths[i], O_RDONLY);
            if (fd < 0) {
                if (errno_means_absent(errno)) { results[i] = -100; continue; }
                results[i] = fail(AFCODEC_E_FORMAT, "chunk file could not be opened"); bad += 1; continue;
            }
            int64_t off = 0, sz = -1;
            if (offsets && lengths && lengths[i] >= 0) { off = offsets[i]; sz = lengths[i]; }
            struct stat stt;
            int64_t r;
            if (fstat(fd, &stt) != 0) {
                r = fail(AFCODEC_E_FORMAT, "chunk file could not be read");
            } else {
                if (sz < 0) sz = (int64_t)stt.st_size - off;
                const int64_t a0 = off - off % page, span = off + sz - a0;
                void* m = (sz > 0 && off + sz <= (int64_t)stt.st_size) ? mmap(NULL, (size_t)span, PROT_READ, MAP_PRIVATE, fd, (off_t)a0) : MAP_FAILED;
                if (m == MAP_FAILED) {
                    r = fail(AFCODEC_E_FORMAT, "chunk file could not be mapped");
                } else {
                    r = afcodec_blosc_decode_mt((const uint8_t*)m + (off - a0), sz, dsts[i], dstsizes[i], nthreads);
                    munmap(m, (size_t)span);
                }
            }
            close(fd);
            results[i] = r;
            if (r < 0) bad += 1;
        }
        return bad ? fail(AFCODEC_E_CODEC, "one or more chunks failed to decode (see results[])") : AFCODEC_OK;
    }
#pragma omp parallel num_threads(nthreads) reduction(+ : bad)
    {
        uint8_t* buf = NULL;
        int64_t cap = 0;
#pragma omp for schedule(dynamic, 1)
        for (int64_t i = 0; i < n; ++i) {
            FILE* f = fopen(paths[i], "rb");
            if (!f) {
                if (errno_means_absent(errno)) { results[i] = -100; continue; }
                results[i] = fail(AFCODEC_E_FORMAT, "chunk file could not be opened"); bad += 1; continue;
            }
            int64_t off = 0, sz = -1;
            if (offsets && lengths && lengths[i] >= 0) { off = offsets[i]; sz = lengths[i]; }
            if (sz < 0) {
                fseek(f, 0, SEEK_END);
                sz = ftell(f);
            }
            int64_t r;
            if (fseek(f, (long)off, SEEK_SET) != 0) {
                r = fail(AFCODEC_E_FORMAT, "chunk range beyond the file");
            } else if (kind == 0 && sz <= dstsizes[i]) {     /* raw, no unshuffle: straight into the destination */
                r = (int64_t)fread(dsts[i], 1, (size_t)sz, f) == sz ? sz : fail(AFCODEC_E_FORMAT, "chunk file could not be read");
            } else {
                if (sz > cap) { free(buf); buf = (uint8_t*)malloc((size_t)sz + 64); cap = buf ? sz : 0; }
                if (!buf || (int64_t)fread(buf, 1, (size_t)sz, f) != sz) r = fail(AFCODEC_E_FORMAT, "chunk file could not be read");
                else r = decode_kind(kind, buf, sz, dsts[i], dstsizes[i]);
            }
            fclose(f);
            results[i] = r;
            if (r < 0) bad += 1;
        }
        free(buf);
    }
    return bad ? fail(AFCODEC_E_CODEC, "one or more chunks failed to decode (see results[])") : AFCODEC_OK;
}
/* Byte ranges of files packed back to back into ONE buffer (the compressed chunk files of the decode-in-HBM route):
 * range i lands at dst + out_off[i], out_off[i + 1] = out_off[i] + its size rounded up to `align`; results[i] = its size,
 * -100 for a missing file (or an empty path), which takes no room.  The sizes are found here (fstat on the team) — the
 * caller does not stat the files first — and the bytes are read in 1 MiB pieces spread over the team. */
int afcodec_read_packed(int64_t n, const char* const* paths, const int64_t* offsets, const int64_t* lengths, void* dst, int64_t cap,
                        int64_t align, int nthreads, int64_t* out_off, int64_t* results) {
    enum { PIECE = 1 << 20 };
    const int nt_copy = nt_copy_default();
    if (n < 0 || !dst || !out_off || !results || align < 1) return fail(AFCODEC_E_SIZE, "read_packed: bad arguments");
    if (nthreads < 1) nthreads = 1;
    out_off[0] = 0;
    if (n == 0) return AFCODEC_OK;
    int64_t* first = (int64_t*)malloc((size_t)(n + 1) * sizeof(int64_t));
    int64_t* foff = (int64_t*)malloc((size_t)n * sizeof(int64_t));
    if (!first || !foff) { free(first); free(foff); return fail(AFCODEC_E_SIZE, "out of memory"); }
#pragma omp parallel for num_threads(nthreads) schedule(dynamic, 8)
    for (int64_t i = 0; i < n; ++i) results[i] = stat_range(paths[i], offsets, lengths, i, &foff[i]);
    int bad = 0;
    first[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t sz = results[i] > 0 ? results[i] : 0;
        if (results[i] < 0 && results[i] != -100) bad += 1;
        out_off[i + 1] = out_off[i] + (sz + align - 1) / align * align;
        first[i + 1] = first[i] + (sz + PIECE - 1) / PIECE;
    }
    int too_big = !bad && out_off[n] > cap;
    if (!bad && !too_big) {
        const int64_t npieces = first[n];
#pragma omp parallel num_threads(nthreads)
        {
            fd_cache fc = {-1, -1};
#pragma omp for schedule(dynamic, 1)
            for (int64_t q = 0; q < npieces; ++q) {
                int64_t lo = 0, hi = n;                               /* the file of piece q: first[lo] <= q < first[lo + 1] */
                while (hi - lo > 1) { const int64_t mid = (lo + hi) / 2; if (first[mid] <= q) lo = mid; else hi = mid; }
                while (first[lo + 1] <= q) ++lo;
                const int64_t at = (q - first[lo]) * PIECE, len = results[lo] - at < PIECE ? results[lo] - at : PIECE;
                int64_t o;
#pragma omp atomic read
                o = foff[lo];
                if (o < 0) continue;
                const int64_t done = read_piece_of(&fc, lo, paths[lo], (uint8_t*)dst + out_off[lo] + at, len, o + at, nt_copy);
                if (done != len) {
#pragma omp atomic write
                    foff[lo] = done == -2 ? -2 : -1;                  /* marks the file as failed (-2: it changed under the read) */
                }
            }
            if (fc.fd >= 0) close(fc.fd);
        }
    }
    int changed = 0;
    for (int64_t i = 0; i < n; ++i)
        if (results[i] >= 0 && foff[i] < 0) { changed += foff[i] == -2; results[i] = AFCODEC_E_FORMAT; bad += 1; }
    free(first); free(foff);
    if (too_big) return fail(AFCODEC_E_SIZE, "read_packed: the files do not fit the buffer");
    if (changed) return fail(AFCODEC_E_CODEC, "a chunk file shrank between stat and read: the store is being rewritten (see results[])");
    return bad ? fail(AFCODEC_E_CODEC, "one or more chunk files could not be read (see results[])") : AFCODEC_OK;
}

int afcodec_decode_files(int kind, int64_t n, const char* const* paths, void* const* dsts, const int64_t* dstsizes,
                         int nthreads, int64_t* results) {
    return afcodec_decode_ranges(kind, n, paths, NULL, NULL, dsts, dstsizes, nthreads, results);
}
int afcodec_blosc_decode_files(int64_t n, const char* const* paths, void* const* dsts, const int64_t* dstsizes,
                               int nthreads, int64_t* results) {
    return afcodec_decode_files(1, n, paths, dsts, dstsizes, nthreads, results);
}

/* Encoder for the writer side (dataset_to_zarr, synthetic stores of the ingestion benchmarks): LZ4 or Zstandard streams, byte or
 * bit shuffle on request.  Readable by any Blosc-1 decoder. */
int64_t afcodec_blosc_bound(int64_t nbytes, int64_t blocksize) {
    if (blocksize <= 0) blocksize = 1 << 16;                     /* the smallest automatic block */
    /* the encoder rounds the block size DOWN to whole elements (and clamps it to the buffer): it may need up to twice the
     * blocks of the nominal size, plus the short last one */
    const int64_t nblocks = 2 * ((nbytes + blocksize - 1) / blocksize) + 2;
    return 16 + nblocks * (4 + 4 * 16) + nbytes + nbytes / 255 + 64;      /* block table + up to 16 stream headers per block */
}
static int64_t blosc_need(int64_t nbytes, int64_t blocksize) {           /* exact need for the block size actually used */
    const int64_t nblocks = (nbytes + blocksize - 1) / blocksize;
    return 16 + nblocks * (4 + 4 * 16) + nbytes + nbytes / 255 + 64;
}
/* The block size the writer uses: the geometry afcodec_blosc_encode and afcodec_blosc_encode_plan share. */
static int64_t blosc_encode_blocksize(int cname, int typesize, int64_t blocksize, int64_t nbytes) {
    if (blocksize <= 0) {
        /* LZ4, like c-blosc at level 5: 64 KiB per byte plane (blocks of 64 KiB x typesize, split into one stream per plane) */
        if (cname == 1) { blocksize = (int64_t)65536 * (typesize <= 16 ? typesize : 1); if (blocksize > (1 << 20)) blocksize = 1 << 20; }
        else blocksize = 256 << 10;
    }
    blocksize -= blocksize % typesize;
    if (blocksize < typesize) blocksize = typesize;
    if (blocksize > nbytes && nbytes > 0) blocksize = nbytes;
    /* the clamp may have left a block that is not a whole number of elements: round down again (c-blosc's compute_blocksize
     * does), so that a split block divides evenly into its byte planes and the remainder becomes the short, unsplit last
     * block — a 1001-byte buffer of 4-byte elements used to lose its last byte */
    if (blocksize > typesize) blocksize -= blocksize % typesize;
    return blocksize;
}
/* streams of a block of an LZ4 chunk: one per byte plane of a full block under a shuffle, else one (the reader's rule in blosc_block) */
static int blosc_encode_nsplits(int split, int typesize, int64_t blocksize, int last_short) {
    return (split && typesize <= 16 && blocksize / typesize >= 128 && !last_short) ? typesize : 1;
}
/* Blosc-1 writer: inner codec LZ4 (cname 1) or Zstandard (cname 4, through the system's libzstd at `level`), shuffle 0 none / 1 byte /
 * 2 bit.  LZ4 chunks are laid out as before (and as c-blosc lays out shuffled ones): split blocks of 64 KiB per byte plane, one
 * stream per plane — also under the bit shuffle, c-blosc's flags 0x24.  Zstandard chunks are what c-blosc 1.21 writes: unsplit
 * blocks (flag 0x10), one frame per block behind its int32 length, 256 KiB blocks by default (its choice at clevel 5). */
int64_t afcodec_blosc_encode(const void* srcv, int64_t nbytes, int typesize, int shuffle, int cname, int level, int64_t blocksize,
                             void* dstv, int64_t cap) {
    const uint8_t* src = (const uint8_t*)srcv;
    uint8_t* dst = (uint8_t*)dstv;
    if (cname != 1 && cname != 4) return fail(AFCODEC_E_UNSUPPORTED, "blosc_encode writes LZ4 (1) or Zstandard (4) streams");
    if (shuffle < 0 || shuffle > 2) return fail(AFCODEC_E_SIZE, "shuffle is 0 (none), 1 (byte) or 2 (bit)");
    int rc = cname == 1 ? need_lz4() : need_zstd();
    if (rc) return rc;
    if (cname == 4 && !p_zstd_enc) return fail(AFCODEC_E_UNSUPPORTED, "libzstd has no ZSTD_compress");
    if (nbytes < 0 || nbytes > 0x7fffffffLL - 64 || typesize < 1 || typesize > 255) return fail(AFCODEC_E_SIZE, "bad nbytes / typesize");
    blocksize = blosc_encode_blocksize(cname, typesize, blocksize, nbytes);
    if (cap < blosc_need(nbytes, blocksize)) return fail(AFCODEC_E_SIZE, "destination smaller than afcodec_blosc_bound()");
    const int do_shuf = shuffle == 1 && typesize > 1, do_bits = shuffle == 2;
    const int filter = do_shuf ? 0x01 : (do_bits ? 0x04 : 0);
    dst[0] = 2; dst[1] = 1; dst[3] = (uint8_t)typesize;
    put32(dst + 4, (uint32_t)nbytes);
    if (nbytes < 128) {                                      /* tiny buffers are stored */
        dst[2] = (uint8_t)(0x02 | filter | (cname << 5) | 0x10);
        put32(dst + 8, (uint32_t)(nbytes ? nbytes : typesize));
        memcpy(dst + 16, src, (size_t)nbytes);
        put32(dst + 12, (uint32_t)(16 + nbytes));
        return 16 + nbytes;
    }
    /* split blocks (flag 0x10 clear), as c-blosc writes LZ4 chunks: a full block of a shuffled buffer is typesize
     * streams, one per byte plane; the short last block is one stream (the reader's rule in blosc_block) */
    const int split = cname == 1 && filter != 0;
    dst[2] = (uint8_t)(filter | (split ? 0 : 0x10) | (cname << 5));
    put32(dst + 8, (uint32_t)blocksize);
    const int64_t nblocks = (nbytes + blocksize - 1) / blocksize;
    const int64_t leftover = nbytes % blocksize;
    uint8_t* tmp = filter ? (uint8_t*)malloc((size_t)blocksize) : NULL;
    if (filter && !tmp) return fail(AFCODEC_E_SIZE, "out of memory");
    int64_t pos = 16 + 4 * nblocks;
    for (int64_t b = 0; b < nblocks; ++b) {
        const int last_short = (b == nblocks - 1) && leftover > 0;
        const int64_t bsize = last_short ? leftover : blocksize;
        const uint8_t* in = src + b * blocksize;
        if (do_shuf) { shuffle_bytes(typesize, bsize, in, tmp); in = tmp; }
        else if (do_bits && bsize >= typesize) { shuffle_bits(typesize, bsize, in, tmp); in = tmp; }
        put32(dst + 16 + 4 * b, (uint32_t)pos);
        const int nsplits = blosc_encode_nsplits(split, typesize, blocksize, last_short);
        const int64_t ne = bsize / nsplits;
        for (int j = 0; j < nsplits; ++j) {
            int64_t csz = 0;                                    /* stays 0 if the stream does not shrink */
            if (cname == 1) csz = p_lz4_enc((const char*)in + j * ne, (char*)dst + pos + 4, (int)ne, (int)(ne - 1));
            else if (ne > 1) {
                const size_t got = p_zstd_enc(dst + pos + 4, (size_t)(ne - 1), in + j * ne, (size_t)ne, level);
                csz = p_zstd_iserr(got) ? 0 : (int64_t)got;
            }
            if (csz <= 0) { memcpy(dst + pos + 4, in + j * ne, (size_t)ne); csz = ne; }
            put32(dst + pos, (uint32_t)csz);
            pos += 4 + csz;
        }
    }
    free(tmp);
    put32(dst + 12, (uint32_t)pos);
    return pos;
}

int64_t afcodec_blosc_encode_lz4(const void* src, int64_t nbytes, int typesize, int shuffle, int64_t blocksize, void* dst, int64_t cap) {
    return afcodec_blosc_encode(src, nbytes, typesize, shuffle ? 1 : 0, 1, 0, blocksize, dst, cap);
}

/* ---- the write side in HBM (libaggfly_hip: afhip_shuffle_blocks, afhip_lz4_encode_streams, afhip_copy_ranges) ---- */
#include "lz4_encode_pass.h"

/* The encoder of lz4_encode_pass.h as the kernel runs it, on the host: src[0 .. n) -> dst (cap >= n) -> csize; n = stored. */
int64_t afcodec_lz4_encode_emulate(const void* src, int64_t n, void* dst, int64_t cap) {
    if (n < 0 || n > 0x7fffffffLL || (n && (!src || !dst))) return fail(AFCODEC_E_SIZE, "lz4_encode_emulate: bad arguments");
    if (cap < n) return fail(AFCODEC_E_SIZE, "lz4_encode_emulate: the slot holds fewer than n bytes");
    uint32_t* table = (uint32_t*)malloc(sizeof(uint32_t) * AFL_TABLE_ENTRIES);
    if (!table) return fail(AFCODEC_E_SIZE, "out of memory");
    const int32_t c = afl_encode_wave((const uint8_t*)src, (int32_t)n, (uint8_t*)dst, table, 0, 0);
    free(table);
    return c;
}

/* Geometry of n chunks of nbytes bytes each, chunk i at offset i * nbytes of the chunk buffer, written as afcodec_blosc_encode writes
 * LZ4 chunks under the byte shuffle with the automatic block size. */
int afcodec_blosc_encode_plan(int64_t n, int64_t nbytes, int typesize, void* streams_v, int64_t cap_streams, int64_t* n_streams,
                              void* blocks_v, int64_t cap_blocks, int64_t* n_blocks, int64_t* layout) {
    typedef struct { int64_t src_off, dst_off; int32_t csize, dsize, to_out, pad; } stream_rec;   /* == afhip_lz4_stream */
    typedef struct { int64_t tmp_off, out_off; int32_t bsize, typesize; } shuf_rec;               /* == afhip_shuffle_block */
    stream_rec* st = (stream_rec*)streams_v;
    shuf_rec* bl = (shuf_rec*)blocks_v;
    if (n < 0 || nbytes <= 0 || nbytes > 0x7fffffffLL - 64 || typesize < 1 || typesize > 255 || !n_streams || !n_blocks || !layout)
        return fail(AFCODEC_E_SIZE, "blosc_encode_plan: bad n / nbytes / typesize");
    const int cname = 1, filter = typesize > 1 ? 0x01 : 0, split = filter != 0;
    const int stored = nbytes < 128;                         /* tiny buffers are stored */
    const int64_t blocksize = stored ? nbytes : blosc_encode_blocksize(cname, typesize, 0, nbytes);
    const int64_t nblocks = stored ? 1 : (nbytes + blocksize - 1) / blocksize, leftover = stored ? 0 : nbytes % blocksize;
    int64_t per_chunk = 0;
    for (int64_t b = 0; b < nblocks; ++b) per_chunk += blosc_encode_nsplits(split && !stored, typesize, blocksize, b == nblocks - 1 && leftover > 0);
    layout[0] = stored ? nbytes : blocksize;                 /* header field */
    layout[1] = stored ? 0 : nblocks;                        /* entries of the bstarts table */
    layout[2] = per_chunk;                                   /* streams per chunk */
    layout[3] = stored ? (0x02 | filter | (cname << 5) | 0x10) : (filter | (split ? 0 : 0x10) | (cname << 5));
    layout[4] = stored ? 0 : 4;                              /* bytes of the length field in front of every stream */
    *n_streams = n * per_chunk;
    *n_blocks = n * nblocks;
    if (!st && !bl) return AFCODEC_OK;                       /* the counts and the layout alone */
    if (!st || !bl || *n_streams > cap_streams || *n_blocks > cap_blocks) return fail(AFCODEC_E_SIZE, "blosc_encode_plan: record list too small");
    int64_t si = 0, bi = 0;
    for (int64_t c = 0; c < n; ++c) {
        for (int64_t b = 0; b < nblocks; ++b) {
            const int last_short = b == nblocks - 1 && leftover > 0;
            const int64_t bsize = last_short ? leftover : blocksize, off = c * nbytes + b * blocksize;
            bl[bi].tmp_off = bl[bi].out_off = off;
            bl[bi].bsize = (int32_t)bsize;
            bl[bi].typesize = (filter && !stored) ? typesize : 1;        /* (a stored chunk holds the raw bytes: a copy) */
            ++bi;
            const int nsplits = blosc_encode_nsplits(split && !stored, typesize, blocksize, last_short);
            const int64_t ne = bsize / nsplits;
            for (int j = 0; j < nsplits; ++j, ++si) {
                st[si].src_off = st[si].dst_off = off + j * ne;
                st[si].csize = 0;
                st[si].dsize = (int32_t)ne;
                st[si].to_out = stored;
                st[si].pad = (int32_t)b;
            }
        }
    }
    return AFCODEC_OK;
}

/* ---- the same for Zstandard streams (libaggfly_hip: afhip_zstd_encode_blocks) ---- */
#include "zstd_encode_pass.h"

/* The encoder of zstd_encode_pass.h as the kernel runs it, on the host: src[0 .. n) -> one block (header and content) at dst
 * (cap >= n + 3) -> its bytes. */
int64_t afcodec_zstd_encode_block_emulate(const void* src, int64_t n, int last, void* dst, int64_t cap) {
    if (n < 1 || n > AFZ_BLOCK_MAX || !src || !dst) return fail(AFCODEC_E_SIZE, "zstd_encode_block_emulate: a block holds 1 .. 131072 bytes");
    if (cap < n + 3) return fail(AFCODEC_E_SIZE, "zstd_encode_block_emulate: the slot holds fewer than n + 3 bytes");
    uint32_t* lds = (uint32_t*)malloc(sizeof(uint32_t) * AFZE_LDS_WORDS);
    uint8_t* tables = (uint8_t*)malloc(AFZE_TAB_BYTES);
    uint8_t* scratch = (uint8_t*)malloc((size_t)afze_scratch_bytes((int32_t)n));
    int64_t c = fail(AFCODEC_E_SIZE, "out of memory");
    if (lds && tables && scratch) {
        afze_build_tables(tables);
        c = afze_encode_block((const uint8_t*)src, (int32_t)n, last, (uint8_t*)dst, scratch, tables, lds, 0);
    }
    free(scratch);
    free(tables);
    free(lds);
    return c;
}

int64_t afcodec_zstd_encode_scratch_bytes(int64_t n) {
    return n <= 0 ? AFZE_TAB_BYTES + (256 - AFZE_TAB_BYTES % 256) % 256 : (n > AFZ_BLOCK_MAX ? -1 : afze_scratch_bytes((int32_t)n));
}

/* The pieces a shuffled Blosc block of bsize bytes is cut into, each one block of its frame: the byte planes when a plane holds 1 ..
 * 128 KiB (then the bsize % typesize trailing bytes, if any), else pieces of 128 KiB.  piece k -> its offset in the block; -> its bytes
 * (0: no such piece). */
static int64_t zstd_encode_piece(int64_t bsize, int typesize, int64_t k, int64_t* off) {
    const int64_t plane = bsize / typesize;
    if (typesize > 1 && plane >= 1 && plane <= AFZ_BLOCK_MAX) {
        if (k < typesize) { *off = k * plane; return plane; }
        *off = (int64_t)typesize * plane;
        return k == typesize ? bsize - *off : 0;
    }
    *off = k * AFZ_BLOCK_MAX;
    return *off >= bsize ? 0 : (bsize - *off < AFZ_BLOCK_MAX ? bsize - *off : AFZ_BLOCK_MAX);
}

/* Geometry of n chunks of nbytes bytes each, written as afcodec_blosc_encode writes Zstandard chunks under the byte shuffle with the
 * automatic block size: unsplit blocks, one frame per block, every frame cut into blocks by zstd_encode_piece. */
int afcodec_blosc_zstd_encode_plan(int64_t n, int64_t nbytes, int typesize, void* zblocks_v, int64_t cap_zblocks, int64_t* n_zblocks,
                                   void* blocks_v, int64_t cap_blocks, int64_t* n_blocks, int64_t* layout) {
    typedef struct { int64_t src_off, dst_off, scratch_off; int32_t n, last; } zblock_rec;      /* == afhip_zstd_encode_block */
    typedef struct { int64_t tmp_off, out_off; int32_t bsize, typesize; } shuf_rec;            /* == afhip_shuffle_block */
    zblock_rec* zb = (zblock_rec*)zblocks_v;
    shuf_rec* bl = (shuf_rec*)blocks_v;
    if (n < 0 || nbytes <= 0 || nbytes > 0x7fffffffLL - 64 || typesize < 1 || typesize > 255 || !n_zblocks || !n_blocks || !layout)
        return fail(AFCODEC_E_SIZE, "blosc_zstd_encode_plan: bad n / nbytes / typesize");
    const int cname = 4, filter = typesize > 1 ? 0x01 : 0;
    const int stored = nbytes < 128;                         /* tiny buffers are stored */
    const int64_t blocksize = stored ? nbytes : blosc_encode_blocksize(cname, typesize, 0, nbytes);
    const int64_t nblocks = stored ? 1 : (nbytes + blocksize - 1) / blocksize, leftover = stored ? 0 : nbytes % blocksize;
    int64_t per_chunk = 0, slot_chunk = 0, scratch_chunk = 0;
    for (int64_t b = 0; b < nblocks && !stored; ++b) {
        const int64_t bsize = b == nblocks - 1 && leftover > 0 ? leftover : blocksize;
        int64_t off, len;
        for (int64_t k = 0; (len = zstd_encode_piece(bsize, filter ? typesize : 1, k, &off)) > 0; ++k) {
            ++per_chunk;
            slot_chunk += len + 3;
            scratch_chunk += afze_scratch_bytes((int32_t)len);
        }
    }
    const int64_t tables = afcodec_zstd_encode_scratch_bytes(0);
    layout[0] = stored ? nbytes : blocksize;                 /* header field */
    layout[1] = stored ? 0 : nblocks;                        /* entries of the bstarts table = frames */
    layout[2] = per_chunk;                                   /* Zstandard blocks per chunk */
    layout[3] = stored ? (0x02 | filter | (cname << 5) | 0x10) : (filter | 0x10 | (cname << 5));
    layout[4] = stored ? 0 : 4;                              /* bytes of the length field in front of every frame */
    layout[5] = (n * nbytes + 255) & ~(int64_t)255;          /* the slots' first byte in the work buffer, behind the shuffled input */
    layout[6] = n * slot_chunk;                              /* bytes of the slots */
    layout[7] = tables + n * scratch_chunk;                  /* bytes of the encoder's scratch */
    *n_zblocks = n * per_chunk;
    *n_blocks = n * nblocks;
    if (!zb && !bl) return AFCODEC_OK;                       /* the counts and the layout alone */
    if (!bl || (!zb && *n_zblocks) || *n_zblocks > cap_zblocks || *n_blocks > cap_blocks)
        return fail(AFCODEC_E_SIZE, "blosc_zstd_encode_plan: record list too small");
    int64_t zi = 0, bi = 0, slot = 0, scratch = tables;
    for (int64_t c = 0; c < n; ++c) {
        for (int64_t b = 0; b < nblocks; ++b) {
            const int last_short = b == nblocks - 1 && leftover > 0;
            const int64_t bsize = last_short ? leftover : blocksize, at = c * nbytes + b * blocksize;
            bl[bi].tmp_off = bl[bi].out_off = at;
            bl[bi].bsize = (int32_t)bsize;
            bl[bi].typesize = (filter && !stored) ? typesize : 1;        /* (a stored chunk holds the raw bytes: a copy) */
            ++bi;
            if (stored) continue;
            int64_t off, len;
            for (int64_t k = 0; (len = zstd_encode_piece(bsize, filter ? typesize : 1, k, &off)) > 0; ++k, ++zi) {
                int64_t off2;
                zb[zi].src_off = at + off;
                zb[zi].dst_off = slot;
                zb[zi].scratch_off = scratch;
                zb[zi].n = (int32_t)len;
                zb[zi].last = zstd_encode_piece(bsize, filter ? typesize : 1, k + 1, &off2) == 0;
                slot += len + 3;
                scratch += afze_scratch_bytes((int32_t)len);
            }
        }
    }
    return AFCODEC_OK;
}

/* Plain Zstandard frames (Zarr compressor id "zstd"). */
int64_t afcodec_zstd_decode(const void* src, int64_t n, void* dst, int64_t cap) {
    int rc = need_zstd();
    if (rc) return rc;
    const size_t got = p_zstd_dec(dst, (size_t)cap, src, (size_t)n);
    if (p_zstd_iserr(got)) return fail(AFCODEC_E_CODEC, "zstd frame failed to decode");
    return (int64_t)got;
}

/* Zstandard frame of src (writer side of Zarr v3 stores); cap >= afcodec_zstd_bound(n). */
int64_t afcodec_zstd_bound(int64_t n) {
    if (need_zstd() || !p_zstd_bound) return n + n / 128 + 512;
    return (int64_t)p_zstd_bound((size_t)n);
}
int64_t afcodec_zstd_encode(const void* src, int64_t n, int level, void* dst, int64_t cap) {
    int rc = need_zstd();
    if (rc) return rc;
    if (!p_zstd_enc) return fail(AFCODEC_E_UNSUPPORTED, "libzstd has no ZSTD_compress");
    const size_t got = p_zstd_enc(dst, (size_t)cap, src, (size_t)n, level);
    if (p_zstd_iserr(got)) return fail(AFCODEC_E_CODEC, "zstd compression failed");
    return (int64_t)got;
}

/* ---- plan of a GPU-side Zstandard decode (include/aggfly_codec.h: afcodec_zstd_plan) ----
 * Walks the frame header, the block headers and, in compressed blocks, the literals and sequences section headers (RFC
 * 8878 §3.1.1); of the entropy descriptions it reads only as much as gives their sizes (an FSE table description has to be
 * walked to find where the next one begins).  Building the tables and decoding is the GPU's (zstd_passes.h). */

static int zstd_literals_header(const uint8_t* q, int64_t bs, afz_block* k) {
    if (bs < 1) return -1;
    const int lt = q[0] & 3, sf = (q[0] >> 2) & 3;
    int64_t hs, regen, comp = 0;
    k->lit_type = lt; k->n_streams = 1; k->huf_desc = -1; k->lit_csize = 0;
    if (lt < 2) {
        hs = (sf & 1) == 0 ? 1 : (sf == 1 ? 2 : 3);
        if (hs > bs) return -1;
        regen = hs == 1 ? q[0] >> 3 : (hs == 2 ? (q[0] >> 4) + (q[1] << 4) : (q[0] >> 4) + (q[1] << 4) + ((int64_t)q[2] << 12));
        comp = lt == 0 ? regen : 1;
        k->lit_src = (int32_t)hs;
    } else {
        hs = sf < 2 ? 3 : sf + 2;
        if (hs > bs) return -1;
        const uint64_t h = (uint64_t)q[0] | ((uint64_t)q[1] << 8) | ((uint64_t)q[2] << 16) | (hs > 3 ? (uint64_t)q[3] << 24 : 0) |
                           (hs > 4 ? (uint64_t)q[4] << 32 : 0);
        const int bits = hs == 3 ? 10 : (hs == 4 ? 14 : 18);
        regen = (int64_t)((h >> 4) & ((1u << bits) - 1));
        comp = (int64_t)((h >> (4 + bits)) & ((1u << bits) - 1));
        k->n_streams = sf == 0 ? 1 : 4;
        if (hs + comp > bs) return -1;
        int64_t desc = 0;
        if (lt == 2) {
            if (comp < 1) return -1;
            const int hb = q[hs];
            desc = hb < 128 ? 1 + hb : 1 + (hb - 127 + 1) / 2;
            k->huf_desc = (int32_t)hs;
        }
        k->lit_src = (int32_t)(hs + desc);
        k->lit_csize = (int32_t)(comp - desc);
        if (k->lit_csize < (k->n_streams == 4 ? 10 : 1)) return -1;
    }
    if (regen > AFZ_BLOCK_MAX || hs + comp > bs) return -1;
    k->lit_size = (int32_t)regen;
    return (int)(hs + comp);
}

/* The walk itself, for afcodec_zstd_plan (all n frames of a batch) and for the Blosc walk (n = 1: the frame of one Blosc block):
 * records are appended to the lists and totals of *z, which a frame that fails leaves as they were. */
static int zstd_plan_frames(zstd_lists* z, const void* base, int64_t n, const int64_t* comp_off, const int64_t* comp_size, const int64_t* out_off,
                            const int64_t* out_size, int64_t* results) {
    afz_frame* frames = z->frames;
    afz_block* blocks = z->blocks;
    const int64_t cap_frames = z->cap_frames, cap_blocks = z->cap_blocks;
    int64_t nf = z->nf, nb = z->nb, lit = z->lit, nsq = z->nsq, dec = z->dec;
    int rc_all = AFCODEC_OK;
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t* c = (const uint8_t*)base + comp_off[i];
        const int64_t csz = comp_size[i];
        const int64_t nb0 = nb, lit0 = lit, nsq0 = nsq;
        int bad = 0;
        const char* why = "malformed frame";
        results[i] = 0;
#define ZBAD(code, msg) do { bad = (code); why = (msg); goto done; } while (0)
        if (csz < 4) ZBAD(AFCODEC_E_FORMAT, "shorter than a frame header");
        const uint32_t magic = le32(c);
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) ZBAD(AFCODEC_E_UNSUPPORTED, "skippable frame: decode on the host");
        if (magic != 0xFD2FB528u) ZBAD(AFCODEC_E_FORMAT, "not a Zstandard frame");
        if (csz < 6) ZBAD(AFCODEC_E_FORMAT, "truncated frame header");
        {
            const int fhd = c[4], fcs_flag = fhd >> 6, single = (fhd >> 5) & 1, did_flag = fhd & 3;
            if (fhd & 0x08) ZBAD(AFCODEC_E_FORMAT, "reserved frame header bit set");
            int64_t pos = 5 + (single ? 0 : 1);
            const int did_size = did_flag == 0 ? 0 : (did_flag == 1 ? 1 : (did_flag == 2 ? 2 : 4));
            const int fcs_size = fcs_flag == 0 ? (single ? 1 : 0) : (fcs_flag == 1 ? 2 : (fcs_flag == 2 ? 4 : 8));
            if (pos + did_size + fcs_size > csz) ZBAD(AFCODEC_E_FORMAT, "truncated frame header");
            uint64_t did = 0, fcs = 0;
            for (int j = 0; j < did_size; ++j) did |= (uint64_t)c[pos + j] << (8 * j);
            pos += did_size;
            for (int j = 0; j < fcs_size; ++j) fcs |= (uint64_t)c[pos + j] << (8 * j);
            pos += fcs_size;
            if (fcs_size == 2) fcs += 256;
            if (did) ZBAD(AFCODEC_E_UNSUPPORTED, "frame needs a dictionary: decode on the host");
            if (!fcs_size) ZBAD(AFCODEC_E_UNSUPPORTED, "frame without Frame_Content_Size: decode on the host");
            if (fhd & 0x04) ZBAD(AFCODEC_E_UNSUPPORTED, "frame with a content checksum: decode on the host");
            if ((int64_t)fcs != out_size[i] || fcs > 0x7fffffffu)
                ZBAD(AFCODEC_E_UNSUPPORTED, "Frame_Content_Size differs from the chunk size: decode on the host");
            if (nf >= cap_frames) return fail(AFCODEC_E_SIZE, "frame list too small");
            int32_t huf = -1, tmode[3] = {-1, -1, -1}, tsym[3] = {0, 0, 0}, tblk[3] = {0, 0, 0}, tdesc[3] = {0, 0, 0};
            for (;;) {
                if (pos + 3 > csz) ZBAD(AFCODEC_E_FORMAT, "truncated block header");
                const uint32_t bh = (uint32_t)c[pos] | ((uint32_t)c[pos + 1] << 8) | ((uint32_t)c[pos + 2] << 16);
                const int last = bh & 1, bt = (bh >> 1) & 3;
                const int64_t bs = bh >> 3;
                if (bt == 3) ZBAD(AFCODEC_E_FORMAT, "reserved block type");
                if (bs > AFZ_BLOCK_MAX) ZBAD(AFCODEC_E_FORMAT, "block larger than 128 KiB");
                const int64_t csize = bt == 1 ? 1 : bs;
                pos += 3;
                if (pos + csize > csz) ZBAD(AFCODEC_E_FORMAT, "block beyond the chunk");
                if (nb >= cap_blocks) return fail(AFCODEC_E_SIZE, "block list too small");
                afz_block k;
                memset(&k, 0, sizeof k);
                k.src = comp_off[i] + pos; k.frame = (int32_t)nf; k.btype = bt; k.csize = (int32_t)csize;
                k.huf_desc = -1; k.huf_block = -1; k.n_streams = 1;
                if (bt < 2) {
                    k.lit_type = bt; k.lit_size = (int32_t)bs; k.lit_src = 0;
                } else {
                    const uint8_t* q = c + pos;
                    const int ls = zstd_literals_header(q, bs, &k);
                    if (ls < 0) ZBAD(AFCODEC_E_FORMAT, "malformed literals section header");
                    if (k.lit_type == 2) huf = (int32_t)nb;
                    if (k.lit_type >= 2) {
                        if (huf < 0) ZBAD(AFCODEC_E_FORMAT, "treeless literals without an earlier Huffman table");
                        k.huf_block = huf;
                    }
                    int64_t s = ls;
                    if (s >= bs) ZBAD(AFCODEC_E_FORMAT, "no sequences section");
                    const int b0 = q[s];
                    if (b0 == 0) { k.nseq = 0; s += 1; if (s != bs) ZBAD(AFCODEC_E_FORMAT, "bytes after an empty sequences section"); }
                    else {
                        if (b0 < 128) { k.nseq = b0; s += 1; }
                        else if (b0 < 255) { if (s + 2 > bs) ZBAD(AFCODEC_E_FORMAT, "truncated sequences header"); k.nseq = ((b0 - 128) << 8) + q[s + 1]; s += 2; }
                        else { if (s + 3 > bs) ZBAD(AFCODEC_E_FORMAT, "truncated sequences header"); k.nseq = q[s + 1] + (q[s + 2] << 8) + 0x7F00; s += 3; }
                        if (k.nseq > AFZ_BLOCK_MAX / 3) ZBAD(AFCODEC_E_FORMAT, "more sequences than a block holds");
                        if (s >= bs) ZBAD(AFCODEC_E_FORMAT, "truncated sequences header");
                        const int modes = q[s++];
                        if (modes & 3) ZBAD(AFCODEC_E_FORMAT, "reserved bits of the compression modes set");
                        for (int t = 0; t < 3; ++t) {
                            const int m = (modes >> (6 - 2 * t)) & 3;
                            if (m == 0) { tmode[t] = 0; }
                            else if (m == 1) {
                                if (s >= bs) ZBAD(AFCODEC_E_FORMAT, "truncated RLE symbol");
                                if (q[s] > afz_max_sym[t]) ZBAD(AFCODEC_E_FORMAT, "RLE symbol out of range");
                                tmode[t] = 1; tsym[t] = q[s++];
                            } else if (m == 2) {
                                int16_t norm[64];
                                int nsym, lg;
                                const int used = afz_read_ncount(q + s, bs - s, norm, afz_max_sym[t], afz_max_log[t], &nsym, &lg);
                                if (used < 0) ZBAD(AFCODEC_E_FORMAT, "malformed FSE table description");
                                tmode[t] = 2; tblk[t] = (int32_t)nb; tdesc[t] = (int32_t)s;
                                s += used;
                            } else if (tmode[t] < 0) ZBAD(AFCODEC_E_FORMAT, "repeat mode without an earlier table");
                            k.mode[t] = tmode[t];
                            k.tab_desc[t] = tmode[t] == 1 ? tsym[t] : (tmode[t] == 2 ? tdesc[t] : 0);
                            k.tab_block[t] = tmode[t] == 2 ? tblk[t] : -1;
                        }
                        if (s >= bs) ZBAD(AFCODEC_E_FORMAT, "no sequences bitstream");
                    }
                    k.seq_src = (int32_t)s;
                }
                k.lit_off = lit; k.seq_off = nsq;
                lit += k.lit_size; nsq += k.nseq;
                if (lit - lit0 + 3 * (nsq - nsq0) > (int64_t)fcs)      /* (every sequence adds a match of 3 bytes or more) */
                    ZBAD(AFCODEC_E_FORMAT, "more literals and sequences than Frame_Content_Size holds");
                blocks[nb++] = k;
                pos += csize;
                if (last) break;
            }
            if (pos != csz) ZBAD(AFCODEC_E_UNSUPPORTED, "bytes after the frame (another frame?): decode on the host");
            frames[nf++] = (afz_frame){out_off[i], dec, (int64_t)fcs, (int32_t)nb0, (int32_t)(nb - nb0)};
            dec += (int64_t)fcs;
            results[i] = (int64_t)fcs;
        }
    done:
#undef ZBAD
        if (bad) {
            nb = nb0; lit = lit0; nsq = nsq0;
            results[i] = bad;
            rc_all = fail(bad, why);
        }
    }
    z->nf = nf; z->nb = nb; z->lit = lit; z->nsq = nsq; z->dec = dec;
    return rc_all;
}

int afcodec_zstd_plan(const void* base, int64_t n, const int64_t* comp_off, const int64_t* comp_size, const int64_t* out_off,
                      const int64_t* out_size, void* frames_v, int64_t cap_frames, int64_t* n_frames, void* blocks_v, int64_t cap_blocks,
                      int64_t* n_blocks, int64_t* lit_bytes, int64_t* n_seqs, int64_t* dec_bytes, int64_t* results) {
    zstd_lists z = {(afz_frame*)frames_v, cap_frames, 0, (afz_block*)blocks_v, cap_blocks, 0, 0, 0, 0};
    const int rc = zstd_plan_frames(&z, base, n, comp_off, comp_size, out_off, out_size, results);
    *n_frames = z.nf; *n_blocks = z.nb; *lit_bytes = z.lit; *n_seqs = z.nsq; *dec_bytes = z.dec;
    return rc;
}

int64_t afcodec_zstd_scratch_bytes(int64_t n_blocks, int64_t n_frames, int64_t lit_bytes, int64_t n_seqs, int64_t dec_bytes) {
    int64_t o[9];
    return afz_layout(n_blocks, n_frames, lit_bytes, n_seqs, dec_bytes, o);
}

/* The passes of the GPU decode (zstd_passes.h) run in order on this thread: the host reference of afhip_zstd_decode. */
int afcodec_zstd_emulate(const void* comp, int64_t comp_bytes, const void* frames, int64_t n_frames, const void* blocks,
                         int64_t n_blocks, int64_t lit_bytes, int64_t n_seqs, int64_t dec_bytes, void* scratch, void* out,
                         int32_t* errors, int32_t* rounds) {
    afz_ctx x;
    memset(&x, 0, sizeof x);
    x.comp = (const uint8_t*)comp; x.comp_bytes = comp_bytes;
    x.frames = (const afz_frame*)frames; x.n_frames = n_frames;
    x.blocks = (const afz_block*)blocks; x.n_blocks = n_blocks;
    afz_bind(&x, (uint8_t*)scratch, n_blocks, n_frames, lit_bytes, n_seqs, dec_bytes);
    x.out = (uint8_t*)out; x.errors = errors;
    memset(x.bad, 0, (size_t)(n_frames + 64) * 4);
    for (int64_t b = 0; b <= n_blocks; ++b) afz_pass_tables(&x, b);
    for (int64_t b = 0; b < n_blocks; ++b)
        for (int q = 0; q < 4; ++q) afz_pass_literals(&x, b, q, NULL);
    for (int64_t b = 0; b < n_blocks; ++b) afz_pass_sequences(&x, b);
    for (int64_t f = 0; f < n_frames; ++f) afz_pass_frame(&x, f);
    for (int64_t b = 0; b < n_blocks; ++b) afz_pass_fill(&x, b, 0, 1);
    const int R = afz_rounds_host(dec_bytes);
    int r = 0;
    for (; r < R && x.flags[r]; ++r) {
        int more = 0;
        for (int64_t p = 0; p < dec_bytes; ++p) more |= afz_jump(&x, p);
        x.flags[r + 1] = more;
    }
    for (int64_t b = 0; b < n_blocks; ++b) afz_pass_gather(&x, b, 0, 1);
    if (rounds) *rounds = r;
    return AFCODEC_OK;
}

/* ---- plan of a GPU-side zlib decode (include/aggfly_codec.h: afcodec_inflate_plan) ----
 * Only the zlib wrapper is read (RFC 1950 §2.2): deflate's block boundaries are found by decoding, which is the GPU's
 * (inflate_passes.h). */
#include "inflate_passes.h"

int afcodec_inflate_plan(const void* base, int64_t n, const int64_t* comp_off, const int64_t* comp_size, const int64_t* out_off,
                         const int64_t* out_size, const int32_t* typesize, void* streams_v, int64_t cap_streams, int64_t* n_streams, void* shuf_v,
                         int64_t cap_shuf, int64_t* n_shuf, int64_t* n_pblocks, int64_t* n_seqs, int64_t* n_pieces, int64_t* dec_bytes,
                         int64_t* tmp_bytes, int64_t* results) {
    typedef struct { int64_t tmp_off, out_off; int32_t bsize, typesize; } shuf_rec;      /* == afhip_shuffle_block */
    afi_stream* streams = (afi_stream*)streams_v;
    shuf_rec* shuf = (shuf_rec*)shuf_v;
    int64_t ns = 0, nsh = 0, nb = 0, nsq = 0, np = 0, dec = 0, tmp = 0;
    int rc_all = AFCODEC_OK;
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t* c = (const uint8_t*)base + comp_off[i];
        const int64_t csz = comp_size[i], dsz = out_size[i];
        const int ts = typesize ? typesize[i] : 1;
        int bad = 0;
        const char* why = "";
        if (ts < 1 || ts > 255) return fail(AFCODEC_E_SIZE, "inflate_plan: element size out of range");
        if (csz < 2) { bad = AFCODEC_E_FORMAT; why = "shorter than a zlib header"; }
        else if (c[0] == 0x1f && c[1] == 0x8b) { bad = AFCODEC_E_UNSUPPORTED; why = "gzip member: decode on the host"; }
        else if ((c[0] & 15) != 8 || (c[0] >> 4) > 7 || ((c[0] << 8) | c[1]) % 31) { bad = AFCODEC_E_FORMAT; why = "not a zlib stream"; }
        else if (c[1] & 0x20) { bad = AFCODEC_E_UNSUPPORTED; why = "zlib stream with a preset dictionary: decode on the host"; }
        else if (dsz < 0 || dsz >= ((int64_t)1 << 30) || csz > 0x7fffffff) { bad = AFCODEC_E_UNSUPPORTED; why = "chunk of 1 GiB or more: decode on the host"; }
        else if (dec + dsz > 0x7fffffff) return fail(AFCODEC_E_SIZE, "inflate_plan: more than 2 GiB decoded in one batch");
        if (bad) {
            results[i] = bad;
            rc_all = fail(bad, why);
            continue;
        }
        const int shuffled = ts > 1 && dsz >= ts;
        if (ns >= cap_streams || (shuffled && nsh >= cap_shuf)) return fail(AFCODEC_E_SIZE, "stream list too small");
        afi_stream s;
        memset(&s, 0, sizeof s);
        s.src = comp_off[i]; s.csize = (int32_t)csz; s.dsize = (int32_t)dsz;
        s.base = dec; s.seq_off = nsq;
        s.first_block = (int32_t)nb; s.n_blocks = (int32_t)(dsz / AFI_PBLOCK_MIN + 1);
        s.first_piece = (int32_t)np;
        if (shuffled) {
            s.to_out = 0; s.dst_off = tmp;
            shuf[nsh++] = (shuf_rec){tmp, out_off[i], (int32_t)dsz, ts};
            tmp += (dsz + 15) & ~(int64_t)15;
        } else {
            s.to_out = 1; s.dst_off = out_off[i];
        }
        streams[ns++] = s;
        nb += s.n_blocks; nsq += dsz / 3 + 1; np += (dsz + AFI_PIECE - 1) / AFI_PIECE; dec += dsz;
        results[i] = dsz;
    }
    *n_streams = ns; *n_shuf = nsh; *n_pblocks = nb; *n_seqs = nsq; *n_pieces = np; *dec_bytes = dec; *tmp_bytes = tmp;
    return rc_all;
}

int64_t afcodec_inflate_scratch_bytes(int64_t n_streams, int64_t n_pblocks, int64_t n_seqs, int64_t n_pieces, int64_t dec_bytes,
                                      int64_t tmp_bytes) {
    int64_t o[9];
    return afi_layout(n_streams, n_pblocks, n_seqs, n_pieces, dec_bytes, tmp_bytes, o);
}

/* The passes of the GPU decode (inflate_passes.h) run in order on this thread: the host reference of afhip_inflate_decode. */
int afcodec_inflate_emulate(const void* comp, int64_t comp_bytes, const void* streams, int64_t n_streams, const void* shuf_v,
                            int64_t n_shuf, int64_t n_pblocks, int64_t n_seqs, int64_t n_pieces, int64_t dec_bytes, int64_t tmp_bytes,
                            void* scratch, void* out, int32_t* errors, int32_t* rounds) {
    typedef struct { int64_t tmp_off, out_off; int32_t bsize, typesize; } shuf_rec;
    const shuf_rec* shuf = (const shuf_rec*)shuf_v;
    afi_ctx x;
    memset(&x, 0, sizeof x);
    x.comp = (const uint8_t*)comp; x.comp_bytes = comp_bytes;
    x.streams = (const afi_stream*)streams; x.n_streams = n_streams;
    x.n_blocks = n_pblocks; x.n_seqs = n_seqs; x.n_pieces = n_pieces; x.dec_bytes = dec_bytes; x.tmp_bytes = tmp_bytes;
    afi_bind(&x, (uint8_t*)scratch);
    x.out = (uint8_t*)out; x.errors = errors;
    memset(x.bad, 0, (size_t)(n_streams + 64) * 4);
    for (int64_t s = 0; s < n_streams; ++s) afi_pass_front(&x, s, NULL);
    for (int64_t b = 0; b < n_pblocks; ++b) afi_pass_fill(&x, b, 0, 1);
    const afz_ctx z = afi_jump_view(&x);
    const int R = afz_rounds_host(dec_bytes);
    int r = 0;
    for (; r < R && x.flags[r]; ++r) {
        int more = 0;
        for (int64_t p = 0; p < dec_bytes; ++p) more |= afz_jump(&z, p);
        x.flags[r + 1] = more;
    }
    for (int64_t b = 0; b < n_pblocks; ++b) afi_pass_gather(&x, b, 0, 1);
    for (int64_t g = 0; g < n_pieces; ++g) {
        uint32_t a;
        uint64_t b;
        afi_adler_share(&x, g, 0, 1, &a, &b);
        afi_adler_put(&x, g, a, b);
    }
    for (int64_t s = 0; s < n_streams; ++s) afi_pass_check(&x, s);
    for (int64_t i = 0; i < n_shuf; ++i) unshuffle_bytes(shuf[i].typesize, shuf[i].bsize, x.tmp + shuf[i].tmp_off, (uint8_t*)out + shuf[i].out_off);
    if (rounds) *rounds = r;
    return AFCODEC_OK;
}

/* ---- CCSDS / AEC (GRIB2 template 5.42): the passes of aec_passes.h in loops ---- */
#include "aec_passes.h"

/* One AEC stream of n_values samples of nbits bits -> out[n_values] (uint32): the host route of a CCSDS-packed GRIB2 field and the
 * host reference of afhip_grib_unpack_ccsds.  The stream is copied into a buffer of whole, aligned dwords first (the passes load those). */
int afcodec_aec_decode(const void* src, int64_t n, int64_t n_values, int nbits, int flags, int block_size, int rsi, uint32_t* out) {
    if ((!src && n) || n < 0 || n_values < 0 || (!out && n_values)) return fail(AFCODEC_E_FORMAT, "aec_decode: bad arguments");
    if (flags & ~(AEC_FLAGS_IGNORED | AEC_FLAG_PREPROCESS)) return fail(AFCODEC_E_UNSUPPORTED, "aec_decode: flags other than 2, 4 and 8 are not read");
    if (nbits < 0 || nbits > 32 || (block_size != 8 && block_size != 16 && block_size != 32 && block_size != 64) || rsi < 1 || rsi > AEC_RSI_MAX)
        return fail(AFCODEC_E_UNSUPPORTED, "aec_decode: bits per sample 0..32, block size 8 / 16 / 32 / 64, rsi 1..4096");
    if (n > ((int64_t)1 << 56)) return fail(AFCODEC_E_SIZE, "aec_decode: stream too long");
    const int64_t per = (int64_t)rsi * block_size, nr = (n_values + per - 1) / per, padded = (n + 3) / 4 * 4;
    uint8_t* stage = (uint8_t*)calloc((size_t)(padded ? padded : 4), 1);
    int64_t* table = (int64_t*)malloc((size_t)(nr ? nr : 1) * sizeof(int64_t));
    if (!stage || !table) {
        free(stage);
        free(table);
        return fail(AFCODEC_E_SIZE, "aec_decode: out of memory");
    }
    if (n) memcpy(stage, src, (size_t)n);
    aec_step st;
    memset(&st, 0, sizeof st);
    st.data_bytes = n; st.bitmap_off = -1; st.n_values = n_values;
    st.nbits = nbits; st.flags = flags; st.block_size = block_size; st.rsi = rsi;
    int32_t sound = 0, errors = 0;
    aec_ctx c;
    memset(&c, 0, sizeof c);
    c.stage = stage; c.stage_bytes = padded; c.steps = &st; c.n_steps = 1; c.n_points = n_values; c.max_rsis = nr;
    c.sound = &sound; c.rsi_bit = table; c.vals = out; c.errors = &errors;
    aec_pass_walk(&c, 0, 1);
    for (int64_t r = 0; r < nr; ++r) aec_pass_rsi(&c, 0, r);
    free(stage);
    free(table);
    return errors ? fail(AFCODEC_E_FORMAT, "aec_decode: the stream is damaged or ends before its last sample") : AFCODEC_OK;
}

/* ---- TIFF LZW: the text of lzw_passes.h on an OpenMP team ---- */
#include "lzw_passes.h"

/* The segments of a TIFF stack: range i of paths[i] is one LZW stream and must fill dsts[i] exactly.  Each thread keeps one span
 * table and one input buffer; the input is an exactly sized copy of the range, so the pass reads nothing else. */
int afcodec_lzw_decode_ranges(int64_t n, const char* const* paths, const int64_t* offsets, const int64_t* lengths,
                              void* const* dsts, const int64_t* dstsizes, int nthreads, int64_t* results) {
    if (n < 0 || (n && (!paths || !offsets || !lengths || !dsts || !dstsizes || !results))) return fail(AFCODEC_E_FORMAT, "lzw_decode_ranges: bad arguments");
    if (nthreads < 1) nthreads = 1;
    int bad = 0;
#pragma omp parallel num_threads(nthreads) reduction(+ : bad)
    {
        uint32_t* tab_pos = (uint32_t*)malloc(LZW_CODES * sizeof(uint32_t));
        uint16_t* tab_len = (uint16_t*)malloc(LZW_CODES * sizeof(uint16_t));
        fd_cache fc = {-1, -1};
#pragma omp for schedule(dynamic, 1)
        for (int64_t i = 0; i < n; ++i) {
            int64_t off = 0;
            const int64_t sz = lengths[i] < 0 ? AFCODEC_E_FORMAT : stat_range(paths[i], offsets, lengths, i, &off);
            int64_t r;
            if (sz < 0 || dstsizes[i] < 0 || dstsizes[i] > 0x7fffffff || (!dsts[i] && dstsizes[i]) || !tab_pos || !tab_len) {
                r = AFCODEC_E_FORMAT;
            } else {
                uint8_t* buf = (uint8_t*)malloc((size_t)(sz ? sz : 1));
                if (!buf || (sz && read_piece_of(&fc, i, paths[i], buf, sz, off, 0) != sz)) r = AFCODEC_E_FORMAT;
                else r = lzw_decode_segment(buf, sz, (uint8_t*)dsts[i], dstsizes[i], tab_pos, tab_len, 1) ? AFCODEC_E_CODEC : dstsizes[i];
                free(buf);
            }
            results[i] = r;
            if (r < 0) bad += 1;
        }
        if (fc.fd >= 0) close(fc.fd);
        free(tab_pos);
        free(tab_len);
    }
    return bad ? fail(AFCODEC_E_CODEC, "lzw_decode_ranges: one or more segments could not be read or are damaged (see results[])") : AFCODEC_OK;
}
