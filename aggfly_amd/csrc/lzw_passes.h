/* lzw_passes.h — TIFF LZW (TIFF 6.0 section 13, as libtiff writes and reads it) decoded with a span table.
 *
 * Written in the common subset of C and C++ so that ONE text serves two builds (as aec_passes.h and inflate_passes.h):
 *   - the HIP kernel of afhip_tiff_kernels.h (AFZ_FN = __device__): k_lzw_decode, one wave per segment, every lane running this text
 *     with the same values, the span table in LDS;
 *   - the host decoder of libaggfly_codec.so (blosc1.c: afcodec_lzw_decode_ranges), the host route of a TIFF stack and the reference
 *     the GPU tests and the sanitizer program hold the kernel to.
 *
 * The stream: codes most significant bit first, 9 to 12 bits wide.  Code 256 is Clear, 257 EndOfInformation, 258 the first free code.
 * Every code read after the first one since a Clear makes one table entry; the width grows when the NEXT FREE code reaches 511, 1023
 * and 2047 (libtiff's "early change": one code before the width is needed).  A stream ends at EndOfInformation or, as some writers leave
 * it out, when the segment's decoded size is reached.  The old bit-reversed form (first bytes 00 01) is refused by tiff.py, not here.
 *
 * The span table.  A table entry is never a chain of prefixes here: it is a span of the output already written.  The entry made while
 * code i is read is the string of code i - 1 followed by the first byte of the string of code i — and in the output the string of code
 * i - 1 IS directly followed by the first byte of the string of code i.  So the entry is out[start(i-1) : start(i-1) + len(i-1) + 1],
 * two numbers (pos, len), and a code is either a literal byte or a copy of an earlier span.  The one code a decoder can meet before its
 * entry is complete (code == next free code, "KwKwK") is the copy of out[start(i-1) : start(i-1) + len(i-1) + 1] to the position
 * start(i-1) + len(i-1): source and destination overlap by one byte, and that byte is the first of the source.  A span is at most 3,839
 * bytes (entry k since a Clear is at most k + 1 bytes long), so pos is a uint32 and len a uint16: 24 KiB for the 4,096 codes.
 *
 * SAFETY CONTRACT, held in the loop below:
 *   - the bit reader (lzw_refill) reads bytes of [src, src + n) only and returns zeros beyond them;
 *   - every iteration consumes one code of at least 9 bits, and a code that begins at or beyond the last staged bit makes the segment
 *     bad, so the trip count is bounded by the stream's bits;
 *   - a segment is bad — lzw_decode_segment returns 1 and the caller counts it once in *errors — when a code is above the next free one
 *     (L1), when the first code after a Clear is no literal (L2), when a span would reach beyond the segment's decoded size (L3), when
 *     the stream is cut short: a code begins beyond the staged bytes (L4), or EndOfInformation comes before the decoded size (L5);
 *   - nothing is written outside out[0, dsize) — a copy is checked against dsize before its first byte — and the table is indexed by
 *     codes below the next free one, itself at most 4,096.
 */
#ifndef AF_LZW_PASSES_H
#define AF_LZW_PASSES_H
#include "zstd_passes.h"

#define LZW_CLEAR 256
#define LZW_EOI 257
#define LZW_FIRST 258
#define LZW_CODES 4096
#define LZW_TABLE_BYTES (LZW_CODES * 6)

/* one segment (strip or tile) of a batch (== afhip_tiff_seg, include/aggfly_hip.h) */
typedef struct lzw_seg {
    int64_t src_off, src_bytes;       /* the compressed stream in the stage (afhip_lzw_decode) */
    int64_t dec_off, dec_bytes;       /* the decoded segment in the decoded buffer: rows * pitch * element size bytes */
    int32_t rows, pitch;              /* rows of the segment; samples from one row to the next (tile width, or image width for strips) */
    int32_t t, y, x;                  /* where its first sample goes: step of the batch, row and column of the image */
    int32_t bad;                      /* set by afhip_lzw_decode; afhip_tiff_place skips the segment */
} lzw_seg;

/* Is the decode half of a record sound?  Every test in a form that cannot overflow: the record is whatever the caller wrote. */
AFZ_FN int lzw_record_ok(const lzw_seg* r, int64_t stage_bytes, int64_t out_bytes) {
    if (r->src_off < 0 || r->src_bytes < 0 || r->src_off > stage_bytes || r->src_bytes > stage_bytes - r->src_off) return 0;
    if (r->dec_off < 0 || r->dec_bytes < 0 || r->dec_off > out_bytes || r->dec_bytes > out_bytes - r->dec_off) return 0;
    return r->dec_bytes <= 0x7fffffff;
}

#if defined(__HIPCC__)
#define LZW_LANE0 ((threadIdx.x & 63) == 0)
#define LZW_TAB volatile
/* One byte of the output this wave stored earlier, served by L2 (the wave's own L1 may hold the line as it was before the store). */
__device__ static inline uint8_t lzw_ld_out(const uint8_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
/* out[op : op + len] = out[from : from + len], len <= op - from + 1, by the 64 lanes: 64 bytes a step, the loads of a step before its
 * stores.  Every source byte lies below op — with the one byte of overlap (i == op - from) read as the span's first —, so no step reads
 * what a step of this copy stores; `acked`: the output below it has reached L2. */
__device__ static inline void lzw_copy(uint8_t* out, int64_t op, int64_t from, int len, int64_t* acked) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t dist = op - from;
    if (from + (len < dist ? len : dist) > *acked) {
        __builtin_amdgcn_s_waitcnt(0);
        *acked = op;
    }
    for (int i0 = 0; i0 < len; i0 += 64) {
        const int i = i0 + lane;
        if (i < len) out[op + i] = lzw_ld_out(out + from + (i < dist ? i : i - dist));
    }
}
#else
#define LZW_LANE0 1
#define LZW_TAB
static inline void lzw_copy(uint8_t* out, int64_t op, int64_t from, int len, int64_t* acked) {
    const int64_t dist = op - from;
    (void)acked;
    for (int i = 0; i < len; ++i) out[op + i] = out[from + (i < dist ? i : i - dist)];
}
#endif

/* the bit reader: `acc` holds the next `nb` bits of the stream at its top; byte `bi` is the next to come in */
typedef struct lzw_bits {
    const uint8_t* src;
    int64_t n, bi;
    uint64_t acc;
    int nb;
} lzw_bits;

AFZ_FN void lzw_refill(lzw_bits* b) {                      /* at least 57 bits afterwards; zeros beyond src[n - 1] */
    while (b->nb <= 56) {
        const uint64_t v = b->bi < b->n ? b->src[b->bi] : 0u;
        b->acc |= v << (56 - b->nb);
        b->nb += 8;
        b->bi += 1;
    }
}

/* One stream src[0, n) -> out[0, dsize), dsize <= 2^31 - 1.  tab_pos / tab_len: LZW_CODES entries each (LDS on the device).  -> 0, or 1:
 * the segment is bad (the contract above); what was written of it by then stays inside out[0, dsize).  write = 0: a dry walk — the codes
 * and the table never depend on the output's bytes, so the same answer comes without a store; the kernel walks dry first and leaves a
 * bad segment's output untouched.  On the device every lane of one wave calls it with the same arguments. */
AFZ_FN int lzw_decode_segment(const uint8_t* src, int64_t n, uint8_t* out, int64_t dsize, LZW_TAB uint32_t* tab_pos, LZW_TAB uint16_t* tab_len,
                              int write) {
    lzw_bits b;
    b.src = src; b.n = n; b.bi = 0; b.acc = 0; b.nb = 0;
    const int64_t nbits = n * 8;
    int64_t used = 0, op = 0, acked = 0, prev_pos = 0;
    int next = LZW_FIRST, width = 9, prev_len = 0;                       /* prev_len 0: the next code is the first since a Clear */
    while (op < dsize) {
        if (used >= nbits) return 1;                                     /* L4: the stream is cut short */
        if (b.nb < 12) lzw_refill(&b);
        const int code = (int)(b.acc >> (64 - width));
        b.acc <<= width;
        b.nb -= width;
        used += width;
        if (code == LZW_EOI) return 1;                                   /* L5: the end before the decoded size */
        if (code == LZW_CLEAR) {
            next = LZW_FIRST;
            width = 9;
            prev_len = 0;
            continue;
        }
        int64_t from = 0;
        int len = 1;
        if (prev_len == 0) {
            if (code > 255) return 1;                                    /* L2: no literal after a Clear */
        } else {
            if (code > next) return 1;                                   /* L1: a code above the next free one */
            if (code == next) {                                          /* KwKwK: the previous string and its own first byte */
                from = prev_pos;
                len = prev_len + 1;
            } else if (code > 255) {
                from = tab_pos[code];
                len = tab_len[code];
            }
            if (next < LZW_CODES) {                                      /* the entry this code completes */
                if (LZW_LANE0) {
                    tab_pos[next] = (uint32_t)prev_pos;
                    tab_len[next] = (uint16_t)(prev_len + 1);
                }
                next += 1;
                if (next + 1 >= (1 << width) && width < 12) width += 1;  /* early change: at 511, 1023, 2047 */
            }
        }
        if (len > dsize - op) return 1;                                  /* L3: a span beyond the decoded size */
        if (!write) {
        } else if (code < 256) {
            if (LZW_LANE0) out[op] = (uint8_t)code;
        } else {
            lzw_copy(out, op, from, len, &acked);
        }
        prev_pos = op;
        prev_len = len;
        op += len;
    }
    return 0;
}

#endif
