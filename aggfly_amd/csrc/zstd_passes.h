/* zstd_passes.h — Zstandard frame decode as independent passes over the blocks of a batch (RFC 8878).
 *
 * Written in the common subset of C and C++ so that ONE text serves two builds:
 *   - the HIP kernels of afhip_zstd_kernels.h (AFZ_FN = __device__), one GPU thread / wave per work item;
 *   - the host planner and the host emulator of libaggfly_codec.so (blosc1.c: afcodec_zstd_plan, afcodec_zstd_emulate),
 *     which runs the same passes in loops — the CPU tests check the GPU algorithm bit-exact against libzstd with it.
 *
 * The planner (host) walks frame, block, literals and sequences headers and emits one afz_block record per block; the
 * device then runs, each pass launch-ordered after the one before and no work item ever waiting for another:
 *   1 tables     Huffman decode table of every block that describes one (compressed literals), FSE decode tables of
 *                every block that describes one (FSE_Compressed mode), the predefined tables once (item n_blocks);
 *   2 literals   Huffman decode of 1 or 4 streams (an item per stream); raw / RLE literals and raw / RLE blocks are
 *                copied / filled (4 items share a block);
 *   3 sequences  FSE decode of a block's sequences into (literal length, match length, offset), the three repeat
 *                offsets tracked SYMBOLICALLY ("entry k of the block's incoming repeat offsets, minus d") so that no block
 *                needs the one before it; the block's decoded size and its outgoing repeat offsets (symbolic) too;
 *   4 frames     per frame: block output positions (prefix sum), the check against Frame_Content_Size, the blocks'
 *                incoming repeat offsets composed in order;
 *   5 fill       per block: src[p] of every output byte p = "literal i" (LIT | i) or "byte p - offset";
 *   6 jump       per byte, repeated: src[p] = src[src[p]] until every entry names a literal (pointer jumping: at most
 *                ceil(log2 frame bytes) rounds; a round that finds nothing left to do ends the rest at once);
 *   7 gather     per block: out[p] = lit[src[p]] at the frame's destination.
 * A damaged frame marks itself bad (and counts once in *errors); later passes skip it, and no pass reads outside the
 * batch's compressed bytes or writes outside the frame's destination and the batch's scratch.
 */
#ifndef AF_ZSTD_PASSES_H
#define AF_ZSTD_PASSES_H
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define AFZ_FN __device__ static inline
#define AFZ_CONST __device__ static const
#else
#define AFZ_FN static inline
#define AFZ_CONST static const
#endif

#define AFZ_BLOCK_MAX 131072          /* Block_Maximum_Size bound (128 KiB) */
#define AFZ_LIT (0x80000000u)         /* src[] tag: the entry names a literal */
#define AFZ_SLOT_BYTES 11264          /* per-block table slot (layout below) */
#define AFZ_SLOT_HUF 0                /* 2048 x u16: symbol | nbits << 8 */
#define AFZ_SLOT_HUFLOG 4096          /* int32: Huffman table log (max number of bits) */
#define AFZ_SLOT_LOGS 4100            /* 3 x int32: accuracy logs of the LL / OF / ML tables */
#define AFZ_SLOT_FSE 4224             /* 3 x 512 x u32 FSE entries: symbol | nbits << 8 | new_state << 16 */
#define AFZ_SLOT_WORK 10368           /* weights[256] | norm[64] int16 | next[64] u16 | weight table 64 x u32 */

/* one block of a batch (== afhip_zstd_block, include/aggfly_hip.h); offsets named "from src" are relative to src */
typedef struct afz_block {
    int64_t src;                      /* block content (after its 3-byte header) in the batch's compressed bytes */
    int64_t lit_off;                  /* its literals in the batch's literal buffer */
    int64_t seq_off;                  /* its first sequence in the batch's sequence buffer */
    int32_t frame;                    /* frame record index */
    int32_t btype;                    /* 0 raw, 1 RLE, 2 compressed */
    int32_t csize;                    /* content bytes */
    int32_t lit_type;                 /* 0 raw, 1 RLE, 2 compressed (with a Huffman description), 3 treeless */
    int32_t lit_size;                 /* regenerated literal bytes (raw / RLE block: Block_Size) */
    int32_t lit_src;                  /* from src: raw literal bytes / the RLE byte / the jump table or single Huffman stream */
    int32_t lit_csize;                /* Huffman streams with their jump table */
    int32_t n_streams;                /* 1 or 4 */
    int32_t huf_desc;                 /* from src: Huffman tree description (lit_type 2), else -1 */
    int32_t huf_block;                /* block whose Huffman table decodes these literals (itself or earlier), else -1 */
    int32_t nseq;                     /* number of sequences */
    int32_t seq_src;                  /* from src: the sequences bitstream (to csize) */
    int32_t mode[3];                  /* LL, OF, ML: 0 predefined, 1 RLE, 2 FSE (Repeat_Mode resolved by the planner) */
    int32_t tab_desc[3];              /* mode 2: from src of tab_block, the FSE table description; mode 1: the symbol */
    int32_t tab_block[3];             /* mode 2: block whose table is meant (itself or earlier) */
    int32_t pad;
} afz_block;

typedef struct afz_frame {            /* == afhip_zstd_frame */
    int64_t dst_off;                  /* decoded bytes go to out + dst_off */
    int64_t base;                     /* the frame's first byte in the batch's decoded space */
    int64_t size;                     /* Frame_Content_Size */
    int32_t first_block, n_blocks;
} afz_frame;

typedef struct afz_seq { uint32_t ll, ml; int32_t off; } afz_seq;

/* ---- specification data (RFC 8878 §3.1.1.3.2.1.1, §3.1.1.3.2.2) ---- */
AFZ_CONST uint32_t afz_ll_base[36] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40,
                                      48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
AFZ_CONST uint8_t afz_ll_bits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3,
                                     4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
AFZ_CONST uint32_t afz_ml_base[53] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26,
                                      27, 28, 29, 30, 31, 32, 33, 34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515,
                                      1027, 2051, 4099, 8195, 16387, 32771, 65539};
AFZ_CONST uint8_t afz_ml_bits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                     1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
AFZ_CONST int16_t afz_ll_default[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2,
                                        2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
AFZ_CONST int16_t afz_ml_default[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                        1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
AFZ_CONST int16_t afz_of_default[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
/* LL / OF / ML: largest symbol, largest accuracy log */
AFZ_CONST int afz_max_sym[3] = {35, 31, 52};
AFZ_CONST int afz_max_log[3] = {9, 8, 9};

AFZ_FN int afz_highbit32(uint32_t v) { /* v > 0 */
    int r = 0;
    while (v >>= 1) ++r;
    return r;
}

/* FSE table description (RFC 8878 §4.1.1) at p (avail bytes): norm[0..*nsym), *log; -> bytes used, or -1 */
AFZ_FN int afz_read_ncount(const uint8_t* p, int64_t avail, int16_t* norm, int max_sym, int max_log, int* nsym, int* log) {
    if (avail < 1) return -1;
    int64_t bit = 0;
#define AFZ_NC_GET(n_, out_)                                                                                   \
    do {                                                                                                       \
        uint32_t v_ = 0;                                                                                       \
        for (int i_ = 0; i_ < (n_); ++i_) {                                                                    \
            const int64_t b_ = bit + i_;                                                                       \
            if ((b_ >> 3) >= avail) return -1;                                                                 \
            v_ |= (uint32_t)((p[b_ >> 3] >> (b_ & 7)) & 1) << i_;                                              \
        }                                                                                                      \
        (out_) = v_;                                                                                           \
    } while (0)
    uint32_t lg;
    AFZ_NC_GET(4, lg);
    lg += 5;
    if ((int)lg > max_log) return -1;
    bit = 4;
    int remaining = (1 << lg) + 1, threshold = 1 << lg, nb = (int)lg + 1, s = 0, prev0 = 0;
    while (remaining > 1 && s <= max_sym) {
        if (prev0) {
            uint32_t r;
            for (;;) {
                AFZ_NC_GET(2, r);
                bit += 2;
                for (uint32_t k = 0; k < r; ++k) {
                    if (s > max_sym) return -1;
                    norm[s++] = 0;
                }
                if (r != 3) break;
            }
            if (s > max_sym) return -1;
        }
        const int mx = 2 * threshold - 1 - remaining;
        uint32_t v;
        int count;
        AFZ_NC_GET(nb, v);     /* nb bits, or nb - 1 when they give a small value */
        if ((int)(v & (uint32_t)(threshold - 1)) < mx) {
            count = (int)(v & (uint32_t)(threshold - 1));
            bit += nb - 1;
        } else {
            count = (int)(v & (uint32_t)(2 * threshold - 1));
            if (count >= threshold) count -= mx;
            bit += nb;
        }
        count -= 1;
        remaining -= count < 0 ? -count : count;
        norm[s++] = (int16_t)count;
        prev0 = count == 0;
        while (remaining < threshold && threshold > 1) { nb--; threshold >>= 1; }
    }
#undef AFZ_NC_GET
    if (remaining != 1 || s < 1) return -1;
    *nsym = s;
    *log = (int)lg;
    return (int)((bit + 7) >> 3);
}

/* FSE decode table (RFC 8878 §4.1.1, "from normalized distribution to decoding tables"); next: nsym u16 of work space.
 * -> 0, or -1 for a distribution that does not fill the table */
AFZ_FN int afz_build_fse(const int16_t* norm, int nsym, int lg, uint32_t* table, uint16_t* next) {
    const int size = 1 << lg;
    int high = size - 1;
    for (int s = 0; s < nsym; ++s) {
        if (norm[s] == -1) {
            if (high < 0) return -1;
            table[high--] = (uint32_t)s;
            next[s] = 1;
        } else {
            next[s] = (uint16_t)norm[s];
        }
    }
    const int step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
    int pos = 0;
    for (int s = 0; s < nsym; ++s)
        for (int i = 0; i < norm[s]; ++i) {
            if (high < 0) return -1;
            table[pos] = (uint32_t)s;
            do pos = (pos + step) & mask; while (pos > high);
        }
    if (pos != 0) return -1;
    for (int u = 0; u < size; ++u) {
        const uint32_t s = table[u] & 0xff;
        const uint32_t ns = next[s]++;
        if (ns == 0) return -1;
        const int nbits = lg - afz_highbit32(ns);
        const uint32_t st = (ns << nbits) - (uint32_t)size;
        table[u] = s | ((uint32_t)nbits << 8) | (st << 16);
    }
    return 0;
}

/* ---- backward bitstream (RFC 8878 §4.1): bits are consumed from the end; below the start they read as 0 ---- */
typedef struct afz_bits {
    const uint8_t* comp;
    int64_t comp_bytes, start, pos;   /* pos: bits left, counted from the stream's first bit */
    int64_t wlo;                      /* w holds the stream's bits [wlo, wlo + 56): refilled (two loads) when a read reaches below */
    uint64_t w;
} afz_bits;

AFZ_FN uint64_t afz_ld64(const uint8_t* comp, int64_t comp_bytes, int64_t a) {   /* a: multiple of 8 */
    if (a >= 0 && a + 8 <= comp_bytes) {
        uint64_t v;
#if defined(__HIPCC__)
        v = *(const uint64_t*)(comp + a);
#else
        memcpy(&v, comp + a, 8);
#endif
        return v;
    }
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) {
        const int64_t j = a + i;
        if (j >= 0 && j < comp_bytes) v |= (uint64_t)comp[j] << (8 * i);
    }
    return v;
}

/* n (<= 56) bits of the stream at bits [lo, lo + n), lo >= 0 */
AFZ_FN uint64_t afz_get(const afz_bits* b, int64_t lo, int n) {
    const int64_t q = b->start * 8 + lo;
    const int64_t w = (q >> 6) << 3;
    const int off = (int)(q & 63);
    uint64_t v = afz_ld64(b->comp, b->comp_bytes, w) >> off;
    if (off + n > 64) v |= afz_ld64(b->comp, b->comp_bytes, w + 8) << (64 - off);
    return n >= 64 ? v : v & ((1ull << n) - 1);
}

AFZ_FN int afz_bits_init(afz_bits* b, const uint8_t* comp, int64_t comp_bytes, int64_t start, int64_t size) {
    b->comp = comp; b->comp_bytes = comp_bytes; b->start = start; b->pos = -1;
    b->wlo = (int64_t)1 << 62; b->w = 0;
    if (size <= 0 || start < 0 || start + size > comp_bytes) return -1;
    const uint8_t last = comp[start + size - 1];
    if (!last) return -1;
    b->pos = (size - 1) * 8 + afz_highbit32(last);
    return 0;
}

/* n <= 32 bits below pos; pos only ever falls, so a window whose top is pos at its refill covers every later read above wlo */
AFZ_FN uint32_t afz_peek(afz_bits* b, int n) {
    const int64_t pos = b->pos, lo = pos - n;
    if (n == 0 || pos <= 0) return 0;
    if (lo < b->wlo) {
        b->wlo = pos > 56 ? pos - 56 : 0;
        b->w = afz_get(b, b->wlo, 56);
    }
    if (lo >= 0) return (uint32_t)((b->w >> (lo - b->wlo)) & ((1ull << n) - 1));
    return (uint32_t)((b->w & ((1ull << pos) - 1)) << (-lo));       /* (wlo == 0 here) */
}

AFZ_FN uint32_t afz_read(afz_bits* b, int n) {
    const uint32_t v = afz_peek(b, n);
    b->pos -= n;
    return v;
}

/* ---- the scratch of one batch ---- */
typedef struct afz_ctx {
    const uint8_t* comp; int64_t comp_bytes;
    const afz_frame* frames; int64_t n_frames;
    const afz_block* blocks; int64_t n_blocks;
    uint8_t* slots;                   /* (n_blocks + 1) table slots; the last holds the predefined tables */
    uint8_t* lit; int64_t lit_bytes;
    afz_seq* seqs; int64_t n_seqs;
    int32_t* dsize;                   /* per block: decoded bytes */
    int32_t* rep_out;                 /* per block: 3 outgoing repeat offsets (symbolic) */
    int32_t* rep_in;                  /* per block: 3 incoming repeat offsets (concrete) */
    int64_t* out_pos;                 /* per block: first byte in the batch's decoded space */
    int32_t* bad;                     /* per frame */
    uint32_t* src; int64_t dec_bytes; /* per decoded byte */
    int32_t* flags;                   /* pointer-jump rounds: flags[r] = 1 if round r has work */
    uint8_t* out;
    int32_t* errors;
} afz_ctx;

/* pointer-jump rounds that always suffice: ceil(log2(dec_bytes)) + 1 */
static inline int afz_rounds_host(int64_t dec_bytes) {
    int r = 1;
    while (((int64_t)1 << (r - 1)) < dec_bytes && r < 40) ++r;
    return r;
}

static inline int64_t afz_align(int64_t v) { return (v + 255) & ~(int64_t)255; }

/* byte layout of the scratch (offsets into it); -> total bytes */
static inline int64_t afz_layout(int64_t n_blocks, int64_t n_frames, int64_t lit_bytes, int64_t n_seqs, int64_t dec_bytes, int64_t* o) {
    int64_t at = 0;
    o[0] = at; at = afz_align(at + (n_blocks + 1) * (int64_t)AFZ_SLOT_BYTES);    /* slots */
    o[1] = at; at = afz_align(at + lit_bytes);                                     /* literals */
    o[2] = at; at = afz_align(at + n_seqs * (int64_t)sizeof(afz_seq));            /* sequences */
    o[3] = at; at = afz_align(at + n_blocks * 4);                                  /* dsize */
    o[4] = at; at = afz_align(at + n_blocks * 12);                                 /* rep_out */
    o[5] = at; at = afz_align(at + n_blocks * 12);                                 /* rep_in */
    o[6] = at; at = afz_align(at + n_blocks * 8);                                  /* out_pos */
    o[7] = at; at = afz_align(at + (n_frames + 64) * 4);                           /* bad flags | jump round flags (64) */
    o[8] = at; at = afz_align(at + dec_bytes * 4);                                 /* src */
    return at;
}

static inline void afz_bind(afz_ctx* c, uint8_t* scratch, int64_t n_blocks, int64_t n_frames, int64_t lit_bytes, int64_t n_seqs,
                            int64_t dec_bytes) {
    int64_t o[9];
    afz_layout(n_blocks, n_frames, lit_bytes, n_seqs, dec_bytes, o);
    c->slots = scratch + o[0];
    c->lit = scratch + o[1]; c->lit_bytes = lit_bytes;
    c->seqs = (afz_seq*)(void*)(scratch + o[2]); c->n_seqs = n_seqs;
    c->dsize = (int32_t*)(void*)(scratch + o[3]);
    c->rep_out = (int32_t*)(void*)(scratch + o[4]);
    c->rep_in = (int32_t*)(void*)(scratch + o[5]);
    c->out_pos = (int64_t*)(void*)(scratch + o[6]);
    c->bad = (int32_t*)(void*)(scratch + o[7]);
    c->flags = c->bad + n_frames;
    c->src = (uint32_t*)(void*)(scratch + o[8]); c->dec_bytes = dec_bytes;
}

AFZ_FN void afz_mark_bad(const afz_ctx* c, int32_t f) {
#if defined(__HIPCC__)
    if (atomicExch(&c->bad[f], 1) == 0) atomicAdd(c->errors, 1);
#else
    if (c->bad[f] == 0) { c->bad[f] = 1; *c->errors += 1; }
#endif
}

AFZ_FN int afz_is_bad(const afz_ctx* c, int32_t f) {
#if defined(__HIPCC__)
    return __hip_atomic_load(&c->bad[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
#else
    return c->bad[f] != 0;
#endif
}

/* The fill pass is the one pass that both asks for the flag and sets it from another work item of the same frame.  It sets 2 and asks
 * for 1, so that what a block of the pass does never depends on when a sibling block found its defect. */
AFZ_FN void afz_mark_bad_in_fill(const afz_ctx* c, int32_t f) {
#if defined(__HIPCC__)
    if (atomicExch(&c->bad[f], 2) == 0) atomicAdd(c->errors, 1);
#else
    if (c->bad[f] == 0) { c->bad[f] = 2; *c->errors += 1; }
#endif
}

AFZ_FN int afz_was_bad_before_fill(const afz_ctx* c, int32_t f) {
#if defined(__HIPCC__)
    return __hip_atomic_load(&c->bad[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1;
#else
    return c->bad[f] == 1;
#endif
}

/* ---- pass 1: tables of block b (b == n_blocks: the predefined FSE tables) ---- */
AFZ_FN int afz_huffman_table(const afz_ctx* c, const afz_block* k, uint8_t* slot) {
    uint8_t* w = slot + AFZ_SLOT_WORK;
    int16_t* norm = (int16_t*)(void*)(w + 256);
    uint16_t* next = (uint16_t*)(void*)(w + 384);
    uint32_t* wt = (uint32_t*)(void*)(w + 512);
    const int64_t d = k->src + k->huf_desc;
    const int64_t end = k->src + k->lit_src;             /* the description ends where the streams begin */
    if (d >= end || end > c->comp_bytes) return -1;
    const int h = c->comp[d];
    int nw = 0;
    if (h < 128) {                                        /* FSE-compressed weights, h bytes */
        if (d + 1 + h != end || h == 0) return -1;
        int nsym, lg;
        const int used = afz_read_ncount(c->comp + d + 1, h, norm, 15, 6, &nsym, &lg);
        if (used < 0 || used >= h) return -1;
        if (afz_build_fse(norm, nsym, lg, wt, next)) return -1;
        afz_bits br;
        if (afz_bits_init(&br, c->comp, c->comp_bytes, d + 1 + used, h - used)) return -1;
        uint32_t s1 = afz_read(&br, lg), s2 = afz_read(&br, lg);
        for (;;) {
            if (nw > 253) return -1;
            w[nw++] = (uint8_t)(wt[s1] & 0xff);
            s1 = (wt[s1] >> 16) + afz_read(&br, (int)((wt[s1] >> 8) & 0xff));
            if (br.pos < 0) { w[nw++] = (uint8_t)(wt[s2] & 0xff); break; }
            if (nw > 253) return -1;
            w[nw++] = (uint8_t)(wt[s2] & 0xff);
            s2 = (wt[s2] >> 16) + afz_read(&br, (int)((wt[s2] >> 8) & 0xff));
            if (br.pos < 0) { w[nw++] = (uint8_t)(wt[s1] & 0xff); break; }
        }
    } else {                                              /* direct: 4 bits a weight */
        nw = h - 127;
        if (d + 1 + (nw + 1) / 2 != end) return -1;
        for (int i = 0; i < nw; ++i) {
            const uint8_t byte = c->comp[d + 1 + i / 2];
            w[i] = (uint8_t)((i & 1) ? (byte & 15) : (byte >> 4));
        }
    }
    if (nw < 1 || nw > 255) return -1;
    uint32_t sum = 0;
    for (int i = 0; i < nw; ++i) {
        if (w[i] > 11) return -1;
        if (w[i]) sum += 1u << (w[i] - 1);
    }
    if (sum == 0) return -1;
    const int maxb = afz_highbit32(sum) + 1;
    if (maxb > 11) return -1;
    const uint32_t rest = (1u << maxb) - sum;
    if (rest & (rest - 1)) return -1;
    w[nw] = (uint8_t)(afz_highbit32(rest) + 1);
    const int nsym = nw + 1;
    uint16_t* tab = (uint16_t*)(void*)(slot + AFZ_SLOT_HUF);
    uint32_t pos = 0;
    for (int wv = 1; wv <= maxb; ++wv)
        for (int s = 0; s < nsym; ++s)
            if (w[s] == wv) {
                const uint32_t len = 1u << (wv - 1);
                const uint16_t e = (uint16_t)(s | ((maxb + 1 - wv) << 8));
                for (uint32_t i = 0; i < len; ++i) tab[pos + i] = e;
                pos += len;
            }
    if (pos != (1u << maxb)) return -1;
    *(int32_t*)(void*)(slot + AFZ_SLOT_HUFLOG) = maxb;
    return 0;
}

AFZ_FN void afz_pass_tables(const afz_ctx* c, int64_t b) {
    if (b > c->n_blocks) return;
    uint8_t* slot = c->slots + b * (int64_t)AFZ_SLOT_BYTES;
    uint8_t* w = slot + AFZ_SLOT_WORK;
    int16_t* norm = (int16_t*)(void*)(w + 256);
    uint16_t* next = (uint16_t*)(void*)(w + 384);
    int32_t* logs = (int32_t*)(void*)(slot + AFZ_SLOT_LOGS);
    if (b == c->n_blocks) {                               /* predefined distributions: accuracy 6 / 5 / 6 */
        for (int t = 0; t < 3; ++t) {
            const int16_t* src = t == 0 ? afz_ll_default : (t == 1 ? afz_of_default : afz_ml_default);
            const int n = t == 0 ? 36 : (t == 1 ? 29 : 53), lg = t == 1 ? 5 : 6;
            for (int s = 0; s < n; ++s) norm[s] = src[s];
            afz_build_fse(norm, n, lg, (uint32_t*)(void*)(slot + AFZ_SLOT_FSE + t * 2048), next);
            logs[t] = lg;
        }
        return;
    }
    const afz_block* k = &c->blocks[b];
    if (afz_is_bad(c, k->frame)) return;
    if (k->btype == 2 && k->lit_type == 2 && afz_huffman_table(c, k, slot)) { afz_mark_bad(c, k->frame); return; }
    for (int t = 0; t < 3; ++t) {
        if (k->btype != 2 || k->nseq == 0 || k->mode[t] != 2 || k->tab_block[t] != b) continue;
        const int64_t d = k->src + k->tab_desc[t];
        int nsym, lg;
        if (afz_read_ncount(c->comp + d, k->src + k->csize - d, norm, afz_max_sym[t], afz_max_log[t], &nsym, &lg) < 0 ||
            afz_build_fse(norm, nsym, lg, (uint32_t*)(void*)(slot + AFZ_SLOT_FSE + t * 2048), next)) {
            afz_mark_bad(c, k->frame);
            return;
        }
        logs[t] = lg;
    }
}

/* ---- pass 2: literals; item q (0..3) of block b; lds_tab: a copy of the block's Huffman table (or NULL) ---- */
AFZ_FN void afz_pass_literals(const afz_ctx* c, int64_t b, int q, const uint16_t* lds_tab) {
    if (b >= c->n_blocks) return;
    const afz_block* k = &c->blocks[b];
    if (afz_is_bad(c, k->frame)) return;
    uint8_t* dst = c->lit + k->lit_off;
    const int64_t n = k->lit_size;
    if (k->lit_type < 2 || k->btype < 2) {                /* raw or RLE: the 4 items share the copy */
        const int64_t a = n * q / 4, e = n * (q + 1) / 4;
        const uint8_t* s = c->comp + k->src + k->lit_src;
        if (k->lit_type == 1) { const uint8_t v = s[0]; for (int64_t i = a; i < e; ++i) dst[i] = v; }
        else for (int64_t i = a; i < e; ++i) dst[i] = s[i];
        return;
    }
    if (q >= k->n_streams) return;
    const uint8_t* slot = c->slots + (int64_t)k->huf_block * AFZ_SLOT_BYTES;
    const uint16_t* tab = lds_tab ? lds_tab : (const uint16_t*)(const void*)(slot + AFZ_SLOT_HUF);
    const int maxb = *(const int32_t*)(const void*)(slot + AFZ_SLOT_HUFLOG);
    int64_t s0 = k->src + k->lit_src, ssz = k->lit_csize, o0 = 0, on = n;
    if (k->n_streams == 4) {
        const uint8_t* j = c->comp + s0;
        const int64_t l1 = j[0] | (j[1] << 8), l2 = j[2] | (j[3] << 8), l3 = j[4] | (j[5] << 8);
        const int64_t l4 = ssz - 6 - l1 - l2 - l3;
        const int64_t seg = (n + 3) / 4;
        if (l4 < 1 || seg * 3 > n) { afz_mark_bad(c, k->frame); return; }
        const int64_t ls[4] = {l1, l2, l3, l4};
        s0 += 6;
        for (int i = 0; i < q; ++i) s0 += ls[i];
        ssz = ls[q];
        o0 = seg * q;
        on = q < 3 ? seg : n - 3 * seg;
    }
    afz_bits br;
    if (afz_bits_init(&br, c->comp, c->comp_bytes, s0, ssz)) { afz_mark_bad(c, k->frame); return; }
    for (int64_t i = 0; i < on; ++i) {
        const uint16_t e = tab[afz_peek(&br, maxb)];
        dst[o0 + i] = (uint8_t)(e & 0xff);
        br.pos -= e >> 8;
    }
    if (br.pos != 0) afz_mark_bad(c, k->frame);
}

/* ---- pass 3: sequences of block b ---- */
#define AFZ_SYM(k_, d_) (-(1 + (k_) + 3 * (d_)))

AFZ_FN void afz_pass_sequences(const afz_ctx* c, int64_t b) {
    if (b >= c->n_blocks) return;
    const afz_block* k = &c->blocks[b];
    int32_t* ro = c->rep_out + 3 * b;
    ro[0] = AFZ_SYM(0, 0); ro[1] = AFZ_SYM(1, 0); ro[2] = AFZ_SYM(2, 0);
    c->dsize[b] = k->lit_size;
    if (afz_is_bad(c, k->frame) || k->btype < 2 || k->nseq == 0) return;
    const uint32_t* tab[3];
    int lg[3];
    uint32_t rle[3];
    for (int t = 0; t < 3; ++t) {
        rle[t] = 0;
        if (k->mode[t] == 1) { tab[t] = 0; lg[t] = 0; rle[t] = (uint32_t)k->tab_desc[t]; continue; }
        const int64_t sb = k->mode[t] == 0 ? c->n_blocks : k->tab_block[t];
        const uint8_t* slot = c->slots + sb * (int64_t)AFZ_SLOT_BYTES;
        tab[t] = (const uint32_t*)(const void*)(slot + AFZ_SLOT_FSE + t * 2048);
        lg[t] = ((const int32_t*)(const void*)(slot + AFZ_SLOT_LOGS))[t];
    }
    afz_bits br;
    if (afz_bits_init(&br, c->comp, c->comp_bytes, k->src + k->seq_src, k->csize - k->seq_src)) { afz_mark_bad(c, k->frame); return; }
    uint32_t st[3];
    st[0] = afz_read(&br, lg[0]); st[1] = afz_read(&br, lg[1]); st[2] = afz_read(&br, lg[2]);
    int32_t r0 = ro[0], r1 = ro[1], r2 = ro[2];
    int64_t sum_ll = 0, sum_ml = 0;
    afz_seq* out = c->seqs + k->seq_off;
    for (int32_t i = 0; i < k->nseq; ++i) {
        const uint32_t llc = tab[0] ? (tab[0][st[0]] & 0xff) : rle[0];
        const uint32_t ofc = tab[1] ? (tab[1][st[1]] & 0xff) : rle[1];
        const uint32_t mlc = tab[2] ? (tab[2][st[2]] & 0xff) : rle[2];
        /* offset code 31 means an offset of 2^31 - 3 or more, past any frame the planner takes; as an int32 it would turn
         * negative and read as a symbolic entry below */
        if (llc > 35 || ofc > 30 || mlc > 52) { afz_mark_bad(c, k->frame); return; }
        const uint32_t ofv = (1u << ofc) + afz_read(&br, (int)ofc);
        const uint32_t ml = afz_ml_base[mlc] + afz_read(&br, afz_ml_bits[mlc]);
        const uint32_t ll = afz_ll_base[llc] + afz_read(&br, afz_ll_bits[llc]);
        int32_t off;
        if (ofv > 3) {
            off = (int32_t)(ofv - 3);
            r2 = r1; r1 = r0; r0 = off;
        } else {
            const int idx = (int)ofv - 1 + (ll == 0);
            if (idx == 0) off = r0;
            else if (idx == 1) { off = r1; r1 = r0; r0 = off; }
            else if (idx == 2) { off = r2; r2 = r1; r1 = r0; r0 = off; }
            else {                                        /* Repeated_Offset1 - 1: a new offset */
                if (r0 > 0) { off = r0 - 1; if (off == 0) { afz_mark_bad(c, k->frame); return; } }
                else off = r0 - 3;                        /* symbolic: one more subtracted */
                r2 = r1; r1 = r0; r0 = off;
            }
        }
        out[i].ll = ll; out[i].ml = ml; out[i].off = off;
        sum_ll += ll; sum_ml += ml;
        if (i + 1 < k->nseq)
            for (int u = 0; u < 3; ++u) {                 /* state updates: LL, then ML, then OF */
                const int t = u == 0 ? 0 : 3 - u;
                if (tab[t]) {
                    const uint32_t e = tab[t][st[t]];
                    st[t] = (e >> 16) + afz_read(&br, (int)((e >> 8) & 0xff));
                }
            }
    }
    if (br.pos != 0 || sum_ll > k->lit_size || k->lit_size + sum_ml > AFZ_BLOCK_MAX) { afz_mark_bad(c, k->frame); return; }
    c->dsize[b] = (int32_t)(k->lit_size + sum_ml);
    ro[0] = r0; ro[1] = r1; ro[2] = r2;
}

/* symbolic offset v against concrete incoming repeat offsets in[3] (-> <= 0 when invalid) */
AFZ_FN int64_t afz_resolve(int32_t v, const int32_t* in) {
    if (v > 0) return v;
    const int32_t m = -v - 1;
    return (int64_t)in[m % 3] - m / 3;
}

/* ---- pass 4: frame f ---- */
AFZ_FN void afz_pass_frame(const afz_ctx* c, int64_t f) {
    if (f >= c->n_frames) return;
    const afz_frame* fr = &c->frames[f];
    int32_t cur[3] = {1, 4, 8};
    int64_t pos = fr->base;
    for (int32_t i = 0; i < fr->n_blocks; ++i) {
        const int64_t b = fr->first_block + i;
        c->out_pos[b] = pos;
        pos += c->dsize[b];
        int32_t* ri = c->rep_in + 3 * b;
        ri[0] = cur[0]; ri[1] = cur[1]; ri[2] = cur[2];
        int64_t nx[3];
        for (int t = 0; t < 3; ++t) nx[t] = afz_resolve(c->rep_out[3 * b + t], ri);
        for (int t = 0; t < 3; ++t) cur[t] = nx[t] > 0 && nx[t] < 0x7fffffff ? (int32_t)nx[t] : 0x7fffffff;   /* (an invalid one fails where it is used) */
    }
    if (pos - fr->base != fr->size) afz_mark_bad(c, (int32_t)f);
}

/* src[] of the bytes [p0, p1) that nobody will fill, clipped to the batch: "a literal", where a pointer-jump round stops.  The
 * rounds visit every byte of the batch, those of a bad frame too; what they find there must not be what the scratch held before
 * the call (the count of rounds with work is an output, and stale entries would be chased). */
AFZ_FN void afz_stop_range(const afz_ctx* c, int64_t p0, int64_t p1, int l, int nl) {
    if (p0 < 0) p0 = 0;
    if (p1 > c->dec_bytes) p1 = c->dec_bytes;
    for (int64_t p = p0 + l; p < p1; p += nl) c->src[p] = AFZ_LIT;
}

/* ---- pass 5: src[] of block b, lane l of nl ---- */
AFZ_FN void afz_pass_fill(const afz_ctx* c, int64_t b, int l, int nl) {
    if (b >= c->n_blocks) return;
    const afz_block* k = &c->blocks[b];
    const afz_frame* fr = &c->frames[k->frame];
    if (afz_was_bad_before_fill(c, k->frame)) {        /* its block sizes may be unknown: this block's share of the frame's bytes */
        const int64_t i = b - fr->first_block, n = fr->n_blocks > 0 ? fr->n_blocks : 1;
        afz_stop_range(c, fr->base + fr->size / n * i, i == n - 1 ? fr->base + fr->size : fr->base + fr->size / n * (i + 1), l, nl);
        return;
    }
    int64_t pos = c->out_pos[b], lit = k->lit_off;
    const int32_t* ri = c->rep_in + 3 * b;
    int any = 0;
    if (k->btype == 2)
        for (int32_t i = 0; i < k->nseq; ++i) {
            const afz_seq s = c->seqs[k->seq_off + i];
            const int64_t off = afz_resolve(s.off, ri);
            if (off <= 0 || off > pos + s.ll - fr->base) {          /* (the same for every lane) */
                if (l == 0) afz_mark_bad_in_fill(c, k->frame);
                afz_stop_range(c, pos, c->out_pos[b] + c->dsize[b], l, nl);
                return;
            }
            for (int64_t j = l; j < s.ll; j += nl) c->src[pos + j] = AFZ_LIT | (uint32_t)(lit + j);
            pos += s.ll; lit += s.ll;
            for (int64_t j = l; j < s.ml; j += nl) c->src[pos + j] = (uint32_t)(pos + j - off);
            pos += s.ml;
            any = 1;
        }
    const int64_t rest = k->lit_off + k->lit_size - lit;
    for (int64_t j = l; j < rest; j += nl) c->src[pos + j] = AFZ_LIT | (uint32_t)(lit + j);
    if (any && l == 0) c->flags[0] = 1;
}

/* ---- pass 6: one pointer-jump round r over byte p ---- */
AFZ_FN int afz_jump(const afz_ctx* c, int64_t p) {   /* -> 1 if the entry still names a byte */
    const uint32_t v = c->src[p];
    if (v & AFZ_LIT) return 0;
    uint32_t w = (int64_t)v < c->dec_bytes ? c->src[v] : AFZ_LIT;    /* (garbage of a bad frame: stop) */
    c->src[p] = w;
    return (w & AFZ_LIT) == 0;
}

/* ---- pass 7: the bytes of block b, lane l of nl ---- */
AFZ_FN void afz_pass_gather(const afz_ctx* c, int64_t b, int l, int nl) {
    if (b >= c->n_blocks) return;
    const afz_block* k = &c->blocks[b];
    if (afz_is_bad(c, k->frame)) return;
    const afz_frame* fr = &c->frames[k->frame];
    const int64_t p0 = c->out_pos[b], n = c->dsize[b];
    uint8_t* o = c->out + fr->dst_off + (p0 - fr->base);
    for (int64_t j = l; j < n; j += nl) {
        const uint32_t v = c->src[p0 + j];
        const int64_t li = (int64_t)(v & ~AFZ_LIT);
        o[j] = (v & AFZ_LIT) && li < c->lit_bytes ? c->lit[li] : 0;
    }
}

#endif
