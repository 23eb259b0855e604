/* inflate_passes.h — zlib streams (RFC 1950 around RFC 1951 deflate) decoded as independent passes over the streams of a batch.
 *
 * Written in the common subset of C and C++ so that ONE text serves two builds (as zstd_passes.h, whose LZ77 back end it shares):
 *   - the HIP kernels of afhip_inflate_kernels.h (AFZ_FN = __device__);
 *   - the host planner and the host emulator of libaggfly_codec.so (blosc1.c: afcodec_inflate_plan, afcodec_inflate_emulate),
 *     which runs the same passes in loops — the CPU tests check the GPU algorithm bit-exact against zlib with it.
 *
 * Taken: chunks that are one zlib stream — stored, fixed and dynamic blocks, any number of them, any window size — optionally
 * followed by a whole-chunk byte unshuffle (HDF5 / netCDF-4 [deflate] and [shuffle, deflate], Zarr v2 "zlib").  NOT taken, left
 * to the host route: gzip members (their CRC-32), streams with a preset dictionary (FDICT), non-native byte order, chunks whose
 * filter mask skips a filter, chunks of 1 GiB and more, deflate inside Blosc.
 *
 * The planner (host) reads only the two zlib header bytes of a chunk and emits one afi_stream record per chunk; block boundaries
 * in deflate are only found by decoding, so the work item of the front end is a stream.  The device then runs, each pass
 * launch-ordered after the one before and no work item ever waiting for another:
 *   1 front     per stream: walks the blocks, builds the literal/length and distance decode tables of each dynamic block and turns
 *               the bit stream into literals and (literal length, match length, distance) records (afz_seq), cut into pseudo-blocks
 *               of <= 128 KiB of output; the stream's Adler-32 trailer is read here;
 *   2 fill      per pseudo-block: src[p] of every output byte p = "literal i" (AFZ_LIT | i) or "byte p - distance";
 *   3 jump      per byte, repeated: src[p] = src[src[p]] until every entry names a literal (zstd_passes.h: afz_jump);
 *   4 gather    per pseudo-block: the bytes, at the stream's destination (the output, or the shuffle scratch);
 *   5 adler     per piece of <= 64 KiB of decoded bytes: partial (a, b) sums;
 *   6 check     per stream: the partial sums combined in order and compared with the trailer;
 *   7 unshuffle per shuffled chunk (afhip_lz4_kernels.h: k_unshuffle_blocks; host: unshuffle_bytes).
 *
 * SAFETY CONTRACT, held in every loop below:
 *   - every iteration consumes at least one input bit or produces at least one output byte, so trip counts are bounded by
 *     8 * csize + dsize (a read past the stream's last bit ends the stream before the next iteration);
 *   - no pass reads outside the stream's compressed bytes (the bit reader returns zeros beyond them), none writes outside the
 *     stream's destination and the batch's scratch (every literal and every match is checked against dsize BEFORE it is recorded);
 *   - a stream is marked bad, and counted once in *errors, when it decodes to another size than planned, names a distance before
 *     its own start, uses literal/length symbols 286 / 287 or distance codes 30 / 31, has a stored block with LEN != ~NLEN, a
 *     reserved block type, an over-subscribed code (or an incomplete one where zlib refuses it), no end-of-block code, a code
 *     length repeat without a predecessor or past the announced counts, runs out of input, or fails its Adler-32;
 *   - later passes skip a bad stream.
 */
#ifndef AF_INFLATE_PASSES_H
#define AF_INFLATE_PASSES_H
#include "zstd_passes.h"

#define AFI_PIECE 65536                          /* decoded bytes per Adler-32 piece */
#define AFI_PBLOCK_MIN (AFZ_BLOCK_MAX - 257)     /* a pseudo-block that is not a stream's last holds at least this many bytes */
#define AFI_FAST 10                              /* bits of the one-lookup decode tables; longer codes take the canonical walk */
#define AFI_SLOT_BYTES 5376                      /* per-stream table slot (layout below) */
#define AFI_SLOT_LFAST 0                         /* 1024 x u16: symbol | code length << 9; 0 = longer than AFI_FAST bits or unassigned */
#define AFI_SLOT_DFAST 2048                      /* 1024 x u16, distance code */
#define AFI_SLOT_LCNT 4096                       /* 16 x u16: codes per length (literal/length) */
#define AFI_SLOT_DCNT 4128                       /* 16 x u16 (distance) */
#define AFI_SLOT_LSYM 4160                       /* 288 x u16: symbols in canonical order */
#define AFI_SLOT_DSYM 4736                       /* 32 x u16 */
#define AFI_SLOT_LENS 4800                       /* 320 x u8: code lengths of the block being described */
#define AFI_SLOT_CFAST 5120                      /* 128 x u16: the code length code (<= 7 bits) */

/* one zlib stream of a batch (== afhip_inflate_stream, include/aggfly_hip.h) */
typedef struct afi_stream {
    int64_t src;                      /* the chunk (zlib header included) in the batch's compressed bytes */
    int64_t dst_off;                  /* decoded bytes go to (to_out ? out : shuffle scratch) + dst_off */
    int64_t base;                     /* the stream's first byte in the batch's decoded space (and its literals' place) */
    int64_t seq_off;                  /* its first record in the batch's sequence buffer (dsize / 3 + 1 of them) */
    int32_t csize;                    /* chunk bytes: 2 header bytes, deflate blocks, 4 bytes of Adler-32 (anything after is ignored) */
    int32_t dsize;                    /* planned decoded bytes */
    int32_t to_out;
    int32_t first_block, n_blocks;    /* its pseudo-block slots: dsize / AFI_PBLOCK_MIN + 1 */
    int32_t first_piece;              /* its Adler-32 pieces: ceil(dsize / AFI_PIECE) */
} afi_stream;

typedef struct afi_pblock {           /* written by the front end */
    int64_t out_pos;                  /* first byte in the batch's decoded space */
    int64_t lit_off, seq_off;
    int32_t stream, nseq, lit_size, dsize;
} afi_pblock;

/* ---- specification data (RFC 1951 §3.2.5, §3.2.7) ---- */
AFZ_CONST uint16_t afi_len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
AFZ_CONST uint8_t afi_len_bits[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
AFZ_CONST uint16_t afi_dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                                        4097, 6145, 8193, 12289, 16385, 24577};
AFZ_CONST uint8_t afi_dist_bits[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
AFZ_CONST uint8_t afi_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

/* ---- forward bit reader over p[0, n): LSB first; bits beyond the end read as 0 (the caller compares pos with its bound) ---- */
typedef struct afi_bits {
    const uint8_t* p;
    int64_t n, pos, wpos;             /* w holds bits [wpos, wpos + 64), wpos a multiple of 8 */
    uint64_t w;
} afi_bits;

AFZ_FN uint64_t afi_ld64(const uint8_t* p, int64_t n, int64_t a) {
    uint64_t v = 0;
    if (a >= 0 && a + 8 <= n) {
        __builtin_memcpy(&v, p + a, 8);
        return v;
    }
    for (int i = 0; i < 8; ++i) {
        const int64_t j = a + i;
        if (j >= 0 && j < n) v |= (uint64_t)p[j] << (8 * i);
    }
    return v;
}

AFZ_FN uint32_t afi_peek(afi_bits* b, int n) {       /* n <= 32 */
    if (n == 0) return 0;
    if (b->pos + n > b->wpos + 64) {
        b->wpos = b->pos & ~(int64_t)7;
        b->w = afi_ld64(b->p, b->n, b->wpos >> 3);
    }
    return (uint32_t)((b->w >> (b->pos - b->wpos)) & ((1ull << n) - 1));
}

AFZ_FN uint32_t afi_take(afi_bits* b, int n) {
    const uint32_t v = afi_peek(b, n);
    b->pos += n;
    return v;
}

/* Canonical Huffman code of lens[0, n) (RFC 1951 §3.2.2): fast[1 << fb], cnt[16], sym[] (symbols by length, then value).
 * -> 0 complete, 1 incomplete (the caller decides, as zlib does), -1 over-subscribed */
AFZ_FN int afi_build(const uint8_t* lens, int n, int fb, uint16_t* fast, uint16_t* cnt, uint16_t* sym) {
    uint16_t offs[16], next[16];
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int i = 0; i < n; ++i) cnt[lens[i] & 15]++;
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - cnt[l];
        if (left < 0) return -1;
    }
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
    uint32_t code = 0;
    next[0] = 0;
    for (int l = 1; l < 16; ++l) {
        code = (code + (l > 1 ? cnt[l - 1] : 0)) << 1;
        next[l] = (uint16_t)code;
    }
    for (int i = 0; i < (1 << fb); ++i) fast[i] = 0;
    for (int i = 0; i < n; ++i) {
        const int l = lens[i] & 15;
        if (!l) continue;
        sym[offs[l]++] = (uint16_t)i;
        const uint32_t cd = next[l]++;
        if (l > fb) continue;
        uint32_t r = 0;
        for (int k = 0; k < l; ++k) r |= ((cd >> k) & 1u) << (l - 1 - k);       /* the stream carries codes most significant bit first */
        for (uint32_t k = r; k < (1u << fb); k += 1u << l) fast[k] = (uint16_t)(i | (l << 9));
    }
    return left > 0;
}

/* one symbol of the code (fast, cnt, sym) at the reader's position -> the symbol, or -1 for bits that are no code */
AFZ_FN int afi_symbol(afi_bits* b, int fb, const uint16_t* fast, const uint16_t* cnt, const uint16_t* sym) {
    uint32_t v = afi_peek(b, 15);
    const uint16_t e = fast[v & ((1u << fb) - 1)];
    if (e) {
        b->pos += e >> 9;
        return e & 511;
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        code |= (int)(v & 1);
        v >>= 1;
        const int k = cnt[l];
        if (code - k < first) {
            b->pos += l;
            return sym[index + (code - first)];
        }
        index += k;
        first = (first + k) << 1;
        code <<= 1;
    }
    return -1;
}

/* ---- the scratch of one batch ---- */
typedef struct afi_ctx {
    const uint8_t* comp; int64_t comp_bytes;
    const afi_stream* streams; int64_t n_streams;
    int64_t n_blocks, n_seqs, n_pieces, dec_bytes, tmp_bytes;
    uint8_t* slots;                   /* n_streams table slots */
    uint8_t* lit;                     /* dec_bytes: stream s's literals from streams[s].base on */
    afz_seq* seqs;
    afi_pblock* pblocks;
    uint32_t* adl;                    /* per piece: a, b (both mod 65521) */
    uint32_t* want;                   /* per stream: the Adler-32 of its trailer */
    int32_t* bad;                     /* per stream */
    int32_t* flags;                   /* pointer-jump rounds (64) */
    uint32_t* src;                    /* per decoded byte */
    uint8_t* tmp;                     /* shuffle scratch */
    uint8_t* out;
    int32_t* errors;
} afi_ctx;

/* byte layout of the scratch (offsets into it); -> total bytes */
static inline int64_t afi_layout(int64_t n_streams, int64_t n_blocks, int64_t n_seqs, int64_t n_pieces, int64_t dec_bytes, int64_t tmp_bytes,
                                 int64_t* o) {
    int64_t at = 0;
    o[0] = at; at = afz_align(at + n_streams * (int64_t)AFI_SLOT_BYTES);           /* slots */
    o[1] = at; at = afz_align(at + dec_bytes);                                      /* literals */
    o[2] = at; at = afz_align(at + n_seqs * (int64_t)sizeof(afz_seq));             /* sequences */
    o[3] = at; at = afz_align(at + n_blocks * (int64_t)sizeof(afi_pblock));        /* pseudo-blocks */
    o[4] = at; at = afz_align(at + n_pieces * 8);                                   /* Adler-32 partial sums */
    o[5] = at; at = afz_align(at + n_streams * 4);                                  /* trailers */
    o[6] = at; at = afz_align(at + (n_streams + 64) * 4);                           /* bad flags | jump round flags (64) */
    o[7] = at; at = afz_align(at + dec_bytes * 4);                                  /* src */
    o[8] = at; at = afz_align(at + tmp_bytes);                                      /* shuffle scratch */
    return at;
}

static inline void afi_bind(afi_ctx* c, uint8_t* scratch) {
    int64_t o[9];
    afi_layout(c->n_streams, c->n_blocks, c->n_seqs, c->n_pieces, c->dec_bytes, c->tmp_bytes, o);
    c->slots = scratch + o[0];
    c->lit = scratch + o[1];
    c->seqs = (afz_seq*)(void*)(scratch + o[2]);
    c->pblocks = (afi_pblock*)(void*)(scratch + o[3]);
    c->adl = (uint32_t*)(void*)(scratch + o[4]);
    c->want = (uint32_t*)(void*)(scratch + o[5]);
    c->bad = (int32_t*)(void*)(scratch + o[6]);
    c->flags = c->bad + c->n_streams;
    c->src = (uint32_t*)(void*)(scratch + o[7]);
    c->tmp = scratch + o[8];
}

/* the part of the context that the shared pointer-jump pass reads (afz_jump; k_zstd_jump) */
static inline afz_ctx afi_jump_view(const afi_ctx* c) {
    afz_ctx z;
    memset(&z, 0, sizeof z);
    z.src = c->src; z.dec_bytes = c->dec_bytes; z.flags = c->flags;
    return z;
}

AFZ_FN void afi_mark_bad(const afi_ctx* c, int64_t s) {
#if defined(__HIPCC__)
    if (atomicExch(&c->bad[s], 1) == 0) atomicAdd(c->errors, 1);
#else
    if (c->bad[s] == 0) { c->bad[s] = 1; *c->errors += 1; }
#endif
}

AFZ_FN int afi_is_bad(const afi_ctx* c, int64_t s) {
#if defined(__HIPCC__)
    return __hip_atomic_load(&c->bad[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
#else
    return c->bad[s] != 0;
#endif
}

/* afz_mark_bad_in_fill / afz_was_bad_before_fill of zstd_passes.h for this context: the fill pass sets 2 and asks for 1. */
AFZ_FN void afi_mark_bad_in_fill(const afi_ctx* c, int64_t s) {
#if defined(__HIPCC__)
    if (atomicExch(&c->bad[s], 2) == 0) atomicAdd(c->errors, 1);
#else
    if (c->bad[s] == 0) { c->bad[s] = 2; *c->errors += 1; }
#endif
}

AFZ_FN int afi_was_bad_before_fill(const afi_ctx* c, int64_t s) {
#if defined(__HIPCC__)
    return __hip_atomic_load(&c->bad[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1;
#else
    return c->bad[s] == 1;
#endif
}

/* ---- pass 1: the front end of stream s; slot: its table slot (NULL: the one in the scratch) ---- */
typedef struct afi_emit {
    uint8_t* lit; afz_seq* seq; afi_pblock* pb;
    int64_t base, seq_off, dsize, outn, nlit, nseq, blk_lit0, blk_seq0;
    int32_t nb, cap_b, pend, cur;
} afi_emit;

AFZ_FN void afi_open(afi_emit* e) {
    afi_pblock* k = &e->pb[e->nb];
    k->out_pos = e->base + e->outn; k->lit_off = e->base + e->nlit; k->seq_off = e->seq_off + e->nseq;
    e->blk_lit0 = e->nlit; e->blk_seq0 = e->nseq; e->pend = 0; e->cur = 0;
}

/* the pending literals stay with the block that closes (its "rest"); -> -1 when the slots are used up (they cannot be: every
 * closed block but the last holds >= AFI_PBLOCK_MIN bytes) */
AFZ_FN int afi_close(afi_emit* e, int last) {
    afi_pblock* k = &e->pb[e->nb];
    k->nseq = (int32_t)(e->nseq - e->blk_seq0); k->lit_size = (int32_t)(e->nlit - e->blk_lit0); k->dsize = e->cur;
    e->nb++;
    if (last) return 0;
    if (e->nb >= e->cap_b) return -1;
    afi_open(e);
    return 0;
}

AFZ_FN int afi_literal(afi_emit* e, uint8_t v) {
    if (e->outn >= e->dsize) return -1;
    e->lit[e->nlit++] = v;
    e->pend++; e->cur++; e->outn++;
    return e->cur == AFZ_BLOCK_MAX ? afi_close(e, 0) : 0;
}

AFZ_FN int afi_match(afi_emit* e, int32_t len, int32_t dist) {
    if (dist > e->outn || e->outn + len > e->dsize) return -1;
    if (e->cur + len > AFZ_BLOCK_MAX && afi_close(e, 0)) return -1;
    afz_seq* q = &e->seq[e->nseq++];               /* (a match is >= 3 bytes: at most dsize / 3 of them) */
    q->ll = (uint32_t)e->pend; q->ml = (uint32_t)len; q->off = dist;
    e->pend = 0; e->cur += len; e->outn += len;
    return e->cur == AFZ_BLOCK_MAX ? afi_close(e, 0) : 0;      /* (as a literal that ends on the limit: literals after it open the next block) */
}

AFZ_FN int afi_front(const afi_ctx* c, const afi_stream* st, afi_emit* e, uint8_t* slot, uint32_t* want) {
    uint16_t* lfast = (uint16_t*)(void*)(slot + AFI_SLOT_LFAST);
    uint16_t* dfast = (uint16_t*)(void*)(slot + AFI_SLOT_DFAST);
    uint16_t* lcnt = (uint16_t*)(void*)(slot + AFI_SLOT_LCNT);
    uint16_t* dcnt = (uint16_t*)(void*)(slot + AFI_SLOT_DCNT);
    uint16_t* lsym = (uint16_t*)(void*)(slot + AFI_SLOT_LSYM);
    uint16_t* dsym = (uint16_t*)(void*)(slot + AFI_SLOT_DSYM);
    uint16_t* cfast = (uint16_t*)(void*)(slot + AFI_SLOT_CFAST);
    uint8_t* lens = slot + AFI_SLOT_LENS;
    if (st->csize < 6 || st->src < 0 || st->src + st->csize > c->comp_bytes) return -1;
    afi_bits br;
    br.p = c->comp + st->src + 2; br.n = (int64_t)st->csize - 2; br.pos = 0; br.wpos = -64; br.w = 0;
    const int64_t nbits = 8 * ((int64_t)st->csize - 6);       /* the deflate blocks end before the 4 bytes of the trailer */
    int last, tables = 0;                                     /* tables: 1 = the fixed code is in the slot */
    do {
        const uint32_t h = afi_take(&br, 3);
        if (br.pos > nbits) return -1;
        last = (int)(h & 1);
        const int type = (int)(h >> 1);
        if (type == 3) return -1;
        if (type == 0) {
            br.pos = (br.pos + 7) & ~(int64_t)7;
            const uint32_t v = afi_take(&br, 32);
            const int64_t len = v & 0xffff;
            if (br.pos > nbits || len != (int64_t)((~v >> 16) & 0xffff) || br.pos + 8 * len > nbits) return -1;
            const uint8_t* q = br.p + (br.pos >> 3);
            for (int64_t i = 0; i < len; ++i)
                if (afi_literal(e, q[i])) return -1;
            br.pos += 8 * len;
            continue;
        }
        int nl, nd;
        if (type == 1) {
            nl = 288; nd = 32;
            if (tables != 1) {
                for (int i = 0; i < 288; ++i) lens[i] = (uint8_t)(i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : 8)));
                for (int i = 0; i < 32; ++i) lens[288 + i] = 5;
                afi_build(lens, 288, AFI_FAST, lfast, lcnt, lsym);
                afi_build(lens + 288, 32, AFI_FAST, dfast, dcnt, dsym);
                tables = 1;
            }
        } else {
            const uint32_t v = afi_take(&br, 14);
            nl = (int)(v & 31) + 257; nd = (int)((v >> 5) & 31) + 1;
            const int nc = (int)(v >> 10) + 4;
            if (nl > 286 || nd > 30) return -1;
            uint8_t cl[19];
            for (int i = 0; i < 19; ++i) cl[i] = 0;
            for (int i = 0; i < nc; ++i) cl[afi_cl_order[i]] = (uint8_t)afi_take(&br, 3);
            if (br.pos > nbits) return -1;
            tables = 2;
            if (afi_build(cl, 19, 7, cfast, dcnt, dsym)) return -1;      /* zlib refuses an incomplete code length code */
            int idx = 0;
            while (idx < nl + nd) {
                const uint16_t en = cfast[afi_peek(&br, 7)];
                if (!en) return -1;
                br.pos += en >> 9;
                const int sy = en & 511;
                if (sy < 16) lens[idx++] = (uint8_t)sy;
                else {
                    uint8_t prev = 0;
                    int rep;
                    if (sy == 16) {
                        if (!idx) return -1;
                        prev = lens[idx - 1];
                        rep = 3 + (int)afi_take(&br, 2);
                    } else if (sy == 17) rep = 3 + (int)afi_take(&br, 3);
                    else rep = 11 + (int)afi_take(&br, 7);
                    if (idx + rep > nl + nd) return -1;
                    while (rep--) lens[idx++] = prev;
                }
                if (br.pos > nbits) return -1;
            }
            if (lens[256] == 0) return -1;                             /* no end-of-block code */
            /* an incomplete code passes only as zlib lets it: a single code of one bit, or (distances) no code at all */
            int r = afi_build(lens, nl, AFI_FAST, lfast, lcnt, lsym);
            if (r < 0 || (r > 0 && !(lcnt[1] == 1 && lcnt[0] == nl - 1))) return -1;
            r = afi_build(lens + nl, nd, AFI_FAST, dfast, dcnt, dsym);
            if (r < 0 || (r > 0 && !(dcnt[0] == nd || (dcnt[1] == 1 && dcnt[0] == nd - 1)))) return -1;
        }
        for (;;) {
            int sy = afi_symbol(&br, AFI_FAST, lfast, lcnt, lsym);
            if (sy < 0 || br.pos > nbits) return -1;
            if (sy < 256) {
                if (afi_literal(e, (uint8_t)sy)) return -1;
                continue;
            }
            if (sy == 256) break;
            if (sy > 285) return -1;
            sy -= 257;
            const int32_t len = (int32_t)afi_len_base[sy] + (int32_t)afi_take(&br, afi_len_bits[sy]);
            const int ds = afi_symbol(&br, AFI_FAST, dfast, dcnt, dsym);
            if (ds < 0 || ds > 29) return -1;
            const int32_t dist = (int32_t)afi_dist_base[ds] + (int32_t)afi_take(&br, afi_dist_bits[ds]);
            if (br.pos > nbits || afi_match(e, len, dist)) return -1;
        }
    } while (!last);
    if (afi_close(e, 1) || e->outn != e->dsize) return -1;
    const uint8_t* t = br.p + ((br.pos + 7) >> 3);                     /* (<= csize - 6 from the stream's start: the trailer is inside) */
    *want = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | (uint32_t)t[3];
    return 0;
}

AFZ_FN void afi_pass_front(const afi_ctx* c, int64_t s, uint8_t* slot) {
    if (s >= c->n_streams) return;
    const afi_stream* st = &c->streams[s];
    afi_emit e;
    e.lit = c->lit + st->base; e.seq = c->seqs + st->seq_off; e.pb = c->pblocks + st->first_block;
    e.base = st->base; e.seq_off = st->seq_off; e.dsize = st->dsize; e.outn = 0; e.nlit = 0; e.nseq = 0;
    e.nb = 0; e.cap_b = st->n_blocks;
    for (int32_t i = 0; i < st->n_blocks; ++i) {                       /* slots the stream leaves unused stay empty */
        afi_pblock* k = &e.pb[i];
        k->out_pos = st->base; k->lit_off = st->base; k->seq_off = st->seq_off;
        k->stream = (int32_t)s; k->nseq = 0; k->lit_size = 0; k->dsize = 0;
    }
    afi_open(&e);
    uint32_t want = 0;
    if (afi_front(c, st, &e, slot ? slot : c->slots + s * (int64_t)AFI_SLOT_BYTES, &want)) afi_mark_bad(c, s);
    c->want[s] = want;
}

/* afz_stop_range of zstd_passes.h for this context: src[] of the bytes [p0, p1) that nobody will fill = "a literal". */
AFZ_FN void afi_stop_range(const afi_ctx* c, int64_t p0, int64_t p1, int l, int nl) {
    if (p0 < 0) p0 = 0;
    if (p1 > c->dec_bytes) p1 = c->dec_bytes;
    for (int64_t p = p0 + l; p < p1; p += nl) c->src[p] = AFZ_LIT;
}

/* ---- pass 2: src[] of pseudo-block b, lane l of nl ---- */
AFZ_FN void afi_pass_fill(const afi_ctx* c, int64_t b, int l, int nl) {
    if (b >= c->n_blocks) return;
    const afi_pblock* k = &c->pblocks[b];
    const afi_stream* st = &c->streams[k->stream];
    if (afi_was_bad_before_fill(c, k->stream)) {       /* the front end stopped somewhere: this slot's share of the stream's bytes */
        const int64_t i = b - st->first_block, n = st->n_blocks > 0 ? st->n_blocks : 1;
        afi_stop_range(c, st->base + st->dsize / n * i, i == n - 1 ? st->base + st->dsize : st->base + st->dsize / n * (i + 1), l, nl);
        return;
    }
    int64_t pos = k->out_pos, lit = k->lit_off;
    for (int32_t i = 0; i < k->nseq; ++i) {
        const afz_seq s = c->seqs[k->seq_off + i];
        if (s.off <= 0 || s.off > pos + s.ll - st->base) {              /* (the same for every lane) */
            if (l == 0) afi_mark_bad_in_fill(c, k->stream);
            afi_stop_range(c, pos, k->out_pos + k->dsize, l, nl);
            return;
        }
        for (int64_t j = l; j < s.ll; j += nl) c->src[pos + j] = AFZ_LIT | (uint32_t)(lit + j);
        pos += s.ll; lit += s.ll;
        for (int64_t j = l; j < s.ml; j += nl) c->src[pos + j] = (uint32_t)(pos + j - s.off);
        pos += s.ml;
    }
    const int64_t rest = k->lit_off + k->lit_size - lit;
    for (int64_t j = l; j < rest; j += nl) c->src[pos + j] = AFZ_LIT | (uint32_t)(lit + j);
    if (k->nseq && l == 0) c->flags[0] = 1;
}

/* ---- pass 4: the bytes of pseudo-block b, lane l of nl ---- */
AFZ_FN void afi_pass_gather(const afi_ctx* c, int64_t b, int l, int nl) {
    if (b >= c->n_blocks) return;
    const afi_pblock* k = &c->pblocks[b];
    if (afi_is_bad(c, k->stream)) return;
    const afi_stream* st = &c->streams[k->stream];
    uint8_t* o = (st->to_out ? c->out : c->tmp) + st->dst_off + (k->out_pos - st->base);
    for (int64_t j = l; j < k->dsize; j += nl) {
        const uint32_t v = c->src[k->out_pos + j];
        const int64_t li = (int64_t)(v & ~AFZ_LIT);
        o[j] = (v & AFZ_LIT) && li < c->dec_bytes ? c->lit[li] : 0;
    }
}

/* ---- pass 5: Adler-32 piece g (RFC 1950 §8.2); lane l of nl returns ITS share of the sums, the caller adds the lanes' shares up
 * and hands the totals to afi_adler_put ---- */
AFZ_FN int64_t afi_piece_stream(const afi_ctx* c, int64_t g) {      /* the stream that piece g belongs to */
    int64_t lo = 0, hi = c->n_streams - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (c->streams[mid].first_piece <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

AFZ_FN void afi_adler_share(const afi_ctx* c, int64_t g, int l, int nl, uint32_t* a, uint64_t* b) {
    *a = 0; *b = 0;
    if (g >= c->n_pieces) return;
    const int64_t s = afi_piece_stream(c, g);
    if (afi_is_bad(c, s)) return;
    const afi_stream* st = &c->streams[s];
    const int64_t p0 = (g - st->first_piece) * (int64_t)AFI_PIECE;
    const int64_t n = st->dsize - p0 < AFI_PIECE ? st->dsize - p0 : AFI_PIECE;
    const uint8_t* d = (st->to_out ? c->out : c->tmp) + st->dst_off + p0;
    uint32_t sa = 0;
    uint64_t sb = 0;
    for (int64_t i = l; i < n; i += nl) { sa += d[i]; sb += (uint64_t)(n - i) * d[i]; }
    *a = sa; *b = sb;
}

AFZ_FN void afi_adler_put(const afi_ctx* c, int64_t g, uint32_t a, uint64_t b) {
    if (g >= c->n_pieces) return;
    c->adl[2 * g] = a % 65521u;
    c->adl[2 * g + 1] = (uint32_t)(b % 65521u);
}

/* ---- pass 6: the pieces of stream s combined in order, against the trailer ---- */
AFZ_FN void afi_pass_check(const afi_ctx* c, int64_t s) {
    if (s >= c->n_streams || afi_is_bad(c, s)) return;
    const afi_stream* st = &c->streams[s];
    uint64_t A = 1, B = 0;
    int64_t g = st->first_piece;
    for (int64_t p0 = 0; p0 < st->dsize; p0 += AFI_PIECE, ++g) {
        const uint64_t n = (uint64_t)(st->dsize - p0 < AFI_PIECE ? st->dsize - p0 : AFI_PIECE);
        B = (B + (n % 65521u) * A + c->adl[2 * g + 1]) % 65521u;
        A = (A + c->adl[2 * g]) % 65521u;
    }
    if ((uint32_t)((B << 16) | A) != c->want[s]) afi_mark_bad(c, s);
}

#endif
