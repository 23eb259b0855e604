/* zstd_encode_pass.h — one Zstandard block encoder in explicit lanes (RFC 8878), for the write side of the ingestion path
 * (dataset_to_zarr, compress="blosc-zstd", encode="gpu": a byte plane of a shuffled Blosc block -> one block of a Zstandard frame).
 *
 * One text in the common subset of C and C++ with two builds, as lz4_encode_pass.h (whose lane macros it uses):
 *   - the HIP kernel k_zstd_encode_blocks (afhip_zstd_encode_kernels.h): one wave of 64 lanes per block, ballots and LDS;
 *   - the host emulation afcodec_zstd_encode_block_emulate (blosc1.c): every lane in a loop.
 * THE BYTES OF A BLOCK ARE A FUNCTION OF ITS INPUT ALONE: table reads happen before inserts, inserts are a maximum over positions,
 * histograms and bit counts are sums, bit streams are assembled with ORs, every choice among lanes is "the first lane of a ballot", and
 * the tree construction below is a fixed rule.  The kernel's bytes and the emulation's are identical (tests/test_gpu_zstd_encode.py).
 *
 * A block is encoded on its own: it carries its own Huffman tree (never treeless), its sequences use the three predefined code
 * tables (Compression_Modes 0), it never uses a repeat offset (Offset_Value = offset + 3 always) and never matches before its start.
 * Input n bytes, 1 <= n <= 131072; output one complete block — 3-byte Block_Header and content — of at most n + 3 bytes in a slot of
 * n + 3: an RLE_Block when all bytes are equal, a Compressed_Block when its content is shorter than n, else a Raw_Block.  Every size
 * is known before the first byte of the slot is written; nothing is written outside the slot and the block's own scratch.
 *
 * Stages (each behind a workgroup barrier; the LDS of one stage is reused by the next):
 *   matches    the rounds of afl_encode_wave (lz4_encode_pass.h): 4-byte hash, 16 KiB LDS table, distances 1, 2 and 4 tried first,
 *              first lane of the ballot, wave-wide extension — to the end of the block, at any distance <= position.  A sequence
 *              becomes a record (literal length, match length, offset) in the block's scratch, its literal bytes go to the
 *              scratch's literal buffer.  At AFZE_MAX_SEQ (16,384) sequences, or n / 4 if that is less, the rest of the block
 *              becomes literals.  Trailing literals are ordinary block literals.
 *   sequences  codes and extra bits of every record in parallel; then ONE lane runs the three FSE state chains backwards over the
 *              predefined tables and writes the bit stream into the scratch (its size decides the block type).  The encoding
 *              tables (for every code and every following state: the decoding-table entry to come from) are built once per launch
 *              from afz_*_default through afz_build_fse (afze_build_tables) and copied into LDS.
 *   literals   histogram in LDS; code lengths <= 11 by this rule, serial on one lane over <= 256 symbols: symbols ordered by falling
 *              count (ties: rising value; the order itself is found in parallel), length = ceil(log2(total / count)) held to 1 .. 11;
 *              while the lengths overfill the code space (only the hold at 11 can do that) the rarest symbol below 11 bits grows by
 *              a bit, rarest first; then the space left is handed out from the most frequent symbol on, a bit at a time to every
 *              symbol whose share fits what is left, until none is left.  The result is a complete prefix code (Kraft sum exactly 1).
 *              Tree description: direct 4-bit weights when the last present symbol is <= 128 and that is not longer, else
 *              FSE-compressed weights (counts normalised to 64 = accuracy log 6, two interleaved states); if neither form exists
 *              the literals are raw.  One stream up to 1023 literals (the only size format with one), four with the jump table
 *              above.  The streams are written by all lanes: tiles of 1024 literals from the end of a stream, 16 a lane, a scan of
 *              the lanes' bit counts, ORs into an LDS tile, bytes out.  Raw literals under AFZE_MIN_HUF (64) literals or when the
 *              Huffman form with its headers is not shorter.  RLE literals cannot arise: the first occurrence of every byte value
 *              is a literal (a match copies earlier bytes of the block), so literals of one value mean a block of one value, and
 *              that is an RLE block.
 */
#ifndef AF_ZSTD_ENCODE_PASS_H
#define AF_ZSTD_ENCODE_PASS_H
#include <stdint.h>
#include <string.h>

#include "lz4_encode_pass.h"
#include "zstd_passes.h"

#define AFZE_MAX_SEQ 16384
#define AFZE_MIN_HUF 64
#define AFZE_HUF_MAXBITS 11
#define AFZE_TILE_PER_LANE 16
#define AFZE_TILE (AFL_LANES * AFZE_TILE_PER_LANE)

/* the launch's encoding tables (bytes): 3 x 64 decoding entries of afz_build_fse, then per table [code][state] -> entry */
#define AFZE_TAB_DEC 0
#define AFZE_TAB_LL 768                       /* 36 x 64 */
#define AFZE_TAB_OF (768 + 36 * 64)           /* 29 x 32 */
#define AFZE_TAB_ML (AFZE_TAB_OF + 29 * 32)   /* 53 x 64 */
#define AFZE_TAB_USED (AFZE_TAB_ML + 53 * 64) /* 7,392 */
#define AFZE_TAB_BYTES 7424

/* LDS of a wave, in uint32 words */
#define AFZE_LDS_MAIN 0                       /* 4,096: hash table | encoding tables | stream tile + weight coder */
#define AFZE_LDS_HIST 4096                    /* 256 */
#define AFZE_LDS_CODE 4352                    /* 256: code | length << 16 */
#define AFZE_LDS_ORDER 4608                   /* 256 */
#define AFZE_LDS_MISC 4864                    /* 64 lane sums, 16 results */
#define AFZE_LDS_WORDS 4944
/* inside AFZE_LDS_MAIN during the literal stage */
#define AFZE_M_TILE 0                         /* 360 words: 1024 x 11 bits + 7, and a word to spare */
#define AFZE_M_WDEC 512                       /* 64: decoding entries of the weight table */
#define AFZE_M_WENC 576                       /* 192 words = 12 x 64 bytes: [weight][state] -> entry */
#define AFZE_M_DESC 768                       /* 64 words = 256 bytes: the FSE-compressed description */
#define AFZE_M_WGT 832                        /* 256: the weights */

#if defined(__HIPCC__)
#define AFZE_HD __host__ __device__ static inline
#define AFZE_ADD(p, v) atomicAdd((p), (v))                              /* LDS sums and ORs: the same for every lane order */
#define AFZE_OR(p, v) atomicOr((p), (v))
#else
#define AFZE_HD static inline
#define AFZE_ADD(p, v) (*(p) += (v))
#define AFZE_OR(p, v) (*(p) |= (v))
#endif

typedef struct afze_seq { uint32_t ll, ml, off, codes; } afze_seq;   /* codes: LL | ML << 8 | OF << 16 */

AFZE_HD int32_t afze_seq_cap(int32_t n) { return n / 4 < AFZE_MAX_SEQ ? n / 4 : AFZE_MAX_SEQ; }
AFZE_HD int64_t afze_align16(int64_t v) { return (v + 15) & ~(int64_t)15; }
/* a block's scratch: literals | sequence records | sequences bit stream (<= 66 bits a sequence) */
AFZE_HD int64_t afze_scratch_seq(int32_t n) { return afze_align16(n); }
AFZE_HD int64_t afze_scratch_bits(int32_t n) { return afze_scratch_seq(n) + (int64_t)afze_seq_cap(n) * (int64_t)sizeof(afze_seq); }
AFZE_HD int64_t afze_scratch_bytes(int32_t n) {
    return (afze_scratch_bits(n) + afze_align16((int64_t)afze_seq_cap(n) * 9 + 16) + 255) & ~(int64_t)255;
}

/* ---- the launch's tables: serial, once ---- */
AFZ_FN void afze_build_tables(uint8_t* tab) {
    int16_t norm[53];
    uint16_t next[53];
    for (int t = 0; t < 3; ++t) {
        const int16_t* src = t == 0 ? afz_ll_default : (t == 1 ? afz_of_default : afz_ml_default);
        const int nsym = t == 0 ? 36 : (t == 1 ? 29 : 53), lg = t == 1 ? 5 : 6, size = 1 << lg;
        uint32_t* dec = (uint32_t*)(void*)(tab + AFZE_TAB_DEC) + 64 * t;
        uint8_t* enc = tab + (t == 0 ? AFZE_TAB_LL : (t == 1 ? AFZE_TAB_OF : AFZE_TAB_ML));
        for (int s = 0; s < nsym; ++s) norm[s] = src[s];
        afz_build_fse(norm, nsym, lg, dec, next);
        for (int u = 0; u < size; ++u) {
            const uint32_t e = dec[u], s = e & 0xff, nb = (e >> 8) & 0xff, base = e >> 16;
            for (uint32_t c = 0; c < (1u << nb); ++c) enc[s * size + base + c] = (uint8_t)u;
        }
    }
}

/* ---- a forward bit writer of one lane (bytes at p; the caller knows the bound) ---- */
typedef struct afze_bits { uint8_t* p; int64_t n; uint64_t acc; int cnt; } afze_bits;
AFZ_FN void afze_put(afze_bits* b, uint32_t v, int nb) {   /* nb <= 24 */
    b->acc |= (uint64_t)v << b->cnt;
    b->cnt += nb;
    while (b->cnt >= 8) { b->p[b->n++] = (uint8_t)b->acc; b->acc >>= 8; b->cnt -= 8; }
}
AFZ_FN int64_t afze_put_end(afze_bits* b) {                /* the closing 1 bit */
    afze_put(b, 1, 1);
    if (b->cnt) { b->p[b->n++] = (uint8_t)b->acc; b->acc = 0; b->cnt = 0; }
    return b->n;
}

AFZ_FN uint32_t afze_code_of(const uint32_t* base, int top, uint32_t v) {   /* the largest code whose baseline is <= v */
    int c = top;
    while (base[c] > v) --c;
    return (uint32_t)c;
}

/* bytes of a literals section header: raw (coded = 0) or Huffman */
AFZ_FN int32_t afze_lit_header_bytes(int32_t regen, int coded) {
    if (!coded) return regen < 32 ? 1 : (regen < 4096 ? 2 : 3);
    return regen < 1024 ? 3 : (regen < 16384 ? 4 : 5);
}

/* ---- the tree description of FSE-compressed weights, serial: wgt[0 .. nw) (each <= 11) -> bytes at desc (<= 255), or 0 = none ---- */
AFZ_FN int32_t afze_weights_fse(const uint32_t* wgt, int nw, uint8_t* desc, uint32_t* wdec, uint8_t* wenc) {
    int16_t norm[12];
    uint16_t next[12];
    int32_t count[12];
    if (nw < 2) return 0;
    for (int s = 0; s < 12; ++s) count[s] = 0;
    for (int i = 0; i < nw; ++i) count[wgt[i]]++;
    int nsym = 0, best = 0, sum = 0;
    for (int s = 0; s < 12; ++s) {
        if (count[s]) nsym = s + 1;
        if (count[s] > count[best]) best = s;
        norm[s] = (int16_t)(count[s] ? (count[s] * 64 / nw ? count[s] * 64 / nw : 1) : 0);
        sum += norm[s];
    }
    if (count[best] == nw) return 0;                       /* one weight value: a table of one symbol codes nothing */
    norm[best] = (int16_t)(norm[best] + 64 - sum);         /* the most frequent weight takes the difference */
    if (norm[best] < 1) return 0;
    /* the normalised counts (RFC 8878 section 4.1.1), accuracy log 6 */
    afze_bits w;
    w.p = desc + 1; w.n = 0; w.acc = 0; w.cnt = 0;
    afze_put(&w, 6 - 5, 4);
    int remaining = 65, threshold = 64, nb = 7, s = 0, prev0 = 0;
    while (s < nsym && remaining > 1) {
        if (prev0) {
            int start = s;
            while (s < nsym && !norm[s]) ++s;
            if (s == nsym) return 0;
            while (s >= start + 3) { start += 3; afze_put(&w, 3, 2); }
            afze_put(&w, (uint32_t)(s - start), 2);
        }
        int c = norm[s++];
        const int mx = 2 * threshold - 1 - remaining;
        remaining -= c;
        ++c;
        if (c >= threshold) c += mx;
        afze_put(&w, (uint32_t)c, nb - (c < mx));
        prev0 = c == 1;
        while (remaining < threshold) { --nb; threshold >>= 1; }
    }
    if (remaining != 1) return 0;
    if (w.cnt) { w.p[w.n++] = (uint8_t)w.acc; w.acc = 0; w.cnt = 0; }
    if (afz_build_fse(norm, nsym, 6, wdec, next)) return 0;
    for (int u = 0; u < 64; ++u) {
        const uint32_t e = wdec[u], sy = e & 0xff, nbits = (e >> 8) & 0xff, base = e >> 16;
        for (uint32_t c = 0; c < (1u << nbits); ++c) wenc[sy * 64 + base + c] = (uint8_t)u;
    }
    /* two interleaved states, backwards: weight j belongs to state j & 1; a chain starts from the entry of its last weight that takes
     * the most bits (the one whose range holds state 63), so the reader runs dry exactly there */
    if (w.n + (nw * 6 + 13 + 7) / 8 > 254) return 0;
    int32_t st[2] = {-1, -1};
    for (int j = nw - 1; j >= 0; --j) {
        const int k = j & 1;
        if (st[k] < 0) { st[k] = wenc[wgt[j] * 64 + 63]; continue; }
        const uint32_t u = wenc[wgt[j] * 64 + st[k]], e = wdec[u];
        afze_put(&w, (uint32_t)st[k] - (e >> 16), (int)((e >> 8) & 0xff));
        st[k] = (int32_t)u;
    }
    afze_put(&w, (uint32_t)st[1], 6);
    afze_put(&w, (uint32_t)st[0], 6);
    const int64_t bytes = afze_put_end(&w);
    if (bytes > 127) return 0;
    desc[0] = (uint8_t)bytes;
    return (int32_t)bytes + 1;
}

/* ---- one Huffman stream of lit[a .. e) at dst, by all lanes -> its bytes (bits / 8 + 1) ---- */
AFL_FN int32_t afze_huf_stream(uint8_t* dst, const uint8_t* lit, int32_t a, int32_t e, uint32_t* lds, int lane) {
    uint32_t* tile = lds + AFZE_LDS_MAIN + AFZE_M_TILE;
    uint32_t* sums = lds + AFZE_LDS_MISC;
    const uint32_t* code = lds + AFZE_LDS_CODE;
    int64_t B = 0;                                          /* bits of the stream so far; the bits below B & 7 of its last byte wait in `carry` */
    uint32_t carry = 0;
    int32_t hi = e;
    while (hi > a) {
        AFL_EACH_LANE {
            uint32_t s = 0;
            for (int k = 0; k < AFZE_TILE_PER_LANE; ++k) {
                const int32_t i = hi - 1 - (lane * AFZE_TILE_PER_LANE + k);
                if (i >= a) s += code[lit[i]] >> 16;
            }
            sums[lane] = s;
            for (int i = lane; i < 360; i += AFL_LANES) tile[i] = 0;
        }
        AFL_SYNC();
        uint32_t tb = 0;
        for (int j = 0; j < AFL_LANES; ++j) tb += sums[j];
        AFL_EACH_LANE {
            uint32_t at = (uint32_t)(B & 7);
            for (int j = 0; j < lane; ++j) at += sums[j];
            if (lane == 0 && carry) AFZE_OR(&tile[0], carry);
            for (int k = 0; k < AFZE_TILE_PER_LANE; ++k) {
                const int32_t i = hi - 1 - (lane * AFZE_TILE_PER_LANE + k);
                if (i < a) break;
                const uint32_t c = code[lit[i]], v = c & 0xffff, nb = c >> 16, sh = at & 31;
                AFZE_OR(&tile[at >> 5], v << sh);
                if (sh + nb > 32) AFZE_OR(&tile[(at >> 5) + 1], v >> (32 - sh));
                at += nb;
            }
        }
        AFL_SYNC();
        const uint32_t bits = (uint32_t)(B & 7) + tb, full = bits >> 3;
        carry = (tile[full >> 2] >> (8 * (full & 3))) & 0xff;
        uint8_t* out = dst + (B >> 3);
        AFL_EACH_LANE {
            for (uint32_t i = (uint32_t)lane; i < full; i += AFL_LANES) out[i] = (uint8_t)(tile[i >> 2] >> (8 * (i & 3)));
        }
        AFL_SYNC();
        B += tb;
        hi -= AFZE_TILE;
    }
    AFL_EACH_LANE {
        if (lane == 0) dst[B >> 3] = (uint8_t)(carry | (1u << (B & 7)));
    }
    return (int32_t)(B >> 3) + 1;
}

AFL_FN void afze_block_header(uint8_t* dst, int type, int32_t size, int last, int lane) {
    const uint32_t h = (uint32_t)(last != 0) | ((uint32_t)type << 1) | ((uint32_t)size << 3);
    AFL_EACH_LANE {
        if (lane < 3) dst[lane] = (uint8_t)(h >> (8 * lane));
    }
}

/* src[0 .. n) -> one block at dst (n + 3 bytes); scratch: afze_scratch_bytes(n) bytes, the block's own; tables: the launch's
 * (afze_build_tables); lds: AFZE_LDS_WORDS words, the wave's own.  lane: the calling lane (kernel) / unused (host).  -> bytes of the block */
AFL_FN int32_t afze_encode_block(const uint8_t* src, int32_t n, int last, uint8_t* dst, uint8_t* scratch, const uint8_t* tables,
                                 uint32_t* lds, int lane) {
    uint32_t* table = lds + AFZE_LDS_MAIN;
    uint32_t* hist = lds + AFZE_LDS_HIST;
    uint32_t* code = lds + AFZE_LDS_CODE;
    uint32_t* order = lds + AFZE_LDS_ORDER;
    uint32_t* misc = lds + AFZE_LDS_MISC + 64;
    uint8_t* lit = scratch;
    afze_seq* seqs = (afze_seq*)(void*)(scratch + afze_scratch_seq(n));
    uint8_t* sbits = scratch + afze_scratch_bits(n);
    const int32_t cap = afze_seq_cap(n);

    /* ---- all bytes equal: an RLE block ---- */
    {
        int same = 1;
        for (int32_t i0 = 0; i0 < n && same; i0 += AFL_LANES) {
            AFL_VAR(uint32_t, differs);
            AFL_EACH_LANE { AFL_L(differs) = i0 + lane < n && src[i0 + lane] != src[0]; }
            if (AFL_BALLOT(differs)) same = 0;
        }
        if (same) {
            afze_block_header(dst, 1, n, last, lane);
            AFL_EACH_LANE { if (lane == 0) dst[3] = src[0]; }
            return 4;
        }
    }

    /* ---- matches ---- */
    int32_t ip = 0, anchor = 0, nlit = 0, nseq = 0;
    AFL_EACH_LANE {
        for (int32_t i = lane; i < AFL_TABLE_ENTRIES; i += AFL_LANES) table[i] = 0;
    }
    AFL_SYNC();
    const int32_t search_end = n - 4;                       /* the last position with a 4-byte word */
    while (ip <= search_end && nseq < cap) {
        AFL_VAR(uint32_t, w);
        AFL_VAR(uint32_t, h);
        AFL_VAR(uint32_t, cand);
        AFL_VAR(uint32_t, dist);
        AFL_EACH_LANE {                                     /* every lane reads ... */
            const int32_t pos = ip + lane;
            AFL_L(w) = 0;
            AFL_L(h) = 0;
            AFL_L(cand) = 0;
            if (pos <= search_end) {
                AFL_L(w) = AFL_LOAD32(src + pos);
                AFL_L(h) = (AFL_L(w) * 2654435761u) >> (32 - AFL_HASH_LOG);
                AFL_L(cand) = table[AFL_L(h)];
            }
        }
        AFL_EACH_LANE {
            const int32_t pos = ip + lane;
            uint32_t d = 0;
            if (pos <= search_end) {
                if (pos >= 1 && AFL_LOAD32(src + pos - 1) == AFL_L(w)) d = 1;
                else if (pos >= 2 && AFL_LOAD32(src + pos - 2) == AFL_L(w)) d = 2;
                else if (pos >= 4 && AFL_LOAD32(src + pos - 4) == AFL_L(w)) d = 4;
                else if (AFL_L(cand)) {
                    const int32_t c = (int32_t)AFL_L(cand) - 1;
                    if (c < pos && AFL_LOAD32(src + c) == AFL_L(w)) d = (uint32_t)(pos - c);
                }
            }
            AFL_L(dist) = d;
        }
        const uint64_t found = AFL_BALLOT(dist);
        const int fm = found ? AFL_CTZ64(found) : AFL_LANES - 1;
        AFL_SYNC();
        AFL_EACH_LANE {                                     /* ... before any lane inserts */
            const int32_t pos = ip + lane;
            if (pos <= search_end && lane <= fm) AFL_TABLE_MAX(table, AFL_L(h), (uint32_t)pos + 1);
        }
        AFL_SYNC();
        if (!found) {
            ip += AFL_LANES;
            continue;
        }
        const int32_t mpos = ip + fm;
        const int32_t off = (int32_t)AFL_LANE_VALUE(dist, fm);
        const int32_t max_len = n - mpos;
        int32_t mlen = 4;
        while (mlen < max_len) {
            AFL_VAR(uint32_t, differs);
            AFL_EACH_LANE {
                const int32_t i = mlen + lane;
                AFL_L(differs) = i >= max_len || src[mpos + i] != src[mpos - off + i];
            }
            const uint64_t stop = AFL_BALLOT(differs);
            if (stop) {
                mlen += AFL_CTZ64(stop);
                break;
            }
            mlen += AFL_LANES;
        }
        const int32_t ll = mpos - anchor;
        afl_copy(lit + nlit, src + anchor, ll, lane);
        AFL_EACH_LANE {
            if (lane == 0) {
                seqs[nseq].ll = (uint32_t)ll;
                seqs[nseq].ml = (uint32_t)mlen;
                seqs[nseq].off = (uint32_t)off;
            }
        }
        nlit += ll;
        ++nseq;
        ip = anchor = mpos + mlen;
    }
    afl_copy(lit + nlit, src + anchor, n - anchor, lane);
    nlit += n - anchor;
    AFL_SYNC();
#if defined(AFZE_STOP_AFTER)                                 /* scripts/probe/zstd_encode_stages.hip alone: the time of the first stages */
    if (AFZE_STOP_AFTER == 1) return nseq;
#endif

    /* ---- sequences: the codes in parallel, the state chains on one lane ---- */
    int32_t seq_bytes = 1;                                  /* Number_of_Sequences = 0 */
    if (nseq) {
        AFL_EACH_LANE {
            for (int32_t i = lane; i < nseq; i += AFL_LANES) {
                const uint32_t llc = afze_code_of(afz_ll_base, 35, seqs[i].ll), mlc = afze_code_of(afz_ml_base, 52, seqs[i].ml);
                seqs[i].codes = llc | (mlc << 8) | ((uint32_t)afz_highbit32(seqs[i].off + 3) << 16);
            }
            for (int32_t i = lane; i < AFZE_TAB_USED / 4; i += AFL_LANES) table[i] = ((const uint32_t*)(const void*)tables)[i];
        }
        AFL_SYNC();
        AFL_EACH_LANE {
            if (lane == 0) {
                const uint32_t* dec = table + AFZE_TAB_DEC / 4;
                const uint8_t* enc_ll = (const uint8_t*)(const void*)table + AFZE_TAB_LL;
                const uint8_t* enc_of = (const uint8_t*)(const void*)table + AFZE_TAB_OF;
                const uint8_t* enc_ml = (const uint8_t*)(const void*)table + AFZE_TAB_ML;
                afze_bits w;
                w.p = sbits; w.n = 0; w.acc = 0; w.cnt = 0;
                uint32_t sl = 0, so = 0, sm = 0;
                for (int32_t i = nseq - 1; i >= 0; --i) {
                    const afze_seq q = seqs[i];
                    const uint32_t llc = q.codes & 0xff, mlc = (q.codes >> 8) & 0xff, ofc = q.codes >> 16;
                    if (i == nseq - 1) {                    /* the last sequence: states that cost nothing */
                        sl = enc_ll[llc * 64 + 63]; so = enc_of[ofc * 32 + 31]; sm = enc_ml[mlc * 64 + 63];
                    } else {                                /* read LL, ML, OF: written OF, ML, LL */
                        uint32_t u = enc_of[ofc * 32 + so], e = dec[64 + u];
                        afze_put(&w, so - (e >> 16), (int)((e >> 8) & 0xff));
                        so = u;
                        u = enc_ml[mlc * 64 + sm]; e = dec[128 + u];
                        afze_put(&w, sm - (e >> 16), (int)((e >> 8) & 0xff));
                        sm = u;
                        u = enc_ll[llc * 64 + sl]; e = dec[u];
                        afze_put(&w, sl - (e >> 16), (int)((e >> 8) & 0xff));
                        sl = u;
                    }
                    /* read OF, ML, LL: written LL, ML, OF */
                    afze_put(&w, q.ll - afz_ll_base[llc], afz_ll_bits[llc]);
                    afze_put(&w, q.ml - afz_ml_base[mlc], afz_ml_bits[mlc]);
                    afze_put(&w, (q.off + 3) - (1u << ofc), (int)ofc);
                }
                afze_put(&w, sm, 6);
                afze_put(&w, so, 5);
                afze_put(&w, sl, 6);
                misc[0] = (uint32_t)afze_put_end(&w);
            }
        }
        AFL_SYNC();
        seq_bytes = (nseq < 128 ? 1 : 2) + 1 + (int32_t)misc[0];
    }
#if defined(AFZE_STOP_AFTER)
    if (AFZE_STOP_AFTER == 2) return seq_bytes;
#endif

    /* ---- literals: histogram, lengths, codes, description, sizes ---- */
    int lit_type = 0;                                       /* 0 raw, 2 Huffman */
    int32_t desc_bytes = 0, n_streams = 1, sbytes[4] = {0, 0, 0, 0}, desc_fse = 0, nw = 0;
    const int32_t seg = (nlit + 3) / 4;
    AFL_EACH_LANE {
        for (int i = lane; i < 256; i += AFL_LANES) hist[i] = 0;
    }
    AFL_SYNC();
    AFL_EACH_LANE {
        for (int32_t i = lane; i < nlit; i += AFL_LANES) AFZE_ADD(&hist[lit[i]], 1u);
    }
    AFL_SYNC();
    if (nlit >= 1) {
        AFL_EACH_LANE {                                     /* order[r] = the symbol of rank r: falling count, rising value */
            for (int s = lane; s < 256; s += AFL_LANES) {
                const uint32_t c = hist[s];
                int r = 0;
                for (int t = 0; t < 256; ++t) r += hist[t] > c || (hist[t] == c && t < s);
                order[r] = (uint32_t)s;
            }
        }
        AFL_SYNC();
    }
    if (nlit >= AFZE_MIN_HUF) {
        uint32_t* wgt = lds + AFZE_LDS_MAIN + AFZE_M_WGT;
        AFL_EACH_LANE {
            if (lane == 0) {
                int nsym = 0;
                while (nsym < 256 && hist[order[nsym]]) ++nsym;
                int32_t kraft = 0;                          /* in units of 2^-11 */
                for (int i = 0; i < 256; ++i) code[i] = 0;
                for (int i = 0; i < nsym; ++i) {
                    const uint32_t c = hist[order[i]];
                    int len = 0;
                    while (((uint64_t)c << len) < (uint64_t)nlit) ++len;
                    if (len < 1) len = 1;
                    if (len > AFZE_HUF_MAXBITS) len = AFZE_HUF_MAXBITS;
                    code[order[i]] = (uint32_t)len << 16;
                    kraft += 1 << (AFZE_HUF_MAXBITS - len);
                }
                int moved = 1;                              /* (a pass that moves nothing ends its loop: no loop here can spin) */
                while (kraft > 2048 && moved) {
                    moved = 0;
                    for (int i = nsym - 1; i >= 0 && kraft > 2048; --i) {
                        const int len = (int)(code[order[i]] >> 16);
                        if (len < AFZE_HUF_MAXBITS) {
                            code[order[i]] = (uint32_t)(len + 1) << 16;
                            kraft -= 1 << (AFZE_HUF_MAXBITS - len - 1);
                            moved = 1;
                        }
                    }
                }
                int32_t spare = 2048 - kraft;
                moved = 1;
                while (spare > 0 && moved) {
                    moved = 0;
                    for (int i = 0; i < nsym && spare > 0; ++i) {
                        const int len = (int)(code[order[i]] >> 16);
                        const int32_t unit = 1 << (AFZE_HUF_MAXBITS - len);
                        if (len > 1 && unit <= spare) {
                            code[order[i]] = (uint32_t)(len - 1) << 16;
                            spare -= unit;
                            moved = 1;
                        }
                    }
                }
                int maxbits = 0, lastsym = 0;
                for (int s = 0; s < 256; ++s)
                    if (code[s]) {
                        lastsym = s;
                        if ((int)(code[s] >> 16) > maxbits) maxbits = (int)(code[s] >> 16);
                    }
                /* canonical codes as the reader builds its table: rising weight, then rising symbol */
                uint32_t start[AFZE_HUF_MAXBITS + 2], pos = 0;
                for (int wv = 1; wv <= maxbits; ++wv) {
                    start[wv] = pos;
                    for (int s = 0; s <= lastsym; ++s)
                        if (code[s] && maxbits + 1 - (int)(code[s] >> 16) == wv) pos += 1u << (wv - 1);
                }
                for (int s = 0; s <= lastsym; ++s) {
                    wgt[s] = 0;
                    if (!code[s]) continue;
                    const int wv = maxbits + 1 - (int)(code[s] >> 16);
                    wgt[s] = (uint32_t)wv;
                    code[s] |= start[wv] >> (wv - 1);
                    start[wv] += 1u << (wv - 1);
                }
                misc[1] = spare == 0 ? (uint32_t)lastsym : 999u;   /* the weights listed: symbols 0 .. lastsym - 1 (999: no complete code, so no tree) */
                misc[2] = spare != 0 ? 0u : (uint32_t)afze_weights_fse(wgt, lastsym, (uint8_t*)(void*)(lds + AFZE_LDS_MAIN + AFZE_M_DESC),
                                                     lds + AFZE_LDS_MAIN + AFZE_M_WDEC, (uint8_t*)(void*)(lds + AFZE_LDS_MAIN + AFZE_M_WENC));
                misc[4] = misc[5] = misc[6] = misc[7] = 0;
            }
        }
        AFL_SYNC();
        nw = (int32_t)misc[1];
        const int32_t fse_bytes = (int32_t)misc[2], direct_bytes = nw <= 128 ? 1 + (nw + 1) / 2 : 0;
        if (direct_bytes && (!fse_bytes || direct_bytes <= fse_bytes)) desc_bytes = direct_bytes;
        else if (fse_bytes) { desc_bytes = fse_bytes; desc_fse = 1; }
        if (desc_bytes) {
            n_streams = nlit < 1024 ? 1 : 4;
            for (int k = 0; k < n_streams; ++k) {           /* bits of every stream: sums */
                const int32_t a = n_streams == 1 ? 0 : k * seg, e = n_streams == 1 || k == 3 ? nlit : (k + 1) * seg;
                AFL_EACH_LANE {
                    uint32_t s = 0;
                    for (int32_t i = a + lane; i < e; i += AFL_LANES) s += code[lit[i]] >> 16;
                    AFZE_ADD(&misc[4 + k], s);
                }
            }
            AFL_SYNC();
            int32_t csize = desc_bytes + (n_streams == 4 ? 6 : 0);
            for (int k = 0; k < n_streams; ++k) {
                sbytes[k] = (int32_t)(misc[4 + k] >> 3) + 1;
                csize += sbytes[k];
            }
            if (afze_lit_header_bytes(nlit, 1) + csize < afze_lit_header_bytes(nlit, 0) + nlit) lit_type = 2;
        }
    }
    int32_t lit_csize = 0, lit_bytes;
    if (lit_type == 2) {
        lit_csize = desc_bytes + (n_streams == 4 ? 6 : 0) + sbytes[0] + sbytes[1] + sbytes[2] + sbytes[3];
        lit_bytes = afze_lit_header_bytes(nlit, 1) + lit_csize;
    } else {
        lit_bytes = afze_lit_header_bytes(nlit, 0) + nlit;
    }

    /* ---- every size is known: the block type ---- */
    const int32_t content = lit_bytes + seq_bytes;
    if (content >= n) {
        afze_block_header(dst, 0, n, last, lane);
        afl_copy(dst + 3, src, n, lane);
        return n + 3;
    }
    afze_block_header(dst, 2, content, last, lane);
    uint8_t* op = dst + 3;
    if (lit_type < 2) {
        const int hb = afze_lit_header_bytes(nlit, 0);
        const uint32_t h = hb == 1 ? (uint32_t)nlit << 3 : ((hb == 2 ? 1u : 3u) << 2) | ((uint32_t)nlit << 4);
        AFL_EACH_LANE {
            if (lane < hb) op[lane] = (uint8_t)(h >> (8 * lane));
        }
        afl_copy(op + hb, lit, nlit, lane);
        op += lit_bytes;
    } else {
        const int hb = afze_lit_header_bytes(nlit, 1), sf = hb == 3 ? (n_streams == 1 ? 0 : 1) : hb - 2, fb = hb == 3 ? 10 : (hb == 4 ? 14 : 18);
        const uint64_t h = 2u | ((uint64_t)sf << 2) | ((uint64_t)nlit << 4) | ((uint64_t)lit_csize << (4 + fb));
        AFL_EACH_LANE {
            if (lane < hb) op[lane] = (uint8_t)(h >> (8 * lane));
        }
        op += hb;
        if (desc_fse) {
            const uint32_t* d = lds + AFZE_LDS_MAIN + AFZE_M_DESC;
            AFL_EACH_LANE {
                for (int i = lane; i < desc_bytes; i += AFL_LANES) op[i] = (uint8_t)(d[i >> 2] >> (8 * (i & 3)));
            }
        } else {
            const uint32_t* wgt = lds + AFZE_LDS_MAIN + AFZE_M_WGT;
            AFL_EACH_LANE {
                if (lane == 0) op[0] = (uint8_t)(127 + nw);
                for (int i = lane; i < (nw + 1) / 2; i += AFL_LANES)
                    op[1 + i] = (uint8_t)((wgt[2 * i] << 4) | (2 * i + 1 < nw ? wgt[2 * i + 1] : 0));
            }
        }
        op += desc_bytes;
        if (n_streams == 4) {
            AFL_EACH_LANE {
                const int32_t sb = lane < 2 ? sbytes[0] : (lane < 4 ? sbytes[1] : sbytes[2]);
                if (lane < 6) op[lane] = (uint8_t)(sb >> (8 * (lane & 1)));
            }
            op += 6;
        }
        AFL_SYNC();
        for (int k = 0; k < n_streams; ++k) {
            const int32_t a = n_streams == 1 ? 0 : k * seg, e = n_streams == 1 || k == 3 ? nlit : (k + 1) * seg;
            op += afze_huf_stream(op, lit, a, e, lds, lane);
        }
    }
    if (!nseq) {
        AFL_EACH_LANE { if (lane == 0) op[0] = 0; }
        return content + 3;
    }
    const int nh = nseq < 128 ? 1 : 2;
    AFL_EACH_LANE {
        if (lane == 0) {
            if (nh == 1) op[0] = (uint8_t)nseq;
            else { op[0] = (uint8_t)((nseq >> 8) + 128); op[1] = (uint8_t)nseq; }
            op[nh] = 0;                                     /* Compression_Modes: predefined, predefined, predefined */
        }
    }
    afl_copy(op + nh + 1, sbits, seq_bytes - nh - 1, lane);
    return content + 3;
}

#endif
