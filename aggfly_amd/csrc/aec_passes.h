/* aec_passes.h — CCSDS 121.0-B adaptive entropy coding (AEC, as libaec writes it; GRIB2 data representation template 5.42) decoded as
 * independent passes over the steps of a slab.
 *
 * Written in the common subset of C and C++ so that ONE text serves two builds (as inflate_passes.h and zstd_passes.h):
 *   - the HIP kernels of afhip_grib_kernels.h (AFZ_FN = __device__): k_grib_awalk, k_grib_arsi;
 *   - the host decoder of libaggfly_codec.so (blosc1.c: afcodec_aec_decode), which runs the same passes in loops — the CPU tests and
 *     the sanitizer program hold the GPU algorithm to libaec with it.
 *
 * The stream (bits most significant first; n bits per sample, J samples per block, `rsi` blocks per reference sample interval; id_len =
 * 3 for n <= 8, 4 for n <= 16, else 5; an FS code of value v is v zero bits and a one bit).  Only the last RSI may be short and only its
 * last block is padded.  With the preprocessor (flag 8) the first block of every RSI carries a reference sample of n raw bits and J - 1
 * further samples.  Every block begins with an ID of id_len bits:
 *   ID 0, bit 0      zero blocks: [reference,] one FS code v, z = v + 1; z = 5 means "to the end of the segment", min(rsi - b, 64 - b % 64)
 *                    blocks from block b on; z > 5 is one less; the z blocks hold delta 0.  A run may pass the last sample of the stream,
 *                    never the RSI's last block.
 *   ID 0, bit 1      second extension: [reference,] J / 2 FS codes m <= 90, each a pair (a, b) with beta the largest integer with
 *                    beta (beta + 1) / 2 <= m, b = m - beta (beta + 1) / 2, a = beta - b; in a first block the first a is dropped.
 *   ID 2^id_len - 1  uncompressed: J fields of n bits (in a first block the first is the reference).
 *   any other ID     k-split, k = ID - 1: [reference,] all FS codes q of the block, then as many k-bit fields r; delta = q 2^k + r.
 * Without the preprocessor delta is the sample X.  With it, from the reference x on: half = (delta >> 1) + (delta & 1), mask = x has its top
 * bit ? xmax : 0, theta = mask ^ x; half <= theta: x += delta / 2 (even) or x -= (delta + 1) / 2 (odd); otherwise x = mask ^ delta.
 *
 * A block boundary needs no decoding: a k-split block of m codes ends m k bits after its m-th 1-bit, a second-extension block at its
 * (J / 2)-th 1-bit, a zero run at its first.  The passes, each launch-ordered after the one before, no work item waiting for another:
 *   1 walk   per step (a wave on the device, every lane running the same text with the same values): checks the record, then walks the
 *            block headers and leaves the bit where every RSI begins in the RSI table.  The m-th 1-bit from a position on is found by
 *            AEC_NTH_ONE: on the device 64 lanes hold 64 consecutive byte-swapped dwords, a prefix popcount and a ballot name the dword
 *            (aec_nth_one_wave); on the host a loop over dwords (aec_nth_one).  No lane reads the stream sample by sample here.
 *   2 rsi    per RSI (a lane): decodes its blocks to delta, undoes the preprocessor — a serial chain of at most rsi * J links that
 *            depends on nothing outside the RSI — and writes X (uint32) into the value scratch.
 *
 * SAFETY CONTRACT, held in every loop below:
 *   - the bit reader (aec_bits32) returns zeros beyond the step's staged bytes and never reads outside [0, stage_bytes);
 *   - every loop iteration consumes at least one bit, produces a sample or finishes a block, so trip counts are bounded by the step's
 *     bits plus its samples; an FS run that reaches the step's last bit ends the step (AEC_NTH_ONE and aec_fs return -1 there);
 *   - every write is bounded by the step's own part of the scratch: RSI r < max_rsis of the table, sample i < n_values <= n_points of
 *     the values;
 *   - a step is flagged bad, and counted once in *errors, when its record is unsound (sizes, flags, offsets outside the stage, more
 *     RSIs than the table holds), when a zero run passes the last block of its RSI, a second-extension code exceeds 90, a delta exceeds
 *     2^n - 1, or the stream runs beyond its staged bytes;
 *   - later passes skip a bad step.
 */
#ifndef AF_AEC_PASSES_H
#define AF_AEC_PASSES_H
#include "zstd_passes.h"

#define AEC_FLAG_PREPROCESS 8
#define AEC_FLAGS_IGNORED (2 | 4)                    /* 3-byte samples, MSB first: the layout of samples in memory, not of the stream */
#define AEC_RSI_MAX 4096
#define AEC_SE_MAX 90

/* one step of a slab (== afhip_grib_astep, include/aggfly_hip.h) */
typedef struct aec_step {
    int64_t data_off;                 /* the body of the step's section 7 in the stage ... */
    int64_t data_bytes;               /* ... this many bytes */
    int64_t bitmap_off;               /* the step's bitmap in the stage, or -1 (the passes do not read it) */
    int64_t n_values;                 /* samples in the stream */
    int32_t nbits, flags, block_size, rsi;
    double R, s, d;
} aec_step;

typedef struct aec_ctx {
    const uint8_t* stage;             /* 4-byte aligned */
    int64_t stage_bytes;              /* a whole number of dwords */
    const aec_step* steps;
    int64_t n_steps;
    int64_t n_points;                 /* elements of the value scratch per step */
    int64_t max_rsis;                 /* entries of the RSI table per step */
    int32_t* sound;                   /* [n_steps] 1 = the step is sound */
    int64_t* rsi_bit;                 /* [n_steps * max_rsis] the stage bit where an RSI begins */
    uint32_t* vals;                   /* [n_steps * n_points] X */
    int32_t* errors;
} aec_ctx;

/* ---- the bit reader: aligned dwords of the stage, byte-swapped; bits at or beyond `end` read as 0 ---- */
AFZ_FN uint32_t aec_be32(const uint8_t* stage, int64_t q, int64_t stage_bytes) {
    return q >= 0 && q * 4 + 4 <= stage_bytes ? __builtin_bswap32(((const uint32_t*)stage)[q]) : 0u;
}

AFZ_FN uint32_t aec_bits32(const aec_ctx* c, int64_t pos, int64_t end) {      /* the 32 bits from stage bit `pos` on */
    const int64_t q = pos >> 5, left = end - pos;
    const uint64_t win = ((uint64_t)aec_be32(c->stage, q, c->stage_bytes) << 32) | aec_be32(c->stage, q + 1, c->stage_bytes);
    uint32_t v = (uint32_t)((win << (pos & 31)) >> 32);
    if (left <= 0) return 0u;
    if (left < 32) v &= ~(0xffffffffu >> left);
    return v;
}

AFZ_FN uint32_t aec_field(const aec_ctx* c, int64_t pos, int width, int64_t end) {   /* width 0..32 */
    return width ? aec_bits32(c, pos, end) >> (32 - width) : 0u;
}

/* the index from the most significant bit (0..31) of the n-th 1-bit of v, 1 <= n <= popcount(v) */
AFZ_FN int aec_nth_in_word(uint32_t v, int n) {
    int at = 0;
    for (int w = 16; w >= 1; w >>= 1) {
        const int cnt = __builtin_popcount(v >> (32 - w));
        if (cnt < n) {
            n -= cnt;
            v <<= w;
            at += w;
        }
    }
    return at;
}

/* The bit after the count-th 1-bit from `pos` on (count >= 1), or -1 when the step's bits end first: a loop over dwords. */
AFZ_FN int64_t aec_nth_one(const aec_ctx* c, int64_t pos, int64_t count, int64_t end) {
    while (pos < end) {
        const uint32_t v = aec_bits32(c, pos, end);
        const int cnt = __builtin_popcount(v);
        if (cnt >= count) return pos + aec_nth_in_word(v, (int)count) + 1;
        count -= cnt;
        pos += 32;
    }
    return -1;
}

#if defined(__HIPCC__)
/* The same by the 64 lanes of a wave, every lane called with the same arguments and given the same answer: lane l holds the aligned dword
 * (pos >> 5) + l, an inclusive prefix of the popcounts and a ballot name the dword of the count-th 1-bit; 2,048 bits a round. */
__device__ static inline int64_t aec_nth_one_wave(const aec_ctx* c, int64_t pos, int64_t count, int64_t end) {
    const int lane = (int)(threadIdx.x & 63);
    while (pos < end) {
        const int64_t q0 = pos >> 5, mine = (q0 + lane) << 5;                /* the first bit of this lane's dword */
        uint32_t v = aec_be32(c->stage, q0 + lane, c->stage_bytes);
        if (mine < pos) v &= 0xffffffffu >> (pos - mine);                    /* (lane 0 only: pos - mine < 32) */
        if (end - mine <= 0) v = 0u;
        else if (end - mine < 32) v &= ~(0xffffffffu >> (end - mine));
        const int cnt = __builtin_popcount(v);
        int incl = cnt;
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        const int total = __shfl(incl, 63, 64);
        if (total >= count) {
            const int L = __builtin_ctzll(__ballot(incl >= count));
            const int before = __shfl(incl - cnt, L, 64);
            const uint32_t word = (uint32_t)__shfl((int)v, L, 64);
            return ((q0 + L) << 5) + aec_nth_in_word(word, (int)count - before) + 1;
        }
        count -= total;
        pos = (q0 + 64) << 5;
    }
    return -1;
}
#define AEC_NTH_ONE aec_nth_one_wave
#define AEC_LANE0 ((threadIdx.x & 63) == 0)
#define AEC_MARK_BAD(c, t)                                                                    \
    do {                                                                                      \
        if (atomicExch(&(c)->sound[t], 0) == 1) atomicAdd((c)->errors, 1);                    \
    } while (0)
#else
#define AEC_NTH_ONE aec_nth_one
#define AEC_LANE0 1
#define AEC_MARK_BAD(c, t)                                                                    \
    do {                                                                                      \
        if ((c)->sound[t] == 1) {                                                             \
            (c)->sound[t] = 0;                                                                \
            *(c)->errors += 1;                                                                \
        }                                                                                     \
    } while (0)
#endif

AFZ_FN int aec_id_len(int nbits) { return nbits <= 8 ? 3 : nbits <= 16 ? 4 : 5; }

/* Is the record of a step sound?  Every test in a form that cannot overflow: the record is whatever the caller wrote. */
AFZ_FN int aec_record_ok(const aec_ctx* c, const aec_step* r) {
    const int J = r->block_size;
    if (r->data_off < 0 || r->data_bytes < 0 || r->data_off > c->stage_bytes || r->data_bytes > c->stage_bytes - r->data_off) return 0;
    if (r->n_values < 0 || r->n_values > c->n_points || r->nbits < 0 || r->nbits > 32) return 0;
    if (r->flags & ~(AEC_FLAGS_IGNORED | AEC_FLAG_PREPROCESS)) return 0;
    if ((J != 8 && J != 16 && J != 32 && J != 64) || r->rsi < 1 || r->rsi > AEC_RSI_MAX) return 0;
    return (r->n_values + (int64_t)r->rsi * J - 1) / ((int64_t)r->rsi * J) <= c->max_rsis;
}

/* ---- pass 1: the boundary walk of step t.  On the device every lane of one wave runs it with the same values; lane 0 writes. ---- */
AFZ_FN void aec_pass_walk(const aec_ctx* c, int64_t t, int record_ok) {
    const aec_step* r = c->steps + t;
    if (!record_ok || !aec_record_ok(c, r)) {
        if (AEC_LANE0) {
            c->sound[t] = 1;
            AEC_MARK_BAD(c, t);
        }
        return;
    }
    const int n = r->nbits, J = r->block_size, rsi = r->rsi, pp = (r->flags & AEC_FLAG_PREPROCESS) != 0;
    const int idl = aec_id_len(n), idmax = (1 << idl) - 1;
    const int64_t N = r->n_values, per = (int64_t)rsi * J, nr = (N + per - 1) / per;
    const int64_t end = (r->data_off + r->data_bytes) * 8;
    int64_t* table = c->rsi_bit + t * c->max_rsis;
    int64_t pos = r->data_off * 8;
    int bad = 0;
    for (int64_t ri = 0; ri < nr && !bad && n > 0; ++ri) {                  /* (n = 0: a constant field, no stream) */
        if (AEC_LANE0) table[ri] = pos;
        const int64_t cnt = N - ri * per < per ? N - ri * per : per;
        const int64_t nb = (cnt + J - 1) / J;
        int64_t b = 0;
        while (b < nb) {                                                     /* every round finishes at least one block */
            if (pos >= end) { bad = 1; break; }
            const int first = pp && b == 0;
            const int id = (int)aec_field(c, pos, idl, end);
            pos += idl;
            if (id == 0) {
                const int se = (int)aec_field(c, pos, 1, end);
                pos += 1 + (first ? n : 0);
                const int64_t p2 = AEC_NTH_ONE(c, pos, se ? J / 2 : 1, end);
                if (p2 < 0) { bad = 1; break; }
                if (se) {
                    b += 1;
                } else {
                    int64_t z = p2 - pos;                                    /* v + 1 */
                    if (z == 5) z = rsi - b < 64 - (b & 63) ? rsi - b : 64 - (b & 63);
                    else if (z > 5) z -= 1;
                    if (z > rsi - b) { bad = 1; break; }                     /* beyond the RSI's last block */
                    b += z;
                }
                pos = p2;
            } else if (id == idmax) {
                pos += (int64_t)J * n;
                b += 1;
            } else {
                const int m = J - first;
                pos += first ? n : 0;
                const int64_t p2 = AEC_NTH_ONE(c, pos, m, end);
                if (p2 < 0) { bad = 1; break; }
                pos = p2 + (int64_t)m * (id - 1);
                b += 1;
            }
        }
        if (pos > end) bad = 1;
    }
    if (AEC_LANE0) {
        c->sound[t] = 1;
        if (bad) AEC_MARK_BAD(c, t);
    }
}

/* ---- pass 2: RSI ri of step t, by one lane ---- */
/* one FS code at *pos: its value, or -1 when the step's bits end first */
AFZ_FN int64_t aec_fs(const aec_ctx* c, int64_t* pos, int64_t end) {
    int64_t v = 0;
    while (*pos < end) {
        const uint32_t w = aec_bits32(c, *pos, end);
        if (w) {
            const int z = __builtin_clz(w);
            *pos += z + 1;
            return v + z;
        }
        v += 32;
        *pos += 32;
    }
    return -1;
}

typedef struct aec_rsi_state {
    uint32_t* out;
    int64_t cnt, made;                /* samples of the RSI that belong to the stream; samples made so far */
    uint32_t x, xmax;
    int pp, bad;
} aec_rsi_state;

AFZ_FN void aec_emit(aec_rsi_state* s, uint32_t X) {
    if (s->made < s->cnt) s->out[s->made] = X;
    s->made += 1;
}

/* one delta: the sample it stands for (the padding of the stream's last block is read and dropped) */
AFZ_FN void aec_delta(aec_rsi_state* s, uint64_t delta) {
    if (s->made >= s->cnt) {
        s->made += 1;
        return;
    }
    if (delta > s->xmax) {
        s->bad = 1;
        return;
    }
    if (s->pp) {
        const uint32_t dl = (uint32_t)delta, x = s->x;
        const uint32_t half = (dl >> 1) + (dl & 1u), med = s->xmax / 2 + 1;
        const uint32_t mask = (x & med) ? s->xmax : 0u, theta = mask ^ x;
        if (half <= theta) s->x = (dl & 1u) ? x - half : x + half;
        else s->x = mask ^ dl;
        aec_emit(s, s->x);
    } else {
        aec_emit(s, (uint32_t)delta);
    }
}

AFZ_FN void aec_pass_rsi(const aec_ctx* c, int64_t t, int64_t ri) {
    if (t >= c->n_steps || ri >= c->max_rsis || c->sound[t] != 1) return;
    const aec_step* r = c->steps + t;
    const int n = r->nbits, J = r->block_size, rsi = r->rsi;
    const int64_t N = r->n_values, per = (int64_t)rsi * J;
    if (ri * per >= N) return;
    aec_rsi_state s;
    s.out = c->vals + t * c->n_points + ri * per;
    s.cnt = N - ri * per < per ? N - ri * per : per;
    s.made = 0;
    s.x = 0;
    s.xmax = n >= 32 ? 0xffffffffu : (1u << n) - 1u;
    s.pp = (r->flags & AEC_FLAG_PREPROCESS) != 0;
    s.bad = 0;
    if (n == 0) {
        for (int64_t i = 0; i < s.cnt; ++i) s.out[i] = 0u;
        return;
    }
    const int idl = aec_id_len(n), idmax = (1 << idl) - 1;
    const int64_t end = (r->data_off + r->data_bytes) * 8;
    int64_t pos = c->rsi_bit[t * c->max_rsis + ri];
    int64_t b = 0;
    while (s.made < s.cnt && !s.bad) {                                       /* (made = b * J < rsi * J: b < rsi) */
        const int first = s.pp && b == 0;
        const int id = (int)aec_field(c, pos, idl, end);
        pos += idl;
        if (id == 0) {
            const int se = (int)aec_field(c, pos, 1, end);
            pos += 1;
            if (first) {
                s.x = aec_field(c, pos, n, end);
                pos += n;
                aec_emit(&s, s.x);
            }
            if (se) {
                for (int i = 0; i < J / 2 && !s.bad; ++i) {
                    const int64_t m = aec_fs(c, &pos, end);
                    if (m < 0 || m > AEC_SE_MAX) { s.bad = 1; break; }
                    int beta = 0;
                    while ((beta + 1) * (beta + 2) / 2 <= m) ++beta;         /* (at most 12) */
                    const int hi = (int)m - beta * (beta + 1) / 2;
                    if (!(first && i == 0)) aec_delta(&s, (uint64_t)(beta - hi));
                    aec_delta(&s, (uint64_t)hi);
                }
                b += 1;
            } else {
                const int64_t v = aec_fs(c, &pos, end);
                if (v < 0) { s.bad = 1; break; }
                int64_t z = v + 1;
                if (z == 5) z = rsi - b < 64 - (b & 63) ? rsi - b : 64 - (b & 63);
                else if (z > 5) z -= 1;
                if (z > rsi - b) { s.bad = 1; break; }
                const uint32_t X = s.pp ? s.x : 0u;                          /* delta 0 leaves x as it is */
                int64_t m = z * J - first;
                if (m > s.cnt - s.made) m = s.cnt - s.made > 0 ? s.cnt - s.made : 0;
                for (int64_t i = 0; i < m; ++i) s.out[s.made + i] = X;
                s.made = (b + z) * J;
                b += z;
            }
        } else if (id == idmax) {
            for (int i = 0; i < J && !s.bad; ++i) {
                const uint32_t v = aec_field(c, pos, n, end);
                pos += n;
                if (first && i == 0) {
                    s.x = v;
                    aec_emit(&s, v);
                } else {
                    aec_delta(&s, v);
                }
            }
            b += 1;
        } else {
            const int k = id - 1, m = J - first;
            if (first) {
                s.x = aec_field(c, pos, n, end);
                pos += n;
                aec_emit(&s, s.x);
            }
            int64_t low = aec_nth_one(c, pos, m, end);                       /* where the k-bit fields begin */
            if (low < 0) { s.bad = 1; break; }
            for (int i = 0; i < m && !s.bad; ++i) {
                const int64_t q = aec_fs(c, &pos, end);
                if (q < 0 || q > (int64_t)(s.xmax >> k)) { s.bad = 1; break; }
                aec_delta(&s, ((uint64_t)q << k) + aec_field(c, low, k, end));
                low += k;
            }
            pos = low;
            b += 1;
        }
        if (pos > end) s.bad = 1;
    }
    if (s.bad) AEC_MARK_BAD(c, t);
}

#endif /* AF_AEC_PASSES_H */
