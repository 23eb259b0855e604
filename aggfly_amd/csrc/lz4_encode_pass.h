/* lz4_encode_pass.h — one LZ4 block encoder in explicit lanes, for the write side of the ingestion path (dataset_to_zarr,
 * encode="gpu": a byte plane of a shuffled Blosc block -> one LZ4 stream).
 *
 * Written in the common subset of C and C++ so that ONE text serves two builds, as zstd_passes.h and inflate_passes.h do:
 *   - the HIP kernel k_lz4_encode_streams (afhip_lz4_encode_kernels.h): one wave of 64 lanes per stream, the lanes of a step run
 *     together, ballots and lane reads are the hardware's;
 *   - the host emulation afcodec_lz4_encode_emulate (blosc1.c): every per-lane value is an array of 64, every step a loop over the
 *     lanes, a ballot a loop over the array.
 * THE BYTES OF A STREAM ARE A FUNCTION OF ITS INPUT ALONE.  Nothing below depends on the order in which lanes run: every lane reads
 * its hash-table entry before any lane inserts, insertion is a maximum over positions, and every choice among lanes is "the first
 * lane of a ballot".  The kernel's output and the emulation's are therefore byte-identical (tests/test_gpu_lz4_encode.py).
 *
 * A round looks at the 64 positions ip .. ip + 63:
 *   1 every lane takes the 4-byte word at its position and hashes it (12 bits: 4,096 table entries of 4 bytes = 16 KiB of LDS, each
 *     the last position + 1 that hashed there, 0 = none: positions of a 256 KiB stream never alias), and reads its entry;
 *   2 every lane looks for a match of its word: at distance 1, 2 and 4 first (runs and short periods inside ONE round are invisible
 *     to a table read before it is written — the nearly constant exponent plane of a float field is exactly that), then at the
 *     table's candidate; a candidate is verified against the input and taken only at distances 1 .. 65,535;
 *   3 a ballot picks the first lane with a match; the lanes up to it (all of them when there is none) insert their positions;
 *   4 no match: the round's bytes stay pending literals, ip += 64.  A match: the wave extends it 64 bytes a step (ballot of the
 *     first mismatch), up to 5 bytes before the end, and emits the sequence — token, literal-length extension, the literals
 *     (copied by all lanes), offset, match-length extension; ip = the match's end.
 * End of block (LZ4 block format): no match starts within the last 12 bytes (nor at the 13th from the end: a little stricter), the
 * last 5 bytes are literals, the last sequence is literals only.
 * A stream that would not fit into n - 1 bytes is STORED: the raw bytes are copied into the slot (capacity n) and n is returned — the rule
 * of afcodec_blosc_encode.  Every sequence is checked against n - 1 BEFORE it is written, so nothing is written outside the slot.
 * Every loop consumes input: a round advances ip by 64 or by a match of 4 bytes at least; an extension step by 64 bytes.  The encoder
 * reads its input and its table only, never its output.
 */
#ifndef AF_LZ4_ENCODE_PASS_H
#define AF_LZ4_ENCODE_PASS_H
#include <stdint.h>
#include <string.h>

#define AFL_LANES 64
#define AFL_HASH_LOG 12
#define AFL_TABLE_ENTRIES (1 << AFL_HASH_LOG)  /* x uint32 = 16 KiB */
#define AFL_MAX_DISTANCE 65535
#define AFL_MFLIMIT 12                         /* no match starts at n - 13 or later */
#define AFL_LASTLITERALS 5                     /* no match ends after n - 5 */
#define AFL_MAX_INPUT 0x7E000000               /* LZ4_MAX_INPUT_SIZE */

#if defined(__HIPCC__)
#define AFL_FN __device__ static inline
/* a per-lane value is a register; the lanes of a step run together */
#define AFL_VAR(type, name) type name
#define AFL_L(name) name
#define AFL_EACH_LANE
#define AFL_BALLOT(name) ((uint64_t)__builtin_amdgcn_ballot_w64((name) != 0))
#define AFL_LANE_VALUE(name, k) ((uint32_t)__builtin_amdgcn_readlane((int)(name), (k)))
#define AFL_TABLE_MAX(table, h, v) atomicMax(&(table)[h], (v))           /* LDS maximum: the same for every lane order */
#define AFL_CTZ64(m) __builtin_ctzll(m)
#define AFL_SYNC() __syncthreads()                                       /* one wave per workgroup: orders its LDS traffic, waits for nobody */
#define AFL_LOAD32(p) afl_load32(p)
AFL_FN uint32_t afl_load32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
#else
#define AFL_FN static inline
#define AFL_VAR(type, name) type name##_lanes[AFL_LANES]
#define AFL_L(name) name##_lanes[lane]
#define AFL_EACH_LANE for (lane = 0; lane < AFL_LANES; ++lane)
#define AFL_BALLOT(name) afl_ballot(name##_lanes)
#define AFL_LANE_VALUE(name, k) (name##_lanes[k])
#define AFL_TABLE_MAX(table, h, v) do { if ((table)[h] < (v)) (table)[h] = (v); } while (0)
#define AFL_CTZ64(m) __builtin_ctzll(m)
#define AFL_SYNC() ((void)0)
#define AFL_LOAD32(p) afl_load32(p)
AFL_FN uint32_t afl_load32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
AFL_FN uint64_t afl_ballot(const uint32_t* v) {
    uint64_t m = 0;
    for (int i = 0; i < AFL_LANES; ++i) m |= (uint64_t)(v[i] != 0) << i;
    return m;
}
#endif

/* bytes of one sequence: token, literal-length extension, literals, and (mlen >= 4) offset + match-length extension; mlen = 0: the last one */
AFL_FN int64_t afl_sequence_bytes(int32_t litlen, int32_t mlen) {
    int64_t s = 1 + (int64_t)litlen + (litlen >= 15 ? (litlen - 15) / 255 + 1 : 0);
    if (mlen) s += 2 + (mlen - 4 >= 15 ? (mlen - 19) / 255 + 1 : 0);
    return s;
}

/* a length field beyond its 4 token bits at dst: floor(v / 255) bytes of 255, then v % 255 -> bytes written */
AFL_FN int32_t afl_put_length(uint8_t* dst, int32_t v, int lane) {
    const int32_t full = v / 255;
    AFL_EACH_LANE {
        for (int32_t i = lane; i <= full; i += AFL_LANES) dst[i] = (uint8_t)(i < full ? 255 : v % 255);
    }
    return full + 1;
}

AFL_FN void afl_copy(uint8_t* dst, const uint8_t* src, int32_t n, int lane) {
    AFL_EACH_LANE {
        for (int32_t i = lane; i < n; i += AFL_LANES) dst[i] = src[i];
    }
}

/* One sequence at dst: litlen literals from lit, then (mlen >= 4) a match of mlen bytes at distance off; mlen = 0: the last one -> bytes */
AFL_FN int32_t afl_put_sequence(uint8_t* dst, const uint8_t* lit, int32_t litlen, int32_t off, int32_t mlen, int lane) {
    const int32_t ml = mlen ? mlen - 4 : 0;
    int32_t o = 1;
    AFL_EACH_LANE {
        if (lane == 0) dst[0] = (uint8_t)(((litlen < 15 ? litlen : 15) << 4) | (ml < 15 ? ml : 15));
    }
    if (litlen >= 15) o += afl_put_length(dst + o, litlen - 15, lane);
    afl_copy(dst + o, lit, litlen, lane);
    o += litlen;
    if (mlen) {
        AFL_EACH_LANE {
            if (lane < 2) dst[o + lane] = (uint8_t)(off >> (8 * lane));
        }
        o += 2;
        if (ml >= 15) o += afl_put_length(dst + o, ml - 15, lane);
    }
    return o;
}

/* src[0 .. n) -> dst[0 .. n) (the stream's slot); table: AFL_TABLE_ENTRIES x uint32 (LDS), the wave's own; store != 0: no search,
 * the stream is stored.  lane: the calling lane (kernel) / unused (host).  -> csize: < n, or n = stored. */
AFL_FN int32_t afl_encode_wave(const uint8_t* src, int32_t n, uint8_t* dst, uint32_t* table, int store, int lane) {
    const int32_t cap = n - 1;
    int32_t ip = 0, anchor = 0, op = 0;
    int fits = !store && n > AFL_MFLIMIT && n <= AFL_MAX_INPUT;
    if (fits) {
        AFL_EACH_LANE {
            for (int32_t i = lane; i < AFL_TABLE_ENTRIES; i += AFL_LANES) table[i] = 0;
        }
    }
    AFL_SYNC();
    const int32_t search_end = n - AFL_MFLIMIT - 1;            /* the last position a match may start at */
    while (fits && ip <= search_end) {
        AFL_VAR(uint32_t, w);
        AFL_VAR(uint32_t, h);
        AFL_VAR(uint32_t, cand);
        AFL_VAR(uint32_t, dist);                                /* the lane's match: its distance, 0 = none */
        AFL_EACH_LANE {                                         /* 1: word, hash, table entry — every lane reads ... */
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
        AFL_EACH_LANE {                                         /* 2: a verified match per lane */
            const int32_t pos = ip + lane;
            uint32_t d = 0;
            if (pos <= search_end) {
                if (pos >= 1 && AFL_LOAD32(src + pos - 1) == AFL_L(w)) d = 1;
                else if (pos >= 2 && AFL_LOAD32(src + pos - 2) == AFL_L(w)) d = 2;
                else if (pos >= 4 && AFL_LOAD32(src + pos - 4) == AFL_L(w)) d = 4;
                else if (AFL_L(cand)) {
                    const int32_t c = (int32_t)AFL_L(cand) - 1;
                    if (c < pos && pos - c <= AFL_MAX_DISTANCE && AFL_LOAD32(src + c) == AFL_L(w)) d = (uint32_t)(pos - c);
                }
            }
            AFL_L(dist) = d;
        }
        const uint64_t found = AFL_BALLOT(dist);                /* 3: the first lane with a match */
        const int fm = found ? AFL_CTZ64(found) : AFL_LANES - 1;
        AFL_SYNC();
        AFL_EACH_LANE {                                         /* ... before any lane inserts */
            const int32_t pos = ip + lane;
            if (pos <= search_end && lane <= fm) AFL_TABLE_MAX(table, AFL_L(h), (uint32_t)pos + 1);
        }
        AFL_SYNC();
        if (!found) {                                           /* 4: the round stays literals */
            ip += AFL_LANES;
            continue;
        }
        const int32_t mpos = ip + fm;
        const int32_t off = (int32_t)AFL_LANE_VALUE(dist, fm);
        const int32_t max_len = n - AFL_LASTLITERALS - mpos;    /* >= 8 */
        int32_t mlen = 4;
        while (mlen < max_len) {                                /* extension, 64 bytes a step */
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
        const int32_t litlen = mpos - anchor;
        if (op + afl_sequence_bytes(litlen, mlen) > cap) {
            fits = 0;
            break;
        }
        op += afl_put_sequence(dst + op, src + anchor, litlen, off, mlen, lane);
        ip = anchor = mpos + mlen;
    }
    if (fits && op + afl_sequence_bytes(n - anchor, 0) > cap) fits = 0;
    if (!fits) {
        afl_copy(dst, src, n, lane);
        return n;
    }
    op += afl_put_sequence(dst + op, src + anchor, n - anchor, 0, 0, lane);
    return op;
}

#endif
