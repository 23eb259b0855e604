/* lz4_encode_check.c — a program of its own around afcodec_lz4_encode_emulate (aggfly_amd/csrc/blosc1.c: the LZ4 block encoder of
 * lz4_encode_pass.h, its 64 lanes run in loops on the host), for the inputs of tests/lz4_encode_cases.py: `make lz4_encode_check_san`
 * (aggfly_amd/csrc/Makefile) writes them to a file, compiles this file with blosc1.c under the address and undefined-behaviour
 * sanitizers and runs it.  Every input and every slot is a heap buffer of exactly its size, so that a read or a write one byte outside
 * is seen; every stream is decoded again by the strict decoder below and compared with its input.
 *
 * File: u32 count, then per input u32 length and the bytes.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aggfly_codec.h"

static uint32_t rd32(FILE* f) {
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { printf("lz4_encode_check: truncated file\n"); exit(2); }
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}

static void* take(size_t n) {
    void* p = malloc(n ? n : 1);
    if (!p) { printf("lz4_encode_check: out of memory\n"); exit(2); }
    return p;
}

/* one LZ4 block s[0 .. n) -> out[0 .. want): 0, or the line that refused it.  Checks the end-of-block rules too. */
static int decode_strict(const uint8_t* s, int64_t n, uint8_t* out, int64_t want) {
    int64_t p = 0, o = 0, last_match_start = -1;
    if (n <= 0) return __LINE__;
    for (;;) {
        if (p >= n) return __LINE__;
        const int token = s[p++];
        int64_t L = token >> 4;
        if (L == 15) {
            int b;
            do { if (p >= n) return __LINE__; b = s[p++]; L += b; } while (b == 255);
        }
        if (p + L > n || o + L > want) return __LINE__;
        memcpy(out + o, s + p, (size_t)L);
        p += L;
        o += L;
        if (p == n) {
            if (o != want) return __LINE__;
            if (last_match_start >= 0 && (L < 5 || last_match_start > want - 12)) return __LINE__;
            return 0;
        }
        if (p + 2 > n) return __LINE__;
        const int64_t off = s[p] | (s[p + 1] << 8);
        p += 2;
        int64_t M = token & 15;
        if (M == 15) {
            int b;
            do { if (p >= n) return __LINE__; b = s[p++]; M += b; } while (b == 255);
        }
        M += 4;
        if (off == 0 || off > o || o + M > want) return __LINE__;
        last_match_start = o;
        for (int64_t i = 0; i < M; ++i, ++o) out[o] = out[o - off];
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: lz4_encode_check FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("lz4_encode_check: cannot open %s\n", argv[1]); return 2; }
    const uint32_t count = rd32(f);
    uint32_t failures = 0, stored = 0;
    int64_t raw = 0, packed = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t n = rd32(f);
        uint8_t* src = (uint8_t*)take(n);                    /* exactly the input, exactly the slot: no byte to spare */
        uint8_t* slot = (uint8_t*)take(n);
        uint8_t* back = (uint8_t*)take(n);
        if (fread(src, 1, n, f) != n) { printf("lz4_encode_check: truncated file\n"); return 2; }
        const int64_t c = afcodec_lz4_encode_emulate(src, n, slot, n);
        int why = 0;
        if (c < 0 || c > n) why = __LINE__;
        else if (c == n) { ++stored; if (n && memcmp(slot, src, n)) why = __LINE__; }
        else {
            why = decode_strict(slot, c, back, n);
            if (!why && memcmp(back, src, n)) why = __LINE__;
        }
        if (why && ++failures <= 20) printf("input %u (%u bytes -> %lld): refused at line %d\n", i, n, (long long)c, why);
        raw += n;
        packed += c < 0 ? 0 : c;
        free(src); free(slot); free(back);
    }
    fclose(f);
    printf("lz4_encode_check: %u inputs, %u stored, %lld -> %lld bytes, %u failures\n", count, stored, (long long)raw, (long long)packed, failures);
    return failures ? 1 : 0;
}
