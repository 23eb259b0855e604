/* zstd_encode_check.c — a program of its own around afcodec_zstd_encode_block_emulate (aggfly_amd/csrc/blosc1.c: the Zstandard block
 * encoder of zstd_encode_pass.h, its 64 lanes run in loops on the host), for the inputs of tests/zstd_encode_cases.py:
 * `make zstd_encode_check_san` (aggfly_amd/csrc/Makefile) writes them to a file, compiles this file with blosc1.c under the address and
 * undefined-behaviour sanitizers and runs it.  Every input and every slot is a heap buffer of exactly its size (n and n + 3 bytes), so
 * that a read or a write one byte outside is seen; every block is put behind a frame header, decoded again (afcodec_zstd_decode:
 * libzstd) and compared with its input.
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
    if (fread(b, 1, 4, f) != 4) { printf("zstd_encode_check: truncated file\n"); exit(2); }
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}

static void* take(size_t n) {
    void* p = malloc(n ? n : 1);
    if (!p) { printf("zstd_encode_check: out of memory\n"); exit(2); }
    return p;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: zstd_encode_check FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("zstd_encode_check: cannot open %s\n", argv[1]); return 2; }
    const uint32_t count = rd32(f);
    uint32_t failures = 0, types[3] = {0, 0, 0};
    int64_t raw = 0, packed = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t n = rd32(f);
        uint8_t* src = (uint8_t*)take(n);                    /* exactly the input, exactly the slot: no byte to spare */
        uint8_t* slot = (uint8_t*)take((size_t)n + 3);
        uint8_t* back = (uint8_t*)take(n);
        if (fread(src, 1, n, f) != n) { printf("zstd_encode_check: truncated file\n"); return 2; }
        const int64_t c = afcodec_zstd_encode_block_emulate(src, n, 1, slot, (int64_t)n + 3);
        int why = 0;
        if (c < 4 || c > (int64_t)n + 3) why = __LINE__;
        else {
            const uint32_t h = (uint32_t)slot[0] | ((uint32_t)slot[1] << 8) | ((uint32_t)slot[2] << 16);
            const uint32_t type = (h >> 1) & 3, size = h >> 3;
            uint8_t* frame = (uint8_t*)take((size_t)c + 9);
            const uint8_t head[9] = {0x28, 0xb5, 0x2f, 0xfd, 0xa0, (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)(n >> 16), (uint8_t)(n >> 24)};
            memcpy(frame, head, 9);
            memcpy(frame + 9, slot, (size_t)c);
            if (!(h & 1) || type > 2) why = __LINE__;
            else if (type == 1 ? (c != 4 || size != n) : size != c - 3) why = __LINE__;
            else if (type == 2 && size >= n) why = __LINE__;
            else if (afcodec_zstd_decode(frame, c + 9, back, n) != (int64_t)n) why = __LINE__;
            else if (memcmp(back, src, n)) why = __LINE__;
            else ++types[type];
            free(frame);
        }
        if (why && ++failures <= 20) printf("input %u (%u bytes -> %lld): refused at line %d\n", i, n, (long long)c, why);
        raw += n;
        packed += c < 0 ? 0 : c;
        free(src); free(slot); free(back);
    }
    fclose(f);
    printf("zstd_encode_check: %u inputs (%u raw, %u RLE, %u compressed blocks), %lld -> %lld bytes, %u failures\n", count, types[0], types[1],
           types[2], (long long)raw, (long long)packed, failures);
    return failures ? 1 : 0;
}
