/* lzw_streams_check.c — a program of its own around afcodec_lzw_decode_ranges (aggfly_amd/csrc/blosc1.c: the text of lzw_passes.h run on the
 * host, the text the kernel of afhip_lzw_decode runs), for the streams `python tests/tiff_cases.py FILE` writes:
 * `make lzw_streams_check_san` (aggfly_amd/csrc/Makefile) builds it with blosc1.c under the address and undefined-behaviour sanitizers
 * and runs it on the CPU.  Every stream is read as a byte range of FILE into a heap buffer of exactly its size (inside the entry) and
 * decoded into a heap buffer of exactly its decoded size, so that a read or write one byte outside them is seen.
 *
 * File: records until its end — i32 kind, i32 stream bytes, i32 decoded bytes, the stream, and for kind 0 the decoded bytes.
 *   0 good     decoded without an error to exactly these bytes;
 *   1 damaged  refused;
 *   2 mutated  (bits flipped, bytes replaced, truncated, extended, decoded size off by a few) whatever comes out, nothing is touched
 *              outside the buffers.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aggfly_codec.h"

static int failures;

static void failf(long i, int kind, const char* what) {
    if (++failures <= 20) printf("stream %ld (kind %d): %s\n", i, kind, what);
}

static void* take(size_t n) {
    void* p = malloc(n ? n : 1);
    if (!p) { printf("lzw_streams_check: out of memory\n"); exit(2); }
    return p;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: lzw_streams_check FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("lzw_streams_check: cannot open %s\n", argv[1]); return 2; }
    long count[3] = {0, 0, 0}, clean = 0, i = 0;
    int32_t head[3];
    while (fread(head, 4, 3, f) == 3) {
        const int kind = head[0];
        const int64_t csz = head[1], dsz = head[2];
        if (kind < 0 || kind > 2 || csz < 0 || dsz < 0) { printf("lzw_streams_check: bad file\n"); return 2; }
        count[kind]++;
        const int64_t at = ftell(f);
        if (fseek(f, (long)csz, SEEK_CUR) != 0) { printf("lzw_streams_check: truncated file\n"); return 2; }
        uint8_t* want = kind == 0 ? (uint8_t*)take((size_t)dsz) : NULL;
        if (want && fread(want, 1, (size_t)dsz, f) != (size_t)dsz) { printf("lzw_streams_check: truncated file\n"); return 2; }
        uint8_t* out = (uint8_t*)take((size_t)dsz);                 /* exactly the decoded size: no byte to spare on either side */
        memset(out, 0xC7, (size_t)dsz);
        const char* path = argv[1];
        void* dst = out;
        int64_t res = 0;
        const int rc = afcodec_lzw_decode_ranges(1, &path, &at, &csz, &dst, &dsz, 1, &res);
        if (kind == 0) {
            if (rc != 0 || res != dsz) failf(i, kind, "a good stream was refused");
            else if (dsz && memcmp(out, want, (size_t)dsz)) failf(i, kind, "decoded bytes differ");
        } else if (kind == 1) {
            if (rc == 0) failf(i, kind, "a damaged stream was accepted");
        } else if (rc == 0) {
            clean++;
        }
        if ((rc == 0) != (res == dsz && res >= 0)) failf(i, kind, "the return code and the result disagree");
        free(out);
        free(want);
        ++i;
    }
    fclose(f);
    printf("lzw_streams_check: %ld good, %ld damaged, %ld mutated (%ld decoded clean)\n", count[0], count[1], count[2], clean);
    printf("lzw_streams_check: %d failures\n", failures);
    return failures || !count[0] || !count[2] ? 1 : 0;
}
