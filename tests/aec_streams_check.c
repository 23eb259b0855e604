/* aec_streams_check.c — a program of its own around afcodec_aec_decode (aggfly_amd/csrc/blosc1.c: the passes of aec_passes.h run on the
 * host, the text the kernels of afhip_grib_unpack_ccsds run), for the streams `python tests/grib_ccsds_cases.py FILE` writes:
 * `make aec_streams_check_san` (aggfly_amd/csrc/Makefile) builds it with blosc1.c under the address and undefined-behaviour sanitizers
 * and runs it on the CPU.  Every stream is decoded out of a heap buffer of exactly its size into one of exactly n_values samples, so that
 * a read or write one byte outside them is seen.  libaec, where the loader finds it (dlopen; $AGGFLY_LIBAEC names a file), decodes the
 * same bytes.
 *
 * File: u32 n, then per stream u32 kind, u32 stream bytes, u32 n_values, u32 nbits, u32 flags, u32 block size, u32 rsi, the stream, and
 * for kind 0 the samples as u32.
 *   0 valid    decoded without an error to exactly these samples; libaec reads the same;
 *   2 mutated  (bits flipped, bytes replaced, truncated, extended) whatever comes out, nothing is touched outside the buffers, and where
 *              both this decoder and libaec accept the stream they read the same samples.
 */
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aggfly_codec.h"

struct aec_stream {
    const unsigned char* next_in;
    size_t avail_in, total_in;
    unsigned char* next_out;
    size_t avail_out, total_out;
    unsigned int bits_per_sample, block_size, rsi, flags;
    void* state;
};
typedef int (*aec_fn)(struct aec_stream*);

static int failures;

static void failf(uint32_t i, uint32_t kind, const char* what) {
    if (++failures <= 20) printf("stream %u (kind %u): %s\n", i, kind, what);
}

static uint32_t rd32(FILE* f) {
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { printf("aec_streams_check: truncated file\n"); exit(2); }
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}

static void* take(size_t n) {
    void* p = malloc(n ? n : 1);
    if (!p) { printf("aec_streams_check: out of memory\n"); exit(2); }
    return p;
}

static aec_fn find_libaec(void) {
    const char* names[] = {getenv("AGGFLY_LIBAEC"), "libaec.so.0", "libaec.so", "/opt/conda/lib/libaec.so.0", "/usr/local/lib/libaec.so.0"};
    for (size_t k = 0; k < sizeof names / sizeof names[0]; ++k) {
        void* h = names[k] ? dlopen(names[k], RTLD_NOW | RTLD_LOCAL) : NULL;
        if (h) {
            aec_fn fn = (aec_fn)dlsym(h, "aec_buffer_decode");
            if (fn) return fn;
        }
    }
    return NULL;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: aec_streams_check FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("aec_streams_check: cannot open %s\n", argv[1]); return 2; }
    const aec_fn libaec = find_libaec();
    const uint32_t n = rd32(f);
    uint32_t count[3] = {0, 0, 0}, clean = 0, both = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t kind = rd32(f), csz = rd32(f), nv = rd32(f), nbits = rd32(f), flags = rd32(f), J = rd32(f), rsi = rd32(f);
        if ((kind != 0 && kind != 2) || nbits < 1 || nbits > 32) { printf("aec_streams_check: bad file\n"); return 2; }
        count[kind]++;
        uint8_t* comp = (uint8_t*)take(csz);                     /* exactly the stream: no byte to spare on either side */
        uint32_t* want = kind == 0 ? (uint32_t*)take((size_t)nv * 4) : NULL;
        if (fread(comp, 1, csz, f) != csz) { printf("aec_streams_check: truncated file\n"); return 2; }
        for (uint32_t k = 0; want && k < nv; ++k) want[k] = rd32(f);
        uint32_t* out = (uint32_t*)take((size_t)nv * 4);
        memset(out, 0xC7, (size_t)nv * 4);
        const int rc = afcodec_aec_decode(comp, csz, nv, (int)nbits, (int)flags, (int)J, (int)rsi, out);
        /* libaec on the same bytes: samples of 1, 2 or 4 bytes, little-endian */
        const size_t bps = nbits <= 8 ? 1 : nbits <= 16 ? 2 : 4;
        uint8_t* lout = (uint8_t*)take(nv * bps);
        int lok = 0;
        if (libaec) {
            struct aec_stream s;
            memset(&s, 0, sizeof s);
            s.next_in = comp; s.avail_in = csz; s.next_out = lout; s.avail_out = nv * bps;
            s.bits_per_sample = nbits; s.block_size = J; s.rsi = rsi; s.flags = flags & 8u;
            lok = libaec(&s) == 0 && s.total_out == nv * bps;
        }
        int same = 1;
        for (uint32_t k = 0; lok && rc == 0 && k < nv; ++k) {
            const uint32_t v = bps == 1 ? lout[k] : bps == 2 ? (uint32_t)lout[2 * k] | ((uint32_t)lout[2 * k + 1] << 8)
                                                            : (uint32_t)lout[4 * k] | ((uint32_t)lout[4 * k + 1] << 8) | ((uint32_t)lout[4 * k + 2] << 16) | ((uint32_t)lout[4 * k + 3] << 24);
            if (v != out[k]) { same = 0; break; }
        }
        if (kind == 0) {
            if (rc != 0) failf(i, kind, "a valid stream was refused");
            else if (nv && memcmp(out, want, (size_t)nv * 4)) failf(i, kind, "decoded samples differ");
            if (libaec && !lok) failf(i, kind, "libaec does not read a stream of the catalogue");
        } else if (rc == 0) {
            clean++;
        }
        if (rc == 0 && lok) {
            both++;
            if (!same) failf(i, kind, "this decoder and libaec accept the stream and read other samples");
        }
        free(lout);
        free(out);
        free(want);
        free(comp);
    }
    fclose(f);
    printf("aec_streams_check: %u valid, %u mutated (%u decoded clean), %u read by both decoders, libaec %s\n", count[0], count[2], clean, both,
           libaec ? "loaded" : "not found");
    printf("aec_streams_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
