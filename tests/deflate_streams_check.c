/* deflate_streams_check.c — a program of its own around afcodec_inflate_plan and afcodec_inflate_emulate (aggfly_amd/csrc/blosc1.c, the
 * passes of inflate_passes.h run on the host), for the streams of tests/deflate_streams.py: tests/test_deflate_streams.py writes them to a
 * file, compiles this file with blosc1.c and runs it; `make deflate_streams_check_san` (aggfly_amd/csrc/Makefile) does the same under the
 * address and undefined-behaviour sanitizers.  Every stream runs as a batch of its own out of buffers of exactly its size, so that a read
 * or write one byte outside them is seen.
 *
 * File: u32 n, then per stream u32 kind, u32 stream bytes, u32 planned size, the stream, and for kind 0 the decoded bytes.
 *   0 valid    the planner takes it, the emulation counts no error, rebuilds it bit for bit and leaves the canaries;
 *   1 damaged  the planner takes it (it reads two bytes), the emulation counts exactly one error and writes nothing outside the
 *              destination; zlib refuses it too;
 *   2 mutated  whatever the planner says, no record leaves its buffers and the emulation writes nothing outside the destination; what
 *              it decodes without an error is what zlib decodes from the same bytes;
 *   3 valid, planned one byte off: exactly one error, although zlib decodes it.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include "aggfly_codec.h"
#include "inflate_passes.h"

#define GAP 48
#define CANARY 0xC7

static int failures;

static void failf(uint32_t i, uint32_t kind, const char* what) {
    if (++failures <= 20) printf("stream %u (kind %u): %s\n", i, kind, what);
}

static uint32_t rd32(FILE* f) {
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { printf("deflate_streams_check: truncated file\n"); exit(2); }
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}

static void* take(size_t n) {
    void* p = malloc(n ? n : 1);
    if (!p) { printf("deflate_streams_check: out of memory\n"); exit(2); }
    return p;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: deflate_streams_check FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("deflate_streams_check: cannot open %s\n", argv[1]); return 2; }
    const uint32_t n = rd32(f);
    uint32_t count[4] = {0, 0, 0, 0}, planned = 0, refused = 0, clean = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t kind = rd32(f), csz = rd32(f), dsz = rd32(f);
        if (kind > 3) { printf("deflate_streams_check: bad file\n"); return 2; }
        count[kind]++;
        uint8_t* comp = (uint8_t*)take(csz);                     /* exactly the stream: no byte to spare on either side */
        uint8_t* want = kind == 0 ? (uint8_t*)take(dsz) : NULL;
        if (fread(comp, 1, csz, f) != csz || (want && fread(want, 1, dsz, f) != dsz)) { printf("deflate_streams_check: truncated file\n"); return 2; }
        const int64_t comp_off = 0, comp_size = csz, out_off = GAP, out_size = dsz;
        int64_t ns = 0, nsh = 0, nb = 0, nsq = 0, np = 0, dec = 0, tmp = 0, result = 0;
        afi_stream st;
        struct { int64_t tmp_off, out_off; int32_t bsize, typesize; } shuf;
        afcodec_inflate_plan(comp, 1, &comp_off, &comp_size, &out_off, &out_size, NULL, &st, 1, &ns, &shuf, 1, &nsh, &nb, &nsq, &np, &dec, &tmp, &result);
        if (result < 0) {
            if (ns || nb) failf(i, kind, "a refused stream left a record");
            if (kind != 2) failf(i, kind, "the planner refused a stream whose header is intact");
        } else {
            planned++;
            if (result != (int64_t)dsz || ns != 1 || nsh != 0 || dec != (int64_t)dsz || tmp != 0) failf(i, kind, "plan totals");
            if (st.src != 0 || st.csize != (int32_t)csz || st.dsize != (int32_t)dsz || st.base != 0 || st.seq_off != 0 || st.first_block != 0 ||
                st.first_piece != 0 || !st.to_out || st.dst_off != GAP || st.n_blocks != nb || nb != (int64_t)dsz / AFI_PBLOCK_MIN + 1 ||
                nsq != (int64_t)dsz / 3 + 1 || np != ((int64_t)dsz + AFI_PIECE - 1) / AFI_PIECE)
                failf(i, kind, "the stream record leaves its buffers");
            const int64_t sb = afcodec_inflate_scratch_bytes(ns, nb, nsq, np, dec, tmp);
            uint8_t* scratch = (uint8_t*)take((size_t)sb);
            memset(scratch, 0x3C, (size_t)sb);
            const size_t nout = (size_t)dsz + 2 * GAP;
            uint8_t* out = (uint8_t*)take(nout);
            memset(out, CANARY, nout);
            int32_t errors = 0, rounds = 0;
            afcodec_inflate_emulate(comp, csz, &st, ns, &shuf, nsh, nb, nsq, np, dec, tmp, scratch, out, &errors, &rounds);
            for (size_t j = 0; j < GAP; ++j)
                if (out[j] != CANARY || out[GAP + dsz + j] != CANARY) { failf(i, kind, "a canary was written"); break; }
            if (errors < 0 || errors > 1) failf(i, kind, "errors outside 0..1 for one stream");
            if (rounds > afz_rounds_host(dec)) failf(i, kind, "more pointer-jump rounds than afz_rounds_host");
            int64_t o[9];
            afi_layout(ns, nb, nsq, np, dec, tmp, o);
            const afi_pblock* pb = (const afi_pblock*)(const void*)(scratch + o[3]);
            for (int64_t b = 0; b < nb && !errors; ++b)
                if (pb[b].dsize < 0 || pb[b].dsize > AFZ_BLOCK_MAX || pb[b].out_pos < 0 || pb[b].out_pos + pb[b].dsize > dec || pb[b].nseq < 0 ||
                    pb[b].seq_off + pb[b].nseq > nsq || pb[b].lit_size < 0 || pb[b].lit_off + pb[b].lit_size > dec) {
                    failf(i, kind, "a pseudo-block record leaves its buffers or AFZ_BLOCK_MAX");
                    break;
                }
            /* zlib on the same bytes, into a buffer of one byte more than planned */
            uLongf zn = (uLongf)dsz + 1;
            uint8_t* zout = (uint8_t*)take((size_t)dsz + 1);
            const int zrc = uncompress(zout, &zn, comp, csz);
            if (kind == 0) {
                if (errors) failf(i, kind, "the emulation marked a valid stream bad");
                else if (memcmp(out + GAP, want, dsz)) failf(i, kind, "decoded bytes differ");
                if (zrc != Z_OK || zn != dsz || memcmp(zout, want, dsz)) failf(i, kind, "zlib reads other bytes than the description means");
            } else if (kind == 1 || kind == 3) {
                if (errors != 1) failf(i, kind, "a damaged stream decoded without an error");
                refused += errors == 1;
                if (kind == 1 && zrc == Z_OK) failf(i, kind, "zlib decodes a stream of the damaged set");
                if (kind == 3 && (zrc != Z_OK || (zn != dsz + 1 && zn + 1 != dsz))) failf(i, kind, "not a valid stream one byte off its planned size");
            } else if (!errors) {
                clean++;
                if (zrc != Z_OK || zn != dsz || memcmp(out + GAP, zout, dsz)) failf(i, kind, "decoded without an error what zlib does not decode to these bytes");
            }
            free(zout);
            free(out);
            free(scratch);
        }
        free(want);
        free(comp);
    }
    fclose(f);
    printf("deflate_streams_check: %u valid, %u damaged and %u planned one byte off (%u refused by the passes), %u mutated (%u decoded clean), %u planned\n",
           count[0], count[1], count[3], refused, count[2], clean, planned);
    printf("deflate_streams_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
