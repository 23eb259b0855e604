/* zstd_frames_check.c — a program of its own around afcodec_zstd_plan and afcodec_zstd_emulate (aggfly_amd/csrc/blosc1.c, the passes
 * of zstd_passes.h run on the host), for the frames of tests/zstd_frames.py: tests/test_zstd_frames.py writes them to a file, compiles
 * this file with blosc1.c and runs it; `make zstd_frames_check_san` (aggfly_amd/csrc/Makefile) does the same under the address and
 * undefined-behaviour sanitizers.  Every frame runs as a batch of its own out of buffers of exactly its size, so that a read or write
 * one byte outside them is seen.
 *
 * File: u32 n, then per frame u32 kind (0 valid: the expected bytes follow the frame; 1 damaged; 2 mutated), u32 frame bytes,
 * u32 Frame_Content_Size, the frame, and for kind 0 the decoded bytes.
 *   valid    the planner takes it, the emulation counts no error, rebuilds it bit for bit and leaves the canaries;
 *   damaged  the planner refuses it, or the emulation counts exactly one error and writes nothing outside the destination;
 *   mutated  whatever the planner says, no record leaves its buffers and the emulation writes nothing outside the destination.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aggfly_codec.h"
#include "zstd_passes.h"

#define GAP 48
#define CANARY 0xC7

static int failures;

static void failf(uint32_t i, uint32_t kind, const char* what) {
    if (++failures <= 20) printf("frame %u (kind %u): %s\n", i, kind, what);
}

static uint32_t rd32(FILE* f) {
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { printf("zstd_frames_check: truncated file\n"); exit(2); }
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}

static void* take(size_t n) {
    void* p = malloc(n ? n : 1);
    if (!p) { printf("zstd_frames_check: out of memory\n"); exit(2); }
    return p;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: zstd_frames_check FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { printf("zstd_frames_check: cannot open %s\n", argv[1]); return 2; }
    const uint32_t n = rd32(f);
    const int64_t cap_blocks = 4096;
    afz_block* blocks = (afz_block*)take(sizeof(afz_block) * (size_t)cap_blocks);
    uint32_t count[3] = {0, 0, 0}, planned = 0, refused_by_passes = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t kind = rd32(f), csz = rd32(f), fcs = rd32(f);
        if (kind > 2) { printf("zstd_frames_check: bad file\n"); return 2; }
        count[kind]++;
        uint8_t* comp = (uint8_t*)take(csz);                     /* exactly the frame: no byte to spare on either side */
        uint8_t* want = kind == 0 ? (uint8_t*)take(fcs) : NULL;
        if (fread(comp, 1, csz, f) != csz || (want && fread(want, 1, fcs, f) != fcs)) { printf("zstd_frames_check: truncated file\n"); return 2; }
        const int64_t comp_off = 0, comp_size = csz, out_off = GAP, out_size = fcs;
        int64_t nf = 0, nb = 0, lit = 0, nsq = 0, dec = 0, result = 0;
        afz_frame frame;
        afcodec_zstd_plan(comp, 1, &comp_off, &comp_size, &out_off, &out_size, &frame, 1, &nf, blocks, cap_blocks, &nb, &lit, &nsq, &dec, &result);
        if (result < 0) {
            if (nf || nb) failf(i, kind, "a refused frame left records");
            if (kind == 0) failf(i, kind, "the planner refused a valid frame");
        } else {
            planned++;
            if (result != (int64_t)fcs || nf != 1 || dec != (int64_t)fcs) failf(i, kind, "plan totals");
            for (int64_t b = 0; b < nb; ++b) {
                const afz_block* k = &blocks[b];
                if (k->src < 0 || k->csize < 0 || k->src + k->csize > (int64_t)csz || k->lit_size < 0 || k->lit_off < 0 ||
                    k->lit_off + k->lit_size > lit || k->seq_off < 0 || k->seq_off + k->nseq > nsq || k->nseq < 0)
                    failf(i, kind, "a block record leaves its buffers");
            }
            const int64_t sb = afcodec_zstd_scratch_bytes(nb, nf, lit, nsq, dec);
            uint8_t* scratch = (uint8_t*)take((size_t)sb);
            memset(scratch, 0x3C, (size_t)sb);
            const size_t nout = (size_t)fcs + 2 * GAP;
            uint8_t* out = (uint8_t*)take(nout);
            memset(out, CANARY, nout);
            int32_t errors = 0, rounds = 0;
            afcodec_zstd_emulate(comp, csz, &frame, nf, blocks, nb, lit, nsq, dec, scratch, out, &errors, &rounds);
            for (size_t j = 0; j < GAP; ++j)
                if (out[j] != CANARY || out[GAP + fcs + j] != CANARY) { failf(i, kind, "a canary was written"); break; }
            if (errors < 0 || errors > 1) failf(i, kind, "errors outside 0..1 for one frame");
            if (rounds > afz_rounds_host(dec)) failf(i, kind, "more pointer-jump rounds than afz_rounds_host");
            if (kind == 0) {
                if (errors) failf(i, kind, "the emulation marked a valid frame bad");
                else if (memcmp(out + GAP, want, fcs)) failf(i, kind, "decoded bytes differ");
            } else if (kind == 1) {
                if (errors != 1) failf(i, kind, "a damaged frame decoded without an error");
                refused_by_passes += errors == 1;
            }
            free(out);
            free(scratch);
        }
        free(want);
        free(comp);
    }
    fclose(f);
    free(blocks);
    printf("zstd_frames_check: %u valid, %u damaged (%u refused by the passes), %u mutated, %u planned\n", count[0], count[1], refused_by_passes,
           count[2], planned);
    printf("zstd_frames_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
