/* aggfly_codec.h — C ABI of libaggfly_codec.so: host-side chunk codecs of the ingestion path
 * (SURVEY.md §8f row N2).  Plain C, no GPU code; every function is re-entrant (OpenMP inside the
 * *_files / *_many calls only).
 *
 * Replaces, for this path, the numcodecs calls the reference makes inside its dask graph when a Zarr
 * store is opened (aggfly/dataset/dataset.py:697-728: zarr chunk decode per task;
 * benchmarks/bench_read_scheduler.py:4-8: GIL-limited to ~2 cores warm).
 *
 * Return values: >= 0 = bytes produced (decode / encode), or AFCODEC_OK for the batch calls;
 * < 0 = error code, text in afcodec_last_error() (thread-local).
 */
#ifndef AGGFLY_CODEC_H
#define AGGFLY_CODEC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define AFCODEC_OK 0
#define AFCODEC_E_FORMAT (-1)      /* not a well-formed container / truncated */
#define AFCODEC_E_UNSUPPORTED (-2) /* codec or library not available (snappy; liblz4 / libzstd missing) */
#define AFCODEC_E_SIZE (-3)        /* destination too small, sizes out of range, out of memory */
#define AFCODEC_E_CODEC (-4)       /* the inner codec failed */
#define AFCODEC_MISSING (-100)     /* results[i] of the *_files calls: the chunk file does not exist */

const char* afcodec_last_error(void);
int afcodec_have(int codec); /* Blosc codec ids: 0 blosclz, 1 lz4, 3 zlib, 4 zstd -> 1 if usable */

/* Blosc-1 container (format version 2; codecs blosclz / lz4 / lz4hc / zlib / zstd; byte- and bit-shuffle). */
int afcodec_blosc_info(const void* chunk, int64_t size, int64_t* nbytes, int64_t* blocksize, int32_t* typesize, int32_t* flags);
int64_t afcodec_blosc_decode(const void* chunk, int64_t csize, void* dst, int64_t dstsize);
/* the blocks of ONE (large) chunk spread over an OpenMP team */
int64_t afcodec_blosc_decode_mt(const void* chunk, int64_t csize, void* dst, int64_t dstsize, int nthreads);
int afcodec_blosc_decode_many(int64_t n, const void* const* chunks, const int64_t* csizes, void* const* dsts,
                              const int64_t* dstsizes, int nthreads, int64_t* results);
int afcodec_blosc_decode_files(int64_t n, const char* const* paths, void* const* dsts, const int64_t* dstsizes,
                               int nthreads, int64_t* results);
int64_t afcodec_blosc_bound(int64_t nbytes, int64_t blocksize);
int64_t afcodec_blosc_encode_lz4(const void* src, int64_t nbytes, int typesize, int shuffle, int64_t blocksize,
                                 void* dst, int64_t cap);
/* Blosc-1 writer: cname 1 (LZ4) or 4 (Zstandard, the system's libzstd at `level`; LZ4 ignores the level); shuffle 0 none, 1 byte,
 * 2 bit (a block whose element count is not a multiple of 8 stays unshuffled, as in c-blosc); blocksize 0 = 64 KiB x typesize for
 * LZ4, 256 KiB for Zstandard.  Zstandard blocks are unsplit (flag 0x10), one frame per block, as c-blosc 1.21 writes them; LZ4
 * blocks under a shuffle are split into typesize streams.  afcodec_blosc_encode_lz4(..., shuffle, ...) is cname 1, level 0. */
int64_t afcodec_blosc_encode(const void* src, int64_t nbytes, int typesize, int shuffle, int cname, int level, int64_t blocksize,
                             void* dst, int64_t cap);

/* The write side in HBM (libaggfly_hip: afhip_take_box, afhip_shuffle_blocks, afhip_lz4_encode_streams, afhip_copy_ranges).
 * afcodec_lz4_encode_emulate: the LZ4 block encoder of aggfly_amd/csrc/lz4_encode_pass.h exactly as the kernel runs it, its 64 lanes
 * in loops: src[0 .. n) into dst (cap >= n) -> the stream's size: an LZ4 block of at most n - 1 bytes, or n with the raw bytes in dst
 * (stored).  The bytes are a function of the input alone, so the kernel's output is byte-identical.
 * afcodec_blosc_encode_plan: the geometry of n chunks of nbytes bytes each (chunk i = bytes [i * nbytes, (i + 1) * nbytes) of the
 * chunk buffer) as afcodec_blosc_encode lays out LZ4 chunks under the byte shuffle with the automatic block size — one function
 * computes the block size for both — into
 *   blocks  [*n_blocks]   afhip_shuffle_block records for afhip_shuffle_blocks (out_off: the block in the chunk buffer, tmp_off: in the
 *                         shuffle scratch, the same offset; typesize 1 where nothing is shuffled);
 *   streams [*n_streams]  afhip_lz4_stream records for afhip_lz4_encode_streams, chunk by chunk, block by block, plane by plane:
 *                         src_off = dst_off = the stream's offset in the scratch and of its slot, dsize its raw length, pad its block,
 *                         to_out = 1 for the single stored stream of a chunk under 128 bytes;
 *   layout [5]            of every chunk's container: the header's blocksize field, the entries of its bstarts table, its streams,
 *                         its flags byte, the bytes of the length field in front of every stream (4; 0 in a stored chunk).
 * With streams and blocks both NULL only the counts and the layout are returned.  Nothing is encoded here. */
int64_t afcodec_lz4_encode_emulate(const void* src, int64_t n, void* dst, int64_t cap);
/* The same for Zstandard streams (afhip_zstd_encode_blocks).
 * afcodec_zstd_encode_block_emulate: the block encoder of aggfly_amd/csrc/zstd_encode_pass.h exactly as the kernel runs it: src[0 .. n),
 * 1 <= n <= 131072, into dst (cap >= n + 3) -> the bytes of one complete Zstandard block with its header (last: the Last_Block bit).
 * afcodec_zstd_encode_scratch_bytes: afhip_zstd_encode_scratch_bytes.
 * afcodec_blosc_zstd_encode_plan: afcodec_blosc_encode_plan for the chunks afcodec_blosc_encode writes with cname 4 under the byte
 * shuffle — unsplit 256 KiB blocks (flag 0x10), one frame per block behind its int32 length — with afhip_zstd_encode_block records in
 * place of the stream records: a frame is cut at the byte planes of its shuffled block when a plane holds at most 128 KiB, else into
 * 128 KiB pieces, each piece one block of the frame (`last` on its last); src_off in the shuffled input, dst_off in the slots (n + 3
 * bytes each, in order), scratch_off in the encoder's scratch.  layout [8]: the five of afcodec_blosc_encode_plan (streams = Zstandard
 * blocks per chunk), then the offset of the slots in a work buffer that starts with the shuffled input, the bytes of the slots, the
 * bytes of the scratch. */
int64_t afcodec_zstd_encode_block_emulate(const void* src, int64_t n, int last, void* dst, int64_t cap);
int64_t afcodec_zstd_encode_scratch_bytes(int64_t n);
int afcodec_blosc_zstd_encode_plan(int64_t n, int64_t nbytes, int typesize, void* zblocks, int64_t cap_zblocks, int64_t* n_zblocks,
                                   void* blocks, int64_t cap_blocks, int64_t* n_blocks, int64_t* layout);
int afcodec_blosc_encode_plan(int64_t n, int64_t nbytes, int typesize, void* streams, int64_t cap_streams, int64_t* n_streams,
                              void* blocks, int64_t cap_blocks, int64_t* n_blocks, int64_t* layout);

/* Plan of a GPU-side decode (libaggfly_hip: afhip_lz4_decode_streams / afhip_unshuffle_blocks, include/aggfly_hip.h): the
 * containers of n Blosc-1 chunks — chunk i = comp_size[i] bytes at base + comp_off[i], its decoded bytes wanted at offset
 * out_off[i] (capacity out_size[i]) of the output buffer — are parsed on the host and turned into
 *   streams [*n_streams]  afhip_lz4_stream records: every LZ4 stream (a block, or one byte plane of a split block) with its
 *                         offset in the compressed bytes (relative to base: the device copy keeps the same offsets) and
 *                         its destination (the output, or the shuffled scratch of *tmp_bytes bytes); stored streams and
 *                         stored chunks appear with csize == dsize;
 *   blocks  [*n_blocks]   afhip_shuffle_block records: blocks whose byte shuffle is undone from the scratch into the output.
 * Nothing is decoded here.  results[i] = the chunk's decoded size, or < 0: AFCODEC_E_UNSUPPORTED marks a chunk the GPU
 * route does not take (another codec than LZ4, bit shuffle: afcodec_blosc_plan below takes more) — decode it on the host; the call
 * then returns that code too.
 * *max_dsize = the longest stream (sizes the kernel's LDS ring). */
int afcodec_blosc_lz4_plan(const void* base, int64_t n, const int64_t* comp_off, const int64_t* comp_size, const int64_t* out_off,
                           const int64_t* out_size, void* streams, int64_t cap_streams, int64_t* n_streams, void* blocks,
                           int64_t cap_blocks, int64_t* n_blocks, int64_t* tmp_bytes, int32_t* max_dsize, int64_t* results);

/* The same walk for every Blosc-1 chunk the GPU decodes (afcodec_blosc_lz4_plan is this walk with Zstandard and bit shuffle filtered
 * out): inner codec LZ4 / LZ4HC or Zstandard, shuffle none, byte or bit.  Five outputs:
 *   streams [*n_streams]  afhip_lz4_stream records: every LZ4 stream, and every plain copy (stored streams, csize == dsize — those
 *                         of Zstandard chunks cut into pieces of at most 64 KiB — and stored chunks, flag 0x02);
 *   frames  [*n_frames] / zblocks [*n_zblocks]  afhip_zstd_frame / afhip_zstd_block records of every Zstandard stream, by the
 *                         per-frame walk of afcodec_zstd_plan, with the batch totals *lit_bytes, *n_seqs, *dec_bytes; their
 *                         dst_off are offsets into the shuffle scratch: call afhip_zstd_decode with out_dev = the scratch;
 *   blocks  [*n_blocks]   afhip_shuffle_block records for afhip_unshuffle_blocks: byte-shuffled blocks, and the unshuffled blocks
 *                         of Zstandard chunks as typesize 1 (a copy scratch -> output);
 *   bits    [*n_bits]     afhip_shuffle_block records for afhip_bitunshuffle_blocks: bit-shuffled blocks;
 *   *tmp_bytes of shuffle scratch, *max_dsize (the longest LZ4 stream) and results[i] = the chunk's nbytes, or < 0:
 *   AFCODEC_E_UNSUPPORTED for blosclz / zlib / snappy inner codecs and for an inner frame afcodec_zstd_plan would refuse — decode the
 *   chunk on the host —, AFCODEC_E_FORMAT for malformed containers.  A chunk that fails leaves no record.
 * Every Zstandard frame and every stream of a shuffled block decodes into the scratch and the block then moves scratch -> output
 * through one of the two unshuffle lists; unshuffled LZ4 streams go straight to the output.  Run, in order, afhip_lz4_decode_streams,
 * afhip_zstd_decode (out_dev = scratch), afhip_unshuffle_blocks, afhip_bitunshuffle_blocks.  Every record lies inside its chunk,
 * the batch's buffers and the chunk's destination, whatever the input bytes are.  Nothing is decoded here. */
int afcodec_blosc_plan(const void* base, int64_t n, const int64_t* comp_off, const int64_t* comp_size, const int64_t* out_off,
                       const int64_t* out_size, void* streams, int64_t cap_streams, int64_t* n_streams, void* blocks,
                       int64_t cap_blocks, int64_t* n_blocks, void* bits, int64_t cap_bits, int64_t* n_bits, void* frames,
                       int64_t cap_frames, int64_t* n_frames, void* zblocks, int64_t cap_zblocks, int64_t* n_zblocks, int64_t* lit_bytes,
                       int64_t* n_seqs, int64_t* dec_bytes, int64_t* tmp_bytes, int32_t* max_dsize, int64_t* results);

/* Plan of a GPU-side Zstandard decode (libaggfly_hip: afhip_zstd_decode, include/aggfly_hip.h): n plain Zstandard frames —
 * chunk i = comp_size[i] bytes at base + comp_off[i], decoded to offset out_off[i] of the output (out_size[i] bytes) — have
 * their frame, block, literals and sequences headers walked on the host (FSE table descriptions only as far as their sizes)
 * into one afhip_zstd_frame record per frame and one afhip_zstd_block record per block: offsets of the literals, of the
 * Huffman description and of the sequences bitstream, literal type and sizes, stream count, number of sequences, the LL / OF
 * / ML modes with Repeat_Mode and treeless literals resolved to the block whose table is meant, and each block's place in the
 * batch's literal and sequence buffers (*lit_bytes bytes, *n_seqs sequences; *dec_bytes = all frames' decoded bytes).
 * results[i] = the frame's decoded size, or < 0: AFCODEC_E_UNSUPPORTED marks a frame the GPU route does not take (content
 * checksum, dictionary, no Frame_Content_Size or one other than out_size[i], skippable frame, more than one frame) — decode
 * it on the host; malformed frames give AFCODEC_E_FORMAT and no record.  Every record lies inside its chunk, the batch's
 * buffers and the frame's destination.  Nothing is decoded here. */
int afcodec_zstd_plan(const void* base, int64_t n, const int64_t* comp_off, const int64_t* comp_size, const int64_t* out_off,
                      const int64_t* out_size, void* frames, int64_t cap_frames, int64_t* n_frames, void* blocks, int64_t cap_blocks,
                      int64_t* n_blocks, int64_t* lit_bytes, int64_t* n_seqs, int64_t* dec_bytes, int64_t* results);
/* Scratch of one batch (== afhip_zstd_scratch_bytes). */
int64_t afcodec_zstd_scratch_bytes(int64_t n_blocks, int64_t n_frames, int64_t lit_bytes, int64_t n_seqs, int64_t dec_bytes);
/* The passes of afhip_zstd_decode run in order on the calling thread (host reference of the GPU algorithm, for tests): the
 * same arguments with host pointers; *errors = damaged frames, *rounds = pointer-jump rounds that had work. */
int afcodec_zstd_emulate(const void* comp, int64_t comp_bytes, const void* frames, int64_t n_frames, const void* blocks,
                         int64_t n_blocks, int64_t lit_bytes, int64_t n_seqs, int64_t dec_bytes, void* scratch, void* out,
                         int32_t* errors, int32_t* rounds);

/* Plan of a GPU-side zlib decode (libaggfly_hip: afhip_inflate_decode, include/aggfly_hip.h): n chunks that are one zlib stream
 * each — chunk i = comp_size[i] bytes at base + comp_off[i], decoded to offset out_off[i] of the output (out_size[i] bytes),
 * byte-unshuffled there when typesize[i] > 1 (HDF5's shuffle filter before deflate; typesize NULL: no chunk is) — have their two header bytes checked (CM, CINFO,
 * the FCHECK sum) into one afhip_inflate_stream record per chunk: the source range, the destination (the output, or the shuffle
 * scratch with one afhip_shuffle_block record: bsize = the chunk, typesize[i]), the expected size, and the stream's place in the
 * batch's buffers (*n_pblocks pseudo-block slots, *n_seqs sequence records, *n_pieces Adler-32 pieces, *dec_bytes decoded bytes,
 * *tmp_bytes of shuffle scratch).  results[i] = out_size[i], or < 0: AFCODEC_E_UNSUPPORTED marks a chunk the GPU route does not
 * take (a preset dictionary — FDICT —, a gzip member, 1 GiB or more) — decode it on the host; other header bytes give
 * AFCODEC_E_FORMAT; neither leaves a record.  Every record lies inside its chunk, the batch's buffers and the destination.
 * Nothing is decoded here. */
int afcodec_inflate_plan(const void* base, int64_t n, const int64_t* comp_off, const int64_t* comp_size, const int64_t* out_off,
                         const int64_t* out_size, const int32_t* typesize, void* streams, int64_t cap_streams, int64_t* n_streams, void* shuf,
                         int64_t cap_shuf, int64_t* n_shuf, int64_t* n_pblocks, int64_t* n_seqs, int64_t* n_pieces, int64_t* dec_bytes,
                         int64_t* tmp_bytes, int64_t* results);
/* Scratch of one batch (== afhip_inflate_scratch_bytes). */
int64_t afcodec_inflate_scratch_bytes(int64_t n_streams, int64_t n_pblocks, int64_t n_seqs, int64_t n_pieces, int64_t dec_bytes,
                                      int64_t tmp_bytes);
/* The passes of afhip_inflate_decode run in order on the calling thread (host reference of the GPU algorithm, for tests): the
 * same arguments with host pointers; *errors = damaged streams, *rounds = pointer-jump rounds that had work. */
int afcodec_inflate_emulate(const void* comp, int64_t comp_bytes, const void* streams, int64_t n_streams, const void* shuf,
                            int64_t n_shuf, int64_t n_pblocks, int64_t n_seqs, int64_t n_pieces, int64_t dec_bytes, int64_t tmp_bytes,
                            void* scratch, void* out, int32_t* errors, int32_t* rounds);

/* Chunk files of one codec kind (0 raw, 1 Blosc-1, 2 Zstandard frame, 3 zlib or gzip stream, 4 numcodecs LZ4;
 * kind + 16 * element_size adds a byte-unshuffle after the codec: HDF5 / netCDF-4 shuffle + deflate chunks): read and
 * decoded paths[i] -> dsts[i], one chunk per OpenMP thread. */
int afcodec_decode_files(int kind, int64_t n, const char* const* paths, void* const* dsts, const int64_t* dstsizes,
                         int nthreads, int64_t* results);

/* The same for byte ranges [offsets[i], offsets[i] + lengths[i]) of the files (inner chunks of Zarr v3
 * shards); lengths[i] < 0 or offsets == NULL = the whole file. */
int afcodec_decode_ranges(int kind, int64_t n, const char* const* paths, const int64_t* offsets, const int64_t* lengths,
                          void* const* dsts, const int64_t* dstsizes, int nthreads, int64_t* results);

/* Byte ranges of files packed back to back into one buffer (what the decode-in-HBM route uploads): range i lands at
 * dst + out_off[i] (out_off has n + 1 entries, steps rounded up to `align`); results[i] = its size, -100 = missing file.
 * Sizes are taken from the files here; lengths[i] < 0 or offsets == NULL = the whole file. */
int afcodec_read_packed(int64_t n, const char* const* paths, const int64_t* offsets, const int64_t* lengths, void* dst, int64_t cap,
                        int64_t align, int nthreads, int64_t* out_off, int64_t* results);

/* TIFF LZW segments (strips or tiles) read and decoded on an OpenMP team, mirroring afcodec_decode_ranges: the stream in
 * [offsets[i], offsets[i] + lengths[i]) of paths[i] -> dsts[i], which it must fill exactly (dstsizes[i] bytes: a stream ends at
 * EndOfInformation or at that size).  results[i] = dstsizes[i], or a negative code for a range beyond the file or a damaged stream (a
 * code above the next free one, no literal after Clear, a span beyond the size, a stream that ends early).  The text of
 * aggfly_amd/csrc/lzw_passes.h, which afhip_lzw_decode runs on the GPU. */
int afcodec_lzw_decode_ranges(int64_t n, const char* const* paths, const int64_t* offsets, const int64_t* lengths,
                              void* const* dsts, const int64_t* dstsizes, int nthreads, int64_t* results);

/* numcodecs' LZ4 codec (Zarr v2 compressor id "lz4"): int32 decoded size + one raw LZ4 block. */
int64_t afcodec_lz4_decode(const void* src, int64_t n, void* dst, int64_t cap);

/* Plain Zstandard frames (Zarr compressor / codec "zstd"). */
int64_t afcodec_zstd_decode(const void* src, int64_t n, void* dst, int64_t cap);
int64_t afcodec_zstd_bound(int64_t n);
int64_t afcodec_zstd_encode(const void* src, int64_t n, int level, void* dst, int64_t cap);

/* One CCSDS 121.0-B (AEC) stream as libaec writes it — the body of section 7 of a GRIB2 message in data representation template
 * 5.42 — of n_values samples of nbits bits (0..32) -> out[n_values].  flags: 8 = the preprocessor; 2 and 4 are ignored, any other is
 * refused, as are block sizes other than 8 / 16 / 32 / 64 and rsi outside 1..4096.  The passes of aec_passes.h (what
 * afhip_grib_unpack_ccsds runs on the GPU) in loops on the calling thread. */
int afcodec_aec_decode(const void* src, int64_t n, int64_t n_values, int nbits, int flags, int block_size, int rsi, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif
