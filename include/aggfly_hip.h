/* aggfly_hip.h — C ABI of the MI355X (gfx950) engine for aggfly's aggregate_dataset() hot path.
 *
 * The reference (dylanhogan/aggfly v0.2.0) is pure Python; it has no FFI layer.  The
 * seams this library sits behind are its numba kernels and numpy block functions, which
 * are already C-shaped: contiguous arrays in, caller-owned output, no exceptions
 * (SURVEY.md §8b).  Each entry point below names the reference interface it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types cross this boundary;
 *   - `*_dev` pointers are device (HBM) addresses owned by the caller; tables marked
 *     HOST are read on the host during the call and may be freed afterwards; an entry reads no byte of a scratch, a workspace, a
 *     `tmp` or a slots buffer that it has not written in the same call: their previous content is not an input;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is
 *     enqueued on it and the call returns without synchronising unless stated;
 *   - cubes are time-major: element (k, cell) at cube[k * n_cells + cell], cell =
 *     iy * NX + ix, exactly the (time, y, x) block the reference hands its kernels
 *     (aggfly/aggregate/nb_kernels.py:280);
 *   - every function returns 0 on success or a negative AFHIP_E_* code;
 *     afhip_last_error() gives the message for the calling thread.  Like the numba
 *     kernels, the GPU kernels themselves never raise: argument errors are reported
 *     before anything is launched.
 */
#ifndef AGGFLY_HIP_H
#define AGGFLY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AFHIP_ABI_VERSION 4

/* status codes */
#define AFHIP_OK            0
#define AFHIP_E_INVALID    -1   /* bad argument (the Python host raises ValueError)      */
#define AFHIP_E_HIP        -2   /* a HIP runtime call failed                              */
#define AFHIP_E_UNSUPPORTED -3  /* valid plan the fused kernels cannot express            */
#define AFHIP_E_NOMEM      -4

/* element type of a climate cube */
#define AFHIP_F32 0
#define AFHIP_F64 1
#define AFHIP_I16 2      /* afhip_plan_desc.dtype: int16 storage, float32 values by afhip_packing */
#define AFHIP_U16 3      /* afhip_plan_desc.dtype: uint16 storage, float32 values by afhip_packing */

/* reducer codes: 0..4 are _STAT_CODE of aggfly/aggregate/nb_kernels.py:33 */
#define AFHIP_MEAN     0
#define AFHIP_SUM      1
#define AFHIP_MIN      2
#define AFHIP_MAX      3
#define AFHIP_NANMEAN  4
#define AFHIP_DD       5   /* _block_dd      nb_kernels.py:158-179 */
#define AFHIP_BINS     6   /* _block_bins    nb_kernels.py:182-199 */
#define AFHIP_SINE_DD  7   /* _block_sine_dd nb_kernels.py:202-251 */
#define AFHIP_IDENTITY 8   /* outer level of a single-level plan: pass the inner value through */

/* element-wise transforms between the two temporal levels */
#define AFHIP_TF_NONE  0
#define AFHIP_TF_POW   1   /* Dataset.power / _power  aggfly/dataset/dataset.py:442-473,527-543 */
#define AFHIP_TF_HINGE 2   /* Dataset.spline hinge (x>knot)*(x-knot), dataset.py:475-481 (knot 20) */
#define AFHIP_TF_INTER 3   /* Dataset.interact / _interact: times a second array, dataset.py:483-518,547-563 */

/* The reference stores every step's output in its input dtype (nb_kernels.py:257-262), so on a
 * float32 cube its intermediates are float32.  This engine keeps float64 throughout unless a
 * column asks for the reference's roundings: */
#define AFHIP_ROUND_INNER 1   /* round the inner reducer's value to float32                  */
#define AFHIP_ROUND_HINGE 2   /* evaluate the hinge / inter transform in float32             */
#define AFHIP_ROUND_FINAL 4   /* round the column's final (outer) value to float32           */

const char* afhip_last_error(void);
int afhip_abi_version(void);
/* What this build of the library holds, as text into buf ("menu=full variants=426 arms=0 region_fused_twins=150 abi=4 packed_variants=69 packed_hist_variants=10 end_bins_variants=26");
 * returns the bytes needed.  menu: full = every kernel the planner can pick; arms = + the tuning arms a `tuning` hint can name (make
 * MENU=arms).  One count per kernel menu ("Kernel menus"): variants / arms / region_fused_twins count the float32 / float64 kernels, packed_variants the general kernels of AFHIP_I16 / AFHIP_U16 cubes,
 * packed_hist_variants their LDS-histogram kernels (plans of four or more contiguous equal-width strict bins), end_bins_variants the
 * LDS-histogram kernels of float32, float64 and packed cubes for such plans whose first and / or last bin is wider, or open-ended. */
int afhip_build_info(char* buf, int buf_len);
/* Kernels of one menu in the loaded build, by the menu's key: "float", "packed", "packed_hist", "end_bins", "cell_map" (the
 * LDS-histogram kernels, of every storage, for bins plans whose interior widths differ) or "packed_short" (the lean short-group kernels
 * of AFHIP_I16 / AFHIP_U16 cubes: inner groups of two to four rows).  -1: no menu of that name. */
int afhip_menu_size(const char* key);
/* Number of visible GPUs (hipGetDeviceCount); 0 when there is none. */
int afhip_device_count(void);
/* Name/arch/CU count of device `dev` into caller buffers (arch e.g. "gfx950"). */
int afhip_device_info(int dev, char* name, int name_len, char* arch, int arch_len, int* n_cus,
                      int64_t* hbm_bytes);

/* ------------------------------------------------------------------------------------
 * Grouped temporal reducers — drop-in for the numba kernels.
 *
 *   afhip_group_stat     replaces _block_stat(cube, bounds, code, out)        nb_kernels.py:121-155
 *   afhip_group_dd       replaces _block_dd(cube, bounds, ddargs, out)        nb_kernels.py:158-179
 *   afhip_group_bins     replaces _block_bins(cube, bounds, ddargs, out)      nb_kernels.py:182-199
 *   afhip_group_sine_dd  replaces _block_sine_dd(cube, bounds, ddargs, out)   nb_kernels.py:202-251
 *
 * cube_dev   [T, n_cells] of `dtype`;  bounds HOST int64[G+1], group g = steps
 *            [bounds[g], bounds[g+1]) (empty groups allowed -> NaN);
 * ddargs     HOST double[D*3] rows (t0, t1, flag) as in the reference;
 * out_dev    [G, n_cells] (stat) or [G, n_cells, D] of `dtype` — the reference's output
 *            layout and dtype (accumulation is float64, the store rounds to `dtype`,
 *            nb_kernels.py:257-268).
 * Numerics: stat / dd / bins are bit-identical to the reference's loops (same operation order, float64 accumulators, no contraction).
 * One rule of its own — min / max of zeros of both signs: -0 < +0, the reference keeps the first seen (the hardware's min / max order
 * the two zeros; equal by value, the sign bit of a zero result may differ from the reference's).
 * sine_dd evaluates the same closed forms by other means (table acos, rsq + Newton, cubic arc tables):
 *     |out - exact| <= 1e-10 |exact| + 1e-12 max(tmax - tmin, |exact|),   exact = the closed forms of nb_kernels.py:202-251 in exact arithmetic
 * (tests/golden/sine_dd_fixtures.json at 50 digits; the reference's own libm evaluation sits at 3.5e-9 relative / 3e-14 of the window's scale next to
 * the window's edges, the (tmin, tmax)-pair forms here at 1.7e-11 / 5.5e-15: profiles/r04_sine_accuracy.json).
 * Windows that hold +-inf, or whose range or sum overflows, are outside sine_dd's contract (the closed forms subtract infinities).
 * D is unbounded, like the reference's loop over ddargs rows (nb_kernels.py:166,190,215): more rows than one pass over the
 * cube holds (16) run as consecutive passes inside the call, each writing its own columns of out_dev.
 * These calls build a temporary plan, own their scratch and synchronise `stream` before they return.
 * ---------------------------------------------------------------------------------- */
int afhip_group_stat(const void* cube_dev, int dtype, int64_t T, int64_t n_cells,
                     const int64_t* bounds, int64_t G, int code, void* out_dev, void* stream);
int afhip_group_dd(const void* cube_dev, int dtype, int64_t T, int64_t n_cells,
                   const int64_t* bounds, int64_t G, const double* ddargs, int64_t D,
                   void* out_dev, void* stream);
int afhip_group_bins(const void* cube_dev, int dtype, int64_t T, int64_t n_cells,
                     const int64_t* bounds, int64_t G, const double* ddargs, int64_t D,
                     void* out_dev, void* stream);
int afhip_group_sine_dd(const void* cube_dev, int dtype, int64_t T, int64_t n_cells,
                        const int64_t* bounds, int64_t G, const double* ddargs, int64_t D,
                        void* out_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Region x cell weights, uploaded once as CSR.
 *
 * Replaces the COO triplets of _weight_triplets (aggfly/aggregate/spatial.py:157-178).
 * Rows are regions in sorted-region-id order; inside a row the entries keep the weights
 * table's order, so sums run in the order np.add.at visits them (spatial.py:185).
 * indptr HOST int64[R+1]; cols HOST int64[nnz] (cell positions, 0 <= col < n_cells);
 * w HOST double[nnz], every weight finite (zero and negative weights are fine; a NaN or infinite one is refused with AFHIP_E_INVALID).
 * Regions without entries and a table without any (nnz == 0) are valid: their sums are 0 and their results NaN.
 * The handle owns device copies; free with afhip_csr_destroy.
 * ---------------------------------------------------------------------------------- */
typedef struct afhip_csr afhip_csr;
int afhip_csr_create(const int64_t* indptr, const int64_t* cols, const double* w, int64_t R,
                     int64_t nnz, int64_t n_cells, afhip_csr** out);
void afhip_csr_destroy(afhip_csr* csr);
/* Devices.  A handle (afhip_csr, afhip_plan) belongs to the device that was current (hipGetDevice) on the calling thread
 * when it was created; its tables and scratch live there.  Every entry point that takes a handle makes that device current
 * for the duration of the call and restores the caller's afterwards, so a worker thread that still sits on device 0 (the
 * reference calls its kernels from dask's thread pool, nb_kernels.py:271-305) drives a handle of device r correctly.  What
 * must match is the data: afhip_plan_run / _run_temporal refuse (AFHIP_E_INVALID) a cube or a CSR that lives on another
 * device than the plan.  Entry points without a handle (afhip_group_*, afhip_transform, afhip_place_box, ...) run on the
 * device that owns their array argument.  `stream` must be a stream of that device (or NULL).  The same holds for every other
 * device pointer handed to a plan: the second cube of afhip_plan_bind_inter, the outputs (num / den / res / cells) and a
 * caller-owned workspace are refused with AFHIP_E_INVALID when the runtime knows them to live on another device.
 * afhip_csr_device / afhip_plan_device: the device a handle was created on (-1 for NULL).
 *
 * Threads.  Entry points without a handle are re-entrant.  An afhip_csr is immutable after creation (the run tables it
 * caches on first use are built under its own lock): share ONE CSR between any number of threads and plans.  An afhip_plan is
 * NOT re-entrant: it owns scratch in HBM, per-launch event pairs and the second-cube bindings, so two calls must never be
 * inside the same plan at once — give every worker thread its own plan (plans are cheap: tables of a few KB) or serialise the
 * calls; `aggfly_amd/engine.py` holds a per-plan lock around bind + run.  Two plans on two streams run concurrently. */
int afhip_csr_device(const afhip_csr* csr);

/* Replaces _scatter_block(block, region_idx, cell_idx, w_vals, n_regions)
 * (spatial.py:181-186): out[r, t] = sum_j w[j] * block[col[j], t], float64, entries in
 * table order, products rounded before each add (no fused multiply-add).
 * block_dev [n_cells, nt] float64; out_dev [R, nt] float64. */
int afhip_scatter_block(const afhip_csr* csr, const double* block_dev, int64_t nt,
                        double* out_dev, void* stream);

/* Element-wise transforms on a whole array — what Dataset.power / Dataset.spline / Dataset.interact do per dask block
 * (`_power` np.power(block, exp) dataset.py:527-543; hinge (x > knot) * (x - knot) dataset.py:475-481; `_interact`
 * np.multiply(block, other) dataset.py:547-563).  x_dev [n] of x_dtype -> out_dev [n] of out_dtype (AFHIP_F32 / AFHIP_F64);
 * transform AFHIP_TF_POW (arg = exponent: integer exponents through the correctly rounded double-double chain, others
 * through pow), AFHIP_TF_HINGE (arg = knot) or AFHIP_TF_INTER (other_dev [n] of other_dtype; arg unused).  Arithmetic is
 * float64 and the store rounds to out_dtype, except that a float32 -> float32 hinge / product is evaluated in float32
 * like numpy's.  In-place (out_dev == x_dev with equal dtypes) is allowed. */
int afhip_transform(const void* x_dev, int x_dtype, int64_t n, int transform, double arg,
                    const void* other_dev, int other_dtype, void* out_dev, int out_dtype, void* stream);

/* Measuring aid (no counterpart in the reference): the streaming-read ceiling of THIS box for a time-major cube — a kernel with the
 * temporal kernels' access pattern and no arithmetic (8 bytes per lane, single-wave workgroups, four non-temporal row loads in
 * flight; rows too short to fill the card are read in time chunks, as the temporal kernels do) launched `launches` times back to back over
 * cube_dev [T rows of row_bytes bytes, row_bytes % 8 == 0]; ms_out[i] = the i-th launch's duration by HIP events.  Synchronises `stream`.  bench.py reports T * row_bytes / min(ms) beside the 8 TB/s spec peak. */
int afhip_read_probe(const void* cube_dev, int64_t T, int64_t row_bytes, int launches, float* ms_out, void* stream);

/* Ingestion helper (no counterpart in the reference, whose chunks are assembled by dask on the host,
 * aggfly/dataset/dataset.py:697-728): copies the part [st, st+nt) x [sy, sy+ny) x [sx, sx+nx) of a
 * decoded chunk [*, by, bx] (contiguous, in HBM) into the time-major cube [*, NY, NX] at (t0, y0, x0).
 * elem_size 2, 4 or 8 bytes; both pointers are device memory; nothing is retained. */
int afhip_place_box(const void* chunk_dev, void* cube_dev, int elem_size,
                    int64_t by, int64_t bx, int64_t st, int64_t sy, int64_t sx,
                    int64_t nt, int64_t ny, int64_t nx,
                    int64_t NY, int64_t NX, int64_t t0, int64_t y0, int64_t x0, void* stream);

/* afhip_place_box for a staged block of BIG-ENDIAN elements — the time steps of a NetCDF classic file (CDF-1 / CDF-2) as they lie in
 * the file, uploaded as raw bytes: the same box arguments, bounds checks and launch-size refusal, and the bytes of every element
 * are reversed on the way (elem_size 2, 4 or 8; block_dev element-aligned).  One pass: each staged byte is read once, each cube
 * byte written once. */
int afhip_place_box_swapped(const void* block_dev, void* cube_dev, int elem_size,
                            int64_t by, int64_t bx, int64_t st, int64_t sy, int64_t sx,
                            int64_t nt, int64_t ny, int64_t nx,
                            int64_t NY, int64_t NX, int64_t t0, int64_t y0, int64_t x0, void* stream);

/* afhip_place_box for a chunk stored with time LAST — the layout the reference's converter writes (aggfly/dataset/zarr_convert.py:83-113:
 * `Dataset.da` is (latitude, longitude, time)): copies the part [sy, sy+ny) x [sx, sx+nx) x [st, st+nt) of a decoded chunk
 * [by, bx, bt] (contiguous, time fastest, in HBM) into the time-major cube [*, NY, NX] at (t0, y0, x0) — a tiled transpose through
 * LDS, each staged byte read once, each cube byte written once.  elem_size 2, 4 or 8 bytes; the box is checked against all three
 * extents of the chunk and against NY and NX (the cube's time extent is the caller's to check); an empty box returns AFHIP_OK
 * without a launch; nothing is retained. */
int afhip_place_box_tlast(const void* chunk_dev, void* cube_dev, int elem_size,
                          int64_t by, int64_t bx, int64_t bt, int64_t sy, int64_t sx, int64_t st,
                          int64_t ny, int64_t nx, int64_t nt,
                          int64_t NY, int64_t NX, int64_t t0, int64_t y0, int64_t x0, void* stream);

/* numcodecs element filters of Zarr format-2 arrays undone in HBM (aggfly_amd/io.py `_ScatterJob`; kernels in afhip_filter_kernels.h).
 *
 * afhip_delta_decode: Delta's decode — an in-place inclusive WRAPPING prefix sum over each of n_chunks decoded chunks that lie back
 * to back in stage_dev, chunk_elems integer elements of elem_size 1, 2, 4 or 8 bytes each (stage_dev element-aligned; 16-byte
 * accesses when it is 16-byte aligned and chunk_elems * elem_size a multiple of 16).  Three launches on `stream` — per-tile sums,
 * a scan of each chunk's tile sums, a per-tile scan seeded with the tile's prefix (tiles of 16 KiB; one launch when a chunk is one
 * tile) —, none of which waits for another workgroup.  scratch_dev: caller-owned, 8-byte aligned, at least
 * afhip_delta_scratch_bytes(n_chunks, chunk_elems, elem_size) bytes (-1 for what the call below refuses); it holds one element per
 * tile and is not read after the call's work is done.  Reads and writes [stage_dev, stage_dev + n_chunks * chunk_elems * elem_size)
 * and that part of the scratch, nothing else.  AFHIP_E_INVALID, with nothing launched: n_chunks < 0, chunk_elems <= 0, a product that overflows int64, another
 * elem_size, more than 2^31 - 1 tiles (or chunks) in one call, a misaligned or null buffer, a scratch that is too small.  n_chunks
 * == 0 returns AFHIP_OK without a launch.
 *
 * afhip_fso_decode: FixedScaleOffset's decode, dst[i] = src[i] / scale + offset for i in [0, n), src_type one of AFHIP_T_I8 ...
 * AFHIP_T_F64, dst_type AFHIP_T_F32 or AFHIP_T_F64.  Integer sources: the division and the sum in float64 (IEEE division, no
 * contraction), rounded once to dst_type.  AFHIP_T_F32 sources: both in float32, scale and offset rounded to float32 first, then
 * converted; AFHIP_T_F64 sources: in float64.  (What numpy gives for `enc / scale + offset` followed by `astype`.)  With scale 1 and
 * offset 0 an integer source is converted exactly as a cast would.  src_dev and dst_dev are distinct, element-aligned device buffers
 * of n elements (16-byte accesses where both are aligned for them); AFHIP_E_INVALID, with nothing launched: another type code, n < 0
 * or beyond one launch (2^31 - 1 workgroups of 256), a scale of 0 or NaN, null, misaligned or overlapping buffers.  Nothing is retained. */
enum { AFHIP_T_I8 = 0, AFHIP_T_U8 = 1, AFHIP_T_I16 = 2, AFHIP_T_U16 = 3, AFHIP_T_I32 = 4, AFHIP_T_U32 = 5, AFHIP_T_F32 = 6, AFHIP_T_F64 = 7 };
int64_t afhip_delta_scratch_bytes(int64_t n_chunks, int64_t chunk_elems, int elem_size);
int afhip_delta_decode(void* stage_dev, int64_t n_chunks, int64_t chunk_elems, int elem_size,
                       void* scratch_dev, int64_t scratch_bytes, void* stream);
int afhip_fso_decode(const void* src_dev, void* dst_dev, int64_t n, int src_type, int dst_type,
                     double scale, double offset, void* stream);

/* GRIB fields (editions 1 and 2, simple packing) unpacked in HBM: aggfly_amd/io.py `_GribSource.to_device`, aggfly_amd/grib.py.
 * stage_dev (4-byte aligned, stage_bytes a multiple of 4) holds, as they lie in the file, the packed bits (and the bitmaps) of n_steps fields of one NY x NX grid; steps_dev one
 * record per field: data_off / data_bytes — its staged packed bits; first_point / first_bit — the value index (= grid point; only
 * without a bitmap) and the bit (0..7, from the most significant) of the first staged byte where that value begins, so that a step
 * may be staged from the middle of its data section; bitmap_off — its bitmap of ceil(NY * NX / 8) bytes (one bit per grid point in
 * scan order, most significant bit first, 1 = a value is there), or -1 (with a bitmap first_point and first_bit are 0: the data
 * section is staged whole); nbits 0..32; R, s, d — the value of a point is (float)(((X * s) + R) * d) in float64, X its nbits
 * big-endian bits at bit (index * nbits), index its grid point or, with a bitmap, the number of 1-bits before it; a point whose bit
 * is 0 becomes NaN (0x7fc00000).  The box [y0, y0 + ny) x [x0, x0 + nx) of step i is written to the float32 cube [cube_nt, cube_NY,
 * cube_NX] at (t0 + i, cy, cx).  rank_dev: caller-owned scratch of afhip_grib_rank_bytes(n_steps, NY * NX) bytes (-1: absurd sizes).
 * A record whose ranges leave [0, stage_bytes), whose nbits > 32, whose staged bytes are too few for the last value the box needs or
 * whose bitmap is shorter than the grid is refused: the step is not written and *errors_dev grows by one.  Whatever the records say,
 * nothing is read outside the stage and the scratch and nothing is written outside the box.  AFHIP_E_INVALID: a box outside the grid
 * or the cube, cube_elem_size != 4, buffers on different devices.  The work is enqueued on `stream`; nothing is retained. */
typedef struct afhip_grib_step { int64_t data_off, data_bytes, first_point, bitmap_off; int32_t first_bit, nbits; double R, s, d; } afhip_grib_step;
int64_t afhip_grib_rank_bytes(int64_t n_steps, int64_t n_points);
int afhip_grib_unpack(const void* stage_dev, int64_t stage_bytes, const afhip_grib_step* steps_dev, int64_t n_steps,
                      int64_t NY, int64_t NX, int64_t y0, int64_t x0, int64_t ny, int64_t nx,
                      void* cube_dev, int cube_elem_size, int64_t cube_nt, int64_t cube_NY, int64_t cube_NX,
                      int64_t t0, int64_t cy, int64_t cx, void* rank_dev, int64_t rank_bytes, int32_t* errors_dev, void* stream);

/* GRIB fields in complex packing (edition 2, data representation templates 5.2 and 5.3: complex packing without and with spatial
 * differencing) unpacked in HBM; the layout of section 7 is written out in aggfly_amd/grib.py.  stage_dev as above; steps_dev one record
 * per field: data_off / data_bytes - the body of its section 7 (from octet 6 on), staged whole; bitmap_off as above; n_values - N, the
 * number of packed values (NY * NX, or with a bitmap its 1-bits); n_groups, ref_len, last_len, nbits_ref, ref_width, nbits_width,
 * len_inc, nbits_len - octets 32-47 and 20 of section 5; order - 0 for template 5.2, 1 or 2 for 5.3; extra - the octets (0..4) of
 * ival1 [, ival2] and minsd at the head of the body; R, s, d as above.  `order` is one number for the whole call, and a record of another
 * order is refused.  X is a signed 64-bit integer here (wrapping sums), and the value (float)(((X * s) + R) * d) is exact while
 * |X| < 2^53.  scratch_dev: caller-owned, 16-byte aligned, afhip_grib_complex_scratch_bytes(n_steps, NY * NX, max_groups) bytes (-1:
 * absurd sizes), max_groups >= every record's n_groups.  Refused - the step is not written and *errors_dev grows by one -: ranges
 * that leave [0, stage_bytes), n_groups > max_groups, table widths above 32 bits, a group width above 32, group lengths that do not sum to
 * n_values, tables or values that run past data_bytes, a bitmap whose 1-bits are not n_values, another order than the call's.  Whatever
 * the records say, nothing is read outside the stage and the scratch and nothing is written outside the box and the scratch.
 * AFHIP_E_INVALID as above, and for an order outside 0..2.  The work is enqueued on `stream`; nothing is retained. */
typedef struct afhip_grib_cstep {
    int64_t data_off, data_bytes, bitmap_off, n_values, n_groups, ref_len, last_len;
    int32_t nbits_ref, ref_width, nbits_width, len_inc, nbits_len, order, extra, pad;
    double R, s, d;
} afhip_grib_cstep;
int64_t afhip_grib_complex_scratch_bytes(int64_t n_steps, int64_t n_points, int64_t max_groups);
int afhip_grib_unpack_complex(const void* stage_dev, int64_t stage_bytes, const afhip_grib_cstep* steps_dev, int64_t n_steps, int order,
                              int64_t max_groups, int64_t NY, int64_t NX, int64_t y0, int64_t x0, int64_t ny, int64_t nx,
                              void* cube_dev, int cube_elem_size, int64_t cube_nt, int64_t cube_NY, int64_t cube_NX,
                              int64_t t0, int64_t cy, int64_t cx, void* scratch_dev, int64_t scratch_bytes, int32_t* errors_dev, void* stream);

/* GRIB2 CCSDS packing (data representation template 5.42) unpacked in HBM: afhip_grib_unpack's arguments and placement, with one
 * afhip_grib_astep per step.  data_off / data_bytes: the whole body of the step's section 7, one CCSDS 121.0-B adaptive-entropy-coded
 * stream as libaec writes it (aggfly_amd/csrc/aec_passes.h has the format) of n_values samples of nbits bits (0: a constant field, no
 * stream); bitmap_off: the step's bitmap, or -1; n_values: the grid points, or with a bitmap its 1-bits; flags, block_size, rsi: octets
 * 22, 23 and 24-25 of section 5 (flag 8: the preprocessor; 2 and 4 are ignored); R, s, d as above.  scratch_dev: caller-owned, 16-byte
 * aligned, afhip_grib_ccsds_scratch_bytes(n_steps, NY * NX, max_rsis) bytes (-1: absurd sizes), max_rsis >= every record's
 * ceil(n_values / (rsi * block_size)).  Refused - the step is not written and *errors_dev grows by one -: ranges that leave
 * [0, stage_bytes), nbits above 32, any flag other than 2, 4 and 8, a block size other than 8 / 16 / 32 / 64, rsi outside 1..4096, more
 * reference sample intervals than max_rsis, a bitmap whose 1-bits are not n_values (without one: n_values other than NY * NX), a zero
 * run beyond its interval's last block, a second-extension code above 90, a delta above 2^nbits - 1, a stream that runs past
 * data_bytes.  Whatever the records and the streams say, nothing is read outside the stage and the scratch and nothing is written
 * outside the box and the scratch.  AFHIP_E_INVALID as above.  The work is enqueued on `stream`; nothing is retained. */
typedef struct afhip_grib_astep {
    int64_t data_off, data_bytes, bitmap_off, n_values;
    int32_t nbits, flags, block_size, rsi;
    double R, s, d;
} afhip_grib_astep;
int64_t afhip_grib_ccsds_scratch_bytes(int64_t n_steps, int64_t n_points, int64_t max_rsis);
int afhip_grib_unpack_ccsds(const void* stage_dev, int64_t stage_bytes, const afhip_grib_astep* steps_dev, int64_t n_steps,
                            int64_t max_rsis, int64_t NY, int64_t NX, int64_t y0, int64_t x0, int64_t ny, int64_t nx,
                            void* cube_dev, int cube_elem_size, int64_t cube_nt, int64_t cube_NY, int64_t cube_NX,
                            int64_t t0, int64_t cy, int64_t cx, void* scratch_dev, int64_t scratch_bytes, int32_t* errors_dev, void* stream);

/* TIFF stacks in HBM (aggfly_amd/tiff.py reads the image file directories; aggfly_amd/io.py: `_TiffSource.to_device`).  One
 * afhip_tiff_seg per staged segment (a strip or a tile) serves both entries.
 *
 * afhip_lzw_decode: the n TIFF LZW streams [src_off, src_off + src_bytes) of the stage (codes most significant bit first, 9 to 12
 * bits, Clear 256, EndOfInformation 257, libtiff's early change; aggfly_amd/csrc/lzw_passes.h has the format, the span table and the
 * safety contract) decoded into [dec_off, dec_off + dec_bytes) of the decoded buffer, one wave per segment.  A stream ends at
 * EndOfInformation or at dec_bytes.  Bad — `bad` of the record is set (else cleared), *errors_dev grows by one and the segment's decoded
 * bytes are left untouched —: ranges that leave the stage or the decoded buffer, dec_bytes above 2^31 - 1, a code above the next free
 * one, a first code after Clear that is no literal, a span beyond dec_bytes, a stream that ends before dec_bytes.  The records are
 * written (bad), so they are not const.
 *
 * afhip_tiff_place: the n decoded segments — `rows` rows of `pitch` samples of elem_size (1, 2, 4, 8) bytes at dec_off, whose first
 * sample belongs at row y, column x of image t of the batch — into the cube (NT, NY, NX) of the same element size: the predictor is
 * undone along every row (1: none; 2: horizontal differencing, a wrapping running sum in the sample's width, after the byte swap; 3:
 * the floating-point predictor, a running sum mod 256 over the row's pitch * elem_size bytes and a gather of the byte planes, most
 * significant first — `swap` is not applied), samples are byte-swapped where swap != 0, and the samples of image rows [y0, y0 + ny) and
 * columns [x0, x0 + nx) are written at cube[t0 + t][cy + row - y0][cx + column - x0]; every other sample (the padding of partial
 * tiles, what the box cuts off) is dropped.  max_rows >= every record's rows.  A record with bad != 0 is skipped; one whose samples
 * leave [0, decoded_bytes), whose dec_off is not a multiple of elem_size, whose t is outside [0, NT - t0) or whose rows / pitch / y / x
 * are negative is not placed and counts in *errors_dev.  AFHIP_E_INVALID: a box that does not fit the cube, an elem_size or predictor
 * other than those, predictor 3 on 1- or 2-byte samples, pointers on different devices or misaligned.  Nothing is written outside the
 * box of the cube.  Both entries enqueue on `stream` and retain nothing. */
typedef struct afhip_tiff_seg {
    int64_t src_off, src_bytes;      /* afhip_lzw_decode: the compressed stream in the stage */
    int64_t dec_off, dec_bytes;      /* the decoded segment in the decoded buffer */
    int32_t rows, pitch;             /* afhip_tiff_place: rows, and samples from one row to the next */
    int32_t t, y, x;                 /* image of the batch, row and column of the segment's first sample */
    int32_t bad;
} afhip_tiff_seg;
int afhip_lzw_decode(const void* stage_dev, int64_t stage_bytes, afhip_tiff_seg* records_dev, int64_t n, void* out_dev, int64_t out_bytes,
                     int32_t* errors_dev, void* stream);
int afhip_tiff_place(const void* decoded_dev, int64_t decoded_bytes, const afhip_tiff_seg* records_dev, int64_t n, int64_t max_rows,
                     int elem_size, int predictor, int swap, void* cube_dev, int64_t NT, int64_t NY, int64_t NX,
                     int64_t y0, int64_t x0, int64_t ny, int64_t nx, int64_t t0, int64_t cy, int64_t cx, int32_t* errors_dev, void* stream);

/* afhip_tiff_place_bands: afhip_tiff_place for chunky multi-band segments (SamplesPerPixel = bands, PlanarConfiguration 1), every band
 * a time step.  The same records: a decoded segment holds rows * pitch * bands samples, `pitch` counts pixels, sample
 * (row, pixel, band) lies at (row * pitch + pixel) * bands + band, and `t` is the step of the segment's band 0.  The predictor is undone
 * at a stride of `bands` samples as libtiff does it (2: sample i adds sample i - bands, after the byte swap; 3: a running sum mod 256
 * over the row's pitch * bands * elem_size bytes at stride `bands`, continuing across the byte planes, sample i gathered from the bytes
 * plane * (pitch * bands) + i, most significant plane first), and the sample goes to
 * cube[t0 + t + band, cy + y + row - y0, cx + x + pixel - x0] when it lies in the box and 0 <= t + band < NT - t0.  t may be negative
 * down to -(bands - 1): a time window that begins or ends inside a page's bands drops the bands outside it.  A record is unsound —
 * not placed, counted in *errors_dev — as for afhip_tiff_place, with rows * pitch * bands samples, or with t <= -bands or
 * t >= NT - t0.  AFHIP_E_INVALID as for afhip_tiff_place, and bands outside 1 .. 65535.  Nothing is read outside the decoded buffer,
 * nothing written outside the box.  A tiled transpose through LDS (aggfly_amd/csrc/afhip_tiff_kernels.h: k_tiff_place_bands); planar
 * files (PlanarConfiguration 2) hold single-band segments and go through afhip_tiff_place.  Parity with a GDAL- or Earth-Engine-written
 * multi-band file is unverified.  Enqueues on `stream` and retains nothing. */
int afhip_tiff_place_bands(const void* decoded_dev, int64_t decoded_bytes, const afhip_tiff_seg* records_dev, int64_t n, int64_t max_rows,
                           int64_t bands, int elem_size, int predictor, int swap, void* cube_dev, int64_t NT, int64_t NY, int64_t NX,
                           int64_t y0, int64_t x0, int64_t ny, int64_t nx, int64_t t0, int64_t cy, int64_t cx, int32_t* errors_dev, void* stream);

/* Chunk decode in HBM ("or GPU-side decode"; the reference decodes on host threads inside its dask
 * graph, aggfly/dataset/dataset.py:697-728).  Blosc-1 chunks whose streams are LZ4 cross PCIe compressed; the host parses
 * the containers (afcodec_blosc_lz4_plan, include/aggfly_codec.h) into the two record lists below, which travel to HBM with
 * the compressed bytes.  afhip_lz4_decode_streams: one wave per stream (any length) resolves the sequences of a 64-byte
 * window in its lanes and writes dsize bytes straight to (to_out ? out_dev : tmp_dev) + dst_off — out_dev may be the data
 * cube itself; stored streams (csize == dsize) are copied.  max_dsize = the longest dsize of the list (checked >= 0, not
 * otherwise used since the decode left LDS).  A malformed stream writes nothing outside its own destination and adds 1 to
 * *errors_dev (read it after the next synchronisation).
 * afhip_unshuffle_blocks: Blosc's byte shuffle undone, tmp_dev -> out_dev (typesize 1: a copy).
 * afhip_bitunshuffle_blocks: Blosc's bit shuffle undone, the same records and launch shape (at most 65,535 blocks a call): with
 * n = bsize / typesize elements, bit k of byte j of element e is bit (e % 8) of tmp[(8j + k) * (n / 8) + e / 8]; a block whose n
 * is not a multiple of 8 is copied as it is (c-blosc leaves it unshuffled), and so are the bsize - n * typesize trailing bytes.
 * The other Blosc-1 flavours — Zstandard streams, the bit shuffle — are planned by afcodec_blosc_plan, whose Zstandard frames
 * afhip_zstd_decode (below) decodes into the same tmp_dev before the two unshuffles run.  All pointers are device memory. */
typedef struct afhip_lz4_stream { int64_t src_off, dst_off; int32_t csize, dsize, to_out, pad; } afhip_lz4_stream;
typedef struct afhip_shuffle_block { int64_t tmp_off, out_off; int32_t bsize, typesize; } afhip_shuffle_block;
int afhip_lz4_decode_streams(const void* comp_dev, const afhip_lz4_stream* streams_dev, int64_t n_streams, int32_t max_dsize,
                             void* tmp_dev, void* out_dev, int32_t* errors_dev, void* stream);
int afhip_unshuffle_blocks(const void* tmp_dev, void* out_dev, const afhip_shuffle_block* blocks_dev, int64_t n_blocks,
                           int32_t max_bsize, void* stream);
int afhip_bitunshuffle_blocks(const void* tmp_dev, void* out_dev, const afhip_shuffle_block* blocks_dev, int64_t n_blocks,
                              int32_t max_bsize, void* stream);

/* Chunk ENCODE in HBM: the write side (dataset_to_zarr with encode="gpu"), the decode route above in reverse.  The cube stays in
 * HBM; per batch of chunks the caller runs, in order:
 * afhip_take_box: the inverse of afhip_place_box — the box [t0, t0+nt) x [y0, y0+ny) x [x0, x0+nx) of the time-major cube
 * [*, NY, NX] into the contiguous chunk buffer [ct, cy, cx] at chunk_dev; every element of the buffer beyond the box (Zarr pads edge
 * chunks to the full chunk shape) takes the low elem_size bytes of `fill` (NaN bits for floats, 0 for integers).  elem_size 1, 2, 4, 8.
 * afhip_shuffle_blocks: Blosc's byte shuffle, out_dev (the chunk buffer) -> tmp_dev (the shuffle scratch), over the records of
 * afhip_unshuffle_blocks with the same meaning of their fields and the same limit of 65,535 blocks a call; typesize 1 is a copy, the
 * bsize % typesize trailing bytes are copied.
 * afhip_lz4_encode_streams: one wave per record — src_off: the stream's raw bytes in in_dev (the shuffled input), dst_off: its slot of
 * dsize bytes in slots_dev, dsize: the raw length, to_out != 0: store without a search; csize and pad are not read.  csize_dev[i]
 * receives the stream's size: an LZ4 block of at most dsize - 1 bytes, or dsize with the raw bytes in the slot (stored: the rule of
 * afcodec_blosc_encode).  The bytes are a function of the input alone (aggfly_amd/csrc/lz4_encode_pass.h; the host runs the same
 * text as afcodec_lz4_encode_emulate).  Nothing is written outside the slot.
 * afhip_zstd_encode_blocks: the same place in the route for Zstandard streams (compress="blosc-zstd"): one wave per record — src_off:
 * the block's n raw bytes (1 .. 131072) in in_dev, dst_off: its slot of n + 3 bytes in slots_dev, scratch_off: its own
 * afhip_zstd_encode_scratch_bytes(n) bytes in scratch_dev, 256-aligned and behind the first afhip_zstd_encode_scratch_bytes(0) bytes,
 * which hold the launch's code tables; last != 0: the Last_Block bit.  csize_dev[i] receives the size of one complete Zstandard block,
 * Block_Header included: RLE, compressed (its own Huffman tree, predefined sequence codes, no repeat offsets, no match before the
 * block) or raw, at most n + 3 bytes.  Blocks in the order of their records behind a frame header are a frame; the caller writes the
 * header.  The bytes are a function of the input alone (aggfly_amd/csrc/zstd_encode_pass.h; the host runs the same text as
 * afcodec_zstd_encode_block_emulate).  Nothing is written outside the slot and the block's scratch.
 * afhip_copy_ranges: bytes [src_off, src_off + n) of src_dev to dst_dev + dst_off per record — after the host has read the sizes,
 * every stream from its slot to its place in the batch's packed output; ranges of one call must not overlap in dst_dev.
 * All pointers are device memory, the work is enqueued on `stream`, nothing is retained. */
typedef struct afhip_copy_range { int64_t src_off, dst_off, n; } afhip_copy_range;
int afhip_take_box(const void* cube_dev, void* chunk_dev, int elem_size, int64_t NY, int64_t NX,
                   int64_t t0, int64_t y0, int64_t x0, int64_t nt, int64_t ny, int64_t nx,
                   int64_t ct, int64_t cy, int64_t cx, uint64_t fill, void* stream);
int afhip_shuffle_blocks(const void* out_dev, void* tmp_dev, const afhip_shuffle_block* blocks_dev, int64_t n_blocks,
                         int32_t max_bsize, void* stream);
int afhip_lz4_encode_streams(const void* in_dev, const afhip_lz4_stream* streams_dev, int64_t n_streams, void* slots_dev,
                             int32_t* csize_dev, void* stream);
int afhip_copy_ranges(const void* src_dev, void* dst_dev, const afhip_copy_range* ranges_dev, int64_t n_ranges, void* stream);
typedef struct afhip_zstd_encode_block { int64_t src_off, dst_off, scratch_off; int32_t n, last; } afhip_zstd_encode_block;
int64_t afhip_zstd_encode_scratch_bytes(int64_t n);
int afhip_zstd_encode_blocks(const void* in_dev, const afhip_zstd_encode_block* blocks_dev, int64_t n_blocks, void* scratch_dev,
                             void* slots_dev, int32_t* csize_dev, void* stream);

/* Zstandard frames decoded in HBM (Zarr v2 compressor "zstd", Zarr v3 bytes -> zstd, shards too).  The host walks the frame,
 * block and section headers (afcodec_zstd_plan, include/aggfly_codec.h) into one record per frame and per block, which
 * travel to HBM with the compressed bytes; the tables are built, literals and sequences decoded and the LZ matches resolved
 * on the GPU, in launch-ordered passes over all blocks of the batch (aggfly_amd/csrc/zstd_passes.h).  Frame f's
 * Frame_Content_Size bytes go to out_dev + dst_off.  scratch_dev: afhip_zstd_scratch_bytes(...) bytes, caller-owned (~4 bytes
 * per decoded byte + 11 KiB per block).  A damaged frame writes nothing outside its own destination and the scratch, and
 * adds 1 to *errors_dev; rounds_dev (may be NULL) receives the number of pointer-jump rounds that had work.  Nothing
 * allocates or synchronises; all pointers are device memory. */
typedef struct afhip_zstd_frame { int64_t dst_off, base, size; int32_t first_block, n_blocks; } afhip_zstd_frame;
typedef struct afhip_zstd_block {
    int64_t src, lit_off, seq_off;
    int32_t frame, btype, csize, lit_type, lit_size, lit_src, lit_csize, n_streams, huf_desc, huf_block, nseq, seq_src;
    int32_t mode[3], tab_desc[3], tab_block[3], pad;
} afhip_zstd_block;
int64_t afhip_zstd_scratch_bytes(int64_t n_blocks, int64_t n_frames, int64_t lit_bytes, int64_t n_seqs, int64_t dec_bytes);
int afhip_zstd_decode(const void* comp_dev, int64_t comp_bytes, const afhip_zstd_frame* frames_dev, int64_t n_frames,
                      const afhip_zstd_block* blocks_dev, int64_t n_blocks, int64_t lit_bytes, int64_t n_seqs, int64_t dec_bytes,
                      void* scratch_dev, int64_t scratch_bytes, void* out_dev, int32_t* errors_dev, int32_t* rounds_dev, void* stream);

/* zlib streams (RFC 1950 around RFC 1951 deflate) decoded in HBM: HDF5 / netCDF-4 [deflate] and [shuffle, deflate] chunks, Zarr v2
 * compressor "zlib".  The host reads only the two header bytes of a chunk (afcodec_inflate_plan, include/aggfly_codec.h) into one
 * record per stream; the blocks are walked, the Huffman tables built, the LZ77 matches resolved and the Adler-32 verified on the GPU,
 * in launch-ordered passes (aggfly_amd/csrc/inflate_passes.h), and the n_shuf chunks written with HDF5's shuffle filter are then
 * byte-unshuffled from the scratch into out_dev (max_bsize: the largest of them).  Stream s's dsize bytes go to out_dev + dst_off
 * (to_out) or to the scratch.  scratch_dev: afhip_inflate_scratch_bytes(...) bytes, caller-owned (~9 bytes per decoded byte + 5.25 KiB
 * per stream).  A damaged stream — malformed, of another size than planned, or failing its Adler-32 — writes nothing outside its own
 * destination and the scratch, and adds 1 to *errors_dev; rounds_dev (may be NULL) receives the number of pointer-jump rounds that
 * had work.  Not taken (the planner marks them for the host): gzip members, preset dictionaries, chunks of 1 GiB and more.
 * Nothing allocates or synchronises; all pointers are device memory. */
typedef struct afhip_inflate_stream {
    int64_t src, dst_off, base, seq_off;
    int32_t csize, dsize, to_out, first_block, n_blocks, first_piece;
} afhip_inflate_stream;
int64_t afhip_inflate_scratch_bytes(int64_t n_streams, int64_t n_pblocks, int64_t n_seqs, int64_t n_pieces, int64_t dec_bytes,
                                    int64_t tmp_bytes);
int afhip_inflate_decode(const void* comp_dev, int64_t comp_bytes, const afhip_inflate_stream* streams_dev, int64_t n_streams,
                         const afhip_shuffle_block* shuf_dev, int64_t n_shuf, int32_t max_bsize, int64_t n_pblocks, int64_t n_seqs,
                         int64_t n_pieces, int64_t dec_bytes, int64_t tmp_bytes, void* scratch_dev, int64_t scratch_bytes, void* out_dev,
                         int32_t* errors_dev, int32_t* rounds_dev, void* stream);

/* Replaces the body of SpatialAggregator.compute (spatial.py:110-133) for K names:
 * shared validity (all K non-NaN), den = W.valid, num_k = W.where(valid, x_k, 0),
 * res = num/den where den != 0 else NaN.
 * x_dev [K, n_cells, nt] float64; num_dev [K, R, nt]; den_dev [R, nt]; res_dev [K, R, nt]
 * (num_dev / den_dev may be NULL). */
int afhip_spatial_wavg(const afhip_csr* csr, const double* x_dev, int64_t K, int64_t nt,
                       double* num_dev, double* den_dev, double* res_dev, void* stream);

/* The divide of SpatialAggregator.compute on its own (spatial.py:127-133): res = num / den where den != 0 else NaN.
 * num_dev [K, R, P], den_dev [R, P], res_dev [K, R, P] float64.  For cell-axis sharding across GPUs: every rank's
 * numerators and denominators are summed first (one all-reduce), then divided once. */
int afhip_panel_divide(const double* num_dev, const double* den_dev, double* res_dev, int64_t K, int64_t R,
                       int64_t P, void* stream);

/* ------------------------------------------------------------------------------------
 * Fused plan: one pass over the raw cube for all output columns.
 *
 * Replaces, for one aggregate_dataset() call, the lazy graph built by aggregate_time
 * (aggfly/aggregate/aggregate.py:101-162) + SpatialAggregator.compute and executed by the
 * single dask.compute at spatial.py:125.  A column is
 *
 *     inner reducer over inner groups of raw steps        ('aggregate', calc @ groupby)
 *       -> element-wise transform                         ('transform', power / spline)
 *       -> outer reducer over outer groups of inner values ('aggregate', calc @ groupby)
 *
 * A single-level spec uses outer = AFHIP_IDENTITY with outer_bounds = [0,1,..,G1].
 * ---------------------------------------------------------------------------------- */
typedef struct afhip_column {
    int32_t inner;          /* AFHIP_MEAN..AFHIP_SINE_DD                                   */
    int32_t transform;      /* AFHIP_TF_*                                                   */
    int32_t outer;          /* AFHIP_MEAN, SUM, MIN, MAX, DD, BINS or AFHIP_IDENTITY        */
    int32_t rounding;       /* AFHIP_ROUND_* bits: emulate the reference's float32 intermediates (0 = all float64) */
    double inner_args[3];   /* (t0, t1, flag) for DD / BINS / SINE_DD                       */
    double transform_arg;   /* exponent (POW) or knot (HINGE)                               */
    double outer_args[3];   /* (t0, t1, flag) for an outer DD / BINS                        */
} afhip_column;

typedef struct afhip_plan_desc {
    int64_t T;                     /* time steps in the cube                                */
    int64_t n_cells;               /* NY*NX                                                  */
    int32_t dtype;                 /* AFHIP_F32 / AFHIP_F64 / AFHIP_I16 / AFHIP_U16 (afhip_plan_bind_packing) */
    int32_t K;                     /* number of columns                                      */
    int64_t G1;                    /* inner groups                                           */
    const int64_t* inner_bounds;   /* HOST int64[G1+1] over time steps                       */
    int64_t P;                     /* outer groups (output periods)                          */
    const int64_t* outer_bounds;   /* HOST int64[P+1] over inner groups                      */
    const afhip_column* columns;   /* HOST [K]                                               */
    int32_t exact_order;           /* 1: never split an outer period across workgroups, so
                                      every per-cell sum runs in the reference's order       */
    int32_t tuning;                /* 0 = default; else a load-path arm pipe*1000+vec*100+depth (a hint:
                                      falls back to the default when that arm is not compiled) */
} afhip_plan_desc;

typedef struct afhip_plan afhip_plan;
int afhip_plan_create(const afhip_plan_desc* desc, afhip_plan** out);
void afhip_plan_destroy(afhip_plan* plan);
int afhip_plan_device(const afhip_plan* plan);
/* AFHIP_TF_INTER columns: bind column `column`'s second cube before the plan runs.  inter_dev [G1, n_cells] of `dtype`
 * (AFHIP_F32 / AFHIP_F64), time-major like the cube: the value the column's inner reducer gives inner group g at a cell
 * is multiplied by inter_dev[g * n_cells + cell] (np.multiply(block, other), dataset.py:563, on the inner level's
 * output, whose time axis is the inner groups).  The pointer is read by every later run until it is bound again; the
 * caller keeps the memory alive.  A run with an unbound AFHIP_TF_INTER column fails with AFHIP_E_INVALID. */
int afhip_plan_bind_inter(afhip_plan* plan, int column, const void* inter_dev, int dtype);
/* 16-bit-packed cubes (AFHIP_I16, AFHIP_U16).  ERA5-style files store a field as int16 with scale_factor / add_offset / _FillValue,
 * other gridded products as uint16 (or as int16 with the attribute _Unsigned = "true": the same bits); such a cube
 * can stay packed in HBM — 2 bytes per cell and step instead of 4 — and the temporal kernel unpacks each element where it uses it.
 * The value of a stored q is, bit for bit what a float32 array library computes one operation at a time:
 *     f = (float)q;   n_pairs times:  f = f * mul[i];  f = f + add[i]   (each rounded to float32, never fused);   NaN if has_fill && q == fill
 * and everything after it is the float32 path (float64 accumulators, thresholds compared in float32 against the edges rounded down / up).
 * A pair half the chain lacks is sent as its exact identity: mul 1.0f, add -0.0f.  At most three pairs (unpack + a unit conversion or two).
 * afhip_plan_bind_packing: like afhip_plan_bind_inter, copied into the plan and read by every later run; an AFHIP_I16 / AFHIP_U16 plan that runs
 * unbound fails with AFHIP_E_INVALID, and binding a plan of another dtype is refused.  Such plans take the general kernels of the
 * direct-load path (no single-level form) and the slot-gather / table-order spatial stage; a plan of several output periods, without
 * exact_order, takes the region-fused period ends as a float plan does where the library holds the twin of its kernel (general and lean
 * short-group kernels at one and two cells per lane: afhip_menu_size("packed_rf"); afhip_plan_describe then says so).  The
 * afhip_group_* entry points and afhip_transform keep to AFHIP_F32 / AFHIP_F64.
 * AFHIP_U16 differs in one thing: the 16 stored bits are unsigned, f = (float)(unsigned)q (exact for 0..65535), and q == fill compares the
 * unsigned value.  A fill must lie in the storage's range (-32768..32767 / 0..65535).  Both dtypes run the same kernels: the signedness is a
 * field of the record the library fills from the plan's dtype at bind time.  `pad` is ignored: whatever the caller writes there is not read.
 * afhip_unpack_i16: the same rule on a whole array, q_dev int16[n] -> out_dev float[n] (a plain stream, 8 bytes read per lane).
 * afhip_unpack_u16: the same for uint16 storage, q_dev uint16[n]; same alignment rules (q_dev 8-byte, out_dev 16-byte aligned).
 * An afhip_packing is ONE rule.  A cube concatenated from several stores (yearly or monthly files, each with its own scale_factor /
 * add_offset / _FillValue) carries one rule per store:
 * afhip_plan_bind_packings: rule i unpacks the time steps bounds[i] .. bounds[i + 1]; rules [n], bounds [n + 1] (host arrays, copied),
 * bounds[0] == 0, bounds[n] == T, strictly increasing, 1 <= n <= T (no other cap on n); every fill in the range of the plan's storage; the
 * signedness is the plan's dtype for all rules alike.  Anything else returns AFHIP_E_INVALID, binds nothing — the earlier binding still
 * holds — and launches nothing.  afhip_plan_bind_packing(plan, p) is the case n == 1.  The same kernels serve both: a time step is a row of
 * the cube, so the rule is uniform per row and chosen by scalar code; with one rule a scalar branch skips the choice.
 * Binding while a run is in flight: a bind never changes what a launch that was already issued reads.  One rule travels by value in the
 * launch's argument record.  Several rules live in a table on the device that the plan owns; a bind writes the plan's host copy only, and
 * the NEXT run brings the table up to date by a copy ordered on that run's stream, in front of its kernel (and only when the rules differ
 * from the table's).  So runs that share a stream may be re-bound between them freely; as with the plan's workspace, runs of one plan on
 * DIFFERENT streams must not overlap.  (That copy reads host memory: a run whose rules changed cannot be captured into a graph.)
 * The afhip_unpack_* entry points take one rule: a multi-rule cube is materialised rule by rule, on its row ranges. */
typedef struct afhip_packing { int32_t n_pairs, has_fill, fill, pad; float mul[3], add[3]; } afhip_packing;
int afhip_plan_bind_packing(afhip_plan* plan, const afhip_packing* p);
int afhip_plan_bind_packings(afhip_plan* plan, const afhip_packing* rules, const int64_t* bounds, int32_t n);
int afhip_unpack_i16(const void* q_dev, int64_t n, const afhip_packing* p, float* out_dev, void* stream);
int afhip_unpack_u16(const void* q_dev, int64_t n, const afhip_packing* p, float* out_dev, void* stream);

/* Bytes of device scratch a run needs.  afhip_plan_workspace_bytes: the temporal stage alone (per-chunk partials; what
 * afhip_plan_run_temporal takes).  afhip_plan_run_workspace_bytes: a whole afhip_plan_run against `csr` (partials + the
 * cell-major panel + the [rows][P][K+1] sums of that table).  A caller-owned workspace must be 256-byte aligned. */
int64_t afhip_plan_workspace_bytes(const afhip_plan* plan);
int64_t afhip_plan_run_workspace_bytes(const afhip_plan* plan, const afhip_csr* csr);
/* Human-readable lowering (kernel variant, chunks, slots) into buf; returns bytes needed.  After an afhip_plan_run it names the
 * spatial route that run took: last-run=region-fused, last-run=slot-gather (one gather over the period partials),
 * last-run=panel (cell-major panel, then weighted sums: exact_order, per-cell output, AFHIP_NO_SLOT_SPMM) or
 * last-run=count-gather/N-lane (bin-count plans). */
int afhip_plan_describe(const afhip_plan* plan, char* buf, int buf_len);

/* Temporal stage only: cells_dev[K, P, n_cells] float64 = the per-cell, per-period value
 * of every column (NaN where the reference's temporal stage yields NaN).  This is what
 * aggregate_time returns before the spatial step (aggregate.py:160-162).
 * workspace_dev / workspace_bytes: caller-owned scratch of at least afhip_plan_workspace_bytes(plan) (AFHIP_E_INVALID when
 * smaller), or NULL / 0: the plan allocates and caches its own (hipMalloc; a plan that outgrows it keeps the old block
 * until afhip_plan_destroy, so that no run ever waits for the device in a hipFree). */
int afhip_plan_run_temporal(afhip_plan* plan, const void* cube_dev, double* cells_dev,
                            void* workspace_dev, int64_t workspace_bytes, void* stream);

/* Whole path: temporal stage, shared validity, CSR weighted sums, divide.
 * num_dev [K, R, P], den_dev [R, P], res_dev [K, R, P] float64 (num/den may be NULL);
 * cells_dev optional as above (NULL to skip materialising it).
 * Routes (results equal to rounding; exact_order plans always take the first): with cells_dev, or exact_order — slot merge into a
 * cell-major panel, then weighted sums in table order; without — one gather over the period partials (no panel), or, for plans with
 * several output periods whose table allows it, weighted sums per region formed inside the temporal kernel at every period end (the
 * per-cell period values are then never written); bin-count plans gather their packed records.  The CSR handle caches the tables of
 * the last route on first use (it is entered through a const pointer but guarded by its own lock).
 * workspace_dev / workspace_bytes: caller-owned scratch of at least afhip_plan_run_workspace_bytes(plan, csr), or NULL / 0 for
 * plan-owned scratch as above.  Nothing on the run path allocates, frees or synchronises when the workspace is the caller's
 * (the Python host hands every plan a block of torch's caching allocator: where a process's first hipMalloc'ed scratch lands
 * decides 7-9 % of the bin-count kernel on some boxes, profiles/r03_plan_order_probe.txt; afhip_plan_describe names which it was).
 * If kernel_ms is not NULL the call records HIP events on `stream` around the temporal
 * kernel and around the whole sequence, synchronises the stream, and writes
 * kernel_ms[0] = temporal kernel ms, kernel_ms[1] = whole sequence ms. */
int afhip_plan_run(afhip_plan* plan, const void* cube_dev, const afhip_csr* csr,
                   double* num_dev, double* den_dev, double* res_dev, double* cells_dev,
                   void* workspace_dev, int64_t workspace_bytes, void* stream, float* kernel_ms);

/* Per-launch device timing of the dominant (temporal) kernel without host syncs in the
 * timed region: _begin arms up to max_launches HIP event pairs; every afhip_plan_run then
 * records one pair around the temporal kernel on its stream; _end waits for the recorded
 * events, writes one duration (ms) per launch into ms_out[0..cap) and returns how many
 * launches were recorded (-1 on error).  Used by bench.py for roofline.achieved. */
int afhip_plan_profile_begin(afhip_plan* plan, int64_t max_launches);
int64_t afhip_plan_profile_end(afhip_plan* plan, float* ms_out, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* AGGFLY_HIP_H */
