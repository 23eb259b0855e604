// afhip_api.hip — C-ABI entry points and kernel dispatch (include/aggfly_hip.h).
//
// A plan is built by the host-only planner (afhip_planner.cpp: build_plan — column lowering, kernel variant, chunk table,
// workspace sizes); afhip_plan_create here hands it the device's facts and uploads the tables it made.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/aggfly_hip.h"
#include "afhip_kernels.h"
#include "afhip_panel_kernels.h"
#include "afhip_lz4_kernels.h"
#include "afhip_lz4_encode_kernels.h"
#include "afhip_zstd_encode_kernels.h"
#include "afhip_zstd_kernels.h"
#include "afhip_inflate_kernels.h"
#include "afhip_grib_kernels.h"
#include "afhip_tiff_kernels.h"
#include "afhip_filter_kernels.h"
#include "afhip_planner.h"
#include "afhip_variants.h"
#include "afhip_sine_p2_table.h"

using namespace afhip;

namespace {

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess)                                                               \
            return fail(AFHIP_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                        __FILE__, __LINE__);                                                 \
    } while (0)

// ---- per-device state ----
// A handle (CSR, plan) belongs to the device that was current when it was created; every entry point that allocates or
// launches for a handle makes that device current for the duration of the call (DeviceGuard) — a caller's worker thread
// starts on device 0 whatever device its parent thread had selected (the reference runs its kernels from dask's pool,
// aggfly/aggregate/nb_kernels.py:271-305), and with one process per GPU on an 8-GPU node rank r's tables must live on card r.
constexpr int MAX_DEVICES = 64;
struct DevState {
    int cus = -1;                  // compute units (hipDeviceProp_t::multiProcessorCount)
    double* sine_tab = nullptr;    // acos table of the sine_dd closed forms (afhip_sine.h: sine_theta), uploaded on first use
    double* sine_p2 = nullptr;     // P2 table of the pair-mode arc (afhip_sine.h: sine_pair_g; afhip_sine_p2_table.h), uploaded on first use
};
DevState g_dev[MAX_DEVICES];
std::mutex g_dev_mu;

int current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return dev;
}

int cu_count(int dev) {
    if (dev < 0 || dev >= MAX_DEVICES) return 256;
    std::lock_guard<std::mutex> lk(g_dev_mu);
    DevState& d = g_dev[dev];
    if (d.cus < 0) {
        hipDeviceProp_t p;
        d.cus = (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256;
    }
    return d.cus;
}

// Makes `dev` the calling thread's current device and puts the previous one back on scope exit.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
        if (dev >= 0 && dev != prev) {
            err = hipSetDevice(dev);
            switched = err == hipSuccess;
        }
    }
    ~DeviceGuard() { if (switched && prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define GUARD_DEVICE(dev)                                                                                  \
    DeviceGuard guard__(dev);                                                                              \
    if (guard__.err != hipSuccess)                                                                         \
        return fail(AFHIP_E_HIP, "hipSetDevice(%d) failed: %s", (int)(dev), hipGetErrorString(guard__.err))

// Device that owns a device pointer (-1: not a device allocation the runtime knows, e.g. NULL or host memory).
int pointer_device(const void* p) {
    if (!p) return -1;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
    if (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged) return -1;
    return at.device;
}

// The acos table of sine_theta (afhip_sine.h), in the layout the kernel copies into LDS: SINE_ROWS pairs of rows
// (C, S, TH, 0); pair k belongs to phi_k = asin(k / 256):
//   row 2k     (a <= g: theta = pi/2 - asin(u)):  (-cos phi_k, +sin phi_k, pi/2 - phi_k)
//   row 2k + 1 (a >  g: theta = asin(u)):         (+cos phi_k, -sin phi_k, phi_k)
std::vector<double> sine_table_host() {
    std::vector<double> t((size_t)2 * SINE_ROWS * 4, 0.0);
    for (int k = 0; k < SINE_ROWS; ++k) {
        const double sn = std::min(1.0, (double)k / (double)SINE_SCALE);
        const double cs = std::sqrt((1.0 - sn) * (1.0 + sn));
        const double phi = std::asin(sn);
        double* lo = &t[(size_t)(2 * k) * 4];               // the two cases of a k sit next to each other (sine_theta's row address)
        double* hi = &t[(size_t)(2 * k + 1) * 4];
        lo[0] = -cs; lo[1] = sn; lo[2] = 1.57079632679489661923 - phi;
        hi[0] = cs; hi[1] = -sn; hi[2] = phi;
    }
    return t;
}

// pair = true: the P2 table of the pair-mode arc; false: the acos table.  Each lives as long as the process (8 / 11.5 KB per device).
int sine_table_dev(int dev, bool pair, const double** out) {
    *out = nullptr;
    if (dev < 0 || dev >= MAX_DEVICES) return fail(AFHIP_E_INVALID, "device %d out of range", dev);
    std::lock_guard<std::mutex> lk(g_dev_mu);
    DevState& d = g_dev[dev];
    double*& slot = pair ? d.sine_p2 : d.sine_tab;
    if (!slot) {
        std::vector<double> h;
        if (pair) {
            static_assert(AFHIP_SINE_P2_N == SINE_P2_N && SINE_P2_BYTES >= (SINE_P2_N + 1) * 4 * (int)sizeof(double), "table layout");
            h.assign(SINE_P2_BYTES / sizeof(double), 0.0);
            std::copy(afhip_sine_p2_table, afhip_sine_p2_table + (SINE_P2_N + 1) * 4, h.begin());
        } else {
            static_assert(SINE_TAB_BYTES == 2 * SINE_ROWS * 4 * sizeof(double), "table layout");
            h = sine_table_host();
        }
        double* p = nullptr;
        HIP_TRY(hipMalloc((void**)&p, h.size() * sizeof(double)));
        hipError_t e = hipMemcpy(p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(p); return fail(AFHIP_E_HIP, "sine table upload failed: %s", hipGetErrorString(e)); }
        slot = p;
    }
    *out = slot;
    return AFHIP_OK;
}

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int upload(const std::vector<T>& h) {
        if (p) { (void)hipFree(p); p = nullptr; }
        n = h.size();
        size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        HIP_TRY(hipMalloc((void**)&p, bytes));
        if (n) HIP_TRY(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
        return AFHIP_OK;
    }
};

}  // namespace

// Long rows (more than four segment lengths) are cut into segments that are summed by separate threads / waves and then added in row order
// (k_csr_combine_segments): real admin-2 tables span four decades of row lengths, and one lane walking a 10^5-entry row
// alone would be the whole kernel's tail.  The segment length follows the table: ~nnz / 4096 entries (64 .. 1024, a
// multiple of 64), so that a table dominated by a few huge rows still spreads over the chip (a 55 k-entry table whose
// longest row holds 19 k: 21.1 ms serial, 1.5 ms in 1024-entry segments, profiles/r02_spmm_skew.txt), while the rows of an
// ordinary table (hundreds of entries) stay whole; a row is cut into at most 128 pieces (the combine adds them serially).
// exact_order plans never segment (table order, one running sum).
constexpr int64_t SPMM_SEG_MIN = 64, SPMM_SEG_MAX = 1024, SPMM_TARGET_SEGS = 4096, SPMM_MAX_PIECES = 128;

struct afhip_csr {
    int device = 0;                // the device the tables live on (current device at afhip_csr_create)
    int64_t R = 0, nnz = 0, n_cells = 0, max_row = 0;
    DevBuf<int64_t> indptr;
    DevBuf<int32_t> cols;
    DevBuf<double> w;
    // work list of the default (non-exact) route: segment v = entries [seg_ptr[v], seg_ptr[v+1]) of one row; its sums go
    // to row seg_dst[v] of the sums buffer: the region's own row (an unsplit region) or scratch row R + k (a piece)
    int64_t nseg = 0, n_extra = 0, n_split = 0;
    DevBuf<int64_t> seg_ptr;
    DevBuf<int32_t> seg_dst;
    DevBuf<int32_t> split_row;      // [n_split] regions that were cut
    DevBuf<int32_t> split_ptr;      // [n_split + 1] their pieces: scratch rows R + [split_ptr[i], split_ptr[i+1])
    // host copies of the table (the run tables of the region-fused period ends are built from them on first use)
    std::vector<int64_t> h_indptr;
    std::vector<int32_t> h_cols;
    std::vector<double> h_w;
    // Region-fused period ends (FusedArgs::rf_w): per wave-tile size (64 * vec cells) the runs of consecutive cells whose e-th table
    // entry (e = 0, 1, in table order) names the same region; the third, fourth ... entries of a cell (junctions of polygons) are kept
    // as "extras" by region.  ok = false: the tables could not be built (no runs at all, or an upload failed).
    struct RfTab {
        bool built = false, ok = false;
        int64_t n_runs = 0;
        DevBuf<double> w2;            // [n_cells][2]
        DevBuf<uint32_t> lane;        // [wave tiles * 64][2] per lane slot: {scan / start / end bits, run indices} (k_fused_temporal: rfbits, rfrid)
        DevBuf<int32_t> tile;         // [wave tiles][2][2]: {first run, need mask} of entry e
        DevBuf<int64_t> reg_ptr;      // [R + 1]
        DevBuf<int32_t> reg_runs;     // [n_runs] run ids by region, ascending inside a region
        // cells in three or more regions: their entries beyond the second ("extras"), by region in table order
        int64_t n_xcells = 0;
        DevBuf<int32_t> xidx;         // [n_cells] index among the cells with extras, -1 = none (empty when the table has none)
        DevBuf<int64_t> xreg_ptr;     // [R + 1]
        DevBuf<int32_t> xcell;        // [extras] index of the entry's cell among the cells with extras
        DevBuf<double> xw;            // [extras]
    };
    RfTab rf[3];                    // vec = 1, 2, 4
    std::mutex rf_mu;
};

// Builds (once) the run tables for wave tiles of 64 * vec cells.  Returns the table, or nullptr when the route does not apply.
static afhip_csr::RfTab* rf_table(afhip_csr* csr, int vec) {
    const int slot = vec == 1 ? 0 : (vec == 2 ? 1 : -1);      // (the twins hold one or two cells per lane)
    if (slot < 0) return nullptr;
    std::lock_guard<std::mutex> lk(csr->rf_mu);
    afhip_csr::RfTab& t = csr->rf[slot];
    if (t.built) return t.ok ? &t : nullptr;
    t.built = true;
    const int64_t C = csr->n_cells, R = csr->R, tc = (int64_t)64 * vec, nt = (C + tc - 1) / tc;
    std::vector<int32_t> reg((size_t)C * 2, -1);
    std::vector<double> w2((size_t)C * 2, 0.0);
    std::vector<int32_t> xidx, xcell;
    std::vector<int64_t> xreg_ptr((size_t)R + 1, 0);
    std::vector<double> xw;
    for (int64_t r = 0; r < R; ++r) {
        for (int64_t j = csr->h_indptr[(size_t)r]; j < csr->h_indptr[(size_t)r + 1]; ++j) {
            const size_t c = (size_t)csr->h_cols[(size_t)j];
            const int e = reg[2 * c] < 0 ? 0 : (reg[2 * c + 1] < 0 ? 1 : 2);
            if (e == 2) {                                            // a third (fourth ...) region on this cell: an extra of region r
                if (xidx.empty()) xidx.assign((size_t)C, -1);
                if (xidx[c] < 0) xidx[c] = (int32_t)t.n_xcells++;
                xcell.push_back(xidx[c]); xw.push_back(csr->h_w[(size_t)j]);
                continue;
            }
            reg[2 * c + e] = (int32_t)r; w2[2 * c + e] = csr->h_w[(size_t)j];
        }
        xreg_ptr[(size_t)r + 1] = (int64_t)xcell.size();
    }
    // (+ 4 empty tiles: the waves of the last workgroup that start beyond the grid look their tile up too)
    // Runs of a tile, numbered in cell order (a run starts where the region changes to one, or at the tile's first cell), and — per lane
    // slot — how the segmented scan of the period end proceeds (k_fused_temporal: rfbits / rfrid / rf_need).  A lane holds `vec`
    // consecutive cells; a cell without an entry e is a stretch of its own, so the scan never adds across the gaps between runs and
    // the steps a wave needs follow its longest RUN.
    std::vector<int32_t> tile((size_t)(nt + 4) * 4, 0), run_region;
    std::vector<uint32_t> lanew((size_t)(nt + 4) * 64 * 2, 0u);
    for (int64_t ti = 0; ti < nt; ++ti)
        for (int e = 0; e < 2; ++e) {
            const int64_t c_lo = ti * tc;
            const int first = (int)run_region.size();
            auto key_of = [&](int64_t c) -> int32_t { return c < C ? reg[(size_t)(2 * c + e)] : -1; };
            bool F[64];
            uint32_t bits[64], rid[64];
            int n_at = 0;
            for (int l = 0; l < 64; ++l) {
                bits[l] = 0; rid[l] = 0; F[l] = false;
                for (int i = 0; i < vec; ++i) {
                    const int64_t c = c_lo + (int64_t)l * vec + i;
                    const int32_t k = key_of(c);
                    const bool first_cell = l == 0 && i == 0, last_cell = l == 63 && i == vec - 1;
                    const bool bnd = first_cell || k != key_of(c - 1) || k < 0;
                    const bool endc = last_cell || key_of(c + 1) != k;
                    if (bnd && k >= 0) { run_region.push_back(k); ++n_at; }
                    rid[l] |= (uint32_t)((n_at - 1) & 0xff) << (8 * i);
                    bits[l] |= (bnd ? 1u : 0u) << (6 + i);
                    bits[l] |= ((endc && k >= 0) ? 1u : 0u) << (8 + i);
                    F[l] = F[l] || bnd;
                }
            }
            int need = n_at > 0 ? 128 : 0;
            // the lane a step reads (k_fused_temporal: dpp64): steps 0 - 3 the lane 1, 2, 4, 8 to the left inside its row of 16; step 4
            // the last lane of the row before (rows 1 and 3); step 5 lane 31 (rows 2 and 3).
            auto src_of = [](int st, int l) -> int {
                if (st < 4) return (l & 15) >= (1 << st) ? l - (1 << st) : -1;
                if (st == 4) return ((l >> 4) & 1) ? (l & ~15) - 1 : -1;
                return l >= 32 ? 31 : -1;
            };
            for (int st = 0; st < 6; ++st) {
                bool Fn[64];
                for (int l = 0; l < 64; ++l) {
                    const int sl = src_of(st, l);
                    if (sl >= 0 && !F[l]) { bits[l] |= 1u << st; need |= 1 << st; }
                    Fn[l] = F[l] || (sl >= 0 && F[sl]);
                }
                for (int l = 0; l < 64; ++l) F[l] = Fn[l];
            }
            for (int l = 0; l < 64; ++l) {
                if (vec == 2 && ((bits[l] >> 8) & 1u)) need |= 64;
                lanew[(size_t)(ti * 64 + l) * 2] |= bits[l] << (16 * e);
                lanew[(size_t)(ti * 64 + l) * 2 + 1] |= rid[l] << (16 * e);
            }
            tile[(size_t)(ti * 2 + e) * 2] = first;
            tile[(size_t)(ti * 2 + e) * 2 + 1] = need;
        }
    t.n_runs = (int64_t)run_region.size();
    if (t.n_runs == 0 || t.n_runs > INT32_MAX) return nullptr;
    // (no condition on how short the runs are: the route measured ahead down to regions of five cells — monthly f64 3.65 against 3.95 ms
    // with 60,000 regions on 215 x 1440 —; afhip_plan_run only checks that the run sums fit the area of the per-cell values)
    std::vector<int64_t> reg_ptr((size_t)R + 1, 0);
    for (int32_t r : run_region) ++reg_ptr[(size_t)r + 1];
    for (int64_t r = 0; r < R; ++r) reg_ptr[(size_t)r + 1] += reg_ptr[(size_t)r];
    std::vector<int32_t> reg_runs((size_t)t.n_runs);
    { std::vector<int64_t> at(reg_ptr.begin(), reg_ptr.end() - 1);
      for (int64_t q = 0; q < t.n_runs; ++q) reg_runs[(size_t)at[(size_t)run_region[(size_t)q]]++] = (int32_t)q; }
    DeviceGuard g(csr->device);
    if (t.lane.upload(lanew) || t.w2.upload(w2) || t.tile.upload(tile) || t.reg_ptr.upload(reg_ptr) || t.reg_runs.upload(reg_runs)) return nullptr;
    if (t.n_xcells && (t.xidx.upload(xidx) || t.xreg_ptr.upload(xreg_ptr) || t.xcell.upload(xcell) || t.xw.upload(xw))) return nullptr;
    t.ok = true;
    return &t;
}

struct afhip_plan : PlanLayout {             // what the planner made (afhip_planner.h) + device tables, scratch and run state
    int device = 0;                       // the device the plan's tables and scratch live on (current device at afhip_plan_create)
    int last_route = 0;                    // 1: the last afhip_plan_run took the region-fused route (afhip_plan_describe tells)
    int last_spatial = 0;                  // the last run's per-cell route: 1 = slot gather (k_csr_spmm_slots), 2 = cell-major panel + k_csr_spmm* (likewise)
    int last_counts_lanes = -1;            // lanes per (row, period) pair of the last run's packed-count gather (1, 4, 8, 16; -1: it did not run)
    // device tables
    DevBuf<int64_t> d_ob;
    DevBuf<int64_t> d_gtab;
    DevBuf<ChunkDesc> d_chunks;
    DevBuf<int32_t> d_slot_ptr;
    DevBuf<uint8_t> d_cmap;                 // the cell map of a FEAT_CELL_MAP plan (256 bytes; FusedArgs::hb_cmap)
    // workspace
    void* own_ws = nullptr;                 // plan-owned scratch (callers that hand no workspace): grown by a new hipMalloc, the
    int64_t own_ws_bytes = 0;               // outgrown block is `retired` until the plan is destroyed — no hipFree (a device-wide
    std::vector<void*> retired;             // synchronisation) ever sits on the run path
    double* sums = nullptr;                 // [rows][P][K + 1] of the current run: behind partial + panel in the run's workspace
    PackArgs unpack{};                      // AFHIP_I16 / AFHIP_U16 plans: the unpack rule (afhip_plan_bind_packing; of several rules the first)
    bool unpack_bound = false;
    // several rules (afhip_plan_bind_packings, n > 1): a bind only writes the host copy below.  The device table — bounds [n + 1], then
    // rules [n] — is written by the NEXT run, by a copy ordered on that run's stream in front of its kernel, and only when it differs from
    // what the table holds: a launch that is still running keeps reading the rules it was launched with.  The table grows by a new
    // hipMalloc, the outgrown block is `retired` like the workspace's.
    std::vector<PackArgs> rules;            // n > 1: the bound rules; empty: one rule (`unpack`)
    std::vector<int64_t> rule_bounds;
    std::vector<unsigned char> rules_dev_image, rules_stage;   // what the device table holds / the bytes of the copy in flight
    void* d_rules = nullptr;
    size_t d_rules_bytes = 0;
    hipEvent_t rules_ev = nullptr;          // recorded behind the table's copy: the next copy waits for it before it rewrites rules_stage
    int last_ws = 0;                        // 1: the last run used a caller-owned workspace, 2: plan-owned (afhip_plan_describe tells)
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    // per-launch profiling ring (afhip_plan_profile_*): event pairs around the temporal kernel
    std::vector<hipEvent_t> prof_ev;
    int64_t prof_count = 0;
    ~afhip_plan() {      // run with `device` current (afhip_plan_destroy): the members below free their buffers after this body
        if (own_ws) (void)hipFree(own_ws);
        if (d_rules) (void)hipFree(d_rules);
        if (rules_ev) (void)hipEventDestroy(rules_ev);
        for (void* q : retired) (void)hipFree(q);
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
        for (auto& e : prof_ev) if (e) (void)hipEventDestroy(e);
    }
};

// ---------------------------------------------------------------------------------------
// misc
// ---------------------------------------------------------------------------------------
extern "C" const char* afhip_last_error(void) { return last_error(); }
extern "C" int afhip_abi_version(void) { return AFHIP_ABI_VERSION; }

extern "C" int afhip_build_info(char* buf, int buf_len) {
    int count[MENU_COUNT], arms = 0, rf = 0;
    for (int m = 0; m < MENU_COUNT; ++m) (void)menu_table((Menu)m, &count[m]);
    int n = 0;
    const Variant* tab = menu_table(MENU_FLOAT, &n);
    for (int i = 0; i < n; ++i) { arms += tab[i].production ? 0 : 1; rf += tab[i].rf() ? 1 : 0; }
    char tmp[240];
    const int len = snprintf(tmp, sizeof tmp, "menu=%s variants=%d arms=%d region_fused_twins=%d abi=%d packed_variants=%d packed_hist_variants=%d end_bins_variants=%d",
                             variants_menu(), n, arms, rf, AFHIP_ABI_VERSION, count[MENU_PACKED], count[MENU_PACKED_HIST], count[MENU_END_BINS]);
    if (buf && buf_len > 0) snprintf(buf, buf_len, "%s", tmp);
    return len + 1;
}

// the menus by their keys in gen_variants.py's MENUS
extern "C" int afhip_menu_size(const char* key) {
    for (int m = 0; key && m < MENU_COUNT; ++m) {
        if (strcmp(key, menu_key((Menu)m)) != 0) continue;
        int n = 0;
        (void)menu_table((Menu)m, &n);
        return n;
    }
    return -1;
}

extern "C" int afhip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

extern "C" int afhip_device_info(int dev, char* name, int name_len, char* arch, int arch_len,
                                 int* n_cus, int64_t* hbm_bytes) {
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, dev));
    if (name && name_len > 0) snprintf(name, name_len, "%s", p.name);
    if (arch && arch_len > 0) snprintf(arch, arch_len, "%s", p.gcnArchName);
    if (n_cus) *n_cus = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
    return AFHIP_OK;
}

// ---------------------------------------------------------------------------------------
// CSR
// ---------------------------------------------------------------------------------------
extern "C" int afhip_csr_create(const int64_t* indptr, const int64_t* cols, const double* w,
                                int64_t R, int64_t nnz, int64_t n_cells, afhip_csr** out) {
    if (!out) return fail(AFHIP_E_INVALID, "csr_create: out is NULL");
    *out = nullptr;
    if (R < 0 || nnz < 0 || n_cells <= 0 || !indptr || (nnz && (!cols || !w)))
        return fail(AFHIP_E_INVALID, "csr_create: bad sizes/pointers (R=%lld nnz=%lld n_cells=%lld)",
                    (long long)R, (long long)nnz, (long long)n_cells);
    if (n_cells > INT32_MAX) return fail(AFHIP_E_INVALID, "csr_create: n_cells exceeds int32");
    if (indptr[0] != 0 || indptr[R] != nnz) return fail(AFHIP_E_INVALID, "csr_create: indptr[0] != 0 or indptr[R] != nnz");
    for (int64_t r = 0; r < R; ++r)
        if (indptr[r + 1] < indptr[r]) return fail(AFHIP_E_INVALID, "csr_create: indptr not monotone at row %lld", (long long)r);
    std::vector<int32_t> c32((size_t)nnz);
    for (int64_t j = 0; j < nnz; ++j) {
        if (cols[j] < 0 || cols[j] >= n_cells)
            return fail(AFHIP_E_INVALID, "csr_create: column %lld out of range at entry %lld", (long long)cols[j], (long long)j);
        c32[(size_t)j] = (int32_t)cols[j];
        // (a NaN or infinite weight: np.add.at then turns every sum of the region into NaN through w * 0 of the cells that are not valid,
        // empty periods included, while the routes here add nothing for a period without steps — not a table the sums are defined for)
        if (!std::isfinite(w[j])) return fail(AFHIP_E_INVALID, "csr_create: weight at entry %lld is not finite", (long long)j);
    }
    auto* h = new afhip_csr();
    h->device = current_device();
    h->R = R; h->nnz = nnz; h->n_cells = n_cells;
    h->h_indptr.assign(indptr, indptr + R + 1); h->h_cols = c32; h->h_w.assign(w, w + nnz);
    std::vector<int64_t> seg_ptr;
    std::vector<int32_t> seg_dst, split_row, split_ptr(1, 0);
    seg_ptr.reserve((size_t)R + 1); seg_dst.reserve((size_t)R);
    auto up64 = [](int64_t x) { return (x + 63) / 64 * 64; };
    int64_t seg = std::min(SPMM_SEG_MAX, std::max(SPMM_SEG_MIN, up64(nnz / SPMM_TARGET_SEGS)));
    if (const char* e = getenv("AFHIP_SPMM_SEG")) seg = std::max<int64_t>(64, up64(atoll(e)));      // experiment knob
    for (int64_t r = 0; r < R; ++r) {
        const int64_t j0 = indptr[r], j1 = indptr[r + 1], len = j1 - j0;
        h->max_row = std::max(h->max_row, len);
        // (rows up to four segments long stay whole: cutting a 150-entry county in two bought nothing and cost every step of an
        // annual panel a segment-merge launch and, with it, the divide fused into the gather)
        if (len <= 4 * seg) {
            seg_ptr.push_back(j0); seg_dst.push_back((int32_t)r);
        } else {
            const int64_t want = std::min(SPMM_MAX_PIECES, (len + seg - 1) / seg);
            const int64_t piece = up64((len + want - 1) / want);
            const int64_t pieces = (len + piece - 1) / piece;
            for (int64_t i = 0; i < pieces; ++i) {
                seg_ptr.push_back(j0 + i * piece);
                seg_dst.push_back((int32_t)(R + h->n_extra + i));
            }
            h->n_extra += pieces;
            split_row.push_back((int32_t)r);
            split_ptr.push_back((int32_t)h->n_extra);
        }
    }
    seg_ptr.push_back(nnz);
    h->nseg = (int64_t)seg_dst.size(); h->n_split = (int64_t)split_row.size();
    if (R + h->n_extra > INT32_MAX) { delete h; return fail(AFHIP_E_INVALID, "csr_create: too many rows"); }
    int rc;
    if ((rc = h->indptr.upload(std::vector<int64_t>(indptr, indptr + R + 1))) ||
        (rc = h->cols.upload(c32)) ||
        (rc = h->w.upload(std::vector<double>(w, w + nnz))) ||
        (rc = h->seg_ptr.upload(seg_ptr)) || (rc = h->seg_dst.upload(seg_dst)) ||
        (rc = h->split_row.upload(split_row)) || (rc = h->split_ptr.upload(split_ptr))) {
        delete h;
        return rc;
    }
    *out = h;
    return AFHIP_OK;
}

extern "C" void afhip_csr_destroy(afhip_csr* csr) {
    if (!csr) return;
    DeviceGuard g(csr->device);
    delete csr;
}

extern "C" int afhip_csr_device(const afhip_csr* csr) { return csr ? csr->device : -1; }

// AGGFLY_HIP_EXACT_ORDER=1 (read once): the standalone spatial entry points then sum in table order like the plans
// created with exact_order.  AFHIP_SPMM_SERIAL=1 (experiment knob): the serial kernel for every route.
static bool env_flag(const char* name) { const char* e = getenv(name); return e && atoi(e) != 0; }
static bool spmm_serial_env() { static const bool v = env_flag("AFHIP_SPMM_SERIAL") || env_flag("AGGFLY_HIP_EXACT_ORDER"); return v; }

static int64_t spmm_rows(const afhip_csr* csr);

// out[r][q] = sum_j w[j] * X[col[j]][q] for every region r (rows [0, R) of `out`, which holds spmm_rows(csr) x Q doubles).
//   exact:  one thread per (r, q) walks the whole row in table order — bit-identical to np.add.at (spatial.py:185);
//   else:   rows in segments of <= SPMM_SEG entries; Q <= 16: one WAVE per segment, lanes stride over the entries and a fixed
//           butterfly adds the 64 partial sums (deterministic, not table order: ~1e-16 from the serial sum); Q > 16: one
//           thread per (segment, q); the pieces of a cut row are then added in row order.
static int launch_spmm(const afhip_csr* csr, const double* X, double* out, int64_t Q, hipStream_t st, bool exact) {
    if (csr->R * Q == 0) return AFHIP_OK;
    if (exact || spmm_serial_env()) {
        const int64_t n = csr->R * Q;
        hipLaunchKernelGGL(k_csr_spmm, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, st, csr->indptr.p, (const int32_t*)nullptr,
                           csr->cols.p, csr->w.p, X, out, csr->R, Q);
        HIP_TRY(hipGetLastError());
        return AFHIP_OK;
    }
    if (Q <= 16) {
        const unsigned blocks = (unsigned)((csr->nseg + (WG / 64) - 1) / (WG / 64));      // one wave per segment
        if (Q <= 2) hipLaunchKernelGGL(k_csr_spmm_wave<2>, dim3(blocks), dim3(WG), 0, st, csr->seg_ptr.p, csr->seg_dst.p, csr->cols.p, csr->w.p, X, out, csr->nseg, (int)Q);
        else if (Q <= 4) hipLaunchKernelGGL(k_csr_spmm_wave<4>, dim3(blocks), dim3(WG), 0, st, csr->seg_ptr.p, csr->seg_dst.p, csr->cols.p, csr->w.p, X, out, csr->nseg, (int)Q);
        else if (Q <= 8) hipLaunchKernelGGL(k_csr_spmm_wave<8>, dim3(blocks), dim3(WG), 0, st, csr->seg_ptr.p, csr->seg_dst.p, csr->cols.p, csr->w.p, X, out, csr->nseg, (int)Q);
        else hipLaunchKernelGGL(k_csr_spmm_wave<16>, dim3(blocks), dim3(WG), 0, st, csr->seg_ptr.p, csr->seg_dst.p, csr->cols.p, csr->w.p, X, out, csr->nseg, (int)Q);
    } else {
        const int64_t n = csr->nseg * Q;
        hipLaunchKernelGGL(k_csr_spmm, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, st, csr->seg_ptr.p, csr->seg_dst.p,
                           csr->cols.p, csr->w.p, X, out, csr->nseg, Q);
    }
    HIP_TRY(hipGetLastError());
    if (csr->n_split) {
        const int64_t n = csr->n_split * Q;
        hipLaunchKernelGGL(k_csr_combine_segments, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, st, out, csr->split_row.p,
                           csr->split_ptr.p, csr->R, Q, csr->n_split);
        HIP_TRY(hipGetLastError());
    }
    return AFHIP_OK;
}

extern "C" int afhip_scatter_block(const afhip_csr* csr, const double* block_dev, int64_t nt,
                                   double* out_dev, void* stream) {
    if (!csr || !block_dev || !out_dev || nt < 0) return fail(AFHIP_E_INVALID, "scatter_block: bad arguments");
    GUARD_DEVICE(csr->device);
    // the drop-in for _scatter_block: always the table-order sum (out_dev holds exactly R rows)
    return launch_spmm(csr, block_dev, out_dev, nt, (hipStream_t)stream, true);
}

// afhip_place_box and afhip_place_box_swapped: one set of bounds checks, one launch shape; `who` names the entry in its errors
template <bool SWAPPED>
static int place_box_launch(const char* who, const void* chunk_dev, void* cube_dev, int elem_size,
                            int64_t by, int64_t bx, int64_t st, int64_t sy, int64_t sx,
                            int64_t nt, int64_t ny, int64_t nx,
                            int64_t NY, int64_t NX, int64_t t0, int64_t y0, int64_t x0, void* stream) {
    if (!chunk_dev || !cube_dev || by <= 0 || bx <= 0 || NY <= 0 || NX <= 0 || nt < 0 || ny < 0 || nx < 0 ||
        st < 0 || sy < 0 || sx < 0 || t0 < 0 || y0 < 0 || x0 < 0 || sy + ny > by || sx + nx > bx || y0 + ny > NY || x0 + nx > NX)
        return fail(AFHIP_E_INVALID, "%s: box outside the chunk or the cube", who);
    const int64_t n = nt * ny * nx;
    if (n == 0) return AFHIP_OK;
    if (n > (int64_t)0x7fffffff * WG) return fail(AFHIP_E_INVALID, "%s: box too large for one launch", who);
    if (elem_size != 2 && elem_size != 4 && elem_size != 8) return fail(AFHIP_E_INVALID, "%s: elem_size must be 2, 4 or 8", who);
    GUARD_DEVICE(pointer_device(cube_dev));
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((n + WG - 1) / WG)), block(WG);
#define PLACE_BOX_AS(TE)                                                                                                          \
    do {                                                                                                                          \
        if (SWAPPED) hipLaunchKernelGGL(k_place_box_swapped<TE>, grid, block, 0, s, (const TE*)chunk_dev, (TE*)cube_dev, by, bx, st, sy, sx, nt, ny, nx, NY, NX, t0, y0, x0); \
        else hipLaunchKernelGGL(k_place_box<TE>, grid, block, 0, s, (const TE*)chunk_dev, (TE*)cube_dev, by, bx, st, sy, sx, nt, ny, nx, NY, NX, t0, y0, x0); \
    } while (0)
    switch (elem_size) {
        case 2: PLACE_BOX_AS(uint16_t); break;
        case 4: PLACE_BOX_AS(uint32_t); break;
        default: PLACE_BOX_AS(uint64_t); break;
    }
#undef PLACE_BOX_AS
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int afhip_place_box(const void* chunk_dev, void* cube_dev, int elem_size,
                               int64_t by, int64_t bx, int64_t st, int64_t sy, int64_t sx,
                               int64_t nt, int64_t ny, int64_t nx,
                               int64_t NY, int64_t NX, int64_t t0, int64_t y0, int64_t x0, void* stream) {
    return place_box_launch<false>("place_box", chunk_dev, cube_dev, elem_size, by, bx, st, sy, sx, nt, ny, nx, NY, NX, t0, y0, x0, stream);
}

extern "C" int afhip_place_box_swapped(const void* block_dev, void* cube_dev, int elem_size,
                                       int64_t by, int64_t bx, int64_t st, int64_t sy, int64_t sx,
                                       int64_t nt, int64_t ny, int64_t nx,
                                       int64_t NY, int64_t NX, int64_t t0, int64_t y0, int64_t x0, void* stream) {
    return place_box_launch<true>("place_box_swapped", block_dev, cube_dev, elem_size, by, bx, st, sy, sx, nt, ny, nx, NY, NX, t0, y0, x0, stream);
}

// afhip_place_box_tlast: the checks of place_box_launch, and the chunk's time extent too (bt is a parameter here)
extern "C" int afhip_place_box_tlast(const void* chunk_dev, void* cube_dev, int elem_size,
                                     int64_t by, int64_t bx, int64_t bt, int64_t sy, int64_t sx, int64_t st,
                                     int64_t ny, int64_t nx, int64_t nt,
                                     int64_t NY, int64_t NX, int64_t t0, int64_t y0, int64_t x0, void* stream) {
    if (!chunk_dev || !cube_dev || by <= 0 || bx <= 0 || bt <= 0 || NY <= 0 || NX <= 0 || nt < 0 || ny < 0 || nx < 0 ||
        st < 0 || sy < 0 || sx < 0 || t0 < 0 || y0 < 0 || x0 < 0 || sy + ny > by || sx + nx > bx || st + nt > bt || y0 + ny > NY || x0 + nx > NX)
        return fail(AFHIP_E_INVALID, "place_box_tlast: box outside the chunk or the cube");
    if (nt * ny * nx == 0) return AFHIP_OK;
    const int64_t tiles_x = (nx + TLAST_TILE - 1) / TLAST_TILE, tiles_t = (nt + TLAST_TILE - 1) / TLAST_TILE;
    if (tiles_x > 0x7fffffff || tiles_t > 0x7fffffff || tiles_x * tiles_t > 0x7fffffff || ny * tiles_x * tiles_t > 0x7fffffff)
        return fail(AFHIP_E_INVALID, "place_box_tlast: box too large for one launch");
    if (elem_size != 2 && elem_size != 4 && elem_size != 8) return fail(AFHIP_E_INVALID, "place_box_tlast: elem_size must be 2, 4 or 8");
    GUARD_DEVICE(pointer_device(cube_dev));
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(ny * tiles_x * tiles_t)), block(WG);
#define PLACE_TLAST_AS(TE)                                                                                                        \
    hipLaunchKernelGGL(k_place_box_tlast<TE>, grid, block, 0, s, (const TE*)chunk_dev, (TE*)cube_dev, bx, bt, sy, sx, st, ny, nx, nt, \
                       NY, NX, t0, y0, x0, tiles_x, tiles_t)
    switch (elem_size) {
        case 2: PLACE_TLAST_AS(uint16_t); break;
        case 4: PLACE_TLAST_AS(uint32_t); break;
        default: PLACE_TLAST_AS(uint64_t); break;
    }
#undef PLACE_TLAST_AS
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

// ---- numcodecs element filters undone in HBM (afhip_filter_kernels.h) ----
// The number of tile sums a call needs, or -1: what afhip_delta_decode refuses (sizes, an overflow, a launch beyond the grid limit).
static int64_t delta_total_tiles(int64_t n_chunks, int64_t chunk_elems, int elem_size) {
    if (n_chunks < 0 || chunk_elems <= 0 || (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8)) return -1;
    if (n_chunks == 0) return 0;
    if (chunk_elems > INT64_MAX / elem_size / n_chunks) return -1;                       // n_chunks * chunk_elems * elem_size overflows
    const int64_t tiles = delta_tiles_per_chunk(chunk_elems, elem_size);
    if (n_chunks > 0x7fffffff || tiles > 0x7fffffff / n_chunks) return -1;               // one workgroup per tile: the grid limit
    return n_chunks * tiles;
}

extern "C" int64_t afhip_delta_scratch_bytes(int64_t n_chunks, int64_t chunk_elems, int elem_size) {
    const int64_t total = delta_total_tiles(n_chunks, chunk_elems, elem_size);
    if (total < 0) return -1;
    // (chunks of one tile need no sums; 16 bytes at least, so that a caller may always allocate what this says)
    const int64_t need = delta_tiles_per_chunk(chunk_elems, elem_size) > 1 ? total * elem_size : 0;
    return (need + 15) / 16 * 16 + 16;
}

template <typename T>
static void delta_launch(void* stage_dev, void* scratch_dev, int64_t n_chunks, int64_t chunk_elems, int64_t tiles, hipStream_t s) {
    // 16-byte accesses when every chunk begins on a 16-byte boundary
    const bool vec = (uintptr_t)stage_dev % 16 == 0 && (chunk_elems * (int64_t)sizeof(T)) % 16 == 0;
    const dim3 grid((unsigned)(n_chunks * tiles)), block(DELTA_WG);
    T* sums = tiles > 1 ? (T*)scratch_dev : nullptr;
    if (sums) {
        if (vec) hipLaunchKernelGGL((k_delta_tile_sums<T, true>), grid, block, 0, s, (const T*)stage_dev, sums, chunk_elems, tiles);
        else hipLaunchKernelGGL((k_delta_tile_sums<T, false>), grid, block, 0, s, (const T*)stage_dev, sums, chunk_elems, tiles);
        hipLaunchKernelGGL(k_delta_scan_sums<T>, dim3((unsigned)n_chunks), block, 0, s, sums, tiles);
    }
    if (vec) hipLaunchKernelGGL((k_delta_scan_tiles<T, true>), grid, block, 0, s, (T*)stage_dev, (const T*)sums, chunk_elems, tiles);
    else hipLaunchKernelGGL((k_delta_scan_tiles<T, false>), grid, block, 0, s, (T*)stage_dev, (const T*)sums, chunk_elems, tiles);
}

extern "C" int afhip_delta_decode(void* stage_dev, int64_t n_chunks, int64_t chunk_elems, int elem_size,
                                  void* scratch_dev, int64_t scratch_bytes, void* stream) {
    if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8)
        return fail(AFHIP_E_INVALID, "delta_decode: elem_size must be 1, 2, 4 or 8");
    if (n_chunks < 0 || chunk_elems <= 0) return fail(AFHIP_E_INVALID, "delta_decode: n_chunks < 0 or chunk_elems <= 0");
    const int64_t total = delta_total_tiles(n_chunks, chunk_elems, elem_size);
    if (total < 0) return fail(AFHIP_E_INVALID, "delta_decode: n_chunks * chunk_elems overflows or is too large for one launch");
    if (n_chunks == 0) return AFHIP_OK;
    if (!stage_dev || (uintptr_t)stage_dev % (uintptr_t)elem_size) return fail(AFHIP_E_INVALID, "delta_decode: stage_dev is null or not element-aligned");
    const int64_t tiles = delta_tiles_per_chunk(chunk_elems, elem_size);
    if (tiles > 1 && (!scratch_dev || (uintptr_t)scratch_dev % 8 || scratch_bytes < afhip_delta_scratch_bytes(n_chunks, chunk_elems, elem_size)))
        return fail(AFHIP_E_INVALID, "delta_decode: scratch_dev is null, not 8-byte aligned or smaller than afhip_delta_scratch_bytes says");
    GUARD_DEVICE(pointer_device(stage_dev));
    hipStream_t s = (hipStream_t)stream;
    switch (elem_size) {
        case 1: delta_launch<uint8_t>(stage_dev, scratch_dev, n_chunks, chunk_elems, tiles, s); break;
        case 2: delta_launch<uint16_t>(stage_dev, scratch_dev, n_chunks, chunk_elems, tiles, s); break;
        case 4: delta_launch<uint32_t>(stage_dev, scratch_dev, n_chunks, chunk_elems, tiles, s); break;
        default: delta_launch<uint64_t>(stage_dev, scratch_dev, n_chunks, chunk_elems, tiles, s); break;
    }
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

template <typename S, typename D>
static void fso_launch(const void* src_dev, void* dst_dev, int64_t n, double scale, double offset, hipStream_t s) {
    constexpr int V = 16 / (int)sizeof(D);
    constexpr uintptr_t src_align = sizeof(S) * V >= 16 ? 16 : sizeof(S) * V;
    const bool vec = (uintptr_t)src_dev % src_align == 0 && (uintptr_t)dst_dev % 16 == 0;
    const int64_t lanes = vec ? (n + V - 1) / V : n;
    const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
    if (vec) hipLaunchKernelGGL((k_fso_decode<S, D, true>), grid, block, 0, s, (const S*)src_dev, (D*)dst_dev, n, scale, offset);
    else hipLaunchKernelGGL((k_fso_decode<S, D, false>), grid, block, 0, s, (const S*)src_dev, (D*)dst_dev, n, scale, offset);
}

extern "C" int afhip_fso_decode(const void* src_dev, void* dst_dev, int64_t n, int src_type, int dst_type,
                                double scale, double offset, void* stream) {
    static const int size_of[8] = {1, 1, 2, 2, 4, 4, 4, 8};
    if (src_type < AFHIP_T_I8 || src_type > AFHIP_T_F64) return fail(AFHIP_E_INVALID, "fso_decode: src_type must be one of AFHIP_T_I8 ... AFHIP_T_F64");
    if (dst_type != AFHIP_T_F32 && dst_type != AFHIP_T_F64) return fail(AFHIP_E_INVALID, "fso_decode: dst_type must be AFHIP_T_F32 or AFHIP_T_F64");
    if (n < 0 || !(scale == scale) || scale == 0.0) return fail(AFHIP_E_INVALID, "fso_decode: n < 0, or a scale that is 0 or NaN");
    if (n == 0) return AFHIP_OK;
    if (n > (int64_t)0x7fffffff * 256) return fail(AFHIP_E_INVALID, "fso_decode: too many elements for one launch");
    if (!src_dev || !dst_dev || (uintptr_t)src_dev % (uintptr_t)size_of[src_type] || (uintptr_t)dst_dev % (uintptr_t)size_of[dst_type])
        return fail(AFHIP_E_INVALID, "fso_decode: a buffer is null or not element-aligned");
    const char *a = (const char*)src_dev, *b = (const char*)dst_dev;
    if (a < b + n * size_of[dst_type] && b < a + n * size_of[src_type]) return fail(AFHIP_E_INVALID, "fso_decode: src and dst overlap");
    GUARD_DEVICE(pointer_device(dst_dev));
    hipStream_t s = (hipStream_t)stream;
#define FSO_FROM(S)                                                                                         \
    do {                                                                                                    \
        if (dst_type == AFHIP_T_F32) fso_launch<S, float>(src_dev, dst_dev, n, scale, offset, s);           \
        else fso_launch<S, double>(src_dev, dst_dev, n, scale, offset, s);                                  \
    } while (0)
    switch (src_type) {
        case AFHIP_T_I8: FSO_FROM(int8_t); break;
        case AFHIP_T_U8: FSO_FROM(uint8_t); break;
        case AFHIP_T_I16: FSO_FROM(int16_t); break;
        case AFHIP_T_U16: FSO_FROM(uint16_t); break;
        case AFHIP_T_I32: FSO_FROM(int32_t); break;
        case AFHIP_T_U32: FSO_FROM(uint32_t); break;
        case AFHIP_T_F32: FSO_FROM(float); break;
        default: FSO_FROM(double); break;
    }
#undef FSO_FROM
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int64_t afhip_grib_rank_bytes(int64_t n_steps, int64_t n_points) {
    if (n_steps < 0 || n_points < 0 || n_points > 0x7fffffff) return -1;
    return n_steps * grib_rank_words(n_points) * (int64_t)sizeof(uint32_t);
}

extern "C" int afhip_grib_unpack(const void* stage_dev, int64_t stage_bytes, const afhip_grib_step* steps_dev, int64_t n_steps,
                                 int64_t NY, int64_t NX, int64_t y0, int64_t x0, int64_t ny, int64_t nx,
                                 void* cube_dev, int cube_elem_size, int64_t cube_nt, int64_t cube_NY, int64_t cube_NX,
                                 int64_t t0, int64_t cy, int64_t cx, void* rank_dev, int64_t rank_bytes, int32_t* errors_dev, void* stream) {
    static_assert(sizeof(afhip_grib_step) == sizeof(GribStep) && sizeof(GribStep) == 64, "record layouts");
    if (!stage_dev || !steps_dev || !cube_dev || !rank_dev || !errors_dev || stage_bytes < 0 || n_steps < 0)
        return fail(AFHIP_E_INVALID, "grib_unpack: bad arguments");
    if (cube_elem_size != 4) return fail(AFHIP_E_INVALID, "grib_unpack: the cube must be float32 (4-byte elements, got %d)", cube_elem_size);
    if (NY <= 0 || NX <= 0 || NY > 0x7fffffff / NX || y0 < 0 || x0 < 0 || ny < 0 || nx < 0 || ny > NY - y0 || nx > NX - x0)
        return fail(AFHIP_E_INVALID, "grib_unpack: box outside the grid");
    if (cube_nt < 0 || cube_NY <= 0 || cube_NX <= 0 || t0 < 0 || cy < 0 || cx < 0 || n_steps > cube_nt - t0 || ny > cube_NY - cy || nx > cube_NX - cx)
        return fail(AFHIP_E_INVALID, "grib_unpack: box outside the cube");
    if (stage_bytes & 3) return fail(AFHIP_E_INVALID, "grib_unpack: the stage must be a whole number of 4-byte words (%lld bytes)", (long long)stage_bytes);
    if (((uintptr_t)stage_dev & 3) || ((uintptr_t)cube_dev & 3) || ((uintptr_t)rank_dev & 3) || ((uintptr_t)steps_dev & 7))
        return fail(AFHIP_E_INVALID, "grib_unpack: the stage, the cube and the rank scratch must be 4-byte aligned, the records 8-byte aligned");
    if (rank_bytes < afhip_grib_rank_bytes(n_steps, NY * NX)) return fail(AFHIP_E_INVALID, "grib_unpack: rank scratch too small (afhip_grib_rank_bytes)");
    const int dev = pointer_device(cube_dev);
    if (dev < 0 || pointer_device(stage_dev) != dev || pointer_device(steps_dev) != dev || pointer_device(rank_dev) != dev || pointer_device(errors_dev) != dev)
        return fail(AFHIP_E_INVALID, "grib_unpack: the stage, the records, the scratch, the error counter and the cube must lie on one device");
    if (n_steps == 0 || ny == 0 || nx == 0) return AFHIP_OK;
    const int64_t lanes = n_steps * ny * ((nx + GRIB_RUN - 1) / GRIB_RUN);
    if (n_steps > 0x7fffffff || lanes > (int64_t)0x7fffffff * GRIB_WG) return fail(AFHIP_E_INVALID, "grib_unpack: box too large for one launch");
    GUARD_DEVICE(dev);
    hipStream_t s = (hipStream_t)stream;
    const GribBox g{NY, NX, y0, x0, ny, nx, cube_NY, cube_NX, t0, cy, cx};
    hipLaunchKernelGGL(k_grib_rank, dim3((unsigned)n_steps), dim3(GRIB_WG), 0, s, (const uint8_t*)stage_dev, stage_bytes, (const GribStep*)steps_dev, g,
                       (uint32_t*)rank_dev, errors_dev);
    hipLaunchKernelGGL(k_grib_unpack, dim3((unsigned)((lanes + GRIB_WG - 1) / GRIB_WG)), dim3(GRIB_WG), 0, s, (const uint8_t*)stage_dev, stage_bytes,
                       (const GribStep*)steps_dev, n_steps, g, (const uint32_t*)rank_dev, (float*)cube_dev);
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

// ---- GRIB complex packing (templates 5.2 / 5.3): the scratch of one call, in bytes from its start ----
struct GribCLayout { int64_t rank, groups, vals, sums, total; };
// false: sizes that afhip_grib_unpack_complex refuses (negative, beyond 2^31 - 1, a product that overflows, beyond one launch)
static bool grib_complex_layout(int64_t n_steps, int64_t n_points, int64_t max_groups, GribCLayout* L) {
    if (n_steps < 0 || n_steps > 0x7fffffff || n_points <= 0 || n_points > 0x7fffffff || max_groups < 0 || max_groups > 0x7fffffff) return false;
    const int64_t lim = (int64_t)1 << 60, per_step = grib_cgroup_words(max_groups) * 8 + n_points * 8 + grib_rank_words(n_points) * 4;
    if (n_steps && per_step > lim / n_steps) return false;
    const int64_t sums = afhip_delta_scratch_bytes(n_steps, n_points, 8);
    if (sums < 0) return false;
    auto up16 = [](int64_t v) { return (v + 15) / 16 * 16; };
    L->rank = 0;
    L->groups = up16(n_steps * grib_rank_words(n_points) * 4);
    L->vals = L->groups + up16(n_steps * grib_cgroup_words(max_groups) * 8);
    L->sums = L->vals + up16(n_steps * n_points * 8);
    L->total = L->sums + sums;
    return true;
}

extern "C" int64_t afhip_grib_complex_scratch_bytes(int64_t n_steps, int64_t n_points, int64_t max_groups) {
    GribCLayout L;
    return grib_complex_layout(n_steps, n_points, max_groups, &L) ? L.total : -1;
}

extern "C" int afhip_grib_unpack_complex(const void* stage_dev, int64_t stage_bytes, const afhip_grib_cstep* steps_dev, int64_t n_steps, int order,
                                         int64_t max_groups, int64_t NY, int64_t NX, int64_t y0, int64_t x0, int64_t ny, int64_t nx,
                                         void* cube_dev, int cube_elem_size, int64_t cube_nt, int64_t cube_NY, int64_t cube_NX,
                                         int64_t t0, int64_t cy, int64_t cx, void* scratch_dev, int64_t scratch_bytes, int32_t* errors_dev, void* stream) {
    static_assert(sizeof(afhip_grib_cstep) == sizeof(GribCStep) && sizeof(GribCStep) == 112, "record layouts");
    if (!stage_dev || !steps_dev || !cube_dev || !scratch_dev || !errors_dev || stage_bytes < 0 || n_steps < 0)
        return fail(AFHIP_E_INVALID, "grib_unpack_complex: bad arguments");
    if (order < 0 || order > 2) return fail(AFHIP_E_INVALID, "grib_unpack_complex: order must be 0 (template 5.2), 1 or 2 (got %d)", order);
    if (cube_elem_size != 4) return fail(AFHIP_E_INVALID, "grib_unpack_complex: the cube must be float32 (4-byte elements, got %d)", cube_elem_size);
    if (NY <= 0 || NX <= 0 || NY > 0x7fffffff / NX || y0 < 0 || x0 < 0 || ny < 0 || nx < 0 || ny > NY - y0 || nx > NX - x0)
        return fail(AFHIP_E_INVALID, "grib_unpack_complex: box outside the grid");
    if (cube_nt < 0 || cube_NY <= 0 || cube_NX <= 0 || t0 < 0 || cy < 0 || cx < 0 || n_steps > cube_nt - t0 || ny > cube_NY - cy || nx > cube_NX - cx)
        return fail(AFHIP_E_INVALID, "grib_unpack_complex: box outside the cube");
    if (stage_bytes & 3) return fail(AFHIP_E_INVALID, "grib_unpack_complex: the stage must be a whole number of 4-byte words (%lld bytes)", (long long)stage_bytes);
    if (((uintptr_t)stage_dev & 3) || ((uintptr_t)cube_dev & 3) || ((uintptr_t)scratch_dev & 15) || ((uintptr_t)steps_dev & 7))
        return fail(AFHIP_E_INVALID, "grib_unpack_complex: the stage and the cube must be 4-byte aligned, the records 8-byte, the scratch 16-byte aligned");
    GribCLayout L;
    if (!grib_complex_layout(n_steps, NY * NX, max_groups, &L))
        return fail(AFHIP_E_INVALID, "grib_unpack_complex: %lld steps of %lld points in up to %lld groups are too many for one call",
                    (long long)n_steps, (long long)(NY * NX), (long long)max_groups);
    if (scratch_bytes < L.total) return fail(AFHIP_E_INVALID, "grib_unpack_complex: scratch too small (afhip_grib_complex_scratch_bytes)");
    const int dev = pointer_device(cube_dev);
    if (dev < 0 || pointer_device(stage_dev) != dev || pointer_device(steps_dev) != dev || pointer_device(scratch_dev) != dev || pointer_device(errors_dev) != dev)
        return fail(AFHIP_E_INVALID, "grib_unpack_complex: the stage, the records, the scratch, the error counter and the cube must lie on one device");
    if (n_steps == 0 || ny == 0 || nx == 0) return AFHIP_OK;
    const int64_t NP = NY * NX, lanes = n_steps * ny * ((nx + GRIB_RUN - 1) / GRIB_RUN);
    if (lanes > (int64_t)0x7fffffff * GRIB_WG || n_steps * NP > (int64_t)0x7fffffff * GRIB_WG)
        return fail(AFHIP_E_INVALID, "grib_unpack_complex: box too large for one launch");
    GUARD_DEVICE(dev);
    hipStream_t s = (hipStream_t)stream;
    const GribBox g{NY, NX, y0, x0, ny, nx, cube_NY, cube_NX, t0, cy, cx};
    const uint8_t* stage = (const uint8_t*)stage_dev;
    const GribCStep* recs = (const GribCStep*)steps_dev;
    uint32_t* rank = (uint32_t*)((char*)scratch_dev + L.rank);
    int64_t* groups = (int64_t*)((char*)scratch_dev + L.groups);
    int64_t* vals = (int64_t*)((char*)scratch_dev + L.vals);
    hipLaunchKernelGGL(k_grib_cgroups, dim3((unsigned)n_steps), dim3(GRIB_WG), 0, s, stage, stage_bytes, recs, order, max_groups, g, rank, groups, errors_dev);
    hipLaunchKernelGGL(k_grib_cvalues, dim3((unsigned)((n_steps * NP + GRIB_WG - 1) / GRIB_WG)), dim3(GRIB_WG), 0, s, stage, stage_bytes, recs, n_steps, NP,
                       max_groups, (const int64_t*)groups, vals);
    // spatial differencing undone: the launches of afhip_delta_decode, over n_steps chunks of NP int64 elements
    for (int k = 0; k < order; ++k)
        delta_launch<uint64_t>(vals, (char*)scratch_dev + L.sums, n_steps, NP, delta_tiles_per_chunk(NP, 8), s);
    hipLaunchKernelGGL((k_grib_cplace<GribCStep, GribCVals>), dim3((unsigned)((lanes + GRIB_WG - 1) / GRIB_WG)), dim3(GRIB_WG), 0, s, stage, stage_bytes,
                       recs, n_steps, g, (const uint32_t*)rank, GribCVals{max_groups, NP, (const int64_t*)groups, (const int64_t*)vals}, (float*)cube_dev);
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

// ---- GRIB CCSDS packing (template 5.42): the scratch of one call, in bytes from its start ----
struct GribALayout { int64_t rank, sound, table, vals, total; };
// false: sizes that afhip_grib_unpack_ccsds refuses (negative, beyond 2^31 - 1, a product that overflows, beyond one launch)
static bool grib_ccsds_layout(int64_t n_steps, int64_t n_points, int64_t max_rsis, GribALayout* L) {
    if (n_steps < 0 || n_steps > 0x7fffffff || n_points <= 0 || n_points > 0x7fffffff || max_rsis < 0 || max_rsis > 0x7fffffff) return false;
    const int64_t lim = (int64_t)1 << 60, per_step = max_rsis * 8 + n_points * 4 + grib_rank_words(n_points) * 4 + 4;
    if (n_steps && per_step > lim / n_steps) return false;
    auto up16 = [](int64_t v) { return (v + 15) / 16 * 16; };
    L->rank = 0;
    L->sound = up16(n_steps * grib_rank_words(n_points) * 4);
    L->table = L->sound + up16(n_steps * 4);
    L->vals = L->table + up16(n_steps * max_rsis * 8);
    L->total = L->vals + up16(n_steps * n_points * 4);
    return true;
}

extern "C" int64_t afhip_grib_ccsds_scratch_bytes(int64_t n_steps, int64_t n_points, int64_t max_rsis) {
    GribALayout L;
    return grib_ccsds_layout(n_steps, n_points, max_rsis, &L) ? L.total : -1;
}

extern "C" int afhip_grib_unpack_ccsds(const void* stage_dev, int64_t stage_bytes, const afhip_grib_astep* steps_dev, int64_t n_steps,
                                       int64_t max_rsis, int64_t NY, int64_t NX, int64_t y0, int64_t x0, int64_t ny, int64_t nx,
                                       void* cube_dev, int cube_elem_size, int64_t cube_nt, int64_t cube_NY, int64_t cube_NX,
                                       int64_t t0, int64_t cy, int64_t cx, void* scratch_dev, int64_t scratch_bytes, int32_t* errors_dev, void* stream) {
    static_assert(sizeof(afhip_grib_astep) == sizeof(aec_step) && sizeof(aec_step) == 72, "record layouts");
    if (!stage_dev || !steps_dev || !cube_dev || !scratch_dev || !errors_dev || stage_bytes < 0 || n_steps < 0)
        return fail(AFHIP_E_INVALID, "grib_unpack_ccsds: bad arguments");
    if (cube_elem_size != 4) return fail(AFHIP_E_INVALID, "grib_unpack_ccsds: the cube must be float32 (4-byte elements, got %d)", cube_elem_size);
    if (NY <= 0 || NX <= 0 || NY > 0x7fffffff / NX || y0 < 0 || x0 < 0 || ny < 0 || nx < 0 || ny > NY - y0 || nx > NX - x0)
        return fail(AFHIP_E_INVALID, "grib_unpack_ccsds: box outside the grid");
    if (cube_nt < 0 || cube_NY <= 0 || cube_NX <= 0 || t0 < 0 || cy < 0 || cx < 0 || n_steps > cube_nt - t0 || ny > cube_NY - cy || nx > cube_NX - cx)
        return fail(AFHIP_E_INVALID, "grib_unpack_ccsds: box outside the cube");
    if (stage_bytes & 3) return fail(AFHIP_E_INVALID, "grib_unpack_ccsds: the stage must be a whole number of 4-byte words (%lld bytes)", (long long)stage_bytes);
    if (((uintptr_t)stage_dev & 3) || ((uintptr_t)cube_dev & 3) || ((uintptr_t)scratch_dev & 15) || ((uintptr_t)steps_dev & 7))
        return fail(AFHIP_E_INVALID, "grib_unpack_ccsds: the stage and the cube must be 4-byte aligned, the records 8-byte, the scratch 16-byte aligned");
    GribALayout L;
    if (!grib_ccsds_layout(n_steps, NY * NX, max_rsis, &L))
        return fail(AFHIP_E_INVALID, "grib_unpack_ccsds: %lld steps of %lld points in up to %lld reference sample intervals are too many for one call",
                    (long long)n_steps, (long long)(NY * NX), (long long)max_rsis);
    if (scratch_bytes < L.total) return fail(AFHIP_E_INVALID, "grib_unpack_ccsds: scratch too small (afhip_grib_ccsds_scratch_bytes)");
    const int dev = pointer_device(cube_dev);
    if (dev < 0 || pointer_device(stage_dev) != dev || pointer_device(steps_dev) != dev || pointer_device(scratch_dev) != dev || pointer_device(errors_dev) != dev)
        return fail(AFHIP_E_INVALID, "grib_unpack_ccsds: the stage, the records, the scratch, the error counter and the cube must lie on one device");
    if (n_steps == 0 || ny == 0 || nx == 0) return AFHIP_OK;
    const int64_t NP = NY * NX, lanes = n_steps * ny * ((nx + GRIB_RUN - 1) / GRIB_RUN), items = n_steps * (max_rsis > 0 ? max_rsis : 1);
    if (lanes > (int64_t)0x7fffffff * GRIB_WG || items > (int64_t)0x7fffffff * GRIB_WG)
        return fail(AFHIP_E_INVALID, "grib_unpack_ccsds: box too large for one launch");
    GUARD_DEVICE(dev);
    hipStream_t s = (hipStream_t)stream;
    const GribBox g{NY, NX, y0, x0, ny, nx, cube_NY, cube_NX, t0, cy, cx};
    aec_ctx c;
    c.stage = (const uint8_t*)stage_dev;
    c.stage_bytes = stage_bytes;
    c.steps = (const aec_step*)steps_dev;
    c.n_steps = n_steps;
    c.n_points = NP;
    c.max_rsis = max_rsis;
    c.sound = (int32_t*)((char*)scratch_dev + L.sound);
    c.rsi_bit = (int64_t*)((char*)scratch_dev + L.table);
    c.vals = (uint32_t*)((char*)scratch_dev + L.vals);
    c.errors = errors_dev;
    uint32_t* rank = (uint32_t*)((char*)scratch_dev + L.rank);
    hipLaunchKernelGGL(k_grib_awalk, dim3((unsigned)n_steps), dim3(GRIB_WG), 0, s, c, g, rank);
    if (max_rsis > 0)
        hipLaunchKernelGGL(k_grib_arsi, dim3((unsigned)((n_steps * max_rsis + GRIB_WG - 1) / GRIB_WG)), dim3(GRIB_WG), 0, s, c);
    hipLaunchKernelGGL((k_grib_cplace<aec_step, GribAVals>), dim3((unsigned)((lanes + GRIB_WG - 1) / GRIB_WG)), dim3(GRIB_WG), 0, s, c.stage, stage_bytes,
                       c.steps, n_steps, g, (const uint32_t*)rank, GribAVals{NP, c.sound, c.vals}, (float*)cube_dev);
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

// ---- TIFF stacks: LZW segments decoded in HBM, predictors undone and segments placed (afhip_tiff_kernels.h) ----
extern "C" int afhip_lzw_decode(const void* stage_dev, int64_t stage_bytes, afhip_tiff_seg* records_dev, int64_t n, void* out_dev, int64_t out_bytes,
                                int32_t* errors_dev, void* stream) {
    static_assert(sizeof(afhip_tiff_seg) == sizeof(TiffSeg) && sizeof(TiffSeg) == 56, "record layouts");
    if (!stage_dev || !records_dev || !out_dev || !errors_dev || stage_bytes < 0 || out_bytes < 0 || n < 0)
        return fail(AFHIP_E_INVALID, "lzw_decode: bad arguments");
    if (n > 0x7fffffff) return fail(AFHIP_E_INVALID, "lzw_decode: too many segments for one launch");
    if ((uintptr_t)records_dev & 7) return fail(AFHIP_E_INVALID, "lzw_decode: the records must be 8-byte aligned");
    const int dev = pointer_device(out_dev);
    if (dev < 0 || pointer_device(stage_dev) != dev || pointer_device(records_dev) != dev || pointer_device(errors_dev) != dev)
        return fail(AFHIP_E_INVALID, "lzw_decode: the stage, the records, the decoded buffer and the error counter must lie on one device");
    if (n == 0) return AFHIP_OK;
    GUARD_DEVICE(dev);
    hipLaunchKernelGGL(k_lzw_decode, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)stage_dev, stage_bytes, (TiffSeg*)records_dev,
                       (uint8_t*)out_dev, out_bytes, errors_dev);
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int afhip_tiff_place(const void* decoded_dev, int64_t decoded_bytes, const afhip_tiff_seg* records_dev, int64_t n, int64_t max_rows,
                                int elem_size, int predictor, int swap, void* cube_dev, int64_t NT, int64_t NY, int64_t NX,
                                int64_t y0, int64_t x0, int64_t ny, int64_t nx, int64_t t0, int64_t cy, int64_t cx, int32_t* errors_dev, void* stream) {
    if (!decoded_dev || !records_dev || !cube_dev || !errors_dev || decoded_bytes < 0 || n < 0 || max_rows < 0)
        return fail(AFHIP_E_INVALID, "tiff_place: bad arguments");
    if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8) return fail(AFHIP_E_INVALID, "tiff_place: elem_size must be 1, 2, 4 or 8 (got %d)", elem_size);
    if (predictor < 1 || predictor > 3) return fail(AFHIP_E_INVALID, "tiff_place: predictor must be 1 (none), 2 (horizontal) or 3 (floating point), got %d", predictor);
    if (predictor == 3 && elem_size != 4 && elem_size != 8) return fail(AFHIP_E_INVALID, "tiff_place: the floating-point predictor needs 4- or 8-byte samples");
    if (NT < 0 || NY <= 0 || NX <= 0 || NY > 0x7fffffff || NX > 0x7fffffff || y0 < 0 || x0 < 0 || ny < 0 || nx < 0 || t0 < 0 || cy < 0 || cx < 0 ||
        y0 > 0x7fffffff || x0 > 0x7fffffff || t0 > NT || ny > NY - cy || nx > NX - cx)
        return fail(AFHIP_E_INVALID, "tiff_place: box outside the cube");
    if (n > 0x7fffffff) return fail(AFHIP_E_INVALID, "tiff_place: too many segments for one launch");
    if (((uintptr_t)decoded_dev | (uintptr_t)cube_dev) & (uintptr_t)(elem_size - 1))
        return fail(AFHIP_E_INVALID, "tiff_place: the decoded buffer and the cube must be aligned to the element size");
    if ((uintptr_t)records_dev & 7) return fail(AFHIP_E_INVALID, "tiff_place: the records must be 8-byte aligned");
    const int dev = pointer_device(cube_dev);
    if (dev < 0 || pointer_device(decoded_dev) != dev || pointer_device(records_dev) != dev || pointer_device(errors_dev) != dev)
        return fail(AFHIP_E_INVALID, "tiff_place: the decoded buffer, the records, the error counter and the cube must lie on one device");
    if (n == 0 || max_rows == 0 || ny == 0 || nx == 0 || NT == t0) return AFHIP_OK;
    GUARD_DEVICE(dev);
    hipStream_t s = (hipStream_t)stream;
    const int64_t per = TIFF_WG / 64, gy = (max_rows + per - 1) / per;
    const dim3 grid((unsigned)n, (unsigned)(gy < 64 ? gy : 64)), block(TIFF_WG);
    const TiffBox g{NT, NY, NX, y0, x0, ny, nx, t0, cy, cx};
#define TIFF_PLACE_AS(TE)                                                                                                               \
    hipLaunchKernelGGL(k_tiff_place<TE>, grid, block, 0, s, (const uint8_t*)decoded_dev, decoded_bytes, (const TiffSeg*)records_dev, predictor, \
                       swap != 0, (TE*)cube_dev, g, errors_dev)
    switch (elem_size) {
        case 1: TIFF_PLACE_AS(uint8_t); break;
        case 2: TIFF_PLACE_AS(uint16_t); break;
        case 4: TIFF_PLACE_AS(uint32_t); break;
        default: TIFF_PLACE_AS(uint64_t); break;
    }
#undef TIFF_PLACE_AS
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int afhip_tiff_place_bands(const void* decoded_dev, int64_t decoded_bytes, const afhip_tiff_seg* records_dev, int64_t n, int64_t max_rows,
                                      int64_t bands, int elem_size, int predictor, int swap, void* cube_dev, int64_t NT, int64_t NY, int64_t NX,
                                      int64_t y0, int64_t x0, int64_t ny, int64_t nx, int64_t t0, int64_t cy, int64_t cx, int32_t* errors_dev,
                                      void* stream) {
    if (!decoded_dev || !records_dev || !cube_dev || !errors_dev || decoded_bytes < 0 || n < 0 || max_rows < 0)
        return fail(AFHIP_E_INVALID, "tiff_place_bands: bad arguments");
    if (bands < 1 || bands > TBAND_MAX) return fail(AFHIP_E_INVALID, "tiff_place_bands: bands must be 1 .. %d (got %lld)", TBAND_MAX, (long long)bands);
    if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8)
        return fail(AFHIP_E_INVALID, "tiff_place_bands: elem_size must be 1, 2, 4 or 8 (got %d)", elem_size);
    if (predictor < 1 || predictor > 3)
        return fail(AFHIP_E_INVALID, "tiff_place_bands: predictor must be 1 (none), 2 (horizontal) or 3 (floating point), got %d", predictor);
    if (predictor == 3 && elem_size != 4 && elem_size != 8) return fail(AFHIP_E_INVALID, "tiff_place_bands: the floating-point predictor needs 4- or 8-byte samples");
    if (NT < 0 || NY <= 0 || NX <= 0 || NY > 0x7fffffff || NX > 0x7fffffff || y0 < 0 || x0 < 0 || ny < 0 || nx < 0 || t0 < 0 || cy < 0 || cx < 0 ||
        y0 > 0x7fffffff || x0 > 0x7fffffff || t0 > NT || ny > NY - cy || nx > NX - cx)
        return fail(AFHIP_E_INVALID, "tiff_place_bands: box outside the cube");
    if (n > 0x7fffffff) return fail(AFHIP_E_INVALID, "tiff_place_bands: too many segments for one launch");
    if (((uintptr_t)decoded_dev | (uintptr_t)cube_dev) & (uintptr_t)(elem_size - 1))
        return fail(AFHIP_E_INVALID, "tiff_place_bands: the decoded buffer and the cube must be aligned to the element size");
    if ((uintptr_t)records_dev & 7) return fail(AFHIP_E_INVALID, "tiff_place_bands: the records must be 8-byte aligned");
    const int dev = pointer_device(cube_dev);
    if (dev < 0 || pointer_device(decoded_dev) != dev || pointer_device(records_dev) != dev || pointer_device(errors_dev) != dev)
        return fail(AFHIP_E_INVALID, "tiff_place_bands: the decoded buffer, the records, the error counter and the cube must lie on one device");
    if (n == 0 || max_rows == 0 || ny == 0 || nx == 0 || NT == t0) return AFHIP_OK;
    GUARD_DEVICE(dev);
    hipStream_t s = (hipStream_t)stream;
    // a workgroup per (segment, row, tile of bands); rows beyond the grid's limit are walked by the same workgroups
    const dim3 grid((unsigned)n, (unsigned)(max_rows < 65535 ? max_rows : 65535), (unsigned)((bands + TBAND_TILE - 1) / TBAND_TILE)), block(TIFF_WG);
    const TiffBox g{NT, NY, NX, y0, x0, ny, nx, t0, cy, cx};
#define TIFF_BANDS_AS(TE)                                                                                                                      \
    hipLaunchKernelGGL(k_tiff_place_bands<TE>, grid, block, 0, s, (const uint8_t*)decoded_dev, decoded_bytes, (const TiffSeg*)records_dev, (int)bands, \
                       predictor, swap != 0, (TE*)cube_dev, g, errors_dev)
    switch (elem_size) {
        case 1: TIFF_BANDS_AS(uint8_t); break;
        case 2: TIFF_BANDS_AS(uint16_t); break;
        case 4: TIFF_BANDS_AS(uint32_t); break;
        default: TIFF_BANDS_AS(uint64_t); break;
    }
#undef TIFF_BANDS_AS
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int afhip_lz4_decode_streams(const void* comp_dev, const afhip_lz4_stream* streams_dev, int64_t n_streams, int32_t max_dsize,
                                        void* tmp_dev, void* out_dev, int32_t* errors_dev, void* stream) {
    static_assert(sizeof(afhip_lz4_stream) == sizeof(Lz4Stream) && sizeof(afhip_shuffle_block) == sizeof(ShufBlock), "record layouts");
    if (!comp_dev || !streams_dev || !errors_dev || n_streams < 0 || (!tmp_dev && !out_dev))
        return fail(AFHIP_E_INVALID, "lz4_decode_streams: NULL argument");
    if (max_dsize < 0) return fail(AFHIP_E_INVALID, "lz4_decode_streams: negative max_dsize");
    if (n_streams == 0) return AFHIP_OK;
    if (n_streams > 0x7fffffff) return fail(AFHIP_E_INVALID, "lz4_decode_streams: too many streams for one launch");
    GUARD_DEVICE(pointer_device(comp_dev));
    const dim3 g((unsigned)n_streams), b(64);
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* c = (const uint8_t*)comp_dev;
    const Lz4Stream* sr = (const Lz4Stream*)streams_dev;
    static const bool prof = [] { const char* e = getenv("AFHIP_LZ4_PROF"); return e && atoi(e) != 0; }();
    if (prof) {      // measuring aid: cycles per phase, summed over the LZ4 streams of this launch, on stderr (synchronous)
        long long* d = nullptr;
        HIP_TRY(hipMalloc(&d, (size_t)n_streams * 8 * sizeof(long long)));
        HIP_TRY(hipMemsetAsync(d, 0, (size_t)n_streams * 8 * sizeof(long long), st));
        hipLaunchKernelGGL((k_lz4_streams_vec<LZ4_NEAR, true>), g, b, 0, st, c, sr, (uint8_t*)tmp_dev, (uint8_t*)out_dev, errors_dev, d);
        std::vector<long long> h((size_t)n_streams * 8);
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpy(h.data(), d, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
        HIP_TRY(hipFree(d));
        long long tot[8] = {0}, mx = 0;
        for (int64_t i = 0; i < n_streams; ++i) {
            long long sum = 0;
            for (int j = 0; j < 7; ++j) { tot[j] += h[i * 8 + j]; sum += h[i * 8 + j]; }
            tot[7] += h[i * 8 + 7];
            mx = std::max(mx, sum);
        }
        fprintf(stderr, "lz4 prof (shader clock cycles, all streams): parse %lld walk %lld scan %lld owner %lld pending %lld store %lld "
                        "generic %lld; windows %lld; longest stream %lld\n", tot[0], tot[1], tot[2], tot[3], tot[4], tot[5], tot[6], tot[7], mx);
        return AFHIP_OK;
    }
    hipLaunchKernelGGL((k_lz4_streams_vec<LZ4_NEAR, false>), g, b, 0, st, c, sr, (uint8_t*)tmp_dev, (uint8_t*)out_dev, errors_dev, (long long*)nullptr);
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int64_t afhip_zstd_scratch_bytes(int64_t n_blocks, int64_t n_frames, int64_t lit_bytes, int64_t n_seqs, int64_t dec_bytes) {
    if (n_blocks < 0 || n_frames < 0 || lit_bytes < 0 || n_seqs < 0 || dec_bytes < 0) return fail(AFHIP_E_INVALID, "zstd_scratch_bytes: negative size");
    int64_t o[9];
    return afz_layout(n_blocks, n_frames, lit_bytes, n_seqs, dec_bytes, o);
}

extern "C" int afhip_zstd_decode(const void* comp_dev, int64_t comp_bytes, const afhip_zstd_frame* frames_dev, int64_t n_frames,
                                 const afhip_zstd_block* blocks_dev, int64_t n_blocks, int64_t lit_bytes, int64_t n_seqs, int64_t dec_bytes,
                                 void* scratch_dev, int64_t scratch_bytes, void* out_dev, int32_t* errors_dev, int32_t* rounds_dev,
                                 void* stream) {
    static_assert(sizeof(afhip_zstd_block) == sizeof(afz_block) && sizeof(afhip_zstd_frame) == sizeof(afz_frame), "record layouts");
    if (!comp_dev || !frames_dev || !blocks_dev || !scratch_dev || !out_dev || !errors_dev || comp_bytes < 0 || n_frames < 0 ||
        n_blocks < 0 || lit_bytes < 0 || n_seqs < 0 || dec_bytes < 0)
        return fail(AFHIP_E_INVALID, "zstd_decode: NULL argument or negative size");
    if (dec_bytes > 0x7fffffff || lit_bytes > 0x7fffffff || n_blocks > 0x7fffffff - 64)
        return fail(AFHIP_E_INVALID, "zstd_decode: more than 2 GiB decoded in one batch");
    if (scratch_bytes < afhip_zstd_scratch_bytes(n_blocks, n_frames, lit_bytes, n_seqs, dec_bytes))
        return fail(AFHIP_E_INVALID, "zstd_decode: scratch smaller than afhip_zstd_scratch_bytes()");
    if (n_frames == 0) return AFHIP_OK;
    GUARD_DEVICE(pointer_device(out_dev));
    hipStream_t st = (hipStream_t)stream;
    afz_ctx c;
    memset(&c, 0, sizeof c);
    c.comp = (const uint8_t*)comp_dev; c.comp_bytes = comp_bytes;
    c.frames = (const afz_frame*)frames_dev; c.n_frames = n_frames;
    c.blocks = (const afz_block*)blocks_dev; c.n_blocks = n_blocks;
    afz_bind(&c, (uint8_t*)scratch_dev, n_blocks, n_frames, lit_bytes, n_seqs, dec_bytes);
    c.out = (uint8_t*)out_dev; c.errors = errors_dev;
    HIP_TRY(hipMemsetAsync(c.bad, 0, (size_t)(n_frames + 64) * 4, st));
    auto waves = [](int64_t n) { return dim3((unsigned)std::max<int64_t>(1, (n + ZSTD_WG - 1) / ZSTD_WG)); };
    hipLaunchKernelGGL(k_zstd_tables, waves(n_blocks + 1), dim3(ZSTD_WG), 0, st, c);
    if (n_blocks) {
        hipLaunchKernelGGL(k_zstd_literals, waves(4 * n_blocks), dim3(ZSTD_WG), 0, st, c);
        hipLaunchKernelGGL(k_zstd_sequences, waves(n_blocks), dim3(ZSTD_WG), 0, st, c);
    }
    hipLaunchKernelGGL(k_zstd_frames, waves(n_frames), dim3(ZSTD_WG), 0, st, c);
    const int R = afz_rounds_host(dec_bytes);
    if (n_blocks) {
        hipLaunchKernelGGL(k_zstd_fill, dim3((unsigned)n_blocks), dim3(ZSTD_WG), 0, st, c);
        const unsigned jg = (unsigned)std::max<int64_t>(1, std::min<int64_t>((dec_bytes + ZSTD_JUMP_WG - 1) / ZSTD_JUMP_WG, 16384));
        for (int r = 0; r < R; ++r) hipLaunchKernelGGL(k_zstd_jump, dim3(jg), dim3(ZSTD_JUMP_WG), 0, st, c, r);
        hipLaunchKernelGGL(k_zstd_gather, dim3((unsigned)n_blocks), dim3(ZSTD_WG), 0, st, c);
    }
    if (rounds_dev) hipLaunchKernelGGL(k_zstd_rounds, dim3(1), dim3(ZSTD_WG), 0, st, c, R, rounds_dev);
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int64_t afhip_inflate_scratch_bytes(int64_t n_streams, int64_t n_pblocks, int64_t n_seqs, int64_t n_pieces, int64_t dec_bytes,
                                               int64_t tmp_bytes) {
    if (n_streams < 0 || n_pblocks < 0 || n_seqs < 0 || n_pieces < 0 || dec_bytes < 0 || tmp_bytes < 0)
        return fail(AFHIP_E_INVALID, "inflate_scratch_bytes: negative size");
    int64_t o[9];
    return afi_layout(n_streams, n_pblocks, n_seqs, n_pieces, dec_bytes, tmp_bytes, o);
}

extern "C" int afhip_inflate_decode(const void* comp_dev, int64_t comp_bytes, const afhip_inflate_stream* streams_dev, int64_t n_streams,
                                    const afhip_shuffle_block* shuf_dev, int64_t n_shuf, int32_t max_bsize, int64_t n_pblocks, int64_t n_seqs,
                                    int64_t n_pieces, int64_t dec_bytes, int64_t tmp_bytes, void* scratch_dev, int64_t scratch_bytes,
                                    void* out_dev, int32_t* errors_dev, int32_t* rounds_dev, void* stream) {
    static_assert(sizeof(afhip_inflate_stream) == sizeof(afi_stream) && sizeof(afhip_shuffle_block) == sizeof(ShufBlock), "record layouts");
    if (!comp_dev || !streams_dev || !scratch_dev || !out_dev || !errors_dev || (n_shuf && !shuf_dev) || comp_bytes < 0 || n_streams < 0 ||
        n_shuf < 0 || max_bsize < 0 || n_pblocks < 0 || n_seqs < 0 || n_pieces < 0 || dec_bytes < 0 || tmp_bytes < 0)
        return fail(AFHIP_E_INVALID, "inflate_decode: NULL argument or negative size");
    if (dec_bytes > 0x7fffffff || n_pblocks > 0x7fffffff - 64 || n_streams > 0x7fffffff - 64 || n_pieces > 0x7fffffff - 64)
        return fail(AFHIP_E_INVALID, "inflate_decode: more than 2 GiB decoded in one batch");
    if (scratch_bytes < afhip_inflate_scratch_bytes(n_streams, n_pblocks, n_seqs, n_pieces, dec_bytes, tmp_bytes))
        return fail(AFHIP_E_INVALID, "inflate_decode: scratch smaller than afhip_inflate_scratch_bytes()");
    if (n_streams == 0) return AFHIP_OK;
    GUARD_DEVICE(pointer_device(out_dev));
    hipStream_t st = (hipStream_t)stream;
    afi_ctx c;
    memset(&c, 0, sizeof c);
    c.comp = (const uint8_t*)comp_dev; c.comp_bytes = comp_bytes;
    c.streams = (const afi_stream*)streams_dev; c.n_streams = n_streams;
    c.n_blocks = n_pblocks; c.n_seqs = n_seqs; c.n_pieces = n_pieces; c.dec_bytes = dec_bytes; c.tmp_bytes = tmp_bytes;
    afi_bind(&c, (uint8_t*)scratch_dev);
    c.out = (uint8_t*)out_dev; c.errors = errors_dev;
    HIP_TRY(hipMemsetAsync(c.bad, 0, (size_t)(n_streams + 64) * 4, st));
    auto waves = [](int64_t n) { return dim3((unsigned)std::max<int64_t>(1, (n + INFLATE_WG - 1) / INFLATE_WG)); };
    hipLaunchKernelGGL(k_inflate_front, dim3((unsigned)n_streams), dim3(INFLATE_WG), 0, st, c);
    const int R = afz_rounds_host(dec_bytes);
    const afz_ctx z = afi_jump_view(&c);
    if (n_pblocks && dec_bytes) {
        hipLaunchKernelGGL(k_inflate_fill, dim3((unsigned)n_pblocks), dim3(INFLATE_WG), 0, st, c);
        const unsigned jg = (unsigned)std::max<int64_t>(1, std::min<int64_t>((dec_bytes + ZSTD_JUMP_WG - 1) / ZSTD_JUMP_WG, 16384));
        for (int r = 0; r < R; ++r) hipLaunchKernelGGL(k_zstd_jump, dim3(jg), dim3(ZSTD_JUMP_WG), 0, st, z, r);
        hipLaunchKernelGGL(k_inflate_gather, dim3((unsigned)n_pblocks), dim3(INFLATE_WG), 0, st, c);
    }
    if (n_pieces) hipLaunchKernelGGL(k_inflate_adler, dim3((unsigned)n_pieces), dim3(INFLATE_WG), 0, st, c);
    hipLaunchKernelGGL(k_inflate_check, waves(n_streams), dim3(INFLATE_WG), 0, st, c);
    const unsigned tiles = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, ((int64_t)max_bsize / 2 + 255) / 256));
    for (int64_t b0 = 0; b0 < n_shuf; b0 += 65535)       // (a launch unshuffles at most 65,535 blocks)
        hipLaunchKernelGGL(k_unshuffle_blocks, dim3(tiles, (unsigned)std::min<int64_t>(65535, n_shuf - b0)), dim3(256), 0, st,
                           (const uint8_t*)c.tmp, (uint8_t*)out_dev, (const ShufBlock*)shuf_dev + b0);
    if (rounds_dev) hipLaunchKernelGGL(k_zstd_rounds, dim3(1), dim3(ZSTD_WG), 0, st, z, R, rounds_dev);
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int afhip_unshuffle_blocks(const void* tmp_dev, void* out_dev, const afhip_shuffle_block* blocks_dev, int64_t n_blocks,
                                      int32_t max_bsize, void* stream) {
    if (!tmp_dev || !out_dev || !blocks_dev || n_blocks < 0 || max_bsize < 0) return fail(AFHIP_E_INVALID, "unshuffle_blocks: bad arguments");
    if (n_blocks == 0) return AFHIP_OK;
    if (n_blocks > 65535) return fail(AFHIP_E_INVALID, "unshuffle_blocks: more than 65535 blocks in one call");
    GUARD_DEVICE(pointer_device(out_dev));
    const unsigned tiles = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, ((int64_t)max_bsize / 2 + 255) / 256));
    hipLaunchKernelGGL(k_unshuffle_blocks, dim3(tiles, (unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)tmp_dev,
                       (uint8_t*)out_dev, (const ShufBlock*)blocks_dev);
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int afhip_bitunshuffle_blocks(const void* tmp_dev, void* out_dev, const afhip_shuffle_block* blocks_dev, int64_t n_blocks,
                                         int32_t max_bsize, void* stream) {
    if (!tmp_dev || !out_dev || !blocks_dev || n_blocks < 0 || max_bsize < 0) return fail(AFHIP_E_INVALID, "bitunshuffle_blocks: bad arguments");
    if (n_blocks == 0) return AFHIP_OK;
    if (n_blocks > 65535) return fail(AFHIP_E_INVALID, "bitunshuffle_blocks: more than 65535 blocks in one call");
    GUARD_DEVICE(pointer_device(out_dev));
    // a lane takes 8 elements: one tile of 256 lanes per 8 KiB of 4-byte elements
    const unsigned tiles = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, ((int64_t)max_bsize / 32 + 255) / 256));
    hipLaunchKernelGGL(k_bitunshuffle_blocks, dim3(tiles, (unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)tmp_dev,
                       (uint8_t*)out_dev, (const ShufBlock*)blocks_dev);
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int afhip_take_box(const void* cube_dev, void* chunk_dev, int elem_size, int64_t NY, int64_t NX,
                              int64_t t0, int64_t y0, int64_t x0, int64_t nt, int64_t ny, int64_t nx,
                              int64_t ct, int64_t cy, int64_t cx, uint64_t fill, void* stream) {
    if (!cube_dev || !chunk_dev || NY <= 0 || NX <= 0 || ct <= 0 || cy <= 0 || cx <= 0 || nt < 0 || ny < 0 || nx < 0 ||
        t0 < 0 || y0 < 0 || x0 < 0 || nt > ct || ny > cy || nx > cx || y0 + ny > NY || x0 + nx > NX)
        return fail(AFHIP_E_INVALID, "take_box: box outside the chunk or the cube");
    const int64_t n = ct * cy * cx;
    GUARD_DEVICE(pointer_device(cube_dev));
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)std::min<int64_t>((n + 255) / 256, 1 << 20)), block(256);     // (grid-stride beyond 2^28 elements)
    switch (elem_size) {
        case 1: hipLaunchKernelGGL(k_take_box<uint8_t>, grid, block, 0, s, (const uint8_t*)cube_dev, (uint8_t*)chunk_dev, NY, NX, t0, y0, x0, nt, ny, nx, ct, cy, cx, (uint8_t)fill); break;
        case 2: hipLaunchKernelGGL(k_take_box<uint16_t>, grid, block, 0, s, (const uint16_t*)cube_dev, (uint16_t*)chunk_dev, NY, NX, t0, y0, x0, nt, ny, nx, ct, cy, cx, (uint16_t)fill); break;
        case 4: hipLaunchKernelGGL(k_take_box<uint32_t>, grid, block, 0, s, (const uint32_t*)cube_dev, (uint32_t*)chunk_dev, NY, NX, t0, y0, x0, nt, ny, nx, ct, cy, cx, (uint32_t)fill); break;
        case 8: hipLaunchKernelGGL(k_take_box<uint64_t>, grid, block, 0, s, (const uint64_t*)cube_dev, (uint64_t*)chunk_dev, NY, NX, t0, y0, x0, nt, ny, nx, ct, cy, cx, (uint64_t)fill); break;
        default: return fail(AFHIP_E_INVALID, "take_box: elem_size must be 1, 2, 4 or 8");
    }
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int afhip_shuffle_blocks(const void* out_dev, void* tmp_dev, const afhip_shuffle_block* blocks_dev, int64_t n_blocks,
                                    int32_t max_bsize, void* stream) {
    if (!tmp_dev || !out_dev || !blocks_dev || n_blocks < 0 || max_bsize < 0) return fail(AFHIP_E_INVALID, "shuffle_blocks: bad arguments");
    if (n_blocks == 0) return AFHIP_OK;
    if (n_blocks > 65535) return fail(AFHIP_E_INVALID, "shuffle_blocks: more than 65535 blocks in one call");
    GUARD_DEVICE(pointer_device(tmp_dev));
    const unsigned tiles = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, ((int64_t)max_bsize / 2 + 255) / 256));
    hipLaunchKernelGGL(k_shuffle_blocks, dim3(tiles, (unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)out_dev,
                       (uint8_t*)tmp_dev, (const ShufBlock*)blocks_dev);
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int afhip_lz4_encode_streams(const void* in_dev, const afhip_lz4_stream* streams_dev, int64_t n_streams, void* slots_dev,
                                        int32_t* csize_dev, void* stream) {
    if (!in_dev || !streams_dev || !slots_dev || !csize_dev || n_streams < 0) return fail(AFHIP_E_INVALID, "lz4_encode_streams: bad arguments");
    if (n_streams == 0) return AFHIP_OK;
    if (n_streams > 0x7fffffff) return fail(AFHIP_E_INVALID, "lz4_encode_streams: too many streams for one launch");
    GUARD_DEVICE(pointer_device(slots_dev));
    hipLaunchKernelGGL(k_lz4_encode_streams, dim3((unsigned)n_streams), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)in_dev,
                       (const Lz4Stream*)streams_dev, (uint8_t*)slots_dev, csize_dev);
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int64_t afhip_zstd_encode_scratch_bytes(int64_t n) {
    if (n <= 0) return AFZE_TAB_BYTES + (256 - AFZE_TAB_BYTES % 256) % 256;
    return n > AFZ_BLOCK_MAX ? -1 : afze_scratch_bytes((int32_t)n);
}

extern "C" int afhip_zstd_encode_blocks(const void* in_dev, const afhip_zstd_encode_block* blocks_dev, int64_t n_blocks, void* scratch_dev,
                                        void* slots_dev, int32_t* csize_dev, void* stream) {
    static_assert(sizeof(afhip_zstd_encode_block) == sizeof(ZstdEncodeBlock), "record layouts");
    if (!in_dev || !blocks_dev || !scratch_dev || !slots_dev || !csize_dev || n_blocks < 0)
        return fail(AFHIP_E_INVALID, "zstd_encode_blocks: bad arguments");
    if (n_blocks == 0) return AFHIP_OK;
    if (n_blocks > (int64_t)65535 * 65535) return fail(AFHIP_E_INVALID, "zstd_encode_blocks: too many blocks for one launch");
    GUARD_DEVICE(pointer_device(slots_dev));
    hipLaunchKernelGGL(k_zstd_encode_tables, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint8_t*)scratch_dev);
    const dim3 grid((unsigned)std::min<int64_t>(n_blocks, 65535), (unsigned)((n_blocks + 65534) / 65535));
    hipLaunchKernelGGL(k_zstd_encode_blocks, grid, dim3(64), 0, (hipStream_t)stream, (const uint8_t*)in_dev,
                       (const ZstdEncodeBlock*)blocks_dev, n_blocks, (uint8_t*)scratch_dev, (uint8_t*)slots_dev, csize_dev);
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int afhip_copy_ranges(const void* src_dev, void* dst_dev, const afhip_copy_range* ranges_dev, int64_t n_ranges, void* stream) {
    static_assert(sizeof(afhip_copy_range) == sizeof(CopyRange), "record layouts");
    if (!src_dev || !dst_dev || !ranges_dev || n_ranges < 0) return fail(AFHIP_E_INVALID, "copy_ranges: bad arguments");
    if (n_ranges == 0) return AFHIP_OK;
    if (n_ranges > 0x7fffffff) return fail(AFHIP_E_INVALID, "copy_ranges: too many ranges for one launch");
    GUARD_DEVICE(pointer_device(dst_dev));
    hipLaunchKernelGGL(k_copy_ranges, dim3((unsigned)n_ranges), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src_dev,
                       (uint8_t*)dst_dev, (const CopyRange*)ranges_dev);
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int afhip_panel_divide(const double* num_dev, const double* den_dev, double* res_dev, int64_t K, int64_t R,
                                  int64_t P, void* stream) {
    if (!num_dev || !den_dev || !res_dev || K < 0 || R < 0 || P < 0) return fail(AFHIP_E_INVALID, "panel_divide: bad arguments");
    const int64_t n = K * R * P;
    if (n == 0) return AFHIP_OK;
    GUARD_DEVICE(pointer_device(res_dev));
    hipLaunchKernelGGL(k_divide_num_den, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, (hipStream_t)stream, num_dev, den_dev, res_dev, n, R * P);
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

// The box's streaming-read ceiling for a time-major cube: `launches` back-to-back launches of k_read_probe over [T][row_bytes],
// HIP events around each, one synchronisation at the end.
extern "C" int afhip_read_probe(const void* cube_dev, int64_t T, int64_t row_bytes, int launches, float* ms_out, void* stream) {
    if (!cube_dev || !ms_out || T <= 0 || row_bytes <= 0 || row_bytes % 8 != 0 || launches <= 0 || launches > 1000)
        return fail(AFHIP_E_INVALID, "read_probe: NULL argument, rows that are not multiples of 8 bytes, or a launch count outside 1..1000");
    const int64_t lanes = row_bytes / 8, blocks = (lanes + 63) / 64;
    if (blocks > 0x7fffffff) return fail(AFHIP_E_INVALID, "read_probe: rows too long for one launch");
    GUARD_DEVICE(pointer_device(cube_dev));
    hipStream_t st = (hipStream_t)stream;
    // (a small grid gets time chunks, like the temporal kernel's launches: about 16 single-wave workgroups per CU in all, chunks of 64 rows and more)
    int64_t chunks = 1;
    { const int64_t want = (int64_t)16 * cu_count(pointer_device(cube_dev));
      if (blocks < want) chunks = std::min<int64_t>(std::max<int64_t>(1, T / 64), std::min<int64_t>(65535, (want + blocks - 1) / blocks)); }
    const int64_t rows_per_chunk = (T + chunks - 1) / chunks;
    chunks = (T + rows_per_chunk - 1) / rows_per_chunk;
    uint32_t* out = nullptr;
    HIP_TRY(hipMalloc((void**)&out, (size_t)lanes * (size_t)chunks * sizeof(uint32_t)));
    std::vector<hipEvent_t> ev((size_t)launches + 1, nullptr);
    int rc = AFHIP_OK;
    for (auto& e : ev)
        if (hipEventCreate(&e) != hipSuccess) { rc = fail(AFHIP_E_HIP, "read_probe: hipEventCreate failed"); break; }
    if (!rc) {
        (void)hipEventRecord(ev[0], st);
        for (int i = 0; i < launches; ++i) {
            hipLaunchKernelGGL(k_read_probe, dim3((unsigned)blocks, (unsigned)chunks), dim3(64), 0, st, (const uint32_t*)cube_dev, row_bytes / 4, T, rows_per_chunk, out);
            (void)hipEventRecord(ev[(size_t)i + 1], st);
        }
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipEventSynchronize(ev[(size_t)launches]);
        if (e != hipSuccess) rc = fail(AFHIP_E_HIP, "read_probe: %s", hipGetErrorString(e));
        for (int i = 0; !rc && i < launches; ++i)
            if (hipEventElapsedTime(&ms_out[i], ev[(size_t)i], ev[(size_t)i + 1]) != hipSuccess) rc = fail(AFHIP_E_HIP, "read_probe: event query failed");
    }
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    (void)hipFree(out);
    return rc;
}

extern "C" int afhip_transform(const void* x_dev, int x_dtype, int64_t n, int transform, double arg,
                               const void* other_dev, int other_dtype, void* out_dev, int out_dtype, void* stream) {
    if (!x_dev || !out_dev || n < 0) return fail(AFHIP_E_INVALID, "transform: NULL array or negative size");
    if ((x_dtype != AFHIP_F32 && x_dtype != AFHIP_F64) || (out_dtype != AFHIP_F32 && out_dtype != AFHIP_F64))
        return fail(AFHIP_E_INVALID, "transform: dtypes must be AFHIP_F32 or AFHIP_F64");
    TransformArgs ta{};
    ta.x = x_dev; ta.other = nullptr; ta.out = out_dev; ta.n = n;
    ta.x_f32 = x_dtype == AFHIP_F32; ta.out_f32 = out_dtype == AFHIP_F32; ta.other_f32 = 0;
    switch (transform) {
        case AFHIP_TF_POW:
            if (arg == std::floor(arg) && std::fabs(arg) <= 64.0) { ta.tf = TF_POWI; ta.iarg = (int)arg; }
            else { ta.tf = TF_POW; ta.arg = arg; }
            break;
        case AFHIP_TF_HINGE: ta.tf = TF_HINGE; ta.arg = arg; break;
        case AFHIP_TF_INTER:
            if (!other_dev || (other_dtype != AFHIP_F32 && other_dtype != AFHIP_F64))
                return fail(AFHIP_E_INVALID, "transform: AFHIP_TF_INTER needs the second array and its dtype");
            ta.tf = TF_INTER; ta.other = other_dev; ta.other_f32 = other_dtype == AFHIP_F32;
            break;
        default: return fail(AFHIP_E_INVALID, "transform: unknown transform %d", transform);
    }
    if (n == 0) return AFHIP_OK;
    GUARD_DEVICE(pointer_device(out_dev));
    const int64_t per_block = (int64_t)WG * TRANSFORM_PER_THREAD;
    const int64_t blocks = (n + per_block - 1) / per_block;
    if (blocks > 0x7fffffff) return fail(AFHIP_E_INVALID, "transform: array too large for one launch");
    const dim3 grid((unsigned)blocks), block(WG);
    hipStream_t st = (hipStream_t)stream;
    switch (ta.tf) {
        case TF_POWI: hipLaunchKernelGGL(k_transform<TF_POWI>, grid, block, 0, st, ta); break;
        case TF_POW: hipLaunchKernelGGL(k_transform<TF_POW>, grid, block, 0, st, ta); break;
        case TF_HINGE: hipLaunchKernelGGL(k_transform<TF_HINGE>, grid, block, 0, st, ta); break;
        default: hipLaunchKernelGGL(k_transform<TF_INTER>, grid, block, 0, st, ta); break;
    }
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

extern "C" int afhip_spatial_wavg(const afhip_csr* csr, const double* x_dev, int64_t K, int64_t nt,
                                  double* num_dev, double* den_dev, double* res_dev, void* stream) {
    if (!csr || !x_dev || !res_dev || K <= 0 || nt < 0) return fail(AFHIP_E_INVALID, "spatial_wavg: bad arguments");
    if (nt == 0) return AFHIP_OK;
    GUARD_DEVICE(csr->device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t C = csr->n_cells, Q = (K + 1) * nt;
    double *panel = nullptr, *sums = nullptr;
    HIP_TRY(hipMallocAsync((void**)&panel, (size_t)(C * Q) * sizeof(double), st));
    hipError_t e = hipMallocAsync((void**)&sums, (size_t)std::max<int64_t>(spmm_rows(csr) * Q, 1) * sizeof(double), st);
    int rc = AFHIP_OK;
    if (e != hipSuccess) {
        rc = fail(AFHIP_E_HIP, "hipMallocAsync failed: %s", hipGetErrorString(e));
    } else {
        const int64_t n = C * nt;
        hipLaunchKernelGGL(k_validity_panel, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, st, x_dev, panel, C, nt, (int)K);
        if ((e = hipGetLastError()) != hipSuccess) rc = fail(AFHIP_E_HIP, "k_validity_panel launch failed: %s", hipGetErrorString(e));
        if (!rc) rc = launch_spmm(csr, panel, sums, Q, st, false);
        const int64_t m = csr->R * nt;                            // one thread per (region, time step)
        if (!rc && m) {
            // (more names than one pass holds: k_panel_divide keeps a record of MAX_COLS + 1 values in registers)
            if (K > MAX_COLS) hipLaunchKernelGGL(k_panel_divide_wide, dim3((unsigned)((m + WG - 1) / WG)), dim3(WG), 0, st, sums, num_dev, den_dev, res_dev, csr->R, nt, (int)K);
            else hipLaunchKernelGGL(k_panel_divide, dim3((unsigned)((m + WG - 1) / WG)), dim3(WG), 0, st, sums, num_dev, den_dev, res_dev, csr->R, nt, (int)K);
            if ((e = hipGetLastError()) != hipSuccess) rc = fail(AFHIP_E_HIP, "k_panel_divide launch failed: %s", hipGetErrorString(e));
        }
    }
    // both scratch buffers go back on every path (stream-ordered: after the kernels that read them)
    (void)hipFreeAsync(panel, st);
    if (sums) (void)hipFreeAsync(sums, st);
    return rc;
}

// ---------------------------------------------------------------------------------------
// plans
// ---------------------------------------------------------------------------------------
// workgroups of kernel `fn` one CU holds at once (registers, LDS, wave slots)
static int resident_wgs_per_cu(const void* fn, int wg, size_t lds) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, wg, lds) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

extern "C" int afhip_plan_create(const afhip_plan_desc* desc, afhip_plan** out) {
    if (!out) return fail(AFHIP_E_INVALID, "plan_create: out is NULL");
    *out = nullptr;
    auto* pl = new afhip_plan();
    pl->device = current_device();
    DeviceFacts dev;
    dev.cu_count = cu_count(pl->device);
    dev.resident_wgs = resident_wgs_per_cu;
    int rc;
    if ((rc = build_plan(desc, dev, pl)) || (rc = pl->d_ob.upload(pl->ob)) || (rc = pl->d_gtab.upload(pl->gtab)) ||
        (rc = pl->d_chunks.upload(pl->chunks)) || (rc = pl->d_slot_ptr.upload(pl->slot_ptr)) ||
        (pl->hb_cells > 0 && (rc = pl->d_cmap.upload(std::vector<uint8_t>(pl->hb_cmap, pl->hb_cmap + sizeof pl->hb_cmap))))) {
        delete pl;
        return rc;
    }
    *out = pl;
    return AFHIP_OK;
}

extern "C" void afhip_plan_destroy(afhip_plan* plan) {
    if (!plan) return;
    DeviceGuard g(plan->device);
    delete plan;
}

extern "C" int afhip_plan_device(const afhip_plan* plan) { return plan ? plan->device : -1; }

// A plan's tables and scratch live on plan->device: a cube (or a second cube, an output, a workspace) on another card would be
// read or written across xGMI at best and, with peer access off, fault.  Refuse it before anything is launched (pointers the
// runtime cannot classify are let through).
static int check_ptr_device(const afhip_plan* pl, const void* ptr_dev, const char* who, const char* what) {
    const int dev = pointer_device(ptr_dev);
    if (dev >= 0 && dev != pl->device)
        return fail(AFHIP_E_INVALID, "%s: %s lives on device %d but the plan was created on device %d "
                    "(create the plan with the data's device current)", who, what, dev, pl->device);
    return AFHIP_OK;
}
static int check_cube_device(const afhip_plan* pl, const void* cube_dev, const char* who) { return check_ptr_device(pl, cube_dev, who, "the cube"); }

extern "C" int afhip_plan_bind_inter(afhip_plan* plan, int column, const void* inter_dev, int dtype) {
    if (!plan || column < 0 || column >= plan->K) return fail(AFHIP_E_INVALID, "plan_bind_inter: no such column");
    if (plan->cols[(size_t)column].tf != TF_INTER) return fail(AFHIP_E_INVALID, "plan_bind_inter: column %d has no inter transform", column);
    if (!inter_dev || (dtype != AFHIP_F32 && dtype != AFHIP_F64)) return fail(AFHIP_E_INVALID, "plan_bind_inter: NULL array or bad dtype");
    int rcd = check_ptr_device(plan, inter_dev, "plan_bind_inter", "the second cube");
    if (rcd) return rcd;
    plan->cols[(size_t)column].inter = inter_dev;
    plan->cols[(size_t)column].inter_f32 = dtype == AFHIP_F32 ? 1 : 0;
    return AFHIP_OK;
}

// `dtype`: the storage the packing belongs to (AFHIP_I16 / AFHIP_U16) — a fill outside its range could never match a stored value
static int check_packing(const afhip_packing* p, int dtype, const char* who) {
    static_assert(sizeof(afhip_packing) == sizeof(PackArgs), "afhip_packing is PackArgs");
    static_assert(offsetof(afhip_packing, pad) == offsetof(PackArgs, is_unsigned), "the public pad is the library's signedness field");
    if (!p) return fail(AFHIP_E_INVALID, "%s: the packing is NULL", who);
    if (p->n_pairs < 0 || p->n_pairs > MAX_PACK_PAIRS) return fail(AFHIP_E_INVALID, "%s: n_pairs must be 0..%d, got %d", who, MAX_PACK_PAIRS, p->n_pairs);
    if (dtype == AFHIP_U16) {
        if (p->has_fill && (p->fill < 0 || p->fill > UINT16_MAX)) return fail(AFHIP_E_INVALID, "%s: the fill value %d is no uint16", who, p->fill);
    } else if (p->has_fill && (p->fill < INT16_MIN || p->fill > INT16_MAX)) {
        return fail(AFHIP_E_INVALID, "%s: the fill value %d is no int16", who, p->fill);
    }
    return AFHIP_OK;
}

// the caller's packing as the kernels' record: has_fill normalised, the signedness from `dtype` (the caller's pad is not read)
static PackArgs pack_args_of(const afhip_packing* p, int dtype) {
    PackArgs pa;
    memcpy(&pa, p, sizeof pa);
    pa.has_fill = p->has_fill ? 1 : 0;
    pa.is_unsigned = dtype == AFHIP_U16 ? 1 : 0;
    return pa;
}

// Every check comes before the first write: a refused bind leaves the earlier binding in place.
extern "C" int afhip_plan_bind_packings(afhip_plan* plan, const afhip_packing* rules, const int64_t* bounds, int32_t n) {
    const char* who = "plan_bind_packings";
    if (!plan) return fail(AFHIP_E_INVALID, "%s: plan is NULL", who);
    if (!is_packed_dtype(plan->desc.dtype)) return fail(AFHIP_E_INVALID, "%s: the plan's dtype is not AFHIP_I16 or AFHIP_U16", who);
    if (!rules || !bounds) return fail(AFHIP_E_INVALID, "%s: the rules or the bounds are NULL", who);
    const int64_t T = plan->desc.T;
    if (n < 1 || (int64_t)n > T) return fail(AFHIP_E_INVALID, "%s: %d rules for %lld time steps (1 .. T)", who, n, (long long)T);
    if (bounds[0] != 0 || bounds[n] != T)
        return fail(AFHIP_E_INVALID, "%s: the bounds must run from 0 to T = %lld, got %lld .. %lld", who, (long long)T, (long long)bounds[0], (long long)bounds[n]);
    for (int32_t i = 0; i < n; ++i) {
        if (bounds[i + 1] <= bounds[i]) return fail(AFHIP_E_INVALID, "%s: the bounds must strictly increase (rule %d covers no time step)", who, i);
        int rc = check_packing(&rules[i], plan->desc.dtype, who);
        if (rc) return rc;
    }
    plan->unpack = pack_args_of(&rules[0], plan->desc.dtype);
    plan->unpack_bound = true;
    plan->rules.clear();
    plan->rule_bounds.clear();
    if (n > 1) {
        for (int32_t i = 0; i < n; ++i) plan->rules.push_back(pack_args_of(&rules[i], plan->desc.dtype));
        plan->rule_bounds.assign(bounds, bounds + n + 1);
    }
    return AFHIP_OK;
}

extern "C" int afhip_plan_bind_packing(afhip_plan* plan, const afhip_packing* p) {
    if (!plan) return fail(AFHIP_E_INVALID, "plan_bind_packing: plan is NULL");
    if (!is_packed_dtype(plan->desc.dtype)) return fail(AFHIP_E_INVALID, "plan_bind_packing: the plan's dtype is not AFHIP_I16 or AFHIP_U16");
    int rc = check_packing(p, plan->desc.dtype, "plan_bind_packing");
    if (rc) return rc;
    const int64_t bounds[2] = {0, plan->desc.T};
    if (plan->desc.T < 1) {                 // (a plan without time steps launches nothing: the one rule is kept as before)
        plan->unpack = pack_args_of(p, plan->desc.dtype);
        plan->unpack_bound = true;
        plan->rules.clear();
        plan->rule_bounds.clear();
        return AFHIP_OK;
    }
    return afhip_plan_bind_packings(plan, p, bounds, 1);
}

// The device table of a multi-rule plan, brought up to date in front of a run's kernel on the run's stream `st` (see afhip_plan::rules).
static int upload_rules(afhip_plan* pl, hipStream_t st) {
    const size_t n = pl->rules.size(), bb = (n + 1) * sizeof(int64_t), bytes = bb + n * sizeof(PackArgs);
    std::vector<unsigned char> img(bytes);
    memcpy(img.data(), pl->rule_bounds.data(), bb);
    memcpy(img.data() + bb, pl->rules.data(), n * sizeof(PackArgs));
    if (pl->d_rules && img == pl->rules_dev_image) return AFHIP_OK;
    if (bytes > pl->d_rules_bytes) {
        if (pl->d_rules) { pl->retired.push_back(pl->d_rules); pl->d_rules = nullptr; pl->d_rules_bytes = 0; }
        HIP_TRY(hipMalloc(&pl->d_rules, bytes));
        pl->d_rules_bytes = bytes;
    }
    if (!pl->rules_ev) HIP_TRY(hipEventCreateWithFlags(&pl->rules_ev, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(pl->rules_ev));        // the earlier copy has read rules_stage
    pl->rules_stage = img;
    pl->rules_dev_image.clear();
    HIP_TRY(hipMemcpyAsync(pl->d_rules, pl->rules_stage.data(), bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(pl->rules_ev, st));
    pl->rules_dev_image.swap(img);
    return AFHIP_OK;
}

// afhip_unpack_i16 / afhip_unpack_u16: one kernel, the signedness in its record
static int unpack_16(const void* q_dev, int64_t n, const afhip_packing* p, int dtype, float* out_dev, void* stream, const char* who) {
    if (!q_dev || !out_dev || n < 0) return fail(AFHIP_E_INVALID, "%s: NULL array or negative size", who);
    int rc = check_packing(p, dtype, who);
    if (rc) return rc;
    if (n == 0) return AFHIP_OK;
    if ((uintptr_t)q_dev % 8 != 0 || (uintptr_t)out_dev % 16 != 0) return fail(AFHIP_E_INVALID, "%s: q_dev must be 8-byte and out_dev 16-byte aligned", who);
    const PackArgs pa = pack_args_of(p, dtype);
    const int64_t lanes = (n + 3) / 4, blocks = (lanes + WG - 1) / WG;
    if (blocks > 0x7fffffff) return fail(AFHIP_E_INVALID, "%s: array too large for one launch", who);
    GUARD_DEVICE(pointer_device(out_dev));
    hipLaunchKernelGGL(k_unpack_i16, dim3((unsigned)blocks), dim3(WG), 0, (hipStream_t)stream, (const int16_t*)q_dev, n, pa, out_dev);
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}
extern "C" int afhip_unpack_i16(const void* q_dev, int64_t n, const afhip_packing* p, float* out_dev, void* stream) {
    return unpack_16(q_dev, n, p, AFHIP_I16, out_dev, stream, "unpack_i16");
}
extern "C" int afhip_unpack_u16(const void* q_dev, int64_t n, const afhip_packing* p, float* out_dev, void* stream) {
    return unpack_16(q_dev, n, p, AFHIP_U16, out_dev, stream, "unpack_u16");
}

extern "C" int64_t afhip_plan_workspace_bytes(const afhip_plan* plan) {
    if (!plan) return 0;
    return plan->ws_partial;
}

// rows of the sums buffer a spatial stage needs: the regions + the scratch rows of cut regions
static int64_t spmm_rows(const afhip_csr* csr) { return csr->R + csr->n_extra; }
static int64_t sums_bytes_of(const afhip_plan* plan, const afhip_csr* csr) {
    const int64_t Q = (int64_t)(plan->K + 1) * plan->desc.P;
    return (std::max<int64_t>(spmm_rows(csr) * Q, 1) * 8 + 255) / 256 * 256;
}

extern "C" int64_t afhip_plan_run_workspace_bytes(const afhip_plan* plan, const afhip_csr* csr) {
    if (!plan || !csr) return 0;
    return plan->ws_partial + plan->ws_panel + sums_bytes_of(plan, csr);
}

extern "C" int afhip_plan_describe(const afhip_plan* plan, char* buf, int buf_len) {
    if (!plan) return 0;
    int64_t min_len = INT64_MAX, max_len = 0;
    for (auto& c : plan->chunks) { min_len = std::min(min_len, c.k_hi - c.k_lo); max_len = std::max(max_len, c.k_hi - c.k_lo); }
    char tmp[1024], cg[48] = "", cm[24] = "";
    if (feat_has(plan->variant->feat, FEAT_CELL_MAP)) snprintf(cm, sizeof cm, " cells=%d", plan->hb_cells);
    if (plan->last_counts_lanes > 0) snprintf(cg, sizeof cg, " last-run=count-gather/%d-lane", plan->last_counts_lanes);
    else if (plan->last_spatial) snprintf(cg, sizeof cg, "%s", plan->last_spatial == 1 ? " last-run=slot-gather" : " last-run=panel");
    int n = snprintf(tmp, sizeof tmp,
                     "variant=%s pipe=%d vec=%d stat=%d slots=%d kmax=%d depth=%d%s | T=%lld cells=%lld K=%d G1=%lld P=%lld | "
                     "wg=%d tiles=%lld chunks=%zu (steps %lld..%lld) out_slots=%lld%s%s | workspace=%.1f MiB%s%s",
                     plan->variant->name, plan->variant->pipe, plan->variant->vec, plan->variant->stat, plan->variant->nthr,
                     plan->variant->kmax, plan->variant->depth, cm, (long long)plan->desc.T, (long long)plan->desc.n_cells,
                     plan->K, (long long)plan->desc.G1, (long long)plan->desc.P, plan->wg, (long long)plan->tiles, plan->chunks.size(),
                     (long long)(plan->chunks.empty() ? 0 : min_len), (long long)max_len, (long long)plan->n_slots,
                     plan->packed ? (plan->pk.nw == 2 ? " packed-counts16" : " packed-counts32")
                                  : (plan->last_route == 1 ? " last-run=region-fused" : (plan->rf_plan_ok ? " region-fused-capable" : "")),
                     cg, (double)(plan->ws_partial + plan->ws_panel) / (1024.0 * 1024.0),
                     plan->last_ws == 1 ? " (caller-owned)" : (plan->last_ws == 2 ? " (plan-owned hipMalloc)" : ""),
                     plan->desc.dtype == AFHIP_U16 ? " storage=uint16" : (plan->desc.dtype == AFHIP_I16 ? " storage=int16" : ""));
    if (buf && buf_len > 0) snprintf(buf, buf_len, "%s", tmp);
    return n + 1;
}

// Layout of the run sums: slot-major [slots][runs][K + 1] (a period end's stores of one wave side by side: one or two cache lines per
// store instruction; k_rf_reduce then deals its (region, period) pairs period-major, so that neighbouring regions read neighbouring
// runs of ONE slot) or run-major [runs][slots][K + 1] (a run's periods side by side: k_rf_reduce reads whole lines — its time falls to
// a half ... a fifth — but every run a wave closes is then a cache line of its own at every period end: +0.25 ... 0.5 ms on the general
// streaming forms, next to nothing on the short-group forms).  Measured (profiles/r04_rf_layout.txt, both tables): run-major pays on the
// short-group forms from ~5e7 (run, period, column) gathers (daily sine_dd on 0.1 deg 12.3 -> 9.5 ms, weekly 5.12 -> 4.60, 6-hourly daily
// 3.21 -> 2.96) and on the general forms nowhere below 5e8 (float64 daily configs[1] panel 4.49 -> 4.87, float32 2.76 -> 2.90).
static bool rf_run_major(const afhip_plan* pl, const afhip_csr::RfTab* rf) {
    if (pl->rf_layout >= 0) return pl->rf_layout == 1;
    return (double)rf->n_runs * (double)pl->desc.P * (double)(pl->K + 1) >= (pl->variant->pair() ? 5e7 : 5e8);
}

static int launch_temporal(afhip_plan* pl, const void* cube, double* partial, hipStream_t st, const afhip_csr::RfTab* rf = nullptr) {
    if (pl->chunks.empty()) return AFHIP_OK;
    for (int j = 0; j < pl->K; ++j)
        if (pl->cols[(size_t)j].tf == TF_INTER && !pl->cols[(size_t)j].inter)
            return fail(AFHIP_E_INVALID, "column %d multiplies by a second array (AFHIP_TF_INTER) that was never bound: call afhip_plan_bind_inter first", j);
    if (is_packed_dtype(pl->desc.dtype) && !pl->unpack_bound)
        return fail(AFHIP_E_INVALID, "the plan reads a 16-bit-packed cube (AFHIP_I16 / AFHIP_U16) whose packing was never bound: call afhip_plan_bind_packing first");
    FusedArgs fa{};
    fa.unpack = pl->unpack;
    fa.n_rules = 1;
    if (is_packed_dtype(pl->desc.dtype) && pl->rules.size() > 1) {
        int rc = upload_rules(pl, st);
        if (rc) return rc;
        fa.n_rules = (int32_t)pl->rules.size();
        fa.pack_bounds = (const int64_t*)pl->d_rules;
        fa.pack_rules = (const PackArgs*)((const char*)pl->d_rules + (pl->rules.size() + 1) * sizeof(int64_t));
    }
    fa.cube = cube; fa.C = pl->desc.n_cells;
    fa.gtab = pl->d_gtab.p; fa.chunks = pl->d_chunks.p;
    fa.partial = partial; fa.K = pl->K; fa.nthr = pl->nthr;
    fa.n_tiles = (int32_t)pl->tiles;
    fa.xcd_remap = 1;        // measured +0.2..1 % on configs[1] (profiles/r01_xcd_remap.txt): harmless, kept on
    fa.sine_tab = nullptr;
    if (pl->has_sine) {
        int rc = sine_table_dev(pl->device, pl->variant->sine_p2(), &fa.sine_tab);
        if (rc) return rc;
    }
    for (int i = 0; i < pl->nthr; ++i) fa.thr[i] = pl->thr[(size_t)i];
    for (int i = pl->nthr; i < MAX_THR; ++i) {       // padded slots never fire
        fa.thr[i] = ThrSlot{};
        fa.thr[i].t0 = INFINITY; fa.thr[i].t1 = -INFINITY;
        fa.thr[i].t0f = INFINITY; fa.thr[i].t1f = -INFINITY;
    }
    for (int j = 0; j < pl->K; ++j) {
        const ColOp& c = pl->cols[(size_t)j];
        fa.cols[j] = c;
        fa.ccode[j] = (uint32_t)c.src | ((uint32_t)c.tf << 4) | ((uint32_t)(uint8_t)(int8_t)c.tf_iarg << 8);
    }
    fa.packed = pl->packed ? 1 : 0;
    fa.pk_nw = pl->pk.nw; fa.pk_mask = pl->pk.mask;
    for (int j = 0; j < MAX_COLS; ++j) { fa.pk_word[j] = pl->pk.word[j]; fa.pk_shift[j] = pl->pk.shift[j]; }
    dim3 grid((unsigned)pl->tiles, (unsigned)pl->chunks.size());
    void* args[] = {&fa};
    size_t lds = plan_lds_bytes(pl);
    const void* fn = pl->variant->fn;
    if (rf) {       // region-fused period ends: the twin variant, per-run sums into the partial area, a parking block per lane in LDS
        fn = pl->variant_rf->fn;
        lds = (lds + 15) / 16 * 16;
        fa.rf_lds_off = (int32_t)lds;
        lds += (size_t)pl->wg * (size_t)rf_lane_bytes(pl->variant->vec);
        fa.rf_w = rf->w2.p; fa.rf_lane = rf->lane.p; fa.rf_tile = rf->tile.p; fa.rf_out = partial;
        fa.rf_slot_stride = rf_run_major(pl, rf) ? (int64_t)(pl->K + 1) : rf->n_runs * (pl->K + 1);
        fa.rf_run_stride = rf_run_major(pl, rf) ? pl->n_slots * (pl->K + 1) : (int64_t)(pl->K + 1);
        fa.rf_x = rf->n_xcells ? rf->xidx.p : nullptr; fa.rf_nx = rf->n_xcells;
        fa.rf_ex = partial + pl->n_slots * rf->n_runs * (pl->K + 1);           // behind the run sums
    }
    if (pl->variant->hb()) {
        fa.hb_n = pl->hb_n; fa.hb_c1 = pl->hb_c1; fa.hb_c0 = pl->hb_c0;
        fa.hb_c1f = (float)pl->hb_c1; fa.hb_c0f = (float)pl->hb_c0;
        fa.hb_shift = pl->wg == 64 ? 6 : (pl->wg == 128 ? 7 : 8);
        for (int i = 0; i < MAX_THR; ++i) fa.hb_bin_of_slot[i] = pl->hb_bin_of_slot[i];
        // (a packed cube's histogram forms compare in float32 and never read the double edges — whose bytes hold the unpack rule stored above)
        const bool double_edges = !is_packed_dtype(pl->desc.dtype);
        for (int k = 0; k <= pl->hb_n; ++k) {
            const double t = pl->hb_edge[k];
            const float f = (float)t;
            if (double_edges) fa.hb_edge[k] = t;
            fa.hb_dn[k] = (double)f > t ? std::nextafterf(f, -INFINITY) : f;     // largest float <= t
            fa.hb_up[k] = (double)f < t ? std::nextafterf(f, INFINITY) : f;      // smallest float >= t
        }
        if (feat_has(pl->variant->feat, FEAT_CELL_MAP)) { fa.hb_cmap = pl->d_cmap.p; fa.hb_cells = pl->hb_cells; }      // (shares the bytes of the next four)
        else { fa.hb_w = pl->hb_w; fa.hb_lo0 = pl->hb_lo0; fa.hb_gl = pl->hb_gl; fa.hb_gh = pl->hb_gh; }
        fa.hb_wf = (float)pl->hb_w; fa.hb_lo0f = (float)pl->hb_lo0; fa.hb_glf = (float)pl->hb_gl; fa.hb_ghf = (float)pl->hb_gh;
        fa.hb_c0b = pl->hb_c0b; fa.hb_c0bf = (float)pl->hb_c0b;
        // wide end bins (FEAT_END_BINS): the slots whose thr[] entries hold the outer limits L (t0 / t0f) and U (t1 / t1f)
        fa.hb_ends = feat_has(pl->variant->feat, FEAT_END_BINS) ? (pl->hb_slot_lo | (pl->hb_slot_hi << 8)) : 0;
    }
    HIP_TRY(hipLaunchKernel(fn, grid, dim3((unsigned)pl->wg), args, lds, st));
    return AFHIP_OK;
}

static int launch_combine(afhip_plan* pl, const double* partial, double* cells, double* panel, hipStream_t st) {
    const int64_t C = pl->desc.n_cells, P = pl->desc.P;
    if (P == 0) return AFHIP_OK;
    CombineArgs ca{};
    ca.partial = partial; ca.slot_ptr = pl->d_slot_ptr.p; ca.outer_bounds = pl->d_ob.p;
    ca.cells_out = cells; ca.panel = panel; ca.C = C; ca.P = P; ca.K = pl->K;
    ca.pk = pl->packed ? pl->pk : PackFmt{};
    for (int j = 0; j < pl->K; ++j) {
        ca.outer[j] = pl->cols[(size_t)j].outer;
        ca.round_final[j] = (pl->cols[(size_t)j].rounding & AFHIP_ROUND_FINAL) ? 1 : 0;
    }
    if (P >= 4 && panel) {      // many periods: the tiled kernel writes the panel in contiguous runs
        dim3 grid((unsigned)((C + CT_CELLS - 1) / CT_CELLS), (unsigned)((P + CT_PER - 1) / CT_PER));
        if (grid.y > 65535) return fail(AFHIP_E_UNSUPPORTED, "more than 524,280 output periods in one call");
        hipLaunchKernelGGL(k_combine_slots_tiled, grid, dim3(WG), 0, st, ca);
    } else {
        dim3 grid((unsigned)((C + WG - 1) / WG), (unsigned)std::min<int64_t>(P, 65535));   // strides over periods
        hipLaunchKernelGGL(k_combine_slots, grid, dim3(WG), 0, st, ca);
    }
    HIP_TRY(hipGetLastError());
    return AFHIP_OK;
}

// sums[row][p][K + 1] straight from partial (k_csr_spmm_slots): slot merge, shared validity and the weighted sums of every
// (segment, period) in one pass; then the pieces of cut rows.  The lanes per (segment, period) follow the table's mean
// segment length — 64 for county-sized rows on a fine grid (and then bit-identical to combine + k_csr_spmm_wave), 8 for
// tables whose regions hold a handful of cells.
static int launch_spmm_slots(afhip_plan* pl, const afhip_csr* csr, const double* partial, hipStream_t st,
                             double* num_dev, double* den_dev, double* res_dev, bool* divided) {
    const int64_t P = pl->desc.P, K = pl->K, Q = (K + 1) * P;
    if (csr->nseg * P == 0) return AFHIP_OK;
    SlotSpmmArgs sa{};
    sa.seg_ptr = csr->seg_ptr.p; sa.dst = csr->seg_dst.p; sa.cols = csr->cols.p; sa.w = csr->w.p;
    sa.partial = partial; sa.slot_ptr = pl->d_slot_ptr.p; sa.outer_bounds = pl->d_ob.p; sa.out = pl->sums;
    sa.nseg = csr->nseg; sa.P = P; sa.C = pl->desc.n_cells; sa.K = (int32_t)K;
    sa.p_major = pl->slot_spmm_order >= 0 ? pl->slot_spmm_order : (P >= 8 ? 1 : 0);
    // no row of the table is cut: a segment IS a region, and the lane that holds its K + 1 sums finishes the panel (no divide kernel)
    *divided = csr->n_split == 0 && csr->nseg == csr->R;
    if (*divided) { sa.num = num_dev; sa.den = den_dev; sa.res = res_dev; sa.R = csr->R; }
    for (int j = 0; j < pl->K; ++j) {
        sa.outer[j] = pl->cols[(size_t)j].outer;
        sa.round_final[j] = (pl->cols[(size_t)j].rounding & AFHIP_ROUND_FINAL) ? 1 : 0;
    }
    const int64_t mean_len = csr->nnz / std::max<int64_t>(csr->nseg, 1);
    int sub = mean_len > 32 ? 64 : (mean_len > 16 ? 32 : (mean_len > 8 ? 16 : 8));
    if (pl->slot_spmm_sub) sub = pl->slot_spmm_sub;
    const int64_t pairs = csr->nseg * P;
    const int64_t blocks = (pairs * sub + WG - 1) / WG;
    if (blocks > INT32_MAX) return fail(AFHIP_E_UNSUPPORTED, "plan_run: %lld (segment, period) pairs in one call", (long long)pairs);
#define AFHIP_SLOTS_SUB(KB)                                                                                                   \
    switch (sub) {                                                                                                            \
        case 8: hipLaunchKernelGGL((k_csr_spmm_slots<KB, 8>), dim3((unsigned)blocks), dim3(WG), 0, st, sa); break;            \
        case 16: hipLaunchKernelGGL((k_csr_spmm_slots<KB, 16>), dim3((unsigned)blocks), dim3(WG), 0, st, sa); break;          \
        case 32: hipLaunchKernelGGL((k_csr_spmm_slots<KB, 32>), dim3((unsigned)blocks), dim3(WG), 0, st, sa); break;          \
        default: hipLaunchKernelGGL((k_csr_spmm_slots<KB, 64>), dim3((unsigned)blocks), dim3(WG), 0, st, sa); break;          \
    }
    if (K <= 2) { AFHIP_SLOTS_SUB(2) }
    else if (K <= 4) { AFHIP_SLOTS_SUB(4) }
    else if (K <= 8) { AFHIP_SLOTS_SUB(8) }
    else { AFHIP_SLOTS_SUB(16) }
#undef AFHIP_SLOTS_SUB
    HIP_TRY(hipGetLastError());
    if (csr->n_split) {
        const int64_t n = csr->n_split * Q;
        hipLaunchKernelGGL(k_csr_combine_segments, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, st, pl->sums, csr->split_row.p,
                           csr->split_ptr.p, csr->R, Q, csr->n_split);
        HIP_TRY(hipGetLastError());
    }
    return AFHIP_OK;
}

// The scratch of a run: the caller's block when given (checked for size, alignment and device: nothing below allocates, frees
// or synchronises then), else the plan's own, grown at need — the outgrown block is kept until afhip_plan_destroy, because
// kernels of an earlier run on another stream may still read it and a hipFree would wait for the whole device.
static int ensure_ws(afhip_plan* pl, int64_t bytes, void* user_ws, int64_t user_bytes, const char* who, char** base) {
    if (user_ws) {
        if (user_bytes < bytes)
            return fail(AFHIP_E_INVALID, "%s: the workspace holds %lld bytes, the run needs %lld (afhip_plan_run_workspace_bytes / afhip_plan_workspace_bytes)",
                        who, (long long)user_bytes, (long long)bytes);
        if ((uintptr_t)user_ws % 256 != 0) return fail(AFHIP_E_INVALID, "%s: the workspace must be 256-byte aligned", who);
        int rc = check_ptr_device(pl, user_ws, who, "the workspace");
        if (rc) return rc;
        *base = (char*)user_ws;
        pl->last_ws = 1;
        return AFHIP_OK;
    }
    if (pl->own_ws_bytes < bytes) {
        if (pl->own_ws) { pl->retired.push_back(pl->own_ws); pl->own_ws = nullptr; pl->own_ws_bytes = 0; }
        HIP_TRY(hipMalloc(&pl->own_ws, (size_t)bytes));
        pl->own_ws_bytes = bytes;
    }
    *base = (char*)pl->own_ws;
    pl->last_ws = 2;
    return AFHIP_OK;
}

extern "C" int afhip_plan_run_temporal(afhip_plan* plan, const void* cube_dev, double* cells_dev,
                                       void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (!plan || !cube_dev || !cells_dev) return fail(AFHIP_E_INVALID, "plan_run_temporal: NULL argument");
    int rcd = check_cube_device(plan, cube_dev, "plan_run_temporal");
    if (!rcd) rcd = check_ptr_device(plan, cells_dev, "plan_run_temporal", "the per-cell output");
    if (rcd) return rcd;
    GUARD_DEVICE(plan->device);
    hipStream_t st = (hipStream_t)stream;
    char* base;
    int rc = ensure_ws(plan, plan->ws_partial, workspace_dev, workspace_bytes, "plan_run_temporal", &base);
    if (rc) return rc;
    double* partial = (double*)base;
    if ((rc = launch_temporal(plan, cube_dev, partial, st))) return rc;
    return launch_combine(plan, partial, cells_dev, nullptr, st);
}

extern "C" int afhip_plan_run(afhip_plan* plan, const void* cube_dev, const afhip_csr* csr,
                              double* num_dev, double* den_dev, double* res_dev, double* cells_dev,
                              void* workspace_dev, int64_t workspace_bytes, void* stream, float* kernel_ms) {
    if (!plan || !cube_dev || !csr || !res_dev) return fail(AFHIP_E_INVALID, "plan_run: NULL argument");
    if (csr->n_cells != plan->desc.n_cells)
        return fail(AFHIP_E_INVALID, "plan_run: CSR has %lld cells, plan has %lld", (long long)csr->n_cells, (long long)plan->desc.n_cells);
    if (csr->device != plan->device)
        return fail(AFHIP_E_INVALID, "plan_run: the CSR lives on device %d, the plan on device %d", csr->device, plan->device);
    int rcd = check_cube_device(plan, cube_dev, "plan_run");
    if (!rcd) rcd = check_ptr_device(plan, res_dev, "plan_run", "the result panel");
    if (!rcd && num_dev) rcd = check_ptr_device(plan, num_dev, "plan_run", "the numerator panel");
    if (!rcd && den_dev) rcd = check_ptr_device(plan, den_dev, "plan_run", "the denominator panel");
    if (!rcd && cells_dev) rcd = check_ptr_device(plan, cells_dev, "plan_run", "the per-cell output");
    if (rcd) return rcd;
    GUARD_DEVICE(plan->device);
    hipStream_t st = (hipStream_t)stream;
    const int64_t K = plan->K, P = plan->desc.P, Q = (K + 1) * P;
    // partial | panel | sums[rows][Q] in one block: the caller's workspace when given, else the plan's own
    char* base;
    int rc = ensure_ws(plan, afhip_plan_run_workspace_bytes(plan, csr), workspace_dev, workspace_bytes, "plan_run", &base);
    if (rc) return rc;
    double* partial = (double*)base;
    double* panel = (double*)(base + plan->ws_partial);
    plan->sums = (double*)(base + plan->ws_partial + plan->ws_panel);
    if (kernel_ms) {
        for (auto& e : plan->ev) if (!e) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipEventRecord(plan->ev[0], st));
    }
    const bool exact = plan->desc.exact_order != 0 || spmm_serial_env();
    // region-fused period ends: the plan allows it, no per-cell output is wanted, and the table's runs exist (built on first use) and
    // fit the partial area (n_runs * 3 <= cells and K + 1 <= 2 K ... checked in bytes)
    const afhip_csr::RfTab* rf = nullptr;
    if (plan->rf_plan_ok && !exact && !cells_dev && !plan->packed) {
        rf = rf_table(const_cast<afhip_csr*>(csr), plan->variant->vec);
        if (rf && plan->n_slots * (rf->n_runs + rf->n_xcells) * (K + 1) * 8 > plan->ws_partial) rf = nullptr;
    }
    const bool prof = !plan->prof_ev.empty() && (size_t)(2 * plan->prof_count + 1) < plan->prof_ev.size();
    if (prof) HIP_TRY(hipEventRecord(plan->prof_ev[(size_t)(2 * plan->prof_count)], st));
    if ((rc = launch_temporal(plan, cube_dev, partial, st, rf))) return rc;
    if (prof) { HIP_TRY(hipEventRecord(plan->prof_ev[(size_t)(2 * plan->prof_count + 1)], st)); ++plan->prof_count; }
    if (kernel_ms) HIP_TRY(hipEventRecord(plan->ev[1], st));
    plan->last_route = rf ? 1 : 0;
    plan->last_counts_lanes = -1;
    plan->last_spatial = 0;
    bool divided = false;          // the count gather wrote num / den / res itself
    if (rf) {
        // a region's runs added in run order -> sums[r][p][K + 1] (no pieces: rows [0, R) only)
        const int64_t n = csr->R * P * (K + 1);
        if (n) {
            uint32_t mean_mask = 0;
            for (int j = 0; j < plan->K; ++j) if (plan->cols[(size_t)j].outer == OUT_MEAN) mean_mask |= 1u << j;
            hipLaunchKernelGGL(k_rf_reduce, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, st, (const double*)partial, rf->reg_ptr.p, rf->reg_runs.p,
                               plan->d_slot_ptr.p, plan->d_ob.p, mean_mask, (const double*)(partial + plan->n_slots * rf->n_runs * (K + 1)), rf->n_xcells,
                               rf->xreg_ptr.p, rf->xcell.p, rf->xw.p, plan->sums, csr->R, P, (int)(K + 1), rf->n_runs,
                               rf_run_major(plan, rf) ? (int64_t)(K + 1) : rf->n_runs * (K + 1), rf_run_major(plan, rf) ? plan->n_slots * (K + 1) : (int64_t)(K + 1),
                               (!rf_run_major(plan, rf) && P >= 8) ? 1 : 0);
            HIP_TRY(hipGetLastError());
        }
    } else if (plan->packed && !cells_dev && plan->n_slots <= P && plan->counts_spmm) {
        // bin-count plan, no per-cell output wanted: the weighted sums gather the packed counts directly
        // (every period has at most one slot: single-level plans are never split); long rows in segments unless exact
        const int64_t nv = exact ? csr->R : csr->nseg, nq = nv * P;
        if (nq) {
            // rows that are never cut (exact order, or a table without long rows): the gather finishes the panel itself, no divide kernel
            divided = (exact || csr->n_split == 0) && nv == csr->R;
            // lanes per pair: one (the table's order: `exact_order`), or a group of lanes over the row's entries with the pairs dealt period-major
            // (one lane per pair leaves a job of few periods with few threads, each walking its row alone: annual bins on 3,100 county-sized
            // regions 0.365 ms against 0.030 with sixteen lanes per pair; many periods turn it around — the group's lanes idle on short
            // rows and every pair pays the group's adds: configs[3], 17 entries x 251 periods, 0.217 against 0.43.  Measured crossover:
            // about as many periods as a row has entries; profiles/r04_counts_gather.txt)
            const int64_t nnz_rows = csr->h_indptr.empty() ? 0 : csr->h_indptr.back();
            const double entries = nv > 0 ? (double)nnz_rows / (double)nv : 0.0;
            const int sub_rule = ((double)P < entries) ? (entries < 12.0 ? 8 : 16) : 0;
            const int sub = exact ? 0 : (plan->counts_spmm_sub >= 0 ? plan->counts_spmm_sub : sub_rule);
            plan->last_counts_lanes = (sub == 4 || sub == 8 || sub == 16) ? sub : 1;
            const int64_t* ip = exact ? csr->indptr.p : csr->seg_ptr.p;
            const int32_t* dr = exact ? (const int32_t*)nullptr : csr->seg_dst.p;
            double* o_num = divided ? num_dev : (double*)nullptr; double* o_den = divided ? den_dev : (double*)nullptr; double* o_res = divided ? res_dev : (double*)nullptr;
            if (sub == 4 || sub == 8 || sub == 16) {
                const dim3 gr((unsigned)((nq * sub + WG - 1) / WG)), bl(WG);
                if (sub == 4) hipLaunchKernelGGL((k_csr_spmm_counts_sub<4>), gr, bl, 0, st, ip, dr, csr->cols.p, csr->w.p, (const void*)partial, plan->d_slot_ptr.p, plan->sums, nv, P, (int)K, plan->desc.n_cells, plan->pk, o_num, o_den, o_res);
                else if (sub == 8) hipLaunchKernelGGL((k_csr_spmm_counts_sub<8>), gr, bl, 0, st, ip, dr, csr->cols.p, csr->w.p, (const void*)partial, plan->d_slot_ptr.p, plan->sums, nv, P, (int)K, plan->desc.n_cells, plan->pk, o_num, o_den, o_res);
                else hipLaunchKernelGGL((k_csr_spmm_counts_sub<16>), gr, bl, 0, st, ip, dr, csr->cols.p, csr->w.p, (const void*)partial, plan->d_slot_ptr.p, plan->sums, nv, P, (int)K, plan->desc.n_cells, plan->pk, o_num, o_den, o_res);
            } else
            hipLaunchKernelGGL(k_csr_spmm_counts, dim3((unsigned)((nq + WG - 1) / WG)), dim3(WG), 0, st, ip, dr, csr->cols.p,
                               csr->w.p, (const void*)partial, plan->d_slot_ptr.p, plan->sums, nv, P, (int)K, plan->desc.n_cells, plan->pk,
                               o_num, o_den, o_res);
            HIP_TRY(hipGetLastError());
            if (!exact && csr->n_split) {
                const int64_t n = csr->n_split * Q;
                hipLaunchKernelGGL(k_csr_combine_segments, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, st, plan->sums, csr->split_row.p,
                                   csr->split_ptr.p, csr->R, Q, csr->n_split);
                HIP_TRY(hipGetLastError());
            }
        }
    } else if (!exact && !cells_dev && !plan->packed && K > 0 && !plan->no_slot_spmm) {
        // no per-cell output wanted, no table-order promise: the weighted sums gather the slots directly (no panel)
        if ((rc = launch_spmm_slots(plan, csr, partial, st, num_dev, den_dev, res_dev, &divided))) return rc;
        plan->last_spatial = 1;
    } else {
        plan->last_spatial = 2;
        if ((rc = launch_combine(plan, partial, cells_dev, panel, st))) return rc;
        if ((rc = launch_spmm(csr, panel, plan->sums, Q, st, exact))) return rc;
    }
    const int64_t n = K > 0 ? csr->R * P : 0;                 // one thread per (region, period)
    if (n && !divided) {
        hipLaunchKernelGGL(k_panel_divide, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, st, plan->sums, num_dev,
                           den_dev, res_dev, csr->R, P, (int)K);
        HIP_TRY(hipGetLastError());
    }
    if (kernel_ms) {
        HIP_TRY(hipEventRecord(plan->ev[2], st));
        HIP_TRY(hipEventSynchronize(plan->ev[2]));
        HIP_TRY(hipEventElapsedTime(&kernel_ms[0], plan->ev[0], plan->ev[1]));
        HIP_TRY(hipEventElapsedTime(&kernel_ms[1], plan->ev[0], plan->ev[2]));
    }
    return AFHIP_OK;
}

extern "C" int afhip_plan_profile_begin(afhip_plan* plan, int64_t max_launches) {
    if (!plan || max_launches < 0) return fail(AFHIP_E_INVALID, "plan_profile_begin: bad arguments");
    GUARD_DEVICE(plan->device);
    for (auto& e : plan->prof_ev) if (e) (void)hipEventDestroy(e);
    plan->prof_ev.assign((size_t)(2 * max_launches), nullptr);
    for (auto& e : plan->prof_ev) HIP_TRY(hipEventCreate(&e));
    plan->prof_count = 0;
    return AFHIP_OK;
}

extern "C" int64_t afhip_plan_profile_end(afhip_plan* plan, float* ms_out, int64_t cap) {
    if (!plan) return 0;
    DeviceGuard guard__(plan->device);
    const int64_t n = plan->prof_count;
    for (int64_t i = 0; i < n && i < cap; ++i) {
        if (hipEventSynchronize(plan->prof_ev[(size_t)(2 * i + 1)]) != hipSuccess ||
            hipEventElapsedTime(&ms_out[i], plan->prof_ev[(size_t)(2 * i)], plan->prof_ev[(size_t)(2 * i + 1)]) != hipSuccess) {
            fail(AFHIP_E_HIP, "plan_profile_end: event query failed");
            return -1;
        }
    }
    for (auto& e : plan->prof_ev) if (e) (void)hipEventDestroy(e);
    plan->prof_ev.clear();
    plan->prof_count = 0;
    return n;
}

// ---------------------------------------------------------------------------------------
// standalone grouped reducers (drop-in for the numba kernels)
// ---------------------------------------------------------------------------------------
static int run_group(const void* cube_dev, int dtype, int64_t T, int64_t n_cells, const int64_t* bounds,
                     int64_t G, int code, const double* ddargs, int64_t D, void* out_dev, void* stream) {
    if (!cube_dev || !bounds || !out_dev) return fail(AFHIP_E_INVALID, "group kernel: NULL argument");
    if (G < 0 || D <= 0) return fail(AFHIP_E_INVALID, "group kernel: bad G/D");
    if (dtype != AFHIP_F32 && dtype != AFHIP_F64) return fail(AFHIP_E_INVALID, "group kernel: dtype must be AFHIP_F32 or AFHIP_F64");
    if (G == 0) return AFHIP_OK;
    GUARD_DEVICE(pointer_device(cube_dev));          // the temporary plans are created, run and freed on the cube's device
    hipStream_t st = (hipStream_t)stream;
    std::vector<int64_t> ob((size_t)G + 1);
    for (int64_t g = 0; g <= G; ++g) ob[(size_t)g] = g;
    // D can exceed one pass's slot / column budget (the reference loops over any number of ddargs rows, nb_kernels.py:166,190,215):
    // passes of <= per_pass columns, each writing its own columns [d0, d0 + n) of out[G][cell][D]
    const int64_t per_pass = std::min<int64_t>(MAX_COLS, MAX_THR);
    for (int64_t d0 = 0; d0 < D; d0 += per_pass) {
        const int64_t n = std::min(per_pass, D - d0);
        std::vector<afhip_column> cols((size_t)n);
        for (int64_t d = 0; d < n; ++d) {
            afhip_column c{};
            c.inner = code; c.transform = AFHIP_TF_NONE; c.outer = AFHIP_IDENTITY;
            if (ddargs) { c.inner_args[0] = ddargs[(d0 + d) * 3]; c.inner_args[1] = ddargs[(d0 + d) * 3 + 1]; c.inner_args[2] = ddargs[(d0 + d) * 3 + 2]; }
            cols[(size_t)d] = c;
        }
        afhip_plan_desc desc{};
        desc.T = T; desc.n_cells = n_cells; desc.dtype = dtype; desc.K = (int32_t)n; desc.G1 = G;
        desc.inner_bounds = bounds; desc.P = G; desc.outer_bounds = ob.data(); desc.columns = cols.data();
        afhip_plan* pl = nullptr;
        int rc = afhip_plan_create(&desc, &pl);
        if (rc) return rc;
        char* base;
        if ((rc = ensure_ws(pl, pl->ws_partial, nullptr, 0, "group kernel", &base))) { delete pl; return rc; }
        double* partial = (double*)base;
        if ((rc = launch_temporal(pl, cube_dev, partial, st))) { delete pl; return rc; }
        dim3 grid((unsigned)((n_cells + WG - 1) / WG), (unsigned)std::min<int64_t>(G, 65535));
        if (dtype == AFHIP_F32)
            hipLaunchKernelGGL(k_slots_to_block<float>, grid, dim3(WG), 0, st, partial, pl->d_slot_ptr.p, (float*)out_dev, n_cells, G, (int)n, (int)D, (int)d0, pl->packed ? pl->pk : PackFmt{});
        else
            hipLaunchKernelGGL(k_slots_to_block<double>, grid, dim3(WG), 0, st, partial, pl->d_slot_ptr.p, (double*)out_dev, n_cells, G, (int)n, (int)D, (int)d0, pl->packed ? pl->pk : PackFmt{});
        hipError_t e = hipGetLastError();
        // the plan owns the scratch the kernels are still reading: drain before freeing it
        hipError_t e2 = hipStreamSynchronize(st);
        delete pl;
        if (e != hipSuccess) return fail(AFHIP_E_HIP, "k_slots_to_block launch failed: %s", hipGetErrorString(e));
        if (e2 != hipSuccess) return fail(AFHIP_E_HIP, "stream synchronize failed: %s", hipGetErrorString(e2));
    }
    return AFHIP_OK;
}

extern "C" int afhip_group_stat(const void* cube_dev, int dtype, int64_t T, int64_t n_cells,
                                const int64_t* bounds, int64_t G, int code, void* out_dev, void* stream) {
    if (code < AFHIP_MEAN || code > AFHIP_NANMEAN) return fail(AFHIP_E_INVALID, "group_stat: code %d is not a stat reducer", code);
    return run_group(cube_dev, dtype, T, n_cells, bounds, G, code, nullptr, 1, out_dev, stream);
}
extern "C" int afhip_group_dd(const void* cube_dev, int dtype, int64_t T, int64_t n_cells, const int64_t* bounds,
                              int64_t G, const double* ddargs, int64_t D, void* out_dev, void* stream) {
    if (!ddargs) return fail(AFHIP_E_INVALID, "group_dd: ddargs is NULL");
    return run_group(cube_dev, dtype, T, n_cells, bounds, G, AFHIP_DD, ddargs, D, out_dev, stream);
}
extern "C" int afhip_group_bins(const void* cube_dev, int dtype, int64_t T, int64_t n_cells, const int64_t* bounds,
                                int64_t G, const double* ddargs, int64_t D, void* out_dev, void* stream) {
    if (!ddargs) return fail(AFHIP_E_INVALID, "group_bins: ddargs is NULL");
    return run_group(cube_dev, dtype, T, n_cells, bounds, G, AFHIP_BINS, ddargs, D, out_dev, stream);
}
extern "C" int afhip_group_sine_dd(const void* cube_dev, int dtype, int64_t T, int64_t n_cells, const int64_t* bounds,
                                   int64_t G, const double* ddargs, int64_t D, void* out_dev, void* stream) {
    if (!ddargs) return fail(AFHIP_E_INVALID, "group_sine_dd: ddargs is NULL");
    return run_group(cube_dev, dtype, T, n_cells, bounds, G, AFHIP_SINE_DD, ddargs, D, out_dev, stream);
}
