// afhip_cell_map.h — the cell map of the LDS-histogram forms for bins of UNEQUAL interior widths (FEAT_CELL_MAP).
//
// Plain C++: no HIP, no variant table — the planner (afhip_planner.cpp: find_partition) and a stand-alone checker
// (tests/cell_map_check.cpp) include it.
//
// A partition has interior edges E[0] < ... < E[n] (n interior bins) between two end bins, which sit on the guard bins 0 and
// n + 1 of the guarded partition (FEAT_END_BINS).  The equal-width forms guess a value's bin with one fma; here the same fma guesses
// a CELL of a lattice of width w laid over [E[0], E[n]) — w is half of the smallest interior width, so a cell holds one edge at most
// — and a byte map sends the cell to a bin:
//     g = clamp(floor(v * c1 + c0), 0, M + 1)      c1 = 1 / w,  c0 = 1 - E[0] / w   (cell 0 and cell M + 1 are the guard cells)
//     b = map[g]                                    the guarded bin that holds the cell's lower end
// The kernel then repairs b by +-1 against the exact edges (hb_count), so the guess may be one bin off and no more.  cell_map_check
// establishes that with the kernel's own fma and floor in the input precision T: both neighbours of every edge E[k] in T (they are
// the edge itself where it is representable) must guess bin k or k + 1, and a point beyond either end must reach its guard bin.  The
// fma, the floor and the map are monotone in v, so every value between two edges then guesses its own bin or a neighbour.
#pragma once
#include <stdint.h>

#include <cmath>

namespace afhip {

constexpr int CELL_MAP_MAX_CELLS = 254;      // M: with the two guard cells a byte-indexed map of 256 entries
constexpr int CELL_MAP_BYTES = 256;          // the map as the kernel copies it into LDS (entries past M + 1 are zero)
constexpr int CELL_MAP_MAX_BINS = 14;        // interior bins: sixteen slots less the two end bins

struct CellMap {
    int cells = 0;                 // M; 0: no map
    int n = 0;                     // interior bins
    double w = 0, c1 = 0, c0 = 0;  // cell width and the guess constants
    uint8_t map[CELL_MAP_BYTES] = {0};
};

// float / double unit roundoff as find_partition's precision bound takes it
template <typename T> constexpr double cell_map_eps() { return sizeof(T) == 4 ? 1.2e-7 : 2.3e-16; }

// Lays the cells over the interior edges E[0..n].  False: the edges are not finite and strictly increasing, the lattice needs more
// than CELL_MAP_MAX_CELLS cells, or the cells are too narrow for a guess in T (the bound find_partition applies to its bins:
// 16 ulps of the larger end of the range must stay below a cell).
template <typename T>
inline bool cell_map_build(const double* E, int n, CellMap* cm) {
    *cm = CellMap{};
    if (n < 1 || n > CELL_MAP_MAX_BINS) return false;
    double wmin = INFINITY;
    for (int k = 0; k <= n; ++k)
        if (!std::isfinite(E[k])) return false;
    for (int k = 0; k < n; ++k) {
        const double d = E[k + 1] - E[k];
        if (!(d > 0)) return false;
        wmin = d < wmin ? d : wmin;
    }
    const double w = 0.5 * wmin;
    if (!(w > 0) || !std::isfinite(w)) return false;
    const double span = (E[n] - E[0]) / w;
    if (!(span <= (double)CELL_MAP_MAX_CELLS + 1e-9)) return false;
    const int M = (int)std::ceil(span - 1e-9);
    if (M < 1 || M > CELL_MAP_MAX_CELLS) return false;
    const double emax = std::fmax(std::fabs(E[0]), std::fabs(E[n]));
    if (!(emax * cell_map_eps<T>() * 16.0 < w)) return false;
    cm->cells = M; cm->n = n; cm->w = w; cm->c1 = 1.0 / w; cm->c0 = 1.0 - E[0] / w;      // + 1: cell 0 is the lower guard cell
    cm->map[0] = 0;
    for (int g = 1; g <= M; ++g) {
        // the bin of the cell's lower end; a lower end ON an edge E[k] (within the lattice's tolerance) belongs to the bin above it
        const double x = E[0] + (g - 1) * w;
        int b = 0;
        for (int k = 0; k < n; ++k) b += (E[k] <= x + 1e-9 * w) ? 1 : 0;
        cm->map[g] = (uint8_t)b;
    }
    cm->map[M + 1] = (uint8_t)(n + 1);
    return true;
}

// The kernel's guess for one value: the guarded bin of the cell that fma and floor in T send v to (NaN: the lower guard bin).
template <typename T>
inline int cell_map_guess(const CellMap& cm, T v) {
    const T c1 = (T)cm.c1, c0 = (T)cm.c0, top = (T)(cm.cells + 1);
    T t = std::fma(v, c1, c0);
    t = t > (T)0 ? t : (T)0;          // (NaN fails the compare: cell 0, as the kernel's fmax / med3 sends it)
    t = t < top ? t : top;
    return cm.map[(int)t];            // t >= 0: the truncation is the floor
}

// the largest value of T that is <= x / the smallest that is >= x
template <typename T> inline T cell_map_dn(double x) { const T f = (T)x; return (double)f > x ? std::nextafter(f, (T)-INFINITY) : f; }
template <typename T> inline T cell_map_up(double x) { const T f = (T)x; return (double)f < x ? std::nextafter(f, (T)INFINITY) : f; }

// The acceptance check (see the head of the file).
template <typename T>
inline bool cell_map_check(const CellMap& cm, const double* E) {
    if (cm.cells < 1) return false;
    const int n = cm.n;
    for (int k = 0; k <= n; ++k) {
        // below the edge lies guarded bin k, above it bin k + 1
        const int lo = cell_map_guess<T>(cm, cell_map_dn<T>(E[k])), hi = cell_map_guess<T>(cm, cell_map_up<T>(E[k]));
        if (lo != k && lo != k + 1) return false;
        if (hi != k && hi != k + 1) return false;
    }
    // a point inside each end bin's guard cell
    if (cell_map_guess<T>(cm, (T)(E[0] - 1.5 * cm.w)) != 0) return false;
    if (cell_map_guess<T>(cm, (T)(E[n] + 1.5 * cm.w)) != n + 1) return false;
    return true;
}

// build + check: the map of the interior edges E[0..n] for input precision T, or false (the partition is not found)
template <typename T>
inline bool cell_map_find(const double* E, int n, CellMap* cm) {
    if (!cell_map_build<T>(E, n, cm) || !cell_map_check<T>(*cm, E)) { *cm = CellMap{}; return false; }
    return true;
}

}  // namespace afhip
