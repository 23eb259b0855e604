// cell_map_check.cpp — stand-alone checker of the cell map (aggfly_amd/csrc/afhip_cell_map.h), host code only.
//
//     g++ -std=c++17 -O1 -I aggfly_amd/csrc tests/cell_map_check.cpp -o cell_map_check && ./cell_map_check
//
// For a few hundred partitions from a fixed seed and a list of hand-picked ones, in float and in double: whenever cell_map_find accepts
// a partition, the emulated guess (the kernel's fma, clamp, truncation and map read) must be within ONE bin of the true bin — which is
// all the kernel's repair step needs — and a value ON an edge must guess one of the edge's two bins; this at every edge, every cell
// boundary, eight ulps to either side of each, and 10^5 random values.  The partitions that must be refused (range over smallest width
// beyond 127, widths of a few ulps) are refused.  Exit status 0 and a summary line, or the failures and status 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "afhip_cell_map.h"

using namespace afhip;

namespace {

struct Rng {      // splitmix64: the same partitions everywhere
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

int g_fail = 0;
long g_points = 0;

// guarded bin of v among the edges E[0..n]: 0 below E[0] (and for NaN, which the kernel sends there), n + 1 from E[n] up; a value ON
// an edge belongs to no bin: it may be taken for either neighbour
template <typename T>
void true_bins(const std::vector<double>& E, T v, int* lo, int* hi) {
    const int n = (int)E.size() - 1;
    if (v != v) { *lo = *hi = 0; return; }
    int below = 0;       // edges strictly below v
    int upto = 0;        // edges <= v
    for (int k = 0; k <= n; ++k) { below += E[k] < (double)v; upto += E[k] <= (double)v; }
    *lo = below; *hi = upto;
}

template <typename T>
bool point_ok(const CellMap& cm, const std::vector<double>& E, T v, const char* what, const char* name) {
    int lo, hi;
    true_bins<T>(E, v, &lo, &hi);
    const int g = cell_map_guess<T>(cm, v);
    ++g_points;
    // (a value on an edge must guess one of the two bins the edge parts: from a bin further off the repair would count it)
    if (lo != hi ? (g >= lo && g <= hi) : (g >= lo - 1 && g <= hi + 1)) return true;
    fprintf(stderr, "FAIL %s (%s, %s): value %.17g guesses bin %d, true bin %d..%d (cells %d, w %.17g)\n", name, sizeof(T) == 4 ? "float" : "double", what,
            (double)v, g, lo, hi, cm.cells, cm.w);
    ++g_fail;
    return false;
}

template <typename T>
bool around_ok(const CellMap& cm, const std::vector<double>& E, double x, const char* what, const char* name) {
    T up = cell_map_up<T>(x), dn = cell_map_dn<T>(x);
    bool ok = point_ok<T>(cm, E, up, what, name) && point_ok<T>(cm, E, dn, what, name);
    for (int s = 0; ok && s < 8; ++s) {
        up = std::nextafter(up, (T)INFINITY); dn = std::nextafter(dn, (T)-INFINITY);
        ok = point_ok<T>(cm, E, up, what, name) && point_ok<T>(cm, E, dn, what, name);
    }
    return ok;
}

// 1: accepted and every point holds, 0: refused, -1: accepted and a point fails
template <typename T>
int run_one(const std::vector<double>& E, const char* name, Rng* rng) {
    const int n = (int)E.size() - 1;
    CellMap cm;
    if (!cell_map_find<T>(E.data(), n, &cm)) return 0;
    bool ok = cm.cells >= 1 && cm.cells <= CELL_MAP_MAX_CELLS && cm.map[0] == 0 && cm.map[cm.cells + 1] == n + 1;
    for (int g = 1; ok && g <= cm.cells + 1; ++g) ok = cm.map[g] >= cm.map[g - 1] && cm.map[g] <= n + 1;      // monotone
    if (!ok) { fprintf(stderr, "FAIL %s: malformed map\n", name); ++g_fail; return -1; }
    for (int k = 0; ok && k <= n; ++k) ok = around_ok<T>(cm, E, E[k], "edge", name);
    for (int g = 0; ok && g <= cm.cells; ++g) ok = around_ok<T>(cm, E, E[0] + g * cm.w, "cell boundary", name);
    const double span = E[n] - E[0];
    for (int i = 0; ok && i < 100000; ++i) ok = point_ok<T>(cm, E, (T)(E[0] - 0.1 * span + 1.2 * span * rng->uni()), "random", name);
    const T special[] = {(T)0, (T)-0.0, (T)INFINITY, (T)-INFINITY, (T)NAN, (T)1e30, (T)-1e30, std::nextafter((T)E[0], (T)-INFINITY)};
    for (T v : special) ok = ok && point_ok<T>(cm, E, v, "special", name);
    return ok ? 1 : -1;
}

std::vector<double> from_widths(double e0, const std::vector<double>& w) {
    std::vector<double> E{e0};
    for (double x : w) E.push_back(E.back() + x);
    return E;
}

void expect(const char* name, int got, int want, const char* type) {
    if (got == want) return;
    fprintf(stderr, "FAIL %s (%s): %s, expected %s\n", name, type, got == 0 ? "refused" : (got == 1 ? "accepted" : "accepted with a wrong guess"),
            want == 0 ? "refused" : "accepted");
    ++g_fail;
}

}  // namespace

int main() {
    Rng rng{20240611};
    int accepted[2] = {0, 0}, refused[2] = {0, 0};
    // random partitions: 4 - 14 interior bins, widths 0.5 ... 20 in steps of 0.5 (ratio of range to smallest width as it comes)
    const double firsts[] = {0.0, -7.3, 250.15, 273.15};
    for (int trial = 0; trial < 300; ++trial) {
        const int n = 4 + rng.below(11);
        std::vector<double> w;
        for (int b = 0; b < n; ++b) w.push_back(trial % 3 == 0 ? 0.5 + 19.5 * rng.uni() : 0.5 * (1 + rng.below(40)));
        const std::vector<double> E = from_widths(firsts[trial % 4], w);
        char name[48];
        snprintf(name, sizeof name, "random %d", trial);
        const int rf = run_one<float>(E, name, &rng), rd = run_one<double>(E, name, &rng);
        (rf == 0 ? refused : accepted)[0] += 1;
        (rd == 0 ? refused : accepted)[1] += 1;
        // a refusal of a random partition must have a reason: too many cells
        double wmin = 1e300;
        for (double x : w) wmin = x < wmin ? x : wmin;
        const bool fits = 2.0 * (E[n] - E[0]) / wmin <= 254.0;
        if (fits) { expect(name, rf, 1, "float"); expect(name, rd, 1, "double"); }
        else { expect(name, rf, 0, "float"); expect(name, rd, 0, "double"); }
    }
    // hand-picked
    {   // Fahrenheit edges 0, 10, 20, 32, 40, 50, 60, 70, 75, 80, 85, 90, 95, 100 F in Celsius
        std::vector<double> E;
        for (double f : {0.0, 10.0, 20.0, 32.0, 40.0, 50.0, 60.0, 70.0, 75.0, 80.0, 85.0, 90.0, 95.0, 100.0}) E.push_back((f - 32.0) * 5.0 / 9.0);
        expect("fahrenheit", run_one<float>(E, "fahrenheit", &rng), 1, "float");
        expect("fahrenheit", run_one<double>(E, "fahrenheit", &rng), 1, "double");
    }
    {   // kelvin edges 250.15 + k with widths 1, 2, 5, 10
        const std::vector<double> E = from_widths(250.15, {10, 5, 5, 2, 2, 1, 1, 2, 5, 10});
        expect("kelvin", run_one<float>(E, "kelvin", &rng), 1, "float");
        expect("kelvin", run_one<double>(E, "kelvin", &rng), 1, "double");
    }
    {   // the issue's eight-bin spec: interior edges -10, 0, 10, 20, 25, 30, 35
        const std::vector<double> E = {-10, 0, 10, 20, 25, 30, 35};
        expect("eight bins", run_one<float>(E, "eight bins", &rng), 1, "float");
        expect("eight bins", run_one<double>(E, "eight bins", &rng), 1, "double");
    }
    {   // smallest width against range 1 : 126 (252 cells) and 1 : 127 (254): accepted; 1 : 127.5 and 1 : 128: refused
        struct { const char* name; double ratio; int want; } cases[] = {{"ratio 126", 126.0, 1}, {"ratio 127", 127.0, 1}, {"ratio 127.5", 127.5, 0}, {"ratio 128", 128.0, 0}};
        for (auto& c : cases) {
            const double rest = 0.5 * c.ratio - 0.5;      // the other four bins beside the one of width 0.5
            const std::vector<double> E = from_widths(-30.0, {rest * 0.25, 0.5, rest * 0.25, rest * 0.125, rest * 0.375});
            expect(c.name, run_one<float>(E, c.name, &rng), c.want, "float");
            expect(c.name, run_one<double>(E, c.name, &rng), c.want, "double");
        }
    }
    {   // widths of a few ulps of the edges: refused in that precision (the double case is wide enough in double: accepted there)
        const double u32 = std::ldexp(1.0, -15), u64 = std::ldexp(1.0, -44);      // 300 has float ulp 2^-15, double ulp 2^-44
        const std::vector<double> Ef = from_widths(300.0, {2 * u32, 4 * u32, 2 * u32, 6 * u32, 2 * u32});
        const std::vector<double> Ed = from_widths(300.0, {2 * u64, 4 * u64, 2 * u64, 6 * u64, 2 * u64});
        expect("few float ulps", run_one<float>(Ef, "few float ulps", &rng), 0, "float");
        expect("few float ulps", run_one<double>(Ef, "few float ulps", &rng), 1, "double");
        expect("few double ulps", run_one<float>(Ed, "few double ulps", &rng), 0, "float");
        expect("few double ulps", run_one<double>(Ed, "few double ulps", &rng), 0, "double");
    }
    {   // not a partition: a width of zero, edges out of order, an infinite edge
        expect("zero width", run_one<double>({0, 1, 1, 3, 6}, "zero width", &rng), 0, "double");
        expect("out of order", run_one<double>({0, 2, 1, 3, 6}, "out of order", &rng), 0, "double");
        expect("infinite edge", run_one<double>({0, 1, 3, 6, INFINITY}, "infinite edge", &rng), 0, "double");
    }
    printf("cell_map_check: %d failures; random partitions accepted float %d double %d, refused float %d double %d; %ld points\n", g_fail, accepted[0],
           accepted[1], refused[0], refused[1], g_points);
    return g_fail ? 1 : 0;
}
