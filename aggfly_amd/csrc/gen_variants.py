#!/usr/bin/env python3
"""Writes the translation units that instantiate k_fused_temporal (afhip_kernels.h).

Usage: gen_variants.py OUTDIR [--menu full|arms|dev] [--per-file N]      (full: the production menu; arms: + the tuning arms)

Each generated unit holds a handful of explicit instantiations so that ``make -j`` compiles them in parallel.  `MENUS` lists the
kernel menus and the stems of their units: the float kernels (`menu`) go to ``variants_NN.hip``, the kernels of int16-packed cubes
(`packed_menu`) to ``packed_NN.hip``, their LDS-histogram forms (`packed_hist_menu`) to ``packed_hist_NN.hip``, and the histogram forms
for partitions with a wide end bin (`end_bins_menu`: Feat.END_BINS, float32, float64 and packed storage together) to ``end_bins_NN.hip``
(float32 / float64) and ``end_bins_packed_NN.hip``, and their twins for interior bins of unequal widths (`cell_map_menu`: Feat.CELL_MAP) to
``cell_map_NN.hip`` and ``cell_map_packed_NN.hip``.  ``variants_table.hip`` collects ONE table, a slice per menu in `MENUS` order, behind
``menu_table`` (afhip_variants.h), which ``find_variant`` and ``find_exact_form`` search; every menu keeps its own count and contents.
`MORE_MENUS` continues the list — the lean short-group kernels of packed cubes (`packed_short_menu`) in ``packed_short_NN.hip`` — and
`ALL_MENUS` is the two together; `LATER_MENUS` goes on behind them — the region-fused twins of packed cubes' general and short-group kernels
(`packed_rf_menu`) in ``packed_rf_NN.hip`` — and `TABLE_MENUS` is all of them, which the table follows.

Adding a menu: a menu function and an entry of `LATER_MENUS` here, the enumerator of the same name in afhip_variants.h's `Menu` (the table asserts
that the two agree), and a recipe module under tests/ beside `variant_recipes` ("Adding a kernel menu").
"""
import os
import sys

CT = {0: "float", 1: "double", 2: "PackedI16"}
I16 = 2        # AFHIP_I16: int16 storage, float32 values
# packed_menu: the (cells per lane, stat, slots, columns) it leaves out, because their kernels hold scratch memory
# (-Rpass-analysis=kernel-resource-usage): the all-purpose (stat 3) sixteen-column forms at two cells per lane (272 bytes per lane, like
# their float32 twins) and one four-cell form (36).  A plan of such a shape takes the next narrower kernel, which has none.
PACKED_DROPPED = {(2, 3, nthr, 16) for nthr in (0, 1, 4, 16)} | {(4, 3, 1, 6)}
PACKED_SHALLOW = {(1, 3, 16, 16)}      # ... and the one that keeps eight rows in flight where its width takes sixteen: 36 bytes of scratch at sixteen (and at twelve)
PACKED_SHORT_DROPPED = {(4, 2, 6)}      # packed_short_menu: the (cells per lane, stat, columns) it leaves out, whatever the group length (scratch memory: see there)
PACKED_HIST_VECS = (2, 1)              # packed_hist_menu: cells per lane (four: every two-level form holds 528 bytes of scratch, the single-level ones one ... two waves per SIMD)


class Feat:
    """The bits of k_fused_temporal's FEAT; afhip_plan_types.h says what each compiles in (FEAT_<name> there: the generated
    variants_table.hip asserts that the two agree)."""
    SINE = 1
    GENERAL_TF = 2
    NT = 4
    INT_BINS = 8
    SINGLE_LEVEL = 16
    HIST = 32
    ARITH_EDGES = 64
    SHORT_GROUP = 128
    LEAN = 256
    LEAN_SINE = 512
    FOUR_ROW = 1024
    REGION_FUSED = 2048
    THREE_ROW = 4096
    MIXED = 8192
    END_BINS = 16384
    CELL_MAP = 32768


FEAT_NAMES = [n for n in vars(Feat) if n.isupper()]
GROUP_LENGTH = Feat.FOUR_ROW | Feat.THREE_ROW | Feat.MIXED      # the short-group forms of other than two rows
# name suffixes, in name order (`_ss` instead of `_lean` for the sine-only lean form)
SUFFIXES = ((Feat.NT, "_nt"), (Feat.INT_BINS, "_ibins"), (Feat.SINGLE_LEVEL, "_sl"), (Feat.HIST, "_hist"), (Feat.ARITH_EDGES, "_arith"), (Feat.END_BINS, "_ends"), (Feat.CELL_MAP, "_cmap"),
            (Feat.SHORT_GROUP, "_pair"), (Feat.LEAN, "_lean"), (Feat.FOUR_ROW, "_quad"), (Feat.THREE_ROW, "_tri"), (Feat.MIXED, "_rag"),
            (Feat.REGION_FUSED, "_rf"))

# packed_rf_menu: the twins that hold scratch memory at their plain kernel's rows in flight — keys (cells per lane, stat, slots, columns,
# short-group feature bits or 0).  PACKED_RF_SHALLOW: those that hold none at HALF the depth, and that depth (sixteen -> eight, the
# stat-2 six-column pair form eight -> four: the depths the packed menus use).  PACKED_RF_DROPPED: those that hold the same 36 bytes per
# lane at every depth probed (1, 2, 4, 6 ... 16; some of them at 52 VGPRs: not a register spill) — no twin, such a plan keeps the per-cell route.
PACKED_RF_SHALLOW = {**{(1, stat, nthr, kmax, 0): 8 for stat, nthr, kmax in ((0, 4, 2), (1, 1, 6))},
                     **{(2, stat, 0, kmax, 0): 8 for stat in (1, 2) for kmax in (2, 6)},
                     **{(vec, 2, 0, 6, Feat.SHORT_GROUP | Feat.LEAN): 4 for vec in (2, 1)}}
PACKED_RF_DROPPED = {(1, 0, 4, 6, 0), (1, 1, 4, 6, 0), (1, 3, 1, 6, 0), (1, 3, 4, 2, 0), (1, 3, 4, 6, 0), (2, 3, 0, 2, 0), (2, 3, 0, 6, 0)}

def menu(kind):
    """(dtype, pipe, vec, stat, nthr, kmax, depth, feat, production)"""
    out = []
    vec16 = {0: 4, 1: 2}

    def add(dtype, pipe, vec, stat, nthr, kmax, depth, nt=1, prod=1, tki=0, sl=0, hb=0, ha=0, pair=0, ss=0, quad=0, rf=0, tri=0, rag=0):
        # sine degree days ride on the min/max accumulators; generic pow() only in the all-purpose (STAT 3) variants
        feat = {0: 0, 1: 0, 2: Feat.SINE, 3: Feat.SINE | Feat.GENERAL_TF}[stat]
        for on, bit in ((nt, Feat.NT), (tki, Feat.INT_BINS), (sl, Feat.SINGLE_LEVEL), (hb, Feat.HIST), (ha, Feat.ARITH_EDGES), (pair, Feat.SHORT_GROUP),
                        (ss, Feat.LEAN), (ss == 2, Feat.LEAN_SINE), (quad, Feat.FOUR_ROW), (rf, Feat.REGION_FUSED), (tri, Feat.THREE_ROW), (rag, Feat.MIXED)):
            if on:
                feat |= bit
        key = (dtype, pipe, vec, stat, nthr, kmax, depth, feat)
        for i, v in enumerate(out):
            if v[:8] == key:
                out[i] = key + (max(v[8], prod),)
                return
        out.append(key + (prod,))

    shapes_all = [(stat, nthr, kmax) for stat in (0, 1, 3) for nthr in (0, 1, 4, 16) for kmax in (2, 6, 16)
                  if not (stat == 0 and nthr == 0)] + [(2, 0, 2), (2, 0, 6)]
    headline = ((1, 1, 6), (1, 0, 2), (2, 0, 2), (0, 16, 16))
    for dtype in (0, 1):
        if kind == "dev":
            add(dtype, 0, 1, 3, 16, 16, 4)
            add(dtype, 0, 1, 1, 1, 6, 4)
            add(dtype, 1, vec16[dtype], 1, 1, 6, 4)
            add(dtype, 1, vec16[dtype], 3, 16, 16, 4)
            continue
        for (stat, nthr, kmax) in shapes_all:
            # production menu, chosen by measurement on MI355X (profiles/r01_sweep_load_arms.txt):
            #   f64: direct 8-byte nt loads, one cell per lane, 4 rows in flight (6.5 TB/s on
            #        configs[1]); the LDS-DMA ring with 2 cells per lane is kept for short inner groups (and as an arm)
            #   f32: direct 8-byte nt loads, two cells per lane, 8 rows in flight; odd row
            #        lengths fall back to one cell per lane
            if dtype == 1:
                add(dtype, 0, 1, stat, nthr, kmax, 4)
                add(dtype, 1, 2, stat, nthr, kmax, 4)
            else:
                add(dtype, 0, 2, stat, nthr, kmax, 8)
                add(dtype, 0, 1, stat, nthr, kmax, 8)
                # short inner groups (2-4 steps: tmin/tmax pairs, 6-hourly data): the LDS-DMA ring prefetches
                # across group ends, the direct path cannot (3.5 vs 4.3 TB/s at 2 steps, 4.4 vs 5.6 at 4)
                add(dtype, 1, 4, stat, nthr, kmax, 4)
        # bins-heavy and multi-threshold single-level plans (CMIP6 temperature bins, configs[3])
        for nthr in (4, 16):
            for kmax in (6, 16):
                if kmax < nthr and nthr == 16:
                    continue
                for (pipe, vec, depth) in (((0, 1, 4), (1, 2, 4)) if dtype == 1 else ((0, 2, 8), (0, 1, 8))):
                    add(dtype, pipe, vec, 0, nthr, kmax, depth, tki=1, sl=1)
                    add(dtype, pipe, vec, 0, nthr, kmax, depth, tki=0, sl=1)
                    add(dtype, pipe, vec, 1, nthr, kmax, depth, tki=1, sl=0)
        # (tmin, tmax) pairs per day (configs[4]): every inner group is two rows
        for kmax in (2, 6):
            for (vec, depth) in (((1, 4), (1, 8)) if dtype == 1 else ((2, 8), (1, 8))):
                add(dtype, 0, vec, 2, 0, kmax, depth, pair=1, prod=1 if depth == (4 if dtype == 1 else 8) else 0)
        # contiguous equal-width bins: per-lane LDS histogram (direct-load path only)
        for (vec, depth) in (((1, 4),) if dtype == 1 else ((1, 8), (2, 8))):
            for stat in (0, 1):
                for sl in (0, 1):
                    add(dtype, 0, vec, stat, 16, 16, depth, tki=1, sl=sl, hb=1)
                    if vec == 1:    # exactly representable edges: computed instead of read from the LDS table
                        add(dtype, 0, vec, stat, 16, 16, depth, tki=1, sl=sl, hb=1, ha=1)
        # tuning arms for the headline shapes (scripts/kbench.py)
        for (stat, nthr, kmax) in headline:
            for depth in (4, 8, 16):
                add(dtype, 1, vec16[dtype], stat, nthr, kmax, depth, prod=0)
            add(dtype, 1, vec16[dtype], stat, nthr, kmax, 4, nt=0, prod=0)
            for depth in (4, 8):
                add(dtype, 0, 1, stat, nthr, kmax, depth, prod=0)
                add(dtype, 0, 2, stat, nthr, kmax, depth, prod=0)
                if dtype == 0:
                    add(dtype, 0, 4, stat, nthr, kmax, depth, prod=0)
    # round 3 arms (appended, so that the translation units above keep their contents): the arithmetic-edge histogram with
    # deeper bursts and with two cells per lane — the C4 kernel is short of bytes in flight (profiles/r03_c4_bound_pmc.txt)
    for dtype in (() if kind == "dev" else (0, 1)):
        for (vec, depth) in (((1, 8), (1, 16), (2, 4), (2, 8)) if dtype == 1 else ((1, 12), (1, 16), (1, 24), (2, 8), (2, 16))):
            add(dtype, 0, vec, 0, 16, 16, depth, tki=1, sl=1, hb=1, ha=1, prod=0)
        # f32, two cells per lane, FOUR rows in flight: +2.6 % over eight on multi-column plans on large grids (configs[1] on float32
        # storage: 6.31 vs 6.15 TB/s, profiles/r03_sweep_chunks_depth.txt); small grids keep eight (5.73 vs 5.41)
        if dtype == 0:
            for (stat, nthr, kmax) in [(st, nt_, km) for st in (0, 1, 3) for nt_ in (0, 1) for km in (2, 6) if not (st == 0 and nt_ == 0)] + [(2, 0, 2), (2, 0, 6)]:
                add(dtype, 0, 2, stat, nthr, kmax, 4)
        # (tmin, tmax) pairs with the lean group end (Feat.LEAN): sine_dd / min / max sources (stat 2) and mean / sum alone (stat 1)
        for (vec, depth) in (((1, 4), (1, 8)) if dtype == 1 else ((2, 8), (1, 8), (2, 4))):
            prod = 1 if (vec, depth) in ((1, 4), (2, 8), (1, 8)) and not (dtype == 1 and depth == 8) else 0
            add(dtype, 0, vec, 2, 0, 2, depth, pair=1, ss=2, prod=prod)      # every column a plain sine_dd (configs[4])
            add(dtype, 0, vec, 2, 0, 2, depth, pair=1, ss=1, prod=prod)
            add(dtype, 0, vec, 2, 0, 6, depth, pair=1, ss=1, prod=prod)
            add(dtype, 0, vec, 1, 0, 2, depth, pair=1, ss=1, prod=prod)
            add(dtype, 0, vec, 1, 0, 6, depth, pair=1, ss=1, prod=prod)
        # (four cells per lane — half the per-wave scalar work per cell — measured level with two: 4.28 vs 4.25 ms on C5; not kept)
        # inner groups of exactly four rows (6-hourly data): the lean short-group form (Feat.FOUR_ROW)
        for (vec, depth) in (((1, 8), (1, 4)) if dtype == 1 else ((2, 8), (1, 8))):
            prod = 0 if (dtype == 1 and depth == 4) else 1
            for stat in (1, 2):
                for kmax in (2, 6):
                    add(dtype, 0, vec, stat, 0, kmax, depth, pair=1, ss=1, quad=1, prod=prod)
        # inner groups of exactly three rows (8-hourly data): the same lean form (Feat.THREE_ROW), two groups per block of six rows
        for vec in ((1,) if dtype == 1 else (2, 1)):
            for stat in (1, 2):
                for kmax in (2, 6):
                    add(dtype, 0, vec, stat, 0, kmax, 6, pair=1, ss=1, tri=1)
    # region-fused period ends (Feat.REGION_FUSED): twins of the production two-level variants on the direct-load path.  Round 3 built the
    # twins that gain from two periods on (up to six columns and four threshold slots, with a statistic; of the short-group forms
    # every lean four-row form and the six-column lean pair form); round 4 adds threshold-only plans (a daily panel of degree days) and
    # every short-group form incl. the sine-only pair form (afhip_planner.cpp: rf_plan_ok says when the planner takes them).  Plans of
    # more than six columns or four threshold slots are bound by their arithmetic and measured level with or behind the per-cell route
    # (13 degree-day columns, daily panel: 20.7 against 21.1 ms; monthly: 15.5 against 14.5): no twins.  Single-level (`sl`),
    # integer-bin and histogram variants have none either.
    # — appended, so that the translation units above keep their contents
    for v in list(out):
        dtype, pipe, vec, stat, nthr, kmax, depth, feat, prod = v
        if prod and pipe == 0 and kmax <= 6 and nthr <= 4 and not (feat & (Feat.INT_BINS | Feat.SINGLE_LEVEL | Feat.HIST)):
            out.append((dtype, pipe, vec, stat, nthr, kmax, depth, feat | Feat.REGION_FUSED, prod))
    # inner groups of MIXED lengths one to four rows (Feat.MIXED; a sub-daily series with missing steps): the four-row form with a
    # scalar trip count per group, and its region-fused twins — appended likewise
    if kind != "dev":
        for dtype in (0, 1):
            for vec in ((1,) if dtype == 1 else (2, 1)):
                for stat in (1, 2):
                    for kmax in (2, 6):
                        add(dtype, 0, vec, stat, 0, kmax, 8, pair=1, ss=1, rag=1)
                        add(dtype, 0, vec, stat, 0, kmax, 8, pair=1, ss=1, rag=1, rf=1)
    # kernels the planner can never pick at tuning 0 are tuning arms, not production (twins go with their plain variants)
    out = [v[:8] + (0,) if v[8] and not pickable(v) else v for v in out]
    # `full` = what the planner can pick; the tuning arms of the headline shapes (kbench.py / r03_arms.py `tuning=`; not production)
    # and the unpickable kernels above are compiled by `make MENU=arms` only
    if kind != "arms":
        out = [v for v in out if v[8]]
    return out


def packed_menu(kind):
    """The kernels of int16-packed cubes (storage tag PackedI16), same tuples as `menu`: the general two-level forms on the direct-load
    path with nt loads — no short-group, lean, single-level, integer-bin or histogram form (the short-group forms and the region-fused twins
    have menus of their own: `packed_short_menu`, `packed_rf_menu`).  Every shape at two cells and
    at one cell per lane (4 / 2 bytes per lane and row); the light shapes also at four (8 bytes, what a float32 lane reads at two cells).
    Rows in flight: eight at four cells per lane — 64 bytes per lane, the float32 production forms' — and sixteen at two and one,
    whose rows are half and a quarter of that (PACKED_SHALLOW: one exception).  Chosen from -Rpass-analysis=kernel-resource-usage, not from a measurement: no kernel of the menu has scratch memory
    (PACKED_DROPPED; profiles/packed_cube.txt has the register table)."""
    def one(vec, stat, nthr, kmax):
        feat = {0: 0, 1: 0, 2: Feat.SINE, 3: Feat.SINE | Feat.GENERAL_TF}[stat] | Feat.NT
        return (I16, 0, vec, stat, nthr, kmax, 8 if (vec == 4 or (vec, stat, nthr, kmax) in PACKED_SHALLOW) else 16, feat, 1)

    if kind == "dev":
        return [one(1, 3, 16, 16), one(4, 1, 1, 6)]
    shapes_all = [(stat, nthr, kmax) for stat in (0, 1, 3) for nthr in (0, 1, 4, 16) for kmax in (2, 6, 16)
                  if not (stat == 0 and nthr == 0)] + [(2, 0, 2), (2, 0, 6)]
    light = [(stat, nthr, kmax) for stat in (0, 1, 3) for nthr in (0, 1) for kmax in (2, 6) if not (stat == 0 and nthr == 0)] + [(2, 0, 2), (2, 0, 6)]
    out = [one(vec, *sh) for vec in (2, 1) for sh in shapes_all] + [one(4, *sh) for sh in light]
    # ... and no kernel that no plan can select (`pickable`: two-column shapes with more threshold slots than two columns lower to)
    return [v for v in out if v[2:6] not in PACKED_DROPPED and pickable(v)]


def packed_hist_menu(kind):
    """The LDS-histogram kernels of int16-packed cubes (contiguous equal-width bins; afhip_planner.cpp: choose_hist_variant), same
    tuples as `menu`: stat 0 / 1, two-level / single-level, edge table / arithmetic edges — the shapes of the float32 histogram menu.  A
    menu and translation units of their own: `packed_menu` keeps its 69.
    Cells per lane, measured form by form on the configs[1] shape (profiles/packed_cube.txt, section 6): every form at one cell per lane
    (odd row lengths, and the faster width of six of the eight forms: two cells take 2 ... 39 % longer); two cells only for the
    single-level edge-table forms, which they carry 27 - 31 % faster.  The planner takes the widest form that divides the rows and that
    the production menu holds; the six other two-cell kernels are arms (`make MENU=arms`, AFHIP_PACKED_HIST_VEC=2).
    Rows in flight, from -Rpass-analysis=kernel-resource-usage (section 5): sixteen for the arithmetic-edge forms, which hold a burst as
    2-byte elements — but eight for the two-cell forms with a mean, which hold 12 bytes of scratch at sixteen — and eight for the table
    forms, which keep the unpacked value, the guess and two edges of every element of a burst in registers.  No kernel of the menu has
    scratch memory."""
    def one(vec, stat, sl, ha):
        feat = Feat.NT | Feat.INT_BINS | Feat.HIST | (Feat.SINGLE_LEVEL if sl else 0) | (Feat.ARITH_EDGES if ha else 0)
        depth = 16 if ha and not (vec == 2 and stat == 1) else 8
        return (I16, 0, vec, stat, 16, 16, depth, feat, 1 if vec == 1 or (sl and not ha) else 0)

    if kind == "dev":
        return [one(1, 0, 1, 1)]
    out = [one(vec, stat, sl, ha) for vec in PACKED_HIST_VECS for stat in (0, 1) for sl in (0, 1) for ha in (0, 1)]
    return out if kind == "arms" else [v for v in out if v[8]]


def end_bins_menu(kind):
    """The LDS-histogram kernels for partitions with a wide end bin on one side or both (Feat.END_BINS; afhip_planner.cpp:
    choose_hist_variant), same tuples as `menu`: the production histogram forms of each storage with the bit set, all of them sixteen
    slots x sixteen columns, nt loads, integer bins.  float32 (eight rows in flight) and float64 (four) at one cell per lane: stat 0 / 1 x
    two-level / single-level x edge table / arithmetic edges.  Packed storage: the ten shapes of the production `packed_hist_menu`, at
    its cells per lane and rows in flight.  No tuning arms; the `dev` menu has none of them (such a plan then routes without them)."""
    if kind == "dev":
        return []
    out = []
    for dtype, depth in ((0, 8), (1, 4)):
        for stat in (0, 1):
            for sl in (0, 1):
                for ha in (0, 1):
                    feat = Feat.NT | Feat.INT_BINS | Feat.HIST | Feat.END_BINS | (Feat.SINGLE_LEVEL if sl else 0) | (Feat.ARITH_EDGES if ha else 0)
                    out.append((dtype, 0, 1, stat, 16, 16, depth, feat, 1))
    out += [v[:7] + (v[7] | Feat.END_BINS, 1) for v in packed_hist_menu("full")]
    return out


def cell_map_menu(kind):
    """The LDS-histogram kernels for partitions whose interior widths differ (Feat.CELL_MAP; afhip_planner.cpp: find_cell_map), same
    tuples as `menu`: the edge-table entries of `end_bins_menu` with the bit set, entry by entry — float32 and float64 at one cell per lane,
    stat 0 / 1 x two-level / single-level; packed storage the same four at one cell per lane and the two single-level forms at two.  No
    arithmetic-edge form (the edges of such a partition are no lattice), no tuning arms; the `dev` menu has none of them.  Rows in flight
    are the end-bin twin's: no kernel of the menu has scratch memory (-Rpass-analysis=kernel-resource-usage; profiles/cell_map_bins.txt)."""
    return [v[:7] + (v[7] | Feat.CELL_MAP, 1) for v in end_bins_menu(kind) if not v[7] & Feat.ARITH_EDGES]


def packed_short_menu(kind):
    """The lean short-group kernels of int16-packed cubes (afhip_planner.cpp: choose_packed_short_variant), same tuples as `menu`: the
    float32 lean menu's seventeen shapes with nt loads — two-row groups: the sine-only form (K <= 2), stat 2 and stat 1 at two and six
    columns; four-row, three-row and mixed (one to four rows) groups: stat 1 / 2 at two and six columns — each at two cells and at one
    cell per lane (4 / 2 bytes per lane and row), and thirteen of them at four (8 bytes, what a float32 lane reads at two cells): 47
    kernels in units of their own.  The rows wait in their registers as 2-byte elements and are unpacked where a group's statistics
    consume them; from there on a kernel is its float32 twin.
    Rows in flight are the float32 twin's — eight, and six for three-row groups: a multiple of the group length, and with one copy of the
    group end per group of a block a deeper block is that much more code.  No kernel of the menu has scratch memory
    (-Rpass-analysis=kernel-resource-usage; profiles/packed_short_groups.txt has the register table).  PACKED_SHORT_DROPPED: the stat-2
    six-column forms at four cells per lane, every group length — 64 to 80 bytes of scratch at these depths, none at half of them but then
    168 to 171 VGPRs and two or three waves per SIMD; such a plan takes two cells per lane.
    All production, by the measurement of scripts/packed_short_bench.py on the configs[1] shape (profiles/packed_short_groups.txt, section
    2): every wider kernel's median lies below the next narrower one's minimum (four cells against two: x0.63 ... x0.96; two against one:
    x0.53 ... x0.82), and every class of plans beats the general packed kernel.  The `dev` menu has none of them.  Their region-fused
    twins, at two cells and at one, are in `packed_rf_menu`."""
    def one(vec, stat, kmax, depth, form=0, ss=1):
        feat = (Feat.SINE if stat == 2 else 0) | Feat.NT | Feat.SHORT_GROUP | Feat.LEAN | (Feat.LEAN_SINE if ss == 2 else 0) | form
        return (I16, 0, vec, stat, 0, kmax, depth, feat, 1)

    if kind == "dev":
        return []
    out = []
    for vec in (2, 1, 4):
        out.append(one(vec, 2, 2, 8, ss=2))
        out += [one(vec, stat, kmax, 8) for stat in (2, 1) for kmax in (2, 6)]
        for form, depth in ((Feat.FOUR_ROW, 8), (Feat.THREE_ROW, 6), (Feat.MIXED, 8)):
            out += [one(vec, stat, kmax, depth, form) for stat in (1, 2) for kmax in (2, 6)]
    return [v for v in out if v[2:4] + v[5:6] not in PACKED_SHORT_DROPPED]


def packed_rf_menu(kind):
    """The region-fused twins (Feat.REGION_FUSED, names `i16_..._rf`) of int16-packed cubes' kernels (afhip_planner.cpp: twin_of), same
    tuples as `menu`: of every production kernel of `packed_menu` at two cells and at one cell per lane with up to six columns and four
    threshold slots — the float rule of `menu` — and of every production kernel of `packed_short_menu` at two cells and at one.  No
    four-cell twin (the period end's scan is written for one and two cells per lane), none for the histogram menus.  Units of their own
    (``packed_rf_NN.hip``, compiled with the Makefile's PACKED_FLAGS): the older menus keep their counts and contents.
    Rows in flight are the plain kernel's, unless the twin then holds scratch memory (-Rpass-analysis=kernel-resource-usage;
    profiles/packed_region_fused.txt has the register table and every depth probed): PACKED_RF_SHALLOW names those and their depth — half
    the plain kernel's, a multiple of the group length and one of the depths the packed menus use; a twin with scratch at every depth is
    left out (PACKED_RF_DROPPED: such a plan keeps the per-cell route).  No kernel of the menu has scratch memory: 61 kernels.
    All production, by the measurement of scripts/packed_rf_bench.py (profiles/packed_region_fused.txt, sections 2 and 3; afhip_planner.cpp:
    rf_plan_ok and packed_rf_candidate hold the thresholds it set): every twin can be selected by some plan.  The `dev` menu has none of them."""
    if kind == "dev":
        return []
    out = []
    plain = [v for v in packed_menu("full") if v[2] <= 2 and v[5] <= 6 and v[4] <= 4] + [v for v in packed_short_menu("full") if v[2] <= 2]
    for dtype, pipe, vec, stat, nthr, kmax, depth, feat, prod in plain:
        if not prod:
            continue
        key = (vec, stat, nthr, kmax, feat & (Feat.SHORT_GROUP | Feat.LEAN | Feat.LEAN_SINE | GROUP_LENGTH))
        if key in PACKED_RF_DROPPED:
            continue
        out.append((dtype, pipe, vec, stat, nthr, kmax, PACKED_RF_SHALLOW.get(key, depth), feat | Feat.REGION_FUSED, 1))
    return out


def pickable(v):
    """False for a kernel that no plan can select by the planner's default rules (afhip_planner.cpp: the stage named in each comment), whatever its shape."""
    dtype, pipe, vec, stat, nthr, kmax, depth, feat, prod = v
    short = feat & (Feat.SHORT_GROUP | GROUP_LENGTH)            # a short-group form
    if kmax == 2 and (nthr == 16 or (nthr == 4 and stat in (1, 2))):
        return False      # every column adds at most one threshold slot, so slots <= K, and <= K - 1 beside a mean / sum / min / max /
        #                   sine_dd source (stat 3 may come from a non-integer pow on a threshold column: s3_t4_k2 stays) — lower_columns
    if dtype == 0 and pipe == 0 and vec == 2 and nthr == 16:
        return False      # load_path: two cells per lane need fewer than four slots (and an LDS-histogram plan takes one cell per lane: choose_variant)
    if dtype == 0 and pipe == 0 and vec == 2 and stat == 1 and nthr == 0 and kmax == 2:
        return False      # load_path: one cell per lane for light float32 plans: stat <= 1, no slot, K <= 2
    if short and stat == 1 and kmax == 2 and (not (feat & GROUP_LENGTH) or (dtype == 0 and feat & (Feat.THREE_ROW | Feat.MIXED))):
        return False      # short_group_form: stat-1 short-group plans need K >= min_k: 3 for two-row groups, and for float32 three-row / mixed groups
    return True


def name_of(v):
    dtype, pipe, vec, stat, nthr, kmax, depth, feat, prod = v
    return (f"{('f32', 'f64', 'i16')[dtype]}_p{pipe}_v{vec}_s{stat}_t{nthr}_k{kmax}_d{depth}"
            + "".join("_ss" if bit == Feat.LEAN and feat & Feat.LEAN_SINE else sfx for bit, sfx in SUFFIXES if feat & bit))


def inst(v):
    dtype, pipe, vec, stat, nthr, kmax, depth, feat, prod = v
    return f"k_fused_temporal<{CT[dtype]}, {pipe}, {vec}, {stat}, {nthr}, {kmax}, {max(depth, 1)}, {feat}>"


class _KeepIfSame:
    """Write a file only when its content changes, so `make` does not recompile an unchanged menu."""

    def __init__(self, fn):
        self.fn, self.parts = fn, []

    def __enter__(self):
        return self

    def write(self, text):
        self.parts.append(text)

    def __exit__(self, *exc):
        new = "".join(self.parts)
        try:
            with open(self.fn) as f:
                if f.read() == new:
                    return False
        except OSError:
            pass
        with open(self.fn, "w") as f:
            f.write(new)
        return False


def write_units(outdir, vs, per_file, stem):
    """The translation units of the kernels `vs`, `per_file` to a file: (file names, number of files)."""
    files = []
    ngroups = 0
    for i in range(0, len(vs), per_file):
        group = vs[i:i + per_file]
        idx = i // per_file
        ngroups += 1
        fn = os.path.join(outdir, f"{stem}_{idx:02d}.hip")
        with _KeepIfSame(fn) as f:
            f.write("// generated by gen_variants.py — do not edit\n")
            f.write('#include "afhip_kernels.h"\n#include "afhip_variants.h"\n')
            f.write("namespace afhip {\n")
            for v in group:
                f.write(f"template __global__ void {inst(v)}(const FusedArgs);\n")
            # host-only registration: kernel handles are taken in the TU that defines them
            f.write(f"int register_{stem}_{idx:02d}(Variant* out) {{\n    int n = 0;\n")
            for v in group:
                dtype, pipe, vec, stat, nthr, kmax, depth, feat, prod = v
                f.write(f"    out[n++] = Variant{{{dtype}, {pipe}, {vec}, {stat}, {nthr}, {kmax}, {depth}, {feat}, {prod}, (const void*)&{inst(v)}, \"{name_of(v)}\"}};\n")
            f.write("    return n;\n}\n}\n")
        files.append(fn)
    return files, ngroups


# The kernel menus, in table order: (key, menu function, ((unit stem, storage dtypes), ...)).  The key is the Menu enumerator of
# afhip_variants.h without its MENU_ prefix, in lower case; a menu's kernels stand in one slice of the table, stem by stem.  A stem's
# units hold the menu's kernels of the dtypes it names: float and packed kernels go to units of their own, because the packed ones are
# compiled with the Makefile's PACKED_FLAGS and the float ones as every float kernel.
MENUS = (
    ("float", menu, (("variants", (0, 1)),)),
    ("packed", packed_menu, (("packed", (I16,)),)),
    ("packed_hist", packed_hist_menu, (("packed_hist", (I16,)),)),
    ("end_bins", end_bins_menu, (("end_bins", (0, 1)), ("end_bins_packed", (I16,)))),
    ("cell_map", cell_map_menu, (("cell_map", (0, 1)), ("cell_map_packed", (I16,)))),
)
# ... continued: the menus that came after those five, same entries, behind them in the table.  (A tuple of its own: the length and
# keys of `MENUS` are what the older menus' recipe modules and tests know.)
MORE_MENUS = (
    ("packed_short", packed_short_menu, (("packed_short", (I16,)),)),
)
ALL_MENUS = MENUS + MORE_MENUS
# ... and on: the menus behind those six (a further tuple for the same reason: `MORE_MENUS` holds one menu and `ALL_MENUS` is the two above,
# by the packed short-group menu's tests).  `TABLE_MENUS` is every menu, in table order.
LATER_MENUS = (
    ("packed_rf", packed_rf_menu, (("packed_rf", (I16,)),)),
)
TABLE_MENUS = ALL_MENUS + LATER_MENUS


def write_table(outdir, kind, slices, units):
    """variants_table.hip: the table of every menu.  `slices`: the kernel count per menu, in TABLE_MENUS order; `units`: every unit's name."""
    fn = os.path.join(outdir, "variants_table.hip")
    starts = [sum(slices[:i]) for i in range(len(slices) + 1)]
    with _KeepIfSame(fn) as f:
        f.write("// generated by gen_variants.py — do not edit\n")
        f.write('#include "afhip_variants.h"\n')
        f.write("namespace afhip {\n")
        for name in FEAT_NAMES:
            f.write(f'static_assert(FEAT_{name} == {getattr(Feat, name)}, "gen_variants.py and afhip_plan_types.h disagree on a FEAT bit");\n')
        f.write(f'static_assert(MENU_COUNT == {len(TABLE_MENUS)}, "gen_variants.py and afhip_variants.h disagree on the menus");\n')
        for i, (key, _, _) in enumerate(TABLE_MENUS):
            f.write(f'static_assert(MENU_{key.upper()} == {i}, "gen_variants.py and afhip_variants.h disagree on the menus");\n')
        for u in units:
            f.write(f"int register_{u}(Variant* out);\n")
        f.write(f"static Variant g_table[{max(starts[-1], 1)}];\nstatic int g_count = -1;\n")
        f.write(f"static const int g_start[MENU_COUNT + 1] = {{{', '.join(map(str, starts))}}};      // each menu's slice of g_table\n")
        f.write(f'const char* variants_menu() {{ return "{kind}"; }}\n')
        keys = ", ".join(f'"{key}"' for key, _, _ in TABLE_MENUS)
        f.write(f"const char* menu_key(Menu m) {{\n    static const char* const keys[MENU_COUNT] = {{{keys}}};\n    return keys[m];\n}}\n")
        f.write("const Variant* menu_table(Menu m, int* n) {\n    if (g_count < 0) {\n        int c = 0;\n")
        for u in units:
            f.write(f"        c += register_{u}(g_table + c);\n")
        f.write("        g_count = c;\n    }\n    *n = g_start[m + 1] - g_start[m];\n    return g_table + g_start[m];\n}\n}\n")
    return fn


def main():
    outdir = sys.argv[1]
    kind = "full"
    per_file = 4
    args = sys.argv[2:]
    while args:
        a = args.pop(0)
        if a == "--menu":
            kind = args.pop(0)
        elif a == "--per-file":
            per_file = int(args.pop(0))
    os.makedirs(outdir, exist_ok=True)
    files, slices = [], []
    for key, fn, stems in TABLE_MENUS:
        vs = fn(kind)
        assert all(sum(v[0] in dtypes for _, dtypes in stems) == 1 for v in vs), key      # every kernel in one stem's units
        slices.append(len(vs))
        for stem, dtypes in stems:
            files += write_units(outdir, [v for v in vs if v[0] in dtypes], per_file, stem)[0]
    units = [os.path.basename(x)[:-len(".hip")] for x in files]
    files.append(write_table(outdir, kind, slices, units))
    print(" ".join(os.path.basename(x) for x in files))


if __name__ == "__main__":
    main()
