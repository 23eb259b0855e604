"""The menu of LDS-histogram kernels for partitions with a wide end bin (gen_variants.py: end_bins_menu) and the recipes that
`tests/test_gpu_end_bins.py` runs on them, checked without a GPU: the menu's shape and names, the loaded library's counts, and that
every recipe is what it claims — a partition with a wide end whose cube holds the values the exactness rule is about."""
import zlib

import numpy as np
import pytest

import end_bins_recipes as eb
import packed_recipes as pr
import variant_recipes as vr

FULL = vr.menu_of("end_bins", "full")
VARIANTS = [vr.variant(t) for t in FULL]


def test_menu_shape_and_names():
    gv = vr.gen_variants()
    assert len(FULL) == 26 and all(t[8] == 1 for t in FULL)
    names = [v.name for v in VARIANTS]
    assert len(set(names)) == len(names)
    others = {gv.name_of(t) for kind in ("full", "arms") for menu in (gv.menu, gv.packed_menu, gv.packed_hist_menu) for t in menu(kind)}
    assert not others & set(names) and not any("_ends" in n for n in others)
    for v in VARIANTS:
        assert "_hist" in v.name and v.name.endswith("_ends") and "_nt_ibins" in v.name, v.name
        assert (v.pipe, v.nthr, v.kmax) == (0, 16, 16) and v.stat in (0, 1)
        assert v.has(eb.EB) and v.has(vr.HB) and v.has(vr.TKI) and v.has(vr.NT)
    # float32 / float64: the eight forms at one cell per lane, eight / four rows in flight
    for dtype, depth in ((vr.F32, 8), (vr.F64, 4)):
        forms = {(v.stat, v.has(vr.SL), v.has(vr.HA)) for v in VARIANTS if v.dtype == dtype}
        assert len(forms) == 8 == sum(v.dtype == dtype for v in VARIANTS)
        assert all((v.vec, v.depth) == (1, depth) for v in VARIANTS if v.dtype == dtype)
    # packed: the production packed_hist_menu with the bit set, entry by entry
    packed = [t for t in FULL if t[0] == pr.I16]
    assert [t[:7] + (t[7] & ~eb.EB,) for t in packed] == [t[:8] for t in vr.menu_of("packed_hist", "full") if t[8]]
    assert sorted(v.vec for v in VARIANTS if v.dtype == pr.I16) == [1] * 8 + [2] * 2
    assert all(v.has(vr.SL) and not v.has(vr.HA) for v in VARIANTS if v.vec == 2)
    # no tuning arms; the dev menu has none of them
    assert vr.menu_of("end_bins", "arms") == FULL and vr.menu_of("end_bins", "dev") == []


def test_the_older_menus_keep_their_counts():
    gv = vr.gen_variants()
    assert len(gv.packed_menu("full")) == 69 and len(gv.packed_hist_menu("full")) == 10 and len(gv.packed_hist_menu("arms")) == 16
    assert not any(t[7] & eb.EB for kind in ("full", "arms", "dev") for menu in (gv.menu, gv.packed_menu, gv.packed_hist_menu) for t in menu(kind))


def test_build_info_counts_the_new_table():
    from aggfly_amd import hip
    gv = vr.gen_variants()
    info = hip.build_info()
    kind = info["menu"]
    assert list(info)[-1] == "end_bins_variants"                        # appended at the end of the string
    assert info["end_bins_variants"] == len(vr.menu_of("end_bins", kind))
    assert info["variants"] == len(gv.menu(kind)) and info["packed_variants"] == len(gv.packed_menu(kind))
    assert info["packed_hist_variants"] == len(gv.packed_hist_menu(kind))
    if kind == "full":
        assert (info["packed_variants"], info["packed_hist_variants"], info["end_bins_variants"]) == (69, 10, 26)


@pytest.mark.parametrize("name", [v.name for v in VARIANTS])
def test_recipe_is_a_partition_with_a_wide_end_and_its_data_are_planted(name):
    v = next(x for x in VARIANTS if x.name == name)
    r = eb.recipe(v)
    bins = eb.bins_of(r.columns)
    assert len(bins) == vr.slots_of(r.columns) == 16 - v.stat and len(r.columns) == 16
    assert all(a[1] == b[0] for a, b in zip(bins[:-1], bins[1:])) and all(t1 > t0 for t0, t1 in bins)
    widths = [t1 - t0 for t0, t1 in bins[1:-1]]
    assert len(widths) >= 2 and np.allclose(widths, widths[0], rtol=1e-9, atol=0)
    assert any(eb.wide_ends(bins))
    assert r.n_cells % v.vec == 0
    exact = all(float(np.float32(x)) == x for x in r.edges)
    assert exact == v.has(vr.HA)
    seed = zlib.crc32(name.encode())
    if eb.is_packed(v.dtype):
        q = eb.stored_cube(r, seed)
        have = eb.planted(r, pr.np_unpack(q), q)
    else:
        have = eb.planted(r, eb.cube_for(r, seed))
    assert all(have.values()), {k: ok for k, ok in have.items() if not ok}


def test_every_kind_of_end_is_among_the_recipes():
    kinds = set()
    for v in VARIANTS:
        bins = eb.bins_of(eb.recipe(v).columns)
        kinds.add((eb.wide_ends(bins), np.isinf(bins[0][0]), np.isinf(bins[-1][1])))
    assert {((True, True), True, True), ((True, True), False, False), ((True, False), False, False), ((False, True), False, True)} <= kinds
