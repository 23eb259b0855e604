"""The menu of LDS-histogram kernels for partitions whose interior widths differ (gen_variants.py: cell_map_menu), the recipes that
`tests/test_gpu_cell_map.py` runs on them and the cell map itself (aggfly_amd/csrc/afhip_cell_map.h), checked without a GPU: the menu's
shape and names, the loaded library's counts (`hip.menu_size`), that every recipe is what it claims and its cube holds the planted
values, and the stand-alone checker `tests/cell_map_check.cpp`, compiled and run."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import cell_map_recipes as cm
import end_bins_recipes as eb
import packed_recipes as pr
import variant_recipes as vr

FULL = vr.menu_of("cell_map", "full")
VARIANTS = [vr.variant(t) for t in FULL]


def test_menu_shape_and_names():
    gv = vr.gen_variants()
    assert len(FULL) == 14 and all(t[8] == 1 for t in FULL)
    # the edge-table forms of the end-bin menu with the bit set, entry by entry
    table_forms = [t for t in vr.menu_of("end_bins", "full") if not t[7] & vr.HA]
    assert [t[:7] + (t[7] & ~cm.CM,) + t[8:] for t in FULL] == table_forms and all(t[7] & cm.CM for t in FULL)
    names = [v.name for v in VARIANTS]
    assert len(set(names)) == len(names)
    others = {gv.name_of(t) for kind in ("full", "arms") for key, menu, _ in gv.MENUS if key != "cell_map" for t in menu(kind)}
    assert not others & set(names) and not any("_cmap" in n for n in others)
    for v in VARIANTS:
        assert v.name.endswith("_hist_ends_cmap") and "_nt_ibins" in v.name and "_arith" not in v.name, v.name
        assert (v.pipe, v.nthr, v.kmax) == (0, 16, 16) and v.stat in (0, 1)
        assert v.has(cm.CM) and v.has(eb.EB) and v.has(vr.HB) and v.has(vr.TKI) and v.has(vr.NT) and not v.has(vr.HA)
    for dtype, depth in ((vr.F32, 8), (vr.F64, 4)):
        forms = {(v.stat, v.has(vr.SL)) for v in VARIANTS if v.dtype == dtype}
        assert len(forms) == 4 == sum(v.dtype == dtype for v in VARIANTS)
        assert all((v.vec, v.depth) == (1, depth) for v in VARIANTS if v.dtype == dtype)
    assert sorted(v.vec for v in VARIANTS if v.dtype == pr.I16) == [1] * 4 + [2] * 2
    assert all(v.has(vr.SL) for v in VARIANTS if v.vec == 2)
    # no tuning arms; the dev menu has none of them
    assert vr.menu_of("cell_map", "arms") == FULL and vr.menu_of("cell_map", "dev") == []
    assert [key for key, _, _ in gv.MENUS] == ["float", "packed", "packed_hist", "end_bins", "cell_map"]


def test_the_older_menus_keep_their_counts():
    gv = vr.gen_variants()
    assert [len(menu("full")) for _, menu, _ in gv.MENUS[:4]] == [367, 69, 10, 26]
    assert not any(t[7] & cm.CM for kind in ("full", "arms", "dev") for _, menu, _ in gv.MENUS[:4] for t in menu(kind))


def test_menu_size_counts_the_loaded_build():
    from aggfly_amd import hip
    gv = vr.gen_variants()
    info = hip.build_info()
    kind = info["menu"]
    assert hip.menu_size("cell_map") == len(vr.menu_of("cell_map", kind))
    assert hip.menu_size("end_bins") == info["end_bins_variants"]
    assert hip.menu_size("float") == info["variants"] and hip.menu_size("packed") == info["packed_variants"]
    assert hip.menu_size("packed_hist") == info["packed_hist_variants"]
    assert hip.menu_size("no_such_menu") == -1 and hip.menu_size("") == -1
    assert list(info)[-1] == "end_bins_variants"                        # the build-info string is as it was
    for key, menu, _ in gv.MENUS:
        assert hip.menu_size(key) == len(menu(kind)), key


@pytest.mark.parametrize("name", [v.name for v in VARIANTS])
def test_recipe_fills_its_tier_and_its_data_are_planted(name):
    v = next(x for x in VARIANTS if x.name == name)
    r = cm.recipe(v)
    bins = eb.bins_of(r.columns)
    assert len(bins) == vr.slots_of(r.columns) == 16 - v.stat and len(r.columns) == 16
    assert all(a[1] == b[0] for a, b in zip(bins[:-1], bins[1:])) and all(t1 > t0 for t0, t1 in bins)
    assert len(cm.distinct_widths(bins)) >= 3
    w, m, inner = cm.cells_of(bins)
    assert 1 <= m <= cm.MAX_CELLS and len(inner) >= 3
    assert r.n_cells % v.vec == 0
    assert set(inner) <= set(r.edges) and {x for b in bins for x in b if np.isfinite(x)} <= set(r.edges)
    seed = zlib.crc32(name.encode())
    if eb.is_packed(v.dtype):
        q = cm.stored_cube(r, seed)
        values, have = pr.np_unpack(q), cm.planted(r, pr.np_unpack(q), q)
    else:
        values = cm.cube_for(r, seed)
        have = cm.planted(r, values)
    assert all(have.values()), {k: ok for k, ok in have.items() if not ok}
    for t0, t1 in bins:                                                 # every bin, the end bins included, is met
        assert ((values > t0) & (values < t1)).sum() > 5, (t0, t1)


def test_every_kind_of_end_is_among_the_recipes():
    kinds = {(np.isinf(b[0][0]), np.isinf(b[-1][1])) for b in (eb.bins_of(cm.recipe(v).columns) for v in VARIANTS)}
    assert kinds == {(True, True), (False, False), (True, False), (False, True)}


def test_cells_of_the_eight_bin_spec():
    w, m, inner = cm.cells_of(cm.EIGHT)
    assert (w, m) == (2.5, 18) and inner == [-7.5, -5.0, -2.5, 2.5, 5.0, 7.5, 12.5, 15.0, 17.5, 22.5, 27.5, 32.5]


def test_the_stand_alone_checker_passes(tmp_path):
    """tests/cell_map_check.cpp: a program of its own that includes afhip_cell_map.h alone — the emulated guess against the true bin on
    random and hand-picked partitions, and the partitions that must be refused."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    root = vr.ROOT
    exe = str(tmp_path / "cell_map_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(root, "aggfly_amd", "csrc"), os.path.join(root, "tests", "cell_map_check.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "cell_map_check: 0 failures" in out.stdout, out.stdout + out.stderr
