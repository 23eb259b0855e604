"""The menu of lean short-group kernels for packed cubes (gen_variants.py: MORE_MENUS, packed_short_menu) and the recipes that
`tests/test_gpu_packed_short.py` runs on them, checked without a GPU: the menu's shape and names, no name shared with another menu or
arm, the older menus as they were, the loaded library's count (`hip.menu_size`), and that every recipe is what it claims — group
lengths, periods, lean columns, cell counts — with the planted fills and stored extremes in its cube."""
import zlib

import numpy as np
import pytest

import packed_recipes as pr
import packed_short_recipes as ps
import variant_recipes as vr

FULL = ps.menu_of("full")
VARIANTS = [vr.variant(t) for t in FULL]
FORM_DEPTH = {"pair": 8, "quad": 8, "tri": 6, "rag": 8}
FORM_SUFFIX = {"pair": "_pair_lean", "quad": "_pair_lean_quad", "tri": "_pair_lean_tri", "rag": "_pair_lean_rag"}


def test_menu_shape_and_names():
    gv = vr.gen_variants()
    assert [key for key, _, _ in gv.MORE_MENUS] == [ps.KEY] and gv.ALL_MENUS == gv.MENUS + gv.MORE_MENUS
    assert len(FULL) == 47 and all(t[8] == 1 for t in FULL)
    assert ps.menu_of("arms") == FULL and ps.menu_of("dev") == []
    names = [v.name for v in VARIANTS]
    assert len(set(names)) == 47
    shapes = {}
    for v in VARIANTS:
        assert (v.dtype, v.pipe, v.nthr) == (pr.I16, 0, 0) and v.stat in (1, 2) and v.kmax in (2, 6) and v.vec in (1, 2, 4), v.name
        assert v.has(vr.NT) and v.has(vr.PAIR) and v.lean >= 1 and not v.has(vr.RF) and v.depth == FORM_DEPTH[v.form], v.name
        assert v.has(_sine_bit()) == (v.stat == 2), v.name
        if v.lean == 2:
            assert v.form == "pair" and v.stat == 2 and v.kmax == 2 and v.name.endswith("_nt_pair_ss"), v.name
        else:
            assert v.name.endswith("_nt" + FORM_SUFFIX[v.form]), v.name
        assert v.name.startswith(f"i16_p0_v{v.vec}_s{v.stat}_t0_k{v.kmax}_d{v.depth}_"), v.name
        shapes.setdefault(v.vec, set()).add((v.form, v.lean, v.stat, v.kmax))
    # the float32 lean menu's seventeen shapes, at two cells and at one cell per lane; at four all but the stat-2 six-column forms
    want = {("pair", 2, 2, 2)} | {(form, 1, stat, kmax) for form in FORM_DEPTH for stat in (1, 2) for kmax in (2, 6)}
    four = {x for x in want if x[2:] != (2, 6)}
    assert len(want) == 17 and len(four) == 13 and shapes == {1: want, 2: want, 4: four}
    # ... the forms the float menu holds for float32, region-fused twins and tuning arms aside, are among them
    lean32 = {(w.form, w.lean, w.stat, w.kmax) for w in (vr.variant(t) for t in vr.menu_of("float", "full"))
              if w.dtype == vr.F32 and w.lean and not w.has(vr.RF)}
    assert lean32 <= want


def _sine_bit():
    return vr.gen_variants().Feat.SINE


def test_no_name_is_shared_with_another_menu_or_arm():
    gv = vr.gen_variants()
    others = [gv.name_of(t) for kind in ("full", "arms") for _, menu, _ in gv.MENUS for t in menu(kind)]
    assert not set(others) & {v.name for v in VARIANTS}
    assert not any(n.startswith("i16_") and "_pair" in n for n in others)


def test_the_older_menus_are_as_they_were():
    gv = vr.gen_variants()
    assert [key for key, _, _ in gv.MENUS] == ["float", "packed", "packed_hist", "end_bins", "cell_map"]
    assert [len(menu("full")) for _, menu, _ in gv.MENUS] == [367, 69, 10, 26, 14]
    assert not any(t[0] == pr.I16 and t[7] & vr.PAIR for kind in ("full", "arms", "dev") for _, menu, _ in gv.MENUS for t in menu(kind))


def test_menu_size_counts_the_loaded_build():
    from aggfly_amd import hip
    gv = vr.gen_variants()
    info = hip.build_info()
    kind = info["menu"]
    assert hip.menu_size(ps.KEY) == len(ps.menu_of(kind))
    for key, menu, _ in gv.ALL_MENUS:
        assert hip.menu_size(key) == len(menu(kind)), key
    assert list(info)[-1] == "end_bins_variants" and ps.KEY not in " ".join(info)          # the build-info string is as it was


@pytest.mark.parametrize("name", [v.name for v in VARIANTS])
def test_recipe_is_what_it_claims(name):
    v = next(x for x in VARIANTS if x.name == name)
    r = ps.recipe(v)
    assert r.name == name and r.dtype == pr.I16 and r.exact_order and r.tuning == 0
    lens = np.diff(r.inner_bounds)
    assert set(lens.tolist()) == set(ps.GROUP_ROWS[v.form]) and r.T == lens.sum()
    assert len(lens) == {"pair": 150, "quad": 75, "tri": 101, "rag": 120}[v.form]
    if v.form == "tri":
        assert len(lens) % (v.depth // 3) == 1                          # a lone group in the last block of six rows
    ob = r.outer_bounds
    per = np.diff(ob)
    assert ob[0] == 0 and ob[-1] == len(lens) and per[1] == 0 and set(per[[0] + list(range(2, len(per) - 1))].tolist()) == {ps.PERIOD} and 0 < per[-1] <= ps.PERIOD
    # K == kmax lean columns of the kernel's statistic tier
    cols = r.columns
    assert len(cols) == v.kmax and vr.slots_of(cols) == 0
    for c in cols:
        assert c["inner"] in (("mean", "sum") if v.stat == 1 else ("mean", "sum", "min", "max", "sine_dd")), c
        assert c["outer"] in ("sum", "mean") and c.get("transform") in (None, "pow"), c
        if c.get("transform") == "pow":
            assert float(c["transform_arg"]).is_integer() and c["transform_arg"] >= 1, c
        if c["inner"] == "sine_dd":
            assert c["inner_args"][0] < c["inner_args"][1], c
    if v.stat == 2:
        assert any(c["inner"] in ("min", "max", "sine_dd") for c in cols)
    if v.lean == 2:
        assert all(c["inner"] == "sine_dd" and c.get("transform") is None for c in cols)
    # cells per lane by the row length: more than one 256-thread workgroup's cells, no multiple of a wave's
    assert r.n_cells > 256 * v.vec and r.n_cells % v.vec == 0 and r.n_cells % (64 * v.vec) != 0
    assert r.n_cells % 2 == 1 if v.vec == 1 else (r.n_cells % 4 == 0 if v.vec == 4 else (r.n_cells % 2 == 0 and r.n_cells % 4 != 0))
    # the data
    q = ps.stored_cube(r, seed=zlib.crc32(name.encode()))
    assert q.shape == (r.T, r.n_cells) and q.dtype == np.int16
    first, last, whole, ocean = ps.fill_census(r, q)
    assert first > 0 and last > 0 and whole > 0 and ocean == 3
    assert {32767, -32768} <= set(np.unique(q).tolist())
    values = pr.np_unpack(q)
    assert all((values == np.float32(e)).any() for e in r.sine_edges) and np.isnan(values).sum() == (q == pr.FILL).sum()
