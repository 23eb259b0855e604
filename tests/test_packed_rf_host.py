"""The menu of region-fused twins for packed cubes (gen_variants.py: LATER_MENUS, packed_rf_menu) and the recipes that
`tests/test_gpu_packed_rf.py` runs on them, checked without a GPU: the menu's shape and names, every twin beside its plain kernel, no name
shared with another menu or arm, the older menus as they were, the loaded library's count (`hip.menu_size`), the build-info keys, and that
every recipe is what it claims — cells per lane, group lengths, periods, columns, the share of the period values — with the planted
fills and stored extremes in its cube."""
import zlib

import numpy as np
import pytest

import packed_recipes as pr
import packed_rf_recipes as prf
import variant_recipes as vr

FULL = prf.menu_of("full")
VARIANTS = [vr.variant(t) for t in FULL]


def test_menu_shape_and_names():
    gv = vr.gen_variants()
    assert [key for key, _, _ in gv.LATER_MENUS] == [prf.KEY] and gv.TABLE_MENUS == gv.MENUS + gv.MORE_MENUS + gv.LATER_MENUS
    assert [stems for key, _, stems in gv.LATER_MENUS] == [(("packed_rf", (pr.I16,)),)]
    assert len(FULL) == 61 and all(t[8] == 1 for t in FULL)
    assert prf.menu_of("arms") == FULL and prf.menu_of("dev") == []
    names = [v.name for v in VARIANTS]
    assert len(set(names)) == len(names)
    for v in VARIANTS:
        assert v.name.startswith(f"i16_p0_v{v.vec}_s{v.stat}_t{v.nthr}_k{v.kmax}_d{v.depth}_nt") and v.name.endswith("_rf"), v.name
        assert (v.dtype, v.pipe) == (pr.I16, 0) and v.vec in (1, 2) and v.kmax <= 6 and v.nthr <= 4 and v.has(vr.RF) and v.has(vr.NT), v.name
        assert not (v.has(vr.TKI) or v.has(vr.SL) or v.has(vr.HB)), v.name
    general = [v for v in VARIANTS if not v.form]
    short = [v for v in VARIANTS if v.form]
    assert len(general) == 27 and len(short) == 34
    # every short-group kernel at two cells and at one has its twin; of the general ones all but the seven that hold scratch memory at every depth
    assert {v.form for v in short} == {"pair", "quad", "tri", "rag"} and all(v.lean >= 1 and v.nthr == 0 for v in short)
    want = {(w.vec, w.stat, w.nthr, w.kmax) for w in (vr.variant(t) for t in vr.menu_of("packed", "full")) if w.vec <= 2 and w.kmax <= 6 and w.nthr <= 4}
    dropped = {(1, 0, 4, 6), (1, 1, 4, 6), (1, 3, 1, 6), (1, 3, 4, 2), (1, 3, 4, 6), (2, 3, 0, 2), (2, 3, 0, 6)}
    assert len(want) == 34 and dropped <= want and {(v.vec, v.stat, v.nthr, v.kmax) for v in general} == want - dropped
    assert {k[:4] for k in gv.PACKED_RF_DROPPED} == dropped and not set(gv.PACKED_RF_DROPPED) & set(gv.PACKED_RF_SHALLOW)


def test_every_twin_stands_beside_its_plain_kernel():
    gv = vr.gen_variants()
    plains = []
    for v in VARIANTS:
        w = prf.plain_of(v)
        assert w is not None, v.name
        # the same fields but `depth`, which is the plain kernel's or half of it
        assert v.depth in (w.depth, w.depth // 2) and v.depth % {"": 1, "pair": 2, "quad": 4, "tri": 3, "rag": 4}[v.form] == 0, (v.name, w.name)
        assert v.name == w.name.replace(f"_d{w.depth}_", f"_d{v.depth}_") + "_rf"
        key = (v.vec, v.stat, v.nthr, v.kmax, v.feat & prf._MASK)
        assert (v.depth < w.depth) == (key in gv.PACKED_RF_SHALLOW) and gv.PACKED_RF_SHALLOW.get(key, w.depth) == v.depth, v.name
        plains.append(w.name)
    assert len(set(plains)) == len(plains)
    # ... and every production short-group kernel at two cells and at one is some twin's plain kernel
    short = [vr.variant(t).name for t in prf.plain_menus() if vr.variant(t).form and vr.variant(t).vec <= 2]
    assert len(short) == 34 and set(short) <= set(plains)


def test_no_name_is_shared_with_another_menu_or_arm():
    gv = vr.gen_variants()
    others = [gv.name_of(t) for kind in ("full", "arms") for _, menu, _ in gv.ALL_MENUS for t in menu(kind)]
    assert not set(others) & {v.name for v in VARIANTS}
    assert not any(n.startswith("i16_") and n.endswith("_rf") for n in others)


def test_the_older_menus_are_as_they_were():
    gv = vr.gen_variants()
    assert [key for key, _, _ in gv.MENUS] == ["float", "packed", "packed_hist", "end_bins", "cell_map"]
    assert [len(menu("full")) for _, menu, _ in gv.MENUS] == [367, 69, 10, 26, 14]
    assert [key for key, _, _ in gv.MORE_MENUS] == ["packed_short"] and gv.ALL_MENUS == gv.MENUS + gv.MORE_MENUS
    assert [len(menu("full")) for _, menu, _ in gv.MORE_MENUS] == [47]
    assert not any(t[0] == pr.I16 and t[7] & vr.RF for kind in ("full", "arms", "dev") for _, menu, _ in gv.ALL_MENUS for t in menu(kind))


def test_menu_size_counts_the_loaded_build():
    from aggfly_amd import hip
    gv = vr.gen_variants()
    info = hip.build_info()
    kind = info["menu"]
    assert hip.menu_size(prf.KEY) == len(prf.menu_of(kind))
    for key, menu, _ in gv.TABLE_MENUS:
        assert hip.menu_size(key) == len(menu(kind)), key
    # the build-info string is as it was: its keys, and region_fused_twins still counts the float menu's
    assert list(info) == ["menu", "variants", "arms", "region_fused_twins", "abi", "packed_variants", "packed_hist_variants", "end_bins_variants"]
    assert info["region_fused_twins"] == sum(1 for t in vr.menu_of("float", kind) if t[7] & vr.RF)


@pytest.mark.parametrize("name", [v.name for v in VARIANTS])
def test_recipe_is_what_it_claims(name):
    v = next(x for x in VARIANTS if x.name == name)
    w = prf.plain_of(v)
    r = prf.recipe(v)
    assert r.name == w.name and r.dtype == pr.I16 and not r.exact_order and r.region_fused and r.tuning == 0
    # cells per lane by the row length: never four, a last wave tile that is partly filled
    assert r.n_cells == 71 * (130 if v.vec == 2 else 129) and r.n_cells % 4 != 0 and r.n_cells % 2 == (0 if v.vec == 2 else 1) and r.n_cells % (64 * v.vec) != 0
    lens = np.diff(r.inner_bounds)
    assert len(lens) == 60 and r.T == lens.sum()
    assert set(lens.tolist()) == {"": {24}, "pair": {2}, "quad": {4}, "tri": {3}, "rag": {2, 3, 4}}[v.form]
    ob = r.outer_bounds
    per = np.diff(ob)
    assert ob[0] == 0 and ob[-1] == 60 and per[1] == 0 and (np.delete(per, 1) > 0).all()
    P = len(per)
    assert P == (61 if prf.daily_panel(w) else (6 if v.form else 13))
    assert prf.daily_panel(w) == (v.stat == 0 or (v.form == "pair" and not (v.lean == 1 and v.kmax == 6)))
    # the share of the period values: far above the planner's thresholds (0.2 %; 10 % for the light two-row forms)
    assert prf.share(r) >= 20 * (0.10 if prf.light_two_row(w) else 0.002)
    # the columns fill the kernel: K == kmax, the slot tier, the statistic tier; nothing the route refuses
    cols = r.columns
    assert len(cols) == v.kmax and not any(c.get("rounding") for c in cols)
    slots = vr.slots_of(cols)
    assert {0: slots == 0, 1: slots == 1, 4: 2 <= slots <= 4}[v.nthr], (slots, cols)
    if v.form:
        for c in cols:
            assert c["inner"] in (("mean", "sum") if v.stat == 1 else ("mean", "sum", "min", "max", "sine_dd")) and c["outer"] in ("sum", "mean"), c
            assert c.get("transform") in (None, "pow") and float(c.get("transform_arg", 1.0)).is_integer(), c
    if v.stat == 0:
        assert all(c["inner"] in ("dd", "bins") for c in cols)
    if v.stat == 2:
        assert any(c["inner"] in ("min", "max", "sine_dd") for c in cols)
    if v.lean == 2:
        assert all(c["inner"] == "sine_dd" and c.get("transform") is None for c in cols)
    if v.stat == 3:
        assert any(c["inner"] == "nanmean" or (c.get("transform") == "pow" and not float(c["transform_arg"]).is_integer()) for c in cols)
    # the data
    q = prf.stored_cube(r, seed=zlib.crc32(name.encode()))
    assert q.shape == (r.T, r.n_cells) and q.dtype == np.int16
    f = q == pr.FILL
    ib = r.inner_bounds
    assert f.all(axis=0).sum() == 3 and f[:, r.n_cells - 1].all()                        # ocean cells, the last one included
    wp = prf.whole_period_cells(r)
    lo, hi = ib[ob[prf.WHOLE_PERIOD]], ib[ob[prf.WHOLE_PERIOD + 1]]
    assert hi > lo and f[lo:hi, wp].all() and not f[:, wp].all(axis=0).any()             # a whole period of fills
    single = sum(int((f[ib[g]] & (f[ib[g]:ib[g + 1]].sum(axis=0) == 1)).sum()) for g in range(60))
    assert single > 100                                                                  # single steps
    assert {32767, -32768} <= set(np.unique(q).tolist())
    values = pr.np_unpack(q)
    assert all((values == np.float32(e)).any() for e in r.edges + r.sine_edges) and np.isnan(values).sum() == f.sum()
