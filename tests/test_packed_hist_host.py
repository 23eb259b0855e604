"""The LDS-histogram menu of int16- / uint16-packed cubes (gen_variants.py: packed_hist_menu) without a GPU: its shape, its names, what
the loaded library reports, and that the recipes of `packed_hist_recipes` are what they claim.  (FusedArgs' layout is held by the
static_asserts of afhip_kernels.h: the library that these tests load compiled with them.)"""
import numpy as np

import packed_hist_recipes as ph
import packed_recipes as pr
import variant_recipes as vr


def test_packed_hist_menu_shape_and_build_info():
    from aggfly_amd import hip
    gv = vr.gen_variants()
    full = gv.packed_hist_menu("full")
    names = [gv.name_of(v) for v in full]
    assert names and len(names) == len(set(names))
    assert all(n.startswith("i16_p0_v") and "_hist" in n and "_nt_ibins" in n for n in names)
    assert not set(names) & {gv.name_of(v) for v in gv.menu("arms")}
    assert not set(names) & {gv.name_of(v) for v in gv.packed_menu("full")}
    # one cell per lane (odd rows): both statistic tiers, both levels, both edge forms; two cells: a part of those forms in the production
    # menu (the widths that measured faster), all of them with the arms; bins only, 16 x 16
    forms = lambda menu, vec: {(v[3], bool(v[7] & gv.Feat.SINGLE_LEVEL), bool(v[7] & gv.Feat.ARITH_EDGES)) for v in menu if v[2] == vec}      # noqa: E731
    every = {(s, sl, ha) for s in (0, 1) for sl in (False, True) for ha in (False, True)}
    arms = gv.packed_hist_menu("arms")
    assert forms(full, 1) == every and forms(full, 2) and forms(full, 2) <= every and {v[2] for v in full} == {1, 2}
    assert forms(arms, 1) == forms(arms, 2) == every and set(full) <= set(arms) and all(v[8] == (v in full) for v in arms)
    assert all(v[0] == pr.I16 and v[1] == 0 and v[4] == 16 and v[5] == 16 and v[7] & gv.Feat.HIST and v[7] & gv.Feat.INT_BINS and v[7] & gv.Feat.NT for v in arms)
    assert len(gv.packed_hist_menu("dev")) <= 1
    info = hip.build_info()
    assert info["packed_hist_variants"] == len(gv.packed_hist_menu(info["menu"]))
    assert info["packed_variants"] == len(gv.packed_menu(info["menu"])) and info["variants"] == len(gv.menu(info["menu"]))       # as before
    assert len(gv.packed_menu("full")) == 69


def test_recipes_are_partitions_with_the_data_on_their_edges():
    for t in vr.menu_of("packed_hist", "full"):
        v = vr.variant(t)
        r = ph.recipe(v)
        bins = [c for c in r.columns if c["inner"] == "bins"]
        assert 13 <= len(bins) <= 16 and len(r.columns) == len(bins) + (v.stat == 1) <= 16 and r.exact_order
        e = np.array(r.edges)
        assert len(e) == len(bins) + 1 and np.all(np.diff(e) > 0) and np.allclose(np.diff(e), e[1] - e[0], rtol=1e-12)
        assert sorted(c["inner_args"][:2] for c in bins) == [(e[i], e[i + 1]) for i in range(len(bins))]           # contiguous: t1[b] == t0[b + 1]
        assert r.n_cells % v.vec == 0 and (v.vec == 2 or r.n_cells % 2 == 1) and r.n_cells > 256 * v.vec
        f32_exact = all(float(np.float32(x)) == x for x in e)
        assert f32_exact == v.has(vr.HA)
        q = ph.stored_cube(r, seed=1)
        vals = pr.np_unpack(q)
        on = ph.stored_on_edges(r.edges)
        assert bool(on) == v.has(vr.HA)                              # an arithmetic plan has an edge that stored integers meet exactly
        assert all((vals == np.float32(x)).any() for x in on)
        lo = pr.np_unpack([pr.stored_near(x) for x in e], fill=None)
        hi = pr.np_unpack([pr.stored_near(x) + 1 for x in e], fill=None)
        assert np.all(lo <= e) and np.all(hi > e) and all((vals == a).any() and (vals == b).any() for a, b in zip(lo, hi))
        assert (vals < e[0]).sum() > 4 and (vals > e[-1]).sum() > 4 and {32767, -32768} <= set(np.unique(q).tolist())      # both guard bins
        ib = r.inner_bounds
        assert np.isnan(vals).all(axis=0).sum() == 3                # whole cells of fills
        assert any(np.isnan(vals[ib[g]:ib[g + 1]]).all(axis=0).sum() > 3 for g in range(len(ib) - 1) if ib[g + 1] > ib[g])
