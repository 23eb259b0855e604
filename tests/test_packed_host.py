"""int16-packed cubes, the parts that need no GPU: the packed kernel menu, the holder's pair folding, the window sizes of the
sharded planner and the layout of the new C structs."""
import ctypes
import json
import os
import re

import numpy as np
import pandas as pd
import pytest

import aggfly_amd as af
from aggfly_amd import distributed as dist
from aggfly_amd import hip
from aggfly_amd import io as afio

import packed_recipes as pr
import variant_recipes as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC4 = os.path.join(ROOT, "tests", "golden", "hdf5", "nc4_like.nc")


def test_packed_menu_is_a_menu_of_its_own():
    gv = vr.gen_variants()
    for kind in ("full", "dev"):
        names = [gv.name_of(v) for v in gv.packed_menu(kind)]
        assert len(names) == len(set(names)) and all(n.startswith("i16_p0_v") and n.endswith("_nt") for n in names)
        assert not set(names) & {gv.name_of(v) for v in gv.menu("arms")}
    assert len(gv.packed_menu("full")) <= 96 and len(gv.packed_menu("dev")) == 2
    info = hip.build_info()
    assert info["packed_variants"] == len(gv.packed_menu(info["menu"]))
    assert info["variants"] == len(gv.menu(info["menu"]))            # the float tables count as before


def test_every_packed_variant_has_a_recipe_that_fills_its_template():
    gv = vr.gen_variants()
    for t in gv.packed_menu("full"):
        v, r = vr.variant(t), pr.recipe(t)
        assert r.dtype == pr.I16 and len(r.columns) == v.kmax and vr.slots_of(r.columns) <= v.nthr
        assert r.n_cells % v.vec == 0 and r.n_cells > vr.WG * v.vec and r.n_cells % (vr.WG * v.vec)
        assert (v.vec == 4) == (r.n_cells % 4 == 0) and (v.vec == 1) == (r.n_cells % 2 == 1)
        lens = np.diff(r.inner_bounds)
        assert (lens == 0).any() and (lens[lens > 0] % v.depth != 0).all()
    q = pr.stored_cube_for(pr.recipe(gv.packed_menu("full")[0]), seed=1)
    assert q.dtype == np.int16 and {32767, -32768, pr.FILL} <= set(np.unique(q).tolist())


def _cube():
    return af.PackedCube(np.arange(24, dtype=np.int16).reshape(2, 3, 4), 0.0017, 281.3, -32767)


def test_scalar_arithmetic_folds_into_the_pair_list():
    x = _cube()
    assert x.n_pairs == 1 and x.dtype.is_floating_point and tuple(x.shape) == (2, 3, 4)
    c = x - 273.15
    assert isinstance(c, af.PackedCube) and c.n_pairs == 2 and c.pairs[1] == (None, np.float32(-273.15))
    f = (x - 273.15) * 1.8 + 32
    assert isinstance(f, af.PackedCube) and f.n_pairs == 3 and f.pairs[2] == (np.float32(1.8), np.float32(32))
    assert x.n_pairs == 1                                    # the operands are left as they were
    for g in (2.0 * x, x * 2, 1 + x):
        assert isinstance(g, af.PackedCube) and g.q is x.q
    bare = af.PackedCube(np.zeros((1, 1, 2), np.int16))
    assert bare.n_pairs == 0 and (bare - 273.15).pairs == [(None, np.float32(-273.15))]
    # a scale-only cube takes the addend into its own pair
    assert (af.PackedCube(np.zeros((1, 1, 2), np.int16), scale_factor=0.01) - 273.15).pairs == [(np.float32(0.01), np.float32(-273.15))]
    p = f.packing()
    assert (p.n_pairs, p.has_fill, p.fill) == (3, 1, -32767)
    assert list(p.mul) == [np.float32(0.0017), 1.0, np.float32(1.8)]
    assert list(p.add) == [np.float32(281.3), np.float32(-273.15), 32.0]
    idle = bare.packing()                                   # halves a chain lacks travel as exact identities: 1.0 and -0.0
    assert list(idle.mul) == [1.0] * 3 and all(a == 0.0 and np.signbit(a) for a in idle.add)
    # views and indexing stay packed and keep the rule
    v = x.permute(1, 2, 0)[1:, [0, 2]]
    assert isinstance(v, af.PackedCube) and tuple(v.shape) == (2, 2, 2) and v.pairs == x.pairs and v.fill_value == -32767
    with pytest.raises(TypeError):
        af.PackedCube(np.zeros(3, np.float32))
    assert not hasattr(x, "data_ptr") and not hasattr(x, "__array__")


def _values_or_refusal(op):
    """What does not fold materialises the float32 values, which takes the GPU: without one it raises `HipEngineError`."""
    if hip.device_count() == 0:
        with pytest.raises(hip.HipEngineError):
            op()
        return
    out = op()
    assert not isinstance(out, af.PackedCube) and out.is_cuda and out.dtype.is_floating_point


def test_what_does_not_fold_asks_for_the_values():
    x = _cube()
    full = (x - 273.15) * 1.8 + 32
    for op in (lambda: x / 2.0, lambda: x ** 2, lambda: 1.0 - x, lambda: -x, lambda: full + 1.0, lambda: full * 2.0, lambda: x.materialize()):
        _values_or_refusal(op)
    ds = af.Dataset(af.DataArray(x, ["time", "latitude", "longitude"],
                                 {"time": pd.date_range("2001-01-01", periods=2), "latitude": [1.0, 2.0, 3.0], "longitude": [1.0, 2.0, 3.0, 4.0]}),
                    preprocess=lambda a: a - 273.15)
    assert ds.is_packed and ds.da.data.n_pairs == 2 and ds.packed_cube().q.dtype.is_floating_point is False
    _values_or_refusal(ds.cube)                             # float values: materialised on demand, on the GPU only


def _int16_store(tmp_path):
    T, ny, nx = 96, 4, 6
    store = str(tmp_path / "p.zarr")
    os.makedirs(store)
    json.dump({"zarr_format": 2}, open(os.path.join(store, ".zgroup"), "w"))
    packed = np.arange(T * ny * nx, dtype=np.int16).reshape(T, ny, nx)
    afio._write_array(store, "t2m", packed, ("time", "latitude", "longitude"), (48, ny, nx),
                      {"scale_factor": 0.0017, "add_offset": 281.3, "_FillValue": -32767}, None)
    afio._write_array(store, "f32", packed.astype(np.float32), ("time", "latitude", "longitude"), (48, ny, nx), {}, None)
    return store, ny * nx


def test_step_bytes_and_windows_follow_the_opt_in(tmp_path, monkeypatch):
    monkeypatch.delenv("AGGFLY_HIP_KEEP_PACKED", raising=False)
    store, cells = _int16_store(tmp_path)
    for path, var, n in ((NC4, "t2m_packed", 9 * 14), (store, "t2m", cells)):
        assert dist._step_bytes(path, var) == 4 * n
        assert dist._step_bytes(path, var, keep_packed=True) == 2 * n
        monkeypatch.setenv("AGGFLY_HIP_KEEP_PACKED", "1")
        assert dist._step_bytes(path, var) == 2 * n
        monkeypatch.delenv("AGGFLY_HIP_KEEP_PACKED")
    # float storage is not packed, whatever is asked for
    assert dist._step_bytes(store, "f32", keep_packed=True) == 4 * cells and dist._step_bytes(NC4, "t2m", keep_packed=True) == 4 * 9 * 14
    bounds = np.arange(0, 97, 8)                            # twelve periods of eight steps
    budget = 16 * 4 * cells                                 # sixteen unpacked steps
    wide = dist.plan_windows(bounds, 0, 12, dist._step_bytes(store, "t2m"), budget)
    packed = dist.plan_windows(bounds, 0, 12, dist._step_bytes(store, "t2m", keep_packed=True), budget)
    assert [b - a for a, b in wide] == [2] * 6 and [b - a for a, b in packed] == [4] * 3


def test_new_structs_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "aggfly_hip.h")).read()
    assert re.search(r"typedef struct afhip_packing \{ int32_t n_pairs, has_fill, fill, pad; float mul\[3\], add\[3\]; \} afhip_packing;", hdr)
    assert ctypes.sizeof(hip.Packing) == 4 * 4 + 4 * 6
    assert [n for n, _ in hip.Packing._fields_] == ["n_pairs", "has_fill", "fill", "pad", "mul", "add"]
    assert ctypes.sizeof(hip.PlanDesc) == 8 + 8 + 4 + 4 + 8 + 8 + 8 + 8 + 8 + 4 + 4      # unchanged: ABI 4
    assert int(re.search(r"#define AFHIP_I16 (\d+)", hdr).group(1)) == hip.I16 == pr.I16
