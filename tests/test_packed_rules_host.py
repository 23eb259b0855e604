"""Packed cubes with several unpack rules along time (`PackedCube.concat`), without a GPU: how the rules join, how views, indexing
and scalar arithmetic carry them, what a multi-rule cube refuses, the loader's decision which stores stay packed
(`io.packed_rules_of`), and the C entry point `afhip_plan_bind_packings`."""
import os
import re

import numpy as np
import pytest

import aggfly_amd as af
from aggfly_amd import hip
from aggfly_amd import io as afio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

A = dict(scale_factor=0.0017, add_offset=281.3, fill_value=-32767)
B = dict(scale_factor=0.002, add_offset=270.0, fill_value=-32768)
C_ = dict(add_offset=250.0)                     # a store without scale_factor, without a fill
D = dict(scale_factor=0.01)                     # ... and one without add_offset
RA = ([(f32(0.0017), f32(281.3))], -32767)
RB = ([(f32(0.002), f32(270.0))], -32768)
RC = ([(None, f32(250.0))], None)
RD = ([(f32(0.01), None)], None)


def _part(n, kw, ny=2, nx=3, seed=0, dtype=np.int16):
    rng = np.random.default_rng(seed)
    return af.PackedCube(rng.integers(0, 30000, (n, ny, nx)).astype(dtype), **kw)


def _three():
    return af.PackedCube.concat([_part(5, A, seed=1), _part(3, B, seed=2), _part(4, C_, seed=3)])


def test_concat_joins_the_rules_along_time():
    parts = [_part(5, A, seed=1), _part(3, B, seed=2), _part(4, C_, seed=3)]
    cube = af.PackedCube.concat(parts)
    assert cube.n_rules == 3 and cube.rule_bounds == [0, 5, 8, 12] and cube.rules == [RA, RB, RC]
    assert tuple(cube.shape) == (12, 2, 3) and cube.storage == "int16" and cube.nbytes() == 12 * 6 * 2
    assert np.array_equal(cube.q.numpy(), np.concatenate([p.q.numpy() for p in parts]))
    assert "rules=3" in repr(cube) and "[0, 5, 8, 12]" in repr(cube)
    # the parts of a multi-rule cube join like cubes
    again = af.PackedCube.concat([cube, _part(2, C_, seed=4), _part(2, A, seed=5)])
    assert again.n_rules == 4 and again.rule_bounds == [0, 5, 8, 14, 16]


def test_equal_neighbours_merge_and_empty_parts_are_dropped():
    one = af.PackedCube.concat([_part(5, A, seed=1), _part(3, A, seed=2), _part(4, A, seed=3)])
    assert one.n_rules == 1 and one.rule_bounds == [0, 12]
    assert one.pairs == RA[0] and one.fill_value == -32767 and one.n_pairs == 1              # a single-rule cube, whole surface
    assert "pairs=" in repr(one) and "rules=" not in repr(one)
    two = af.PackedCube.concat([_part(5, A), _part(0, B), _part(3, A), _part(4, B)])
    assert two.n_rules == 2 and two.rule_bounds == [0, 8, 12] and two.rules == [RA, RB]
    assert af.PackedCube.concat([_part(0, B), _part(4, A)]).pairs == RA[0]
    # equal means equal in float32, the fill included
    near = dict(A, fill_value=-32766)
    assert af.PackedCube.concat([_part(2, A), _part(2, near)]).n_rules == 2
    assert af.PackedCube.concat([_part(2, A), _part(2, dict(A, scale_factor=float(f32(0.0017))))]).n_rules == 1


def test_mixed_storage_raises():
    with pytest.raises(ValueError, match="int16 and uint16"):
        af.PackedCube.concat([_part(2, A), _part(2, dict(scale_factor=0.1), dtype=np.uint16)])
    u = af.PackedCube.concat([_part(2, dict(scale_factor=0.1, fill_value=65535), dtype=np.uint16), _part(3, dict(scale_factor=0.2), dtype=np.uint16)])
    assert u.n_rules == 2 and u.storage == "uint16" and u.rules[0][1] == 65535
    with pytest.raises(TypeError):
        af.PackedCube.concat([_part(2, A), np.zeros((2, 2, 3), np.int16)])


def test_time_slices_rebase_the_bounds_and_integers_pick_their_rule():
    cube = _three()
    s = cube[3:10]
    assert s.n_rules == 3 and s.rule_bounds == [0, 2, 5, 7] and np.array_equal(s.q.numpy(), cube.q.numpy()[3:10])
    s = cube[5:]
    assert s.n_rules == 2 and s.rule_bounds == [0, 3, 7] and s.rules == [RB, RC]
    s = cube[-6:-1]
    assert s.n_rules == 2 and s.rule_bounds == [0, 2, 5]
    inside = cube[5:8]                                      # inside one rule: a single-rule cube whose surface is that rule's
    assert inside.n_rules == 1 and inside.pairs == RB[0] and inside.fill_value == -32768 and inside.packing().fill == -32768
    assert cube[6:7].pairs == RB[0] and cube[:5].fill_value == -32767
    for t, r in ((0, RA), (4, RA), (5, RB), (7, RB), (8, RC), (11, RC), (-1, RC), (-12, RA)):
        x = cube[t]
        assert x.n_rules == 1 and tuple(x.shape) == (2, 3) and (x.pairs, x.fill_value) == r, t
        assert np.array_equal(x.q.numpy(), cube.q.numpy()[t])
    with pytest.raises(IndexError):
        cube[12]
    # a slice of a slice
    assert cube[2:11][2:7].rule_bounds == [0, 1, 4, 5]


def test_views_track_the_time_axis():
    cube = _three()
    p = cube.permute(1, 2, 0)                               # (lat, lon, time), what Dataset holds
    assert tuple(p.shape) == (2, 3, 12) and p.n_rules == 3 and p.rule_bounds == [0, 5, 8, 12]
    s = p[:, :, 4:9]
    assert s.n_rules == 3 and s.rule_bounds == [0, 1, 4, 5] and tuple(s.shape) == (2, 3, 5)
    assert p[:, :, 6].pairs == RB[0] and p[..., 9:].pairs == RC[0] and p[..., 6].fill_value == -32768
    k = p[1:, :2]                                           # keys on the spatial axes keep the rules
    assert k.n_rules == 3 and k.rule_bounds == [0, 5, 8, 12] and tuple(k.shape) == (1, 2, 12)
    assert p[0].rule_bounds == [0, 5, 8, 12] and p[0][:, 5:].rule_bounds == [0, 3, 7]
    assert cube[:, 1].n_rules == 3 and cube[:, 1][6:].rule_bounds == [0, 2, 6]
    back = p.permute(2, 0, 1).contiguous()
    assert back.rule_bounds == [0, 5, 8, 12] and np.array_equal(back.q.numpy(), cube.q.numpy())
    t = cube.transpose(0, 2)
    assert t[:, :, 5:8].pairs == RB[0] and t.transpose(0, 2)[8:].pairs == RC[0]
    u = cube.unsqueeze(0)
    assert tuple(u.shape) == (1, 12, 2, 3) and u[:, 7:].rule_bounds == [0, 1, 5] and cube.unsqueeze(-1)[5:].n_rules == 2
    assert cube.clone().rules == cube.rules and cube.to("cpu").rule_bounds == cube.rule_bounds
    da = af.DataArray(cube, ["time", "latitude", "longitude"], {"time": np.arange(12)}).transpose("latitude", "longitude", "time")
    assert da.isel(time=slice(4, 9)).data.rule_bounds == [0, 1, 4, 5] and da.isel(latitude=1).data.n_rules == 3


def test_scalar_arithmetic_lands_in_every_rule():
    cube = af.PackedCube.concat([_part(5, A), _part(3, C_), _part(4, D), _part(2, {})])
    c = cube - 273.15
    assert isinstance(c, af.PackedCube) and c.rule_bounds == cube.rule_bounds
    k = f32(-273.15)
    assert c.rules == [([(f32(0.0017), f32(281.3)), (None, k)], -32767), ([(None, f32(250.0)), (None, k)], None),
                       ([(f32(0.01), k)], None), ([(None, k)], None)]       # the add lands in the half a rule lacks
    f = cube * 1.8 + 32
    assert isinstance(f, af.PackedCube) and f.rules == [
        ([(f32(0.0017), f32(281.3)), (f32(1.8), f32(32))], -32767), ([(None, f32(250.0)), (f32(1.8), f32(32))], None),
        ([(f32(0.01), None), (f32(1.8), f32(32))], None), ([(f32(1.8), f32(32))], None)]
    assert cube.rules[0] == RA                                           # the operands are left as they were
    assert (3.0 + cube).rules[3] == ([(None, f32(3.0))], None) and (2 * cube).rules[2][0] == [(f32(0.01), None), (f32(2.0), None)]
    # a fold makes rules equal or keeps them apart as they come: two stores that differ in the offset only still differ afterwards
    assert af.PackedCube.concat([_part(2, A), _part(2, dict(A, add_offset=280.0))]).__sub__(273.15).n_rules == 2


def test_a_fold_one_rule_cannot_take_asks_for_the_values():
    full = (_part(3, A) - 273.15) * 1.8                      # three pairs, the last without its add
    assert full.n_pairs == 3
    cube = af.PackedCube.concat([_part(4, C_), full])
    assert cube.n_rules == 2
    more = cube + 32                                         # room in both rules: the free half of one, a new pair of the other
    assert isinstance(more, af.PackedCube) and more.rules[1][0][2] == (f32(1.8), f32(32)) and more.rules[0][0] == [(None, f32(250.0)), (None, f32(32))]
    with pytest.raises(hip.HipEngineError):                  # one rule is full: the whole cube goes to values — and here is no GPU,
        cube * 2.0                                           # the values have no host form
    with pytest.raises(hip.HipEngineError):
        more + 1.0
    for op in (lambda x: x / 2.0, lambda x: x ** 2, lambda x: -x, lambda x: 1.0 - x, lambda x: x.detach(), lambda x: x[::2], lambda x: x[[0, 5]]):
        with pytest.raises(hip.HipEngineError):
            op(cube)


def test_a_multi_rule_cube_has_no_single_packing():
    cube = _three()
    for read in (lambda: cube.pairs, lambda: cube.n_pairs, lambda: cube.fill_value, lambda: cube.packing()):
        with pytest.raises(ValueError, match="rules"):
            read()
    arr, bounds = cube.packings()
    assert len(arr) == 3 and bounds.dtype == np.int64 and bounds.tolist() == [0, 5, 8, 12]
    assert [(p.n_pairs, p.has_fill, p.fill) for p in arr] == [(1, 1, -32767), (1, 1, -32768), (1, 0, 0)]
    assert arr[2].mul[0] == 1.0 and arr[2].add[0] == f32(250.0) and np.signbit(arr[0].add[1]) and arr[0].mul[1] == 1.0
    # single-rule cubes: the surface tests/test_packed_host.py reads
    x = af.PackedCube(np.zeros((2, 3, 4), np.int16), 0.0017, 281.3, -32767)
    assert x.n_rules == 1 and x.rule_bounds == [0, 2] and x.rules == [RA] and x.pairs == RA[0] and x.fill_value == -32767
    p = ((x - 273.15) * 1.8 + 32).packing()
    assert (p.n_pairs, p.has_fill, p.fill) == (3, 1, -32767)
    v = x.permute(1, 2, 0)[:2, :2, :]
    assert v.pairs == x.pairs and v.fill_value == -32767 and v[..., ::2].pairs == x.pairs       # any key keeps a single rule
    assert len(x.packings()[0]) == 1


P_A, P_B = (0.0017, 281.3, -32767, False), (0.002, 270.0, -32767, False)


def test_the_loaders_decision():
    assert afio.packed_rules_of([P_A, P_B, P_A]) == [P_A, P_B, P_A]                  # different packings: one rule per store
    same = afio.packed_rules_of([P_A, P_A, P_A])
    assert same == [P_A] * 3
    cube = af.PackedCube.concat([af.PackedCube(np.zeros((2, 1, 1), np.int16), *r) for r in same])
    assert cube.n_rules == 1 and cube.rule_bounds == [0, 6]                          # ... equal packings: one rule
    assert afio.packed_rules_of([P_A, (0.1, 0.0, None, True)]) is None               # int16 beside uint16
    assert afio.packed_rules_of([(0.1, 0.0, 65535, True), (0.2, None, None, True)]) is not None
    assert afio.packed_rules_of([P_A, None, P_B]) is None                            # a float store (`packing_of` gives None)
    assert afio.packed_rules_of([]) is None and afio.packed_rules_of([P_A]) == [P_A]

    class Z:
        def __init__(self, dtype, attrs):
            self.dtype, self.attrs = dtype, attrs
    stores = [Z("<i2", {"scale_factor": 0.0017, "add_offset": 281.3, "_FillValue": -32767}), Z("<i2", {"add_offset": 250.0}), Z("<f4", {})]
    assert afio.packed_rules_of([afio.packing_of(z) for z in stores[:2]]) == [(0.0017, 281.3, -32767, False), (None, 250.0, None, False)]
    assert afio.packed_rules_of([afio.packing_of(z) for z in stores]) is None


def test_the_entry_point_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "aggfly_hip.h")).read()
    assert re.search(r"int afhip_plan_bind_packings\(afhip_plan\* plan, const afhip_packing\* rules, const int64_t\* bounds, int32_t n\);", hdr)
    assert "#define AFHIP_ABI_VERSION 4" in hdr and "afhip_plan_bind_packings" in hip.EXPORTS
    lib = hip.load()
    assert hasattr(lib, "afhip_plan_bind_packings") and hasattr(lib, "afhip_plan_bind_packing")
    assert lib.afhip_plan_bind_packings(None, None, None, 1) == hip.E_INVALID        # no plan: refused before anything is touched
