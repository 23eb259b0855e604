"""The public read and write paths with every buffer of aggfly_amd/io.py poisoned: staging, `tmp`, decode scratch, slots and the cube
itself come from `torch.empty`, which hands out each fill of tests/poison.py while a route runs (`poisoned_empty`).

Every route runs through its existing route test — the smallest store or file of that test, a request box that cuts chunks where the
test has one, and the test's own assertion that the `device="cuda"` cube equals the host route's bit for bit — once per fill, one
fill twice first; on top, every dataset the route opens on the device is recorded, and the cubes must be the same bits under all fills
(under `ones` a cell nobody wrote would read as NaN or -1).  The write side: `dataset_to_zarr(encode="gpu")` (take_box, shuffle_blocks
into the poisoned `tmp`, the two encoders into poisoned slots, copy_ranges) writes byte-identical trees, poisoned or not
(`zstd_encode_cases.tree_hashes`)."""
import inspect

import numpy as np
import pytest

import poison
import zstd_encode_cases as zc

import test_gpu_blosc_flavours as t_flavours
import test_gpu_decode as t_decode
import test_gpu_grib as t_grib
import test_gpu_grib_ccsds as t_ccsds
import test_gpu_grib_complex as t_complex
import test_gpu_inflate_decode as t_inflate
import test_gpu_netcdf3 as t_nc3
import test_gpu_packed as t_packed
import test_gpu_packed_rules as t_rules
import test_gpu_tiff as t_tiff
import test_gpu_tiff_bands as t_bands
import test_gpu_time_last as t_tlast
import test_gpu_zarr_filters as t_filters
import test_gpu_zstd_decode as t_zstd

# the fixtures of the existing route tests, under names of their own here
from test_gpu_blosc_flavours import store_cube as flavours_store_cube                          # noqa: F401
from test_gpu_grib import no_host_route as grib_no_host_route, windows_files as grib_windows_files            # noqa: F401
from test_gpu_grib_ccsds import no_host_route as ccsds_no_host_route, windows_files as ccsds_windows_files    # noqa: F401
from test_gpu_grib_complex import no_host_route as complex_no_host_route, windows_files as complex_windows_files  # noqa: F401
from test_gpu_netcdf3 import files as nc3_files, no_host_route as nc3_no_host_route            # noqa: F401
from test_gpu_tiff import files as tiff_files, no_host_route as tiff_no_host_route             # noqa: F401
from test_gpu_tiff_bands import files as bands_files, no_host_route as bands_no_host_route     # noqa: F401
from test_gpu_zarr_filters import spies as filters_spies                                       # noqa: F401

import aggfly_amd as af

pytestmark = pytest.mark.gpu

ORDER = ("random", "random", "zero", "ones", "plausible")
FIXTURES = {t_flavours: "flavours", t_grib: "grib", t_ccsds: "ccsds", t_complex: "complex", t_nc3: "nc3", t_tiff: "tiff", t_bands: "bands", t_filters: "filters"}


def _param(fn, **match):
    """The parameter set of ``fn``'s (single, multi-name) parametrize mark whose named values are ``match`` -> dict."""
    for m in fn.pytestmark:
        if m.name == "parametrize" and "," in m.args[0]:
            names = [n.strip() for n in m.args[0].split(",")]
            for values in m.args[1]:
                row = dict(zip(names, values))
                if all((row[k]["name"] if isinstance(row[k], dict) else row[k]) == v for k, v in match.items()):
                    return row
    raise KeyError(match)


def _case(fn, case):
    """The parameter set of ``fn`` for the catalogue case ``case``, decoded in HBM where the test has that arm."""
    try:
        return _param(fn, case=case, gpu_decode="1")
    except KeyError:
        return _param(fn, case=case, gpu_decode="0")


def _tiff_case(torch_cuda, monkeypatch, files, name, gpu_decode):
    """One file of tests/tiff_cases.py on the device route (`test_every_case_streams_into_hbm` of tests/test_gpu_tiff.py without its
    `monkeypatch.undo()`, which would take the poison away): the cube equals the host route's bit for bit."""
    case = next(c for c in t_tiff.CASES if c["name"] == name)
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", gpu_decode)
    calls = []
    real = t_tiff.hip.lzw_decode
    monkeypatch.setattr(t_tiff.hip, "lzw_decode", lambda *a: calls.append(a[2]) or real(*a))
    ds = af.dataset_from_path(files[name], "v", device="cuda", lon_is_360=False, tiff_time=case["tiff_time"])
    monkeypatch.setattr(t_tiff.hip, "lzw_decode", real)
    assert ds.cube().is_cuda and not ds.is_packed and (len(calls) > 0) == (gpu_decode == "1")
    host = af.dataset_from_path(files[name], "v", lon_is_360=False, tiff_time=case["tiff_time"])
    got = ds.cube().cpu().numpy()
    t_tiff._same_bits(got, t_tiff._host_as(host.cube(), got.dtype))


# route -> [(module, test function name, its parameters)]: the existing route tests
ROUTES = {
    "zarr-v2-blosc-lz4-byte-shuffle": [(t_decode, "test_store_to_hbm_gpu_decode_equals_host_decode", dict(layout="space_tiled"))],
    "zarr-v2-blosc-zstd": [(t_flavours, "test_stores_of_the_new_flavours_read_the_same_on_both_routes", dict(compress="blosc-zstd", layout="space_tiled"))],
    "zarr-v2-blosc-bit-shuffle": [(t_flavours, "test_stores_of_the_new_flavours_read_the_same_on_both_routes", dict(compress="blosc-bitshuffle", layout="space_tiled"))],
    "zarr-v2-zlib": [(t_inflate, "test_zarr_v2_zlib_store_equal_across_routes", {})],
    "zarr-v2-delta-fixedscaleoffset": [(t_filters, "test_device_read_equals_the_host_read", dict(name="fso_delta", route=t_filters.ROUTES[1])),
                                       (t_filters, "test_device_read_equals_the_host_read", dict(name="fso_i32_f64_delta", route=t_filters.ROUTES[2])),
                                       (t_filters, "test_windows_time_last_and_keep_packed", dict(route=t_filters.ROUTES[1]))],
    "zarr-v3-zstd-sharded": [(t_zstd, "test_zstd_stores_read_bit_exact_on_both_routes", {}), (t_decode, "test_format3_stores_and_shards_decode_in_hbm", dict(shards={"time": 96, "latitude": 24, "longitude": 64}))],
    "zarr-time-last": [(t_tlast, "test_time_last_stores_on_every_device_route", dict(dtype=np.float32, fmt=2, compress=True, chunks=(5, 7, 96))),
                       (t_tlast, "test_a_sharded_time_last_store", {})],
    "netcdf-classic": [(t_nc3, "test_windows_read_the_same_box_as_the_host_cube", dict(name="float_cdf1", time="window", space="regions")),
                       (t_nc3, "test_windows_read_the_same_box_as_the_host_cube", dict(name="short_cdf2_two", time="sel", space="band"))],
    "hdf5-shuffle-deflate": [(t_inflate, "test_netcdf4_files_read_bit_exact_on_both_routes", dict(fn="nc4_like.nc")),
                             (t_inflate, "test_netcdf4_files_read_bit_exact_on_both_routes", dict(fn="old_style.h5"))],
    "grib-simple-bitmap": [(t_grib, "test_windows_read_the_same_box", dict(name="bitmap12", time="window", space="regions")),
                           (t_grib, "test_windows_read_the_same_box", dict(name="plain12", time="sel", space="band"))],
    "grib-complex": [(t_complex, "test_windows_read_the_same_box", dict(name="bitmap", time="window", space="regions")),
                     (t_complex, "test_windows_read_the_same_box", dict(name="plain", time="sel", space="band"))],
    "grib-ccsds": [(t_ccsds, "test_windows_read_the_same_box", dict(name="bitmap", time="window", space="regions")),
                   (t_ccsds, "test_windows_read_the_same_box", dict(name="plain", time="sel", space="band"))],
    "geotiff-lzw-predictor-2": [(None, "_tiff_case", dict(name="u2 comp5 pred2 tiles", gpu_decode="1")), (None, "_tiff_case", dict(name="u2 comp5 pred2 strips", gpu_decode="0"))],
    "geotiff-deflate-predictor-3": [(None, "_tiff_case", dict(name="f4 comp8 pred3 tiles", gpu_decode="0")),
                                    (t_tiff, "test_windows_read_what_the_host_route_reads",
                                     lambda: dict(_param(t_tiff.test_windows_read_what_the_host_route_reads, name="f4 nodata -9999 seven days", gpu_decode="1"), time="window", space="regions+band"))],
    "geotiff-multi-band-chunky": [(t_bands, "test_every_case_streams_into_hbm", lambda: _case(t_bands.test_every_case_streams_into_hbm, "chunky B2 u1 pred2 comp5 tiles II BigTIFF")),
                                  (t_bands, "test_every_case_streams_into_hbm", lambda: _case(t_bands.test_every_case_streams_into_hbm, "chunky B3 f4 pred3 comp8 tiles II")),
                                  (t_bands, "test_windows_select_bands_and_segments",
                                   lambda: dict(_param(t_bands.test_windows_select_bands_and_segments, name="two pages x three bands chunky f4 pred3"), space="regions"))],
    "keep-packed-int16": [(t_packed, "test_keep_packed_zarr_store_against_the_float32_route", dict(comp=t_packed.LZ4, chunks=(100, 4, 5)))],
    "keep-packed-uint16-multi-store": [(t_rules, "test_stores_of_one_packing_and_of_mixed_signedness", {}), (t_rules, "test_three_stores_of_different_packings_stay_packed", {})],
}


def _bytes_of(ds):
    """What a dataset on the device holds, on the host: the cube's bytes, or a packed cube's stored integers."""
    try:
        c = ds.cube()
    except Exception:
        return None
    q = getattr(c, "q", c)
    if not getattr(q, "is_cuda", False):
        return None
    return q.contiguous().cpu().numpy().copy()


def _run_once(request, torch, tmp, fill, calls):
    """Every test of ``calls`` once under ``fill`` -> the device datasets they opened, in order."""
    seen = []
    with pytest.MonkeyPatch.context() as mp:
        real = af.dataset_from_path

        def spy(*a, **k):
            ds = real(*a, **k)
            got = _bytes_of(ds)
            if got is not None:
                seen.append(got)
            return ds

        mp.setattr(af, "dataset_from_path", spy)
        handed = poison.poisoned_empty(mp, torch, fill)
        for i, (mod, name, params) in enumerate(calls):
            fn = getattr(mod, name) if mod is not None else globals()[name]
            mod = mod if mod is not None else t_tiff
            params = params() if callable(params) else params
            kw = {}
            for arg in inspect.signature(fn).parameters:
                if arg in params:
                    kw[arg] = params[arg]
                elif arg == "torch_cuda":
                    kw[arg] = torch
                elif arg == "tmp_path":
                    kw[arg] = tmp / f"{fill}-{len(list(tmp.iterdir()))}"
                    kw[arg].mkdir()
                elif arg == "monkeypatch":
                    kw[arg] = mp
                else:
                    kw[arg] = request.getfixturevalue(f"{FIXTURES[mod]}_{arg}")
            if isinstance(kw.get("spies"), dict):                  # a function-scoped fixture there, one object for every call here
                kw["spies"].update({k: 0 for k in kw["spies"]})
            fn(**kw)
        assert handed, "the route took nothing from torch.empty"
    assert seen, "the route opened no dataset on the device"
    return seen


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_under_every_fill(torch_cuda, request, tmp_path, route):
    first = None
    for fill in ORDER:
        seen = _run_once(request, torch_cuda, tmp_path, fill, ROUTES[route])
        if first is None:
            first = seen
            continue
        assert len(seen) == len(first)
        for k, (a, b) in enumerate(zip(first, seen)):
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)), \
                f"{route}: dataset {k} under {fill!r} differs from the first run"


@pytest.mark.parametrize("compress", ["blosc", "blosc-zstd"], ids=["blosc-lz4", "blosc-zstd"])
def test_gpu_written_trees_are_byte_identical_poisoned_or_not(torch_cuda, tmp_path, compress):
    """take_box, shuffle_blocks (into `tmp`), lz4_encode_streams / zstd_encode_blocks (into the slots), copy_ranges."""
    ds = zc.small_dataset()
    cube = np.asarray(ds.cube()).copy()
    kw = dict(chunks=zc.SMALL_CHUNKS, compress=compress)
    af.dataset_to_zarr(ds.to_device(), str(tmp_path / "plain"), encode="gpu", **kw)
    want = zc.tree_hashes(str(tmp_path / "plain"))
    assert len(want) > 4
    back = af.dataset_from_path(str(tmp_path / "plain"), "var", lon_is_360=True).cube()
    assert np.asarray(back).tobytes() == cube.tobytes()                               # (the tree decodes to the cube)
    for fill in ORDER:
        with pytest.MonkeyPatch.context() as mp:
            handed = poison.poisoned_empty(mp, torch_cuda, fill)
            path = str(tmp_path / f"{fill}-{len(list(tmp_path.iterdir()))}")
            af.dataset_to_zarr(ds.to_device(), path, encode="gpu", **kw)
            assert handed
        assert zc.tree_hashes(path) == want, fill
