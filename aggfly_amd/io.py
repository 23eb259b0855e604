"""Loaders feeding the hot path: ``dataset_from_path``, a dependency-free Zarr (formats 2 and 3) reader /
writer, and the streaming routes that put chunked stores (Zarr, netCDF-4) straight into HBM.

The reference opens stores through xarray (`aggfly/dataset/dataset.py:636-740`) and converts
to time-contiguous Zarr with `dataset_to_zarr` / `zarr_from_path`
(`aggfly/dataset/zarr_convert.py:50-156`).  Neither xarray nor zarr/netCDF4 is installed here
or on the GPU box, so this module reads the containers itself, with numpy, the standard library
and the native chunk codecs of `csrc/blosc1.c`:

* Zarr directory stores, format 2 and format 3 (``zarr.json``): C-order chunks, ``compressor`` null / zlib / gzip / lz4 / blosc (every
  Blosc-1 codec and shuffle, decoded natively by ``csrc/blosc1.c``) / zstd, ``_ARRAY_DIMENSIONS``
  attributes, CF time decoding (``units`` + ``calendar``; non-standard calendars go to
  ``cfcalendar``), ``scale_factor`` / ``add_offset`` / ``_FillValue``; time-major stores and, with ``device=`` set, time-last ones —
  ``(latitude, longitude, time)``, the reference's converter's own order, written here by ``dataset_to_zarr(layout="time-last")`` —,
  whose chunks one kernel transposes into the time-major cube (``hip.place_box_tlast``); format-2 ``filters``: the byte shuffle and
  numcodecs' element filters (``fixedscaleoffset``, ``delta``, ``quantize``, ``bitround``, ``astype``), undone on the host by
  ``unfilter_elements`` and, with ``device=`` set, in HBM on the stored elements (``hip.delta_decode``, ``hip.fso_decode``);
* netCDF-4 / HDF5 files through the built-in reader ``hdf5.py`` (chunked + shuffle + deflate variables,
  dimension scales, either group style; no netCDF4 / h5py needed);
* ``.npz`` bundles with ``data``, ``time``, ``latitude``, ``longitude``;
* NetCDF classic files (CDF-1 / CDF-2): with ``device=`` set, the header is read by ``netcdf3.py`` and the time steps of a
  short / int / float / double variable go from the file to HBM as stored — ``pread`` into page-locked slabs, big-endian
  bytes over PCIe, swapped and placed by one kernel (``hip.place_box_swapped``), CF mask and unpack in HBM, ``keep_packed``,
  windows and several files as on the Zarr route (``_Nc3Source.to_device``); on the host, and for whatever that route
  declines (byte / char variables, arrays that are not time-leading, CDF-5), through ``scipy.io.netcdf_file``;
* GRIB files (editions 1 and 2, regular latitude / longitude grids, simple packing and edition 2's complex and CCSDS packing; ``engine="cfgrib"`` or none): ``grib.py`` indexes
  the messages from their section headers; with ``device=`` set the packed bits go from the file to HBM as stored and one kernel
  (``hip.grib_unpack``; for complex packing ``hip.grib_unpack_complex``, for CCSDS packing ``hip.grib_unpack_ccsds``) extracts, scales and places them (``_GribSource.to_device``), on the host ``grib.GribFile.read`` decodes
  them in numpy; what ``grib.py`` refuses raises with its reason.

On the host route chunks are decoded on host threads into one time-major host buffer, which
``Dataset.to_device()`` then uploads in a single copy.
"""
from __future__ import annotations

import gzip
import json
import os
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import Optional

import numpy as np
import pandas as pd

from .cfcalendar import STANDARD_CALENDARS, CFTimeIndex, decode_cf_time
from .dataarray import DataArray
from .dataset import Dataset, Grid

_ZARR_MARKERS = ("zarr.json", ".zmetadata", ".zgroup", ".zarray")
_NON_ZARR_SUFFIXES = (".nc", ".nc4", ".netcdf", ".cdf", ".h5", ".hdf5", ".grib", ".grb", ".grib2", ".tif", ".tiff")


def _looks_like_zarr(path, storage_options=None) -> bool:
    """`dataset.py:589-617`, local paths only."""
    if not isinstance(path, str):
        return False
    lowered = path.lower().rstrip("/")
    if ".zarr" in lowered:
        return True
    if lowered.endswith(_NON_ZARR_SUFFIXES):
        return False
    return os.path.isdir(path) and any(os.path.exists(os.path.join(path, m)) for m in _ZARR_MARKERS)


# --------------------------------------------------------------------------------------
# Zarr (formats 2 and 3)
# --------------------------------------------------------------------------------------
def _decompress(buf: bytes, comp, nbytes: Optional[int] = None):
    """Decoded bytes of one chunk.  ``nbytes`` = decoded size when known (needed for zstd frames)."""
    if comp is None:
        return buf
    cid = comp.get("id")
    if cid == "zlib":
        return zlib.decompress(buf)
    if cid == "gzip":
        return gzip.decompress(buf)
    if cid == "blosc":
        from . import codec
        return codec.blosc_decode(buf)               # native Blosc-1 decoder (csrc/blosc1.c), GIL released
    if cid == "zstd":
        from . import codec
        if nbytes is None:
            raise ValueError("zstd chunks need the decoded size")
        return codec.zstd_decode(buf, nbytes)
    if cid == "lz4":
        from . import codec
        if nbytes is None:
            raise ValueError("lz4 chunks need the decoded size")
        return codec.lz4_decode(buf, nbytes)
    raise ValueError(f"unsupported Zarr compressor {cid!r}")


_V3_DTYPES = {"bool": "|b1", "int8": "|i1", "int16": "<i2", "int32": "<i4", "int64": "<i8", "uint8": "|u1", "uint16": "<u2",
              "uint32": "<u4", "uint64": "<u8", "float16": "<f2", "float32": "<f4", "float64": "<f8"}


def is_zarr_array(path: str) -> bool:
    if os.path.exists(os.path.join(path, ".zarray")):
        return True
    zj = os.path.join(path, "zarr.json")
    if os.path.exists(zj):
        with open(zj) as f:
            return json.load(f).get("node_type") == "array"
    return False


_ELEM_FILTER_IDS = ("fixedscaleoffset", "delta", "quantize", "bitround", "astype")


def _parse_elem_filters(filters, array_dtype):
    """The ``filters`` of a format-2 array -> (element filters, byte shuffles), both in write order.  An element filter is
    ``{"id", "dtype", "astype"}`` (numpy dtypes: what the filter decodes to and what it stores) plus ``scale`` / ``offset`` for
    ``fixedscaleoffset``; the configs are numcodecs' (FixedScaleOffset, Delta, Quantize, BitRound, AsType), restated from its documentation.  ``bitround`` decodes to its input: it is
    checked and dropped.  Refused, by name: an unknown id, a chain whose types do not connect, a big-endian type inside a chain, an
    element size other than 1, 2, 4 or 8 bytes, ``delta`` on floating-point data, and a byte shuffle that is not the last step before
    the compressor."""
    elem, shuffles = [], []
    cur = np.dtype(array_dtype)
    for k, flt in enumerate(filters):
        fid = flt.get("id")
        if fid == "shuffle":
            shuffles.append(flt)
            continue
        if fid not in _ELEM_FILTER_IDS:
            raise ValueError(f"Zarr filter {fid!r} is not supported (the byte shuffle and the element filters "
                             f"{', '.join(_ELEM_FILTER_IDS)} are)")
        if shuffles:
            raise ValueError(f"Zarr filter {fid!r} follows a byte shuffle: element filters are read before the shuffle only")
        if fid == "bitround":
            if cur.kind != "f":
                raise ValueError(f"Zarr filter 'bitround' on {cur.name} data: it rounds floating-point mantissas only")
            continue
        if fid == "astype":
            dec, enc = flt.get("decode_dtype"), flt.get("encode_dtype")
        else:
            dec = flt.get("dtype")
            enc = flt.get("astype") or dec
        if dec is None or enc is None:
            raise ValueError(f"Zarr filter {fid!r} does not name its types ({'decode_dtype / encode_dtype' if fid == 'astype' else 'dtype'})")
        dec, enc = np.dtype(dec), np.dtype(enc)
        for dt in (cur, dec, enc):
            if not dt.isnative:
                raise ValueError(f"Zarr filter {fid!r}: big-endian type {dt.str} inside a filter chain is not supported")
            if dt.kind not in "iuf" or dt.itemsize not in (1, 2, 4, 8):
                raise ValueError(f"Zarr filter {fid!r}: type {dt.str} is not supported (integers and floats of 1, 2, 4 or 8 bytes are)")
        if dec != cur:
            what = "the array's dtype" if not elem else f"astype of filter {k - 1} ({elem[-1]['id']!r})"
            raise ValueError(f"Zarr filter {fid!r} (filter {k}) decodes to {dec.str}, but {what} is {cur.str}: the chain's types do not connect")
        if fid == "delta" and (dec.kind == "f" or enc.kind == "f"):
            # (refused since before the element filters were read: a float running sum is rounded at every step, so the values
            # depend on the order of the additions, and one order is all a reader could offer)
            raise ValueError(f"Zarr filter 'delta' on floating-point data ({dec.str}) is not supported: integer differences are read "
                             "(a fixedscaleoffset in front of it makes them)")
        e = {"id": fid, "dtype": dec, "astype": enc}
        if fid == "fixedscaleoffset":
            if flt.get("scale") is None or flt.get("offset") is None or float(flt["scale"]) == 0.0:
                raise ValueError("Zarr filter 'fixedscaleoffset' needs an offset and a scale other than 0")
            e["scale"], e["offset"] = float(flt["scale"]), float(flt["offset"])
        elif fid == "quantize":
            e["digits"] = int(flt.get("digits", 0))
        elem.append(e)
        cur = enc
    return elem, shuffles


def unfilter_elements(enc, elem_filters):
    """The flattened C-order elements of one decoded chunk (the last filter's ``astype``) -> the array's values: every element
    filter undone in reverse write order, by numcodecs' decode definitions.  ``fixedscaleoffset``: ``enc / scale + offset``, in
    float64 for stored integers (numpy's true division of an integer array) and in the stored float type otherwise, rounded once
    to ``dtype``; ``delta``: a running sum in ``dtype`` (integers wrap); ``quantize`` / ``astype``: a conversion."""
    x = np.asarray(enc).reshape(-1)
    for f in reversed(elem_filters):
        if f["id"] == "fixedscaleoffset":
            w = np.float64 if x.dtype.kind in "iu" else x.dtype.type
            y = x.astype(w) / w(f["scale"])
            y += w(f["offset"])
            x = y.astype(f["dtype"], copy=False)
        elif f["id"] == "delta":
            x = np.cumsum(x, dtype=f["dtype"])
        else:
            x = x.astype(f["dtype"], copy=False)
    return x


def filter_elements(values, elem_filters):
    """`unfilter_elements` the other way, by numcodecs' encode definitions: the flattened C-order values of one chunk -> what the
    compressor is given.  ``fixedscaleoffset``: ``around((x - offset) * scale)``; ``delta``: differences with the first element kept;
    ``quantize``: ``around(x, digits)`` scaled by the power of two that keeps ``digits`` decimal digits."""
    x = np.asarray(values).reshape(-1)
    for f in elem_filters:
        if f["id"] == "fixedscaleoffset":
            x = np.around((x - f["offset"]) * f["scale"]).astype(f["astype"])
        elif f["id"] == "delta":
            x = x.astype(f["dtype"], copy=False)             # differences in ``dtype`` (integers wrap), stored as ``astype``
            d = np.empty(x.shape, dtype=f["astype"])
            d[:1] = x[:1]
            d[1:] = x[1:] - x[:-1]
            x = d
        elif f["id"] == "quantize":
            exp = np.log10(10.0 ** -int(f["digits"]))
            exp = int(np.floor(exp)) if exp < 0 else int(np.ceil(exp))
            scale = 2.0 ** int(np.ceil(np.log2(10.0 ** -exp)))
            x = (np.around(scale * x.astype(f["dtype"], copy=False)) / scale).astype(f["astype"])
        else:
            x = x.astype(f["astype"], copy=False)
    return x


class ZarrArray:
    """One array of a Zarr directory store, format 2 (``.zarray`` / ``.zattrs``, chunk files ``i.j.k``)
    or format 3 (``zarr.json``, chunk files ``c/i/j/k``, codec pipeline) — what zarr-python 2 and 3
    write by default.  Both reduce to: a chunk file name, a chain of bytes -> bytes decoders, a dtype — and, for format-2 arrays
    written with numcodecs element filters, ``elem_filters`` (`_parse_elem_filters`) that turn the decoded elements of
    ``stored_dtype`` into values of ``dtype``.

    Format 3 is implemented from the specification (bytes / gzip / zstd / blosc / crc32c codecs, default
    and v2 chunk-key encodings, ``dimension_names``, ``sharding_indexed`` shards); no zarr-python 3 is available
    in this image to cross-check against."""

    def __init__(self, path: str):
        self.path = path
        self.elem_filters = []                                          # element filters, in write order (format 2 only)
        if os.path.exists(os.path.join(path, ".zarray")):
            self._init_v2()
        elif os.path.exists(os.path.join(path, "zarr.json")):
            self._init_v3()
        else:
            raise FileNotFoundError(f"{path} is not a Zarr array (no .zarray / zarr.json)")
        self.disk_dtype = self.dtype                                    # as stored (may be big-endian)
        self.dtype = self.dtype.newbyteorder("=") if not self.dtype.isnative else self.dtype
        # what a decoded chunk holds: the array's type, or what the element filters (`_parse_elem_filters`) left for the compressor
        self.stored_dtype = self.elem_filters[-1]["astype"] if self.elem_filters else self.dtype
        self.chunk_nbytes = int(np.prod(self.chunks)) * self.stored_dtype.itemsize if self.shape else self.stored_dtype.itemsize

    # ---- format 2 ----
    def _init_v2(self):
        with open(os.path.join(self.path, ".zarray")) as f:
            self.meta = json.load(f)
        if self.meta.get("zarr_format") != 2:
            raise ValueError("a .zarray file must declare zarr_format 2")
        if self.meta.get("order", "C") != "C":
            raise ValueError("only C-order Zarr chunks are supported")
        self.filters = list(self.meta.get("filters") or [])
        self.format = 2
        self.shard_shape = None
        self.shape = tuple(self.meta["shape"])
        self.chunks = tuple(self.meta["chunks"])
        self.dtype = np.dtype(self.meta["dtype"])
        self.sep = self.meta.get("dimension_separator", ".")
        self.key_prefix = ""
        comp = self.meta.get("compressor")
        self.codecs = [] if comp is None else [dict(comp)]             # bytes -> bytes decoders, in decode order
        # numcodecs filters run before the compressor on write, so they are undone after it on read: the byte shuffle with the
        # bytes -> bytes decoders, the element filters (in ``elem_filters``, write order) on the decoded elements after them
        self.elem_filters, shuffles = _parse_elem_filters(self.filters, self.dtype)
        for flt in reversed(shuffles):
            self.codecs.append({"id": "unshuffle", "elementsize": int(flt.get("elementsize", 4))})
        self.fill_value = self.meta.get("fill_value")
        self.attrs = {}
        ap = os.path.join(self.path, ".zattrs")
        if os.path.exists(ap):
            with open(ap) as f:
                self.attrs = json.load(f)
        self._dims = self.attrs.get("_ARRAY_DIMENSIONS")

    # ---- format 3 ----
    def _init_v3(self):
        with open(os.path.join(self.path, "zarr.json")) as f:
            self.meta = m = json.load(f)
        if m.get("zarr_format") != 3 or m.get("node_type") != "array":
            raise ValueError(f"{self.path}/zarr.json is not a format-3 array node")
        self.format = 3
        self.shape = tuple(m["shape"])
        grid = m.get("chunk_grid", {})
        if grid.get("name") != "regular":
            raise ValueError(f"unsupported chunk grid {grid.get('name')!r}")
        self.chunks = tuple(grid["configuration"]["chunk_shape"])
        dt = m["data_type"]
        if not isinstance(dt, str) or dt not in _V3_DTYPES:
            raise ValueError(f"unsupported Zarr v3 data_type {dt!r}")
        self.dtype = np.dtype(_V3_DTYPES[dt])
        enc = m.get("chunk_key_encoding", {"name": "default"})
        conf = enc.get("configuration", {})
        if enc.get("name") == "default":
            self.sep, self.key_prefix = conf.get("separator", "/"), "c"
        elif enc.get("name") == "v2":
            self.sep, self.key_prefix = conf.get("separator", "."), ""
        else:
            raise ValueError(f"unsupported chunk key encoding {enc.get('name')!r}")
        codecs = m.get("codecs", [])
        self.shard_shape = None
        if len(codecs) == 1 and codecs[0].get("name") == "sharding_indexed":
            # a chunk file is a SHARD: inner chunks back to back plus an index of (offset, nbytes) uint64 pairs,
            # one per inner chunk in C order, at the end (default) or the start of the file
            cf = codecs[0].get("configuration", {}) or {}
            if "chunk_shape" not in cf:
                raise ValueError("sharding_indexed without an inner chunk_shape")
            self.shard_shape, self.chunks = self.chunks, tuple(cf["chunk_shape"])
            if any(s_ % c_ for s_, c_ in zip(self.shard_shape, self.chunks)):
                raise ValueError("shard shape must be a multiple of the inner chunk shape")
            idx_names = [c.get("name") for c in cf.get("index_codecs", [{"name": "bytes"}, {"name": "crc32c"}])]
            if idx_names not in (["bytes"], ["bytes", "crc32c"]):
                raise ValueError(f"unsupported shard index codecs {idx_names}")
            self.shard_index_crc = "crc32c" in idx_names
            self.shard_index_at_end = cf.get("index_location", "end") == "end"
            self._shard_index_cache = {}
            codecs = cf.get("codecs", [])
        elif any(c.get("name") == "sharding_indexed" for c in codecs):
            raise ValueError("sharding_indexed must be the only codec of the array")
        self.codecs = []
        seen_bytes = False
        for c in codecs:
            name, cf = c.get("name"), c.get("configuration", {}) or {}
            if name == "bytes":
                if cf.get("endian", "little") != "little" and self.dtype.itemsize > 1:
                    self.dtype = self.dtype.newbyteorder(">")
                seen_bytes = True
            elif name == "transpose":
                if list(cf.get("order", [])) != list(range(len(self.shape))):
                    raise ValueError("Zarr v3 transpose codecs other than the identity are not supported")
            elif name in ("gzip", "zstd", "blosc", "crc32c"):
                self.codecs.insert(0, dict(cf, id=name))                # decode order is the reverse of encode order
            elif name == "sharding_indexed":
                raise ValueError("nested sharding is not supported")
            else:
                raise ValueError(f"unsupported Zarr v3 codec {name!r}")
        if not seen_bytes:
            raise ValueError("Zarr v3 codec chain has no array -> bytes codec")
        self.fill_value = m.get("fill_value")
        self.attrs = dict(m.get("attributes", {}))
        self._dims = m.get("dimension_names")

    @property
    def dims(self):
        d = self._dims
        return tuple(d) if d and all(x is not None for x in d) else tuple(f"dim_{i}" for i in range(len(self.shape)))

    @property
    def native_kind(self):
        """'raw' / 'blosc' / 'zstd' / 'zlib' / 'gzip' when a chunk file is at most ONE codec the native
        batch decoder handles (the common case), else None."""
        if not self.disk_dtype.isnative or len(self.codecs) > 1:
            return None                                                 # (element filters do not count: they follow the decode)
        if not self.codecs:
            return "raw"
        cid = self.codecs[0].get("id")
        return cid if cid in ("blosc", "zstd", "zlib", "gzip", "lz4") else None

    @property
    def scatter_kind(self):
        """`native_kind`, or None when the array has element filters that are not undone in HBM (`_hbm_filter_plan`): what decides
        between the scatter routes of `array_to_device` and the host's `_chunk`."""
        return self.native_kind if not self.elem_filters or _hbm_filter_plan(self) is not None else None

    @property
    def blosc_only(self) -> bool:
        return self.native_kind == "blosc"

    def chunk_path(self, idx) -> str:
        if self.format == 2:
            key = self.sep.join(str(i) for i in idx) if idx else "0"
        else:
            key = self.sep.join([self.key_prefix] + [str(i) for i in idx]) if self.key_prefix else self.sep.join(str(i) for i in idx)
        return os.path.join(self.path, *key.split("/"))

    def _shard_index(self, path):
        """(offsets, nbytes) uint64 arrays of one shard file, C order over its inner chunks; None if absent."""
        hit = self._shard_index_cache.get(path)
        if hit is not None or path in self._shard_index_cache:
            return hit
        n = int(np.prod([s_ // c_ for s_, c_ in zip(self.shard_shape, self.chunks)]))
        nb = n * 16 + (4 if self.shard_index_crc else 0)
        idx = None
        if os.path.exists(path):
            with open(path, "rb") as f:
                if self.shard_index_at_end:
                    f.seek(-nb, os.SEEK_END)
                raw = f.read(nb)
            tab = np.frombuffer(raw[:n * 16], dtype="<u8").reshape(n, 2)
            idx = (tab[:, 0].copy(), tab[:, 1].copy())
        if len(self._shard_index_cache) > 4096:
            self._shard_index_cache.clear()
        self._shard_index_cache[path] = idx
        return idx

    def chunk_locator(self, idx, probe: bool = True):
        """(file, offset, nbytes) of chunk ``idx`` — nbytes -1 = the whole file — or None when it is absent.  ``probe=False``
        leaves the question whether an unsharded chunk's file exists to the reader (one system call less per chunk)."""
        if self.shard_shape is None:
            fn = self.chunk_path(idx)
            return (fn, 0, -1) if not probe or os.path.exists(fn) else None
        per = [s_ // c_ for s_, c_ in zip(self.shard_shape, self.chunks)]
        fn = self.chunk_path(tuple(i // p_ for i, p_ in zip(idx, per)))
        tab = self._shard_index(fn)
        if tab is None:
            return None
        k = int(np.ravel_multi_index(tuple(i % p_ for i, p_ in zip(idx, per)), per))
        off, nb = int(tab[0][k]), int(tab[1][k])
        if off == 0xFFFFFFFFFFFFFFFF and nb == 0xFFFFFFFFFFFFFFFF:
            return None
        return fn, off, nb

    def _fill(self):
        fv = self.fill_value
        if self.dtype.kind == "f":
            if fv in (None, "NaN"):
                return np.nan
            if fv in ("Infinity", "-Infinity"):
                return np.inf if fv == "Infinity" else -np.inf
        return 0 if fv is None else fv

    def decode(self, buf):
        """Chunk file bytes -> decoded bytes (ndarray or bytes) through the codec chain."""
        for c in self.codecs:
            if c["id"] == "crc32c":
                buf = bytes(buf)[:-4]                                   # 4-byte checksum trailer (not verified)
            elif c["id"] == "unshuffle":                                # numcodecs Shuffle: byte planes back to elements
                es = c["elementsize"]
                raw = np.frombuffer(buf, dtype=np.uint8)
                n = len(raw) // es
                buf = np.concatenate([raw[:n * es].reshape(es, n).T.reshape(-1), raw[n * es:]])
            else:
                buf = _decompress(buf, c, self.chunk_nbytes)
        return buf

    def _chunk(self, idx):
        loc = self.chunk_locator(idx)
        if loc is None:
            return np.full(self.chunks, self._fill(), dtype=self.dtype)
        with open(loc[0], "rb") as f:
            f.seek(loc[1])
            raw = self.decode(f.read() if loc[2] < 0 else f.read(loc[2]))
        if self.elem_filters:
            enc = np.frombuffer(raw, dtype=self.stored_dtype, count=int(np.prod(self.chunks)) if self.shape else 1)
            return unfilter_elements(enc, self.elem_filters).reshape(self.chunks)
        arr = np.frombuffer(raw, dtype=self.disk_dtype, count=int(np.prod(self.chunks)) if self.shape else 1).reshape(self.chunks)
        return arr if self.disk_dtype.isnative else arr.astype(self.dtype)

    def read(self, out: Optional[np.ndarray] = None, threads: int = 8) -> np.ndarray:
        if out is None:
            out = np.empty(self.shape, dtype=self.dtype)
        if not self.shape:
            out[...] = self._chunk(())
            return out
        grid = [range((s + c - 1) // c) for s, c in zip(self.shape, self.chunks)]
        idxs = list(np.ndindex(*[len(g) for g in grid]))

        def work(idx):
            blk = self._chunk(idx)
            sl_out, sl_blk = [], []
            for i, c, s in zip(idx, self.chunks, self.shape):
                lo, hi = i * c, min((i + 1) * c, s)
                sl_out.append(slice(lo, hi))
                sl_blk.append(slice(0, hi - lo))
            out[tuple(sl_out)] = blk[tuple(sl_blk)]

        if threads > 1 and len(idxs) > 1:
            with ThreadPoolExecutor(max_workers=threads) as ex:
                list(ex.map(work, idxs))
        else:
            for i in idxs:
                work(i)
        return out


# --------------------------------------------------------------------------------------
# host -> HBM streaming
# --------------------------------------------------------------------------------------
def _torch_dtype(np_dtype):
    import torch
    table = {"float32": torch.float32, "float64": torch.float64, "int8": torch.int8, "uint8": torch.uint8,
             "int16": torch.int16, "int32": torch.int32, "int64": torch.int64}
    name = np.dtype(np_dtype).name
    if name in ("uint32", "uint64"):
        raise ValueError(f"dtype {name} has no device representation on the streaming path: unsigned storage is streamed up to 16 bits "
                         "(uint8, uint16); wider unsigned integers go through the host route")
    if name not in table:
        raise ValueError(f"dtype {name} has no device representation on the streaming path")
    return table[name]


def _attr_unsigned(attrs):
    """The NetCDF User's Guide attribute ``_Unsigned``: True / False as written ("true" / "false" in any letter case), None: absent."""
    u = attrs.get("_Unsigned")
    if u is None:
        return None
    if isinstance(u, bytes):
        u = u.decode("ascii", "replace")
    if isinstance(u, np.ndarray) and u.size == 1:
        u = u.reshape(-1)[0]
    return str(u).strip().lower() == "true"


def _stored_unsigned(np_dtype, attrs) -> bool:
    """Whether the stored integers are unsigned: unsigned storage, or signed storage under ``_Unsigned = "true"`` (the same bits).
    ``_Unsigned = "false"`` on unsigned storage (signed values in an unsigned container) is refused: no route reads it."""
    np_dtype, u = np.dtype(np_dtype), _attr_unsigned(attrs)
    if np_dtype.kind == "u":
        if u is False:
            raise ValueError(f'_Unsigned = "false" on {np_dtype.name} storage is not supported')
        return True
    return np_dtype.kind == "i" and u is True


def _wire_dtype(np_dtype, attrs):
    """(dtype the stored bits travel and sit in HBM as, modulus).  torch holds no uint16 worth the name (no indexing, no
    arithmetic), so unsigned 16-bit values travel as the int16 of the same bits and ``modulus`` = 65536.0 puts the float32 values
    right in HBM (``x.remainder_(modulus)``: -1 -> 65535, exact in float32) — likewise int8 under ``_Unsigned`` (256.0).  None: the
    values are right as converted.  Wider unsigned storage is refused."""
    np_dtype = np.dtype(np_dtype)
    if np_dtype.kind not in "iu" or not _stored_unsigned(np_dtype, attrs):
        return np_dtype, None
    if np_dtype.itemsize > 2:
        raise ValueError(f"unsigned {8 * np_dtype.itemsize}-bit storage ({np_dtype.name}"
                         + (', _Unsigned = "true"' if np_dtype.kind == "i" else "") + ") has no device representation on the streaming path: "
                         "unsigned storage is streamed up to 16 bits; wider unsigned integers go through the host route")
    if np_dtype == np.dtype(np.uint8):
        return np_dtype, None
    return np.dtype(f"i{np_dtype.itemsize}"), float(1 << (8 * np_dtype.itemsize))


_PINNED_STAGE = {}      # (thread, nbytes rounded up) -> [pinned uint8 tensors]: page-locking is slow, so it is done once per process
_STAGED_DEVICES = set() # indices of the devices this process uploaded to through the staging buffers (`_pinned_stage`)


def _release_staging_at_exit():
    """Interpreter teardown: wait for every stream of the devices this process uploaded to (only those: with one rank per GPU a
    rank must not open a context on the other ranks' cards on its way out), then give the page-locked staging
    buffers back while the HIP runtime is still alive.  The ingest routes drain their own copy / work streams before they
    return, but the cached buffers outlived the runtime's teardown order: under `rocprofv3 --memory-copy-trace` the process
    ended with "completion callbacks were not delivered" for the last asynchronous uploads (round 2's timeline run)."""
    try:
        import torch
        if _PINNED_STAGE and torch.cuda.is_available() and torch.cuda.is_initialized():
            for d in sorted(_STAGED_DEVICES):
                torch.cuda.synchronize(d)
    except Exception:      # teardown must never raise
        pass
    _PINNED_STAGE.clear()


import atexit  # noqa: E402

if os.environ.get("AGGFLY_HIP_NO_EXIT_HOOK") != "1":
    atexit.register(_release_staging_at_exit)


def _pinned_stage(nbytes: int, count: int, device=None):
    """``count`` page-locked host buffers of >= nbytes, cached for the life of the process (the CLI's
    year loop and every later dataset reuse them).  Pinning costs ~0.1 s per GB, which is why a
    per-call pinned buffer measured slower than a pageable one; a cached one makes the H2D copy
    truly asynchronous, so slab i uploads at PCIe rate while slab i+1 decodes."""
    import torch
    if torch.cuda.is_available():
        idx = None if device is None else torch.device(device).index
        _STAGED_DEVICES.add(int(torch.cuda.current_device() if idx is None else idx))
    size = 1 << max(20, (int(nbytes) - 1).bit_length())
    # (per calling thread: two threads that read stores at the same time — a worker per GPU in one process — must not stage through the same buffers)
    import threading
    bufs = _PINNED_STAGE.setdefault((threading.get_ident(), size), [])
    while len(bufs) < count:
        bufs.append(torch.empty(size, dtype=torch.uint8, pin_memory=True))
    return bufs[:count]


def stream_to_device(T: int, spatial: tuple, np_dtype, read_slab, slab_steps: int, device="cuda", post=None, out_dtype=None, wire_dtype=None,
                     place=None, stage_step_bytes=None, slabs=None):
    """Fill a (T, *spatial) HBM tensor slab by slab through two cached page-locked staging buffers.

    ``read_slab(k0, k1, out)`` fills ``out[:k1-k0]`` with time steps [k0, k1) (a Zarr chunk
    decode on host threads).  The upload of slab i is queued on its own HIP stream while slab
    i+1 is decoded, and the host never holds a second full copy of the cube.  Measured on the
    MI355X box (16 host cores, `profiles/r01_ingest_bench.json`): native Blosc decode 66 GB/s,
    pageable H2D 56 GB/s.  ``wire_dtype`` (`_wire_dtype`): the dtype of the same size the bits are uploaded as where torch
    cannot hold ``np_dtype`` (uint16 as int16); ``read_slab`` still fills an array of ``np_dtype``.
    ``place(raw, dst, n)`` with ``stage_step_bytes`` (the NetCDF classic route, `_Nc3Source.to_device`): a slab is then
    ``stage_step_bytes`` raw bytes per step, as they lie in the file — ``read_slab`` fills a uint8 array —, uploaded as they are
    into one HBM staging buffer, and ``place`` (a kernel on the copy stream) writes the ``n`` steps of ``raw`` into ``dst`` =
    ``cube[k0:k1]``; ``post`` follows as usual.  One HBM buffer serves every slab: upload and kernel are ordered on the copy stream.
    ``slabs`` (with ``place``; the TIFF route, whose pages hold different numbers of steps): the slabs themselves, [(k0, k1, staged
    bytes)] in step order, in place of slabs of ``slab_steps`` steps of ``stage_step_bytes`` each."""
    import torch
    np_dtype = np.dtype(np_dtype)
    tdt = _torch_dtype(np_dtype if wire_dtype is None else wire_dtype)     # as stored (packed integers stay packed on the wire)
    cube = torch.empty((T,) + tuple(spatial), dtype=_torch_dtype(out_dtype) if out_dtype is not None else tdt, device=device)
    if T == 0:
        return cube
    slab_steps = max(1, min(slab_steps, T))
    row = int(np.prod(spatial)) * np_dtype.itemsize if place is None else int(stage_step_bytes)
    if slabs is None:
        slabs = [(k0, min(T, k0 + slab_steps), (min(T, k0 + slab_steps) - k0) * row) for k0 in range(0, T, slab_steps)]
        stage_bytes = slab_steps * row
    else:
        stage_bytes = max(max(nb for _, _, nb in slabs), 1)
    nstage = 2 if len(slabs) > 1 else 1
    if place is None:
        stage_t = [b[:slab_steps * row].view(tdt).reshape((slab_steps,) + tuple(spatial)) for b in _pinned_stage(slab_steps * row, nstage, device)]
        stage = [t.numpy().view(np_dtype) for t in stage_t]
    else:
        stage_t = [b[:stage_bytes] for b in _pinned_stage(stage_bytes, nstage, device)]
        stage = [t.numpy() for t in stage_t]
        raw_dev = torch.empty(stage_bytes, dtype=torch.uint8, device=device)
    copy_stream = torch.cuda.Stream(device=device)
    # the cube (and the staging tensors) come from the caching allocator on the CURRENT stream: a block freed there may
    # still be read by queued kernels (the previous HBM window's fused pass) — order the copies behind them
    copy_stream.wait_stream(torch.cuda.current_stream(device))
    done = [None, None]
    uploaded = [None, None]
    for i, (k0, k1, nb) in enumerate(slabs):
        b = i % nstage
        if done[b] is not None:
            done[b].synchronize()                       # staging buffer b is free again
        read_slab(k0, k1, stage[b])
        with torch.cuda.stream(copy_stream):
            dst = cube[k0:k1]
            if place is None:
                dst.copy_(stage_t[b][:k1 - k0], non_blocking=True)
            else:
                raw = raw_dev[:nb]
                raw.copy_(stage_t[b][:nb], non_blocking=True)
                place(raw, dst, k1 - k0)
            if post is not None:
                post(dst)                                # e.g. fill-value masking, applied in HBM
            ev = torch.cuda.Event()
            ev.record(copy_stream)
            done[b] = ev
    copy_stream.synchronize()
    torch.cuda.current_stream(device).wait_stream(copy_stream)
    return cube


def zarr_to_device(path: str, var: str, device="cuda", threads: int = 16, slab_bytes: int = 128 << 20, t_range=None, yx_box=None, keep_packed=False,
                   time_axis=0):
    """Decode a time-major Zarr array — or, ``time_axis=2``, a time-last one (`array_to_device`) — straight into HBM.  Returns (tensor, ZarrArray)."""
    return array_to_device(ZarrArray(os.path.join(path, var)), device, threads, slab_bytes, t_range, yx_box, keep_packed, time_axis)


def keep_packed_requested(keep_packed=False) -> bool:
    """``keep_packed=True`` of `dataset_from_path`, or AGGFLY_HIP_KEEP_PACKED=1 in the environment (the way in for the CLI)."""
    return bool(keep_packed) or os.environ.get("AGGFLY_HIP_KEEP_PACKED", "0") == "1"


def packing_of(za):
    """(scale_factor, add_offset, fill value, unsigned) under which a streamed array can stay packed in HBM — the arguments of
    `packed.PackedCube` —, or None: int16 or uint16 storage only, and a fill value — if any — that is a stored integer.
    ``unsigned``: uint16 storage, or int16 storage under ``_Unsigned = "true"`` (the same bits: both give the same packing); a
    fill value written in the signed type is then taken modulo 2^16 (-1 means 65535, as xarray reads it)."""
    dt = np.dtype(za.dtype)
    if dt not in (np.dtype(np.int16), np.dtype(np.uint16)):
        return None
    unsigned = _stored_unsigned(dt, za.attrs)
    fv = _attr_fill(za.attrs)
    if fv is not None and isinstance(fv, float) and np.isnan(fv):
        fv = None
    if fv is not None:
        if int(fv) != fv:
            return None
        fv = int(fv)
        if unsigned and dt.kind == "i" and -32768 <= fv < 0:
            fv += 65536
        if not ((0 <= fv <= 65535) if unsigned else (-32768 <= fv <= 32767)):
            return None
    sf, ao = za.attrs.get("scale_factor"), za.attrs.get("add_offset")
    return (None if sf is None else float(sf), None if ao is None else float(ao), fv, unsigned)


def packed_rules_of(packings):
    """Whether a dataset read from several stores stays packed: ``packings`` is what `packing_of` says of each store, in time order.
    -> the stores' unpack rules [(scale_factor, add_offset, fill value, unsigned)], one per store — equal neighbours are merged later, by
    `packed.PackedCube.concat`, so stores of ONE packing give one rule — or None: a store that cannot stay packed (float storage,
    a fill value that is no stored integer), or int16 beside uint16 storage (one plan reads one storage).  Then all take the float32 route."""
    packings = list(packings)
    if not packings or any(p is None for p in packings):
        return None
    if len({bool(p[3]) for p in packings}) != 1:
        return None
    return packings


def _cf_in_hbm(np_dtype, attrs):
    """How a streamed array of stored ``np_dtype`` (native byte order) under ``attrs`` becomes values in HBM: -> (post, need_post,
    out_np, wire).  ``post(dst)`` is the CF mask + unpack of one uploaded slab, ``need_post`` whether it has anything to do, ``out_np``
    the cube's dtype — CF decoding as on the host route (`_cf_mask_scale`): int8/int16 -> float32, wider integers -> float64 —
    and ``wire`` the dtype the stored bits travel as (`_wire_dtype`)."""
    np_dtype = np.dtype(np_dtype)
    sf, ao = attrs.get("scale_factor"), attrs.get("add_offset")
    packed = np_dtype.kind in "iu" or sf is not None or ao is not None
    if np_dtype.kind not in "fiu":
        raise ValueError(f"dtype {np_dtype} is not streamed")
    out_np = np_dtype if np_dtype.kind == "f" else np.dtype(np.float64 if np_dtype.itemsize > 2 else np.float32)
    wire, modulus = _wire_dtype(np_dtype, attrs)                    # uint16 (and int16 / int8 under _Unsigned) travel as signed bits
    _torch_dtype(wire)                                              # refuses what torch cannot hold (uint32, ...)
    fv = _attr_fill(attrs)
    has_fv = fv is not None and not (isinstance(fv, float) and np.isnan(fv))
    if has_fv and modulus is not None and np_dtype.kind == "i" and fv < 0:
        fv = fv + modulus                                   # a fill written in the signed type, read as the unsigned value (xarray)

    def post(dst):
        """CF mask + unpack in HBM, in the order and precision of the host route: the packed integers travel
        over PCIe as stored (half / quarter of the decoded bytes) and are unpacked at HBM speed."""
        if modulus is not None:
            dst.remainder_(modulus)                         # unsigned bits that came as signed: -1 -> 65535, in place and exact
        if has_fv:
            dst[dst == fv] = float("nan")                   # exact: the cast from the stored integers is exact
        if sf is not None:
            dst.mul_(sf)
        if ao is not None:
            dst.add_(ao)

    return post, has_fv or packed, out_np, wire


def _scatter_kind(za):
    """`ZarrArray.scatter_kind`; sources without element filters (`hdf5.ChunkSource`): their ``native_kind``."""
    return za.scatter_kind if hasattr(za, "scatter_kind") else za.native_kind


def _hbm_filter_plan(za):
    """How the element filters of ``za`` are undone in HBM: -> None (there are none, or they go through the host's `ZarrArray._chunk`),
    or (n_delta, conv) — ``n_delta`` running sums over each staged chunk in the stored integer type (`hip.delta_decode`), then, after
    the placement, ``conv``: None (the stored type is the array's), ("fso", scale, offset) or ("cast",), from the stored type to the array's float32 /
    float64 (`hip.fso_decode`; a cast from stored floats is torch's).  The chains taken: in write order one converting filter at most,
    first, then ``delta`` filters on its integers.  The host keeps ``delta`` with ``astype`` other than ``dtype``,
    several conversions, conversions to integers and 64-bit or 16-bit-float stored types under a conversion."""
    from . import hip
    chain = list(getattr(za, "elem_filters", ()))
    if not chain or za.native_kind is None:                      # (a byte shuffle in the chain, a compressor without a native kind)
        return None
    conv = None
    if chain[0]["id"] != "delta":
        f = chain.pop(0)
        if f["dtype"].name not in ("float32", "float64") or f["astype"].name not in hip.FSO_TYPE:
            return None
        conv = ("fso", f["scale"], f["offset"]) if f["id"] == "fixedscaleoffset" else ("cast",)
    for f in chain:
        if f["id"] != "delta" or f["dtype"].kind not in "iu" or f["astype"] != f["dtype"]:
            return None
    return len(chain), conv


def _slab_bytes(default: int) -> int:
    """The bytes of one staging slab: ``default``, or AGGFLY_HIP_SLAB_MB from the environment (a tuning knob; scripts/e2e_bench.py sweeps it)."""
    mb = os.environ.get("AGGFLY_HIP_SLAB_MB")
    return int(float(mb) * (1 << 20)) if mb else default


def array_to_device(za, device="cuda", threads: int = 16, slab_bytes: int = 128 << 20, t_range=None, yx_box=None, keep_packed=False,
                    time_axis=0):
    """Stream a chunked (time, y, x) array — a `ZarrArray` or an `hdf5.ChunkSource` — straight into HBM: each
    slab is a whole number of time chunks, decoded chunk-parallel by the native codec into page-locked memory
    and uploaded while the next slab decodes.  Returns (tensor, source).  ``keep_packed`` (int16 / uint16 storage, `packing_of`): the
    tensor stays int16 as stored (uint16: the int16 of the same bits) — the CF unpacking in HBM is skipped and left to the kernels that read a `packed.PackedCube`.
    ``time_axis=2``: the array is (y, x, time) — what the reference's converter writes — and a codec the native decoder handles:
    the tensor comes back TIME-MAJOR, (time, y, x), through `_stream_chunks_scatter` (each chunk transposed into the cube in HBM);
    ``t_range`` counts steps of the last axis and ``yx_box`` cells of the first two.  A codec chain without a native kind ignores
    ``time_axis``: the array streams as stored.  Element filters (`ZarrArray.elem_filters`): the chains `_hbm_filter_plan` takes always
    go through `_stream_chunks_scatter`, which un-filters the stored elements in HBM; the others count as a codec chain without a
    native kind (`ZarrArray.scatter_kind`) and are un-filtered by `ZarrArray._chunk`."""
    if len(za.shape) != 3:
        raise ValueError("zarr_to_device expects a (time, y, x) array")
    slab_bytes = _slab_bytes(slab_bytes)
    post, need_post, out_np, wire = _cf_in_hbm(za.dtype, za.attrs)
    kind = _scatter_kind(za)                                       # (None also for element filters that the host undoes)
    filtered = bool(getattr(za, "elem_filters", ()))
    if time_axis == 2 and kind is not None:
        if keep_packed and packing_of(za) is not None:
            need_post, out_np = False, wire
        return _stream_chunks_scatter(za, device, threads, slab_bytes, post if need_post else None, out_np, t_range, yx_box, time_axis=2), za
    T, ny, nx = za.shape
    tc = za.chunks[0]
    grid_yx = [(iy, ix) for iy in range((ny + za.chunks[1] - 1) // za.chunks[1]) for ix in range((nx + za.chunks[2] - 1) // za.chunks[2])]
    # a slab is a whole number of time chunks: ~slab_bytes, but never fewer chunks than decode threads
    slab = max(tc * -(-threads // len(grid_yx)), (slab_bytes // max(ny * nx * za.dtype.itemsize, 1)) // tc * tc)
    slab = max(tc, min(slab, ((1 << 30) // max(tc * ny * nx * za.dtype.itemsize, 1)) * tc))      # <= 1 GiB of staging per buffer

    pool = ThreadPoolExecutor(max_workers=threads) if threads > 1 else None

    whole_rows = za.chunks[1] == ny and za.chunks[2] == nx

    def read_blosc_slab(k0, k1, out):
        """Time-contiguous store (every chunk spans the whole grid): each chunk (raw / Blosc / zstd / zlib) decodes straight
        into its rows of the staging slab, all chunks of the slab on one OpenMP team — no per-chunk
        temporary, no Python between chunks."""
        from . import codec
        its = list(range(k0 // tc, (k1 + tc - 1) // tc))
        paths, outs, spans, tails = [], [], [], []
        for it in its:
            t0, t1 = it * tc, min((it + 1) * tc, T)
            paths.append(za.chunk_locator((it, 0, 0)))
            spans.append((t0, t1))
            if t1 - t0 == tc:
                outs.append(out[t0 - k0:t1 - k0])
                tails.append(None)
            else:                                   # the last, padded chunk: decode beside, copy the real steps
                tmp = np.empty((tc, ny, nx), dtype=za.dtype)
                outs.append(tmp)
                tails.append(tmp)
        res = codec.decode_ranges(za.native_kind, paths, outs, threads=threads)
        for (t0, t1), r, tmp in zip(spans, res, tails):
            if r == -100:                           # absent chunk = fill value
                out[t0 - k0:t1 - k0] = za._fill()
            elif tmp is not None:
                out[t0 - k0:t1 - k0] = tmp[:t1 - t0]

    def read(k0, k1, out):
        if whole_rows and kind is not None and not filtered and out.flags.c_contiguous:
            return read_blosc_slab(k0, k1, out)
        jobs = [(it, iy, ix) for it in range(k0 // tc, (k1 + tc - 1) // tc) for (iy, ix) in grid_yx]

        def work(j):
            it, iy, ix = j
            blk = za._chunk((it, iy, ix))
            t0, t1 = it * tc, min((it + 1) * tc, T)
            y0, y1 = iy * za.chunks[1], min((iy + 1) * za.chunks[1], ny)
            x0, x1 = ix * za.chunks[2], min((ix + 1) * za.chunks[2], nx)
            out[t0 - k0:t1 - k0, y0:y1, x0:x1] = blk[:t1 - t0, :y1 - y0, :x1 - x0]

        if pool is not None and len(jobs) > 1:
            list(pool.map(work, jobs))
        else:
            for j in jobs:
                work(j)

    if keep_packed and packing_of(za) is not None:
        need_post, out_np = False, wire
    if t_range is not None and tuple(t_range) == (0, T):
        t_range = None
    if yx_box is not None and tuple(yx_box) == (0, ny, 0, nx):
        yx_box = None
    try:
        if t_range is not None or yx_box is not None:
            if kind is None:
                raise ValueError("a time / space window on a codec chain goes through the host route")
            return _stream_chunks_scatter(za, device, threads, slab_bytes, post if need_post else None, out_np, t_range, yx_box), za
        if (not whole_rows or filtered) and kind is not None:     # (element filters are undone on the scatter route only)
            return _stream_chunks_scatter(za, device, threads, slab_bytes, post if need_post else None, out_np), za
        if (kind in ("blosc", "zstd") or _deflate_typesize(kind)) and _gpu_decodable(za, T * ny * nx * za.dtype.itemsize):
            # Blosc-LZ4 / Zstandard / deflate chunks cross PCIe compressed and are decoded in HBM: the scatter route, whatever the chunk grid
            return _stream_chunks_scatter(za, device, threads, slab_bytes, post if need_post else None, out_np), za
        return stream_to_device(T, (ny, nx), za.dtype, read, slab, device, post if need_post else None, out_np, wire), za
    finally:
        if pool is not None:
            pool.shutdown()


GPU_DECODE_AUTO_BYTES = 96 << 20                  # requests this large take the decode-in-HBM route (round 2: 256 MB) ...
GPU_DECODE_AUTO_BYTES_WHOLE_ROWS = 256 << 20      # ... also when every chunk holds whole time steps of the grid (round 2: 768 MB; see _gpu_decodable)
GPU_DECODE_AUTO_BYTES_ZSTD = 100 << 20            # Zstandard stores: requests this large (any chunk grid; profiles/zstd_ingest.txt)
# zlib / deflate chunks (netCDF-4, HDF5, Zarr v2 "zlib"): the smallest measured request from which the decode in HBM takes <= 0.9 x the
# host route's time on all three layouts of profiles/deflate_ingest.txt.  None: measured 64 MiB ... 820 MiB, there is no such size — ahead
# on 98 KB chunks at 256 / 512 MiB (0.85 / 0.57 x), 8-84 x behind on 2.4 MB and 9 MB chunks, whose few streams each keep one lane of the
# front end busy for 0.4-1.4 s — so the route is opt-in (AGGFLY_HIP_GPU_DECODE=1)
GPU_DECODE_AUTO_BYTES_DEFLATE = None
# Blosc-1 chunks beyond LZ4 + byte shuffle (`_BloscRoute`): the same rule, on the three layouts of scripts/blosc_ingest_bench.py.  None: not
# measured yet (profiles/blosc_flavours_ingest.txt), so both flavours are opt-in (AGGFLY_HIP_GPU_DECODE=1)
GPU_DECODE_AUTO_BYTES_BLOSC_BITSHUFFLE = None     # LZ4 / LZ4HC streams under the bit shuffle
GPU_DECODE_AUTO_BYTES_BLOSC_ZSTD = None           # Zstandard streams, any shuffle
# TIFF LZW segments (`_TiffSource`, `hip.lzw_decode`): the same rule, on the two LZW layouts of scripts/tiff_ingest_bench.py.  None: measured
# 64 MiB ... 820 MiB, there is no such size — 1.19-1.38 x the host team's minimum on strips of 8 rows, 1.20-2.64 x on 256 x 256 tiles (one
# wave walks a tile's 256 KiB code by code; profiles/tiff_ingest.txt) — so the route is opt-in (AGGFLY_HIP_GPU_DECODE=1)
GPU_DECODE_AUTO_BYTES_LZW = None


def _deflate_typesize(kind):
    """Element size of the byte unshuffle behind a deflate chunk kind — 1 for plain ``"zlib"``, n for ``("zlib", n)`` — else None."""
    if kind == "zlib":
        return 1
    if isinstance(kind, tuple) and len(kind) == 2 and kind[0] == "zlib":
        return int(kind[1])
    return None


def _blosc_auto_bytes(flavour, whole_rows: bool):
    """The auto threshold of a Blosc store by the flavour of its first chunk — (inner codec id, shuffle 0 / 1 / 2)."""
    if flavour[0] == 4:
        return GPU_DECODE_AUTO_BYTES_BLOSC_ZSTD
    if flavour[1] == 2:
        return GPU_DECODE_AUTO_BYTES_BLOSC_BITSHUFFLE
    return GPU_DECODE_AUTO_BYTES_WHOLE_ROWS if whole_rows else GPU_DECODE_AUTO_BYTES


def _gpu_decodable(za, request_bytes: int = 0) -> bool:
    """Whether a request of ``request_bytes`` decoded bytes on this array takes the decode-in-HBM route; the format is judged from
    the first present chunk's header, the size by ``AGGFLY_HIP_GPU_DECODE``: ``1`` always, ``0`` never, unset / ``auto``: from the
    flavour's threshold on — never while that threshold is None (the route is then opt-in).

    Blosc-1 chunks with LZ4 streams (lz4 / lz4hc), byte shuffle or none — what `afhip_lz4_decode_streams` takes (`_Lz4Route`): requests
    of `GPU_DECODE_AUTO_BYTES` decoded bytes or more — `GPU_DECODE_AUTO_BYTES_WHOLE_ROWS` for stores whose chunks hold whole time
    steps of the grid.  The host route is at its best on those (each chunk decodes straight into its rows of the slab; 40-53 GB/s),
    and round 2 kept them on it up to 768 MB; with round 4's equal batches and host-decoded tail the decode in HBM is ahead from
    ~220 MB on (0.34 GB: 8.3 against 8.8 ms, 0.49 GB: 9.9 against 11.4, smooth fields 8.1 against 9.9 / 10.9 against 13.1;
    `profiles/r04_ingest_batches.txt`); on other chunk grids (space-tiled 12 MB chunks) it is level at 50 MB and ahead from there
    on (74 MB: 4.2 against 5.2 ms, 99 MB: 5.5 against 7.6; round 2 measured 0.26 GB on its pipeline).  Measured on MI355X (`profiles/r02_gpu_decode_by_ratio*.json`,
    DESIGN.md §8) the chunks of a 0.9-3.4 GB store reach HBM at 48-85 GB/s this way against 32-53 GB/s with the decode on
    16 host threads; a small request is over before the decode kernel's ~2 ms (one wave walks one stream) are.

    The other Blosc-1 flavours the GPU takes (`_BloscRoute`; the flavour of the first chunk is kept in ``za._blosc_flavour``): LZ4 /
    LZ4HC under the bit shuffle from `GPU_DECODE_AUTO_BYTES_BLOSC_BITSHUFFLE` on, Zstandard streams with any shuffle from
    `GPU_DECODE_AUTO_BYTES_BLOSC_ZSTD` on, chunks below 1 GiB (a Zstandard batch's bound); blosclz, zlib and snappy inside Blosc
    stay on the host.  Both constants follow profiles/blosc_flavours_ingest.txt."""
    mode = os.environ.get("AGGFLY_HIP_GPU_DECODE", "auto")
    whole_rows = len(za.shape) == 3 and tuple(za.chunks[1:]) == tuple(za.shape[1:])
    # plain Zstandard frames (`hip.zstd_decode`): from `GPU_DECODE_AUTO_BYTES_ZSTD` on under auto, chunks below 1 GiB (a batch's bound)
    zstd = za.native_kind == "zstd"
    # zlib streams (`hip.inflate_decode`; HDF5 / netCDF-4 deflate with or without shuffle, Zarr v2 "zlib"): from
    # `GPU_DECODE_AUTO_BYTES_DEFLATE` on under auto — never while that is None —, chunks below 1 GiB; gzip members stay on the host
    deflate = _deflate_typesize(za.native_kind) is not None
    blosc = za.native_kind == "blosc"
    if blosc:
        # (the flavour is in the first chunk's header: under auto no file is opened for a request below every Blosc threshold)
        cands = [_blosc_auto_bytes(f, whole_rows) for f in ((1, 1), (1, 2), (4, 1))]
        auto_bytes = min([c for c in cands if c is not None], default=None)
    else:
        auto_bytes = GPU_DECODE_AUTO_BYTES_DEFLATE if deflate else GPU_DECODE_AUTO_BYTES_ZSTD
    if (mode == "0" or not (deflate or blosc or zstd) or (mode != "1" and (auto_bytes is None or request_bytes < auto_bytes))
            or ((zstd or deflate) and za.chunk_nbytes >= 1 << 30)):
        return False
    def flavour_allows():
        """Blosc: the threshold (and the Zstandard batch's 1 GiB bound) of the flavour the first chunk's header showed."""
        if not blosc:
            return True
        flavour = getattr(za, "_blosc_flavour", (1, 1))
        limit = _blosc_auto_bytes(flavour, whole_rows)
        return (mode == "1" or (limit is not None and request_bytes >= limit)) and not (flavour[0] == 4 and za.chunk_nbytes >= 1 << 30)

    hit = getattr(za, "_gpu_decodable", None)
    if hit is not None:
        return hit and flavour_allows()
    ok = False
    try:
        for idx in np.ndindex(*[-(-s_ // c_) for s_, c_ in zip(za.shape, za.chunks)]):
            loc = za.chunk_locator(tuple(int(i) for i in idx))
            if loc is None:
                continue
            with open(loc[0], "rb") as f:
                f.seek(loc[1])
                h = f.read(2 if deflate else 18 if zstd else 16)
            if deflate:
                ok = _zlib_header_taken(h)
            elif zstd:
                ok = _zstd_frame_taken(h, za.chunk_nbytes)
            elif len(h) == 16 and h[0] == 2:
                flags, ts = h[2], h[3]
                nbytes, blocksize = int.from_bytes(h[4:8], "little"), int.from_bytes(h[8:12], "little")
                inner = (flags >> 5) & 7
                ok = bool(flags & 0x02) or (inner in (1, 4) and blocksize > 0 and nbytes == za.chunk_nbytes
                                            and -(-nbytes // blocksize) <= 65535)      # (one launch unshuffles at most 65,535 blocks)
                za._blosc_geometry = (max(blocksize, 1), max(ts, 1))
                # (inner codec id, shuffle): picks the threshold and the route; a stored chunk of another codec keeps `_Lz4Route`
                za._blosc_flavour = (inner if inner in (1, 4) else 1, 1 if flags & 0x01 and ts > 1 else 2 if flags & 0x04 else 0)
            break
    except OSError:
        ok = False
    try:
        za._gpu_decodable = ok
    except AttributeError:
        pass
    return ok and flavour_allows()


def _zstd_frame_taken(h: bytes, nbytes: int) -> bool:
    """A Zstandard frame header (the first 18 bytes of a chunk) that `afcodec_zstd_plan` takes: no checksum, no dictionary,
    a Frame_Content_Size equal to the chunk's decoded size."""
    if len(h) < 6 or int.from_bytes(h[:4], "little") != 0xFD2FB528:
        return False
    fhd = h[4]
    fcs_flag, single, did_flag = fhd >> 6, (fhd >> 5) & 1, fhd & 3
    if fhd & 0x0C or did_flag:
        return False
    fcs_size = (1 if single else 0) if fcs_flag == 0 else (2, 4, 8)[fcs_flag - 1]
    pos = 5 + (0 if single else 1)
    if fcs_size == 0 or len(h) < pos + fcs_size:
        return False
    fcs = int.from_bytes(h[pos:pos + fcs_size], "little") + (256 if fcs_size == 2 else 0)
    return fcs == nbytes


def _zlib_header_taken(h: bytes) -> bool:
    """The two header bytes of a zlib stream (RFC 1950) that `afcodec_inflate_plan` takes: deflate, a window of at most 32 KiB, a
    valid check sum, no preset dictionary (a gzip member fails the first test)."""
    return len(h) >= 2 and (h[0] & 15) == 8 and (h[0] >> 4) <= 7 and ((h[0] << 8) | h[1]) % 31 == 0 and not (h[1] & 0x20)


class _ScatterJob:
    """What both routes of `_stream_chunks_scatter` share: the window, the chunks that touch it, the cube, and the
    placement of decoded chunks into it."""

    def __init__(self, za, device, out_dtype, t_range, yx_box, time_axis=0):
        """``time_axis``: 0 — the array is (time, y, x) —, or 2 — (y, x, time), the reference's converter's layout: ``idxs`` stay
        chunk indices in the store's own order, the cube is time-major either way and `place` transposes each chunk into it."""
        import torch
        if time_axis not in (0, 2):
            raise ValueError("time_axis must be 0 or 2")
        self.za, self.device, self.time_axis = za, device, time_axis
        tm = (lambda s: (s[2], s[0], s[1])) if time_axis == 2 else tuple      # the store's own order -> (time, y, x)
        T, ny, nx = tm(za.shape)
        self.tc, self.yc, self.xc = tm(za.chunks)
        self.wire = wire = _wire_dtype(za.dtype, za.attrs)[0]              # the stored bits as torch holds them (uint16: int16)
        self.tdt = _torch_dtype(wire)
        self.same_dtype = (out_dtype is None or np.dtype(out_dtype) == wire) and za.dtype.itemsize in (2, 4, 8)
        # element filters (`_hbm_filter_plan`): running sums over the staged chunks, then — with a conversion — the placement goes to a
        # buffer of the STORED type beside the cube, which `finish` converts into the cube
        filtered = bool(getattr(za, "elem_filters", ()))
        fplan = _hbm_filter_plan(za)
        if filtered and fplan is None:
            raise ValueError("these element filters are undone on the host")
        self.n_delta, self.conv = fplan if fplan else (0, None)
        self.sdt = sdt = np.dtype(getattr(za, "stored_dtype", za.dtype))
        if self.conv is not None:                                          # (an integer of the stored size stands for unsigned types)
            self.tdt = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[sdt.itemsize] if sdt.kind in "iu" else _torch_dtype(sdt)
            self.same_dtype = sdt.itemsize in (2, 4, 8)
        self.ka, self.kb = (0, T) if t_range is None else (max(0, int(t_range[0])), min(T, int(t_range[1])))   # time window [ka, kb)
        self.ya, self.yb, self.xa, self.xb = (0, ny, 0, nx) if yx_box is None else yx_box                    # spatial box
        self.cube = torch.empty((self.kb - self.ka, self.yb - self.ya, self.xb - self.xa),
                                dtype=_torch_dtype(out_dtype) if out_dtype is not None else self.tdt, device=device)
        self.dest = self.cube if self.conv is None else torch.empty(tuple(self.cube.shape), dtype=self.tdt, device=device)
        self.absent = []                                                   # boxes of absent chunks, filled after the conversion
        self._delta_scratch = {}                                           # stream -> tile-sum scratch of `undelta`
        self.cb = za.chunk_nbytes
        tc, yc, xc = self.tc, self.yc, self.xc
        its, iys, ixs = range(self.ka // tc, -(-self.kb // tc)), range(self.ya // yc, -(-self.yb // yc)), range(self.xa // xc, -(-self.xb // xc))
        if time_axis == 2:
            self.idxs = [(iy, ix, it) for iy in iys for ix in ixs for it in its]
        else:
            self.idxs = [(it, iy, ix) for it in its for iy in iys for ix in ixs]
        # a chunk of whole time steps of the window (full grid, same dtype) is one contiguous run of the cube — never a time-last one
        self.whole_steps = (time_axis == 0 and self.same_dtype and (self.ya, self.xa) == (0, 0)
                            and (yc, xc) == (self.yb, self.xb) == (ny, nx) and not filtered)
        self.step_bytes = ny * nx * sdt.itemsize

    def absent_value(self) -> float:
        """The array's fill value as the cube holds it: an unsigned one in a cube of the signed bits (a uint16 cube kept packed) is
        the signed integer of the same bits."""
        fill = self.za._fill()
        if not self.cube.dtype.is_floating_point and self.wire != self.za.dtype:
            return float(np.array(fill).astype(self.za.dtype).view(self.wire))
        return float(fill)

    def undelta(self, staged, n_chunks: int):
        """Queue (on the current stream) numcodecs Delta's decode over the ``n_chunks`` decoded chunks at the start of ``staged``: one
        running sum per ``delta`` filter over each flattened chunk, in place, before `place` — the sum runs over the chunk, not the cube."""
        if not self.n_delta or not n_chunks:
            return
        import torch
        from . import hip
        es = self.sdt.itemsize
        # one scratch per stream for the whole job (batches on one stream run in order; two streams never share one), grown if a
        # later batch holds more chunks
        key, need = torch.cuda.current_stream(self.device).cuda_stream, hip.delta_scratch_bytes(n_chunks, self.cb // es, es)
        scratch = self._delta_scratch.get(key)
        if scratch is None or scratch.numel() < need:
            scratch = self._delta_scratch[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        for _ in range(self.n_delta):
            hip.delta_decode(staged, n_chunks, self.cb // es, es, scratch)

    def finish(self):
        """Queue (on the current stream, after every `place`) what turns the stored elements into the array's values: the conversion
        from the stored-type buffer into the cube, then the fill value — in the decoded type — over the boxes of absent chunks."""
        if self.conv is None:
            return
        from . import hip
        if self.conv[0] == "fso":
            hip.fso_decode(self.dest, self.cube, self.cube.numel(), self.sdt.name, self.conv[1], self.conv[2])
        elif self.sdt.kind in "iu":                  # Quantize / AsType from integers: x / 1.0 + 0.0 in float64 is the cast
            hip.fso_decode(self.dest, self.cube, self.cube.numel(), self.sdt.name, 1.0, 0.0)
        else:                                        # from floats: the cast itself (it keeps -0.0, which x + 0.0 does not)
            self.cube.copy_(self.dest)
        for box in self.absent:
            self.cube[box].fill_(float(self.za._fill()))
        self.dest = None

    def inside(self, it) -> bool:
        """All time steps of chunk row ``it`` lie in the window."""
        return self.ka <= it * self.tc and (it + 1) * self.tc <= self.kb

    def place(self, batch, res, staged, skip_present=False):
        """Queue (on the current stream) the placement of a batch: decoded chunk i sits at ``staged[i * cb:]``; absent
        chunks (``res[i] == -100``) become the fill value.  ``skip_present``: the present chunks are in place already."""
        from . import hip
        tc, yc, xc, ka, kb, ya, yb, xa, xb, cb, cube = self.tc, self.yc, self.xc, self.ka, self.kb, self.ya, self.yb, self.xa, self.xb, self.cb, self.dest
        tlast = self.time_axis == 2
        for i, (idx, r) in enumerate(zip(batch, res)):
            if skip_present and r != -100:
                continue
            it, iy, ix = (idx[2], idx[0], idx[1]) if tlast else idx
            c0 = it * tc                            # first step of the chunk
            t0, t1 = max(c0, ka), min(c0 + tc, kb)  # the part of it inside the window
            y0, y1 = max(iy * yc, ya), min((iy + 1) * yc, yb)
            x0, x1 = max(ix * xc, xa), min((ix + 1) * xc, xb)
            dst = cube[t0 - ka:t1 - ka, y0 - ya:y1 - ya, x0 - xa:x1 - xa]
            if r == -100:                           # absent chunk = fill value (with a conversion: after it, in `finish`)
                if self.conv is not None:
                    self.absent.append((slice(t0 - ka, t1 - ka), slice(y0 - ya, y1 - ya), slice(x0 - xa, x1 - xa)))
                else:
                    dst.fill_(self.absent_value())
                continue
            if tlast:                               # a chunk [yc][xc][tc]: transposed into the cube by one kernel
                blk = staged[i * cb:(i + 1) * cb].view(self.tdt).view(yc, xc, tc)
                if self.same_dtype:
                    hip.place_box_tlast(blk, cube, (y0 - iy * yc, x0 - ix * xc, t0 - c0, y1 - y0, x1 - x0, t1 - t0), (t0 - ka, y0 - ya, x0 - xa))
                else:                               # packed integers read to float32: the cast happens in this (strided) copy
                    dst.copy_(blk[y0 - iy * yc:y1 - iy * yc, x0 - ix * xc:x1 - ix * xc, t0 - c0:t1 - c0].permute(2, 0, 1))
                continue
            blk = staged[i * cb:(i + 1) * cb].view(self.tdt).view(tc, yc, xc)
            if self.same_dtype:                     # one coalesced pass (torch's strided copy ran at 22 GB/s here)
                hip.place_box(blk, cube, (t0 - c0, y0 - iy * yc, x0 - ix * xc, t1 - t0, y1 - y0, x1 - x0), (t0 - ka, y0 - ya, x0 - xa))
            else:                                   # packed integers: the cast happens in this copy
                dst.copy_(blk[t0 - c0:t1 - c0, y0 - iy * yc:y1 - iy * yc, x0 - ix * xc:x1 - ix * xc])


class _IngestTrace:
    """``AGGFLY_HIP_INGEST_TRACE=1``: host phases of a read (ms) and, on the decode-in-HBM route, a HIP-event timeline of
    its batches.  Costs nothing when off."""

    def __init__(self):
        import time
        self.on = os.environ.get("AGGFLY_HIP_INGEST_TRACE") == "1"
        self.clock = time.perf_counter
        self.phase = {"wait": 0.0, "read": 0.0, "plan": 0.0, "enqueue": 0.0}
        self.batches, self.t0, self._mark = [], self.clock(), self.clock()

    def lap(self, name):
        now = self.clock()
        self.phase[name] += now - self._mark
        self._mark = now

    def skip(self):
        self._mark = self.clock()

    def drained(self):
        """The wait for the GPU at the end of a read (since the last `skip`)."""
        self.phase["drain"] = self.clock() - self._mark

    def report(self, origin_event, **head):
        if not self.on:
            return
        for e in self.batches:                       # ms since the first upload could have started
            print("ingest timeline: batch %2d  %4d chunks  host read done %7.2f | upload %7.2f .. %7.2f | kernels done %7.2f" % (
                e["batch"], e["chunks"], e["host_read_done_ms"], origin_event.elapsed_time(e["h2d0"]), origin_event.elapsed_time(e["h2d1"]),
                origin_event.elapsed_time(e["k1"])), flush=True)
        print("ingest trace:", {**head, **{k_: round(v * 1e3, 2) for k_, v in self.phase.items()}}, flush=True)


def _stream_chunks_scatter(za: "ZarrArray", device, threads: int, slab_bytes: int, post=None, out_dtype=None, t_range=None, yx_box=None,
                           time_axis=0):
    """Any chunk grid, any time / space window: batches of chunks reach HBM through page-locked staging and the GPU
    places every chunk into its (time, y, x) box of the cube (a strided device-to-device copy at HBM speed — the part a
    CPU is bad at: 472-byte row pieces).  Two routes: the chunks decoded by the host's OpenMP team
    (`_scatter_host_decode`), or — Blosc-LZ4, larger requests — uploaded compressed and decoded in HBM
    (`_scatter_gpu_decode`, `_gpu_decodable`).  ``time_axis=2``: a (y, x, time) array — both routes decode its chunks as they
    are and `_ScatterJob.place` transposes them into the same time-major cube."""
    job = _ScatterJob(za, device, out_dtype, t_range, yx_box, time_axis)
    if _gpu_decodable(za, len(job.idxs) * job.cb):
        try:
            return _scatter_gpu_decode(job, threads, post)
        except _NotForTheGpuRoute:
            # `_gpu_decodable` judged the store by its first chunk; a later one differs (another codec, bit shuffle, another
            # block size).  include/aggfly_codec.h's contract for such a chunk is "decode it on the host": the whole
            # request goes through the host route (the GPU route has drained its streams before raising, so nothing is
            # still writing the cube), and so do later requests on this array
            za._gpu_decodable = False
    return _scatter_host_decode(job, threads, slab_bytes, post)


class _NotForTheGpuRoute(Exception):
    """A chunk of the request cannot be decoded in HBM (raised by `_scatter_gpu_decode` after it has drained its streams)."""


def _scatter_host_decode(job: _ScatterJob, threads: int, slab_bytes: int, post):
    """The host only ever decodes chunks CONTIGUOUSLY — a batch of chunk files is read and decoded by one OpenMP team
    back to back into a cached page-locked buffer — and the batch goes to HBM in one asynchronous copy, two buffers
    taking turns."""
    import torch
    from . import codec
    za, device, cb, idxs = job.za, job.device, job.cb, job.idxs
    # chunks per batch: ~slab_bytes, at least one per decode thread, but never more than 1 GiB of page-locked
    # staging per buffer (the reference's own converter writes ~256 MB chunks)
    per = max(1, min(max(threads, slab_bytes // cb), max(1, (1 << 30) // cb), 4096))
    if cb >= (64 << 20):
        per = 1          # big chunks decode block-parallel on the whole team: one per batch pipelines best with the upload
    nstage = 2 if len(idxs) > per else 1
    host = _pinned_stage(per * cb, nstage, device)
    dev = [torch.empty(per * cb, dtype=torch.uint8, device=device) for _ in range(nstage)]
    copy_stream = torch.cuda.Stream(device=device)
    # the cube (and the staging tensors) come from the caching allocator on the CURRENT stream: a block freed there may
    # still be read by queued kernels (the previous HBM window's fused pass) — order the copies behind them
    copy_stream.wait_stream(torch.cuda.current_stream(device))
    done = [None] * nstage
    trace = _IngestTrace()
    for b, lo in enumerate(range(0, len(idxs), per)):
        batch = idxs[lo:lo + per]
        k = b % nstage
        trace.skip()
        if done[k] is not None:
            done[k].synchronize()                       # both staging buffers of slot k are free again
        trace.lap("wait")
        hbuf = host[k][:len(batch) * cb].numpy()
        res = codec.decode_ranges(za.native_kind, [za.chunk_locator(i) for i in batch], [hbuf[i * cb:(i + 1) * cb] for i in range(len(batch))],
                                  threads=threads)
        trace.lap("read")
        with torch.cuda.stream(copy_stream):
            dev[k][:len(batch) * cb].copy_(host[k][:len(batch) * cb], non_blocking=True)
            job.undelta(dev[k], len(batch))
            job.place(batch, res, dev[k])
            done[k] = torch.cuda.Event()
            done[k].record(copy_stream)
        trace.lap("enqueue")
    with torch.cuda.stream(copy_stream):
        job.finish()
        if post is not None:
            post(job.cube)
    trace.skip()
    copy_stream.synchronize()
    trace.drained()
    trace.report(None, gpu_decode=False, batches=-(-len(idxs) // per), chunks_per_batch=per)
    torch.cuda.current_stream(device).wait_stream(copy_stream)
    return job.cube


def _decode_batches(n_chunks: int, cb: int, nblk: int, whole_steps: bool, max_per: int = 4096, target_bytes: int = 144 << 20,
                    max_bytes: int = 512 << 20):
    """How `_scatter_gpu_decode` cuts a request of ``n_chunks`` chunks (``cb`` decoded bytes, ``nblk`` Blosc blocks each):
    -> (cuts: batch boundaries over the chunks that cross PCIe compressed, per: chunks of the largest batch, n_tail: chunks at the
    request's end that the host threads decode)."""
    # One stream of a chunk is decoded by one wave, start to end (~2 ms for a 64 KiB byte plane), and a batch of ~60 chunks of this
    # shape (9 k streams) fills the card's wave slots once: smaller batches take as long as that one, larger ones scale.  Equal
    # batches of ~144 MB decoded (at most 16 of them; 512 MB at most each) measured best on 0.34 / 0.86 / 3.4 GB stores — 9.2 / 15.6 /
    # 48.8 ms against 11.4 / 17.1 / 51.3 for round 2's rule (a quarter of the request per batch, 128-512 MB, with a quarter-size first
    # and last batch): profiles/r04_ingest_batches.txt
    env_mb = os.environ.get("AGGFLY_HIP_GPU_DECODE_BATCH_MB")
    # The last chunks of the request are decoded by the HOST threads — idle once the files are read, while the compressed uploads
    # still queue — and go up decoded behind them: the decode kernels of the last compressed batch (~2.9 ms, a latency no batch size
    # shortens) then run under that upload instead of after everything else.  As many chunks as cross PCIe decoded in that time
    # (~128-160 MB), at most a fifth of the request.
    # (AGGFLY_HIP_GPU_DECODE_HOST_TAIL_MB: 128 measured best — 0.34 / 0.86 / 3.4 GB stores 9.3 / 15.6 / 48.5 -> 8.3 / 14.0 / 46.7 ms;
    # ..._MIN_MB: requests below it have no such tail — the route itself starts at 256 MB by default; tests set 0)
    tail_mb = int(os.environ.get("AGGFLY_HIP_GPU_DECODE_HOST_TAIL_MB", "128"))
    tail_min = int(os.environ.get("AGGFLY_HIP_GPU_DECODE_HOST_TAIL_MIN_MB", "256")) << 20
    tail_pct = int(os.environ.get("AGGFLY_HIP_GPU_DECODE_HOST_TAIL_MAX_PCT", "20"))
    n_tail = min(max((tail_mb << 20) // cb, 1 if tail_mb > 0 else 0), n_chunks * tail_pct // 100) if n_chunks * cb >= tail_min else 0
    # (chunks of whole time steps only — measured +10 % there; space-tiled chunks and the converter's whole-series tiles go through the placement kernel either
    # way and measured 3 % behind with a host-decoded tail: 51.1 against 53.0, 43.2 against 44.6 GB/s; ..._MIN_MB=0, the tests' setting, lifts this too)
    if not whole_steps and tail_min > 0:
        n_tail = 0
    n = n_chunks - n_tail                                 # chunks that cross PCIe compressed
    total = n * cb
    n_batches = min(16, max(1, -(-total // target_bytes)))
    batch_bytes = (int(env_mb) << 20) if env_mb else min(-(-total // n_batches), max_bytes)
    per = max(1, min(-(-batch_bytes // cb), 65535 // nblk, max_per, max(n, 1)))
    n_batches = max(1, -(-n // per))
    cuts = sorted(set(int(round(i * n / n_batches)) for i in range(n_batches + 1)))
    per = max([b - a for a, b in zip(cuts, cuts[1:])] or [1])
    env_cuts = os.environ.get("AGGFLY_HIP_GPU_DECODE_CUTS")      # experiment knob: batch ends as fractions of the request, e.g. "0.1,0.5,0.9"
    if env_cuts:
        cuts = sorted(set([0, n] + [min(n, max(0, int(round(float(f) * n)))) for f in env_cuts.split(",")]))
        per = max(b - a for a, b in zip(cuts, cuts[1:]))
    return cuts, per, n_tail


class _Lz4Route:
    """The codec half of the decode-in-HBM route for Blosc-1 chunks of LZ4 streams: the record lists of
    `codec.blosc_lz4_plan` (streams, shuffled blocks), `hip.lz4_decode_streams` + `hip.unshuffle_blocks`."""

    what = "LZ4 stream(s)"

    def __init__(self, job):
        bsz, self.tsz = getattr(job.za, "_blosc_geometry", (65536, 1))
        self.cb = job.cb
        self.nblk = max(1, -(-job.cb // bsz))
        self.max_per, self.target_bytes, self.max_bytes = 4096, 144 << 20, 512 << 20

    def size(self, per, nstage, device):
        import torch
        from . import codec
        cb, nblk = self.cb, self.nblk
        self.cmax = (int(codec.load().afcodec_blosc_bound(cb, 0)) + 63) // 64 * 64
        self.cap_streams = per * (nblk * self.tsz + cb // 65536 + 2)          # one stream per byte plane of a block; stored chunks in 64 KiB pieces
        self.cap_blocks = per * nblk
        self.rec_bytes = self.cap_streams * codec.LZ4_STREAM.itemsize + self.cap_blocks * codec.SHUFFLE_BLOCK.itemsize
        self.tmp_dev = [torch.empty(per * (cb + 16 * nblk + 16), dtype=torch.uint8, device=device) for _ in range(nstage)]

    def plan(self, k, hall, rec0, offs, sizes, present, out_offs):
        """Records of a batch into the page-locked slot behind its compressed bytes -> the byte ranges of the slot to upload."""
        from . import codec
        streams = hall[rec0:rec0 + self.cap_streams * codec.LZ4_STREAM.itemsize].view(codec.LZ4_STREAM)
        bl0 = rec0 + streams.nbytes
        blocks = hall[bl0:bl0 + self.cap_blocks * codec.SHUFFLE_BLOCK.itemsize].view(codec.SHUFFLE_BLOCK)
        try:
            n_st, n_bl, tmp_bytes, max_d, pres = codec.blosc_lz4_plan(hall, offs[:-1][present], sizes[present], out_offs,
                                                                        np.full(len(present), self.cb, dtype=np.int64), streams, blocks)
        except codec.PlanCapacityError:
            raise _NotForTheGpuRoute() from None
        if (pres == codec.E_UNSUPPORTED).any() or tmp_bytes > self.tmp_dev[k].numel() or n_st > self.cap_streams or n_bl > self.cap_blocks:
            # a chunk the GPU decoder does not take (aggfly_codec.h: "decode it on the host"), or one whose geometry differs
            # from the first chunk's, which sized the buffers: the request falls back to the host route
            raise _NotForTheGpuRoute()
        self.rec0, self.bl0, self.n_st, self.n_bl, self.max_d = rec0, bl0, n_st, n_bl, max_d
        self.max_bsize = int(blocks["bsize"][:n_bl].max()) if n_bl else 0
        ranges = [(0, rec0 + n_st * codec.LZ4_STREAM.itemsize)]                              # compressed bytes + stream records: one copy
        if n_bl:
            ranges.append((bl0, bl0 + n_bl * codec.SHUFFLE_BLOCK.itemsize))
        return pres, ranges

    def decode(self, k, comp, target, errors):
        from . import hip
        if self.n_st:
            hip.lz4_decode_streams(comp, comp[self.rec0:], self.n_st, self.max_d, self.tmp_dev[k], target, errors)
        if self.n_bl:
            hip.unshuffle_blocks(self.tmp_dev[k], target, comp[self.bl0:], self.n_bl, self.max_bsize)


class _BloscRoute:
    """The codec half of the decode-in-HBM route for the Blosc-1 flavours beyond `_Lz4Route`'s — Zstandard streams with any shuffle,
    LZ4 streams under the bit shuffle; it takes `_Lz4Route`'s chunks too, so a store may mix them —: the five record lists of
    `codec.blosc_plan`, then `hip.lz4_decode_streams`, `hip.zstd_decode` into the shuffle scratch (with a Zstandard scratch per slot,
    grown on the slot's stream when a batch needs more), `hip.unshuffle_blocks` and `hip.bitunshuffle_blocks`.  The lists are sized
    from the first chunk's header; a batch that needs more falls back to the host.  Zstandard batches decode at most 1 GiB."""

    what = "LZ4 stream(s) / Zstandard frame(s)"

    def __init__(self, job):
        self.bsz, self.tsz = getattr(job.za, "_blosc_geometry", (65536, 1))
        self.zstd = getattr(job.za, "_blosc_flavour", (1, 1))[0] == 4
        self.cb = job.cb
        self.nblk = max(1, -(-job.cb // self.bsz))
        if self.zstd:          # as `_ZstdRoute`: the passes are a thread or a wave per Zstandard block, latency-bound
            self.max_per = max(1, min(4096, (1 << 30) // job.cb))
            self.target_bytes = self.max_bytes = 1 << 30
        else:
            self.max_per, self.target_bytes, self.max_bytes = 4096, 144 << 20, 512 << 20

    def size(self, per, nstage, device):
        import torch
        from . import codec
        cb, nblk = self.cb, self.nblk
        a64 = lambda n: (n + 63) // 64 * 64
        self.cmax = a64(int(codec.load().afcodec_blosc_bound(cb, 0)))
        # one frame, or one stream per byte plane, per Blosc block; stored streams and chunks in 64 KiB pieces
        self.cap_streams = per * (nblk * (1 if self.zstd else self.tsz) + cb // 65536 + nblk + 2)
        self.cap_blocks = per * nblk                                          # each of the two unshuffle lists
        self.cap_frames = per * nblk if self.zstd else 1
        # libzstd writes 128 KiB blocks: 8x headroom and 4 per frame, more goes to the host (as `_ZstdRoute.size`)
        self.cap_zblocks = per * (cb // 16384 + 4 * nblk) if self.zstd else 1
        sizes = (self.cap_streams * codec.LZ4_STREAM.itemsize, self.cap_blocks * codec.SHUFFLE_BLOCK.itemsize,
                 self.cap_blocks * codec.SHUFFLE_BLOCK.itemsize, self.cap_frames * codec.ZSTD_FRAME.itemsize,
                 self.cap_zblocks * codec.ZSTD_BLOCK.itemsize)
        self.at = [0]
        for n in sizes:
            self.at.append(self.at[-1] + a64(n))
        self.rec_bytes = self.at[-1]
        self.device = device
        self.tmp_dev = [torch.empty(per * (cb + 16 * nblk + 16), dtype=torch.uint8, device=device) for _ in range(nstage)]
        self.scratch = [None] * nstage
        self.rounds = None

    def plan(self, k, hall, rec0, offs, sizes, present, out_offs):
        from . import codec
        dts = (codec.LZ4_STREAM, codec.SHUFFLE_BLOCK, codec.SHUFFLE_BLOCK, codec.ZSTD_FRAME, codec.ZSTD_BLOCK)
        caps = (self.cap_streams, self.cap_blocks, self.cap_blocks, self.cap_frames, self.cap_zblocks)
        self.lo = [rec0 + a for a in self.at[:5]]
        lists = [hall[lo:lo + cap * dt.itemsize].view(dt) for lo, cap, dt in zip(self.lo, caps, dts)]
        try:
            pl = codec.blosc_plan(hall, offs[:-1][present], sizes[present], out_offs, np.full(len(present), self.cb, dtype=np.int64), *lists)
        except codec.PlanCapacityError:
            raise _NotForTheGpuRoute() from None
        if (pl.results == codec.E_UNSUPPORTED).any() or pl.tmp_bytes > self.tmp_dev[k].numel() or pl.dec_bytes > 0x7fffffff:
            # a chunk the GPU decoders do not take (aggfly_codec.h: "decode it on the host"), or one whose geometry differs from
            # the first chunk's, which sized the buffers: the request falls back to the host route
            raise _NotForTheGpuRoute()
        self.plan_, self.rec0 = pl, rec0
        counts = (pl.n_streams, pl.n_shuf, pl.n_bits, pl.n_frames, pl.n_blocks)
        ranges = [(0, self.lo[0] + counts[0] * dts[0].itemsize)]                # compressed bytes + stream records: one copy
        ranges += [(lo, lo + n * dt.itemsize) for lo, n, dt in zip(self.lo[1:], counts[1:], dts[1:])]
        return pl.results, ranges

    def decode(self, k, comp, target, errors):
        import torch
        from . import hip
        pl, lo, tmp = self.plan_, self.lo, self.tmp_dev[k]
        if pl.n_streams:
            hip.lz4_decode_streams(comp, comp[lo[0]:], pl.n_streams, pl.max_dsize, tmp, target, errors)
        if pl.n_frames:
            need = hip.zstd_scratch_bytes(pl)
            if self.scratch[k] is None or self.scratch[k].numel() < need:
                self.scratch[k] = None
                self.scratch[k] = torch.empty(need, dtype=torch.uint8, device=self.device)
            if self.rounds is None and os.environ.get("AGGFLY_HIP_INGEST_TRACE") == "1":
                self.rounds = torch.zeros(1, dtype=torch.int32, device=self.device)
            hip.zstd_decode(comp, self.rec0, comp[lo[3]:], comp[lo[4]:], pl, self.scratch[k], tmp, errors, self.rounds)
        if pl.n_shuf:
            hip.unshuffle_blocks(tmp, target, comp[lo[1]:], pl.n_shuf, pl.max_shuf)
        if pl.n_bits:
            hip.bitunshuffle_blocks(tmp, target, comp[lo[2]:], pl.n_bits, pl.max_bits)


class _ZstdRoute:
    """The codec half of the decode-in-HBM route for plain Zstandard frames: the frame and block records of
    `codec.zstd_plan`, `hip.zstd_decode` with a scratch per slot (grown on the slot's stream when a batch needs more).
    Batches decode at most 1 GiB (the scratch's byte map is ~4 bytes per decoded byte)."""

    what = "Zstandard frame(s)"

    def __init__(self, job):
        self.cb = job.cb
        self.nblk = 1
        # large batches: every pass is a thread (or a wave) per block, latency-bound, and a batch of one 265 MB frame fills
        # only ~125 waves of the card (profiles/zstd_ingest.txt)
        self.max_per = max(1, min(4096, (1 << 30) // job.cb))
        self.target_bytes = self.max_bytes = 1 << 30

    def size(self, per, nstage, device):
        from . import codec
        cb = self.cb
        self.cmax = (int(codec.load().afcodec_zstd_bound(cb)) + 63) // 64 * 64
        self.cap_frames = per
        self.cap_blocks = per * (cb // 16384 + 4)          # libzstd writes 128 KiB blocks: 8x headroom, more goes to the host
        self.rec_bytes = (self.cap_frames * codec.ZSTD_FRAME.itemsize + 63) // 64 * 64 + self.cap_blocks * codec.ZSTD_BLOCK.itemsize
        self.device = device
        self.scratch = [None] * nstage
        self.rounds = None

    def plan(self, k, hall, rec0, offs, sizes, present, out_offs):
        from . import codec
        frames = hall[rec0:rec0 + self.cap_frames * codec.ZSTD_FRAME.itemsize].view(codec.ZSTD_FRAME)
        bl0 = rec0 + (frames.nbytes + 63) // 64 * 64
        blocks = hall[bl0:bl0 + self.cap_blocks * codec.ZSTD_BLOCK.itemsize].view(codec.ZSTD_BLOCK)
        try:
            pl = codec.zstd_plan(hall, offs[:-1][present], sizes[present], out_offs, np.full(len(present), self.cb, dtype=np.int64),
                                 frames, blocks)
        except codec.PlanCapacityError:
            raise _NotForTheGpuRoute() from None
        if (pl.results == codec.E_UNSUPPORTED).any():
            raise _NotForTheGpuRoute()             # a checksum, a dictionary, another frame: aggfly_codec.h's "decode it on the host"
        self.plan_, self.rec0, self.bl0 = pl, rec0, bl0
        return pl.results, [(0, rec0 + pl.n_frames * codec.ZSTD_FRAME.itemsize), (bl0, bl0 + pl.n_blocks * codec.ZSTD_BLOCK.itemsize)]

    def decode(self, k, comp, target, errors):
        import torch
        from . import hip
        need = hip.zstd_scratch_bytes(self.plan_)
        if self.scratch[k] is None or self.scratch[k].numel() < need:
            self.scratch[k] = None
            self.scratch[k] = torch.empty(need, dtype=torch.uint8, device=self.device)
        if self.rounds is None and os.environ.get("AGGFLY_HIP_INGEST_TRACE") == "1":
            self.rounds = torch.zeros(1, dtype=torch.int32, device=self.device)
        hip.zstd_decode(comp, self.rec0, comp[self.rec0:], comp[self.bl0:], self.plan_, self.scratch[k], target, errors, self.rounds)


class _DeflateRoute:
    """The codec half of the decode-in-HBM route for zlib streams (HDF5 / netCDF-4 deflate chunks, Zarr v2 "zlib"): one stream
    record per chunk and one shuffle record per shuffled chunk from `codec.inflate_plan`, `hip.inflate_decode` with a scratch per
    slot (grown on the slot's stream when a batch needs more).  Batches decode at most 256 MiB: the scratch holds ~9 bytes per
    decoded byte (literals, sequence records, the byte map), i.e. up to 2.3 GiB per staging slot and 9.2 GiB of HBM for a request of
    four batches and more.  A chunk larger than a batch is a batch of its own (6 slots): 9 bytes per byte of the chunk in each,
    54 GiB for chunks just below the 1 GiB the route takes."""

    what = "zlib stream(s)"
    rounds_key = "inflate_jump_rounds"

    def __init__(self, job):
        self.cb = job.cb
        self.tsz = _deflate_typesize(job.za.native_kind)
        self.nblk = 1
        # large batches: the front end walks a stream from its first bit to its last on one lane, so a batch takes as long as its
        # longest stream however many streams it holds — 36 ms for 98 KB, 400 ms for 2.4 MB (profiles/deflate_ingest.txt)
        self.max_per = max(1, min(4096, (256 << 20) // job.cb))
        self.target_bytes = self.max_bytes = 256 << 20

    def size(self, per, nstage, device):
        from . import codec
        cb = self.cb
        self.cmax = (cb + cb // 8 + 1024 + 63) // 64 * 64            # (deflate's worst case is stored blocks: 5 bytes per 64 KiB more)
        self.cap = per
        self.rec_bytes = (per * codec.INFLATE_STREAM.itemsize + 63) // 64 * 64 + per * codec.SHUFFLE_BLOCK.itemsize
        self.device = device
        self.scratch = [None] * nstage
        self.rounds = None

    def plan(self, k, hall, rec0, offs, sizes, present, out_offs):
        from . import codec
        streams = hall[rec0:rec0 + self.cap * codec.INFLATE_STREAM.itemsize].view(codec.INFLATE_STREAM)
        sh0 = rec0 + (streams.nbytes + 63) // 64 * 64
        shuf = hall[sh0:sh0 + self.cap * codec.SHUFFLE_BLOCK.itemsize].view(codec.SHUFFLE_BLOCK)
        try:
            pl = codec.inflate_plan(hall, offs[:-1][present], sizes[present], out_offs, np.full(len(present), self.cb, dtype=np.int64),
                                    streams, shuf, typesize=self.tsz)
        except codec.PlanCapacityError:
            raise _NotForTheGpuRoute() from None
        if (pl.results == codec.E_UNSUPPORTED).any():
            raise _NotForTheGpuRoute()             # a preset dictionary, a gzip member: aggfly_codec.h's "decode it on the host"
        self.plan_, self.rec0, self.sh0 = pl, rec0, sh0
        return pl.results, [(0, rec0 + pl.n_streams * codec.INFLATE_STREAM.itemsize), (sh0, sh0 + pl.n_shuf * codec.SHUFFLE_BLOCK.itemsize)]

    def decode(self, k, comp, target, errors):
        import torch
        from . import hip
        need = hip.inflate_scratch_bytes(self.plan_)
        if self.scratch[k] is None or self.scratch[k].numel() < need:
            self.scratch[k] = None
            self.scratch[k] = torch.empty(need, dtype=torch.uint8, device=self.device)
        if self.rounds is None and os.environ.get("AGGFLY_HIP_INGEST_TRACE") == "1":
            self.rounds = torch.zeros(1, dtype=torch.int32, device=self.device)
        hip.inflate_decode(comp, self.rec0, comp[self.rec0:], comp[self.sh0:], self.plan_, self.scratch[k], target, errors, self.rounds)


def _scatter_gpu_decode(job: _ScatterJob, threads: int, post):
    """Blosc-LZ4 chunks, Zstandard frames or zlib streams cross PCIe compressed: per batch the host reads the chunk files as
    they are into a page-locked slot and walks their headers into the codec's record lists (`_Lz4Route`, `_BloscRoute`, `_ZstdRoute`, `_DeflateRoute`); one
    upload carries the compressed bytes and the records; the codec's kernels decode on the slot's stream — straight into the
    cube when every chunk of the batch holds whole time steps of the window, else into a staging buffer that `job.place`
    empties.  The page-locked slot is free again when its upload is over; the device-side one is handed from the kernels to
    the slot's next upload by an event."""
    import torch
    from . import codec
    za, device, cb, idxs, cube = job.za, job.device, job.cb, job.idxs, job.cube
    flavour = getattr(za, "_blosc_flavour", (1, 1))
    route = (_ZstdRoute(job) if za.native_kind == "zstd" else _DeflateRoute(job) if _deflate_typesize(za.native_kind) is not None
             else _BloscRoute(job) if flavour[0] == 4 or flavour[1] == 2 else _Lz4Route(job))
    cuts, per, n_tail = _decode_batches(len(idxs), cb, route.nblk, job.whole_steps, route.max_per, route.target_bytes, route.max_bytes)
    all_idxs, idxs = idxs, idxs[:len(idxs) - n_tail]
    # staging slots in flight: 4 (3 measured 7 % slower), 6 when every batch is one big chunk (the converter's 265 MB chunks)
    nstage = max(1, min(int(os.environ.get("AGGFLY_HIP_GPU_DECODE_SLOTS", "6" if per == 1 else "4")), len(cuts) - 1))
    cube_bytes = cube.view(torch.uint8).reshape(-1) if job.whole_steps else None
    # compressed bytes + the record lists of a batch share one page-locked slot and one upload
    route.size(per, nstage, device)
    cmax, rec_bytes = route.cmax, route.rec_bytes
    # (the page-locked buffers are cached per size class: the tail's is one MORE of the slots' class when the two coincide)
    cls = lambda n: 1 << max(20, (int(n) - 1).bit_length())
    shared = n_tail > 0 and cls(n_tail * cb) == cls(per * cmax + rec_bytes)
    host = _pinned_stage(per * cmax + rec_bytes, nstage + (1 if shared else 0), device)
    thost = host[nstage] if shared else (_pinned_stage(n_tail * cb, 1, device)[0] if n_tail else None)
    host = host[:nstage]
    comp_dev = [torch.empty(per * cmax + rec_bytes, dtype=torch.uint8, device=device) for _ in range(nstage)]
    staged = [None] * nstage                             # decoded chunks of batches that cannot go straight into the cube
    errors = torch.zeros(1, dtype=torch.int32, device=device)
    copy_stream = torch.cuda.Stream(device=device)
    copy_stream.wait_stream(torch.cuda.current_stream(device))    # (as on the host route: order behind the allocator's stream)
    # two kernel streams whatever the number of slots: HIP maps streams onto a few hardware queues (4 by default), and an upload
    # that shares its queue with a kernel stream waits for that stream's kernels — seen as uploads starting exactly when the
    # previous batch's kernels ended (profiles/r02_ingest_timeline_queues.txt)
    two = [torch.cuda.Stream(device=device) for _ in range(min(2, nstage))]
    for ws in two:
        ws.wait_stream(torch.cuda.current_stream(device))
    work_streams = [two[k % len(two)] for k in range(nstage)]
    done, uploaded = [None] * nstage, [None] * nstage
    trace = _IngestTrace()
    origin = torch.cuda.Event(enable_timing=True)
    if trace.on:
        origin.record(copy_stream)

    def drain():
        # earlier batches' uploads and kernels may still be in flight on the copy / work streams: nothing of this request
        # (cube, staging, page-locked slots) may go back to its pool — or to a retry on the host route — before they are done
        copy_stream.synchronize()
        for ws in two:
            ws.synchronize()

    try:
        _gpu_decode_batches(job, threads, cuts, per, cmax, route, nstage, host, comp_dev, staged, errors,
                            copy_stream, work_streams, done, uploaded, trace, cube_bytes)
        if n_tail:
            tail = all_idxs[len(idxs):]
            tdev = torch.empty(n_tail * cb, dtype=torch.uint8, device=device)
            hbuf = thost[:n_tail * cb].numpy()
            res = codec.decode_ranges(za.native_kind, [za.chunk_locator(i) for i in tail], [hbuf[i * cb:(i + 1) * cb] for i in range(n_tail)],
                                      threads=threads)
            trace.lap("read")
            with torch.cuda.stream(copy_stream):        # behind the compressed uploads; the placement runs on the copy stream too
                tdev.copy_(thost[:n_tail * cb], non_blocking=True)
                job.undelta(tdev, n_tail)
                job.place(tail, res, tdev)
            trace.lap("enqueue")
    except BaseException:
        drain()
        raise
    last = two[0]
    for ws in two[1:]:
        last.wait_stream(ws)
    if n_tail:
        last.wait_stream(copy_stream)                    # (the tail's placement ran there)
    with torch.cuda.stream(last):
        job.finish()
        if post is not None:
            post(cube)
    trace.skip()
    last.synchronize()
    copy_stream.synchronize()
    trace.drained()
    extra = {getattr(route, "rounds_key", "zstd_jump_rounds"): int(route.rounds.item())} if getattr(route, "rounds", None) is not None else {}
    trace.report(origin, gpu_decode=True, batches=len(cuts) - 1, chunks_per_batch=per, **extra)
    if int(errors.item()):
        raise codec.CodecError(f"{int(errors.item())} {route.what} of {za.path} are malformed (GPU decode); "
                               "AGGFLY_HIP_GPU_DECODE=0 decodes on the host and names the chunk")
    torch.cuda.current_stream(device).wait_stream(last)
    return cube


def _gpu_decode_batches(job, threads, cuts, per, cmax, route, nstage, host, comp_dev, staged, errors,
                        copy_stream, work_streams, done, uploaded, trace, cube_bytes):
    """The batch loop of `_scatter_gpu_decode` (which drains the streams if anything here raises)."""
    import torch
    from . import codec
    za, device, cb, idxs = job.za, job.device, job.cb, job.idxs
    for b, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        batch = idxs[lo:hi]
        k = b % nstage
        trace.skip()
        if uploaded[k] is not None:
            uploaded[k].synchronize()                    # the page-locked slot is free once its upload is over
        trace.lap("wait")
        # ---- host: the chunk files as they are, packed back to back; then the record lists ----
        hall = host[k].numpy()
        offs, sizes = codec.read_packed([za.chunk_locator(i, probe=False) for i in batch], hall[:per * cmax], 64, threads)
        res = sizes.tolist()
        trace.lap("read")
        present = np.nonzero(sizes != -100)[0]
        rec0 = int(offs[-1])
        direct = job.whole_steps and all(job.inside(it) for it, _, _ in batch)       # (whole_steps: a time-leading array)
        out_offs = (np.array([batch[i][0] * job.tc - job.ka for i in present], dtype=np.int64) * job.step_bytes if direct
                    else present.astype(np.int64) * cb)
        pres, ranges = route.plan(k, hall, rec0, offs, sizes, present, out_offs)
        if (pres != cb).any():
            badc = [za.chunk_locator(batch[int(present[i])])[0] for i in np.nonzero(pres != cb)[0][:4]]
            raise codec.CodecError(f"chunks {badc} are damaged or decode to another size than {cb} bytes")
        trace.lap("plan")
        # ---- upload (copy stream), then decode + placement (the slot's stream) ----
        with torch.cuda.stream(copy_stream):
            if done[k] is not None:
                copy_stream.wait_event(done[k])          # the kernels of the slot's previous batch have read comp_dev[k]
            if trace.on:
                trace.batches.append({"batch": b, "chunks": len(batch), "host_read_done_ms": (trace.clock() - trace.t0) * 1e3,
                                      **{n: torch.cuda.Event(enable_timing=True) for n in ("h2d0", "h2d1", "k1")}})
                trace.batches[-1]["h2d0"].record(copy_stream)
            for a_, b_ in ranges:
                if b_ > a_:
                    comp_dev[k][a_:b_].copy_(host[k][a_:b_], non_blocking=True)
            uploaded[k] = torch.cuda.Event()
            uploaded[k].record(copy_stream)
            if trace.on:
                trace.batches[-1]["h2d1"].record(copy_stream)
        work_streams[k].wait_event(uploaded[k])
        with torch.cuda.stream(work_streams[k]):
            if not direct and staged[k] is None:
                staged[k] = torch.empty(per * cb, dtype=torch.uint8, device=device)
            target = cube_bytes if direct else staged[k]
            route.decode(k, comp_dev[k], target, errors)
            if not direct:
                job.undelta(staged[k], len(batch))
            job.place(batch, res, staged[k], skip_present=direct)
            done[k] = torch.cuda.Event()
            done[k].record(work_streams[k])
            if trace.on:
                trace.batches[-1]["k1"].record(work_streams[k])
        trace.lap("enqueue")


def _decode_time(values, attrs):
    units, cal = attrs.get("units"), attrs.get("calendar", "standard")
    if units is None:
        return pd.DatetimeIndex(values)
    if cal in STANDARD_CALENDARS:
        unit, _, epoch = units.partition(" since ")
        unit = unit.strip().lower().rstrip("s")
        factor = {"second": 1e9, "minute": 60e9, "hour": 3600e9, "day": 86400e9}[unit]
        base = pd.Timestamp(epoch.strip())
        return pd.DatetimeIndex(base.value + np.round(np.asarray(values, dtype=np.float64) * factor).astype(np.int64))
    return decode_cf_time(values, units, cal)


def _decoded_coord(values, attrs):
    """A coordinate as its container stores it: the decoded time index where ``units`` read "<unit> since <epoch>" (CF), else the values."""
    return _decode_time(values, attrs) if " since " in str(attrs.get("units", "")) else values


def _py(v):
    """A numpy scalar (an attribute of an HDF5 or a classic file) as the Python number it holds; anything else as it is."""
    return v.item() if isinstance(v, np.generic) else v


def _py_attrs(attrs, skip=()) -> dict:
    return {k: _py(v) for k, v in attrs.items() if k not in skip}


def _zarr_coords(path, dims) -> dict:
    """{dim: values} of the dimensions of a Zarr store that have a coordinate array, the time axis decoded."""
    coords = {}
    for d in dims:
        cp = os.path.join(path, d)
        if is_zarr_array(cp):
            c = ZarrArray(cp)
            coords[d] = _decoded_coord(c.read(threads=1), c.attrs)
    return coords


def _attr_fill(attrs):
    """``_FillValue`` / ``missing_value`` attribute; xarray writes it base64-packed into format-3 stores."""
    fv = attrs.get("_FillValue", attrs.get("missing_value"))
    if isinstance(fv, str):
        if fv in ("NaN", "nan"):
            return float("nan")
        try:
            import base64
            import struct
            raw = base64.standard_b64decode(fv)
            fv = struct.unpack("<d", raw)[0] if len(raw) == 8 else (struct.unpack("<f", raw)[0] if len(raw) == 4 else None)
        except Exception:
            fv = None
    return fv


def _cf_mask_scale(arr, attrs):
    fv = _attr_fill(attrs)
    unsigned = arr.dtype.kind in "iu" and _stored_unsigned(arr.dtype, attrs)      # (refuses _Unsigned = "false" on unsigned storage)
    if unsigned and arr.dtype.kind == "i":
        # _Unsigned = "true": the same bits read as the unsigned type, and a fill written in the signed type likewise (xarray)
        arr = arr.view(np.dtype(f"u{arr.dtype.itemsize}").newbyteorder(arr.dtype.byteorder))    # (a classic file's integers are big-endian)
        if fv is not None and not isinstance(fv, str) and not (isinstance(fv, float) and np.isnan(fv)) and int(fv) == fv and fv < 0:
            fv = int(fv) + (1 << (8 * arr.dtype.itemsize))
    # numbers, not numpy scalars: a float64 scalar (a classic file's attribute, as scipy hands it on) would widen `out *= sf` to
    # float64 under NumPy 2's promotion rules, where every other container — and every device route — unpacks in the cube's type
    sf, ao = _py(attrs.get("scale_factor")), _py(attrs.get("add_offset"))
    if fv is None and sf is None and ao is None:
        return arr
    out = arr.astype(np.float64 if arr.dtype.itemsize > 2 and arr.dtype.kind != "f" else (arr.dtype if arr.dtype.kind == "f" else np.float32))
    if fv is not None and not (isinstance(fv, float) and np.isnan(fv)):
        out[arr == fv] = np.nan
    if sf is not None:
        out *= sf
    if ao is not None:
        out += ao
    return out


def open_zarr(path: str, var: str, threads: int = 8) -> DataArray:
    arr = ZarrArray(os.path.join(path, var))
    dims = arr.dims
    data = _cf_mask_scale(arr.read(threads=threads), arr.attrs)
    return DataArray(data, dims, _zarr_coords(path, dims), name=var, attrs=arr.attrs)


_CRC32C_TABLE = None


def _crc32c(data: bytes) -> int:
    """CRC-32C (Castagnoli), bytewise table — only ever run over a shard index (a few KiB)."""
    global _CRC32C_TABLE
    if _CRC32C_TABLE is None:
        tab = []
        for i in range(256):
            c = i
            for _ in range(8):
                c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
            tab.append(c)
        _CRC32C_TABLE = tab
    c = 0xFFFFFFFF
    for b in data:
        c = _CRC32C_TABLE[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


class _DeviceCube:
    """Stands for the array in `_write_array` when the chunks are cut and encoded in HBM (`_write_chunks_gpu`): the shape and the numpy
    dtype the metadata is written from, and the HBM tensor."""

    def __init__(self, tensor):
        self.tensor = tensor
        self.shape = tuple(int(n) for n in tensor.shape)
        self.dtype = np.dtype(str(tensor.dtype).replace("torch.", ""))
        self.nbytes = int(tensor.numel()) * int(tensor.element_size())


def _write_array(path, name, data, dims, chunks, attrs, compressor, zarr_format: int = 2, shards=None, filters=None):
    """``filters`` (format 2, host arrays): numcodecs element-filter configs in write order; every chunk goes through
    `filter_elements` before the compressor and the configs are written into ``.zarray`` as given."""
    d = os.path.join(path, name)
    os.makedirs(d, exist_ok=True)
    if not isinstance(data, _DeviceCube):
        data = np.ascontiguousarray(data)
    chunks = tuple(int(min(c, s)) if s else 1 for c, s in zip(chunks, data.shape))
    cid = compressor["id"] if compressor else None
    elem = []
    if filters:
        if zarr_format != 2 or isinstance(data, _DeviceCube):
            raise ValueError("filters are written into format-2 stores, from a host array")
        elem, shuffles = _parse_elem_filters(filters, data.dtype)
        if shuffles:
            raise ValueError("filters: the byte shuffle is the compressor's (compress='blosc'); element filters only")
    stored_itemsize = elem[-1]["astype"].itemsize if elem else data.dtype.itemsize
    if zarr_format == 2:
        meta = {"zarr_format": 2, "shape": list(data.shape), "chunks": list(chunks), "dtype": data.dtype.str,
                "compressor": compressor, "fill_value": "NaN" if data.dtype.kind == "f" else 0, "order": "C",
                "filters": [dict(f) for f in filters] if filters else None}
        with open(os.path.join(d, ".zarray"), "w") as f:
            json.dump(meta, f)
        with open(os.path.join(d, ".zattrs"), "w") as f:
            json.dump(dict(attrs, _ARRAY_DIMENSIONS=list(dims)), f)
    elif zarr_format == 3:
        v3name = {v: k for k, v in _V3_DTYPES.items()}[data.dtype.newbyteorder("<").str if data.dtype.itemsize > 1 else data.dtype.str]
        codecs = [{"name": "bytes", "configuration": {"endian": "little"}}]
        if cid == "blosc":
            codecs.append({"name": "blosc", "configuration": {"cname": compressor.get("cname", "lz4"), "clevel": compressor.get("clevel", 5),
                                                               "shuffle": {0: "noshuffle", 1: "shuffle", 2: "bitshuffle"}[compressor.get("shuffle", 1)],
                                                               "typesize": data.dtype.itemsize, "blocksize": compressor.get("blocksize", 0)}})
        elif cid == "zstd":
            codecs.append({"name": "zstd", "configuration": {"level": compressor.get("level", 0), "checksum": False}})
        elif cid in ("zlib", "gzip"):
            cid = "gzip"
            codecs.append({"name": "gzip", "configuration": {"level": compressor.get("level", 1)}})
        if shards is not None:
            shards = tuple(int(x) for x in shards)
            if any(s_ % c_ for s_, c_ in zip(shards, chunks)):
                raise ValueError("shards must be multiples of chunks")
            codecs = [{"name": "sharding_indexed", "configuration": {
                "chunk_shape": list(chunks), "codecs": codecs, "index_location": "end",
                "index_codecs": [{"name": "bytes", "configuration": {"endian": "little"}}, {"name": "crc32c"}]}}]
        meta = {"zarr_format": 3, "node_type": "array", "shape": list(data.shape), "data_type": v3name,
                "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": list(shards if shards is not None else chunks)}},
                "chunk_key_encoding": {"name": "default", "configuration": {"separator": "/"}},
                "fill_value": "NaN" if data.dtype.kind == "f" else 0, "codecs": codecs, "attributes": dict(attrs),
                "dimension_names": list(dims), "storage_transformers": []}
        with open(os.path.join(d, "zarr.json"), "w") as f:
            json.dump(meta, f)
    else:
        raise ValueError("zarr_format must be 2 or 3")
    grid = [range((s + c - 1) // c) for s, c in zip(data.shape, chunks)]

    if shards is not None and zarr_format != 3:
        raise ValueError("shards need zarr_format=3")
    if isinstance(data, _DeviceCube):
        return _write_chunks_gpu(d, data, chunks, zarr_format, shards, compressor.get("cname", "lz4"))

    def encode_chunk(idx):
        sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunks, data.shape))
        part = data[sl]
        if part.shape == tuple(chunks):
            blk = np.ascontiguousarray(part)
        else:                                               # edge chunk: padded with the fill value
            blk = np.full(chunks, np.nan if data.dtype.kind == "f" else 0, dtype=data.dtype)
            blk[tuple(slice(0, n) for n in part.shape)] = part
        if elem:                                            # (the padding of an edge chunk is NaN: its stored integer is arbitrary)
            with np.errstate(invalid="ignore"):
                blk = filter_elements(blk, elem)
        raw = blk.tobytes() if cid in (None, "zlib", "gzip") else None
        if cid == "zlib":
            raw = zlib.compress(raw, compressor.get("level", 1))
        elif cid == "gzip":
            raw = gzip.compress(raw, compressor.get("level", 1))
        elif cid == "blosc":
            from . import codec
            raw = codec.blosc_encode(blk, stored_itemsize, shuffle=compressor.get("shuffle", 1) == 1,
                                     blocksize=compressor.get("blocksize", 0), cname=compressor.get("cname", "lz4"),
                                     bitshuffle=compressor.get("shuffle", 1) == 2)
        elif cid == "zstd":
            from . import codec
            raw = codec.zstd_encode(blk, compressor.get("level", 3) or 3)
        elif cid is not None:
            raise ValueError(f"cannot write Zarr compressor {cid!r}")
        return raw

    def write_chunk(idx):
        raw = encode_chunk(idx)
        fn = os.path.join(d, ".".join(str(i) for i in idx)) if zarr_format == 2 else os.path.join(d, "c", *[str(i) for i in idx])
        os.makedirs(os.path.dirname(fn), exist_ok=True)
        with open(fn, "wb") as f:
            f.write(raw)

    if shards is not None:
        per = [s_ // c_ for s_, c_ in zip(shards, chunks)]
        nshard = [-(-n // s_) for n, s_ in zip(data.shape, shards)]
        for sidx in np.ndindex(*nshard):
            body, index = [], np.full((int(np.prod(per)), 2), 0xFFFFFFFFFFFFFFFF, dtype="<u8")
            pos = 0
            for k, inner in enumerate(np.ndindex(*per)):
                idx = tuple(si * p_ + ii for si, p_, ii in zip(sidx, per, inner))
                if any(i * c >= n for i, c, n in zip(idx, chunks, data.shape)):
                    continue                                # an inner chunk wholly outside the array stays empty
                raw = encode_chunk(idx)
                index[k] = (pos, len(raw))
                body.append(raw)
                pos += len(raw)
            tail = index.tobytes()
            fn = os.path.join(d, "c", *[str(i) for i in sidx])
            os.makedirs(os.path.dirname(fn), exist_ok=True)
            with open(fn, "wb") as f:
                f.write(b"".join(body) + tail + _crc32c(tail).to_bytes(4, "little"))
        return

    idxs = list(np.ndindex(*[len(g) for g in grid]))
    if len(idxs) > 4 and data.nbytes > (8 << 20):           # compress + write chunk-parallel (the codecs drop the GIL)
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
            list(ex.map(write_chunk, idxs))
    else:
        for idx in idxs:
            write_chunk(idx)


# The write side in HBM.  `dataset_to_zarr(..., encode="gpu")`: the decode-in-HBM route (`_Lz4Route`) in reverse — the cube stays in HBM,
# chunks are cut out of it, byte-shuffled and LZ4-encoded there, and cross PCIe compressed; the host fills the Blosc-1 headers and tables
# and writes the files.  encode="auto" takes it for device-resident cubes of GPU_ENCODE_AUTO_BYTES and more, or when
# AGGFLY_HIP_GPU_ENCODE=1 asks for it (=0: never).
# Set by the rule of GPU_DECODE_AUTO_BYTES_DEFLATE: the smallest size from which, on every layout of scripts/encode_bench.py ((1, ny, nx),
# (24, ny, nx), whole-series tiles of the configs[0] cube, 64 MiB ... 860 MB), the GPU route's median is <= 0.9 x the host route's minimum
# AND the store it writes is at most 1.10 x the host-written one.  Measured (profiles/lz4_encode.txt): 0.68 / 0.61 / 0.46 / 0.45 x at
# 128 / 256 / 512 / 860 MB on the worst layout, 1.07 x at 64 MiB; stores 1.005-1.007 x.  None would mean: never without the environment.
GPU_ENCODE_AUTO_BYTES = 128 << 20
# The same rule for compress="blosc-zstd" (Zstandard streams from `hip.zstd_encode_blocks`), the host-written store being libzstd's at
# level 3.  Measured (profiles/zstd_encode.txt): stores 0.97-1.093 x, within the rule; the time rule fails on the (24, ny, nx) layout at
# every size — 1.36 / 0.99 / 0.95 / 0.93 x at 64 / 256 / 512 / 860 MB — while whole-series tiles run at 0.18-0.34 x.  No size meets the rule
# on every layout, so None: "auto" never takes the route for Zstandard streams without AGGFLY_HIP_GPU_ENCODE=1.
GPU_ENCODE_AUTO_BYTES_BLOSC_ZSTD = None
GPU_ENCODE_BATCH_BYTES = 256 << 20                # decoded bytes of a batch of chunks (one chunk at least)
_GPU_ENCODE_DTYPES = ("f4", "f8", "i1", "u1", "i2", "u2", "i4", "u4", "i8", "u8")


def _gpu_encode_refusal(compress, np_dtype, ctuple) -> Optional[str]:
    """None, or why `dataset_to_zarr` cannot take the GPU route for this call."""
    if compress not in (True, "blosc", "blosc-zstd"):
        return (f"compress={compress!r}: the GPU route writes Blosc-1 chunks of LZ4 or Zstandard streams under the byte shuffle "
                "(compress=True, 'blosc' or 'blosc-zstd') only")
    if np.dtype(np_dtype).str[1:] not in _GPU_ENCODE_DTYPES:
        return f"dtype {np.dtype(np_dtype)}: the GPU route takes float32, float64 and integers of 1, 2, 4 or 8 bytes"
    if int(np.prod(ctuple)) * np.dtype(np_dtype).itemsize > 0x7fffffff - 64:
        return "a chunk of 2 GiB or more does not fit a Blosc-1 container"
    return None


def _write_chunks_gpu(d, data: "_DeviceCube", chunks, zarr_format, shards, cname="lz4"):
    """The chunk files (or shard files) of one array, encoded in HBM.  Per batch of chunks of up to GPU_ENCODE_BATCH_BYTES:
    `hip.take_box` per chunk (edge chunks padded with the fill value) -> `hip.shuffle_blocks` -> `hip.lz4_encode_streams` into one
    slot per stream (``cname`` "zstd": `hip.zstd_encode_blocks` into one slot per block of a frame, planned by
    `codec.BloscZstdEncodePlan`; everything else is shared) -> the sizes to the host (a small D2H) -> `hip.copy_ranges` packs the
    streams into their containers (a Zstandard frame that did not shrink: the shuffled bytes instead) -> one D2H
    into a page-locked buffer -> `codec.BloscEncodePlan.finish` fills headers, block tables and stream lengths -> files, from a small
    thread pool.  Two packed buffers on each side: batch i's D2H and file writes overlap batch i + 1's kernels.  Shard bodies and the
    shard index with its crc32c are host work over the compressed chunks."""
    import torch
    from . import codec, hip
    hip.require_gpu()
    cube = data.tensor.contiguous()
    dev = cube.device
    shape, item = data.shape, data.dtype.itemsize
    cb = int(np.prod(chunks)) * item
    fill_bits = int(np.array([np.nan], dtype=data.dtype).view(f"u{item}")[0]) if data.dtype.kind == "f" else 0
    grid = [(s + c - 1) // c for s, c in zip(shape, chunks)]
    if shards is None:
        order = [(idx, None) for idx in np.ndindex(*grid)]
    else:                                                   # shard by shard, the inner chunks in the order of the shard's index
        per_shard = [s_ // c_ for s_, c_ in zip(shards, chunks)]
        nshard = [-(-n // s_) for n, s_ in zip(shape, shards)]
        order = []
        for sidx in np.ndindex(*nshard):
            for k, inner in enumerate(np.ndindex(*per_shard)):
                idx = tuple(si * p_ + ii for si, p_, ii in zip(sidx, per_shard, inner))
                if all(i * c < n for i, c, n in zip(idx, chunks, shape)):      # (an inner chunk wholly outside the array stays empty)
                    order.append((idx, (sidx, k)))
        n_inner = int(np.prod(per_shard))
    if not order:
        return
    per = max(1, min(len(order), GPU_ENCODE_BATCH_BYTES // cb))
    plans = {}
    zstd = cname == "zstd"                                   # the flavour decides the plan class, the buffers and the encode call: nothing else
    plan_class = codec.BloscZstdEncodePlan if zstd else codec.BloscEncodePlan

    def plan_of(n):                                         # (two at most: the full batch and the last one)
        if n not in plans:
            pl = plan_class(n, cb, item)
            rec = np.concatenate([pl.streams.view(np.uint8), pl.blocks.view(np.uint8)])
            plans[n] = (pl, torch.from_numpy(rec).to(dev), pl.streams.nbytes)
        return plans[n]

    pl0 = plan_of(per)[0]
    if zstd:                                                 # one work buffer, the shuffled input and behind it the slots: `copy_ranges` takes either
        packed_cap = per * (cb + pl0.header_bytes + 4 * pl0.frames)
        chunk_dev = torch.empty(per * cb, dtype=torch.uint8, device=dev)
        tmp_dev = torch.empty(pl0.work_bytes, dtype=torch.uint8, device=dev)
        scratch_dev = torch.empty(pl0.scratch_bytes, dtype=torch.uint8, device=dev)
        slots_dev = tmp_dev

        def encode(pl, rec_dev):
            if len(pl.streams):                              # (chunks under 128 bytes are stored: nothing to encode)
                hip.zstd_encode_blocks(tmp_dev, rec_dev, len(pl.streams), scratch_dev, tmp_dev[pl.slot_base:], csize_dev)
    else:
        packed_cap = per * (cb + pl0.header_bytes + 4 * pl0.per_chunk)
        chunk_dev, tmp_dev, slots_dev = (torch.empty(per * cb, dtype=torch.uint8, device=dev) for _ in range(3))

        def encode(pl, rec_dev):
            hip.lz4_encode_streams(tmp_dev, rec_dev, len(pl.streams), slots_dev, csize_dev)
    csize_dev = torch.empty(max(1, per * pl0.per_chunk), dtype=torch.int32, device=dev)
    packed_dev = [torch.empty(packed_cap, dtype=torch.uint8, device=dev) for _ in range(2)]
    pinned = _pinned_stage(packed_cap, 2, dev)
    work, copy = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
    cview = chunk_dev.view(cube.dtype)
    shard_body = {}                                          # sidx -> {k: bytes}, until the shard's last chunk has arrived

    def chunk_file(idx):
        fn = os.path.join(d, ".".join(str(i) for i in idx)) if zarr_format == 2 else os.path.join(d, "c", *[str(i) for i in idx])
        os.makedirs(os.path.dirname(fn), exist_ok=True)
        return fn

    def write_file(fn, buf):
        with open(fn, "wb") as f:
            f.write(buf)

    def write_files(items):                                  # (one task per group of files: a task per file costs more than a small file)
        for idx, buf in items:
            write_file(chunk_file(idx), buf)

    def write_shard(sidx, parts):
        index = np.full((n_inner, 2), 0xFFFFFFFFFFFFFFFF, dtype="<u8")
        pos, body = 0, []
        for k in sorted(parts):
            index[k] = (pos, len(parts[k]))
            body.append(parts[k])
            pos += len(parts[k])
        tail = index.tobytes()
        write_file(chunk_file(sidx), b"".join(body) + tail + _crc32c(tail).to_bytes(4, "little"))

    def kernels(batch):
        """take, shuffle, encode: everything up to the stream sizes."""
        pl, rec_dev, blocks_at = plan_of(len(batch))
        j = 0
        while j < len(batch):
            # chunks that follow one another in time over the same cells are one box of m * chunks[0] steps: one launch (a store of
            # whole-grid chunks, (1, ny, nx) or (24, ny, nx), is one launch per batch, not thousands)
            idx, m = batch[j][0], 1
            while j + m < len(batch) and batch[j + m][0] == (idx[0] + m,) + tuple(idx[1:]):
                m += 1
            at = tuple(i * c for i, c in zip(idx, chunks))
            run = (m * chunks[0],) + tuple(chunks[1:])
            box = tuple(min(c, n - a) for c, n, a in zip(run, shape, at))
            hip.take_box(cube, cview[j * (cb // item):(j + m) * (cb // item)].view(run), at, box, fill_bits)
            j += m
        nb = len(pl.blocks)
        for b0 in range(0, nb, 65535):
            hip.shuffle_blocks(chunk_dev, tmp_dev, rec_dev[blocks_at + b0 * codec.SHUFFLE_BLOCK.itemsize:], min(65535, nb - b0), pl.max_bsize)
        encode(pl, rec_dev)
        return pl

    def pack(k, pl):
        """The sizes to the host, the streams into their containers, the containers on their way to the host."""
        csizes = csize_dev[:len(pl.streams)].cpu().numpy()   # (waits for the batch's kernels)
        ranges, off, size = pl.place(csizes)
        total = int(size.sum())
        hip.copy_ranges(slots_dev, packed_dev[k % 2], torch.from_numpy(ranges.view(np.uint8)).to(dev), len(ranges))
        done = torch.cuda.Event()
        done.record(work)
        with torch.cuda.stream(copy):
            copy.wait_event(done)
            pinned[k % 2][:total].copy_(packed_dev[k % 2][:total], non_blocking=True)
            arrived = torch.cuda.Event()
            arrived.record(copy)
        return arrived, off, size, total

    def finish(k, batch, pl, arrived, off, size, total, pool):
        arrived.synchronize()
        host = pinned[k % 2][:total].numpy()
        pl.finish(host)
        futures, plain = [], []
        for (idx, shard), o, z in zip(batch, off, size):
            if shard is None:
                plain.append((idx, host[o:o + z]))
            else:
                sidx, kk = shard
                parts = shard_body.setdefault(sidx, {})
                parts[kk] = host[o:o + z].tobytes()
                if shard_last[sidx] == idx:
                    futures.append(pool.submit(write_shard, sidx, shard_body.pop(sidx)))
        group = max(1, -(-len(plain) // (4 * n_workers)))
        futures += [pool.submit(write_files, plain[i:i + group]) for i in range(0, len(plain), group)]
        return futures

    shard_last = {sh[0]: idx for idx, sh in order if sh is not None}
    batches = [order[i:i + per] for i in range(0, len(order), per)]
    writes = [[], []]                                        # the file writes still reading pinned[0] / pinned[1]
    n_workers = min(8, os.cpu_count() or 1)
    with ThreadPoolExecutor(max_workers=n_workers) as pool:
        pending = None
        for k, batch in enumerate(batches):
            pl = kernels(batch)
            if pending is not None:                          # batch k - 1 arrives and is written while batch k's kernels run
                writes[(k - 1) % 2] = finish(*pending, pool)
            for f in writes[k % 2]:                          # (batch k - 2's files: its page-locked buffer is about to be overwritten)
                f.result()
            pending = (k, batch, pl) + pack(k, pl)
        writes[(len(batches) - 1) % 2] = finish(*pending, pool)
        for w in writes:
            for f in w:
                f.result()
    torch.cuda.synchronize(dev)


def _encode_time(t):
    if isinstance(t, CFTimeIndex):
        return (t.seconds / 3600.0), {"units": "hours since 0000-01-01 00:00:00", "calendar": t.calendar}
    t = pd.DatetimeIndex(t)
    hours = (t.values.astype("datetime64[s]").astype(np.int64) - np.datetime64("1900-01-01", "s").astype(np.int64)) / 3600.0
    return hours, {"units": "hours since 1900-01-01 00:00:00", "calendar": "proleptic_gregorian"}


def _auto_chunks(sizes: dict, itemsize: int, target_mb: float = 256) -> dict:
    """Chunk policy of `_auto_chunks` (`zarr_convert.py:31-47`): keep time in one chunk when a
    square spatial tile of >= 32 cells fits the byte budget (tile capped at 256 and at the
    grid extent); otherwise split time next to a 128-cell tile."""
    ny, nx, nt = int(sizes["latitude"]), int(sizes["longitude"]), max(int(sizes["time"]), 1)
    budget = max(1, int(target_mb * 1024 * 1024 / itemsize))
    side = int((budget / nt) ** 0.5)
    if side >= 32:
        side = int(min(side, 256, ny, nx))
        return {"time": -1, "latitude": side, "longitude": side}
    side = int(min(128, ny, nx))
    return {"time": int(min(max(1, budget // (side * side)), nt)), "latitude": side, "longitude": side}


def dataset_to_zarr(dataset: Dataset, path: str, var: str = "var", chunks=None, compress=True, mode: str = "w", zarr_format: int = 2,
                    shards=None, encode: str = "auto", layout: str = "time-major", filters=None):
    """`dataset_to_zarr` (`zarr_convert.py:50-121`): write a time-major, time-contiguous store.
    ``layout``: "time-major" — the data variable is (time, latitude, longitude) — or "time-last" — (latitude, longitude, time), the
    reference's converter's own layout (it writes `Dataset.da` as it stands, `zarr_convert.py:83-113`): the same ``chunks`` /
    `_auto_chunks` policy and ``shards``, reordered.  "time-last" is encoded on the host: ``encode="gpu"`` raises `ValueError`
    (the encoder's `take_box` cuts time-major chunks only), "auto" takes the host route.
    ``compress``: True / "blosc" -> Blosc-1 LZ4 + byte shuffle (what zarr-python 2 / numcodecs write by
    default and read back), "blosc-zstd" / "blosc-bitshuffle" / "blosc-zstd-bitshuffle" -> Blosc-1 with Zstandard streams and the byte
    shuffle, LZ4 streams and the bit shuffle, or both (the Zarr v3 ``blosc`` codec's default ``cname`` is zstd), "zstd" (zarr-python
    3's default codec), "zlib" -> zlib level 1, False -> raw.
    ``zarr_format``: 2 (``.zarray``) or 3 (``zarr.json``, ``c/`` chunk keys); ``shards`` (format 3): a dict like
    ``chunks`` giving the shard shape in which the chunks are bundled (``sharding_indexed``).
    ``encode``: where the data variable's chunks are cut, shuffled and compressed.  "host": on host threads, from a host copy of
    the cube.  "gpu": in HBM (`_write_chunks_gpu`; Blosc-1 under the byte shuffle with LZ4 streams, ``compress`` True or "blosc", or
    Zstandard streams, "blosc-zstd"; a host-resident cube is uploaded first) — the chunks cross PCIe compressed; anything else
    raises `ValueError`.  The store decodes to the same values; its streams are the GPU encoders', not liblz4's or libzstd's.
    "auto": the GPU route for a device-resident cube of `GPU_ENCODE_AUTO_BYTES` (``compress="blosc-zstd"``: `GPU_ENCODE_AUTO_BYTES_BLOSC_ZSTD`) or more (None: never) or when
    ``AGGFLY_HIP_GPU_ENCODE=1`` is set (``0``: never), and the call is
    eligible; else the host route — always for a host-resident cube.  Coordinates and metadata are written by the same code on every route.
    ``filters`` (format 2 only): numcodecs element filters for the data variable, a list of their configs in write order — e.g.
    ``[{"id": "fixedscaleoffset", "scale": 10.0, "offset": 273.15, "dtype": "<f4", "astype": "<i2"}, {"id": "delta", "dtype": "<i2"}]``
    — applied by numcodecs' encode definitions (`filter_elements`) on the host and written into ``.zarray``; ``encode="gpu"`` raises
    `ValueError`, "auto" takes the host route.  Such a store is read back through `ZarrArray`'s element filters."""
    if encode not in ("auto", "host", "gpu"):
        raise ValueError(f"encode must be 'auto', 'host' or 'gpu', got {encode!r}")
    if filters:
        if zarr_format != 2:
            raise ValueError("dataset_to_zarr(filters=...): element filters are a format-2 feature (zarr_format=3 has no such codecs)")
        if encode == "gpu":
            raise ValueError("dataset_to_zarr(encode='gpu'): filters are applied on the host (the GPU encoder takes the cube's own elements)")
        encode = "host"
    if layout not in ("time-major", "time-last"):
        raise ValueError(f"layout must be 'time-major' or 'time-last', got {layout!r}")
    tlast = layout == "time-last"
    if tlast:
        if encode == "gpu":
            raise ValueError("dataset_to_zarr(encode='gpu'): layout='time-last' is encoded on the host (the GPU encoder cuts "
                             "time-major chunks only)")
        encode = "host"
    cube = dataset.cube()
    on_host = isinstance(cube, np.ndarray)
    np_dtype = cube.dtype if on_host else np.dtype(str(cube.dtype).replace("torch.", ""))
    sizes = {"time": cube.shape[0], "latitude": cube.shape[1], "longitude": cube.shape[2]}
    ch = dict(_auto_chunks(sizes, np_dtype.itemsize)) if chunks is None else dict(chunks)
    ctuple = tuple(sizes[d] if ch.get(d, -1) in (-1, None) else ch[d] for d in ("time", "latitude", "longitude"))
    use_gpu = False
    if encode != "host":
        refusal = _gpu_encode_refusal(compress, np_dtype, tuple(int(min(c, s)) if s else 1 for c, s in zip(ctuple, cube.shape)))
        if encode == "gpu":
            if refusal:
                raise ValueError(f"dataset_to_zarr(encode='gpu'): {refusal}")
            use_gpu = True
        elif refusal is None and not on_host and cube.is_cuda:
            nbytes = int(cube.numel()) * int(cube.element_size())
            mode = os.environ.get("AGGFLY_HIP_GPU_ENCODE", "auto")
            auto_bytes = GPU_ENCODE_AUTO_BYTES_BLOSC_ZSTD if compress == "blosc-zstd" else GPU_ENCODE_AUTO_BYTES
            use_gpu = mode == "1" or (mode != "0" and auto_bytes is not None and nbytes >= auto_bytes)
    if use_gpu:
        if on_host:
            import torch
            cube = torch.from_numpy(cube).to("cuda")
        cube = _DeviceCube(cube)
    elif not on_host:
        cube = cube.cpu().numpy()
    os.makedirs(path, exist_ok=True)
    if zarr_format == 2:
        with open(os.path.join(path, ".zgroup"), "w") as f:
            json.dump({"zarr_format": 2}, f)
    else:
        with open(os.path.join(path, "zarr.json"), "w") as f:
            json.dump({"zarr_format": 3, "node_type": "group", "attributes": {}}, f)
    if compress in (True, "blosc"):
        comp = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}
    elif compress in ("blosc-zstd", "blosc-bitshuffle", "blosc-zstd-bitshuffle"):
        comp = {"id": "blosc", "cname": "zstd" if "zstd" in compress else "lz4", "clevel": 5, "shuffle": 2 if "bitshuffle" in compress else 1,
                "blocksize": 0}
    elif compress == "zstd":
        comp = {"id": "zstd", "level": 3}
    elif compress == "zlib":
        comp = {"id": "zlib", "level": 1}
    elif not compress:
        comp = None
    else:
        raise ValueError("compress must be True, False, 'blosc', 'blosc-zstd', 'blosc-bitshuffle', 'blosc-zstd-bitshuffle', 'zstd' or 'zlib', "
                         f"got {compress!r}")
    stuple = None
    if shards is not None:
        stuple = tuple(sizes[d] if shards.get(d, -1) in (-1, None) else shards[d] for d in ("time", "latitude", "longitude"))
        stuple = tuple(-(-s_ // c_) * c_ for s_, c_ in zip(stuple, ctuple))          # whole chunks per shard
    if tlast:                                               # (latitude, longitude, time): chunks and shards reordered alike
        last = lambda t: (t[1], t[2], t[0])
        _write_array(path, var, np.ascontiguousarray(cube.transpose(1, 2, 0)), ("latitude", "longitude", "time"), last(ctuple), {}, comp,
                     zarr_format, None if stuple is None else last(stuple), filters=filters or None)
    else:
        _write_array(path, var, cube, ("time", "latitude", "longitude"), ctuple, {}, comp, zarr_format, stuple, filters=filters or None)
    tv, tattrs = _encode_time(dataset.time)
    _write_array(path, "time", np.asarray(tv, dtype=np.float64), ("time",), (len(tv),), tattrs, None, zarr_format)
    _write_array(path, "latitude", dataset.latitude, ("latitude",), (len(dataset.latitude),), {}, None, zarr_format)
    _write_array(path, "longitude", dataset.longitude, ("longitude",), (len(dataset.longitude),), {}, None, zarr_format)
    return path


def zarr_from_path(src: str, dst: str, var: str, **kwargs):
    """`zarr_from_path` (`zarr_convert.py:124-156`): convert any readable source to Zarr.  ``device`` goes to `dataset_from_path`
    (the cube is read into HBM), ``encode`` with the other keywords to `dataset_to_zarr`."""
    ds_kw = {k: kwargs.pop(k) for k in ("xycoords", "timecoord", "lon_is_360", "time_sel", "device") if k in kwargs}
    ds = dataset_from_path(src, var, **ds_kw)
    return dataset_to_zarr(ds, dst, var=var, **kwargs)


# --------------------------------------------------------------------------------------
# other containers
# --------------------------------------------------------------------------------------
def _open_npz(path, var):
    z = np.load(path, allow_pickle=False)
    data = z[var] if var in z.files else z["data"]
    dims = ("time", "latitude", "longitude")
    t = z["time"]
    time = pd.DatetimeIndex(t) if t.dtype.kind == "M" else decode_cf_time(t, str(z["time_units"]), str(z["calendar"]))
    return DataArray(data, dims, {"time": time, "latitude": z["latitude"], "longitude": z["longitude"]}, name=var)


def _open_hdf5(path, var, xycoords=("longitude", "latitude"), timecoord="time", keep_packed=False):
    """netCDF-4 / HDF5 containers through the built-in reader (`hdf5.py`): variable, CF mask / scale, coordinates
    by dimension name (``DIMENSION_LIST``; for plain HDF5 files without dimension scales, by matching the axis
    lengths to the 1-D datasets named like the coordinates).  ``keep_packed``: an int16- / uint16-packed variable (`packing_of`) is
    left as stored, in a `packed.PackedCube` on the host — for variables the streaming route does not take (contiguous
    layout), whose one upload then moves 2 bytes per value."""
    from . import hdf5
    with hdf5.H5File(path) as f:
        if var not in f.datasets:
            raise KeyError(f"{var!r} not in {path}: {sorted(f.datasets)}")
        ds = f.datasets[var]
        dims = ds.dims
        if dims is None:
            cands = {n: d for n, d in f.datasets.items() if len(d.shape) == 1 and n != var}
            dims = []
            for ax, n in enumerate(ds.shape):
                names = [c for c in (timecoord, xycoords[1], xycoords[0]) if c in cands and cands[c].shape[0] == n and c not in dims]
                names += [c for c, d in cands.items() if d.shape[0] == n and c not in dims and c not in names]
                dims.append(names[0] if names else f"dim_{ax}")
            dims = tuple(dims)
        attrs = _py_attrs(ds.attrs, _H5_INTERNAL_ATTRS)
        if keep_packed and packing_of(ds) is not None:
            from .packed import PackedCube
            data = PackedCube(np.ascontiguousarray(ds.read()), *packing_of(ds))
        else:
            data = _cf_mask_scale(ds.read(), attrs)
        coords = _hdf5_coords(f, dims)
    return DataArray(data, dims, coords, name=var, attrs=attrs)


_H5_INTERNAL_ATTRS = ("DIMENSION_LIST", "REFERENCE_LIST", "CLASS", "NAME", "_Netcdf4Dimid", "_Netcdf4Coordinates")


def _hdf5_coords(f, dims) -> dict:
    """{dim: values} of the dimensions of an open `hdf5.H5File` that have a 1-D dataset of their name, the time axis decoded."""
    coords = {}
    for d in dims:
        c = f.datasets.get(d)
        if c is not None and len(c.shape) == 1:
            coords[d] = _decoded_coord(c.read(threads=1), _py_attrs(c.attrs))
    return coords


def _nc3_coords(nc, dims) -> dict:
    """{dim: values} of the dimensions of a `netcdf3.NC3File` that have a 1-D variable of their name, in native byte order, the time
    axis decoded."""
    coords = {}
    for d in dims:
        c = nc.variables.get(d)
        if c is not None and len(c.shape) == 1:
            vals = nc.read(d)
            coords[d] = _decoded_coord(vals.astype(vals.dtype.newbyteorder("=")), _py_attrs(c.attrs))
    return coords


def _open_netcdf3(path, var):
    from scipy.io import netcdf_file
    with netcdf_file(path, "r", mmap=False) as nc:
        v = nc.variables[var]
        dims = tuple(v.dimensions)
        attrs = {k: (val.decode() if isinstance(val, bytes) else val) for k, val in v._attributes.items()}
        data = _cf_mask_scale(np.array(v.data), attrs)
        coords = {}
        for d in dims:
            if d in nc.variables:
                cv = nc.variables[d]
                cattrs = {k: (val.decode() if isinstance(val, bytes) else val) for k, val in cv._attributes.items()}
                coords[d] = _decoded_coord(np.array(cv.data), cattrs)
    return DataArray(data, dims, coords, name=var, attrs=attrs)


def read_time_coordinate(path, var, timecoord="time"):
    """The decoded time coordinate of a Zarr store (or of the dimension ``timecoord`` of a netCDF-4 or NetCDF classic file, or the valid
    times of the messages of ``var`` in a GRIB file) without touching the data variable."""
    t = None
    if _looks_like_zarr(path):
        t = _zarr_coords(path, (timecoord,)).get(timecoord)
    elif _is_hdf5(path):
        from . import hdf5
        with hdf5.H5File(path) as f:
            t = _hdf5_coords(f, (timecoord,)).get(timecoord)
    elif _is_netcdf3(path):
        from . import netcdf3
        t = _nc3_coords(netcdf3.NC3File(path), (timecoord,)).get(timecoord)
    elif _is_grib(path):
        from . import grib
        return grib.open_index(path).select(var).time               # the valid times of the variable's messages, in time order
    elif _is_tiff(path):
        from . import tiff
        return tiff.TiffStack(path).time                            # a single-page file: the step its name gives
    if t is None:
        raise ValueError(f"cannot read a time coordinate from {path}")
    return t if isinstance(t, (pd.DatetimeIndex, CFTimeIndex)) else pd.DatetimeIndex(t)     # (datetime64 values stored as such)


def _clip_box(dims, coords, xycoords, georegions, lon_is_360):
    """(y0, y1, x0, x1) on the STORED axes when the clip to the regions' extent (`grid.py:150-217`) keeps one
    contiguous run along both spatial axes, else None (the clip then happens after the load)."""
    from .dataset import Grid
    xname, yname = xycoords
    if dims[1] not in (xname, yname) or dims[2] not in (xname, yname) or dims[1] == dims[2]:
        return None
    if xname not in coords or yname not in coords:
        return None
    try:
        g = Grid(np.asarray(coords[xname], dtype=float), np.asarray(coords[yname], dtype=float), lon_is_360=lon_is_360)
        inlat, inlon = g.clip_grid_to_georegions_extent(georegions)
    except (ValueError, AttributeError, TypeError):
        return None

    def run(mask):
        idx = np.nonzero(np.asarray(mask))[0]
        if len(idx) == 0 or idx[-1] - idx[0] + 1 != len(idx):
            return None
        return int(idx[0]), int(idx[-1]) + 1

    ry, rx = run(inlat), run(inlon)
    if ry is None or rx is None:
        return None
    return (ry + rx) if dims[1] == yname else (rx + ry)


def _band_of_box(dims, shape, xycoords, box, lat_window):
    """The stored-axes box (a0, a1, b0, b1) of latitude rows ``lat_window`` inside ``box`` (None = the whole grid)."""
    full = tuple(box) if box is not None else (0, int(shape[1]), 0, int(shape[2]))
    j0, j1 = int(lat_window[0]), int(lat_window[1])
    out = list(full)
    k = 0 if dims[1] == xycoords[1] else 2                          # where the latitude range sits in the box
    if not (0 <= j0 <= j1 <= full[k + 1] - full[k]):
        raise ValueError(f"lat_window {lat_window} outside the {full[k + 1] - full[k]} latitude rows of the grid")
    out[k], out[k + 1] = full[k] + j0, full[k] + j1
    return tuple(out)


class _StreamedSource:
    """One variable of one store or file that a store-to-HBM route takes — what `_streamed_source` returns and `dataset_from_path`,
    `distributed._step_bytes` and the CLI ask of it, whatever the container:

    * ``dims``, ``shape``: time-major, as the tensor will lie in HBM (a time-last Zarr array reports its transposed order);
    * ``dtype``: the stored type in native byte order; ``attrs``: the variable's attributes, Python numbers, not numpy scalars;
    * ``name``: the variable's; ``packing``: what `packing_of` says of it (None: it cannot stay packed);
    * ``coords()``: {dim: values} of the dimensions that have a coordinate, the time axis decoded;
    * ``to_device(device, window, box, keep_packed)`` -> the tensor of steps ``window`` (None: all) and stored-axes ``box`` (None:
      the whole grid), by the format's own streaming.  `ValueError`: the request is not for this route;
    * ``takes(n_parts, time_window, lat_window)``: whether the route serves such a request on ``n_parts`` stores or files at all;
    * ``host_route``: whether a `ValueError` sends the request on to the host route (a GRIB file has no other: it raises)."""

    beside_bytes = 0                # bytes per cell of a stored-type buffer that lies beside the cube while it is read
    host_route = True

    def takes(self, n_parts, time_window, lat_window) -> bool:
        return True

    def step_bytes(self, keep_packed=False) -> int:
        """Bytes one time step takes in HBM (the full stored grid: a clipped read takes less).  ``keep_packed`` (or
        AGGFLY_HIP_KEEP_PACKED=1): a variable that stays packed counts its 2 stored bytes per cell."""
        dt = np.dtype(self.dtype)
        item = dt.itemsize if dt.kind == "f" else 4           # packed integers are unpacked to float32 in HBM ...
        if self.packing is not None and keep_packed_requested(keep_packed):
            item = 2                                          # ... unless the cube stays packed
        return int(np.prod(self.shape[1:], dtype=np.int64)) * (item + self.beside_bytes)


def _resolve_request(dims, shape, coords, xycoords, timecoord, time_sel=None, time_window=None, georegions=None, lon_is_360=True,
                     lat_window=None):
    """What a request reads of a streamed source of ``dims`` / ``shape`` / ``coords``: -> (window, box), the time steps [k0, k1) and the
    stored-axes box (a0, a1, b0, b1), each None for "all of it"."""
    # a time selection on a time-leading (or time-last) array: only the chunks / steps that hold the selected steps are read (a
    # decade out of a 40-year store reads a quarter of it); one that is no contiguous run is applied by `Dataset` after the load
    window = None
    if time_window is not None:
        if not (dims and dims[0] == timecoord):
            raise ValueError("time_window needs a time-leading or a time-last array")
        window = (int(time_window[0]), int(time_window[1]))
    elif time_sel is not None and dims and dims[0] == timecoord and timecoord in coords:
        window = _time_window(coords[timecoord], time_sel)
    # a clip to the regions' extent (`dataset.py:150-175`): only the chunks / rows that touch the box are read, and only the box
    # reaches HBM; `Dataset` repeats the clip on the clipped grid (a no-op)
    box = None
    if georegions is not None and len(dims) == 3:
        box = _clip_box(dims, coords, xycoords, georegions, lon_is_360)
        if box is None and lat_window is not None:
            raise ValueError("lat_window on a non-contiguous clip goes through the host route")
    if lat_window is not None:
        box = _band_of_box(dims, shape, xycoords, box, lat_window)
    return window, box


def _cut_coords(dims, coords, window, box) -> dict:
    """``coords`` of what `_resolve_request`'s (window, box) read."""
    out = dict(coords)
    if window is not None:
        out[dims[0]] = out[dims[0]][window[0]:window[1]]
    if box is not None:
        out[dims[1]] = out[dims[1]][box[0]:box[1]]
        out[dims[2]] = out[dims[2]][box[2]:box[3]]
    return out


class _ZarrSource(_StreamedSource):
    """The array ``var`` of a Zarr store.  A time-last array (latitude, longitude, time) — what the reference's converter writes — with
    a codec the native decoder handles comes back time-major (`array_to_device(time_axis=2)`): ``dims`` / ``shape`` are those of the
    tensor in HBM, and every window is cut on them."""

    def __init__(self, path, var, xycoords, timecoord):
        self.path, self.name = path, var
        za = self.za = ZarrArray(os.path.join(path, var))
        self.tlast = (len(za.dims) == 3 and za.dims[2] == timecoord and set(za.dims[:2]) == set(xycoords) and len(set(xycoords)) == 2
                      and za.scatter_kind is not None)
        major = (lambda t: (t[2], t[0], t[1])) if self.tlast else tuple
        self.dims, self.shape, self.dtype, self.attrs, self.packing = major(za.dims), major(za.shape), za.dtype, za.attrs, packing_of(za)
        if za.elem_filters and za.stored_dtype != za.dtype:    # converting element filters: the stored elements lie beside the cube
            self.beside_bytes = za.stored_dtype.itemsize

    def coords(self):
        return _zarr_coords(self.path, self.za.dims)

    def to_device(self, device, window, box, keep_packed):
        return zarr_to_device(self.path, self.name, device=device, t_range=window, yx_box=box, keep_packed=keep_packed,
                              time_axis=2 if self.tlast else 0)[0]


class _H5Source(_StreamedSource):
    """A chunked variable of a netCDF-4 file, from its object header (`hdf5.py`), through `array_to_device` (native inflate + unshuffle,
    GPU-side placement).  The file is open only while it is read: by `_hdf5_source` for the header and the coordinates, by `to_device`
    for the chunks."""

    def __init__(self, path, ds, coords):
        self.path, self.name, self._coords = path, ds.name, coords
        self.dims, self.shape, self.dtype, self.attrs = tuple(ds.dims), tuple(ds.shape), ds.dtype, _py_attrs(ds.attrs, _H5_INTERNAL_ATTRS)
        self.packing = packing_of(self)

    def takes(self, n_parts, time_window, lat_window) -> bool:
        return n_parts == 1 and lat_window is None

    def coords(self):
        return dict(self._coords)

    def to_device(self, device, window, box, keep_packed):
        from . import hdf5
        with hdf5.H5File(self.path) as f:
            return array_to_device(hdf5.ChunkSource(f.datasets[self.name]), device=device, t_range=window, yx_box=box, keep_packed=keep_packed)[0]


def _hdf5_source(path, var, timecoord="time", any_layout=False):
    """The `_H5Source` of ``var`` when the streaming route takes it — chunked, numeric, 3-D, time-leading, with dimension scales —
    else None (contiguous, not time-leading, ...): the host route then reads the file.  ``any_layout``: a contiguous variable too,
    for its header (`distributed._step_bytes`: the host route uploads it whole, packed if asked — the same bytes per step)."""
    from . import hdf5
    with hdf5.H5File(path) as f:
        ds = f.datasets.get(var)
        if ds is None or ds.dtype is None or ds.dims is None or len(ds.shape) != 3 or ds.dims[0] != timecoord:
            return None
        return _H5Source(path, ds, _hdf5_coords(f, ds.dims)) if any_layout or ds.layout[0] == "chunked" else None


def _is_netcdf3(path) -> bool:
    from . import netcdf3
    return isinstance(path, str) and os.path.isfile(path) and netcdf3.is_classic(path)


def _netcdf3_source(path, var, timecoord="time"):
    """The `_Nc3Source` of ``var`` when the streaming route takes it — a header `netcdf3.NC3File` reads, a 3-D time-leading variable
    of type short / int / float / double — else None: the host route (scipy) then reads the file."""
    from . import netcdf3
    try:
        nc = netcdf3.NC3File(path)
    except (ValueError, OSError):
        return None
    v = nc.variables.get(var)
    if v is None or len(v.shape) != 3 or v.dims[0] != timecoord or v.dtype.str[1:] not in netcdf3.STREAMED_TYPES:
        return None
    return _Nc3Source(nc, v)


class _FileSource(_StreamedSource):
    """A variable of a file whose time steps are read as they lie in it (NetCDF classic, GRIB)."""

    def takes(self, n_parts, time_window, lat_window) -> bool:
        return n_parts == 1 or time_window is None      # (on several files it counts steps of the concatenation: the host route cuts it)

    def _steps(self, window):
        """[k_lo, k_hi) of ``window`` (None: every step).  The chunked routes clamp a window (`_ScatterJob`); a file has no step outside its own."""
        T = self.shape[0]
        if window is not None and not (0 <= window[0] <= window[1] <= T):
            raise ValueError(f"time_window {window} outside the {T} steps of {self.name!r}")
        return window if window is not None else (0, T)


class _Nc3Source(_FileSource):
    """A 3-D, time-leading short / int / float / double variable of a NetCDF classic file, from the header alone (`netcdf3.py`);
    ``var.dtype`` is big-endian as stored."""

    def __init__(self, nc, var):
        self.nc, self.var, self.name = nc, var, var.name
        self.dims, self.shape, self.dtype, self.attrs = var.dims, var.shape, var.dtype.newbyteorder("="), _py_attrs(var.attrs)
        self.packing = packing_of(self)

    def coords(self):
        return _nc3_coords(self.nc, self.dims)

    def to_device(self, device, window, box, keep_packed, threads: int = 16, slab_bytes: int = 128 << 20):
        """One classic file into HBM.  Step ``t`` of the variable is one run of big-endian bytes at
        ``plane_offset(t)``; slabs are whole time steps, a thread pool (the native reader's OpenMP team) `pread`s the rows of the
        requested box of every step into the page-locked slab, packed densely, the slab crosses PCIe as stored (2 bytes per value for int16), and one kernel
        (`hip.place_box_swapped`) reverses the bytes of every element and writes the box — the x clip included — into the cube.  The
        host never touches the data.  CF mask and unpack follow in HBM as for every other format (`_cf_in_hbm`)."""
        import torch
        from . import hip
        src, v = self, self.var
        slab_bytes = _slab_bytes(slab_bytes)
        post, need_post, out_np, wire = _cf_in_hbm(src.dtype, src.attrs)
        if keep_packed and src.packing is not None:
            need_post, out_np = False, wire
        T, NY, NX = src.shape
        k_lo, k_hi = src._steps(window)
        a0, a1, b0, b1 = box if box is not None else (0, NY, 0, NX)
        isz = src.dtype.itemsize
        step_bytes = (a1 - a0) * NX * isz                                 # the rows of the box, whole: one run of the file per step
        n = k_hi - k_lo
        slab = max(1, min(slab_bytes, 1 << 30) // max(step_bytes, 1))
        wire_t, out_t = _torch_dtype(wire), _torch_dtype(out_np)
        # integers that become floats in HBM: the kernel writes the stored type beside the cube, the conversion is the copy into it
        beside = torch.empty((min(slab, max(n, 1)), a1 - a0, b1 - b0), dtype=wire_t, device=device) if wire_t != out_t else None
        stride, first = v.step_stride, (v.plane_offset(k_lo) if n > 0 else 0) + a0 * NX * isz
        path = src.nc.path

        def read(k0, k1, out):
            # the native reader's team (`afcodec_read_packed`: pread, the ranges packed back to back): one range per step — or one for
            # the slab where the steps follow each other in the file, which the team cuts into pieces itself.  (Python threads, each
            # reading a run of steps, took 44 - 57 ms for the 8760 steps of the configs[0] cube where the team takes 18:
            # profiles/netcdf3_ingest.txt.)
            from . import codec
            if stride == step_bytes:
                locs = [(path, first + k0 * stride, (k1 - k0) * step_bytes)]
            else:
                locs = [(path, first + k * stride, step_bytes) for k in range(k0, k1)]
            _, got = codec.read_packed(locs, out[:(k1 - k0) * step_bytes], align=1, threads=threads)
            if any(int(g) != loc[2] for g, loc in zip(got, locs)):
                raise OSError(f"{path}: the file ends inside the steps {k_lo + k0}..{k_lo + k1} of {v.name!r}")

        def place(raw, dst, m):
            blk = raw.view(wire_t).view(m, a1 - a0, NX)
            into = dst if beside is None else beside[:m]
            hip.place_box_swapped(blk, into, (0, 0, b0, m, a1 - a0, b1 - b0), (0, 0, 0))
            if beside is not None:
                dst.copy_(into)

        return stream_to_device(n, (a1 - a0, b1 - b0), src.dtype, read, slab, device, post if need_post else None, out_np, wire,
                                place=place, stage_step_bytes=step_bytes)


class _GribSource(_FileSource):
    """The messages of one variable of a GRIB file in time order (`grib.Field`), from the section headers alone; ``dtype`` is float32
    and ``packing`` None (a GRIB field has no stored type to keep: every step has its own R / E / D, so ``keep_packed`` is ignored).
    Whatever `grib.py` or the unpack kernels refuse raises with its reason: a GRIB file has no other route to fall back to."""

    packing, host_route = None, False

    def __init__(self, field, xycoords, timecoord):
        self.field, self.path, self.name = field, field.path, field.var
        self.dims, self.shape, self.dtype, self.attrs = (timecoord, xycoords[1], xycoords[0]), field.shape, np.dtype(np.float32), dict(field.attrs)

    def coords(self):
        c = self.field.coords()
        return {self.dims[0]: c["time"], self.dims[1]: c["latitude"], self.dims[2]: c["longitude"]}

    def to_device(self, device, window, box, keep_packed=False, threads: int = 16, slab_bytes: int = 128 << 20):
        """One GRIB file into HBM, as `_Nc3Source.to_device` does it for a classic file.  Step ``t`` is one
        message: slabs are whole time steps, the native reader's team `pread`s the packed bits of every step — without a bitmap only the
        bytes that hold the rows of the requested box, with one the bitmap and the data section whole — into the page-locked slab, the slab
        crosses PCIe as stored (2 bytes per value for ERA5's 16 bits), and `hip.grib_unpack` extracts the integers, scales them, writes NaN
        where the bitmap has 0 and places the box — the x clip included — in the float32 cube.  The host never touches the data.  The
        steps' ``nbits`` / ``E`` / ``D`` / ``R`` differ: each step has its record, with ``R``, ``2.0 ** E`` and ``10.0 ** -D`` as the
        host route computes them.  Steps in complex packing (edition 2, templates 5.2 / 5.3) stage the whole body of their section 7 and go
        to `hip.grib_unpack_complex`, which reads the group tables, cuts the values out, undoes the spatial differencing by running sums and
        places the box; a file may mix them with simple-packed steps (a writer falls back to simple packing for a constant field).  Steps
        in CCSDS packing (template 5.42) are staged whole in the same way and go to `hip.grib_unpack_ccsds`: a walk over the block headers
        of the stream, a decode of every reference sample interval on its own, and the same placement."""
        import torch
        from . import codec, hip
        src = self
        slab_bytes = _slab_bytes(slab_bytes)
        T, NY, NX = src.shape
        k_lo, k_hi = src._steps(window)
        a0, a1, b0, b1 = box if box is not None else (0, NY, 0, NX)
        msgs = src.field.messages[k_lo:k_hi]
        n = len(msgs)
        path = src.path
        # what is staged of every step: (file offset, bytes) of the bitmap and of the packed bits, and the record that says so
        rec = np.zeros(n, dtype=hip.GRIB_STEP)
        arr = {k: v[k_lo:k_hi] for k, v in src.field.arrays().items()}
        nb, d_off, d_len, m_off = arr["nbits"], arr["data_offset"], arr["data_length"], arr["bitmap_offset"]
        has_map = m_off >= 0
        # a step in complex packing (templates 5.2 / 5.3) has no random access: its section 7 is staged whole, like a step with a bitmap.
        # kind: 0 simple packing, 1 + order complex packing (order 0: template 5.2), 4 CCSDS packing - `place` calls one entry per run of one kind
        is_cc = arr["packing"] == 42
        is_cx = (arr["packing"] != 0) & ~is_cc
        kind = np.where(is_cc, 4, np.where(is_cx, 1 + arr["order"], 0))
        whole = has_map | is_cx | is_cc
        lo = np.where(whole, 0, (a0 * NX * nb) // 8)                         # simple packing without a bitmap: the bytes of rows [a0, a1) only
        hi = np.where(whole, d_len, -((-a1 * NX * nb) // 8))
        short = hi > d_len
        if short.any():
            k = int(np.argmax(short))
            raise ValueError(f"{path}: the data section of the message at offset {msgs[k].offset} holds {int(d_len[k])} bytes, "
                             f"{NY * NX} values of {int(nb[k])} bits need {int(hi[k])}")
        map_bytes = np.where(has_map, (NY * NX + 7) // 8, 0)
        rec["nbits"], rec["first_bit"] = nb, np.where(whole, 0, (a0 * NX * nb) & 7)
        rec["first_point"], rec["data_bytes"] = np.where(whole, 0, a0 * NX), hi - lo
        rec["R"], rec["s"], rec["d"] = arr["R"], arr["s"], arr["d"]
        crec = np.zeros(n, dtype=hip.GRIB_CSTEP)                              # the records of the complex steps (unused rows for the others)
        crec["data_bytes"], crec["nbits_ref"] = d_len, nb
        for k in ("n_values", "n_groups", "ref_len", "last_len", "ref_width", "nbits_width", "len_inc", "nbits_len", "order", "extra", "R", "s", "d"):
            crec[k] = arr[k]
        max_groups = int(arr["n_groups"][is_cx].max()) if is_cx.any() else 0
        arec = np.zeros(n, dtype=hip.GRIB_ASTEP)                              # the records of the CCSDS steps (unused rows for the others)
        arec["data_bytes"], arec["nbits"], arec["flags"] = d_len, nb, arr["ccsds_flags"]
        for k in ("n_values", "block_size", "rsi", "R", "s", "d"):
            arec[k] = arr[k]
        per_rsi = np.maximum(arr["rsi"] * arr["block_size"], 1)
        max_rsis = int((-(-arr["n_values"] // per_rsi))[is_cc].max()) if is_cc.any() else 0
        pad4 = lambda v: (v + 3) // 4 * 4                                     # every staged range begins on a 4-byte boundary (`read_packed`, align=4)
        step_bytes = pad4(map_bytes) + pad4(hi - lo)
        row = int(step_bytes.max()) if n else 4
        row = max(row, 4)
        slab = max(1, min(slab_bytes, 1 << 30) // row)
        scratch = None
        if is_cx.any():
            # the scratch of the complex steps (8 bytes per value and step, 16 per group, the rank tables, the tile sums) is capped at four
            # slabs of staged bytes, and a slab holds no more steps than that serves
            per_step = hip.grib_complex_scratch_bytes(1, NY * NX, max_groups)
            slab = max(1, min(slab, (4 * min(slab_bytes, 1 << 30)) // per_step))
            scratch = torch.empty(hip.grib_complex_scratch_bytes(min(slab, n), NY * NX, max_groups), dtype=torch.uint8, device=device)
        ascratch = None
        if is_cc.any():
            # the scratch of the CCSDS steps (4 bytes per value and step, 8 per reference sample interval, the rank tables): the same cap
            per_step = hip.grib_ccsds_scratch_bytes(1, NY * NX, max_rsis)
            slab = max(1, min(slab, (4 * min(slab_bytes, 1 << 30)) // per_step))
            ascratch = torch.empty(hip.grib_ccsds_scratch_bytes(min(slab, n), NY * NX, max_rsis), dtype=torch.uint8, device=device)
        rank = torch.empty(hip.grib_rank_bytes(min(slab, max(n, 1)), NY * NX), dtype=torch.uint8, device=device)
        errors = torch.zeros(1, dtype=torch.int32, device=device)
        pending = []                                                          # the records of the slab just read, for `place`

        def read(k0, k1, out):
            # one range per staged piece, packed back to back by the reader's team; a step's ranges follow each other in the slab
            start = np.concatenate([[0], np.cumsum(step_bytes[k0:k1])])[:-1]
            r, c, a = rec[k0:k1].copy(), crec[k0:k1].copy(), arec[k0:k1].copy()
            r["bitmap_off"] = c["bitmap_off"] = a["bitmap_off"] = np.where(has_map[k0:k1], start, -1)
            r["data_off"] = c["data_off"] = a["data_off"] = start + pad4(map_bytes[k0:k1])
            # per step the bitmap, then the packed bits; pieces of no bytes (a field of 0 bits per value) are not asked for
            two = lambda a_, b_: np.stack([a_, b_], axis=1).ravel()
            keep = two(has_map[k0:k1], hi[k0:k1] > lo[k0:k1])
            src_off, nbytes = two(m_off[k0:k1], (d_off + lo)[k0:k1])[keep], two(map_bytes[k0:k1], (hi - lo)[k0:k1])[keep]
            want = two(r["bitmap_off"], r["data_off"])[keep]
            if len(want):
                locs = [(path, o, nby) for o, nby in zip(src_off.tolist(), nbytes.tolist())]
                offs, got = codec.read_packed(locs, out[:(k1 - k0) * row], align=4, threads=threads)
                if not np.array_equal(got, nbytes):
                    raise OSError(f"{path}: the file ends inside the steps {k_lo + k0}..{k_lo + k1} of {src.field.var!r}")
                if not np.array_equal(offs[:-1], want):
                    raise RuntimeError("grib: the reader packed the staged ranges differently from the records")
            pending[:] = [(r, c, a, kind[k0:k1])]

        def place(raw, dst, m):
            r, c, a, kd = pending[0]
            grid, box = (NY, NX), (a0, b0, a1 - a0, b1 - b0)
            if not kd.any():                                                  # simple packing throughout: one call, as ever
                steps = torch.from_numpy(r.view(np.uint8).reshape(-1)).to(dst.device)
                hip.grib_unpack(raw, steps, m, grid, box, dst, (0, 0, 0), rank, errors)
                return
            # runs of consecutive steps of one kind, each with its own records and its offset along time
            cuts = np.concatenate([[0], np.flatnonzero(kd[1:] != kd[:-1]) + 1, [m]])
            for i, j in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
                if kd[i] == 0:
                    steps = torch.from_numpy(r[i:j].view(np.uint8).reshape(-1)).to(dst.device)
                    hip.grib_unpack(raw, steps, j - i, grid, box, dst, (i, 0, 0), rank, errors)
                elif kd[i] == 4:
                    steps = torch.from_numpy(a[i:j].view(np.uint8).reshape(-1)).to(dst.device)
                    hip.grib_unpack_ccsds(raw, steps, j - i, max_rsis, grid, box, dst, (i, 0, 0), ascratch, errors)
                else:
                    steps = torch.from_numpy(c[i:j].view(np.uint8).reshape(-1)).to(dst.device)
                    hip.grib_unpack_complex(raw, steps, j - i, int(kd[i]) - 1, max_groups, grid, box, dst, (i, 0, 0), scratch, errors)

        data = stream_to_device(n, (a1 - a0, b1 - b0), np.float32, read, slab, device, None, np.float32, None, place=place, stage_step_bytes=row)
        if n and int(errors.item()):
            raise ValueError(f"{path}: {int(errors.item())} step(s) of {src.field.var!r} were refused by the unpack kernels (records outside the staged bytes"
                             + ("; or group tables of complex packing that are unsound: widths above 32 bits, lengths that do not sum to the number "
                                "of values, values beyond section 7 - `grib.GribFile.read` names which" if is_cx.any() else "")
                             + ("; or CCSDS streams that are damaged or end before their last sample, or bitmaps whose 1-bits are not the "
                                "number of values - `grib.GribFile.read` names which" if is_cc.any() else "") + ")")
        return data


def _is_grib(path) -> bool:
    from . import grib
    return isinstance(path, str) and os.path.isfile(path) and grib.is_grib(path)


def _grib_filter(kwargs) -> dict | None:
    """``filter_by_keys`` as cfgrib takes it: a keyword of its own, or inside ``backend_kwargs``."""
    fbk = dict((kwargs.get("backend_kwargs") or {}).get("filter_by_keys") or {})
    fbk.update(kwargs.get("filter_by_keys") or {})
    return fbk or None


def _grib_source(path, var, xycoords=("longitude", "latitude"), timecoord="time", filter_by_keys=None):
    """The `_GribSource` of ``var`` in the GRIB file ``path``.  Whatever `grib.py` refuses raises here, with its reason: a GRIB file has
    no other route to fall back to."""
    from . import grib
    return _GribSource(grib.open_index(path).select(var, filter_by_keys), xycoords, timecoord)


def _open_grib(path, var, xycoords=("longitude", "latitude"), timecoord="time", filter_by_keys=None):
    """A GRIB file on the host: the index of `grib.py` and its numpy decode (float32, NaN where a bitmap has 0)."""
    src = _grib_source(path, var, xycoords, timecoord, filter_by_keys)
    return DataArray(src.field.file.read(src.field), src.dims, src.coords(), name=var, attrs=src.attrs)


class _TiffSource(_FileSource):
    """The pages of a stack of GeoTIFF files in time order (`tiff.TiffStack`), from the image file directories alone: ONE source over
    the whole stack — 365 daily files are one stream into one cube, not 365 parts to join; every band of a multi-band page is a time
    step, so are 24 files of 365 bands.  ``dtype`` is the stored type, ``attrs`` carry
    ``_FillValue`` where the files name a nodata value, ``packing`` is None (``keep_packed`` is accepted and ignored).  Whatever
    `tiff.py` or the kernels refuse raises with its reason: a TIFF has no other route to fall back to."""

    packing, host_route = None, False

    def __init__(self, stack, var, xycoords, timecoord):
        self.stack, self.path, self.name = stack, stack.paths[0], var
        self.dims, self.shape, self.dtype, self.attrs = (timecoord, xycoords[1], xycoords[0]), stack.shape, stack.dtype, dict(stack.attrs)

    def takes(self, n_parts, time_window, lat_window) -> bool:
        return True                                     # (the stack is one source whatever the number of files: a window counts its steps)

    def coords(self):
        c = self.stack.coords()
        return {self.dims[0]: c["time"], self.dims[1]: c["latitude"], self.dims[2]: c["longitude"]}

    def to_device(self, device, window, box, keep_packed=False, threads: int = 16, slab_bytes: int = 128 << 20):
        """A TIFF stack into HBM, as `_Nc3Source.to_device` does it for a classic file.  A time step is one band of one page, and what
        is staged comes in groups: a single-band page, or one band of a planar page (PlanarConfiguration 2: single-band segments of
        its own), is a group of one step; a chunky multi-band page (PlanarConfiguration 1) is one group of all its steps the window
        holds, its segments — every band of a pixel interleaved — staged once however many bands are asked for.  Only the segments that
        touch the requested box are read.  A slab is a whole number of groups: as many as fit ``slab_bytes`` at the size of the largest
        group, and one where a page of many bands is larger than that — the staging buffers are then sized to that page.  Where the
        host team decodes, a slab holds no fewer groups than give every thread of the team a segment, up to 1 GiB of staging (the
        rule of `array_to_device` for chunks): a compressed segment is one stream and one thread's work, and a 365-band page in one
        tile would otherwise be decoded by one thread while fifteen wait (profiles/tiff_bands_ingest.txt).
        Uncompressed segments are `pread` into the page-locked slab by the native reader's team, Deflate and LZW segments are decoded
        into it by the same team (`codec.decode_ranges`, `codec.lzw_decode_ranges`); with AGGFLY_HIP_GPU_DECODE=1 the LZW streams of a
        stack that is LZW throughout cross PCIe compressed instead and `hip.lzw_decode` decodes them into a scratch in HBM, one wave
        per segment.  Then `hip.tiff_place` undoes the predictor along every segment row, swaps the bytes of a big-endian file and
        writes the box — the clip included, the padding of partial tiles dropped — into the cube, or into a buffer of the stored type
        beside it when integers become floats; the segments of chunky pages go to `hip.tiff_place_bands`, which also takes the bands
        apart — band b of a segment whose band 0 is step t goes to step t + b, and a window that begins or ends inside a page drops
        the bands outside it (t is then negative, or t + b beyond the slab).  Runs of groups that share predictor, byte order, band
        count and configuration share a launch.  CF masking of the nodata value follows in HBM as for every other format
        (`_cf_in_hbm`)."""
        import torch
        from . import codec, hip, tiff
        src = self
        slab_bytes = _slab_bytes(slab_bytes)
        post, need_post, out_np, wire = _cf_in_hbm(src.dtype, src.attrs)
        T, NY, NX = src.shape
        k_lo, k_hi = src._steps(window)
        a0, a1, b0, b1 = box if box is not None else (0, NY, 0, NX)
        n, isz = k_hi - k_lo, src.dtype.itemsize
        wire_t, out_t = _torch_dtype(wire), _torch_dtype(out_np)
        if n == 0 or a1 <= a0 or b1 <= b0:
            return torch.empty((n, max(a1 - a0, 0), max(b1 - b0, 0)), dtype=out_t, device=device)
        # the groups of the window: (page, band or -1 for a chunky page, first step, steps [g_lo, g_hi) of the window it fills)
        groups = []
        for k in range(k_lo, k_hi):
            st = src.stack.steps[k]
            if not st.page.chunky:
                groups.append((st.page, st.band, k - k_lo, k - k_lo, k - k_lo + 1))
            elif not groups or groups[-1][0] is not st.page:
                groups.append((st.page, -1, k - st.band - k_lo, k - k_lo, min(k - st.band + st.page.bands, k_hi) - k_lo))
        pages = [g[0] for g in groups]
        ng = len(groups)
        t_first = np.array([g[2] for g in groups], dtype=np.int64)            # the step of a group's band 0: negative where the window begins inside a page
        g_lo, g_hi = np.array([g[3] for g in groups], dtype=np.int64), np.array([g[4] for g in groups], dtype=np.int64)
        # the segments of every group that touch the box (groups of one layout share the list), all groups back to back
        layouts, per = {}, []
        for pg, band, *_ in groups:
            key = (pg.tiled, pg.seg_w, pg.seg_h, pg.width, pg.height, pg.bands if pg.chunky else 1)
            if key not in layouts:
                layouts[key] = pg.segments((a0, a1, b0, b1))
            g = layouts[key]
            per.append(g if band <= 0 else (g[0] + band * pg.across * pg.down,) + g[1:])
        nseg = np.array([len(g[0]) for g in per], dtype=np.int64)
        seg0 = np.concatenate([[0], np.cumsum(nseg)])
        group_of = np.repeat(np.arange(ng, dtype=np.int64), nseg)
        rec = np.zeros(int(seg0[-1]), dtype=hip.TIFF_SEG)
        for name, j in (("y", 1), ("x", 2), ("rows", 3), ("pitch", 4), ("dec_bytes", 5)):
            rec[name] = np.concatenate([g[j] for g in per])
        f_off = np.concatenate([pg.offsets[g[0]] for pg, g in zip(pages, per)])
        f_cnt = np.concatenate([pg.counts[g[0]] for pg, g in zip(pages, per)])
        kind = np.repeat(np.array([0 if pg.compression == tiff.COMPRESSION_NONE else 1 if pg.compression == tiff.COMPRESSION_LZW else 2
                                   for pg in pages]), nseg)               # 0 as stored, 1 LZW, 2 Deflate
        f_cnt = np.where(kind == 0, rec["dec_bytes"], f_cnt)                # (an uncompressed segment: the bytes of its samples, no more)
        # per group: predictor, swap, the bands of a chunky page (0: single-band segments)
        undo = np.array([(pg.predictor, pg.byteorder == ">" and isz > 1, pg.bands if pg.chunky else 0) for pg in pages], dtype=np.int64)
        paths = [pg.path for pg in pages]
        file_of = np.unique(np.array(paths), return_inverse=True)[1]          # per group: which file
        max_rows = int(rec["rows"].max())
        in_hbm = bool((kind == 1).all()) and os.environ.get("AGGFLY_HIP_GPU_DECODE", "auto") == "1"    # (GPU_DECODE_AUTO_BYTES_LZW is None: opt-in)
        staged = f_cnt if in_hbm else rec["dec_bytes"]                      # what a segment takes in the slab
        per_group = lambda v: np.add.reduceat(v, seg0[:-1])                 # (every group has a segment: the box is not empty)
        row = int(-(-int(per_group(staged).max()) // 8) * 8)
        dec_row = int(per_group(rec["dec_bytes"]).max())
        slab = max(1, min(slab_bytes, 1 << 30) // max(row, 1))              # groups to a slab
        if in_hbm:
            slab = max(1, min(slab, (4 * min(slab_bytes, 1 << 30)) // max(dec_row, 1)))     # the decoded scratch: at most four slabs of staged bytes
        elif kind.any():
            slab = max(slab, min(-(-threads // int(nseg.min())), (1 << 30) // max(row, 1)))     # a segment for every thread of the team
        slab = min(slab, ng)
        cut = list(range(0, ng, slab)) + [ng]
        slabs = [(int(g_lo[i]), int(g_hi[j - 1]), (j - i) * row) for i, j in zip(cut[:-1], cut[1:])]
        groups_of_slab = {int(g_lo[i]): (i, j) for i, j in zip(cut[:-1], cut[1:])}
        m_max = max(k1 - k0 for k0, k1, _ in slabs)
        decoded = torch.empty(slab * dec_row, dtype=torch.uint8, device=device) if in_hbm else None
        # integers that become floats in HBM: the kernel writes the stored type beside the cube, the conversion is the copy into it
        beside = torch.empty((m_max, a1 - a0, b1 - b0), dtype=wire_t, device=device) if wire_t != out_t else None
        errors = torch.zeros(1, dtype=torch.int32, device=device)
        pending = []                                                        # the records of the slab just read, for `place`

        def read(k0, k1, out):
            i0, i1 = groups_of_slab[k0]
            s0, s1 = int(seg0[i0]), int(seg0[i1])
            r = rec[s0:s1].copy()
            r["t"] = t_first[group_of[s0:s1]] - k0
            r["dec_off"] = np.cumsum(r["dec_bytes"]) - r["dec_bytes"]
            size = staged[s0:s1]
            at = np.cumsum(size) - size                                      # where a segment's staged bytes begin in the slab
            st, fo, fc, kd = group_of[s0:s1], f_off[s0:s1], f_cnt[s0:s1], kind[s0:s1]
            try:
                if in_hbm or not kd.any():
                    # bytes as they lie in the files, packed back to back by the reader's team: compressed streams, or stored samples.
                    # Segments that follow each other in one file — the strips of a page, as a rule — are one range
                    r["src_off"], r["src_bytes"] = at, size
                    head = np.ones(len(fo), dtype=bool)
                    head[1:] = (file_of[st[1:]] != file_of[st[:-1]]) | (fo[1:] != fo[:-1] + fc[:-1])
                    head = np.flatnonzero(head)
                    runs = np.add.reduceat(fc, head)
                    locs = [(paths[t], o, c) for t, o, c in zip(st[head].tolist(), fo[head].tolist(), runs.tolist())]
                    offs, got = codec.read_packed(locs, out, align=1, threads=threads)
                    if not np.array_equal(got, runs):
                        raise OSError(f"{src.path}: a file ends inside the steps {k_lo + k0}..{k_lo + k1} of the stack")
                else:
                    locs = [(paths[t], o, c) for t, o, c in zip(st.tolist(), fo.tolist(), fc.tolist())]
                    bufs = [out[a:a + c] for a, c in zip(at.tolist(), size.tolist())]
                    for code, decode in ((0, lambda l, b: codec.decode_ranges("raw", l, b, threads=threads)),
                                         (1, lambda l, b: codec.lzw_decode_ranges(l, b, threads=threads)),
                                         (2, lambda l, b: codec.decode_ranges("zlib", l, b, threads=threads))):
                        idx = np.flatnonzero(kd == code).tolist()
                        if idx:
                            decode([locs[i] for i in idx], [bufs[i] for i in idx])
            except codec.CodecError as e:
                raise ValueError(f"{src.path}: steps {k_lo + k0}..{k_lo + k1} of the stack: {e}") from None
            pending[:] = [(r, undo[i0:i1], seg0[i0:i1 + 1] - s0)]

        def place(raw, dst, m):
            r, un, first = pending[0]
            into = dst if beside is None else beside[:m]
            recs = torch.from_numpy(r.view(np.uint8).reshape(-1)).to(dst.device)
            if in_hbm:
                hip.lzw_decode(raw, recs, len(r), decoded, errors)
            # runs of consecutive groups of one predictor, byte order, band count and configuration (one, as a rule), each with its records
            cuts = np.concatenate([[0], np.flatnonzero((un[1:] != un[:-1]).any(axis=1)) + 1, [len(un)]])
            for i, lo, hi in zip(cuts[:-1].tolist(), first[cuts[:-1]].tolist(), first[cuts[1:]].tolist()):
                some = recs[lo * hip.TIFF_SEG.itemsize:hi * hip.TIFF_SEG.itemsize]
                args = (int(un[i, 0]), bool(un[i, 1]), into, (a0, b0, a1 - a0, b1 - b0), (0, 0, 0), errors)
                if un[i, 2]:
                    hip.tiff_place_bands(decoded if in_hbm else raw, some, hi - lo, max_rows, int(un[i, 2]), *args)
                else:
                    hip.tiff_place(decoded if in_hbm else raw, some, hi - lo, max_rows, *args)
            if beside is not None:
                dst.copy_(into)

        data = stream_to_device(n, (a1 - a0, b1 - b0), src.dtype, read, m_max, device, post if need_post else None, out_np, wire,
                                place=place, stage_step_bytes=row, slabs=slabs)
        if int(errors.item()):
            raise ValueError(f"{src.path}: {int(errors.item())} segment(s) of the stack were refused by the kernels (LZW streams that are damaged or end "
                             "before their decoded size; AGGFLY_HIP_GPU_DECODE=0 decodes on the host and names them)")
        return data


def _is_tiff(path) -> bool:
    from . import tiff
    return isinstance(path, str) and os.path.isfile(path) and tiff.is_tiff(path)


def _tiff_source(paths, var, xycoords=("longitude", "latitude"), timecoord="time", tiff_time=None):
    """The `_TiffSource` of the stack of the TIFF files ``paths`` (one path, or several in time order).  Whatever `tiff.py` refuses
    raises here, with its reason."""
    from . import tiff
    return _TiffSource(tiff.TiffStack(paths, tiff_time), var, xycoords, timecoord)


def _open_tiff(paths, var, xycoords=("longitude", "latitude"), timecoord="time", tiff_time=None):
    """A TIFF stack on the host: the directories of `tiff.py`, the codec library's decode and numpy's predictors (`TiffStack.read`)."""
    src = _tiff_source(paths, var, xycoords, timecoord, tiff_time)
    return DataArray(src.stack.read(), src.dims, src.coords(), name=var, attrs=src.attrs)


def _streamed_source(path, var, xycoords=("longitude", "latitude"), timecoord="time", engine=None, filter_by_keys=None, tiff_time=None):
    """The `_StreamedSource` of ``var`` in the store or file ``path`` — the one probe of `dataset_from_path`, `distributed._step_bytes`
    and the CLI — or None when no streaming route takes it.  ``engine``: the reader `dataset_from_path` was asked for, which narrows
    the formats looked for.  A Zarr store or a classic file that cannot be read gives None (the host route then says why), a GRIB file
    that `grib.py` refuses raises with its reason, and so does a TIFF file that `tiff.py` refuses (``path`` may be the list of a stack's files:
    they are one source)."""
    if engine == "zarr" or (engine is None and _looks_like_zarr(path)):
        try:
            return _ZarrSource(path, var, xycoords, timecoord)
        except ValueError:
            return None
    if engine in (None, "netcdf4", "h5netcdf") and _is_hdf5(path):
        return _hdf5_source(path, var, timecoord)
    if engine in (None, "scipy") and _is_netcdf3(path):
        return _netcdf3_source(path, var, timecoord)
    if engine in (None, "cfgrib") and _is_grib(path):
        return _grib_source(path, var, xycoords, timecoord, filter_by_keys)
    if engine in (None, "rasterio") and all(_is_tiff(p) for p in (path if isinstance(path, (list, tuple)) else [path])):
        return _tiff_source(path, var, xycoords, timecoord, tiff_time)
    return None


def _part_to_device(src, device, xycoords, timecoord, keep_packed=False, **request):
    """One streamed source into HBM: -> (tensor, source, coords), tensor and coordinates cut to ``request`` (the ``time_sel``,
    ``time_window``, ``georegions``, ``lon_is_360`` and ``lat_window`` of `dataset_from_path`; `_resolve_request`)."""
    coords = src.coords()
    window, box = _resolve_request(src.dims, src.shape, coords, xycoords, timecoord, **request)
    return src.to_device(device, window, box, keep_packed), src, _cut_coords(src.dims, coords, window, box)


def _concat_time(times):
    """The time coordinates of the parts of a multi-file dataset as one index, on a CF calendar (`CFTimeIndex`) as on the standard one."""
    if isinstance(times[0], CFTimeIndex):
        return CFTimeIndex(np.concatenate([t.seconds for t in times]), times[0].calendar)
    return pd.DatetimeIndex(np.concatenate([np.asarray(t) for t in times]))


def _join_device_parts(got, rules, timecoord):
    """(data, source, coords) of a dataset streamed part by part — [(tensor, source, coords)], one per store or file in time order —,
    concatenated along time like open_mfdataset.  ``rules``: the parts' unpack rules when they stayed packed (`packed_rules_of`), else None."""
    if len(got) == 1:
        data, src, coords = got[0]
        if rules is not None:
            from .packed import PackedCube
            data = PackedCube(data, *rules[0])
        return data, src, coords
    import torch
    if any(g[1].dims != got[0][1].dims or g[1].dims[0] != timecoord for g in got):
        raise ValueError("stores of a multi-file dataset must share their (time-leading) dimensions")
    coords = dict(got[0][2])
    coords[timecoord] = _concat_time([g[2][timecoord] for g in got])
    if rules is not None:                  # (the parts were cut by time_window / time_sel already: the bounds are those of what was read)
        from .packed import PackedCube
        data = PackedCube.concat([PackedCube(g[0], *r) for g, r in zip(got, rules)])
    else:
        data = torch.cat([g[0] for g in got], dim=0)
    return data, got[0][1], coords


def _is_hdf5(path) -> bool:
    from . import hdf5
    return isinstance(path, str) and os.path.isfile(path) and hdf5.is_hdf5(path)


def _time_window(tindex, time_sel):
    """(k0, k1) when ``time_sel`` (as `Dataset` applies it, `dataset.py:88-92`) picks one contiguous run of an
    ascending time index, else None (the selection is then applied after the load)."""
    n = len(tindex)
    try:
        if isinstance(tindex, pd.DatetimeIndex):
            if not tindex.is_monotonic_increasing:
                return None
            loc = tindex.slice_indexer(time_sel.start, time_sel.stop) if isinstance(time_sel, slice) else tindex.get_loc(time_sel)
            if isinstance(loc, (int, np.integer)):
                return int(loc), int(loc) + 1
            if isinstance(loc, slice) and loc.step in (None, 1):
                k0, k1, _ = loc.indices(n)
                return (k0, k1) if k1 > k0 else (0, 0)          # nothing selected in this store: nothing is read
            return None
        idx = tindex.sel_positions(time_sel)             # the exact selection `Dataset(time_sel=)` applies on a CF calendar
        if len(idx) == 0:
            return 0, 0
        if idx[-1] - idx[0] + 1 == len(idx):
            return int(idx[0]), int(idx[-1]) + 1
    except (KeyError, TypeError, ValueError, AttributeError):
        pass
    return None


def dataset_from_path(path, var, xycoords=("longitude", "latitude"), timecoord="time", time_sel=None,
                      georegions=None, lon_is_360=True, time_fix=False, preprocess=None, name=None,
                      chunks=None, preprocess_at_load=False, parallel=True, device=None, time_window=None, lat_window=None,
                      keep_packed=False, **kwargs) -> Dataset:
    """`dataset_from_path` (`dataset.py:636-740`), same signature.  ``chunks`` / ``parallel``
    are accepted and ignored (there is no dask graph); a list / glob of paths is concatenated
    along time like ``open_mfdataset``.  ``device="cuda"`` (extension) streams a single float
    Zarr array straight into HBM (``zarr_to_device``) and applies ``preprocess`` there; ``time_window=(k0, k1)``
    (extension, streaming route only) restricts the read to those time steps — what a rank of a time-sharded
    job asks for (`distributed.aggregate_store_sharded`); ``lat_window=(j0, j1)`` (extension) keeps rows ``j0..j1`` of the
    latitude axis AFTER the clip to the regions' extent — the band of a cell-sharded job
    (`distributed.aggregate_store_cells`); on the streaming route only the chunks that touch the band are read.
    ``keep_packed=True`` (extension; or AGGFLY_HIP_KEEP_PACKED=1): an int16- or uint16-packed variable (``scale_factor`` / ``add_offset`` /
    ``_FillValue``; int16 under ``_Unsigned = "true"`` counts as uint16) stays packed in HBM as a `packed.PackedCube` — half the memory, half the bytes the temporal kernel reads — and
    ``preprocess`` folds into its unpack rule.  Honoured on the streaming routes (``device=``) only, for 16-bit integer storage.  Several Zarr
    stores — yearly or monthly ERA5 files, each with its own ``scale_factor`` / ``add_offset`` / ``_FillValue`` — stay packed too: the cube
    carries one unpack rule per store along time (``PackedCube.rules``; stores of one packing share one rule) and the kernel picks the rule per
    time step.  They take the float32 route only when a store has no packing or int16 stands beside uint16 storage; ``Dataset.is_packed``
    tells which route was taken."""
    import glob
    keep_packed = keep_packed_requested(keep_packed)
    if isinstance(path, str) and "://" in path:
        raise ImportError(f"remote stores ({path.split('://')[0]}://) need fsspec backends that are not available here")
    paths = sorted(glob.glob(path)) if isinstance(path, str) and "*" in path else (list(path) if isinstance(path, (list, tuple)) else [path])
    if not paths:
        raise FileNotFoundError(path)
    engine, grib_filter, tiff_time = kwargs.pop("engine", None), _grib_filter(kwargs), kwargs.get("tiff_time")
    # the files of a TIFF stack — one raster per day or month — are ONE source and one stream into one cube, not a part per file
    tiffs = engine in (None, "rasterio") and all(_is_tiff(p) for p in paths)
    if tiffs:
        paths = [list(paths)]
    first = _streamed_source(paths[0], var, xycoords, timecoord, engine, grib_filter, tiff_time) if device is not None else None
    if first is not None and first.takes(len(paths), time_window, lat_window):
        # the streaming routes (`_StreamedSource`): every store or file is probed and streamed into HBM under the same request, the parts
        # are joined along time.  Several — yearly or monthly, each with its own packing — stay packed when each has a packing and all
        # share their signedness: one unpack rule per part.  A `ValueError` on the way sends the request on to the host route below —
        # but for GRIB files, which have no other
        got = None
        srcs = [first] + [_streamed_source(p, var, xycoords, timecoord, engine, grib_filter) for p in paths[1:]]
        if all(type(s_) is type(first) for s_ in srcs):
            rules = packed_rules_of([s_.packing for s_ in srcs]) if keep_packed else None
            try:
                got = _join_device_parts([_part_to_device(s_, device, xycoords, timecoord, rules is not None, time_sel=time_sel,
                                                          time_window=time_window, georegions=georegions, lon_is_360=lon_is_360,
                                                          lat_window=lat_window) for s_ in srcs], rules, timecoord)
            except ValueError:
                if not first.host_route:
                    raise
        if got is not None:
            data, src, coords = got
            da = DataArray(data, src.dims, coords, name=var, attrs=src.attrs)
            # a band was cut out of the already clipped box: the clip is not repeated on the band's own grid
            return Dataset(da, xycoords=xycoords, timecoord=timecoord, time_sel=time_sel, lon_is_360=lon_is_360,
                           preprocess=preprocess, georegions=None if lat_window is not None else georegions, time_fix=time_fix, name=name)
    parts = []
    for p in paths:
        if tiffs:
            da = _open_tiff(p, var, xycoords, timecoord, tiff_time)
        elif engine == "zarr" or (engine is None and _looks_like_zarr(p)):
            da = open_zarr(p, var)
        elif p.endswith(".npz"):
            da = _open_npz(p, var)
        elif _is_hdf5(p):
            # (a packed variable outside the streaming route stays packed for its one upload: a single file bound for a device)
            da = _open_hdf5(p, var, xycoords, timecoord, keep_packed=keep_packed and device is not None and len(paths) == 1)
        elif engine == "cfgrib" or _is_grib(p):
            da = _open_grib(p, var, xycoords, timecoord, grib_filter)
        else:
            da = _open_netcdf3(p, var)
        if preprocess is not None and (preprocess_at_load or len(paths) > 1):
            da = preprocess(da)
        parts.append(da)
    if len(parts) > 1:
        tdim = timecoord
        ax = parts[0].dims.index(tdim)
        data = np.concatenate([p_.values for p_ in parts], axis=ax)
        coords = dict(parts[0].coords)
        coords[tdim] = _concat_time([p_.coords[tdim] for p_ in parts])
        da = DataArray(data, parts[0].dims, coords, name=var)
        preprocess = None
    else:
        da = parts[0]
        if preprocess_at_load:
            preprocess = None
    if time_window is not None:                                     # the streaming route was not taken: cut on the host
        da = da.isel(**{timecoord: slice(int(time_window[0]), int(time_window[1]))})
    ds = Dataset(da, xycoords=xycoords, timecoord=timecoord, time_sel=time_sel, lon_is_360=lon_is_360,
                 preprocess=preprocess, georegions=georegions, time_fix=time_fix, name=name)
    if lat_window is not None:                                      # the streaming route was not taken: cut on the host
        ds.da = ds.da.isel(latitude=slice(int(lat_window[0]), int(lat_window[1])))
        ds.grid = Grid(ds.longitude, ds.latitude, ds.name, ds.lon_is_360)
    return ds.to_device(device) if device is not None else ds      # containers without a streaming route: one upload
