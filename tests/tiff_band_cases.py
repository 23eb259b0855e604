"""An independent writer of multi-band TIFF files — a band per time step — and the catalogue the band tests share.  Nothing here imports
the package: the container is written from the TIFF 6.0 specification, the predictors at a stride of SamplesPerPixel from libtiff's
tif_predict.c, in numpy; the LZW encoder, `compress`, `geo_tags` and `field` are tests/tiff_cases.py's.

    chunky (PlanarConfiguration 1): a segment holds rows x pitch x B samples, the B samples of a pixel together
    planar (PlanarConfiguration 2): B x across x down single-band segments, those of band b at b * across * down + k
"""
from __future__ import annotations

import os
import struct
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_cases as TC  # noqa: E402

H0, W0 = TC.H0, TC.W0
_TYPE_FMT = {1: "B", 2: "s", 3: "H", 4: "I", 11: "f", 12: "d", 16: "Q"}


# ---- predictors (forward), at a stride of B samples ----
def apply_band_predictor(a: np.ndarray, predictor: int, byteorder: str) -> bytes:
    """(rows, pitch, B) native samples of a chunky segment -> the bytes a writer hands to the compressor."""
    rows, pitch, B = a.shape
    E = a.dtype.itemsize
    if predictor == 3:
        # the row's samples as big-endian bytes, regrouped into E planes of pitch * B bytes (most significant first), then every byte
        # but the first B replaced by its difference from the byte B before it — across the planes' borders too
        b = np.ascontiguousarray(a.astype(a.dtype.newbyteorder(">"))).view(np.uint8).reshape(rows, pitch * B, E)
        planes = np.ascontiguousarray(b.transpose(0, 2, 1)).reshape(rows, E * pitch * B)
        d = planes.copy()
        d[:, B:] = planes[:, B:] - planes[:, :-B]
        return d.tobytes()
    if predictor == 2:
        u = np.ascontiguousarray(a).view(np.dtype(f"u{E}"))
        d = u.copy()
        d[:, 1:, :] = u[:, 1:, :] - u[:, :-1, :]
        a = d
    return np.ascontiguousarray(a.astype(a.dtype.newbyteorder(byteorder))).tobytes()


def gdal_metadata(descriptions) -> bytes:
    """The GDAL_METADATA tag (42112) of a file whose bands carry ``descriptions`` (None: that band has none), as GDAL writes it."""
    items = "".join(f'  <Item name="DESCRIPTION" sample="{k}" role="description">{d}</Item>\n' for k, d in enumerate(descriptions) if d is not None)
    return ("<GDALMetadata>\n" + '  <Item name="AREA_OR_POINT">Area</Item>\n' + items + "</GDALMetadata>\n").encode() + b"\0"


def band_page(array, planar=1, compression=1, predictor=1, tile=None, rows_per_strip=None, nodata=None, descriptions=None, extra=False,
              tags=None, junk_seed=11, geo=None, deflate_level=6):
    """One page of `write_band_tiff`: ``array`` (B, H, W); ``planar`` 1 (chunky) or 2; ``descriptions``: one text (or None) per band;
    ``extra``: an ExtraSamples tag for every band beyond those of the photometric interpretation; ``tags``: {tag: (type, values) or None} that replace or remove; ``geo``: the tags
    of another grid than `tiff_cases.geo_tags`'s default."""
    return dict(array=np.ascontiguousarray(array), planar=planar, compression=compression, predictor=predictor, tile=tile,
                rows_per_strip=rows_per_strip, nodata=nodata, descriptions=descriptions, extra=extra, tags=dict(tags or {}), junk_seed=junk_seed,
                geo=geo, deflate_level=deflate_level)


def _segments(pg):
    """[(rows, pitch[, B]) arrays] in the order of the offsets: chunky segments hold all bands; planar ones band by band."""
    a = pg["array"]
    B, H, W = a.shape
    E = a.dtype.itemsize
    if pg["tile"]:
        tw, th = pg["tile"]
        PH, PW = -(-H // th) * th, -(-W // tw) * tw
        rng = np.random.default_rng(pg["junk_seed"])
        padded = rng.integers(0, 256, B * PH * PW * E, dtype=np.uint8).view(a.dtype).reshape(B, PH, PW).copy()          # junk in the padding
        if a.dtype.kind == "f":
            padded = np.nan_to_num(padded, nan=1.5, posinf=2.5, neginf=-2.5)
        padded[:, :H, :W] = a
        cut = [(slice(y, y + th), slice(x, x + tw)) for y in range(0, PH, th) for x in range(0, PW, tw)]
        a = padded
    else:
        rps = pg["rows_per_strip"] or H
        cut = [(slice(y, min(y + rps, H)), slice(0, W)) for y in range(0, H, rps)]
    if pg["planar"] == 2:
        return [a[b][ys, xs] for b in range(B) for ys, xs in cut]
    return [np.ascontiguousarray(a[:, ys, xs].transpose(1, 2, 0)) for ys, xs in cut]


def write_band_tiff(path, pages, byteorder="<", bigtiff=False):
    bo = byteorder
    buf = bytearray()
    if bigtiff:
        buf += (b"II" if bo == "<" else b"MM") + struct.pack(bo + "HHHQ", 43, 8, 0, 0)
        ptr_at, ow, of, cf, otype = 8, 8, "Q", "Q", 16
    else:
        buf += (b"II" if bo == "<" else b"MM") + struct.pack(bo + "HI", 42, 0)
        ptr_at, ow, of, cf, otype = 4, 4, "I", "H", 4

    def align():
        while len(buf) % 8:
            buf.append(0)

    for pg in pages:
        a = pg["array"]
        B, H, W = a.shape
        E = a.dtype.itemsize
        fmt = {"u": 1, "i": 2, "f": 3}[a.dtype.kind]
        offsets, counts = [], []
        for s in _segments(pg):
            raw = apply_band_predictor(s, pg["predictor"], bo) if s.ndim == 3 else TC.apply_predictor(np.ascontiguousarray(s), pg["predictor"], bo)
            data = zlib.compress(raw, pg["deflate_level"]) if pg["compression"] == 8 else TC.compress(raw, pg["compression"])
            align()
            offsets.append(len(buf))
            counts.append(len(data))
            buf += data
        tags = {254: (4, [0]), 256: (4, [W]), 257: (4, [H]), 258: (3, [8 * E] * B), 259: (3, [pg["compression"]]),
                262: (3, [2 if B >= 3 else 1]),                               # three bands and more: RGB, the rest extra samples (readers ignore both)
                277: (3, [B]), 284: (3, [pg["planar"]]), 339: (3, [fmt] * B)}
        if pg["predictor"] != 1:
            tags[317] = (3, [pg["predictor"]])
        if pg["tile"]:
            tags.update({322: (4, [pg["tile"][0]]), 323: (4, [pg["tile"][1]]), 324: (otype, offsets), 325: (4, counts)})
        else:
            tags.update({278: (4, [pg["rows_per_strip"] or H]), 273: (otype, offsets), 279: (4, counts)})
        tags.update(pg["geo"] or TC.geo_tags())
        if pg["extra"] and B > 1:
            tags[338] = (3, [2] * (B - (3 if B >= 3 else 1)))                 # (2: unassociated alpha)
        if pg["descriptions"] is not None:
            tags[42112] = (2, gdal_metadata(pg["descriptions"]))
        if pg["nodata"] is not None:
            tags[42113] = (2, str(pg["nodata"]).encode() + b"\0")
        for t, v in pg["tags"].items():
            if v is None:
                tags.pop(t, None)
            else:
                tags[t] = v
        entries = bytearray()
        for t in sorted(tags):
            typ, vals = tags[t]
            if typ == 2:
                raw, count = bytes(vals), len(vals)
            else:
                raw, count = struct.pack(bo + str(len(vals)) + _TYPE_FMT[typ], *vals), len(vals)
            if len(raw) <= ow:
                value = raw + b"\0" * (ow - len(raw))
            else:
                align()
                value = struct.pack(bo + of, len(buf))
                buf += raw
            entries += struct.pack(bo + "HH" + of, t, typ, count) + value
        align()
        struct.pack_into(bo + of, buf, ptr_at, len(buf))
        buf += struct.pack(bo + cf, len(tags)) + entries
        ptr_at = len(buf)
        buf += struct.pack(bo + of, 0)
    with open(path, "wb") as f:
        f.write(buf)
    return path


# ---- the catalogue ----
def field(dtype, n, seed=0, nodata=None, height=H0, width=W0):
    """`tiff_cases.field` for any number of steps (it makes seven at the most): runs of seven, each shifted in x by its number so
    that no two bands are alike."""
    return np.concatenate([np.roll(TC.field(dtype, min(7, n - i), height=height, width=width, seed=seed + i, nodata=nodata), i, axis=2)
                           for i in range(0, n, 7)])


def days(n, start="2020-01-01"):
    return list(np.datetime64(start) + np.arange(n))


def band_catalogue():
    """[dict(name, files=[(file name, [page, ...], byteorder, bigtiff)], values (T, H, W), nodata, tiff_time or None (the band
    descriptions give the time), times)]: every band of every page is a step, in file, page and band order."""
    cases = []

    def add(name, a, files, nodata=None, tiff_time="days", times=None):
        times = days(len(a)) if times is None else times
        cases.append(dict(name=name, values=a, files=files, nodata=nodata, tiff_time=times if tiff_time == "days" else tiff_time, times=times))

    def one(a, bo="<", big=False, **kw):
        return [("bands.tif", [band_page(a, **kw)], bo, big)]

    k = 0
    # chunky, few bands: B x type x predictor x compression x layout, rotating through byte order and container
    few = [(2, "u1", 2, 5), (3, "u2", 2, 8), (4, "i4", 2, 5), (3, "f4", 3, 8), (2, "f8", 3, 5), (3, "i8", 2, 8), (12, "f4", 3, 8), (12, "u2", 2, 5),
           (4, "f4", 1, 1), (3, "u1", 1, 8), (2, "f4", 3, 5)]
    for B, dt, pred, comp in few:
        for tile in (None, (16, 16)):
            k += 1
            bo, big = ("<", ">")[k % 2], (k % 4) >= 2
            a = field(dt, B, seed=200 + k)
            add(f"chunky B{B} {dt} pred{pred} comp{comp} {'tiles' if tile else 'strips'} {'MM' if bo == '>' else 'II'}{' BigTIFF' if big else ''}", a,
                one(a, bo, big, planar=1, compression=comp, predictor=pred, tile=tile, rows_per_strip=None if tile else 5, extra=(k % 3 == 0)))
    # what Pillow's libtiff reads back: RGB, and RGB with one extra sample
    a = field("u1", 3, seed=280)
    add("chunky B3 u1 pred2 comp5 tiles II rgb", a, one(a, planar=1, compression=5, predictor=2, tile=(16, 16)))
    a = field("u1", 4, seed=281)
    add("chunky B4 u1 pred2 comp8 strips II rgb extra", a, one(a, planar=1, compression=8, predictor=2, rows_per_strip=5, extra=True))
    # past one wave's lanes: 70 bands (Deflate: the Python LZW encoder is slow on 700 KB)
    for dt, pred, tile, bo in (("f4", 3, (16, 16), "<"), ("u2", 2, None, ">"), ("f8", 3, None, "<"), ("u1", 2, (16, 16), "<")):
        k += 1
        a = field(dt, 70, seed=200 + k)
        add(f"chunky B70 {dt} pred{pred} comp8 {'tiles' if tile else 'strips'} {'MM' if bo == '>' else 'II'}", a,
            one(a, bo, False, planar=1, compression=8, predictor=pred, tile=tile, rows_per_strip=None if tile else 5))
    # planar
    for B, dt, pred, comp, tile, bo in ((3, "f4", 3, 5, (16, 16), "<"), (4, "u2", 2, 8, None, ">"), (12, "i4", 2, 8, (16, 16), "<"), (2, "f8", 1, 1, None, ">"),
                                        (70, "f4", 3, 8, None, "<")):
        k += 1
        a = field(dt, B, seed=200 + k)
        add(f"planar B{B} {dt} pred{pred} comp{comp} {'tiles' if tile else 'strips'} {'MM' if bo == '>' else 'II'}", a,
            one(a, bo, k % 2 == 0, planar=2, compression=comp, predictor=pred, tile=tile, rows_per_strip=None if tile else 5))
    # two pages x three bands; two files with 3 and 4 bands; one chunky file beside one planar file
    a = field("f4", 6, seed=290)
    add("two pages x three bands chunky f4 pred3", a,
        [("pages.tif", [band_page(a[:3], compression=5, predictor=3, tile=(16, 16)), band_page(a[3:], compression=5, predictor=3, tile=(16, 16))], "<", False)])
    a = field("i2", 7, seed=291, nodata=-32768)
    add("two files of 3 and 4 bands i2 nodata", a,
        [("y2001.tif", [band_page(a[:3], compression=8, predictor=2, rows_per_strip=5, nodata="-32768")], "<", False),
         ("y2002.tif", [band_page(a[3:], compression=8, predictor=2, rows_per_strip=5, nodata="-32768")], "<", False)], nodata=-32768)
    a = field("f4", 7, seed=292, nodata=-9999.0)
    add("chunky file beside planar file f4 nodata", a,
        [("a_chunky.tif", [band_page(a[:3], planar=1, compression=5, predictor=3, tile=(16, 16), nodata="-9999")], "<", False),
         ("b_planar.tif", [band_page(a[3:], planar=2, compression=8, predictor=3, rows_per_strip=5, nodata="-9999")], ">", False)], nodata=-9999.0)
    a = field("u1", 5, seed=293, nodata=255)
    add("chunky B5 u1 nodata 255 lzw", a, one(a, planar=1, compression=5, predictor=2, tile=(16, 16), nodata="255"), nodata=255)
    # the time from the band descriptions of GDAL_METADATA (no tiff_time): Earth Engine's toBands() names, GDAL's free text
    a = field("f4", 4, seed=294)
    t4 = [np.datetime64(d) for d in ("2019-12-30", "2019-12-31", "2020-01-01", "2020-01-02")]
    add("descriptions give the time chunky", a,
        one(a, compression=8, predictor=3, tile=(16, 16), descriptions=["20191230_tmean", "20191231_tmean", "20200101_tmean", "20200102_tmean"]),
        tiff_time=None, times=t4)
    add("descriptions give the time planar", a,
        one(a, planar=2, compression=5, predictor=3, rows_per_strip=5,
            descriptions=["tmean 2019-12-30", "tmean 2019-12-31 &amp; more", "tmean 2020-01-01", "tmean 2020-01-02"]), tiff_time=None, times=t4)
    return cases


def write_case(case, directory):
    os.makedirs(directory, exist_ok=True)
    return [write_band_tiff(os.path.join(directory, fn), pages, bo, big) for fn, pages, bo, big in case["files"]]


def as_single_pages(case, directory):
    """The same values one page per step in one multi-page file, by tests/tiff_cases.py's writer."""
    os.makedirs(directory, exist_ok=True)
    pred = 3 if case["values"].dtype.kind == "f" else 2
    nod = None if case["nodata"] is None else str(int(case["nodata"]) if float(case["nodata"]).is_integer() else case["nodata"])
    return TC.write_tiff(os.path.join(directory, "single.tif"),
                         [TC.page(v, compression=8, predictor=pred, tile=(16, 16), nodata=nod) for v in case["values"]])
