"""Header reader for GeoTIFF stacks — one single-band raster per day or month, one multi-page file, or files with a band per time step:
how PRISM, CHIRPS, WorldClim, Daymet mosaics and Earth Engine exports arrive —, written from the TIFF 6.0 specification, the BigTIFF
design note and the GeoTIFF specification (OGC 19-008r4).  It tells where the bytes of every strip or tile of every page lie in the
files; no pixel is touched here.  `io._TiffSource.to_device` `pread`s those bytes into page-locked memory and kernels (`hip.lzw_decode`,
`hip.tiff_place`, `hip.tiff_place_bands`) decode them, undo the predictor and place them in the cube in HBM; `TiffStack.read` is the
same on the host, in numpy.

    header  = byte order ('II' little-endian, 'MM' big-endian) magic (42 classic, 43 BigTIFF) offset of the first IFD
    IFD     = count [tag type count value-or-offset ...] offset of the next IFD (0: the last)
              classic: 2-byte count, 12-byte entries, 4-byte offsets; BigTIFF: 8-byte count, 20-byte entries, 8-byte offsets

A page (one IFD) is cut into strips of RowsPerStrip whole rows, or into tiles of TileWidth x TileLength samples — the right and bottom
tiles padded to full size —, each compressed on its own.  Before compression a predictor may have replaced every sample of a row but
the first by its difference from the sample before (2; in the sample's width, wrapping), or split the row's floats into byte planes,
most significant bytes first, and differenced those bytes (3).  The predictor is part of the LZW and Deflate codecs: on uncompressed
segments the tag means nothing, as in libtiff.

A page of SamplesPerPixel = B > 1 holds B bands, and every band of every full-resolution page is one time step, in page order, then
band order (GDAL's `-separate` merges, Earth Engine's `toBands()` exports, rioxarray's `to_raster` of a (time, y, x) array).
PlanarConfiguration 1 (chunky, GDAL's INTERLEAVE=PIXEL) interleaves the bands of a pixel: a segment holds rows x pitch x B samples, and
the predictors run at stride B as libtiff applies them (tif_predict.c) — predictor 2 adds sample i - B to sample i; predictor 3 is a
running sum over the row's pitch * B * size bytes at stride B, continuing across the byte planes, and sample i = pixel * B + band is
gathered from the bytes plane * (pitch * B) + i.  PlanarConfiguration 2 (INTERLEAVE=BAND) stores band b as single-band segments of its
own at indices b * across * down + k.  BitsPerSample and SampleFormat hold one value or B equal ones; ExtraSamples and
PhotometricInterpretation are ignored (a band is a band).  Parity with a GDAL- or Earth-Engine-written multi-band file is unverified:
none was at hand; the files tested are an independent writer's and libtiff's through Pillow (chunky uint8, predictor 2).

What is read: compression 1 (none), 5 (LZW) and 8 / 32946 (Deflate: zlib streams); predictors 1, 2 (integers) and 3 (float32 / float64);
integers of 8 / 16 / 32 / 64 bits of either sign, float32, float64; strips and tiles; any number of bands per pixel in either planar
configuration; any number of pages per file.
Pages whose NewSubfileType has bit 0 (a reduced-resolution overview) or bit 2 (a mask) set are skipped: every cloud-optimised GeoTIFF
has them.  Whatever else is met raises ValueError with the reason:

    any other compression, by number and name (JPEG, PackBits, ZSTD 50000, LERC, WebP, ...)
    old-style LZW (least significant bit first, a stream that begins 00 01) and FillOrder 2
    bits per sample other than 8 / 16 / 32 / 64; floats of 16 bits; complex samples
    predictor 2 on floats, predictor 3 on integers
    bands of one page that differ in width or format (mixed BitsPerSample / SampleFormat); a PlanarConfiguration other than 1 and 2
    a projected coordinate reference system (GTModelTypeGeoKey 1), rotated or sheared transformations, no georeferencing at all
    pages of one stack that differ in grid, type or nodata value
    offsets or byte counts that leave the file

Coordinates come from ModelPixelScale + ModelTiepoint, or from a ModelTransformation without rotation or shear: cell centres for
RasterPixelIsArea (the default), the grid points themselves for RasterPixelIsPoint.  Rows stay in stored order (north first, as a rule).
A TIFF has no time axis: ``tiff_time`` gives one, else the time is read from every file's name (`time_from_name`), or, for a
single-page multi-band file, from the band descriptions of GDAL_METADATA (tag 42112) where every band has one that holds a date.
"""
from __future__ import annotations

import os
import re
import struct

import numpy as np
import pandas as pd

# the tags that are read (every other entry of an IFD is skipped unread)
T_SUBFILE, T_WIDTH, T_LENGTH, T_BITS, T_COMPRESSION, T_FILL_ORDER, T_STRIP_OFFSETS, T_SPP, T_ROWS_PER_STRIP = 254, 256, 257, 258, 259, 266, 273, 277, 278
T_STRIP_COUNTS, T_PLANAR, T_PREDICTOR, T_TILE_WIDTH, T_TILE_LENGTH, T_TILE_OFFSETS, T_TILE_COUNTS, T_SAMPLE_FORMAT = 279, 284, 317, 322, 323, 324, 325, 339
T_PIXEL_SCALE, T_TIEPOINT, T_TRANSFORMATION, T_GEO_KEYS, T_GDAL_METADATA, T_GDAL_NODATA = 33550, 33922, 34264, 34735, 42112, 42113
_READ_TAGS = frozenset((T_SUBFILE, T_WIDTH, T_LENGTH, T_BITS, T_COMPRESSION, T_FILL_ORDER, T_STRIP_OFFSETS, T_SPP, T_ROWS_PER_STRIP, T_STRIP_COUNTS,
                        T_PLANAR, T_PREDICTOR, T_TILE_WIDTH, T_TILE_LENGTH, T_TILE_OFFSETS, T_TILE_COUNTS, T_SAMPLE_FORMAT, T_PIXEL_SCALE,
                        T_TIEPOINT, T_TRANSFORMATION, T_GEO_KEYS, T_GDAL_METADATA, T_GDAL_NODATA))
# field type -> (struct letter, bytes); 2 ASCII and 7 UNDEFINED are bytes; 5 / 10 (rationals) are pairs
_TYPES = {1: ("B", 1), 2: ("c", 1), 3: ("H", 2), 4: ("I", 4), 5: ("I", 4), 6: ("b", 1), 7: ("c", 1), 8: ("h", 2), 9: ("i", 4), 10: ("i", 4),
          11: ("f", 4), 12: ("d", 8), 13: ("I", 4), 16: ("Q", 8), 17: ("q", 8), 18: ("Q", 8)}
COMPRESSION_NONE, COMPRESSION_LZW, COMPRESSION_DEFLATE = 1, 5, 8
_DEFLATE_CODES = (8, 32946)
COMPRESSION_NAMES = {1: "none", 2: "CCITT modified Huffman RLE", 3: "CCITT Group 3 fax", 4: "CCITT Group 4 fax", 5: "LZW", 6: "old-style JPEG",
                     7: "JPEG", 8: "Deflate", 9: "JBIG", 32773: "PackBits", 32946: "Deflate", 34712: "JPEG 2000", 34887: "LERC", 34925: "LZMA",
                     50000: "ZSTD", 50001: "WebP", 50002: "JPEG XL"}
GT_MODEL_TYPE, GT_RASTER_TYPE = 1024, 1025
MAX_PAGES = 1 << 20


def is_tiff(path) -> bool:
    """Does ``path`` start with the magic of a TIFF file (classic or BigTIFF, either byte order)?"""
    try:
        with open(path, "rb") as f:
            m = f.read(4)
    except (OSError, TypeError):
        return False
    return m in (b"II*\0", b"MM\0*", b"II+\0", b"MM\0+")


_NAME_DATE = re.compile(r"(?<!\d)(?:(\d{4})[._-](\d{2})[._-](\d{2})|(\d{8})|(\d{6})|(\d{4}))(?!\d)")


def time_from_name(path) -> pd.Timestamp:
    """The time step a single-page file's name gives: the LAST run of its base name that reads as ``YYYYMMDD``, ``YYYY[._-]MM[._-]DD``,
    ``YYYYMM`` or ``YYYY`` (digits not next to other digits) and is a date between the years 1000 and 2999."""
    base = os.path.basename(str(path))
    base = base[:base.rfind(".")] if "." in base and base.lower().endswith((".tif", ".tiff")) else base
    found = _date_in(base)
    if found is None:
        raise ValueError(f"{path}: no time step can be read from the file name (YYYYMMDD, YYYY-MM-DD, YYYYMM or YYYY); pass tiff_time=")
    return found


def _date_in(text):
    """The last date `time_from_name`'s patterns find in ``text``, or None."""
    found = None
    for m in _NAME_DATE.finditer(text):
        y, mo, d, ymd, ym, yy = m.groups()
        if ymd:
            y, mo, d = ymd[:4], ymd[4:6], ymd[6:]
        elif ym:
            y, mo, d = ym[:4], ym[4:], "01"
        elif yy:
            y, mo, d = yy, "01", "01"
        try:
            if 1000 <= int(y) <= 2999:
                found = pd.Timestamp(year=int(y), month=int(mo), day=int(d))
        except ValueError:
            pass
    return found


class Page:
    """One image file directory: what it says of the image, and where its segments lie (no data)."""

    def __init__(self, path, index, byteorder, tags, file_size):
        self.path, self.index, self.byteorder = path, index, byteorder
        one = lambda t, default: int(tags[t][0]) if t in tags and len(tags[t]) else default
        where = f"{path}: page {index}"
        self.subfile = one(T_SUBFILE, 0)
        self.skipped = bool(self.subfile & 5)                       # bit 0: a reduced-resolution overview, bit 2: a mask
        self.width, self.height = one(T_WIDTH, 0), one(T_LENGTH, 0)
        self.spp, self.planar = one(T_SPP, 1), one(T_PLANAR, 1)
        self.compression, self.predictor, self.fill_order = one(T_COMPRESSION, 1), one(T_PREDICTOR, 1), one(T_FILL_ORDER, 1)
        self.bits = [int(b) for b in tags.get(T_BITS, (1,))]
        self.sample_format = [int(b) for b in tags.get(T_SAMPLE_FORMAT, (1,))]
        self.nodata_text, self.gdal_metadata = tags.get(T_GDAL_NODATA), tags.get(T_GDAL_METADATA)
        self.pixel_scale, self.tiepoint = tags.get(T_PIXEL_SCALE), tags.get(T_TIEPOINT)
        self.transformation, self.geo_keys = tags.get(T_TRANSFORMATION), tags.get(T_GEO_KEYS)
        self.tiled = T_TILE_WIDTH in tags or T_TILE_OFFSETS in tags
        if self.skipped:
            return
        if self.width <= 0 or self.height <= 0 or self.width > 0x7fffffff or self.height > 0x7fffffff:
            raise ValueError(f"{where}: ImageWidth / ImageLength missing or absurd ({self.width} x {self.height})")
        B = self.bands = self.spp
        if B < 1:
            raise ValueError(f"{where}: SamplesPerPixel = {B}")
        if self.planar not in (1, 2):
            raise ValueError(f"{where}: PlanarConfiguration {self.planar} is not read: 1 (chunky) and 2 (planar) are")
        self.chunky = B > 1 and self.planar == 1                    # (one band: the two configurations are the same file)
        for what, vals in (("BitsPerSample", self.bits), ("SampleFormat", self.sample_format)):
            if len(vals) not in (1, B) or len(set(vals)) != 1:
                if len(vals) > 1 and len(set(vals)) > 1:
                    raise ValueError(f"{where}: the bands differ in {what} ({', '.join(str(v) for v in vals)}): mixed band types are not read")
                raise ValueError(f"{where}: {what} holds {len(vals)} values for SamplesPerPixel = {B}: one value, or one per band")
        if self.compression not in (COMPRESSION_NONE, COMPRESSION_LZW) + _DEFLATE_CODES:
            raise ValueError(f"{where}: compression {self.compression} ({COMPRESSION_NAMES.get(self.compression, 'unknown')}) is not read: "
                             "none (1), LZW (5) and Deflate (8, 32946) are")
        if self.fill_order != 1:
            raise ValueError(f"{where}: FillOrder {self.fill_order} (bits least significant first) is not read")
        bits, fmt = self.bits[0], self.sample_format[0]
        if fmt in (5, 6):
            raise ValueError(f"{where}: complex samples (SampleFormat {fmt}) are not read")
        if fmt not in (1, 2, 3):
            raise ValueError(f"{where}: SampleFormat {fmt} is not read: unsigned (1), signed (2) and floating-point (3) samples are")
        if bits not in (8, 16, 32, 64):
            raise ValueError(f"{where}: {bits} bits per sample are not read: 8, 16, 32 and 64 are")
        if fmt == 3 and bits < 32:
            raise ValueError(f"{where}: floating-point samples of {bits} bits per sample are not read: float32 and float64 are")
        self.dtype = np.dtype({1: "u", 2: "i", 3: "f"}[fmt] + str(bits // 8))          # native byte order
        if self.predictor not in (1, 2, 3):
            raise ValueError(f"{where}: predictor {self.predictor} is not read: 1 (none), 2 (horizontal) and 3 (floating point) are")
        if self.predictor == 2 and fmt == 3:
            raise ValueError(f"{where}: predictor 2 (horizontal differencing) on floating-point samples is not read")
        if self.predictor == 3 and fmt != 3:
            raise ValueError(f"{where}: predictor 3 (floating point) on integer samples is not read")
        if self.compression == COMPRESSION_NONE:
            self.predictor = 1                  # the predictor belongs to the LZW and Deflate codecs: libtiff applies none to stored samples
        E = self.dtype.itemsize
        if self.tiled:
            self.seg_w, self.seg_h = one(T_TILE_WIDTH, 0), one(T_TILE_LENGTH, 0)
            if self.seg_w <= 0 or self.seg_h <= 0 or self.seg_w > 0x7fffffff or self.seg_h > 0x7fffffff:
                raise ValueError(f"{where}: TileWidth / TileLength missing or absurd ({self.seg_w} x {self.seg_h})")
            offs, cnts = tags.get(T_TILE_OFFSETS), tags.get(T_TILE_COUNTS)
        else:
            self.seg_w, self.seg_h = self.width, max(1, min(one(T_ROWS_PER_STRIP, self.height), self.height))
            offs, cnts = tags.get(T_STRIP_OFFSETS), tags.get(T_STRIP_COUNTS)
        self.across, self.down = -(-self.width // self.seg_w), -(-self.height // self.seg_h)
        n = self.across * self.down * (1 if self.planar == 1 else B)
        per = f" (SamplesPerPixel = {B}, PlanarConfiguration {self.planar})" if B > 1 else ""
        if offs is None or cnts is None or len(offs) != n or len(cnts) != n:
            raise ValueError(f"{where}: {n} {'tiles' if self.tiled else 'strips'} need as many offsets and byte counts{per} "
                             f"({0 if offs is None else len(offs)} and {0 if cnts is None else len(cnts)} are there)")
        self.offsets, self.counts = np.asarray(offs, dtype=np.uint64), np.asarray(cnts, dtype=np.uint64)
        if n and (int(self.offsets.max()) > file_size or int(self.counts.max()) > file_size or int((self.offsets + self.counts).max()) > file_size):
            k = int(np.argmax(self.offsets + self.counts > file_size))
            raise ValueError(f"{where}: {'tile' if self.tiled else 'strip'} {k} (offset {int(self.offsets[k])}, {int(self.counts[k])} bytes) "
                             f"leaves the file ({file_size} bytes)")
        self.offsets, self.counts = self.offsets.astype(np.int64), self.counts.astype(np.int64)
        Bs = B if self.chunky else 1                                # the samples of a pixel in one segment
        if (self.seg_h * self.seg_w * E * Bs) > 0x7fffffff:
            raise ValueError(f"{where}: a {'tile' if self.tiled else 'strip'} of {self.seg_h} x {self.seg_w} samples{per} is larger than 2 GiB")
        if self.compression == COMPRESSION_NONE:
            k0 = (np.arange(n) % (self.across * self.down)) // self.across
            need = (np.minimum(self.seg_h, self.height - k0 * self.seg_h) if not self.tiled else self.seg_h) * self.seg_w * E * Bs
            if (self.counts < need).any():
                k = int(np.argmax(self.counts < need))
                raise ValueError(f"{where}: {'tile' if self.tiled else 'strip'} {k} holds {int(self.counts[k])} bytes, its samples{per} need "
                                 f"{int(np.broadcast_to(need, (n,))[k])}")
        if self.compression == COMPRESSION_LZW and n:
            k = int(np.argmax(self.counts > 1)) if (self.counts > 1).any() else -1
            if k >= 0:
                fd = os.open(path, os.O_RDONLY)
                try:
                    head = os.pread(fd, 2, int(self.offsets[k]))
                finally:
                    os.close(fd)
                if len(head) == 2 and head[0] == 0 and (head[1] & 1):
                    raise ValueError(f"{where}: old-style LZW (codes least significant bit first, as TIFF 5.0 writers left them) is not read")
        self.nodata = self._nodata(where)
        self.longitude, self.latitude = self._coordinates(where)

    # ---- what the tags say ----
    def _nodata(self, where):
        """GDAL_NODATA as a number of the samples' type, or None (absent; "nan"; a value the type cannot hold)."""
        if self.nodata_text is None:
            return None
        text = self.nodata_text.strip().strip("\0").strip()
        try:
            v = float(text)
        except ValueError:
            raise ValueError(f"{where}: GDAL_NODATA {text!r} is no number") from None
        if np.isnan(v):
            return None
        if self.dtype.kind == "f":
            return float(self.dtype.type(v))
        try:
            iv = int(text)
        except ValueError:
            iv = int(v) if v == int(v) else None
        info = np.iinfo(self.dtype)
        return iv if iv is not None and info.min <= iv <= info.max else None

    def _geo_key(self, key):
        g = self.geo_keys
        if g is None or len(g) < 4:
            return None
        for i in range(int(g[3])):
            e = g[4 + 4 * i: 8 + 4 * i]
            if len(e) == 4 and int(e[0]) == key and int(e[1]) == 0:
                return int(e[3])
        return None

    def _coordinates(self, where):
        model = self._geo_key(GT_MODEL_TYPE)
        if model == 1:
            raise ValueError(f"{where}: a projected coordinate reference system (GTModelTypeGeoKey 1) is not read: geographic "
                             "(longitude / latitude) grids only, there is no reprojection")
        if model == 3:
            raise ValueError(f"{where}: a geocentric coordinate reference system (GTModelTypeGeoKey 3) is not read")
        half = 0.0 if self._geo_key(GT_RASTER_TYPE) == 2 else 0.5            # RasterPixelIsPoint: the tie point is the grid point itself
        cols, rows = np.arange(self.width, dtype=np.float64), np.arange(self.height, dtype=np.float64)
        if self.pixel_scale is not None and self.tiepoint is not None and len(self.pixel_scale) >= 2 and len(self.tiepoint) >= 6:
            sx, sy = float(self.pixel_scale[0]), float(self.pixel_scale[1])
            i, j, _, x, y = (float(v) for v in self.tiepoint[:5])
            return x + (cols - i + half) * sx, y - (rows - j + half) * sy
        if self.transformation is not None and len(self.transformation) >= 8:
            m = [float(v) for v in self.transformation]
            if m[1] != 0.0 or m[4] != 0.0:
                raise ValueError(f"{where}: a rotated or sheared ModelTransformation is not read (its terms {m[1]} and {m[4]} must be 0)")
            return m[3] + (cols + half) * m[0], m[7] + (rows + half) * m[5]
        raise ValueError(f"{where}: no georeferencing (neither ModelPixelScale + ModelTiepoint nor ModelTransformation): the grid has no coordinates")

    @property
    def n_segments(self):
        """The segments of the page; of a planar page: of all its bands."""
        return self.across * self.down * (1 if self.planar == 1 else self.bands)

    def band_descriptions(self):
        """The DESCRIPTION item of every band in GDAL_METADATA (tag 42112), or None where a band has none:
        ``<Item name="DESCRIPTION" sample="k" role="description">text</Item>``, found by an explicit search for that form — no XML parser
        reads a file's bytes here."""
        out = [None] * self.bands
        for attrs, text in _ITEM.findall(self.gdal_metadata or ""):
            a = dict(_ATTR.findall(attrs))
            if a.get("name") == "DESCRIPTION" and a.get("role", "description") == "description" and a.get("sample", "").isdigit():
                k = int(a["sample"])
                if k < self.bands and out[k] is None:
                    out[k] = _unescape(text.strip())
        return out

    def grid_key(self):
        return (self.width, self.height, self.dtype.str, self.nodata, self.longitude.tobytes(), self.latitude.tobytes())

    def segments(self, box=None, band=0):
        """The segments that touch the stored-axes ``box`` (a0, a1, b0, b1) (None: all), as arrays: index, first row, first column,
        rows (of a bottom strip: those it holds; of a tile: all, padding included), pitch (in pixels), decoded bytes.  A chunky page's
        segments hold all its bands (rows x pitch x bands samples); a planar page's are those of ``band``, single-band segments."""
        a0, a1, b0, b1 = box if box is not None else (0, self.height, 0, self.width)
        k = np.arange(self.across * self.down, dtype=np.int64)
        y, x = (k // self.across) * self.seg_h, (k % self.across) * self.seg_w
        rows = np.full_like(k, self.seg_h) if self.tiled else np.minimum(self.seg_h, self.height - y)
        keep = (y < a1) & (y + rows > a0) & (x < b1) & (x + self.seg_w > b0)
        k, y, x, rows = k[keep], y[keep], x[keep], rows[keep]
        if self.chunky:
            return k, y, x, rows, np.full_like(k, self.seg_w), rows * self.seg_w * self.dtype.itemsize * self.bands
        if not 0 <= band < self.bands:
            raise IndexError(f"band {band} of a page of {self.bands}")
        return k + band * self.across * self.down, y, x, rows, np.full_like(k, self.seg_w), rows * self.seg_w * self.dtype.itemsize

    def __repr__(self):
        return (f"<tiff.Page {self.index} of {self.path!r} {self.width}x{self.height} {getattr(self, 'dtype', '?')} compression={self.compression} "
                f"predictor={self.predictor} bands={getattr(self, 'bands', '?')} {'tiles' if self.tiled else 'strips'} {self.seg_w}x{getattr(self, 'seg_h', '?')}>")


_ITEM = re.compile(r"<Item\b([^>]*)>(.*?)</Item\s*>", re.S)
_ATTR = re.compile(r"""([A-Za-z_][\w.-]*)\s*=\s*["']([^"']*)["']""")


def _unescape(text):
    for a, b in (("&lt;", "<"), ("&gt;", ">"), ("&quot;", '"'), ("&apos;", "'"), ("&amp;", "&")):
        text = text.replace(a, b)
    return text


class Step:
    """One time step of a stack: band ``band`` of ``page``.  What the page says of the image (``compression``, ``predictor``, ``dtype``,
    ...) reads through; ``segments`` are those that hold the band."""

    __slots__ = ("page", "band")

    def __init__(self, page, band):
        self.page, self.band = page, band

    def __getattr__(self, name):
        return getattr(self.page, name)

    def segments(self, box=None):
        return self.page.segments(box, self.band)

    def __repr__(self):
        return f"<tiff.Step band {self.band} of {self.page!r}>"


class TiffFile:
    """The image file directories of one TIFF file: ``pages`` are the full-resolution ones, in file order (overviews and masks are
    counted in ``n_skipped``); ``bigtiff``, ``byteorder`` ("<" or ">")."""

    def __init__(self, path):
        self.path = path = str(path)
        self.size = size = os.path.getsize(path)
        fd = os.open(path, os.O_RDONLY)
        try:
            head = os.pread(fd, 16, 0)
            if len(head) < 8 or head[:2] not in (b"II", b"MM"):
                raise ValueError(f"{path}: not a TIFF file")
            bo = self.byteorder = "<" if head[:2] == b"II" else ">"
            magic = struct.unpack(bo + "H", head[2:4])[0]
            if magic == 42:
                self.bigtiff, pos = False, struct.unpack(bo + "I", head[4:8])[0]
            elif magic == 43:
                if len(head) < 16 or struct.unpack(bo + "HH", head[4:8]) != (8, 0):
                    raise ValueError(f"{path}: a BigTIFF header with offsets of other than 8 bytes")
                self.bigtiff, pos = True, struct.unpack(bo + "Q", head[8:16])[0]
            else:
                raise ValueError(f"{path}: not a TIFF file (magic {magic})")
            self.pages, self.n_skipped, seen = [], 0, set()
            while pos:
                if pos in seen or len(seen) >= MAX_PAGES:
                    raise ValueError(f"{path}: the chain of image file directories runs in a circle (offset {pos} twice)")
                seen.add(pos)
                tags, pos = self._ifd(fd, pos)
                page = Page(path, len(seen) - 1, bo, tags, size)
                if page.skipped:
                    self.n_skipped += 1
                else:
                    self.pages.append(page)
        finally:
            os.close(fd)
        if not self.pages:
            raise ValueError(f"{path}: no full-resolution page (every page is an overview or a mask)")

    def _ifd(self, fd, pos):
        bo, size, path = self.byteorder, self.size, self.path
        cw, ew, ow, cf, of = (8, 20, 8, "Q", "Q") if self.bigtiff else (2, 12, 4, "H", "I")
        raw = os.pread(fd, cw, pos)
        if len(raw) != cw:
            raise ValueError(f"{path}: an image file directory at offset {pos} leaves the file ({size} bytes)")
        n = struct.unpack(bo + cf, raw)[0]
        if n > 65536 or pos + cw + n * ew + ow > size:
            raise ValueError(f"{path}: an image file directory of {n} entries at offset {pos} leaves the file ({size} bytes)")
        raw = os.pread(fd, n * ew + ow, pos + cw)
        tags = {}
        for i in range(n):
            e = raw[i * ew:(i + 1) * ew]
            tag, typ = struct.unpack(bo + "HH", e[:4])
            if tag not in _READ_TAGS:
                continue
            count = struct.unpack(bo + of, e[4:4 + ow])[0]
            if typ not in _TYPES:
                raise ValueError(f"{path}: tag {tag} has the unknown field type {typ}")
            letter, each = _TYPES[typ]
            k = count * (2 if typ in (5, 10) else 1)
            nbytes = k * each
            if nbytes <= ow:
                val = e[4 + ow:4 + ow + nbytes]
            else:
                off = struct.unpack(bo + of, e[4 + ow:4 + 2 * ow])[0]
                if off + nbytes > size:
                    raise ValueError(f"{path}: the {count} values of tag {tag} at offset {off} leave the file ({size} bytes)")
                val = os.pread(fd, nbytes, off)
                if len(val) != nbytes:
                    raise ValueError(f"{path}: the values of tag {tag} are cut short")
            if typ in (2, 7):
                tags[tag] = val.decode("latin-1")
            else:
                arr = np.frombuffer(val, dtype=np.dtype(bo + {"B": "u1", "H": "u2", "I": "u4", "b": "i1", "h": "i2", "i": "i4", "f": "f4",
                                                              "d": "f8", "Q": "u8", "q": "i8"}[letter]))
                tags[tag] = arr[0::2] / np.maximum(arr[1::2], 1) if typ in (5, 10) else arr
        nxt = struct.unpack(bo + of, raw[n * ew:n * ew + ow])[0]
        if nxt > size:
            raise ValueError(f"{path}: the next image file directory (offset {nxt}) lies beyond the file ({size} bytes)")
        return tags, nxt


def _timestamps(v):
    if isinstance(v, (str, bytes)) or not hasattr(v, "__len__"):
        v = [v]
    return list(pd.DatetimeIndex(pd.to_datetime(list(v))))


class TiffStack:
    """The pages of one or many TIFF files in time order, as one (time, latitude, longitude) variable: ``shape``, ``dtype`` (the
    stored type, native byte order), ``nodata``, ``attrs`` (``_FillValue`` where there is a nodata value), ``time``, ``latitude``,
    ``longitude``, and ``steps``: the `Step` (page, band) of every time step — every band of every page, in page order, then band
    order.  Pages of one stack share grid, type and nodata value; they may differ in band count and planar configuration."""

    def __init__(self, paths, tiff_time=None):
        paths = [paths] if isinstance(paths, (str, os.PathLike)) else list(paths)
        if not paths:
            raise ValueError("a TIFF stack needs a file")
        self.files = [TiffFile(p) for p in paths]
        self.paths = [f.path for f in self.files]
        self.pages = [pg for f in self.files for pg in f.pages]
        self.steps = [Step(pg, b) for pg in self.pages for b in range(pg.bands)]
        first = self.pages[0]
        key = first.grid_key()
        for pg in self.pages[1:]:
            if pg.grid_key() != key:
                what = ("size" if (pg.width, pg.height) != (first.width, first.height) else "type" if pg.dtype != first.dtype else
                        "nodata value" if pg.nodata != first.nodata else "grid coordinates")
                raise ValueError(f"{pg.path}: page {pg.index} differs from the first page of the stack ({first.path}) in its {what}: "
                                 "the pages of one stack share grid, type and nodata")
        self.dtype, self.nodata = first.dtype, first.nodata
        self.latitude, self.longitude = first.latitude, first.longitude
        self.shape = (len(self.steps), first.height, first.width)
        self.attrs = {} if self.nodata is None else {"_FillValue": self.nodata}
        self.time = self._time(tiff_time)

    def _time(self, tiff_time):
        n = len(self.steps)
        if tiff_time is None:
            times = []
            for f in self.files:
                if len(f.pages) == 1 and f.pages[0].bands == 1:
                    times.append(time_from_name(f.path))
                    continue
                got = _times_from_descriptions(f.pages[0]) if len(f.pages) == 1 else None
                if got is None:
                    kind = "multi-page" if len(f.pages) > 1 else "multi-band"
                    raise ValueError(f"{f.path}: a {kind} file has no time axis and its name gives one step: pass tiff_time= "
                                     "(a sequence of timestamps, or a callable path -> timestamps), or band descriptions that hold a date")
                times += got
        elif callable(tiff_time):
            times = []
            for f in self.files:
                got = _timestamps(tiff_time(f.path))
                want = sum(pg.bands for pg in f.pages)
                if len(got) != want:
                    bands = "" if want == len(f.pages) else f" of {want} band(s) in all"
                    raise ValueError(f"{f.path}: tiff_time gave {len(got)} timestamp(s) for {len(f.pages)} page(s){bands}")
                times += got
        else:
            times = _timestamps(tiff_time)
            if len(times) != n:
                raise ValueError(f"tiff_time holds {len(times)} timestamps, the stack has {n} steps")
        return pd.DatetimeIndex(times)

    def coords(self) -> dict:
        return {"time": self.time, "latitude": self.latitude, "longitude": self.longitude}

    def read_raw(self, steps=None, threads: int = 8) -> np.ndarray:
        """The stored samples of ``steps`` (None: all; a range or a sequence of step numbers) as (time, latitude, longitude) in the
        stored type: the segments are decoded by the codec library (`codec.lzw_decode_ranges`, `codec.decode_ranges`, `codec.read_packed`)
        and the predictor is undone in numpy."""
        from . import codec
        idx = list(range(self.shape[0])) if steps is None else list(steps)
        _, H, W = self.shape
        out = np.empty((len(idx), H, W), dtype=self.dtype)
        # what is decoded: a planar or single-band step's own segments; a chunky page's segments once, for all of its bands asked for
        jobs = {}
        for i, t in enumerate(idx):
            st = self.steps[t]
            jobs.setdefault((id(st.page), st.band if not st.page.chunky else -1), (st, []))[1].append((i, st.band))
        for st, takes in jobs.values():
            pg = st.page
            B = pg.bands if pg.chunky else 1
            k, y, x, rows, pitch, nbytes = st.segments()
            bufs = [np.empty(int(b), dtype=np.uint8) for b in nbytes]
            locs = [(pg.path, int(pg.offsets[j]), int(pg.counts[j])) for j in k]
            if pg.compression == COMPRESSION_LZW:
                codec.lzw_decode_ranges(locs, bufs, threads=threads)
            elif pg.compression in _DEFLATE_CODES:
                codec.decode_ranges("zlib", locs, bufs, threads=threads)
            else:
                locs = [(p, o, int(b)) for (p, o, _), b in zip(locs, nbytes)]
                codec.decode_ranges("raw", locs, bufs, threads=threads)
            for buf, yy, xx, r, p in zip(bufs, y.tolist(), x.tolist(), rows.tolist(), pitch.tolist()):
                seg = undo_predictor(buf, r, p, pg.dtype, pg.predictor, pg.byteorder, B)
                hh, ww = min(r, H - yy), min(p, W - xx)
                for i, band in takes:
                    out[i, yy:yy + hh, xx:xx + ww] = seg[:hh, :ww] if B == 1 else seg[:hh, :ww, band]
        return out

    def read(self, steps=None, threads: int = 8) -> np.ndarray:
        """`read_raw` with the nodata value masked as every other container's ``_FillValue`` is (`io._cf_mask_scale`): NaN in floats;
        integers with a nodata value become floats with NaN (float32 up to 16 bits, float64 beyond)."""
        from .io import _cf_mask_scale
        return _cf_mask_scale(self.read_raw(steps, threads), self.attrs)


def _times_from_descriptions(page):
    """The time steps the band descriptions of ``page`` give (`Page.band_descriptions`, `time_from_name`'s patterns), or None unless
    every band has a description that holds a date."""
    times = [None if d is None else _date_in(d) for d in page.band_descriptions()]
    return None if any(t is None for t in times) else times


def undo_predictor(buf: np.ndarray, rows: int, pitch: int, dtype, predictor: int, byteorder: str, bands: int = 1) -> np.ndarray:
    """One decoded segment (uint8) -> its (rows, pitch) samples — (rows, pitch, bands) of a chunky segment of ``bands`` > 1 — in native
    byte order, the predictor undone along every row at a stride of ``bands`` samples, as libtiff does it."""
    dtype = np.dtype(dtype)
    E, B = dtype.itemsize, int(bands)
    shape = (rows, pitch) if B == 1 else (rows, pitch, B)
    if predictor == 3:
        # a running sum over the row's bytes at stride B — the bytes of one band are one chain through all the planes, since pitch * B is
        # a multiple of B —, then sample i = pixel * B + band is the bytes i, pitch * B + i, 2 pitch * B + i, ... — most significant
        # first, whatever the file's byte order
        b = np.cumsum(buf.reshape(rows, pitch * E, B), axis=1, dtype=np.uint8)
        return np.ascontiguousarray(b.reshape(rows, E, pitch * B).transpose(0, 2, 1)).view(dtype.newbyteorder(">")).reshape(shape).astype(dtype)
    a = buf.view(dtype.newbyteorder(byteorder)).reshape(rows, pitch, B).astype(dtype)
    if predictor == 2:
        a = np.cumsum(a, axis=1, dtype=dtype)                       # wraps in the sample's width
    return a.reshape(shape)
