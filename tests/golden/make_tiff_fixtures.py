"""Writes tests/golden/tiff/: small GeoTIFF files written by Pillow's libtiff (LZW and Deflate, predictors 2 and 3, uint8 / uint16 /
float32, single- and multi-page) with their values as .npy and an index (index.json), so that tests/test_tiff.py and
tests/test_gpu_tiff.py hold the reader to files of an independent writer without needing Pillow.

    python3 tests/golden/make_tiff_fixtures.py        (Pillow with libtiff)
"""
import json
import os

import numpy as np
from PIL import Image, TiffImagePlugin

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tiff")
H, W = 23, 41


def values(dtype, pages, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([np.sin(x / 6.0 + t) * 30 + np.cos(y / 4.0) * 20 + 60 + t for t in range(pages)])
    if np.dtype(dtype).kind == "f":
        return (base + rng.normal(0, 0.05, base.shape)).astype(dtype)
    top = np.iinfo(dtype).max
    return np.clip(base / 120 * top + rng.integers(0, 3, base.shape), 0, top).astype(dtype)


def tags(predictor, nodata=None):
    ifd = TiffImagePlugin.ImageFileDirectory_v2()
    ifd[33550] = (0.5, 0.5, 0.0)                                   # ModelPixelScale
    ifd[33922] = (0.0, 0.0, 0.0, 10.0, 60.0, 0.0)                  # ModelTiepoint: the upper-left corner at 10 E, 60 N
    ifd[34735] = (1, 1, 0, 2, 1024, 0, 1, 2, 1025, 0, 1, 1)        # geographic, RasterPixelIsArea
    ifd[317] = predictor
    if nodata is not None:
        ifd[42113] = str(nodata)
    return ifd


def main():
    os.makedirs(OUT, exist_ok=True)
    index = []
    for name, dtype, comp, pred, pages, nodata in (("lzw_p2_u8", "u1", "tiff_lzw", 2, 1, None), ("lzw_p2_u16", "u2", "tiff_lzw", 2, 1, 65535),
                                                   ("lzw_p3_f32", "f4", "tiff_lzw", 3, 1, None), ("lzw_p1_f32", "f4", "tiff_lzw", 1, 1, None),
                                                   ("deflate_p2_u16", "u2", "tiff_adobe_deflate", 2, 1, None),
                                                   ("deflate_p3_f32", "f4", "tiff_adobe_deflate", 3, 1, -9999),
                                                   ("lzw_p3_f32_pages", "f4", "tiff_lzw", 3, 4, None), ("deflate_p2_u8_pages", "u1", "tiff_adobe_deflate", 2, 3, None)):
        a = values(dtype, pages, len(index))
        if nodata is not None:
            a[:, 2:4, 5:9] = nodata
        ims = [Image.fromarray(p) for p in a]
        fn = f"{name}_20200{len(index) + 1}01.tif"
        # (every frame is given the tags: a frame appended without them has no georeferencing)
        for im in ims:
            im.encoderinfo = {"tiffinfo": tags(pred, nodata), "compression": comp}
        ims[0].save(os.path.join(OUT, fn), compression=comp, tiffinfo=tags(pred, nodata), save_all=pages > 1, append_images=ims[1:])
        np.save(os.path.join(OUT, name + ".npy"), a)
        index.append(dict(name=name, file=fn, values=name + ".npy", dtype=np.dtype(dtype).str, pages=pages, nodata=nodata, predictor=pred,
                          compression=5 if comp == "tiff_lzw" else 8))
    with open(os.path.join(OUT, "index.json"), "w") as f:
        json.dump(index, f, indent=1)


if __name__ == "__main__":
    main()
