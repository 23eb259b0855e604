"""Writes tests/golden/tiff_bands/: small multi-band GeoTIFF files written by Pillow's libtiff — chunky uint8 RGB (SamplesPerPixel 3)
and RGBA (SamplesPerPixel 4, with ExtraSamples), LZW and Deflate, predictor 2 at a stride of SamplesPerPixel — with their values as
(band, y, x) .npy and an index (index.json), so that tests/test_tiff_bands.py and tests/test_gpu_tiff_bands.py hold the reader to files
of an independent writer without needing Pillow.  Pillow writes no readable PlanarConfiguration 2 file and no multi-band samples wider
than 8 bits: those rest on tests/tiff_band_cases.py.

    python3 tests/golden/make_tiff_band_fixtures.py        (Pillow with libtiff)
"""
import json
import os

import numpy as np
from PIL import Image, TiffImagePlugin

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tiff_bands")
H, W = 23, 71                                   # rows of more than 64 pixels


def values(bands, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([np.sin(x / 6.0 + 1.3 * b) * 50 + np.cos(y / 4.0 - b) * 40 + 110 + 7 * b for b in range(bands)])
    return np.clip(base + rng.integers(0, 3, base.shape), 0, 255).astype(np.uint8)


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
    for name, mode, comp, pred, nodata in (("lzw_p2_rgb", "RGB", "tiff_lzw", 2, None), ("deflate_p2_rgb", "RGB", "tiff_adobe_deflate", 2, 255),
                                           ("lzw_p2_rgba", "RGBA", "tiff_lzw", 2, None), ("deflate_p2_rgba", "RGBA", "tiff_adobe_deflate", 2, None),
                                           ("deflate_p1_rgb", "RGB", "tiff_adobe_deflate", 1, None)):
        a = values(len(mode), len(index))
        if nodata is not None:
            a[:, 2:4, 5:9] = nodata
        fn = name + ".tif"
        Image.fromarray(np.ascontiguousarray(a.transpose(1, 2, 0)), mode).save(os.path.join(OUT, fn), compression=comp, tiffinfo=tags(pred, nodata))
        np.save(os.path.join(OUT, name + ".npy"), a)
        index.append(dict(name=name, file=fn, values=name + ".npy", bands=len(mode), nodata=nodata, predictor=pred,
                          compression=5 if comp == "tiff_lzw" else 8))
    with open(os.path.join(OUT, "index.json"), "w") as f:
        json.dump(index, f, indent=1)


if __name__ == "__main__":
    main()
