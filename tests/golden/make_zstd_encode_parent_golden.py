"""Writes tests/golden/zstd_encode_parent.json: sha256 of every file `dataset_to_zarr(..., encode="host")` writes for the small cube of
tests/zstd_encode_cases.py under compress="blosc-zstd" and "zstd" (formats 2 and 3, one sharded store).  It was run on the commit
BEFORE the GPU route learnt Zstandard streams (AGGFLY_TREE pointing at a built checkout of that commit); tests/test_zstd_encode.py
holds every later build's host route to these bytes.

    AGGFLY_TREE=/path/to/parent/checkout python tests/golden/make_zstd_encode_parent_golden.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.environ.get("AGGFLY_TREE", os.path.dirname(os.path.dirname(HERE))))

import aggfly_amd as af                         # noqa: E402
import zstd_encode_cases as zc                  # noqa: E402

stores = []
for kw in zc.HOST_ROUTE_STORES:
    with tempfile.TemporaryDirectory() as tmp:
        extra = {"encode": "host"} if "encode" in af.io.dataset_to_zarr.__code__.co_varnames else {}
        af.io.dataset_to_zarr(zc.small_dataset(), os.path.join(tmp, "s.zarr"), chunks=zc.SMALL_CHUNKS, **kw, **extra)
        stores.append(dict(kw, files=zc.tree_hashes(os.path.join(tmp, "s.zarr"))))
json.dump({"stores": stores}, open(os.path.join(HERE, "zstd_encode_parent.json"), "w"), indent=0)
print(len(stores), "stores,", sum(len(s["files"]) for s in stores), "files")
