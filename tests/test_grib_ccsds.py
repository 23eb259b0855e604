"""GRIB2 CCSDS packing (data representation template 5.42) on the host: `afcodec_aec_decode` — the passes of aec_passes.h in loops, the
text the GPU kernels run — and `grib.unpack_ccsds` against the streams of tests/golden/grib_ccsds_streams.json (written by libaec and by
the forcing writer of tests/grib_ccsds_cases.py, each decoded by libaec before it was committed) and, where libaec can be loaded,
against libaec itself on random fields; the index and `GribFile.read` on the catalogue, every refusal with its reason, and the C-ABI
surface of the device entry.  Every comparison is exact."""
import ctypes
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib_cases as C  # noqa: E402
import grib_ccsds_cases as A  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import codec, distributed as D, grib, hip, io as afio  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = A.build_cases()
BY = {c.name: c for c in CASES}
GOLDEN = A.golden()
needs_libaec = pytest.mark.skipif(A.load_libaec() is None, reason="libaec cannot be loaded on this machine")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("griba")
    return {c.name: c.write(d) for c in CASES}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (a.shape, a.dtype, b.shape, b.dtype)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def _decode(row):
    return codec.aec_decode(bytes.fromhex(row["hex"]), len(row["samples"]), row["nbits"], A.PREPROCESS if row["preprocess"] else 0,
                            row["block_size"], row["rsi"])


class _M:
    """What `grib.unpack_ccsds` reads of a message."""

    def __init__(self, row):
        self.n_values, self.nbits, self.block_size, self.rsi = len(row["samples"]), row["nbits"], row["block_size"], row["rsi"]
        self.ccsds_flags = (A.PREPROCESS if row["preprocess"] else 0) | 4


# ---------------------------------------------------------------------------------------
# the golden streams
# ---------------------------------------------------------------------------------------
def test_the_known_answer_of_the_issue():
    row = GOLDEN[0]
    assert (row["name"], row["writer"], row["nbits"], row["block_size"], row["rsi"], row["preprocess"]) == ("known_answer", "libaec", 8, 8, 2, True)
    assert row["hex"] == "ec804080003f5fe0e10079c2f8"
    assert row["samples"] == [100, 101, 103, 103, 102, 250, 0] + [7] * 19 + [9, 8]
    got = _decode(row)
    assert got.dtype == np.uint32 and got.tolist() == row["samples"]
    # an uncompressed block, two zero runs of one block (the second a first block), a k-split block that is padded
    assert [blk[:3] for blk in _blocks(row)] == [(0, 0, "unc"), (0, 1, "zero"), (1, 0, "zero"), (1, 1, "k")]
    # the forcing writer takes other options for the first blocks (it is no copy of libaec's chooser); its stream decodes to the same samples
    assert codec.aec_decode(A.encode(row["samples"], 8, 8, 2), 28, 8, 8, 8, 2).tolist() == row["samples"]


@pytest.mark.parametrize("row", GOLDEN, ids=lambda r: r["name"])
def test_golden_stream(row):
    assert _decode(row).tolist() == row["samples"]
    X = grib.unpack_ccsds(_M(row), bytes.fromhex(row["hex"]))
    assert X.dtype == np.int64 and X.tolist() == row["samples"]
    if row["writer"] == "forced":                                        # the writer still writes what was committed
        spec = {n: c for n, _, _, _, _, _, _, c in A.golden_inputs()}[row["name"]]
        assert A.encode(row["samples"], row["nbits"], row["block_size"], row["rsi"], row["preprocess"], A._choose_of(spec)).hex() == row["hex"]


def _blocks(row):
    """The options of a golden stream's blocks, re-read here with a walker of this test's own: [(ri, b, option, k or run length)]."""
    s = "".join(format(b, "08b") for b in bytes.fromhex(row["hex"]))
    n, J, rsi, pp, N = row["nbits"], row["block_size"], row["rsi"], row["preprocess"], len(row["samples"])
    idl, pos, out = A.id_len(n), 0, []

    def ones(count):
        nonlocal pos
        for _ in range(count):
            pos = s.index("1", pos) + 1

    for ri, s0 in enumerate(range(0, N, rsi * J)):
        nb, b = -(-min(rsi * J, N - s0) // J), 0
        while b < nb:
            first = pp and b == 0
            ident = int(s[pos:pos + idl], 2)
            pos += idl
            if ident == 0:
                se = s[pos] == "1"
                pos += 1 + (n if first else 0)
                start = pos
                ones(J // 2 if se else 1)
                if se:
                    out.append((ri, b, "se", 0))
                    b += 1
                else:
                    z = pos - start
                    ros = z == 5
                    z = min(rsi - b, 64 - b % 64) if ros else z - 1 if z > 5 else z
                    out.append((ri, b, "ros" if ros else "zero", z))
                    b += z
            elif ident == (1 << idl) - 1:
                pos += J * n
                out.append((ri, b, "unc", 0))
                b += 1
            else:
                pos += n if first else 0
                start = pos
                ones(J - first)
                out.append((ri, b, "k", ident - 1, pos - start))
                pos += (J - first) * (ident - 1)
                b += 1
    assert pos <= len(s) < pos + 8 and not int(s[pos:] or "0", 2)
    return out


def test_the_fixture_holds_what_it_should():
    rows = {r["name"]: r for r in GOLDEN}
    assert all(len(r["samples"]) <= 640 for r in GOLDEN) and {r["writer"] for r in GOLDEN} == {"libaec", "forced"}
    blocks = {name: _blocks(r) for name, r in rows.items()}
    every = [(name,) + blk for name, v in blocks.items() for blk in v]
    # every option, also as the first block of an RSI (with the preprocessor: where the reference stands)
    for opt in ("unc", "k", "se", "zero"):
        assert any(e[3] == opt and e[2] == 0 and rows[e[0]]["preprocess"] for e in every), opt
        assert any(e[3] == opt and e[2] > 0 for e in every), opt
    # k = 0 and the largest k of each id_len
    for n, idl in ((8, 3), (16, 4), (32, 5)):
        ks = {e[4] for e in every if e[3] == "k" and A.id_len(rows[e[0]]["nbits"]) == idl}
        assert {0, (1 << idl) - 3} <= ks, (n, ks)
    runs = {e[4] for e in every if e[3] == "zero"}
    assert {1, 4} <= runs and any(z >= 6 for z in runs)
    assert any(e[3] == "ros" and e[2] % 64 != 0 for e in every)
    assert any(e[3] == "ros" and 64 - e[2] % 64 < rows[e[0]]["rsi"] - e[2] for e in every)     # ... and one that the segment ends, not the RSI
    # a run that passes n_values: the run's last block lies beyond the last block that holds a sample
    for name in ("forced_ros_past_n_values", "forced_zero_count_past_n_values"):
        r = rows[name]
        _, b, _, z = blocks[name][-1][:4]
        assert (b + z) * r["block_size"] >= len(r["samples"]) + r["block_size"], name
    assert any(e[3] == "k" and e[4] == 0 and e[5] > 2048 for e in every if e[0] == "forced_long_fs")
    assert {r["nbits"] for r in GOLDEN} >= {1, 8, 12, 16, 24, 32} and any(max(r["samples"]) >= 1 << 31 for r in GOLDEN)
    for J in (8, 16, 32, 64):
        assert {1, J - 1, J + 1, 2 * J + 1} <= {len(r["samples"]) for r in GOLDEN if r["block_size"] == J and r["rsi"] == 2}
    assert any(not r["preprocess"] for r in GOLDEN)
    # both branches of the inverse mapping at x near 0 and near xmax: in the "ends" streams a small step (delta <= theta) and a jump to
    # the other end (delta > theta) follow a sample at 0 and one at xmax
    for n in (1, 8, 12, 16, 24, 32):
        X, hi = rows[f"ends_n{n}"]["samples"], (1 << n) - 1
        pairs = set(zip(X, X[1:]))
        assert (0, hi) in pairs and (hi, 0) in pairs and ((0, 1) in pairs or n == 1) and ((hi, hi - 1) in pairs or n == 1)


@needs_libaec
@pytest.mark.parametrize("row", [r for r in GOLDEN], ids=lambda r: r["name"])
def test_libaec_reads_and_writes_the_fixture(row):
    flags = A.PREPROCESS if row["preprocess"] else 0
    back = A.libaec_decode(bytes.fromhex(row["hex"]), len(row["samples"]), row["nbits"], row["block_size"], row["rsi"], flags)
    assert back is not None and back.tolist() == row["samples"]
    if row["writer"] == "libaec":
        assert A.libaec_encode(row["samples"], row["nbits"], row["block_size"], row["rsi"], flags).hex() == row["hex"]


@needs_libaec
@pytest.mark.parametrize("kind", ["smooth", "noisy", "constant", "near_constant", "ends"])
def test_random_fields_against_libaec(kind):
    rng = np.random.default_rng({"smooth": 1, "noisy": 2, "constant": 3, "near_constant": 4, "ends": 5}[kind])
    for trial in range(60):
        n = int(rng.choice([1, 2, 7, 8, 12, 16, 17, 24, 31, 32]))
        J, rsi = int(rng.choice([8, 16, 32, 64])), int(rng.choice([1, 2, 8, 64, 128, 512, 4096]))
        flags = A.PREPROCESS if trial % 5 else 0
        count = int(rng.choice([1, J - 1, J + 1, 33, rsi * J + 1, 4097, 6149])) if trial % 2 else int(rng.integers(1, 3000))
        hi = (1 << n) - 1
        if kind == "smooth":
            X = A.smooth(rng, count, n, step=int(rng.choice([1, 9, 300])))
        elif kind == "noisy":
            X = rng.integers(0, hi + 1, size=count, dtype=np.uint64).tolist()
        elif kind == "constant":
            X = [int(rng.integers(0, hi + 1))] * count
        elif kind == "near_constant":
            X = np.minimum(A.near_constant(rng, count, n), hi).tolist()
        else:
            X = np.where(rng.random(count) < 0.5, hi - rng.integers(0, min(hi, 3) + 1, size=count), rng.integers(0, min(hi, 3) + 1, size=count)).tolist()
        data = A.libaec_encode(X, n, J, rsi, flags)
        got = codec.aec_decode(data, count, n, flags, J, rsi)
        assert got.tolist() == [int(v) for v in X], (kind, trial, n, J, rsi, flags, count)


def test_damaged_streams_are_refused_not_read_past():
    row = GOLDEN[0]
    data = bytes.fromhex(row["hex"])
    for cut in range(1, len(data) + 1):
        with pytest.raises(codec.CodecError, match="damaged or ends"):
            codec.aec_decode(data[:-cut], 28, 8, 8, 8, 2)
    with pytest.raises(codec.CodecError):
        codec.aec_decode(b"", 1, 8, 8, 8, 2)
    # a zero run beyond the RSI's last block, a second-extension code above 90, a delta above xmax
    idl = 3
    run = A.bits(0, idl) + "0" + A.bits(5, 8) + A.fs(2)                      # 3 zero blocks where the RSI has 2
    se = A.bits(0, idl) + "1" + A.bits(5, 8) + A.fs(91) + A.fs(0) * 3
    big = A.bits(5, idl) + A.bits(5, 8) + A.fs(16) + A.fs(0) * 6 + A.bits(0, 4) * 7   # k = 4, q = 16: delta = 256 in 8 bits
    for s in (run, se, big):
        s += "0" * (-len(s) % 8)
        with pytest.raises(codec.CodecError, match="damaged or ends"):
            codec.aec_decode(int(s, 2).to_bytes(len(s) // 8, "big"), 8, 8, 8, 8, 2)
    for bad in (dict(flags=1), dict(flags=16), dict(flags=32), dict(flags=64), dict(J=12), dict(rsi=0), dict(rsi=4097), dict(n=33)):
        with pytest.raises(codec.CodecError):
            codec.aec_decode(data, 28, bad.get("n", 8), bad.get("flags", 8), bad.get("J", 8), bad.get("rsi", 2))
    assert codec.aec_decode(data, 28, 8, 8 | 4 | 2, 8, 2).tolist() == row["samples"]        # flags 2 and 4 do not touch the stream
    assert codec.aec_decode(b"", 0, 8, 8, 8, 2).tolist() == []


# ---------------------------------------------------------------------------------------
# the catalogue on the host route
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_case_on_the_host_route(case, files):
    gf = grib.GribFile(files[case.name])
    f = gf.select(case.var)
    want = case.expected
    got = gf.read(case.var)
    _same_bits(got, want)
    assert f.shape == want.shape and list(f.time) == [pd.Timestamp(t) for t in case.times]
    raw = open(files[case.name], "rb").read()
    for m, st in zip(f.messages, case.steps):
        if isinstance(st, A.AStep):
            assert (m.packing, m.n_values, m.nbits, m.ccsds_flags, m.block_size, m.rsi, m.E, m.D, m.R) == \
                (42, len(st.X), st.nbits, st.flags, st.J, st.rsi, st.E, st.D, st.R)
            assert raw[m.data_offset:m.data_offset + m.data_length] == st.body
            assert grib.unpack_ccsds(m, st.body).tolist() == st.X                # the integers, before any float
        else:
            assert (m.packing, m.nbits) == (0, st.nbits)
    ds = af.dataset_from_path(files[case.name], case.var, device=None)
    _same_bits(np.asarray(ds.cube()), want)
    a = f.arrays()
    assert a["packing"].tolist() == [m.packing for m in f.messages] and a["rsi"].tolist() == [m.rsi for m in f.messages]
    assert a["block_size"].tolist() == [m.block_size for m in f.messages] and a["ccsds_flags"].tolist() == [m.ccsds_flags for m in f.messages]


@needs_libaec
def test_a_file_of_libaec_streams_at_the_defaults(tmp_path):
    """Section 7 written by libaec itself at ecCodes' defaults (J = 32, rsi = 128, flags 14), 70 x 61: one full RSI and a short one."""
    rng = np.random.default_rng(11)
    nj, ni = 70, 61
    grid = (ni, nj, 50.0, 230.0, 50.0 - 0.25 * (nj - 1), 230.0 + 0.25 * (ni - 1), 0x00)
    steps = []
    for k in range(3):
        X = A.smooth(rng, nj * ni, 16, step=40)
        steps.append(A.AStep(X, 16, E=-4, R=250.0, valid=A.hours(k), stream=A.libaec_encode(X, 16, 32, 128, A.PREPROCESS)))
    case = C.Case("libaec_defaults", "t2m", [A.message(s, grid) for s in steps], steps, grid=grid, edition=2)
    _same_bits(grib.GribFile(case.write(tmp_path)).read("t2m"), case.expected)


def test_the_catalogue_covers_what_it_should():
    steps = [s for c in CASES for s in c.steps if isinstance(s, A.AStep)]
    assert {s.nbits for s in steps} >= {0, 1, 8, 12, 16, 24, 32} and {s.J for s in steps} == {8, 16, 32, 64}
    assert {1, 128, 4096} <= {s.rsi for s in steps} and any(not s.flags & A.PREPROCESS for s in steps)
    assert any(s.bitmap is not None and 0 < len(s.X) < A.NP for s in steps) and any(s.nbits == 0 and s.body == b"" for s in steps)
    assert any(isinstance(s, C.Step) for s in BY["a_shuffled"].steps) is False and len(BY["a_shuffled"].pieces) > 2 * C.STEPS
    assert len({(s.E, s.D, s.R, s.nbits, s.J, s.rsi) for s in BY["a_varying_forced_options"].steps}) == C.STEPS
    assert np.isnan(BY["a_bitmap"].expected).any()


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,raw,reason,at_index", A.refusals(), ids=[r[0] for r in A.refusals()])
def test_refusals_name_their_reason(name, raw, reason, at_index, tmp_path):
    path = str(tmp_path / (name + ".grib2"))
    with open(path, "wb") as f:
        f.write(raw)
    if at_index:
        with pytest.raises(ValueError, match=re.escape(reason)):
            grib.GribFile(path)
    else:
        gf = grib.GribFile(path)                                          # the headers are sound: the stream is not
        with pytest.raises(ValueError, match=re.escape(reason)):
            gf.read("t2m")
    with pytest.raises(ValueError, match=re.escape(reason)) as e:
        af.dataset_from_path(path, "t2m", device=None, lon_is_360=False)
    assert "5.42" in str(e.value) or name == "nbits_33"                      # (the width is checked before the template's own octets)


def test_the_earlier_catalogues_still_refuse_their_short_section_5(tmp_path):
    """A message whose template number is 42 over the 21 octets of template 5.0 (tests/grib_cases.py: e2_ccsds) fails on its length."""
    rng = np.random.default_rng(7)
    path = str(tmp_path / "short.grib2")
    with open(path, "wb") as f:
        f.write(C.message2(C.field(rng, 12, 0), C.GRID, drt=42))
    with pytest.raises(ValueError, match=re.escape("data representation section of 21 bytes for template 5.42 (CCSDS), which takes 25")):
        grib.GribFile(path)


# ---------------------------------------------------------------------------------------
# the routes around the decode, and the C ABI
# ---------------------------------------------------------------------------------------
def test_time_coordinate_step_bytes_and_time_sel(files):
    case = BY["a_shuffled"]
    assert afio.read_time_coordinate(files[case.name], "t2m").equals(pd.DatetimeIndex(case.times))
    assert D._step_bytes(files[case.name], "t2m") == A.NJ * A.NI * 4
    ds = af.dataset_from_path(files[case.name], "t2m", time_sel=slice("2024-07-15T01:00", "2024-07-15T03:00"), lon_is_360=False)
    _same_bits(np.asarray(ds.cube()), case.expected[1:4])


def test_header_exports_and_record_size():
    hdr = open(os.path.join(ROOT, "include", "aggfly_hip.h")).read()
    assert "#define AFHIP_ABI_VERSION 4" in hdr and hip.ABI_VERSION == 4                     # additive: the ABI version stays
    for name in ("afhip_grib_unpack_ccsds", "afhip_grib_ccsds_scratch_bytes"):
        assert name in hip.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    chdr = open(os.path.join(ROOT, "include", "aggfly_codec.h")).read()
    assert "afcodec_aec_decode" in codec.EXPORTS and re.search(r"\bafcodec_aec_decode\s*\(", chdr)
    assert hip.GRIB_STEP.itemsize == 64 and hip.GRIB_CSTEP.itemsize == 112                   # the other entries are as they were
    body = re.search(r"typedef struct afhip_grib_astep \{(.*?)\} afhip_grib_astep;", hdr, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    sizes = {"int64_t": ("<i8", 8), "int32_t": ("<i4", 4), "double": ("<f8", 8)}
    assert [(n, sizes[t][0]) for n, t in fields] == [(n, hip.GRIB_ASTEP[n].str) for n in hip.GRIB_ASTEP.names]
    assert hip.GRIB_ASTEP.itemsize == sum(sizes[t][1] for _, t in fields) == 72
    # the passes' own record (aec_passes.h) has the same fields in the same order
    passes = open(os.path.join(ROOT, "aggfly_amd", "csrc", "aec_passes.h")).read()
    rec = re.search(r"typedef struct aec_step \{(.*?)\} aec_step;", passes, re.S).group(1)
    names = [n.strip() for decl in re.sub(r"/\*.*?\*/", "", rec, flags=re.S).split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == list(hip.GRIB_ASTEP.names)
    lib = hip.load()
    assert lib.afhip_grib_ccsds_scratch_bytes.restype is ctypes.c_int64
    # the size query: monotone, 16-byte multiples, -1 for absurd sizes
    one = hip.grib_ccsds_scratch_bytes(1, 4270, 2)
    assert one % 16 == 0 and one >= 4270 * 4 + 2 * 8 and hip.grib_ccsds_scratch_bytes(3, 4270, 2) >= 3 * (4270 * 4 + 2 * 8)
    assert hip.grib_ccsds_scratch_bytes(0, 4270, 0) >= 0
    for bad in ((-1, 10, 1), (1, 0, 1), (1, 1 << 31, 1), (1, 10, -1), (1, 10, 1 << 31), (1 << 31, 10, 1), ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1)):
        with pytest.raises(ValueError):
            hip.grib_ccsds_scratch_bytes(*bad)
