"""The tables of the poisoned-scratch and far-offset tests cannot fall behind include/aggfly_hip.h: every `afhip_*` entry that takes
caller-owned scratch (a parameter named scratch_dev, workspace_dev, rank_dev, tmp_dev or slots_dev) has a row in
`poison.POISON_ENTRIES`, every entry that places into or takes from a cube (extents NY / NX with an origin t0) or that reads records
with a `dst_off` / `out_off` field has a row in `test_gpu_far_offsets.FAR_ENTRIES`, every row names a test file that is there and
speaks of the entry, and no row names an entry the header no longer has.  A new entry without a row fails here."""
import os
import re

import poison
import test_gpu_far_offsets as far

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRATCH_PARAMS = {"scratch_dev", "workspace_dev", "rank_dev", "tmp_dev", "slots_dev"}


def _header():
    text = open(os.path.join(ROOT, "include", "aggfly_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _entries(code):
    """name -> [(type, parameter name)] of every function the header declares."""
    out = {}
    for m in re.finditer(r"\b(afhip_\w+)\s*\(([^;{}]*?)\)\s*;", code, flags=re.S):
        params = []
        for p in m.group(2).split(","):
            p = " ".join(p.split())
            if p and p != "void":
                pm = re.match(r"(.*?)(\w+)$", p)
                params.append((pm.group(1).strip(), pm.group(2)))
        out[m.group(1)] = params
    return out


def _record_types(code):
    """The struct types of the header that carry a destination offset."""
    return {m.group(2) for m in re.finditer(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", code, flags=re.S)
            if re.search(r"\b(dst_off|out_off)\b", m.group(1))}


def test_the_header_parses_as_expected():
    code = _header()
    entries, records = _entries(code), _record_types(code)
    assert len(entries) >= 55 and {"afhip_plan_run", "afhip_place_box", "afhip_zstd_decode", "afhip_last_error"} <= set(entries)
    assert [n for _, n in entries["afhip_delta_decode"]] == ["stage_dev", "n_chunks", "chunk_elems", "elem_size", "scratch_dev", "scratch_bytes", "stream"]
    assert records == {"afhip_lz4_stream", "afhip_shuffle_block", "afhip_copy_range", "afhip_zstd_encode_block", "afhip_zstd_frame", "afhip_inflate_stream"}


def test_every_entry_with_caller_owned_scratch_is_in_the_poison_table():
    entries = _entries(_header())
    need = {name for name, params in entries.items() if SCRATCH_PARAMS & {n for _, n in params}}
    assert need - set(poison.POISON_ENTRIES) == set(), "entries with scratch and no poison test"
    assert set(poison.POISON_ENTRIES) - need == set(), "rows whose entry takes no scratch (or is gone)"


def test_every_placing_entry_and_every_offset_record_is_in_the_far_offset_table():
    code = _header()
    entries, records = _entries(code), _record_types(code)
    need = set()
    for name, params in entries.items():
        names = {n for _, n in params}
        places = "t0" in names and any(re.fullmatch(r"(cube_)?NX", n) for n in names)
        takes_records = any(t.replace("const", "").replace("*", "").strip() in records for t, _ in params)
        if places or takes_records:
            need.add(name)
    assert need - set(far.FAR_ENTRIES) == set(), "entries that write at an offset and have no far-offset test"
    assert set(far.FAR_ENTRIES) - need == set(), "rows whose entry neither places nor reads offset records (or is gone)"


def test_every_row_names_a_test_file_that_speaks_of_the_entry():
    rows = [(e, f) for e, (f, _) in poison.POISON_ENTRIES.items()] + [(e, "test_gpu_far_offsets.py") for e in far.FAR_ENTRIES]
    for entry, fname in rows:
        path = os.path.join(ROOT, "tests", fname)
        assert os.path.exists(path), (entry, fname)
        text = open(path).read()
        short = entry[len("afhip_"):]
        assert short in text or entry in text, f"{fname} does not mention {short}"
