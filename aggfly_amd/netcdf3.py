"""Header reader for NetCDF classic files (CDF-1, CDF-2), written from the format specification ("The NetCDF Classic
Format Specification", NetCDF User's Guide, appendix C).  It tells where the bytes of every time step of a variable lie in the
file; the data are never touched here.  `io._netcdf3_to_device` `pread`s those bytes into page-locked memory and a kernel
(`hip.place_box_swapped`) turns their big-endian elements into the cube in HBM.

    header   = magic numrecs dim_list gatt_list var_list
    magic    = 'C' 'D' 'F' version            version 1: 32-bit offsets, 2: 64-bit offsets (5: CDF-5, refused)
    dim_list = ABSENT | NC_DIMENSION nelems [name length ...]         length 0 marks the record dimension
    att_list = ABSENT | NC_ATTRIBUTE nelems [name type nelems values ...]
    var_list = ABSENT | NC_VARIABLE  nelems [name nelems [dimid ...] att_list type vsize begin ...]

Everything is big-endian; names and attribute values are padded to 4 bytes.  The fixed variables follow the header, each one
contiguous block at ``begin``; then come ``numrecs`` records of ``recsize`` bytes, each holding one step of every record
variable, so step ``t`` of a record variable lies at ``begin + t * recsize``.  ``recsize`` is the sum of the record variables'
per-record sizes, each padded to 4 bytes — except that a file with exactly ONE record variable does not pad it.  Sizes are
computed from the dimensions and the type: the header's ``vsize`` saturates at 2^32 - 1 in CDF-2 files and is not read.

Whatever is refused raises ValueError with the reason, and `io.dataset_from_path` reads the file on the host route.
"""
from __future__ import annotations

import os
import struct

import numpy as np

NC_DIMENSION, NC_VARIABLE, NC_ATTRIBUTE = 0x0A, 0x0B, 0x0C
# nc_type -> the dtype as stored (big-endian); NC_CHAR is bytes
NC_TYPES = {1: np.dtype(">i1"), 2: np.dtype("S1"), 3: np.dtype(">i2"), 4: np.dtype(">i4"), 5: np.dtype(">f4"), 6: np.dtype(">f8")}
STREAMING = 0xFFFFFFFF
STREAMED_TYPES = ("i2", "i4", "f4", "f8")         # short / int / float / double: what the device route takes (kind + itemsize)


def is_classic(path) -> bool:
    """Does ``path`` start with the magic of a NetCDF classic file (any version, CDF-5 included)?"""
    try:
        with open(path, "rb") as f:
            m = f.read(4)
    except (OSError, TypeError):
        return False
    return len(m) == 4 and m[:3] == b"CDF" and m[3] in (1, 2, 5)


class _Truncated(ValueError):
    pass


class _Cursor:
    def __init__(self, buf: bytes, size: int):
        self.buf, self.pos, self.size = buf, 0, size          # size: of the whole file, of which buf is the head

    def take(self, n: int) -> bytes:
        if n < 0 or self.pos + n > len(self.buf):
            raise _Truncated("truncated header")
        out = self.buf[self.pos:self.pos + n]
        self.pos += n
        return out

    def u32(self) -> int:
        return struct.unpack(">I", self.take(4))[0]

    def u64(self) -> int:
        return struct.unpack(">Q", self.take(8))[0]

    def count(self, what: str, each: int) -> int:
        """An element count: a non-negative 32-bit integer no larger than the header bytes left could hold."""
        n = self.u32()
        if n >= 0x80000000:
            raise ValueError(f"negative count of {what} ({n - (1 << 32)})")
        if n * each > self.size - self.pos:
            raise ValueError(f"absurd count of {what} ({n}: more than the file could hold)")
        return n

    def name(self) -> str:
        n = self.count("name bytes", 1)
        s = self.take(n)
        self.take(-n % 4)
        return s.decode("utf-8")


class Variable:
    """One variable of a classic file: where it lies and what its header says (no data)."""

    def __init__(self, name, dims, shape, dtype, attrs, begin, is_record, plane_bytes):
        self.name, self.dims, self.shape, self.dtype, self.attrs = name, tuple(dims), tuple(shape), dtype, attrs
        self.begin, self.is_record, self.plane_bytes = int(begin), bool(is_record), int(plane_bytes)
        self.recsize = 0                      # the file's record size (record variables; set by NC3File)

    @property
    def step_stride(self) -> int:
        """Bytes from one step of the leading axis to the next."""
        return self.recsize if self.is_record else self.plane_bytes

    def plane_offset(self, t: int) -> int:
        """Byte offset in the file of step ``t`` of the leading axis: ``plane_bytes`` contiguous bytes, C order, big-endian."""
        if not self.shape or not (0 <= t < self.shape[0]):
            raise IndexError(f"step {t} outside the {self.shape[0] if self.shape else 0} steps of {self.name!r}")
        return self.begin + int(t) * self.step_stride

    def __repr__(self):
        return f"<netcdf3.Variable {self.name!r} {self.dtype.str} {dict(zip(self.dims, self.shape))} begin={self.begin}>"


class NC3File:
    """The parsed header of a classic file: ``version``, ``numrecs``, ``dimensions`` {name: length, None for the record
    dimension}, ``attrs`` (global), ``variables`` {name: `Variable`}, ``recsize``."""

    def __init__(self, path):
        self.path = path
        size = os.path.getsize(path)
        want = 1 << 16
        with open(path, "rb") as f:
            while True:
                f.seek(0)
                buf = f.read(min(want, size))
                try:
                    self._parse(_Cursor(buf, size), size)
                    break
                except _Truncated:
                    if len(buf) >= size:
                        raise ValueError(f"{path}: truncated header") from None
                    want *= 8                                     # a header longer than the bytes read so far
        self.size = size

    # ---- parsing ----
    @staticmethod
    def _values(cur, what):
        code = cur.u32()
        if code not in NC_TYPES:
            raise ValueError(f"unknown type code {code} of {what}")
        dt = NC_TYPES[code]
        n = cur.count(f"values of {what}", dt.itemsize)
        raw = cur.take(n * dt.itemsize)
        cur.take(-(n * dt.itemsize) % 4)
        return code, n, raw

    def _attrs(self, cur, what):
        tag = cur.u32()
        n = cur.count(f"attributes of {what}", 12)
        if tag == 0 and n == 0:
            return {}
        if tag != NC_ATTRIBUTE:
            raise ValueError(f"attribute list of {what} starts with tag {tag:#x}")
        out = {}
        for _ in range(n):
            name = cur.name()
            code, cnt, raw = self._values(cur, f"attribute {name!r}")
            if code == 2:                                         # char: text, as the host route hands it on
                out[name] = raw.decode("utf-8", "replace")
            else:
                v = np.frombuffer(raw, dtype=NC_TYPES[code]).astype(NC_TYPES[code].newbyteorder("="))
                out[name] = v[0] if cnt == 1 else v               # one element: a scalar
        return out

    def _parse(self, cur, size):
        magic = cur.take(4)
        if magic[:3] != b"CDF":
            raise ValueError("not a NetCDF classic file")
        self.version = magic[3]
        if self.version == 5:
            raise ValueError("CDF-5 (64-bit data) files are not read")
        if self.version not in (1, 2):
            raise ValueError(f"unknown classic format version {self.version}")
        self.numrecs = cur.u32()
        if self.numrecs == STREAMING:
            raise ValueError("numrecs is the streaming marker (0xFFFFFFFF): the record count is not in the header")
        tag = cur.u32()
        n = cur.count("dimensions", 8)
        if not (tag == NC_DIMENSION or (tag == 0 and n == 0)):
            raise ValueError(f"dimension list starts with tag {tag:#x}")
        names, lengths, self.record_dim = [], [], None
        for i in range(n):
            names.append(cur.name())
            ln = cur.u32()
            if ln >= 0x80000000:
                raise ValueError(f"negative length of dimension {names[-1]!r}")
            if ln == 0:
                if self.record_dim is not None:
                    raise ValueError("more than one record dimension")
                self.record_dim = i
            lengths.append(ln)
        self.dimensions = {nm: (None if i == self.record_dim else ln) for i, (nm, ln) in enumerate(zip(names, lengths))}
        self.attrs = self._attrs(cur, "the file")
        tag = cur.u32()
        n = cur.count("variables", 28)
        if not (tag == NC_VARIABLE or (tag == 0 and n == 0)):
            raise ValueError(f"variable list starts with tag {tag:#x}")
        self.variables = {}
        for _ in range(n):
            name = cur.name()
            rank = cur.count(f"dimensions of {name!r}", 4)
            ids = [cur.u32() for _ in range(rank)]
            if any(i >= len(names) for i in ids):
                raise ValueError(f"variable {name!r} names a dimension that does not exist")
            attrs = self._attrs(cur, f"variable {name!r}")
            code = cur.u32()
            if code not in NC_TYPES:
                raise ValueError(f"unknown type code {code} of variable {name!r}")
            cur.u32()                                             # vsize: not read (saturates in CDF-2), sizes come from the dimensions
            begin = cur.u32() if self.version == 1 else cur.u64()
            is_record = rank > 0 and ids[0] == self.record_dim
            if self.record_dim in ids[1:]:
                raise ValueError(f"variable {name!r} has the record dimension on an inner axis")
            inner = [lengths[i] for i in (ids[1:] if rank else [])]
            lead = [] if rank == 0 else [self.numrecs if is_record else lengths[ids[0]]]
            plane = NC_TYPES[code].itemsize
            for ln in inner:
                plane *= ln                                       # (Python integers: no overflow)
            self.variables[name] = Variable(name, [names[i] for i in ids], lead + inner, NC_TYPES[code], attrs, begin, is_record, plane)
        self.header_bytes = cur.pos
        recs = [v for v in self.variables.values() if v.is_record]
        self.recsize = recs[0].plane_bytes if len(recs) == 1 else sum(v.plane_bytes + (-v.plane_bytes % 4) for v in recs)
        for v in self.variables.values():
            if v.is_record:
                v.recsize = self.recsize
                if self.numrecs == 0:
                    continue                                      # no step of it is in the file: `begin` is where the first would go
                last = v.begin + (self.numrecs - 1) * self.recsize + v.plane_bytes
            else:
                last = v.begin + v.plane_bytes * (v.shape[0] if v.shape else 1)
            if v.begin < self.header_bytes:
                raise ValueError(f"variable {v.name!r} begins inside the header (begin = {v.begin})")
            if v.begin > size:
                raise ValueError(f"variable {v.name!r} begins beyond the end of the file (begin = {v.begin}, {size} bytes)")
            if last > size:
                raise ValueError(f"variable {v.name!r} ends beyond the end of the file ({last} > {size} bytes): "
                                 + ("the last record is not there" if v.is_record else "the file is cut short"))

    # ---- small reads (coordinates) ----
    def read(self, name) -> np.ndarray:
        """The whole variable ``name`` as a big-endian array: for the coordinates.  A fixed variable is one read; a record variable
        one `pread` per record (mapping the file instead costs a page fault per record: 24 against 6 ms for a year of hourly steps)."""
        v = self.variables[name]
        count = 1
        for n in v.shape:
            count *= n
        if count == 0:
            return np.empty(v.shape, dtype=v.dtype)
        fd = os.open(self.path, os.O_RDONLY)
        try:
            if v.is_record and v.step_stride != v.plane_bytes:
                raw = b"".join(os.pread(fd, v.plane_bytes, v.begin + t * v.step_stride) for t in range(v.shape[0]))
            else:
                raw = os.pread(fd, count * v.dtype.itemsize, v.begin)
        finally:
            os.close(fd)
        if len(raw) != count * v.dtype.itemsize:
            raise ValueError(f"{self.path}: variable {name!r} is cut short")
        return np.frombuffer(raw, dtype=v.dtype).reshape(v.shape).copy()
