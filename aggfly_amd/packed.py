"""A 16-bit-packed climate cube that stays packed in HBM (`PackedCube`).

ERA5-style files store a field as int16 with ``scale_factor`` / ``add_offset`` / ``_FillValue``; other gridded products use
uint16, or int16 with the netCDF attribute ``_Unsigned = "true"`` (the same bits).  The default device routes
unpack such a cube to float32 once it is in HBM (`io.array_to_device`: ``post``): 4 bytes per cell and step for data that
carries 2.  A `PackedCube` keeps the stored integers and the rule that turns them into values; the temporal kernel of the HIP
library unpacks each element where it uses it (``AFHIP_I16`` / ``AFHIP_U16`` plans, include/aggfly_hip.h), so the cube takes half the HBM and
the kernel reads half the bytes.

The holder is deliberately NOT a tensor.  It offers what `DataArray` and the engine need around the hot path — shape, views,
indexing, and arithmetic with a real scalar, which is folded into the unpack rule — and nothing that would let code that does
not know it read the integers as values: there is no ``data_ptr``, no ``__array__``, and every other operation first
materialises the float32 values (`materialize`, the library's ``afhip_unpack_i16`` / ``afhip_unpack_u16``) and continues on those.

The unpack rule is a chain of at most three (multiply, add) pairs in float32, one rounding per operation and never a fused
multiply-add — bit for bit what torch computes for ``q.to(float32) * scale + offset - 273.15`` one operation at a time; the
fill value becomes NaN.

Unsigned storage is held as an int16 tensor of the same bits plus ``unsigned=True`` (a `view`, never a conversion): torch's
uint16 has no indexing or arithmetic kernels, while every view, slice and move the holder offers works on int16.  Only the
library's unpack reads the flag.
"""
from __future__ import annotations

import numpy as np

MAX_PAIRS = 3          # MAX_PACK_PAIRS of the library (afhip_packing.mul / .add)


def _real_scalar(c) -> bool:
    """A Python int / float (np.float64 is one): what torch treats as a weak scalar beside a float32 tensor."""
    return isinstance(c, (int, float)) and not isinstance(c, bool)


class PackedCube:
    """``q``: an int16 or uint16 torch tensor (HBM, or the host before `to`) or numpy array of stored values.
    ``scale_factor`` / ``add_offset``: the CF attributes (None: absent — that half of the first pair is left out, as the
    float32 route leaves it out); ``fill_value``: the stored integer that means missing (None or NaN: none), in the range of
    the storage; ``unsigned``: the 16 bits are uint16 (None: what ``q``'s dtype says; True beside int16 bits: read them as
    unsigned, the way ``_Unsigned = "true"`` asks)."""

    _aggfly_packed = True

    def __init__(self, q, scale_factor=None, add_offset=None, fill_value=None, unsigned=None, _pairs=None):
        import torch
        if isinstance(q, np.ndarray):
            if q.dtype not in (np.int16, np.uint16):
                raise TypeError(f"PackedCube holds int16 or uint16 storage, got {q.dtype}")
            q = torch.from_numpy(q)
        if not isinstance(q, torch.Tensor) or q.dtype not in (torch.int16, torch.uint16):
            raise TypeError(f"PackedCube holds an int16 or uint16 tensor, got {getattr(q, 'dtype', type(q).__name__)}")
        if q.dtype == torch.uint16:
            if unsigned is not None and not unsigned:
                raise ValueError("uint16 storage cannot be read as signed")
            q, unsigned = q.view(torch.int16), True            # the same bits
        self.q = q
        self.unsigned = bool(unsigned)
        if fill_value is not None and isinstance(fill_value, float) and np.isnan(fill_value):
            fill_value = None
        if fill_value is not None:
            lo, hi = (0, 65535) if self.unsigned else (-32768, 32767)
            if int(fill_value) != fill_value or not lo <= int(fill_value) <= hi:
                raise ValueError(f"fill_value {fill_value!r} is no {self.storage} value")
            fill_value = int(fill_value)
        self.fill_value = fill_value
        if _pairs is not None:
            self.pairs = [tuple(p) for p in _pairs]
        else:
            self.pairs = []
            if scale_factor is not None or add_offset is not None:
                self.pairs.append((None if scale_factor is None else np.float32(scale_factor),
                                   None if add_offset is None else np.float32(add_offset)))
        if len(self.pairs) > MAX_PAIRS:
            raise ValueError(f"at most {MAX_PAIRS} (multiply, add) pairs")

    # ---- what the values look like ----
    @property
    def shape(self):
        return self.q.shape

    @property
    def ndim(self):
        return self.q.ndim

    @property
    def dtype(self):
        """The dtype of the VALUES: float32."""
        import torch
        return torch.float32

    @property
    def storage(self) -> str:
        """What the 16 stored bits are: "int16" or "uint16"."""
        return "uint16" if self.unsigned else "int16"

    @property
    def device(self):
        return self.q.device

    @property
    def is_cuda(self):
        return self.q.is_cuda

    @property
    def n_pairs(self) -> int:
        return len(self.pairs)

    def numel(self):
        return self.q.numel()

    def nbytes(self) -> int:
        """Bytes the cube holds in memory: 2 per value."""
        return int(self.q.numel()) * 2

    def __len__(self):
        return len(self.q)

    def _like(self, q, pairs=None):
        return PackedCube(q, fill_value=self.fill_value, unsigned=self.unsigned, _pairs=self.pairs if pairs is None else pairs)

    # ---- views and copies: on the integers, the rule rides along ----
    def permute(self, *order):
        return self._like(self.q.permute(*order))

    def transpose(self, a, b):
        return self._like(self.q.transpose(a, b))

    def contiguous(self):
        return self if self.q.is_contiguous() else self._like(self.q.contiguous())

    def is_contiguous(self):
        return self.q.is_contiguous()

    def clone(self):
        return self._like(self.q.clone())

    def unsqueeze(self, axis):
        return self._like(self.q.unsqueeze(axis))

    def __getitem__(self, key):
        return self._like(self.q[key])

    def to(self, *args, **kwargs):
        """A move between devices keeps the cube packed; a dtype asks for values and materialises."""
        import torch
        if any(isinstance(a, torch.dtype) for a in args) or "dtype" in kwargs:
            return self.materialize().to(*args, **kwargs)
        return self._like(self.q.to(*args, **kwargs))

    def cuda(self, *args, **kwargs):
        return self._like(self.q.cuda(*args, **kwargs))

    # ---- arithmetic with a real scalar folds into the rule; everything else works on the values ----
    def _fold_add(self, c):
        c = np.float32(c)                      # torch's scalar semantics beside a float32 tensor: the scalar is cast to float32
        pairs = list(self.pairs)
        if pairs and pairs[-1][1] is None:
            pairs[-1] = (pairs[-1][0], c)
        elif len(pairs) < MAX_PAIRS:
            pairs.append((None, c))
        else:
            return None
        return self._like(self.q, pairs)

    def _fold_mul(self, c):
        c = np.float32(c)
        if len(self.pairs) >= MAX_PAIRS:
            return None
        return self._like(self.q, list(self.pairs) + [(c, None)])

    def __add__(self, o):
        out = self._fold_add(o) if _real_scalar(o) else None
        return self.materialize() + o if out is None else out

    __radd__ = __add__                         # float32 addition commutes exactly

    def __sub__(self, o):
        # x - c == x + (-c) exactly: the cast of c to float32 and the negation commute
        out = self._fold_add(-float(o)) if _real_scalar(o) else None
        return self.materialize() - o if out is None else out

    def __mul__(self, o):
        out = self._fold_mul(o) if _real_scalar(o) else None
        return self.materialize() * o if out is None else out

    __rmul__ = __mul__

    def __rsub__(self, o): return o - self.materialize()
    def __truediv__(self, o): return self.materialize() / o
    def __rtruediv__(self, o): return o / self.materialize()
    def __pow__(self, o): return self.materialize() ** o
    def __neg__(self): return -self.materialize()

    def detach(self):
        """The values (what ``DataArray.values`` walks through ``detach().cpu().numpy()``)."""
        return self.materialize()

    def cpu(self):
        return self.materialize().cpu()

    # ---- the library's view ----
    def packing(self):
        """The rule as the library's ``afhip_packing``: a pair half the chain lacks travels as its exact identity (multiply by 1.0,
        add -0.0: ``x + -0.0 == x`` for every x, the sign of zero included).  The signedness is not part of it: the library takes
        it from the plan's dtype (`hip._dtype_code`) or from the entry point (`hip.unpack_i16`), and ignores ``pad``."""
        from . import hip
        p = hip.Packing()
        p.n_pairs = len(self.pairs)
        p.has_fill = 0 if self.fill_value is None else 1
        p.fill = 0 if self.fill_value is None else self.fill_value
        for i in range(MAX_PAIRS):
            m, a = self.pairs[i] if i < len(self.pairs) else (None, None)
            p.mul[i] = 1.0 if m is None else float(m)
            p.add[i] = -0.0 if a is None else float(a)
        return p

    def materialize(self):
        """The float32 values as an HBM tensor of the same shape (``afhip_unpack_i16`` / ``afhip_unpack_u16``: the kernel's own unpack rule).  Raises
        `hip.HipEngineError` without a GPU: the values have no host form here."""
        from . import hip
        hip.require_gpu()
        return hip.unpack_i16(self)

    def __repr__(self):
        return f"<aggfly_amd.PackedCube {self.storage} {tuple(self.shape)} pairs={self.pairs} fill={self.fill_value} on {self.device}>"


def is_packed(x) -> bool:
    return isinstance(x, PackedCube)
