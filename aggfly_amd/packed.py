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

A cube concatenated from several stores — yearly or monthly ERA5 files, each with its own ``scale_factor`` / ``add_offset`` and
often its own ``_FillValue`` — carries one rule per store: ``rules`` along its time axis, rule ``i`` for the time steps
``rule_bounds[i] .. rule_bounds[i + 1]`` (`PackedCube.concat`).  The kernel picks the rule per row (a row of the cube is a time step),
so such a record stays packed too.  Neighbouring equal rules merge: stores that share their packing give a single-rule cube.

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


def _fold_add_pairs(pairs, c):
    """``pairs`` followed by ``+ c`` (c a float32), or None when the chain is full."""
    pairs = list(pairs)
    if pairs and pairs[-1][1] is None:
        pairs[-1] = (pairs[-1][0], c)
    elif len(pairs) < MAX_PAIRS:
        pairs.append((None, c))
    else:
        return None
    return pairs


def _fold_mul_pairs(pairs, c):
    return None if len(pairs) >= MAX_PAIRS else list(pairs) + [(c, None)]


def _same_rule(a, b) -> bool:
    return a[1] == b[1] and len(a[0]) == len(b[0]) and all(
        (x is None) == (y is None) and (x is None or np.float32(x).tobytes() == np.float32(y).tobytes())
        for pa, pb in zip(a[0], b[0]) for x, y in zip(pa, pb))


def _join_rules(rules, bounds):
    """Drop the rules that cover no time step, merge equal neighbours -> (rules, bounds); of nothing but empty parts the first rule."""
    out_r, out_b = [], [0]
    for r, lo, hi in zip(rules, bounds[:-1], bounds[1:]):
        if hi <= lo:
            continue
        if out_r and _same_rule(out_r[-1], r):
            out_b[-1] = out_b[-1] + (hi - lo)
        else:
            out_r.append(r)
            out_b.append(out_b[-1] + (hi - lo))
    if not out_r:
        out_r, out_b = [rules[0]], [0, 0]
    return out_r, out_b


class PackedCube:
    """``q``: an int16 or uint16 torch tensor (HBM, or the host before `to`) or numpy array of stored values, time-leading.
    ``scale_factor`` / ``add_offset``: the CF attributes (None: absent — that half of the first pair is left out, as the
    float32 route leaves it out); ``fill_value``: the stored integer that means missing (None or NaN: none), in the range of
    the storage; ``unsigned``: the 16 bits are uint16 (None: what ``q``'s dtype says; True beside int16 bits: read them as
    unsigned, the way ``_Unsigned = "true"`` asks).

    The constructor makes a cube of ONE rule; `concat` joins cubes along time into one of several (``n_rules``, ``rules``,
    ``rule_bounds``).  A single-rule cube also answers ``pairs`` / ``n_pairs`` / ``fill_value`` / ``packing()``; on a multi-rule cube
    those raise ``ValueError``: read ``rules``."""

    _aggfly_packed = True

    def __init__(self, q, scale_factor=None, add_offset=None, fill_value=None, unsigned=None, _pairs=None, _rules=None, _bounds=None,
                 _taxis=0):
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
        # the axis of `q` that is time (None: indexed away, or never there): the rules lie along it
        self._taxis = _taxis if (_taxis is not None and q.ndim > 0) else None
        if _rules is not None:
            rules = [(list(p), self._check_fill(f)) for p, f in _rules]
            bounds = [int(b) for b in _bounds]
            if len(bounds) != len(rules) + 1 or bounds[0] != 0 or (len(rules) > 1 and (self._taxis is None or bounds[-1] != q.shape[self._taxis])):
                raise ValueError(f"rule bounds {bounds} do not cover the time axis")
            self._rules, self._bounds = _join_rules(rules, bounds)
        else:
            if _pairs is not None:
                pairs = [tuple(p) for p in _pairs]
            else:
                pairs = []
                if scale_factor is not None or add_offset is not None:
                    pairs.append((None if scale_factor is None else np.float32(scale_factor),
                                  None if add_offset is None else np.float32(add_offset)))
            self._rules, self._bounds = [(pairs, self._check_fill(fill_value))], None
        if any(len(p) > MAX_PAIRS for p, _ in self._rules):
            raise ValueError(f"at most {MAX_PAIRS} (multiply, add) pairs")

    def _check_fill(self, fill_value):
        if fill_value is not None and isinstance(fill_value, float) and np.isnan(fill_value):
            fill_value = None
        if fill_value is not None:
            lo, hi = (0, 65535) if self.unsigned else (-32768, 32767)
            if int(fill_value) != fill_value or not lo <= int(fill_value) <= hi:
                raise ValueError(f"fill_value {fill_value!r} is no {self.storage} value")
            fill_value = int(fill_value)
        return fill_value

    # ---- the rules ----
    @property
    def n_rules(self) -> int:
        return len(self._rules)

    @property
    def rules(self):
        """[(pairs, fill_value)] in time order: rule ``i`` unpacks the time steps ``rule_bounds[i] .. rule_bounds[i + 1]``."""
        return [(list(p), f) for p, f in self._rules]

    @property
    def rule_bounds(self):
        if len(self._rules) == 1:
            return [0, int(self.q.shape[self._taxis]) if self._taxis is not None else 1]
        return list(self._bounds)

    def _one_rule(self, what):
        if len(self._rules) != 1:
            raise ValueError(f"the cube carries {len(self._rules)} unpack rules along time, there is no single `{what}`: read `rules` / `rule_bounds`")
        return self._rules[0]

    @property
    def pairs(self):
        return self._one_rule("pairs")[0]

    @property
    def fill_value(self):
        return self._one_rule("fill_value")[1]

    @classmethod
    def concat(cls, cubes):
        """Join cubes of equal storage along their time axis: the rules follow one another; parts without a time step are
        dropped and equal neighbours merge, so parts of one packing give a single-rule cube."""
        import torch
        cubes = list(cubes)
        if not cubes or not all(isinstance(c, PackedCube) for c in cubes):
            raise TypeError("PackedCube.concat joins PackedCubes")
        ax = cubes[0]._taxis
        if len({c.unsigned for c in cubes}) != 1:
            raise ValueError("PackedCube.concat: the cubes mix int16 and uint16 storage")
        if ax is None or any(c._taxis != ax for c in cubes):
            raise ValueError("PackedCube.concat: the cubes must share their time axis")
        rules, bounds = [], [0]
        for c in cubes:
            for r, lo, hi in zip(c._rules, c.rule_bounds[:-1], c.rule_bounds[1:]):
                rules.append(r)
                bounds.append(bounds[-1] + (hi - lo))
        return cls(torch.cat([c.q for c in cubes], dim=ax), unsigned=cubes[0].unsigned, _rules=rules, _bounds=bounds, _taxis=ax)

    def rule_parts(self):
        """[(single-rule PackedCube of the rule's time steps — a view —, lo, hi)] in time order."""
        if len(self._rules) == 1:
            b = self.rule_bounds
            return [(self, b[0], b[1])]
        return [(PackedCube(self.q.narrow(self._taxis, lo, hi - lo), fill_value=r[1], unsigned=self.unsigned, _pairs=r[0], _taxis=self._taxis), lo, hi)
                for r, lo, hi in zip(self._rules, self._bounds[:-1], self._bounds[1:])]

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

    def _like(self, q, pairs=None, taxis="same", rules=None):
        """The same rules (or ``rules``; or, single-rule, ``pairs``) on other integers; ``taxis``: where their time axis is."""
        taxis = self._taxis if taxis == "same" else taxis
        if rules is None and len(self._rules) == 1:
            return PackedCube(q, fill_value=self._rules[0][1], unsigned=self.unsigned, _pairs=self._rules[0][0] if pairs is None else pairs, _taxis=taxis)
        return PackedCube(q, unsigned=self.unsigned, _rules=self._rules if rules is None else rules, _bounds=self.rule_bounds, _taxis=taxis)

    # ---- views and copies: on the integers, the rules ride along ----
    def _axis(self, a, n=None):
        n = self.q.ndim if n is None else n
        a = int(a)
        return a + n if a < 0 else a

    def permute(self, *order):
        if len(order) == 1 and isinstance(order[0], (tuple, list)):
            order = tuple(order[0])
        taxis = None if self._taxis is None else [self._axis(a) for a in order].index(self._taxis)
        return self._like(self.q.permute(*order), taxis=taxis)

    def transpose(self, a, b):
        a_, b_ = self._axis(a), self._axis(b)
        taxis = b_ if self._taxis == a_ else (a_ if self._taxis == b_ else self._taxis)
        return self._like(self.q.transpose(a, b), taxis=taxis)

    def contiguous(self):
        return self if self.q.is_contiguous() else self._like(self.q.contiguous())

    def is_contiguous(self):
        return self.q.is_contiguous()

    def clone(self):
        return self._like(self.q.clone())

    def unsqueeze(self, axis):
        at = self._axis(axis, self.q.ndim + 1)
        taxis = self._taxis if self._taxis is None or at > self._taxis else self._taxis + 1
        return self._like(self.q.unsqueeze(axis), taxis=taxis)

    def __getitem__(self, key):
        """Indexing on the integers.  On the time axis a step-1 slice rebases the rule bounds (and may leave one rule), an integer picks
        its own rule; keys on the other axes keep the rules; any other key on the time axis of a multi-rule cube works on the values."""
        keys = list(key) if isinstance(key, tuple) else [key]
        n_real = sum(1 for k in keys if k is not None and k is not Ellipsis)
        if sum(1 for k in keys if k is Ellipsis) > 1:
            raise IndexError("an index can only have a single ellipsis")
        if Ellipsis in keys:
            at = keys.index(Ellipsis)
            keys[at:at + 1] = [slice(None)] * (self.q.ndim - n_real)
        # walk the key: which output axis the time axis becomes, and what is asked of it
        ax_in, ax_out, taxis, tkey, fancy = 0, 0, None, slice(None), 0
        for k in keys:
            if k is None:
                ax_out += 1
                continue
            if ax_in == self._taxis:
                taxis, tkey = ax_out, k
            simple = isinstance(k, slice) or (isinstance(k, (int, np.integer)) and not isinstance(k, bool))
            fancy += 0 if simple else 1
            ax_out += 0 if (simple and not isinstance(k, slice)) else 1
            ax_in += 1
        if self._taxis is not None and ax_in <= self._taxis:
            taxis = ax_out + (self._taxis - ax_in)              # the key stops before the time axis
        if fancy > 1 or (fancy == 1 and any(getattr(k, "ndim", 1) != 1 or getattr(k, "dtype", None) in (bool, np.bool_) for k in keys
                                            if not (k is None or isinstance(k, (slice, int, np.integer))))):
            taxis = "lost"                                      # several / masked advanced indices: where the axes land is torch's business
        if len(self._rules) == 1:
            if isinstance(tkey, (int, np.integer)) or taxis == "lost":
                taxis = None
            return self._like(self.q[key], taxis=taxis)
        T = int(self.q.shape[self._taxis])
        if taxis != "lost" and isinstance(tkey, (int, np.integer)) and not isinstance(tkey, bool):
            t = int(tkey) + T if tkey < 0 else int(tkey)
            if not 0 <= t < T:
                raise IndexError(f"index {int(tkey)} is out of bounds for the time axis of {T} steps")
            r = self._rules[int(np.searchsorted(self._bounds, t, side="right")) - 1]
            return PackedCube(self.q[key], fill_value=r[1], unsigned=self.unsigned, _pairs=r[0], _taxis=None)
        if taxis != "lost" and isinstance(tkey, slice) and tkey.step in (None, 1):
            lo, hi, _ = tkey.indices(T)
            hi = max(hi, lo)
            bounds = [min(max(b, lo), hi) - lo for b in self._bounds]
            return PackedCube(self.q[key], unsigned=self.unsigned, _rules=self._rules, _bounds=bounds, _taxis=taxis)
        return self.materialize()[key]

    def to(self, *args, **kwargs):
        """A move between devices keeps the cube packed; a dtype asks for values and materialises."""
        import torch
        if any(isinstance(a, torch.dtype) for a in args) or "dtype" in kwargs:
            return self.materialize().to(*args, **kwargs)
        return self._like(self.q.to(*args, **kwargs))

    def cuda(self, *args, **kwargs):
        return self._like(self.q.cuda(*args, **kwargs))

    # ---- arithmetic with a real scalar folds into every rule; everything else works on the values ----
    def _fold(self, fold, c):
        c = np.float32(c)                      # torch's scalar semantics beside a float32 tensor: the scalar is cast to float32
        rules = [(fold(p, c), f) for p, f in self._rules]
        if any(p is None for p, _ in rules):   # a rule whose chain is full: the whole cube goes to values
            return None
        if len(rules) == 1:
            return self._like(self.q, rules[0][0])
        return self._like(self.q, rules=rules)

    def _fold_add(self, c):
        return self._fold(_fold_add_pairs, c)

    def _fold_mul(self, c):
        return self._fold(_fold_mul_pairs, c)

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
    @staticmethod
    def _packing_of(rule, p=None):
        from . import hip
        pairs, fill = rule
        p = hip.Packing() if p is None else p
        p.n_pairs = len(pairs)
        p.has_fill = 0 if fill is None else 1
        p.fill = 0 if fill is None else fill
        for i in range(MAX_PAIRS):
            m, a = pairs[i] if i < len(pairs) else (None, None)
            p.mul[i] = 1.0 if m is None else float(m)
            p.add[i] = -0.0 if a is None else float(a)
        return p

    def packing(self):
        """The rule as the library's ``afhip_packing``: a pair half the chain lacks travels as its exact identity (multiply by 1.0,
        add -0.0: ``x + -0.0 == x`` for every x, the sign of zero included).  The signedness is not part of it: the library takes
        it from the plan's dtype (`hip._dtype_code`) or from the entry point (`hip.unpack_i16`), and ignores ``pad``.  A multi-rule
        cube has no single packing (``ValueError``): see `packings`."""
        return self._packing_of(self._one_rule("packing()"))

    def packings(self):
        """All rules for ``afhip_plan_bind_packings``: (a ctypes array of ``n_rules`` ``afhip_packing``, the int64 bounds)."""
        from . import hip
        arr = (hip.Packing * len(self._rules))()
        for i, r in enumerate(self._rules):
            self._packing_of(r, arr[i])
        return arr, np.asarray(self.rule_bounds, dtype=np.int64)

    def materialize(self):
        """The float32 values as an HBM tensor of the same shape (``afhip_unpack_i16`` / ``afhip_unpack_u16``: the kernel's own unpack rule;
        a multi-rule cube rule by rule, on the rules' ranges of time steps).  Raises
        `hip.HipEngineError` without a GPU: the values have no host form here."""
        from . import hip
        hip.require_gpu()
        return hip.unpack_i16(self)

    def __repr__(self):
        if len(self._rules) > 1:
            return f"<aggfly_amd.PackedCube {self.storage} {tuple(self.shape)} rules={len(self._rules)} bounds={self._bounds} on {self.device}>"
        return f"<aggfly_amd.PackedCube {self.storage} {tuple(self.shape)} pairs={self.pairs} fill={self.fill_value} on {self.device}>"


def is_packed(x) -> bool:
    return isinstance(x, PackedCube)
