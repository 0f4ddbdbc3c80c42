"""The two adapters through which engine.py looks at a caller's buffers and makes a query's results: Torch for tensors on the
scene's device (refuses what is not exactly right), Numpy for host arrays (coerces, as the _host forms always did).  Same
interface, so that the device form and the host form of a query are one function given one or the other; every check and
every allocation of such a buffer is written here and nowhere else.

A dtype is a pair (torch, numpy) of names, since the two forms differ in signedness: torch has no uint32 / uint64 tensors to
speak of.  The torch name is spelled as the error message spells it ("int64" or "torch.int64": both exist in the messages
callers may match on); a tuple of names accepts any of them and reports the first.

A result table is {name: (rows, cols, dtype pair, numpy fill)}: rows "n", "2n" or "cap" -- or a (torch, numpy) pair of those
where the two forms differ ("max(n,1)") --, cols None for a vector.  rows "frame": one entry, or one row of `cols`, per pixel of
a frame whose (rows, width) is given as `frame` (the grid AOVs, aov.py)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._capi import CGRT_NCOUNTERS

F64, I32, I64, U8 = ("float64", "float64"), ("int32", "int32"), ("int64", "int64"), ("uint8", "uint8")
U32, U64 = ("int32", "uint32"), ("int64", "uint64")  # bit patterns of unsigned values in signed tensors


def _shape(row, form, n, cap, frame=None):
    rows, cols = row[0] if isinstance(row[0], str) else row[0][form], row[1]
    lead = tuple(frame) if rows == "frame" else ({"n": n, "2n": 2 * n, "cap": cap, "max(n,1)": max(n, 1)}[rows],)
    return lead if cols is None else lead + (cols,)


def _differ(what, names):
    return ValueError("%s: %s and %s differ in length" % (what, ", ".join(names[:-1]), names[-1]))


class Torch:
    """Tensors on cuda:`device`."""
    form, host, suffix = 0, False, ""

    def __init__(self, device):
        import torch

        self.torch = torch
        self.dev = torch.device("cuda", device)

    def _ok(self, t, dtypes, shape):
        """shape: a None entry is any size."""
        return (isinstance(t, self.torch.Tensor) and t.dtype in dtypes and t.dim() == len(shape) and
                all(s is None or s == d for s, d in zip(shape, t.shape)) and t.is_contiguous() and t.device == self.dev)

    def rays(self, what, coerce=True, **arrays):
        """org=, dirs= (and flux=): contiguous float64 [n,3] of one length.  Returns (n, *arrays)."""
        for name, t in arrays.items():
            if not self._ok(t, (self.torch.float64,), (None, 3)):
                raise ValueError("%s: %s must be a contiguous float64 [n,3] tensor on %s" % (what, name, self.dev))
        n = arrays["org"].shape[0]
        if any(t.shape[0] != n for t in arrays.values()):
            raise _differ(what, list(arrays))
        return (n,) + tuple(arrays.values())

    def per_ray(self, what, name, t, n, dtype, cols=None, required=False, coerce=True, per="ray"):
        """An optional (or required) buffer of one entry, or one row of `cols`, per ray; n None: of any length."""
        if t is None and not required:
            return None
        spelled = dtype[0] if isinstance(dtype[0], tuple) else (dtype[0],)
        if not self._ok(t, [getattr(self.torch, s.split(".")[-1], None) for s in spelled], (n,) if cols is None else (n, cols)):
            raise ValueError("%s: %s must be a contiguous %s [n%s] tensor on %s" % (what, name, spelled[0], "" if cols is None else ",%d" % cols,
                                                                                   self.dev))
        return t

    def triangles(self, what, t):
        """A mesh's vertices: contiguous float64 [n,9] or [n,3,3].  Returns (n, t)."""
        if not (self._ok(t, (self.torch.float64,), (None, 9)) or self._ok(t, (self.torch.float64,), (None, 3, 3))):
            raise ValueError("%s: tris must be a contiguous float64 [n,9] or [n,3,3] tensor on %s" % (what, self.dev))
        return t.shape[0], t

    def results(self, what, spec, names, out, n, cap=0, frame=None):
        """{name: the caller's out[name], validated, or a fresh tensor} for `names` of the table `spec`."""
        res = {}
        for name in names:
            shape, dtype = _shape(spec[name], 0, n, cap, frame), getattr(self.torch, spec[name][2][0])
            t = out.get(name) if out else None
            if t is None:
                t = self.torch.empty(shape, dtype=dtype, device=self.dev)
            elif not self._ok(t, (dtype,), shape):
                raise ValueError("%s: out[%r] must be a contiguous %s %r tensor on %s" % (what, name, dtype, shape, self.dev))
            res[name] = t
        return res

    def counters(self, what, counters=None):
        if counters is None:
            return self.torch.zeros((CGRT_NCOUNTERS,), dtype=self.torch.int64, device=self.dev)
        if not (isinstance(counters, self.torch.Tensor) and counters.dtype == self.torch.int64 and counters.numel() == CGRT_NCOUNTERS and
                counters.is_contiguous() and counters.device == self.dev):
            raise ValueError("%s: counters must be a contiguous int64 [%d] tensor on %s" % (what, CGRT_NCOUNTERS, self.dev))
        return counters

    def ptr(self, x):
        return None if x is None else x.data_ptr()

    def stream(self, stream=None):
        """The trailing stream argument of a device entry point: `stream`, or torch's current one."""
        return (C.c_void_p(stream if stream is not None else self.torch.cuda.current_stream(self.dev).cuda_stream),)


class Numpy:
    """Host arrays."""
    form, host, suffix = 1, True, "_host"

    def rays(self, what, coerce=True, **arrays):
        """coerce=False: [n,3] is asked of the caller, not made by reshape."""
        arrays = {k: np.ascontiguousarray(a, np.float64) for k, a in arrays.items()}
        if not coerce:
            org = arrays["org"]
            if org.ndim != 2 or org.shape[1] != 3 or any(a.shape != org.shape for a in arrays.values()):
                raise ValueError("%s: %s must be [n,3] arrays of one length" % (what, " and ".join(arrays)))
            return (len(org),) + tuple(arrays.values())
        arrays = {k: a.reshape(-1, 3) for k, a in arrays.items()}
        n = len(arrays["org"])
        if any(len(a) != n for a in arrays.values()):
            raise _differ(what, list(arrays))
        return (n,) + tuple(arrays.values())

    def per_ray(self, what, name, t, n, dtype, cols=None, required=False, coerce=True, per="ray"):
        if t is None and not required:
            return None
        t = np.ascontiguousarray(t, dtype[1] if coerce else None)
        if t.shape != ((n,) if cols is None else (n, cols)) or t.dtype != np.dtype(dtype[1]):
            if not coerce:
                raise ValueError("%s: %s must be a%s %s [n] array" % (what, name, "n" if dtype[1][0] in "aeiou" else "", dtype[1]))
            raise ValueError("%s: %s must %s" % (what, name, "have one entry per %s" % per if cols is None else "be an [n,%d] array" % cols))
        return t

    def triangles(self, what, t):
        t = np.ascontiguousarray(t, np.float64)
        if t.size % 9 or (t.ndim > 1 and t.shape[1:] not in ((9,), (3, 3))):
            raise ValueError("%s: tris must be an [n,9] or [n,3,3] array" % what)
        return t.size // 9, t

    def results(self, what, spec, names, out, n, cap=0, frame=None):
        make = lambda shape, dtype, fill: np.full(shape, fill, dtype) if fill else np.zeros(shape, dtype)
        return {k: make(_shape(spec[k], 1, n, cap, frame), spec[k][2][1], spec[k][3]) for k in names}

    def counters(self, what, counters=None):
        return np.zeros((CGRT_NCOUNTERS,), np.uint64)

    def ptr(self, x):
        return None if x is None else x.ctypes.data

    def stream(self, stream=None):
        return ()


NUMPY = Numpy()
