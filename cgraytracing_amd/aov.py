"""Grid AOVs: a frame's feature buffers -- albedo, shading normal, depth, coverage and object id of the camera's first hit
(include/cgrt.h, "grid AOVs").

`Scene` here is refit.Scene with the AOV calls added, and it is what `cgraytracing_amd.Scene` names: engine.py's public
surface is pinned to a recorded table (tests/test_py_binding_host.py), so the calls of a new capability live in a module of
their own and reach the user through the subclass.  Buffers are checked by the adapters of _buffers.py, as everywhere."""
from __future__ import annotations

import ctypes as C

from . import _buffers, _capi, engine, refit
from ._capi import check

_F32 = ("float32", "float32")
# result -> (rows, cols, (torch, numpy) dtype, numpy fill), in the order of cgrt_grid_aov's fields
_AOV = dict(albedo=("frame", 3, _F32, 0), normal=("frame", 3, _F32, 0), depth=("frame", None, _F32, 0),
            hits=("frame", None, _buffers.U32, 0), obj_id=("frame", None, _buffers.I32, -1))
_ADDED_TO = ("albedo", "normal", "depth", "hits")  # what accumulate=True adds to (obj_id is overwritten)


def _want(what, want):
    want = tuple(want)
    if not want or any(w not in _AOV for w in want):
        raise ValueError("%s: want is a non-empty subset of %r" % (what, tuple(_AOV)))
    return [k for k in _AOV if k in want]


class Scene(refit.Scene):
    __doc__ = engine.Scene.__doc__

    def trace_grid_aov(self, width, height, spp=1, camera=None, seed=12345, rows=None, row_offset=0, stripe=None, sample_offset=0,
                       spp_total=None, want=("albedo", "normal", "depth", "hits", "obj_id"), out=None, accumulate=False, counters=None,
                       stream=None):
        """cgrt_trace_grid_aov: the first-hit feature buffers of the frame trace_grid renders for the same grid arguments, by
        one launch (no ray list).  want: which of "albedo" (float32 [rows,width,3]: getSurfaceColor at the first hit, averaged
        over spp_total), "normal" (float32 [rows,width,3]: the normal turned against the ray, averaged likewise -- not unit
        length), "depth" (float32 [rows,width]: sum of the hit distances / spp_total; the mean over the hits is depth *
        spp_total / hits), "hits" (int32 [rows,width], bit pattern uint32: the samples that hit) and "obj_id" (int32
        [rows,width]: the object sample `sample_offset` hits, or -1).  out: dict of preallocated tensors to write into.
        accumulate=True: CGRT_GRID_ACCUMULATE -- albedo, normal, depth and hits are added to (those not given in `out` start
        from zero), obj_id is overwritten.  Asynchronous on torch's current stream (or `stream`); counters (int64 [8]) are
        ADDED to.  Returns a dict of the tensors and "counters"."""
        return self._aov(self._torch(), "trace_grid_aov", width, height, spp, camera, seed, rows, row_offset, stripe, sample_offset, spp_total,
                         want, out, accumulate, counters, stream)

    def trace_grid_aov_host(self, width, height, spp=1, camera=None, seed=12345, rows=None, row_offset=0, stripe=None, sample_offset=0,
                            spp_total=None, want=("albedo", "normal", "depth", "hits", "obj_id")):
        """Synchronous form of trace_grid_aov with numpy outputs (no torch needed): dict of the arrays in `want` (hits
        uint32), counters (uint64 [8]) and nrays."""
        return self._aov(_buffers.NUMPY, "trace_grid_aov_host", width, height, spp, camera, seed, rows, row_offset, stripe, sample_offset,
                         spp_total, want, None, False, None, None)

    def _aov(self, A, what, width, height, spp, camera, seed, rows, row_offset, stripe, sample_offset, spp_total, want, out, accumulate,
             counters, stream):
        rows = height - row_offset if rows is None else rows
        names = _want(what, want)
        res = A.results(what, _AOV, names, out, 0, frame=(rows, width))
        cnt = A.counters(what, counters)
        if accumulate:  # a buffer of this call's own has nothing in it yet
            for k in names:
                if k in _ADDED_TO and not (out and out.get(k) is not None):
                    res[k].zero_()
        cc, g = self._structs(camera, width, height, rows, spp, 1, seed, row_offset, stripe, sample_offset, spp_total,
                              _capi.GRID_ACCUMULATE if accumulate else 0)
        o = _capi.GridAov(*[A.ptr(res.get(k)) for k in _AOV])
        check(getattr(self._L, "cgrt_trace_grid_aov" + A.suffix)(self._h, C.byref(cc), C.byref(g), C.byref(o), A.ptr(cnt), *A.stream(stream)))
        res["counters"] = cnt
        if A.host:
            res["nrays"] = int(cnt[_capi.CNT_RAYS])
        return res

    def aov_variant(self, width, height, camera=None, rows=None, stripe=None):
        """Name of the aov_grid_kernel instantiation trace_grid_aov launches for this scene (cgrt_trace_grid_aov_variant)."""
        rows = height if rows is None else rows
        cc, g = self._structs(camera, width, height, rows, 1, 1, 0, 0, stripe, 0, None, 0)
        return engine._variant_name(self._L.cgrt_trace_grid_aov_variant, self._h, C.byref(cc), C.byref(g))
