"""Refit and rebuild: new vertices for a committed opaque mesh (include/cgrt.h, "refit" and "rebuild"; DESIGN.md sections 16, 17).

`Scene` here is engine.Scene with the refit calls added, and it is what `cgraytracing_amd.Scene` names: engine.py's public
surface is pinned to a recorded table (tests/test_py_binding_host.py), so the calls of a new capability live in a module of
their own and reach the user through the subclass.  Buffers are checked by the adapters of _buffers.py, as everywhere."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _buffers, _capi, engine
from ._capi import check


class Scene(engine.Scene):
    __doc__ = engine.Scene.__doc__

    def refit_mesh(self, obj, tris, stream=None):
        """cgrt_scene_refit_mesh on a torch tensor: tris float64 [n,9] or [n,3,3] (pa, pb, pc per triangle in construction
        order), contiguous on the scene's device, n the mesh's triangle count.  The hierarchy of object `obj` -- an opaque mesh
        -- keeps its topology and gets boxes, triangle records, bounding and cover spheres for these vertices, by kernels on
        torch's current stream (or `stream`): every launch that follows on that stream sees the moved mesh.  Asynchronous
        after the mesh's first refit, which builds the plan.  tris must stay alive until the kernels have run.  Parity class
        and refusals: include/cgrt.h."""
        self._refit(self._torch(), "refit_mesh", obj, tris, stream)

    def _refit(self, A, what, obj, tris, stream, call="refit"):
        n, tris = A.triangles(what, tris)
        check(getattr(self._L, "cgrt_scene_%s_mesh" % call + A.suffix)(self._h, int(obj), A.ptr(tris), n, *A.stream(stream)))

    def refit_mesh_host(self, obj, tris):
        """Synchronous form of refit_mesh on a numpy array (no torch needed); it also refreshes the handle's host mirrors
        (what tree_dump returns as the triangles)."""
        self._refit(_buffers.NUMPY, "refit_mesh_host", obj, tris, None)

    def refit_info(self, obj):
        """cgrt_scene_refit_info: dict(refits, nwide, ntris, plan_built, ms_plan, geometry_gen)."""
        ri = _capi.RefitInfo()
        check(self._L.cgrt_scene_refit_info(self._h, int(obj), C.byref(ri)))
        return {f: getattr(ri, f) for f, _ in ri._fields_}

    def rebuild_mesh(self, obj, tris, stream=None):
        """cgrt_scene_rebuild_mesh on a torch tensor (as refit_mesh's): object `obj` -- an opaque mesh whose tree was built on
        the device (build="device") -- gets these vertices and the hierarchy a fresh device-build commit of them builds, in
        place, by kernels on torch's current stream (or `stream`), which the call synchronises.  Refusals: include/cgrt.h."""
        self._refit(self._torch(), "rebuild_mesh", obj, tris, stream, "rebuild")

    def rebuild_mesh_host(self, obj, tris):
        """The same on a numpy array (no torch needed); it also refreshes the triangles tree_dump returns."""
        self._refit(_buffers.NUMPY, "rebuild_mesh_host", obj, tris, None, "rebuild")

    def rebuild_info(self, obj):
        """cgrt_scene_rebuild_info: dict(rebuilds, nwide, stack_need, balanced, levels, readbacks, ms_last, scratch_bytes)."""
        ri = _capi.RebuildInfo()
        check(self._L.cgrt_scene_rebuild_info(self._h, int(obj), C.byref(ri)))
        return {f: getattr(ri, f) for f, _ in ri._fields_ if f != "pad_"}

    def mesh_cost(self, obj):
        """cgrt_scene_mesh_cost_host: dict(node_cost, tri_cost, root_area), the surface-area cost of the 4-wide hierarchy the
        device walks for mesh `obj` now.  Rule of thumb: rebuild when node_cost + tri_cost exceeds some multiple of its value
        after the last build."""
        tc = _capi.TreeCost()
        check(self._L.cgrt_scene_mesh_cost_host(self._h, int(obj), C.byref(tc)))
        return {f: getattr(tc, f) for f, _ in tc._fields_}

    def mesh_bounds(self, obj):
        """cgrt_scene_mesh_bounds_host: dict(centre float64 [3], s0 float, bmax np.float32, cover float64 [n,4]) -- the bounding
        sphere, the tree's coordinate bound and the cover spheres of mesh `obj` as the device holds them now."""
        n, s0, bmax, centre = C.c_int32(), C.c_double(), C.c_float(), np.zeros(3)
        check(self._L.cgrt_scene_mesh_bounds_host(self._h, int(obj), None, None, None, None, 0, C.byref(n)))
        cover = np.zeros((n.value, 4))
        check(self._L.cgrt_scene_mesh_bounds_host(self._h, int(obj), centre.ctypes.data, C.byref(s0), C.byref(bmax),
                                                  cover.ctypes.data if n.value else None, n.value, C.byref(n)))
        return dict(centre=centre, s0=s0.value, bmax=np.float32(bmax.value), cover=cover)

    def refit_plan(self, t=0):
        """(parent [nwide], slot [nwide], arrivals [nwide], src [ntris]): see cgrt_scene_refit_plan_host."""
        nw, nt = C.c_int32(), C.c_int32()
        check(self._L.cgrt_scene_refit_plan_host(self._h, t, C.byref(nw), C.byref(nt), None, None, None, None))
        parent, slot, arrivals = (np.zeros(max(nw.value, 1), np.int32) for _ in range(3))
        src = np.zeros(max(nt.value, 1), np.int32)
        check(self._L.cgrt_scene_refit_plan_host(self._h, t, C.byref(nw), C.byref(nt), parent.ctypes.data, slot.ctypes.data,
                                                 arrivals.ctypes.data, src.ctypes.data))
        return parent[: nw.value], slot[: nw.value], arrivals[: nw.value], src[: nt.value]
