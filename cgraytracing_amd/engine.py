"""Host-side `render(objs)` over the C ABI: flattens a list of scene objects into a cgrt_scene handle and
launches the eye pass (the loop nest of main.cpp:185-219) on the GPU."""
from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np

from . import _capi
from ._capi import Camera as _CCamera
from ._capi import Grid as _CGrid
from ._capi import check
from .scene import Camera


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def _ccamera(camera):
    """(the cgrt_camera a call is given, the grid flag that goes with it): a Camera with a pose becomes a cgrt_posed_camera
    and the call gets its `base` -- a view into the same memory, which keeps the whole struct alive -- with CGRT_GRID_POSED."""
    camera = camera or Camera()
    base = _CCamera(_d3(camera.cam), camera.half_width, camera.focus_plane, camera.lens_radius)
    if getattr(camera, "pose", None) is None:
        return base, 0
    origin, right, up, forward = camera.pose
    pc = _capi.PosedCamera(base, _d3(origin), _d3(right), _d3(up), _d3(forward))
    return pc.base, _capi.GRID_POSED


_RELAY_ORDERS = ("chunks_first", "mirror_first", "interleaved")  # CGRT_GRID_RELAY_CHUNKS_FIRST / _MIRROR_FIRST / _INTERLEAVED
_RELAY_STARTS = ("list", "cost")  # CGRT_GRID_NO_RELAY_COST_START / CGRT_GRID_RELAY_COST_START


def _grid_flags(stats, split_samples, reorder, force_reorder, tile_order, diffuse_tiles, sphere_pairs, sphere_masks, lens_stage, sure_tiles, lens_table=None, inside_trips=True):
    """The CGRT_GRID_* flags of trace_grid's switches, the relay's apart (_relay_flag)."""
    on = (stats, _capi.GRID_STATS), (split_samples, _capi.GRID_SPLIT_SAMPLES), (force_reorder, _capi.GRID_FORCE_REORDER), (diffuse_tiles, _capi.GRID_DIFFUSE_TILES)
    off = ((reorder, _capi.GRID_NO_REORDER), (tile_order, _capi.GRID_NO_TILE_ORDER), (sphere_pairs, _capi.GRID_NO_SPHERE_PAIRS),
           (sphere_masks, _capi.GRID_NO_SPHERE_MASKS), (lens_stage, _capi.GRID_NO_LENS_STAGE), (sure_tiles, _capi.GRID_NO_SURE_TILES),
           (inside_trips, _capi.GRID_NO_INSIDE_TRIPS))
    table = 0 if lens_table is None else _capi.GRID_LENS_TABLE if lens_table else _capi.GRID_NO_LENS_TABLE
    return sum(f for v, f in on if v) | sum(f for v, f in off if not v) | table


def _relay_flag(sample_relay, relay_mirror=None, relay_order=None, relay_start=None, relay_boost=None):
    """CGRT_GRID_SAMPLE_RELAY / _NO_SAMPLE_RELAY / _SAMPLE_RELAY_4 for trace_grid's sample_relay=None|True|False|2|4, with
    CGRT_GRID_RELAY_MIRROR / _NO_MIRROR for relay_mirror=None|True|False, the order field for relay_order=None|a name and
    CGRT_GRID_RELAY_COST_START / _NO_RELAY_COST_START for relay_start=None|"cost"|"list" and CGRT_GRID_RELAY_BOOST /
    _NO_RELAY_BOOST for relay_boost=None|True|False."""
    form = 0 if relay_mirror is None else (_capi.GRID_RELAY_MIRROR if relay_mirror else _capi.GRID_RELAY_NO_MIRROR)
    if relay_boost is not None:
        form |= _capi.GRID_RELAY_BOOST if relay_boost else _capi.GRID_NO_RELAY_BOOST
    if relay_start is not None:
        if relay_start not in _RELAY_STARTS:
            raise ValueError("relay_start: None, " + ", ".join(repr(o) for o in _RELAY_STARTS))
        form |= _capi.GRID_RELAY_COST_START if relay_start == "cost" else _capi.GRID_NO_RELAY_COST_START
    if relay_order is not None:
        if relay_order not in _RELAY_ORDERS:
            raise ValueError("relay_order: None, " + ", ".join(repr(o) for o in _RELAY_ORDERS))
        form |= (_capi.GRID_RELAY_CHUNKS_FIRST, _capi.GRID_RELAY_MIRROR_FIRST, _capi.GRID_RELAY_INTERLEAVED)[_RELAY_ORDERS.index(relay_order)]
    if sample_relay is None:
        return form
    if sample_relay is True or sample_relay is False:
        return form | (_capi.GRID_SAMPLE_RELAY if sample_relay else _capi.GRID_NO_SAMPLE_RELAY)
    if int(sample_relay) not in (2, 4):
        raise ValueError("sample_relay: None, True, False, 2 or 4")
    return form | _capi.GRID_SAMPLE_RELAY | (_capi.GRID_SAMPLE_RELAY_4 if int(sample_relay) == 4 else 0)


def relay_boost_host(k, chunk_spp, spp, cap, mirror, plan, tile_list, wcost, width, rows, k_boost, boost_chunk_spp, boost_cap, num, den,
                     wg_slots):
    """The promoted set and its start table on the host (cgrt_relay_boost_host; no GPU): relay_start_host's arguments, then a
    promoted tile's k_boost workgroups of boost_chunk_spp samples, the second area's boost_cap tiles and the threshold num / den
    over wg_slots workgroup slots.  dict(start [t] uint32, bslot [relayed tiles] uint32, promoted, S) -- what last_relay_start()
    and last_relay_boost() hold for such a launch."""
    lib = _capi.lib()
    lst, wc = np.ascontiguousarray(tile_list, np.uint32), np.ascontiguousarray(wcost, np.uint32)
    assert wc.size == ((width + 15) // 16) * ((rows + 3) // 4) and lst.size == int(plan[4])
    args = (int(k), int(chunk_spp), int(spp), int(cap), 1 if mirror else 0, int(plan[2]), int(plan[3]), int(plan[4]), lst.ctypes.data,
            wc.ctypes.data, int(width), int(rows), int(k_boost), int(boost_chunk_spp), int(boost_cap), int(num), int(den), int(wg_slots))
    t, p, S = C.c_int64(), C.c_int64(), C.c_uint64()
    n_split = min(int(plan[3]) if mirror else int(plan[2]), int(cap))
    start = np.zeros(max(int(plan[3]) + (int(k_boost) - 1) * n_split, 1), np.uint32)
    bslot = np.zeros(max(n_split, 1), np.uint32)
    check(lib.cgrt_relay_boost_host(*args, start.ctypes.data, start.size, bslot.ctypes.data, bslot.size, C.byref(t), C.byref(p), C.byref(S)))
    return dict(start=start[:t.value], bslot=bslot[:n_split], promoted=int(p.value), S=int(S.value))


def relay_start_host(k, chunk_spp, spp, cap, mirror, plan, tile_list, wcost, width, rows):
    """The relay's start table on the host (cgrt_relay_start_host; no GPU): for last_tile_order()'s plan and list, an area of
    `cap` tiles relayed by k workgroups of chunk_spp samples out of spp (mirror: the class-2 tiles too) and the wave tiles' costs
    of a width x rows grid, uint32 [t]: entry << 2 | chunk of workgroup b -- what last_relay_start()["start"] holds."""
    lib = _capi.lib()
    lst, wc = np.ascontiguousarray(tile_list, np.uint32), np.ascontiguousarray(wcost, np.uint32)
    assert wc.size == ((width + 15) // 16) * ((rows + 3) // 4) and lst.size == int(plan[4])
    args = (int(k), int(chunk_spp), int(spp), int(cap), 1 if mirror else 0, int(plan[2]), int(plan[3]), int(plan[4]), lst.ctypes.data,
            wc.ctypes.data, int(width), int(rows))
    t = C.c_int64()
    check(lib.cgrt_relay_start_host(*args, None, 0, C.byref(t)))
    start = np.zeros(max(t.value, 1), np.uint32)
    check(lib.cgrt_relay_start_host(*args, start.ctypes.data, start.size, C.byref(t)))
    return start[:t.value]


class Scene:
    """Owns a cgrt_scene handle.  `objs` order is the reference's `objs` order.  commit=False keeps the scene
    on the host only (mesh loading / tree build can then be inspected without a GPU)."""

    def __init__(self, objs, device=0, commit=True, build=None):
        """build: None (the library's default: host, or what CGRT_BUILD says), "host" or "device" (cgrt_scene_set_build: opaque
        owners' structures built on the GPU at commit; tolerance-class parity, see include/cgrt.h)."""
        L = _capi.lib()
        h = C.c_void_p()
        check(L.cgrt_scene_create(C.byref(h)))
        if build is not None:
            check(L.cgrt_scene_set_build(h, {"host": _capi.BUILD_HOST, "device": _capi.BUILD_DEVICE}[build]))
        self._h = h
        self._L = L
        self.device = int(device)
        self._sessions = weakref.WeakSet()  # live PpmSessions: closed before the scene handle goes
        self.obj_index = []
        tex_ids = {}
        try:
            for o in objs:
                k = o.kind
                if k == "sphere":
                    i = L.cgrt_scene_add_sphere(h, _d3(o.center), o.radius, _d3(o.surfaceColor), o.reflection,
                                                o.transparency)
                elif k == "plane":
                    tid = -1
                    t = o.texture
                    if t is not None:
                        if id(t) not in tex_ids:
                            tex_ids[id(t)] = check(L.cgrt_scene_add_texture(
                                h, t.data.ctypes.data, t.data.shape[0], t.data.shape[1], _d3(t.normal),
                                _d3(t.position), t.lenx, t.leny, int(t.isbump)))
                        tid = tex_ids[id(t)]
                    i = L.cgrt_scene_add_plane(h, _d3(o.position), _d3(o.normal), _d3(o.surfaceColor), o.reflection,
                                               o.transparency, tid)
                elif k == "mesh":
                    if o.triangles is not None:
                        i = L.cgrt_scene_add_mesh_triangles(h, o.triangles.ctypes.data, len(o.triangles),
                                                            _d3(o.surfaceColor), o.reflection, o.transparency,
                                                            o.typeofdata)
                    else:
                        i = L.cgrt_scene_add_mesh_file(h, o.filename.encode(), o.a, _d3(o.b), _d3(o.surfaceColor),
                                                       o.reflection, o.transparency, o.typeofdata)
                elif k == "bezier":
                    i = L.cgrt_scene_add_bezier(h, o.cpoints.ctypes.data, len(o.cpoints), _d3(o.position),
                                                _d3(o.surfaceColor), o.reflection, o.transparency)
                else:
                    raise TypeError("not a scene object: %r" % (o,))
                self.obj_index.append(check(i))
            if commit:
                check(L.cgrt_scene_commit(h, self.device))
        except Exception:
            self.close()
            raise

    def close(self):
        for ses in list(getattr(self, "_sessions", ())):
            ses.close()
        if getattr(self, "_h", None):
            self._L.cgrt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # ---- introspection ----
    def stats(self):
        st = _capi.SceneStats()
        check(self._L.cgrt_scene_get_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def build_info(self):
        bi = _capi.BuildInfo()
        check(self._L.cgrt_scene_build_info(self._h, C.byref(bi)))
        return {f: getattr(bi, f) for f, _ in bi._fields_}

    def tree_dump(self, t=0):
        nn, nl, nt = C.c_int32(), C.c_int32(), C.c_int32()
        check(self._L.cgrt_scene_tree_sizes(self._h, t, C.byref(nn), C.byref(nl), C.byref(nt)))
        nodes = np.zeros((nn.value, 3), np.int32)
        leaf = np.zeros((nl.value,), np.int32)
        bbox = np.zeros((nn.value, 6), np.float64)
        tris = np.zeros((nt.value, 9), np.float64)
        check(self._L.cgrt_scene_tree_dump(self._h, t, nodes.ctypes.data, leaf.ctypes.data, bbox.ctypes.data,
                                           tris.ctypes.data))
        return nodes, leaf, bbox, tris

    def bvh_dump(self, t=0):
        """The hierarchy the device traverses (cgrt_scene_bvh_dump): boxes [8, n, 6] float32, skip [8, n], leaf [8, n]."""
        nn = C.c_int32()
        check(self._L.cgrt_scene_bvh_dump(self._h, t, C.byref(nn), None, None))
        n = nn.value
        box = np.zeros((8, n, 6), np.float32)
        sl = np.zeros((8, n, 2), np.int32)
        check(self._L.cgrt_scene_bvh_dump(self._h, t, C.byref(nn), box.ctypes.data, sl.ctypes.data))
        return box, sl[:, :, 0].copy(), sl[:, :, 1].copy()

    def bvh_order(self, t=0):
        """(tri_level, order): see cgrt_scene_bvh_order."""
        nn, nl, nt = C.c_int32(), C.c_int32(), C.c_int32()
        check(self._L.cgrt_scene_tree_sizes(self._h, t, C.byref(nn), C.byref(nl), C.byref(nt)))
        lvl = C.c_int32()
        order = np.zeros(max(nt.value, 1), np.int32)
        check(self._L.cgrt_scene_bvh_order(self._h, t, C.byref(lvl), order.ctypes.data))
        return bool(lvl.value), order[: nt.value]

    def wide_dump(self, t=0):
        """(box[nwide, 4, 6], ref[nwide, 4], stack_need): see cgrt_scene_wide_dump."""
        n, need = C.c_int32(), C.c_int32()
        check(self._L.cgrt_scene_wide_dump(self._h, t, C.byref(n), C.byref(need), None, None))
        box = np.zeros((max(n.value, 1), 4, 6), np.float32)
        ref = np.zeros((max(n.value, 1), 4), np.int32)
        check(self._L.cgrt_scene_wide_dump(self._h, t, C.byref(n), C.byref(need), box.ctypes.data, ref.ctypes.data))
        return box[: n.value], ref[: n.value], need.value

    # ---- the hot path ----
    def _structs(self, camera, width, height, rows, spp, max_depth, seed, row_offset, stripe, sample_offset,
                 spp_total, flags):
        cc, posed = _ccamera(camera)
        s_rows, s_rank, s_n = stripe if stripe else (0, 0, 1)
        g = _CGrid(width, height, rows, row_offset, s_rows, s_rank, s_n, spp, sample_offset,
                   spp_total if spp_total else spp, max_depth, flags | posed, seed)
        return cc, g

    def trace_grid(self, width, height, spp=1, camera=None, max_depth=5, seed=12345, rows=None, row_offset=0,
                   stripe=None, sample_offset=0, spp_total=None, out=None, nhit=None, counters=None, stream=None,
                   stats=False, accumulate=False, split_samples=False, reorder=True, force_reorder=False, tile_order=True,
                   diffuse_tiles=False, sphere_pairs=True, sphere_masks=True, sample_relay=None,
                   relay_mirror=None, relay_order=None, lens_stage=True, sure_tiles=True, relay_start=None, relay_boost=None, lens_table=None,
                   inside_trips=True):
        """Asynchronous launch on torch's current stream (or `stream`).  reorder=False: CGRT_GRID_NO_REORDER (tiles in image
        order instead of heaviest-first; same image).  tile_order=False: CGRT_GRID_NO_TILE_ORDER (an image-order launch starts
        its tiles row-major instead of mirror / glass tiles first; same image).  diffuse_tiles=True: CGRT_GRID_DIFFUSE_TILES (a
        sphere-only scene's tiles that see no mirror or glass are rendered by the terminal-diffuse launch beside the main one,
        not by the full kernel; same image, off by default).  sphere_pairs=False: CGRT_GRID_NO_SPHERE_PAIRS (a glass sphere
        scene's kernel tests one sphere at a time and renders every tile with the full body; same image).  sphere_masks=False:
        CGRT_GRID_NO_SPHERE_MASKS (the terminal-diffuse body tests every sphere, not only its wave tile's candidates; same image).
        sample_relay: None -- a glass sphere scene's launch of at least 4 tiles per compute unit and 32 samples renders the tiles
        that may see a refracting or a reflecting sphere by 2 workgroups each, summed in sample order (same image; last_sample_relay);
        True or 2: CGRT_GRID_SAMPLE_RELAY (whatever the tile count); 4: that with CGRT_GRID_SAMPLE_RELAY_4 (up to 4 workgroups a
        tile); False: CGRT_GRID_NO_SAMPLE_RELAY.  relay_mirror: True -- the relay takes the tiles that see only a mirror sphere
        too (CGRT_GRID_RELAY_MIRROR), False -- it does not; relay_order: "chunks_first", "mirror_first" or "interleaved" -- where
        those tiles' workgroups start among the glass tiles'; None: what sample_relay has always meant when it is given, the
        measured form when it is not (last_relay_form tells).  relay_start: "cost" -- the relay's workgroups of classes 0-2 start
        longest first by a probed cost (CGRT_GRID_RELAY_COST_START; same image, hit counts and counters; last_relay_start),
        "list" -- in the order named (CGRT_GRID_NO_RELAY_COST_START); None: by cost where the launch relays by default and names
        no order.  relay_boost: True -- a launch with that table at 48 samples or more renders its heaviest relayed tiles by 3 or 4
        workgroups instead of 2 (CGRT_GRID_RELAY_BOOST; same image, hit counts, rays and Hitpoints; last_relay_boost), False --
        CGRT_GRID_NO_RELAY_BOOST; None: where the launch starts by cost by default.  lens_stage=False: CGRT_GRID_NO_LENS_STAGE (the thin-lens
        terminal-diffuse body inside the main launch draws every lens point by its own rejection loop instead of staging 16
        samples' draws ahead; same image; last_lens_stage).  lens_table=False: CGRT_GRID_NO_LENS_TABLE (under a thin lens the tiles that
        may see a mirror or a glass sphere run the rejection loop per sample instead of reading their lens draws from the table a
        small kernel writes ahead of the frame; same image, hit counts and counters; last_lens_table), True: CGRT_GRID_LENS_TABLE
        (a launch that does not find its draws in the table writes them wherever it stands), None: it writes them only beside
        its cost probe and otherwise goes without a table.  sure_tiles=False: CGRT_GRID_NO_SURE_TILES (a wave of the
        terminal-diffuse body traces its samples even where every ray of its 16x4 wave tile provably hits the same sphere first;
        same image, hit counts and counters; sphere_masks=False implies it; last_sure_tiles).  inside_trips=False:
        CGRT_GRID_NO_INSIDE_TRIPS (a glass sphere scene's pair kernel tests every sphere in every iteration, also where all its
        lanes' rays start inside the refracting sphere and can only leave it; same image, hit counts and counters;
        inside_spheres).  split_samples: CGRT_GRID_SPLIT_SAMPLES (several
        workgroups share a tile's samples; reproducible, fp64 summation order differs from the sample-by-sample sum).  Returns (rgb, nhit, counters) torch
        tensors on the scene's device: float32 [rows,width,3], int32 [rows,width] (bit pattern uint32),
        int64 [8] (counters are ADDED to)."""
        import torch

        rows = height - row_offset if rows is None else rows
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.zeros((rows, width, 3), dtype=torch.float32, device=dev)
        if nhit is None:
            nhit = torch.zeros((rows, width), dtype=torch.int32, device=dev)
        elif nhit is False:  # skip the optional per-pixel hitpoint-count plane
            nhit = None
        if counters is None:
            counters = torch.zeros((_capi.CGRT_NCOUNTERS,), dtype=torch.int64, device=dev)
        assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (rows, width, 3)
        cc, g = self._structs(camera, width, height, rows, spp, max_depth, seed, row_offset, stripe, sample_offset,
                              spp_total, (_capi.GRID_ACCUMULATE if accumulate else 0) |
                              _grid_flags(stats, split_samples, reorder, force_reorder, tile_order, diffuse_tiles, sphere_pairs, sphere_masks, lens_stage, sure_tiles, lens_table, inside_trips) |
                              _relay_flag(sample_relay, relay_mirror, relay_order, relay_start, relay_boost))
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(self._L.cgrt_trace_grid(self._h, C.byref(cc), C.byref(g), out.data_ptr(),
                                      nhit.data_ptr() if nhit is not None else None,
                                      counters.data_ptr(), C.c_void_p(st)))
        return out, nhit, counters

    # ---- caller-supplied rays ----
    _WANT = ("acc", "nhit", "hit")

    def camera_rays(self, width, height, spp=1, camera=None, seed=12345, rows=None, row_offset=0, stripe=None,
                    sample_offset=0, stream=None):
        """The primary rays trace_grid starts for samples sample_offset .. sample_offset + spp - 1 of the grid's rows
        (cgrt_camera_rays), made on the device: (org [n,3] float64, dirs [n,3] float64, keys [n] int64 (bit pattern uint64))
        torch tensors, n = spp * rows * width, ray index = (k * rows + local row) * width + w.  Rows beyond `height` of a
        striped grid have dirs = 0 and are not traced by trace_rays."""
        import torch

        rows = height - row_offset if rows is None else rows
        dev = torch.device("cuda", self.device)
        n = spp * rows * width
        org = torch.empty((n, 3), dtype=torch.float64, device=dev)
        dirs = torch.empty((n, 3), dtype=torch.float64, device=dev)
        keys = torch.empty((n,), dtype=torch.int64, device=dev)
        cc, g = self._structs(camera, width, height, rows, spp, 1, seed, row_offset, stripe, sample_offset, None, 0)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            check(self._L.cgrt_camera_rays(C.byref(cc), C.byref(g), org.data_ptr(), dirs.data_ptr(), keys.data_ptr(),
                                           C.c_void_p(st)))
        return org, dirs, keys

    def trace_rays(self, org, dirs, keys=None, max_depth=5, seed=12345, first_index=0, want=("acc", "nhit", "hit"),
                   counters=None, stream=None, stats=False, out=None, sign_pass=True):
        """cgrt_trace_rays on torch tensors: org, dirs float64 [n,3] contiguous on the scene's device, keys int64 [n] or None.
        want: which results -- "acc" (float64 [n,3]: the ray tree's sum of f*adj), "nhit" (int32 [n]), "hit" (hit_obj int32
        [n], hit_t float64 [n], hit_normal float64 [n,3]: the ray's own nearest hit).  want=("hit",) is a nearest-hit query
        (one scene walk per ray, no shading).  out: dict of preallocated result tensors to write into.  Asynchronous on torch's
        current stream (or `stream`); counters (int64 [8]) are ADDED to.  sign_pass=False: CGRT_RAYS_NO_SIGN_PASS (an opaque
        mesh's hit_normal is then right up to its sign; saves an unpruned mesh walk per ray).  Returns a dict of the tensors
        and "counters"."""
        import torch

        dev = torch.device("cuda", self.device)
        for name, t in (("org", org), ("dirs", dirs)):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.dim() == 2 and t.shape[1] == 3 and
                    t.is_contiguous() and t.device == dev):
                raise ValueError("trace_rays: %s must be a contiguous float64 [n,3] tensor on %s" % (name, dev))
        n = org.shape[0]
        if dirs.shape[0] != n:
            raise ValueError("trace_rays: org and dirs differ in length")
        if keys is not None and not (isinstance(keys, torch.Tensor) and keys.dtype == torch.int64 and tuple(keys.shape) == (n,) and
                                     keys.is_contiguous() and keys.device == dev):
            raise ValueError("trace_rays: keys must be a contiguous int64 [n] tensor on %s" % (dev,))
        want = tuple(want)
        if not want or any(w not in self._WANT for w in want):
            raise ValueError("trace_rays: want is a non-empty subset of %r" % (self._WANT,))
        shapes = {}
        if "acc" in want:
            shapes["acc"] = ((n, 3), torch.float64)
        if "nhit" in want:
            shapes["nhit"] = ((n,), torch.int32)
        if "hit" in want:
            shapes.update(hit_obj=((n,), torch.int32), hit_t=((n,), torch.float64), hit_normal=((n, 3), torch.float64))
        res = {}
        for name, (shape, dtype) in shapes.items():
            t = out.get(name) if out else None
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=dev)
            elif not (t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev):
                raise ValueError("trace_rays: out[%r] must be a contiguous %s %r tensor on %s" % (name, dtype, shape, dev))
            res[name] = t
        if counters is None:
            counters = torch.zeros((_capi.CGRT_NCOUNTERS,), dtype=torch.int64, device=dev)
        elif not (counters.dtype == torch.int64 and counters.numel() == _capi.CGRT_NCOUNTERS and counters.is_contiguous() and
                  counters.device == dev):
            raise ValueError("trace_rays: counters must be a contiguous int64 [8] tensor on %s" % (dev,))
        res["counters"] = counters
        if n == 0:
            return res
        ptr = lambda k: res[k].data_ptr() if k in res else None
        r = _capi.Rays(n, org.data_ptr(), dirs.data_ptr(), keys.data_ptr() if keys is not None else None, first_index, seed,
                       max_depth, (_capi.RAYS_STATS if stats else 0) | (0 if sign_pass else _capi.RAYS_NO_SIGN_PASS))
        o = _capi.RayResults(ptr("acc"), ptr("nhit"), ptr("hit_obj"), ptr("hit_t"), ptr("hit_normal"))
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(self._L.cgrt_trace_rays(self._h, C.byref(r), C.byref(o), counters.data_ptr(), C.c_void_p(st)))
        return res

    def trace_rays_host(self, org, dirs, keys=None, max_depth=5, seed=12345, first_index=0, want=("acc", "nhit", "hit"),
                        stats=False, sign_pass=True):
        """Synchronous form of trace_rays on numpy arrays (no torch needed): dict(acc, nhit (uint32), hit_obj, hit_t,
        hit_normal -- those in `want` --, counters (uint64 [8]), nrays, nhp)."""
        org = np.ascontiguousarray(org, np.float64).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
        n = len(org)
        if len(dirs) != n:
            raise ValueError("trace_rays_host: org and dirs differ in length")
        if keys is not None:
            keys = np.ascontiguousarray(keys, np.uint64)
            if keys.shape != (n,):
                raise ValueError("trace_rays_host: keys must have one entry per ray")
        want = tuple(want)
        if not want or any(w not in self._WANT for w in want):
            raise ValueError("trace_rays_host: want is a non-empty subset of %r" % (self._WANT,))
        res = {}
        if "acc" in want:
            res["acc"] = np.zeros((n, 3), np.float64)
        if "nhit" in want:
            res["nhit"] = np.zeros(n, np.uint32)
        if "hit" in want:
            res.update(hit_obj=np.zeros(n, np.int32), hit_t=np.zeros(n, np.float64), hit_normal=np.zeros((n, 3), np.float64))
        cnt = np.zeros((_capi.CGRT_NCOUNTERS,), np.uint64)
        ptr = lambda k: res[k].ctypes.data if k in res else None
        r = _capi.Rays(n, org.ctypes.data, dirs.ctypes.data, keys.ctypes.data if keys is not None else None, first_index, seed,
                       max_depth, (_capi.RAYS_STATS if stats else 0) | (0 if sign_pass else _capi.RAYS_NO_SIGN_PASS))
        o = _capi.RayResults(ptr("acc"), ptr("nhit"), ptr("hit_obj"), ptr("hit_t"), ptr("hit_normal"))
        check(self._L.cgrt_trace_rays_host(self._h, C.byref(r), C.byref(o), cnt.ctypes.data))
        res.update(counters=cnt, nrays=int(cnt[_capi.CNT_RAYS]), nhp=int(cnt[_capi.CNT_HITPOINTS]))
        return res

    # ---- hit attributes of caller-supplied rays ----
    _ATTR_WANT = ("prim", "uv", "color", "material")

    def hit_attributes(self, org, dirs, hit_obj, hit_t, want=("prim", "uv", "color", "material"), out=None, stream=None):
        """cgrt_ray_hit_attributes on torch tensors: org, dirs float64 [n,3], hit_obj int32 [n] and hit_t float64 [n] -- the
        last two as trace_rays(want=("hit",)) wrote them for the same rays --, all contiguous on the scene's device.  want:
        which attributes -- "prim" (int32 [n]: the triangle's index in its mesh's or bump floor's construction order, -1 where
        the hit is no triangle), "uv" (float64 [n,2]: the hit point is (1-u-v)*pa + u*pb + v*pc), "color" (float64 [n,3]:
        getSurfaceColor at the hit) and "material" (float64 [n,2]: reflection, transparency).  out: dict of preallocated
        result tensors to write into.  Asynchronous on torch's current stream (or `stream`).  Returns a dict of the tensors."""
        import torch

        dev = torch.device("cuda", self.device)
        for name, t in (("org", org), ("dirs", dirs)):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.dim() == 2 and t.shape[1] == 3 and
                    t.is_contiguous() and t.device == dev):
                raise ValueError("hit_attributes: %s must be a contiguous float64 [n,3] tensor on %s" % (name, dev))
        n = org.shape[0]
        if dirs.shape[0] != n:
            raise ValueError("hit_attributes: org and dirs differ in length")
        for name, t, dtype in (("hit_obj", hit_obj, torch.int32), ("hit_t", hit_t, torch.float64)):
            if not (isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == (n,) and t.is_contiguous() and
                    t.device == dev):
                raise ValueError("hit_attributes: %s must be a contiguous %s [n] tensor on %s" % (name, dtype, dev))
        want = tuple(want)
        if not want or any(w not in self._ATTR_WANT for w in want):
            raise ValueError("hit_attributes: want is a non-empty subset of %r" % (self._ATTR_WANT,))
        shapes = dict(prim=((n,), torch.int32), uv=((n, 2), torch.float64), color=((n, 3), torch.float64),
                      material=((n, 2), torch.float64))
        res = {}
        for name in self._ATTR_WANT:
            if name not in want:
                continue
            shape, dtype = shapes[name]
            t = out.get(name) if out else None
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=dev)
            elif not (isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and
                      t.device == dev):
                raise ValueError("hit_attributes: out[%r] must be a contiguous %s %r tensor on %s" % (name, dtype, shape, dev))
            res[name] = t
        if n == 0:
            return res
        ptr = lambda k: res[k].data_ptr() if k in res else None
        r = _capi.Rays(n, org.data_ptr(), dirs.data_ptr(), None, 0, 0, 1, 0)
        o = _capi.HitAttributes(ptr("prim"), ptr("uv"), ptr("color"), ptr("material"))
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(self._L.cgrt_ray_hit_attributes(self._h, C.byref(r), hit_obj.data_ptr(), hit_t.data_ptr(), C.byref(o), C.c_void_p(st)))
        return res

    def hit_attributes_host(self, org, dirs, hit_obj, hit_t, want=("prim", "uv", "color", "material")):
        """Synchronous form of hit_attributes on numpy arrays (no torch needed): dict of the arrays in `want`."""
        org = np.ascontiguousarray(org, np.float64)
        dirs = np.ascontiguousarray(dirs, np.float64)
        if org.ndim != 2 or org.shape[1] != 3 or dirs.shape != org.shape:
            raise ValueError("hit_attributes_host: org and dirs must be [n,3] arrays of one length")
        n = len(org)
        hit_obj = np.ascontiguousarray(hit_obj)
        hit_t = np.ascontiguousarray(hit_t)
        if hit_obj.dtype != np.int32 or hit_obj.shape != (n,):
            raise ValueError("hit_attributes_host: hit_obj must be an int32 [n] array")
        if hit_t.dtype != np.float64 or hit_t.shape != (n,):
            raise ValueError("hit_attributes_host: hit_t must be a float64 [n] array")
        want = tuple(want)
        if not want or any(w not in self._ATTR_WANT for w in want):
            raise ValueError("hit_attributes_host: want is a non-empty subset of %r" % (self._ATTR_WANT,))
        res = {}
        if "prim" in want:
            res["prim"] = np.full(n, -1, np.int32)
        if "uv" in want:
            res["uv"] = np.zeros((n, 2), np.float64)
        if "color" in want:
            res["color"] = np.zeros((n, 3), np.float64)
        if "material" in want:
            res["material"] = np.zeros((n, 2), np.float64)
        if n == 0:
            return res
        ptr = lambda k: res[k].ctypes.data if k in res else None
        r = _capi.Rays(n, org.ctypes.data, dirs.ctypes.data, None, 0, 0, 1, 0)
        o = _capi.HitAttributes(ptr("prim"), ptr("uv"), ptr("color"), ptr("material"))
        check(self._L.cgrt_ray_hit_attributes_host(self._h, C.byref(r), hit_obj.ctypes.data, hit_t.ctypes.data, C.byref(o)))
        return res

    # ---- occlusion queries of caller-supplied rays ----
    def occluded(self, org, dirs, tmax=None, keys=None, seed=12345, first_index=0, skip_transparent=False, stats=False, out=None,
                 stream=None):
        """cgrt_occlusion_rays on torch tensors: org, dirs float64 [n,3] contiguous on the scene's device, tmax float64 [n] or
        None (no limit), keys int64 [n] or None.  occluded[i] = 1 exactly when some object's intersect() length is < tmax[i]
        -- hit_obj >= 0 and hit_t < tmax of trace_rays(want=("hit",)) on the same rays --, else 0; a NaN tmax, a tmax <= 0
        (unless an object returns a length below zero: a ray starting on a sphere's surface) and a dirs row of zeros give 0.  skip_transparent: objects with transparency >= 1e-4 are no occluders (shadow rays through
        glass).  out: a preallocated uint8 [n] tensor, or a dict holding one as "occluded".  Asynchronous on torch's current
        stream (or `stream`).  Returns {"occluded": uint8 [n], "counters": int64 [8]}."""
        import torch

        dev = torch.device("cuda", self.device)
        for name, t in (("org", org), ("dirs", dirs)):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.dim() == 2 and t.shape[1] == 3 and
                    t.is_contiguous() and t.device == dev):
                raise ValueError("occluded: %s must be a contiguous float64 [n,3] tensor on %s" % (name, dev))
        n = org.shape[0]
        if dirs.shape[0] != n:
            raise ValueError("occluded: org and dirs differ in length")
        if tmax is not None and not (isinstance(tmax, torch.Tensor) and tmax.dtype == torch.float64 and tuple(tmax.shape) == (n,) and
                                     tmax.is_contiguous() and tmax.device == dev):
            raise ValueError("occluded: tmax must be a contiguous float64 [n] tensor on %s" % (dev,))
        if keys is not None and not (isinstance(keys, torch.Tensor) and keys.dtype == torch.int64 and tuple(keys.shape) == (n,) and
                                     keys.is_contiguous() and keys.device == dev):
            raise ValueError("occluded: keys must be a contiguous int64 [n] tensor on %s" % (dev,))
        occ = out.get("occluded") if isinstance(out, dict) else out
        if occ is None:
            occ = torch.empty((n,), dtype=torch.uint8, device=dev)
        elif not (isinstance(occ, torch.Tensor) and occ.dtype == torch.uint8 and tuple(occ.shape) == (n,) and occ.is_contiguous() and
                  occ.device == dev):
            raise ValueError("occluded: out must be a contiguous uint8 [n] tensor on %s" % (dev,))
        counters = torch.zeros((_capi.CGRT_NCOUNTERS,), dtype=torch.int64, device=dev)
        res = {"occluded": occ, "counters": counters}
        if n == 0:
            return res
        r = _capi.Rays(n, org.data_ptr(), dirs.data_ptr(), keys.data_ptr() if keys is not None else None, first_index, seed, 1,
                       (_capi.RAYS_STATS if stats else 0) | (_capi.RAYS_SKIP_TRANSPARENT if skip_transparent else 0))
        o = _capi.Occlusion(tmax.data_ptr() if tmax is not None else None, occ.data_ptr())
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(self._L.cgrt_occlusion_rays(self._h, C.byref(r), C.byref(o), counters.data_ptr(), C.c_void_p(st)))
        return res

    def occluded_host(self, org, dirs, tmax=None, keys=None, seed=12345, first_index=0, skip_transparent=False, stats=False):
        """Synchronous form of occluded on numpy arrays (no torch needed): dict(occluded (uint8 [n]), counters (uint64 [8]),
        nrays)."""
        org = np.ascontiguousarray(org, np.float64).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
        n = len(org)
        if len(dirs) != n:
            raise ValueError("occluded_host: org and dirs differ in length")
        if tmax is not None:
            tmax = np.ascontiguousarray(tmax, np.float64)
            if tmax.shape != (n,):
                raise ValueError("occluded_host: tmax must have one entry per ray")
        if keys is not None:
            keys = np.ascontiguousarray(keys, np.uint64)
            if keys.shape != (n,):
                raise ValueError("occluded_host: keys must have one entry per ray")
        occ = np.zeros(max(n, 1), np.uint8)
        cnt = np.zeros((_capi.CGRT_NCOUNTERS,), np.uint64)
        r = _capi.Rays(n, org.ctypes.data, dirs.ctypes.data, keys.ctypes.data if keys is not None else None, first_index, seed, 1,
                       (_capi.RAYS_STATS if stats else 0) | (_capi.RAYS_SKIP_TRANSPARENT if skip_transparent else 0))
        o = _capi.Occlusion(tmax.ctypes.data if tmax is not None else None, occ.ctypes.data)
        check(self._L.cgrt_occlusion_rays_host(self._h, C.byref(r), C.byref(o), cnt.ctypes.data))
        return dict(occluded=occ[:n], counters=cnt, nrays=int(cnt[_capi.CNT_RAYS]))

    def occlusion_variant(self, stats=False):
        """Name of the occlusion_rays_kernel instantiation occluded launches on this scene (cgrt_occlusion_rays_variant)."""
        r = _capi.Rays(1, None, None, None, 0, 0, 1, _capi.RAYS_STATS if stats else 0)
        buf = C.create_string_buffer(160)
        check(self._L.cgrt_occlusion_rays_variant(self._h, C.byref(r), buf, len(buf)))
        return buf.value.decode()

    # ---- bounce queries of caller-supplied rays: one step of trace() ----
    _BOUNCE = ("step", "hit_obj", "hit_t", "pos", "normal", "value", "child_org", "child_dir", "child_adj", "child_path", "child_keys")
    _BOUNCE_GROUPS = {"hit": ("hit_obj", "hit_t"), "children": ("child_org", "child_dir", "child_adj", "child_path", "child_keys")}

    def _bounce_want(self, what, want):
        names = []
        for w in tuple(want):
            for k in self._BOUNCE_GROUPS.get(w, (w,)):
                if k not in self._BOUNCE:
                    raise ValueError("%s: want is a non-empty subset of %r" % (what, self._BOUNCE + tuple(self._BOUNCE_GROUPS)))
                names.append(k)
        if not names:
            raise ValueError("%s: want is a non-empty subset of %r" % (what, self._BOUNCE + tuple(self._BOUNCE_GROUPS)))
        return [k for k in self._BOUNCE if k in names]

    def bounce(self, org, dirs, adj=None, path=None, keys=None, seed=12345, first_index=0,
               want=("step", "hit", "pos", "normal", "value", "children"), stats=False, out=None, stream=None, counters=None):
        """cgrt_bounce_rays on torch tensors: one scene walk per ray, then exactly the step trace() takes at the hit.  org, dirs
        float64 [n,3] contiguous on the scene's device; adj float64 [n,3] or None (the ray's throughput, (1,1,1)); path int32 [n]
        or None (position in the ray tree: root 1, reflected child 2p, refracted child 2p+1); keys int64 [n] or None.  want:
        which results -- "step" (uint8 [n]: _capi.STEP_NONE / _HITPOINT / _REFLECT / _SPLIT), "hit_obj" (int32 [n]), "hit_t"
        (float64 [n]), "pos", "normal" (float64 [n,3]: the hit point and the normal after trace()'s flip), "value" (float64
        [n,3]: f * adj of a Hitpoint, else 0), "child_org", "child_dir", "child_adj" (float64 [2n,3]), "child_path" (int32
        [2n]), "child_keys" (int64 [2n]): row i the reflected child of ray i, row n + i the refracted one, zeros where there is
        none -- the five can be passed back as the next level's org, dirs, adj, path, keys as they are (dirs = 0 rows are not
        traced) or compacted first.  "hit" and "children" name the groups.  There is no depth limit: the caller's loop decides.
        out: dict of preallocated result tensors to write into.  Asynchronous on torch's current stream (or `stream`); counters
        (int64 [8]) are ADDED to.  Returns a dict of the tensors and "counters"."""
        import torch

        dev = torch.device("cuda", self.device)
        n = self._ray_tensors("bounce", org, dirs, keys)
        if adj is not None and not (isinstance(adj, torch.Tensor) and adj.dtype == torch.float64 and tuple(adj.shape) == (n, 3) and
                                    adj.is_contiguous() and adj.device == dev):
            raise ValueError("bounce: adj must be a contiguous float64 [n,3] tensor on %s" % (dev,))
        if path is not None and not (isinstance(path, torch.Tensor) and path.dtype == torch.int32 and tuple(path.shape) == (n,) and
                                     path.is_contiguous() and path.device == dev):
            raise ValueError("bounce: path must be a contiguous int32 [n] tensor on %s" % (dev,))
        names = self._bounce_want("bounce", want)
        shapes = dict(step=((n,), torch.uint8), hit_obj=((n,), torch.int32), hit_t=((n,), torch.float64), pos=((n, 3), torch.float64),
                      normal=((n, 3), torch.float64), value=((n, 3), torch.float64), child_org=((2 * n, 3), torch.float64),
                      child_dir=((2 * n, 3), torch.float64), child_adj=((2 * n, 3), torch.float64), child_path=((2 * n,), torch.int32),
                      child_keys=((2 * n,), torch.int64))
        res = {}
        for name in names:
            shape, dtype = shapes[name]
            t = out.get(name) if out else None
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=dev)
            elif not (isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and
                      t.device == dev):
                raise ValueError("bounce: out[%r] must be a contiguous %s %r tensor on %s" % (name, dtype, shape, dev))
            res[name] = t
        if counters is None:
            counters = torch.zeros((_capi.CGRT_NCOUNTERS,), dtype=torch.int64, device=dev)
        elif not (counters.dtype == torch.int64 and counters.numel() == _capi.CGRT_NCOUNTERS and counters.is_contiguous() and
                  counters.device == dev):
            raise ValueError("bounce: counters must be a contiguous int64 [8] tensor on %s" % (dev,))
        res["counters"] = counters
        if n == 0:
            return res
        ptr = lambda k: res[k].data_ptr() if k in res else None
        r = _capi.Rays(n, org.data_ptr(), dirs.data_ptr(), keys.data_ptr() if keys is not None else None, first_index, seed, 1,
                       _capi.RAYS_STATS if stats else 0)
        b = _capi.Bounce(adj.data_ptr() if adj is not None else None, path.data_ptr() if path is not None else None,
                         *[ptr(k) for k in self._BOUNCE])
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(self._L.cgrt_bounce_rays(self._h, C.byref(r), C.byref(b), counters.data_ptr(), C.c_void_p(st)))
        return res

    def bounce_host(self, org, dirs, adj=None, path=None, keys=None, seed=12345, first_index=0,
                    want=("step", "hit", "pos", "normal", "value", "children"), stats=False):
        """Synchronous form of bounce on numpy arrays (no torch needed): dict of the arrays in `want` (child_path uint32,
        child_keys uint64), counters (uint64 [8]), nrays, nhp."""
        org = np.ascontiguousarray(org, np.float64).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
        n = len(org)
        if len(dirs) != n:
            raise ValueError("bounce_host: org and dirs differ in length")
        if adj is not None:
            adj = np.ascontiguousarray(adj, np.float64)
            if adj.shape != (n, 3):
                raise ValueError("bounce_host: adj must be an [n,3] array")
        if path is not None:
            path = np.ascontiguousarray(path, np.uint32)
            if path.shape != (n,):
                raise ValueError("bounce_host: path must have one entry per ray")
        if keys is not None:
            keys = np.ascontiguousarray(keys, np.uint64)
            if keys.shape != (n,):
                raise ValueError("bounce_host: keys must have one entry per ray")
        names = self._bounce_want("bounce_host", want)
        make = dict(step=lambda: np.zeros(n, np.uint8), hit_obj=lambda: np.full(n, -1, np.int32), hit_t=lambda: np.zeros(n, np.float64),
                    pos=lambda: np.zeros((n, 3), np.float64), normal=lambda: np.zeros((n, 3), np.float64),
                    value=lambda: np.zeros((n, 3), np.float64), child_org=lambda: np.zeros((2 * n, 3), np.float64),
                    child_dir=lambda: np.zeros((2 * n, 3), np.float64), child_adj=lambda: np.zeros((2 * n, 3), np.float64),
                    child_path=lambda: np.zeros(2 * n, np.uint32), child_keys=lambda: np.zeros(2 * n, np.uint64))
        res = {k: make[k]() for k in names}
        cnt = np.zeros((_capi.CGRT_NCOUNTERS,), np.uint64)
        ptr = lambda k: res[k].ctypes.data if k in res else None
        r = _capi.Rays(n, org.ctypes.data, dirs.ctypes.data, keys.ctypes.data if keys is not None else None, first_index, seed, 1,
                       _capi.RAYS_STATS if stats else 0)
        b = _capi.Bounce(adj.ctypes.data if adj is not None else None, path.ctypes.data if path is not None else None,
                         *[ptr(k) for k in self._BOUNCE])
        check(self._L.cgrt_bounce_rays_host(self._h, C.byref(r), C.byref(b), cnt.ctypes.data))
        res.update(counters=cnt, nrays=int(cnt[_capi.CNT_RAYS]), nhp=int(cnt[_capi.CNT_HITPOINTS]))
        return res

    def bounce_variant(self, stats=False):
        """Name of the bounce_rays_kernel instantiation bounce launches on this scene (cgrt_bounce_rays_variant)."""
        r = _capi.Rays(1, None, None, None, 0, 0, 1, _capi.RAYS_STATS if stats else 0)
        buf = C.create_string_buffer(160)
        check(self._L.cgrt_bounce_rays_variant(self._h, C.byref(r), buf, len(buf)))
        return buf.value.decode()

    # ---- wavefront trace of caller-supplied rays: any depth, the depth loop inside the library ----
    _WAVEFRONT = ("acc", "nhit", "hp")

    def _wavefront_want(self, what, want):
        want = tuple(want)
        if any(w not in self._WAVEFRONT for w in want):
            raise ValueError("%s: want is a subset of %r" % (what, self._WAVEFRONT))
        return want

    def last_wavefront(self):
        """What the last wavefront call on this scene did (cgrt_scene_last_wavefront, _rays): dict(slices, halvings, levels,
        rays_per_level (the rays traced at levels 1 .. levels))."""
        sl, hv, lv = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        check(self._L.cgrt_scene_last_wavefront(self._h, C.byref(sl), C.byref(hv), C.byref(lv)))
        rays = np.zeros(_capi.WAVEFRONT_MAX_DEPTH, np.int64)
        check(self._L.cgrt_scene_last_wavefront_rays(self._h, rays.ctypes.data))
        return dict(slices=int(sl.value), halvings=int(hv.value), levels=int(lv.value), rays_per_level=[int(x) for x in rays[:lv.value]])

    def wavefront(self, org, dirs, keys=None, max_depth=8, min_adj=0.0, seed=12345, first_index=0, want=("acc", "nhit"), hp_cap=None,
                  work_bytes=0, stats=False, out=None, stream=None, counters=None):
        """cgrt_wavefront_rays on torch tensors: every ray traced to max_depth levels (1..31) as a wavefront on the device -- the
        depth loop over bounce with its compaction and its emission-order sum, inside the library.  org, dirs float64 [n,3]
        contiguous on the scene's device, keys int64 [n] or None.  min_adj: a child whose throughput has max(x,y,z) < min_adj
        is not spawned (0 drops nothing).  want: "acc" (float64 [n,3]) and "nhit" (int32 [n]) as trace_rays gives them for
        max_depth <= 5; "hp": the Hitpoint records by ray, then emission order -- hp9 (float64 [m,9]: value, pos, normal), hp_ray
        (int64 [m]), hp_path (int32 [m]), m = min(hp_count, hp_cap); hp_cap defaults to 4n.  work_bytes: device work memory
        (0 = automatic); the results never depend on it.  out: dict of preallocated tensors (acc, nhit; hp9, hp_ray, hp_path
        of hp_cap rows).  The call runs on torch's current stream (or `stream`) and SYNCHRONISES it; counters (int64 [8]) are
        ADDED to.  Returns a dict of the tensors, "counters", "hp_count" and last_wavefront()'s entries."""
        import torch

        dev = torch.device("cuda", self.device)
        n = self._ray_tensors("wavefront", org, dirs, keys)
        want = self._wavefront_want("wavefront", want)
        if not (isinstance(max_depth, int) and 1 <= max_depth <= _capi.WAVEFRONT_MAX_DEPTH):
            raise ValueError("wavefront: max_depth must be 1..%d" % _capi.WAVEFRONT_MAX_DEPTH)
        if not (min_adj >= 0.0) or work_bytes < 0 or (hp_cap is not None and hp_cap < 0):
            raise ValueError("wavefront: min_adj, work_bytes and hp_cap must be >= 0")
        cap = int(hp_cap if hp_cap is not None else 4 * n) if "hp" in want else 0
        shapes = {}
        if "acc" in want:
            shapes["acc"] = ((n, 3), torch.float64)
        if "nhit" in want:
            shapes["nhit"] = ((n,), torch.int32)
        if cap > 0:
            shapes.update(hp9=((cap, 9), torch.float64), hp_ray=((cap,), torch.int64), hp_path=((cap,), torch.int32))
        res = {}
        for name, (shape, dtype) in shapes.items():
            t = out.get(name) if out else None
            if t is None:
                t = torch.empty(shape, dtype=dtype, device=dev)
            elif not (isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and
                      t.device == dev):
                raise ValueError("wavefront: out[%r] must be a contiguous %s %r tensor on %s" % (name, dtype, shape, dev))
            res[name] = t
        if counters is None:
            counters = torch.zeros((_capi.CGRT_NCOUNTERS,), dtype=torch.int64, device=dev)
        elif not (counters.dtype == torch.int64 and counters.numel() == _capi.CGRT_NCOUNTERS and counters.is_contiguous() and
                  counters.device == dev):
            raise ValueError("wavefront: counters must be a contiguous int64 [8] tensor on %s" % (dev,))
        ptr = lambda k: res[k].data_ptr() if k in res else None
        r = _capi.Rays(n, org.data_ptr(), dirs.data_ptr(), keys.data_ptr() if keys is not None else None, first_index, seed, 1,
                       _capi.RAYS_STATS if stats else 0)
        w = _capi.Wavefront(max_depth, 0, float(min_adj), int(work_bytes), ptr("acc"), ptr("nhit"), ptr("hp9"), ptr("hp_ray"),
                            ptr("hp_path"), cap)
        cnt = C.c_uint64(0)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(self._L.cgrt_wavefront_rays(self._h, C.byref(r), C.byref(w), counters.data_ptr(), C.byref(cnt), C.c_void_p(st)))
        m = min(int(cnt.value), cap)
        for k in ("hp9", "hp_ray", "hp_path"):
            if k in res:
                res[k] = res[k][:m]
        if "hp" in want and cap == 0:
            res.update(hp9=torch.empty((0, 9), dtype=torch.float64, device=dev), hp_ray=torch.empty((0,), dtype=torch.int64, device=dev),
                       hp_path=torch.empty((0,), dtype=torch.int32, device=dev))
        res.update(counters=counters, hp_count=int(cnt.value))
        res.update(self.last_wavefront() if n > 0 else dict(slices=0, halvings=0, levels=0, rays_per_level=[]))
        return res

    def wavefront_host(self, org, dirs, keys=None, max_depth=8, min_adj=0.0, seed=12345, first_index=0, want=("acc", "nhit"),
                       hp_cap=None, work_bytes=0, stats=False):
        """Synchronous form of wavefront on numpy arrays (no torch needed): dict of acc, nhit (uint32), hp9, hp_ray, hp_path
        (uint32) -- those in `want` --, counters (uint64 [8]), nrays, nhp, hp_count and last_wavefront()'s entries."""
        org = np.ascontiguousarray(org, np.float64).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
        n = len(org)
        if len(dirs) != n:
            raise ValueError("wavefront_host: org and dirs differ in length")
        if keys is not None:
            keys = np.ascontiguousarray(keys, np.uint64)
            if keys.shape != (n,):
                raise ValueError("wavefront_host: keys must have one entry per ray")
        want = self._wavefront_want("wavefront_host", want)
        if not (isinstance(max_depth, int) and 1 <= max_depth <= _capi.WAVEFRONT_MAX_DEPTH):
            raise ValueError("wavefront_host: max_depth must be 1..%d" % _capi.WAVEFRONT_MAX_DEPTH)
        if not (min_adj >= 0.0) or work_bytes < 0 or (hp_cap is not None and hp_cap < 0):
            raise ValueError("wavefront_host: min_adj, work_bytes and hp_cap must be >= 0")
        cap = int(hp_cap if hp_cap is not None else 4 * n) if "hp" in want else 0
        res = {}
        if "acc" in want:
            res["acc"] = np.zeros((n, 3), np.float64)
        if "nhit" in want:
            res["nhit"] = np.zeros(n, np.uint32)
        if "hp" in want:
            res.update(hp9=np.zeros((cap, 9), np.float64), hp_ray=np.zeros(cap, np.int64), hp_path=np.zeros(cap, np.uint32))
        cnt = np.zeros((_capi.CGRT_NCOUNTERS,), np.uint64)
        ptr = lambda k: res[k].ctypes.data if k in res and res[k].size else None
        r = _capi.Rays(n, org.ctypes.data, dirs.ctypes.data, keys.ctypes.data if keys is not None else None, first_index, seed, 1,
                       _capi.RAYS_STATS if stats else 0)
        w = _capi.Wavefront(max_depth, 0, float(min_adj), int(work_bytes), ptr("acc"), ptr("nhit"), ptr("hp9"), ptr("hp_ray"),
                            ptr("hp_path"), cap)
        hpc = C.c_uint64(0)
        check(self._L.cgrt_wavefront_rays_host(self._h, C.byref(r), C.byref(w), cnt.ctypes.data, C.byref(hpc)))
        m = min(int(hpc.value), cap)
        for k in ("hp9", "hp_ray", "hp_path"):
            if k in res:
                res[k] = res[k][:m]
        res.update(counters=cnt, nrays=int(cnt[_capi.CNT_RAYS]), nhp=int(cnt[_capi.CNT_HITPOINTS]), hp_count=int(hpc.value))
        res.update(self.last_wavefront() if n > 0 else dict(slices=0, halvings=0, levels=0, rays_per_level=[]))
        return res

    def wavefront_variant(self, stats=False):
        """Name of the wavefront_step_kernel instantiation wavefront launches on this scene (cgrt_wavefront_rays_variant)."""
        r = _capi.Rays(1, None, None, None, 0, 0, 1, _capi.RAYS_STATS if stats else 0)
        buf = C.create_string_buffer(160)
        check(self._L.cgrt_wavefront_rays_variant(self._h, C.byref(r), buf, len(buf)))
        return buf.value.decode()

    def rays_variant(self, max_depth=5, want=("acc", "nhit", "hit"), stats=False):
        """Name of the trace_rays_kernel instantiation trace_rays launches for these arguments (cgrt_trace_rays_variant)."""
        full = 1 if ("acc" in want or "nhit" in want) else None
        r = _capi.Rays(1, None, None, None, 0, 0, max_depth, _capi.RAYS_STATS if stats else 0)
        o = _capi.RayResults(full, None, 1 if "hit" in want else None, None, None)
        buf = C.create_string_buffer(160)
        check(self._L.cgrt_trace_rays_variant(self._h, C.byref(r), C.byref(o), buf, len(buf)))
        return buf.value.decode()

    def trace_grid_host(self, width, height, spp=1, camera=None, max_depth=5, seed=12345, rows=None, row_offset=0,
                        stripe=None, sample_offset=0, spp_total=None, stats=False, split_samples=False, reorder=True,
                        force_reorder=False, tile_order=True, diffuse_tiles=False, sphere_pairs=True, sphere_masks=True, sample_relay=None,
                        relay_mirror=None, relay_order=None, lens_stage=True, sure_tiles=True, relay_start=None, relay_boost=None, lens_table=None,
                   inside_trips=True):
        """Synchronous form with numpy outputs (no torch needed): dict(rgb, nhit, counters)."""
        rows = height - row_offset if rows is None else rows
        rgb = np.zeros((rows, width, 3), np.float32)
        nhit = np.zeros((rows, width), np.uint32)
        cnt = np.zeros((_capi.CGRT_NCOUNTERS,), np.uint64)
        cc, g = self._structs(camera, width, height, rows, spp, max_depth, seed, row_offset, stripe, sample_offset,
                              spp_total,
                              _grid_flags(stats, split_samples, reorder, force_reorder, tile_order, diffuse_tiles, sphere_pairs, sphere_masks, lens_stage, sure_tiles, lens_table, inside_trips) |
                              _relay_flag(sample_relay, relay_mirror, relay_order, relay_start, relay_boost))
        check(self._L.cgrt_trace_grid_host(self._h, C.byref(cc), C.byref(g), rgb.ctypes.data, nhit.ctypes.data,
                                           cnt.ctypes.data))
        return dict(rgb=rgb, nhit=nhit, counters=cnt, nrays=int(cnt[_capi.CNT_RAYS]),
                    nhp=int(cnt[_capi.CNT_HITPOINTS]))

    def last_tile_order(self):
        """The tile order of this scene's last trace_grid / trace_grid_host (cgrt_scene_last_tile_order; synchronises the
        device): None when that launch ran no ordering kernel, else dict(plan [5] uint32: tiles of classes < c,
        list [n] uint32: the tile workgroup i rendered, cls [n] uint8: class of tile t)."""
        n = C.c_int64()
        check(self._L.cgrt_scene_last_tile_order(self._h, None, None, None, 0, C.byref(n)))
        if n.value == 0:
            return None
        plan, lst, cls = np.zeros(5, np.uint32), np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint8)
        check(self._L.cgrt_scene_last_tile_order(self._h, plan.ctypes.data, lst.ctypes.data, cls.ctypes.data, n.value, C.byref(n)))
        return dict(plan=plan, list=lst, cls=cls)

    def last_sphere_masks(self):
        """The sphere masks of this scene's last trace_grid / trace_grid_host (cgrt_scene_last_sphere_masks; synchronises the
        device): None when that launch wrote none, else uint32 [wave tiles], bit i = sphere i may be met by a primary ray of
        the 16x4 wave tile wy * ceil(width / 16) + wx."""
        n = C.c_int64()
        check(self._L.cgrt_scene_last_sphere_masks(self._h, None, 0, C.byref(n)))
        if n.value == 0:
            return None
        masks = np.zeros(n.value, np.uint32)
        check(self._L.cgrt_scene_last_sphere_masks(self._h, masks.ctypes.data, n.value, C.byref(n)))
        return masks

    def last_sure_tiles(self):
        """The sure tiles of this scene's last trace_grid / trace_grid_host (cgrt_scene_last_sure_tiles; synchronises the device):
        None when that launch wrote none, else uint8 [wave tiles]: the sphere every primary ray of the 16x4 wave tile
        wy * ceil(width / 16) + wx hits first, or 255 (none proven, or its 32x8 tile is not of class 3)."""
        n = C.c_int64()
        check(self._L.cgrt_scene_last_sure_tiles(self._h, None, 0, C.byref(n)))
        if n.value == 0:
            return None
        sure = np.zeros(n.value, np.uint8)
        check(self._L.cgrt_scene_last_sure_tiles(self._h, sure.ctypes.data, n.value, C.byref(n)))
        return sure

    def inside_spheres(self):
        """The committed scene's inside spheres (cgrt_scene_inside_spheres; a scene trait, no launch): a list of
        dict(index: the refracting sphere's place in the object list, mask: bit j = sphere j can be the first hit of a ray that
        starts inside it -- all bits: the unchanged loop --, rin2: the squared radius below which an origin counts as inside).
        Empty: the scene has no such trait (several refracting spheres, more than 32 objects, an object that is no sphere)."""
        n = C.c_int32()
        check(self._L.cgrt_scene_inside_spheres(self._h, None, None, None, 0, C.byref(n)))
        idx, mask, rin2 = np.zeros(max(n.value, 1), np.int32), np.zeros(max(n.value, 1), np.uint32), np.zeros(max(n.value, 1), np.float64)
        check(self._L.cgrt_scene_inside_spheres(self._h, idx.ctypes.data, mask.ctypes.data, rin2.ctypes.data, n.value, C.byref(n)))
        return [dict(index=int(idx[k]), mask=int(mask[k]), rin2=float(rin2[k])) for k in range(n.value)]

    def inside_probe(self, rays):
        """cgrt_inside_probe(CGRT_PROBE_INSIDE_LOOP): the pair kernels' sphere loop over this scene for rays [n,6] = origin,
        direction; elements 64k .. 64k+63 are the lanes of one wave.  Returns float64 [n,5]: t, id of the pair loop, t, id of
        the guarded loop, 1 where the element's wave took the one-by-one loop."""
        rays = np.ascontiguousarray(rays, np.float64)
        assert rays.ndim == 2 and rays.shape[1] == 6
        out = np.zeros((rays.shape[0], 5), np.float64)
        check(self._L.cgrt_inside_probe(self._h, _capi.PROBE_INSIDE_LOOP, rays.ctypes.data, rays.shape[0], out.ctypes.data))
        return out

    def last_tile_order_reused(self):
        """True when this scene's last trace_grid / trace_grid_host ran no ordering kernel because the handle still held the
        order of the same camera and frame geometry (cgrt_scene_last_tile_order_reused)."""
        f = C.c_int32()
        check(self._L.cgrt_scene_last_tile_order_reused(self._h, C.byref(f)))
        return bool(f.value)

    def last_sample_relay(self):
        """What this scene's last trace_grid / trace_grid_host relayed (cgrt_scene_last_sample_relay; synchronises the device):
        dict(tiles: tiles rendered by several workgroups (0: none), chunks: workgroups of each, parked_values: Hitpoint values
        that went through the relay area, 24 bytes each)."""
        t, k, v = C.c_int64(), C.c_int32(), C.c_int64()
        check(self._L.cgrt_scene_last_sample_relay(self._h, C.byref(t), C.byref(k), C.byref(v)))
        return dict(tiles=int(t.value), chunks=int(k.value), parked_values=int(v.value))

    def last_relay_form(self):
        """The form of that relay (cgrt_scene_last_relay_form): None when the launch did not relay, else dict(mirror: the tiles
        that see only a mirror sphere were relayed too, order: "chunks_first", "mirror_first" or "interleaved")."""
        m, o = C.c_int32(), C.c_int32()
        check(self._L.cgrt_scene_last_relay_form(self._h, C.byref(m), C.byref(o)))
        return None if m.value < 0 else dict(mirror=bool(m.value), order=_RELAY_ORDERS[o.value])

    def last_relay_start(self):
        """The start table of that relay (cgrt_scene_last_relay_start; synchronises the device): None when the launch had none,
        else dict(t: workgroups of classes 0-2, start [t] uint32: entry << 2 | chunk of workgroup b, wcost [wave tiles] uint32:
        the probe's iteration counts, reused: probe and ranking were an earlier launch's)."""
        t, n, r = C.c_int64(), C.c_int64(), C.c_int32()
        check(self._L.cgrt_scene_last_relay_start(self._h, None, 0, None, 0, C.byref(t), C.byref(n), C.byref(r)))
        if n.value == 0:
            return None
        start, wcost = np.zeros(max(t.value, 1), np.uint32), np.zeros(n.value, np.uint32)
        check(self._L.cgrt_scene_last_relay_start(self._h, start.ctypes.data, start.size, wcost.ctypes.data, n.value, C.byref(t),
                                                  C.byref(n), C.byref(r)))
        return dict(t=int(t.value), start=start[:t.value], wcost=wcost, reused=bool(r.value))

    def last_relay_boost(self):
        """Promotion in that launch (cgrt_scene_last_relay_boost; synchronises the device): None when the launch promoted by no
        table, else dict(promoted: tiles rendered by k_boost workgroups, k_boost, boost_cap: tiles the second area held, S: the
        sum of tile cost x samples over classes 0-2, num, den: the threshold, wg_slots, bslot [relayed tiles] uint32: boost
        slot + 1 of list entry e, 0 where it was not promoted)."""
        p, k, cap, S = C.c_int64(), C.c_int32(), C.c_int64(), C.c_uint64()
        num, den, ws = C.c_int32(), C.c_int32(), C.c_int32()
        tiles = self.last_sample_relay()["tiles"]
        bslot = np.zeros(max(tiles, 1), np.uint32)
        check(self._L.cgrt_scene_last_relay_boost(self._h, C.byref(p), C.byref(k), C.byref(cap), C.byref(S), C.byref(num), C.byref(den),
                                                  C.byref(ws), bslot.ctypes.data, bslot.size))
        if k.value == 0:
            return None
        return dict(promoted=int(p.value), k_boost=int(k.value), boost_cap=int(cap.value), S=int(S.value), num=int(num.value),
                    den=int(den.value), wg_slots=int(ws.value), bslot=bslot[:tiles])

    def last_lens_table(self):
        """The lens table in this scene's last trace_grid / trace_grid_host (cgrt_scene_last_lens_table; synchronises the device):
        dict(entries: tile-order list entries whose workgroups read their lens draws from the table, capacity: the entries the table
        held, reused: the launch found it written by an earlier one).  All zero: the launch read no table."""
        a, b, r = C.c_int64(), C.c_int64(), C.c_int32()
        check(self._L.cgrt_scene_last_lens_table(self._h, C.byref(a), C.byref(b), C.byref(r)))
        return dict(entries=int(a.value), capacity=int(b.value), reused=bool(r.value))

    def last_lens_stage(self):
        """Lens points staged ahead by this scene's last trace_grid / trace_grid_host (cgrt_scene_last_lens_stage; synchronises
        the device): dict(lds_tiles: tiles whose workgroups staged their lens draws in LDS batches, area_tiles: always 0)."""
        a, b = C.c_int64(), C.c_int64()
        check(self._L.cgrt_scene_last_lens_stage(self._h, C.byref(a), C.byref(b)))
        return dict(lds_tiles=int(a.value), area_tiles=int(b.value))

    def last_diffuse_tiles(self):
        """Tiles the terminal-diffuse launch of this scene's last trace_grid / trace_grid_host rendered
        (cgrt_scene_last_diffuse_tiles; synchronises the device); 0: that call issued none."""
        n = C.c_int64()
        check(self._L.cgrt_scene_last_diffuse_tiles(self._h, C.byref(n)))
        return int(n.value)

    def last_inkernel_diffuse_tiles(self):
        """Tiles of this scene's last trace_grid / trace_grid_host whose workgroups ran the terminal-diffuse body inside the
        main launch (cgrt_scene_last_inkernel_diffuse_tiles; synchronises the device); 0: none did."""
        n = C.c_int64()
        check(self._L.cgrt_scene_last_inkernel_diffuse_tiles(self._h, C.byref(n)))
        return int(n.value)

    def trace_grid_hitpoints(self, width, height, spp=1, camera=None, max_depth=5, seed=12345, rows=None,
                             row_offset=0, cap=None):
        """The reference's Hitpoint records for the grid (unordered): dict(hp [n,9] = f,pos,normal; pix [n];
        smp [n]; count)."""
        rows = height - row_offset if rows is None else rows
        cap = int(cap if cap is not None else rows * width * spp * 16)
        rec = np.zeros((max(cap, 1), 10), np.float64)
        n = C.c_uint64(0)
        cc, g = self._structs(camera, width, height, rows, spp, max_depth, seed, row_offset, None, 0, None, 0)
        check(self._L.cgrt_trace_grid_hitpoints(self._h, C.byref(cc), C.byref(g), rec.ctypes.data, cap, C.byref(n)))
        m = min(int(n.value), cap)
        lab = rec[:m, 9].astype(np.int64)
        seq, lab = lab & 15, lab >> 4
        return dict(hp=rec[:m, :9].copy(), pix=lab % (rows * width), smp=lab // (rows * width), seq=seq,
                    count=int(n.value))

    def ppm_render(self, width, height, spp=1, camera=None, max_depth=5, seed=12345, nphotons=100000, photon_seed=777,
                   hashsize=1000001, light=(0.0, 19.999, 20.0), jitter=2.0, power=700.0, alpha=0.7, batch=0,
                   want_hitpoints=False, want_rgb8=False, rows=None, row_offset=0, stripe=None, initial_radius=0.0,
                   pair_cap=0):
        """Eye pass + photon pass + final gather (+ tone map): render() main.cpp:169-258 with the serial photon
        semantics, and the PNG pixel loop of main.cpp:403-412.
        rows / row_offset / stripe select this rank's share of the frame exactly as in trace_grid (every rank traces
        all photons and owns only its rows' hitpoints; the rows equal those of a full-frame call bit for bit).
        initial_radius: the reference's 200/height of main.cpp:84,183 (0 = 200/768, its committed height); pair_cap: size
        of the per-batch pair buffer (0 = automatic; the result does not depend on it).
        Returns dict(image [rows,W,3] float64 (row 0 = bottom), count, n_events, n_pairs, ms (stage times); with
        want_hitpoints: hp [n,16]; with want_rgb8 (contiguous rows only): rgb8 [rows,W,3] uint8, top row first)."""
        rows = height if rows is None else rows
        cc, g = self._structs(camera, width, height, rows, spp, max_depth, seed, row_offset, stripe, 0, None, 0)
        ph = _capi.Photons(_d3(light), jitter, power, alpha, nphotons, hashsize, batch, photon_seed, initial_radius, pair_cap)
        height = rows
        img = np.zeros((height, width, 3), np.float64)
        cap = height * width * spp * 16 if want_hitpoints else 0
        hp = np.zeros((max(cap, 1), 16), np.float64)
        rgb8 = np.zeros((height, width, 3), np.uint8)
        res = _capi.PpmResult(img.ctypes.data, rgb8.ctypes.data if want_rgb8 else None,
                              hp.ctypes.data if want_hitpoints else None, cap)
        check(self._L.cgrt_ppm_render(self._h, C.byref(cc), C.byref(g), C.byref(ph), C.byref(res)))
        out = dict(image=img, count=int(res.hp_count), n_events=int(res.n_events), n_pairs=int(res.n_pairs),
                   n_batch_halvings=int(res.n_batch_halvings),
                   ms=dict(eye=res.ms_eye, table=res.ms_table, photons=res.ms_photons, gather=res.ms_gather))
        if want_hitpoints:
            out["hp"] = hp[: int(res.hp_count)]
        if want_rgb8:
            out["rgb8"] = rgb8
        return out

    def ppm_session(self, width, height, spp=1, camera=None, max_depth=5, seed=12345, nphotons=0, photon_seed=777,
                    hashsize=1000001, light=(0.0, 19.999, 20.0), jitter=2.0, power=700.0, alpha=0.7, batch=0, rows=None,
                    row_offset=0, stripe=None, initial_radius=0.0, pair_cap=0, lookahead=True):
        """A live photon-mapping render (cgrt_ppm_session): eye pass and table now, then `nphotons` photons (0 allowed);
        PpmSession.add_photons(n) traces more.  Same keywords as ppm_render; after photons totalling k the image, rgb8 and
        hitpoints are ppm_render(nphotons=k)'s bit for bit.  lookahead=False: CGRT_PPM_SESSION_NO_LOOKAHEAD (no batch is
        traced ahead for the next call)."""
        rows = height if rows is None else rows
        cc, g = self._structs(camera, width, height, rows, spp, max_depth, seed, row_offset, stripe, 0, None, 0)
        ph = _capi.Photons(_d3(light), jitter, power, alpha, nphotons, hashsize, batch, photon_seed, initial_radius, pair_cap)
        h = C.c_void_p()
        check(self._L.cgrt_ppm_session_create(self._h, C.byref(cc), C.byref(g), C.byref(ph),
                                              0 if lookahead else _capi.PPM_SESSION_NO_LOOKAHEAD, C.byref(h)))
        ses = PpmSession(self, h, width, rows, spp)
        self._sessions.add(ses)
        return ses

    def sppm_session(self, width, height, spp=1, camera=None, photon_depth=5, max_depth=5, seed=12345, photon_seed=777,
                     hashsize=1000001, light=(0.0, 19.999, 20.0), jitter=2.0, power=700.0, alpha=0.7, batch=0, rows=None,
                     row_offset=0, stripe=None, initial_radius=0.0, pair_cap=0):
        """Stochastic progressive photon mapping (cgrt_sppm_session): N, R2 and tau belong to the texel, every pass traces
        fresh eye samples and fresh photons, memory does not grow with the passes.  Returns an SppmSession without a pass;
        add_passes(n, photons_per_pass) renders with `camera` (kept here; max_depth is the eye depth, seed the lens streams')
        at sample_offset = passes * spp, add_pass_rays with the caller's rays.  rows / row_offset / stripe: this rank's share
        of a width x height frame as in ppm_session (every rank traces all photons)."""
        rows = height if rows is None else rows
        ph = _capi.Photons(_d3(light), jitter, power, alpha, 0, hashsize, batch, photon_seed, initial_radius, pair_cap)
        h = C.c_void_p()
        check(self._L.cgrt_sppm_session_create(self._h, width, rows, spp, photon_depth, C.byref(ph), 0, C.byref(h)))
        ses = SppmSession(self, h, width, rows, spp, dict(camera=camera, height=height, max_depth=max_depth, seed=seed,
                                                          row_offset=row_offset, stripe=stripe))
        self._sessions.add(ses)
        return ses

    def _ray_tensors(self, what, org, dirs, keys, pixel=None):
        """The argument checks of trace_rays for the ray-buffer calls; returns n."""
        import torch

        dev = torch.device("cuda", self.device)
        for name, t in (("org", org), ("dirs", dirs)):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.dim() == 2 and t.shape[1] == 3 and
                    t.is_contiguous() and t.device == dev):
                raise ValueError("%s: %s must be a contiguous float64 [n,3] tensor on %s" % (what, name, dev))
        n = org.shape[0]
        if dirs.shape[0] != n:
            raise ValueError("%s: org and dirs differ in length" % what)
        for name, t in (("keys", keys), ("pixel", pixel)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.int64 and tuple(t.shape) == (n,) and
                                      t.is_contiguous() and t.device == dev):
                raise ValueError("%s: %s must be a contiguous int64 [n] tensor on %s" % (what, name, dev))
        return n

    def trace_rays_hitpoints(self, org, dirs, keys=None, max_depth=5, seed=12345, first_index=0, cap=None):
        """cgrt_trace_rays_hitpoints: the Hitpoints of the rays' trees (torch tensors as for trace_rays), unordered:
        dict(hp [m,9] = f, pos, normal (after the flip of main.cpp:73-76); ray [m]; seq [m] (position in the ray tree's
        emission order); count (Hitpoints produced; m = min(count, cap))).  Synchronous."""
        if not self.stats()["committed"]:
            check(self._L.cgrt_trace_rays_hitpoints(self._h, C.byref(_capi.Rays(0, None, None, None, 0, 0, max_depth, 0)), None, 0,
                                                    C.byref(C.c_uint64(0))))
        n = self._ray_tensors("trace_rays_hitpoints", org, dirs, keys)
        cap = int(cap if cap is not None else n * 16)
        rec = np.zeros((max(cap, 1), 10), np.float64)
        cnt = C.c_uint64(0)
        r = _capi.Rays(n, org.data_ptr(), dirs.data_ptr(), keys.data_ptr() if keys is not None else None, first_index, seed,
                       max_depth, 0)
        check(self._L.cgrt_trace_rays_hitpoints(self._h, C.byref(r), rec.ctypes.data, cap, C.byref(cnt)))
        m = min(int(cnt.value), cap)
        lab = rec[:m, 9].astype(np.int64)
        return dict(hp=rec[:m, :9].copy(), ray=lab >> 4, seq=lab & 15, count=int(cnt.value))

    def ppm_session_rays(self, org, dirs, keys=None, *, width, rows, spp=1, pixel=None, max_depth=5, seed=12345, first_index=0,
                         nphotons=0, photon_seed=777, hashsize=1000001, light=(0.0, 19.999, 20.0), jitter=2.0, power=700.0,
                         alpha=0.7, batch=0, initial_radius=0.0, pair_cap=0, lookahead=True):
        """A live photon-mapping render over caller-supplied rays (cgrt_ppm_session_create_rays): org, dirs, keys as for
        trace_rays; the session gathers into a [rows, width, 3] image, ray i into texel pixel[i] (int64 [n] on the scene's
        device; negative: the ray is not traced), or i % (width * rows) without `pixel` -- camera_rays' order.  spp is the
        gather's normaliser (rays per texel).  Returns a PpmSession; its hitpoints()[:, 0] is the ray index.  For
        camera_rays(width, rows, spp, ...) without `pixel` the session equals ppm_session on that grid bit for bit."""
        if not self.stats()["committed"]:  # the library's own answer (no tensor is looked at)
            check(self._L.cgrt_ppm_session_create_rays(self._h, C.byref(_capi.Rays(0, None, None, None, 0, 0, max_depth, 0)),
                                                       C.byref(_capi.RayPixels(width, rows, spp, 0, None)),
                                                       C.byref(_capi.Photons(_d3(light), jitter, power, alpha, 0, hashsize, batch,
                                                                             photon_seed, initial_radius, pair_cap)),
                                                       0, C.byref(C.c_void_p())))
        n = self._ray_tensors("ppm_session_rays", org, dirs, keys, pixel)
        r = _capi.Rays(n, org.data_ptr(), dirs.data_ptr(), keys.data_ptr() if keys is not None else None, first_index, seed,
                       max_depth, 0)
        px = _capi.RayPixels(width, rows, spp, 0, pixel.data_ptr() if pixel is not None else None)
        ph = _capi.Photons(_d3(light), jitter, power, alpha, nphotons, hashsize, batch, photon_seed, initial_radius, pair_cap)
        h = C.c_void_p()
        import torch

        torch.cuda.current_stream(org.device).synchronize()  # the session's eye stage runs on the null stream
        check(self._L.cgrt_ppm_session_create_rays(self._h, C.byref(r), C.byref(px), C.byref(ph),
                                                   0 if lookahead else _capi.PPM_SESSION_NO_LOOKAHEAD, C.byref(h)))
        ses = PpmSession(self, h, width, rows, spp)
        self._sessions.add(ses)
        return ses

    def ppm_session_hitpoints(self, hp9, ray=None, path=None, pixel=None, *, width, rows, spp=1, max_depth=5, nphotons=0,
                              photon_seed=777, hashsize=1000001, light=(0.0, 19.999, 20.0), jitter=2.0, power=700.0, alpha=0.7,
                              batch=0, initial_radius=0.0, pair_cap=0, lookahead=True):
        """A live photon-mapping render over caller-supplied Hitpoint records (cgrt_ppm_session_create_hitpoints): hp9 float64
        [n,9] (value = f * adj, pos, normal after the flip: wavefront's hp9), ray int64 [n] (the record's ray or probe id; None:
        its index), path int32 or uint32 [n] (its place in the ray's tree; None: the root), pixel int64 [n] (the texel it gathers
        into; None: ray % (width * rows)) -- contiguous tensors on the scene's device.  A record without a texel in the image,
        with path 0, a negative ray or a non-finite pos is dropped.  spp is the gather's normaliser and max_depth the PHOTONS'
        depth limit (1..5).  Returns a PpmSession; hitpoints()[:, 0] is the ray id, [:, 1] the record's rank within its ray.  The
        records wavefront(max_depth <= 5, want=("hp",)) returns give ppm_session_rays' session on the same rays bit for bit."""
        ph = _capi.Photons(_d3(light), jitter, power, alpha, nphotons, hashsize, batch, photon_seed, initial_radius, pair_cap)
        if not self.stats()["committed"]:  # the library's own answer (no tensor is looked at)
            check(self._L.cgrt_ppm_session_create_hitpoints(self._h, C.byref(_capi.Hitpoints(0, None, None, None, None, width, rows,
                                                                                             spp, max_depth)),
                                                            C.byref(ph), 0, C.byref(C.c_void_p())))
        import torch

        dev = torch.device("cuda", self.device)
        if not (isinstance(hp9, torch.Tensor) and hp9.dtype == torch.float64 and hp9.dim() == 2 and hp9.shape[1] == 9 and
                hp9.is_contiguous() and hp9.device == dev):
            raise ValueError("ppm_session_hitpoints: hp9 must be a contiguous float64 [n,9] tensor on %s" % (dev,))
        n = hp9.shape[0]
        uint32 = getattr(torch, "uint32", torch.int32)
        for name, t, dts in (("ray", ray, (torch.int64,)), ("path", path, (torch.int32, uint32)), ("pixel", pixel, (torch.int64,))):
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype in dts and tuple(t.shape) == (n,) and
                                      t.is_contiguous() and t.device == dev):
                raise ValueError("ppm_session_hitpoints: %s must be a contiguous %s [n] tensor on %s" % (name, dts[0], dev))
        ptr = lambda t: t.data_ptr() if t is not None and n > 0 else None
        hps = _capi.Hitpoints(n, ptr(hp9), ptr(ray), ptr(path), ptr(pixel), width, rows, spp, max_depth)
        h = C.c_void_p()
        torch.cuda.current_stream(dev).synchronize()  # the table build runs on the null stream
        check(self._L.cgrt_ppm_session_create_hitpoints(self._h, C.byref(hps), C.byref(ph),
                                                        0 if lookahead else _capi.PPM_SESSION_NO_LOOKAHEAD, C.byref(h)))
        ses = PpmSession(self, h, width, rows, spp)
        self._sessions.add(ses)
        return ses

    def ppm_session_wavefront(self, org, dirs, keys=None, *, width, rows, spp=1, pixel=None, eye_depth=12, min_adj=0.0, max_depth=5,
                              seed=12345, first_index=0, work_bytes=0, **photon_kw):
        """Photon mapping behind an eye pass of any depth: wavefront(max_depth=eye_depth, min_adj) traces the rays' trees (1..31
        levels) and their Hitpoint records start a ppm_session_hitpoints session whose photons run to max_depth (1..5).  The
        wavefront runs twice: once without record arrays to learn the number of Hitpoints, once with room for exactly that
        many.  pixel (int64 [n], per RAY; None: ray i belongs to texel i % (width * rows)) is mapped to the records; a ray with
        a negative texel contributes nothing.  photon_kw: ppm_session_hitpoints' photon keywords (nphotons, photon_seed, batch,
        ...).  Returns (PpmSession, wavefront's dict with hp9, hp_ray, hp_path).  At eye_depth <= 5 the session is
        ppm_session_rays' on the same rays bit for bit."""
        self._ray_tensors("ppm_session_wavefront", org, dirs, keys, pixel)
        count = self.wavefront(org, dirs, keys, max_depth=eye_depth, min_adj=min_adj, seed=seed, first_index=first_index, want=(),
                               work_bytes=work_bytes)["hp_count"]
        wf = self.wavefront(org, dirs, keys, max_depth=eye_depth, min_adj=min_adj, seed=seed, first_index=first_index, want=("hp",),
                            hp_cap=count, work_bytes=work_bytes)
        assert wf["hp_count"] == count and wf["hp9"].shape[0] == count  # the trace is deterministic
        rec_pixel = pixel[wf["hp_ray"]].contiguous() if pixel is not None else None
        ses = self.ppm_session_hitpoints(wf["hp9"], wf["hp_ray"], wf["hp_path"], rec_pixel, width=width, rows=rows, spp=spp,
                                         max_depth=max_depth, **photon_kw)
        return ses, wf

    def capture_variant(self, max_depth=5):
        """Name of the capture_rays_kernel instantiation trace_rays_hitpoints / ppm_session_rays launch (cgrt_trace_rays_variant
        with CGRT_RAYS_HITPOINTS)."""
        r = _capi.Rays(1, None, None, None, 0, 0, max_depth, _capi.RAYS_HITPOINTS)
        buf = C.create_string_buffer(160)
        check(self._L.cgrt_trace_rays_variant(self._h, C.byref(r), None, buf, len(buf)))
        return buf.value.decode()

    def photon_events(self, first, count, max_depth=5, photon_seed=777, light=(0.0, 19.999, 20.0), jitter=2.0,
                      power=700.0):
        """Verification probe: diffuse hits of photons [first, first+count): [n,10] = photon, P, n, flux in serial
        order (slot order)."""
        ph = _capi.Photons(_d3(light), jitter, power, 0.7, count, 1000001, 0, photon_seed, 0.0, 0)
        ev = np.zeros((count * 8, 9), np.float64)
        va = np.zeros(count * 8, np.uint8)
        check(self._L.cgrt_photon_events(self._h, C.byref(ph), max_depth, first, count, ev.ctypes.data, va.ctypes.data))
        idx = np.nonzero(va)[0]
        return np.concatenate([(first + idx // 8)[:, None].astype(np.float64), ev[idx]], axis=1)

    def emit_photons(self, first, count, photon_seed=777, light=(0.0, 19.999, 20.0), jitter=2.0, power=700.0, stream=None):
        """cgrt_photon_emit: the built-in emitter's photons [first, first + count) as device tensors (org [n,3], dirs [n,3],
        flux [n,3] float64; keys [n] int64 (bit pattern uint64); draws [n] int32 (bit pattern uint32)) -- what
        PpmSession.add_photon_rays takes.  Fed to a session with the same photon_seed at photons_done == first they are
        add_photons(count) bit for bit.  Asynchronous on torch's current stream (or `stream`)."""
        import torch

        dev = torch.device("cuda", self.device)
        n = int(count)
        org, dirs, flux = (torch.empty((n, 3), dtype=torch.float64, device=dev) for _ in range(3))
        keys = torch.empty((n,), dtype=torch.int64, device=dev)
        draws = torch.empty((n,), dtype=torch.int32, device=dev)
        ph = _capi.Photons(_d3(light), jitter, power, 0.7, 0, 1000001, 0, photon_seed, 0.0, 0)
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            check(self._L.cgrt_photon_emit(C.byref(ph), int(first), n, org.data_ptr(), dirs.data_ptr(), flux.data_ptr(),
                                           keys.data_ptr(), draws.data_ptr(), C.c_void_p(st)))
        return org, dirs, flux, keys, draws

    def photon_ray_events(self, org, dirs, flux, keys=None, draws=None, max_depth=5, photon_seed=777, first_index=0):
        """Verification probe (cgrt_photon_ray_events): the diffuse hits of caller-supplied photons (numpy arrays: org, dirs,
        flux [n,3]; keys uint64 [n] and draws uint32 [n] or None) as photon_events returns them: [m,10] = photon (first_index +
        position), P, n, flux in slot order."""
        org, dirs, flux = (np.ascontiguousarray(a, np.float64).reshape(-1, 3) for a in (org, dirs, flux))
        n = len(org)
        if len(dirs) != n or len(flux) != n:
            raise ValueError("photon_ray_events: org, dirs and flux differ in length")
        if keys is not None:
            keys = np.ascontiguousarray(keys, np.uint64)
        if draws is not None:
            draws = np.ascontiguousarray(draws, np.uint32)
        for name, a in (("keys", keys), ("draws", draws)):
            if a is not None and a.shape != (n,):
                raise ValueError("photon_ray_events: %s must have one entry per photon" % name)
        pr = _capi.PhotonRays(n, org.ctypes.data, dirs.ctypes.data, flux.ctypes.data, keys.ctypes.data if keys is not None else None,
                              draws.ctypes.data if draws is not None else None)
        ev = np.zeros((max(n, 1) * 8, 9), np.float64)
        va = np.zeros(max(n, 1) * 8, np.uint8)
        check(self._L.cgrt_photon_ray_events(self._h, C.byref(pr), photon_seed, int(first_index), max_depth, ev.ctypes.data,
                                             va.ctypes.data))
        idx = np.nonzero(va)[0]
        return np.concatenate([(first_index + idx // 8)[:, None].astype(np.float64), ev[idx]], axis=1)

    def surface_colors(self, obj, pts):
        """objs[obj]->getSurfaceColor(P) on the device for each row of pts [n,3] (function-level probe)."""
        pts = np.ascontiguousarray(pts, np.float64)
        out = np.zeros_like(pts)
        check(self._L.cgrt_surface_colors(self._h, self.obj_index[obj], pts.ctypes.data, len(pts), out.ctypes.data))
        return out

    def kernel_variant(self, width, height, spp=1, camera=None, max_depth=5, rows=None, stripe=None, flags=0,
                       hitpoints=False):
        """Name of the trace_grid_kernel instantiation this grid launches (what a rocprofv3 kernel trace shows).
        hitpoints: the one the Hitpoint capture launches (trace_grid_hitpoints, the eye pass of ppm_render)."""
        rows = height if rows is None else rows
        flags |= _capi.GRID_HITPOINTS if hitpoints else 0
        cc, g = self._structs(camera, width, height, rows, spp, max_depth, 0, 0, stripe, 0, None, flags)
        buf = C.create_string_buffer(160)
        check(self._L.cgrt_trace_grid_variant(self._h, C.byref(cc), C.byref(g), buf, len(buf)))
        return buf.value.decode()

    def diffuse_variant(self, width, height, spp=1, camera=None, max_depth=5, rows=None, stripe=None, flags=0):
        """Name of the terminal-diffuse kernel instantiation this grid launches beside kernel_variant's with
        flags including 128 (CGRT_GRID_DIFFUSE_TILES; sphere-only scenes in tile order: the tiles that see no mirror or glass),
        or "" when it launches none."""
        rows = height if rows is None else rows
        cc, g = self._structs(camera, width, height, rows, spp, max_depth, 0, 0, stripe, 0, None, flags)
        buf = C.create_string_buffer(160)
        check(self._L.cgrt_trace_grid_diffuse_variant(self._h, C.byref(cc), C.byref(g), buf, len(buf)))
        return buf.value.decode()

    def intersect_rays(self, obj, org, dirs, keys=None):
        org = np.ascontiguousarray(org, np.float64)
        dirs = np.ascontiguousarray(dirs, np.float64)
        n = len(org)
        hit = np.zeros(n, np.int32)
        ln = np.zeros(n, np.float64)
        nv = np.zeros((n, 3), np.float64)
        kp = None
        if keys is not None:
            keys = np.ascontiguousarray(keys, np.uint64)
            kp = keys.ctypes.data
        check(self._L.cgrt_intersect_rays(self._h, self.obj_index[obj], org.ctypes.data, dirs.ctypes.data, kp, n,
                                          hit.ctypes.data, ln.ctypes.data, nv.ctypes.data))
        return hit, ln, nv


class PpmSession:
    """Owns a cgrt_ppm_session (Scene.ppm_session).  Holds a reference to its Scene, which therefore outlives it; closing the
    Scene closes its sessions first."""

    def __init__(self, scene, h, width, rows, spp):
        self._scene = scene
        self._L = scene._L
        self._h = h
        self.width, self.rows, self.spp = width, rows, spp

    def close(self):
        if getattr(self, "_h", None):
            self._L.cgrt_ppm_session_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def add_photons(self, n):
        """Traces photons [photons_done, photons_done + n) and applies them; returns when they are applied."""
        check(self._L.cgrt_ppm_session_add_photons(self._h, int(n)))
        return self

    def add_photon_rays(self, org, dirs, flux, keys=None, draws=None):
        """cgrt_ppm_session_add_photon_rays: photons whose start the caller made (a spot, area or coloured light, several
        lights).  org, dirs, flux: contiguous float64 [n,3] tensors on the scene's device; keys int64 [n] (bit pattern uint64) and
        draws int32 [n] (bit pattern uint32) or None (the stream (photon_seed, photon index) from its start).  The photons take
        the indices [photons_done, photons_done + n) -- a photon with dirs == 0 goes nowhere and still counts -- and the gather
        divides by photons_done.  Waits for torch's current stream (the tensors' producer), returns when the photons are
        applied; Scene.emit_photons makes the built-in light's photons in this form."""
        import torch

        dev = torch.device("cuda", self._scene.device)
        for name, t in (("org", org), ("dirs", dirs), ("flux", flux)):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.dim() == 2 and t.shape[1] == 3 and
                    t.is_contiguous() and t.device == dev):
                raise ValueError("add_photon_rays: %s must be a contiguous float64 [n,3] tensor on %s" % (name, dev))
        n = org.shape[0]
        if dirs.shape[0] != n or flux.shape[0] != n:
            raise ValueError("add_photon_rays: org, dirs and flux differ in length")
        for name, t, dt in (("keys", keys, torch.int64), ("draws", draws, torch.int32)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == dt and tuple(t.shape) == (n,) and
                                      t.is_contiguous() and t.device == dev):
                raise ValueError("add_photon_rays: %s must be a contiguous %s [n] tensor on %s" % (name, dt, dev))
        if n == 0:
            return self
        pr = _capi.PhotonRays(n, org.data_ptr(), dirs.data_ptr(), flux.data_ptr(), keys.data_ptr() if keys is not None else None,
                              draws.data_ptr() if draws is not None else None)
        torch.cuda.current_stream(dev).synchronize()  # the session traces on streams of its own
        check(self._L.cgrt_ppm_session_add_photon_rays(self._h, C.byref(pr)))
        return self

    def info(self):
        inf = _capi.PpmSessionInfo()
        check(self._L.cgrt_ppm_session_get_info(self._h, C.byref(inf)))
        return {f: getattr(inf, f) for f, _ in inf._fields_}

    @property
    def photons_done(self):
        return self.info()["photons_done"]

    def image(self):
        """[rows, W, 3] float64, row 0 = bottom: ppm_render(nphotons=photons_done)["image"]."""
        img = np.zeros((self.rows, self.width, 3), np.float64)
        check(self._L.cgrt_ppm_session_image(self._h, img.ctypes.data, None))
        return img

    def rgb8(self):
        """[rows, W, 3] uint8, top row first (contiguous rows only): ppm_render(..., want_rgb8=True)["rgb8"]."""
        out = np.zeros((self.rows, self.width, 3), np.uint8)
        check(self._L.cgrt_ppm_session_image(self._h, None, out.ctypes.data))
        return out

    def image_tensor(self, out=None, rgb8_out=None, stream=None):
        """The image as a float64 [rows, W, 3] torch tensor on the scene's device, gathered on torch's current stream (or
        `stream`) without a host copy.  rgb8_out (uint8 [rows, W, 3], optional) receives the tone-mapped bytes in the same
        pass.  Returns `out`."""
        import torch

        dev = torch.device("cuda", self._scene.device)
        if out is None:
            out = torch.empty((self.rows, self.width, 3), dtype=torch.float64, device=dev)
        assert out.is_contiguous() and out.dtype == torch.float64 and tuple(out.shape) == (self.rows, self.width, 3)
        if rgb8_out is not None:
            assert rgb8_out.is_contiguous() and rgb8_out.dtype == torch.uint8 and rgb8_out.numel() == self.rows * self.width * 3
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(self._L.cgrt_ppm_session_image_device(self._h, out.data_ptr(),
                                                    rgb8_out.data_ptr() if rgb8_out is not None else None, C.c_void_p(st)))
        return out

    def hitpoints(self):
        """[n, 16] of the current state: ppm_render(want_hitpoints=True)["hp"] at photons_done photons."""
        n = self.info()["hp_count"]
        hp = np.zeros((max(n, 1), 16), np.float64)
        cnt = C.c_uint64(0)
        check(self._L.cgrt_ppm_session_hitpoints(self._h, hp.ctypes.data, n, C.byref(cnt)))
        return hp[:n]


class SppmSession:
    """Owns a cgrt_sppm_session (Scene.sppm_session).  Holds a reference to its Scene, which therefore outlives it; closing the
    Scene closes its sessions first."""

    def __init__(self, scene, h, width, rows, spp, grid):
        self._scene = scene
        self._L = scene._L
        self._h = h
        self.width, self.rows, self.spp = width, rows, spp
        self._grid = grid  # what add_passes renders with

    def close(self):
        if getattr(self, "_h", None):
            self._L.cgrt_sppm_session_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def add_passes(self, n, photons_per_pass, flags=0):
        """n passes of the session's camera, each with `photons_per_pass` fresh photons: pass k (counted over the session's
        life) traces samples k * spp .. k * spp + spp - 1 of every pixel.  flags: CGRT_GRID_* scheduling flags of the eye pass."""
        g = self._grid
        for _ in range(int(n)):
            cc, cg = self._scene._structs(g["camera"], self.width, g["height"], self.rows, self.spp, g["max_depth"], g["seed"],
                                          g["row_offset"], g["stripe"], self.info()["passes"] * self.spp, None, flags)
            check(self._L.cgrt_sppm_session_pass_grid(self._h, C.byref(cc), C.byref(cg), int(photons_per_pass)))
        return self

    def add_pass_rays(self, org, dirs, nphotons, keys=None, pixel=None, max_depth=5, seed=12345, first_index=0):
        """One pass over caller-supplied rays (cgrt_sppm_session_pass_rays): org, dirs, keys as for trace_rays; ray i gathers
        into texel pixel[i] (int64 [n] on the scene's device; negative: not traced), or i % (width * rows) without `pixel` --
        camera_rays' order.  max_depth is the eye depth.  Waits for torch's current stream, returns when the pass is applied."""
        import torch

        n = self._scene._ray_tensors("add_pass_rays", org, dirs, keys, pixel)
        r = _capi.Rays(n, org.data_ptr(), dirs.data_ptr(), keys.data_ptr() if keys is not None else None, first_index, seed,
                       max_depth, 0)
        torch.cuda.current_stream(org.device).synchronize()  # the pass runs on the null stream
        check(self._L.cgrt_sppm_session_pass_rays(self._h, C.byref(r), pixel.data_ptr() if pixel is not None else None,
                                                  int(nphotons)))
        return self

    def info(self):
        inf = _capi.SppmSessionInfo()
        check(self._L.cgrt_sppm_session_get_info(self._h, C.byref(inf)))
        return {f: getattr(inf, f) for f, _ in inf._fields_}

    @property
    def passes(self):
        return self.info()["passes"]

    @property
    def photons_done(self):
        return self.info()["photons_done"]

    def image(self):
        """[rows, W, 3] float64, row 0 = bottom: tau / (PI * R2 * photons_done * spp)."""
        img = np.zeros((self.rows, self.width, 3), np.float64)
        check(self._L.cgrt_sppm_session_image(self._h, img.ctypes.data, None))
        return img

    def rgb8(self):
        """[rows, W, 3] uint8, top row first (contiguous rows only)."""
        out = np.zeros((self.rows, self.width, 3), np.uint8)
        check(self._L.cgrt_sppm_session_image(self._h, None, out.ctypes.data))
        return out

    def image_tensor(self, out=None, rgb8_out=None, stream=None):
        """The image as a float64 [rows, W, 3] torch tensor on the scene's device, written on torch's current stream (or
        `stream`) without a host copy.  rgb8_out (uint8 [rows, W, 3], optional) receives the tone-mapped bytes in the same
        pass.  Returns `out`."""
        import torch

        dev = torch.device("cuda", self._scene.device)
        if out is None:
            out = torch.empty((self.rows, self.width, 3), dtype=torch.float64, device=dev)
        assert out.is_contiguous() and out.dtype == torch.float64 and tuple(out.shape) == (self.rows, self.width, 3)
        if rgb8_out is not None:
            assert rgb8_out.is_contiguous() and rgb8_out.dtype == torch.uint8 and rgb8_out.numel() == self.rows * self.width * 3
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(self._L.cgrt_sppm_session_image_device(self._h, out.data_ptr(),
                                                     rgb8_out.data_ptr() if rgb8_out is not None else None, C.c_void_p(st)))
        return out

    def pixels(self):
        """[rows * W, 8] float64: per texel {N, R2, tau[3], M_p of the last pass, Hitpoints of the last pass, 0}."""
        px = np.zeros((self.rows * self.width, 8), np.float64)
        check(self._L.cgrt_sppm_session_pixels(self._h, px.ctypes.data))
        return px

    def last_hitpoints(self):
        """[n, 16]: the last pass's table in PpmSession.hitpoints()' layout and order, flux = Phi_h, r2 = the radius the pass
        searched with, n = M_h."""
        n = self.info()["hp_count"]
        hp = np.zeros((max(n, 1), 16), np.float64)
        cnt = C.c_uint64(0)
        check(self._L.cgrt_sppm_session_last_hitpoints(self._h, hp.ctypes.data, n, C.byref(cnt)))
        return hp[:n]


def camera_rays_host(width, height, spp=1, camera=None, seed=12345, rows=None, row_offset=0, stripe=None, sample_offset=0):
    """cgrt_camera_rays_host: the primary rays of the eye pass evaluated on the host -- no GPU and no scene needed.
    Returns (org [n,3] float64, dirs [n,3] float64, keys [n] uint64) numpy arrays, n = spp * rows * width, ray index =
    (k * rows + local row) * width + w; the same bits Scene.camera_rays makes on the device."""
    rows = height - row_offset if rows is None else rows
    cc, posed = _ccamera(camera)
    s_rows, s_rank, s_n = stripe if stripe else (0, 0, 1)
    g = _CGrid(width, height, rows, row_offset, s_rows, s_rank, s_n, spp, sample_offset, spp, 1, posed, seed)
    n = spp * rows * width
    org = np.zeros((n, 3), np.float64)
    dirs = np.zeros((n, 3), np.float64)
    keys = np.zeros(n, np.uint64)
    check(_capi.lib().cgrt_camera_rays_host(C.byref(cc), C.byref(g), org.ctypes.data, dirs.ctypes.data, keys.ctypes.data))
    return org, dirs, keys


def emit_photons_host(first, count, photon_seed=777, light=(0.0, 19.999, 20.0), jitter=2.0, power=700.0):
    """cgrt_photon_emit_host: the built-in emitter's photons [first, first + count) evaluated on the host -- no GPU and no scene
    needed.  Returns numpy arrays (org [n,3], dirs [n,3], flux [n,3] float64, keys [n] uint64, draws [n] uint32): the same bits
    Scene.emit_photons makes on the device."""
    n = int(count)
    org, dirs, flux = (np.zeros((max(n, 0), 3), np.float64) for _ in range(3))
    keys = np.zeros(max(n, 0), np.uint64)
    draws = np.zeros(max(n, 0), np.uint32)
    ph = _capi.Photons(_d3(light), jitter, power, 0.7, 0, 1000001, 0, photon_seed, 0.0, 0)
    check(_capi.lib().cgrt_photon_emit_host(C.byref(ph), int(first), n, org.ctypes.data, dirs.ctypes.data, flux.ctypes.data,
                                            keys.ctypes.data, draws.ctypes.data))
    return org, dirs, flux, keys, draws


def render(objs, width=1024, height=768, num_of_samples=1, camera=None, max_depth=5, seed=12345, device=0):
    """Drop-in for the eye pass of render(objs) (main.cpp:169-219): returns the per-pixel accumulator
    float32 [height, width, 3] (row 0 = bottom) as a numpy array."""
    sc = Scene(objs, device)
    try:
        return sc.trace_grid_host(width, height, num_of_samples, camera, max_depth, seed)["rgb"]
    finally:
        sc.close()


def tonemap_rgb8(image, device=0):
    """gammaCorr + vertical flip (util.h:45-47, main.cpp:403-412) on the device: [H,W,3] float64, row 0 = bottom ->
    [H,W,3] uint8, top row first."""
    image = np.ascontiguousarray(image, np.float64)
    h, w = image.shape[:2]
    out = np.zeros((h, w, 3), np.uint8)
    check(_capi.lib().cgrt_tonemap_rgb8(device, image.ctypes.data, w, h, out.ctypes.data))
    return out


def math_probe(op, values, device=0):
    """cgrt_math_probe: the kernels' own inline device math on a numpy array (function-level probe).  op "sqrt": [n] -> [n];
    "normalized": [n,3] -> [n,3]; "sphere_len": [n,10] = centre, radius2, origin, direction -> [n]; "sphere_len_pair": [n,14]
    = centre A, radius2 A, centre B, radius2 B, origin, direction -> [n,2].  Elements 64k .. 64k+63 are the lanes of one wave."""
    code, cols = {"sqrt": (_capi.PROBE_SQRT, 1), "normalized": (_capi.PROBE_NORMALIZED, 3),
                  "sphere_len": (_capi.PROBE_SPHERE_LEN, 10), "sphere_len_pair": (_capi.PROBE_SPHERE_LEN_PAIR, 14)}[op]
    values = np.ascontiguousarray(values, np.float64)
    if values.shape[1:] != (() if cols == 1 else (cols,)):
        raise ValueError("math_probe(%r): expected shape [n%s], got %r" % (op, "" if cols == 1 else ",%d" % cols, values.shape))
    n = values.shape[0]
    out = np.zeros((n, 3) if cols == 3 else ((n, 2) if cols == 14 else (n,)), np.float64)
    check(_capi.lib().cgrt_math_probe(device, code, values.ctypes.data, n, out.ctypes.data))
    return out


def write_png(path, rgb8):
    """stbi_write_png's role at main.cpp:412: [H,W,3] uint8, top row first."""
    rgb8 = np.ascontiguousarray(rgb8, np.uint8)
    h, w = rgb8.shape[:2]
    check(_capi.lib().cgrt_write_png(os.fsencode(path), w, h, rgb8.ctypes.data))
