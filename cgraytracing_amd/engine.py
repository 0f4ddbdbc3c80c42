"""Host-side `render(objs)` over the C ABI: flattens a list of scene objects into a cgrt_scene handle and
launches the eye pass (the loop nest of main.cpp:185-219) on the GPU."""
from __future__ import annotations

import collections
import ctypes as C
import os
import weakref

import numpy as np

from . import _buffers, _capi
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


def _grid_flags(stats=False, split_samples=False, reorder=True, force_reorder=False, tile_order=True, diffuse_tiles=False, sphere_pairs=True,
                sphere_masks=True, sample_relay=None, relay_mirror=None, relay_order=None, lens_stage=True, sure_tiles=True, relay_start=None,
                relay_boost=None, lens_table=None, inside_trips=True):
    """The CGRT_GRID_* flags of trace_grid's scheduling switches, in the order of its signature.  The relay's: CGRT_GRID_SAMPLE_RELAY
    / _NO_SAMPLE_RELAY / _SAMPLE_RELAY_4 for sample_relay=None|True|False|2|4, CGRT_GRID_RELAY_MIRROR / _NO_MIRROR for
    relay_mirror=None|True|False, the order field for relay_order=None|a name, CGRT_GRID_RELAY_COST_START / _NO_RELAY_COST_START
    for relay_start=None|"cost"|"list" and CGRT_GRID_RELAY_BOOST / _NO_RELAY_BOOST for relay_boost=None|True|False."""
    f = ((_capi.GRID_STATS if stats else 0) | (_capi.GRID_SPLIT_SAMPLES if split_samples else 0) | (0 if reorder else _capi.GRID_NO_REORDER) |
         (_capi.GRID_FORCE_REORDER if force_reorder else 0) | (0 if tile_order else _capi.GRID_NO_TILE_ORDER) |
         (_capi.GRID_DIFFUSE_TILES if diffuse_tiles else 0) | (0 if sphere_pairs else _capi.GRID_NO_SPHERE_PAIRS) |
         (0 if sphere_masks else _capi.GRID_NO_SPHERE_MASKS) | (0 if lens_stage else _capi.GRID_NO_LENS_STAGE) |
         (0 if sure_tiles else _capi.GRID_NO_SURE_TILES) | (0 if inside_trips else _capi.GRID_NO_INSIDE_TRIPS))
    if lens_table is not None:
        f |= _capi.GRID_LENS_TABLE if lens_table else _capi.GRID_NO_LENS_TABLE
    if relay_mirror is not None:
        f |= _capi.GRID_RELAY_MIRROR if relay_mirror else _capi.GRID_RELAY_NO_MIRROR
    if relay_boost is not None:
        f |= _capi.GRID_RELAY_BOOST if relay_boost else _capi.GRID_NO_RELAY_BOOST
    if relay_start is not None:
        if relay_start not in _RELAY_STARTS:
            raise ValueError("relay_start: None, " + ", ".join(repr(o) for o in _RELAY_STARTS))
        f |= _capi.GRID_RELAY_COST_START if relay_start == "cost" else _capi.GRID_NO_RELAY_COST_START
    if relay_order is not None:
        if relay_order not in _RELAY_ORDERS:
            raise ValueError("relay_order: None, " + ", ".join(repr(o) for o in _RELAY_ORDERS))
        f |= (_capi.GRID_RELAY_CHUNKS_FIRST, _capi.GRID_RELAY_MIRROR_FIRST, _capi.GRID_RELAY_INTERLEAVED)[_RELAY_ORDERS.index(relay_order)]
    if sample_relay is None:
        return f
    if sample_relay is True or sample_relay is False:
        return f | (_capi.GRID_SAMPLE_RELAY if sample_relay else _capi.GRID_NO_SAMPLE_RELAY)
    if int(sample_relay) not in (2, 4):
        raise ValueError("sample_relay: None, True, False, 2 or 4")
    return f | _capi.GRID_SAMPLE_RELAY | (_capi.GRID_SAMPLE_RELAY_4 if int(sample_relay) == 4 else 0)


def _photons(light, jitter, power, alpha=0.7, nphotons=0, hashsize=1000001, batch=0, photon_seed=777, initial_radius=0.0, pair_cap=0):
    return _capi.Photons(_d3(light), jitter, power, alpha, nphotons, hashsize, batch, photon_seed, initial_radius, pair_cap)


def _variant_name(fn, *args):
    """The kernel instantiation's name a cgrt_*_variant entry point writes for `args`."""
    buf = C.create_string_buffer(160)
    check(fn(*args, buf, len(buf)))
    return buf.value.decode()


def _hitpoint_records(rec, count, cap):
    """10-column Hitpoint records: (hp [m,9], label >> 4, label & 15) of the m = min(count, cap) that were written."""
    m = min(int(count), cap)
    lab = rec[:m, 9].astype(np.int64)
    return rec[:m, :9].copy(), lab >> 4, lab & 15


def _photon_event_rows(first, ev, va):
    """A photon-event probe's answer: the valid slots' [photon, P, n, flux] rows in slot order, 8 slots a photon from `first`."""
    idx = np.nonzero(va)[0]
    return np.concatenate([(first + idx // 8)[:, None].astype(np.float64), ev[idx]], axis=1)


# ---- caller-supplied rays: one table per query, from which its torch form and its numpy form are both made ----
# spec: result -> (rows, cols, (torch, numpy) dtype, numpy fill), see _buffers; want: what `want` may name, groups: the names that
# stand for several results; host_counts: what the numpy form adds from its counters; skip_empty: whether the (torch, numpy)
# form returns before the library call when there are no rays; coerce: whether the numpy form makes its inputs fit or refuses.
_Query = collections.namedtuple("_Query", "fn spec want groups host_counts skip_empty coerce empty_want inputs",
                                defaults=({}, (), (True, False), True, False, None))
_F64, _I32, _I64, _U8, _U32, _U64 = _buffers.F64, _buffers.I32, _buffers.I64, _buffers.U8, _buffers.U32, _buffers.U64
_N3, _2N3 = ("n", 3, _F64, 0), ("2n", 3, _F64, 0)
_TRACE_RAYS = _Query("cgrt_trace_rays", dict(acc=_N3, nhit=("n", None, _U32, 0), hit_obj=("n", None, _I32, 0), hit_t=("n", None, _F64, 0),
                                             hit_normal=_N3),
                     ("acc", "nhit", "hit"), {"hit": ("hit_obj", "hit_t", "hit_normal")}, ("nrays", "nhp"))
_HIT_ATTRIBUTES = _Query("cgrt_ray_hit_attributes", dict(prim=("n", None, _I32, -1), uv=("n", 2, _F64, 0), color=_N3, material=("n", 2, _F64, 0)),
                         ("prim", "uv", "color", "material"), skip_empty=(True, True), coerce=False)
_OCCLUDED = _Query("cgrt_occlusion_rays", dict(occluded=(("n", "max(n,1)"), None, _U8, 0)), (), host_counts=("nrays",))
_BOUNCE = _Query("cgrt_bounce_rays", dict(step=("n", None, _U8, 0), hit_obj=("n", None, _I32, -1), hit_t=("n", None, _F64, 0), pos=_N3, normal=_N3,
                                          value=_N3, child_org=_2N3, child_dir=_2N3, child_adj=_2N3, child_path=("2n", None, _U32, 0),
                                          child_keys=("2n", None, _U64, 0)),
                 ("step", "hit_obj", "hit_t", "pos", "normal", "value", "child_org", "child_dir", "child_adj", "child_path", "child_keys", "hit",
                  "children"),
                 {"hit": ("hit_obj", "hit_t"), "children": ("child_org", "child_dir", "child_adj", "child_path", "child_keys")}, ("nrays", "nhp"),
                 inputs=(("keys", "adj", "path"), ("adj", "path", "keys")))  # the order the (torch, numpy) form checks them in
_WAVEFRONT = _Query("cgrt_wavefront_rays", dict(acc=_N3, nhit=("n", None, _U32, 0), hp9=("cap", 9, _F64, 0), hp_ray=("cap", None, _I64, 0),
                                                hp_path=("cap", None, _U32, 0)),
                    ("acc", "nhit", "hp"), {"hp": ("hp9", "hp_ray", "hp_path")}, ("nrays", "nhp"), skip_empty=(False, False), empty_want=True)
_CAMERA_RAYS = dict(org=_N3, dirs=_N3, keys=("n", None, _U64, 0))
_PHOTON_RAYS = dict(org=_N3, dirs=_N3, flux=_N3, keys=("n", None, _U64, 0), draws=("n", None, _U32, 0))
_INPUT = dict(keys=(_U64, None), adj=(_F64, 3), path=(_U32, None))  # bounce's optional per-ray inputs -> (dtype, cols)
_HOST_COUNTS = dict(nrays=_capi.CNT_RAYS, nhp=_capi.CNT_HITPOINTS)


def _want(what, q, want):
    """The results `want` asks of the query q, in the table's order."""
    want = tuple(want)
    if (not want and not q.empty_want) or any(w not in q.want for w in want):
        raise ValueError("%s: want is a %ssubset of %r" % (what, "" if q.empty_want else "non-empty ", q.want))
    names = [k for w in want for k in q.groups.get(w, (w,))]
    return [k for k in q.spec if k in names]


def _with_counters(A, q, res, cnt):
    """The result dict with its counters, and in the numpy form what is read out of them."""
    res["counters"] = cnt
    if A.host:
        res.update({k: int(cnt[_HOST_COUNTS[k]]) for k in q.host_counts})
    return res


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


class _Closing:
    """An owner of a library handle: close() also ends a `with` block and comes with collection."""

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


class Scene(_Closing):
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
                              _grid_flags(stats, split_samples, reorder, force_reorder, tile_order, diffuse_tiles, sphere_pairs, sphere_masks,
                                          sample_relay, relay_mirror, relay_order, lens_stage, sure_tiles, relay_start, relay_boost, lens_table,
                                          inside_trips))
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        check(self._L.cgrt_trace_grid(self._h, C.byref(cc), C.byref(g), out.data_ptr(),
                                      nhit.data_ptr() if nhit is not None else None,
                                      counters.data_ptr(), C.c_void_p(st)))
        return out, nhit, counters

    # ---- caller-supplied rays ----
    def _torch(self):
        return _buffers.Torch(self.device)

    def _rays(self, A, n, org, dirs, keys, first_index, seed, max_depth, flags):
        return _capi.Rays(n, A.ptr(org), A.ptr(dirs), A.ptr(keys), first_index, seed, max_depth, flags)

    def _query(self, A, q, n, stream, *args):
        """The library call of query q in A's form -- unless there are no rays and that form then goes without the call."""
        if n > 0 or not q.skip_empty[A.form]:
            check(getattr(self._L, q.fn + A.suffix)(self._h, *args, *A.stream(stream)))

    def _ray_tensors(self, what, org, dirs, keys, pixel=None):
        """The argument checks of trace_rays for the ray-buffer calls; returns n."""
        A = self._torch()
        n = A.rays(what, org=org, dirs=dirs)[0]
        A.per_ray(what, "keys", keys, n, _I64)
        A.per_ray(what, "pixel", pixel, n, _I64)
        return n

    def _unless_committed(self, call):
        """An uncommitted scene gets the library's own answer from the empty call `call`, before any tensor is looked at."""
        if not self.stats()["committed"]:
            check(call())

    def _open_session(self, cls, h, *args):
        ses = cls(self, h, *args)
        self._sessions.add(ses)
        return ses

    def camera_rays(self, width, height, spp=1, camera=None, seed=12345, rows=None, row_offset=0, stripe=None,
                    sample_offset=0, stream=None):
        """The primary rays trace_grid starts for samples sample_offset .. sample_offset + spp - 1 of the grid's rows
        (cgrt_camera_rays), made on the device: (org [n,3] float64, dirs [n,3] float64, keys [n] int64 (bit pattern uint64))
        torch tensors, n = spp * rows * width, ray index = (k * rows + local row) * width + w.  Rows beyond `height` of a
        striped grid have dirs = 0 and are not traced by trace_rays."""
        A = self._torch()
        rows = height - row_offset if rows is None else rows
        org, dirs, keys = A.results("camera_rays", _CAMERA_RAYS, _CAMERA_RAYS, None, spp * rows * width).values()
        cc, g = self._structs(camera, width, height, rows, spp, 1, seed, row_offset, stripe, sample_offset, None, 0)
        st = A.stream(stream)
        with A.torch.cuda.device(A.dev):
            check(self._L.cgrt_camera_rays(C.byref(cc), C.byref(g), org.data_ptr(), dirs.data_ptr(), keys.data_ptr(), *st))
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
        return self._trace_rays(self._torch(), "trace_rays", org, dirs, keys, max_depth, seed, first_index, want, counters, stream, stats, out,
                                sign_pass)

    def _trace_rays(self, A, what, org, dirs, keys, max_depth, seed, first_index, want, counters, stream, stats, out, sign_pass):
        q = _TRACE_RAYS
        n, org, dirs = A.rays(what, org=org, dirs=dirs)
        keys = A.per_ray(what, "keys", keys, n, _U64)
        res = A.results(what, q.spec, _want(what, q, want), out, n)
        cnt = A.counters(what, counters)
        r = self._rays(A, n, org, dirs, keys, first_index, seed, max_depth,
                       (_capi.RAYS_STATS if stats else 0) | (0 if sign_pass else _capi.RAYS_NO_SIGN_PASS))
        o = _capi.RayResults(*[A.ptr(res.get(k)) for k in q.spec])
        self._query(A, q, n, stream, C.byref(r), C.byref(o), A.ptr(cnt))
        return _with_counters(A, q, res, cnt)

    def trace_rays_host(self, org, dirs, keys=None, max_depth=5, seed=12345, first_index=0, want=("acc", "nhit", "hit"),
                        stats=False, sign_pass=True):
        """Synchronous form of trace_rays on numpy arrays (no torch needed): dict(acc, nhit (uint32), hit_obj, hit_t,
        hit_normal -- those in `want` --, counters (uint64 [8]), nrays, nhp)."""
        return self._trace_rays(_buffers.NUMPY, "trace_rays_host", org, dirs, keys, max_depth, seed, first_index, want, None, None, stats, None,
                                sign_pass)

    # ---- hit attributes of caller-supplied rays ----
    def hit_attributes(self, org, dirs, hit_obj, hit_t, want=("prim", "uv", "color", "material"), out=None, stream=None):
        """cgrt_ray_hit_attributes on torch tensors: org, dirs float64 [n,3], hit_obj int32 [n] and hit_t float64 [n] -- the
        last two as trace_rays(want=("hit",)) wrote them for the same rays --, all contiguous on the scene's device.  want:
        which attributes -- "prim" (int32 [n]: the triangle's index in its mesh's or bump floor's construction order, -1 where
        the hit is no triangle), "uv" (float64 [n,2]: the hit point is (1-u-v)*pa + u*pb + v*pc), "color" (float64 [n,3]:
        getSurfaceColor at the hit) and "material" (float64 [n,2]: reflection, transparency).  out: dict of preallocated
        result tensors to write into.  Asynchronous on torch's current stream (or `stream`).  Returns a dict of the tensors."""
        return self._hit_attributes(self._torch(), "hit_attributes", org, dirs, hit_obj, hit_t, want, out, stream)

    def _hit_attributes(self, A, what, org, dirs, hit_obj, hit_t, want, out, stream):
        q = _HIT_ATTRIBUTES
        n, org, dirs = A.rays(what, coerce=q.coerce, org=org, dirs=dirs)
        hit_obj = A.per_ray(what, "hit_obj", hit_obj, n, ("torch.int32", "int32"), required=True, coerce=q.coerce)
        hit_t = A.per_ray(what, "hit_t", hit_t, n, ("torch.float64", "float64"), required=True, coerce=q.coerce)
        res = A.results(what, q.spec, _want(what, q, want), out, n)
        r = self._rays(A, n, org, dirs, None, 0, 0, 1, 0)
        o = _capi.HitAttributes(*[A.ptr(res.get(k)) for k in q.spec])
        self._query(A, q, n, stream, C.byref(r), A.ptr(hit_obj), A.ptr(hit_t), C.byref(o))
        return res

    def hit_attributes_host(self, org, dirs, hit_obj, hit_t, want=("prim", "uv", "color", "material")):
        """Synchronous form of hit_attributes on numpy arrays (no torch needed): dict of the arrays in `want`."""
        return self._hit_attributes(_buffers.NUMPY, "hit_attributes_host", org, dirs, hit_obj, hit_t, want, None, None)

    # ---- occlusion queries of caller-supplied rays ----
    def occluded(self, org, dirs, tmax=None, keys=None, seed=12345, first_index=0, skip_transparent=False, stats=False, out=None,
                 stream=None):
        """cgrt_occlusion_rays on torch tensors: org, dirs float64 [n,3] contiguous on the scene's device, tmax float64 [n] or
        None (no limit), keys int64 [n] or None.  occluded[i] = 1 exactly when some object's intersect() length is < tmax[i]
        -- hit_obj >= 0 and hit_t < tmax of trace_rays(want=("hit",)) on the same rays --, else 0; a NaN tmax, a tmax <= 0
        (unless an object returns a length below zero: a ray starting on a sphere's surface) and a dirs row of zeros give 0.  skip_transparent: objects with transparency >= 1e-4 are no occluders (shadow rays through
        glass).  out: a preallocated uint8 [n] tensor, or a dict holding one as "occluded".  Asynchronous on torch's current
        stream (or `stream`).  Returns {"occluded": uint8 [n], "counters": int64 [8]}."""
        return self._occluded(self._torch(), "occluded", org, dirs, tmax, keys, seed, first_index, skip_transparent, stats,
                              out.get("occluded") if isinstance(out, dict) else out, stream)

    def _occluded(self, A, what, org, dirs, tmax, keys, seed, first_index, skip_transparent, stats, occ, stream):
        q = _OCCLUDED
        n, org, dirs = A.rays(what, org=org, dirs=dirs)
        tmax = A.per_ray(what, "tmax", tmax, n, _F64)
        keys = A.per_ray(what, "keys", keys, n, _U64)
        occ = A.per_ray(what, "out", occ, n, _U8)
        if occ is None:
            occ = A.results(what, q.spec, q.spec, None, n)["occluded"]
        cnt = A.counters(what)
        res = {"occluded": occ if len(occ) == n else occ[:n]}  # (the numpy form's array is never empty)
        r = self._rays(A, n, org, dirs, keys, first_index, seed, 1,
                       (_capi.RAYS_STATS if stats else 0) | (_capi.RAYS_SKIP_TRANSPARENT if skip_transparent else 0))
        o = _capi.Occlusion(A.ptr(tmax), A.ptr(occ))
        self._query(A, q, n, stream, C.byref(r), C.byref(o), A.ptr(cnt))
        return _with_counters(A, q, res, cnt)

    def occluded_host(self, org, dirs, tmax=None, keys=None, seed=12345, first_index=0, skip_transparent=False, stats=False):
        """Synchronous form of occluded on numpy arrays (no torch needed): dict(occluded (uint8 [n]), counters (uint64 [8]),
        nrays)."""
        return self._occluded(_buffers.NUMPY, "occluded_host", org, dirs, tmax, keys, seed, first_index, skip_transparent, stats, None, None)

    def occlusion_variant(self, stats=False):
        """Name of the occlusion_rays_kernel instantiation occluded launches on this scene (cgrt_occlusion_rays_variant)."""
        return self._rays_variant_name(self._L.cgrt_occlusion_rays_variant, stats)

    def _rays_variant_name(self, fn, stats, max_depth=1, *results, flags=0):
        r = _capi.Rays(1, None, None, None, 0, 0, max_depth, flags | (_capi.RAYS_STATS if stats else 0))
        return _variant_name(fn, self._h, C.byref(r), *results)

    # ---- bounce queries of caller-supplied rays: one step of trace() ----
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
        return self._bounce(self._torch(), "bounce", org, dirs, adj, path, keys, seed, first_index, want, stats, out, stream, counters)

    def _bounce(self, A, what, org, dirs, adj, path, keys, seed, first_index, want, stats, out, stream, counters):
        q = _BOUNCE
        n, org, dirs = A.rays(what, org=org, dirs=dirs)
        given = dict(adj=adj, path=path, keys=keys)
        for name in q.inputs[A.form]:
            given[name] = A.per_ray(what, name, given[name], n, *_INPUT[name])
        res = A.results(what, q.spec, _want(what, q, want), out, n)
        cnt = A.counters(what, counters)
        r = self._rays(A, n, org, dirs, given["keys"], first_index, seed, 1, _capi.RAYS_STATS if stats else 0)
        b = _capi.Bounce(A.ptr(given["adj"]), A.ptr(given["path"]), *[A.ptr(res.get(k)) for k in q.spec])
        self._query(A, q, n, stream, C.byref(r), C.byref(b), A.ptr(cnt))
        return _with_counters(A, q, res, cnt)

    def bounce_host(self, org, dirs, adj=None, path=None, keys=None, seed=12345, first_index=0,
                    want=("step", "hit", "pos", "normal", "value", "children"), stats=False):
        """Synchronous form of bounce on numpy arrays (no torch needed): dict of the arrays in `want` (child_path uint32,
        child_keys uint64), counters (uint64 [8]), nrays, nhp."""
        return self._bounce(_buffers.NUMPY, "bounce_host", org, dirs, adj, path, keys, seed, first_index, want, stats, None, None, None)

    def bounce_variant(self, stats=False):
        """Name of the bounce_rays_kernel instantiation bounce launches on this scene (cgrt_bounce_rays_variant)."""
        return self._rays_variant_name(self._L.cgrt_bounce_rays_variant, stats)

    # ---- wavefront trace of caller-supplied rays: any depth, the depth loop inside the library ----
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
        return self._wavefront(self._torch(), "wavefront", org, dirs, keys, max_depth, min_adj, seed, first_index, want, hp_cap, work_bytes,
                               stats, out, stream, counters)

    def _wavefront(self, A, what, org, dirs, keys, max_depth, min_adj, seed, first_index, want, hp_cap, work_bytes, stats, out, stream,
                   counters):
        q = _WAVEFRONT
        n, org, dirs = A.rays(what, org=org, dirs=dirs)
        keys = A.per_ray(what, "keys", keys, n, _U64)
        names = _want(what, q, want)
        if not (isinstance(max_depth, int) and 1 <= max_depth <= _capi.WAVEFRONT_MAX_DEPTH):
            raise ValueError("%s: max_depth must be 1..%d" % (what, _capi.WAVEFRONT_MAX_DEPTH))
        if not (min_adj >= 0.0) or work_bytes < 0 or (hp_cap is not None and hp_cap < 0):
            raise ValueError("%s: min_adj, work_bytes and hp_cap must be >= 0" % what)
        hp = [k for k in names if k in q.groups["hp"]]
        cap = int(hp_cap if hp_cap is not None else 4 * n) if hp else 0
        res = A.results(what, q.spec, [k for k in names if cap > 0 or k not in hp], out, n, cap)
        cnt = A.counters(what, counters)
        ptr = lambda k: A.ptr(res[k]) if k in res and len(res[k]) else None
        r = self._rays(A, n, org, dirs, keys, first_index, seed, 1, _capi.RAYS_STATS if stats else 0)
        w = _capi.Wavefront(max_depth, 0, float(min_adj), int(work_bytes), *[ptr(k) for k in q.spec], cap)
        count = C.c_uint64(0)
        self._query(A, q, n, stream, C.byref(r), C.byref(w), A.ptr(cnt), C.byref(count))
        if cap > 0:
            res.update({k: res[k][:min(int(count.value), cap)] for k in hp})
        else:
            res.update(A.results(what, q.spec, hp, None, n))
        res["hp_count"] = int(count.value)
        res.update(self.last_wavefront() if n > 0 else dict(slices=0, halvings=0, levels=0, rays_per_level=[]))
        return _with_counters(A, q, res, cnt)

    def wavefront_host(self, org, dirs, keys=None, max_depth=8, min_adj=0.0, seed=12345, first_index=0, want=("acc", "nhit"),
                       hp_cap=None, work_bytes=0, stats=False):
        """Synchronous form of wavefront on numpy arrays (no torch needed): dict of acc, nhit (uint32), hp9, hp_ray, hp_path
        (uint32) -- those in `want` --, counters (uint64 [8]), nrays, nhp, hp_count and last_wavefront()'s entries."""
        return self._wavefront(_buffers.NUMPY, "wavefront_host", org, dirs, keys, max_depth, min_adj, seed, first_index, want, hp_cap,
                               work_bytes, stats, None, None, None)

    def wavefront_variant(self, stats=False):
        """Name of the wavefront_step_kernel instantiation wavefront launches on this scene (cgrt_wavefront_rays_variant)."""
        return self._rays_variant_name(self._L.cgrt_wavefront_rays_variant, stats)

    def rays_variant(self, max_depth=5, want=("acc", "nhit", "hit"), stats=False):
        """Name of the trace_rays_kernel instantiation trace_rays launches for these arguments (cgrt_trace_rays_variant)."""
        full = 1 if ("acc" in want or "nhit" in want) else None
        o = _capi.RayResults(full, None, 1 if "hit" in want else None, None, None)
        return self._rays_variant_name(self._L.cgrt_trace_rays_variant, stats, max_depth, C.byref(o))

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
                              _grid_flags(stats, split_samples, reorder, force_reorder, tile_order, diffuse_tiles, sphere_pairs, sphere_masks,
                                          sample_relay, relay_mirror, relay_order, lens_stage, sure_tiles, relay_start, relay_boost, lens_table,
                                          inside_trips))
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

    def last_eye_launches(self):
        """The eye kernels this scene's last eye pass launched (cgrt_scene_last_eye_launches; host state, no synchronisation), in
        launch order, probes included: a list of tuples (kind, TREES, BEZ, DOF, GLASS, SPH, STATS, HPS, NT, SPILL, HFONLY, DIFF,
        PAIR, START, LTAB, POSE); kind 0 trace_grid_kernel, 1 trace_grid_sched_kernel, 2 primary_walk_kernel (DOF only)."""
        n = C.c_int64()
        rows = np.zeros((16, 16), np.int32)
        check(self._L.cgrt_scene_last_eye_launches(self._h, rows.ctypes.data, rows.shape[0], C.byref(n)))
        return [tuple(int(v) for v in rows[i]) for i in range(n.value)]

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
        hp, lab, seq = _hitpoint_records(rec, n.value, cap)
        return dict(hp=hp, pix=lab % (rows * width), smp=lab // (rows * width), seq=seq, count=int(n.value))

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
        ph = _photons(light, jitter, power, alpha, nphotons, hashsize, batch, photon_seed, initial_radius, pair_cap)
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
        ph = _photons(light, jitter, power, alpha, nphotons, hashsize, batch, photon_seed, initial_radius, pair_cap)
        h = C.c_void_p()
        check(self._L.cgrt_ppm_session_create(self._h, C.byref(cc), C.byref(g), C.byref(ph),
                                              0 if lookahead else _capi.PPM_SESSION_NO_LOOKAHEAD, C.byref(h)))
        return self._open_session(PpmSession, h, width, rows, spp)

    def sppm_session(self, width, height, spp=1, camera=None, photon_depth=5, max_depth=5, seed=12345, photon_seed=777,
                     hashsize=1000001, light=(0.0, 19.999, 20.0), jitter=2.0, power=700.0, alpha=0.7, batch=0, rows=None,
                     row_offset=0, stripe=None, initial_radius=0.0, pair_cap=0):
        """Stochastic progressive photon mapping (cgrt_sppm_session): N, R2 and tau belong to the texel, every pass traces
        fresh eye samples and fresh photons, memory does not grow with the passes.  Returns an SppmSession without a pass;
        add_passes(n, photons_per_pass) renders with `camera` (kept here; max_depth is the eye depth, seed the lens streams')
        at sample_offset = passes * spp, add_pass_rays with the caller's rays.  rows / row_offset / stripe: this rank's share
        of a width x height frame as in ppm_session (every rank traces all photons)."""
        rows = height if rows is None else rows
        ph = _photons(light, jitter, power, alpha, 0, hashsize, batch, photon_seed, initial_radius, pair_cap)
        h = C.c_void_p()
        check(self._L.cgrt_sppm_session_create(self._h, width, rows, spp, photon_depth, C.byref(ph), 0, C.byref(h)))
        return self._open_session(SppmSession, h, width, rows, spp, dict(camera=camera, height=height, max_depth=max_depth, seed=seed,
                                                                         row_offset=row_offset, stripe=stripe))

    def trace_rays_hitpoints(self, org, dirs, keys=None, max_depth=5, seed=12345, first_index=0, cap=None):
        """cgrt_trace_rays_hitpoints: the Hitpoints of the rays' trees (torch tensors as for trace_rays), unordered:
        dict(hp [m,9] = f, pos, normal (after the flip of main.cpp:73-76); ray [m]; seq [m] (position in the ray tree's
        emission order); count (Hitpoints produced; m = min(count, cap))).  Synchronous."""
        self._unless_committed(lambda: self._L.cgrt_trace_rays_hitpoints(
            self._h, C.byref(_capi.Rays(0, None, None, None, 0, 0, max_depth, 0)), None, 0, C.byref(C.c_uint64(0))))
        n = self._ray_tensors("trace_rays_hitpoints", org, dirs, keys)
        cap = int(cap if cap is not None else n * 16)
        rec = np.zeros((max(cap, 1), 10), np.float64)
        cnt = C.c_uint64(0)
        r = self._rays(self._torch(), n, org, dirs, keys, first_index, seed, max_depth, 0)
        check(self._L.cgrt_trace_rays_hitpoints(self._h, C.byref(r), rec.ctypes.data, cap, C.byref(cnt)))
        hp, ray, seq = _hitpoint_records(rec, cnt.value, cap)
        return dict(hp=hp, ray=ray, seq=seq, count=int(cnt.value))

    def ppm_session_rays(self, org, dirs, keys=None, *, width, rows, spp=1, pixel=None, max_depth=5, seed=12345, first_index=0,
                         nphotons=0, photon_seed=777, hashsize=1000001, light=(0.0, 19.999, 20.0), jitter=2.0, power=700.0,
                         alpha=0.7, batch=0, initial_radius=0.0, pair_cap=0, lookahead=True):
        """A live photon-mapping render over caller-supplied rays (cgrt_ppm_session_create_rays): org, dirs, keys as for
        trace_rays; the session gathers into a [rows, width, 3] image, ray i into texel pixel[i] (int64 [n] on the scene's
        device; negative: the ray is not traced), or i % (width * rows) without `pixel` -- camera_rays' order.  spp is the
        gather's normaliser (rays per texel).  Returns a PpmSession; its hitpoints()[:, 0] is the ray index.  For
        camera_rays(width, rows, spp, ...) without `pixel` the session equals ppm_session on that grid bit for bit."""
        self._unless_committed(lambda: self._L.cgrt_ppm_session_create_rays(
            self._h, C.byref(_capi.Rays(0, None, None, None, 0, 0, max_depth, 0)), C.byref(_capi.RayPixels(width, rows, spp, 0, None)),
            C.byref(_photons(light, jitter, power, alpha, 0, hashsize, batch, photon_seed, initial_radius, pair_cap)), 0,
            C.byref(C.c_void_p())))
        n = self._ray_tensors("ppm_session_rays", org, dirs, keys, pixel)
        A = self._torch()
        r = self._rays(A, n, org, dirs, keys, first_index, seed, max_depth, 0)
        px = _capi.RayPixels(width, rows, spp, 0, A.ptr(pixel))
        ph = _photons(light, jitter, power, alpha, nphotons, hashsize, batch, photon_seed, initial_radius, pair_cap)
        h = C.c_void_p()
        A.torch.cuda.current_stream(org.device).synchronize()  # the session's eye stage runs on the null stream
        check(self._L.cgrt_ppm_session_create_rays(self._h, C.byref(r), C.byref(px), C.byref(ph),
                                                   0 if lookahead else _capi.PPM_SESSION_NO_LOOKAHEAD, C.byref(h)))
        return self._open_session(PpmSession, h, width, rows, spp)

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
        what = "ppm_session_hitpoints"
        ph = _photons(light, jitter, power, alpha, nphotons, hashsize, batch, photon_seed, initial_radius, pair_cap)
        self._unless_committed(lambda: self._L.cgrt_ppm_session_create_hitpoints(
            self._h, C.byref(_capi.Hitpoints(0, None, None, None, None, width, rows, spp, max_depth)), C.byref(ph), 0, C.byref(C.c_void_p())))
        A = self._torch()
        A.per_ray(what, "hp9", hp9, None, _F64, 9, required=True)
        n = hp9.shape[0]
        A.per_ray(what, "ray", ray, n, ("torch.int64",))
        A.per_ray(what, "path", path, n, (("torch.int32", "torch.uint32"),))
        A.per_ray(what, "pixel", pixel, n, ("torch.int64",))
        ptr = lambda t: A.ptr(t) if n > 0 else None
        hps = _capi.Hitpoints(n, ptr(hp9), ptr(ray), ptr(path), ptr(pixel), width, rows, spp, max_depth)
        h = C.c_void_p()
        A.torch.cuda.current_stream(A.dev).synchronize()  # the table build runs on the null stream
        check(self._L.cgrt_ppm_session_create_hitpoints(self._h, C.byref(hps), C.byref(ph),
                                                        0 if lookahead else _capi.PPM_SESSION_NO_LOOKAHEAD, C.byref(h)))
        return self._open_session(PpmSession, h, width, rows, spp)

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
        return self._rays_variant_name(self._L.cgrt_trace_rays_variant, False, max_depth, None, flags=_capi.RAYS_HITPOINTS)

    def photon_events(self, first, count, max_depth=5, photon_seed=777, light=(0.0, 19.999, 20.0), jitter=2.0,
                      power=700.0):
        """Verification probe: diffuse hits of photons [first, first+count): [n,10] = photon, P, n, flux in serial
        order (slot order)."""
        ph = _photons(light, jitter, power, nphotons=count, photon_seed=photon_seed)
        ev = np.zeros((count * 8, 9), np.float64)
        va = np.zeros(count * 8, np.uint8)
        check(self._L.cgrt_photon_events(self._h, C.byref(ph), max_depth, first, count, ev.ctypes.data, va.ctypes.data))
        return _photon_event_rows(first, ev, va)

    def emit_photons(self, first, count, photon_seed=777, light=(0.0, 19.999, 20.0), jitter=2.0, power=700.0, stream=None):
        """cgrt_photon_emit: the built-in emitter's photons [first, first + count) as device tensors (org [n,3], dirs [n,3],
        flux [n,3] float64; keys [n] int64 (bit pattern uint64); draws [n] int32 (bit pattern uint32)) -- what
        PpmSession.add_photon_rays takes.  Fed to a session with the same photon_seed at photons_done == first they are
        add_photons(count) bit for bit.  Asynchronous on torch's current stream (or `stream`)."""
        A = self._torch()
        with A.torch.cuda.device(A.dev):
            return _emit_photons(A, self._L.cgrt_photon_emit, first, int(count), int(count), photon_seed, light, jitter, power, stream)

    def photon_ray_events(self, org, dirs, flux, keys=None, draws=None, max_depth=5, photon_seed=777, first_index=0):
        """Verification probe (cgrt_photon_ray_events): the diffuse hits of caller-supplied photons (numpy arrays: org, dirs,
        flux [n,3]; keys uint64 [n] and draws uint32 [n] or None) as photon_events returns them: [m,10] = photon (first_index +
        position), P, n, flux in slot order."""
        pr = _photon_rays(_buffers.NUMPY, "photon_ray_events", org, dirs, flux, keys, draws, _U64, _U32)
        ev = np.zeros((max(pr.n, 1) * 8, 9), np.float64)
        va = np.zeros(max(pr.n, 1) * 8, np.uint8)
        check(self._L.cgrt_photon_ray_events(self._h, C.byref(pr), photon_seed, int(first_index), max_depth, ev.ctypes.data,
                                             va.ctypes.data))
        return _photon_event_rows(first_index, ev, va)

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
        return _variant_name(self._L.cgrt_trace_grid_variant, self._h, C.byref(cc), C.byref(g))

    def diffuse_variant(self, width, height, spp=1, camera=None, max_depth=5, rows=None, stripe=None, flags=0):
        """Name of the terminal-diffuse kernel instantiation this grid launches beside kernel_variant's with
        flags including 128 (CGRT_GRID_DIFFUSE_TILES; sphere-only scenes in tile order: the tiles that see no mirror or glass),
        or "" when it launches none."""
        rows = height if rows is None else rows
        cc, g = self._structs(camera, width, height, rows, spp, max_depth, 0, 0, stripe, 0, None, flags)
        return _variant_name(self._L.cgrt_trace_grid_diffuse_variant, self._h, C.byref(cc), C.byref(g))

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


def _photon_rays(A, what, org, dirs, flux, keys, draws, keys_dtype, draws_dtype):
    """The cgrt_photon_rays of a caller's photons, checked (or coerced) by the adapter A."""
    n, org, dirs, flux = A.rays(what, org=org, dirs=dirs, flux=flux)
    keys = A.per_ray(what, "keys", keys, n, keys_dtype, per="photon")
    draws = A.per_ray(what, "draws", draws, n, draws_dtype, per="photon")
    pr = _capi.PhotonRays(n, A.ptr(org), A.ptr(dirs), A.ptr(flux), A.ptr(keys), A.ptr(draws))
    pr.buffers = org, dirs, flux, keys, draws  # coerced copies live as long as the struct that points into them
    return pr


def _emit_photons(A, fn, first, n, rows, photon_seed, light, jitter, power, stream=None):
    """The built-in emitter's photons [first, first + n) written by `fn` into buffers of `rows` rows that A makes."""
    res = A.results("emit_photons", _PHOTON_RAYS, _PHOTON_RAYS, None, rows)
    ph = _photons(light, jitter, power, photon_seed=photon_seed)
    check(fn(C.byref(ph), int(first), n, *[A.ptr(x) for x in res.values()], *A.stream(stream)))
    return tuple(res.values())


class _Session(_Closing):
    """Owns a session handle of the library.  Holds a reference to its Scene, which therefore outlives it; closing the Scene
    closes its sessions first.  A subclass names the C prefix of its entry points, its info struct and its Hitpoint getter."""
    _PREFIX = _INFO = _HITPOINTS = None

    def __init__(self, scene, h, width, rows, spp):
        self._scene = scene
        self._L = scene._L
        self._h = h
        self.width, self.rows, self.spp = width, rows, spp

    def _fn(self, name):
        return getattr(self._L, self._PREFIX + name)

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    def info(self):
        inf = self._INFO()
        check(self._fn("get_info")(self._h, C.byref(inf)))
        return {f: getattr(inf, f) for f, _ in inf._fields_}

    @property
    def photons_done(self):
        return self.info()["photons_done"]

    def image(self):
        """[rows, W, 3] float64, row 0 = bottom: ppm_render(nphotons=photons_done)["image"] of a PpmSession,
        tau / (PI * R2 * photons_done * spp) of an SppmSession."""
        img = np.zeros((self.rows, self.width, 3), np.float64)
        check(self._fn("image")(self._h, img.ctypes.data, None))
        return img

    def rgb8(self):
        """[rows, W, 3] uint8, top row first (contiguous rows only): ppm_render(..., want_rgb8=True)["rgb8"]."""
        out = np.zeros((self.rows, self.width, 3), np.uint8)
        check(self._fn("image")(self._h, None, out.ctypes.data))
        return out

    def image_tensor(self, out=None, rgb8_out=None, stream=None):
        """The image as a float64 [rows, W, 3] torch tensor on the scene's device, gathered on torch's current stream (or
        `stream`) without a host copy.  rgb8_out (uint8 [rows, W, 3], optional) receives the tone-mapped bytes in the same
        pass.  Returns `out`."""
        A = self._scene._torch()
        torch = A.torch
        if out is None:
            out = torch.empty((self.rows, self.width, 3), dtype=torch.float64, device=A.dev)
        assert out.is_contiguous() and out.dtype == torch.float64 and tuple(out.shape) == (self.rows, self.width, 3)
        if rgb8_out is not None:
            assert rgb8_out.is_contiguous() and rgb8_out.dtype == torch.uint8 and rgb8_out.numel() == self.rows * self.width * 3
        check(self._fn("image_device")(self._h, out.data_ptr(), A.ptr(rgb8_out), *A.stream(stream)))
        return out

    def _hitpoint_dump(self):
        """[n, 16] float64: the records of the session's Hitpoint table."""
        n = self.info()["hp_count"]
        hp = np.zeros((max(n, 1), 16), np.float64)
        check(self._fn(self._HITPOINTS)(self._h, hp.ctypes.data, n, C.byref(C.c_uint64(0))))
        return hp[:n]


class PpmSession(_Session):
    """Owns a cgrt_ppm_session (Scene.ppm_session)."""
    _PREFIX, _INFO, _HITPOINTS = "cgrt_ppm_session_", _capi.PpmSessionInfo, "hitpoints"

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
        A = self._scene._torch()
        pr = _photon_rays(A, "add_photon_rays", org, dirs, flux, keys, draws, ("torch.int64",), ("torch.int32",))
        if pr.n == 0:
            return self
        A.torch.cuda.current_stream(A.dev).synchronize()  # the session traces on streams of its own
        check(self._L.cgrt_ppm_session_add_photon_rays(self._h, C.byref(pr)))
        return self

    def hitpoints(self):
        """[n, 16] of the current state: ppm_render(want_hitpoints=True)["hp"] at photons_done photons."""
        return self._hitpoint_dump()


class SppmSession(_Session):
    """Owns a cgrt_sppm_session (Scene.sppm_session)."""
    _PREFIX, _INFO, _HITPOINTS = "cgrt_sppm_session_", _capi.SppmSessionInfo, "last_hitpoints"

    def __init__(self, scene, h, width, rows, spp, grid):
        super().__init__(scene, h, width, rows, spp)
        self._grid = grid  # what add_passes renders with

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
        n = self._scene._ray_tensors("add_pass_rays", org, dirs, keys, pixel)
        A = self._scene._torch()
        r = self._scene._rays(A, n, org, dirs, keys, first_index, seed, max_depth, 0)
        A.torch.cuda.current_stream(org.device).synchronize()  # the pass runs on the null stream
        check(self._L.cgrt_sppm_session_pass_rays(self._h, C.byref(r), A.ptr(pixel), int(nphotons)))
        return self

    @property
    def passes(self):
        return self.info()["passes"]

    def pixels(self):
        """[rows * W, 8] float64: per texel {N, R2, tau[3], M_p of the last pass, Hitpoints of the last pass, 0}."""
        px = np.zeros((self.rows * self.width, 8), np.float64)
        check(self._L.cgrt_sppm_session_pixels(self._h, px.ctypes.data))
        return px

    def last_hitpoints(self):
        """[n, 16]: the last pass's table in PpmSession.hitpoints()' layout and order, flux = Phi_h, r2 = the radius the pass
        searched with, n = M_h."""
        return self._hitpoint_dump()


def camera_rays_host(width, height, spp=1, camera=None, seed=12345, rows=None, row_offset=0, stripe=None, sample_offset=0):
    """cgrt_camera_rays_host: the primary rays of the eye pass evaluated on the host -- no GPU and no scene needed.
    Returns (org [n,3] float64, dirs [n,3] float64, keys [n] uint64) numpy arrays, n = spp * rows * width, ray index =
    (k * rows + local row) * width + w; the same bits Scene.camera_rays makes on the device."""
    rows = height - row_offset if rows is None else rows
    cc, posed = _ccamera(camera)
    s_rows, s_rank, s_n = stripe if stripe else (0, 0, 1)
    g = _CGrid(width, height, rows, row_offset, s_rows, s_rank, s_n, spp, sample_offset, spp, 1, posed, seed)
    org, dirs, keys = _buffers.NUMPY.results("camera_rays_host", _CAMERA_RAYS, _CAMERA_RAYS, None, spp * rows * width).values()
    check(_capi.lib().cgrt_camera_rays_host(C.byref(cc), C.byref(g), org.ctypes.data, dirs.ctypes.data, keys.ctypes.data))
    return org, dirs, keys


def emit_photons_host(first, count, photon_seed=777, light=(0.0, 19.999, 20.0), jitter=2.0, power=700.0):
    """cgrt_photon_emit_host: the built-in emitter's photons [first, first + count) evaluated on the host -- no GPU and no scene
    needed.  Returns numpy arrays (org [n,3], dirs [n,3], flux [n,3] float64, keys [n] uint64, draws [n] uint32): the same bits
    Scene.emit_photons makes on the device."""
    return _emit_photons(_buffers.NUMPY, _capi.lib().cgrt_photon_emit_host, first, int(count), max(int(count), 0), photon_seed, light, jitter,
                         power)


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
