"""CPU: what the Python binding (cgraytracing_amd/engine.py) promises its callers apart from numbers -- the signature of every
public function and method, and the first error of every bad call of the ray-list entry points -- against tables recorded from
the binding before its argument checks and result allocation moved into cgraytracing_amd/_buffers.py
(tests/golden/py_binding_signatures.json, py_binding_errors.json).  Needs no device: the scene is uncommitted, so a call whose
Python checks all pass is answered "scene not committed" by the library, and the "device" tensors are CPU tensors of a subclass
whose `device` says cuda:0.  A case that would touch a device (an allocation, torch's current stream) is not in the record."""
import inspect
import itertools
import json
import os

import numpy as np
import torch

import scenes
import cgraytracing_amd as cg
from cgraytracing_amd import engine
from cgraytracing_amd._capi import CgrtError

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIGNATURES = os.path.join(GOLDEN, "py_binding_signatures.json")
ERRORS = os.path.join(GOLDEN, "py_binding_errors.json")
N = 4  # rays of a good call


class OnDevice(torch.Tensor):
    """A CPU tensor that says it lives on cuda:0: passes the binding's checks, and its data_ptr() is never read because the
    library refuses the uncommitted scene first."""

    @property
    def device(self):
        return torch.device("cuda", 0)


def dev(shape, dtype):
    return torch.zeros(shape, dtype=dtype).as_subclass(OnDevice)


# ---------------------------------------------------------------- signatures
def _signatures():
    out = {}
    for name, f in vars(engine).items():
        if inspect.isfunction(f) and f.__module__ == engine.__name__ and not name.startswith("_"):
            out[name] = str(inspect.signature(f))
    for cls in (engine.Scene, engine.PpmSession, engine.SppmSession):
        for name, f in inspect.getmembers(cls):
            if name.startswith("_") and name != "__init__":
                continue
            if isinstance(f, property):
                out["%s.%s" % (cls.__name__, name)] = "property"
            elif inspect.isfunction(f):
                out["%s.%s" % (cls.__name__, name)] = str(inspect.signature(f))
    return out


# ---------------------------------------------------------------- bad calls
_WRONG = {torch.float64: torch.float32, torch.int64: torch.int32, torch.int32: torch.int64, torch.uint8: torch.int8}
_NP = {torch.float64: np.float64, torch.int64: np.uint64, torch.int32: np.int32, torch.uint8: np.uint8, torch.float32: np.float32,
       torch.int8: np.int8}
PAIR_FAULTS = ("list", "dtype", "cols", "length")


def faults(dtype, cols, host, n=N):
    """{fault: value} for an argument that is a [n] (cols None) or [n, cols] buffer of `dtype`; host: numpy arrays."""
    shape = (n,) if cols is None else (n, cols)
    bad_cols = (n, (cols or 1) + 1)
    longer = (n + 1,) + shape[1:]
    if host:
        mk = lambda s, dt=dtype: np.zeros(s, _NP[dt])
        return {"good": mk(shape), "none": None, "cpu": torch.zeros(shape, dtype=dtype), "list": np.zeros(shape).tolist(),
                "dtype": mk(shape, _WRONG[dtype]), "cols": mk(bad_cols), "length": mk(longer), "strided": mk((2 * n,) + shape[1:])[::2]}
    return {"good": dev(shape, dtype), "none": None, "cpu": torch.zeros(shape, dtype=dtype), "list": torch.zeros(shape).tolist(),
            "dtype": dev(shape, _WRONG[dtype]), "cols": dev(bad_cols, dtype), "length": dev(longer, dtype),
            "strided": dev((2 * n,) + shape[1:], dtype)[::2]}


def buffer_cases(args, host):
    """(case name, {argument: value}) over the buffers `args` = [(name, dtype, cols)]: all good at n = N and n = 0, every fault
    of every argument in turn, and PAIR_FAULTS x PAIR_FAULTS of every two arguments (which of two faults is reported)."""
    table = {name: faults(dt, cols, host) for name, dt, cols in args}
    good = {name: table[name]["good"] for name, _, _ in args}
    yield "good", dict(good)
    yield "good,n=0", {name: faults(dt, cols, host, 0)["good"] for name, dt, cols in args}
    for name, _, _ in args:
        for fault, v in table[name].items():
            if fault != "good":
                yield "%s=%s" % (name, fault), dict(good, **{name: v})
    for (a, _, _), (b, _, _) in itertools.combinations(args, 2):
        for fa, fb in itertools.product(PAIR_FAULTS, PAIR_FAULTS):
            yield "%s=%s,%s=%s" % (a, fa, b, fb), dict(good, **{a: table[a][fa], b: table[b][fb]})


F64, I64, I32, U8 = torch.float64, torch.int64, torch.int32, torch.uint8
ORG, DIRS, KEYS, PIXEL = ("org", F64, 3), ("dirs", F64, 3), ("keys", I64, None), ("pixel", I64, None)
# result name -> (dtype, shape at n rays): the docstrings' promises, preallocated so that a good call allocates nothing
TRACE_OUT = {"acc": (F64, (N, 3)), "nhit": (I32, (N,)), "hit_obj": (I32, (N,)), "hit_t": (F64, (N,)), "hit_normal": (F64, (N, 3))}
ATTR_OUT = {"prim": (I32, (N,)), "uv": (F64, (N, 2)), "color": (F64, (N, 3)), "material": (F64, (N, 2))}
BOUNCE_OUT = {"step": (U8, (N,)), "hit_obj": (I32, (N,)), "hit_t": (F64, (N,)), "pos": (F64, (N, 3)), "normal": (F64, (N, 3)),
              "value": (F64, (N, 3)), "child_org": (F64, (2 * N, 3)), "child_dir": (F64, (2 * N, 3)), "child_adj": (F64, (2 * N, 3)),
              "child_path": (I32, (2 * N,)), "child_keys": (I64, (2 * N,))}
WAVE_OUT = {"acc": (F64, (N, 3)), "nhit": (I32, (N,)), "hp9": (F64, (4 * N, 9)), "hp_ray": (I64, (4 * N,)), "hp_path": (I32, (4 * N,))}


def prealloc(spec, n=N):
    return {k: dev(tuple(s * n // N if i == 0 else s for i, s in enumerate(shape)), dt) for k, (dt, shape) in spec.items()}


def out_cases(spec):
    """(case name, out dict): one entry of a preallocated `out` wrong at a time."""
    for name, (dt, shape) in spec.items():
        for fault, v in (("dtype", dev(shape, _WRONG[dt])), ("shape", dev(shape + (2,), dt)), ("length", dev((shape[0] + 1,) + shape[1:], dt)),
                         ("ndarray", np.zeros(shape)), ("list", [0] * shape[0]), ("cpu", torch.zeros(shape, dtype=dt)),
                         ("strided", dev((2 * shape[0],) + shape[1:], dt)[::2])):
            yield "out[%s]=%s" % (name, fault), dict(prealloc(spec), **{name: v})


def counter_cases():
    yield "counters=dtype", dev((8,), I32)
    yield "counters=size", dev((7,), I64)
    yield "counters=ndarray", np.zeros(8, np.int64)
    yield "counters=list", [0] * 8
    yield "counters=cpu", torch.zeros(8, dtype=I64)
    yield "counters=strided", dev((16,), I64)[::2]


def cases(sc):
    """Every (entry point, case name, thunk) of the record, in a fixed order."""
    C8 = lambda: dev((8,), I64)
    zero = lambda spec: prealloc(spec, 0)

    def device_query(entry, f, args, spec, wants, counters=True, **fixed):
        """A torch query f(**buffers, out=, counters=, stream=0, **fixed) with results `spec`."""
        kw = dict(fixed, stream=0)
        cnt = lambda: dict(counters=C8()) if counters else {}
        for name, bufs in buffer_cases(args, False):
            out = zero(spec) if name == "good,n=0" else prealloc(spec)
            yield entry, name, lambda bufs=bufs, out=out: f(**bufs, out=out, **cnt(), **kw)
        for w in wants:
            yield entry, "want=%r" % (w,), lambda w=w: f(**dict(next(buffer_cases(args, False))[1]), out=prealloc(spec), **cnt(),
                                                         **dict(kw, want=w))
        for name, out in out_cases(spec):
            yield entry, name, lambda out=out: f(**dict(next(buffer_cases(args, False))[1]), out=out, **cnt(), **kw)
        if counters:
            for name, c in counter_cases():
                yield entry, name, lambda c=c: f(**dict(next(buffer_cases(args, False))[1]), out=prealloc(spec), counters=c, **kw)

    def host_query(entry, f, args, wants, **fixed):
        for name, bufs in buffer_cases(args, True):
            yield entry, name, lambda bufs=bufs: f(**bufs, **fixed)
        for w in wants:
            yield entry, "want=%r" % (w,), lambda w=w: f(**dict(next(buffer_cases(args, True))[1]), **dict(fixed, want=w))

    trace_wants = ((), ("nope",), ("hit",), ("hit_obj",), ("acc", "nope"), ("nhit", "acc"))
    attr_wants = ((), ("nope",), ("uv",), ("hit",), ("prim", "nope"))
    bounce_wants = ((), ("nope",), ("hit",), ("children",), ("step", "nope"), ("child_keys", "step"))
    wave_wants = ((), ("nope",), ("hp",), ("hp9",), ("acc", "nope"))
    all_trace = ("acc", "nhit", "hit")

    yield from device_query("trace_rays", sc.trace_rays, [ORG, DIRS, KEYS], TRACE_OUT, trace_wants)
    yield from host_query("trace_rays_host", sc.trace_rays_host, [ORG, DIRS, KEYS], trace_wants)
    attr_args = [ORG, DIRS, ("hit_obj", I32, None), ("hit_t", F64, None)]
    yield from device_query("hit_attributes", sc.hit_attributes, attr_args, ATTR_OUT, attr_wants, counters=False)
    yield from host_query("hit_attributes_host", sc.hit_attributes_host, attr_args, attr_wants)
    occ_args = [ORG, DIRS, ("tmax", F64, None), KEYS]
    # (occluded makes its own counters on the device: only its refusals are in the record)
    yield from device_query("occluded", sc.occluded, occ_args, {"occluded": (U8, (N,))}, (), counters=False)
    for fault, v in faults(U8, None, False).items():
        yield "occluded", "out=%s (a tensor)" % fault, lambda v=v: sc.occluded(**dict(next(buffer_cases(occ_args, False))[1]), out=v, stream=0)
    yield from host_query("occluded_host", sc.occluded_host, occ_args, ())
    bounce_args = [ORG, DIRS, ("adj", F64, 3), ("path", I32, None), KEYS]
    yield from device_query("bounce", sc.bounce, bounce_args, BOUNCE_OUT, bounce_wants)
    yield from host_query("bounce_host", sc.bounce_host, bounce_args, bounce_wants)
    yield from device_query("wavefront", sc.wavefront, [ORG, DIRS, KEYS], WAVE_OUT, wave_wants, want=("acc", "nhit", "hp"))
    yield from host_query("wavefront_host", sc.wavefront_host, [ORG, DIRS, KEYS], wave_wants, want=("acc", "nhit", "hp"))
    for kw in (dict(max_depth=0), dict(max_depth=31), dict(max_depth=32), dict(max_depth=8.0), dict(min_adj=-1), dict(min_adj=float("nan")),
               dict(hp_cap=-1), dict(hp_cap=0), dict(work_bytes=-1), dict(max_depth=0, min_adj=-1), dict(want=("nope",), max_depth=0)):
        good = lambda: dict(next(buffer_cases([ORG, DIRS, KEYS], False))[1])
        out = prealloc({k: v for k, v in WAVE_OUT.items() if k in ("acc", "nhit")})
        yield "wavefront", repr(kw), lambda kw=kw, out=out: sc.wavefront(**good(), out=out, counters=C8(), stream=0, **kw)
        yield "wavefront_host", repr(kw), lambda kw=kw: sc.wavefront_host(**dict(next(buffer_cases([ORG, DIRS, KEYS], True))[1]), **kw)

    # the ray-buffer calls behind _ray_tensors; an uncommitted scene is refused by the library before a tensor is looked at
    for name, bufs in buffer_cases([ORG, DIRS, KEYS], False):
        yield "trace_rays_hitpoints", name, lambda bufs=bufs: sc.trace_rays_hitpoints(**bufs)
    for name, bufs in buffer_cases([ORG, DIRS, KEYS, PIXEL], False):
        yield "ppm_session_rays", name, lambda bufs=bufs: sc.ppm_session_rays(**bufs, width=2, rows=2)
        yield "ppm_session_wavefront", name, lambda bufs=bufs: sc.ppm_session_wavefront(**bufs, width=2, rows=2)
    for name, bufs in buffer_cases([("hp9", F64, 9), ("ray", I64, None), ("path", I32, None), PIXEL], False):
        yield "ppm_session_hitpoints", name, lambda bufs=bufs: sc.ppm_session_hitpoints(**bufs, width=2, rows=2)
    ppm, sppm = engine.PpmSession(sc, None, 2, 2, 1), engine.SppmSession(sc, None, 2, 2, 1, {})
    for name, bufs in buffer_cases([ORG, DIRS, ("flux", F64, 3), KEYS, ("draws", I32, None)], False):
        yield "PpmSession.add_photon_rays", name, lambda bufs=bufs: ppm.add_photon_rays(**bufs) is ppm
    for name, bufs in buffer_cases([ORG, DIRS, KEYS, PIXEL], False):
        yield "SppmSession.add_pass_rays", name, lambda bufs=bufs: sppm.add_pass_rays(nphotons=10, **bufs)

    for kw in (dict(), dict(relay_order="nope"), dict(relay_order="interleaved"), dict(relay_order=1), dict(relay_start="nope"),
               dict(relay_start="cost"), dict(relay_start=0), dict(sample_relay=3), dict(sample_relay=4), dict(sample_relay=2.5),
               dict(sample_relay="4"), dict(sample_relay=0), dict(sample_relay=True), dict(relay_order="nope", relay_start="nope"),
               dict(relay_order="nope", sample_relay=3), dict(relay_start="nope", sample_relay=3), dict(relay_boost=True, relay_mirror=False)):
        yield "trace_grid_host", repr(kw), lambda kw=kw: sc.trace_grid_host(8, 8, **kw)


def _outcome(thunk):
    """[kind, text]: "ok" and what came back, or the exception's type -- with its message for a ValueError and a CgrtError."""
    try:
        r = thunk()
    except CgrtError as e:
        return ["CgrtError", str(e)]
    except ValueError as e:  # the binding's own begin "name: "; numpy's wording of a failed coercion is not part of the record
        return ["ValueError", str(e) if str(e).split(":")[0].isidentifier() else ""]
    except Exception as e:
        return [type(e).__name__, ""]
    return ["ok", ",".join(sorted(r)) if isinstance(r, dict) else repr(r) if isinstance(r, bool) else ""]


def _run():
    sc = cg.Scene(scenes.scene_c1(), commit=False)
    try:
        got = {}
        for entry, name, thunk in cases(sc):
            assert name not in got.setdefault(entry, {}), (entry, name)
            got[entry][name] = _outcome(thunk)
        return got
    finally:
        sc.close()


KEPT = ("ok", "ValueError", "CgrtError", "AttributeError", "TypeError")  # everything else needed a device to get further


def record():
    """Writes both tables from the binding that is imported -- run by hand on the commit whose behaviour is to be kept, never by
    pytest: python -c "import test_py_binding_host as t; t.record()"."""
    with open(SIGNATURES, "w") as f:
        json.dump(_signatures(), f, indent=0, sort_keys=True)
        f.write("\n")
    got = {e: {k: o for k, o in v.items() if o[0] in KEPT} for e, v in _run().items()}
    outcomes = sorted({tuple(o) for v in got.values() for o in v.values()})
    table = {"outcomes": [list(o) for o in outcomes], "calls": {e: {k: outcomes.index(tuple(o)) for k, o in v.items()} for e, v in got.items()}}
    with open(ERRORS, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")


def test_signatures_are_the_recorded_ones():
    """Every public function of engine and every public method and property of Scene, PpmSession and SppmSession: the same
    names, parameter names, order and defaults as recorded."""
    want = json.load(open(SIGNATURES))
    got = _signatures()
    assert sorted(got) == sorted(want)
    assert not {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert len(got) >= 80 and {"relay_start_host", "relay_boost_host", "camera_rays_host", "emit_photons_host", "Scene.trace_grid",
                               "PpmSession.image_tensor", "SppmSession.last_hitpoints", "SppmSession.photons_done"} <= set(got)


def test_first_error_of_every_bad_call_is_the_recorded_one():
    """trace_rays, hit_attributes, occluded, bounce, wavefront and their _host forms, trace_rays_hitpoints, the three ray- and
    Hitpoint-fed session creators, PpmSession.add_photon_rays and SppmSession.add_pass_rays: for every buffer argument in turn
    None, a CPU tensor, a list, a wrong dtype, column count or length and a strided view, two faults at once for every pair of
    arguments, bad `want`, `out[...]` and `counters`, the wavefront's scalar limits and trace_grid_host's relay switches.  The
    exception type, and for ValueError and CgrtError the message, of every case is the recorded one -- in particular which of
    two faults is reported.  The one change: a non-tensor in out[...] or counters, once an AttributeError, is the ValueError
    its siblings always raised."""
    table = json.load(open(ERRORS))
    got = _run()
    assert sorted(table["calls"]) == sorted(got)
    total, fixed, diff = 0, [], []
    for entry, calls in table["calls"].items():
        assert set(calls) <= set(got[entry]), (entry, sorted(set(calls) - set(got[entry]))[:5])
        for name, i in calls.items():
            want, g = table["outcomes"][i], got[entry][name]
            total += 1
            if want[0] == "AttributeError":
                fixed.append((entry, name, g))
            elif g != want:
                diff.append((entry, name, g, want))
    assert not diff, (len(diff), diff[:8])
    assert total >= 1000, total
    # the cases that changed: trace_rays' out[...] and counters, bounce's and wavefront's counters -- given an ndarray or a list
    assert 0 < len(fixed) <= 16, len(fixed)
    for entry, name, g in fixed:
        assert entry in ("trace_rays", "bounce", "wavefront") and name.split("=")[1] in ("ndarray", "list"), (entry, name)
        what = "counters" if name.startswith("counters") else "out[%r]" % name[4:name.index("]")]
        assert g[0] == "ValueError" and g[1].startswith("%s: %s must be a contiguous " % (entry, what)), (entry, name, g)
    bad = [(e, k, o) for e, v in got.items() for k, o in v.items() if k in table["calls"][e] and o[0] in ("AttributeError", "TypeError")]
    assert not bad, bad[:8]
    texts = {o[1] for v in got.values() for o in v.values()}
    assert any(t.endswith("scene not committed") for t in texts) and "trace_rays: org and dirs differ in length" in texts
