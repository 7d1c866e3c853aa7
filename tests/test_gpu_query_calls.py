"""The host-array queries of the ABI - pt_ctx_radiance, pt_ctx_intersect, pt_ctx_intersect_streams, pt_ctx_intersect_bounds,
pt_ctx_orbit_point, pt_ctx_numerics_probe, pt_ctx_numerics_sweep, pt_ctx_sincos_sweep, pt_ctx_primary_rays, pt_ctx_scatter - held
to THEMSELVES: what their staging (check, upload, one launch, the requested downloads) owes a caller whatever the kernels compute.
Every comparison is of bytes, for equality.  What the kernels compute is test_gpu_parity.py's and test_gpu_scatter.py's.

- Optional outputs and scratch reuse: the three interactive queries at n = 65, 1, 64 on one context (the scratch grows, then is
  larger than needed), with every output and with each output alone - the same bytes, nothing written past n elements.
- Stream boundaries: pt_ctx_intersect_streams on the first 1, 4095, 4096 and 4097 rays of one set - result i is result i of the
  longest call, and a hit's distance is pt_ctx_intersect's.
- Refusals with a live context: PT_ERR_INVALID, no output byte written, and the valid call right afterwards gives its bytes.
An output buffer starts as bytes of 0xAB (as binary32 about -1.2e-12, as int32 below -10^9: no result of these calls)."""
import ctypes as C

import numpy as np
import pytest

import gpudev
import ptlib
import scatter_walk as sw
from gpudev import L, same_bytes  # noqa: F401  (fixture)
from ptlib import PtScatterItem, PtScatterOut

pytestmark = pytest.mark.gpu
F32, I32, U32 = np.float32, np.int32, np.uint32
SCENES = ["cornell", "mesh"]  # without a BVH, with one
GUARD = 65  # rows behind the n a call may write: as many as the largest scratch of these tests holds
INVALID = ptlib.abi.PT_ERR_INVALID


def blank(rows, width, dtype):
    return np.full(rows * width * np.dtype(dtype).itemsize, 0xAB, np.uint8).view(dtype).reshape(rows, width)


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xAB).all())


def ptr(a):
    if a is None:
        return None
    return a.ctypes.data_as({F32: ptlib.fp, I32: ptlib.i32p, U32: ptlib.u32p}[a.dtype.type])


def make_rays(n):
    """the parity tests' rays from inside the scene: origins in (-2, 2)^3 - inside the box of both scenes - and unit directions"""
    rng = np.random.default_rng(11)
    o = rng.uniform(-2.0, 2.0, size=(n, 3)).astype(F32)
    v = rng.normal(size=(n, 3))
    return o, np.ascontiguousarray((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32))


O, D = make_rays(4097)

# the outputs of the three interactive queries, in argument order: (name, dtype, floats or ints per ray)
INTERSECT = (("t", F32, 1), ("object_id", I32, 1), ("tri_id", I32, 1), ("x", F32, 3), ("normal", F32, 3))
BOUNDS = (("hit", I32, 1), ("t", F32, 1), ("x", F32, 3), ("normal", F32, 3))
ORBIT = (("found", I32, 1), ("point", F32, 3), ("object_id", I32, 1), ("t", F32, 1))


def query(call, spec, n, given, o=O, d=D):
    """call(o, d, n, outputs..) with the outputs named in `given` and NULL for the others: (rc, every buffer)"""
    bufs = {name: blank(n + GUARD, width, dtype) for name, dtype, width in spec}
    rc = call(ptr(o), ptr(d), n, *[ptr(bufs[name]) if name in given else None for name, _, _ in spec])
    return rc, bufs


@pytest.fixture(scope="module", params=SCENES)
def dev(request, L):
    with gpudev.Device(L, gpudev.scene(request.param)) as d:
        d.n_objs = gpudev.scene(request.param).n_objs
        yield d


def interactive_calls(L, dev):
    ctx = dev.ctx
    return [("intersect", INTERSECT, lambda *a: L.pt_ctx_intersect(ctx, *a)),
            ("bounds[0]", BOUNDS, lambda *a: L.pt_ctx_intersect_bounds(ctx, 0, *a)),
            ("bounds[last]", BOUNDS, lambda *a: L.pt_ctx_intersect_bounds(ctx, dev.n_objs - 1, *a)),
            ("orbit", ORBIT, lambda *a: L.pt_ctx_orbit_point(ctx, *a))]


# ---------------------------------------------------------------------------------------- optional outputs and scratch reuse
def test_optional_outputs_and_scratch_reuse(L, dev):
    for what, spec, call in interactive_calls(L, dev):
        first = None
        for n in (65, 1, 64):
            rc, full = query(call, spec, n, {name for name, _, _ in spec})
            assert rc == 0, (what, n, L.pt_last_error())
            for name, _, _ in spec:
                assert untouched(full[name][n:]), "%s n=%d: %s was written past its n elements" % (what, n, name)
                assert not untouched(full[name][:n]), (what, n, name)
            if first is None:
                first = full
            for name, _, _ in spec:  # the same rays in a scratch larger than they need
                same_bytes(full[name][:n], first[name][:n], "%s n=%d: %s against the call of 65" % (what, n, name))
            for alone, _, _ in spec:
                rc, got = query(call, spec, n, {alone})
                assert rc == 0, (what, n, alone, L.pt_last_error())
                same_bytes(got[alone][:n], full[alone][:n], "%s n=%d: %s alone" % (what, n, alone))
                assert untouched(got[alone][n:]), "%s n=%d: %s alone was written past its n elements" % (what, n, alone)
                for name, _, _ in spec:
                    assert name == alone or untouched(got[name]), "%s n=%d: %s written with only %s given" % (what, n, name, alone)


# ------------------------------------------------------------------------------------------------------- stream boundaries
def streams(L, dev, n, flags):
    t, ids = blank(n + GUARD, 1, F32), blank(n + GUARD, 1, I32)
    rc = L.pt_ctx_intersect_streams(dev.ctx, ptr(O), ptr(D), n, flags, ptr(t), ptr(ids))
    assert rc == 0, (n, flags, L.pt_last_error())
    assert untouched(t[n:]) and untouched(ids[n:]), "n=%d flags=%d: written past n results" % (n, flags)
    return t[:n, 0], ids[:n, 0]


def test_stream_boundaries(L, dev):
    rc, q = query(lambda *a: L.pt_ctx_intersect(dev.ctx, *a), INTERSECT, 4097, {"t"})
    assert rc == 0, L.pt_last_error()
    for flags in (0, ptlib.FLAG_NO_BVH):
        t_all, id_all = streams(L, dev, 4097, flags)
        hit = id_all >= 0
        assert 0 < hit.sum() and np.isinf(t_all[~hit]).all()
        same_bytes(t_all[hit], q["t"][:4097, 0][hit], "flags=%d: a hit's t against pt_ctx_intersect's" % flags)
        for n in (1, 4095, 4096):
            t, ids = streams(L, dev, n, flags)
            same_bytes(t, t_all[:n], "flags=%d n=%d: t against the call of 4097" % (flags, n))
            same_bytes(ids, id_all[:n], "flags=%d n=%d: id against the call of 4097" % (flags, n))


# ------------------------------------------------------------------------------------------- refusals with a live context
class Call:
    """One entry point with a valid argument list: args maps each argument's name to its value, in order; `outs` names the
    output arguments (numpy arrays, blanked before every call)."""

    def __init__(self, fn, args, outs):
        self.fn, self.args, self.outs = fn, args, outs

    def __call__(self, **changed):
        for name in self.outs:
            self.args[name].view(np.uint8)[...] = 0xAB
        args = dict(self.args, **changed)
        rc = self.fn(*[ptr(v) if isinstance(v, np.ndarray) and v.dtype.type in (F32, I32, U32) else
                       (v.ctypes.data_as(C.POINTER(PtScatterOut)) if isinstance(v, np.ndarray) else v) for v in args.values()])
        return rc, {name: self.args[name].copy() for name in self.outs}


def the_calls(L, dev):
    ctx, n = dev.ctx, 5
    o, d = np.ascontiguousarray(O[:n]), np.ascontiguousarray(D[:n])
    rays = dict(ctx=ctx, o=o, d=d, n=n)

    def outputs(spec, rows=n):
        return {name: blank(rows, width, dtype) for name, dtype, width in spec}

    def u8(rows, size):
        return np.full((rows, size), 0xAB, np.uint8)

    items = (PtScatterItem * n)(*[sw.item(o[i], d[i], (1, 1, 1), 3 + i, i, i % 3, 1 + i % 7) for i in range(n)])
    deep = (PtScatterItem * n)(*[sw.item(o[i], d[i], (1, 1, 1), 3 + i, i, 12 if i == n - 1 else 0, 1) for i in range(n)])
    pix = np.arange(n, dtype=U32) * 7
    smp = np.arange(n, dtype=U32)
    outside = pix.copy()
    outside[n - 1] = 96 * 64
    return {
        "radiance": (Call(L.pt_ctx_radiance, dict(ctx=ctx, o=o[:1], d=d[:1], depth=0, n_samples=4, seed=5, pixel=7, backend=0, flags=0,
                                                  out_rgb=blank(1, 3, F32), stats=None), ["out_rgb"]),
                     [dict(ctx=None), dict(o=None), dict(d=None), dict(out_rgb=None), dict(depth=12), dict(n_samples=0),
                      dict(flags=2 << 8)], None),  # (PT_FLAG_PIPELINES(2))
        "intersect": (Call(L.pt_ctx_intersect, dict(rays, **outputs(INTERSECT)), [s[0] for s in INTERSECT]),
                      [dict(ctx=None), dict(o=None), dict(d=None)], dict(n=0)),
        "intersect_streams": (Call(L.pt_ctx_intersect_streams, dict(rays, flags=0, t=blank(n, 1, F32), id=blank(n, 1, I32)), ["t", "id"]),
                              [dict(ctx=None), dict(o=None), dict(d=None), dict(t=None), dict(id=None)], dict(n=0)),
        "intersect_bounds": (Call(L.pt_ctx_intersect_bounds, dict(dict(ctx=ctx, object=dev.n_objs - 1), o=o, d=d, n=n, **outputs(BOUNDS)),
                                  [s[0] for s in BOUNDS]),
                             [dict(ctx=None), dict(o=None), dict(d=None), dict(object=dev.n_objs), dict(object=dev.n_objs, n=0)], dict(n=0)),
        "orbit_point": (Call(L.pt_ctx_orbit_point, dict(rays, **outputs(ORBIT)), [s[0] for s in ORBIT]),
                        [dict(ctx=None), dict(o=None), dict(d=None)], dict(n=0)),
        "primary_rays": (Call(L.pt_ctx_primary_rays, dict(ctx=ctx, width=96, height=64, seed=3, pixel=pix, sample=smp, n=n, form=1,
                                                          o=blank(n, 3, F32), d=blank(n, 3, F32)), ["o", "d"]),
                         [dict(ctx=None), dict(pixel=None), dict(sample=None), dict(o=None), dict(d=None), dict(n=0), dict(form=2),
                          dict(pixel=outside)], None),
        "scatter": (Call(L.pt_ctx_scatter, dict(ctx=ctx, seed=9, form=sw.BY_ID, items=items, surfaces=None, n=n,
                                                out=u8(n, C.sizeof(PtScatterOut))), ["out"]),
                    [dict(items=None), dict(out=None), dict(n=0), dict(form=0x40 | sw.BY_ID), dict(form=sw.GIVEN), dict(items=deep),
                     dict(ctx=None)], None),
    }


def check_refusals(L, name, call, refusals, empty):
    rc, want = call()
    assert rc == 0, (name, L.pt_last_error())
    assert not any(untouched(v) for v in want.values()), name
    for bad in refusals:
        rc, got = call(**bad)
        assert rc == INVALID and L.pt_last_error(), (name, sorted(bad), rc)
        assert all(untouched(v) for v in got.values()), "%s refused for %s, yet an output was written" % (name, sorted(bad))
        rc, got = call()  # nothing is left sticky
        assert rc == 0, (name, sorted(bad), L.pt_last_error())
        for k in want:
            same_bytes(got[k], want[k], "%s after the refusal of %s: %s" % (name, sorted(bad), k))
    if empty is not None:  # n == 0 is a call of no rays, not an error
        rc, got = call(**empty)
        assert rc == 0 and all(untouched(v) for v in got.values()), (name, rc)


def test_refusals_leave_nothing_behind(L, dev):
    for name, (call, refusals, empty) in the_calls(L, dev).items():
        check_refusals(L, name, call, refusals, empty)


def test_refusals_of_the_scene_free_diagnostics(L):
    """the numerics calls need no scene; the two sweeps are run once, after their refusals, for what the header says of them"""
    n = 5
    with gpudev.Device(L) as bare:
        ctx = bare.ctx
        probe = Call(L.pt_ctx_numerics_probe, dict(ctx=ctx, x=np.linspace(0.5, 6.0, n).astype(F32), n=n, out_sin=blank(n, 1, F32),
                                                   out_cos=blank(n, 1, F32), out_sqrt=blank(n, 1, F32), out_rcp=blank(n, 1, F32),
                                                   out_philox=blank(n, 4, U32)),
                     ["out_sin", "out_cos", "out_sqrt", "out_rcp", "out_philox"])
        check_refusals(L, "numerics_probe", probe, [dict(ctx=None), dict(x=None), dict(out_sin=None), dict(out_cos=None),
                                                    dict(out_sqrt=None), dict(out_rcp=None), dict(out_philox=None), dict(n=0)], None)
        for fn, k in ((L.pt_ctx_numerics_sweep, 4), (L.pt_ctx_sincos_sweep, 2)):
            out = np.full(k * 8, 0xAB, np.uint8)
            p = out.ctypes.data_as(ptlib.u64p)
            assert fn(None, p) == INVALID and fn(ctx, None) == INVALID and untouched(out)
            assert fn(ctx, p) == 0, L.pt_last_error()
            got = out.view(np.uint64).tolist()
            assert (got[:3] == [0, 0, 1 << 32] and got[3] > 0) if k == 4 else got == [0, 1 << 24], got


def test_refusals_without_a_scene(L):
    """the calls that need a scene, on a context that has none"""
    with gpudev.Device(L) as bare:
        bare.n_objs = 1
        for name, (call, _, _) in the_calls(L, bare).items():
            rc, got = call()
            assert rc == INVALID and all(untouched(v) for v in got.values()), (name, rc)
