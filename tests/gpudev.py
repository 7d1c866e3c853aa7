"""The device harness of the GPU tests and of tools/: a context and the device memory that goes with it, host <-> device copies,
streams, the guard protocol, the one pt_config builder, the byte comparer and the `L` fixture.  Nothing here knows a feature.
Importing this module loads no library and touches no device: GPU test modules are collected where there is no GPU."""
import contextlib
import ctypes as C
import os
import threading

import numpy as np
import pytest

import ptlib
from ptlib import PtConfig, PtStats

F32 = np.float32
_hip = None


def hip_runtime():
    """the HIP runtime the product is bound to: the copy already mapped into this process that is not torch's"""
    global _hip
    if _hip is None:
        ptlib.product()  # maps it
        paths = {line.split()[-1] for line in open("/proc/self/maps") if "/libamdhip64.so" in line}
        own = sorted(p for p in paths if "/torch/" not in p)
        assert own, "libptrace_hip.so has not mapped a HIP runtime: %r" % sorted(paths)
        hip = C.CDLL(own[0])
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        hip.hipLaunchHostFunc.argtypes = [C.c_void_p, HOST_FN, C.c_void_p]
        hip.hipStreamDestroy.argtypes = [C.c_void_p]
        hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        hip.hipEventSynchronize.argtypes = [C.c_void_p]
        hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        _hip = hip
    return _hip


@contextlib.contextmanager
def stream(nonblocking=False):
    """a HIP stream, destroyed on exit.  The default is what hipStreamCreate gives, a blocking stream: it synchronises implicitly
    with the null stream.  nonblocking=True is hipStreamNonBlocking, what torch or a GUI hands over (and what the library's own
    context stream is): nothing orders it against the null stream's copies."""
    hip, st = hip_runtime(), C.c_void_p()
    if nonblocking:
        assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0  # hipStreamNonBlocking
    else:
        assert hip.hipStreamCreate(C.byref(st)) == 0
    try:
        yield st
    finally:
        assert hip.hipStreamDestroy(st) == 0


HOST_FN = C.CFUNCTYPE(None, C.c_void_p)  # hipHostFn_t


class Gate:
    """Holds a stream at a known point: a host function (hipLaunchHostFunc) that waits until the gate is opened.  Whatever is
    enqueued on the stream behind it runs only after open() - or after `timeout` seconds, which is why a gate can delay a stream
    but never hang it: a gate that ran into its timeout says so (timed_out) and check() fails the test with that.  The callback
    makes no HIP call.  The Gate object, and with it the callback, has to stay referenced until the stream has been synchronised."""

    def __init__(self, st, timeout=2.0):
        self.timeout = timeout
        self._open, self._done = threading.Event(), threading.Event()
        self.released = self.timed_out = False
        self._timer = None
        self._fn = HOST_FN(self._wait)
        rc = hip_runtime().hipLaunchHostFunc(st, self._fn, None)
        assert rc == 0, "hipLaunchHostFunc: %d" % rc

    def _wait(self, _user):
        self.released = self._open.wait(self.timeout)
        self.timed_out = not self.released
        self._done.set()

    @property
    def finished(self):
        """the host function has returned: the stream has moved on"""
        return self._done.is_set()

    def open(self):
        self._open.set()

    def open_after(self, seconds):
        self._timer = threading.Timer(seconds, self._open.set)
        self._timer.daemon = True
        self._timer.start()

    def check(self, what=""):
        assert self.finished, "%s: the gate still holds its stream" % what
        assert not self.timed_out, "%s: the gate was never opened and ran into its %.1f s timeout" % (what, self.timeout)

    def close(self):
        """open it, whatever happened, and stop the timer: for a finally"""
        if self._timer is not None:
            self._timer.cancel()
        self._open.set()


def new_ctx(L, env=None):
    """A context created under the given tuning variables (they are read when the context is created)."""
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = C.c_void_p()
        assert L.pt_ctx_create(0, C.byref(ctx)) == 0, L.pt_last_error()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return ctx


def set_scene(L, ctx, sc, cam=None):
    cam = sc.cam if cam is None else cam
    assert L.pt_ctx_set_scene(ctx, C.byref(cam), sc.objs, sc.n_objs, sc.tris, sc.n_tris) == 0, L.pt_last_error()


class Device:
    """a context and the device memory that goes with it; an allocation may carry a name (a plane of a call), and every method
    that takes a device pointer takes such a name as well"""

    def __init__(self, L, scene=None, cam=None, env=None):
        self.L, self.ctx, self._owned, self.p = L, new_ctx(L, env), [], {}
        if scene is not None:
            self.set_scene(scene, cam)

    def set_scene(self, sc, cam=None):
        set_scene(self.L, self.ctx, sc, cam)

    def alloc(self, nbytes, name=None):
        p = C.c_void_p()
        assert self.L.pt_device_malloc(0, nbytes, C.byref(p)) == 0, self.L.pt_last_error()
        self._owned.append(p)
        if name is not None:
            self.p[name] = p
        return p

    def _at(self, ptr, offset=0):
        ptr = self.p[ptr] if isinstance(ptr, str) else ptr
        return C.c_void_p((ptr.value if isinstance(ptr, C.c_void_p) else int(ptr)) + offset) if offset else ptr

    def free(self, ptr):
        """give one allocation back before close() does"""
        self._owned.remove(ptr)
        self.L.pt_device_free(0, ptr)

    def upload(self, ptr, host, offset=0):
        """host array -> device, `offset` bytes into the allocation"""
        host = np.ascontiguousarray(host)
        assert hip_runtime().hipMemcpy(self._at(ptr, offset), host.ctypes.data_as(C.c_void_p), host.nbytes, 1) == 0  # host to device

    def download(self, ptr, count, dtype=F32, offset=0):
        """`count` elements of `dtype`, from `offset` bytes into the allocation"""
        host = np.zeros(count, dtype=dtype)
        assert self.L.pt_device_download(0, host.ctypes.data_as(C.c_void_p), self._at(ptr, offset), host.nbytes) == 0, \
            self.L.pt_last_error()
        return host

    def pixels(self, ptr, npix):
        """an (npix, 3) float frame"""
        return self.download(ptr, npix * 3).reshape(npix, 3)

    def stream(self, nonblocking=False):
        return stream(nonblocking)

    def render(self, cfg, ptr, accumulate=False, cancel=None, cb=None, want=0, stream=None):
        """pt_ctx_render (or pt_ctx_accumulate) into ptr, on `stream` (None: the context's own): ((npix, 3) image, stats)"""
        st = PtStats()
        call = self.L.pt_ctx_accumulate if accumulate else self.L.pt_ctx_render
        rc = call(self.ctx, C.byref(cfg), self._at(ptr), stream, C.cast(cancel, C.c_void_p) if cancel else None,
                  C.cast(cb, C.c_void_p) if cb else None, None, C.byref(st))
        assert rc == want, (rc, self.L.pt_last_error())
        return self.pixels(ptr, self.L.pt_config_pixels(C.byref(cfg))), st

    # the guard protocol: a sentinel behind what a call may write, looked at after the call
    def fill_guarded(self, ptr, n, guard, sentinel, dtype=F32, tail_only=False):
        """[0, n + guard) elements of ptr set to the sentinel; tail_only: [n, n + guard), the first n hold an input"""
        if tail_only:
            self.upload(ptr, np.full(guard, sentinel, dtype=dtype), n * np.dtype(dtype).itemsize)
        else:
            self.upload(ptr, np.full(n + guard, sentinel, dtype=dtype))

    def read_guarded(self, ptr, n, guard, sentinel, what, dtype=F32):
        """the first n elements of ptr; the guard elements behind them still hold the sentinel"""
        got = self.download(ptr, n + guard, dtype)
        assert (got[n:] == sentinel).all(), "%s was written past its %d elements" % (what, n)
        return got[:n]

    def close(self):
        for p in self._owned:
            self.L.pt_device_free(0, p)
        self._owned = []
        if self.ctx is not None:
            self.L.pt_ctx_destroy(self.ctx)
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def config(width, height, spp, *, backend=0, seed=0, band=None, chunks=None, rays_per_pass=0, flags=0):
    cfg = PtConfig(width, height, spp, backend, seed, 0, 0, rays_per_pass, flags)
    if band:
        cfg.idx_begin, cfg.idx_end = band
    if chunks:
        cfg.chunk_pixels, cfg.chunk_first, cfg.chunk_step = chunks
    return cfg


def same_bytes(got, want, what):
    """byte for byte equal, or how many words differ, where the first one is and both values"""
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert a.shape == b.shape and a.itemsize == b.itemsize, "%s: %s %s vs %s %s" % (what, a.dtype, a.shape, b.dtype, b.shape)
    if a.tobytes() != b.tobytes():
        word = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        bad = np.argwhere(a.view(word) != b.view(word))
        at = tuple(bad[0])
        raise AssertionError("%s: %d of %d words differ, first at %s: %r vs %r" % (
            what, len(bad), a.size, [int(i) for i in at], a[at], b[at]))


@pytest.fixture(scope="module")
def L():
    L = ptlib.product()
    assert L.pt_device_count() >= 1, "no HIP device visible: the product has no CPU fallback"
    return L


# ---------------------------------------------------------------------------------------------------- scenes and PFM files
_scenes = {}


def scene(sid):
    if sid not in _scenes:
        _scenes[sid] = ptlib.load_scene_py(ptlib.scene_path(sid), triangulate=(sid == "mesh-hdodec"))
    return _scenes[sid]


def read_pfm(path):
    data = open(path, "rb").read()
    magic, dims, scale, body = data.split(b"\n", 3)
    ch = {b"PF": 3, b"Pf": 1}[magic]
    w, h = (int(v) for v in dims.split())
    assert float(scale) == -1.0
    return np.frombuffer(body, dtype="<f4").reshape(h, w, ch)


def pfm_to_framebuffer(rows):
    """PFM row q from the bottom, column c = framebuffer index q*W + (W-1-c)"""
    h, w, ch = rows.shape
    return rows[:, ::-1, :].reshape(h * w, ch)
