"""pt_ctx_reproject_var_weighted / pt_ctx_spp_plane at the ABI and their contract, without a device.

- The header declares both and states the contract; the library exports them; PT_ABI_VERSION is still 5; the Rust shim, abi.py
  and the Python binding mirror them.
- Every refusal of both calls, in the header's order: none needs a device (the context is a pointer that is never dereferenced,
  because the call is refused first).  d_spp changes no refusal.
- tests/reproject_weighted_ref.py against the restatements it stands on: a constant plane is reproject_var_moved, byte for byte.
- make reproject-weighted-check: the stand-alone host program under AddressSanitizer and UBSan exits 0.
The GPU side is tests/test_gpu_reproject_weighted.py."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import kats_camera as kc
import ptlib
import reproject_moved_ref as mref
import reproject_ref as ref
import reproject_weighted_ref as wref
from reproject_moved_ref import IDENTITY, MARKER
from reproject_ref import F32

ROOT = ptlib.ROOT
PT_ERR_INVALID = ptlib.abi.PT_ERR_INVALID


def _header(strip=True):
    text = open(os.path.join(ROOT, "include", "ptrace.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip else text


@pytest.fixture(scope="module")
def L():
    return ptlib.product()


# ---------------------------------------------------------------------------------------------------------- the ABI
def _names(h, name):
    return [q.split()[-1].lstrip("*") for q in re.search(r"\bint %s\((.*?)\);" % name, h, flags=re.S).group(1).split(",")]


def test_header_declares_them():
    h = _header()
    own, base = _names(h, "pt_ctx_reproject_var_weighted"), _names(h, "pt_ctx_reproject_var_moved")
    at = base.index("d_normal") + 1
    assert own == base[:at] + ["d_spp"] + base[at:] and len(own) == 24
    assert re.search(r"const uint32_t \*d_spp\s*,\s*const pt_camera \*hist_cam", h)
    assert re.search(r"\bint pt_ctx_spp_plane\(pt_ctx \*ctx, uint32_t width, uint32_t height, uint32_t base, const uint8_t \*d_mask\s*,"
                     r"\s*uint32_t masked, uint32_t \*d_spp, void \*hip_stream\);", h)
    assert re.search(r"#define PT_ABI_VERSION 5\b", h)  # symbols were added, nothing changed


def test_header_states_the_contract():
    def norm(t):
        return " ".join(t.replace("*", " ").split())

    text = _header(strip=False)
    at = text.index("reprojection with per-pixel sample counts")
    doc = norm(text[at:text.index("int pt_ctx_reproject_var_weighted", at)])
    for phrase in ("the layout pt_ctx_render_adaptive writes as its d_spp for a cfg without a band", "d_spp may alias no output",
                   "d_spp is never refused", "with d_spp == NULL the call is pt_ctx_reproject_var_moved",
                   "w0 = (float)weight (0 stands for 1)", "c = spp[idx] and wp = (float)c", "round-to-nearest",
                   "Every wt in steps 1 and 5 of pt_ctx_reproject, in the moments and in k = wt / len_out, is wp",
                   "long = len_out >= (float)min_frames * wp", "formed on the device in binary32",
                   "len_out = 0, m1 = s, m2 = s*s, e = +inf", "if n' > max_history, n' = max_history",
                   "out[c] = h[c], m1 = h1, m2 = h2", "not h + (x - h)*0", "-0 stays -0",
                   "long = len_out >= (float)min_frames * w0", "k = w0 / len_out", "not long: e = +inf",
                   "spp[q] == spp[idx]", "k = wp / len_out", "never read by a taken tap",
                   "A plane that holds the constant w everywhere gives, bit for bit, pt_ctx_reproject_var_moved with weight = w",
                   "spp[p] = (d_mask && mask[p] != 0) ? masked : base"):
        assert norm(phrase) in doc, phrase
    order = ["width or height 0; width * height above 2^28; NULL d_spp; NULL ctx"]
    assert all(norm(p) in doc for p in order)


def test_library_exports_them_and_the_abi_version_stays(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", ptlib.PRODUCT_SO], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"pt_ctx_reproject_var_weighted", "pt_ctx_spp_plane"} <= exported
    assert L.pt_abi_version() == 5


def test_rust_shim_mirrors_them():
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "ffi", "hip.rs")).read())
    ext = re.search(r'extern "C" \{(.*?)\n\}', rust, flags=re.S).group(1)

    def params(name):
        m = re.search(r"pub fn %s\((.*?)\)\s*->\s*i32;" % name, ext, flags=re.S)
        return [(q.split(":", 1)[0].strip(), q.split(":", 1)[1].strip()) for q in m.group(1).split(",") if ":" in q]

    base = params("pt_ctx_reproject_var_moved")
    at = [n for n, _ in base].index("d_normal") + 1
    assert params("pt_ctx_reproject_var_weighted") == base[:at] + [("d_spp", "*const u32")] + base[at:]
    assert [n for n, _ in params("pt_ctx_reproject_var_weighted")] == _names(_header(), "pt_ctx_reproject_var_weighted")
    assert params("pt_ctx_spp_plane") == [("ctx", "*mut PtCtx"), ("width", "u32"), ("height", "u32"), ("base", "u32"),
                                          ("d_mask", "*const u8"), ("masked", "u32"), ("d_spp", "*mut u32"),
                                          ("hip_stream", "*mut c_void")]


def test_python_binding_offers_them():
    pkg = importlib.import_module("path-tracer-rust_amd")
    assert callable(pkg.Context.reproject_var_weighted) and callable(pkg.Context.spp_plane)
    sig = ptlib.abi.SIGNATURES
    moved, own = sig["pt_ctx_reproject_var_moved"][1], sig["pt_ctx_reproject_var_weighted"][1]
    assert own == moved[:9] + [C.c_void_p] + moved[9:] and len(own) == 24
    assert sig["pt_ctx_spp_plane"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                                 C.c_void_p])
    import inspect
    p = inspect.signature(pkg.Context.reproject_var_weighted).parameters
    assert p["spp"].default is None and p["motion"].default is None


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_in_order_without_a_device(L):
    """pt_ctx_reproject_var_moved's refusals in its order, with and without a plane.  Each call breaks one rule and every rule
    checked AFTER it: the message names the first."""
    p = [C.c_void_p(0x1000 * (i + 1)) for i in range(16)]
    ctx = C.c_void_p(0x100000)
    cam = ref.pt_camera(kc.CORNELL_CAM)
    nan, inf = float("nan"), float("inf")
    bad = mref.table([IDENTITY, MARKER, (0.0, inf, 0.0, -2.0)])
    P = ptlib.PtReprojectVarParams

    def call(spp, cx, motion, n, width=4, params=None, err=p[13], hist_len=p[5], hist_cam=True):
        rc = L.pt_ctx_reproject_var_weighted(cx, width, 4, C.byref(params) if params else None, C.byref(cam), p[0], p[1], p[2], p[3], spp,
                                             C.byref(cam) if hist_cam else None, p[4], hist_len, p[11], p[6], p[7], p[8], p[9], p[10],
                                             p[12], err, motion, n, None)
        return rc, L.pt_last_error().decode()

    big = (1 << 20) + 1
    for spp in (None, p[14]):
        cases = [
            (call(spp, None, None, big, width=0, params=P(0, -1.0, 0, 0, 0, 9, 1), err=None), "max_history"),
            (call(spp, None, None, big, width=0, params=P(0, 0, 0, nan, 0, 9, 1), err=None), "normal_min"),
            (call(spp, None, None, big, width=0, params=P(0, 0, 0, 0, 0, 9, 1), err=None), "radius"),
            (call(spp, None, None, big, width=0, params=P(0, 0, 0, 0, 0, 0, 1), err=None), "flags"),
            (call(spp, None, None, big, width=0, err=None), "width and height"),
            (call(spp, None, None, big, width=1 << 27, err=None), "2^28"),
            (call(spp, None, None, big, err=None, hist_len=None, hist_cam=False), "d_error is NULL"),
            (call(spp, None, None, big, hist_len=None, hist_cam=False), "history"),
            (call(spp, None, None, big, hist_cam=False), "hist_cam"),
            (call(spp, None, None, big), "ctx"),
            (call(spp, ctx, None, big), "2^20"),
            (call(spp, ctx, bad, big), "2^20"),
            (call(spp, ctx, None, 3), "motion is NULL"),
            (call(spp, ctx, bad, 3), "finite scale"),
            (call(spp, ctx, mref.table([(0.0, 0.0, 0.0, nan)]), 1), "finite scale"),
        ]
        for i, ((rc, msg), word) in enumerate(cases):
            assert rc == PT_ERR_INVALID and word in msg, (spp, i, rc, msg, word)


def test_spp_plane_refusals_in_order_without_a_device(L):
    ctx, spp, mask = C.c_void_p(0x100000), C.c_void_p(0x2000), C.c_void_p(0x3000)

    def call(cx, w, h, out, m=mask):
        rc = L.pt_ctx_spp_plane(cx, w, h, 8, m, 32, out, None)
        return rc, L.pt_last_error().decode()

    cases = [
        (call(None, 0, 1 << 20, None), "must be positive"),
        (call(None, 1 << 20, 0, None), "must be positive"),
        (call(None, 1 << 14, (1 << 14) + 1, None), "2^28"),
        (call(None, 1 << 14, 1 << 14, None), "d_spp"),      # 2^28 itself passes
        (call(ctx, 4, 4, None, m=None), "d_spp"),
        (call(None, 4, 4, spp), "ctx"),
        (call(None, 4, 4, spp, m=None), "ctx"),             # a NULL mask is never refused
    ]
    for i, ((rc, msg), word) in enumerate(cases):
        assert rc == PT_ERR_INVALID and word in msg, (i, rc, msg, word)


# ------------------------------------------------------------------------------------ the restatement against its base
def _frames(w, h, seed):
    rng = np.random.default_rng(seed)
    n = w * h
    planes = np.array([2.0, 6.0, 6.25, 9.0], dtype=F32)

    def frame():
        return dict(color=rng.random((n, 3)).astype(F32), depth=planes[rng.integers(0, 4, n)], oid=rng.integers(-1, 3, n).astype(np.int32),
                    normal=(rng.random((n, 3)) - 0.5).astype(F32))

    cur, hist = frame(), frame()
    keep = rng.random(n) < 0.7
    for k in ("depth", "oid", "normal"):
        hist[k] = np.where(keep.reshape((n,) + (1,) * (cur[k].ndim - 1)), cur[k], hist[k])
    hist["len"] = (rng.integers(0, 5, n) * 4).astype(F32)
    m1 = (rng.random(n) * 3).astype(F32)
    hist["mom"] = np.stack([m1, m1 * m1 + rng.random(n).astype(F32)], axis=1).astype(F32)
    return cur, hist


@pytest.mark.parametrize("camera", ["identical", "orbited"])
def test_a_constant_plane_is_the_uniform_restatement(camera):
    w, h = 33, 9
    cam = kc.CORNELL_CAM
    hist_cam = dict(cam) if camera == "identical" else ref.orbit(cam, ref.ORBIT_DEGREES)
    cur, hist = _frames(w, h, 5)
    motion = (IDENTITY, (0.11, -0.05, 0.02, 1.0), MARKER)
    kw = dict(hist_cam=hist_cam, hist_color=hist["color"], hist_len=hist["len"], hist_moments=hist["mom"], hist_depth=hist["depth"],
              hist_object_id=hist["oid"], max_history=24.0, depth_tol=0.05, normal_min=0.5, min_frames=3, radius=2)
    blended = 0
    for weight in (1, 4, 40):  # 40: a count above max_history
        for normal in (True, False):
            for mo in ((), motion):
                args = (w, h, cam, cur["color"], cur["depth"], cur["oid"], cur["normal"] if normal else None)
                k2 = dict(kw, hist_normal=hist["normal"] if normal else None, motion=mo)
                want = mref.reproject_var_moved(*args, weight=weight, **k2)
                got = wref.reproject_var_weighted(*args, spp=np.full(w * h, weight, np.uint32), weight=7, **k2)
                for a, b, what in zip(got, want, ("colour", "length", "moments", "error")):
                    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), (camera, weight, normal, bool(mo), what)
                blended += int((want[1] > weight).sum())
        first = wref.reproject_var_weighted(w, h, cam, cur["color"], cur["depth"], cur["oid"], spp=np.full(w * h, weight, np.uint32),
                                            min_frames=3, radius=2, depth_tol=0.05)
        want = mref.reproject_var_moved(w, h, cam, cur["color"], cur["depth"], cur["oid"], weight=weight, min_frames=3, radius=2,
                                        depth_tol=0.05)
        for a, b in zip(first, want):
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    assert blended > 100


def test_restatement_of_a_pixel_without_samples():
    """by hand, on a still camera: one tap, so h is the history pixel itself"""
    w, h = 4, 1
    cam = kc.CORNELL_CAM
    color = np.array([[np.nan, 1, 1], [0.5, 0.5, 0.5], [0.25, 0.25, 0.25], [1, 1, 1]], dtype=F32)
    hcolor = np.array([[-0.0, 0.125, 0.25], [0.5, 0.25, 0.0], [9, 9, 9], [0.75, 0.5, 0.25]], dtype=F32)
    hist = dict(hist_cam=dict(cam), hist_color=hcolor, hist_len=np.array([100, 6, 0, 8], dtype=F32),
                hist_moments=np.array([[0.375, 0.25], [0.75, 0.75], [1, 1], [1.5, 3.0]], dtype=F32),
                hist_depth=np.full(4, 5.0, F32), hist_object_id=np.zeros(4, np.int32))
    out, ln, mom, e = wref.reproject_var_weighted(w, h, cam, color, np.full(4, 5.0, F32), np.zeros(4, np.int32), spp=np.zeros(4, np.uint32),
                                                  weight=4, max_history=64.0, min_frames=2, **hist)
    # capped, no NaN; the history's -0 went through step 4's sum, 0 + (-0)*1 = +0, as in every reprojection call
    assert out[0].tobytes() == np.array([0.0, 0.125, 0.25], F32).tobytes() and ln[0] == 64 and mom[0].tolist() == [0.375, 0.25]
    assert out[1].tobytes() == hcolor[1].tobytes() and ln[1] == 6 and e[1] == np.inf                          # 6 < 2 * 4: not long
    assert out[2].tobytes() == color[2].tobytes() and ln[2] == 0 and e[2] == np.inf and mom[2].tolist() == [0.75, 0.5625]
    k = F32(4) / F32(8)
    assert ln[3] == 8 and e[3] == np.sqrt(F32(0.75) * k) / np.sqrt(F32(2.0 ** -6) + F32(1.5))                 # long: k = w0 / len
    assert wref.spp_plane(4, 8, np.array([0, 1, 0, 255], np.uint8), 32).tolist() == [8, 32, 8, 32]
    assert wref.spp_plane(3, 5).tolist() == [5, 5, 5]


# ------------------------------------------------------------------------------------------- the stand-alone program
def test_make_reproject_weighted_check():
    """the host side - both calls' refusals, the weighted pixel with its count reads, taps and window over buffers of the exact
    size, the constant-plane consequence - under AddressSanitizer and UBSan, as a program of its own: no device, nothing loaded
    into this process"""
    ptlib.host_check("reproject-weighted")
