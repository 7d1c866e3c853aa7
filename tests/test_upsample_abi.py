"""pt_ctx_upsample at the ABI and its contract, without a device.

- The header declares pt_upsample_params and the three functions and states the contract; the library exports them;
  PT_ABI_VERSION is still 5; the Rust shim and the Python binding mirror them.
- Every refusal, in the header's order, with a NULL context (the last thing checked): none needs a device.
- pt_upsample_tap_host == tests/upsample_ref.py's tap, bit for bit, over whole axes.
- Properties of the restatement: identity, plain bilinear interpolation on one plane, what removes a tap, the fallback,
  whose albedo an edge pixel gets.
- The synthetic inputs of tests/test_gpu_upsample.py reach every path of the restatement.
The GPU side is tests/test_gpu_upsample.py."""
import ctypes as C
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ptlib
from ptlib import PtUpsampleParams
import upsample_ref as ref
from upsample_ref import F32, I32

ROOT = ptlib.ROOT
PT_ERR_INVALID = ptlib.abi.PT_ERR_INVALID
AXES = ((1, 1), (7, 3), (3, 7), (257, 129), (33, 33), (16384, 1), (1, 16384))
NAMES = ["ctx", "width", "height", "lo_width", "lo_height", "params", "d_lo_color", "d_lo_depth", "d_lo_object_id", "d_lo_normal",
         "d_lo_albedo", "d_depth", "d_object_id", "d_normal", "d_albedo", "d_out_color", "d_out_weight", "hip_stream"]


def _header(strip=True):
    text = open(os.path.join(ROOT, "include", "ptrace.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip else text


@pytest.fixture(scope="module")
def L():
    return ptlib.product()


def host_tap(L, size, lo, coord):
    first, frac = C.c_int32(-7), C.c_float(-7.0)
    rc = L.pt_upsample_tap_host(size, lo, coord, C.byref(first), C.byref(frac))
    return rc, first.value, F32(frac.value)


# ---------------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_them():
    h = _header()
    body = re.search(r"typedef struct pt_upsample_params \{(.*?)\} pt_upsample_params;", h, flags=re.S).group(1)
    fields = [(t, n.strip()) for t, names in re.findall(r"\b(uint32_t|float)\s+([\w\s,]+);", body) for n in names.split(",")]
    assert fields == [("float", "depth_tol"), ("float", "normal_min"), ("uint32_t", "flags")]
    assert [n for n, _ in PtUpsampleParams._fields_] == [n for _, n in fields]
    assert C.sizeof(PtUpsampleParams) == 12
    m = re.search(r"\bint pt_ctx_upsample\((.*?)\);", h, flags=re.S)
    params = [q.strip() for q in m.group(1).split(",")]
    assert "".join("p" if "*" in q else "i" for q in params) == "piiii" + "p" * 13
    assert [q.split()[-1].lstrip("*") for q in params] == NAMES
    assert re.search(r"\bint pt_upsample_defaults\(\s*pt_upsample_params \*\w+\);", h)
    m = re.search(r"\bint pt_upsample_tap_host\((.*?)\);", h, flags=re.S)
    assert "".join("p" if "*" in q else "i" for q in m.group(1).split(",")) == "iiipp"
    assert re.search(r"#define PT_ABI_VERSION 5\b", h)  # symbols were added, nothing changed


def test_header_states_the_contract():
    def norm(t):
        return " ".join(t.replace("*", " ").split())

    text = _header(strip=False)
    at = text.index("pt_ctx_upsample fills")
    doc = norm(text[at:text.index("typedef struct pt_upsample_params", at)])
    for phrase in ("THE ARITHMETIC", "The rules are pt_ctx_denoise's", "max(a, b) = a > b ? a : b", "clamp(v) = v < 0 ? 0 : (v > 1 ? 1 : v)",
                   "albedo[c] > 2^-6 ? albedo[c] : 1", "unless BOTH albedo planes are given", "x = idx % W, r = idx / W",
                   "ax = (2x + 1) * w + W", "x0 = (int)(ax / (2W)) - 1", "ex = ax % (2W)", "fx = (float)ex / (float)(2W)",
                   "ar = (2r + 1) * h + H", "fr = (float)er / (float)(2H)", "-1 <= x0 <= w-1 and 0 <= fx < 1", "x0 = x, fx = 0",
                   "b = (i ? fx : 1 - fx) * (j ? fr : 1 - fr)", "u_q[c] = lo_color[q][c] / m_c^lo(q)",
                   "lo_object_id[q] != object_id[idx]", "|depth[idx] - lo_depth[q]| <= depth_tol * max(depth[idx], lo_depth[q])",
                   "dot(N(idx), N_lo(q)) >= normal_min", "held to the id test alone", "sum[c] = sum[c] + u_q[c] * b",
                   "weight = bsum", "weight = 0", "out[c] = clamp((sum[c] / bsum) * m_c(idx))", "the output is clamp(color)",
                   "No scene is needed", "No scratch is taken", "changes no state of the context", "checked in this order",
                   "no output may alias any input or the other output", "SAME camera", "profiles/upsample_cpu_study.json",
                   "only when both normals are given", "only when both albedos are given"):
        assert norm(phrase) in doc, phrase
    order = ["depth_tol that is negative", "normal_min outside", "flags != 0", "four sizes 0", "above 2^14", "NULL d_lo_color", "NULL ctx"]
    where = [doc.index(p) for p in order]
    assert where == sorted(where)


def test_library_exports_them_and_the_abi_version_stays(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", ptlib.PRODUCT_SO], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"pt_ctx_upsample", "pt_upsample_defaults", "pt_upsample_tap_host"} <= exported
    assert L.pt_abi_version() == 5


def test_defaults_are_what_the_header_and_the_study_say(L):
    d = ref.defaults(L)
    assert 0 < d["depth_tol"] < 1 and 0 < d["normal_min"] <= 1
    doc = " ".join(_header(strip=False).replace("*", " ").split())
    m = re.search(r"pt_upsample_defaults fills in the values a zero field stands for: depth_tol 2\^-(\d+) \((\S+)\), "
                  r"normal_min (\S+), flags 0", doc)
    assert (2.0 ** -int(m.group(1)), float(m.group(2)), float(F32(m.group(3).rstrip(",")))) == (
        d["depth_tol"], d["depth_tol"], d["normal_min"])
    study = json.load(open(os.path.join(ROOT, "profiles", "upsample_cpu_study.json")))
    assert {k: float(F32(v)) for k, v in study["chosen"].items()} == d
    # ... and the chosen point is the grid's minimum of (c) after the filter, as the study defines the choice
    best = min(study["grid"], key=lambda g: g["score"])
    assert (best["depth_tol"], best["normal_min"]) == (study["chosen"]["depth_tol"], study["chosen"]["normal_min"])
    assert L.pt_upsample_defaults(None) == PT_ERR_INVALID


def test_rust_shim_mirrors_them():
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "ffi", "hip.rs")).read())
    body = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct PtUpsampleParams \{(.*?)\n\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", body) == [("depth_tol", "f32"), ("normal_min", "f32"), ("flags", "u32")]
    ext = re.search(r'extern "C" \{(.*?)\n\}', rust, flags=re.S).group(1)
    m = re.search(r"pub fn pt_ctx_upsample\((.*?)\)\s*->\s*i32;", ext, flags=re.S)
    params = [(q.split(":", 1)[0].strip(), q.split(":", 1)[1].strip()) for q in m.group(1).split(",") if ":" in q]
    assert [n for n, _ in params] == NAMES
    assert [t for _, t in params] == ["*mut PtCtx", "u32", "u32", "u32", "u32", "*const PtUpsampleParams", "*const f32", "*const f32",
                                      "*const i32", "*const f32", "*const f32", "*const f32", "*const i32", "*const f32", "*const f32",
                                      "*mut f32", "*mut f32", "*mut c_void"]
    assert re.search(r"pub fn pt_upsample_defaults\(out: \*mut PtUpsampleParams\) -> i32;", ext)
    assert re.search(r"pub fn pt_upsample_tap_host\(size: u32, lo_size: u32, coord: u32, first: \*mut i32, frac: \*mut f32\) -> i32;", ext)
    helper = rust[rust.index("pub fn upsample_into("):]
    helper = helper[:helper.index("\n}\n")]
    assert "pt_ctx_upsample(" in helper and "pt_device_download" not in helper


def test_python_binding_offers_them():
    pkg = importlib.import_module("path-tracer-rust_amd")
    assert [n for n, _ in pkg.pt_upsample_params._fields_] == [n for n, _ in PtUpsampleParams._fields_]
    assert C.sizeof(pkg.pt_upsample_params) == 12
    assert callable(pkg.Context.upsample)
    d = pkg.upsample_defaults()
    assert set(d) == {"depth_tol", "normal_min"}
    first, frac = ref.tap(7, 3, [5])
    assert pkg.upsample_tap_host(7, 3, 5) == (int(first[0]), float(frac[0]))
    with pytest.raises(Exception):
        pkg.upsample_tap_host(7, 3, 7)


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_in_order_without_a_device(L):
    """Each call breaks one rule and every rule checked AFTER it: the message names the first.  The context is NULL throughout."""
    p = [C.c_void_p(0x1000 * (i + 1)) for i in range(11)]  # never dereferenced: every call is refused before a device is touched
    P = PtUpsampleParams
    BIG = (1 << 14) + 1

    def call(sizes, prm, lo, own, outs):
        """lo: (color, depth, id, normal, albedo); own: (depth, id, normal, albedo); outs: (color, weight)"""
        rc = L.pt_ctx_upsample(None, *sizes, C.byref(prm) if prm is not None else None, *lo, *own, *outs, None)
        return rc, L.pt_last_error().decode()

    none5, none4, none2 = (None,) * 5, (None,) * 4, (None,) * 2
    lo, own, outs = tuple(p[0:5]), tuple(p[5:9]), (p[9], p[10])
    zero = (0, 0, 0, 0)
    nan, inf = float("nan"), float("inf")
    cases = [
        (call(zero, P(-0.5, 2.0, 6), none5, none4, none2), "depth_tol"),
        (call(zero, P(inf, 2.0, 6), none5, none4, none2), "depth_tol"),
        (call(zero, P(nan, 2.0, 6), none5, none4, none2), "depth_tol"),
        (call(zero, P(0.1, 1.5, 6), none5, none4, none2), "normal_min"),
        (call(zero, P(0.1, -1.5, 6), none5, none4, none2), "normal_min"),
        (call(zero, P(0.1, nan, 6), none5, none4, none2), "normal_min"),
        (call(zero, P(0.1, -1.0, 6), none5, none4, none2), "flags"),
        (call((0, 5, 5, BIG), P(0.1, 1.0, 0), none5, none4, none2), "must be positive"),
        (call((5, 0, 5, BIG), None, none5, none4, none2), "must be positive"),
        (call((5, 5, 0, BIG), None, none5, none4, none2), "must be positive"),
        (call((BIG, 5, 5, 0), None, none5, none4, none2), "must be positive"),
        (call((BIG, 5, 5, 5), None, none5, none4, none2), "2^14"),
        (call((5, BIG, 5, 5), None, none5, none4, none2), "2^14"),
        (call((5, 5, BIG, 5), None, none5, none4, none2), "2^14"),
        (call((5, 5, 5, BIG), None, none5, none4, none2), "2^14"),
        (call((4, 4, 2, 2), None, (None,) + lo[1:], own, outs), "is NULL"),
        (call((4, 4, 2, 2), None, (lo[0], None) + lo[2:], own, outs), "is NULL"),
        (call((4, 4, 2, 2), None, lo[:2] + (None,) + lo[3:], own, outs), "is NULL"),
        (call((4, 4, 2, 2), None, lo, (None,) + own[1:], outs), "is NULL"),
        (call((4, 4, 2, 2), None, lo, (own[0], None) + own[2:], outs), "is NULL"),
        (call((4, 4, 2, 2), None, lo, own, (None, p[10])), "is NULL"),
        (call((4, 4, 2, 2), None, lo, own, outs), "ctx"),
        (call((4, 4, 2, 2), P(0.1, -1.0, 0), lo[:3] + (None, None), own[:2] + (None, None), (p[9], None)), "ctx"),  # the optional ones
        (call((1 << 14, 1 << 14, 1 << 14, 1 << 14), None, lo, own, outs), "ctx"),                                 # 2^14 is allowed
        (call((1, 1 << 14, 1 << 14, 1), None, lo, own, outs), "ctx"),
    ]
    for i, ((rc, msg), word) in enumerate(cases):
        assert rc == PT_ERR_INVALID and word in msg, (i, rc, msg, word)


def test_tap_host_refusals(L):
    first, frac = C.c_int32(-7), C.c_float(-7.0)
    a, b = C.byref(first), C.byref(frac)
    assert L.pt_upsample_tap_host(4, 2, 0, None, b) == PT_ERR_INVALID
    assert L.pt_upsample_tap_host(4, 2, 0, a, None) == PT_ERR_INVALID
    assert L.pt_upsample_tap_host(0, 2, 0, a, b) == PT_ERR_INVALID
    assert L.pt_upsample_tap_host(4, 0, 0, a, b) == PT_ERR_INVALID
    assert L.pt_upsample_tap_host((1 << 14) + 1, 2, 0, a, b) == PT_ERR_INVALID
    assert L.pt_upsample_tap_host(4, (1 << 14) + 1, 0, a, b) == PT_ERR_INVALID
    assert L.pt_upsample_tap_host(4, 2, 4, a, b) == PT_ERR_INVALID
    assert (first.value, frac.value) == (-7, -7.0)  # nothing is written
    assert L.pt_upsample_tap_host(4, 2, 3, a, b) == 0 and (first.value, frac.value) == (1, 0.25)


# ------------------------------------------------------------------------------------ the tap position, bit for bit
@pytest.mark.parametrize("size,lo", AXES, ids=["%d<-%d" % a for a in AXES])
def test_tap_host_is_the_restatement(L, size, lo):
    coords = np.arange(size)
    first, frac = ref.tap(size, lo, coords)
    assert (first >= -1).all() and (first <= lo - 1).all() and (frac >= 0).all() and (frac < 1).all()
    # wherever one tap of the axis is outside the low-resolution frame, the other one's weight is > 0
    assert (frac[first < 0] > 0).all() and ((F32(1) - frac)[first + 1 > lo - 1] > 0).all()
    if size == lo:
        assert (first == coords).all() and (frac == 0).all()
    # the position means what the contract says: the centre of pixel x on the axis of the low-resolution centres
    centre = (coords + 0.5) * lo / size - 0.5
    assert np.abs(first + frac.astype(np.float64) - centre).max() <= 2.0 ** -24
    for c in coords:
        rc, gf, gfrac = host_tap(L, size, lo, int(c))
        assert rc == 0 and gf == first[c] and gfrac.tobytes() == frac[c].tobytes(), (size, lo, c, gf, gfrac, first[c], frac[c])


# -------------------------------------------------------------------------------------- properties of the restatement
def _guides(rng, n):
    return dict(depth=(rng.random(n) * 4 + 1).astype(F32), oid=rng.integers(-1, 3, n).astype(I32),
                normal=(rng.random((n, 3)) - 0.3).astype(F32), albedo=(rng.random((n, 3)) * 0.9 + 0.05).astype(F32))


def test_ref_equal_sizes_and_guides_return_the_colour():
    rng = np.random.default_rng(1)
    w, h = 9, 7
    g = _guides(rng, w * h)
    g["depth"][g["oid"] < 0] = np.inf
    g["normal"][::5] = 0  # a zero normal fails the normal test: the fallback is the same single tap
    color = (rng.random((w * h, 3)) * 1.5).astype(F32)  # some above 1: the output is clamp(color)
    out, wgt = ref.upsample(w, h, w, h, color, g["depth"], g["oid"], g["depth"], g["oid"], lo_normal=g["normal"], normal=g["normal"])
    assert out.tobytes() == np.minimum(color, F32(1)).tobytes()
    assert (wgt[::5][g["oid"][::5] >= 0] == 0).all() and (wgt[1::5] == 1).all()
    # with the albedos (c / m) * m is the colour within an ulp
    out2, _ = ref.upsample(w, h, w, h, color, g["depth"], g["oid"], g["depth"], g["oid"], lo_albedo=g["albedo"], albedo=g["albedo"])
    assert np.abs(out2 - np.minimum(color, F32(1))).max() <= 2.0 ** -23


def test_ref_one_object_on_one_plane_is_plain_bilinear():
    rng = np.random.default_rng(2)
    for W, H, w, h in ((7, 5, 3, 2), (33, 25, 16, 12), (16, 12, 33, 25), (5, 9, 5, 4)):
        color = rng.random((w * h, 3)).astype(F32)
        out, wgt = ref.upsample(W, H, w, h, color, np.full(w * h, 3.0, F32), np.ones(w * h, I32), np.full(W * H, 3.0, F32),
                                np.ones(W * H, I32))
        # bilinear interpolation at the pixel centres with the border clamped, in binary64
        img = color.reshape(h, w, 3).astype(np.float64)
        px = np.clip((np.arange(W) + 0.5) * w / W - 0.5, 0, w - 1)
        pr = np.clip((np.arange(H) + 0.5) * h / H - 0.5, 0, h - 1)
        x0, r0 = np.minimum(np.floor(px).astype(int), max(w - 2, 0)), np.minimum(np.floor(pr).astype(int), max(h - 2, 0))
        x1, r1 = np.minimum(x0 + 1, w - 1), np.minimum(r0 + 1, h - 1)
        fx, fr = (px - x0)[None, :, None], (pr - r0)[:, None, None]
        exp = (img[r0][:, x0] * (1 - fx) + img[r0][:, x1] * fx) * (1 - fr) + (img[r1][:, x0] * (1 - fx) + img[r1][:, x1] * fx) * fr
        assert np.abs(out.reshape(H, W, 3) - exp).max() < 1e-6, (W, H, w, h)
        assert (wgt > 0).all() and (wgt <= 1 + 2.0 ** -22).all()


def _flat(W, H, w, h, rng):
    n, nl = W * H, w * h
    nrm = np.array([0.0, 0.0, 2.0], dtype=F32)
    return dict(lo_color=rng.random((nl, 3)).astype(F32), lo_depth=np.full(nl, 6.0, F32), lo_object_id=np.ones(nl, I32),
                depth=np.full(n, 6.0, F32), object_id=np.ones(n, I32), lo_normal=np.tile(nrm, (nl, 1)), normal=np.tile(nrm, (n, 1)))


def test_ref_each_test_alone_removes_a_tap():
    """each of an id mismatch, a depth beyond tolerance and a flipped normal removes the low-resolution pixel it is put on from every
    frame pixel that tapped it - the result is the same whichever of them did it - and changes nothing else"""
    W, H, w, h = 12, 10, 6, 5
    rng = np.random.default_rng(3)
    A = _flat(W, H, w, h, rng)
    P = dict(depth_tol=0.05, normal_min=0.5)
    base, base_w, det = ref.upsample(W, H, w, h, **A, **P, detail=True)
    assert det["taken"][det["inside"]].all()
    q = 2 * w + 3
    results = []
    for key, value in (("lo_object_id", 2), ("lo_object_id", -1), ("lo_depth", 6.0 * 1.06), ("lo_depth", 6.0 / 1.06), ("lo_depth", np.nan),
                       ("lo_normal", (0.0, 0.0, -1.0)), ("lo_normal", (0.0, 0.0, 0.0)), ("lo_normal", (1.0, 0.0, 0.1))):
        B = dict(A, **{key: A[key].copy()})
        B[key][q] = value
        results.append(ref.upsample(W, H, w, h, **B, **P))
    for got in results[1:]:
        assert got[0].tobytes() == results[0][0].tobytes() and got[1].tobytes() == results[0][1].tobytes()
    changed = np.flatnonzero(results[0][1] != base_w)
    assert 4 <= len(changed) <= 16 and (results[0][1][changed] < base_w[changed]).all()
    same = np.setdiff1d(np.arange(W * H), changed)
    assert results[0][0][same].tobytes() == base[same].tobytes()
    # within the tolerances nothing is removed
    for key, value in (("lo_depth", 6.0 * 1.04), ("lo_normal", (0.0, 1.0, 1.0))):
        B = dict(A, **{key: A[key].copy()})
        B[key][q] = value
        got = ref.upsample(W, H, w, h, **B, **P)
        assert got[0].tobytes() == base.tobytes() and got[1].tobytes() == base_w.tobytes(), (key, value)
    # the normal test runs only when both normals are given
    flipped = dict(A, lo_normal=-A["lo_normal"])
    assert (ref.upsample(W, H, w, h, **flipped, **P)[1] == 0).all()
    for drop in ("normal", "lo_normal"):
        got = ref.upsample(W, H, w, h, **dict(flipped, **{drop: None}), **P)
        assert got[0].tobytes() == base.tobytes() and got[1].tobytes() == base_w.tobytes()
    # a miss is held to the id test alone: its taps' depths and normals do not matter
    M = dict(A, object_id=np.full(W * H, -1, I32), depth=np.full(W * H, np.inf, F32), lo_object_id=np.full(w * h, -1, I32),
             lo_depth=np.full(w * h, np.inf, F32), lo_normal=np.zeros((w * h, 3), F32))
    got = ref.upsample(W, H, w, h, **M, **P)
    assert got[0].tobytes() == base.tobytes() and got[1].tobytes() == base_w.tobytes()


def test_ref_no_tap_passes_takes_the_fallback_with_weight_zero():
    W, H, w, h = 12, 10, 6, 5
    rng = np.random.default_rng(4)
    A = _flat(W, H, w, h, rng)
    base, base_w = ref.upsample(W, H, w, h, **A)
    idx = 4 * W + 5
    B = dict(A, object_id=A["object_id"].copy())
    B["object_id"][idx] = 0  # an object the low-resolution frame does not hold
    got, got_w = ref.upsample(W, H, w, h, **B)
    assert got_w[idx] == 0 and base_w[idx] > 0
    assert got[idx].tobytes() == base[idx].tobytes()  # every tap inside the frame: plain bilinear, what the flat frame gave
    others = np.arange(W * H) != idx
    assert got[others].tobytes() == base[others].tobytes() and got_w[others].tobytes() == base_w[others].tobytes()


def test_ref_demodulation_puts_the_frames_albedo_on_an_edge_pixel():
    """a low-resolution pixel straddles an albedo edge (its albedo is the mix); the frame's pixels lie on one side each.  With
    constant irradiance the upsampled colour is irradiance times the FRAME's albedo - the edge is as sharp as the guides - while
    without the albedos it is the mix on both sides."""
    W, H, w, h = 8, 2, 4, 1
    A = _flat(W, H, w, h, np.random.default_rng(5))
    left, right = np.array([0.8, 0.2, 0.2], F32), np.array([0.2, 0.2, 0.8], F32)
    albedo = np.where((np.arange(W * H) % W < 4)[:, None], left, right).astype(F32)
    lo_albedo = np.stack([left, (left + right) / 2, (left + right) / 2, right]).astype(F32)
    irradiance = F32(0.5)
    A["lo_color"] = (lo_albedo * irradiance).astype(F32)
    out, _ = ref.upsample(W, H, w, h, **A, lo_albedo=lo_albedo, albedo=albedo)
    assert np.abs(out - albedo * irradiance).max() < 1e-6
    plain, _ = ref.upsample(W, H, w, h, **A)
    edge = [3, 4, W + 3, W + 4]
    assert np.abs(plain[edge] - albedo[edge] * irradiance).max() > 0.05
    # one albedo plane alone does not demodulate
    for kw in (dict(albedo=albedo), dict(lo_albedo=lo_albedo)):
        assert ref.upsample(W, H, w, h, **A, **kw)[0].tobytes() == plain.tobytes()


# --------------------------------------------------------------------------- the GPU tests' inputs reach every path
@pytest.mark.parametrize("case", ref.CASES + ref.LARGE, ids=["%dx%d<-%dx%d" % c for c in ref.CASES + ref.LARGE])
def test_synthetic_inputs_reach_every_path(case):
    """What keeps the byte comparison on the GPU from being empty, checked in the restatement alone.  On every case of more than
    64 frame pixels there is a pixel of each kind.  One kind cannot exist in one case: with a low-resolution frame LARGER on both
    axes every frame pixel's centre lies between two low-resolution centres (x0 = -1 needs w < W, x0 = w-1 needs w <= W), so no tap
    is outside it - that is asserted instead.  Another cannot exist where a low-resolution axis is ONE pixel long (three of
    upsample_ref.LARGE): of the two taps along it one is always outside, so no pixel takes all four - asserted instead, with what
    can exist there: each of the four tap positions is taken by some pixel, taps on both sides of both axes."""
    W, H, w, h = case
    hi, lo = ref.synthetic(W, H, w, h)
    for k in ("depth", "oid", "normal", "albedo"):
        assert len(hi[k]) == W * H and len(lo[k]) == w * h
    assert ((hi["oid"] >= -1) & (hi["oid"] <= 2)).all() and np.isinf(hi["depth"][hi["oid"] < 0]).all()
    out, wgt, det = ref.want(W, H, w, h, hi, lo, detail=True)
    kinds = ref.kinds(hi, wgt, det)
    print(case, kinds)
    if W * H > 64:
        for k in ("all_four", "some", "fallback", "miss_taken"):
            if k == "all_four" and (w == 1 or h == 1):
                assert kinds[k] == 0, (k, kinds)
                continue
            assert kinds[k] > 0, (k, kinds)
        assert det["taken"].any(axis=0).all(), det["taken"].sum(axis=0)  # each of the four tap positions, somewhere
        if w > W and h > H:
            assert kinds["outside"] == 0
        else:
            assert kinds["outside"] > 0
        # the optional planes matter on these inputs: each changes the result
        assert ref.want(W, H, w, h, hi, lo, normal=(False, False))[1].tobytes() != wgt.tobytes()
        assert ref.want(W, H, w, h, hi, lo, albedo=(False, False))[0].tobytes() != out.tobytes()
    assert ((out >= 0) & (out <= 1)).all() and ((wgt >= 0) & (wgt <= 1 + 2.0 ** -22)).all()
