"""pt_ctx_denoise_var at the ABI and its contract, without a device.

- The header declares pt_denoise_var_params, pt_denoise_var_defaults and pt_ctx_denoise_var; the Rust shim mirrors them; the
  library exports them; the Python binding offers them; every invalid argument is refused with PT_ERR_INVALID before a device
  is touched, in the header's order (a NULL context is the LAST thing checked, so each case is refused for its own reason).
- Known answers on tests/denoise_var_ref.py, the numpy restatement of the header's arithmetic, with values exact in binary32.
- The CPU study as a regression test of the contract's quality (tools/denoise_var_cpu_study.py,
  profiles/denoise_var_cpu_study.json, inputs by tests/denoise_var_inputs.py): in each of the four (scene, n) cells the
  restatement at the library's defaults stays within 1.15 x the ratio the study recorded (the frames are deterministic; the
  15 % is room for a later deliberate change of a constant), and at 256 samples the guided filter improves the frame (ratio
  below 1) and beats pt_ctx_denoise's restatement at pt_ctx_denoise's defaults on the same input.
The GPU side is tests/test_gpu_denoise_var.py."""
import ctypes as C
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref
import denoise_var_inputs as inp
import denoise_var_ref as ref
import ptlib
from ptlib import PtDenoiseVarParams
from denoise_var_ref import F32

ROOT = ptlib.ROOT
PT_ERR_INVALID = ptlib.abi.PT_ERR_INVALID
BIG = float(2.0 ** 16)  # a sigma_var so large that, with e = 12, fall(xc) is exactly 1 for colour differences up to 1
STUDY = json.load(open(os.path.join(ROOT, "profiles", "denoise_var_cpu_study.json")))
CELLS = [(sid, n) for sid in inp.SCENES for n in inp.SPP]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptrace.h")).read(), flags=re.S)


def _lib():
    L = ptlib.product()
    return L


# ---------------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_them():
    h = _header()
    body = re.search(r"typedef struct pt_denoise_var_params \{(.*?)\} pt_denoise_var_params;", h, flags=re.S).group(1)
    assert re.findall(r"\b(uint32_t|float)\s+(\w+);", body) == [
        ("uint32_t", "levels"), ("float", "sigma_var"), ("float", "sigma_depth"), ("uint32_t", "flags")]
    assert [(n, t) for n, t in PtDenoiseVarParams._fields_] == [
        ("levels", C.c_uint32), ("sigma_var", C.c_float), ("sigma_depth", C.c_float), ("flags", C.c_uint32)]
    m = re.search(r"\bint pt_ctx_denoise_var\((.*?)\);", h, flags=re.S)
    kinds = "".join("p" if "*" in q else "i" for q in m.group(1).split(","))
    assert kinds == "piipppppppp"  # ctx, width, height, params, color, error, albedo, normal, depth, out, stream
    names = [q.split()[-1].lstrip("*") for q in m.group(1).split(",")]
    assert names[4:6] == ["d_color", "d_error"]
    assert re.search(r"\bint pt_denoise_var_defaults\(\s*pt_denoise_var_params \*\w+\);", h)
    assert re.search(r"#define PT_ABI_VERSION 5\b", h)  # symbols were added, nothing changed


def test_rust_shim_mirrors_them():
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "ffi", "hip.rs")).read())
    body = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct PtDenoiseVarParams \{(.*?)\n\}", rust,
                     flags=re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", body) == [("levels", "u32"), ("sigma_var", "f32"), ("sigma_depth", "f32"),
                                                      ("flags", "u32")]
    ext = re.search(r'extern "C" \{(.*?)\n\}', rust, flags=re.S).group(1)
    m = re.search(r"pub fn pt_ctx_denoise_var\((.*?)\)\s*->\s*i32;", ext, flags=re.S)
    params = [q.split(":", 1)[1].strip() for q in m.group(1).split(",") if ":" in q]
    assert "".join("p" if t.startswith("*") else "i" for t in params) == "piipppppppp"
    assert params[3] == "*const PtDenoiseVarParams"
    assert re.search(r"pub fn pt_denoise_var_defaults\(\s*out: \*mut PtDenoiseVarParams\s*\)\s*->\s*i32;", ext)


def test_library_exports_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", ptlib.PRODUCT_SO], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"pt_ctx_denoise_var", "pt_denoise_var_defaults"} <= exported


def test_python_binding_offers_them():
    pkg = importlib.import_module("path-tracer-rust_amd")
    L = pkg.lib()
    assert L.pt_ctx_denoise_var.argtypes is not None and len(L.pt_ctx_denoise_var.argtypes) == 11
    assert L.pt_denoise_var_defaults.argtypes is not None
    assert [n for n, _ in pkg.pt_denoise_var_params._fields_] == ["levels", "sigma_var", "sigma_depth", "flags"]
    assert callable(getattr(pkg.Context, "denoise_var", None))
    lv, sv, sd = ref.defaults(_lib())
    assert pkg.denoise_var_defaults() == {"levels": lv, "sigma_var": sv, "sigma_depth": sd}


def test_defaults_are_the_study_s_chosen_point():
    L = _lib()
    p = PtDenoiseVarParams(9, -1.0, -1.0, 77)
    assert L.pt_denoise_var_defaults(C.byref(p)) == 0
    assert p.levels == 5 and p.flags == 0
    assert L.pt_denoise_var_defaults(None) == PT_ERR_INVALID
    assert (p.sigma_var, p.sigma_depth) == (STUDY["chosen"]["sigma_var"], STUDY["chosen"]["sigma_depth"])
    # the chosen point is the grid's minimum of the mean over the four cells, and the grid is the one asked for
    best = min(STUDY["grid"], key=lambda g: g["mean"])
    assert best == STUDY["chosen"]
    assert sorted({g["sigma_var"] for g in STUDY["grid"]}) == [2.0 ** k for k in range(-2, 4)]
    assert sorted({g["sigma_depth"] for g in STUDY["grid"]}) == [2.0 ** k for k in range(-7, 2)]
    assert sorted(STUDY["chosen"]["ratio"]) == sorted("%s_%d" % c for c in CELLS)


def test_invalid_arguments_are_refused_without_a_device_in_the_stated_order():
    L = _lib()
    buf = C.c_void_p(256)  # never dereferenced: every call below is refused before a device is touched
    nan, inf = float("nan"), float("inf")

    def call(params=None, w=8, h=8, color=buf, error=buf, out=buf):
        pp = C.byref(PtDenoiseVarParams(*params)) if params is not None else None
        rc = L.pt_ctx_denoise_var(None, w, h, pp, color, error, buf, buf, buf, out, None)
        return rc, L.pt_last_error().decode()

    cases = [
        (dict(params=(9, 0, 0, 0)), "levels"),
        (dict(params=(5, -1.0, 0, 0)), "sigma"),
        (dict(params=(5, nan, 0, 0)), "sigma"),
        (dict(params=(5, inf, 0, 0)), "sigma"),
        (dict(params=(5, 0, -0.5, 0)), "sigma"),
        (dict(params=(5, 0, nan, 0)), "sigma"),
        (dict(params=(5, 0, inf, 0)), "sigma"),
        (dict(params=(5, 0, 0, 2)), "flags"),
        (dict(params=(5, 0, 0, 0x80000001)), "flags"),
        (dict(w=0), "width"),
        (dict(h=0), "width"),
        (dict(w=16385, h=16384), "2^28"),
        (dict(w=0xffffffff, h=0xffffffff), "2^28"),
        (dict(color=None), "d_color"),
        (dict(error=None), "d_error"),
        (dict(out=None), "d_out"),
        (dict(), "ctx"),                           # everything valid but the context
        (dict(params=(8, 1.0, 1.0, 1)), "ctx"),    # the limits themselves are accepted
        (dict(w=16384, h=16384), "ctx"),
        # the order: an earlier field wins over every later one
        (dict(params=(9, -1.0, 0, 2), w=0, color=None, error=None, out=None), "levels"),
        (dict(params=(8, -1.0, 0, 2), w=0, color=None, error=None, out=None), "sigma"),
        (dict(params=(8, 1.0, 0, 2), w=0, color=None, error=None, out=None), "flags"),
        (dict(w=0, h=0, color=None, error=None, out=None), "width"),
        (dict(w=16385, h=16384, color=None, error=None, out=None), "2^28"),
        (dict(color=None, error=None, out=None), "d_color"),
        (dict(error=None, out=None), "d_error"),
    ]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == PT_ERR_INVALID, (kw, rc)
        assert word in msg, (kw, msg)
    assert "pt_ctx_denoise" in call(error=None)[1].replace("pt_ctx_denoise_var", "")  # it points to the filter without a map


# ------------------------------------------------------------------------------------------- known answers on the rebuild
@pytest.mark.parametrize("levels", range(1, 9))
def test_a_constant_frame_is_a_fixed_point(levels):
    """Colour (1/4, 1/2, 3/4) everywhere: every colour difference is 0, so xc = 0 * r = 0 (r is finite: kv V + 2^-20 > 0) and
    fall = 1 whatever the error map says; every product with a weight, every partial sum and the quotient are exact."""
    w, h = 7, 5
    col = np.tile(np.array([0.25, 0.5, 0.75], F32), (w * h, 1))
    alb = np.full((w * h, 3), 0.5, F32)  # u = colour / 0.5 is exact, and so is the way back
    nrm = np.tile(np.array([0.0, 0.0, 2.0], F32), (w * h, 1))
    dep = np.full(w * h, 3.0, F32)
    col2 = col * F32(0.5)
    mixed = np.resize(np.array([0.0, 0.25, 12.0, np.inf, np.nan], F32), w * h)
    for e in (0.0, 0.25, 12.0, np.inf, np.nan, mixed):
        err = np.broadcast_to(np.asarray(e, F32), (w * h,))
        out = ref.denoise_var(col, err, w, h, levels=levels, sigma_var=1.0, sigma_depth=1.0)
        assert out.tobytes() == col.tobytes()
        out = ref.denoise_var(col2, err, w, h, alb, nrm, dep, levels=levels, sigma_var=1.0, sigma_depth=1.0)
        assert out.tobytes() == col2.tobytes()


@pytest.mark.parametrize("levels", [1, 3, 5])
def test_without_noise_a_checkerboard_comes_back(levels):
    """e = 0 everywhere: V = 0, r = 1 / 2^-20 = 2^20.  The two colours differ by 1/4 in every channel at least, so between
    them xc >= (1/16) * 2^20 >= 8 and fall = 0: those taps add u * 0 and 0.  Between equal colours xc = 0 and w = h, a
    multiple of 1/256; colour * h, the partial sums and the quotient (c * S) / S are exact for these short mantissas."""
    w, h = 11, 7
    yy, xx = np.mgrid[0:h, 0:w]
    odd = ((xx + yy) & 1).astype(bool).reshape(-1)
    col = np.where(odd[:, None], np.array([0.25, 0.75, 0.5], F32), np.array([0.5, 0.25, 0.75], F32)).astype(F32)
    out = ref.denoise_var(col, np.zeros(w * h, F32), w, h, levels=levels, sigma_var=1.0, sigma_depth=1.0)
    assert out.tobytes() == col.tobytes()
    # and the estimate is what lets it through: the same frame under e = 12 is smoothed
    out = ref.denoise_var(col, np.full(w * h, 12.0, F32), w, h, levels=levels, sigma_var=BIG, sigma_depth=1.0)
    assert out.tobytes() != col.tobytes()


def test_one_bright_pixel_gives_the_renormalised_b_spline():
    """5x5, pixel (2, 2) = (1, 1, 1), the others 0, no guides, one level, e = 12, sigma_var 2^16: Vraw >= 3 (12 sqrt(2^-6))^2 =
    6.75 everywhere, so r <= 1 / (2^32 * 6.75) and xc <= 3 r < 2^-32; 1 - xc/8 rounds to 1, fall = 1.  Every tap inside the
    frame has w = h, only the tap onto (2, 2) adds anything, and - as for pt_ctx_denoise -
        out(x, y) = B[|2-y|] B[|2-x|] / (S(y) S(x)),  S(c) = sum of B[|d|] over d in -2..2 with 0 <= c + d < 5,
    one correctly rounded division of two exact numbers."""
    w = h = 5
    col = np.zeros((h, w, 3), F32)
    col[2, 2] = 1.0
    out = ref.denoise_var(col.reshape(-1, 3), np.full(w * h, 12.0, F32), w, h, levels=1, sigma_var=BIG,
                          sigma_depth=1.0).reshape(h, w, 3)
    S = [11 / 16, 15 / 16, 1.0, 15 / 16, 11 / 16]
    b = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    for y in range(h):
        for x in range(w):
            want = F32(b[y] * b[x]) / F32(S[y] * S[x])
            assert (out[y, x] == want).all(), (x, y, out[y, x], want)
    assert out[2, 2, 0] == F32(9 / 64) and out[2, 1, 0] == F32(0.1) and out[0, 0, 0] == F32(1.0) / F32(121.0)


def test_the_variance_is_carried_with_the_squared_weights():
    """5x5, colour (5/64, 5/64, 5/64), e = 2, no albedo: 2^-6 + ((5/64 + 5/64) + 5/64) = 1/4, d = 2 * 1/2 = 1, t_c = 1 and
    Vraw = 3 everywhere.  The prefilter gives (3 * gsum) / gsum = 3 (exact: g is a power of two).  In level 0 the frame is
    constant, so every tap of the centre pixel (2, 2) is taken with w = h, wsum = 1, and
        V_1(2, 2) = 3 * sum of h^2 / (1 * 1),  sum of h^2 = (sum of B[|d|]^2)^2 = ((1 + 16 + 36 + 16 + 1) / 256)^2 = (70/256)^2
    = 3 * 4900 / 65536 = 14700 / 65536: every partial sum is a multiple of 3 / 65536 below 2^24 of them, hence exact.
    The corner (0, 0) takes 9 taps: wsum = (11/16)^2 = 121/256, vs = 3 * ((36 + 16 + 1) / 256)^2 = 3 * 2809 / 65536, and
    V_1 = vs / (wsum * wsum), two correctly rounded operations on exact numbers."""
    w = h = 5
    col = np.full((w * h, 3), 5 / 64, F32)
    u, V = ref.denoise_var(col, np.full(w * h, 2.0, F32), w, h, levels=1, sigma_var=1.0, sigma_depth=1.0,
                           return_variance=True)
    assert u.tobytes() == col.tobytes()
    V = V.reshape(h, w)
    assert V[2, 2] == F32(14700 / 65536)
    ws = F32(121 / 256)
    assert V[0, 0] == F32(3 * 2809 / 65536) / F32(ws * ws)
    assert (V < F32(3.0)).all()  # filtering only ever lowers it


def _halves(w, h):
    left = np.zeros((h, w), bool)
    left[:, : w // 2] = True
    left = left.reshape(-1)
    col = np.where(left[:, None], F32(0.25), F32(0.75)).astype(F32)
    return left, np.ascontiguousarray(np.broadcast_to(col, (w * h, 3)))


def test_a_hit_miss_boundary_is_not_crossed():
    w, h = 12, 6
    left, col = _halves(w, h)
    e = np.full(w * h, 12.0, F32)
    dep = np.where(left, F32(1.0), F32(np.inf)).astype(F32)
    for levels in (1, 3, 5):
        out = ref.denoise_var(col, e, w, h, depth=dep, levels=levels, sigma_var=BIG, sigma_depth=1.0)
        assert out.tobytes() == col.tobytes()
    out = ref.denoise_var(col, e, w, h, levels=1, sigma_var=BIG, sigma_depth=1.0)
    assert out.tobytes() != col.tobytes()


def test_normals_at_right_angles_do_not_blend():
    w, h = 12, 6
    left, col = _halves(w, h)
    e = np.full(w * h, 12.0, F32)
    nrm = np.where(left[:, None], np.array([1, 0, 0], F32), np.array([0, 1, 0], F32)).astype(F32)
    dep = np.full(w * h, 1.0, F32)
    for levels in (1, 3, 5):
        out = ref.denoise_var(col, e, w, h, normal=nrm, depth=dep, levels=levels, sigma_var=BIG, sigma_depth=1.0)
        assert out.tobytes() == col.tobytes()  # wn = 0 exactly: the other side adds u * 0
    out = ref.denoise_var(col, e, w, h, depth=dep, levels=1, sigma_var=BIG, sigma_depth=1.0)
    assert out.tobytes() != col.tobytes()


def test_no_estimate_is_the_largest_estimate():
    """+inf ("no estimate"), NaN and anything from 12 on give the bytes of 12; a negative estimate and -0.0 those of 0."""
    w, h = 13, 9
    rng = np.random.default_rng(7)
    col = rng.random((w * h, 3), dtype=F32)
    alb = (rng.random((w * h, 3), dtype=F32) * F32(0.9) + F32(0.05)).astype(F32)
    base = (rng.random(w * h, dtype=F32) * F32(0.5)).astype(F32)
    pick = rng.random(w * h) < 0.3
    want = ref.denoise_var(col, np.where(pick, F32(12.0), base), w, h, alb, levels=3, sigma_var=1.0, sigma_depth=1.0)
    for v in (np.inf, np.nan, 13.0, 3.0e38):
        got = ref.denoise_var(col, np.where(pick, F32(v), base), w, h, alb, levels=3, sigma_var=1.0, sigma_depth=1.0)
        assert got.tobytes() == want.tobytes(), v
    assert want.tobytes() != ref.denoise_var(col, base, w, h, alb, levels=3, sigma_var=1.0, sigma_depth=1.0).tobytes()
    zero = ref.denoise_var(col, np.where(pick, F32(0.0), base), w, h, alb, levels=3, sigma_var=1.0, sigma_depth=1.0)
    for v in (-1.0, -0.0, -np.inf):
        got = ref.denoise_var(col, np.where(pick, F32(v), base), w, h, alb, levels=3, sigma_var=1.0, sigma_depth=1.0)
        assert got.tobytes() == zero.tobytes(), v


# --------------------------------------------------------------------------------------------------- the CPU study
def cell_ratios(cell, levels, sigma_var, sigma_depth):
    """(guided ratio, pt_ctx_denoise's ratio at its defaults) of one (scene, n) cell"""
    noisy, e, albedo, normal, depth, conv = inp.inputs(*cell)
    base = inp.rmse(noisy, conv)
    out = ref.denoise_var(noisy, e, inp.W, inp.H, albedo, normal, depth, levels, sigma_var, sigma_depth)
    flv, fsc, fsd = denoise_ref.defaults(ptlib.product())
    fixed = denoise_ref.denoise(noisy, inp.W, inp.H, albedo, normal, depth, flv, fsc, fsd)
    return inp.rmse(out, conv) / base, inp.rmse(fixed, conv) / base


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: "%s_%d" % c)
def test_cpu_study_quality(cell):
    key = "%s_%d" % cell
    levels, sigma_var, sigma_depth = ref.defaults(_lib())
    guided, fixed = cell_ratios(cell, levels, sigma_var, sigma_depth)
    recorded = STUDY["chosen"]["ratio"][key]
    print("%s: guided ratio %.4f (recorded %.4f, bound %.4f), pt_ctx_denoise %.4f (recorded %.4f)"
          % (key, guided, recorded, 1.15 * recorded, fixed, STUDY["pt_ctx_denoise_defaults"][key]))
    assert guided <= 1.15 * recorded, (key, guided, recorded)
    if cell[1] == 256:
        assert guided < 1.0, (key, guided)
        assert guided < fixed, (key, guided, fixed)
