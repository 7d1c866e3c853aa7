"""pt_ctx_denoise at the ABI and its contract, without a device.

- The header declares pt_denoise_params, pt_denoise_defaults and pt_ctx_denoise; the Rust shim mirrors them; the library
  exports them; the Python binding offers them; every invalid argument is refused with PT_ERR_INVALID before a device is
  touched (a NULL context is the LAST thing checked, so each case below is refused for its own reason: the message says so).
- Known answers on tests/denoise_ref.py, the numpy restatement of the header's arithmetic, with values exact in binary32.
- The CPU study as a regression test of the contract's quality: a 16-sample oracle frame of cornell and mesh, denoised by the
  restatement with the library's defaults and the oracle's first-hit guides, must be closer to the oracle's 4096-sample frame
  than R times the noisy frame's distance.  R = 1.15 x the ratio tools/denoise_cpu_study.py measured at the chosen defaults
  (profiles/denoise_cpu_study.json: cornell 0.381820, mesh 0.316506); the frames are deterministic, the 15 % is room for a later
  deliberate change of a constant.
- `make denoise-check` - both filters' refusals, the limits they accept and the levels' schedule against this restatement's
  formula bit for bit, host only under AddressSanitizer and UBSan - builds and passes.
The GPU side is tests/test_gpu_denoise.py."""
import ctypes as C
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref
import ptlib
from ptlib import PtDenoiseParams
from denoise_ref import F32

ROOT = ptlib.ROOT
PT_ERR_INVALID = ptlib.abi.PT_ERR_INVALID
MEASURED = {"cornell": 0.381820, "mesh": 0.316506}  # profiles/denoise_cpu_study.json, "chosen"
R = {sid: 1.15 * v for sid, v in MEASURED.items()}
BIG = float(2.0 ** 16)  # a sigma_color so large that fall(xc) is exactly 1 for colour differences up to 1


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptrace.h")).read(), flags=re.S)


def _lib():
    L = ptlib.product()
    return L


# ---------------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_them():
    h = _header()
    body = re.search(r"typedef struct pt_denoise_params \{(.*?)\} pt_denoise_params;", h, flags=re.S).group(1)
    assert re.findall(r"\b(uint32_t|float)\s+(\w+);", body) == [
        ("uint32_t", "levels"), ("float", "sigma_color"), ("float", "sigma_normal_pow"), ("float", "sigma_depth"),
        ("uint32_t", "flags")]
    assert [(n, t) for n, t in PtDenoiseParams._fields_] == [
        ("levels", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal_pow", C.c_float), ("sigma_depth", C.c_float),
        ("flags", C.c_uint32)]
    m = re.search(r"\bint pt_ctx_denoise\((.*?)\);", h, flags=re.S)
    kinds = "".join("p" if "*" in q else "i" for q in m.group(1).split(","))
    assert kinds == "piippppppp"  # ctx, width, height, params, color, albedo, normal, depth, out, stream
    assert re.search(r"\bint pt_denoise_defaults\(\s*pt_denoise_params \*\w+\);", h)
    assert re.search(r"#define PT_DENOISE_NO_DEMODULATE 1u\b", h)
    assert re.search(r"#define PT_ABI_VERSION 5\b", h)


def test_rust_shim_mirrors_them():
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "ffi", "hip.rs")).read())
    body = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct PtDenoiseParams \{(.*?)\n\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", body) == [("levels", "u32"), ("sigma_color", "f32"), ("sigma_normal_pow", "f32"),
                                                      ("sigma_depth", "f32"), ("flags", "u32")]
    ext = re.search(r'extern "C" \{(.*?)\n\}', rust, flags=re.S).group(1)
    m = re.search(r"pub fn pt_ctx_denoise\((.*?)\)\s*->\s*i32;", ext, flags=re.S)
    params = [q.split(":", 1)[1].strip() for q in m.group(1).split(",") if ":" in q]
    assert "".join("p" if t.startswith("*") else "i" for t in params) == "piippppppp"
    assert params[3] == "*const PtDenoiseParams"
    assert re.search(r"pub fn pt_denoise_defaults\(\s*out: \*mut PtDenoiseParams\s*\)\s*->\s*i32;", ext)


def test_library_exports_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", ptlib.PRODUCT_SO], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"pt_ctx_denoise", "pt_denoise_defaults"} <= exported


def test_python_binding_offers_them():
    pkg = importlib.import_module("path-tracer-rust_amd")
    L = pkg.lib()
    assert L.pt_ctx_denoise.argtypes is not None and L.pt_denoise_defaults.argtypes is not None
    assert callable(getattr(pkg.Context, "denoise", None))
    d = pkg.denoise_defaults()
    lv, sc, sd = denoise_ref.defaults(_lib())
    assert d == {"levels": lv, "sigma_color": sc, "sigma_depth": sd}


def test_defaults():
    L = _lib()
    p = PtDenoiseParams(9, -1.0, 3.0, -1.0, 77)
    assert L.pt_denoise_defaults(C.byref(p)) == 0
    assert p.levels == 5 and p.sigma_normal_pow == 0.0 and p.flags == 0
    assert p.sigma_color > 0 and p.sigma_depth > 0
    assert L.pt_denoise_defaults(None) == PT_ERR_INVALID
    # they are the point the CPU study chose
    study = json.load(open(os.path.join(ROOT, "profiles", "denoise_cpu_study.json")))
    assert (p.sigma_color, p.sigma_depth) == (study["chosen"]["sigma_color"], study["chosen"]["sigma_depth"])
    for sid, v in MEASURED.items():
        assert abs(study["chosen"]["ratio"][sid] - v) < 1e-6


def test_invalid_arguments_are_refused_without_a_device():
    L = _lib()
    buf = C.c_void_p(256)  # never dereferenced: every call below is refused before a device is touched
    nan, inf = float("nan"), float("inf")

    def call(params=None, w=8, h=8, color=buf, out=buf):
        pp = C.byref(PtDenoiseParams(*params)) if params is not None else None
        rc = L.pt_ctx_denoise(None, w, h, pp, color, buf, buf, buf, out, None)
        return rc, L.pt_last_error().decode()

    cases = [
        (dict(params=(9, 0, 0, 0, 0)), "levels"),
        (dict(params=(5, -1.0, 0, 0, 0)), "sigma"),
        (dict(params=(5, nan, 0, 0, 0)), "sigma"),
        (dict(params=(5, inf, 0, 0, 0)), "sigma"),
        (dict(params=(5, 0, 0, -0.5, 0)), "sigma"),
        (dict(params=(5, 0, 0, nan, 0)), "sigma"),
        (dict(params=(5, 0, 0, inf, 0)), "sigma"),
        (dict(params=(5, 0, 1.0, 0, 0)), "sigma_normal_pow"),
        (dict(params=(5, 0, nan, 0, 0)), "sigma_normal_pow"),
        (dict(params=(5, 0, 0, 0, 2)), "flags"),
        (dict(params=(5, 0, 0, 0, 0x80000001)), "flags"),
        (dict(w=0), "width"),
        (dict(h=0), "width"),
        (dict(w=16385, h=16384), "2^28"),
        (dict(w=0xffffffff, h=0xffffffff), "2^28"),
        (dict(color=None), "d_color"),
        (dict(out=None), "d_out"),
        (dict(), "ctx"),                              # everything valid but the context
        (dict(params=(8, 1.0, 0, 1.0, 1)), "ctx"),    # the limits themselves are accepted
        (dict(w=16384, h=16384), "ctx"),
    ]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == PT_ERR_INVALID, (kw, rc)
        assert word in msg, (kw, msg)


# ---------------------------------------------------------------------------------------------------------- make denoise-check
def test_denoise_check_builds_and_passes():
    ptlib.host_check("denoise")


# ------------------------------------------------------------------------------------------- known answers on the rebuild
def test_fall():
    assert denoise_ref.fall(F32(8.0)) == F32(0.0)
    assert denoise_ref.fall(F32(0.0)) == F32(1.0)
    assert denoise_ref.fall(F32(1e9)) == F32(0.0) and denoise_ref.fall(F32(np.nan)) == F32(0.0)
    assert denoise_ref.fall(F32(4.0)) == F32(2.0 ** -8)  # t = 1/2


@pytest.mark.parametrize("levels", range(1, 9))
def test_a_constant_frame_is_a_fixed_point(levels):
    """Colour (1/4, 1/2, 3/4) everywhere: every product with a weight, every partial sum and the quotient are exact."""
    w, h = 7, 5
    col = np.tile(np.array([0.25, 0.5, 0.75], F32), (w * h, 1))
    out = denoise_ref.denoise(col, w, h, levels=levels, sigma_color=1.0, sigma_depth=1.0)
    assert out.tobytes() == col.tobytes()
    alb = np.full((w * h, 3), 0.5, F32)  # u = colour / 0.5 is exact, and so is the way back: (3/4 / 1/2) * 1/2
    nrm = np.tile(np.array([0.0, 0.0, 2.0], F32), (w * h, 1))
    dep = np.full(w * h, 3.0, F32)
    col2 = col * F32(0.5)
    out = denoise_ref.denoise(col2, w, h, alb, nrm, dep, levels=levels, sigma_color=1.0, sigma_depth=1.0)
    assert out.tobytes() == col2.tobytes()


def test_one_bright_pixel_gives_the_renormalised_b_spline():
    """5x5, pixel (2, 2) = 1, the others 0, no guides, one level, sigma_color 2^16: xc <= 2^-32, 1 - xc/8 rounds to 1, fall = 1,
    so every tap inside the frame has w = h = B[|dy|] B[|dx|] and only the tap onto (2, 2) adds anything:
        out(x, y) = B[|2-y|] B[|2-x|] / (S(y) S(x)),   S(c) = sum of B[|d|] over d in -2..2 with 0 <= c + d < 5
        S(2) = 1,  S(1) = S(3) = 1 - 1/16 = 15/16,  S(0) = S(4) = 3/8 + 1/4 + 1/16 = 11/16
        b(c) = B[|2-c|] = 1/16, 1/4, 3/8, 1/4, 1/16   for c = 0..4
    e.g. out(2,2) = 9/64, out(1,2) = (3/32)/(15/16) = 1/10, out(0,0) = (1/256)/(121/256) = 1/121.  Numerator and denominator
    are exact in binary32 (multiples of 1/256 below 1), so each value is ONE correctly rounded division."""
    w = h = 5
    col = np.zeros((h, w, 3), F32)
    col[2, 2] = 1.0
    out = denoise_ref.denoise(col.reshape(-1, 3), w, h, levels=1, sigma_color=BIG, sigma_depth=1.0).reshape(h, w, 3)
    S = [11 / 16, 15 / 16, 1.0, 15 / 16, 11 / 16]
    b = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    for y in range(h):
        for x in range(w):
            want = F32(b[y] * b[x]) / F32(S[y] * S[x])
            assert (out[y, x] == want).all(), (x, y, out[y, x], want)
    assert out[2, 2, 0] == F32(9 / 64) and out[2, 1, 0] == F32(0.1) and out[0, 0, 0] == F32(1.0) / F32(121.0)


def _halves(w, h):
    left = np.zeros((h, w), bool)
    left[:, : w // 2] = True
    left = left.reshape(-1)
    col = np.where(left[:, None], F32(0.25), F32(0.75)).astype(F32)
    return left, np.ascontiguousarray(np.broadcast_to(col, (w * h, 3)))


def test_a_hit_miss_boundary_is_not_crossed():
    w, h = 12, 6
    left, col = _halves(w, h)
    dep = np.where(left, F32(1.0), F32(np.inf)).astype(F32)
    for levels in (1, 3, 5):
        out = denoise_ref.denoise(col, w, h, depth=dep, levels=levels, sigma_color=BIG, sigma_depth=1.0)
        assert out.tobytes() == col.tobytes()
    # the same frame without the depth buffer does blend across the line
    out = denoise_ref.denoise(col, w, h, levels=1, sigma_color=BIG, sigma_depth=1.0)
    assert out.tobytes() != col.tobytes()


def test_normals_at_right_angles_do_not_blend():
    w, h = 12, 6
    left, col = _halves(w, h)
    nrm = np.where(left[:, None], np.array([1, 0, 0], F32), np.array([0, 1, 0], F32)).astype(F32)
    dep = np.full(w * h, 1.0, F32)
    for levels in (1, 3, 5):
        out = denoise_ref.denoise(col, w, h, normal=nrm, depth=dep, levels=levels, sigma_color=BIG, sigma_depth=1.0)
        assert out.tobytes() == col.tobytes()  # wn = 0 exactly: the other side adds u * 0
    out = denoise_ref.denoise(col, w, h, depth=dep, levels=1, sigma_color=BIG, sigma_depth=1.0)
    assert out.tobytes() != col.tobytes()


# --------------------------------------------------------------------------------------------------- the CPU study
def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


@pytest.mark.parametrize("sid", ["cornell", "mesh"])
def test_cpu_study_quality(sid):
    from test_gpu_aov import call_pixels, rebuild

    w, h, spp, seed = 96, 64, 16, 5
    gold = np.load(os.path.join(ROOT, "tests", "golden", "denoise_%s_96x64_4096.npz" % sid))
    assert (int(gold["width"]), int(gold["height"]), int(gold["spp"]), int(gold["seed"])) == (w, h, 4096, seed)
    conv = gold["frame"]
    sc = ptlib.load_scene_py(ptlib.scene_path(sid))
    noisy, _, _ = ptlib.oracle_render(sc, w, h, spp, seed)
    albedo, normal, depth, _ = rebuild(sc, w, h, seed, call_pixels(w, h), spp)
    levels, sigma_color, sigma_depth = denoise_ref.defaults(_lib())
    out = denoise_ref.denoise(noisy, w, h, albedo, normal, depth, levels, sigma_color, sigma_depth)
    e_noisy, e_out = rmse(noisy, conv), rmse(out, conv)
    print("%s: rmse noisy %.5f, denoised %.5f, ratio %.4f, R %.4f" % (sid, e_noisy, e_out, e_out / e_noisy, R[sid]))
    assert e_out <= R[sid] * e_noisy, (sid, e_out / e_noisy, R[sid])
