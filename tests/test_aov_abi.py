"""First-hit AOVs (pt_ctx_render_aov) and the PFM writer (pt_write_pfm) at the ABI, without a device: the header declares
them, the Rust shim and the Python binding bind them, the library exports them, NULL arguments are refused before any device
is touched, and pt_write_pfm writes the stated bytes, placed over pt_write_ppm's image pixel for pixel.  The GPU side is
tests/test_gpu_aov.py."""
import ctypes as C
import importlib
import os
import re
import struct
import subprocess

import numpy as np

import ptlib

ROOT = ptlib.ROOT
PT_ERR_INVALID, PT_ERR_IO = ptlib.abi.PT_ERR_INVALID, ptlib.abi.PT_ERR_IO
NAMES = ("pt_ctx_render_aov", "pt_write_pfm")
# parameter kinds, p = pointer, i = integer (the header's declarations, in order)
KINDS = {"pt_ctx_render_aov": "ppppppp", "pt_write_pfm": "ppiii"}
W, H = 3, 2


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptrace.h")).read(), flags=re.S)


def _lib():
    L = ptlib.product()
    return L


def _image(channels):
    """A 3x2 frame in framebuffer order whose values are all distinct, and whose pixels stay distinct after the PPM's
    gamma mapping (value v -> a different 0..255 integer per pixel and channel)."""
    n = W * H * channels
    return (np.arange(n, dtype=np.float32) + 1.0) / np.float32(n + 1)


def _write_pfm(L, path, img, channels):
    return L.pt_write_pfm(str(path).encode(), img.ctypes.data_as(C.c_void_p), W, H, channels)


def read_pfm(path):
    """(channels, width, height, rows bottom-up as a (height, width, channels) float32 array)."""
    data = open(path, "rb").read()
    magic, dims, scale, body = data.split(b"\n", 3)
    channels = {b"PF": 3, b"Pf": 1}[magic]
    w, h = (int(v) for v in dims.split())
    assert float(scale) < 0  # little-endian
    return channels, w, h, np.frombuffer(body, dtype="<f4").reshape(h, w, channels)


def test_header_declares_them():
    h = _header()
    for name in NAMES:
        m = re.search(r"\bint %s\((.*?)\);" % name, h, flags=re.S)
        assert m, name
        kinds = "".join("p" if "*" in q else "i" for q in m.group(1).split(","))
        assert kinds == KINDS[name], (name, kinds)
    assert re.search(r"#define PT_ABI_VERSION 5\b", h)


def test_rust_shim_binds_them():
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "ffi", "hip.rs")).read())
    ext = re.search(r'extern "C" \{(.*?)\n\}', rust, flags=re.S).group(1)
    for name in NAMES:
        m = re.search(r"pub fn %s\((.*?)\)\s*->\s*i32;" % name, ext, flags=re.S)
        assert m, name
        params = [q.split(":", 1)[1].strip() for q in m.group(1).split(",") if ":" in q]
        kinds = "".join("p" if t.startswith("*") else "i" for t in params)
        assert kinds == KINDS[name], (name, kinds)


def test_library_exports_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", ptlib.PRODUCT_SO], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= exported


def test_python_binding_offers_them():
    pkg = importlib.import_module("path-tracer-rust_amd")
    L = pkg.lib()
    for name in NAMES:
        assert getattr(L, name).argtypes is not None, name
    assert callable(getattr(pkg.Context, "render_aov", None))
    assert callable(getattr(pkg, "write_pfm", None))


def test_null_arguments_are_refused_without_a_device():
    L = _lib()
    cfg = ptlib.PtConfig(8, 8, 4, 0, 1, 0, 0, 0, 0)
    buf = C.c_void_p(16)
    assert L.pt_ctx_render_aov(None, C.byref(cfg), buf, buf, buf, buf, None) == PT_ERR_INVALID
    assert L.pt_ctx_render_aov(None, None, None, None, None, None, None) == PT_ERR_INVALID


def test_pfm_bytes_three_channels(tmp_path):
    L = _lib()
    img = _image(3)
    p = tmp_path / "a.pfm"
    assert _write_pfm(L, p, img, 3) == 0, L.pt_last_error()
    fb = img.reshape(W * H, 3)
    # PFM row q from the bottom, column c = framebuffer index q*W + (W-1-c)
    body = b"".join(struct.pack("<3f", *fb[q * W + (W - 1 - c)]) for q in range(H) for c in range(W))
    assert open(p, "rb").read() == b"PF\n3 2\n-1.0\n" + body


def test_pfm_bytes_one_channel(tmp_path):
    L = _lib()
    img = _image(1)
    p = tmp_path / "d.pfm"
    assert _write_pfm(L, p, img, 1) == 0, L.pt_last_error()
    body = b"".join(struct.pack("<f", img[q * W + (W - 1 - c)]) for q in range(H) for c in range(W))
    assert open(p, "rb").read() == b"Pf\n3 2\n-1.0\n" + body
    # special values pass through unchanged (depth holds +inf on a miss, the id map -1)
    img2 = np.array([np.inf, -1.0, 0.0, -0.0, 2.5, 1e30], dtype=np.float32)
    assert _write_pfm(L, p, img2, 1) == 0
    _, _, _, rows = read_pfm(p)
    got = rows[:, ::-1, 0].reshape(-1)  # bottom-up rows, columns reversed back = framebuffer order
    assert got.tobytes() == img2.tobytes()


def test_pfm_lies_over_the_ppm(tmp_path):
    """The same frame through pt_write_ppm and pt_write_pfm: the PFM's pixels, gamma-mapped, are the PPM's pixels."""
    L = _lib()
    img = _image(3)
    ppm, pfm = tmp_path / "f.ppm", tmp_path / "f.pfm"
    assert L.pt_write_ppm(str(ppm).encode(), img.ctypes.data_as(C.c_void_p), W, H, 1, b"t", 0) == 0
    assert _write_pfm(L, pfm, img, 3) == 0
    text = open(ppm).read()
    head, vals = text.split("255\n", 1)
    assert head.split("\n")[3] == "%d %d" % (W, H)
    ppm_px = np.array(vals.split(), dtype=np.int64).reshape(H, W, 3)  # rows from the top
    ch, w, h, rows = read_pfm(pfm)
    assert (ch, w, h) == (3, W, H)
    top_down = rows[::-1]
    mapped = np.array([[[L.pt_to_int_with_gamma_correction(float(v)) for v in px] for px in row] for row in top_down])
    assert len({tuple(px) for px in ppm_px.reshape(-1, 3)}) == W * H  # every pixel distinct: a misplacement shows
    assert (mapped == ppm_px).all(), (mapped, ppm_px)


def test_pfm_errors(tmp_path):
    L = _lib()
    img = _image(3)
    for bad in (0, 2, 4):
        assert _write_pfm(L, tmp_path / "x.pfm", img, bad) == PT_ERR_INVALID, bad
    assert not (tmp_path / "x.pfm").exists()
    assert _write_pfm(L, tmp_path / "no-such-dir" / "x.pfm", img, 3) == PT_ERR_IO
    assert L.pt_write_pfm(str(tmp_path / "x.pfm").encode(), None, W, H, 3) == PT_ERR_INVALID
    assert L.pt_write_pfm(None, img.ctypes.data_as(C.c_void_p), W, H, 3) == PT_ERR_INVALID


def test_python_write_pfm(tmp_path):
    pkg = importlib.import_module("path-tracer-rust_amd")
    L = _lib()
    img = _image(3)
    pkg.write_pfm(str(tmp_path / "py.pfm"), img.reshape(H, W, 3))
    assert _write_pfm(L, tmp_path / "c.pfm", img, 3) == 0
    assert open(tmp_path / "py.pfm", "rb").read() == open(tmp_path / "c.pfm", "rb").read()
    d = _image(1)
    pkg.write_pfm(str(tmp_path / "py1.pfm"), d.reshape(H, W))
    assert _write_pfm(L, tmp_path / "c1.pfm", d, 1) == 0
    assert open(tmp_path / "py1.pfm", "rb").read() == open(tmp_path / "c1.pfm", "rb").read()
