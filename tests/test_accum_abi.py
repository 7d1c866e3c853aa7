"""Progressive accumulation (pt_ctx_accumulate and its four companions) at the ABI, without a device: the header declares
them, the Rust shim and the Python binding bind them, the library exports them, and NULL arguments are refused before any
device is touched.  The GPU side is tests/test_gpu_accumulate.py."""
import ctypes as C
import importlib
import os
import re
import subprocess

import ptlib

ROOT = ptlib.ROOT
PT_ERR_INVALID = ptlib.abi.PT_ERR_INVALID
NAMES = ("pt_ctx_accumulate", "pt_ctx_accum_info", "pt_ctx_accum_reset", "pt_ctx_accum_save", "pt_ctx_accum_load")
# parameter kinds, p = pointer, i = integer (the header's declarations, in order)
KINDS = {"pt_ctx_accumulate": "pppppppp", "pt_ctx_accum_info": "pppp", "pt_ctx_accum_reset": "p",
         "pt_ctx_accum_save": "pp", "pt_ctx_accum_load": "pp"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptrace.h")).read(), flags=re.S)


def _lib():
    L = ptlib.product()
    return L


def test_header_declares_the_accumulate_functions():
    h = _header()
    for name in NAMES:
        m = re.search(r"\bint %s\((.*?)\);" % name, h, flags=re.S)
        assert m, name
        kinds = "".join("p" if "*" in q or q.strip().startswith("pt_progress_fn") else "i" for q in m.group(1).split(","))
        assert kinds == KINDS[name], (name, kinds)
    # the additions are backward compatible: the ABI version stays
    assert re.search(r"#define PT_ABI_VERSION 5\b", h)


def test_rust_shim_binds_them():
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "ffi", "hip.rs")).read())
    ext = re.search(r'extern "C" \{(.*?)\n\}', rust, flags=re.S).group(1)
    for name in NAMES:
        m = re.search(r"pub fn %s\((.*?)\)\s*->\s*i32;" % name, ext, flags=re.S)
        assert m, name
        params = [q.split(":", 1)[1].strip() for q in m.group(1).split(",") if ":" in q]
        kinds = "".join("p" if t.startswith("*") or t.startswith("Option<") else "i" for t in params)
        assert kinds == KINDS[name], (name, kinds)


def test_library_exports_them():
    L = ptlib.product()
    for name in NAMES:
        assert hasattr(L, name), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", ptlib.PRODUCT_SO], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= exported


def test_null_arguments_are_refused_without_a_device():
    L = _lib()
    cfg = ptlib.PtConfig(8, 8, 4, 0, 1, 0, 0, 0, 0)
    st = ptlib.PtStats()
    lo, hi = C.c_uint32(7), C.c_uint32(7)
    assert L.pt_ctx_accumulate(None, C.byref(cfg), C.c_void_p(16), None, None, None, None, C.byref(st)) == PT_ERR_INVALID
    assert L.pt_ctx_accumulate(None, None, None, None, None, None, None, None) == PT_ERR_INVALID
    assert L.pt_ctx_accum_info(None, C.byref(cfg), C.byref(lo), C.byref(hi)) == PT_ERR_INVALID
    assert L.pt_ctx_accum_info(None, None, None, None) == PT_ERR_INVALID
    assert L.pt_ctx_accum_reset(None) == PT_ERR_INVALID
    assert L.pt_ctx_accum_save(None, b"/nonexistent/x.ptacc") == PT_ERR_INVALID
    assert L.pt_ctx_accum_load(None, b"/nonexistent/x.ptacc") == PT_ERR_INVALID
    assert L.pt_ctx_accum_load(None, None) == PT_ERR_INVALID
    assert b"NULL" in L.pt_last_error() or b"ctx" in L.pt_last_error()


def test_python_binding_offers_them():
    pkg = importlib.import_module("path-tracer-rust_amd")
    L = pkg.lib()
    for name in NAMES:
        assert getattr(L, name).argtypes is not None, name
    for meth in ("accumulate", "accum_info", "accum_reset", "accum_save", "accum_load"):
        assert callable(getattr(pkg.Context, meth, None)), meth
    assert (pkg.PT_ERR_IO, pkg.PT_ERR_PARSE) == (-6, -7)


def test_cli_checkpoint_needs_one_gpu(tmp_path):
    """--checkpoint renders through one context: with --gpus 2 the CLI refuses before it looks for a device."""
    cli = os.path.join(ptlib.PKG, "ptrace")
    assert os.path.exists(cli), "the CLI is built by build()"
    r = subprocess.run([cli, "4", "24", "cornell", "--root", ROOT, "--checkpoint", str(tmp_path / "f.ptacc"), "--gpus", "2"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "one GPU" in r.stderr, r.stdout + r.stderr
    assert not (tmp_path / "f.ptacc").exists()
    r = subprocess.run([cli, "4", "24", "cornell", "--root", ROOT, "--checkpoint"], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1 and "--checkpoint FILE" in r.stderr
