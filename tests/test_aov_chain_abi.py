"""AOVs through mirror and glass surfaces (pt_ctx_render_aov_ex, pt_aov_defaults) at the ABI, without a device: the header
declares them, the Rust shim and the Python binding mirror them, the library exports them; every refusal the call makes before
it looks at the context is exercised with a NULL context; the Python wrapper hands its arguments on; the command line refuses a
bad --aov-chain K.  The restatement's own statistics on the test scenes are held to the counts the GPU tests rest on.  The GPU
side is tests/test_gpu_aov_chain.py."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest

import ptlib
from ptlib import PtAovParams

ROOT = ptlib.ROOT
PT_ERR_INVALID = ptlib.abi.PT_ERR_INVALID
THROUGH_DELTA, MAX_CHAIN = ptlib.abi.PT_AOV_THROUGH_DELTA, ptlib.abi.PT_AOV_MAX_CHAIN
KINDS = {"pt_aov_defaults": "p", "pt_ctx_render_aov_ex": "ppppppppp"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptrace.h")).read(), flags=re.S)


def _lib():
    L = ptlib.product()
    return L


def test_header_declares_them():
    h = _header()
    for name, want in KINDS.items():
        m = re.search(r"\bint %s\((.*?)\);" % name, h, flags=re.S)
        assert m, name
        assert "".join("p" if "*" in q else "i" for q in m.group(1).split(",")) == want, name
    assert re.search(r"#define PT_AOV_THROUGH_DELTA 1u\b", h) and re.search(r"#define PT_AOV_MAX_CHAIN 16u\b", h)
    body = re.search(r"typedef struct pt_aov_params \{(.*?)\} pt_aov_params;", h, flags=re.S).group(1)
    assert re.findall(r"\buint32_t\s+(\w+)", body) == ["flags", "max_chain"]
    assert re.search(r"#define PT_ABI_VERSION 5\b", h)  # symbols were added, nothing changed
    # the plain call's declaration is as it was
    assert re.search(r"int pt_ctx_render_aov\(pt_ctx \*ctx, const pt_config \*cfg, float \*d_albedo, float \*d_normal, float \*d_depth,"
                     r"\s+int32_t \*d_object_id, void \*hip_stream\);", h)


def test_rust_shim_binds_them():
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "ffi", "hip.rs")).read())
    ext = re.search(r'extern "C" \{(.*?)\n\}', rust, flags=re.S).group(1)
    for name, want in KINDS.items():
        m = re.search(r"pub fn %s\((.*?)\)\s*->\s*i32;" % name, ext, flags=re.S)
        assert m, name
        params = [q.split(":", 1)[1].strip() for q in m.group(1).split(",") if ":" in q]
        assert "".join("p" if t.startswith("*") else "i" for t in params) == want, name
    body = re.search(r"pub struct PtAovParams \{(.*?)\n\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): u32", body) == ["flags", "max_chain"]
    assert re.search(r"pub const PT_AOV_THROUGH_DELTA: u32 = 1;", rust) and re.search(r"pub const PT_AOV_MAX_CHAIN: u32 = 16;", rust)


def test_library_exports_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", ptlib.PRODUCT_SO], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(KINDS) <= exported


def test_struct_size_and_defaults():
    L = _lib()
    pkg = importlib.import_module("path-tracer-rust_amd")
    assert C.sizeof(PtAovParams) == 8 == C.sizeof(pkg.pt_aov_params)
    p = PtAovParams(77, 99)
    assert L.pt_aov_defaults(C.byref(p)) == 0
    # a through-delta call with every default written out: a set the call accepts as it stands
    assert (p.flags, p.max_chain) == (THROUGH_DELTA, 8)
    assert L.pt_aov_defaults(None) == PT_ERR_INVALID
    assert pkg.aov_defaults() == {"through_delta": True, "max_chain": 8}
    assert (pkg.PT_AOV_THROUGH_DELTA, pkg.PT_AOV_MAX_CHAIN) == (THROUGH_DELTA, MAX_CHAIN)


def _refusal(L, params, outputs=True, cfg=True):
    """the call with a NULL context: its return code and the reason it gave"""
    c = ptlib.PtConfig(8, 8, 4, 0, 1, 0, 0, 0, 0)
    buf = C.c_void_p(16) if outputs else None
    rc = L.pt_ctx_render_aov_ex(None, C.byref(c) if cfg else None, C.byref(params) if params is not None else None,
                                buf, buf, buf, buf, buf, None)
    return rc, L.pt_last_error().decode()


def test_refusals_before_the_context_is_looked_at():
    L = _lib()
    on = PtAovParams(THROUGH_DELTA, 0)
    # each case breaks the rules BEHIND its own as well (a NULL context at least): the reason names the first one broken
    cases = [(PtAovParams(2, MAX_CHAIN + 1), True, "unknown bits"),
             (PtAovParams(0x80000001, 0), True, "unknown bits"),
             (PtAovParams(0, MAX_CHAIN + 1), False, "exceeds PT_AOV_MAX_CHAIN"),
             (PtAovParams(THROUGH_DELTA, MAX_CHAIN + 1), False, "exceeds PT_AOV_MAX_CHAIN"),
             (PtAovParams(0, 1), False, "without PT_AOV_THROUGH_DELTA"),
             (PtAovParams(0, MAX_CHAIN), False, "without PT_AOV_THROUGH_DELTA"),
             (on, False, "every output is NULL"),
             (None, False, "every output is NULL"),
             (PtAovParams(0, 0), False, "every output is NULL")]
    for params, outputs, why in cases:
        rc, msg = _refusal(L, params, outputs)
        assert rc == PT_ERR_INVALID and why in msg, (params and (params.flags, params.max_chain), msg)
    # past those four: the NULL context (and a NULL cfg) like the plain call
    for params in (on, None, PtAovParams(THROUGH_DELTA, MAX_CHAIN)):
        rc, msg = _refusal(L, params)
        assert rc == PT_ERR_INVALID and "NULL argument" in msg, msg
    rc, msg = _refusal(L, on, cfg=False)
    assert rc == PT_ERR_INVALID and "NULL argument" in msg, msg


def test_python_wrapper_hands_its_arguments_on():
    pkg = importlib.import_module("path-tracer-rust_amd")
    assert pkg.lib().pt_ctx_render_aov_ex.argtypes is not None and pkg.lib().pt_aov_defaults.argtypes is not None
    ctx = object.__new__(pkg.Context)  # a wrapper around the NULL context: every call is refused, and says at which check
    ctx._h = C.c_void_p()

    def refused(**kw):
        with pytest.raises(pkg.PtraceError) as e:
            ctx.render_aov(8, 8, 4, **kw)
        assert e.value.code == PT_ERR_INVALID
        return str(e.value)

    assert "exceeds PT_AOV_MAX_CHAIN" in refused(depth=16, through_delta=True, max_chain=MAX_CHAIN + 1)
    assert "without PT_AOV_THROUGH_DELTA" in refused(depth=16, max_chain=3)
    assert "every output is NULL" in refused(through_delta=True)
    assert "NULL argument" in refused(through_delta=True, max_chain=MAX_CHAIN, chain=16)  # the chain plane counts as an output
    assert "NULL argument" in refused(chain=16)  # flags 0 through the new call
    assert "NULL argument" in refused(depth=16)  # the plain call
    ctx._h = C.c_void_p()  # (nothing to close)


def test_cli_refuses_a_bad_chain_length(tmp_path):
    cli = os.path.join(ptlib.PKG, "ptrace")
    for bad in ("0", "17", "x", "1.5", "99999999999999999999"):
        r = subprocess.run([cli, "6", "24", "cornell", "--root", ROOT, "--aov", "4", "--aov-chain", bad], cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--aov-chain" in r.stderr, (bad, r.stderr)
    # nothing would read the guides
    r = subprocess.run([cli, "6", "24", "cornell", "--root", ROOT, "--aov-chain"], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "--aov-chain" in r.stderr
    assert not os.listdir(tmp_path)


def test_restatement_statistics_of_the_test_scenes():
    """64x40, seed 8, sample 0: the counts tests/test_gpu_aov_chain.py's preconditions rest on, from the oracle alone"""
    import aov_chain_ref as R
    from gpudev import scene
    from test_gpu_aov import call_pixels

    px = call_pixels(64, 40)
    all_mirror = R.with_reflect(scene("cornell"), lambda i, o: 1 if not any(o.emission) else None)
    st = R.stats(R.chain_record(all_mirror, 64, 40, 8, px, 1))
    assert (st["at_cap"], st["miss_after_delta"], st["lengths"]) == (137, 623, list(range(9))), st
    glass = R.with_reflect(scene("mesh"), lambda i, o: 2 if i == 0 else None)
    st = R.stats(R.chain_record(glass, 64, 40, 8, px, 1))
    assert (st["tir_steps"], st["transmissions"], st["delta_pixels"]) == (39, 298, 116), st
    three = R.with_reflect(scene("three-spheres"), lambda i, o: (1, 2, 1)[i])
    st = R.stats(R.chain_record(three, 64, 40, 8, px, 1))
    assert st["miss_after_delta"] == 153 and st["on_surface_after_delta"] == 0, st
    st = R.stats(R.chain_record(scene("cornell"), 64, 40, 8, px, 1))
    assert st["delta_pixels"] == 203 and st["on_surface_after_delta"] == 203 and st["max_length"] == 2, st  # 7.9 % of 2560
