"""pt_ctx_scatter at the ABI, without a device, and the restatement it is held to (tests/kats_scatter.py) on the CPU.

- The header declares the three structs and the function; their sizes; the library exports it; PT_ABI_VERSION is still 5; the
  Rust shim and the Python binding mirror them.
- Every refusal, in the header's order.  The context is checked last, so a NULL context reaches every earlier refusal without a
  device; without a device a call that passes them all returns PT_ERR_NO_DEVICE.
- The constants found by search (kats_scatter.DRAWS) against the restatement's Philox.
- Every edge case's outcome as the restatement reports it, and for every boundary both outcomes among its neighbours.
- `make scatter-check` - the validator under AddressSanitizer and UBSan as a stand-alone program - builds and exits 0.
The GPU side is tests/test_gpu_scatter.py; the restatement against the oracle's paths is in tests/test_oracle.py."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import kats_scatter as ks
import ptlib
from ptlib import PtScatterItem, PtScatterOut, PtScatterSurface
import scatter_walk as sw

ROOT = ptlib.ROOT
PT_ERR_INVALID, PT_ERR_NO_DEVICE = ptlib.abi.PT_ERR_INVALID, ptlib.abi.PT_ERR_NO_DEVICE
NAMES = ["ctx", "seed", "form", "items", "surfaces", "n", "out"]
f32 = np.float32


def _header(strip=True):
    text = open(os.path.join(ROOT, "include", "ptrace.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip else text


@pytest.fixture(scope="module")
def L():
    return ptlib.product()


# ---------------------------------------------------------------------------------------------------------- the ABI
def _fields(h, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, flags=re.S).group(1)
    out = []
    for t, names in re.findall(r"\b(uint32_t|int32_t|float)\s+([^;]+);", body):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", n)
            out.append((t, m.group(1), int(m.group(2) or 1)))
    return out


def test_header_declares_them():
    h = _header()
    for name, cls, size in (("pt_scatter_item", PtScatterItem, 52), ("pt_scatter_surface", PtScatterSurface, 52),
                            ("pt_scatter_out", PtScatterOut, 104)):
        fields = _fields(h, name)
        assert [n for _, n, _ in fields] == [n for n, _ in cls._fields_], name
        assert sum(4 * k for _, _, k in fields) == size == C.sizeof(cls), name
        for (t, n, k), (_, ct) in zip(fields, cls._fields_):
            assert C.sizeof(ct) == 4 * k and (t == "float") == (ct is sw.f3), (name, n)
    m = re.search(r"\bint pt_ctx_scatter\((.*?)\);", h, flags=re.S)
    params = [q.strip() for q in m.group(1).split(",")]
    assert "".join("p" if "*" in q else "i" for q in params) == "piippip"
    assert [q.split()[-1].lstrip("*") for q in params] == NAMES
    for name, value in (("GIVEN", "0u"), ("BY_ID", "1u"), ("BY_RANK", "2u"), ("DEFER_REFRACT", "0x10u"), ("REFRACT_ONLY", "0x20u"),
                        ("NOT_SHADED", "(-2)")):
        assert re.search(r"#define PT_SCATTER_%s %s\n" % (name, re.escape(value)), h), name
    assert re.search(r"#define PT_ABI_VERSION 5\b", h)  # a symbol was added, nothing changed


def test_header_states_the_contract():
    def norm(t):
        return " ".join(t.replace("*", " ").split())

    text = _header(strip=False)
    at = text.index("ONE radiance() invocation after its intersect_scene call")
    doc = norm(text[at:text.index("#define PT_SCATTER_GIVEN", at)])
    for phrase in ("called, not copied", "(branch << 8) | (depth + 1)", "by the routine that fills them for a scene's materials",
                   "Refused for a scene without candidate tables", "comes back `deferred` with no rays",
                   "thr0 = fl(fl(thr * colour') * factor)", "This proves the functions, not each kernel's use of them",
                   "hit = -1 for a miss", "PT_SCATTER_NOT_SHADED"):
        assert norm(phrase) in doc, phrase
    at = doc.index("checked in this order")
    order = ["NULL items or out", "n == 0", "unknown form bits", "without surfaces", "sample >= 2^24", "a reflect type above 2",
             "NULL ctx", "PT_ERR_NO_DEVICE", "without a scene", "without candidate tables"]
    where = [doc.index(p, at) for p in order]
    assert where == sorted(where)


def test_library_exports_it_and_the_abi_version_stays(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", ptlib.PRODUCT_SO], text=True)
    assert "pt_ctx_scatter" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert L.pt_abi_version() == 5


def test_rust_shim_mirrors_it():
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "ffi", "hip.rs")).read())
    for name, cls in (("PtScatterItem", PtScatterItem), ("PtScatterSurface", PtScatterSurface), ("PtScatterOut", PtScatterOut)):
        body = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct %s \{(.*?)\n\}" % name, rust, flags=re.S).group(1)
        got = re.findall(r"pub (\w+): ([^,]+),", body)
        want = [(n, "[f32; 3]" if ct is sw.f3 else ("i32" if ct is C.c_int32 else "u32")) for n, ct in cls._fields_]
        assert got == want, name
    ext = re.search(r'extern "C" \{(.*?)\n\}', rust, flags=re.S).group(1)
    m = re.search(r"pub fn pt_ctx_scatter\((.*?)\)\s*->\s*i32;", ext, flags=re.S)
    params = [(q.split(":", 1)[0].strip(), q.split(":", 1)[1].strip()) for q in m.group(1).split(",") if ":" in q]
    assert [n for n, _ in params] == NAMES
    assert [t for _, t in params] == ["*mut PtCtx", "u64", "u32", "*const PtScatterItem", "*const PtScatterSurface", "u32",
                                      "*mut PtScatterOut"]
    for name, value in (("GIVEN", "0"), ("BY_ID", "1"), ("BY_RANK", "2"), ("DEFER_REFRACT", "0x10"), ("REFRACT_ONLY", "0x20")):
        assert re.search(r"pub const PT_SCATTER_%s: u32 = %s;" % (name, value), rust), name
    assert re.search(r"pub const PT_SCATTER_NOT_SHADED: i32 = -2;", rust)


def test_python_binding_offers_it():
    pkg = importlib.import_module("path-tracer-rust_amd")
    for mine, theirs in ((PtScatterItem, pkg.pt_scatter_item), (PtScatterSurface, pkg.pt_scatter_surface),
                         (PtScatterOut, pkg.pt_scatter_out)):
        assert [n for n, _ in theirs._fields_] == [n for n, _ in mine._fields_] and C.sizeof(theirs) == C.sizeof(mine)
    assert (pkg.PT_SCATTER_GIVEN, pkg.PT_SCATTER_BY_ID, pkg.PT_SCATTER_BY_RANK, pkg.PT_SCATTER_DEFER_REFRACT,
            pkg.PT_SCATTER_REFRACT_ONLY, pkg.PT_SCATTER_NOT_SHADED) == (0, 1, 2, 0x10, 0x20, -2)
    assert callable(pkg.Context.scatter) and len(pkg.lib().pt_ctx_scatter.argtypes) == 7


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_in_order_without_a_device(L):
    """Each call breaks one rule and every rule checked AFTER it: the message names the first.  The context is NULL throughout."""
    good = sw.item((0, 0, 0), (0, 0, -1), (1, 1, 1), 0, 0, 0, 1)
    glass = PtScatterSurface(sw.f3(0, 0, 0), sw.f3(0, 0, 1), sw.f3(1, 1, 1), sw.f3(0, 0, 0), 2)
    matte = PtScatterSurface(sw.f3(0, 0, 0), sw.f3(0, 0, 1), sw.f3(1, 1, 1), sw.f3(0, 0, 0), 0)
    bad_kind = PtScatterSurface(sw.f3(0, 0, 0), sw.f3(0, 0, 1), sw.f3(1, 1, 1), sw.f3(0, 0, 0), 3)
    out = (PtScatterOut * 2)()
    out[0].hit = out[1].hit = 77

    def bad(**kw):
        it = sw.item((0, 0, 0), (0, 0, -1), (1, 1, 1), 0, 0, 0, 1)
        for k, v in kw.items():
            setattr(it, k, v)
        return it

    def call(form, items, surfs, n, o=out):
        ia = (PtScatterItem * len(items))(*items) if items is not None else None
        sa = (PtScatterSurface * len(surfs))(*surfs) if surfs is not None else None
        rc = L.pt_ctx_scatter(None, 1, form, ia, sa, n, o)
        return rc, L.pt_last_error().decode()

    worst = bad(sample=1 << 24, depth=12, branch=0)
    cases = [
        (call(0x40 | 3, None, None, 0), "items or out"),
        (call(0x40 | 3, [worst], None, 0, None), "items or out"),
        (call(0x40 | 3, [worst], None, 0), "n is 0"),
        (call(0x40, [worst], None, 1), "form"),
        (call(0x100, [worst], None, 1), "form"),
        (call(3, [worst], None, 1), "form"),                                   # source 3
        (call(sw.BY_ID | sw.DEFER_REFRACT | sw.REFRACT_ONLY, [worst], None, 1), "form"),  # both modes
        (call(sw.GIVEN, [worst], None, 1), "surfaces is NULL"),
        (call(sw.GIVEN, [bad(sample=1 << 24)], [bad_kind], 1), "sample"),
        (call(sw.GIVEN, [good, bad(depth=12)], [bad_kind, bad_kind], 2), "depth"),
        (call(sw.BY_ID, [bad(branch=0)], None, 1), "branch"),
        (call(sw.BY_RANK, [good, bad(branch=8)], None, 2), "branch"),
        (call(sw.GIVEN, [good], [bad_kind], 1), "reflect type"),
        (call(sw.GIVEN | sw.REFRACT_ONLY, [good, good], [glass, matte], 2), "not Refract"),
        (call(sw.GIVEN | sw.REFRACT_ONLY, [good], [glass], 1), "ctx"),
        (call(sw.GIVEN | sw.DEFER_REFRACT, [good, good], [glass, matte], 2), "ctx"),
        (call(sw.GIVEN, [bad(sample=(1 << 24) - 1, depth=11, branch=7, pixel=0xFFFFFFFF)], [matte], 1), "ctx"),  # the largest allowed
        (call(sw.BY_ID, [good], None, 1), "ctx"),
        (call(sw.BY_RANK | sw.REFRACT_ONLY, [good], None, 1), "ctx"),
    ]
    for i, ((rc, msg), word) in enumerate(cases):
        assert rc == PT_ERR_INVALID and word in msg, (i, rc, msg, word)
    assert out[0].hit == 77 and out[1].hit == 77  # a refused call writes nothing


def test_no_device_is_reported_after_the_arguments(L):
    if L.pt_device_count() > 0:
        pytest.skip("a device is present: the GPU tests run the call")
    items, surfs = sw.case_arrays(ks.CASES[:2])
    out = (PtScatterOut * 2)()
    ctx = C.create_string_buffer(64)  # never dereferenced: the device count is asked first
    assert L.pt_ctx_scatter(C.cast(ctx, C.c_void_p), ks.SEED, sw.GIVEN, items, surfs, 2, out) == PT_ERR_NO_DEVICE


# ------------------------------------------------------------------------------------------ the restatement's own cases
def test_searched_draws_have_the_wanted_bits():
    assert set(ks.DRAWS) == {t[0] for t in ks.DRAW_TARGETS}
    for name, word, k, depth, branch in ks.DRAW_TARGETS:
        pixel, sample = ks.DRAWS[name]
        w = ks.philox4x32([pixel, sample, (branch << 8) | (depth + 1), 0], [ks.SEED & 0xFFFFFFFF, ks.SEED >> 32])
        assert w[word] >> 8 == k, name
        assert ks.draws(ks.SEED, pixel, sample, depth, branch)[word] == f32(k) * f32(2.0 ** -24), name
    assert ks.draws(ks.SEED, *ks.DRAWS["r2_zero"], 0, 1)[2] == 0.0
    assert ks.draws(ks.SEED, *ks.DRAWS["r2_last"], 0, 1)[2] == f32(1.0) - f32(2.0 ** -24)
    # a quarter turn of sinf / cosf changes between k - 1 and k at the odd eighths, and not at the even ones
    for m, k in enumerate(ks.R1_TURNS, 1):
        assert (ks.quadrant(k - 1) != ks.quadrant(k)) == (m % 2 == 1) and ks.quadrant(k) == ks.quadrant(k + 1), m


def _outcome(case, key, want, got):
    if key == "tir":
        return (got["kind"] == "tir") == want
    if key == "branches":
        return tuple(ch[3] for ch in got["children"]) == want
    if key == "draw":
        return ks.draws(ks.SEED, case["pixel"], case["sample"], case["depth"], case["branch"])[want[0]] == f32(want[1]) * f32(2.0 ** -24)
    return got.get(key) == want


def test_every_case_has_the_outcome_it_was_built_for():
    names = [c["name"] for c in ks.CASES]
    assert len(set(names)) == len(names)
    for c in ks.CASES:
        for arr in (c["d"], c["n"], c["color"], c["emission"], c["x"]):
            assert arr.dtype == f32
        got = ks.expected(c)
        for key, want in c["expect"].items():
            assert _outcome(c, key, want, got), (c["name"], key, want, got["kind"], got.get(key))
        for d, w, depth, branch in got["children"]:
            assert d.dtype == f32 and w.dtype == f32 and depth == c["depth"] + 1


def test_every_boundary_shows_both_outcomes():
    """For each boundary the restatement itself reports both outcomes among the case and its neighbours."""
    got = {c["name"]: ks.expected(c) for c in ks.CASES}

    def seen(prefix, key):
        return {str(r.get(key)) for n, r in got.items() if n.startswith(prefix)}

    assert seen("diffuse_wx_+0.1f", "axis") == {"X", "Y"} and seen("diffuse_wx_-0.1f", "axis") == {"X", "Y"}
    assert got["diffuse_wx_+0.1f+0ulp"]["axis"] == "X" and got["diffuse_wx_+0.1f+1ulp"]["axis"] == "Y"
    assert got["diffuse_wx_-0.1f+0ulp"]["axis"] == "X" and got["diffuse_wx_-0.1f-1ulp"]["axis"] == "X"
    assert seen("facing_dot_", "flipped") == {"True", "False"}
    assert got["facing_dot_+0ulp_0"]["flipped"] and not got["facing_dot_-1ulp_0"]["flipped"]
    for depth in (5, 10):
        for ch in range(3):
            assert seen("roulette_draw_eq_max", "alive") == {"True", "False"}
            assert not got["roulette_draw_eq_max+0ulp_ch%d_depth%d" % (ch, depth)]["alive"]
            assert got["roulette_draw_eq_max+1ulp_ch%d_depth%d" % (ch, depth)]["alive"]
    assert {got["roulette_depth%d_1" % d]["alive"] for d in (4, 5, 10, 11)} == {True, False}
    assert got["roulette_depth10_0"]["alive"] and not got["roulette_depth11_0"]["alive"]
    assert {"tir", "split"} <= seen("glass_tir_edge", "kind") <= {"tir", "split", "choice_refl", "choice_trans"}
    assert got["glass_tir_edge-1ulp_depth0"]["kind"] == "tir" and got["glass_tir_edge+0ulp_depth0"]["kind"] == "split"
    assert got["glass_tir_edge+0ulp_depth0"]["cos2t"] >= 0 > got["glass_tir_edge-1ulp_depth0"]["cos2t"]
    assert got["glass_into_depth1"]["kind"] == "split" and got["glass_into_depth2"]["kind"].startswith("choice")
    assert got["glass_choice_eq_p"]["kind"] == "choice_trans" and got["glass_choice_eq_p_prev"]["kind"] == "choice_refl"
    u = ks.draws(ks.SEED, *ks.DRAWS["choice_eq_p"], 2, 1)[1]
    assert u == got["glass_choice_eq_p"]["p"]
    assert [tuple(ch[3] for ch in got["glass_branch%d" % b]["children"]) for b in (1, 2, 3)] == [(2, 3), (4, 5), (6, 7)]
    kinds = {r["kind"] for r in got.values()}
    assert kinds == {"dead", "diffuse", "mirror", "tir", "split", "choice_refl", "choice_trans"}


def test_throughput_contract_reduces_to_the_rust_weights():
    """with thr = (1, 1, 1) the top-down weights are the Rust text's, bit for bit"""
    for c in ks.CASES:
        a, b = ks.expected(c), ks.expected(c, thr=(1, 1, 1))
        assert len(a["children"]) == len(b["children"])
        for (da, wa, _, _), (db, wb, _, _) in zip(a["children"], b["children"]):
            assert da.tobytes() == db.tobytes() and wa.tobytes() == wb.tobytes(), c["name"]
        assert b["contrib"].tobytes() == c["emission"].tobytes()


# -------------------------------------------------------------------------------------------- the stand-alone program
def test_scatter_check_builds_and_passes():
    """`make scatter-check`: the validator and what it hands the kernel, under AddressSanitizer and UBSan as a program of its own"""
    ptlib.host_check("scatter")
