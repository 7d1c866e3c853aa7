"""The noise estimate's surface without a GPU: the header's section, the exports, the bindings, the refusals that come before
any device is touched, and the numpy restatement (tests/noise_ref.py) against cases worked by hand."""
import ctypes as C
import importlib
import json
import math
import os
import re
import subprocess

import numpy as np

import noise_ref
import ptlib
from ptlib import PtConfig, PtNoiseStats, PtNoiseTarget, PtStats

ROOT = ptlib.ROOT
PT_ERR_INVALID = ptlib.abi.PT_ERR_INVALID
NAMES = ("pt_ctx_accum_track_noise", "pt_ctx_accum_noise", "pt_ctx_accumulate_until", "pt_noise_stats", "pt_noise_target")
f32 = np.float32


def _header():
    return open(os.path.join(ROOT, "include", "ptrace.h")).read()


def test_header_declares_them_and_abi_stays_5():
    h = _header()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"#define PT_ABI_VERSION 5\b", code)
    for name in NAMES:
        assert re.search(r"\b%s\b" % name, code), name
    body = re.search(r"typedef struct pt_noise_stats \{(.*?)\} pt_noise_stats;", code, flags=re.S).group(1)
    assert re.findall(r"\b(?:float|double|uint32_t|uint64_t)\s+(\w+)", body) == [
        "spp_min", "spp_a_min", "pixels", "mean_error", "histogram"]  # (one declarator per type keyword: spp_max, spp_b_min follow)
    assert "spp_min, spp_max;" in body and "spp_a_min, spp_b_min;" in body and "histogram[64]" in body
    body = re.search(r"typedef struct pt_noise_target \{(.*?)\} pt_noise_target;", code, flags=re.S).group(1)
    assert re.findall(r"\b(?:float|uint32_t)\s+(\w+)", body) == ["mean_error", "quantile", "quantile_error", "min_spp"]
    # the contract is stated: the fixed-point format and why it cannot overflow, the bins, the dependence on history
    for text in ("THE NOISE ESTIMATE", "2^28", "below 2^63", ">> 21", "history"):
        assert text in h, text


def test_struct_sizes_match_the_header_layout():
    assert C.sizeof(PtNoiseStats) == 4 * 4 + 8 + 8 + 64 * 4
    assert PtNoiseStats.pixels.offset == 16 and PtNoiseStats.mean_error.offset == 24 and PtNoiseStats.histogram.offset == 32
    assert C.sizeof(PtNoiseTarget) == 16


def test_library_exports_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", ptlib.PRODUCT_SO], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"pt_ctx_accum_track_noise", "pt_ctx_accum_noise", "pt_ctx_accumulate_until"} <= exported


def test_rust_shim_and_python_binding_offer_them():
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "ffi", "hip.rs")).read())
    body = re.search(r"pub struct PtNoiseStats \{(.*?)\n\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): ([\w\[\]; ]+),", body) == [
        ("spp_min", "u32"), ("spp_max", "u32"), ("spp_a_min", "u32"), ("spp_b_min", "u32"), ("pixels", "u64"),
        ("mean_error", "f64"), ("histogram", "[u32; 64]")]
    body = re.search(r"pub struct PtNoiseTarget \{(.*?)\n\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", body) == [("mean_error", "f32"), ("quantile", "f32"), ("quantile_error", "f32"),
                                                      ("min_spp", "u32")]
    ext = re.search(r'extern "C" \{(.*?)\n\}', rust, flags=re.S).group(1)
    for fn in ("pt_ctx_accum_track_noise", "pt_ctx_accum_noise", "pt_ctx_accumulate_until"):
        assert re.search(r"pub fn %s\(" % fn, ext), fn
    pkg = importlib.import_module("path-tracer-rust_amd")
    L = pkg.lib()
    assert L.pt_ctx_accum_noise.argtypes is not None and L.pt_ctx_accumulate_until.argtypes is not None
    for m in ("accum_track_noise", "accum_noise", "accumulate_until"):
        assert callable(getattr(pkg.Context, m, None)), m
    assert C.sizeof(pkg.pt_noise_stats) == C.sizeof(PtNoiseStats) and C.sizeof(pkg.pt_noise_target) == C.sizeof(PtNoiseTarget)


def test_refusals_without_a_device():
    L = ptlib.product()
    cfg = PtConfig(64, 40, 256, 0, 1, 0, 0, 0, 0)
    buf = C.c_void_p(256)  # never dereferenced: every call below is refused before a device is touched
    ns, st = PtNoiseStats(), PtStats()
    ctx = C.c_void_p(0)  # there is no context without a device

    def until(tgt, cfg_=cfg, out=buf, noise=ns):
        return L.pt_ctx_accumulate_until(ctx, C.byref(cfg_) if cfg_ is not None else None,
                                         C.byref(tgt) if tgt is not None else None, out, None, None, None, None, C.byref(st),
                                         C.byref(noise) if noise is not None else None)

    good = PtNoiseTarget(0.05, 0.0, 0.0, 0)
    assert until(None) == PT_ERR_INVALID and until(good, cfg_=None) == PT_ERR_INVALID
    assert until(good, out=None) == PT_ERR_INVALID and until(good, noise=None) == PT_ERR_INVALID
    bad = {
        "neither criterion": PtNoiseTarget(0.0, 0.0, 0.0, 0),
        "only quantile_error": PtNoiseTarget(0.0, 0.0, 0.5, 0),
        "quantile 1": PtNoiseTarget(0.0, 1.0, 0.1, 0),
        "quantile above 1": PtNoiseTarget(0.05, 1.5, 0.1, 0),
        "negative quantile": PtNoiseTarget(0.05, -0.5, 0.1, 0),
        "negative mean_error": PtNoiseTarget(-0.05, 0.0, 0.0, 0),
        "nan mean_error": PtNoiseTarget(float("nan"), 0.0, 0.0, 0),
        "inf mean_error": PtNoiseTarget(float("inf"), 0.0, 0.0, 0),
        "nan quantile": PtNoiseTarget(0.0, float("nan"), 0.1, 0),
        "negative quantile_error": PtNoiseTarget(0.0, 0.5, -0.1, 0),
        "inf quantile_error": PtNoiseTarget(0.0, 0.5, float("inf"), 0),
    }
    for name, tgt in bad.items():
        assert until(tgt) == PT_ERR_INVALID, name
        assert b"noise target" in L.pt_last_error(), (name, L.pt_last_error())
    # a good target gets as far as the context
    for tgt in (good, PtNoiseTarget(0.0, 0.9, 0.1, 0), PtNoiseTarget(0.05, 0.5, 0.0, 32)):
        assert until(tgt) == PT_ERR_INVALID and b"ctx is NULL" in L.pt_last_error(), L.pt_last_error()
    assert L.pt_ctx_accum_track_noise(None, 1) == PT_ERR_INVALID
    assert L.pt_ctx_accum_noise(None, C.byref(cfg), None, C.byref(ns), None) == PT_ERR_INVALID


def fx(v):
    """a value as a 32.32 sum of one sample"""
    return int(round(v * 2 ** 32))


def test_reference_on_hand_computed_cases():
    # equal halves, 4 + 4 samples, grey pixel: a = 0.5, b = 0.25 in every channel, m = 0.375
    A = np.array([[fx(0.5) * 4]] * 3, dtype=np.uint64)
    H = A + np.uint64(fx(0.25) * 4)
    assert noise_ref.weight(4, 4) == f32(0.5)
    e = noise_ref.error(H, A, 4, 4)
    want = f32(f32(0.75) * f32(0.5)) / np.sqrt(f32(0.015625) + f32(1.125), dtype=f32)  # 0.375 / sqrt(1.140625)
    assert e.dtype == f32 and e[0] == want and abs(float(e[0]) - 0.375 / math.sqrt(1.140625)) < 1e-7
    # a pixel with a = b: e = 0 exactly, the first bin, nothing in the sum
    Hs = np.array([[fx(0.25) * 8]] * 3, dtype=np.uint64)
    As = np.array([[fx(0.25) * 4]] * 3, dtype=np.uint64)
    e0 = noise_ref.error(Hs, As, 4, 4)
    assert e0[0] == f32(0) and noise_ref.bins(e0)[0] == 0 and noise_ref.fixed_sum(e0) == 0
    # unequal halves: nA = 4, nB = 12 -> w = sqrt(48) / 16 in binary32; a = (1, 0, 0), b = (0, 0, 0), m = (0.25, 0, 0)
    w = noise_ref.weight(4, 12)
    assert w == f32(np.sqrt(f32(48), dtype=f32) / f32(16)) and abs(float(w) - math.sqrt(3) / 4) < 1e-7
    A2 = np.array([[fx(1.0) * 4], [0], [0]], dtype=np.uint64)
    e2 = noise_ref.error(A2.copy(), A2, 4, 12)
    assert e2[0] == f32(w / np.sqrt(f32(0.265625), dtype=f32))
    # the clamp: a half whose mean exceeds 1 counts as 1 (a light source), so two saturated halves agree
    A3 = np.array([[fx(3.0) * 4]] * 3, dtype=np.uint64)
    H3 = A3 + np.uint64(fx(7.0) * 4)
    assert noise_ref.error(H3, A3, 4, 4)[0] == f32(0)
    # the largest value: a = 1, b = 0 in every channel at m = 0 cannot happen (m is their mean), but the bound 12 holds
    assert float(noise_ref.error_from_means(np.ones((3, 1)), np.zeros((3, 1)), np.zeros((3, 1)), 0.5)[0]) == 12.0


def test_reference_bins_and_sum():
    e = np.array([0.0, 2.0 ** -13, 2.0 ** -12, 1.25 * 2.0 ** -12, 0.5, 0.75, 1.0, 12.0, 14.0, 100.0], dtype=f32)
    assert noise_ref.bins(e).tolist() == [0, 0, 0, 1, 44, 46, 48, 62, 63, 63]
    assert noise_ref.bin_upper(0) == 1.25 * 2.0 ** -12 and noise_ref.bin_upper(47) == 1.0 and noise_ref.bin_upper(62) == 14.0
    assert noise_ref.bin_upper(63) == float("inf")
    for b in range(1, 63):  # a bin holds [upper(b - 1), upper(b))
        lo, hi = f32(noise_ref.bin_upper(b - 1)), f32(noise_ref.bin_upper(b))
        assert noise_ref.bins(np.array([lo, np.nextafter(hi, f32(0))], dtype=f32)).tolist() == [b, b]
    assert noise_ref.histogram(e).sum() == len(e)
    assert noise_ref.fixed_sum(np.array([0.5, 2.0 ** -28, 2.0 ** -29, 12.0], dtype=f32)) == (1 << 27) + 1 + 0 + 12 * (1 << 28)
    assert noise_ref.mean_error(3 << 28, 2) == 1.5
    assert (1 << 28) * 12 * (1 << 31) < 1 << 63  # the header's overflow argument at pt_ctx_accumulate's largest frame
    # quantiles from a histogram
    hist = np.zeros(64, dtype=np.uint32)
    hist[10], hist[20], hist[30] = 50, 40, 10
    assert noise_ref.quantile_bin(hist, 100, 0.5) == 10 and noise_ref.quantile_bin(hist, 100, 0.51) == 20
    assert noise_ref.quantile_bin(hist, 100, 0.9) == 20 and noise_ref.quantile_bin(hist, 100, 0.95) == 30


def test_checkpoint_parser_on_built_files():
    import struct
    n, parts = 5, 1
    head = b"PTACCUM1" + struct.pack("<I7I2Q3I", 1, 5, 1, 0, 5, 0, 0, 0, 9, 77, n, n, parts)
    sums = np.arange(3 * n, dtype="<u8")
    v1 = head + struct.pack("<I", 6) + sums.tobytes() + b"\0" * 8
    d = noise_ref.parse_checkpoint(v1)
    assert d["version"] == 1 and d["counts"].tolist() == [6] and d["n_a"] is None and d["a"] is None
    assert d["sums"].shape == (3, n) and d["sums"][2, 4] == 14 and d["seed"] == 9 and d["fingerprint"] == 77
    head2 = head[:8] + struct.pack("<I", 2) + head[12:]
    v2 = head2 + struct.pack("<I", 6) + struct.pack("<I", 4) + sums.tobytes() + (sums // 2).astype("<u8").tobytes() + b"\0" * 8
    d = noise_ref.parse_checkpoint(v2)
    assert d["version"] == 2 and d["n_a"].tolist() == [4] and d["a"][2, 4] == 7 and len(v2) == len(v1) + 4 + 24 * n


def test_study_file_holds_the_bounds_the_gpu_tests_use():
    study = json.load(open(os.path.join(ROOT, "profiles", "noise_cpu_study.json")))
    assert study["margin"] == 1.15
    for sid in ("cornell", "mesh"):
        rows, b = study["rows"][sid], study["bounds"][sid]
        assert all(len(rows[n]["estimate"]) >= 8 for n in ("16", "64", "256"))
        assert abs(b["fall_256_over_16"] - max(rows["256"]["estimate"]) / min(rows["16"]["estimate"]) * 1.15) < 1e-12
        for n in ("16", "64", "256"):
            assert abs(b["ratio_lo"][n] - min(rows[n]["ratio"]) / 1.15) < 1e-12
            assert abs(b["ratio_hi"][n] - max(rows[n]["ratio"]) * 1.15) < 1e-12
        assert max(rows["256"]["estimate"]) < b["target"] < min(rows["64"]["estimate"])
