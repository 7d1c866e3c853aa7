"""The held adaptive frame's surface without a GPU (include/ptrace.h, "the adaptive frame held across calls"): the header's
section, the exports, the bindings, the refusals that come before any device is touched, the pure host function that says which
class of tiles a call takes next (host::AdaptiveSchedule), and the checkpoint codec (host::adckpt_*)."""
import ctypes as C
import importlib
import os
import re
import struct
import subprocess

import adaptive_ref
import ptlib
from ptlib import PtAdaptiveInfo, PtAdaptiveParams, PtAdaptiveStats, PtConfig, PtStats

ROOT = ptlib.ROOT
PT_ERR_INVALID = ptlib.abi.PT_ERR_INVALID
NONE = (1 << 64) - 1  # "no E"
NEW = ("pt_ctx_accumulate_adaptive", "pt_ctx_adaptive_info", "pt_ctx_adaptive_resolve", "pt_ctx_adaptive_reset",
       "pt_ctx_adaptive_save", "pt_ctx_adaptive_load")


# ---- the ABI ---------------------------------------------------------------------------------------------------------

def test_header_declares_them_and_abi_stays_5():
    h = open(os.path.join(ROOT, "include", "ptrace.h")).read()
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"#define PT_ABI_VERSION 5\b", code) and ptlib.product().pt_abi_version() == 5
    body = re.search(r"typedef struct pt_adaptive_info \{(.*?)\} pt_adaptive_info;", code, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == ["tiles", "tiles_open", "tiles_at_cap", "spp_min", "spp_max", "samples", "mean_error"]
    counts = {"pt_ctx_accumulate_adaptive": 12, "pt_ctx_adaptive_info": 4, "pt_ctx_adaptive_resolve": 6, "pt_ctx_adaptive_reset": 1,
              "pt_ctx_adaptive_save": 2, "pt_ctx_adaptive_load": 2}
    for name, n in counts.items():
        m = re.search(r"int %s\((.*?)\);" % name, code, flags=re.S)
        assert m and len(m.group(1).split(",")) == n, name
    for text in ("PTADAPT1", "a tie to A", "kept whole or", "the smallest ladder value > c", "Equality with a from-scratch render",
                 "replaces a\n *   held adaptive frame"):
        assert text in h, text


def test_struct_layout():
    assert C.sizeof(PtAdaptiveInfo) == 40  # five u32, four bytes of padding, a u64 and a double
    assert (PtAdaptiveInfo.tiles_at_cap.offset, PtAdaptiveInfo.spp_max.offset) == (8, 16)
    assert (PtAdaptiveInfo.samples.offset, PtAdaptiveInfo.mean_error.offset) == (24, 32)


def test_library_exports_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", ptlib.PRODUCT_SO], text=True)
    assert set(NEW) <= {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_rust_shim_and_python_binding_follow_the_header():
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "ffi", "hip.rs")).read())
    body = re.search(r"pub struct PtAdaptiveInfo \{(.*?)\n\}", rust, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", body) == [("tiles", "u32"), ("tiles_open", "u32"), ("tiles_at_cap", "u32"),
                                                      ("spp_min", "u32"), ("spp_max", "u32"), ("samples", "u64"), ("mean_error", "f64")]
    ext = re.search(r'extern "C" \{(.*?)\n\}', rust, flags=re.S).group(1)
    for name in NEW:
        assert re.search(r"pub fn %s\(" % name, ext), name
    pkg = importlib.import_module("path-tracer-rust_amd")
    L = pkg.lib()
    assert C.sizeof(pkg.pt_adaptive_info) == C.sizeof(PtAdaptiveInfo)
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name
    for name in ("accumulate_adaptive", "adaptive_info", "adaptive_resolve", "adaptive_reset", "adaptive_save", "adaptive_load"):
        assert callable(getattr(pkg.Context, name, None)), name


def test_refusals_come_in_the_stated_order_without_a_device():
    L = ptlib.product()
    cfg = PtConfig(64, 40, 256, 0, 1, 0, 0, 0, 0)
    buf = C.c_void_p(256)  # never dereferenced: every call below is refused before a device is touched
    st, ast, info = PtStats(), PtAdaptiveStats(), PtAdaptiveInfo()
    ctx = C.c_void_p(0)    # there is no context without a device

    def call(par, cfg_=cfg, out=buf, astats=ast):
        rc = L.pt_ctx_accumulate_adaptive(ctx, C.byref(cfg_) if cfg_ is not None else None, C.byref(par) if par is not None else None,
                                          out, None, None, None, None, None, None, C.byref(st),
                                          C.byref(astats) if astats is not None else None)
        return rc, L.pt_last_error().decode()

    def ask(par, cfg_=cfg, out=info):
        rc = L.pt_ctx_adaptive_info(ctx, C.byref(cfg_) if cfg_ is not None else None, C.byref(par) if par is not None else None,
                                    C.byref(out) if out is not None else None)
        return rc, L.pt_last_error().decode()

    good = PtAdaptiveParams(0.08, 8, 0)
    # pt_ctx_render_adaptive's, in its order: the NULLs, tile_error, the tile, the context
    for kw in (dict(par=None), dict(par=good, cfg_=None), dict(par=good, out=None), dict(par=good, astats=None)):
        rc, msg = call(**kw)
        assert rc == PT_ERR_INVALID and "NULL" in msg, (kw, msg)
    for kw in (dict(par=None), dict(par=good, cfg_=None), dict(par=good, out=None)):
        rc, msg = ask(**kw)
        assert rc == PT_ERR_INVALID and "NULL" in msg, (kw, msg)
    for f in (call, ask):
        for v in (-0.5, float("inf"), float("nan")):
            rc, msg = f(PtAdaptiveParams(v, 7, 0))
            assert rc == PT_ERR_INVALID and "tile_error" in msg, (v, msg)
        for v in (1, 7, 12, 64):
            rc, msg = f(PtAdaptiveParams(0.0, v, 0))
            assert rc == PT_ERR_INVALID and "tile must be" in msg, (v, msg)
        for v in (0, 4, 8, 16, 32):
            rc, msg = f(PtAdaptiveParams(0.08, v, 0))
            assert rc == PT_ERR_INVALID and "ctx" in msg, (v, msg)
    assert L.pt_ctx_adaptive_resolve(ctx, C.byref(cfg), buf, None, None, None) == PT_ERR_INVALID
    assert L.pt_ctx_adaptive_reset(ctx) == PT_ERR_INVALID
    assert L.pt_ctx_adaptive_save(ctx, b"x") == PT_ERR_INVALID and L.pt_ctx_adaptive_load(ctx, b"x") == PT_ERR_INVALID


# ---- which class is next ---------------------------------------------------------------------------------------------

def _steps(out):
    keys = ("c", "na", "n", "T", "m", "runs", "to_a0", "to_a1", "na_end")
    rows = []
    for line in out.splitlines():
        if line.startswith("step"):
            rows.append(dict(zip(keys, [int(v) for v in re.findall(r"-?\d+", line)])))
    ends = [tuple(int(v) for v in re.findall(r"\d+", line)) for line in out.splitlines() if line.startswith("open")]
    return rows, ends


def test_class_scheduler():
    tool = ptlib.host_program("adaptive_schedule_probe")
    zero = ["0:0:-"] * 6  # 12 x 8 pixels in tiles of 4: 3 x 2 tiles

    def run(q, cap, n0, tiles, closes="-", width=12, rows=8, shift=2):
        return _steps(tool(q, cap, n0, width, rows, shift, closes, *tiles))

    # from zero it is pt_ctx_render_adaptive's level sequence and halves, whatever the cap
    for min_spp, cap in ((0, 256), (9, 44), (16, 3), (64, 40), (0, 5), (24, 1000)):
        n0 = (min_spp or 16) + 7 & ~7
        steps, ends = run(0, cap, n0, zero)
        lv = adaptive_ref.levels(min_spp, cap)
        assert [s["T"] for s in steps] == lv, (min_spp, cap)
        assert [(s["na_end"], s["T"] - s["na_end"]) for s in steps] == adaptive_ref.halves(lv)
        assert all(s["n"] == 6 and s["to_a0"] == 1 and s["to_a1"] == 0 for s in steps)
        assert [s["c"] for s in steps] == [0] + lv[:-1] and ends == [(6, 0), (6, 6)]
    # tiles that close leave; the rest go on together; nothing open ends the call
    steps, ends = run(0, 256, 16, zero, closes="2,0,4")
    assert [(s["T"], s["n"]) for s in steps] == [(16, 6), (32, 4), (64, 4)] and ends[-1] == (0, 0)
    # mixed counts: ascending c, then ascending nA; classes that reach the same (c, nA) merge; a closed tile is never taken
    q = 10
    tiles = ["32:16:999", "16:8:999", "32:12:999", "16:8:%d" % (q * 16), "16:8:999", "64:32:999"]  # tile 3 is AT the threshold: closed
    steps, ends = run(q, 64, 16, tiles)
    assert [(s["c"], s["na"], s["n"], s["T"]) for s in steps] == [(16, 8, 2, 32), (32, 12, 1, 64), (32, 16, 3, 64)]
    assert steps[1]["to_a0"] == 1 and steps[1]["na_end"] == 12 + 16  # 12 <= 20: run one to A, then 28 > 20: run two to B
    assert ends == [(5, 1), (5, 5)]
    # the same table under a larger q closes everything without a step; under q = 0 the tile at the threshold reopens
    assert run(1000, 64, 16, tiles) == ([], [(0, 0), (0, 0)])
    assert run(0, 64, 16, tiles)[1][0] == (6, 1)
    # a partial tile's threshold counts its pixels inside the band: 10 x 6 in tiles of 4, the corner tile has 2 x 2
    part = ["16:8:999"] * 5 + ["16:8:%d" % (q * 4)]
    assert run(q, 16, 16, part, width=10, rows=6)[1][0] == (5, 5)
    assert run(q, 16, 16, ["16:8:999"] * 5 + ["16:8:%d" % (q * 4 + 1)], width=10, rows=6)[1][0] == (6, 6)
    # a tile at the cap, or beyond it, is skipped and counted; a cap below what is held is no error
    steps, ends = run(0, 32, 16, ["32:16:5", "16:8:5", "64:32:5", "32:16:5", "32:16:5", "32:16:5"])
    assert [(s["c"], s["n"], s["T"]) for s in steps] == [(16, 1, 32)] and ends == [(6, 5), (6, 6)]
    # off the ladder: 100 -> 128.  A tile brought to a cap of 100 holds (52, 48); 16 go to B, the half with fewer, then 12 to A
    steps, _ = run(0, 256, 16, ["100:52:5"] * 6)
    assert steps[0] == dict(c=100, na=52, n=6, T=128, m=116, runs=2, to_a0=0, to_a1=1, na_end=64)
    assert [(s["T"], s["na_end"]) for s in steps] == [(128, 64), (256, 128)]
    assert adaptive_ref.halves([16, 32, 64, 100])[-1] == (52, 48)
    # a cap below n_0 is the first count; the next call leaves it for the ladder
    steps, _ = run(0, 5, 16, zero)
    assert [(s["T"], s["m"], s["na_end"]) for s in steps] == [(5, 4, 4)]
    steps, _ = run(0, 40, 16, ["5:4:5"] * 6)
    assert [(s["c"], s["T"], s["m"], s["to_a0"], s["to_a1"], s["na_end"]) for s in steps] == [(5, 16, 13, 0, 1, 7), (16, 32, 24, 1, 0, 15),
                                                                                             (32, 40, 36, 1, 0, 19)]
    # nothing wraps near 2^31: the ladder value above c does not fit 32 bits, the cap is the next count
    big, cap = (1 << 31) + 8, 0xfffffff0
    steps, _ = run(0, cap, 1 << 30, ["%d:%d:5" % (big, 1 << 30)] * 6)
    assert len(steps) == 1 and steps[0]["T"] == cap and big < steps[0]["m"] < cap
    assert steps[0]["m"] == big + 4 * ((cap - big + 7) // 8)
    steps, _ = run(0, cap, 0xfffffff8, zero)
    assert [(s["c"], s["T"]) for s in steps] == [(0, cap)]


# ---- the checkpoint codec --------------------------------------------------------------------------------------------

def adaptive_checkpoint(L, key, tile, n0, fp, total, table, sums, a, version=1, magic=b"PTADAPT1"):
    """a checkpoint file from the layout include/ptrace.h documents; key as PTACCUM1's; table: (count, nA, E) per tile"""
    b = magic + struct.pack("<I", version) + struct.pack("<7IQ", *key) + struct.pack("<2I", tile, n0) + struct.pack("<Q", fp)
    b += struct.pack("<2I", total, len(table)) + b"".join(struct.pack("<2IQ", *t) for t in table) + sums + a
    return b + struct.pack("<Q", L.pt_siphash(1, 3, 0, 0, b, len(b)))


def parse_adaptive_checkpoint(data):
    """the fields of a file pt_ctx_adaptive_save wrote (the trailing hash is not checked here)"""
    assert data[:8] == b"PTADAPT1"
    version, *key = struct.unpack_from("<I7IQ", data, 8)
    tile, n0, fp, total, tiles = struct.unpack_from("<2IQ2I", data, 48)
    table = [struct.unpack_from("<2IQ", data, 72 + 16 * i) for i in range(tiles)]
    at = 72 + 16 * tiles
    assert len(data) == at + 48 * total + 8
    return dict(version=version, key=tuple(key), tile=tile, n0=n0, fp=fp, total=total, table=table, sums=data[at:at + 24 * total],
                a=data[at + 24 * total:at + 48 * total])


def test_checkpoint_codec(tmp_path):
    import numpy as np
    L = ptlib.product()
    ptlib.host_check("ckpt")  # its own run must pass
    tool = ptlib.host_program("ckpt_check")

    def run(data, *args):
        p = tmp_path / "c.ptad"
        p.write_bytes(data)
        return tool("adaptive", p, *args).strip()

    planes = lambda total, salt: (np.arange(3 * total, dtype="<u8") * np.uint64(0x9e3779b97f4a7c15) + np.uint64(salt)).tobytes()
    # a band of four rows of a 10 x 8 frame in tiles of 4: 3 tiles, the last one 2 wide
    key = (10, 8, 20, 60, 0, 0, 0, 0xfedcba9876543210)
    table = [(32, 16, 12345), (16, 8, NONE), (100, 52, 0)]
    good = adaptive_checkpoint(L, key, 4, 16, 0x1122334455667788, 40, table, planes(40, 1), planes(40, 2))
    assert len(good) == 72 + 16 * 3 + 48 * 40 + 8
    assert run(good) == ("OK key 10 8 20 60 0 0 0 %d tile 4 n0 16 fp %d total 40 tiles 3 sums_at 120 a_at %d table 32:16:12345 16:8:%d "
                         "100:52:0 SAME" % (key[7], 0x1122334455667788, 120 + 960, NONE))
    assert parse_adaptive_checkpoint(good)["table"] == table
    # every truncation and every flip of its lowest and highest bit of every byte is refused, each for a reason of the loader's
    got = {}
    for line in run(good, "sweep").splitlines():
        kind, why, n = line.split("|")
        got.setdefault(kind, {})[why] = int(n)
    assert sum(got["cut"].values()) == len(good) and set(got["cut"]) == {"too short", "truncated"}
    assert sum(got["flip"].values()) == 2 * len(good) and "NOT REFUSED" not in got["flip"]
    assert got["flip"]["bad trailing hash"] >= 2 * (len(good) - 72)  # whatever lies behind the header is the hash's business
    assert set(got["flip"]) <= {"bad trailing hash", "wrong magic", "unknown format version", "the frame key is not a valid frame",
                                "the tile edge or n_0 is not one the call writes", "sizes that do not fit each other", "truncated",
                                "trailing bytes"}

    def resealed(at, fmt, value, data=good):
        b = data[:at] + struct.pack(fmt, value) + data[at + struct.calcsize(fmt):-8]
        return b + struct.pack("<Q", L.pt_siphash(1, 3, 0, 0, b, len(b)))

    for data, why in ((good[:-10], "truncated"), (good + b"\0", "trailing bytes"), (b"", "too short"), (good[:79], "too short"),
                      (b"PTACCUM1" + good[8:], "wrong magic"), (resealed(8, "<I", 2), "unknown format version"),
                      (resealed(12, "<I", 0), "the frame key is not a valid frame"),            # width 0
                      (resealed(20, "<I", 21), "the frame key is not a valid frame"),           # a band that is not whole rows
                      (resealed(36, "<I", 2), "the frame key is not a valid frame"),            # chunks
                      (resealed(48, "<I", 5), "the tile edge or n_0 is not one the call writes"),
                      (resealed(48, "<I", 0), "the tile edge or n_0 is not one the call writes"),
                      (resealed(52, "<I", 12), "the tile edge or n_0 is not one the call writes"),
                      (resealed(52, "<I", 0), "the tile edge or n_0 is not one the call writes"),
                      (resealed(48, "<I", 8), "sizes that do not fit each other"),               # tiles of 8: 2 of them, not 3
                      (resealed(64, "<I", 30), "sizes that do not fit each other"),              # call pixels
                      (resealed(68, "<I", 4), "sizes that do not fit each other"),               # tiles
                      (resealed(72, "<I", (1 << 24) + 1), "a sample count above 2^24"),
                      (resealed(72 + 4, "<I", 33), "half A holds more samples than the tile"),
                      (resealed(72 + 4, "<I", 32), "an E of a tile with an empty half"),        # an E, and nothing in half B
                      (resealed(72 + 4, "<I", 0), "an E of a tile with an empty half")):
        assert run(data) == "BAD " + why, why
    # at the limits: a count of 2^24; a tile without an E may have everything in one half
    assert run(resealed(72, "<I", 1 << 24)).startswith("OK ") and run(resealed(72 + 16 + 4, "<I", 16)).startswith("OK ")
    # the order of the checks: nothing behind the header is looked at before the size fits, and the hash comes before the table
    assert run(resealed(72, "<I", 1 << 25)[:-20]) == "BAD truncated"
    bad = bytearray(resealed(72, "<I", 1 << 25))
    bad[-1] ^= 1
    assert run(bytes(bad)) == "BAD bad trailing hash"
