"""Range counters of a -DPT_RANGE_STATS build of the library (never the shipped one) on one GPU: per call site of
f_sqrt_ranged / normalize_ranged (csrc/pt_device.h), how many arguments a frame evaluated and how many lay outside
[2^-96, largest float] - where the bound in the site's comment would not hold.  Every site must report 0 outside.
  make -C path-tracer-rust_amd range
  PT_LIB=scratch/libptrace_range.so python tools/range_stats.py [scene] [spp] [backend]
Exit status 1 when some site saw an argument outside the range, or no site evaluated anything."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import ptlib
from ptlib import PtConfig, PtStats

L = ptlib.abi.load(os.environ["PT_LIB"])
scene = sys.argv[1] if len(sys.argv) > 1 else "cornell"
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 64
backend = int(sys.argv[3]) if len(sys.argv) > 3 else 0
W, H = 1024, 768
SITES = ["f_sqrt_ranged(1 - r2)", "normalize_ranged(axis x w)", "normalize_ranged(diffuse dir)", "normalize_ranged(tdir)"]
sc = ptlib.load_scene_py(ptlib.scene_path(scene))
ctx = C.c_void_p()
assert L.pt_ctx_create(0, C.byref(ctx)) == 0
assert L.pt_ctx_set_scene(ctx, C.byref(sc.cam), sc.objs, sc.n_objs, sc.tris, sc.n_tris) == 0
cfg = PtConfig(W, H, spp, backend, 1, 0, 0, 512 << 20, 0, 0, 0, 0, 0)
d = C.c_void_p()
assert L.pt_device_malloc(0, W * H * 12, C.byref(d)) == 0
st = PtStats()
assert L.pt_ctx_render(ctx, C.byref(cfg), d, None, None, None, None, C.byref(st)) == 0, L.pt_last_error()
total = [[0, 0] for _ in SITES]
for unit in ("flat", "main", "tile"):
    fn = getattr(L, "pt_debug_range_stats_" + unit)
    out = (C.c_ulonglong * (2 * len(SITES)))()
    assert fn(out, len(out)) == len(SITES)
    for i in range(len(SITES)):
        total[i][0] += out[2 * i]
        total[i][1] += out[2 * i + 1]
    print("unit %-5s %s" % (unit, " ".join("%d/%d" % (out[2 * i + 1], out[2 * i]) for i in range(len(SITES)))))
print("%s %dx%d @%d backend %d: %d bounces" % (scene, W, H, spp, backend, st.ray_bounces))
for name, (n, bad) in zip(SITES, total):
    print("%-32s evaluated %14d   outside [2^-96, max] %d" % (name, n, bad))
sys.exit(1 if any(bad for _, bad in total) or not any(n for n, _ in total) else 0)
