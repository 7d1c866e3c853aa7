#!/usr/bin/env python3
"""What guides taken THROUGH mirror and glass surfaces (pt_ctx_render_aov_ex, PT_AOV_THROUGH_DELTA) do to the image passes that
read them, against the first-hit guides: the CPU study behind the README's advice on when to switch them on.

cornell at WxH, everything from the oracle and the numpy restatements: frames are oracle renders, first-hit guides are built as
tests/test_gpu_aov.py builds its expectation, chain guides as tests/aov_chain_ref.py (max_chain 8), the filters are
tests/denoise_ref.py, tests/denoise_var_ref.py and tests/upsample_ref.py at the library's defaults.  Truth is the oracle at
TRUTH_SPP samples at full size.  For each seed offset in SEEDS and n in N_SPP, as tools/upsample_cpu_study.py:
  (a) full size at n spp (two oracle frames of n/2 samples: their mean is the frame, their difference its noise map)
      -> pt_ctx_denoise, and -> pt_ctx_denoise_var with that noise map;
  (b) half size at 4n spp (the rays of (a)) -> pt_ctx_upsample -> pt_ctx_denoise;
  (c) half size at n spp -> pt_ctx_upsample -> pt_ctx_denoise
- six rows for pt_ctx_denoise and two for pt_ctx_denoise_var (an upsampled frame has no noise map).  Every row is computed
twice, with all guides (of both sizes) first-hit and with all of them chain guides, and measured as the mean absolute error
against truth over (1) the full-size pixels whose sample 0 hits anything and (2) those whose first hit is a mirror or glass
surface.  Every row is reported, the ones that get worse included.  No GPU is involved.

    python tools/aov_chain_cpu_study.py            # writes profiles/aov_chain_cpu_study.json
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aov_chain_ref as chain  # noqa: E402
import denoise_ref  # noqa: E402
import denoise_var_ref  # noqa: E402
import noise_ref  # noqa: E402
import ptlib  # noqa: E402
import test_gpu_aov as aov  # noqa: E402
import upsample_ref  # noqa: E402

SCENE = "cornell"
W, H = 192, 128
LW, LH = W // 2, H // 2
N_SPP = (8, 2)
SEEDS = (0, 100)
TRUTH_SPP = 2048
MAX_CHAIN = 8
F32 = np.float32


def defaults():
    d = json.load(open(os.path.join(ROOT, "profiles", "denoise_cpu_study.json")))["chosen"]
    v = json.load(open(os.path.join(ROOT, "profiles", "denoise_var_cpu_study.json")))["chosen"]
    u = json.load(open(os.path.join(ROOT, "profiles", "upsample_cpu_study.json")))["chosen"]
    return (dict(levels=5, sigma_color=d["sigma_color"], sigma_depth=d["sigma_depth"]),
            dict(levels=5, sigma_var=v["sigma_var"], sigma_depth=v["sigma_depth"]),
            dict(depth_tol=u["depth_tol"], normal_min=u["normal_min"]))


DENOISE, DENOISE_VAR, UPSAMPLE = defaults()


def guides(sc, w, h, spp, seed):
    """{"first": ..., "chain": ...}: albedo, normal, depth, oid of both kinds for the frame (w, h, seed) over spp samples"""
    px = aov.call_pixels(w, h)
    rays = aov.oracle_rays(sc, w, h, seed, px, spp)
    names = ("albedo", "normal", "depth", "oid")
    first = dict(zip(names, aov.rebuild(sc, w, h, seed, px, spp, rays)))
    rec = chain.chain_record(sc, w, h, seed, px, spp, rays, MAX_CHAIN)
    return {"first": first, "chain": dict(zip(names, chain.planes(rec, spp, MAX_CHAIN)[:4])), "chain_stats": chain.stats(rec, MAX_CHAIN)}


def mae(a, b, mask):
    return float(np.abs(np.asarray(a).reshape(-1, 3)[mask].astype(np.float64) - b[mask]).mean())


def study():
    sc = ptlib.load_scene_py(ptlib.scene_path(SCENE))
    truth = ptlib.oracle_render(sc, W, H, TRUTH_SPP, 1000)[0].reshape(W * H, 3)
    print("truth rendered", flush=True)
    refl = np.array([sc.objs[i].reflect_type for i in range(sc.n_objs)])
    rows = []
    for off in SEEDS:
        for n in N_SPP:
            a_seed, b_seed, c_seed = off + 20 + n, off + 40 + n, off + 60 + n
            halves = [ptlib.oracle_render(sc, W, H, n // 2, s)[0].reshape(W * H, 3).astype(F32) for s in (a_seed, a_seed + 1000)]
            color = (halves[0] + halves[1]) * F32(0.5)
            m = noise_ref.clamp01(color)
            e = noise_ref.error_from_means(halves[0].T, halves[1].T, m.T, F32(0.5))
            full = guides(sc, W, H, n, a_seed)
            oid = full["first"]["oid"]
            masks = {"hit": oid >= 0, "delta": (oid >= 0) & (refl[np.maximum(oid, 0)] != 0)}
            lo = {"b": (ptlib.oracle_render(sc, LW, LH, 4 * n, b_seed)[0], guides(sc, LW, LH, 4 * n, b_seed)),
                  "c": (ptlib.oracle_render(sc, LW, LH, n, c_seed)[0], guides(sc, LW, LH, n, c_seed))}
            print("seed offset %d n %d: frames and guides made; chains %s" % (off, n, full["chain_stats"]), flush=True)

            def measure(name, make):
                row = {"row": name, "n": n, "seed_offset": off, "hit_pixels": int(masks["hit"].sum()),
                       "delta_pixels": int(masks["delta"].sum())}
                for kind in ("first", "chain"):
                    out = make(kind)
                    row[kind] = {k: mae(out, truth, v) for k, v in masks.items()}
                row["chain_over_first"] = {k: row["chain"][k] / row["first"][k] for k in masks}
                rows.append(row)
                print("  %-58s first %.4f (%.4f)  chain %.4f (%.4f)  delta pixels x%.3f  all x%.3f" % (
                    name, row["first"]["delta"], row["first"]["hit"], row["chain"]["delta"], row["chain"]["hit"],
                    row["chain_over_first"]["delta"], row["chain_over_first"]["hit"]), flush=True)

            def g3(g):
                return dict(albedo=g["albedo"], normal=g["normal"], depth=g["depth"])

            measure("full size %d spp -> denoise" % n, lambda k: denoise_ref.denoise(color, W, H, **g3(full[k]), **DENOISE))
            measure("full size %d spp -> denoise_var" % n,
                    lambda k: denoise_var_ref.denoise_var(m, e, W, H, **g3(full[k]), **DENOISE_VAR))
            for tag, spp in (("b", 4 * n), ("c", n)):
                lo_color, lo_g = lo[tag]

                def up(k):
                    out, _ = upsample_ref.upsample(W, H, LW, LH, lo_color, lo_g[k]["depth"], lo_g[k]["oid"], full[k]["depth"], full[k]["oid"],
                                                   lo_normal=lo_g[k]["normal"], lo_albedo=lo_g[k]["albedo"], normal=full[k]["normal"],
                                                   albedo=full[k]["albedo"], **UPSAMPLE)
                    return denoise_ref.denoise(out, W, H, **g3(full[k]), **DENOISE)

                measure("half size %d spp%s -> upsample -> denoise" % (spp, " (the rays of full size %d)" % n if tag == "b" else ""), up)
    return rows


def main():
    rows = study()
    names = []
    for r in rows:
        if (r["row"], r["n"]) not in names:
            names.append((r["row"], r["n"]))
    summary = []
    for name, n in names:
        rs = [r for r in rows if r["row"] == name and r["n"] == n]
        s = {"row": name, "seeds": len(rs)}
        for kind in ("first", "chain"):
            s[kind] = {k: float(np.mean([r[kind][k] for r in rs])) for k in ("hit", "delta")}
        s["chain_over_first"] = {k: s["chain"][k] / s["first"][k] for k in ("hit", "delta")}
        worse = [k for k in ("hit", "delta") if not s["chain_over_first"][k] < 1]
        s["verdict"] = "better" if not worse else "WORSE over %s pixels" % " and ".join(worse)
        summary.append(s)
    doc = {"command": "python tools/aov_chain_cpu_study.py",
           "what": "mean |frame - truth| over the full-size pixels whose sample 0 hits anything (hit) and over those whose first hit is a "
                   "mirror or glass surface (delta), with first-hit guides and with chain guides (max_chain %d) in every pass; %s at %dx%d, "
                   "half size %dx%d; frames = oracle, truth = oracle at %d spp seed 1000; filters = the numpy restatements at the "
                   "library's defaults; summary = the mean over the seed offsets" % (MAX_CHAIN, SCENE, W, H, LW, LH, TRUTH_SPP),
           "scene": SCENE, "size": [W, H], "lo_size": [LW, LH], "n": list(N_SPP), "seed_offsets": list(SEEDS), "truth_spp": TRUTH_SPP,
           "denoise": DENOISE, "denoise_var": DENOISE_VAR, "upsample": UPSAMPLE, "max_chain": MAX_CHAIN,
           "summary": summary, "rows": rows}
    path = os.path.join(ROOT, "profiles", "aov_chain_cpu_study.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for s in summary:
        print("%-62s delta %.4f -> %.4f (x%.3f)   all %.4f -> %.4f (x%.3f)  %s" % (
            s["row"], s["first"]["delta"], s["chain"]["delta"], s["chain_over_first"]["delta"], s["first"]["hit"], s["chain"]["hit"],
            s["chain_over_first"]["hit"], s["verdict"]))
    print("->", path)


if __name__ == "__main__":
    main()
