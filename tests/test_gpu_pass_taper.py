"""k_pass_cand's taper - the last streams of a launch run as pieces, (stream, a share of the pass's samples) per workgroup, with a
stack slice per workgroup and an atomic flush into the stream's accumulators (pt_kernels.hip: "THE TAPER"; host::plan_taper) -
against code that shares none of it and against the oracle's integers.  Every comparison is ==.  -m gpu.

The yardsticks are tests/test_gpu_finish_half.py's: the pass kernel without the candidate scan (PT_FLAG_NO_BVH -> k_pass, whole
streams, its own flush), and tests/frame_sums.py's raw 32.32 sums chained down the oracle's paths.  At these sizes every
workgroup of a launch is resident at once, so the pieces of a stream really run side by side and add into the same slots.

The frames (PT_TAPER_CUT streams cut into PT_TAPER_PIECES pieces; knobs set by hand are taken as given):
- cornell 16x12 @8, four streams, all four cut into 2, 4 and 8 pieces (8: pieces of one sample);
- the same with only the last stream cut into 4: whole streams and pieces in one launch;
- the same as ONE stream cut into 8;
- cornell 16x12 @7 cut into 4: shares of 2, 2, 2 and 1 samples;
- cornell 16x12 @3 cut into 8: five pieces of every stream have no sample and return at once;
- the glass close-up 12x8 @4 cut into 4: every path splits twice - a piece's stacks hold its own rays' descendants;
- scenes/mesh.json 16x12 @4 cut into 4: the instance with walks, whose parking areas are per workgroup too.
Each frame is rendered twice in one context, and accumulated in two calls - the second starts from the held sums of the first and
flushes on top of them.  The bounce counts are the oracle's ray count; passes and launches are those of the same frame with the
taper off."""
import pytest

import frame_sums as fs
import gpudev
import ptlib
import scatter_walk
from gpudev import L, same_bytes  # noqa: F401  (L: fixture)
from ptlib import PtConfig
from test_gpu_finish_half import GLASS, _cornell
from test_gpu_frame_sums import _saved, assert_planes

pytestmark = pytest.mark.gpu

SEED = scatter_walk.SEED


def _env(streams, cut, pieces):
    return {"PT_STREAMS": str(streams), "PT_TAPER_CUT": str(cut), "PT_TAPER_PIECES": str(pieces)}


CONTEXTS = {
    "off_4": _env(4, 0, 4), "off_1": _env(1, 0, 8),
    "all4_x2": _env(4, 4, 2), "all4_x4": _env(4, 4, 4), "all4_x8": _env(4, 4, 8),
    "last_x4": _env(4, 1, 4), "one_x8": _env(1, 1, 8),
}
# (name, scene, width, height, samples, (tapered context, the context with the taper off) ...)
FRAMES = [
    ("cornell-16x12@8", "cornell", 16, 12, 8, (("all4_x2", "off_4"), ("all4_x4", "off_4"), ("all4_x8", "off_4"), ("last_x4", "off_4"),
                                                ("one_x8", "off_1"))),
    ("cornell-16x12@7", "cornell", 16, 12, 7, (("all4_x4", "off_4"),)),
    ("cornell-16x12@3", "cornell", 16, 12, 3, (("all4_x8", "off_4"),)),
    ("glass_closeup-12x8@4", "glass_closeup", 12, 8, 4, (("all4_x4", "off_4"),)),
    ("mesh-16x12@4", "mesh", 16, 12, 4, (("all4_x4", "off_4"),)),
]
CASES = [(f, c) for f in FRAMES for c in f[5]]
CASE_IDS = ["%s-%s" % (f[0], c[0]) for f, c in CASES]


@pytest.fixture(scope="module")
def ctxs(L):
    made = {name: gpudev.Device(L, env=env) for name, env in CONTEXTS.items()}
    yield made
    for d in made.values():
        d.close()


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pass_taper")
    return {
        "cornell": scatter_walk._scene("cornell"),
        "glass_closeup": _cornell(tmp, "glass_closeup", camera=([1.3, -1.2, 0.9], [0.0, 0.0, -1.0])),
        "mesh": scatter_walk._scene("mesh"),
    }


@pytest.fixture(scope="module")
def walks(scenes):
    """(walk, sums per sample) of each frame from the oracle's paths, computed once per process and left unchanged"""
    out = {}
    for name, sid, w, h, spp, _ in FRAMES:
        if sid == "cornell" and (w, h, spp) == (16, 12, 8):
            out[name] = fs.frame("cornell", w, h, spp, SEED)  # (the frame tests/test_gpu_frame_sums.py walks: shared)
        else:
            W = scatter_walk.walk_scene(scenes[sid], w, h, spp, SEED)
            out[name] = (W, fs.walk_sums(W))
    return out


def test_the_frames_reach_their_cases(walks):
    """from the oracle alone: the glass close-up's paths split twice, and mesh.json's rays reach its mesh"""
    W, _ = walks["glass_closeup-12x8@4"]
    assert {int(W.oid[i]) for i in range(W.n) if W.keys[i][2] == 0} == {GLASS}
    assert scatter_walk.kinds(W)["split_pair"] >= 2 * 12 * 8 * 4
    W, _ = walks["mesh-16x12@4"]
    sc = W.scene
    meshes = {i for i in range(sc.n_objs) if sc.objs[i].kind == ptlib.PT_MESH and sc.objs[i].tri_count >= 16}
    assert meshes and sum(1 for i in range(W.n) if int(W.oid[i]) in meshes) >= 64, "rays hit the mesh that has a BVH"


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_tapered_frame_is_k_pass_and_the_oracle_sums(L, ctxs, scenes, walks, case, tmp_path):
    (name, sid, w, h, spp, _), (cname, off_name) = case
    dev, dev_off, sc = ctxs[cname], ctxs[off_name], scenes[sid]
    ctx, off = dev.ctx, dev_off.ctx
    W, sums = walks[name]
    total = fs.total_over(sums, range(spp))
    what = "%s %s" % (name, cname)
    out = dev.alloc(w * h * 12)
    try:
        for c in (ctx, off):
            gpudev.set_scene(L, c, sc)
            assert L.pt_ctx_pass_kernel(c, 0).decode() == ("k_pass_cand_bvh" if sid == "mesh" else "k_pass_cand")
        assert L.pt_ctx_pass_kernel(ctx, ptlib.FLAG_NO_BVH).decode() == "k_pass"
        cfg = PtConfig(w, h, spp, 0, SEED, 0, 0, 0, 0)
        want, st_ref = dev.render(PtConfig(w, h, spp, 0, SEED, 0, 0, 0, ptlib.FLAG_NO_BVH), out)
        assert st_ref.ray_bounces == W.n, (what, st_ref.ray_bounces, W.n)
        plain, st_off = dev_off.render(cfg, out)
        assert st_off.ray_bounces == W.n, (what, st_off.ray_bounces, W.n)
        same_bytes(plain, want, what + ", taper off against k_pass")
        for turn in ("first frame", "second frame"):
            got, st = dev.render(cfg, out)
            assert st.ray_bounces == W.n, (what, turn, st.ray_bounces, W.n)
            assert (st.passes, st.intersect_launches) == (st_off.passes, st_off.intersect_launches), (what, turn)
            same_bytes(got, want, "%s, %s against k_pass" % (what, turn))
        # two calls: the second gathers the held sums of the first into the accumulators and the pieces add on top
        first = max(1, spp // 2)
        assert L.pt_ctx_accum_reset(ctx) == 0
        _, st1 = dev.render(PtConfig(w, h, first, 0, SEED, 0, 0, 0, 0), out, accumulate=True)
        assert_planes(_saved(L, ctx, tmp_path / "first.ptacc")["sums"], fs.planes(fs.total_over(sums, range(first))), what + " first call")
        img, st2 = dev.render(cfg, out, accumulate=True)
        assert st1.ray_bounces + st2.ray_bounces == W.n, (what, st1.ray_bounces, st2.ray_bounces, W.n)
        assert_planes(_saved(L, ctx, tmp_path / "frame.ptacc")["sums"], fs.planes(total), what)
        same_bytes(img, fs.resolved(total, spp, clamp=True), what + " resolved")
        same_bytes(img, want, what + " accumulated against k_pass")
    finally:
        dev.free(out)
