"""The finish half of a k_pass_cand trip - shade_surface's second ray written only on a split, the emitter test taken from a bit
of the surface record, the adds into the stream's accumulators without their tests for a zero sum, the Philox round keys through
a three-input logic op - against code that shares none of the kernel and against the oracle's integers.  Every comparison is ==.
-m gpu.

The yardsticks: the pass kernel without the candidate scan (PT_FLAG_NO_BVH -> k_pass: surfaces by id from the material table, its
own append and its own adds with the zero tests), and tests/frame_sums.py's raw 32.32 sums chained down the oracle's paths.

The frames, each the smallest that reaches its case:
- cornell 16x12 @8 as ONE stream and as FOUR (PT_STREAMS);
- one stream of 63, 64 and 65 primary rays: a partial chunk, a full one, a full one and a chunk of one ray;
- a close-up in which every primary ray hits the glass sphere: every path splits at depth <= 2, so the second ray is stored;
- a view in which every primary ray hits the ceiling light: every lane of the first trips adds radiance;
- an emitter of emission (1.5, 0, 0), and a wall whose diffuse colour has a zero channel: sums of zero reach the adds.
Every frame is rendered twice in one context (the second frame finds the accumulators and the staged records of the first), and
all of it again with PT_GLASS_DEFER=1 (glass hits collected per wave and shaded 64 at a time: DEFER's readers of the second ray)."""
import json

import pytest

import frame_sums as fs
import gpudev
import ptlib
import scatter_walk
from gpudev import L, same_bytes  # noqa: F401  (L: fixture)
from ptlib import PtConfig
from test_gpu_frame_sums import _saved, assert_planes

pytestmark = pytest.mark.gpu

SEED = scatter_walk.SEED
GLASS, EMITTER, RED_WALL, LIGHT = 1, 2, 4, 10  # cornell.json's objects
CONTEXTS = {"one_stream": {"PT_STREAMS": "1"}, "four_streams": {"PT_STREAMS": "4"},
            "one_stream_defer": {"PT_STREAMS": "1", "PT_GLASS_DEFER": "1"},
            "four_streams_defer": {"PT_STREAMS": "4", "PT_GLASS_DEFER": "1"}}


@pytest.fixture(scope="module")
def ctxs(L):
    made = {name: gpudev.Device(L, env=env) for name, env in CONTEXTS.items()}
    yield made
    for d in made.values():
        d.close()


def _cornell(tmp, name, camera=None, edit=None):
    """cornell.json with another camera (position, direction) and / or edited objects"""
    d = json.load(open(ptlib.scene_path("cornell")))
    if camera is not None:
        d["camera"]["position"], d["camera"]["direction"] = camera
    if edit is not None:
        edit(d["objects"])
    d["id"] = name
    path = tmp / (name + ".json")
    path.write_text(json.dumps(d))
    return ptlib.load_scene_py(str(path), base_dir=ptlib.ROOT)


def _red_emitter(objs):
    """both emitters of the room - the small sphere and the ceiling light - emit (1.5, 0, 0)"""
    assert objs[EMITTER]["material"]["emmission"] == [1.96, 2.0, 1.8] and objs[LIGHT]["material"]["emmission"][1] == 0.9
    objs[EMITTER]["material"]["emmission"] = objs[LIGHT]["material"]["emmission"] = [1.5, 0.0, 0.0]


def _zero_channel_wall(objs):
    assert objs[RED_WALL]["material"]["color"] == [0.85, 0.25, 0.25]
    objs[RED_WALL]["material"]["color"] = [0.85, 0.0, 0.25]


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("finish_half")
    return {
        "cornell": scatter_walk._scene("cornell"),
        "glass_closeup": _cornell(tmp, "glass_closeup", camera=([1.3, -1.2, 0.9], [0.0, 0.0, -1.0])),
        "light_closeup": _cornell(tmp, "light_closeup", camera=([0.0, 1.2, 0.0], [0.0, 0.9982048, -0.05989229])),
        "red_emitter": _cornell(tmp, "red_emitter", edit=_red_emitter),
        "zero_channel_wall": _cornell(tmp, "zero_channel_wall", edit=_zero_channel_wall),
    }


# (name, scene, width, height, samples, contexts)
FRAMES = [
    ("cornell-16x12@8", "cornell", 16, 12, 8, ("one_stream", "four_streams", "one_stream_defer", "four_streams_defer")),
    ("cornell-63", "cornell", 9, 7, 1, ("one_stream", "one_stream_defer")),
    ("cornell-64", "cornell", 8, 8, 1, ("one_stream", "one_stream_defer")),
    ("cornell-65", "cornell", 13, 5, 1, ("one_stream", "one_stream_defer")),
    ("glass_closeup-12x8@4", "glass_closeup", 12, 8, 4, ("one_stream", "four_streams", "one_stream_defer")),
    ("light_closeup-12x8@4", "light_closeup", 12, 8, 4, ("one_stream", "one_stream_defer")),
    ("red_emitter-12x8@4", "red_emitter", 12, 8, 4, ("one_stream", "one_stream_defer")),
    ("zero_channel_wall-12x8@4", "zero_channel_wall", 12, 8, 4, ("one_stream", "one_stream_defer")),
]
CASES = [(f, c) for f in FRAMES for c in f[5]]
CASE_IDS = ["%s-%s" % (f[0], c) for f, c in CASES]


@pytest.fixture(scope="module")
def walks(scenes):
    """(walk, pixel totals) of each frame from the oracle's paths, computed once per process and left unchanged"""
    out = {}
    for name, sid, w, h, spp, _ in FRAMES:
        if sid == "cornell" and (w, h, spp) == (16, 12, 8):
            W, sums = fs.frame("cornell", w, h, spp, SEED)  # (the frame tests/test_gpu_frame_sums.py walks: shared)
        else:
            W = scatter_walk.walk_scene(scenes[sid], w, h, spp, SEED)
            sums = fs.walk_sums(W)
        out[name] = (W, fs.total_over(sums, range(spp)))
    return out


def _primary_hits(W):
    return {int(W.oid[i]) for i in range(W.n) if W.keys[i][2] == 0}


def test_the_frames_reach_their_cases(walks):
    """from the oracle alone: what each frame is there for happens in it"""
    for name, n in (("cornell-63", 63), ("cornell-64", 64), ("cornell-65", 65)):
        W = walks[name][0]
        assert sum(1 for k in W.keys if k[2] == 0) == n and W.n > n
    W, _ = walks["glass_closeup-12x8@4"]
    assert _primary_hits(W) == {GLASS}
    assert scatter_walk.kinds(W)["split_pair"] >= 2 * 12 * 8 * 4  # the first hit splits, and so does a child of it
    W, total = walks["light_closeup-12x8@4"]
    assert _primary_hits(W) == {LIGHT} and all(v > 0 for px in total for v in px)
    W, total = walks["red_emitter-12x8@4"]
    hits = [i for i in range(W.n) if W.oid[i] in (EMITTER, LIGHT)]
    assert len(hits) >= 64 and sum(px[0] > 0 for px in total) >= 64, "emitters are hit"
    assert all(px[1] == 0 and px[2] == 0 for px in total), "every green and blue contribution is a sum of zero"
    W, total = walks["zero_channel_wall-12x8@4"]
    zero_green = [c for c in fs.contributions(W) if c[3][1] == 0 and (c[3][0] > 0 or c[3][2] > 0)]
    assert len(zero_green) >= 16, "contributions with a zero channel: paths that met the wall before a light"
    W, _ = walks["cornell-16x12@8"]
    k = scatter_walk.kinds(W)
    assert min(k["split_pair"], k["chosen_reflection"], k["chosen_transmission"], k["mirror_child"], k["roulette_death"]) > 0


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_frame_is_k_pass_and_the_oracle_sums(L, ctxs, scenes, walks, case, tmp_path):
    (name, sid, w, h, spp, _), cname = case
    dev, sc = ctxs[cname], scenes[sid]
    ctx = dev.ctx
    W, total = walks[name]
    what = "%s %s" % (name, cname)
    out = dev.alloc(w * h * 12)
    try:
        gpudev.set_scene(L, ctx, sc)
        assert L.pt_ctx_pass_kernel(ctx, 0).decode() == "k_pass_cand" and L.pt_ctx_pass_kernel(ctx, ptlib.FLAG_NO_BVH).decode() == "k_pass"
        cfg = PtConfig(w, h, spp, 0, SEED, 0, 0, 0, 0)
        want, st_ref = dev.render(PtConfig(w, h, spp, 0, SEED, 0, 0, 0, ptlib.FLAG_NO_BVH), out)
        assert st_ref.ray_bounces == W.n, (what, st_ref.ray_bounces, W.n)
        for turn in ("first frame", "second frame"):
            got, st = dev.render(cfg, out)
            assert st.ray_bounces == W.n, (what, turn, st.ray_bounces, W.n)
            same_bytes(got, want, "%s, %s against k_pass" % (what, turn))
        img, st = dev.render(cfg, out, accumulate=True)
        assert st.ray_bounces == W.n, (what, st.ray_bounces, W.n)
        assert_planes(_saved(L, ctx, tmp_path / "frame.ptacc")["sums"], fs.planes(total), what)
        same_bytes(img, fs.resolved(total, spp, clamp=True), what + " resolved")
        same_bytes(img, want, what + " accumulated against k_pass")
    finally:
        dev.free(out)
