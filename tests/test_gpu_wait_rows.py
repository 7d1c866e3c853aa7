"""k_pass_cand without walks keeps a waiting ray's throughput and bookkeeping word in a row of LDS - one float4 per lane, written
in the trip that starts the ray (a popped ray's straight from the wave's stack, a primary ray's made on the spot), read in the trip
that finishes it - instead of in four registers.  Every check here is bit for bit, with ==, against code that has no such row.
-m gpu.

The yardsticks: the pass kernel WITHOUT the candidate scan (PT_FLAG_NO_BVH -> k_pass), and the oracle's own integer sums
(tests/frame_sums.py) against the raw 32.32 sums pt_ctx_accum_save writes.

The shapes are the smallest at which the rows can go wrong:
- cornell 7x9, 8x8, 13x5 @1 as ONE stream (PT_STREAMS=1): 63, 64 and 65 primary rays - a partial chunk whose idle lanes write rows
  nobody may read, a full chunk, a full chunk beside a chunk of one ray; each ends with trips that finish a chunk and start none;
- cornell 16x12 @8 as one stream (192 pixels: the unstaged instance) and as four (the staged one): a wave takes six chunks of
  primaries (or one to two) between pops, the row of the ray being finished is read in the trip that overwrites it with the
  row of the ray just started, and the wave's last trips pop ever fewer rays;
- a close-up of cornell's glass sphere, every primary ray on glass: the second ray of a split takes its word from the row;
- all of these with PT_GLASS_DEFER=1 too (the DEFER instances read throughput and word of a deferred hit from the row);
- mesh.json 12x8 @4: the instance with walks, which keeps the four values in registers and parks them with the ray;
- one pt_ctx_radiance probe per material (65 samples: a full chunk and a chunk of one): the PROBE instances;
- every frame twice in one context: the rows a call leaves behind are not the next call's."""
import ctypes as C
import json

import numpy as np
import pytest

import frame_sums as fs
import gpudev
import ptlib
import scatter_walk
from gpudev import L, same_bytes  # noqa: F401  (L: fixture)
from ptlib import PtConfig, PtStats, _np_f
from test_gpu_frame_sums import _saved, assert_planes

pytestmark = pytest.mark.gpu

SEED = scatter_walk.SEED
ENVS = {"plain": {}, "defer": {"PT_GLASS_DEFER": "1"}}
GLASS = 1  # cornell.json's object 1


@pytest.fixture(scope="module")
def ctxs(L):
    """contexts by (form, streams), made on demand: the tuning variables are read when a context is created"""
    made = {}

    def get(form, streams=0):
        if (form, streams) not in made:
            env = dict(ENVS[form])
            if streams:
                env["PT_STREAMS"] = str(streams)
            made[(form, streams)] = gpudev.Device(L, env=env)
        return made[(form, streams)]

    yield get
    for dev in made.values():
        dev.close()


@pytest.fixture(scope="module")
def glass_closeup(tmp_path_factory):
    """cornell.json seen from 2.2 in front of its glass sphere through a narrow sensor: the frame lies inside the sphere's disc"""
    d = json.load(open(ptlib.scene_path("cornell")))
    assert d["objects"][GLASS]["material"]["reflect_type"] == "Refract"
    x, y, z = d["objects"][GLASS]["position"]
    d["camera"].update(position=[x, y, z + 2.2], direction=[0.0, 0.0, -1.0], sensor_width=0.012)
    d["id"] = "cornell_glass"
    path = tmp_path_factory.mktemp("wait_rows") / "cornell_glass.json"
    path.write_text(json.dumps(d))
    return ptlib.load_scene_py(str(path), base_dir=ptlib.ROOT)


def _set_scene(L, dev, sc, kernel="k_pass_cand"):
    gpudev.set_scene(L, dev.ctx, sc)
    assert L.pt_ctx_pass_kernel(dev.ctx, 0).decode() == kernel, sc.id
    assert L.pt_ctx_pass_kernel(dev.ctx, ptlib.FLAG_NO_BVH).decode() == "k_pass", sc.id


def _twice_against_k_pass(L, dev, w, h, spp, what):
    """the frame through the candidate scan, twice, and through k_pass: the same floats and the same bounce count"""
    out = dev.alloc(w * h * 12)
    try:
        want, st_ref = dev.render(PtConfig(w, h, spp, 0, SEED, 0, 0, 0, ptlib.FLAG_NO_BVH), out)
        for call in (1, 2):
            got, st = dev.render(PtConfig(w, h, spp, 0, SEED, 0, 0, 0, 0), out)
            assert st.ray_bounces == st_ref.ray_bounces and st.ray_bounces >= w * h * spp, (what, call, st.ray_bounces, st_ref.ray_bounces)
            same_bytes(got, want, "%s, call %d, against k_pass" % (what, call))
        assert np.isfinite(want).all() and want.max() > 0.0, what
    finally:
        dev.free(out)


def _twice_against_oracle(L, dev, W, sums, tmp_path, what):
    """the raw sums of the frame, accumulated twice from nothing, are the integers chained down the oracle's paths"""
    total = fs.total_over(sums, range(W.spp))
    out = dev.alloc(W.width * W.height * 12)
    try:
        for call in (1, 2):
            assert L.pt_ctx_accum_reset(dev.ctx) == 0, L.pt_last_error()
            _, st = dev.render(PtConfig(W.width, W.height, W.spp, 0, SEED, 0, 0, 0, 0), out, accumulate=True)
            assert st.ray_bounces == W.n, (what, call, st.ray_bounces, W.n)
            assert_planes(_saved(L, dev.ctx, tmp_path / "frame.ptacc")["sums"], fs.planes(total), "%s, call %d" % (what, call))
    finally:
        dev.free(out)


@pytest.mark.parametrize("form", list(ENVS))
@pytest.mark.parametrize("size", [(7, 9), (8, 8), (13, 5)], ids=["63", "64", "65"])
def test_chunk_boundaries_of_one_stream(L, ctxs, form, size):
    dev = ctxs(form, 1)
    _set_scene(L, dev, scatter_walk._scene("cornell"))
    _twice_against_k_pass(L, dev, size[0], size[1], 1, "cornell %dx%d @1, one stream, %s" % (size + (form,)))


@pytest.mark.parametrize("form", list(ENVS))
@pytest.mark.parametrize("streams", [1, 4])
def test_primary_trips_between_pops_and_the_fading_tail(L, ctxs, form, streams, tmp_path):
    W, sums = fs.frame("cornell", 16, 12, 8, SEED)
    dev = ctxs(form, streams)
    _set_scene(L, dev, W.scene)
    what = "cornell 16x12 @8, %d stream(s), %s" % (streams, form)
    _twice_against_k_pass(L, dev, 16, 12, 8, what)
    _twice_against_oracle(L, dev, W, sums, tmp_path, what)


@pytest.mark.parametrize("form", list(ENVS))
def test_splits_on_glass_take_their_word_from_the_row(L, ctxs, form, glass_closeup, tmp_path):
    W = scatter_walk.walk_scene(glass_closeup, 8, 8, 2, SEED)
    first = W.keys[:W.n, 2] == 0
    assert first.sum() == 8 * 8 * 2 and (W.oid[:W.n][first] == GLASS).all(), "every primary ray hits the glass sphere"
    assert sum(len(c) == 2 for c in W.children[:W.n]) >= 64, "and splits"
    for streams in (0, 1):
        dev = ctxs(form, streams)
        _set_scene(L, dev, glass_closeup)
        what = "glass close-up 8x8 @2, streams %d, %s" % (streams, form)
        _twice_against_k_pass(L, dev, 8, 8, 2, what)
        _twice_against_oracle(L, dev, W, fs.walk_sums(W), tmp_path, what)


def test_parked_rays_carry_throughput_and_word(L, ctxs, tmp_path):
    W, sums = fs.frame("mesh", 12, 8, 4, SEED)
    dev = ctxs("plain")
    _set_scene(L, dev, W.scene, "k_pass_cand_bvh")
    _twice_against_k_pass(L, dev, 12, 8, 4, "mesh 12x8 @4")
    _twice_against_oracle(L, dev, W, sums, tmp_path, "mesh 12x8 @4")


PROBE_O = np.array((0.3, 0.4, 2.0), np.float32)  # inside the room, every target in plain view
PROBE_AT = {"mirror": (-1.3, -1.2, -1.3), "glass": (1.3, -1.2, -0.2), "emitter": (0.08, -1.2, -0.8), "diffuse": (-0.08, -1.2, 0.7),
            "wall": (2.6, 0.5, 1.0)}


@pytest.mark.parametrize("form", list(ENVS))
def test_one_probe_per_material(L, ctxs, form):
    dev = ctxs(form)
    _set_scene(L, dev, scatter_walk._scene("cornell"))
    for k, (name, at) in enumerate(PROBE_AT.items()):
        d = np.array(at, np.float64) - PROBE_O
        d = (d / np.linalg.norm(d)).astype(np.float32)
        res = []
        for flags in (0, 0, ptlib.FLAG_NO_BVH):
            out, st = np.zeros(3, np.float32), PtStats()
            rc = L.pt_ctx_radiance(dev.ctx, _np_f(PROBE_O), _np_f(d), 0, 65, SEED, k, 0, flags, _np_f(out), C.byref(st))
            assert rc == 0, L.pt_last_error()
            res.append((out.view(np.uint32).tolist(), st.ray_bounces))
        assert res[0] == res[1] == res[2], (form, name, res)
        assert res[0][1] > 65, (name, "the probe hits its target and goes on")
