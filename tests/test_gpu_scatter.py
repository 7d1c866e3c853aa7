"""pt_ctx_scatter on the GPU: shade_surface, fetch_surface and fetch_surface_rank as the frame kernels call them, ray by ray.
Every comparison is of the bytes of float32 words or of integers, for equality; nothing here has a tolerance.

- The edge cases of tests/kats_scatter.py through the given-surface form in the three shading modes, against the restatement.
- Incoming throughputs of (1, 1, 1) and of random binary32 triples in (0, 4]: thr0 / thr1 = fl(fl(thr * colour') * factor), contrib =
  fl(thr * emission), the emits flag (an emission with one non-zero channel, an emission of -0.0).
- The oracle's paths (pto_dump_paths) of three small frames by hit id and, where the scene has candidate tables, by rank: hit id
  and hit point against pto_intersect_batch, the children against the dump, their depth and branch against the keys, n_rays.
- A generated scene (tests/boundary_rays.py) whose surf table does not fit k_pass_cand's LDS: ranks on both sides of the staged
  head, by rank against by id and against the oracle.
The probe proves the functions, not each kernel's use of them: that stays with the bounce counts and the frame tests."""
import numpy as np
import pytest

import boundary_rays
import gpudev
import kats_scatter as ks
import lds_layouts
import ptlib
from gpudev import L  # noqa: F401  (fixture)
from ptlib import PtScatterOut
import scatter_walk as sw
from scatter_walk import bits

pytestmark = pytest.mark.gpu
f32 = np.float32
MODES = {"all": 0, "defer": sw.DEFER_REFRACT, "refract_only": sw.REFRACT_ONLY}


@pytest.fixture(scope="module")
def ctx(L):
    with gpudev.Device(L) as dev:
        yield dev.ctx


def scatter(L, ctx, form, items, surfs=None, seed=ks.SEED):
    out = (PtScatterOut * len(items))()
    for o in out:
        o.hit = 12345
    assert L.pt_ctx_scatter(ctx, seed, form, items, surfs, len(items), out) == 0, L.pt_last_error().decode()
    return out


def check_against_restatement(name, o, want, depth):
    """one device result against kats_scatter.scatter's"""
    assert o.hit == 0 and o.deferred == 0, name
    assert o.n_rays == len(want["children"]), (name, o.n_rays, want["kind"])
    assert bool(o.emits) == bool((want["emission"] != 0).any()), name
    for (d, w, cdepth, cbranch), (gd, gw, gdepth, gbranch) in zip(
            want["children"], ((o.d0, o.thr0, o.depth0, o.branch0), (o.d1, o.thr1, o.depth1, o.branch1))):
        assert bits(gd) == d.tobytes(), (name, want["kind"], list(gd), d)
        assert bits(gw) == w.tobytes(), (name, want["kind"], list(gw), w)
        assert (gdepth, gbranch) == (cdepth, cbranch) and cdepth == depth + 1, name


# ------------------------------------------------------------------------------------------------------ the edge cases
@pytest.fixture(scope="module")
def edge_all(L, ctx):
    items, surfs = sw.case_arrays(ks.CASES)
    return scatter(L, ctx, sw.GIVEN, items, surfs)


def test_edge_cases_shade_all(edge_all):
    """kShadeAll on every case: every ulp neighbour of every boundary takes the side the restatement takes, bit for bit"""
    for c, o in zip(ks.CASES, edge_all):
        want = ks.expected(c, thr=(1, 1, 1))
        check_against_restatement(c["name"], o, want, c["depth"])
        assert bits(o.x) == c["x"].tobytes() and bits(o.contrib) == want["contrib"].tobytes(), c["name"]
        # (1, 1, 1) above: the weights are the Rust text's own
        for (_, w, _, _), (_, w1, _, _) in zip(ks.expected(c)["children"], want["children"]):
            assert w.tobytes() == w1.tobytes()


def test_edge_cases_defer_refract(L, ctx, edge_all):
    """kShadeDeferRefract: glass comes back deferred with no rays; everything else is its kShadeAll result, byte for byte"""
    items, surfs = sw.case_arrays(ks.CASES)
    got = scatter(L, ctx, sw.GIVEN | sw.DEFER_REFRACT, items, surfs)
    n_glass = 0
    for c, o, a in zip(ks.CASES, got, edge_all):
        if c["reflect"] == ks.REFRACT:
            n_glass += 1
            assert (o.hit, o.deferred, o.n_rays, o.emits) == (0, 1, 0, 0), c["name"]
        else:
            assert bytes(o) == bytes(a), c["name"]
    assert 0 < n_glass < len(ks.CASES)


def test_edge_cases_refract_only(L, ctx, edge_all):
    """kShadeRefractOnly on the glass cases: the same bytes as kShadeAll, and the restatement's"""
    cases = [c for c in ks.CASES if c["reflect"] == ks.REFRACT]
    items, surfs = sw.case_arrays(cases)
    got = scatter(L, ctx, sw.GIVEN | sw.REFRACT_ONLY, items, surfs)
    by_name = {c["name"]: a for c, a in zip(ks.CASES, edge_all)}
    for c, o in zip(cases, got):
        assert bytes(o) == bytes(by_name[c["name"]]), c["name"]
        check_against_restatement(c["name"], o, ks.expected(c, thr=(1, 1, 1)), c["depth"])
    # a surface that is not glass is refused for the whole call, before the device
    items, surfs = sw.case_arrays(ks.CASES[:1])
    out = (PtScatterOut * 1)()
    assert L.pt_ctx_scatter(ctx, ks.SEED, sw.GIVEN | sw.REFRACT_ONLY, items, surfs, 1, out) == -1
    assert "not Refract" in L.pt_last_error().decode()


# --------------------------------------------------------------------------------------------------------- throughput
@pytest.mark.parametrize("mode", ["all", "refract_only"])
def test_throughput_goes_down_the_path(L, ctx, mode):
    """random incoming throughputs in (0, 4]: thr0 / thr1 = fl(fl(thr * colour') * factor), contrib = fl(thr * emission)"""
    rng = np.random.default_rng(20261019)
    cases = [c for c in ks.CASES if mode == "all" or c["reflect"] == ks.REFRACT]
    emissions = [(0, 0, 0), (0, 2.5, 0), (-0.0, -0.0, -0.0), (1.5, 0.25, 3), (0, 0, 2.0 ** -140), (-0.0, 0, 7)]
    cases = [dict(c, emission=ks.v3(*emissions[i % len(emissions)])) for i, c in enumerate(cases)]
    thrs = (f32(4.0) - rng.random((len(cases), 3), dtype=f32) * f32(4.0)).astype(f32)  # (0, 4]
    assert (thrs > 0).all() and (thrs <= 4).all()
    thrs[:3] = 1.0
    items, surfs = sw.case_arrays(cases, thrs)
    got = scatter(L, ctx, sw.GIVEN | MODES[mode], items, surfs)
    seen_emits = set()
    for c, thr, o in zip(cases, thrs, got):
        want = ks.expected(c, thr=thr)
        check_against_restatement(c["name"], o, want, c["depth"])
        assert bits(o.contrib) == want["contrib"].tobytes(), (c["name"], list(o.contrib), want["contrib"])
        seen_emits.add((bool(o.emits), tuple(float(v) for v in c["emission"])))
    assert (False, (-0.0, -0.0, -0.0)) in seen_emits and (True, (0.0, 2.5, 0.0)) in seen_emits and (True, (0.0, 0.0, 2.0 ** -140)) in seen_emits


# ----------------------------------------------------------------------------------------------------------- the walk
def check_walk(W, got, name):
    """device results for every dumped ray of a walk against the oracle: hit, hit point, children, keys, n_rays"""
    for i, o in enumerate(got):
        assert o.hit == sw.hit_id(W, i), (name, i, o.hit, sw.hit_id(W, i))
        if o.hit < 0:
            continue
        kids = W.children[i]
        assert bits(o.x) == W.x[i].tobytes(), (name, i)
        assert o.n_rays == len(kids) and o.deferred == 0, (name, i, o.n_rays, len(kids))
        for k, (gd, gdepth, gbranch) in zip(kids, ((o.d0, o.depth0, o.branch0), (o.d1, o.depth1, o.branch1))):
            assert bits(o.x) == W.o[k].tobytes() and bits(gd) == W.d[k].tobytes(), (name, i, k)
            assert (gdepth, gbranch) == (int(W.keys[k][2]), int(W.keys[k][3])), (name, i, k)
        emission = W.scene.objs[int(W.oid[i])].emission
        assert bits(o.contrib) == bits(emission) and bool(o.emits) == any(v != 0 for v in emission), (name, i)


@pytest.mark.parametrize("frame", sw.FRAMES, ids=[f[0] for f in sw.FRAMES])
def test_oracle_paths_by_id_and_by_rank(L, frame):
    W = sw.walk(*frame)
    sc = W.scene
    with gpudev.Device(L, sc) as dev:
        c = dev.ctx
        items = sw.walk_items(W)
        by_id = scatter(L, c, sw.BY_ID, items, seed=sw.SEED)
        check_walk(W, by_id, frame[0] + " by id")
        out = (PtScatterOut * W.n)()
        if boundary_rays.scene_tables(sc)["cand_ok"]:
            by_rank = scatter(L, c, sw.BY_RANK, items, seed=sw.SEED)
            check_walk(W, by_rank, frame[0] + " by rank")
            assert bytes(by_rank) == bytes(by_id)
        else:
            assert L.pt_ctx_scatter(c, sw.SEED, sw.BY_RANK, items, None, W.n, out) == -1
            assert "candidate tables" in L.pt_last_error().decode()
        # kShadeDeferRefract: glass deferred, the rest as above; kShadeRefractOnly: glass as above, the rest not shaded
        defer = scatter(L, c, sw.BY_ID | sw.DEFER_REFRACT, items, seed=sw.SEED)
        only = scatter(L, c, sw.BY_ID | sw.REFRACT_ONLY, items, seed=sw.SEED)
        for i in range(W.n):
            glass = W.oid[i] >= 0 and sc.objs[int(W.oid[i])].reflect_type == ks.REFRACT
            if glass:
                assert (defer[i].hit, defer[i].deferred, defer[i].n_rays) == (by_id[i].hit, 1, 0), i
                assert bytes(only[i]) == bytes(by_id[i]), i
            else:
                assert bytes(defer[i]) == bytes(by_id[i]), i
                assert only[i].hit == (sw.NOT_SHADED if W.oid[i] >= 0 else -1) and only[i].n_rays == 0, i


def test_scene_needed_for_the_hit_forms(L, ctx):
    items, _ = sw.case_arrays(ks.CASES[:1])
    out = (PtScatterOut * 1)()
    for form in (sw.BY_ID, sw.BY_RANK):
        assert L.pt_ctx_scatter(ctx, 1, form, items, None, 1, out) == -1 and "no scene" in L.pt_last_error().decode()


# ------------------------------------------------------------------------------------------- tables that did not fit
def test_surf_table_that_does_not_fit_lds(L):
    """boundary_rays' "ties" scene: k_pass_cand<BVH> stages the candidate records and only a head of the surf table (pt_layout.h),
    so fetch_surface_rank reads the ranks below the head from LDS and the others from global memory.  The probe stages that same
    head; rays of a small frame hit ranks on both sides, spheres and triangles; by rank must equal by id and the oracle."""
    sc = dict((s.id, s) for _, s in boundary_rays.build_scenes(20261016))["ties"]
    lay = lds_layouts.layout(sc)[0]
    tabs = boundary_rays.scene_tables(sc)
    n_ranks = sc.n_objs + sc.n_tris
    assert tabs["cand_ok"] and lay["staged"] == 1 and lay["surf_staged"] == 0 and 0 < lay["surf_head"] < n_ranks, lay
    W = sw.walk_scene(sc, 24, 16, 2)
    rank_of = {int(h): r for r, h in enumerate(tabs["rank_id"])}
    ranks = np.array([rank_of[sw.hit_id(W, i)] for i in range(W.n) if W.oid[i] >= 0])
    below, above = ranks[ranks < lay["surf_head"]], ranks[ranks >= lay["surf_head"]]
    assert len(set(below)) >= 4 and len(set(above)) >= 4, (len(below), len(above))
    kinds = {sc.objs[int(W.oid[i])].kind for i in range(W.n) if W.oid[i] >= 0}
    assert kinds == {ptlib.PT_SPHERE, ptlib.PT_MESH}
    with gpudev.Device(L, sc) as dev:
        c = dev.ctx
        items = sw.walk_items(W)
        by_rank = scatter(L, c, sw.BY_RANK, items, seed=sw.SEED)
        by_id = scatter(L, c, sw.BY_ID, items, seed=sw.SEED)
        check_walk(W, by_rank, "ties by rank")
        assert bytes(by_rank) == bytes(by_id)


def test_by_rank_refused_without_candidate_tables(L):
    """513 one-triangle meshes make 513 candidate records, one more than a queue entry numbers: the scene has no candidate tables"""
    objs, tris = [], []
    for k in range(513):
        x, y = float(k % 27) * 0.25 - 3.5, float(k // 27) * 0.25 - 2.5
        objs.append(ptlib.make_mesh((0, 0, 0), (0.5, 0.5, 0.5), (0, 0, 0), "Diffuse", len(tris), 1, (x, y, 0.0), 1.0))
        tris.append(ptlib.make_tri((x, y, 0), (x + 0.2, y, 0), (x, y + 0.2, 0)))
    sc = ptlib.Scene("many-meshes", ptlib.make_camera((0, 0, 6), (0, 0, -1)), objs, tris)
    assert not boundary_rays.scene_tables(sc)["cand_ok"]
    with gpudev.Device(L, sc) as dev:
        c = dev.ctx
        items = (ptlib.PtScatterItem * 2)(sw.item((0.05, 0.05, 6), (0, 0, -1), (1, 1, 1), 0, 0, 0, 1),
                                       sw.item((-3.45, -2.45, 6), (0, 0, -1), (1, 1, 1), 1, 0, 0, 1))
        out = (PtScatterOut * 2)()
        assert L.pt_ctx_scatter(c, 1, sw.BY_RANK, items, None, 2, out) == -1
        assert "candidate tables" in L.pt_last_error().decode()
        got = scatter(L, c, sw.BY_ID, items, seed=1)  # by id still runs
        assert got[1].hit == sc.n_objs + 0 and got[1].n_rays == 1
