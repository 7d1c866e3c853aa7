"""The boundary ray sets of tests/boundary_rays.py really sit on the boundaries (CPU only).

A generator that produces no boundary rays would pass every device test, so the ray set is tested itself: the oracle's
verdict flips across the ulp variants, exact ties occur, the clamp family is there, every scene has hits and misses, the
tables the rays are aimed at are the product's, and the set is a function of the seed."""

import numpy as np
import pytest

import boundary_rays as br
import ptlib

SEED = 20261016


@pytest.fixture(scope="module")
def sets():
    out = []
    for rs in br.build(SEED):
        t, oid, tid, x, nr = ptlib.oracle_intersect(rs.scene, rs.o, rs.d)
        out.append((rs, (t, oid, tid)))
    return out


def _verdict_ids(oid, tid):
    return np.where(oid < 0, -1, oid.astype(np.int64) * (1 << 20) + np.maximum(tid, 0))


def test_rays_keep_the_header_contract(sets):
    """Unit directions (f32-normalised: within a few ulp) and origins inside the bounding box of objects and camera."""
    for rs, _ in sets:
        lo, hi = br.scene_box(rs.scene)
        assert np.all(rs.o >= lo) and np.all(rs.o <= hi), rs.scene.id
        n = np.sqrt(np.sum(rs.d.astype(np.float64) ** 2, 1))
        assert np.all(np.abs(n - 1.0) < 6e-7), (rs.scene.id, float(np.abs(n - 1.0).max()))
        assert rs.n % br.VARIANTS == 0 and rs.n > 5000


# Targets whose verdict flips across their ulp variants.  Observed with SEED: 59 .. 440 per scene in all, 79 .. 158 per scene
# among the rays aimed at vertices and edges, 200 .. 1 000 per ray family over all scenes.  With the aiming broken (targets
# moved by 1e-3 of the scene's size) the vertex and edge rays flip 0 .. 6 times per scene and 4 / 2 times in all.
MIN_FLIPS_PER_SCENE = 25
MIN_AIMED_FLIPS_PER_SCENE = 25
MIN_FLIPS_PER_KIND = {"vertex": 100, "edge": 100, "surface": 100, "zero_dir": 50, "tiny_dir": 50, "sphere": 50}
# scale 1e-2: triangles of |N| ~ 1e-4 sit at the |det| < 1e-4 rejection, which rejects nearly every ray aimed at them
NEAR_DET_ONLY = ("scale0.01",)


def test_verdicts_flip_across_the_ulp_variants(sets):
    """For every scene, and for every ray family aimed at a boundary, the oracle's verdict (hit or miss, object, triangle)
    changes across the +-1 / +-2 ulp variants of many targets: the rays straddle the boundaries."""
    per_kind = {k: 0 for k in br.RAY_KINDS}
    aimed = [br.RAY_KINDS.index("vertex"), br.RAY_KINDS.index("edge")]
    for rs, (t, oid, tid) in sets:
        flips = br.verdict_flips(_verdict_ids(oid, tid))
        kinds = rs.kind[::br.VARIANTS]
        assert flips.sum() >= MIN_FLIPS_PER_SCENE, (rs.scene.id, int(flips.sum()))
        if rs.scene.id not in NEAR_DET_ONLY:
            assert flips[np.isin(kinds, aimed)].sum() >= MIN_AIMED_FLIPS_PER_SCENE, rs.scene.id
        for k, name in enumerate(br.RAY_KINDS):
            per_kind[name] += int(flips[kinds == k].sum())
    for name, least in MIN_FLIPS_PER_KIND.items():
        assert per_kind[name] >= least, (name, per_kind)


def test_every_scene_has_hits_and_misses(sets):
    for rs, (t, oid, tid) in sets:
        frac = float((oid >= 0).mean())
        assert 0.05 < frac < 0.99, (rs.scene.id, frac)


def test_clamp_family_is_present(sets):
    """Directions with exact +-0 components, components below 1e-18 (1/d beyond the +-1e18 clamp) and subnormal ones."""
    d = np.concatenate([rs.d for rs, _ in sets])
    a = np.abs(d)
    assert (d == 0).any(1).sum() > 2000
    assert (np.signbit(d) & (d == 0)).any(1).sum() > 500  # -0 as well as +0
    assert ((a > 0) & (a < 1e-18)).any(1).sum() > 2000
    assert ((a > 0) & (a < np.finfo(np.float32).tiny)).any(1).sum() > 500


def _reversed(sc):
    """The scene with the objects in reverse order and every mesh's triangles in reverse order: the reference's scan
    order reversed, the geometry the same."""
    objs, tris = [], []
    for i in reversed(range(sc.n_objs)):
        o = sc.objs[i]
        if o.kind == ptlib.PT_MESH:
            seg = [sc.tris[k] for k in range(o.tri_offset, o.tri_offset + o.tri_count)][::-1]
            objs.append(ptlib.make_mesh(list(o.position), list(o.color), list(o.emission), o.reflect_type, len(tris),
                                        o.tri_count, list(o.bs_center), o.bs_radius))
            tris.extend(seg)
        else:
            objs.append(o)
    return ptlib.Scene(sc.id + "_rev", sc.cam, objs, tris)


def test_exact_ties_occur(sets):
    """The ties family holds rays whose closest hit is an exact tie - the scan order decides - of every kind: duplicated
    triangles in one mesh, coincident BVH meshes, coplanar overlapping triangles, coincident spheres, a sphere and a
    triangle at the same distance.  Found as the rays whose winner changes when the scan order is reversed."""
    rs, (t, oid, tid) = [s for s in sets if s[0].scene.id == "ties"][0]
    sc = rs.scene
    rev = _reversed(sc)
    t2, oid2, tid2, _, _ = ptlib.oracle_intersect(rev, rs.o, rs.d)
    n = sc.n_objs
    back_obj = np.where(oid2 < 0, -1, n - 1 - oid2)
    cnt = np.array([sc.objs[i].tri_count if sc.objs[i].kind == ptlib.PT_MESH else 0 for i in range(n)])
    back_tri = np.where(tid2 < 0, -1, cnt[np.maximum(back_obj, 0)] - 1 - tid2)
    hit = oid >= 0
    assert np.array_equal(hit, oid2 >= 0)
    assert np.array_equal(t[hit].view(np.uint32), t2[hit].view(np.uint32))  # the same distance whichever wins
    tie = hit & ((back_obj != oid) | (back_tri != tid))
    kind = np.array([sc.objs[i].kind for i in range(n)])
    sph = lambda o: kind[np.maximum(o, 0)] == ptlib.PT_SPHERE
    within_mesh = tie & (back_obj == oid)
    mesh_mesh = tie & (back_obj != oid) & ~sph(oid) & ~sph(back_obj)
    sph_sph = tie & sph(oid) & sph(back_obj)
    sph_tri = tie & (sph(oid) != sph(back_obj))
    for name, m in (("within a mesh", within_mesh), ("mesh and mesh", mesh_mesh), ("sphere and sphere", sph_sph),
                    ("sphere and triangle", sph_tri)):
        assert m.sum() >= (10 if name == "sphere and triangle" else 20), (name, int(m.sum()))
    # the reference keeps the first in scan order: the reversed scan keeps the other one
    assert np.all(oid[mesh_mesh | sph_sph] > back_obj[mesh_mesh | sph_sph])


def test_tables_are_the_products(sets):
    """Consistency of the dumped tables: the helper calls the library's own host::flatten_scene, the function
    pt_ctx_set_scene uploads from (tests/test_gpu_boundary_rays.py checks on the device that each scene gets the pass kernel
    its dump implies; no entry point reports the table sizes).  Here: tri_rank inverts
    rank_id, one BVH per mesh of kBvhMinTris (16) or more triangles, the four-wide tree is the smaller, the filter records add up, the
    references fit the walkers' 26 bits, and the largest mesh has more nodes than the LDS stages (512)."""
    L = ptlib.product()
    most = 0
    for rs, _ in sets:
        sc, tb = rs.scene, rs.tables
        n = sc.n_objs
        assert len(tb["tri_rank"]) == sc.n_tris and len(np.unique(tb["tri_rank"])) == sc.n_tris
        assert np.array_equal(tb["rank_id"][tb["tri_rank"]], n + np.arange(sc.n_tris))
        big = [i for i in range(n) if sc.objs[i].kind == ptlib.PT_MESH and sc.objs[i].tri_count >= 16]
        assert len(tb["bvh_meshes"]) == len(big), sc.id
        assert (len(tb["bvh_nodes"]) > 0) == any(sc.objs[i].tri_count > 2 * 2 for i in big)
        assert len(tb["bvh_nodes4"]) <= len(tb["bvh_nodes"])
        assert all(tb["objs"]["bvh_root"][i] != 0x7fffffff for i in big)
        halves = int((tb["flat_pairs"]["pair"] != br.NO_PAIR).sum())
        assert len(tb["cand_pairs"]) == tb["n_other_pairs"] + halves and tb["cand_ok"]
        assert L.pt_bvh_refs_fit(len(tb["bvh_nodes"]), len(tb["tri_pairs"])) == 1
        most = max(most, len(tb["bvh_nodes"]))
        # (a second dump of the same scene gives the same bytes: the tables are a function of the scene)
        assert np.array_equal(br.scene_tables(sc)["bvh_nodes"].view(np.uint8), tb["bvh_nodes"].view(np.uint8))
    assert most > 512


def test_walls_get_the_sign_rule_only_when_axis_perpendicular(sets):
    """Axis-perpendicular walls get FlatPairRec.sign_exact; walls tilted by 1e-7, 1e-5 and 1e-3 rad are no flat records
    at all; the record holding the sliver keeps the conservative distance test."""
    rs = [s for s, _ in sets if s.scene.id == "walls"][0]
    sc, tb = rs.scene, rs.tables
    owner = {}
    for i in range(sc.n_objs):
        for k in range(sc.objs[i].tri_offset, sc.objs[i].tri_offset + sc.objs[i].tri_count):
            owner[k] = i
    exact_of = {}
    for k in range(len(tb["flat_pairs"])):
        for hf in range(2):
            for tri in br.flat_record_triangles(sc, tb, k, hf):
                exact_of[owner[tri]] = int(tb["flat_pairs"]["sign_exact"][k])
    assert [exact_of.get(i) for i in range(sc.n_objs)] == [1, 1, 1, 1, None, None, None, 0], exact_of


def test_ray_set_is_a_function_of_the_seed():
    a, b, c = br.build(SEED, per_kind=40), br.build(SEED, per_kind=40), br.build(SEED + 1, per_kind=40)
    assert [s.scene.id for s in a] == [s.scene.id for s in b]
    for x, y in zip(a, b):
        assert np.array_equal(x.o.view(np.uint32), y.o.view(np.uint32)) and np.array_equal(x.d.view(np.uint32), y.d.view(np.uint32))
        assert np.array_equal(x.kind, y.kind)
        assert bytes(x.scene.tris)[:x.scene.n_tris * 36] == bytes(y.scene.tris)[:y.scene.n_tris * 36]
    assert any(not np.array_equal(x.o, z.o) for x, z in zip(a, c) if x.o.shape == z.o.shape) or \
        any(x.o.shape != z.o.shape for x, z in zip(a, c))


def test_tables_dump_is_clean_under_the_sanitizers(tmp_path):
    """tests/boundary_rays.py asks the plain build of host/tables_dump.cpp (GPU tests come through it); here the build under
    AddressSanitizer and UBSan runs on the smallest scene of build_scenes: it exits 0, prints what the plain build prints and
    writes the same bytes."""
    sc = min((s for _, s in br.build_scenes(SEED)), key=lambda s: s.n_objs + s.n_tris)
    path = br.write_scene(sc, tmp_path / "scene.bin")
    said = [ptlib.host_program("tables_dump", sanitize=san)(path, tmp_path / ("tables%d.bin" % san)) for san in (True, False)]
    assert said[0] == said[1] and said[0].startswith("OK ")
    assert (tmp_path / "tables1.bin").read_bytes() == (tmp_path / "tables0.bin").read_bytes() != b""
