"""The ladder of LDS-layout cliffs (tests/lds_layouts.py), without a GPU: every layout lds_layout can choose is reached on both
sides of its cliff, each pair differs in exactly its decision, and the ladder depends on its seed alone.  Also prints which of
those layouts the scenes the rest of the suite renders reach (at one pixel per stream: pt_ctx_radiance and the small frames)."""
import numpy as np

import boundary_rays as br
import lds_layouts as ll
import ptlib

SEED = 20261016


def _scene_bytes(sc):
    return bytes(sc.cam) + bytes(sc.objs)[:sc.n_objs * 128] + bytes(sc.tris)[:sc.n_tris * 36]


def test_every_layout_on_both_sides_of_its_cliff(capsys):
    ladder = ll.build(SEED)
    assert [name for name, _, _ in ladder] == [c["name"] for c in ll.CLIFFS]
    reached = set()
    for (name, a, b), cl in zip(ladder, ll.CLIFFS):
        # one step of the knob apart, the decision flips, both sides are the layout the cliff is about
        assert b.knob == a.knob + 1, name
        assert cl["decide"](a.L) != cl["decide"](b.L), name
        assert cl["pre"](a.L) and cl["pre"](b.L), (name, a.L, b.L)
        # and nothing else changes but what follows from the decision and the knob (bytes, offsets, counts)
        other = {k for k in a.L if k not in ll.DERIVED and a.L[k] != b.L[k]}
        assert other == cl["differs"], (name, other)
        for r in (a, b):
            # the line the library says under PT_LDS_PAD is the layout's own
            assert r.lines[0].startswith(("k_pass_cand: ", "k_pass_cand<BVH>: ", "k_pass: ")), r.lines
            assert ("m = %d," % r.L["m"]) in r.lines[0]
            assert r.lines[2].startswith("k_mega_cand: " if r.L["mega_cand"] else "k_mega: ")
            reached |= ll.kinds(r.L)
    missing = [k for k in ll.LADDER_KINDS if k not in reached]
    assert not missing, missing
    # the stream-length cliffs: a stream one pixel longer, and the pairs of scenes: one record, rank or node more
    m_pairs = [(a.L["m"], b.L["m"]) for name, a, b in ladder if name.endswith("_m")]
    assert m_pairs and all(mb == ma + 1 for ma, mb in m_pairs)
    with capsys.disabled():
        print("\nLDS-layout ladder (seed %d):" % SEED)
        for name, a, b in ladder:
            print("  %-26s knob %5d | %5d   %s" % (name, a.knob, b.knob, sorted(ll.kinds(a.L) ^ ll.kinds(b.L))))


def test_the_ladder_is_a_function_of_its_seed():
    a, b, c = ll.build(SEED), ll.build(SEED), ll.build(SEED + 1)
    for (n1, x1, y1), (n2, x2, y2) in zip(a, b):
        assert n1 == n2 and x1.knob == x2.knob and y1.knob == y2.knob and x1.L == x2.L and y1.L == y2.L
        assert _scene_bytes(x1.scene) == _scene_bytes(x2.scene) and _scene_bytes(y1.scene) == _scene_bytes(y2.scene)
    assert any(_scene_bytes(x1.scene) != _scene_bytes(x3.scene) for (_, x1, _), (_, x3, _) in zip(a, c))


def test_probe_rays_hit_the_ranks_at_the_table_edges():
    """The probe rays of every scene rung (test_gpu_lds_layouts) include the first and last rank, the ranks of the first and last
    candidate record, and - with a partly staged shading table - the last staged rank and the first one outside; and each of
    them first hits (by the oracle) the very sphere or triangle of its rank."""
    n_rays = 0
    for name, a, b in ll.build(SEED):
        for r in (a, b):
            if name.endswith("_m"):
                continue
            tabs = br.scene_tables(r.scene)
            rays = ll.probe_rays(r, tabs)
            got = {t[0] for t in rays}
            n_ranks = r.scene.n_objs + r.scene.n_tris
            assert {0, n_ranks - 1} <= got, name
            if r.L["surf_head"]:
                assert {r.L["surf_head"] - 1, r.L["surf_head"]} <= got, name
            if len(tabs["cand_pairs"]):
                ends = {int(x) for x in np.concatenate([tabs["cand_pairs"]["id"][0], tabs["cand_pairs"]["id"][-1]]) if x != br.NO_TRI}
                assert ends <= got, name
            o = np.array([t[3] for t in rays])
            d = np.array([t[4] for t in rays])
            _, oid, tid, _, _ = ptlib.oracle_intersect(r.scene, o, d)
            assert [(int(x), int(y)) for x, y in zip(oid, tid)] == [(t[1], t[2]) for t in rays], (name, r.side)
            n_rays += len(rays)
    assert n_rays > 100


def test_coverage_of_the_existing_suite(capsys):
    """Which ladder layouts the scenes the rest of the suite renders reach at one pixel per stream (informational)."""
    import test_gpu_parity as tgp

    scenes = [ptlib.load_scene_py(ptlib.scene_path(s)) for s in ("cornell", "mesh", "cartesian", "single-sphere",
                                                                  "two-spheres", "three-spheres")]
    rng = np.random.default_rng(2026)
    scenes += [tgp._random_scene(rng, k) for k in range(40)]
    scenes += [sc for _, sc in br.build_scenes(SEED)]
    old = set()
    for sc in scenes:
        for sw in (0, ll.SW_NO_CAND, ll.SW_DEFER, ll.SW_NO_CAND_BVH, ll.SW_NO_NODES):
            old |= ll.kinds(ll.layout(sc, 1, sw)[0])
    # cornell at 4096^2 (test_largest_frame_geometry): 1024 pixels per stream
    old |= ll.kinds(ll.layout(scenes[0], 1024, 0)[0])
    new = set()
    for _, a, b in ll.build(SEED):
        new |= ll.kinds(a.L) | ll.kinds(b.L)
    with capsys.disabled():
        print("\n%-40s %-14s %s" % ("layout", "old suite", "ladder"))
        for k in ll.LADDER_KINDS:
            print("%-40s %-14s %s" % (k, "yes" if k in old else "no", "yes" if k in new else "no"))
    assert set(ll.LADDER_KINDS) <= new


def test_layout_dump_is_clean_under_the_sanitizers(tmp_path):
    """tests/lds_layouts.py asks the plain build of host/layout_dump.cpp (GPU tests come through it); here the build under
    AddressSanitizer and UBSan runs on one scene with two queries: it exits 0 and prints the plain build's bytes."""
    path = br.write_scene(ll._cornell(), tmp_path / "scene.bin")
    args = (path, "1,0", "64,%d" % ll.SW_DEFER)
    clean = ptlib.host_program("layout_dump")(*args)
    assert clean == ptlib.host_program("layout_dump", sanitize=False)(*args) and clean.count("\n") == 8
