// object_check — pt_ctx_set_object's host side under a sanitizer, as a program of its own (make object-check builds it with
// -fsanitize=address,undefined and runs it; no device, no Python).  The refusals in the header's order; the reach test at its
// edges and the growth rule; edit_object's tables against flatten_scene of the edited scene under the same origin box; the refit
// plan run on the host through the functions the kernels call (pt_refit.h) - whole tables equal on exact fixtures, records and
// normals equal and every box conservative on inexact moves; two meshes with a BVH, of which only the moved one changes.  A
// failed check or a sanitizer report ends it with a non-zero status.
// argv[1]: the directory that holds meshes/ (the built-in "mesh" scene loads its OFF file from there).
#include <algorithm>

#include "check_common.h"
#include "../csrc/pt_host.h"

using namespace pt;
using host::FlatScene;
using host::Reach;

template <class T>
static bool same_table(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

struct Scene {
    pt_camera cam;
    std::vector<pt_object> objs;
    std::vector<pt_triangle> tris;
};

// A terrain of q x q quads, two triangles each, the first n of them: every coordinate a multiple of 1/8 (`exact`), heights from
// a generator so that no two SAH costs tie
static void terrain(uint32_t q, uint32_t n, uint32_t seed, std::vector<pt_triangle> &out) {
    std::vector<float> h((size_t)(q + 1u) * (q + 1u));
    uint32_t s = seed;
    for (float &v : h) v = (float)(lcg(s) >> 26) * 0.125f;
    auto vert = [&](uint32_t i, uint32_t j, float v[3]) {
        v[0] = (float)i * 0.375f - 1.0f, v[1] = h[(size_t)i * (q + 1u) + j], v[2] = (float)j * 0.625f - 2.0f;
    };
    uint32_t made = 0;
    for (uint32_t i = 0; i < q && made < n; ++i)
        for (uint32_t j = 0; j < q && made < n; ++j) {
            pt_triangle a, b;
            vert(i, j, a.a), vert(i + 1, j, a.b), vert(i + 1, j + 1, a.c);
            vert(i, j, b.a), vert(i + 1, j + 1, b.b), vert(i, j + 1, b.c);
            out.push_back(a), ++made;
            if (made < n) out.push_back(b), ++made;
        }
}

static pt_object mesh_object(const std::vector<pt_triangle> &tris, uint32_t off, uint32_t n, float px, float py, float pz) {
    pt_object o{};
    o.kind = PT_MESH;
    o.position[0] = px, o.position[1] = py, o.position[2] = pz;
    o.color[0] = 0.75f, o.color[1] = 0.5f, o.color[2] = 0.25f;
    o.reflect_type = PT_DIFFUSE;
    o.tri_offset = off, o.tri_count = n;
    host::mesh_bounding_sphere(tris.data() + off, n, o.bs_center, &o.bs_radius);
    return o;
}

static pt_object sphere_object(float px, float py, float pz, float r) {
    pt_object o{};
    o.kind = PT_SPHERE;
    o.position[0] = px, o.position[1] = py, o.position[2] = pz;
    o.radius = r;
    o.color[0] = o.color[1] = o.color[2] = 0.5f;
    o.emission[0] = 2.0f;
    return o;
}

// what pt_ctx_set_object does to its host tables on an in-reach edit, with the refit run on the host: fs is the FULL FlatScene
static bool apply_edit(FlatScene &fs, const Reach &B, Scene &sc, uint32_t index, const pt_object &to) {
    const bool moved = !host::same_geometry(to, sc.objs[index]);
    sc.objs[index] = to;
    host::ObjectEdit e;
    host::edit_object(fs, B, sc.objs.data(), (uint32_t)sc.objs.size(), sc.tris.data(), index, moved, e);
    for (size_t k = 0; k < e.surf.size(); ++k) fs.surf[e.rank + k] = e.surf[k];
    for (size_t k = 0; k < e.tail.size(); ++k) fs.surf[e.tail_at + k] = e.tail[k];
    if (!e.on_device) return true;
    if (moved) {
        host::RefitPlan plan;
        if (!host::build_refit_plan(fs, index, plan)) return false;
        RefitTables T{};
        T.tri_pairs = fs.tri_pairs.data(), T.tri_shade = fs.tri_shade.data(), T.surf = fs.surf.data();
        T.nodes = fs.bvh_nodes.data(), T.nodes4 = fs.bvh_nodes4.data(), T.tri_rank = fs.tri_rank.data();
        T.local = sc.tris.data() + to.tri_offset, T.tri_offset = to.tri_offset;
        T.px = to.position[0], T.py = to.position[1], T.pz = to.position[2];
        T.scene_R = e.scene_R;
        host::run_refit_plan(plan, T);
    }
    for (uint32_t k = 0; k < to.tri_count; ++k) surf_material(fs.surf[e.rank + k], fs.mats[index], true);
    return true;
}

static bool flatten(const Scene &sc, FlatScene &fs, const Reach *B, Reach *used) {
    std::string err;
    return host::flatten_scene(sc.cam, sc.objs.data(), (uint32_t)sc.objs.size(), sc.tris.data(), (uint32_t)sc.tris.size(), fs, err, B, used);
}

// every table and count; the first one that differs is named on stderr
static bool same_tables(const FlatScene &a, const FlatScene &b) {
    const char *differ = nullptr;
#define PT_X(ID, T, name) \
    if (!differ && !same_table(a.name, b.name)) differ = #name;
    PT_SCENE_TABLES(PT_X)
#undef PT_X
    if (!differ && !(a.n_other_pairs == b.n_other_pairs && a.n_flat_exact == b.n_flat_exact &&
                     std::equal(a.n_flat_exact_axis, a.n_flat_exact_axis + 3, b.n_flat_exact_axis) && a.cand_ok == b.cand_ok))
        differ = "the counts";
    if (differ) fprintf(stderr, "same_tables: %s differ\n", differ);
    return !differ;
}

// the tables that hold no tree: equal whatever the trees are
static bool same_small_tables(const FlatScene &a, const FlatScene &b) {
    return same_table(a.mats, b.mats) && same_table(a.tri_shade, b.tri_shade) && same_table(a.sph_pairs, b.sph_pairs) &&
           same_table(a.flat_pairs, b.flat_pairs) && same_table(a.cand_pairs, b.cand_pairs) && same_table(a.surf, b.surf) &&
           a.n_other_pairs == b.n_other_pairs && a.n_flat_exact == b.n_flat_exact &&
           std::equal(a.n_flat_exact_axis, a.n_flat_exact_axis + 3, b.n_flat_exact_axis) && a.cand_ok == b.cand_ok;
}

// the (bounding) spheres of the objects and of the meshes that have a BVH, and the shortcut radii: no tree enters them
static bool same_spheres(const FlatScene &a, const FlatScene &b) {
    if (a.objs.size() != b.objs.size() || a.bvh_meshes.size() != b.bvh_meshes.size()) return false;
    for (size_t i = 0; i < a.objs.size(); ++i) {
        const float x[5] = {a.objs[i].cx, a.objs[i].cy, a.objs[i].cz, a.objs[i].rr, a.objs[i].rr_in};
        const float y[5] = {b.objs[i].cx, b.objs[i].cy, b.objs[i].cz, b.objs[i].rr, b.objs[i].rr_in};
        const ObjPairRec &p = a.obj_pairs[(a.objs.size() - 1u - i) / 2u], &q = b.obj_pairs[(a.objs.size() - 1u - i) / 2u];
        const size_t hf = (a.objs.size() - 1u - i) & 1u;
        if (memcmp(x, y, sizeof x) != 0 || p.cx[hf] != q.cx[hf] || p.cy[hf] != q.cy[hf] || p.cz[hf] != q.cz[hf] || p.rr[hf] != q.rr[hf] ||
            p.admit[hf] != q.admit[hf] || p.obj[hf] != q.obj[hf])
            return false;
    }
    for (size_t m = 0; m < a.bvh_meshes.size(); ++m)
        if (memcmp(&a.bvh_meshes[m], &b.bvh_meshes[m], 4 * sizeof(float)) != 0) return false;
    return true;
}

// Trees that may differ in topology: the record halves of every triangle equal by id; every leaf box of `a` holds its
// triangles' padded boxes, every node box its children's, every four-wide box is the binary one it was widened from
static bool refit_is_sound(const FlatScene &a, const FlatScene &b, const Scene &sc, const Reach &B) {
    const float scene_R = length(mk(B.hi[0] - B.lo[0], B.hi[1] - B.lo[1], B.hi[2] - B.lo[2]));
    std::vector<const TriPairRec *> rec_b(sc.tris.size(), nullptr);
    std::vector<uint32_t> half_b(sc.tris.size(), 0u), owner(sc.tris.size(), 0u);
    for (const TriPairRec &r : b.tri_pairs)
        for (uint32_t hf = 0; hf < 2u; ++hf)
            if (r.id[hf] != kNoTri) rec_b[r.id[hf]] = &r, half_b[r.id[hf]] = hf;
    for (uint32_t i = 0; i < sc.objs.size(); ++i)
        for (uint32_t k = 0; sc.objs[i].kind == PT_MESH && k < sc.objs[i].tri_count; ++k) owner[sc.objs[i].tri_offset + k] = i;
    size_t seen = 0;
    for (const TriPairRec &r : a.tri_pairs)
        for (uint32_t hf = 0; hf < 2u; ++hf) {
            if (r.id[hf] == kNoTri) {
                const float z[9] = {r.ax[hf], r.ay[hf], r.az[hf], r.e1x[hf], r.e1y[hf], r.e1z[hf], r.e2x[hf], r.e2y[hf], r.e2z[hf]};
                for (float v : z)
                    if (v != 0.0f) return false;
                continue;
            }
            const TriPairRec *q = rec_b[r.id[hf]];
            if (!q) return false;
            const uint32_t h2 = half_b[r.id[hf]];
            const float x[9] = {r.ax[hf], r.ay[hf], r.az[hf], r.e1x[hf], r.e1y[hf], r.e1z[hf], r.e2x[hf], r.e2y[hf], r.e2z[hf]};
            const float y[9] = {q->ax[h2], q->ay[h2], q->az[h2], q->e1x[h2], q->e1y[h2], q->e1z[h2], q->e2x[h2], q->e2y[h2], q->e2z[h2]};
            if (memcmp(x, y, sizeof x) != 0) return false;
            ++seen;
        }
    if (seen != sc.tris.size()) return false;
    auto holds = [](const BvhNode &n, uint32_t h, vec3 lo, vec3 hi) {
        return n.lox[h] <= lo.x && n.loy[h] <= lo.y && n.loz[h] <= lo.z && n.hix[h] >= hi.x && n.hiy[h] >= hi.y && n.hiz[h] >= hi.z;
    };
    for (const BvhNode &n : a.bvh_nodes)
        for (uint32_t h = 0; h < 2u; ++h) {
            if (n.c[h] < 0) {
                const uint32_t code = (uint32_t)~n.c[h];
                for (uint32_t r = 0; r < leaf_count(code); ++r)
                    for (uint32_t hf = 0; hf < 2u; ++hf) {
                        const uint32_t id = a.tri_pairs[leaf_first(code) + r].id[hf];
                        if (id == kNoTri) continue;
                        const pt_object &o = sc.objs[owner[id]];
                        const WorldTri w = world_triangle(sc.tris[id], mk(o.position[0], o.position[1], o.position[2]), scene_R);
                        if (!holds(n, h, w.lo, w.hi)) return false;
                    }
            } else {
                const BvhNode &k = a.bvh_nodes[(size_t)n.c[h]];
                for (uint32_t g = 0; g < 2u; ++g)
                    if (!holds(n, h, mk(k.lox[g], k.loy[g], k.loz[g]), mk(k.hix[g], k.hiy[g], k.hiz[g]))) return false;
            }
        }
    for (size_t d = 0; d < a.wide_src.size(); ++d) {
        const BvhNode4 &w = a.bvh_nodes4[d >> 2];
        const uint32_t j = (uint32_t)d & 3u, src = a.wide_src[d];
        if (src == kRefitNone) {
            if (!std::isnan(w.lox[j]) || !std::isnan(w.hiz[j])) return false;
            continue;
        }
        const BvhNode &n = a.bvh_nodes[src >> 1];
        const uint32_t h = src & 1u;
        const float x[6] = {w.lox[j], w.loy[j], w.loz[j], w.hix[j], w.hiy[j], w.hiz[j]};
        const float y[6] = {n.lox[h], n.loy[h], n.loz[h], n.hix[h], n.hiy[h], n.hiz[h]};
        if (memcmp(x, y, sizeof x) != 0) return false;
    }
    return true;
}

int main(int argc, char **argv) {
    const char *base = argc > 1 ? argv[1] : ".";
    // ---- 1. the refusals, in the header's order: each one with everything after it wrong too
    {
        std::vector<pt_triangle> tris;
        terrain(4, 20, 1u, tris);
        const pt_object objs[2] = {sphere_object(0, 0, 0, 1), mesh_object(tris, 0, 20, 0, 0, 0)};
        pt_object bad = objs[1];
        bad.kind = PT_SPHERE, bad.reflect_type = 7u, bad.position[1] = NAN;
        CHECK(refused(host::check_object_edit(false, nullptr, false, nullptr, 0, 9), "ctx is NULL"));
        CHECK(refused(host::check_object_edit(true, nullptr, false, nullptr, 0, 9), "obj is NULL"));
        CHECK(refused(host::check_object_edit(true, &bad, false, nullptr, 0, 9), "no scene"));
        CHECK(refused(host::check_object_edit(true, &bad, true, objs, 2, 2), "index"));
        CHECK(refused(host::check_object_edit(true, &bad, true, objs, 2, 1), "topology"));
        bad.kind = PT_MESH, bad.tri_offset = 1;
        CHECK(refused(host::check_object_edit(true, &bad, true, objs, 2, 1), "topology"));
        bad.tri_offset = 0, bad.tri_count = 19;
        CHECK(refused(host::check_object_edit(true, &bad, true, objs, 2, 1), "topology"));
        bad.tri_count = 20;
        CHECK(refused(host::check_object_edit(true, &bad, true, objs, 2, 1), "reflect_type"));
        bad.reflect_type = PT_REFRACT;
        CHECK(refused(host::check_object_edit(true, &bad, true, objs, 2, 1), "not finite"));
        bad.position[1] = 0.0f;
        for (float *f : {&bad.position[2], &bad.radius, &bad.bs_center[0], &bad.bs_radius}) {
            const float keep = *f;
            *f = INFINITY;
            CHECK(refused(host::check_object_edit(true, &bad, true, objs, 2, 1), "not finite"));
            *f = keep;
        }
        // the material, last: a component of color or emission that is negative or not finite, the message naming the field
        for (int k = 0; k < 6; ++k) {
            float *f = k < 3 ? &bad.color[k] : &bad.emission[k - 3];
            const float keep = *f;
            for (float v : {-1.0f, -1e-45f, NAN, INFINITY, -INFINITY}) {
                *f = v;
                CHECK(refused(host::check_object_edit(true, &bad, true, objs, 2, 1), k < 3 ? "of color is negative or not finite"
                                                                                           : "of emission is negative or not finite"));
            }
            for (float v : {-0.0f, 0.0f, 1e-45f, 3e38f}) {
                *f = v;
                CHECK(host::check_object_edit(true, &bad, true, objs, 2, 1) == PT_OK);
            }
            *f = keep;
        }
        CHECK(host::check_object_edit(true, &bad, true, objs, 2, 1) == PT_OK);
    }
    // ---- 2. the reach test at its edges and the growth rule
    {
        const Reach B = {{-4.0f, -2.0f, -8.0f}, {3.0f, 2.0f, 8.0f}};
        Reach none{}, box;
        pt_object s = sphere_object(2.0f, 0.0f, 0.0f, -1.0f);  // |radius|
        host::object_bounds(s, none, box);
        CHECK(box.lo[0] == 1.0f && box.hi[0] == 3.0f && box.lo[1] == -1.0f && box.hi[2] == 1.0f);
        CHECK(B.holds(box));  // a bound equal to B's is inside
        s.position[0] = nextafterf(2.0f, 3.0f);
        host::object_bounds(s, none, box);
        CHECK(box.hi[0] == nextafterf(3.0f, 4.0f) && !B.holds(box));  // one ulp beyond is outside
        std::vector<pt_triangle> tris;
        terrain(4, 32, 3u, tris);
        Reach local, moved, direct;
        host::local_vertex_box(tris.data(), 32, local);
        pt_object m = mesh_object(tris, 0, 32, 0.1f, -1.0f / 3.0f, 0.07f);
        host::object_bounds(m, local, moved);
        Scene sc{camera(0, 0, 0, 0, 0, 1), {m}, tris};
        sc.cam.focal_length = 0.0f;
        memcpy(sc.cam.position, tris[0].a, sizeof sc.cam.position);
        for (int a = 0; a < 3; ++a) sc.cam.position[a] += m.position[a];  // (a lens centre on the mesh: the box is the mesh's)
        host::scene_reach(sc.cam, sc.objs.data(), 1, tris.data(), 32, direct);
        CHECK(memcmp(&moved, &direct, sizeof moved) == 0);  // local box + position IS the box of the translated vertices
        Reach G = B;
        const Reach out = {{-5.0f, -1.0f, 0.0f}, {1.0f, 2.5f, 8.0f}};
        CHECK(host::grow_reach_box(G, out));
        CHECK(G.lo[0] == -6.0f && G.hi[0] == 3.0f && G.lo[1] == -2.0f && G.hi[1] == 3.0f && G.lo[2] == -8.0f && G.hi[2] == 8.0f);
        CHECK(G.holds(out) && G.holds(B));
        const Reach again = G;
        CHECK(!host::grow_reach_box(G, out) && memcmp(&G, &again, sizeof G) == 0);
        const Reach further = {{-6.5f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};  // a second, smaller push: half of what the first one reserved
        CHECK(!again.holds(further) && host::grow_reach_box(G, further) && G.lo[0] == -7.0f);
    }
    // ---- 3. spheres and listed meshes (cornell.json): edit_object's tables ARE flatten_scene's under the same box, inexact moves
    {
        pt_scene *ps = nullptr;
        CHECK(pt_scene_builtin("cornell", base, &ps) == PT_OK);
        uint32_t n_objs = 0, n_tris = 0;
        const pt_object *o0 = pt_scene_objects(ps, &n_objs);
        const pt_triangle *t0 = pt_scene_triangles(ps, &n_tris);
        Scene sc{*pt_scene_camera(ps), std::vector<pt_object>(o0, o0 + n_objs), std::vector<pt_triangle>(t0, t0 + n_tris)};
        pt_scene_free(ps);
        Reach B;
        FlatScene fs;
        CHECK(flatten(sc, fs, nullptr, &B));
        for (int a = 0; a < 3; ++a) B.lo[a] -= 1.0f, B.hi[a] += 1.0f;  // room to move in
        CHECK(flatten(sc, fs, &B, nullptr));
        uint32_t edits = 0;
        for (uint32_t i = 0; i < n_objs; ++i) {
            pt_object to = sc.objs[i];
            to.position[0] += 0.1f, to.position[1] -= 1.0f / 3.0f, to.position[2] += 0.07f;
            if (i % 3u == 0u) to.reflect_type = (to.reflect_type + 1u) % 3u, to.color[1] *= 0.5f;
            CHECK(host::check_object_edit(true, &to, true, sc.objs.data(), n_objs, i) == PT_OK);
            CHECK(apply_edit(fs, B, sc, i, to));
            FlatScene fresh;
            Reach used;
            CHECK(flatten(sc, fresh, &B, &used));
            CHECK(memcmp(&used, &B, sizeof B) == 0);
            CHECK(same_tables(fs, fresh));
            ++edits;
        }
        CHECK(edits >= 8u && fs.bvh_nodes.empty() && !fs.flat_pairs.empty());
        // a material edit alone touches no geometry table
        const FlatScene before = fs;
        pt_object to = sc.objs[0];
        to.emission[0] = 3.0f, to.reflect_type = PT_REFRACT;
        CHECK(apply_edit(fs, B, sc, 0, to));
        CHECK(same_table(fs.objs, before.objs) && same_table(fs.tri_pairs, before.tri_pairs) && same_table(fs.cand_pairs, before.cand_pairs) &&
              same_table(fs.flat_pairs, before.flat_pairs) && same_table(fs.sph_pairs, before.sph_pairs) && same_table(fs.tri_shade, before.tri_shade));
        FlatScene fresh;
        CHECK(flatten(sc, fresh, &B, nullptr) && same_tables(fs, fresh));
    }
    // ---- 4. meshes with a BVH: 16 (the smallest), 17 (a half-filled record), 19 (the cnt == 3 split), one with a zero-area
    // triangle, 5 000 (a dozen heights, leaves and root included).  Exact moves: the tables of a fresh build, whole.  Inexact ones: sound.
    for (uint32_t n : {16u, 17u, 19u, 64u, 5000u}) {
        Scene sc;
        sc.cam = camera(0.5f, 7.0f, -14.0f, 0.0f, -0.3125f, 1.0f);
        terrain(n > 1000u ? 50u : 6u, n, 7u + n, sc.tris);
        CHECK(sc.tris.size() == n);
        if (n == 64u) {
            memcpy(sc.tris[5].b, sc.tris[5].a, sizeof sc.tris[5].a);   // a zero-length edge: the normal is NaN
            memcpy(sc.tris[9].c, sc.tris[9].b, sizeof sc.tris[9].b);   // zero area
        }
        // (the scene of tests/test_gpu_set_object.py: a floor sphere whose box holds every move made here, the terrain, a light)
        sc.objs = {sphere_object(0.0f, -64.0f, 0.0f, 62.0f), mesh_object(sc.tris, 0, n, 0.0f, 0.0f, 0.0f), sphere_object(2.0f, 14.0f, -1.0f, 3.0f)};
        Reach B;
        FlatScene fs;
        CHECK(flatten(sc, fs, nullptr, &B));
        CHECK(fs.objs[1].bvh_root != kNoBvh && fs.bvh_meshes.size() == 1u);
        host::RefitPlan plan;
        CHECK(host::build_refit_plan(fs, 1, plan) && !host::build_refit_plan(fs, 0, plan));
        CHECK(host::build_refit_plan(fs, 1, plan));
        CHECK(plan.nodes.size() + 1u == fs.bvh_nodes.size() && plan.level_begin.size() >= 2u);
        // 5 000 triangles: 1 476 leaves (six workgroups of the leaf kernel), ten heights of inner nodes below the root (ten launches)
        if (n == 5000u) CHECK(plan.level_begin.size() - 1u >= 10u && plan.leaves.size() > 1024u);
        {
            size_t recs = 0;
            for (const RefitLeaf &lf : plan.leaves) {
                CHECK(lf.count >= 1u && lf.count <= kBvhLeafPairs);
                recs += lf.count;
            }
            CHECK(recs == fs.tri_pairs.size());
        }
        const float exact[3][3] = {{0.125f, -0.5f, 1.0f}, {-2.25f, 0.375f, -0.125f}, {0.0f, 0.0f, 0.0f}};
        for (const float *d : exact) {
            pt_object to = sc.objs[1];
            for (int a = 0; a < 3; ++a) to.position[a] = d[a];
            if (d[0] < 0.0f) to.color[0] = 0.125f, to.reflect_type = PT_SPECULAR;
            CHECK(apply_edit(fs, B, sc, 1, to));
            FlatScene fresh;
            CHECK(flatten(sc, fresh, &B, nullptr));
            CHECK(refit_is_sound(fs, fresh, sc, B) && same_small_tables(fs, fresh));
            CHECK(same_tables(fs, fresh));  // exact arithmetic: the SAH tree of the moved scene is the tree of the original
        }
        uint32_t s = 99u;
        for (int step = 0; step < 4; ++step) {
            pt_object to = sc.objs[1];
            to.position[0] = 0.1f + unit(s), to.position[1] = -1.0f / 3.0f * (float)step, to.position[2] = 0.07f - unit(s);
            CHECK(apply_edit(fs, B, sc, 1, to));
            FlatScene fresh;
            CHECK(flatten(sc, fresh, &B, nullptr));
            CHECK(refit_is_sound(fs, fresh, sc, B) && same_small_tables(fs, fresh));
            CHECK(same_spheres(fs, fresh));
        }
    }
    // ---- 5. two meshes with a BVH: the second is moved, the first's ranges are untouched
    {
        Scene sc;
        sc.cam = camera(0.5f, 7.0f, -14.0f, 0.0f, -0.3125f, 1.0f);
        terrain(6, 40, 21u, sc.tris);
        terrain(6, 33, 22u, sc.tris);
        sc.objs = {sphere_object(0.0f, -64.0f, 0.0f, 62.0f), mesh_object(sc.tris, 0, 40, -3.0f, 0.0f, 0.0f),
                   mesh_object(sc.tris, 40, 33, 3.0f, 0.0f, 0.0f), sphere_object(2.0f, 14.0f, -1.0f, 3.0f)};
        Reach B;
        FlatScene fs;
        CHECK(flatten(sc, fs, nullptr, &B));
        CHECK(fs.bvh_meshes.size() == 2u);
        const FlatScene before = fs;
        pt_object to = sc.objs[2];
        to.position[0] += 0.1f, to.position[1] -= 1.0f / 3.0f, to.position[2] += 0.07f;
        CHECK(apply_edit(fs, B, sc, 2, to));
        const ObjRec &first = before.objs[1], &second = before.objs[2];
        CHECK(memcmp(&fs.tri_pairs[first.pair_begin], &before.tri_pairs[first.pair_begin], first.pair_count * sizeof(TriPairRec)) == 0);
        CHECK(memcmp(&fs.tri_pairs[second.pair_begin], &before.tri_pairs[second.pair_begin], second.pair_count * sizeof(TriPairRec)) != 0);
        CHECK(memcmp(&fs.tri_shade[0], &before.tri_shade[0], 40 * sizeof(TriShade)) == 0);
        host::RefitPlan p0, p2;
        CHECK(host::build_refit_plan(fs, 1, p0) && host::build_refit_plan(fs, 2, p2));
        std::vector<uint8_t> mine(fs.bvh_nodes.size(), 0);
        for (const RefitNode &nd : p2.nodes) mine[nd.node] = 1, mine[nd.parent] = 1;
        for (const RefitNode &nd : p0.nodes) CHECK(!mine[nd.node] && !mine[nd.parent]);
        for (size_t i = 0; i < fs.bvh_nodes.size(); ++i)
            if (!mine[i]) CHECK(memcmp(&fs.bvh_nodes[i], &before.bvh_nodes[i], sizeof(BvhNode)) == 0);
        for (const RefitWide &w : p0.wide) {
            const BvhNode4 &x = fs.bvh_nodes4[w.dst >> 2], &y = before.bvh_nodes4[w.dst >> 2];
            CHECK(memcmp(&x, &y, sizeof x) == 0);
        }
        FlatScene fresh;
        CHECK(flatten(sc, fresh, &B, nullptr));
        CHECK(refit_is_sound(fs, fresh, sc, B) && same_small_tables(fs, fresh) && same_spheres(fs, fresh));
        // and the first one, exactly: whole tables again
        pt_object to0 = sc.objs[1];
        to0.position[1] += 0.25f;
        to = sc.objs[2];
        to.position[0] = 3.5f, to.position[1] = 0.0f, to.position[2] = 0.0f;
        CHECK(apply_edit(fs, B, sc, 1, to0) && apply_edit(fs, B, sc, 2, to));
        CHECK(flatten(sc, fresh, &B, nullptr));
        CHECK(same_tables(fs, fresh));
    }
    printf("object_check: ok\n");
    return 0;
}
