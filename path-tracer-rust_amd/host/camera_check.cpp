// camera_check — pt_ctx_set_camera's host side under a sanitizer, as a program of its own (make camera-check builds it with
// -fsanitize=address,undefined and runs it; no device, no Python).  flatten_scene with and without an origin box on the built-in
// scenes, the growth rule over a scripted walk, and the same walk with the rebuilds it asks for on mesh.json with its mesh
// replaced by a generated one of 20 000 triangles: a failed check or a sanitizer report ends it with a non-zero status.
// argv[1]: the directory that holds meshes/ (the built-in "mesh" scene loads its OFF file from there).
#include "check_common.h"
#include "../csrc/pt_host.h"

using namespace pt;
using host::FlatScene;
using host::Reach;

static bool same_bits(const float *a, const float *b, size_t n) { return memcmp(a, b, n * sizeof(float)) == 0; }

// b's boxes hold a's, component by component (a NaN - an empty slot of a four-wide node - on both sides or on neither)
template <class Node, size_t W>
static bool boxes_hold(const std::vector<Node> &a, const std::vector<Node> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) {
        if (memcmp(a[i].c, b[i].c, sizeof a[i].c) != 0) return false;
        const float *alo[3] = {a[i].lox, a[i].loy, a[i].loz}, *ahi[3] = {a[i].hix, a[i].hiy, a[i].hiz};
        const float *blo[3] = {b[i].lox, b[i].loy, b[i].loz}, *bhi[3] = {b[i].hix, b[i].hiy, b[i].hiz};
        for (int k = 0; k < 3; ++k)
            for (size_t j = 0; j < W; ++j) {
                if (std::isnan(alo[k][j]) != std::isnan(blo[k][j]) || std::isnan(ahi[k][j]) != std::isnan(bhi[k][j])) return false;
                if (blo[k][j] > alo[k][j] || bhi[k][j] < ahi[k][j]) return false;
            }
    }
    return true;
}

// What does not depend on the origin box: the objects, materials, shading records and surfaces, one per object or triangle.  (The
// trees may: the SAH build sees the padded boxes, so leaves and pair records may be cut differently.)
static bool same_counts(const FlatScene &a, const FlatScene &b) {
    return a.objs.size() == b.objs.size() && a.obj_pairs.size() == b.obj_pairs.size() && a.mats.size() == b.mats.size() &&
           a.tri_shade.size() == b.tri_shade.size() && a.surf.size() == b.surf.size() && a.rank_id.size() == b.rank_id.size() &&
           a.tri_rank.size() == b.tri_rank.size() && a.bvh_meshes.size() == b.bvh_meshes.size() && a.bvh_nodes.empty() == b.bvh_nodes.empty() &&
           a.bvh_stack <= kBvhStack && b.bvh_stack <= kBvhStack;
}
// the same box: the same records in the same order, the same trees
static bool same_structure(const FlatScene &a, const FlatScene &b) {
    return a.objs.size() == b.objs.size() && a.obj_pairs.size() == b.obj_pairs.size() && a.tri_pairs.size() == b.tri_pairs.size() &&
           a.mats.size() == b.mats.size() && a.tri_shade.size() == b.tri_shade.size() && a.sph_pairs.size() == b.sph_pairs.size() &&
           a.flat_pairs.size() == b.flat_pairs.size() && a.cand_pairs.size() == b.cand_pairs.size() && a.surf.size() == b.surf.size() &&
           a.bvh_meshes.size() == b.bvh_meshes.size() && a.rank_id == b.rank_id && a.tri_rank == b.tri_rank &&
           a.n_other_pairs == b.n_other_pairs && a.cand_ok == b.cand_ok && a.bvh_stack == b.bvh_stack &&
           a.bvh_pair_base == b.bvh_pair_base && a.bvh_pair_span == b.bvh_pair_span;
}

struct Walk {
    float lens[3];
    bool grows;
};

// in, out on one axis, out on three, back in - around a box B0
static std::vector<Walk> scripted_walk(const Reach &B0) {
    const float cx = 0.5f * (B0.lo[0] + B0.hi[0]), cy = 0.5f * (B0.lo[1] + B0.hi[1]), cz = 0.5f * (B0.lo[2] + B0.hi[2]);
    const float ex = B0.hi[0] - B0.lo[0] + 1.0f, ey = B0.hi[1] - B0.lo[1] + 1.0f, ez = B0.hi[2] - B0.lo[2] + 1.0f;
    return {{{cx, cy, cz}, false},
            {{B0.lo[0], B0.hi[1], cz}, false},  // on the boundary: inside
            {{B0.hi[0] + 0.25f * ex, cy, cz}, true},
            {{B0.hi[0] + 0.4f * ex, cy, cz}, false},  // inside what the step before reserved (the overshoot doubled)
            {{B0.lo[0] - ex, B0.lo[1] - 0.5f * ey, B0.hi[2] + 2.0f * ez}, true},
            {{B0.lo[0] - 1.5f * ex, cy, B0.hi[2] + 3.0f * ez}, false},
            {{cx, cy, cz}, false}};
}

int main(int argc, char **argv) {
    const char *base = argc > 1 ? argv[1] : ".";
    // ---- 1. flatten_scene with and without an origin box, on the built-in scenes
    CHECK(pt_builtin_scene_count() == 6u);
    for (uint32_t s = 0; s < pt_builtin_scene_count(); ++s) {
        pt_scene *sc = nullptr;
        CHECK(pt_scene_builtin(pt_builtin_scene_id(s), base, &sc) == PT_OK);
        uint32_t n_objs = 0, n_tris = 0;
        const pt_object *objs = pt_scene_objects(sc, &n_objs);
        const pt_triangle *tris = pt_scene_triangles(sc, &n_tris);
        const pt_camera cam = *pt_scene_camera(sc);
        std::string err;
        FlatScene plain, own, wide;
        Reach r0, r_plain, r_own, r_wide;
        host::scene_reach(cam, objs, n_objs, tris, n_tris, r0);
        float lens[3], su[3], sv[3];
        host::camera_basis(cam, lens, su, sv);
        CHECK(r0.holds(lens));
        CHECK(host::flatten_scene(cam, objs, n_objs, tris, n_tris, plain, err, nullptr, &r_plain));
        CHECK(same_bits(r_plain.lo, r0.lo, 3) && same_bits(r_plain.hi, r0.hi, 3));
        // its own box, or one inside it, changes nothing at all
        CHECK(host::flatten_scene(cam, objs, n_objs, tris, n_tris, own, err, &r0, &r_own));
        CHECK(same_bits(r_own.lo, r0.lo, 3) && same_bits(r_own.hi, r0.hi, 3));
        CHECK(same_structure(plain, own));
        CHECK(own.bvh_nodes.size() == plain.bvh_nodes.size() &&
              (plain.bvh_nodes.empty() || memcmp(own.bvh_nodes.data(), plain.bvh_nodes.data(), plain.bvh_nodes.size() * sizeof(BvhNode)) == 0));
        CHECK(own.bvh_nodes4.size() == plain.bvh_nodes4.size() &&
              (plain.bvh_nodes4.empty() ||
               memcmp(own.bvh_nodes4.data(), plain.bvh_nodes4.data(), plain.bvh_nodes4.size() * sizeof(BvhNode4)) == 0));
        // a wider one: as many records per object and triangle, root boxes that hold the ones before
        Reach w = r0;
        for (int a = 0; a < 3; ++a) w.lo[a] -= 3.0f + (float)a, w.hi[a] += 7.0f;
        CHECK(host::flatten_scene(cam, objs, n_objs, tris, n_tris, wide, err, &w, &r_wide));
        CHECK(same_bits(r_wide.lo, w.lo, 3) && same_bits(r_wide.hi, w.hi, 3));
        CHECK(same_counts(plain, wide));
        CHECK((boxes_hold<BvhNode, 2>(plain.bvh_nodes, own.bvh_nodes)));
        CHECK((boxes_hold<BvhNode4, 4>(plain.bvh_nodes4, own.bvh_nodes4)));
        pt_scene_free(sc);
    }
    // ---- 2. the growth rule over the scripted walk
    {
        Reach B = {{-1.0f, -2.0f, -3.0f}, {1.0f, 2.0f, 3.0f}};
        for (const Walk &st : scripted_walk(B)) {
            const Reach before = B;
            const bool inside = B.holds(st.lens);
            CHECK(inside == !st.grows);
            CHECK(host::grow_reach(B, st.lens) == st.grows);
            CHECK(B.holds(st.lens) && B.holds(before));
            for (int a = 0; a < 3; ++a) {
                const float lo = st.lens[a] < before.lo[a] ? st.lens[a] - (before.lo[a] - st.lens[a]) : before.lo[a];
                const float hi = st.lens[a] > before.hi[a] ? st.lens[a] + (st.lens[a] - before.hi[a]) : before.hi[a];
                CHECK(same_bits(&B.lo[a], &lo, 1) && same_bits(&B.hi[a], &hi, 1));
            }
        }
        const float nan3[3] = {NAN, 0.0f, 0.0f};
        const Reach before = B;
        CHECK(!B.holds(nan3) && !host::grow_reach(B, nan3) && memcmp(&B, &before, sizeof B) == 0);
    }
    // ---- 3. the walk, with the rebuilds it asks for, on mesh.json's room around a generated mesh of 20 000 triangles
    {
        pt_scene *sc = nullptr;
        CHECK(pt_scene_builtin("mesh", base, &sc) == PT_OK);
        uint32_t n_objs = 0, n_tris = 0;
        const pt_object *o0 = pt_scene_objects(sc, &n_objs);
        const pt_triangle *t0 = pt_scene_triangles(sc, &n_tris);
        pt_camera cam = *pt_scene_camera(sc);
        std::vector<pt_object> objs(o0, o0 + n_objs);
        uint32_t big = n_objs;
        for (uint32_t i = 0; i < n_objs; ++i)
            if (objs[i].kind == PT_MESH && (big == n_objs || objs[i].tri_count > objs[big].tri_count)) big = i;
        CHECK(big < n_objs);
        // a 100 x 100 grid of quads, two triangles each, rippled, as wide as the mesh it replaces; the other meshes keep theirs
        std::vector<pt_triangle> tris;
        const float R = objs[big].bs_radius * 0.5f;
        auto vert = [&](uint32_t i, uint32_t j, float v[3]) {
            const float x = ((float)i / 100.0f - 0.5f) * 2.0f * R, z = ((float)j / 100.0f - 0.5f) * 2.0f * R;
            v[0] = objs[big].bs_center[0] + x;
            v[1] = objs[big].bs_center[1] + 0.1f * R * sinf(9.0f * x / R) * cosf(7.0f * z / R);
            v[2] = objs[big].bs_center[2] + z;
        };
        for (uint32_t i = 0; i < 100u; ++i)
            for (uint32_t j = 0; j < 100u; ++j) {
                pt_triangle a, b;
                vert(i, j, a.a), vert(i + 1, j, a.b), vert(i + 1, j + 1, a.c);
                vert(i, j, b.a), vert(i + 1, j + 1, b.b), vert(i, j + 1, b.c);
                tris.push_back(a);
                tris.push_back(b);
            }
        CHECK(tris.size() == 20000u);
        for (uint32_t i = 0; i < n_objs; ++i) {
            if (objs[i].kind != PT_MESH) continue;
            const uint32_t off = (uint32_t)tris.size();
            if (i == big) {
                objs[i].tri_offset = 0u;
                objs[i].tri_count = 20000u;
                host::mesh_bounding_sphere(tris.data(), 20000u, objs[i].bs_center, &objs[i].bs_radius);
            } else {
                tris.insert(tris.end(), t0 + objs[i].tri_offset, t0 + objs[i].tri_offset + objs[i].tri_count);
                objs[i].tri_offset = off;
            }
        }
        pt_scene_free(sc);
        const uint32_t nt = (uint32_t)tris.size();
        // the objects' box: the reach of a camera whose lens centre sits on an object
        Reach B, obj_box;
        host::scene_reach(cam, objs.data(), n_objs, tris.data(), nt, B);
        {
            pt_camera on = cam;
            memcpy(on.position, tris[0].a, sizeof on.position);
            for (int a = 0; a < 3; ++a) on.position[a] += objs[big].position[a];
            on.focal_length = 0.0f;
            host::scene_reach(on, objs.data(), n_objs, tris.data(), nt, obj_box);
        }
        CHECK(B.holds(obj_box));
        std::string err;
        FlatScene first, fs;
        CHECK(host::flatten_scene(cam, objs.data(), n_objs, tris.data(), nt, first, err));
        CHECK(!first.bvh_nodes.empty());
        uint32_t rebuilds = 0;
        std::vector<Walk> seen;
        for (const Walk &st : scripted_walk(B)) {
            // a camera whose lens centre is the step's point exactly (focal length 0: the lens centre is the position)
            cam.focal_length = 0.0f;
            memcpy(cam.position, st.lens, sizeof cam.position);
            float lens[3], su[3], sv[3];
            host::camera_basis(cam, lens, su, sv);
            const Reach before = B;
            const bool inside = B.holds(lens);
            if (!inside) {
                CHECK(host::grow_reach(B, lens));
                Reach used;
                CHECK(host::flatten_scene(cam, objs.data(), n_objs, tris.data(), nt, fs, err, &B, &used));
                CHECK(memcmp(&used, &B, sizeof B) == 0);  // (B held the objects and the lens centre already)
                CHECK(same_counts(first, fs));
                ++rebuilds;
            } else {
                CHECK(!host::grow_reach(B, lens) && memcmp(&B, &before, sizeof B) == 0);  // no rebuild on a lens centre inside B
            }
            CHECK(B.holds(before));   // B never shrinks
            CHECK(B.holds(obj_box));  // B always holds the objects
            seen.push_back({{lens[0], lens[1], lens[2]}, false});
            for (const Walk &p : seen) CHECK(B.holds(p.lens));  // ... and every lens centre seen
        }
        CHECK(rebuilds == 2u);
    }
    printf("camera_check: ok\n");
    return 0;
}
