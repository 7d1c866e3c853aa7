// flatten_tables_check — host::flatten_scene's tables for the walk queue of k_pass_cand<.., BVH> on a scene file: tri_rank inverts
// rank_id, the BVH mesh list in visiting order, every triangle in exactly one leaf, the four-wide tree against the binary one, the
// advertised stack depth, the candidate records.  argv: SCENE.json and the directory that holds meshes/.  Judges itself (FAIL and
// the table) and prints OK with the number of BVH meshes, the stack depth and the deepest tree, which
// tests/test_host_logic.py (test_flatten_tables_of_the_walk_queue) holds to the two built-in scenes.
#include "check_common.h"
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>
#include "../csrc/pt_host.h"
using namespace pt;
static int depth_of(const host::FlatScene &fs, int32_t ref, std::vector<int> &leaf_hits, uint32_t pair_lo, uint32_t pair_hi, bool &ok) {
    if (ref < 0) {
        const uint32_t code = (uint32_t)~ref, first = leaf_first(code), cnt = leaf_count(code);
        if (cnt < 1 || cnt > kBvhLeafPairs || first < pair_lo || first + cnt > pair_hi) ok = false;
        for (uint32_t r = 0; r < cnt && ok; ++r)
            for (int hf = 0; hf < 2; ++hf)
                if (fs.tri_pairs[first + r].id[hf] != kNoTri) leaf_hits[fs.tri_pairs[first + r].id[hf]]++;
        return 0;
    }
    const BvhNode &n = fs.bvh_nodes[ref];
    const int a = depth_of(fs, n.c[0], leaf_hits, pair_lo, pair_hi, ok), b = depth_of(fs, n.c[1], leaf_hits, pair_lo, pair_hi, ok);
    return 1 + (a > b ? a : b);
}
// the four-wide tree below ref4: every leaf reference it holds, and that each of its boxes is a box of the binary tree
// (the child boxes of some binary node: collected in `bin_boxes` as lo.x of each, a cheap identity)
static void walk4(const host::FlatScene &fs, int32_t ref4, std::vector<int32_t> &leaves, bool &ok, int depth, int &deepest) {
    if (ref4 < 0) { leaves.push_back(ref4); return; }
    if ((size_t)ref4 >= fs.bvh_nodes4.size() || depth > 64) { ok = false; return; }
    deepest = depth > deepest ? depth : deepest;
    const BvhNode4 &n = fs.bvh_nodes4[(size_t)ref4];
    int live = 0;
    for (int j = 0; j < 4; ++j) {
        const bool filler = n.lox[j] != n.lox[j];  // NaN
        if (filler) {
            // a filler box is NaN in every bound (never hit: pt_device.h) and repeats child 0's reference; fillers come last
            if (n.hix[j] == n.hix[j] || n.loy[j] == n.loy[j] || n.hiz[j] == n.hiz[j] || n.c[j] != n.c[0] || j < 2) ok = false;
            continue;
        }
        if (live != j) ok = false;
        ++live;
        bool found = false;  // the box is one of the binary tree's child boxes, with the same reference kind
        for (const BvhNode &b : fs.bvh_nodes)
            for (int h = 0; h < 2; ++h)
                if (b.lox[h] == n.lox[j] && b.loy[h] == n.loy[j] && b.loz[h] == n.loz[j] && b.hix[h] == n.hix[j] && b.hiy[h] == n.hiy[j] &&
                    b.hiz[h] == n.hiz[j] && ((b.c[h] < 0) == (n.c[j] < 0)) && (b.c[h] >= 0 || b.c[h] == n.c[j]))
                    found = true;
        if (!found) ok = false;
        walk4(fs, n.c[j], leaves, ok, depth + 1, deepest);
    }
}
static void leaves2(const host::FlatScene &fs, int32_t ref, std::vector<int32_t> &leaves) {
    if (ref < 0) { leaves.push_back(ref); return; }
    leaves2(fs, fs.bvh_nodes[(size_t)ref].c[0], leaves);
    leaves2(fs, fs.bvh_nodes[(size_t)ref].c[1], leaves);
}
int main(int argc, char **argv) {
    pt_scene *sc = nullptr;
    if (pt_scene_load(argv[1], argv[2], &sc) != 0) { printf("FAIL load %s\n", pt_last_error()); return 1; }
    uint32_t n_objs, n_tris;
    const pt_object *objs = pt_scene_objects(sc, &n_objs);
    const pt_triangle *tris = pt_scene_triangles(sc, &n_tris);
    host::FlatScene fs;
    std::string err;
    if (!host::flatten_scene(*pt_scene_camera(sc), objs, n_objs, tris, n_tris, fs, err)) { printf("FAIL flatten %s\n", err.c_str()); return 1; }
    // ranks: rank_id and tri_rank are inverse on the triangles; objects from the last to the first
    if (fs.tri_rank.size() < n_tris) { printf("FAIL tri_rank size\n"); return 1; }
    for (uint32_t k = 0; k < n_tris; ++k)
        if (fs.rank_id[fs.tri_rank[k]] != n_objs + k) { printf("FAIL tri_rank %u\n", k); return 1; }
    // the BVH mesh list: exactly the objects with a BVH, in visiting order
    size_t q = 0;
    uint32_t deepest = 0;
    for (uint32_t v = 0; v < n_objs; ++v) {
        const ObjRec &r = fs.objs[n_objs - 1u - v];
        if (r.kind != kKindMesh || r.bvh_root == kNoBvh) continue;
        if (q >= fs.bvh_meshes.size() || fs.bvh_meshes[q].root != r.bvh_root || fs.bvh_meshes[q].rr != r.rr ||
            fs.bvh_meshes[q].cx != r.cx) { printf("FAIL bvh_meshes %zu\n", q); return 1; }
        ++q;
        // the tree: every triangle of the mesh in exactly one leaf, leaves within the mesh's records, depth within the stack
        std::vector<int> hits(n_tris, 0);
        bool ok = true;
        const int d = depth_of(fs, r.bvh_root, hits, r.pair_begin, r.pair_begin + r.pair_count, ok);
        if (!ok) { printf("FAIL leaf\n"); return 1; }
        for (uint32_t k = 0; k < n_tris; ++k)
            if (hits[k] != ((k >= r.tri_begin && k < r.tri_begin + r.tri_count) ? 1 : 0)) { printf("FAIL cover %u\n", k); return 1; }
        deepest = (uint32_t)d > deepest ? (uint32_t)d : deepest;
        // the four-wide form of the same tree (the walk queue's): the same leaves in the same order, each once, every box one
        // of the binary tree's, at most half as deep (+1)
        std::vector<int32_t> l2, l4;
        leaves2(fs, r.bvh_root, l2);
        int deep4 = 0;
        walk4(fs, fs.bvh_meshes[q - 1].root4, l4, ok, 1, deep4);
        if (!ok || l2 != l4 || 2 * deep4 > d + 2) { printf("FAIL four-wide tree %d %zu %zu %d %d\n", (int)ok, l2.size(), l4.size(), deep4, d); return 1; }
        if (fs.bvh_nodes4.size() * 2 > fs.bvh_nodes.size() + 2) { printf("FAIL four-wide node count %zu %zu\n", fs.bvh_nodes4.size(), fs.bvh_nodes.size()); return 1; }
    }
    if (q != fs.bvh_meshes.size()) { printf("FAIL bvh_meshes count\n"); return 1; }
    if (q != 0 && (fs.bvh_stack < deepest + 1u || fs.bvh_stack > kBvhStack)) { printf("FAIL stack %u %u\n", fs.bvh_stack, deepest); return 1; }
    // the candidate records are those of the meshes without a BVH
    size_t want = 0;
    for (uint32_t i = 0; i < n_objs; ++i)
        if (fs.objs[i].kind == kKindMesh && fs.objs[i].bvh_root == kNoBvh) want += fs.objs[i].pair_count;
    if (fs.cand_pairs.size() != want || !fs.cand_ok) { printf("FAIL cand %zu %zu\n", fs.cand_pairs.size(), want); return 1; }
    pt_scene_free(sc);
    printf("OK %zu %u %u\n", fs.bvh_meshes.size(), fs.bvh_stack, deepest);
    return 0;
}
