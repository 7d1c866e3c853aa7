// tables_dump — host::flatten_scene's tables of a scene file - what pt_ctx_set_scene uploads - written out raw: the table generator of
// tests/boundary_rays.py.  GPU tests reach it through that module, so it is built WITHOUT the sanitizers there (make SAN=);
// tests/test_boundary_rays.py holds the sanitized build to the same output.
#include "check_common.h"
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>
#include "../csrc/pt_host.h"
using namespace pt;
// argv[1]: scene file (u32 n_objs, u32 n_tris, pt_camera, pt_object[n_objs], pt_triangle[n_tris]); argv[2]: output file.
// Writes host::flatten_scene's tables - what pt_ctx_set_scene uploads - as a count header followed by the raw records.
template <class T> static void put(FILE *f, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb");
    uint32_t n[2];
    if (!in || fread(n, 4, 2, in) != 2) { printf("FAIL read\n"); return 1; }
    pt_camera cam;
    std::vector<pt_object> objs(n[0]);
    std::vector<pt_triangle> tris(n[1] ? n[1] : 1);
    if (fread(&cam, sizeof cam, 1, in) != 1 || fread(objs.data(), sizeof(pt_object), n[0], in) != n[0] ||
        fread(tris.data(), sizeof(pt_triangle), n[1], in) != n[1]) { printf("FAIL read\n"); return 1; }
    fclose(in);
    host::FlatScene fs;
    std::string err;
    if (!host::flatten_scene(cam, objs.data(), n[0], tris.data(), n[1], fs, err)) { printf("FAIL flatten %s\n", err.c_str()); return 1; }
    FILE *out = fopen(argv[2], "wb");
    const uint32_t h[16] = {(uint32_t)fs.objs.size(), (uint32_t)fs.tri_pairs.size(), (uint32_t)fs.bvh_nodes.size(),
                            (uint32_t)fs.bvh_nodes4.size(), (uint32_t)fs.flat_pairs.size(), (uint32_t)fs.cand_pairs.size(),
                            (uint32_t)fs.bvh_meshes.size(), fs.n_flat_exact, fs.n_other_pairs, (uint32_t)fs.tri_rank.size(),
                            (uint32_t)fs.rank_id.size(), (uint32_t)fs.cand_ok, fs.bvh_stack, 0, 0, 0};
    fwrite(h, 4, 16, out);
    put(out, fs.objs); put(out, fs.tri_pairs); put(out, fs.bvh_nodes); put(out, fs.bvh_nodes4); put(out, fs.flat_pairs);
    put(out, fs.cand_pairs); put(out, fs.bvh_meshes); put(out, fs.tri_rank); put(out, fs.rank_id);
    fclose(out);
    printf("OK %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ObjRec), sizeof(TriPairRec), sizeof(BvhNode), sizeof(BvhNode4),
           sizeof(FlatPairRec), sizeof(CandPairRec), sizeof(BvhMeshRec));
    return 0;
}
