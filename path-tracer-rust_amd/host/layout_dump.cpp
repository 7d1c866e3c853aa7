// layout_dump — lds_layout's (csrc/pt_layout.h) answer for a scene file at each query, with the DevScene counts filled from
// host::flatten_scene as pt_ctx_set_scene fills them, and the lines the library writes under PT_LDS_PAD: the table generator of
// tests/lds_layouts.py.  GPU tests reach it through that module, so it is built WITHOUT the sanitizers there (make SAN=);
// tests/test_lds_layouts.py holds the sanitized build to the same output.
#include "check_common.h"
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>
#include "../csrc/pt_host.h"
#include "../csrc/pt_layout.h"
using namespace pt;
// argv[1]: scene file (u32 n_objs, u32 n_tris, pt_camera, pt_object[n_objs], pt_triangle[n_tris]); argv[2..]: queries "m,switches".
// The DevScene counts as pt_ctx_set_scene and cand_scan_for set them; then lds_layout and its three stderr lines per query.
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
    bool glass = false;
    for (uint32_t i = 0; i < n[0]; ++i) glass = glass || objs[i].reflect_type == PT_REFRACT;
    for (int a = 2; a < argc; ++a) {
        unsigned m = 0, sw = 0;
        if (sscanf(argv[a], "%u,%u", &m, &sw) != 2) { printf("FAIL query\n"); return 1; }
        DevScene S{};
        const uint32_t nodes = (uint32_t)fs.bvh_nodes.size();
        S.n_objs = n[0];
        S.n_tris = n[1];
        S.n_cand_pairs = (uint32_t)fs.cand_pairs.size();
        S.n_bvh_nodes4 = (uint32_t)fs.bvh_nodes4.size();
        S.n_bvh_nodes = nodes;
        S.bvh_stack = fs.bvh_stack;
        const bool ref16 = nodes < 0x8000u && ((uint64_t)fs.bvh_pair_span << kBvhLeafBits) < 0x8000u;
        S.bvh_in_lds = ref16 ? 2u : 0u;
        S.nodes_in_lds_ok = (sw & 8u) ? 0u : 1u;
        S.glass_defer_ok = ((sw & 4u) && glass) ? 1u : 0u;
        S.cand_scan = (!(sw & 1u) && fs.cand_ok && !(nodes != 0u && (sw & 2u))) ? 1u : 0u;
        const LdsLayout L = lds_layout(S, m, 0u);
        printf("Q %u %u %u %u %u %u %u %u %u %u %d %d %d %u %u %zu %d %zu %d %u %u %u %zu\n", S.n_objs, S.n_tris, S.n_cand_pairs,
               S.n_bvh_nodes, S.n_bvh_nodes4, S.bvh_stack, S.cand_scan, L.pass, L.m, L.bvh_in_lds, (int)L.staged, (int)L.defer,
               (int)L.nodes_lds, L.surf_staged, L.surf_head, L.pass_lds, (int)L.isect_staged, L.isect_lds, (int)L.mega_cand,
               L.mega_depth, L.mega_spare_off, L.mega_surf_off, L.mega_lds);
        for (int w = 0; w < 3; ++w) printf("L%d %s\n", w, lds_layout_line(L, w).c_str());
    }
    return 0;
}
