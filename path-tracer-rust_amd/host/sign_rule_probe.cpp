// sign_rule_probe — FlatPairRec.sign_exact (csrc/pt_host.cpp: flatten_scene) on a quad of well-shaped triangles (argv[1] = 0) and on
// one with a sliver (1).  Prints the record's axis and sign_exact for
// tests/test_host_logic.py (test_flat_filter_sign_rule_needs_well_shaped_triangles).
#include "check_common.h"
#include <cstdio>
#include <string>
#include <vector>
#include "../csrc/pt_host.h"
using namespace pt;
// argv[1] = 0: two quads in the plane z = 1 made of well-shaped triangles; 1: the same plane, but one triangle whose two edge
// products nearly cancel (a sliver: e1 = (1, 1), e2 = (1, 1.0005)): the plane normal's component is 0.0005 of the products
int main(int argc, char **argv) {
    const bool sliver = argv[1][0] == '1';
    pt_camera cam = {{0, 0, 5}, {0, 0, -1}, 0.035f, 0.036f, 1.5f};
    std::vector<pt_triangle> tris;
    tris.push_back({{0, 0, 1}, {1, 0, 1}, {0, 1, 1}});
    tris.push_back({{1, 0, 1}, {1, 1, 1}, {0, 1, 1}});
    if (sliver) tris[1] = {{0, 0, 1}, {1, 1, 1}, {1, 1.0005f, 1}};
    pt_object o{};
    o.kind = PT_MESH;
    o.tri_count = 2;
    o.bs_radius = 100.0f;
    host::FlatScene fs;
    std::string err;
    if (!host::flatten_scene(cam, &o, 1, tris.data(), 2, fs, err)) { printf("FAIL %s\n", err.c_str()); return 1; }
    if (fs.flat_pairs.size() != 1) { printf("FAIL flat_pairs %zu\n", fs.flat_pairs.size()); return 1; }
    printf("OK axis %u sign_exact %u\n", fs.flat_pairs[0].axis, fs.flat_pairs[0].sign_exact);
    return 0;
}
