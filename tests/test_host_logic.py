"""Host-side pieces of the device layout that can be checked without a GPU: the round-robin deal of pixels to ray
streams (pt_device.h: stream_pixel / stream_pixel_count / global_pixel) and the bookkeeping word."""
import os
import subprocess
import textwrap

import ptlib

SRC = textwrap.dedent(r"""
    #include <cstdio>
    #include <cstdint>
    #include <vector>
    #include "pt_device.h"
    using namespace pt;
    struct P { uint32_t idx_begin, chunk_pixels, chunk_first, chunk_step, k_begin; };
    int main() {
        // 1. every pixel of a call belongs to exactly one (stream, slot); the accumulator slot k_resolve reads back is
        //    the one k_pass / k_shade wrote
        const uint32_t cases[][2] = {{1, 1}, {7, 3}, {786432, 16050}, {98304, 16384}, {3072, 1536}, {1000, 999}, {5, 64}};
        for (auto &c : cases) {
            const uint32_t npix = c[0], K = c[1];
            const uint32_t m = (npix + K - 1) / K;
            std::vector<int> seen(npix, 0);
            uint64_t total = 0;
            for (uint32_t b = 0; b < K; ++b) {
                const uint32_t mb = stream_pixel_count(npix, K, b);
                if (mb > m) { printf("FAIL count %u %u %u\n", npix, K, b); return 1; }
                total += mb;
                for (uint32_t j = 0; j < mb; ++j) {
                    const uint32_t p = stream_pixel(K, b, j);
                    if (p >= npix || seen[p]++) { printf("FAIL deal %u %u\n", npix, K); return 1; }
                    if (p % K != b || p / K != j) { printf("FAIL resolve %u %u\n", npix, K); return 1; }  // k_resolve's inverse
                }
            }
            if (total != npix) { printf("FAIL total %u %u\n", npix, K); return 1; }
        }
        // 2. interleaved partition: ranks' global pixels are disjoint and cover the band
        {
            const uint32_t W = 37, H = 11, step = 3;
            std::vector<int> seen(W * H, 0);
            for (uint32_t r = 0; r < step; ++r) {
                P f{0, W, r, step};
                uint32_t owned = 0;
                for (uint32_t ck = r; ck * W < W * H; ck += step) owned += W;
                for (uint32_t k = 0; k < owned; ++k) {
                    const uint32_t g = global_pixel(f, k);
                    if (g >= W * H || seen[g]++) { printf("FAIL chunks\n"); return 1; }
                }
            }
            for (int v : seen) if (v != 1) { printf("FAIL cover\n"); return 1; }
        }
        // 3. the bookkeeping word round-trips at its limits
        const uint32_t w = pack_word(1023, 32767, 11, 7);
        if (word_pix(w) != 1023 || word_sample(w) != 32767 || word_depth(w) != 11 || word_branch(w) != 7) { printf("FAIL word\n"); return 1; }
        printf("OK\n");
        return 0;
    }
""")


def test_stream_deal_and_partition(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text(SRC)
    exe = str(tmp_path / "t")
    inc = os.path.join(ptlib.PKG, "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", inc, "-I", os.path.join(ptlib.ROOT, "include"), str(src),
                           "-o", exe])
    assert subprocess.check_output([exe]).decode().strip() == "OK"


def test_rust_shim_mirrors_the_header():
    """ffi/hip.rs cannot be compiled here (no rustc): hold its #[repr(C)] structs to include/ptrace.h field by field
    (names and order; emission is the header's spelling of the reference's `emmission`)."""
    import re

    root = ptlib.ROOT
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ptrace.h")).read(), flags=re.S)
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(root, "ffi", "hip.rs")).read())
    for c_name, r_name in (("pt_camera", "PtCamera"), ("pt_triangle", "PtTriangle"), ("pt_object", "PtObject"),
                           ("pt_config", "PtConfig"), ("pt_stats", "PtStats")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), header, flags=re.S).group(1)
        c_fields = re.findall(r"\b(?:float|double|uint32_t|uint64_t)\s+(\w+)", body)
        rbody = re.search(r"pub struct %s \{(.*?)\n\}" % r_name, rust, flags=re.S).group(1)
        r_fields = re.findall(r"pub (\w+):", rbody)
        assert c_fields == r_fields, (c_name, c_fields, r_fields)
    for name in ("PT_OK", "PT_CANCELLED"):
        c_val = int(re.search(r"#define %s \(?(-?\d+)\)?" % name, header).group(1))
        r_val = int(re.search(r"pub const %s: i32 = (-?\d+);" % name, rust).group(1))
        assert c_val == r_val
    assert len(re.findall(r"pub fn pt_render\(", rust)) == 1 and "pub fn flatten(" in rust
    # every function the shim binds is declared in the header with the same number of parameters, in the same order by
    # kind (pointer / integer / float), and the preview path uses the resident form
    ext = re.search(r'extern "C" \{(.*?)\n\}', rust, flags=re.S).group(1)
    bound = re.findall(r"pub fn (\w+)\((.*?)\)\s*(?:->\s*([\w\s\*]+))?;", ext, flags=re.S)
    assert {"pt_ctx_create", "pt_ctx_destroy", "pt_ctx_set_scene", "pt_ctx_render", "pt_ctx_snapshot", "pt_device_malloc",
            "pt_device_free", "pt_device_download", "pt_render"} <= {b[0] for b in bound}

    def kind_rust(t):
        t = t.strip()
        return "p" if t.startswith("*") or t.startswith("Option<") else ("f" if t in ("f32", "f64") else "i")

    def kind_c(t):
        t = t.strip()
        return "p" if "*" in t or "[" in t or t.startswith("pt_progress_fn") else ("f" if t.split()[0] in ("float", "double") else "i")

    for fname, params, _ in bound:
        m = re.search(r"\b%s\((.*?)\);" % fname, header, flags=re.S)
        assert m, fname + " is not declared in include/ptrace.h"
        c_params = [q for q in m.group(1).split(",") if q.strip() and q.strip() != "void"]
        r_params = [q.split(":", 1)[1] for q in params.split(",") if ":" in q]
        assert [kind_c(q) for q in c_params] == [kind_rust(q) for q in r_params], (fname, c_params, r_params)
    body = rust[rust.index("pub fn render_pixels_hip"):]
    for call in ("pt_ctx_create", "pt_ctx_set_scene", "pt_ctx_render", "pt_device_download", "pt_ctx_destroy"):
        assert call + "(" in body, call
    assert "pt_ctx_snapshot(" in rust[rust.index('extern "C" fn on_progress'):rust.index("pub fn render_pixels_hip")]

FLATTEN_SRC = r"""
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>
#include "ptrace.h"
#include "pt_host.h"
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
    printf("OK %zu %u %u\n", fs.bvh_meshes.size(), fs.bvh_stack, deepest);
    return 0;
}
"""


def test_flatten_tables_of_the_walk_queue(tmp_path):
    """flatten_scene's tables for k_pass_cand<.., BVH> on mesh.json and cornell.json: tri_rank inverts rank_id, the BVH mesh
    list holds the meshes with a BVH in visiting order, every triangle of such a mesh sits in exactly one leaf of at most
    kBvhLeafPairs records inside the mesh's record range, the advertised stack depth covers the tree, and the candidate
    records are exactly those of the meshes without a BVH."""
    src = tmp_path / "f.cpp"
    src.write_text(FLATTEN_SRC)
    exe = str(tmp_path / "f")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ptlib.PKG, "csrc"), "-I", os.path.join(ptlib.ROOT, "include"),
                           str(src), "-o", exe, "-L", ptlib.PKG, "-lptrace_hip", "-Wl,-rpath," + ptlib.PKG])
    out = subprocess.check_output([exe, ptlib.scene_path("mesh"), ptlib.ROOT]).decode().split()
    assert out[0] == "OK" and out[1] == "1" and int(out[2]) > int(out[3]) >= 5  # one BVH mesh; stack deeper than the tree
    out = subprocess.check_output([exe, ptlib.scene_path("cornell"), ptlib.ROOT]).decode().split()
    assert out[:2] == ["OK", "0"]


def test_bvh_reference_limit():
    """The BVH walkers pack a node index or a leaf code (first pair record << 1 | records - 1: leaves of one or two records) into 26 bits of a queue entry
    (csrc/pt_device.h: WalkQueue, LeafLds); flatten_scene refuses a scene beyond that instead of letting references wrap."""
    L = ptlib.product()
    assert L.pt_bvh_refs_fit(141, 300) == 1                      # mesh.json
    assert L.pt_bvh_refs_fit((1 << 26) - 1, 1000) == 1
    assert L.pt_bvh_refs_fit(1 << 26, 1000) == 0                 # node indices need 27 bits
    assert L.pt_bvh_refs_fit(1000, (1 << 25) - 1) == 1
    assert L.pt_bvh_refs_fit(1000, 1 << 25) == 0                 # leaf codes need 27 bits


def test_build_flags_are_reported():
    L = ptlib.product()
    flags = L.pt_build_flags().decode()
    # "<set of the general unit> | flat: <set of k_pass_cand without walks>" (Makefile: MLLVM, MLLVM_FLAT)
    general, sep, flat = flags.partition("| flat:")
    assert sep and all(tok.startswith("-") or tok == "" for part in (general, flat) for tok in part.split(" ")), flags


SIGN_SRC = r"""
#include <cstdio>
#include <string>
#include <vector>
#include "ptrace.h"
#include "pt_host.h"
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
"""


def test_flat_filter_sign_rule_needs_well_shaped_triangles(tmp_path):
    """FlatPairRec.sign_exact (filter_flat drops rays that do not move towards the plane: the sign of Triangle::intersect's
    distance is then known exactly) is only set when the two edge products whose difference is the plane normal do not
    nearly cancel; a sliver keeps the conservative distance test.  cornell.json's walls all qualify."""
    src = tmp_path / "s.cpp"
    src.write_text(SIGN_SRC)
    exe = str(tmp_path / "s")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ptlib.PKG, "csrc"), "-I", os.path.join(ptlib.ROOT, "include"),
                           str(src), "-o", exe, "-L", ptlib.PKG, "-lptrace_hip", "-Wl,-rpath," + ptlib.PKG])
    assert subprocess.check_output([exe, "0"]).decode().split() == ["OK", "axis", "2", "sign_exact", "1"]
    assert subprocess.check_output([exe, "1"]).decode().split() == ["OK", "axis", "2", "sign_exact", "0"]


DOOR_SRC = r"""
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#include "ptrace.h"
#include "pt_host.h"
using namespace pt;
// a sphere and a two-triangle mesh; each colour and emission component of each object in turn set to a value the door must
// refuse (the message names the object and the field) or must let through
int main() {
    pt_camera cam = {{0, 0, 5}, {0, 0, -1}, 0.035f, 0.036f, 1.5f};
    std::vector<pt_triangle> tris = {{{0, 0, 1}, {1, 0, 1}, {0, 1, 1}}, {{1, 0, 1}, {1, 1, 1}, {0, 1, 1}}};
    pt_object objs[2] = {};
    objs[0].kind = PT_SPHERE, objs[0].radius = 1.0f, objs[0].position[2] = -3.0f;
    objs[1].kind = PT_MESH, objs[1].tri_count = 2, objs[1].bs_radius = 100.0f;
    for (pt_object &o : objs) o.color[0] = 0.75f, o.color[1] = 0.5f, o.color[2] = 0.25f, o.emission[1] = 12.0f;
    host::FlatScene fs;
    std::string err;
    if (!host::flatten_scene(cam, objs, 2, tris.data(), 2, fs, err)) { printf("FAIL clean scene: %s\n", err.c_str()); return 1; }
    const float bad[] = {-1.0f, -1e-45f, NAN, INFINITY, -INFINITY}, fine[] = {-0.0f, 0.0f, 1e-45f, 4294967296.0f, 3e38f};
    int refusals = 0;
    for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 6; ++k) {
            float *f = k < 3 ? &objs[i].color[k] : &objs[i].emission[k - 3];
            const float keep = *f;
            const std::string want = "object " + std::to_string(i) + ": a component of " + (k < 3 ? "color" : "emission") +
                                     " is negative or not finite";
            for (float v : bad) {
                *f = v;
                err.clear();
                if (host::flatten_scene(cam, objs, 2, tris.data(), 2, fs, err) || err != want) {
                    printf("FAIL object %d field %d value %g: `%s`\n", i, k, v, err.c_str());
                    return 1;
                }
                if (host::bad_material(objs[i]) == nullptr) { printf("FAIL bad_material %d %d %g\n", i, k, v); return 1; }
                ++refusals;
            }
            for (float v : fine) {
                *f = v;
                if (!host::flatten_scene(cam, objs, 2, tris.data(), 2, fs, err)) { printf("FAIL refused %g: %s\n", v, err.c_str()); return 1; }
            }
            *f = keep;
        }
    printf("OK %d\n", refusals);
    return 0;
}
"""


def test_the_door_refuses_negative_and_non_finite_materials(tmp_path):
    """flatten_scene - what pt_ctx_set_scene, and through it pt_render and pt_render_multi, build a scene with - refuses a colour
    or emission component that is negative, NaN or infinite, naming the object and the field, and lets -0.0f, denormals and
    large finite values through: to_fixed (csrc/pt_device.h) is defined for finite values >= 0 only.  pt_ctx_set_object's
    refusals (check_object_edit) are in host/object_check.cpp."""
    import re
    src = tmp_path / "door.cpp"
    src.write_text(DOOR_SRC)
    exe = str(tmp_path / "door")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ptlib.PKG, "csrc"), "-I", os.path.join(ptlib.ROOT, "include"),
                           str(src), "-o", exe, "-L", ptlib.PKG, "-lptrace_hip", "-Wl,-rpath," + ptlib.PKG])
    assert subprocess.check_output([exe]).decode().split() == ["OK", "60"]
    h = open(os.path.join(ptlib.ROOT, "include", "ptrace.h")).read()
    assert "a component of color or emission that is negative or not finite" in re.sub(r"\s*\n \* ", " ", h)
    assert "SATURATES at 4294967040" in h and "WRAPS at 2^32 radiance units" in h


PLAN_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include "ptrace.h"
#include "pt_host.h"
using namespace pt;
// argv: npix spp want default(0/1) stack_form stack_park cand_scan has_bvh streams per_stream wave_stack n_cus budget groups_per_cu
// prints OK spp_pass m K cap bytes0 bytes1 retries.  groups_per_cu by hand: plan_pass itself, once (RETRY: it asks for a smaller pass);
// groups_per_cu 0: the library's, through host::plan_frame, which follows plan_pass's retries (no taper)
int main(int argc, char **argv) {
    if (argc != 15) return 2;
    host::PassPlanIn in;
    in.npix = strtoull(argv[1], 0, 10);
    in.spp = (uint32_t)strtoul(argv[2], 0, 10);
    in.want = strtoull(argv[3], 0, 10);
    in.want_is_default = argv[4][0] == '1';
    in.stack_form = argv[5][0] == '1';
    in.stack_park = argv[6][0] == '1';
    in.cand_scan = argv[7][0] == '1';
    in.has_bvh = argv[8][0] == '1';
    in.streams = strtoull(argv[9], 0, 10);
    in.per_stream = (uint32_t)strtoul(argv[10], 0, 10);
    in.wave_stack = (uint32_t)strtoul(argv[11], 0, 10);
    in.n_cus = (uint32_t)strtoul(argv[12], 0, 10);
    in.stack_budget = (size_t)strtoull(argv[13], 0, 10);
    in.groups_per_cu = (uint32_t)strtoul(argv[14], 0, 10);
    host::FramePlan f;
    int rc;
    if (in.groups_per_cu) {
        uint64_t next = in.want;
        rc = host::plan_pass(in, f.pass, &next);
    } else {
        host::FramePlanIn fin;
        fin.pass = in;
        fin.rays_per_pass = in.want_is_default ? 0u : in.want;
        host::FrameRequest req;
        req.want = in.want;
        req.stack_budget = in.stack_budget;
        rc = host::plan_frame(fin, req, f);
    }
    if (rc == host::kPlanTooLarge) { printf("TOOLARGE\n"); return 0; }
    if (rc == host::kPlanRetry) { printf("RETRY\n"); return 0; }
    printf("OK %u %u %u %u %zu %zu %d\n", f.pass.spp_pass, f.pass.m, f.pass.K, f.pass.cap, f.pass.bytes0, f.pass.bytes1, f.retries);
    return 0;
}
"""


def test_pass_plan(tmp_path):
    """host::plan_pass - how a wavefront frame is cut into passes and streams; host::plan_frame follows its retries - on the CPU:
    the bench frame (six passes of 683 samples, stacks of 1024 slots per wave, nothing in the second container), mesh.json (parking areas), a frame of few
    samples (at most 64 pixels per stream), the memory budget (passes halved until the stacks fit), small stacks on request,
    tiny passes (smaller stacks), the level-by-level forms (slices of 4 slots per primary ray, two containers), and a pass
    that 32-bit slot indices cannot hold."""
    src = tmp_path / "p.cpp"
    src.write_text(PLAN_SRC)
    exe = str(tmp_path / "p")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ptlib.PKG, "csrc"), "-I", os.path.join(ptlib.ROOT, "include"),
                           str(src), "-o", exe, "-L", ptlib.PKG, "-lptrace_hip", "-Wl,-rpath," + ptlib.PKG])

    def plan(npix, spp, want, default=1, stack=1, park=0, cand=1, bvh=0, streams=0, per_stream=0, wave_stack=0, n_cus=256, budget=0, groups=None,
             follow=False):
        # workgroups a CU holds, by hand: five for k_pass_cand without walks (its waves per SIMD when these figures were pinned).
        # follow: through host::plan_frame, which derives them and follows plan_pass's retries
        groups = 0 if follow else groups or (4 if bvh or not stack else 5)
        out = subprocess.check_output([exe] + [str(v) for v in (npix, spp, want, default, stack, park, cand, bvh, streams, per_stream,
                                                                wave_stack, n_cus, budget, groups)]).decode().split()
        if out[0] != "OK":
            return out[0]
        spp_pass, m, K, cap, b0, b1, retries = map(int, out[1:])
        assert K * m >= npix > (K - 1) * m and 1 <= m <= 1024 and 1 <= spp_pass <= spp and cap % 4 == 0
        if stack:
            w = cap // 4
            most = min(m * spp_pass, -(-(-(-m * spp_pass // 64)) // 4) * 64)  # primaries of the wave with the most chunks of 64
            assert w & (w - 1) == 0 and 128 <= w <= 1024 and (4 * most + 3 <= w or w == (wave_stack or 1024))
            assert b0 == K * cap * 40 and b1 == (K * 4 * 128 * 48 if park else 0)
        else:
            assert cap >= 4 * m * spp_pass + 16 and cap % 256 == 0 and b0 == b1 == K * cap * 40
        return spp_pass, m, K, cap, retries

    npix = 1024 * 768
    spp_pass, m, K, cap, _ = plan(npix, 4096, 512 << 20)
    assert spp_pass == 683 and cap == 4096 and -(-4096 // spp_pass) == 6 and 4096 - 5 * spp_pass > 600  # six equal passes
    assert (m, K) == (22, 35747)  # streams of about 16 Ki primaries (24 pixels), nudged to the fewest rounds of 1280 resident workgroups x pixels
    assert plan(npix, 4096, 512 << 20, groups=4)[1:3] == (24, 32768)  # (rounds of 1024: 32.0)
    spp_pass, m, K, cap, _ = plan(npix, 1024, 512 << 20, park=1, bvh=1)  # mesh.json: two passes of 512, streams of 22 Ki primaries for scenes with walks, no nudge
    assert spp_pass == 512 and m == -(-npix // -(-npix * 512 // 22528)) and cap == 4096
    spp_pass, m, K, cap, _ = plan(npix, 128, 512 << 20)  # few samples: one pass, short streams of at most 64 (+ nudge) pixels
    assert spp_pass == 128 and m <= 72 and K >= 10922
    spp_pass, m, K, cap, retries = plan(128 * 96, 64, 512 << 20, budget=8 << 20, follow=True)  # the budget test of the GPU suite
    assert spp_pass == 1 and retries == 6 and cap == 512
    spp_pass, m, K, cap, _ = plan(npix, 4096, 512 << 20, wave_stack=512)
    assert cap == 2048
    spp_pass, m, K, cap, _ = plan(48 * 32, 8, 512 << 20)  # a tiny frame: 2048 streams of one pixel, 8 + 8 <= 128 slots
    assert (spp_pass, m, cap) == (8, 1, 512)
    spp_pass, m, K, cap, _ = plan(npix, 4096, 96 << 20, stack=0)  # level by level: 128 samples per pass, 4 slots per primary
    assert spp_pass == 128 and cap >= 4 * m * 128
    assert plan(1 << 20, 32767, 1 << 31, default=0, stack=0) == "TOOLARGE"
    spp_pass, m, K, cap, retries = plan(1 << 20, 32767, 1 << 31, default=1, stack=0, follow=True)  # the same as a default: halved until it fits
    assert retries >= 1 and K * cap <= 0x7fffffff


PASS_SRC = r"""
#include <cstdio>
#include <cstdint>
#include "pt_host.h"
using namespace pt;
int main() {
    const uint64_t npix = 1024u * 768u, probe = 1u << 20;
    // nothing measured yet: the probe (1 Mi primary rays = one sample per pixel of this frame)
    if (host::next_pass_samples(0.0, 100.0, npix, probe, 0, 4096, 683) != 1) { printf("FAIL probe\n"); return 1; }
    // a tiny frame's probe is never less than one sample
    if (host::next_pass_samples(0.0, 100.0, 4096u * 4096u, probe, 0, 100, 32) != 1) { printf("FAIL probe floor\n"); return 1; }
    // a measured rate is followed, but a pass grows at most sixteen-fold (short passes measure overheads), plus the fifth by which a
    // pass may be stretched: 19 after 1, 292 after 16
    const double rate = 5.5e6;  // primary samples per ms: cornell.json on an MI355X
    if (host::next_pass_samples(rate, 100.0, npix, probe, 1, 4095, 683) != 19) { printf("FAIL growth\n"); return 1; }
    if (host::next_pass_samples(rate, 100.0, npix, probe, 16, 4079, 683) != 292) { printf("FAIL growth 2 %u\n", host::next_pass_samples(rate, 100.0, npix, probe, 16, 4079, 683)); return 1; }
    // steady state: 699 samples would fit 100 ms, the plan allows 683: the bench frame is six equal passes of 683
    if (host::next_pass_samples(rate, 100.0, npix, probe, 683, 4096, 683) != 683) { printf("FAIL steady\n"); return 1; }
    // equal passes over what is left, each at most a fifth longer than the target rather than one pass more:
    // mesh.json's rate fits 448 samples into 100 ms; 1024 left -> two passes of 512 (114 ms), not three of 342
    if (host::next_pass_samples(3.52e6, 100.0, npix, probe, 512, 1024, 683) != 512) { printf("FAIL stretch\n"); return 1; }
    if (host::next_pass_samples(3.52e6, 100.0, npix, probe, 512, 1100, 683) != 367) { printf("FAIL equal %u\n", host::next_pass_samples(3.52e6, 100.0, npix, probe, 512, 1100, 683)); return 1; }
    // a scene fifty times dearer: passes of a tenth of a second are a handful of samples; never zero, never beyond what is left
    if (host::next_pass_samples(rate / 50.0, 100.0, npix, probe, 8, 10000, 683) != 15) { printf("FAIL dear %u\n", host::next_pass_samples(rate / 50.0, 100.0, npix, probe, 8, 10000, 683)); return 1; }
    if (host::next_pass_samples(1.0, 100.0, npix, probe, 1, 3, 683) != 1) { printf("FAIL floor\n"); return 1; }
    if (host::next_pass_samples(rate, 100.0, npix, probe, 683, 5, 683) != 5) { printf("FAIL left\n"); return 1; }
    printf("OK\n");
    return 0;
}
"""


def test_pass_length_follows_the_measured_rate(tmp_path):
    """host::next_pass_samples (render_wavefront / render_mega): the probe, the sixteen-fold growth limit, the plan's cap, equal
    passes stretched by at most a fifth, floors - the arithmetic behind "a cancel comes back within a tenth of a second"."""
    src = tmp_path / "p.cpp"
    src.write_text(PASS_SRC)
    exe = str(tmp_path / "p")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ptlib.PKG, "csrc"), "-I", os.path.join(ptlib.ROOT, "include"),
                           str(src), "-o", exe, "-L", ptlib.PKG, "-lptrace_hip", "-Wl,-rpath," + ptlib.PKG])
    assert subprocess.check_output([exe]).decode().strip() == "OK"


def _host_tool(tmp_path, name, source):
    """a small g++ program over csrc/pt_host.h, linked against the library"""
    src = tmp_path / (name + ".cpp")
    src.write_text(source)
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ptlib.PKG, "csrc"), "-I", os.path.join(ptlib.ROOT, "include"),
                           str(src), "-o", exe, "-L", ptlib.PKG, "-lptrace_hip", "-Wl,-rpath," + ptlib.PKG])
    return lambda *args: subprocess.check_output([exe] + [str(a) for a in args]).decode()


def ckpt_check_tool(tmp_path):
    """host/ckpt_check.cpp built by `make ckpt-check` (AddressSanitizer and UBSan; its own run must pass): ckpt_check ARGS' output"""
    r = subprocess.run(["make", "-C", ptlib.PKG, "ckpt-check", "B=%s" % tmp_path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ckpt_check: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    exe = str(tmp_path / "ckpt_check")
    return lambda *args: subprocess.check_output([exe] + [str(a) for a in args]).decode()


def _checkpoint(L, key, fp, total, part_px, counts, n_a, sums, a, version=None, seal=True):
    """a checkpoint file from the layout include/ptrace.h documents; key: (width, height, idx_begin, idx_end, chunk_pixels,
    chunk_first, chunk_step, seed); n_a / a: None for version 1"""
    import struct
    b = b"PTACCUM1" + struct.pack("<I", version or (1 if n_a is None else 2)) + struct.pack("<7IQ", *key) + struct.pack("<Q", fp)
    b += struct.pack("<3I", total, part_px, len(counts)) + struct.pack("<%dI" % len(counts), *counts)
    if n_a is not None:
        b += struct.pack("<%dI" % len(n_a), *n_a)
    b += sums + (a if a is not None else b"")
    return b + struct.pack("<Q", L.pt_siphash(1, 3, 0, 0, b, len(b))) if seal else b


def test_checkpoint_codec(tmp_path):
    """host::ckpt_encode_head / ckpt_seal / ckpt_decode against files built here from the documented layout: a plain and a
    noise-tracked checkpoint (a chunked band; a frame of two parts) decode to their fields and encode to the same bytes again;
    the header alone is asked for first, the rest only when the size fits; every damaged file is refused with the loader's
    reason, in the loader's order."""
    import numpy as np
    L = ptlib.product()
    tool = ckpt_check_tool(tmp_path)

    def run(data, *n):
        p = tmp_path / "c.ptacc"
        p.write_bytes(data)
        return tool("accum", p, *n).strip()

    planes = lambda total, salt: (np.arange(3 * total, dtype="<u8") * np.uint64(0x9e3779b97f4a7c15) + np.uint64(salt)).tobytes()
    # version 1: a whole 8x4 frame, one part
    key1 = (8, 4, 0, 32, 0, 0, 0, 0xfedcba9876543210)
    v1 = _checkpoint(L, key1, 0x1122334455667788, 32, 32, [12], None, planes(32, 1), None)
    assert len(v1) == 68 + 4 + 24 * 32 + 8
    assert run(v1) == "OK key 8 4 0 32 0 0 0 %d fp %d total 32 part_px 32 tracked 0 sums_at 72 a_at %d cnt 12 na SAME" % (
        key1[7], 0x1122334455667788, 72 + 768)
    # version 2: chunks 1, 3, 5 of four pixels of the band [4, 28) of that frame: 12 pixels
    key2 = (8, 4, 4, 28, 4, 1, 2, 7)
    v2 = _checkpoint(L, key2, 5, 12, 12, [12], [8], planes(12, 2), planes(12, 3))
    assert run(v2) == "OK key 8 4 4 28 4 1 2 7 fp 5 total 12 part_px 12 tracked 1 sums_at 76 a_at %d cnt 12 na 8 SAME" % (76 + 288)
    # version 2, a frame of two parts (more than 1.5 Mi pixels: parts of 2^20) at unequal counts
    total = 1600 * 1000
    big = _checkpoint(L, (1600, 1000, 0, total, 0, 0, 0, 1), 9, total, 1 << 20, [4, 2], [2, 2], planes(total, 4), planes(total, 5))
    assert run(big) == "OK key 1600 1000 0 %d 0 0 0 1 fp 9 total %d part_px 1048576 tracked 1 sums_at 84 a_at %d cnt 4 2 na 2 2 SAME" % (
        total, total, 84 + 24 * total)
    del big
    # the loader's two reads: the header, then the whole file - and nothing behind the header when the size does not fit it
    assert run(v2, 0) == "MORE 68" and run(v2, 68) == "MORE %d" % len(v2) and run(v2, 67) == "MORE 68"
    assert run(v2[:-10], 68) == "BAD truncated" and run(v2 + b"\0" * 4, 68) == "BAD trailing bytes"
    # every truncation and every flip of the lowest and highest bit of every byte is refused, each for a reason of the loader's
    for good in (v1, v2):
        got = {}
        for line in run(good, "sweep").splitlines():
            kind, why, n = line.split("|")
            got.setdefault(kind, {})[why] = int(n)
        assert sum(got["cut"].values()) == len(good) and set(got["cut"]) == {"too short", "truncated"}
        assert sum(got["flip"].values()) == 2 * len(good) and "NOT REFUSED" not in got["flip"]
        assert got["flip"]["bad trailing hash"] >= 2 * (len(good) - 68)  # whatever lies behind the header is the hash's business
        assert set(got["flip"]) <= {"bad trailing hash", "wrong magic", "unknown format version", "the frame key is not a valid frame",
                                    "sizes that do not fit each other", "truncated", "trailing bytes"}

    def resealed(data, at, fmt, value):
        import struct
        b = data[:at] + struct.pack(fmt, value) + data[at + struct.calcsize(fmt):-8]
        return b + struct.pack("<Q", L.pt_siphash(1, 3, 0, 0, b, len(b)))

    flipped = bytearray(v1)
    flipped[200] ^= 0x10
    for data, why in ((v1[:-10], "truncated"), (bytes(flipped), "bad trailing hash"), (b"PTACCUM2" + v1[8:], "wrong magic"),
                      (v1[:40], "too short"), (b"", "too short"), (v1[:75], "too short"),
                      (resealed(v1, 8, "<I", 3), "unknown format version"), (resealed(v2, 8, "<I", 0), "unknown format version"),
                      (v1 + b"\0", "trailing bytes"), (v2 + v2[-8:], "trailing bytes"),
                      (resealed(v1, 68, "<I", (1 << 24) + 1), "a sample count above 2^24"),
                      (resealed(v2, 72, "<I", 13), "half A holds more samples than the part"),
                      (resealed(v1, 12, "<I", 0), "the frame key is not a valid frame"),           # width 0
                      (resealed(v1, 28, "<I", 5), "the frame key is not a valid frame"),           # chunk_pixels without chunk_step
                      (resealed(v2, 36, "<I", 3), "sizes that do not fit each other"),             # another chunk_step: 8 pixels
                      (resealed(v1, 60, "<I", 16), "sizes that do not fit each other"),            # part_px
                      (resealed(v1, 64, "<I", 2), "sizes that do not fit each other")):            # number of parts
        assert run(data) == "BAD " + why, why
    assert run(resealed(v1, 68, "<I", 1 << 24)).startswith("OK ") and run(resealed(v2, 72, "<I", 12)).startswith("OK ")
    # the order of the checks: a wrong magic in a truncated file of an unknown version is a wrong magic, and so on down the list
    bad_all = resealed(b"PTACCUM2" + v2[8:], 8, "<I", 9)[:-20]
    assert run(bad_all) == "BAD wrong magic" and run(b"PTACCUM1" + bad_all[8:]) == "BAD unknown format version"
    assert run(resealed(v2, 72, "<I", 13)[:-20]) == "BAD truncated"
    bad_hash_and_count = bytearray(resealed(v1, 68, "<I", 1 << 25))
    bad_hash_and_count[-1] ^= 1
    assert run(bytes(bad_hash_and_count)) == "BAD bad trailing hash"


SCHED_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ptrace.h"
#include "pt_host.h"
using namespace pt;
// argv: spp megakernel total n_parts cnt.. [na..]: the jobs of one pt_ctx_accumulate call that is not cancelled, in order, with the
// half each goes to, the counts following as keep_job moves them (pt_api.hip); then the counts at the end
int main(int argc, char **argv) {
    const uint32_t spp = (uint32_t)atoi(argv[1]);
    const bool mega = atoi(argv[2]) != 0;
    host::FrameCounts f;
    f.total = (uint32_t)atoi(argv[3]);
    f.part_px = host::part_pixels(f.total, true);
    const int n_parts = atoi(argv[4]);
    if ((uint32_t)n_parts != host::part_count(f.total, f.part_px)) return 2;
    for (int i = 0; i < n_parts; ++i) f.cnt.push_back((uint32_t)atoi(argv[5 + i]));
    for (int i = 5 + n_parts; i < argc; ++i) f.na.push_back((uint32_t)atoi(argv[i]));
    for (const host::Job &j : host::accum_jobs(f, spp, mega)) {
        const uint32_t end = j.s_end ? j.s_end : spp;
        if (j.s_first >= end) continue;  // run_frame_call: nothing left to trace here
        const bool to_a = f.tracked() && host::deal_to_a(f.cnt[j.part_lo], f.na[j.part_lo]);
        printf("job %u %u %u %u %d %u %u %.9g %.9g %.9g\n", j.k0, j.n, j.s_first, end, (int)to_a, j.part_lo, j.part_hi, j.base, j.scale,
               j.boundary);
        for (uint32_t i = j.part_lo; i < j.part_hi; ++i) {
            if (to_a) f.na[i] += end - j.s_first;
            f.cnt[i] = end;
        }
    }
    printf("cnt");
    for (uint32_t v : f.cnt) printf(" %u", v);
    printf(" na");
    for (uint32_t v : f.na) printf(" %u", v);
    printf("\n");
    return 0;
}
"""


def test_accumulate_schedule_is_the_deal(tmp_path):
    """host::accum_jobs and host::deal_to_a - what pt_ctx_accumulate renders and which half keep_job gives it to - against
    deal(), the header's rule as tests/test_gpu_noise.py restates it: the issue's sequence 0 -> 8 -> 24 -> 64, a part already at
    the target, an untracked frame, parts of 2^20 pixels, and the megakernel's whole-call job only when every part is even."""
    import numpy as np
    from test_gpu_noise import deal
    tool = _host_tool(tmp_path, "sched", SCHED_SRC)
    f32 = np.float32

    def call(spp, mega, total, cnt, na=None):
        lines = tool(spp, int(mega), total, len(cnt), *(list(cnt) + list(na or []))).strip().split("\n")
        jobs = [ln.split()[1:] for ln in lines[:-1]]
        end = lines[-1].split()
        return ([tuple(int(v) for v in j[:7]) + tuple(float(f32(v)) for v in j[7:]) for j in jobs],
                [int(v) for v in end[1:end.index("na")]], [int(v) for v in end[end.index("na") + 1:]])

    def expect(spp, total, pieces, cnt, na):
        """pieces: (k0, n, part_lo, part_hi) in order -> the jobs deal() gives them, with their progress fractions"""
        jobs = []
        for k0, n, lo, hi in pieces:
            runs, _ = deal(cnt[lo], na[lo], spp) if na else ([(cnt[lo], spp, False)] if cnt[lo] < spp else [], 0)
            base, scale = f32(k0) / f32(total), f32(n) / f32(total)
            f1 = f32(runs[0][1]) / f32(spp) if runs else None
            for r, (s0, s1, to_a) in enumerate(runs):
                first = r == 0 and bool(na)  # the first of a tracked part's two jobs: its fractions are scaled to the call's
                jobs.append((k0, n, s0, s1, int(to_a), lo, hi, float(base), float(scale * f1 if first else scale),
                             float(base + scale * f1) if r == 1 else -1.0))
        return jobs

    # the issue's sequence on one part of 96x64, wavefront and megakernel alike
    total = 96 * 64
    for mega in (False, True):
        cnt, na, runs = [0], [0], []
        for t in (8, 24, 64):
            jobs, cnt2, na2 = call(t, mega, total, cnt, na)
            assert jobs == expect(t, total, [(0, total, 0, 1)], cnt, na)
            assert (cnt2, na2) == ([t], [deal(cnt[0], na[0], t)[1]])
            runs += [(j[2], j[3], bool(j[4])) for j in jobs]
            cnt, na = cnt2, na2
        assert runs == [(0, 4, True), (4, 8, False), (8, 16, True), (16, 24, False), (24, 44, True), (44, 64, False)] and na == [32]
    # a part already at the target: nothing to render, the counts stay
    assert call(64, False, total, [64], [32]) == ([], [64], [32])
    assert call(64, False, total, [64]) == ([], [64], [])
    # a step of one sample is one job (m = spp); a plain frame is one job per part whatever the step
    assert call(9, False, total, [8], [4]) == ([(0, total, 8, 9, 1, 0, 1, 0.0, 1.0, -1.0)], [9], [5])
    assert call(64, False, total, [5]) == ([(0, total, 5, 64, 0, 0, 1, 0.0, 1.0, -1.0)], [64], [])
    # two parts (2^20 pixels and the rest): the wavefront goes part by part; the megakernel takes the call at once while every
    # part holds the same counts, and goes part by part when they do not - each part dealt by its own counts
    total, p0 = 1600 * 1000, 1 << 20
    parts = [(0, p0, 0, 1), (p0, total - p0, 1, 2)]
    for mega, cnt, na, pieces in ((False, [8, 8], [4, 4], parts), (True, [8, 8], [4, 4], [(0, total, 0, 2)]),
                                  (True, [16, 8], [8, 4], parts), (True, [8, 8], [8, 4], parts), (True, [24, 0], [12, 0], parts),
                                  (True, [8, 8], None, [(0, total, 0, 2)]), (True, [8, 2], None, parts), (False, [8, 8], None, parts)):
        jobs, cnt2, na2 = call(24, mega, total, cnt, na)
        assert jobs == expect(24, total, pieces, cnt, na), (mega, cnt, na)
        assert cnt2 == [24, 24] and na2 == ([deal(c, a, 24)[1] for c, a in zip(cnt, na)] if na else [])


NOISE_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ptrace.h"
#include "pt_host.h"
using namespace pt;
// argv: pixels stats.mean_error target.mean_error target.quantile target.quantile_error [bin count]..: the quantile bin, the bits of
// its upper edge, whether the target is met
int main(int argc, char **argv) {
    if (argv[1][0] == 'w') {  // w nA nB ..: the bits of a part's weight, pair by pair
        for (int i = 2; i + 1 < argc; i += 2) {
            const float w = host::noise_part_weight((uint32_t)atoi(argv[i]), (uint32_t)atoi(argv[i + 1]));
            uint32_t bits;
            memcpy(&bits, &w, 4);
            printf("%u\n", bits);
        }
        return 0;
    }
    pt_noise_stats s{};
    s.pixels = strtoull(argv[1], 0, 10);
    s.mean_error = atof(argv[2]);
    pt_noise_target t{};
    t.mean_error = (float)atof(argv[3]);
    t.quantile = (float)atof(argv[4]);
    t.quantile_error = (float)atof(argv[5]);
    for (int i = 6; i + 1 < argc; i += 2) s.histogram[atoi(argv[i])] = (uint32_t)atoi(argv[i + 1]);
    const uint32_t b = host::noise_quantile_bin(s, t.quantile);
    const float up = host::noise_bin_upper(b);
    uint32_t bits;
    memcpy(&bits, &up, 4);
    printf("%u %u %d\n", b, bits, (int)host::noise_target_met(s, t));
    return 0;
}
"""


def test_noise_target_decision(tmp_path):
    """host::noise_quantile_bin / noise_bin_upper / noise_target_met / noise_part_weight - pt_ctx_accumulate_until's decision
    and pt_ctx_accum_noise's weights - on hand-made histograms, against tests/noise_ref.py's restatement of the header."""
    import numpy as np
    import noise_ref
    tool = _host_tool(tmp_path, "noise", NOISE_SRC)
    bits = lambda v: int(np.array([v], dtype=np.float32).view(np.uint32)[0])

    def ask(pixels, hist, mean=0.0, t_mean=0.0, q=0.0, q_err=0.0):
        flat = [v for kv in sorted(hist.items()) for v in kv]
        b, up, met = (int(v) for v in tool(pixels, repr(mean), repr(t_mean), repr(q), repr(q_err), *flat).split())
        if q:
            full = np.zeros(64, dtype=np.uint32)
            for k, v in hist.items():
                full[k] = v
            assert b == noise_ref.quantile_bin(full, pixels, q) and up == bits(noise_ref.bin_upper(b))
        return b, bool(met)

    edge = noise_ref.bin_upper  # bin b holds errors below edge(b)
    # `need` exactly on a bin's cumulative count, and one above it
    assert ask(100, {3: 10, 7: 40, 20: 50}, q=0.5, q_err=edge(7)) == (7, True)
    assert ask(100, {3: 10, 7: 39, 20: 51}, q=0.5, q_err=edge(7)) == (20, False)
    assert ask(100, {3: 10, 7: 39, 20: 51}, q=0.5, q_err=edge(20)) == (20, True)
    assert ask(100, {3: 10, 7: 40, 20: 50}, q=0.5, q_err=float(np.nextafter(np.float32(edge(7)), np.float32(0)))) == (7, False)
    # the ceiling is of the DOUBLE product of the binary32 quantile: 0.4f * 100 is a little more than 40
    assert ask(100, {3: 10, 7: 30, 20: 60}, q=0.4, q_err=1.0) == (20, True)
    # quantile * pixels below 1 (and at 0 pixels) asks for one pixel
    assert ask(100, {5: 1, 9: 99}, q=0.001, q_err=edge(5)) == (5, True)
    assert ask(3, {9: 3}, q=1e-30, q_err=edge(9)) == (9, True)
    assert ask(0, {}, q=0.5, q_err=3e38) == (64, False)  # no bin reaches it: past the last bin, whose edge is +inf
    # the last bin's upper edge is +inf: no finite quantile_error is met there
    assert ask(10, {63: 10}, q=0.9, q_err=3e38) == (63, False) and noise_ref.bin_upper(63) == float("inf")
    assert ask(10, {62: 10}, q=0.9, q_err=3e38) == (62, True)
    # mean only, quantile only, both
    h = {3: 10, 7: 40, 20: 50}
    assert ask(100, h, mean=0.01, t_mean=0.02)[1] and not ask(100, h, mean=0.03, t_mean=0.02)[1]
    assert ask(100, h, mean=float(np.float32(0.02)), t_mean=0.02)[1]  # (<=, against the double of the binary32 target)
    assert not ask(100, h, mean=float("nan"), t_mean=0.02)[1]
    assert ask(100, h, mean=9.0, q=0.5, q_err=edge(7))[1]  # the mean is not in use
    assert ask(100, h, mean=0.01, t_mean=0.02, q=0.5, q_err=edge(7))[1]
    assert not ask(100, h, mean=0.03, t_mean=0.02, q=0.5, q_err=edge(7))[1]
    assert not ask(100, h, mean=0.01, t_mean=0.02, q=0.5, q_err=edge(6))[1]
    # a part's weight, every operation in binary32 (rounding a double result once gives other bits for (1, 5), (1, 6), ...)
    pairs = [(a, b) for a in range(1, 33) for b in range(1, 33)] + [(20, 44), (3, 16777213), (1, 16777215), (8388608, 8388608)]
    got = [int(v) for v in tool("w", *[n for p in pairs for n in p]).split()]
    assert got == [bits(noise_ref.weight(a, b)) for a, b in pairs]


SCHEDULE_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ptrace.h"
#include "pt_host.h"
using namespace pt;
static uint64_t num(const char *s) { return strtoull(s, 0, 0); }
// argv[1] names the function, the rest are its arguments in order; prints its results (a refusal: REFUSED and the message)
int main(int argc, char **argv) {
    const char *f = argv[1];
    auto arg = [&](int i) { return num(argv[1 + i]); };
    if (!strcmp(f, "rounds")) {  // entries spp_left rays_per_pass item_mult n_cus s_here..: the plan, then each launch
        const host::RoundPlan p = host::plan_rounds(arg(1), (uint32_t)arg(2), arg(3), (uint32_t)arg(4), (uint32_t)arg(5));
        printf("%u %u", p.round_spp, p.n_split);
        for (int i = 6; 1 + i < argc; ++i) {
            const host::RoundLaunch l = host::round_launch(arg(1), p.n_split, (uint32_t)arg(i), (uint32_t)arg(5));
            printf(" %u %u %u", l.split, l.lane_spp, l.grid);
        }
        printf("\n");
    } else if (!strcmp(f, "launch")) {  // entries n_split s_here n_cus
        const host::RoundLaunch l = host::round_launch(arg(1), (uint32_t)arg(2), (uint32_t)arg(3), (uint32_t)arg(4));
        printf("%u %u %u\n", l.split, l.lane_spp, l.grid);
    } else if (!strcmp(f, "split")) {  // c T
        printf("%u\n", host::tracked_split((uint32_t)arg(1), (uint32_t)arg(2)));
    } else if (!strcmp(f, "adaptive") || !strcmp(f, "until")) {  // [held] min_spp cap: the counts up to the cap
        const bool ad = f[0] == 'a';
        const uint32_t cap = (uint32_t)arg(ad ? 2 : 3);
        uint32_t t = ad ? host::adaptive_first_level((uint32_t)arg(1), cap) : host::until_first_target((uint32_t)arg(1), (uint32_t)arg(2), cap);
        for (int i = 0; i < 40; ++i, t = host::next_target(t, cap)) {
            printf("%u ", t);
            if (t >= cap) break;
        }
        printf("\n");
    } else if (!strcmp(f, "params")) {  // tile_error tile
        pt_adaptive_params p{(float)atof(argv[2]), (uint32_t)arg(2), 0u};
        uint32_t shift = 99;
        if (host::check_adaptive_params(p, &shift)) printf("REFUSED %s\n", pt_last_error());
        else printf("%u\n", shift);
    } else if (!strcmp(f, "cfg")) {  // width idx_begin idx_end chunk_step flags
        pt_config c{};
        c.width = (uint32_t)arg(1), c.idx_begin = (uint32_t)arg(2), c.idx_end = (uint32_t)arg(3), c.chunk_step = (uint32_t)arg(4), c.flags = (uint32_t)arg(5);
        if (host::check_adaptive_cfg(c)) printf("REFUSED %s\n", pt_last_error());
        else printf("OK\n");
    } else if (!strcmp(f, "target")) {  // mean_error quantile quantile_error
        pt_noise_target t{(float)atof(argv[2]), (float)atof(argv[3]), (float)atof(argv[4]), 0u};
        if (host::check_noise_target(t)) printf("REFUSED %s\n", pt_last_error());
        else printf("OK\n");
    } else if (!strcmp(f, "tiles")) {  // width rows tile_shift [err_sum (spp err)..]: err "-" = no error yet
        host::TileGeometry g{};
        if (host::tile_geometry((uint32_t)arg(1), (uint32_t)arg(2), (uint32_t)arg(3), g)) { printf("REFUSED %s\n", pt_last_error()); return 0; }
        printf("%u %u %u", g.tile_shift, g.tiles_x, g.tiles);
        if (argc > 5) {
            std::vector<uint32_t> spp;
            std::vector<unsigned long long> err;
            for (int i = 5; 1 + i + 1 < argc; i += 2) {
                spp.push_back((uint32_t)arg(i));
                err.push_back(argv[1 + i + 1][0] == '-' ? kTileNoError : arg(i + 1));
            }
            if (spp.size() != g.tiles) return 2;
            const host::TileTotals t = host::tile_totals((uint32_t)arg(1), (uint32_t)arg(2), g, spp.data(), err.data(), arg(4));
            printf(" %llu %llu %.17g", (unsigned long long)t.samples, (unsigned long long)t.est_pixels, t.mean_error);
        }
        printf("\n");
    } else {
        return 2;
    }
    return 0;
}
"""


def test_rounds_schedules_and_tiles(tmp_path):
    """The host arithmetic of the megakernel's and the tile pass's rounds (host::plan_rounds / round_launch), the sample schedules
    of the calls that render to a noise target (tracked_split, next_target and the two first counts), and pt_ctx_render_adaptive's
    refusals, tile geometry and totals - on values worked by hand from their definitions."""
    tool = _host_tool(tmp_path, "schedule", SCHEDULE_SRC)
    ask = lambda *a: tool(*a).strip()
    nums = lambda *a: [int(v) for v in ask(*a).split()]
    # the bench frame on 256 CUs: 256 Mi / 786432 = 341 samples per round; 8 x 256 x 2048 items are wanted, 786432 x 8 reaches
    # them; a round of 341 is 8 lanes of ceil(341 / 8) = 43 samples per pixel, on the 8 x 256 workgroups the grid is capped at
    assert nums("rounds", 1024 * 768, 4096, 0, 8, 256, 341) == [341, 8, 8, 43, 2048]
    # three open tiles of 8 x 8 with 8 samples left: split eightfold (4 x 256 x 2048 items is out of reach: n_split <= round_spp),
    # 192 x 8 = 1536 items in 6 workgroups of 256
    assert nums("rounds", 192, 8, 0, 4, 256, 8) == [8, 8, 8, 1, 6]
    assert nums("rounds", 1024, 100, 4096, 8, 256)[0] == 4                # an explicit budget: 4096 / 1024
    assert nums("rounds", 5000, 100, 4096, 8, 256)[:2] == [1, 1]          # more entries than the budget: one sample, no split
    assert nums("rounds", 1024, 3, 0, 8, 256)[:2] == [3, 3]               # clipped to what is left; n_split to round_spp
    assert nums("rounds", 1 << 25, 64, 0, 8, 256) == [8, 1]               # enough items without a split
    assert nums("launch", 192, 8, 3, 256) == [3, 1, 3]                    # fewer samples than lanes: one lane per sample
    assert nums("launch", 192, 8, 5, 256) == [5, 1, 4]
    assert nums("launch", 1024, 4, 7, 256) == [4, 2, 16]
    assert nums("launch", 0, 1, 1, 256) == [1, 1, 1]                      # never an empty grid
    assert nums("launch", 1 << 31, 8, 8, 256) == [8, 1, 2048]             # (64-bit item counts)
    # m = min(T, c + 4 * ceil((T - c) / 8))
    for c, t, m in ((0, 16, 8), (16, 32, 24), (64, 100, 84), (0, 10, 8), (0, 3, 3), (0, 4, 4), (0, 5, 4), (7, 7, 7), (0, 0, 0),
                    (0, 1 << 24, 1 << 23), (0, 0xffffffff, 0x80000000), (0xfffffff0, 0xffffffff, 0xfffffff8)):
        assert nums("split", c, t) == [m], (c, t)
    # accum_jobs cuts a tracked part at exactly this value
    sched = _host_tool(tmp_path, "sched", SCHED_SRC)
    for c, na, t in ((0, 0, 16), (16, 8, 32), (64, 32, 100), (0, 0, 10), (0, 0, 3)):
        jobs = [ln.split() for ln in sched(t, 0, 96 * 64, 1, c, na).strip().split("\n")[:-1]]
        m = nums("split", c, t)[0]
        assert [(int(j[3]), int(j[4])) for j in jobs] == ([(c, m), (m, t)] if m < t else [(c, t)]), (c, t)
    # the levels of the adaptive call (min_spp, cap) and the targets of pt_ctx_accumulate_until (held, min_spp, cap)
    assert nums("adaptive", 0, 100) == [16, 32, 64, 100]
    assert nums("adaptive", 5, 100)[0] == 8 and nums("adaptive", 16, 10) == [10] and nums("adaptive", 17, 1000)[0] == 24
    assert nums("adaptive", 0xfffffffa, 1 << 24) == [1 << 24] and nums("adaptive", 0xfffffff8, 1 << 24) == [1 << 24]
    assert nums("adaptive", 0, 0xffffffff)[-3:] == [1 << 30, 1 << 31, 0xffffffff]  # (no wrap in the doubling)
    assert nums("until", 20, 0, 100) == [20, 40, 80, 100] and nums("until", 0, 24, 30) == [24, 30]
    assert nums("until", 0, 0, 100) == [16, 32, 64, 100] and nums("until", 0, 5, 100)[0] == 5  # (not rounded to 8s)
    assert nums("until", 20, 64, 100) == [64, 100] and nums("until", 0, 64, 10) == [10] and nums("until", 100, 0, 100) == [100]
    # tiles: 20 x 12 in tiles of 8 is 3 x 2, the right column 4 wide, the bottom row 4 high
    assert nums("tiles", 20, 12, 3) == [3, 3, 6]
    assert [nums("params", "0.5", t) for t in (4, 8, 16, 32, 0)] == [[2], [3], [4], [5], [3]]
    for t in (1, 2, 7, 12, 64, 0xffffffff):
        assert "tile must be 4, 8, 16 or 32" in ask("params", "0.5", t)
    for v in ("-0.5", "inf", "nan"):
        assert "tile_error must be finite and not negative" in ask("params", v, 7)  # before the tile
    assert nums("params", "0", 8) == [3]
    # 2^32 entries or more, from the arithmetic alone (nothing is allocated): a band one pixel wide has tile^2 entries for every
    # `tile` pixels; a wide frame of 2^31 pixels stays far below
    assert nums("tiles", 65536, 32767, 5) == [5, 2048, 2048 * 1024]
    assert nums("tiles", 1, (1 << 30) - 4, 2)[2] == (1 << 28) - 1 and "2^32 pixels or more" in ask("tiles", 1, (1 << 30) - 3, 2)
    assert nums("tiles", 1, (1 << 27) - 32, 5)[2] == (1 << 22) - 1 and "2^32 pixels or more" in ask("tiles", 1, (1 << 27) - 31, 5)
    assert "2^32 pixels or more" in ask("tiles", 1, 0x7fffffff, 5)
    # the band and the chunks, in this order
    assert ask("cfg", 96, 0, 0, 0, 0) == "OK" and ask("cfg", 96, 96 * 20, 96 * 46, 1, 1) == "OK"
    assert "whole image rows" in ask("cfg", 96, 10, 900, 2, 0) and "whole image rows" in ask("cfg", 96, 0, 961, 0, 0)
    assert "chunk_step" in ask("cfg", 96, 0, 0, 2, 0) and "PT_FLAG_PIPELINES" in ask("cfg", 96, 0, 0, 0, 2 << 8)
    # the noise target, in the header's order
    assert ask("target", "0.1", "0", "0") == "OK" and ask("target", "0", "0.5", "0.2") == "OK"
    for bad in (("-1", "2", "0"), ("0", "nan", "0"), ("0", "0", "inf")):
        assert "finite and not negative" in ask("target", *bad)
    assert "neither" in ask("target", "0", "0", "0.5") and "(0, 1)" in ask("target", "0.1", "1", "0")
    # totals: the counts weigh 64, 64, 32 / 32, 32, 16 pixels; one tile without an error leaves the mean at +inf
    spp = [16, 32, 64, 16, 32, 64]
    some = [v for pair in zip(spp, [5, 0, "-", 7, 9, 11]) for v in pair]
    out = ask("tiles", 20, 12, 3, 1000, *some).split()
    assert int(out[3]) == 16 * 64 + 32 * 64 + 64 * 32 + 16 * 32 + 32 * 32 + 64 * 16 and int(out[4]) == 240 - 32 and out[5] == "inf"
    every = [v for pair in zip(spp, [5, 0, 1 << 40, 7, 9, 11]) for v in pair]
    out = ask("tiles", 20, 12, 3, (1 << 40) + 32, *every).split()
    assert int(out[4]) == 240 and float(out[5]) == ((1 << 40) + 32) * 2.0 ** -28 / 240
    out = ask("tiles", 20, 12, 3, 0, *[v for s in spp for v in (0, "-")]).split()
    assert (int(out[3]), int(out[4]), out[5]) == (0, 0, "inf")
