// pt_host.cpp — once-per-frame host arithmetic feeding the kernels.  Built with -ffp-contract=off: the
// values produced here must be the f32 values the reference computes (per frame for the camera, per ray
// for the triangle edges — see pt_device.h).
#include "pt_host.h"
#include "pt_denoise.h"
#include "pt_despike.h"
#include "pt_layout.h"
#include "pt_masked.h"
#include "pt_overlay.h"
#include "pt_present.h"
#include "pt_probe.h"
#include "pt_refit.h"
#include "pt_reproject.h"
#include "pt_solid.h"
#include "pt_tone.h"
#include "pt_upsample.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace pt {
namespace host {

static vec3 ld(const float *p) { return mk(p[0], p[1], p[2]); }
static void st(float *p, vec3 v) {
    p[0] = v.x;
    p[1] = v.y;
    p[2] = v.z;
}

void camera_basis(const pt_camera &cam, float lens_center[3], float su_out[3], float sv_out[3]) {
    const vec3 position = ld(cam.position), direction = ld(cam.direction);
    const float sensor_height = cam.sensor_width / cam.aspect_ratio;  // mod.rs:211-213
    const vec3 lens = position + direction * cam.focal_length;        // mod.rs:216-218
    const vec3 helper = f_abs(direction.y) < 0.9f ? mk(0.0f, 1.0f, 0.0f) : mk(0.0f, 0.0f, 1.0f);
    const vec3 su = normalize(cross(direction, helper));  // mod.rs:223-229
    const vec3 sv = cross(su, direction);                 // mod.rs:230
    st(lens_center, lens);
    st(su_out, su * cam.sensor_width);  // mod.rs:231
    st(sv_out, sv * sensor_height);
}

void mesh_bounding_sphere(const pt_triangle *tris, uint32_t n, float center[3], float *radius) {
    const float inf = std::numeric_limits<float>::infinity();
    vec3 lo = mk(inf, inf, inf), hi = mk(-inf, -inf, -inf);
    for (uint32_t i = 0; i < n; ++i) {
        const float *corners[3] = {tris[i].a, tris[i].b, tris[i].c};
        for (const float *v : corners) {
            lo.x = v[0] < lo.x ? v[0] : lo.x;
            lo.y = v[1] < lo.y ? v[1] : lo.y;
            lo.z = v[2] < lo.z ? v[2] : lo.z;
            hi.x = v[0] > hi.x ? v[0] : hi.x;
            hi.y = v[1] > hi.y ? v[1] : hi.y;
            hi.z = v[2] > hi.z ? v[2] : hi.z;
        }
    }
    // the reference's centre is min + max*0.5 (mod.rs:478-482), kept as is
    const vec3 c = mk(lo.x + hi.x * 0.5f, lo.y + hi.y * 0.5f, lo.z + hi.z * 0.5f);
    const float to_lo = length(lo - c), to_hi = length(hi - c);
    st(center, c);
    *radius = to_lo > to_hi ? to_lo : to_hi;  // max_by keeps the last of equal maxima
}

void mesh_bounding_box(const pt_triangle *tris, uint32_t n, pt_triangle out[12]) {
    const float inf = std::numeric_limits<float>::infinity();
    vec3 lo = mk(inf, inf, inf), hi = mk(-inf, -inf, -inf);
    for (uint32_t i = 0; i < n; ++i) {
        const float *corners[3] = {tris[i].a, tris[i].b, tris[i].c};
        for (const float *v : corners) {
            lo.x = v[0] < lo.x ? v[0] : lo.x;
            lo.y = v[1] < lo.y ? v[1] : lo.y;
            lo.z = v[2] < lo.z ? v[2] : lo.z;
            hi.x = v[0] > hi.x ? v[0] : hi.x;
            hi.y = v[1] > hi.y ? v[1] : hi.y;
            hi.z = v[2] > hi.z ? v[2] : hi.z;
        }
    }
    // bounding_box_to_triangles, mod.rs:501-536: vertex and index tables as written there
    const vec3 vtx[8] = {mk(lo.x, lo.y, lo.z), mk(hi.x, lo.y, lo.z), mk(hi.x, hi.y, lo.z), mk(lo.x, hi.y, lo.z),
                         mk(lo.x, lo.y, hi.z), mk(hi.x, lo.y, hi.z), mk(hi.x, hi.y, hi.z), mk(lo.x, hi.y, hi.z)};
    static const int idx[12][3] = {{0, 1, 2}, {0, 2, 3}, {4, 6, 5}, {4, 7, 6}, {0, 4, 5}, {0, 5, 1},
                                   {3, 2, 6}, {3, 6, 7}, {1, 5, 6}, {1, 6, 2}, {0, 3, 7}, {0, 7, 4}};
    for (int k = 0; k < 12; ++k) {
        st(out[k].a, vtx[idx[k][0]]);
        st(out[k].b, vtx[idx[k][1]]);
        st(out[k].c, vtx[idx[k][2]]);
    }
}

void box_pair_records(const pt_triangle box[12], const float position[3], TriPairRec out[6]) {
    const vec3 pos = ld(position);
    for (int k = 0; k < 12; ++k) {
        const vec3 a = ld(box[k].a) + pos, b = ld(box[k].b) + pos, c = ld(box[k].c) + pos;
        const vec3 e1 = b - a, e2 = c - a;
        TriPairRec &r = out[k / 2];
        const int hf = k & 1;
        r.ax[hf] = a.x, r.ay[hf] = a.y, r.az[hf] = a.z;
        r.e1x[hf] = e1.x, r.e1y[hf] = e1.y, r.e1z[hf] = e1.z;
        r.e2x[hf] = e2.x, r.e2y[hf] = e2.y, r.e2z[hf] = e2.z;
        r.id[hf] = (uint32_t)k;
    }
}

namespace {

struct BuildTri {
    vec3 lo, hi, mid;
    vec3 a, e1, e2;
    uint32_t id;  // flattened triangle index
};

struct BvhBuilder {
    FlatScene &out;
    std::vector<BuildTri> &t;  // lo/hi already padded per triangle
    bool use_sah = true;       // false: median split (balanced: depth <= log2(n) + 1)
    uint32_t depth_max = 0;

    static void grow(vec3 &lo, vec3 &hi, const vec3 &l, const vec3 &h) {
        lo = mk(std::fmin(lo.x, l.x), std::fmin(lo.y, l.y), std::fmin(lo.z, l.z));
        hi = mk(std::fmax(hi.x, h.x), std::fmax(hi.y, h.y), std::fmax(hi.z, h.z));
    }

    // returns the child reference of the subtree over t[b,e) and its padded box
    int32_t build(size_t b, size_t e, vec3 &lo, vec3 &hi, uint32_t depth) {
        const float inf = std::numeric_limits<float>::infinity();
        lo = mk(inf, inf, inf);
        hi = mk(-inf, -inf, -inf);
        depth_max = depth > depth_max ? depth : depth_max;
        // (splitting such a run further where the surface-area heuristic would - a node step priced at 1, 2 or 4 triangle
        // tests - loses on mesh.json: 15.8, 16.8, 17.5 against 17.8 G bounces/s; it is the node steps that cost)
        if (e - b <= 2u * kBvhLeafPairs) {  // leaf = up to kBvhLeafPairs consecutive TriPairRecs
            const size_t first = out.tri_pairs.size();
            for (size_t k0 = b; k0 < e; k0 += 2) {
                TriPairRec rec{};
                rec.id[0] = rec.id[1] = kNoTri;  // a filler half is all zeros: determinant 0, rejected (mod.rs:571)
                for (size_t k = k0; k < e && k < k0 + 2; ++k) {
                    const uint32_t hf = (uint32_t)(k - k0);
                    const BuildTri &q = t[k];
                    rec.ax[hf] = q.a.x, rec.ay[hf] = q.a.y, rec.az[hf] = q.a.z;
                    rec.e1x[hf] = q.e1.x, rec.e1y[hf] = q.e1.y, rec.e1z[hf] = q.e1.z;
                    rec.e2x[hf] = q.e2.x, rec.e2y[hf] = q.e2.y, rec.e2z[hf] = q.e2.z;
                    rec.id[hf] = q.id;
                    grow(lo, hi, q.lo, q.hi);
                }
                out.tri_pairs.push_back(rec);
            }
            const size_t count = out.tri_pairs.size() - first;
            return ~(int32_t)((first << kBvhLeafBits) | (count - 1));
        }
        // surface-area-heuristic split: for each axis sort by centroid and sweep; only even left counts are
        // considered so that leaves are full pairs wherever possible.  Ties are broken by triangle id: the tree
        // (and with it the traversal order) is a pure function of the scene.
        const size_t cnt = e - b;
        size_t half = 0;
        int best_axis = -1;
        float best_cost = inf;
        std::vector<float> right_area(cnt + 1);
        auto area = [](const vec3 &l, const vec3 &h) {
            const vec3 d = h - l;
            return 2.0f * (d.x * d.y + d.y * d.z + d.z * d.x);
        };
        for (int axis = 0; use_sah && axis < 3; ++axis) {
            auto key = [axis](const BuildTri &q) { return axis == 0 ? q.mid.x : (axis == 1 ? q.mid.y : q.mid.z); };
            std::sort(t.begin() + (long)b, t.begin() + (long)e, [&](const BuildTri &x, const BuildTri &y) {
                const float kx = key(x), ky = key(y);
                return kx < ky || (kx == ky && x.id < y.id);
            });
            vec3 l = mk(inf, inf, inf), h = mk(-inf, -inf, -inf);
            for (size_t k = cnt; k-- > 0;) {
                grow(l, h, t[b + k].lo, t[b + k].hi);
                right_area[k] = area(l, h);
            }
            l = mk(inf, inf, inf), h = mk(-inf, -inf, -inf);
            for (size_t k = 1; k < cnt; ++k) {
                grow(l, h, t[b + k - 1].lo, t[b + k - 1].hi);
                if (k & 1) continue;
                const float cost = area(l, h) * (float)k + right_area[k] * (float)(cnt - k);
                if (cost < best_cost) {
                    best_cost = cost;
                    best_axis = axis;
                    half = k;
                }
            }
        }
        if (best_axis < 0 && use_sah) {  // cnt == 3: one full pair + one half-filled leaf
            best_axis = 2;
            half = 2;
        }
        if (!use_sah) {  // median of the widest centroid axis, left count even
            vec3 clo = mk(inf, inf, inf), chi = mk(-inf, -inf, -inf);
            for (size_t k = b; k < e; ++k) grow(clo, chi, t[k].mid, t[k].mid);
            const vec3 ext = chi - clo;
            best_axis = (ext.x >= ext.y && ext.x >= ext.z) ? 0 : (ext.y >= ext.z ? 1 : 2);
            half = ((cnt / 2) + 1) & ~(size_t)1;
            if (half >= cnt) half = 2;
            const int axis = best_axis;
            auto key = [axis](const BuildTri &q) { return axis == 0 ? q.mid.x : (axis == 1 ? q.mid.y : q.mid.z); };
            std::sort(t.begin() + (long)b, t.begin() + (long)e, [&](const BuildTri &x, const BuildTri &y) {
                const float kx = key(x), ky = key(y);
                return kx < ky || (kx == ky && x.id < y.id);
            });
        } else if (best_axis != 2) {  // the array is currently sorted along z: restore the winning order
            const int axis = best_axis;
            auto key = [axis](const BuildTri &q) { return axis == 0 ? q.mid.x : q.mid.y; };
            std::sort(t.begin() + (long)b, t.begin() + (long)e, [&](const BuildTri &x, const BuildTri &y) {
                const float kx = key(x), ky = key(y);
                return kx < ky || (kx == ky && x.id < y.id);
            });
        }
        const size_t node_at = out.bvh_nodes.size();
        out.bvh_nodes.push_back(BvhNode{});
        vec3 l0, h0, l1, h1;
        const int32_t c0 = build(b, b + half, l0, h0, depth + 1);
        const int32_t c1 = build(b + half, e, l1, h1, depth + 1);
        BvhNode &n = out.bvh_nodes[node_at];
        n.lox[0] = l0.x, n.loy[0] = l0.y, n.loz[0] = l0.z, n.hix[0] = h0.x, n.hiy[0] = h0.y, n.hiz[0] = h0.z;
        n.lox[1] = l1.x, n.loy[1] = l1.y, n.loz[1] = l1.z, n.hix[1] = h1.x, n.hiy[1] = h1.y, n.hiz[1] = h1.z;
        n.c[0] = c0;
        n.c[1] = c1;
        grow(lo, hi, l0, h0);
        grow(lo, hi, l1, h1);
        return (int32_t)node_at;
    }
};

// The binary tree below `ref` four children wide (BvhNode4): a node's children are its two children, and while there is
// room the inner child with the largest box is replaced by ITS two children - boxes and leaf references are the binary
// tree's.  Returns the reference in the wide tree (a leaf reference stays what it is).
// src (FlatScene.wide_src) gets, per child slot, the binary (node, half) the box was taken from: 2 * node + half, kRefitNone for none.
int32_t widen(const std::vector<BvhNode> &bin, int32_t ref, std::vector<BvhNode4> &wide, std::vector<uint32_t> &src) {
    if (ref < 0) return ref;
    struct Kid {
        int32_t ref;
        uint32_t src;
        float lo[3], hi[3];
    };
    auto kid_of = [&](const BvhNode &n, int h) {
        Kid k;
        k.ref = n.c[h];
        k.src = 2u * (uint32_t)(&n - bin.data()) + (uint32_t)h;
        k.lo[0] = n.lox[h], k.lo[1] = n.loy[h], k.lo[2] = n.loz[h];
        k.hi[0] = n.hix[h], k.hi[1] = n.hiy[h], k.hi[2] = n.hiz[h];
        return k;
    };
    auto area = [](const Kid &k) {
        const float dx = k.hi[0] - k.lo[0], dy = k.hi[1] - k.lo[1], dz = k.hi[2] - k.lo[2];
        return dx * dy + dy * dz + dz * dx;
    };
    std::vector<Kid> kids = {kid_of(bin[(size_t)ref], 0), kid_of(bin[(size_t)ref], 1)};
    while (kids.size() < 4u) {
        int best = -1;
        for (int i = 0; i < (int)kids.size(); ++i)
            if (kids[(size_t)i].ref >= 0 && (best < 0 || area(kids[(size_t)i]) > area(kids[(size_t)best]))) best = i;
        if (best < 0) break;
        const BvhNode &n = bin[(size_t)kids[(size_t)best].ref];
        kids[(size_t)best] = kid_of(n, 0);  // (the first child takes the parent's place: the order stays a function of the scene)
        kids.insert(kids.begin() + best + 1, kid_of(n, 1));
    }
    const size_t at = wide.size();
    wide.push_back(BvhNode4{});
    src.resize(4u * wide.size(), kRefitNone);
    for (size_t j = 0; j < kids.size(); ++j) src[4u * at + j] = kids[j].src;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    int32_t refs[4];
    for (size_t j = 0; j < 4u; ++j) refs[j] = j < kids.size() ? widen(bin, kids[j].ref, wide, src) : 0;
    BvhNode4 &w = wide[at];
    for (size_t j = 0; j < 4u; ++j) {
        const bool has = j < kids.size();
        w.lox[j] = has ? kids[j].lo[0] : nan, w.loy[j] = has ? kids[j].lo[1] : nan, w.loz[j] = has ? kids[j].lo[2] : nan;
        w.hix[j] = has ? kids[j].hi[0] : nan, w.hiy[j] = has ? kids[j].hi[1] : nan, w.hiz[j] = has ? kids[j].hi[2] : nan;
        w.c[j] = has ? refs[j] : refs[0];
    }
    return (int32_t)at;
}

}  // namespace

// The per-wave walk queue (bvh_closest_queue) and the leaf list (bvh_closest_postponed) pack `owner lane | reference << 6`
// into 32 bits: a node index, or a leaf code first_record << kBvhLeafBits | count - 1, has 26 bits.
bool bvh_refs_fit(uint64_t n_nodes, uint64_t n_pair_records) {
    return n_nodes < (1ull << 26) && (n_pair_records << kBvhLeafBits) < (1ull << 26);
}

void scene_reach(const pt_camera &cam, const pt_object *objs, uint32_t n_objs, const pt_triangle *tris, uint32_t n_tris, Reach &out) {
    const float finf = std::numeric_limits<float>::infinity();
    vec3 slo = mk(finf, finf, finf), shi = mk(-finf, -finf, -finf);
    float lens[3], su[3], sv[3];
    camera_basis(cam, lens, su, sv);
    BvhBuilder::grow(slo, shi, ld(lens), ld(lens));
    for (uint32_t i = 0; i < n_objs; ++i) {
        const vec3 pos = ld(objs[i].position);
        if (objs[i].kind == PT_SPHERE) {
            const float r = f_abs(objs[i].radius);
            BvhBuilder::grow(slo, shi, pos - mk(r, r, r), pos + mk(r, r, r));
        } else if (objs[i].kind == PT_MESH && (uint64_t)objs[i].tri_offset + objs[i].tri_count <= n_tris) {
            for (uint32_t k = objs[i].tri_offset; k < objs[i].tri_offset + objs[i].tri_count; ++k) {
                BvhBuilder::grow(slo, shi, ld(tris[k].a) + pos, ld(tris[k].a) + pos);
                BvhBuilder::grow(slo, shi, ld(tris[k].b) + pos, ld(tris[k].b) + pos);
                BvhBuilder::grow(slo, shi, ld(tris[k].c) + pos, ld(tris[k].c) + pos);
            }
        }
    }
    st(out.lo, slo);
    st(out.hi, shi);
}

bool grow_reach(Reach &B, const float lens[3]) {
    bool grew = false;
    for (int a = 0; a < 3; ++a) {
        if (lens[a] < B.lo[a]) {
            B.lo[a] = lens[a] - (B.lo[a] - lens[a]);
            grew = true;
        }
        if (lens[a] > B.hi[a]) {
            B.hi[a] = lens[a] + (lens[a] - B.hi[a]);
            grew = true;
        }
    }
    return grew;
}

// ---- flatten_scene's per-object steps, which edit_object runs again for the one object that changed -------------------------
// everything of an object's record but its triangle ranges and its tree: the (bounding) sphere and rr_in, from the object and
// the box [slo, shi] that bounds every ray origin.  A sphere's record is complete afterwards.
static void object_head(const pt_object &o, vec3 slo, vec3 shi, ObjRec &r) {
    const vec3 position = ld(o.position);
    r.kind = o.kind;
    if (o.kind == PT_SPHERE) {
        r.cx = position.x;
        r.cy = position.y;
        r.cz = position.z;
        r.rr = o.radius * o.radius;  // radius.powi(2), mod.rs:416
        r.rr_in = -1.0f;
        r.tri_begin = 0;
        r.tri_count = 0;
        r.pair_begin = 0;
        r.pair_count = 0;
        r.bvh_root = kNoBvh;
        return;
    }
    const vec3 gate = ld(o.bs_center) + position;  // mod.rs:268
    r.cx = gate.x;
    r.cy = gate.y;
    r.cz = gate.z;
    r.rr = o.bs_radius * o.bs_radius;
    // rr_in: see intersect_scene_dev.  A point of the ray, ahead of the origin, within (1 - eta) r of the
    // centre with eta = 1e-3: the chord through it is >= 0.09 r long, so the exact discriminant is
    // >= 2e-3 r^2 and the far root lies >= 1e-3 r ahead of the origin.  With every origin within 4 r of the
    // centre (origins lie in the scene's bounding box) the f32 discriminant is off by <= 4 e (16+16+1) r^2
    // ~ 8e-6 r^2, its root by <= 9e-5 r, so the computed far root is >= 9e-4 r >= 1e-4 for r >= 0.2: the
    // gate passes.  The factor 0.998 and the absolute term cover the device's own o + d*t and distance.
    const float rad = f_abs(o.bs_radius);
    float far2 = 0.0f;  // squared distance from the centre to the farthest corner of the scene's box
    for (int k = 0; k < 8; ++k) {
        const vec3 corner = mk((k & 1) ? shi.x : slo.x, (k & 2) ? shi.y : slo.y, (k & 4) ? shi.z : slo.z);
        far2 = f_max(far2, dot(corner - gate, corner - gate));
    }
    const bool offer = std::isfinite(rad) && rad >= 0.2f && far2 <= 16.0f * rad * rad;
    r.rr_in = offer ? r.rr * 0.998f - 1e-4f * (1.0f + rad) : -1.0f;
    r.bvh_root = kNoBvh;
}

static void object_material(const pt_object &o, MatRec &m) {
    m.cr = o.color[0];
    m.cg = o.color[1];
    m.cb = o.color[2];
    m.er = o.emission[0];
    m.eg = o.emission[1];
    m.eb = o.emission[2];
    material_reflectance(o.color, m.max_refl, m.inv_max_refl);
    m.px = o.position[0];
    m.py = o.position[1];
    m.pz = o.position[2];
    m.reflect = o.reflect_type;
}

// a mesh's triangles in world space (pt_refit.h: world_triangle), in list order; their shading records
static void mesh_triangles(uint32_t i, const pt_object &o, const pt_triangle *tris, float scene_R, std::vector<TriShade> &tri_shade,
                           std::vector<BuildTri> &bt) {
    const vec3 position = ld(o.position);
    bt.clear();
    bt.reserve(o.tri_count);
    for (uint32_t k = o.tri_offset; k < o.tri_offset + o.tri_count; ++k) {
        const WorldTri w = world_triangle(tris[k], position, scene_R);
        TriShade &s = tri_shade[k];
        s.nx = w.nrm.x;
        s.ny = w.nrm.y;
        s.nz = w.nrm.z;
        s.owner = i;
        BuildTri q;
        q.a = w.a, q.e1 = w.e1, q.e2 = w.e2, q.id = k;
        q.lo = w.lo, q.hi = w.hi, q.mid = w.mid;
        bt.push_back(q);
    }
}

// a mesh without a BVH: its triangles in list order, two per record, into dst[0, (n + 1) / 2)
static void list_pairs(const std::vector<BuildTri> &bt, TriPairRec *dst) {
    for (size_t k = 0; k < bt.size(); k += 2) {
        TriPairRec rec{};
        rec.id[0] = rec.id[1] = kNoTri;
        for (size_t hf = 0; hf < 2 && k + hf < bt.size(); ++hf) {
            const BuildTri &q = bt[k + hf];
            rec.ax[hf] = q.a.x, rec.ay[hf] = q.a.y, rec.az[hf] = q.a.z;
            rec.e1x[hf] = q.e1.x, rec.e1y[hf] = q.e1.y, rec.e1z[hf] = q.e1.z;
            rec.e2x[hf] = q.e2.x, rec.e2y[hf] = q.e2.y, rec.e2z[hf] = q.e2.z;
            rec.id[hf] = q.id;
        }
        dst[k / 2] = rec;
    }
}

// The tables that hold a few records per object (never one per triangle of a mesh with a BVH): obj_pairs, sph_pairs, and the
// candidate scan's flat_pairs and cand_pairs - from out.objs and the pair records of the meshes WITHOUT a BVH.  flatten_scene
// runs it once; edit_object runs it again after it rewrote one object's records.
static void derive_small(const pt_object *objs, uint32_t n_objs, float scene_R, FlatScene &out) {
    const float finf = std::numeric_limits<float>::infinity();
    // pairs in visiting order (mod.rs:637: highest index first)
    out.obj_pairs.assign((n_objs + 1u) / 2u, ObjPairRec{});
    for (uint32_t v = 0; v < 2u * (uint32_t)out.obj_pairs.size(); ++v) {
        ObjPairRec &pr = out.obj_pairs[v / 2u];
        const uint32_t hf = v & 1u;
        if (v < n_objs) {
            const ObjRec &r = out.objs[n_objs - 1u - v];
            pr.cx[hf] = r.cx, pr.cy[hf] = r.cy, pr.cz[hf] = r.cz, pr.rr[hf] = r.rr;
            pr.kind[hf] = r.kind;
            pr.pair_begin[hf] = r.pair_begin;
            pr.pair_count[hf] = r.pair_count;
            pr.bvh_root[hf] = r.bvh_root;
            pr.obj[hf] = n_objs - 1u - v;
            // A gate pays when a whole wave of 64 unrelated rays misses the sphere, i.e. when a single ray hits it
            // with probability well under 1/64: roughly (radius / distance)^2 / 4 with distances of the order of the
            // scene.  Spheres above an eighth of the scene diagonal are not worth their arithmetic.
            // (a mesh with a BVH keeps its gate: there it saves a whole walk, and the deferred walks need its result)
            pr.admit[hf] = (r.kind == kKindMesh && r.bvh_root == kNoBvh && r.rr > (scene_R * 0.125f) * (scene_R * 0.125f)) ? 1u : 0u;
            // a mesh scanned pair by pair whose triangles all lie in one axis-aligned plane: which axis (bits 1-2)
            if (r.kind == kKindMesh && r.bvh_root == kNoBvh) {
                for (uint32_t ax = 0; ax < 3; ++ax) {
                    bool flat = r.pair_count != 0u;
                    for (uint32_t pp = r.pair_begin; flat && pp < r.pair_begin + r.pair_count; ++pp) {
                        const TriPairRec &tp = out.tri_pairs[pp];
                        const float *e1 = ax == 0 ? tp.e1x : (ax == 1 ? tp.e1y : tp.e1z);
                        const float *e2 = ax == 0 ? tp.e2x : (ax == 1 ? tp.e2y : tp.e2z);
                        flat = e1[0] == 0.0f && e1[1] == 0.0f && e2[0] == 0.0f && e2[1] == 0.0f;  // fillers are all zero
                    }
                    if (flat) {
                        pr.admit[hf] |= (ax + 1u) << 1;
                        break;
                    }
                }
            }
        } else {  // filler: a sphere whose discriminant is -inf for every finite ray
            pr.cx[hf] = pr.cy[hf] = pr.cz[hf] = 0.0f;
            pr.rr[hf] = -std::numeric_limits<float>::infinity();
            pr.kind[hf] = kKindSphere;
            pr.bvh_root[hf] = kNoBvh;
            pr.obj[hf] = 0;
            pr.admit[hf] = 0u;
        }
    }
    // ranks of the objects: the reference's visiting sequence - objects from the last to the first (mod.rs:637), a mesh's
    // triangles in list order (mod.rs:558): triangle k of object i has rank obj_rank[i] + k
    std::vector<uint32_t> obj_rank(n_objs, 0u);
    {
        uint32_t next = 0;
        for (uint32_t v = 0; v < n_objs; ++v) {
            const uint32_t i = n_objs - 1u - v;
            obj_rank[i] = next;
            next += objs[i].kind == PT_SPHERE ? 1u : objs[i].tri_count;
        }
    }
    out.sph_pairs.clear();
    out.flat_pairs.clear();
    out.cand_pairs.clear();
    std::vector<CandPairRec> filtered;  // records that have a filter (appended after the unfiltered ones below)
    // the exact-test record of pair record pp of object i
    auto cand_rec = [&](uint32_t i, uint32_t pp) {
        const TriPairRec &tp = out.tri_pairs[pp];
        CandPairRec c{};
        for (int hf = 0; hf < 2; ++hf) {
            c.ax[hf] = tp.ax[hf], c.ay[hf] = tp.ay[hf], c.az[hf] = tp.az[hf];
            c.e1x[hf] = tp.e1x[hf], c.e1y[hf] = tp.e1y[hf], c.e1z[hf] = tp.e1z[hf];
            c.e2x[hf] = tp.e2x[hf], c.e2y[hf] = tp.e2y[hf], c.e2z[hf] = tp.e2z[hf];
            c.id[hf] = tp.id[hf] == kNoTri ? kNoTri : obj_rank[i] + (tp.id[hf] - objs[i].tri_offset);
        }
        c.gx = out.objs[i].cx, c.gy = out.objs[i].cy, c.gz = out.objs[i].cz;
        c.grr = out.objs[i].rr;
        c.grr_in = out.objs[i].rr_in;
        return c;
    };
    {
        const float ninf = -std::numeric_limits<float>::infinity();
        uint32_t n_sph = 0;
        for (uint32_t v = 0; v < n_objs; ++v) {
            const uint32_t i = n_objs - 1u - v;
            if (objs[i].kind != PT_SPHERE) continue;
            if ((n_sph & 1u) == 0u) {
                SphPairRec f{};
                f.rr[0] = f.rr[1] = ninf;
                out.sph_pairs.push_back(f);
            }
            SphPairRec &sp = out.sph_pairs.back();
            const uint32_t hf = n_sph & 1u;
            sp.cx[hf] = out.objs[i].cx, sp.cy[hf] = out.objs[i].cy, sp.cz[hf] = out.objs[i].cz, sp.rr[hf] = out.objs[i].rr;
            sp.rank[hf] = obj_rank[i];
            ++n_sph;
        }
        // pair records of meshes without a BVH: flat ones (both triangles in one axis-aligned plane) get a filter,
        // grouped by axis so that two of them share a record; the rest are candidates for every ray
        std::vector<FlatPairRec> by_axis[3];
        uint32_t fill[3] = {0, 0, 0};
        for (uint32_t i = 0; i < n_objs; ++i) {
            const ObjRec &r = out.objs[i];
            if (r.kind != kKindMesh || r.bvh_root != kNoBvh) continue;
            for (uint32_t pp = r.pair_begin; pp < r.pair_begin + r.pair_count; ++pp) {
                const TriPairRec &tp = out.tri_pairs[pp];
                int axis = -1;
                for (int ax = 0; ax < 3 && axis < 0; ++ax) {
                    const float *e1 = ax == 0 ? tp.e1x : (ax == 1 ? tp.e1y : tp.e1z);
                    const float *e2 = ax == 0 ? tp.e2x : (ax == 1 ? tp.e2y : tp.e2z);
                    const float *aa = ax == 0 ? tp.ax : (ax == 1 ? tp.ay : tp.az);
                    const bool two = tp.id[1] != kNoTri;
                    if (e1[0] == 0.0f && e2[0] == 0.0f && (!two || (e1[1] == 0.0f && e2[1] == 0.0f && aa[1] == aa[0]))) axis = ax;
                }
                // |N| of the record's triangles (the smaller one), their longest edge, their bounds in the plane
                float n_min = std::numeric_limits<float>::infinity(), L = 0.0f;
                vec3 lo = mk(finf, finf, finf), hi = mk(-finf, -finf, -finf);
                for (int hf = 0; hf < 2; ++hf) {
                    if (tp.id[hf] == kNoTri) continue;
                    const vec3 a = mk(tp.ax[hf], tp.ay[hf], tp.az[hf]);
                    const vec3 e1 = mk(tp.e1x[hf], tp.e1y[hf], tp.e1z[hf]), e2 = mk(tp.e2x[hf], tp.e2y[hf], tp.e2z[hf]);
                    n_min = std::fmin(n_min, length(cross(e1, e2)));
                    L = std::fmax(L, std::fmax(length(e1), std::fmax(length(e2), length(e2 - e1))));
                    BvhBuilder::grow(lo, hi, a, a);
                    BvhBuilder::grow(lo, hi, a + e1, a + e1);
                    BvhBuilder::grow(lo, hi, a + e2, a + e2);
                }
                // The filter only judges rays with |d_a| >= kGrazing, for which |determinant| = |d_a| |N| >= |N| / 64
                // (and >= 1e-4, mod.rs:571): the forward-error bound of the BVH boxes above with that determinant in
                // place of 1e-4, plus the filter's own arithmetic (an approximate reciprocal and two fmas on
                // distances up to R / kGrazing).
                const float e = 5.9604645e-8f;
                const float det_min = std::fmax(1e-4f, n_min * kGrazing);
                const float pad = 3.0f * (16.0f * e * L * L * (scene_R + L) / det_min) + (32.0f / kGrazing) * e * (scene_R + L) + 1e-5f;
                const bool usable = axis >= 0 && std::isfinite(pad) && std::isfinite(n_min) && n_min > 0.0f;
                if (!usable) {
                    out.cand_pairs.push_back(cand_rec(i, pp));
                    continue;
                }
                const int a = axis, b = (axis + 1) % 3, c = (axis + 2) % 3;
                const float lov[3] = {lo.x, lo.y, lo.z}, hiv[3] = {hi.x, hi.y, hi.z};
                if ((fill[a] & 1u) == 0u) {
                    FlatPairRec f{};
                    f.pair[0] = f.pair[1] = kNoPair;
                    f.hb[0] = f.hb[1] = f.hc[0] = f.hc[1] = -1.0f;  // empty rectangle: |x - c| <= -1 never holds
                    f.tpad[0] = f.tpad[1] = 0.0f;
                    f.axis = (uint32_t)a;
                    f.sign_exact = 1u;  // (cleared by the first half that does not qualify; a filler half qualifies)
                    by_axis[a].push_back(f);
                }
                FlatPairRec &f = by_axis[a].back();
                const uint32_t hf = fill[a] & 1u;
                f.pc[hf] = lov[a];
                f.cb[hf] = 0.5f * (lov[b] + hiv[b]);
                f.hb[hf] = 0.5f * (hiv[b] - lov[b]) + pad + 4.0f * e * (f_abs(lov[b]) + f_abs(hiv[b]));
                f.cc[hf] = 0.5f * (lov[c] + hiv[c]);
                f.hc[hf] = 0.5f * (hiv[c] - lov[c]) + pad + 4.0f * e * (f_abs(lov[c]) + f_abs(hiv[c]));
                f.tpad[hf] = pad;
                // filter_flat's sign rule: the two products whose difference is the plane normal's component along the axis
                // must not nearly cancel, for both triangles of the record, in Triangle::intersect's `distance` numerator and
                // in its determinant alike (the same two products of edge components, mod.rs:563-564, 583-589)
                for (int h2 = 0; h2 < 2; ++h2) {
                    if (tp.id[h2] == kNoTri) continue;
                    const float e1v[3] = {tp.e1x[h2], tp.e1y[h2], tp.e1z[h2]}, e2v[3] = {tp.e2x[h2], tp.e2y[h2], tp.e2z[h2]};
                    const double pa = (double)e1v[b] * e2v[c], pb = (double)e1v[c] * e2v[b];
                    if (!(std::fabs(pa - pb) >= 1e-3 * (std::fabs(pa) + std::fabs(pb))) || !std::isfinite(pa) || !std::isfinite(pb))
                        f.sign_exact = 0u;
                }
                f.pair[hf] = (uint32_t)filtered.size();  // + n_other_pairs below
                filtered.push_back(cand_rec(i, pp));
                ++fill[a];
            }
        }
        for (int a = 0; a < 3; ++a) out.flat_pairs.insert(out.flat_pairs.end(), by_axis[a].begin(), by_axis[a].end());
        // records with the exact sign rule first: the kernels run them in a loop of their own (no branch on the rule per record)
        out.n_flat_exact = (uint32_t)(std::stable_partition(out.flat_pairs.begin(), out.flat_pairs.end(),
                                                            [](const FlatPairRec &f) { return f.sign_exact != 0u; }) -
                                      out.flat_pairs.begin());
        // by_axis went in x, y, z and the partition is stable: the exact records are sorted by axis, and the kernels run one loop
        // per axis over them without looking at a record's `axis` (cand_filter_and_drain)
        for (uint32_t &n : out.n_flat_exact_axis) n = 0u;
        for (uint32_t k = 0; k < out.n_flat_exact; ++k) ++out.n_flat_exact_axis[out.flat_pairs[k].axis];
        out.n_other_pairs = (uint32_t)out.cand_pairs.size();
        for (FlatPairRec &f : out.flat_pairs)
            for (int hf = 0; hf < 2; ++hf)
                if (f.pair[hf] != kNoPair) f.pair[hf] += out.n_other_pairs;
        out.cand_pairs.insert(out.cand_pairs.end(), filtered.begin(), filtered.end());
        out.cand_ok = out.cand_pairs.size() <= kCandMaxPairs;
    }
}

const char *bad_material(const pt_object &o) {
    for (float v : o.color)
        if (!finite_nonneg(v)) return "color";
    for (float v : o.emission)
        if (!finite_nonneg(v)) return "emission";
    return nullptr;
}

bool flatten_scene(const pt_camera &cam, const pt_object *objs, uint32_t n_objs, const pt_triangle *tris,
                   uint32_t n_tris, FlatScene &out, std::string &err, const Reach *origin_box, Reach *used) {
    if (n_objs >= (1u << 30) || n_tris >= (1u << 30)) {
        err = "scene too large";
        return false;
    }
    out.objs.assign(n_objs, ObjRec{});
    out.mats.assign(n_objs, MatRec{});
    out.tri_pairs.clear();
    out.bvh_nodes.clear();
    out.bvh_nodes4.clear();
    out.wide_src.clear();
    out.tri_shade.assign(n_tris, TriShade{});
    // R: bound on |ray origin - any vertex|: ray origins are the lens centre or points on objects - or, with an origin box,
    // the lens centre of any camera inside it
    Reach reach;
    scene_reach(cam, objs, n_objs, tris, n_tris, reach);
    vec3 slo = ld(reach.lo), shi = ld(reach.hi);
    if (origin_box) BvhBuilder::grow(slo, shi, ld(origin_box->lo), ld(origin_box->hi));
    if (used) {
        st(used->lo, slo);
        st(used->hi, shi);
    }
    const float scene_R = n_objs ? length(shi - slo) : 0.0f;
    std::vector<uint8_t> claimed(n_tris, 0);
    bool have_bvh = false;
    out.bvh_pair_base = 0;
    out.bvh_stack = 0;
    out.bvh_pair_span = 0;
    for (uint32_t i = 0; i < n_objs; ++i) {
        const pt_object &o = objs[i];
        if (o.kind != PT_SPHERE && o.kind != PT_MESH) {
            err = "object " + std::to_string(i) + ": unknown kind";
            return false;
        }
        if (o.reflect_type > PT_REFRACT) {
            err = "object " + std::to_string(i) + ": unknown reflect_type";
            return false;
        }
        if (const char *field = bad_material(o)) {
            err = "object " + std::to_string(i) + ": a component of " + field + " is negative or not finite";
            return false;
        }
        ObjRec &r = out.objs[i];
        object_head(o, slo, shi, r);
        if (o.kind == PT_MESH) {
            if ((uint64_t)o.tri_offset + o.tri_count > n_tris) {
                err = "object " + std::to_string(i) + ": triangle range outside the triangle array";
                return false;
            }
            r.tri_begin = o.tri_offset;
            r.tri_count = o.tri_count;
            r.pair_begin = (uint32_t)out.tri_pairs.size();
            for (uint32_t k = o.tri_offset; k < o.tri_offset + o.tri_count; ++k) {
                if (claimed[k]) {
                    err = "triangle " + std::to_string(k) + " belongs to two objects";
                    return false;
                }
                claimed[k] = 1;
            }
            std::vector<BuildTri> bt;
            mesh_triangles(i, o, tris, scene_R, out.tri_shade, bt);
            if (o.tri_count >= kBvhMinTris) {
                const size_t pairs_mark = out.tri_pairs.size(), nodes_mark = out.bvh_nodes.size();
                const std::vector<BuildTri> keep = bt;
                for (int attempt = 0; attempt < 2; ++attempt) {
                    BvhBuilder bb{out, bt};
                    bb.use_sah = attempt == 0;
                    vec3 blo, bhi;
                    r.bvh_root = bb.build(0, bt.size(), blo, bhi, 0);
                    if (bb.depth_max + 2 < kBvhStack) {
                        out.bvh_stack = std::max(out.bvh_stack, (uint32_t)bb.depth_max + 2u);
                        break;
                    }
                    if (attempt == 1) {
                        err = "object " + std::to_string(i) + ": BVH deeper than the traversal stack";
                        return false;
                    }
                    out.tri_pairs.resize(pairs_mark);  // SAH tree too deep for the stack: rebuild balanced
                    out.bvh_nodes.resize(nodes_mark);
                    bt = keep;
                }
                if (!have_bvh) out.bvh_pair_base = (uint32_t)pairs_mark;
                have_bvh = true;
                out.bvh_pair_span = (uint32_t)out.tri_pairs.size() - out.bvh_pair_base;
                if (!bvh_refs_fit(out.bvh_nodes.size(), out.tri_pairs.size())) {
                    err = "mesh too large for the BVH walkers: node indices and leaf codes are packed into 26 bits of a queue entry "
                          "(2^26 nodes, 2^25 pair records with leaves of two records)";
                    return false;
                }
            } else {
                out.tri_pairs.resize(out.tri_pairs.size() + (bt.size() + 1u) / 2u);
                list_pairs(bt, out.tri_pairs.data() + r.pair_begin);
            }
            r.pair_count = (uint32_t)out.tri_pairs.size() - r.pair_begin;
        }
        object_material(o, out.mats[i]);
    }
    derive_small(objs, n_objs, scene_R, out);
    // ranks: the reference's visiting sequence - objects from the last to the first (mod.rs:637), a mesh's triangles in
    // list order (mod.rs:558)
    std::vector<uint32_t> tri_rank(n_tris ? n_tris : 1u, 0u);
    out.rank_id.assign((size_t)n_objs + n_tris + 1u, 0u);
    {
        uint32_t next = 0;
        for (uint32_t v = 0; v < n_objs; ++v) {
            const uint32_t i = n_objs - 1u - v;
            if (objs[i].kind == PT_SPHERE) {
                out.rank_id[next++] = i;
            } else {
                for (uint32_t k = 0; k < objs[i].tri_count; ++k) {
                    tri_rank[objs[i].tri_offset + k] = next;
                    out.rank_id[next++] = n_objs + objs[i].tri_offset + k;
                }
            }
        }
    }
    // shading records by rank
    out.surf.assign(out.rank_id.size(), SurfRec{});
    for (size_t rk = 0; rk + 1 < out.rank_id.size(); ++rk) {
        const uint32_t id = out.rank_id[rk];
        SurfRec &sr = out.surf[rk];
        uint32_t owner = id;
        if (id >= n_objs) {
            const TriShade &ts = out.tri_shade[id - n_objs];
            sr.vx = ts.nx, sr.vy = ts.ny, sr.vz = ts.nz;
            owner = ts.owner;
        }
        const MatRec &mm = out.mats[owner];
        if (id < n_objs) sr.vx = mm.px, sr.vy = mm.py, sr.vz = mm.pz;
        surf_material(sr, mm, id >= n_objs);
    }
    out.tri_rank = tri_rank;
    out.bvh_meshes.clear();
    for (uint32_t v = 0; v < n_objs; ++v) {
        const ObjRec &r = out.objs[n_objs - 1u - v];
        if (r.kind != kKindMesh || r.bvh_root == kNoBvh) continue;
        BvhMeshRec bm{};
        bm.cx = r.cx, bm.cy = r.cy, bm.cz = r.cz, bm.rr = r.rr;
        bm.root = r.bvh_root;
        bm.root4 = widen(out.bvh_nodes, r.bvh_root, out.bvh_nodes4, out.wide_src);
        out.bvh_meshes.push_back(bm);
    }
    return true;
}

// ---------------------------------------------------------------------------------------------
// pt_ctx_set_object: the host side of an edit in place
int check_object_edit(bool has_ctx, const pt_object *obj, bool has_scene, const pt_object *objs, uint32_t n_objs, uint32_t index) {
    if (!has_ctx) return refuse("ctx is NULL");
    if (!obj) return refuse("obj is NULL");
    if (!has_scene) return refuse("no scene set: pt_ctx_set_object edits an object of the scene pt_ctx_set_scene gave");
    if (index >= n_objs) return refuse("index is not an object of the scene");
    const pt_object &have = objs[index];
    if (obj->kind != have.kind || obj->tri_offset != have.tri_offset || obj->tri_count != have.tri_count)
        return refuse("kind, tri_offset or tri_count differ from the object's: topology edits go through pt_ctx_set_scene");
    if (obj->reflect_type > PT_REFRACT) return refuse("unknown reflect_type");
    const float geo[] = {obj->position[0], obj->position[1], obj->position[2], obj->radius,
                         obj->bs_center[0], obj->bs_center[1], obj->bs_center[2], obj->bs_radius};
    for (float v : geo)
        if (!std::isfinite(v)) return refuse("a position, radius, bs_center or bs_radius that is not finite");
    if (const char *field = bad_material(*obj))
        return refuse((std::string("a component of ") + field + " is negative or not finite").c_str());
    return PT_OK;
}

bool same_geometry(const pt_object &a, const pt_object &b) {
    return memcmp(a.position, b.position, sizeof a.position) == 0 && memcmp(&a.radius, &b.radius, sizeof a.radius) == 0 &&
           memcmp(a.bs_center, b.bs_center, sizeof a.bs_center) == 0 && memcmp(&a.bs_radius, &b.bs_radius, sizeof a.bs_radius) == 0;
}

void local_vertex_box(const pt_triangle *tris, uint32_t n, Reach &out) {
    const float finf = std::numeric_limits<float>::infinity();
    vec3 lo = mk(finf, finf, finf), hi = mk(-finf, -finf, -finf);
    for (uint32_t k = 0; k < n; ++k) {
        BvhBuilder::grow(lo, hi, ld(tris[k].a), ld(tris[k].a));
        BvhBuilder::grow(lo, hi, ld(tris[k].b), ld(tris[k].b));
        BvhBuilder::grow(lo, hi, ld(tris[k].c), ld(tris[k].c));
    }
    st(out.lo, lo);
    st(out.hi, hi);
}

void object_bounds(const pt_object &o, const Reach &local, Reach &out) {
    const vec3 pos = ld(o.position);
    if (o.kind == PT_SPHERE) {
        const float r = f_abs(o.radius);
        st(out.lo, pos - mk(r, r, r));
        st(out.hi, pos + mk(r, r, r));
    } else {  // rounding is monotone: min over (v + pos) is (min over v) + pos
        st(out.lo, ld(local.lo) + pos);
        st(out.hi, ld(local.hi) + pos);
    }
}

bool grow_reach_box(Reach &B, const Reach &box) {
    bool grew = false;
    for (int a = 0; a < 3; ++a) {
        if (box.lo[a] < B.lo[a]) {
            B.lo[a] = box.lo[a] - (B.lo[a] - box.lo[a]);
            grew = true;
        }
        if (box.hi[a] > B.hi[a]) {
            B.hi[a] = box.hi[a] + (box.hi[a] - B.hi[a]);
            grew = true;
        }
    }
    return grew;
}

uint32_t object_rank(const pt_object *objs, uint32_t n_objs, uint32_t index) {
    uint32_t next = 0;
    for (uint32_t i = n_objs; i-- > index + 1u;) next += objs[i].kind == PT_SPHERE ? 1u : objs[i].tri_count;
    return next;
}

void edit_object(FlatScene &fs, const Reach &B, const pt_object *objs, uint32_t n_objs, const pt_triangle *tris, uint32_t index,
                 bool moved, ObjectEdit &e) {
    const pt_object &o = objs[index];
    const vec3 slo = ld(B.lo), shi = ld(B.hi);
    const float scene_R = n_objs ? length(shi - slo) : 0.0f;
    ObjRec &r = fs.objs[index];
    e.rank = object_rank(objs, n_objs, index);
    e.scene_R = scene_R;
    e.on_device = o.kind == PT_MESH && r.bvh_root != kNoBvh;
    e.obj_pair = (n_objs - 1u - index) / 2u;
    e.bvh_mesh = kRefitNone;
    if (e.on_device) {
        e.bvh_mesh = 0;
        for (uint32_t i = n_objs; i-- > index + 1u;) e.bvh_mesh += fs.objs[i].kind == kKindMesh && fs.objs[i].bvh_root != kNoBvh ? 1u : 0u;
    }
    object_material(o, fs.mats[index]);
    if (moved) {
        const ObjRec ranges = r;  // object_head writes the sphere's and clears the tree: the triangle ranges and the tree stay
        object_head(o, slo, shi, r);
        if (o.kind == PT_MESH) {
            r.tri_begin = ranges.tri_begin, r.tri_count = ranges.tri_count;
            r.pair_begin = ranges.pair_begin, r.pair_count = ranges.pair_count;
            r.bvh_root = ranges.bvh_root;
            if (!e.on_device) {
                std::vector<BuildTri> bt;
                mesh_triangles(index, o, tris, scene_R, fs.tri_shade, bt);
                list_pairs(bt, fs.tri_pairs.data() + r.pair_begin);
            }
        }
        derive_small(objs, n_objs, scene_R, fs);  // the small tables again, whole (bvh_meshes is not among them: the roots stay)
        if (e.on_device) {
            BvhMeshRec &bm = fs.bvh_meshes[e.bvh_mesh];
            bm.cx = r.cx, bm.cy = r.cy, bm.cz = r.cz, bm.rr = r.rr;
        }
    }
    // the surface records at the object's ranks: a sphere's one, a listed mesh's few; a mesh with a BVH gets its on the device
    e.surf.clear();
    e.tail.clear();
    if (index == 0u) {
        // flatten_scene fills the slots of surf past the last rank - one per mesh: rank_id has n_objs + n_tris entries, the
        // ranks are the spheres and the triangles - from rank_id's zeros: as a sphere's record of object 0.  No kernel reads them.
        uint32_t ranks = 0;
        for (uint32_t i = 0; i < n_objs; ++i) ranks += objs[i].kind == PT_SPHERE ? 1u : objs[i].tri_count;
        SurfRec sr{};
        sr.vx = fs.mats[0].px, sr.vy = fs.mats[0].py, sr.vz = fs.mats[0].pz;
        surf_material(sr, fs.mats[0], false);
        e.tail_at = ranks;
        e.tail.assign((size_t)n_objs + fs.tri_shade.size() - ranks, sr);
    }
    if (o.kind == PT_SPHERE) {
        SurfRec sr{};
        sr.vx = fs.mats[index].px, sr.vy = fs.mats[index].py, sr.vz = fs.mats[index].pz;
        surf_material(sr, fs.mats[index], false);
        e.surf.push_back(sr);
    } else if (!e.on_device) {
        for (uint32_t k = o.tri_offset; k < o.tri_offset + o.tri_count; ++k) {
            SurfRec sr{};
            sr.vx = fs.tri_shade[k].nx, sr.vy = fs.tri_shade[k].ny, sr.vz = fs.tri_shade[k].nz;
            surf_material(sr, fs.mats[index], true);
            e.surf.push_back(sr);
        }
    }
}

bool build_refit_plan(const FlatScene &fs, uint32_t index, RefitPlan &p) {
    p = RefitPlan{};
    const ObjRec &r = fs.objs[index];
    if (r.kind != kKindMesh || r.bvh_root == kNoBvh) return false;
    std::vector<std::vector<RefitNode>> by_height;
    uint32_t node_lo = kRefitNone, node_hi = 0;
    // height above the leaves of the subtree at `ref`, which is child `slot` of `parent` (the recursion is as deep as the tree: < kBvhStack)
    struct Walk {
        const FlatScene &fs;
        RefitPlan &p;
        std::vector<std::vector<RefitNode>> &by_height;
        uint32_t &node_lo, &node_hi;
        uint32_t go(int32_t ref, uint32_t parent, uint32_t slot) {
            if (ref < 0) {
                const uint32_t code = (uint32_t)~ref;
                p.leaves.push_back(RefitLeaf{leaf_first(code), leaf_count(code), parent, slot});
                return 0u;
            }
            const BvhNode &n = fs.bvh_nodes[(size_t)ref];
            node_lo = std::min(node_lo, (uint32_t)ref);
            node_hi = std::max(node_hi, (uint32_t)ref + 1u);
            const uint32_t h = 1u + std::max(go(n.c[0], (uint32_t)ref, 0u), go(n.c[1], (uint32_t)ref, 1u));
            if (parent != kRefitNone) {
                if (by_height.size() < h) by_height.resize(h);
                by_height[h - 1u].push_back(RefitNode{(uint32_t)ref, parent, slot});
            }
            return h;
        }
    } walk{fs, p, by_height, node_lo, node_hi};
    walk.go(r.bvh_root, kRefitNone, 0u);
    for (const std::vector<RefitNode> &level : by_height) {
        p.level_begin.push_back((uint32_t)p.nodes.size());
        p.nodes.insert(p.nodes.end(), level.begin(), level.end());
    }
    p.level_begin.push_back((uint32_t)p.nodes.size());
    for (size_t d = 0; d < fs.wide_src.size(); ++d) {
        const uint32_t src = fs.wide_src[d];
        if (src != kRefitNone && (src >> 1) >= node_lo && (src >> 1) < node_hi) p.wide.push_back(RefitWide{(uint32_t)d, src});
    }
    return true;
}

void run_refit_plan(const RefitPlan &p, const RefitTables &T) {
    for (const RefitLeaf &lf : p.leaves) refit_leaf(T, lf);
    for (const RefitNode &n : p.nodes) refit_node(T.nodes, n);  // (by height, ascending: children before parents)
    for (const RefitWide &w : p.wide) refit_wide(T.nodes4, T.nodes, w);
}

// ---------------------------------------------------------------------------------------------
// Passes and streams of a wavefront frame (plan_frame, below, follows the retries and adds the taper; shrink_request is the
// step after a failed allocation).
int plan_pass(const PassPlanIn &in, PassPlan &out, uint64_t *want_next) {
    const uint64_t npix = in.npix;
    uint32_t spp_pass = (uint32_t)std::min<uint64_t>(in.want / (npix ? npix : 1u), 0xffffffffull);
    if (spp_pass == 0) spp_pass = 1;
    if (spp_pass > in.spp) spp_pass = in.spp;
    if (spp_pass > kMaxPassSpp) spp_pass = kMaxPassSpp;  // sample-in-pass field of the stream bookkeeping word
    if (in.stack_form && spp_pass < in.spp) {
        // passes of equal length (4096 samples in passes of 682 at most would end with one of 4 samples: short streams,
        // a launch that cannot fill the chip); a pass may be up to a twentieth longer than asked for that - k_pass_cand's
        // memory does not grow with the pass
        const uint32_t stretch = spp_pass + spp_pass / 20u;
        const uint32_t n_eq = (in.spp + stretch - 1u) / stretch;
        const uint32_t eq = (in.spp + n_eq - 1u) / n_eq;
        if (eq <= kMaxPassSpp) spp_pass = eq;
    }
    // Streams: many more than the 2048 workgroups the chip holds at once, so that the dispatcher keeps every CU busy
    // until a launch ends, but each still a few launches' worth of work for its workgroup - about 2048 primary rays
    // per stream and pass (measured on cornell 1024x768: 2048 streams 22.0, 8192 24.3, 16384 24.7, 65536 23.2 G
    // bounces/s).  A stream owns at most kMaxStreamPixels pixels (their accumulators live in LDS inside k_shade).
    // (scenes with a BVH stage its nodes into LDS once per workgroup: twice the work per stream; mesh.json 2048 streams
    // 7.3, 8192 7.6, 16384 7.0)
    // (candidate scan, four waves per SIMD: 12288 streams 35.8, 16384 35.4, 8192 32.2, 24576 33.7 G bounces/s)
    // (candidate scan with walks, mesh.json: 24576 streams 19.8, 26624 20.5, 28672 20.1, 30720 20.3, 32768 19.9 G bounces/s)
    // (k_pass_cand's waves run without levels: a wave's first and last trips - the stack fills, the last rays die - are
    // the only ones that are not full, so its streams are long: 12 Ki primaries 43.4, 24 Ki 44.3, 48 Ki 43.8.  Fewer, much
    // longer streams - 2 048 of 384 pixels, two rounds of resident workgroups - lose: 42.0 against 46.4; 4 096: 43.4; 8 192:
    // 45.1 - same instruction count, but a fifth of the launch with few workgroups left (PMC: busy cycles per bounce 1.97
    // against 1.64 at fewer wave-cycles): streams are not equally long and two rounds cannot average that out)
    // (round 4, with the walk queue over the four-wide tree: scenes with walks a little shorter - mesh.json 1024x768 @1024,
    // 18 Ki primaries per stream 29.0, 20 Ki 29.1, 21-22 Ki 29.2, 24 Ki 28.7, 32 Ki 28.5 G bounces/s; cornell.json is flat from 12 Ki to
    // 48 Ki: 47.2-47.7)
    const uint64_t per_stream = in.stack_form ? (uint64_t)(in.per_stream ? in.per_stream : (in.has_bvh ? 22528u : 16384u))
                                              : (in.has_bvh ? 4096u : 2048u);
    uint64_t k_target = (npix * spp_pass + per_stream - 1u) / per_stream;
    if (k_target < 2048u) k_target = 2048u;
    if (in.streams) k_target = in.streams;
    uint32_t m = (uint32_t)((npix + k_target - 1) / k_target);
    if (m == 0) m = 1;
    if (m > kMaxStreamPixels) m = kMaxStreamPixels;
    // k_pass_cand: frames of few samples get more, shorter streams rather than a handful of workgroups per CU slot, each
    // with hundreds of pixels' accumulators and tables (36 B per pixel) in LDS (1024x768 @128: 12 288 streams of 64
    // pixels, not 4 096 of 192)
    // (round 4, final kernels: with walks up to 128 - 3000x2000 @100, parts of 2^20 pixels: 64 pixels 25.2, 96: 27.1, 128: 27.7, 192: 24.2 G
    // bounces/s on mesh.json, 1024x768 @128: 26.4 / 27.0 / 26.9 / 23.4; without walks the two frames disagree - 49.0 / 50.4 / 50.6 / 48.5
    // and 50.4 / 49.5 / 49.0 / 47.9 - and 64 stays)
    const uint32_t m_few = in.has_bvh ? 128u : 64u;
    if (in.stack_form && !in.streams && m > m_few) m = m_few;
    // A launch runs its workgroups in rounds of as many as the chip holds (four per CU); a stream's work grows with its m
    // pixels, so a launch takes about ceil(K / resident) x m: among the m within -15 % / +20 % of the tuned size take the
    // one for which that is smallest (cornell 1024x768: m = 21 -> 24, 37 450 streams in 36.6 rounds -> 32 768 in 32.0,
    // 37.3 -> 37.7 G bounces/s).  Not for scenes with walks, whose streams differ too much in length for rounds to show
    // (mesh.json: 24.0 rounds are slower than 25.6).
    // SMALL FRAMES (round 4: the reference's own sizes - its launch configuration is 450x300 @500, .vscode/launch.json).  When
    // the tuned stream size gives the launch fewer than eight rounds of resident workgroups, what a launch takes is
    // ceil(K / resident) x m to a good approximation, and a last round that is mostly empty costs a whole round: 450x300
    // @500 at the tuned size is 2 756 streams of 49 pixels = 2.7 rounds, mesh.json 21.3 G bounces/s; 4 120 streams of 33
    // pixels = 4.02 rounds: 26.2; 5 493 of 25 = 5.4 rounds: 23.6; 8 240 of 17 = 8.05: 25.0 (cornell.json: 42.1 / 43.0 / 43.2 /
    // 43.8 - the same order, flatter).  So among the stream sizes from a quarter of the tuned one up to it, the one with the
    // least ceil(K / resident) x m; of equals the longer streams where rays walk (their streams differ most in length), the
    // shorter ones otherwise.
    bool small_frame = false;
    if (in.stack_form && !in.streams && in.n_cus != 0u && m >= 4u) {
        const uint64_t resident = (uint64_t)in.n_cus * (in.groups_per_cu ? in.groups_per_cu : 4u);
        const uint64_t k_tuned = (npix + m - 1u) / m;
        // (fewer than EIGHT rounds - sixteen until the final kernels of round 4: at 12.8 rounds, 3000x2000 @100 in parts of 2^20
        // pixels, the rule took streams of 20 pixels for the whole rounds' sake and lost 6 % to the 64-pixel streams it replaced)
        if ((k_tuned + resident - 1u) / resident < 8u) {
            small_frame = true;
            uint32_t best_m = m;
            uint64_t best_cost = ~0ull;
            for (uint32_t mm = m / 4u ? m / 4u : 1u; mm <= m; ++mm) {
                const uint64_t kk = (npix + mm - 1u) / mm;
                const uint64_t cost = ((kk + resident - 1u) / resident) * mm;
                if (cost < best_cost || (cost == best_cost && in.has_bvh)) {
                    best_cost = cost;
                    best_m = mm;
                }
            }
            m = best_m;
        }
    }
    if (!small_frame && in.cand_scan && !in.has_bvh && !in.streams && in.n_cus != 0u && m >= 8u) {
        const uint64_t resident = (uint64_t)in.n_cus * (in.groups_per_cu ? in.groups_per_cu : 4u);
        uint32_t best_m = m;
        uint64_t best_cost = ~0ull;
        for (uint32_t mm = m - m * 15u / 100u; mm <= m + m / 5u && mm <= (in.stack_form ? 72u : kMaxStreamPixels); ++mm) {
            const uint64_t kk = (npix + mm - 1u) / mm;
            const uint64_t cost = ((kk + resident - 1u) / resident) * mm;
            if (cost < best_cost || (cost == best_cost && (mm > m ? mm - m : m - mm) < (best_m > m ? best_m - m : m - best_m))) {
                best_cost = cost;
                best_m = mm;
            }
        }
        m = best_m;
    }
    const uint32_t K = (uint32_t)((npix + m - 1) / m);
    // a primary ray has at most 4 descendants alive at one depth (two refract splits, mod.rs:760); k_pass_cand gives each
    // of its four waves a quarter of the slice and ceil(n / 4) of the stream's n primaries: 4 * ceil(n / 4) <= n + 3
    uint64_t cap64 = (4ull * m * spp_pass + 16u + kBlock - 1) / kBlock * kBlock;
    // k_pass_cand keeps a wave's waiting rays on a stack of at most kWaveStackMax slots (a quarter of the stream's slice
    // per wave, a power of two of at least 128 slots; a pass whose waves' whole quarters fit a smaller stack gets that)
    if (in.stack_form) {
        // (a wave gets every fourth chunk of 64 of the stream's m * spp_pass primaries: at most ceil(chunks / 4) * 64 of them, each
        // with at most four descendants waiting at a time - k_pass_cand's `room_for_all`)
        const uint64_t n_prim = (uint64_t)m * spp_pass, most = ((n_prim + 63u) / 64u + 3u) / 4u * 64u;
        const uint64_t need_w = 4u * (most < n_prim ? most : n_prim) + 3u;
        uint64_t cap_w = 128u;
        const uint64_t stack_max = in.wave_stack ? in.wave_stack : kWaveStackMax;
        while (cap_w < need_w && cap_w < stack_max) cap_w *= 2u;
        cap64 = 4u * cap_w;
        const size_t need = queue_bytes(K, (uint32_t)cap64) + (in.stack_park ? (size_t)K * 4u * kWaveParkBytes : 0u);
        if (in.stack_budget && need > in.stack_budget && spp_pass > 1u) {
            // the default pass does not fit the budget: smaller passes have fewer streams or smaller stacks
            *want_next = npix * (spp_pass / 2u);
            return kPlanRetry;
        }
    }
    // (slot indices are 32-bit over the whole queue, byte offsets 32-bit inside a stream's slice of cap * 40 bytes)
    if (cap64 * K > 0xffffffffull / 2 || cap64 * kRayBytes > 0xffffffffull) {
        if (spp_pass > 1u && in.want_is_default) {  // (a default this large only on a device with > 680 GB)
            *want_next = in.want / 2;
            return kPlanRetry;
        }
        return kPlanTooLarge;
    }
    out.spp_pass = spp_pass;
    out.m = m;
    out.K = K;
    out.cap = (uint32_t)cap64;
    out.bytes0 = queue_bytes(K, out.cap);
    out.bytes1 = in.stack_form ? (in.stack_park ? (size_t)K * 4u * kWaveParkBytes : 0u) : out.bytes0;
    return kPlanOk;
}

Taper plan_taper(const PassPlan &plan, const TaperIn &in) {
    Taper off;
    if (in.n_cut == 0u || in.pieces < 2u || in.probe || plan.K == 0u) return off;
    Taper t;
    t.n_cut = in.n_cut < plan.K ? in.n_cut : plan.K;
    while (t.lg_pieces < 6u && (2u << t.lg_pieces) <= in.pieces) ++t.lg_pieces;
    t.pieces = 1u << t.lg_pieces;
    if (!in.forced && in.pass_samples < t.pieces) return off;
    if (!in.forced && in.resident != 0u && plan.K < (uint64_t)kTaperMinRounds * in.resident) return off;
    const uint64_t more = (uint64_t)t.n_cut * (t.pieces - 1u);
    t.extra0 = queue_bytes(more, plan.cap);
    t.extra1 = in.stack_park ? (size_t)more * 4u * kWaveParkBytes : 0u;
    if (in.budget && plan.bytes0 + plan.bytes1 + t.extra0 + t.extra1 > in.budget) return off;
    // (slot indices are 32-bit over the whole container, as in plan_pass)
    if ((uint64_t)plan.cap * (plan.K + more) > 0xffffffffull / 2) return off;
    return t;
}

// ---------------------------------------------------------------------------------------------
// The plan of a wavefront frame (pt_host.h).  The staging question is asked of lds_layout itself: pt_layout.h is host-only.
uint32_t pass_groups_per_cu(bool stack_form, bool has_bvh) {
    return !stack_form ? 4u : (has_bvh ? (uint32_t)PT_CAND_BVH_WAVES : (uint32_t)PT_CAND_WAVES);
}

// Level-by-level forms (k_pass, k_pass_bvh, the separate kernels): 96 Mi primary rays per pass by default, 36 GB of ray
// queues of the 288 GB of HBM - fewer, longer launches: cornell 1024x768 @4096 spp 32 Mi 35.7, 48 Mi 35.7, 64 Mi 36.2, 96 Mi
// 36.4 G bounces/s (a launch ends with its slowest streams).  k_pass_cand (`stack_form`) keeps a wave's waiting rays on a stack
// of at most kWaveStackMax slots whatever the pass holds: its passes are sized by TIME (pt_api.hip: PassPacer) - 512 Mi primary
// rays at most - and its memory is the streams' (K x 4 waves x stack x 40 B: 4.0 GB for the 24 576 streams of the bench frame's
// pass).  Passes only change how the samples are batched, never the image.
FrameRequest first_request(const FramePlanIn &in) {
    FrameRequest r;
    r.want = in.rays_per_pass ? in.rays_per_pass : in.rays_per_pass_tuned;
    const bool given = r.want != 0u, stack_form = in.pass.stack_form;
    const uint64_t dflt = stack_form ? (512u << 20) : (96u << 20);
    // bytes the pass may take (0: unbounded); an explicit size without an explicit budget is taken as given
    size_t avail = in.mem_budget;
    if (!given) {
        r.want = dflt;
        if (!avail) avail = (size_t)((double)in.mem_avail * 0.85) / (in.mem_share ? in.mem_share : 1u);
    }
    if (stack_form)
        r.stack_budget = avail;  // (plan_pass retries with smaller passes until the streams' stacks fit)
    else if (avail)
        r.want = std::min<uint64_t>(r.want, avail / kLevelBytesPerPrimary);
    if (!given && in.mem_share > 1u) r.want = std::min(r.want, dflt / in.mem_share);  // (co-resident contexts also share the chip)
    if (!given || in.mem_budget) r.want = std::max(r.want, in.pass.npix);  // one sample per pixel and pass at least
    r.try_taper = stack_form;  // (k_pass_cand's alone; plan_taper has the rules, knobs by hand and PROBE instances among them)
    return r;
}

int plan_frame(const FramePlanIn &in, const FrameRequest &req, FramePlan &out) {
    PassPlanIn pin = in.pass;
    pin.want = req.want;
    pin.want_is_default = !in.rays_per_pass;
    pin.groups_per_cu = pass_groups_per_cu(pin.stack_form, pin.has_bvh);
    pin.stack_budget = req.stack_budget;
    out = FramePlan{};
    int pr;
    uint64_t want_next = pin.want;
    while ((pr = plan_pass(pin, out.pass, &want_next)) == kPlanRetry) {  // (every retry asks for less: it ends)
        pin.want = want_next;
        ++out.retries;
    }
    if (pr != kPlanOk || !req.try_taper) return pr;
    // the taper's knobs by hand (PT_TAPER_CUT, PT_TAPER_PIECES, PT_PER_STREAM) are taken as given; the defaults are kTaper*
    const bool walks = pin.has_bvh;
    TaperIn tin;
    tin.forced = in.taper_cut >= 0;
    tin.resident = (uint64_t)pin.n_cus * pin.groups_per_cu;
    const uint64_t cut_dflt = (uint64_t)(walks ? kTaperCutHalfRoundsBvh : kTaperCutHalfRounds) * tin.resident / 2u;
    tin.n_cut = (uint32_t)std::min<uint64_t>(tin.forced ? (uint64_t)in.taper_cut : cut_dflt, 0xffffffffu);
    tin.pieces = in.taper_pieces ? in.taper_pieces : (walks ? kTaperPiecesBvh : kTaperPieces);
    tin.pass_samples = out.pass.spp_pass;
    tin.budget = req.stack_budget;
    tin.stack_park = pin.stack_park;
    tin.probe = in.probe;
    // longer streams with the default taper - if the plan is otherwise the same pass and the records stay staged
    PassPlan plan_t = out.pass;
    const uint32_t long_stream = walks ? kTaperPerStreamBvh : kTaperPerStream;
    if (!tin.forced && !pin.per_stream && !pin.streams && long_stream != 0u) {
        PassPlanIn pin_t = pin;
        pin_t.per_stream = long_stream;
        uint64_t unused = pin.want;
        if (plan_pass(pin_t, plan_t, &unused) != kPlanOk || plan_t.spp_pass != out.pass.spp_pass ||
            lds_layout(in.scene, plan_t.m, in.lds_pad).staged != lds_layout(in.scene, out.pass.m, in.lds_pad).staged)
            plan_t = out.pass;
    }
    out.taper = plan_taper(plan_t, tin);
    if (out.taper.on()) out.pass = plan_t;
    return kPlanOk;
}

bool shrink_request(const FramePlanIn &in, const FramePlan &plan, FrameRequest &req) {
    if (plan.taper.on()) {  // the taper goes before a pass is halved
        req.try_taper = false;
        return true;
    }
    if (plan.pass.spp_pass <= 1u) return false;
    req.want = in.pass.npix * std::max(1u, plan.pass.spp_pass / 2u);
    return true;
}

uint32_t next_pass_samples(double rate, double target_ms, uint64_t npix, uint64_t probe, uint32_t s_prev, uint32_t left,
                           uint32_t max_pass) {
    if (npix == 0u) npix = 1u;
    uint64_t fit = rate > 0.0 ? (uint64_t)(rate * target_ms / (double)npix) : probe / npix;
    if (s_prev && fit > 16ull * s_prev) fit = 16ull * s_prev;
    if (fit < 1u) fit = 1u;
    if (fit > max_pass) fit = max_pass;
    uint64_t stretch = fit + fit / 5u;
    if (stretch > max_pass) stretch = max_pass;
    const uint32_t n_left = (uint32_t)((left + stretch - 1u) / stretch);
    return (left + n_left - 1u) / n_left;
}

RoundPlan plan_rounds(uint64_t entries, uint32_t spp_left, uint64_t rays_per_pass, uint32_t item_mult, uint32_t n_cus) {
    const uint64_t round_budget = rays_per_pass ? rays_per_pass : (256ull << 20);  // primary samples per launch
    uint64_t round_spp = round_budget / entries;
    if (round_spp == 0) round_spp = 1;
    if (round_spp > spp_left) round_spp = spp_left;
    RoundPlan p{(uint32_t)round_spp, 1u};
    // (k_mega_cand hands its items out dynamically: finer ones - 8 per lane the chip holds, cornell 41.3 G bounces/s; 4: 39.1,
    // 16: 40.5, 32: 38.4 - so that a launch's last items are a small part of it)
    const uint64_t want_items = (uint64_t)item_mult * n_cus * 2048u;
    while (entries * p.n_split < want_items && p.n_split < p.round_spp) p.n_split *= 2;
    if (p.n_split > p.round_spp) p.n_split = p.round_spp;
    return p;
}

RoundLaunch round_launch(uint64_t entries, uint32_t n_split, uint32_t s_here, uint32_t n_cus) {
    RoundLaunch l;
    l.split = n_split < s_here ? n_split : s_here;
    l.lane_spp = (s_here + l.split - 1) / l.split;
    const uint64_t grid = (entries * l.split + kBlock - 1) / kBlock, max_grid = (uint64_t)n_cus * 8u;
    l.grid = (uint32_t)(grid < max_grid ? grid : max_grid);
    if (l.grid == 0u) l.grid = 1u;
    return l;
}

// ---------------------------------------------------------------------------------------------
// Frame calls and the held frame of pt_ctx_accumulate
int check_cfg(const pt_config *cfg, uint32_t *idx_begin, uint32_t *idx_end) {
    if (!cfg) return refuse("cfg is NULL");
    if (cfg->width == 0 || cfg->height == 0 || cfg->spp == 0) return refuse("width, height and spp must be positive");
    const uint64_t npix = (uint64_t)cfg->width * cfg->height;
    if (npix > 0x7fffffffull) return refuse("width*height exceeds 2^31-1");
    if (cfg->spp > (1u << 24)) return refuse("spp exceeds 2^24");
    uint32_t b = cfg->idx_begin, e = cfg->idx_end;
    if (b == 0 && e == 0) e = (uint32_t)npix;
    if (b >= e || e > npix) return refuse("band [idx_begin, idx_end) is empty or outside the frame");
    if (cfg->backend != PT_BACKEND_WAVEFRONT && cfg->backend != PT_BACKEND_MEGAKERNEL) return refuse("unknown backend");
    if (cfg->chunk_step > 1u && (cfg->chunk_pixels == 0u || cfg->chunk_first >= cfg->chunk_step))
        return refuse("chunk_pixels must be positive and chunk_first < chunk_step");
    *idx_begin = b;
    *idx_end = e;
    return PT_OK;
}

uint32_t owned_pixels(const pt_config *cfg, uint32_t b, uint32_t e) {
    const uint64_t span = e - b;
    if (cfg->chunk_step <= 1u) return (uint32_t)span;
    const uint64_t C = cfg->chunk_pixels, n_chunks = (span + C - 1) / C;
    uint64_t total = 0;
    for (uint64_t c = cfg->chunk_first; c < n_chunks; c += cfg->chunk_step) {
        const uint64_t lo = c * C, hi = (lo + C < span) ? lo + C : span;
        total += hi - lo;
    }
    return (uint32_t)total;
}

uint32_t part_pixels(uint32_t total, bool wavefront) { return (wavefront && total > (3u << 19)) ? (1u << 20) : total; }

AccumKey accum_key(const pt_config *cfg, uint32_t b, uint32_t e) {
    AccumKey k{};
    k.width = cfg->width;
    k.height = cfg->height;
    k.idx_begin = b;
    k.idx_end = e;
    if (cfg->chunk_step > 1u) {
        k.chunk_pixels = cfg->chunk_pixels;
        k.chunk_first = cfg->chunk_first;
        k.chunk_step = cfg->chunk_step;
    }
    k.seed = cfg->seed;
    return k;
}

std::vector<Job> accum_jobs(const FrameCounts &f, uint32_t spp, bool megakernel) {
    std::vector<Job> jobs;
    auto job = [&](Part p, uint32_t part_lo, uint32_t part_hi) {
        const uint32_t c = f.cnt[part_lo];
        const float base = (float)p.k0 / (float)f.total, scale = (float)p.n / (float)f.total;
        if (f.tracked() && c < spp) {
            const uint32_t m = tracked_split(c, spp);
            // (a renderer reports the samples issued over its job's last sample: the first job's fractions are scaled to the call's)
            const float f1 = (float)m / (float)spp;
            jobs.push_back({p.k0, p.n, c, base, scale * f1, part_lo, part_hi, m});
            if (m < spp) jobs.push_back({p.k0, p.n, m, base, scale, part_lo, part_hi, spp, base + scale * f1});
            return;
        }
        jobs.push_back({p.k0, p.n, c, base, scale, part_lo, part_hi});
    };
    bool even = true;
    for (uint32_t v : f.cnt) even = even && v == f.cnt[0];
    for (uint32_t v : f.na) even = even && v == f.na[0];
    if (megakernel && even)
        job({0u, f.total}, 0u, f.n_parts());
    else
        for (uint32_t i = 0; i < f.n_parts(); ++i) job(f.part(i), i, i + 1u);
    return jobs;
}

// ---------------------------------------------------------------------------------------------
// The checkpoint file.  Its layout is written down here and nowhere else: magic, u32 version, the key (7 x u32, u64 seed), u64
// scene fingerprint, u32 total, part_px, number of parts - 68 bytes; the parts' counts; half A's counts (version 2); the held
// sums; half A's sums (version 2); u64 SipHash-1-3 of everything before it.
namespace {
constexpr char kCkptMagic[8] = {'P', 'T', 'A', 'C', 'C', 'U', 'M', '1'};
constexpr uint32_t kCkptVersion = 1u;         // the held sums
constexpr uint32_t kCkptVersionTracked = 2u;  // ... and half A of a noise-tracked frame: its counts after the counts, its planes after the sums
constexpr size_t kCkptHead = 8 + 4 + 7 * 4 + 8 + 8 + 3 * 4;  // magic .. number of parts: 68 bytes

template <class T>
void put(std::vector<uint8_t> &b, T v) {
    const size_t at = b.size();
    b.resize(at + sizeof v);
    memcpy(b.data() + at, &v, sizeof v);
}
template <class T>
T get(const uint8_t *&r) {
    T v;
    memcpy(&v, r, sizeof v);
    r += sizeof v;
    return v;
}

// The wire form both formats share.  The head: magic, u32 version, the key (7 x u32, u64 seed).
void put_head(std::vector<uint8_t> &b, const char (&magic)[8], uint32_t version, const AccumKey &k) {
    b.insert(b.end(), magic, magic + 8);
    put<uint32_t>(b, version);
    for (uint32_t v : {k.width, k.height, k.idx_begin, k.idx_end, k.chunk_pixels, k.chunk_first, k.chunk_step}) put<uint32_t>(b, v);
    put<uint64_t>(b, k.seed);
}
AccumKey get_key(const uint8_t *&r) {
    AccumKey k;
    for (uint32_t *v : {&k.width, &k.height, &k.idx_begin, &k.idx_end, &k.chunk_pixels, &k.chunk_first, &k.chunk_step}) *v = get<uint32_t>(r);
    k.seed = get<uint64_t>(r);
    return k;
}
// the pt_config a key stands for (one sample), and whether the key is one check_cfg accepts and accum_key writes: [ib, ie) its band
bool key_frame(const AccumKey &k, pt_config &kc, uint32_t &ib, uint32_t &ie) {
    kc = pt_config{};
    kc.width = k.width;
    kc.height = k.height;
    kc.spp = 1;
    kc.idx_begin = k.idx_begin;
    kc.idx_end = k.idx_end;
    kc.chunk_pixels = k.chunk_pixels;
    kc.chunk_first = k.chunk_first;
    kc.chunk_step = k.chunk_step;
    kc.seed = k.seed;
    return check_cfg(&kc, &ib, &ie) == PT_OK && accum_key(&kc, ib, ie) == k;
}

// The frame of a sealed file, whose order of refusals is part of the contract: too short, the first `head` bytes asked for, magic,
// version (1 .. versions), the format's header - header(version, r, want_size) reads its fields from r, behind the version, and
// says what is wrong with them or how long they imply the file to be -, truncated / trailing bytes, the whole file asked for, the
// trailing hash, the format's body - body(): what lies behind the header, or what is wrong with it.  Nothing behind the header
// is looked at before the file's size is the one the header implies.
template <class Header, class Body>
int sealed_decode(uint64_t file_size, const uint8_t *b, size_t n, const char (&magic)[8], uint32_t versions, size_t head, SealedFile &out,
                  std::string &why, Header header, Body body) {
    auto bad = [&](const char *w) {
        why = w;
        return kCkptBad;
    };
    auto more = [&](size_t need) {
        out.need = need;
        return kCkptMore;
    };
    if (file_size < head + 8) return bad("too short");
    if (n < head) return more(head);
    if (memcmp(b, magic, 8) != 0) return bad("wrong magic");
    const uint8_t *r = b + 8;
    const uint32_t version = get<uint32_t>(r);
    if (version < 1u || version > versions) return bad("unknown format version");
    uint64_t want_size = 0;
    if (const char *w = header(version, r, want_size)) return bad(w);
    if (file_size != want_size) return bad(file_size < want_size ? "truncated" : "trailing bytes");
    if (n < want_size) return more((size_t)want_size);
    uint64_t tag;
    memcpy(&tag, b + want_size - 8, 8);
    if (tag != pt_siphash(1, 3, 0, 0, b, (size_t)want_size - 8)) return bad("bad trailing hash");
    if (const char *w = body()) return bad(w);
    return kCkptOk;
}
}  // namespace

void ckpt_encode_head(const Checkpoint &ck, std::vector<uint8_t> &b) {
    const size_t halves = ck.tracked() ? 2u : 1u;
    b.reserve(b.size() + kCkptHead + halves * (4 * ck.cnt.size() + 24 * (size_t)ck.total) + 8);
    put_head(b, kCkptMagic, ck.tracked() ? kCkptVersionTracked : kCkptVersion, ck.key);
    put<uint64_t>(b, ck.scene_fp);
    put<uint32_t>(b, ck.total);
    put<uint32_t>(b, ck.part_px);
    put<uint32_t>(b, (uint32_t)ck.cnt.size());
    for (uint32_t v : ck.cnt) put<uint32_t>(b, v);
    for (uint32_t v : ck.na) put<uint32_t>(b, v);
}

void ckpt_seal(std::vector<uint8_t> &b) { put<uint64_t>(b, pt_siphash(1, 3, 0, 0, b.data(), b.size())); }

int ckpt_decode(uint64_t file_size, const uint8_t *b, size_t n, Checkpoint &out, std::string &why) {
    uint32_t n_parts = 0;
    size_t halves = 1;
    auto header = [&](uint32_t version, const uint8_t *r, uint64_t &want_size) -> const char * {
        halves = version == kCkptVersionTracked ? 2u : 1u;
        out.key = get_key(r);
        out.scene_fp = get<uint64_t>(r);
        const uint32_t total = out.total = get<uint32_t>(r), part_px = out.part_px = get<uint32_t>(r);
        n_parts = get<uint32_t>(r);
        // the key must be a valid frame's, and the sizes must be the ones it implies
        pt_config kc;
        uint32_t ib = 0, ie = 0;
        if (!key_frame(out.key, kc, ib, ie)) return "the frame key is not a valid frame";
        const uint32_t want_total = owned_pixels(&kc, ib, ie);
        if (total != want_total || want_total == 0u || part_px != part_pixels(total, true) || n_parts != part_count(total, part_px))
            return "sizes that do not fit each other";
        out.sums_at = kCkptHead + halves * 4 * (size_t)n_parts;
        out.a_at = out.sums_at + 24 * (size_t)total;
        want_size = kCkptHead + halves * (4ull * n_parts + 24ull * total) + 8ull;
        return nullptr;
    };
    auto body = [&]() -> const char * {
        out.cnt.resize(n_parts);
        memcpy(out.cnt.data(), b + kCkptHead, 4 * (size_t)n_parts);
        for (uint32_t v : out.cnt)
            if (v > (1u << 24)) return "a sample count above 2^24";
        out.na.assign(halves == 2u ? n_parts : 0u, 0u);
        if (halves == 2u) {
            memcpy(out.na.data(), b + kCkptHead + 4 * (size_t)n_parts, 4 * (size_t)n_parts);
            for (uint32_t i = 0; i < n_parts; ++i)
                if (out.na[i] > out.cnt[i]) return "half A holds more samples than the part";
        }
        return nullptr;
    };
    return sealed_decode(file_size, b, n, kCkptMagic, kCkptVersionTracked, kCkptHead, out, why, header, body);
}

// ---------------------------------------------------------------------------------------------
// The noise estimate
float noise_part_weight(uint32_t na, uint32_t nb) {
    const float fa = (float)na, fb = (float)nb;
    return __builtin_sqrtf(fa * fb) / (fa + fb);
}

static constexpr uint32_t kNoiseBinCount = sizeof(pt_noise_stats::histogram) / sizeof(uint32_t);

float noise_bin_upper(uint32_t b) {
    if (b >= kNoiseBinCount - 1u) return std::numeric_limits<float>::infinity();
    const uint32_t bits = (461u + b) << 21;
    float v;
    memcpy(&v, &bits, 4);
    return v;
}

uint32_t noise_quantile_bin(const pt_noise_stats &s, float quantile) {
    const double need_d = (double)quantile * (double)s.pixels;
    uint64_t need = (uint64_t)need_d;
    if ((double)need < need_d) ++need;
    need = need ? need : 1u;
    uint64_t cum = 0;
    uint32_t b = 0;
    for (; b < kNoiseBinCount; ++b)
        if ((cum += s.histogram[b]) >= need) break;
    return b;
}

bool noise_target_met(const pt_noise_stats &s, const pt_noise_target &t) {
    if (t.mean_error != 0.0f && !(s.mean_error <= (double)t.mean_error)) return false;
    return t.quantile == 0.0f || noise_bin_upper(noise_quantile_bin(s, t.quantile)) <= t.quantile_error;
}

int check_noise_target(const pt_noise_target &t) {
    if (!finite_nonneg(t.mean_error) || !finite_nonneg(t.quantile) || !finite_nonneg(t.quantile_error))
        return refuse("noise target: mean_error, quantile and quantile_error must be finite and not negative");
    if (t.mean_error == 0.0f && t.quantile == 0.0f) return refuse("noise target: neither mean_error nor quantile is in use");
    if (!(t.quantile < 1.0f)) return refuse("noise target: quantile must lie in (0, 1)");
    return PT_OK;
}

// ---------------------------------------------------------------------------------------------
// Adaptive sampling
int check_adaptive_params(const pt_adaptive_params &p, uint32_t *tile_shift) {
    if (!finite_nonneg(p.tile_error)) return refuse("adaptive: tile_error must be finite and not negative");
    const uint32_t tile = p.tile ? p.tile : 8u;
    if (tile != 4u && tile != 8u && tile != 16u && tile != 32u) return refuse("adaptive: tile must be 4, 8, 16 or 32 (0 = 8)");
    *tile_shift = tile == 4u ? 2u : (tile == 8u ? 3u : (tile == 16u ? 4u : 5u));
    return PT_OK;
}

int check_adaptive_cfg(const pt_config &cfg) {
    if (cfg.width != 0u && (cfg.idx_begin % cfg.width != 0u || cfg.idx_end % cfg.width != 0u))
        return refuse("adaptive: the band must consist of whole image rows");
    if (cfg.chunk_step > 1u || ((cfg.flags >> 8) & 15u) != 0u)
        return refuse("adaptive: chunk_step > 1 and PT_FLAG_PIPELINES are not supported");
    return PT_OK;
}

int tile_geometry(uint32_t width, uint32_t rows, uint32_t tile_shift, TileGeometry &out) {
    const uint64_t tile = 1ull << tile_shift;
    const uint64_t tiles_x = (width + tile - 1u) / tile, tiles = tiles_x * ((rows + tile - 1u) / tile);
    if (tiles * tile * tile >= (1ull << 32)) return refuse("adaptive: the band's tiles hold 2^32 pixels or more");
    out = {tile_shift, (uint32_t)tiles_x, (uint32_t)tiles};
    return PT_OK;
}

TileTotals tile_totals(uint32_t width, uint32_t rows, const TileGeometry &g, const uint32_t *tile_spp, const unsigned long long *tile_err,
                       unsigned long long err_sum) {
    const uint32_t tile = 1u << g.tile_shift;
    TileTotals t{};
    for (uint32_t i = 0; i < g.tiles; ++i) {
        const uint32_t x0 = i % g.tiles_x * tile, y0 = i / g.tiles_x * tile;
        const uint64_t pixels = (uint64_t)std::min(width - x0, tile) * std::min(rows - y0, tile);
        t.samples += pixels * tile_spp[i];
        if (tile_err[i] != kTileNoError) t.est_pixels += pixels;
    }
    const uint64_t npix = (uint64_t)width * rows;
    t.mean_error = t.est_pixels == npix ? (double)err_sum * (1.0 / 268435456.0) / (double)npix : std::numeric_limits<double>::infinity();
    return t;
}

// ---------------------------------------------------------------------------------------------
// The held adaptive frame: which class is next, what is held, the checkpoint
AdaptiveSchedule::AdaptiveSchedule(const TileTable &t, uint32_t width, uint32_t rows, const TileGeometry &g, unsigned long long q,
                                   uint32_t cap, uint32_t n0)
    : cap_(cap), n0_(n0) {
    std::vector<uint64_t> keys;
    for (uint32_t i = 0; i < g.tiles; ++i)
        if (!tile_closed(t.err[i], q, tile_pixels(width, rows, g, i))) keys.push_back((uint64_t)t.cnt[i] << 32 | t.na[i]);
    std::sort(keys.begin(), keys.end());
    for (uint64_t k : keys) {
        if (classes_.empty() || classes_.back().first != k) classes_.push_back({k, 0u});
        ++classes_.back().second;
    }
    open_ = (uint32_t)keys.size();
}

bool AdaptiveSchedule::next(AdaptiveStep &s) const {
    if (classes_.empty() || (uint32_t)(classes_.front().first >> 32) >= cap_) return false;  // (ascending: no class is below the cap)
    s.c = (uint32_t)(classes_.front().first >> 32);
    s.na = (uint32_t)classes_.front().first;
    s.n = classes_.front().second;
    s.T = adaptive_next_count(s.c, n0_, cap_);
    s.m = tracked_split(s.c, s.T);
    s.to_a[0] = deal_to_a(s.c, s.na);
    s.na_end = s.na + (s.to_a[0] ? s.m - s.c : 0u);
    s.to_a[1] = s.m < s.T && deal_to_a(s.m, s.na_end);
    if (s.to_a[1]) s.na_end += s.T - s.m;
    return true;
}

void AdaptiveSchedule::done(const AdaptiveStep &s, uint32_t still_open, uint32_t closed) {
    classes_.erase(classes_.begin());
    open_ -= closed;
    if (still_open == 0u) return;
    const uint64_t k = (uint64_t)s.T << 32 | s.na_end;
    auto at = std::lower_bound(classes_.begin(), classes_.end(), std::make_pair(k, 0u));
    if (at != classes_.end() && at->first == k)
        at->second += still_open;
    else
        classes_.insert(at, {k, still_open});
}

uint32_t AdaptiveSchedule::tiles_at_cap() const {
    uint32_t n = 0;
    for (const auto &c : classes_)
        if ((uint32_t)(c.first >> 32) >= cap_) n += c.second;
    return n;
}

// The adaptive checkpoint's layout: magic, u32 version, the key as PTACCUM1 writes it (7 x u32, u64 seed), u32 tile edge, u32 n_0,
// u64 scene fingerprint, u32 call pixels, u32 tiles - 72 bytes; per tile u32 count, u32 nA, u64 E; the held sums; half A's sums;
// u64 SipHash-1-3 of everything before it.
namespace {
constexpr char kAdCkptMagic[8] = {'P', 'T', 'A', 'D', 'A', 'P', 'T', '1'};
constexpr uint32_t kAdCkptVersion = 1u;
constexpr size_t kAdCkptHead = 8 + 4 + 7 * 4 + 8 + 2 * 4 + 8 + 2 * 4;  // 72 bytes
}  // namespace

void adckpt_encode_head(const AdaptiveCheckpoint &ck, std::vector<uint8_t> &b) {
    b.reserve(b.size() + kAdCkptHead + 16 * (size_t)ck.tiles + 48 * (size_t)ck.total + 8);
    put_head(b, kAdCkptMagic, kAdCkptVersion, ck.key.frame);
    put<uint32_t>(b, ck.key.tile);
    put<uint32_t>(b, ck.key.n0);
    put<uint64_t>(b, ck.scene_fp);
    put<uint32_t>(b, ck.total);
    put<uint32_t>(b, ck.tiles);
    for (uint32_t i = 0; i < ck.tiles; ++i) {
        put<uint32_t>(b, ck.table.cnt[i]);
        put<uint32_t>(b, ck.table.na[i]);
        put<uint64_t>(b, ck.table.err[i]);
    }
}

int adckpt_decode(uint64_t file_size, const uint8_t *b, size_t n, AdaptiveCheckpoint &out, std::string &why) {
    auto header = [&](uint32_t, const uint8_t *r, uint64_t &want_size) -> const char * {
        const AccumKey &k = out.key.frame = get_key(r);
        const uint32_t tile = out.key.tile = get<uint32_t>(r), n0 = out.key.n0 = get<uint32_t>(r);
        out.scene_fp = get<uint64_t>(r);
        const uint32_t total = out.total = get<uint32_t>(r), tiles = out.tiles = get<uint32_t>(r);
        // the key must be one the call accepts and writes, and the sizes must be the ones it implies
        pt_config kc;
        pt_adaptive_params kp{};
        kp.tile = tile;
        uint32_t ib = 0, ie = 0, tile_shift = 0;
        if (!key_frame(k, kc, ib, ie) || check_adaptive_cfg(kc) != PT_OK) return "the frame key is not a valid frame";
        if (tile == 0u || check_adaptive_params(kp, &tile_shift) != PT_OK || n0 == 0u || n0 % 8u != 0u || n0 > 0xfffffff8u)
            return "the tile edge or n_0 is not one the call writes";
        TileGeometry g{};
        if (total != ie - ib || tile_geometry(k.width, total / k.width, tile_shift, g) != PT_OK || tiles != g.tiles || tiles == 0u)
            return "sizes that do not fit each other";
        out.sums_at = kAdCkptHead + 16 * (size_t)tiles;
        out.a_at = out.sums_at + 24 * (size_t)total;
        want_size = kAdCkptHead + 16ull * tiles + 48ull * total + 8ull;
        return nullptr;
    };
    auto body = [&]() -> const char * {
        TileTable &t = out.table;
        t.cnt.resize(out.tiles);
        t.na.resize(out.tiles);
        t.err.resize(out.tiles);
        const uint8_t *r = b + kAdCkptHead;
        for (uint32_t i = 0; i < out.tiles; ++i) {
            t.cnt[i] = get<uint32_t>(r);
            t.na[i] = get<uint32_t>(r);
            t.err[i] = get<uint64_t>(r);
            if (t.cnt[i] > (1u << 24)) return "a sample count above 2^24";
            if (t.na[i] > t.cnt[i]) return "half A holds more samples than the tile";
            if (t.err[i] != kTileNoError && (t.na[i] == 0u || t.na[i] == t.cnt[i])) return "an E of a tile with an empty half";
        }
        return nullptr;
    };
    return sealed_decode(file_size, b, n, kAdCkptMagic, kAdCkptVersion, kAdCkptHead, out, why, header, body);
}

// ---- pt_ctx_denoise, pt_ctx_denoise_var (ptrace.h, pt_denoise.h)
// What the two filters share once their parameters are read: the frame's size, the planes (`var`: pt_ctx_denoise_var's, with its
// error map), the context, then the frame and the levels' schedule - sigma is sigma_color or sigma_var.
static int denoise_tail(const void *ctx, uint32_t width, uint32_t height, uint32_t levels, float sigma, float sigma_depth,
                        uint32_t flags, bool var, const float *d_color, const float *d_error, const float *d_albedo, const float *d_normal,
                        const float *d_depth, float *d_out, DenoiseCall &call) {
    if (!width || !height) return refuse("width and height must be positive");
    if ((uint64_t)width * height > (1ull << 28)) return refuse("width*height exceeds 2^28");
    if (!var && (!d_color || !d_out)) return refuse("d_color or d_out is NULL");
    if (!d_color) return refuse("d_color is NULL");
    if (var && !d_error) return refuse("d_error is NULL: pt_ctx_denoise is the filter without a noise estimate");
    if (!d_out) return refuse("d_out is NULL");
    if (!ctx) return refuse("ctx is NULL");
    call = DenoiseCall{};
    DenoiseFrame &f = call.f;
    f.width = width;
    f.height = height;
    f.color = d_color;
    f.albedo = (flags & PT_DENOISE_NO_DEMODULATE) ? nullptr : d_albedo;
    f.normal = d_normal;
    f.depth = d_depth;
    f.error = d_error;
    f.out = d_out;
    call.levels = levels;
    const float kv = sigma * sigma;
    float scale = 1.0f;  // 2^-i
    for (uint32_t i = 0; i < levels; ++i, scale *= 0.5f) {
        const float sc = sigma * scale;
        call.rc[i] = d_error ? kv : 1.0f / (sc * sc);  // with an error map the colour scale is per pixel, from kv
        call.sds[i] = sigma_depth * (float)(1u << i);
    }
    return PT_OK;
}

int check_denoise(const void *ctx, uint32_t width, uint32_t height, const pt_denoise_params *params, const float *d_color,
                  const float *d_albedo, const float *d_normal, const float *d_depth, float *d_out, DenoiseCall &call) {
    pt_denoise_params P = kDenoiseDefaults;
    if (params) {
        if (params->levels > kDenoiseMaxLevels) return refuse("pt_denoise_params.levels exceeds 8");
        if (!finite_nonneg(params->sigma_color) || !finite_nonneg(params->sigma_depth))
            return refuse("pt_denoise_params: a sigma is negative or not finite");
        if (!(params->sigma_normal_pow == 0.0f)) return refuse("pt_denoise_params.sigma_normal_pow is reserved and must be 0");
        if (params->flags & ~PT_DENOISE_NO_DEMODULATE) return refuse("pt_denoise_params.flags: unknown bits");
        if (params->levels) P.levels = params->levels;
        if (params->sigma_color != 0.0f) P.sigma_color = params->sigma_color;
        if (params->sigma_depth != 0.0f) P.sigma_depth = params->sigma_depth;
        P.flags = params->flags;
    }
    return denoise_tail(ctx, width, height, P.levels, P.sigma_color, P.sigma_depth, P.flags, false, d_color, nullptr, d_albedo, d_normal,
                        d_depth, d_out, call);
}

int check_denoise_var(const void *ctx, uint32_t width, uint32_t height, const pt_denoise_var_params *params, const float *d_color,
                      const float *d_error, const float *d_albedo, const float *d_normal, const float *d_depth, float *d_out,
                      DenoiseCall &call) {
    pt_denoise_var_params P = kDenoiseVarDefaults;
    if (params) {
        if (params->levels > kDenoiseMaxLevels) return refuse("pt_denoise_var_params.levels exceeds 8");
        if (!finite_nonneg(params->sigma_var) || !finite_nonneg(params->sigma_depth))
            return refuse("pt_denoise_var_params: a sigma is negative or not finite");
        if (params->flags & ~PT_DENOISE_NO_DEMODULATE) return refuse("pt_denoise_var_params.flags: unknown bits");
        if (params->levels) P.levels = params->levels;
        if (params->sigma_var != 0.0f) P.sigma_var = params->sigma_var;
        if (params->sigma_depth != 0.0f) P.sigma_depth = params->sigma_depth;
        P.flags = params->flags;
    }
    return denoise_tail(ctx, width, height, P.levels, P.sigma_var, P.sigma_depth, P.flags, true, d_color, d_error, d_albedo, d_normal,
                        d_depth, d_out, call);
}

// ---- pt_ctx_present (ptrace.h, pt_present.h)
int check_present(const void *ctx, uint32_t width, uint32_t height, const pt_present_params *params, const float *d_rgb, uint8_t *d_out,
                  PresentFrame &f) {
    pt_present_params P{};
    if (params) P = *params;
    if (!finite_nonneg(P.exposure)) return refuse("pt_present_params.exposure is negative or not finite");
    if (P.format != PT_PRESENT_RGBA8 && P.format != PT_PRESENT_RGB8) return refuse("pt_present_params.format: unknown format");
    if (P.flags & ~PT_PRESENT_FRAMEBUFFER_ORDER) return refuse("pt_present_params.flags: unknown bits");
    if (!width || !height) return refuse("width and height must be positive");
    if ((P.out_width == 0u) != (P.out_height == 0u)) return refuse("pt_present_params: one of out_width, out_height is 0 alone");
    const uint32_t ow = P.out_width ? P.out_width : width, oh = P.out_height ? P.out_height : height;
    if ((uint64_t)width * height > (1ull << 28) || (uint64_t)ow * oh > (1ull << 28))
        return refuse("width*height or out_width*out_height exceeds 2^28");
    if (!d_rgb) return refuse("d_rgb is NULL");
    if (!d_out) return refuse("d_out is NULL");
    if (!ctx) return refuse("ctx is NULL");
    f = PresentFrame{};
    f.rgb = d_rgb;
    f.out = d_out;
    f.width = width;
    f.height = height;
    f.out_width = ow;
    f.out_height = oh;
    f.bpp = P.format == PT_PRESENT_RGBA8 ? 4u : 3u;
    f.flip = !(P.flags & PT_PRESENT_FRAMEBUFFER_ORDER);
    f.exposure = P.exposure == 0.0f ? 1.0f : P.exposure;
    return PT_OK;
}

// ---- pt_ctx_overlay (ptrace_overlay.h, pt_overlay.h)
int check_overlay_params(const pt_overlay_params *params, pt_overlay_params &P) {
    P = pt_overlay_params{};
    if (params) P = *params;
    if (P.flags & ~(PT_OVERLAY_SKY | PT_OVERLAY_GRID)) return refuse("pt_overlay_params.flags: unknown bits");
    if (P.n_selected > PT_OVERLAY_MAX_SELECTED) return refuse("pt_overlay_params.n_selected exceeds 16");
    for (uint32_t i = 0; i < P.n_selected; ++i)
        if (P.selected[i] < 0) return refuse("pt_overlay_params.selected: an object index is negative");
    if (P.radius > PT_OVERLAY_MAX_RADIUS) return refuse("pt_overlay_params.radius exceeds 8");
    const float *colours[] = {P.outline_color, P.fill_color, P.sky_top, P.sky_bottom, P.grid_color};
    for (const float *c : colours)
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(c[a])) return refuse("pt_overlay_params: a colour component is not finite");
    for (float a : {P.outline_alpha, P.fill_alpha, P.grid_alpha})
        if (!(a >= 0.0f && a <= 1.0f)) return refuse("pt_overlay_params: an alpha is not finite or outside [0, 1]");
    if (P.flags & PT_OVERLAY_GRID) {
        for (float v : {P.grid_spacing, P.grid_half_width, P.grid_extent})
            if (!(v > 0.0f && v < __builtin_inff())) return refuse("pt_overlay_params: the grid's spacing, half width and extent must be finite and positive");
        if (!std::isfinite(P.grid_y)) return refuse("pt_overlay_params.grid_y is not finite");
    }
    if (!P.radius) P.radius = kOverlayRadius;
    if (P.outline_alpha == 0.0f) P.outline_alpha = 1.0f;
    if (P.grid_alpha == 0.0f) P.grid_alpha = 1.0f;
    return PT_OK;
}

int overlay_view(const pt_camera &cam, OverlayFrame &f) {
    float lens[3], su[3], sv[3];
    camera_basis(cam, lens, su, sv);
    if (!std::isfinite(lens[0]) || !std::isfinite(lens[1]) || !std::isfinite(lens[2])) return refuse("cam: the lens centre is not finite");
    f.C = ld(cam.position);
    f.L = ld(lens);
    f.su = ld(su);
    f.sv = ld(sv);
    return PT_OK;
}

int check_overlay(const void *ctx, uint32_t width, uint32_t height, const pt_overlay_params *params, const pt_camera *cam,
                  const float *d_rgb, const int32_t *d_object_id, const float *d_depth, float *d_out, OverlayFrame &f) {
    f = OverlayFrame{};
    const int rc = check_overlay_params(params, f.p);
    if (rc) return rc;
    if (!width || !height) return refuse("width and height must be positive");
    if ((uint64_t)width * height > (1ull << 28)) return refuse("width*height exceeds 2^28");
    if (!d_rgb) return refuse("d_rgb is NULL");
    if (!d_out) return refuse("d_out is NULL");
    if (!d_object_id && (f.p.n_selected || (f.p.flags & PT_OVERLAY_SKY)))
        return refuse("d_object_id is NULL with a selection or PT_OVERLAY_SKY");
    if (!d_depth && (f.p.flags & PT_OVERLAY_GRID)) return refuse("d_depth is NULL with PT_OVERLAY_GRID");
    if (f.p.flags) {
        if (!cam) return refuse("cam is NULL with PT_OVERLAY_SKY or PT_OVERLAY_GRID");
        const int rv = overlay_view(*cam, f);
        if (rv) return rv;
    }
    if (!ctx) return refuse("ctx is NULL");
    f.width = width;
    f.height = height;
    f.rgb = d_rgb;
    f.out = d_out;
    // the planes the call does not need are not handed to the kernel: without ids it stages nothing
    f.object_id = f.p.n_selected || (f.p.flags & PT_OVERLAY_SKY) ? d_object_id : nullptr;
    f.depth = (f.p.flags & PT_OVERLAY_GRID) ? d_depth : nullptr;
    return PT_OK;
}

// ---- pt_ctx_solid (ptrace_solid.h, pt_solid.h)
int check_solid_params(const pt_solid_params *params, pt_solid_params &P) {
    P = params ? *params : kSolidDefaults;
    if (P.flags & ~(PT_SOLID_HEADLIGHT | PT_SOLID_REFLECT_SKY)) return refuse("pt_solid_params.flags: unknown bits");
    if (P.shininess_log2 > PT_SOLID_MAX_SHININESS_LOG2) return refuse("pt_solid_params.shininess_log2 exceeds 10");
    for (float v : {P.ambient, P.diffuse, P.specular})
        if (!finite_nonneg(v)) return refuse("pt_solid_params: ambient, diffuse or specular is negative or not finite");
    if (!(P.flags & PT_SOLID_HEADLIGHT))
        for (float v : P.light)
            if (!std::isfinite(v)) return refuse("pt_solid_params.light: a component is not finite");
    const float *colours[] = {P.background, P.sky_top, P.sky_bottom};
    for (const float *c : colours)
        for (int a = 0; a < 3; ++a)
            if (!finite_nonneg(c[a])) return refuse("pt_solid_params: a colour component of background, sky_top or sky_bottom is negative or not finite");
    return PT_OK;
}

int check_solid_look(const pt_solid_look &look) {
    if (look.reflect_type > PT_REFRACT) return refuse("looks: a reflect_type is above PT_REFRACT");
    for (float v : look.emission)
        if (!finite_nonneg(v)) return refuse("looks: an emission component is negative or not finite");
    return PT_OK;
}

int check_solid_view(uint32_t width, uint32_t height, const pt_camera *cam, SolidFrame &f) {
    if (!width || !height) return refuse("width and height must be positive");
    if ((uint64_t)width * height > (1ull << 28)) return refuse("width*height exceeds 2^28");
    if (!cam) return refuse("cam is NULL");
    float lens[3], su[3], sv[3];
    camera_basis(*cam, lens, su, sv);
    if (!std::isfinite(lens[0]) || !std::isfinite(lens[1]) || !std::isfinite(lens[2])) return refuse("cam: the lens centre is not finite");
    f.width = width;
    f.height = height;
    f.C = ld(cam->position);
    f.L = ld(lens);
    f.su = ld(su);
    f.sv = ld(sv);
    return PT_OK;
}

int check_solid(const void *ctx, uint32_t width, uint32_t height, const pt_solid_params *params, const pt_camera *cam, const float *d_albedo,
                const float *d_normal, const float *d_depth, const int32_t *d_object_id, const pt_solid_look *looks, uint32_t n_looks,
                float *d_out, SolidFrame &f) {
    f = SolidFrame{};
    int rc = check_solid_params(params, f.p);
    if (!rc) rc = check_solid_view(width, height, cam, f);
    if (rc) return rc;
    if (!d_normal) return refuse("d_normal is NULL");
    if (!d_depth) return refuse("d_depth is NULL");
    if (!d_object_id) return refuse("d_object_id is NULL");
    if (!d_out) return refuse("d_out is NULL");
    if (n_looks > kSolidMaxLooks) return refuse("n_looks exceeds 2^20");
    if (!looks && n_looks) return refuse("looks is NULL with n_looks != 0");
    for (uint32_t i = 0; i < n_looks; ++i) {
        rc = check_solid_look(looks[i]);
        if (rc) return rc;
    }
    if (!ctx) return refuse("ctx is NULL");
    f.albedo = d_albedo;
    f.normal = d_normal;
    f.depth = d_depth;
    f.object_id = d_object_id;
    f.out = d_out;
    f.looks = n_looks ? looks : nullptr;
    f.n_looks = n_looks;
    return PT_OK;
}

bool solid_wide(const SolidFrame &f) {
    const uintptr_t all = (uintptr_t)f.albedo | (uintptr_t)f.normal | (uintptr_t)f.depth | (uintptr_t)f.object_id | (uintptr_t)f.out;
    return (all & 15u) == 0u && (uint64_t)f.width * f.height >= kSolidLanePixels;
}

// ---- the tone stage (ptrace_tone.h, pt_tone.h)
static bool finite_pos(float v) { return v > 0.0f && v < __builtin_inff(); }

int check_tonemap_params(const pt_tonemap_params *params, ToneFrame &f) {
    const pt_tonemap_params P = params ? *params : kTonemapDefaults;
    if (P.curve > PT_TONE_ACES) return refuse("pt_tonemap_params.curve: unknown curve");
    if (P.flags & ~PT_TONE_LUMA) return refuse("pt_tonemap_params.flags: unknown bits");
    if (!finite_pos(P.exposure)) return refuse("pt_tonemap_params.exposure is not finite and above 0");
    if (P.curve == PT_TONE_REINHARD && !finite_pos(P.white)) return refuse("pt_tonemap_params.white is not finite and above 0");
    f.curve = P.curve;
    f.luma = (P.flags & PT_TONE_LUMA) != 0u;
    f.exposure = P.exposure;
    f.iw2 = P.curve == PT_TONE_REINHARD ? 1.0f / (P.white * P.white) : 0.0f;
    return PT_OK;
}

int check_tonemap(const void *ctx, uint32_t width, uint32_t height, const pt_tonemap_params *params, const float *d_rgb, float *d_out,
                  ToneFrame &f) {
    f = ToneFrame{};
    const int rc = check_tonemap_params(params, f);
    if (rc) return rc;
    if (!width || !height) return refuse("width and height must be positive");
    if ((uint64_t)width * height > (1ull << 28)) return refuse("width*height exceeds 2^28");
    if (!d_rgb) return refuse("d_rgb is NULL");
    if (!d_out) return refuse("d_out is NULL");
    if (!ctx) return refuse("ctx is NULL");
    f.width = width;
    f.height = height;
    f.rgb = d_rgb;
    f.out = d_out;
    return PT_OK;
}

int check_meter(const void *ctx, uint32_t width, uint32_t height, const pt_meter_params *params, const float *d_rgb,
                const int32_t *d_object_id, const pt_meter_stats *out, MeterFrame &f) {
    pt_meter_params P{};
    if (params) P = *params;
    if (P.flags & ~PT_METER_SKIP_MISSES) return refuse("pt_meter_params.flags: unknown bits");
    if (!width || !height) return refuse("width and height must be positive");
    if ((uint64_t)width * height > (1ull << 28)) return refuse("width*height exceeds 2^28");
    if (P.x0 | P.y0 | P.x1 | P.y1) {
        if (P.x0 >= P.x1 || P.y0 >= P.y1) return refuse("pt_meter_params: the rectangle is empty");
        if (P.x1 > width || P.y1 > height) return refuse("pt_meter_params: the rectangle leaves the frame");
    } else {
        P.x1 = width, P.y1 = height;
    }
    if (!d_rgb) return refuse("d_rgb is NULL");
    if ((P.flags & PT_METER_SKIP_MISSES) && !d_object_id) return refuse("PT_METER_SKIP_MISSES without d_object_id");
    if (!out) return refuse("out is NULL");
    if (!ctx) return refuse("ctx is NULL");
    f = MeterFrame{};
    f.rgb = d_rgb;
    f.object_id = (P.flags & PT_METER_SKIP_MISSES) ? d_object_id : nullptr;
    f.npix = width * height;
    f.pitch = width;
    if (P.x0 == 0u && P.x1 == width) {  // whole rows: one run
        f.first = P.y0 * width;
        f.span = (P.y1 - P.y0) * width;
        f.rows = 1u;
    } else {
        f.first = P.y0 * width + P.x0;
        f.span = P.x1 - P.x0;
        f.rows = P.y1 - P.y0;
    }
    f.row_groups = (f.span + 3u) / 4u + 1u;
    return PT_OK;
}

int check_meter_exposure(const pt_meter_exposure_params *params, pt_meter_exposure_params &P) {
    P = params ? *params : kMeterExposureDefaults;
    if (!finite_pos(P.key)) return refuse("pt_meter_exposure_params.key is not finite and above 0");
    for (float v : {P.low_fraction, P.high_fraction})
        if (!(v >= 0.0f && v < 1.0f)) return refuse("pt_meter_exposure_params: a fraction is outside [0, 1)");
    if (!((double)P.low_fraction + (double)P.high_fraction < 1.0)) return refuse("pt_meter_exposure_params: the fractions leave nothing");
    if (!finite_pos(P.min_exposure)) return refuse("pt_meter_exposure_params.min_exposure is not finite and above 0");
    if (!(P.max_exposure >= P.min_exposure && P.max_exposure < __builtin_inff()))
        return refuse("pt_meter_exposure_params.max_exposure is not finite or below min_exposure");
    return PT_OK;
}

void meter_weights(const pt_meter_stats &s, const pt_meter_exposure_params &P, double kept[PT_METER_BINS], double *sum_w, double *sum_wl) {
    uint64_t N = 0;
    for (uint32_t b = 0; b < PT_METER_BINS; ++b) N += s.histogram[b];
    const double n = (double)N, lo = (double)P.low_fraction * n, hi = n - (double)P.high_fraction * n;
    double sw = 0.0, swl = 0.0;
    uint64_t c = 0;
    for (uint32_t b = 0; b < PT_METER_BINS; ++b) {
        const double below = (double)c, upto = (double)(c + s.histogram[b]);
        const double w = (upto < hi ? upto : hi) - (below > lo ? below : lo);
        kept[b] = w > 0.0 ? w : 0.0;
        sw += kept[b];
        swl += kept[b] * (-20.0 + ((double)b + 0.5) / 8.0);
        c += s.histogram[b];
    }
    *sum_w = sw;
    *sum_wl = swl;
}

bool tone_wide(const ToneFrame &f) {
    return (((uintptr_t)f.rgb | (uintptr_t)f.out) & 15u) == 0u && (uint64_t)f.width * f.height >= kToneLanePixels;
}

bool meter_wide(const MeterFrame &f) { return (((uintptr_t)f.rgb | (uintptr_t)f.object_id) & 15u) == 0u; }

bool hdr_wide(const HdrFrame &f) {
    // the three planes are `total` u64 apart: all 16-byte aligned when the first is and total is even; a lane's four pixels
    // share one count: there is one part, or no part boundary inside a group of four
    return (((uintptr_t)f.sums | (uintptr_t)f.out) & 15u) == 0u && (f.total & 1u) == 0u && f.total >= kToneLanePixels &&
           (!f.counts || f.part_px % kToneLanePixels == 0u);
}

void meter_stats_of(const uint32_t counters[kMeterWords], pt_meter_stats *out) {
    memset(out, 0, sizeof *out);
    out->dark = counters[kMeterDark];
    out->pixels = out->dark;
    for (uint32_t b = 0; b < PT_METER_BINS; ++b) {
        out->histogram[b] = counters[b];
        out->pixels += counters[b];
    }
    memcpy(&out->max_luminance, &counters[kMeterMax], 4);
}

// ---- the firefly stage (ptrace_despike.h, pt_despike.h)
int check_despike(const void *ctx, uint32_t width, uint32_t height, const pt_despike_params *params, const float *d_rgb,
                  const int32_t *d_object_id, float *d_out, uint8_t *d_mask, DespikeFrame &f) {
    const pt_despike_params P = params ? *params : kDespikeDefaults;
    if (P.radius < 1u || P.radius > kDespikeMaxRadius) return refuse("pt_despike_params.radius is not 1 or 2");
    if (P.rank < 1u || P.rank > kDespikeMaxRank || P.rank > (2u * P.radius + 1u) * (2u * P.radius + 1u) - 1u)
        return refuse("pt_despike_params.rank is not in 1..4");
    if (P.flags & ~PT_DESPIKE_SAME_OBJECT) return refuse("pt_despike_params.flags: unknown bits");
    if (!(P.threshold >= 1.0f && P.threshold < __builtin_inff())) return refuse("pt_despike_params.threshold is not finite and at least 1");
    if (!(P.floor >= 0.0f && P.floor < __builtin_inff())) return refuse("pt_despike_params.floor is not finite and at least 0");
    if (!width || !height) return refuse("width and height must be positive");
    if ((uint64_t)width * height > (1ull << 28)) return refuse("width*height exceeds 2^28");
    if (!d_rgb) return refuse("d_rgb is NULL");
    if (!d_out) return refuse("d_out is NULL");
    if (d_out == d_rgb) return refuse("d_out is d_rgb: the pass gathers and cannot run in place");
    if ((P.flags & PT_DESPIKE_SAME_OBJECT) && !d_object_id) return refuse("PT_DESPIKE_SAME_OBJECT without d_object_id");
    if (!ctx) return refuse("ctx is NULL");
    f = DespikeFrame{};
    f.width = width;
    f.height = height;
    f.rgb = d_rgb;
    f.object_id = (P.flags & PT_DESPIKE_SAME_OBJECT) ? d_object_id : nullptr;
    f.out = d_out;
    f.mask = d_mask;
    f.radius = P.radius;
    f.rank = P.rank;
    f.threshold = P.threshold;
    f.floor = P.floor;
    return PT_OK;
}

template <int RANK>
static void despike_frame_rank(const DespikeFrame &f, unsigned long long counts[2]) {
    const int64_t W = f.width, H = f.height, R = f.radius;
    for (int64_t r = 0; r < H; ++r) {
        for (int64_t x = 0; x < W; ++x) {
            const size_t idx = (size_t)(r * W + x);
            const float *v = f.rgb + idx * 3u;
            float o[3] = {0.0f, 0.0f, 0.0f};
            uint32_t m = kDespikeNonfinite;
            if (!despike_nonfinite(v[0], v[1], v[2])) {
                float t[RANK];
                for (int k = 0; k < RANK; ++k) t[k] = kDespikeNone;
                for (int64_t qr = r - R; qr <= r + R; ++qr) {
                    for (int64_t qx = x - R; qx <= x + R; ++qx) {
                        if ((qr == r && qx == x) || qx < 0 || qx >= W || qr < 0 || qr >= H) continue;
                        const size_t q = (size_t)(qr * W + qx);
                        if (f.object_id && f.object_id[q] != f.object_id[idx]) continue;
                        despike_push<RANK>(t, despike_y(f.rgb[q * 3u], f.rgb[q * 3u + 1u], f.rgb[q * 3u + 2u]));
                    }
                }
                m = despike_verdict(f.threshold, f.floor, t[RANK - 1], v, o);
            }
            memcpy(f.out + idx * 3u, o, sizeof o);
            if (f.mask) f.mask[idx] = (uint8_t)m;
            if (m == kDespikeSpike) ++counts[0];
            if (m == kDespikeNonfinite) ++counts[1];
        }
    }
}

void despike_frame(const DespikeFrame &f, unsigned long long counts[2]) {
    counts[0] = counts[1] = 0ull;
    switch (f.rank) {
        case 1u: return despike_frame_rank<1>(f, counts);
        case 2u: return despike_frame_rank<2>(f, counts);
        case 3u: return despike_frame_rank<3>(f, counts);
        default: return despike_frame_rank<4>(f, counts);
    }
}

// ---- pt_ctx_reproject (ptrace.h, pt_reproject.h)
void reproject_view(const pt_camera &cam, const pt_camera *hist_cam, ReprojectView &out) {
    out = ReprojectView{};
    float lens[3], su[3], sv[3];
    camera_basis(cam, lens, su, sv);
    out.C = ld(cam.position);
    out.L = ld(lens);
    out.su = ld(su);
    out.sv = ld(sv);
    if (!hist_cam) return;
    camera_basis(*hist_cam, lens, su, sv);
    out.hL = ld(lens);
    out.hD = ld(hist_cam->direction);
    out.hDf = out.hD * hist_cam->focal_length;
    out.hsu = ld(su);
    out.hsv = ld(sv);
    out.hfdd = hist_cam->focal_length * dot(out.hD, out.hD);
    out.hsuu = dot(out.hsu, out.hsu);
    out.hsvv = dot(out.hsv, out.hsv);
    out.same = memcmp(&cam, hist_cam, sizeof(pt_camera)) == 0 ? 1u : 0u;  // nine floats, no padding
}

// ---- the motion table of pt_ctx_reproject_moved, pt_ctx_reproject_var_moved and pt_ctx_reproject_var_weighted
int check_reproject_motion(int rc_plain, const pt_object_motion *motion, uint32_t n_motion, int *how) {
    if (rc_plain) return rc_plain;
    if (n_motion > kReprojectMaxMotion) return refuse("n_motion exceeds 2^20");
    if (!motion && n_motion) return refuse("motion is NULL with n_motion != 0");
    bool plain = true;
    for (uint32_t i = 0; i < (motion ? n_motion : 0u); ++i) {
        const pt_object_motion &r = motion[i];
        if (reproject_rec_identity(r) || reproject_rec_marker(r)) {
            plain = plain && !reproject_rec_marker(r);
            continue;
        }
        plain = false;
        const bool fin = std::isfinite(r.offset[0]) && std::isfinite(r.offset[1]) && std::isfinite(r.offset[2]);
        if (!(r.scale > 0.0f && r.scale < __builtin_inff()) || !fin)
            return refuse("motion: a record that is neither IDENTITY nor the marker needs a finite scale > 0 and finite offsets");
    }
    *how = plain ? kMotionPlain : kMotionTable;
    return PT_OK;
}

// ---- the five entry points: one call (pt_reproject.h, ReprojectArgs).  A colour-only call is a var call whose min_frames and
// radius are 0 and which has no moments, error or plane; what differs in a refusal is the params struct's name and the two
// lists of pointers.
int check_reproject(const ReprojectArgs &a, ReprojectCall &call) {
    pt_reproject_var_params P{};
    if (a.var && a.var_params) P = *a.var_params;
    if (!a.var && a.params) P = {a.params->weight, a.params->max_history, a.params->depth_tol, a.params->normal_min, 0u, 0u, a.params->flags};
    // (the message is put together only when there is one: an accepted call allocates nothing)
    auto refuse_params = [&](const char *what) {
        return refuse((std::string(a.var ? "pt_reproject_var_params" : "pt_reproject_params") + what).c_str());
    };
    if (!finite_nonneg(P.max_history) || !finite_nonneg(P.depth_tol))
        return refuse_params(": max_history or depth_tol is negative or not finite");
    if (!(P.normal_min >= -1.0f && P.normal_min <= 1.0f)) return refuse_params(".normal_min is outside [-1, 1]");
    if (P.radius > kReprojectVarMaxRadius) return refuse_params(".radius exceeds 3");
    if (P.flags) return refuse_params(".flags: none is defined");
    if (!a.width || !a.height) return refuse("width and height must be positive");
    if ((uint64_t)a.width * a.height > (1ull << 28)) return refuse("width*height exceeds 2^28");
    if (!a.cam || !a.color || !a.depth || !a.object_id || !a.out_color || !a.out_len || (a.var && (!a.out_moments || !a.error)))
        return refuse(a.var ? "cam, d_color, d_depth, d_object_id, d_out_color, d_out_len, d_out_moments or d_error is NULL"
                            : "cam, d_color, d_depth, d_object_id, d_out_color or d_out_len is NULL");
    const int n_hist = (a.hist_color != nullptr) + (a.hist_len != nullptr) + (a.hist_depth != nullptr) + (a.hist_object_id != nullptr) +
                       (a.var && a.hist_moments != nullptr);
    if (n_hist != 0 && n_hist != (a.var ? 5 : 4))
        return refuse(a.var ? "history: d_hist_color, d_hist_len, d_hist_moments, d_hist_depth and d_hist_object_id are all NULL or none is"
                            : "history: d_hist_color, d_hist_len, d_hist_depth and d_hist_object_id are all NULL or none is");
    if (n_hist && !a.hist_cam) return refuse("hist_cam is NULL with a history");
    if (!a.ctx) return refuse("ctx is NULL");
    int how = kMotionPlain;
    const int rc = check_reproject_motion(PT_OK, a.motion, a.n_motion, &how);
    if (rc) return rc;
    call = ReprojectCall{};
    call.var = a.var;
    call.weighted = a.var && a.spp;
    call.how = how;
    ReprojectFrame &f = call.v.f;
    f.width = a.width;
    f.height = a.height;
    f.color = a.color;
    f.depth = a.depth;
    f.normal = a.normal;
    f.object_id = a.object_id;
    f.hist_color = a.hist_color;
    f.hist_len = a.hist_len;
    f.hist_depth = a.hist_depth;
    f.hist_normal = n_hist ? a.hist_normal : nullptr;
    f.hist_object_id = a.hist_object_id;
    f.out_color = a.out_color;
    f.out_len = a.out_len;
    f.wt = (float)(P.weight ? P.weight : 1u);
    f.max_history = P.max_history != 0.0f ? P.max_history : kReprojectMaxHistory;
    f.depth_tol = P.depth_tol != 0.0f ? P.depth_tol : kReprojectDepthTol;
    f.normal_min = P.normal_min != 0.0f ? P.normal_min : kReprojectNormalMin;
    reproject_view(*a.cam, n_hist ? a.hist_cam : nullptr, f.view);
    if (!a.var) return PT_OK;
    call.v.hist_moments = reinterpret_cast<const ReprojectMom *>(a.hist_moments);
    call.v.out_moments = reinterpret_cast<ReprojectMom *>(a.out_moments);
    call.v.error = a.error;
    call.wts.spp = a.spp;
    call.wts.min_frames = (float)(P.min_frames ? P.min_frames : kReprojectVarMinFrames);
    call.v.long_len = call.wts.min_frames * f.wt;
    call.v.radius = P.radius ? P.radius : kReprojectVarRadius;
    return PT_OK;
}

// ---- pt_ctx_upsample (ptrace.h, pt_upsample.h)
int check_upsample(const void *ctx, uint32_t width, uint32_t height, uint32_t lo_width, uint32_t lo_height,
                   const pt_upsample_params *params, const float *d_lo_color, const float *d_lo_depth, const int32_t *d_lo_object_id,
                   const float *d_lo_normal, const float *d_lo_albedo, const float *d_depth, const int32_t *d_object_id,
                   const float *d_normal, const float *d_albedo, float *d_out_color, float *d_out_weight, UpsampleFrame &f) {
    pt_upsample_params P{};
    if (params) P = *params;
    if (!finite_nonneg(P.depth_tol)) return refuse("pt_upsample_params.depth_tol is negative or not finite");
    if (!(P.normal_min >= -1.0f && P.normal_min <= 1.0f)) return refuse("pt_upsample_params.normal_min is outside [-1, 1]");
    if (P.flags) return refuse("pt_upsample_params.flags: none is defined");
    if (!width || !height || !lo_width || !lo_height) return refuse("width, height, lo_width and lo_height must be positive");
    if (width > kUpsampleMaxSize || height > kUpsampleMaxSize || lo_width > kUpsampleMaxSize || lo_height > kUpsampleMaxSize)
        return refuse("width, height, lo_width or lo_height exceeds 2^14");
    if (!d_lo_color || !d_lo_depth || !d_lo_object_id || !d_depth || !d_object_id || !d_out_color)
        return refuse("d_lo_color, d_lo_depth, d_lo_object_id, d_depth, d_object_id or d_out_color is NULL");
    if (!ctx) return refuse("ctx is NULL");
    f = UpsampleFrame{};
    f.width = width;
    f.height = height;
    f.lo_width = lo_width;
    f.lo_height = lo_height;
    f.lo_color = d_lo_color;
    f.lo_depth = d_lo_depth;
    f.lo_object_id = d_lo_object_id;
    f.depth = d_depth;
    f.object_id = d_object_id;
    if (d_lo_normal && d_normal) f.lo_normal = d_lo_normal, f.normal = d_normal;  // a test of both or of neither
    if (d_lo_albedo && d_albedo) f.lo_albedo = d_lo_albedo, f.albedo = d_albedo;
    f.out_color = d_out_color;
    f.out_weight = d_out_weight;
    f.depth_tol = P.depth_tol != 0.0f ? P.depth_tol : kUpsampleDepthTol;
    f.normal_min = P.normal_min != 0.0f ? P.normal_min : kUpsampleNormalMin;
    f.div_w = upsample_div_make(width);
    f.div_2w = upsample_div_make(2u * width);
    f.div_2h = upsample_div_make(2u * height);
    return PT_OK;
}

// ---- pt_ctx_select_pixels, pt_ctx_render_masked (ptrace.h, pt_masked.h)
int check_select_pixels(const void *ctx, uint32_t width, uint32_t height, const pt_select_params *params, const float *d_weight,
                        const float *d_len, uint8_t *d_mask, SelectFrame &f) {
    pt_select_params P{};
    if (params) P = *params;
    if (P.weight_max != P.weight_max || P.len_max != P.len_max) return refuse("pt_select_params: weight_max or len_max is NaN");
    if (P.flags) return refuse("pt_select_params.flags: none is defined");
    if (!width || !height) return refuse("width and height must be positive");
    if ((uint64_t)width * height > (1ull << 28)) return refuse("width*height exceeds 2^28");
    if (!d_weight && !d_len) return refuse("d_weight and d_len are both NULL");
    if (!d_mask) return refuse("d_mask is NULL");
    if (!params) return refuse("params is NULL");
    if (!ctx) return refuse("ctx is NULL");
    f = SelectFrame{};
    f.npix = width * height;
    f.weight = d_weight;
    f.len = d_len;
    f.mask = d_mask;
    f.weight_max = P.weight_max;
    f.len_max = P.len_max;
    return PT_OK;
}

int check_spp_plane(const void *ctx, uint32_t width, uint32_t height, const uint32_t *d_spp) {
    if (!width || !height) return refuse("width and height must be positive");
    if ((uint64_t)width * height > (1ull << 28)) return refuse("width*height exceeds 2^28");
    if (!d_spp) return refuse("d_spp is NULL");
    if (!ctx) return refuse("ctx is NULL");
    return PT_OK;
}

int check_masked_cfg(const pt_config &cfg) {
    if (cfg.width != 0u && (cfg.idx_begin % cfg.width != 0u || cfg.idx_end % cfg.width != 0u))
        return refuse("masked: the band must consist of whole image rows");
    if (cfg.chunk_step > 1u || ((cfg.flags >> 8) & 15u) != 0u)
        return refuse("masked: chunk_step > 1 and PT_FLAG_PIPELINES are not supported");
    return PT_OK;
}

// ---- pt_ctx_scatter (ptrace.h, pt_probe.h)
void material_reflectance(const float color[3], float &max_refl, float &inv_max_refl) {
    max_refl = f_max(color[0], f_max(color[1], color[2]));  // mod.rs:668
    inv_max_refl = 1.0f / max_refl;                         // mod.rs:679
}

int check_scatter(const void *ctx, uint32_t form, const pt_scatter_item *items, const pt_scatter_surface *surfaces, uint32_t n,
                  const pt_scatter_out *out, std::vector<ScatterSurf> &given) {
    if (!items || !out) return refuse("items or out is NULL");
    if (n == 0u) return refuse("n is 0");
    const uint32_t src = form & kScatterSourceMask, mode = form & kScatterModeMask;
    if ((form & ~(kScatterSourceMask | kScatterModeMask)) || src == 3u || mode == kScatterModeMask)
        return refuse("form: unknown bits, source 3 or both mode flags");
    if (src == PT_SCATTER_GIVEN && !surfaces) return refuse("surfaces is NULL with PT_SCATTER_GIVEN");
    for (uint32_t i = 0; i < n; ++i)
        if (items[i].sample >= (1u << 24) || items[i].depth > 11u || items[i].branch < 1u || items[i].branch > 7u)
            return refuse("an item's sample >= 2^24, depth > 11 or branch outside 1..7");
    if (src == PT_SCATTER_GIVEN)
        for (uint32_t i = 0; i < n; ++i) {
            if (surfaces[i].reflect > PT_REFRACT) return refuse("a surface's reflect type is unknown");
            if (mode == PT_SCATTER_REFRACT_ONLY && surfaces[i].reflect != PT_REFRACT)
                return refuse("PT_SCATTER_REFRACT_ONLY with a surface that is not Refract");
        }
    if (!ctx) return refuse("ctx is NULL");
    given.clear();
    if (src != PT_SCATTER_GIVEN) return PT_OK;
    given.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        const pt_scatter_surface &s = surfaces[i];
        ScatterSurf &g = given[i];
        memcpy(g.x, s.x, sizeof g.x);
        memcpy(g.n, s.n, sizeof g.n);
        memcpy(g.color, s.color, sizeof g.color);
        memcpy(g.emission, s.emission, sizeof g.emission);
        material_reflectance(s.color, g.max_refl, g.inv_max_refl);
        g.reflect = s.reflect;
    }
    return PT_OK;
}

// ---- host-array queries (ptrace.h, pt_host.h)
int check_radiance(const void *ctx, bool has_scene, const float *o, const float *d, uint32_t depth, uint32_t n_samples, uint32_t backend,
                   uint32_t flags, const float *out_rgb) {
    if (!ctx || !o || !d || !out_rgb) return refuse("NULL argument");
    if (!has_scene) return refuse("no scene set");
    if (n_samples == 0u || n_samples > (1u << 24) || depth >= (uint32_t)kMaxDepth ||
        (backend != PT_BACKEND_WAVEFRONT && backend != PT_BACKEND_MEGAKERNEL) || ((flags >> 8) & 15u) > 1u)
        return refuse("n_samples outside 1..2^24, depth >= MAX_DEPTH, unknown backend, or PT_FLAG_PIPELINES (not offered for a one-ray call)");
    return PT_OK;
}

int check_primary_rays(const void *ctx, bool has_scene, uint32_t width, uint32_t height, uint64_t seed, const uint32_t *pixel,
                       const uint32_t *sample, uint32_t n, uint32_t form, const float *o, const float *d, pt_config &cfg,
                       uint32_t *idx_begin, uint32_t *idx_end) {
    if (!ctx || !pixel || !sample || !o || !d || n == 0 || form > 1u) return refuse("NULL argument, n == 0 or an unknown form");
    if (!has_scene) return refuse("no scene (the camera comes with it): call pt_ctx_set_scene first");
    cfg = pt_config{};
    cfg.width = width;
    cfg.height = height;
    cfg.spp = 1;
    cfg.seed = seed;
    const int rc = check_cfg(&cfg, idx_begin, idx_end);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i)
        if (pixel[i] >= (uint64_t)width * height || sample[i] >= (1u << 24))
            return refuse("pixel index outside the frame or sample >= 2^24");
    return PT_OK;
}

int check_bounds_query(const void *ctx, bool has_scene, uint32_t mode, uint32_t object, uint32_t n_objs, const float *o, const float *d) {
    if (!ctx || !o || !d) return refuse("NULL argument");
    if (!has_scene) return refuse("no scene set");
    if (mode == 0u && object >= n_objs) return refuse("object index out of range");
    return PT_OK;
}

void pack_ray_streams(const float *o, const float *d, uint32_t n, uint32_t cap, std::vector<char> &bytes, std::vector<uint32_t> &counts) {
    const uint32_t K = (n + cap - 1u) / cap;
    bytes.assign(queue_bytes(K, cap), 0);  // slice b: [od0: cap x 16][tp: cap x 16][od1: cap x 8]
    counts.resize(K);
    for (uint32_t i = 0; i < n; ++i) {
        char *slice = bytes.data() + (size_t)(i / cap) * cap * kRayBytes;
        const uint32_t j = i % cap;
        const float od0[4] = {o[3 * i], o[3 * i + 1], o[3 * i + 2], d[3 * i]}, od1[2] = {d[3 * i + 1], d[3 * i + 2]};
        memcpy(slice + (size_t)j * 16u, od0, sizeof od0);
        memcpy(slice + (size_t)cap * 32u + (size_t)j * 8u, od1, sizeof od1);
    }
    for (uint32_t b = 0; b < K; ++b) counts[b] = (n - b * cap) < cap ? (n - b * cap) : cap;
}

void unpack_stream_hits(const void *hits, uint32_t n, float *t, int32_t *id) {
    for (uint32_t i = 0; i < n; ++i) {
        memcpy(&t[i], (const char *)hits + (size_t)i * 8u, 4);
        memcpy(&id[i], (const char *)hits + (size_t)i * 8u + 4u, 4);
    }
}

}  // namespace host
}  // namespace pt
