// pt_refit.h — the per-triangle arithmetic of the scene tables and the steps of a BVH refit (pt_ctx_set_object), stated once for
// the host (flatten_scene, host/object_check.cpp) and the device (pt_refit.hip).
//
// NUMERICS.  world_triangle is what flatten_scene has always computed per triangle, in the same order of operations.  Its
// square roots and divisions are written as the language's own (__builtin_sqrtf, `/`): on the host sqrtss / divss, on the
// device the compiler's correctly rounded expansions (-fhip-fp32-correctly-rounded-divide-sqrt, part of COMMON), which are IEEE
// on EVERY input - zero, denormal, infinite - unlike pt_math.h's f_rcp, which is proven on normal divisors only.  A zero-area
// triangle's normal is v * (1 / 0): infinities where v is not zero, NaN where it is.  The invalid operations 0 * inf and
// inf - inf give the default NaN, which x86 spells 0xffc00000 and the GPU 0x7fc00000: the device form rewrites a NaN
// component to the host's spelling, so tables refit on the device equal tables flattened on the host to the bit for every mesh
// of finite vertices (a NaN vertex keeps its payload on the host; no kernel reads the payload of a NaN).  min / max never see
// a zero of either sign from the two sides differently: every box bound has a positive pad subtracted or added first.
// The refit unit is not a hot loop of the frame: nothing here is tuned.
#pragma once

#include "../../include/ptrace.h"
#include "pt_device.h"

namespace pt {

PT_HD float refit_min(float a, float b) { return __builtin_fminf(a, b); }
PT_HD float refit_max(float a, float b) { return __builtin_fmaxf(a, b); }
PT_HD float refit_length(vec3 v) { return __builtin_sqrtf(dot(v, v)); }
PT_HD float refit_host_nan(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return x != x ? __uint_as_float(0xffc00000u) : x;
#else
    return x;
#endif
}

// One triangle of a mesh in world space: what a pair record, a shading record and a BVH leaf hold of it
struct WorldTri {
    vec3 a, e1, e2;  // tri.a + position, and the two edges from it (mod.rs:546-552, 560-561)
    vec3 nrm;        // va_vb.cross(va_vc).normalize() (mod.rs:605)
    vec3 lo, hi;     // its box, padded
    vec3 mid;        // the centre of the box before padding (the SAH build sorts by it)
};

// scene_R: the diagonal of the box B that bounds every ray origin (flatten_scene)
PT_HD WorldTri world_triangle(const pt_triangle &t, vec3 position, float scene_R) {
    WorldTri w;
    const vec3 a = mk(t.a[0], t.a[1], t.a[2]) + position;  // Triangle::transformed, mod.rs:546-552
    const vec3 b = mk(t.b[0], t.b[1], t.b[2]) + position;
    const vec3 c = mk(t.c[0], t.c[1], t.c[2]) + position;
    const vec3 e1 = b - a, e2 = c - a;  // mod.rs:560-561
    const vec3 n = cross(e1, e2);
    const vec3 nrm = n * (1.0f / refit_length(n));  // glam's normalize: v * (1 / length)
    w.a = a, w.e1 = e1, w.e2 = e2;
    w.nrm = mk(refit_host_nan(nrm.x), refit_host_nan(nrm.y), refit_host_nan(nrm.z));
    w.lo = mk(refit_min(a.x, refit_min(b.x, c.x)), refit_min(a.y, refit_min(b.y, c.y)), refit_min(a.z, refit_min(b.z, c.z)));
    w.hi = mk(refit_max(a.x, refit_max(b.x, c.x)), refit_max(a.y, refit_max(b.y, c.y)), refit_max(a.z, refit_max(b.z, c.z)));
    w.mid = (w.lo + w.hi) * 0.5f;
    // Padding = bound on how far from the exact triangle a hit accepted by the f32 Moller-Trumbore
    // arithmetic can lie.  With |det| >= 1e-4 (mod.rs:571), |tvec| <= R (scene diagonal), this
    // triangle's edges <= L and unit roundoff e = 2^-24, forward error analysis of mod.rs:560-589
    // gives |du|,|dv| <= e L (7L + 8R) / 1e-4 (the hit point moves by that times L) and
    // |dt| <= e L^2 (7 t + 8R) / 1e-4 with t <= R; 16 e L^2 (R+L) / 1e-4 covers each of the three,
    // so three times that (the 16 already holds a factor 2 of slack), plus the slab test's own roundoff.
    const float L = refit_max(refit_length(e1), refit_max(refit_length(e2), refit_length(c - b)));
    const float e = 5.9604645e-8f;
    const float pad = 3.0f * (16.0f * e * L * L * (scene_R + L) / 1e-4f) + 16.0f * e * (scene_R + L) + 1e-6f;
    w.lo = w.lo - mk(pad, pad, pad);
    w.hi = w.hi + mk(pad, pad, pad);
    return w;
}

// BvhBuilder::grow: a box grown by another
PT_HD void refit_grow(vec3 &lo, vec3 &hi, vec3 l, vec3 h) {
    lo = mk(refit_min(lo.x, l.x), refit_min(lo.y, l.y), refit_min(lo.z, l.z));
    hi = mk(refit_max(hi.x, h.x), refit_max(hi.y, h.y), refit_max(hi.z, h.z));
}

// ---- the refit plan of one mesh that has a BVH (host::build_refit_plan makes it from the tree flatten_scene built; the tree's
// topology - which records a leaf holds, which node is whose child - never changes under a translation, only its floats do)
constexpr uint32_t kRefitNone = 0xffffffffu;
// a leaf: pair records [first, first + count), whose box is child `slot` of binary node `parent` (kRefitNone: the leaf is the root)
struct RefitLeaf {
    uint32_t first, count, parent, slot;
};
// an inner node that is not the root: the union of its two child boxes is child `slot` of `parent`
struct RefitNode {
    uint32_t node, parent, slot;
};
// child j of four-wide node i (dst = 4 i + j) holds the box of child h of binary node n (src = 2 n + h): widen copies verbatim
struct RefitWide {
    uint32_t dst, src;
};
// the tables a refit writes, and the mesh it is for
struct RefitTables {
    TriPairRec *tri_pairs;
    TriShade *tri_shade;
    SurfRec *surf;
    BvhNode *nodes;
    BvhNode4 *nodes4;
    const uint32_t *tri_rank;
    const pt_triangle *local;  // the mesh's object-local triangles, [0, tri_count)
    uint32_t tri_offset;       // triangle id of local[0]
    float px, py, pz;          // the object's position
    float scene_R;
};

PT_HD void refit_store_box(BvhNode &n, uint32_t h, vec3 lo, vec3 hi) {
    n.lox[h] = lo.x, n.loy[h] = lo.y, n.loz[h] = lo.z;
    n.hix[h] = hi.x, n.hiy[h] = hi.y, n.hiz[h] = hi.z;
}

// STEP 1, per leaf: every half that holds a triangle gets its record, its shading normal and its surface normal from the
// object-local triangle the record's id names; the union of the padded boxes, grown in record order from the empty box as
// BvhBuilder::build grows it, goes to the parent's slot.  A filler half (kNoTri) is all zeros and stays.
PT_HD void refit_leaf(const RefitTables &T, const RefitLeaf &lf) {
    const float inf = __builtin_inff();
    vec3 lo = mk(inf, inf, inf), hi = mk(-inf, -inf, -inf);
    const vec3 position = mk(T.px, T.py, T.pz);
    for (uint32_t r = 0; r < lf.count; ++r) {
        TriPairRec &rec = T.tri_pairs[lf.first + r];
        for (uint32_t hf = 0; hf < 2u; ++hf) {
            const uint32_t id = rec.id[hf];
            if (id == kNoTri) continue;
            const WorldTri w = world_triangle(T.local[id - T.tri_offset], position, T.scene_R);
            rec.ax[hf] = w.a.x, rec.ay[hf] = w.a.y, rec.az[hf] = w.a.z;
            rec.e1x[hf] = w.e1.x, rec.e1y[hf] = w.e1.y, rec.e1z[hf] = w.e1.z;
            rec.e2x[hf] = w.e2.x, rec.e2y[hf] = w.e2.y, rec.e2z[hf] = w.e2.z;
            TriShade &s = T.tri_shade[id];
            s.nx = w.nrm.x, s.ny = w.nrm.y, s.nz = w.nrm.z;
            SurfRec &sr = T.surf[T.tri_rank[id]];
            sr.vx = w.nrm.x, sr.vy = w.nrm.y, sr.vz = w.nrm.z;
            refit_grow(lo, hi, w.lo, w.hi);
        }
    }
    if (lf.parent != kRefitNone) refit_store_box(T.nodes[lf.parent], lf.slot, lo, hi);
}

// STEP 2, per inner node, one height above the leaves after the other: the union of its two child boxes, grown from the empty
// box as BvhBuilder::build grows it, goes to its parent's slot
PT_HD void refit_node(BvhNode *nodes, const RefitNode &n) {
    const float inf = __builtin_inff();
    vec3 lo = mk(inf, inf, inf), hi = mk(-inf, -inf, -inf);
    const BvhNode &me = nodes[n.node];
    refit_grow(lo, hi, mk(me.lox[0], me.loy[0], me.loz[0]), mk(me.hix[0], me.hiy[0], me.hiz[0]));
    refit_grow(lo, hi, mk(me.lox[1], me.loy[1], me.loz[1]), mk(me.hix[1], me.hiy[1], me.hiz[1]));
    refit_store_box(nodes[n.parent], n.slot, lo, hi);
}

// STEP 3, per child slot of the four-wide nodes: the six floats of the binary node's half it was widened from
PT_HD void refit_wide(BvhNode4 *nodes4, const BvhNode *nodes, const RefitWide &w) {
    const BvhNode &s = nodes[w.src >> 1];
    const uint32_t h = w.src & 1u, j = w.dst & 3u;
    BvhNode4 &d = nodes4[w.dst >> 2];
    d.lox[j] = s.lox[h], d.loy[j] = s.loy[h], d.loz[j] = s.loz[h];
    d.hix[j] = s.hix[h], d.hiy[j] = s.hiy[h], d.hiz[j] = s.hiz[h];
}

// the material half of a surface record (flatten_scene fills every record through this; STEP 4 runs it per rank of a large mesh)
PT_HD void surf_material(SurfRec &sr, const MatRec &mm, bool triangle) {
    sr.kind = (triangle ? kSurfTriangle : 0u) | (mm.reflect & 3u) | ((mm.er != 0.0f || mm.eg != 0.0f || mm.eb != 0.0f) ? kSurfEmits : 0u);
    sr.cr = mm.cr, sr.cg = mm.cg, sr.cb = mm.cb, sr.max_refl = mm.max_refl;
    sr.er = mm.er, sr.eg = mm.eg, sr.eb = mm.eb, sr.inv_max_refl = mm.inv_max_refl;
}

#if defined(__HIPCC__)
// ---- the kernels (pt_refit.hip): one lane per item of the plan's device lists.  The node pass is one launch per height, on
// the host's lists: no lane ever waits for another workgroup.
void launch_refit_leaves(hipStream_t st, const RefitTables &T, const RefitLeaf *leaves, uint32_t n);
void launch_refit_nodes(hipStream_t st, BvhNode *nodes, const RefitNode *items, uint32_t n);
void launch_refit_wide(hipStream_t st, BvhNode4 *nodes4, const BvhNode *nodes, const RefitWide *items, uint32_t n);
// STEP 4, the materials of a large mesh: one lane per rank rewrites the material half of surf[0, n) (surf: the object's first rank)
void launch_refit_materials(hipStream_t st, SurfRec *surf, uint32_t n, const MatRec &mm);
#endif

}  // namespace pt
