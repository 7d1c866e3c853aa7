// door_check — the door of host::flatten_scene: colour and emission components that must be refused, with the object and the field
// named, and those that must pass.  Judges itself: prints OK and the number of refusals
// (tests/test_host_logic.py: test_the_door_refuses_negative_and_non_finite_materials).
#include "check_common.h"
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#include "../csrc/pt_host.h"
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
