"""Host-side pieces of the device layout that can be checked without a GPU: the round-robin deal of pixels to ray
streams (pt_device.h: stream_pixel / stream_pixel_count / global_pixel) and the bookkeeping word.  The C++ side of each test is a
program under path-tracer-rust_amd/host/ (ptlib.host_program: built under AddressSanitizer and UBSan)."""
import os

import ptlib


def test_stream_deal_and_partition():
    assert ptlib.host_program("stream_deal_check")().strip() == "OK"


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


def test_flatten_tables_of_the_walk_queue():
    """flatten_scene's tables for k_pass_cand<.., BVH> on mesh.json and cornell.json: tri_rank inverts rank_id, the BVH mesh
    list holds the meshes with a BVH in visiting order, every triangle of such a mesh sits in exactly one leaf of at most
    kBvhLeafPairs records inside the mesh's record range, the advertised stack depth covers the tree, and the candidate
    records are exactly those of the meshes without a BVH."""
    tool = ptlib.host_program("flatten_tables_check")
    out = tool(ptlib.scene_path("mesh"), ptlib.ROOT).split()
    assert out[0] == "OK" and out[1] == "1" and int(out[2]) > int(out[3]) >= 5  # one BVH mesh; stack deeper than the tree
    out = tool(ptlib.scene_path("cornell"), ptlib.ROOT).split()
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


def test_flat_filter_sign_rule_needs_well_shaped_triangles():
    """FlatPairRec.sign_exact (filter_flat drops rays that do not move towards the plane: the sign of Triangle::intersect's
    distance is then known exactly) is only set when the two edge products whose difference is the plane normal do not
    nearly cancel; a sliver keeps the conservative distance test.  cornell.json's walls all qualify."""
    tool = ptlib.host_program("sign_rule_probe")
    assert tool("0").split() == ["OK", "axis", "2", "sign_exact", "1"]
    assert tool("1").split() == ["OK", "axis", "2", "sign_exact", "0"]


def test_the_door_refuses_negative_and_non_finite_materials():
    """flatten_scene - what pt_ctx_set_scene, and through it pt_render and pt_render_multi, build a scene with - refuses a colour
    or emission component that is negative, NaN or infinite, naming the object and the field, and lets -0.0f, denormals and
    large finite values through: to_fixed (csrc/pt_device.h) is defined for finite values >= 0 only.  pt_ctx_set_object's
    refusals (check_object_edit) are in host/object_check.cpp."""
    import re
    assert ptlib.host_program("door_check")().split() == ["OK", "60"]
    h = open(os.path.join(ptlib.ROOT, "include", "ptrace.h")).read()
    assert "a component of color or emission that is negative or not finite" in re.sub(r"\s*\n \* ", " ", h)
    assert "SATURATES at 4294967040" in h and "WRAPS at 2^32 radiance units" in h


def test_pass_plan():
    """host::plan_pass - how a wavefront frame is cut into passes and streams; host::plan_frame follows its retries - on the CPU:
    the bench frame (six passes of 683 samples, stacks of 1024 slots per wave, nothing in the second container), mesh.json (parking areas), a frame of few
    samples (at most 64 pixels per stream), the memory budget (passes halved until the stacks fit), small stacks on request,
    tiny passes (smaller stacks), the level-by-level forms (slices of 4 slots per primary ray, two containers), and a pass
    that 32-bit slot indices cannot hold."""
    tool = ptlib.host_program("pass_plan_probe")

    def plan(npix, spp, want, default=1, stack=1, park=0, cand=1, bvh=0, streams=0, per_stream=0, wave_stack=0, n_cus=256, budget=0, groups=None,
             follow=False):
        # workgroups a CU holds, by hand: five for k_pass_cand without walks (its waves per SIMD when these figures were pinned).
        # follow: through host::plan_frame, which derives them and follows plan_pass's retries
        groups = 0 if follow else groups or (4 if bvh or not stack else 5)
        out = tool(npix, spp, want, default, stack, park, cand, bvh, streams, per_stream, wave_stack, n_cus, budget, groups).split()
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


def test_pass_length_follows_the_measured_rate():
    """host::next_pass_samples (render_wavefront / render_mega): the probe, the sixteen-fold growth limit, the plan's cap, equal
    passes stretched by at most a fifth, floors - the arithmetic behind "a cancel comes back within a tenth of a second"."""
    assert ptlib.host_program("pass_length_check")().strip() == "OK"


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
    ptlib.host_check("ckpt")  # its own run must pass
    tool = ptlib.host_program("ckpt_check")

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


def test_accumulate_schedule_is_the_deal():
    """host::accum_jobs and host::deal_to_a - what pt_ctx_accumulate renders and which half keep_job gives it to - against
    deal(), the header's rule as tests/test_gpu_noise.py restates it: the issue's sequence 0 -> 8 -> 24 -> 64, a part already at
    the target, an untracked frame, parts of 2^20 pixels, and the megakernel's whole-call job only when every part is even."""
    import numpy as np
    from test_gpu_noise import deal
    tool = ptlib.host_program("accum_schedule_probe")
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


def test_noise_target_decision():
    """host::noise_quantile_bin / noise_bin_upper / noise_target_met / noise_part_weight - pt_ctx_accumulate_until's decision
    and pt_ctx_accum_noise's weights - on hand-made histograms, against tests/noise_ref.py's restatement of the header."""
    import numpy as np
    import noise_ref
    tool = ptlib.host_program("noise_target_probe")
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


def test_rounds_schedules_and_tiles():
    """The host arithmetic of the megakernel's and the tile pass's rounds (host::plan_rounds / round_launch), the sample schedules
    of the calls that render to a noise target (tracked_split, next_target and the two first counts), and pt_ctx_render_adaptive's
    refusals, tile geometry and totals - on values worked by hand from their definitions."""
    tool = ptlib.host_program("rounds_probe")
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
    sched = ptlib.host_program("accum_schedule_probe")
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
