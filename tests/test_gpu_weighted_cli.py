"""ptrace ... --orbit N --preview FILE.ppm --boost K: the pixels that find no history are traced again at K times the frame's
samples (pt_ctx_select_pixels, pt_ctx_render_masked) and the frame enters the loop with its true per-pixel counts
(pt_ctx_spp_plane, pt_ctx_reproject_var_weighted).  cornell at 64x48, three frames, K = 4."""
import os
import re
import subprocess

import pytest

import ptlib

pytestmark = pytest.mark.gpu

CLI = os.path.join(ptlib.PKG, "ptrace")
RES_Y, W = 48, 64
N = 3


def run(tmp_path, args):
    return subprocess.run([CLI, "2", str(RES_Y), "cornell", "--width", str(W), "--root", ptlib.ROOT, "--seed", "5"] + args,
                          cwd=str(tmp_path), capture_output=True, text=True, timeout=120)


def test_cli_boost(tmp_path):
    assert os.path.exists(CLI), "the CLI is built with the library"
    r = run(tmp_path, ["--orbit", str(N), "--preview", str(tmp_path / "boost.ppm"), "--boost", "4"])
    assert r.returncode == 0, r.stdout + r.stderr
    counts = [(int(a), int(b)) for a, b in re.findall(r"Boosted (\d+) of (\d+) pixels", r.stdout)]
    total = W * RES_Y
    assert len(counts) == N and all(t == total for _, t in counts), r.stdout
    assert counts[0][0] == total                         # the first frame has no history: every pixel is one frame old
    assert all(0 < n < total // 4 for n, _ in counts[1:]), counts    # then the disocclusions of a 2 degree step
    plain = run(tmp_path, ["--orbit", str(N), "--preview", str(tmp_path / "plain.ppm")])
    assert plain.returncode == 0 and "Boosted" not in plain.stdout, plain.stdout + plain.stderr
    boosted = [open(tmp_path / ("boost-%03d.ppm" % k), "rb").read() for k in range(N)]
    base = [open(tmp_path / ("plain-%03d.ppm" % k), "rb").read() for k in range(N)]
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("boost")) == ["boost-%03d.ppm" % k for k in range(N)]
    assert all(len(a) == len(b) for a, b in zip(boosted, base)) and boosted[0] != base[0] and boosted[2] != base[2]


def test_cli_boost_is_refused_without_orbit(tmp_path):
    r = run(tmp_path, ["--preview", str(tmp_path / "no.ppm"), "--boost", "4"])
    assert r.returncode == 1 and "--boost" in r.stderr and "--orbit" in r.stderr, (r.returncode, r.stderr)
    for bad in ("1", "0", "x", "65"):
        r = run(tmp_path, ["--orbit", "2", "--preview", str(tmp_path / "no.ppm"), "--boost", bad])
        assert r.returncode == 1 and "--boost" in r.stderr, (bad, r.returncode, r.stderr)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no")]
