"""`ptrace --preview F --hdr G --despike [T]`, end to end on the GPU: the PFM is what tests/despike_ref.py makes of the PFM the
same run writes without the switch, the line on stderr carries the reference's counts, and without the switch the program prints
what it printed before there was one - two runs of this tree are compared on everything the switch does not own."""
import os
import re
import subprocess

import numpy as np
import pytest

import despike_ref as ref
import gpudev
import ptlib
from despike_ref import F32

pytestmark = pytest.mark.gpu
CLI = os.path.join(ptlib.PKG, "ptrace")
SPP, RES_Y, SEED = 8, 24, 3
W, H = 36, 24
LINE = re.compile(r"^despike: (\d+) spikes, (\d+) non-finite of (\d+) pixels$", re.M)


def run_cli(tmp_path, name, *extra):
    r = subprocess.run([CLI, str(SPP), str(RES_Y), "cornell", "--root", ptlib.ROOT, "--seed", str(SEED), "--out", str(tmp_path / "out"),
                        "--no-ppm", "--preview", str(tmp_path / (name + ".ppm")), "--hdr", str(tmp_path / (name + ".pfm"))] + list(extra),
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r, np.ascontiguousarray(gpudev.pfm_to_framebuffer(gpudev.read_pfm(str(tmp_path / (name + ".pfm")))), dtype=F32)


def steady(text, name):
    """a run's output without what differs from run to run (the timings) and without the file names' stem"""
    keep = [ln for ln in text.splitlines() if "ms_total" not in ln and "despike:" not in ln]
    return "\n".join(keep).replace(name + ".", "X.")


def test_despike_writes_what_the_restatement_predicts(tmp_path):
    plain, hdr = run_cli(tmp_path, "plain")
    assert hdr.max() > 1 and "despike:" not in plain.stderr and "despike:" not in plain.stdout
    for name, extra, threshold in (("dflt", ["--despike"], 2.0), ("d1", ["--despike", "1"], 1.0)):
        run, got = run_cli(tmp_path, name, *extra)
        want, _, (pixels, spikes, nonfinite) = ref.despike(hdr, W, H, threshold=threshold)
        print(name, "spikes", spikes, "non-finite", nonfinite)
        assert spikes > 0 or name == "dflt"  # at a threshold of 1 this frame has pixels to clip (two already at rank 2 and floor 1)
        gpudev.same_bytes(got, want, "--hdr with --despike " + name)
        (m,) = LINE.findall(run.stderr)
        assert tuple(int(v) for v in m) == (spikes, nonfinite, pixels) and pixels == W * H
        # everything the switch does not own is what the run without it prints
        assert steady(run.stdout, name) == steady(plain.stdout, "plain")
        assert steady(run.stderr, name) == steady(plain.stderr, "plain")
    again, hdr2 = run_cli(tmp_path, "plain2")
    gpudev.same_bytes(hdr2, hdr, "two runs without the switch")
    assert steady(again.stdout, "plain2") == steady(plain.stdout, "plain") and steady(again.stderr, "plain2") == steady(plain.stderr, "plain")
    assert (tmp_path / "plain2.ppm").read_bytes() == (tmp_path / "plain.ppm").read_bytes()


def test_despike_under_orbit_reports_every_frame(tmp_path):
    """two frames of --orbit: a line per frame with the switch, none without, and the same files either way"""
    def orbit(*extra):
        r = subprocess.run([CLI, str(SPP), str(RES_Y), "cornell", "--root", ptlib.ROOT, "--seed", str(SEED), "--orbit", "2", "--preview",
                            str(tmp_path / "o.ppm")] + list(extra), cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return r

    plain = orbit()
    assert not LINE.findall(plain.stderr)
    run = orbit("--despike", "1")
    lines = LINE.findall(run.stderr)
    assert len(lines) == 2 and all(int(m[2]) == W * H and int(m[1]) == 0 and int(m[0]) <= W * H for m in lines), lines
    assert [ln for ln in run.stdout.splitlines() if ln.startswith("wrote")] == [ln for ln in plain.stdout.splitlines() if ln.startswith("wrote")]
    assert (tmp_path / "o-000.ppm").exists() and (tmp_path / "o-001.ppm").exists()


def test_despike_needs_a_preview_and_a_threshold_of_one_or_more(tmp_path):
    for extra in (["--despike"], ["--preview", "p.ppm", "--despike", "0.5"], ["--preview", "p.ppm", "--despike", "--trace-scale", "2"],
                  ["--preview", "p.ppm", "--despike", "--solid"]):
        r = subprocess.run([CLI, "4", "16", "cornell", "--root", ptlib.ROOT] + extra, cwd=str(tmp_path), capture_output=True, text=True)
        assert r.returncode == 1 and "--despike" in r.stderr, (extra, r.stderr)
