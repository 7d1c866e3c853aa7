"""host::plan_taper and host::taper_piece - how a k_pass_cand launch's last streams are cut into pieces (pt_host.h: "THE TAPER")
- on the CPU, as tests/test_host_logic.py checks plan_pass: a program of its own over the host code, host/taper_plan_check.cpp.

- COVERAGE: with workgroup n_whole + j being piece j % pieces of stream n_whole + j / pieces (the kernel's rule, restated here),
  every (stream, sample) of a pass lies in exactly one piece, the piece is not empty, shares differ by at most one and are
  contiguous - for K, samples, n_cut and pieces over small ranges: fewer samples than pieces, samples that pieces does not divide,
  every stream cut.
- ORDER: every workgroup of a piece comes after every whole stream's.
- the EXTRA BYTES: n_cut x (pieces - 1) more slices of the first container, and of the second when it holds parking areas.
- OFF: no streams to cut; fewer than kTaperMinRounds rounds of resident workgroups; fewer samples than pieces; the budget; 32-bit
  slot indices; a PROBE instance.  Knobs set by hand lift the two rules that are about speed, not the others.
- plan_pass's outputs for the bench frame and for the budget frame of the GPU suite are what tests/test_host_logic.py pins,
  whether a taper is planned on them or not (plan_taper takes the plan by const reference; its inputs are not plan_pass's)."""
import ptlib


def test_taper_plan():
    out = ptlib.host_program("taper_plan_check")().strip()
    assert out == "OK", out
