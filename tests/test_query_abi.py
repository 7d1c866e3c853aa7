"""The host side of the host-array queries (pt_ctx_radiance .. pt_ctx_scatter), without a device: `make query-check` - the validators
of csrc/pt_host.h and the packing of rays into ray streams, under AddressSanitizer and UBSan as a stand-alone program - builds and
exits 0.  The GPU side is tests/test_gpu_query_calls.py."""
import subprocess

import ptlib


def test_query_check_builds_and_passes(tmp_path):
    r = subprocess.run(["make", "-C", ptlib.PKG, "query-check", "B=" + str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "query_check: ok" in r.stdout
    assert "-fsanitize=address,undefined" in r.stdout and "--cuda-host-only" in r.stdout
