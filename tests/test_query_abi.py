"""The host side of the host-array queries (pt_ctx_radiance .. pt_ctx_scatter), without a device: `make query-check` - the validators
of csrc/pt_host.h and the packing of rays into ray streams, under AddressSanitizer and UBSan as a stand-alone program - builds and
exits 0.  The GPU side is tests/test_gpu_query_calls.py."""
import ptlib


def test_query_check_builds_and_passes():
    ptlib.host_check("query")
