"""No device needed: the case table of tests/test_gpu_streams.py against include/ptrace.h.  Every prototype of the header with a
`hip_stream` parameter has at least one case there, and every case names such a prototype - an entry point added later cannot go
without its stream test.  And the header states the contract those cases hold the calls to."""
import os
import re

import ptlib
import test_gpu_streams as gs

HEADER = open(os.path.join(ptlib.ROOT, "include", "ptrace.h")).read()


def stream_entry_points(text):
    """the functions whose parameter list names hip_stream, from the header without its comments"""
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = re.findall(r"\b(pt_\w+)\s*\(([^;{}]*)\)\s*;", code)
    return sorted(name for name, params in protos if re.search(r"\bhip_stream\b", params))


def test_the_parser_sees_a_prototype_behind_comments_and_line_breaks():
    text = """/* int pt_old(void *hip_stream); */
    int pt_a(pt_ctx *ctx, const float *d_in /* may be NULL */,
             void *hip_stream);
    int pt_b(pt_ctx *ctx, void *stream);
    typedef void (*pt_fn)(void *user, float fraction);
    int pt_c(void *hip_stream, pt_fn cb);"""
    assert stream_entry_points(text) == ["pt_a", "pt_c"]


def test_every_entry_point_with_a_stream_has_a_case():
    declared = stream_entry_points(HEADER)
    assert len(declared) >= 22 and "pt_ctx_render" in declared and "pt_comm_gather_frame" in declared, declared
    covered = sorted({entry for _id, entry, _family, _make in gs.CASES})
    assert covered == declared, "without a case: %s; cases of no prototype: %s" % (
        sorted(set(declared) - set(covered)), sorted(set(covered) - set(declared)))
    # and what the table says of itself: ids are unique, every family has its run on a blocking stream
    ids = [c[0] for c in gs.CASES]
    assert len(ids) == len(set(ids))
    assert {c[2] for c, s in gs.RUNS if s == "blocking"} == {c[2] for c in gs.CASES}
    for c in gs.CASES:
        assert sum(1 for r, s in gs.RUNS if r is c and s.startswith("nonblocking")) == 2, c[0]


def test_the_signatures_put_a_pointer_where_the_stream_goes():
    """abi.py types a stream c_void_p: a case passes the hipStream_t as it is"""
    from ctypes import c_void_p
    for name in stream_entry_points(HEADER):
        assert c_void_p in ptlib.abi.SIGNATURES[name][1], name


def test_the_header_states_the_contract():
    i = HEADER.index("`hip_stream` is a hipStream_t")
    para = " ".join(HEADER[i:HEADER.index("*/", i)].split())
    for phrase in ("NULL = the context's own stream", "ordered on that stream", "pending on it when the call is made",
                   "has completed when the call returns", "every entry point that takes a `hip_stream`"):
        assert phrase in para.replace(" * ", " "), phrase
