"""pt_ctx_render_aov_ex with PT_AOV_THROUGH_DELTA (include/ptrace.h) restated on the test side.

Every sample's chain is built from the oracle: the primary rays are pto_primary_ray's (test_gpu_aov.oracle_rays), every hit is
pto_intersect_batch's (ptlib.oracle_intersect: distance, object, hit point, normal), and the direction a mirror or glass hit
hands on is kats_scatter.scatter's - the independent restatement of radiance()'s step, asked at depth 0, branch 1, where no draw
decides anything: children[0] of a 'mirror' or a 'tir' step, children[1] (the transmitted ray) of a 'split'.  thr, L and the
normal's flip are numpy binary32; the sums and their means are test_gpu_aov's integer arithmetic.

follow() walks every ray to PT_AOV_MAX_CHAIN steps ONCE and keeps what each step saw; planes() and stats() then read off the
call's five planes, and what the chains did, for any max_chain up to that - a chain cut at a smaller cap is a prefix of the
recorded one.  Nothing here reads the product."""
import numpy as np

import kats_scatter
import ptlib
from test_gpu_aov import oracle_rays, resolve, to_fixed, to_fixed_signed

F32 = np.float32
MAX_CHAIN = ptlib.abi.PT_AOV_MAX_CHAIN
DEFAULT_CHAIN = 8
DIFFUSE = ptlib.abi.PT_DIFFUSE
_NO_DRAWS = (F32(0), F32(0), F32(0))  # depth 0: no roulette, both subtrees - scatter() reads none of them
MISS, SURFACE, CAP = 0, 1, 2  # how a chain ends: no hit, a diffuse surface, a delta surface after max_chain steps


def with_reflect(sc, reflect_of, sid=None):
    """a copy of the scene `sc` in which object i has reflect type reflect_of(i, object) (None: as it is)"""
    objs = []
    for i in range(sc.n_objs):
        o = ptlib.PtObject.from_buffer_copy(sc.objs[i])
        r = reflect_of(i, o)
        if r is not None:
            o.reflect_type = r
        objs.append(o)
    return ptlib.Scene(sid or sc.id, sc.cam, objs, [sc.tris[k] for k in range(sc.n_tris)])


def materials(sc):
    col = np.array([list(sc.objs[i].color) for i in range(sc.n_objs)], dtype=F32)
    emi = np.array([list(sc.objs[i].emission) for i in range(sc.n_objs)], dtype=F32)
    refl = np.array([sc.objs[i].reflect_type for i in range(sc.n_objs)], dtype=np.int64)
    return col, emi, refl


class Record:
    """steps[j]: the rays that reached step j (idx into the flattened (pixel, sample) array), and per such ray the direction it
    travelled, the oracle's t / object / normal, and the kind of scatter step it took from there ('' if none was taken)"""

    def __init__(self, sc, n, spp):
        self.sc, self.n, self.spp, self.steps, self.max_chain = sc, n, spp, [], 0


def follow(sc, o, d, max_chain=MAX_CHAIN):
    """o, d: (n, spp, 3) primary rays"""
    n, spp = o.shape[:2]
    col, emi, refl = materials(sc)
    rec = Record(sc, n, spp)
    rec.max_chain = max_chain
    idx = np.arange(n * spp)
    co, cd = np.ascontiguousarray(o.reshape(-1, 3)), np.ascontiguousarray(d.reshape(-1, 3))
    for j in range(max_chain + 1):
        t, oid, _, x, nr = ptlib.oracle_intersect(sc, co, cd)
        kind = np.zeros(len(idx), dtype="U6")
        rec.steps.append(dict(idx=idx, d=cd, t=t, oid=oid, nr=nr, kind=kind))
        delta = (oid >= 0) & (refl[np.maximum(oid, 0)] != DIFFUSE)
        sel = np.nonzero(delta)[0]
        if j == max_chain or len(sel) == 0:
            break
        nd = np.zeros((len(sel), 3), F32)
        for a, i in enumerate(sel):
            ob = oid[i]
            r = kats_scatter.scatter(cd[i], nr[i], col[ob], emi[ob], int(refl[ob]), 0, 1, _NO_DRAWS)
            assert r["kind"] in ("mirror", "tir", "split") and r["alive"], r["kind"]
            nd[a] = r["children"][1 if r["kind"] == "split" else 0][0]
            kind[i] = r["kind"]
        idx, co, cd = idx[sel], np.ascontiguousarray(x[sel]), nd
    return rec


def _walk(rec, cap):
    """per flattened ray: the albedo and normal terms, sample depth / id / chain, how it ended, and the steps it took"""
    assert 1 <= cap <= rec.max_chain, cap
    col, _, refl = materials(rec.sc)
    m = rec.n * rec.spp
    thr, L = np.ones((m, 3), F32), np.zeros(m, F32)
    alb, nl = np.zeros((m, 3), F32), np.zeros((m, 3), F32)
    depth, oid_out = np.full(m, np.inf, F32), np.full(m, -1, np.int32)
    chain, end = np.zeros(m, np.uint32), np.full(m, -1, np.int64)
    taken = {k: np.zeros(m, np.int64) for k in ("mirror", "tir", "split")}
    live = np.ones(m, bool)
    for j, st in enumerate(rec.steps[:cap + 1]):
        idx, oid, nr, d = st["idx"], st["oid"], st["nr"], st["d"]
        a = live[idx]
        hit = oid >= 0
        miss = a & ~hit
        chain[idx[miss]], end[idx[miss]] = j, MISS
        h = a & hit
        L[idx[h]] = L[idx[h]] + st["t"][h]  # one binary32 addition per hit, in chain order
        ob = np.maximum(oid, 0)
        diffuse = refl[ob] == DIFFUSE
        term = h & (diffuse | (j == cap))
        it = idx[term]
        alb[it] = thr[it] * col[ob[term]]
        # normal_towards_ray against the current ray: the oracle's vdot, (a.x*b.x + a.y*b.y) + a.z*b.z, in binary32
        dn = (nr[:, 0] * d[:, 0] + nr[:, 1] * d[:, 1]) + nr[:, 2] * d[:, 2]
        nl[it] = np.where((dn < 0)[:, None], nr, nr * F32(-1.0))[term]
        depth[it], oid_out[it], chain[it] = L[it], oid[term], j
        end[it] = np.where(diffuse[term], SURFACE, CAP)
        cont = h & ~term
        thr[idx[cont]] = thr[idx[cont]] * col[ob[cont]]
        for k in taken:
            taken[k][idx[cont & (st["kind"] == k)]] += 1
        assert (st["kind"][cont] != "").all()
        live[idx[miss | term]] = False
    assert not live.any()
    return alb, nl, depth, oid_out, chain, end, taken


def planes(rec, spp=None, cap=DEFAULT_CHAIN):
    """(albedo, normal, depth, object_id, chain) of the record's pixels over its first `spp` samples"""
    spp = spp or rec.spp
    alb, nl, depth, oid, chain, _, _ = _walk(rec, cap)
    sh = (rec.n, rec.spp)
    albedo = resolve(to_fixed(alb.reshape(sh + (3,))[:, :spp]).sum(axis=1, dtype=np.uint64), spp)
    normal = resolve(to_fixed_signed(nl.reshape(sh + (3,))[:, :spp]).sum(axis=1, dtype=np.int64), spp)
    return albedo, normal, depth.reshape(sh)[:, 0].copy(), oid.reshape(sh)[:, 0].copy(), chain.reshape(sh)[:, 0].copy()


def stats(rec, cap=DEFAULT_CHAIN, sample=0):
    """what the chains of one sample per pixel did: a dict of counts over the record's pixels"""
    _, _, _, _, chain, end, taken = _walk(rec, cap)
    pick = lambda a: a.reshape(rec.n, rec.spp)[:, sample]  # noqa: E731
    chain, end = pick(chain), pick(end)
    return dict(pixels=rec.n,
                delta_pixels=int((chain > 0).sum()),  # the first hit is a mirror or glass surface
                at_cap=int((end == CAP).sum()),
                on_surface_after_delta=int(((end == SURFACE) & (chain > 0)).sum()),
                miss_after_delta=int(((end == MISS) & (chain > 0)).sum()),
                lengths=sorted(int(v) for v in np.unique(chain)),
                max_length=int(chain.max()),
                mirror_steps=int(pick(taken["mirror"]).sum()),
                tir_steps=int(pick(taken["tir"]).sum()),
                transmissions=int(pick(taken["split"]).sum()))


def chain_record(sc, w, h, seed, pixels, spp, rays=None, max_chain=MAX_CHAIN):
    o, d = rays if rays is not None else oracle_rays(sc, w, h, seed, pixels, spp)
    return follow(sc, o[:, :spp], d[:, :spp], max_chain)
