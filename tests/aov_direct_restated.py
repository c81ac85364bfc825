"""The contract of crt_render_aov_direct (include/crt.h) restated in numpy float32 on the oracle's pieces: its primary rays (orc_render at
p_rr = 0 under the ray log), its draws (rng_draw), its light triangles, its vector functions (fn: normalized, norm, dot) and its closest hit
(OracleScene.intersect) for blocked().  Every ufunc is one IEEE fp32 operation per element."""
import numpy as np

import oracle_lib as O
import util

F = np.float32
NAMES = ("direct", "unshadowed", "direct_variance", "visibility")
RNG_NEE = 2
EPSILON = F(0.00001)


def _fn(name, *cols):
    return O.fn(name, np.ascontiguousarray(np.concatenate(cols, axis=1), dtype=F)).view(F)


def samples(name, width, height, spp, lsn, seed=0):
    """Per path (pixel order, then sample order) of the width x height frame: the oracle's primary rays and per-path radiance L of a
    p_rr = 0 render, its ray log, and per (path, q) the restated contribution c, limit tl, ray (pos, dir handed to Ray), traced and
    blocked flags.  q runs over lights x lsn."""
    osc = util.oracle_scene(name)
    eye, iv, fov = util.camera(name)
    O.ray_log_begin()
    _, mean, L, _ = osc.render(eye, iv, fov, width, height, spp, 0.0, lsn, seed=seed, want_L=True)
    log = O.ray_log_end()
    prim = np.isnan(log[:, 8])
    assert int(prim.sum()) == width * height * spp
    o, d, t, tri = log[prim, 0:3], log[prim, 3:6], log[prim, 6], log[prim, 7].astype(np.int32)
    tris = osc.tris()
    n = o.shape[0]
    hit = tri >= 0
    ti = np.where(hit, tri, 0)
    vertex = hit & (tris["has_emit"][ti] == 0)   # a miss or an emitter contributes nothing
    with np.errstate(all="ignore"):
        pos = (o + t[:, None] * d).astype(F)
        f_r = (tris["kd"][ti].astype(F) / F(np.pi)).astype(F)
    nrm = tris["normal"][ti].astype(F)
    n_lights = osc.num_lights
    n_q = n_lights * lsn
    pixel = np.repeat(np.arange(width * height, dtype=np.int64), spp)
    k = np.tile(np.arange(spp, dtype=np.int64), width * height)
    c = np.zeros((n, n_q, 3), dtype=F)
    tl = np.zeros((n, n_q), dtype=F)
    dirs = np.zeros((n, n_q, 3), dtype=F)
    traced = np.zeros((n, n_q), dtype=bool)
    blocked = np.zeros((n, n_q), dtype=bool)
    idx = np.nonzero(vertex)[0]
    for q in range(n_q):
        li = q // lsn
        lt = osc.light_tris(li)
        u = np.zeros((len(idx), 4), dtype=np.uint32)
        uni = np.zeros((len(idx), 4), dtype=F)
        for r, p in enumerate(idx):
            u[r], uni[r] = O.rng_draw(seed, int(pixel[p]), int(k[p]), 0, RNG_NEE, q)
        T = lt[(u[:, 0].astype(np.uint64) % np.uint64(len(lt))).astype(np.int64)]
        with np.errstate(all="ignore"):
            alpha = uni[:, 1]
            beta = uni[:, 2] * (F(1) - alpha)
            gamma = F(1) - alpha - beta
            lpos = (alpha[:, None] * T["v1"] + beta[:, None] * T["v2"]) + gamma[:, None] * T["v3"]
            dist = (lpos - pos[idx]).astype(F)
            dr = _fn("normalized", dist)
            lim = dist[:, 0] / dr[:, 0]
            ln = _fn("norm", dist)[:, 0]
            t2 = ln * ln
            ct = _fn("dot", dr, nrm[idx])[:, 0]
            ct2 = -_fn("dot", dr, T["normal"].astype(F))[:, 0]
            ct = np.where(ct > 0, ct, F(0))
            ct2 = np.where(ct2 > 0, ct2, F(0))
            cq = T["ke"].astype(F) * f_r[idx]
            cq = cq * ct[:, None]
            cq = cq * ct2[:, None]
            cq = cq * T["area_of_obj"].astype(F)[:, None]
            cq = cq / t2[:, None]
            cq = cq / F(lsn)
        assert cq.dtype == F and lim.dtype == F and dist.dtype == F
        _, th, _ = osc.intersect(pos[idx], dr)   # (Ray normalises dr again, as Render.cuh's Ray back(pos, dir))
        with np.errstate(all="ignore"):
            bl = (lim - th) > EPSILON
        c[idx, q] = cq
        tl[idx, q] = lim
        dirs[idx, q] = dr
        traced[idx, q] = ~((cq[:, 0] == 0) & (cq[:, 1] == 0) & (cq[:, 2] == 0))
        blocked[idx, q] = bl
    return {"L": L.reshape(n, 3), "mean": mean, "log": log, "prim": prim, "tri": tri, "vertex": vertex, "pos": pos, "c": c, "tl": tl, "dir": dirs,
            "traced": traced, "blocked": blocked, "n_q": n_q, "tris": tris}


def sample_sums(S):
    """Ld_k and U_k of every path: from +0, in q order"""
    n, n_q = S["traced"].shape
    Ld = np.zeros((n, 3), dtype=F)
    U = np.zeros((n, 3), dtype=F)
    with np.errstate(all="ignore"):
        for q in range(n_q):
            tr = S["traced"][:, q]
            U = np.where(tr[:, None], U + S["c"][:, q], U)
            Ld = np.where((tr & ~S["blocked"][:, q])[:, None], Ld + S["c"][:, q], Ld)
    return Ld, U


def fold(S, width, height, spp):
    """The four buffers and the traced count from the per-path sums"""
    Ld, U = sample_sums(S)
    p = width * height
    Ld, U = Ld.reshape(p, spp, 3), U.reshape(p, spp, 3)
    fs = F(spp)
    c = np.zeros((p, 3), dtype=F)
    q = np.zeros((p, 3), dtype=F)
    u = np.zeros((p, 3), dtype=F)
    with np.errstate(all="ignore"):
        for k in range(spp):
            x = Ld[:, k] / fs
            c = c + x
            q = q + x * x
            u = u + U[:, k] / fs
        if spp > 1:
            d = fs * q - c * c
            d = np.where(d < 0, F(0), d)
            var = (F(1) * d) / (fs - F(1))
        else:
            var = np.zeros((p, 3), dtype=F)
        traced = S["traced"].reshape(p, -1).sum(axis=1)
        lit = (S["traced"] & ~S["blocked"]).reshape(p, -1).sum(axis=1)
        vis = np.where(traced > 0, lit.astype(F) / np.maximum(traced, 1).astype(F), F(1)).astype(F)
    assert c.dtype == F and q.dtype == F and var.dtype == F
    return {"direct": c.reshape(height, width, 3), "unshadowed": u.reshape(height, width, 3), "direct_variance": var.astype(F).reshape(height, width, 3),
            "visibility": vis.reshape(height, width), "traced": int(S["traced"].sum())}


def expected(name, width, height, spp, lsn, seed=0):
    return fold(samples(name, width, height, spp, lsn, seed), width, height, spp)
