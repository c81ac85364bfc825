"""The contract of crt_render_aov_ao (include/crt.h) restated in numpy float32 on the oracle's pieces: its primary rays (orc_render under the
ray log), its draws (rng_draw with the purpose 4), its vector functions (fn: sample_hemisphere, normalized, bounce_dir, dot) and its closest
hit (OracleScene.intersect) for blocked().  Every ufunc is one IEEE fp32 operation per element."""
import numpy as np

import oracle_lib as O
import util

F = np.float32
NAMES = ("ao", "openness", "bent_normal")
RNG_AO = 4
EPSILON = F(0.00001)


def _fn(name, *cols):
    return O.fn(name, np.ascontiguousarray(np.concatenate(cols, axis=1), dtype=F)).view(F)


def samples(osc, eye, iv, fov, width, height, spp, ao_samples, max_distance, seed=0):
    """Per path (pixel order, then sample order) of the width x height frame of scene `osc`: the oracle's primary rays and, per (path, q),
    the restated direction, cosine and blocked flag of the occlusion ray; `vertex`: the paths that hit."""
    o, d, t, tri, _ = util.primary_rays_of(osc, eye, iv, fov, 1, width, height, spp, seed=seed)
    tris = osc.tris()
    n = o.shape[0]
    vertex = tri >= 0                                # every hit is a vertex, an emitter too
    ti = np.where(vertex, tri, 0)
    nrm = tris["normal"][ti].astype(F)
    with np.errstate(all="ignore"):
        pos = (o + t[:, None] * d).astype(F)
        dn = _fn("dot", d, nrm)[:, 0]
        nf = np.where((dn > 0)[:, None], -nrm, nrm).astype(F)   # (a NaN dot keeps n)
    pixel = np.repeat(np.arange(width * height, dtype=np.int64), spp)
    k = np.tile(np.arange(spp, dtype=np.int64), width * height)
    dirs = np.zeros((n, ao_samples, 3), dtype=F)
    w = np.zeros((n, ao_samples), dtype=F)
    blocked = np.zeros((n, ao_samples), dtype=bool)
    idx = np.nonzero(vertex)[0]
    tl = F(max_distance)
    for q in range(ao_samples):
        u = np.zeros((len(idx), 4), dtype=np.uint32)
        for r, p in enumerate(idx):
            u[r], _ = O.rng_draw(seed, int(pixel[p]), int(k[p]), 0, RNG_AO, q)
        rec = np.concatenate([nf[idx].view(np.uint32), u[:, 1:3]], axis=1)   # (N, word1, word2), as orc_fn takes the samplers' records
        hs = O.fn("sample_hemisphere", rec).view(F)
        dr = _fn("normalized", hs)
        assert (dr.view(np.uint32) == O.fn("bounce_dir", rec)).all()          # dir = bounce_dir(nf, r)
        with np.errstate(all="ignore"):
            wq = _fn("dot", dr, nf[idx])[:, 0]
            wq = np.where(wq > 0, wq, F(0)).astype(F)
        _, th, _ = osc.intersect(pos[idx], hs)   # (Ray normalises what it is given: hs becomes dr, the direction the query is handed)
        with np.errstate(all="ignore"):
            bl = (tl - th) > EPSILON
        assert wq.dtype == F and th.dtype == F
        dirs[idx, q] = dr
        w[idx, q] = wq
        blocked[idx, q] = bl
    return {"vertex": vertex, "tri": tri, "pos": pos, "nf": nf, "dir": dirs, "w": w, "blocked": blocked}


def fold(S, width, height, spp):
    """The three buffers, the per-pixel sums and counts, and the number of occlusion rays, from the per-ray values: from +0, in (k, q) order"""
    p = width * height
    n_q = S["w"].shape[1]
    vertex = S["vertex"].reshape(p, spp)
    w, bl, dr = S["w"].reshape(p, spp, n_q), S["blocked"].reshape(p, spp, n_q), S["dir"].reshape(p, spp, n_q, 3)
    A = np.zeros(p, dtype=F)
    V = np.zeros(p, dtype=F)
    b = np.zeros((p, 3), dtype=F)
    rays = np.zeros(p, dtype=np.int64)
    opened = np.zeros(p, dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(spp):
            for q in range(n_q):
                v = vertex[:, k]
                op = v & ~bl[:, k, q]
                A = np.where(v, A + w[:, k, q], A)
                V = np.where(op, V + w[:, k, q], V)
                b = np.where(op[:, None], b + dr[:, k, q], b)
                rays += v
                opened += op
        ao = np.where(A == 0, F(1), V / np.where(A == 0, F(1), A)).astype(F)
        openness = np.where(rays > 0, opened.astype(F) / np.maximum(rays, 1).astype(F), F(1)).astype(F)
        bent = np.where((opened > 0)[:, None], _fn("normalized", b), F(0)).astype(F)
    assert A.dtype == F and V.dtype == F and b.dtype == F
    return {"ao": ao.reshape(height, width), "openness": openness.reshape(height, width), "bent_normal": bent.reshape(height, width, 3),
            "A": A.reshape(height, width), "V": V.reshape(height, width), "b": b.reshape(height, width, 3), "rays_per_pixel": rays.reshape(height, width),
            "open_per_pixel": opened.reshape(height, width), "rays": int(rays.sum())}


def expected_of(osc, eye, iv, fov, width, height, spp, ao_samples, max_distance, seed=0):
    return fold(samples(osc, eye, iv, fov, width, height, spp, ao_samples, max_distance, seed), width, height, spp)


def expected(name, width, height, spp, ao_samples, max_distance, seed=0):
    """Of a shipped scene at its own camera"""
    eye, iv, fov = util.camera(name)
    return expected_of(util.oracle_scene(name), eye, iv, fov, width, height, spp, ao_samples, max_distance, seed)


def default_max_distance(osc):
    """crt_aov_ao_defaults' max_distance: a quarter of the diagonal of the root node's box, in double, rounded once"""
    root = osc.nodes()[osc.root]
    d = root["bb"].astype(np.float64) - root["aa"].astype(np.float64)
    return F(0.25 * np.sqrt((d * d).sum()))
