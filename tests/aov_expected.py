"""Expected first-hit AOVs: the oracle's primary rays (orc_render with p_rr = 0 under the ray log) folded in numpy float32 exactly as
the contract of crt_render_aov says, and the GPU pass they are compared with."""
import numpy as np

import cudaraytracing_amd as crt
import util

NAMES = ("albedo", "normal", "depth", "coverage", "tri", "material")


def primary_rays(name, width, height, spp, crop=None, seed=0):
    """The oracle's primary rays of a render (crop of a width x height frame): (origins, directions, t, tri) as (pixels, spp, ...)
    arrays in pixel order, then sample order."""
    eye, iv, fov = util.camera(name)
    o, d, t, tri, (ch, cw) = util.primary_rays_of(util.oracle_scene(name), eye, iv, fov, util.task(name).light_sample_n, width, height, spp, crop, seed)
    p = cw * ch
    return o.reshape(p, spp, 3), d.reshape(p, spp, 3), t.reshape(p, spp), tri.reshape(p, spp), (ch, cw)


def expected_aov(name, width, height, spp, crop=None, seed=0):
    """The contract of include/crt.h, restated in numpy float32 on the oracle's primary rays."""
    _, _, t, tri, (ch, cw) = primary_rays(name, width, height, spp, crop, seed)
    return fold_aov(t, tri, ch, cw, util.oracle_scene(name).tris(), util.host_scene(name).triangles()["material"].astype(np.int32))


def expected_aov_of(osc, scene, view, light_sample_n, width, height, spp, seed=0):
    """The same for a scene of a test's own: osc and scene are its oracle and host forms, view = (eye, inverse view matrix, fov)."""
    _, _, t, tri, (ch, cw) = util.primary_rays_of(osc, *view, light_sample_n, width, height, spp, None, seed)
    return fold_aov(t.reshape(ch * cw, spp), tri.reshape(ch * cw, spp), ch, cw, osc.tris(), scene.triangles()["material"].astype(np.int32))


def fold_aov(t, tri, ch, cw, tris, mat):
    """The buffers from the primary rays' answers t, tri: (pixels, spp); tris: the oracle's triangles; mat: material index per triangle"""
    spp = tri.shape[1]
    p = tri.shape[0]
    a = np.zeros((p, 3), dtype=np.float32)
    nrm = np.zeros((p, 3), dtype=np.float32)
    d = np.zeros(p, dtype=np.float32)
    hits = np.zeros(p, dtype=np.int64)
    fs = np.float32(spp)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for k in range(spp):
            hit = tri[:, k] >= 0
            ti = np.where(hit, tri[:, k], 0)
            a = np.where(hit[:, None], a + tris["kd"][ti].astype(np.float32) / fs, a)
            nrm = np.where(hit[:, None], nrm + tris["normal"][ti].astype(np.float32) / fs, nrm)
            d = np.where(hit, d + t[:, k], d)
            hits += hit
        depth = np.where(hits > 0, d / hits.astype(np.float32), np.float32(0.0)).astype(np.float32)
    cov = (hits.astype(np.float32) / fs).astype(np.float32)
    tri0 = tri[:, 0]
    mat0 = np.where(tri0 >= 0, mat[np.maximum(tri0, 0)], -1).astype(np.int32)
    return {"albedo": a.reshape(ch, cw, 3), "normal": nrm.reshape(ch, cw, 3), "depth": depth.reshape(ch, cw),
            "coverage": cov.reshape(ch, cw), "tri": tri0.reshape(ch, cw), "material": mat0.reshape(ch, cw)}


def run_aov(r, name, spp, width=None, height=None, traversal=crt.TRAVERSAL_EXACT, seed=0):
    eye, iv, fov = util.camera(name)
    r.set_spp(spp)
    r.seed = seed
    r.traversal = traversal
    try:
        return r.run_view_aov(eye, iv, fov, width=width, height=height)
    finally:
        r.traversal = crt.TRAVERSAL_EXACT
        r.seed = 0
