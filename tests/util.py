"""Shared helpers for the test-suite (scene setup for both the product and the oracle, bit comparisons, the oracle's ray log, PFM files)."""
import ctypes as C
import functools
import os

import numpy as np

import cudaraytracing_amd as crt
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {"cornell-box": os.path.join(ROOT, "scenes", "cornell-box", "config.json"),
          "veach-mis": os.path.join(ROOT, "scenes", "veach-mis", "config.json")}


@functools.lru_cache(maxsize=None)
def task(name):
    return crt.Task(SCENES[name], base_dir=ROOT)


@functools.lru_cache(maxsize=None)
def host_scene(name):
    return crt.Scene.from_task(task(name))


@functools.lru_cache(maxsize=None)
def oracle_scene(name):
    t = task(name)
    return O.OracleScene(t.OBJ_paths, t.bvh_thresh_n)


def camera(name):
    t = task(name)
    return t.eye_pos, crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up), crt.fov_to_radians(t.fov_y)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def restated_sums(L, S, n):
    """c and q of the crt_variance contract (include/crt.h) after samples 0 .. n-1 of S, from the oracle's per-path radiance
    L (h, w, S, 3): every ufunc is one IEEE fp32 operation per element."""
    F = np.float32
    fs = F(S)
    c = np.zeros(L.shape[:2] + (3,), dtype=F)
    q = np.zeros_like(c)
    with np.errstate(all="ignore"):
        for k in range(n):
            x = L[:, :, k, :] / fs
            c = c + x
            q = q + x * x
    assert c.dtype == F and q.dtype == F
    return c, q


def assert_bits(got, want, where=""):
    """float32 arrays equal on their uint32 views; NaN matches NaN"""
    F = np.float32
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    nan = np.isnan(want)
    same = np.where(nan, np.isnan(got), got.view(np.uint32) == want.view(np.uint32))
    assert same.all(), "%s: %d of %d values differ (first at %r)" % (where, int((~same).sum()), same.size, tuple(np.argwhere(~same)[0]))


def assert_same(got, want, names, where=""):
    """The buffers `names` of the dicts got and want have one shape and type and the same bits (float32 on its uint32 view)"""
    for n in names:
        g, w = np.ascontiguousarray(got[n]), np.ascontiguousarray(want[n])
        assert g.shape == w.shape and g.dtype == w.dtype, (where, n, g.shape, w.shape, g.dtype, w.dtype)
        same = g.view(np.uint32) == w.view(np.uint32) if g.dtype == np.float32 else g == w
        assert same.all(), "%s %s: %d of %d values differ (first at %r)" % (where, n, int((~same).sum()), same.size, tuple(np.argwhere(~same)[0]))


def read_pfm(path):
    """((kind, dimensions, scale) header lines, array with row 0 = image top) of a little-endian PFM, read with numpy alone."""
    kind, dims, scale, body = open(path, "rb").read().split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    ch = {b"PF": 3, b"Pf": 1}[kind]
    assert float(scale) < 0
    a = np.frombuffer(body, dtype="<f4")
    assert a.size == w * h * ch
    return (kind, dims, scale), np.ascontiguousarray(a.reshape((h, w, ch) if ch == 3 else (h, w))[::-1])


def primary_rays_of(osc, eye, iv, fov, lsn, width, height, spp, crop=None, seed=0):
    """The oracle's primary rays of a render of scene `osc` (crop of a width x height frame), from its ray log: (origins, directions, t,
    tri) as (pixels x spp, ...) arrays in pixel order, then sample order, and (h, w)."""
    L = O.lib()
    L.orc_ray_log_begin.restype = None
    L.orc_ray_log_end.restype = C.c_uint64
    L.orc_ray_log_end.argtypes = [C.c_void_p, C.c_uint64]
    L.orc_ray_log_begin()
    osc.render(eye, iv, fov, width, height, spp, 0.0, lsn, seed=seed, crop=crop)
    n = int(L.orc_ray_log_end(None, 0))
    log = np.zeros((n, 10), dtype=np.float32)
    L.orc_ray_log_end(log.ctypes.data_as(C.c_void_p), n)
    eye32 = np.asarray(eye, dtype=np.float32)
    keep = np.isnan(log[:, 8]) & np.all(log[:, 0:3].view(np.uint32) == eye32.view(np.uint32), axis=1)
    prim = log[keep]
    cw, ch = (crop[2], crop[3]) if crop else (width, height)
    assert prim.shape[0] == cw * ch * spp
    # (pixel, sample) order: with p_rr = 0 each path is its camera ray and that vertex's next-event samples, so the camera rays are
    # the log's closest-hit rays from the eye, one path after the other
    return prim[:, 0:3].copy(), prim[:, 3:6].copy(), prim[:, 6].copy(), prim[:, 7].astype(np.int32), (ch, cw)


def random_rays(name, n, seed):
    """Rays from inside the scene bounds towards random directions plus camera-like rays."""
    rng = np.random.default_rng(seed)
    nodes = oracle_scene(name).nodes()
    root = nodes[oracle_scene(name).root]
    lo, hi = root["aa"], root["bb"]
    o = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    eye = np.asarray(task(name).eye_pos, dtype=np.float32)
    half = n // 2
    o[:half] = eye
    tgt = (lo + (hi - lo) * rng.random((half, 3))).astype(np.float32)
    d[:half] = tgt - eye
    # axis-parallel directions and directions with one zero component (inv_dir = +-inf, DeviceBVH.cuh:97-121
    # relies on IEEE inf/NaN semantics), some starting exactly on a box plane (0 * inf = NaN in the slab test)
    d[half:half + 6] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)
    k = min(n // 8, 256)
    z = d[half + 6:half + 6 + k]
    z[np.arange(k), rng.integers(0, 3, k)] = 0.0
    z[::3, rng.integers(0, 3)] = 0.0
    ob = o[half + 6:half + 6 + k]
    pick = nodes[rng.integers(0, len(nodes), k)]
    ax = rng.integers(0, 3, k)
    side = rng.integers(0, 2, k)
    ob[np.arange(k), ax] = np.where(side == 0, pick["aa"][np.arange(k), ax], pick["bb"][np.arange(k), ax])
    return o, d
