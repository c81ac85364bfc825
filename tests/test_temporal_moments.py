"""Variance from temporal moments (crt_temporal_moments / crt_variance_estimate and their device forms, include/crt.h; moments= of temporal
and temporal_device, variance_estimate, variance_estimate_device and Render.run_view_temporal(variance="moments") in Python; crt_cli
--temporal-variance).

The two contracts are restated in numpy float32.  crt_temporal_moments stands on temporal_clamp_restated.restated_clamped, which stays the
statement of everything the call shares with crt_temporal_clamped; the interpolated moments h1 / ws and h2 / ws are read out of
temporal_restated.restated by temporal_clamp_restated.history_colour with a moment plane in the place of the history colour, and only the two
blends are written here.  crt_variance_estimate is written out in full, with the oracle's det_expf.  The device results must match bit
for bit, counts included.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import oracle_lib as O
import temporal_clamp_restated as TC
import temporal_restated as T
import util
from frames import renders  # noqa: F401
from util import assert_bits

F = np.float32
INF = float("inf")
NAN = float("nan")
ESTIMATE_DEFAULTS = {"min_history": 4, "radius": 3, "sigma_normal": 0.5, "sigma_depth": 0.05, "of_mean": 0, "history_cap": 39.0}


def restated_moments(cur, cam, prev=None, pcam=None, prev_moments=None, clamp=None, depth_tolerance=0.05, normal_tolerance=0.5, alpha_min=0.05):
    """crt_temporal_moments in numpy float32.  prev_moments: dict(m1=, m2=) of the history (None iff prev is None); clamp: None or
    (radius, gamma).  Returns restated_clamped's five -- (color, variance or None, history, took, clamped) -- and (m1, m2)."""
    out_c, out_v, out_h, took, clamped = TC.restated_clamped(cur, cam, prev, pcam, clamp=clamp, depth_tolerance=depth_tolerance,
                                                             normal_tolerance=normal_tolerance, alpha_min=alpha_min)
    color = np.ascontiguousarray(cur["color"], dtype=F)
    with np.errstate(all="ignore"):
        cc = color * color
        if prev is None:
            assert prev_moments is None
            return out_c, out_v, out_h, took, clamped, color.copy(), cc
        h1 = TC.history_colour(cur, cam, dict(prev, color=np.ascontiguousarray(prev_moments["m1"], dtype=F)), pcam, depth_tolerance, normal_tolerance)
        h2 = TC.history_colour(cur, cam, dict(prev, color=np.ascontiguousarray(prev_moments["m2"], dtype=F)), pcam, depth_tolerance, normal_tolerance)
        a = F(1) / out_h                                    # out_history = n where the history was taken
        a = np.where(a < F(alpha_min), F(alpha_min), a)
        k = F(1) - a
        m1 = np.where(took[..., None], h1 * k[..., None] + color * a[..., None], color)
        m2 = np.where(took[..., None], h2 * k[..., None] + cc * a[..., None], cc)
    assert m1.dtype == F and m2.dtype == F
    return out_c, out_v, out_h, took, clamped, m1, m2


def restated_estimate(m1, m2, history, normal=None, depth=None, min_history=4, radius=3, sigma_normal=0.5, sigma_depth=0.05, of_mean=0,
                      history_cap=39.0):
    """crt_variance_estimate in numpy float32: every ufunc is one IEEE fp32 operation per element, sums in tap order (dy outer, dx
    inner).  Returns (variance, the mask of the pixels of the spatial branch)."""
    m1, m2, n = (np.ascontiguousarray(a, dtype=F) for a in (m1, m2, history))
    h, w = n.shape
    fm, sn, sd, cap = F(min_history), F(sigma_normal), F(sigma_depth), F(history_cap)
    zero = np.zeros((h, w), dtype=F)
    if normal is not None:
        normal = np.ascontiguousarray(normal, dtype=F)
    if depth is not None:
        depth = np.ascontiguousarray(depth, dtype=F)
    with np.errstate(all="ignore"):
        e = m2 - m1 * m1
        e = np.where(e < F(0), F(0), e)
        s1, s2, sw = np.zeros((h, w, 3), dtype=F), np.zeros((h, w, 3), dtype=F), np.zeros((h, w), dtype=F)
        for dy in range(-radius, radius + 1):
            yq = np.arange(h) + dy
            ys = np.clip(yq, 0, h - 1)
            for dx in range(-radius, radius + 1):
                xq = np.arange(w) + dx
                xs = np.clip(xq, 0, w - 1)
                valid = ((yq >= 0) & (yq < h))[:, None] & ((xq >= 0) & (xq < w))[None, :]
                if normal is not None:
                    d = normal - normal[ys][:, xs]
                    e_n = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) / (sn * sn)
                else:
                    e_n = zero
                if depth is not None:
                    dq = depth[ys][:, xs]
                    m = np.where(depth > dq, depth, dq)
                    r = (depth - dq) / (sd * m)
                    e_d = np.where(m > 0, r * r, F(0))
                else:
                    e_d = zero
                wgt = O.math_fn("exp", -(e_n + e_d))
                assert wgt.dtype == F
                s1 = np.where(valid[..., None], s1 + m1[ys][:, xs] * wgt[..., None], s1)
                s2 = np.where(valid[..., None], s2 + m2[ys][:, xs] * wgt[..., None], s2)
                sw = np.where(valid, sw + wgt, sw)
        mu = s1 / sw[..., None]
        es = s2 / sw[..., None] - mu * mu
        es = np.where(es < F(0), F(0), es)
        spatial = ~(n >= fm)
        var = np.where(spatial[..., None], es * (fm / n)[..., None], e)
        if of_mean:
            ne = np.where(n > cap, cap, n)
            var = var / ne[..., None]
    assert var.dtype == F
    return var, spatial


def scalar_estimate(m1, m2, history, normal, depth, x, y, ch, min_history, radius, sigma_normal, sigma_depth, of_mean, history_cap):
    """one pixel and one channel of the contract in numpy float32 scalars and plain loops, without the masks and clipped gathers above"""
    H, W = history.shape
    n, fm = history[y, x], F(min_history)
    exp = lambda v: O.math_fn("exp", np.array([v], dtype=F))[0]
    with np.errstate(all="ignore"):
        if n >= fm:
            e = m2[y, x, ch] - m1[y, x, ch] * m1[y, x, ch]
            var = F(0) if e < 0 else e
        else:
            s1, s2, sw = F(0), F(0), F(0)
            for dy in range(-radius, radius + 1):
                for dx in range(-radius, radius + 1):
                    qy, qx = y + dy, x + dx
                    if not (0 <= qy < H and 0 <= qx < W):
                        continue
                    d = normal[y, x] - normal[qy, qx]
                    e_n = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) / (F(sigma_normal) * F(sigma_normal))
                    m = depth[y, x] if depth[y, x] > depth[qy, qx] else depth[qy, qx]
                    r = (depth[y, x] - depth[qy, qx]) / (F(sigma_depth) * m)
                    e_d = r * r if m > 0 else F(0)
                    wgt = exp(-(e_n + e_d))
                    s1, s2, sw = s1 + m1[qy, qx, ch] * wgt, s2 + m2[qy, qx, ch] * wgt, sw + wgt
            mu = s1 / sw
            e = s2 / sw - mu * mu
            e = F(0) if e < 0 else e
            var = e * (fm / n)
        if of_mean:
            var = var / (F(history_cap) if n > F(history_cap) else n)
    return F(var)


def as_clamp(clamp):
    return None if clamp is None else {"radius": clamp[0], "gamma": clamp[1]}


def check_moments(cur, cam, prev, pcam, pm, clamp, where, **kw):
    """crt.temporal(moments=...) against the restatement, bit for bit, and -- colour, variance, history, RGB8, counts -- against
    crt_temporal_clamped's own bits on the same inputs; returns (rgb, color, variance, history, m1, m2, info, took, clamped)"""
    rgb, color, var, hist, m1, m2, info = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, return_info=True, clamp=as_clamp(clamp),
                                                       moments=pm if prev is not None else True, **kw)
    want_c, want_v, want_h, took, clamped, want_m1, want_m2 = restated_moments(cur, cam, prev, pcam, pm, clamp=clamp, **kw)
    assert_bits(color, want_c, where + ": colour")
    assert_bits(hist, want_h, where + ": history")
    assert_bits(m1, want_m1, where + ": m1")
    assert_bits(m2, want_m2, where + ": m2")
    if want_v is None:
        assert var is None
    else:
        assert_bits(var, want_v, where + ": variance")
    assert np.array_equal(rgb, O.tonemap(color)), where + ": rgb is not the tone map of the colour"
    assert info["reprojected"] == int(took.sum()), (where, info, int(took.sum()))
    assert info["clamped"] == int(clamped.sum()), (where, info, int(clamped.sum()))
    old = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, return_info=True, clamp=as_clamp(clamp), **kw)
    assert np.array_equal(rgb, old[0]), where
    assert_bits(color, old[1], where + ": colour against crt_temporal_clamped")
    assert_bits(hist, old[3], where + ": history against crt_temporal_clamped")
    if var is not None:
        assert_bits(var, old[2], where + ": variance against crt_temporal_clamped")
    assert info["reprojected"] == old[4]["reprojected"] and info["clamped"] == old[4].get("clamped", 0), where
    return rgb, color, var, hist, m1, m2, info, took, clamped


def check_estimate(m1, m2, hist, normal, depth, where, **kw):
    """crt.variance_estimate against the restatement, bit for bit, and its count; returns (variance, the mask of the spatial branch).
    of_mean is always given: the Python call's default is 1, the library's and the restatement's 0."""
    kw.setdefault("of_mean", 0)
    got, info = crt.variance_estimate(m1, m2, hist, normal=normal, depth=depth, return_info=True, **kw)
    want, spatial = restated_estimate(m1, m2, hist, normal=normal, depth=depth, **kw)
    assert_bits(got, want, where)
    assert info["spatial"] == int(spatial.sum()), (where, info, int(spatial.sum()))
    return got, spatial


def moment_planes_of(prev):
    """moment planes that go with a synthetic history: its colour as m1, colour^2 + variance as m2"""
    c = np.ascontiguousarray(prev["color"], dtype=F)
    return {"m1": c.copy(), "m2": (c * c + prev["variance"]).astype(F)}


# ------------------------------------------------------------------------------------------------------------------ CPU --

def static_chain(frames_colour, W, H, alpha_min=2.0 ** -20):
    """colour frames of a static camera on a plane (every pixel reprojects onto itself, to rounding), accumulated by the restatement"""
    cam, depth, _ = T.plane_setup(W, H, (0, 0, 0))
    prev = pm = out = None
    for c in frames_colour:
        cur = {"color": c.astype(F), "depth": depth.astype(F)}
        out = restated_moments(cur, cam, prev, cam if prev is not None else None, pm, alpha_min=alpha_min)
        prev, pm = T.as_history(cur, out[0], None, out[2]), {"m1": out[5], "m2": out[6]}
    return out


def test_restated_moments_of_constant_frames_have_no_variance():
    """Static camera, the running mean (alpha_min 2^-20, so a = 1 / n), frames that show one colour whose channels are powers of two:
    a product with a power of two is exact, so the interpolated moments are u and u^2 whatever the four weights are
    (sum(u b) = u sum(b)), and k + a rounds to 1 for every a (k = fl(1 - a) is within 2^-25 of 1 - a, and 1 is the nearest float of
    everything within 2^-25 of it), so u k + u a = u.  m2 - m1^2 is then exactly +0 after any number of frames, and so is the estimate."""
    W, H = 16, 12
    u = np.array([0.5, 2.0, 8.0], dtype=F)
    for frames in (1, 2, 3, 8):
        out = static_chain([np.broadcast_to(u, (H, W, 3))] * frames, W, H)
        took, hist, m1, m2 = out[3], out[2], out[5], out[6]
        assert took.all() == (frames > 1) and (np.abs(hist - frames) < 1e-4).all()
        assert_bits(m1, np.broadcast_to(u, (H, W, 3)), "m1 after %d frames" % frames)
        assert_bits(m2, np.broadcast_to(u * u, (H, W, 3)), "m2 after %d frames" % frames)
        for of_mean in (0, 1):
            var, spatial = restated_estimate(m1, m2, hist, min_history=1, of_mean=of_mean)
            assert not spatial.any()
            assert_bits(var, np.zeros((H, W, 3), dtype=F), "variance after %d frames" % frames)
            var, spatial = restated_estimate(m1, m2, hist, min_history=1000, radius=2, of_mean=of_mean)   # the same through the window
            assert spatial.all()
            assert_bits(var, np.zeros((H, W, 3), dtype=F), "spatial variance after %d frames" % frames)


def test_restated_moments_of_two_frames_are_their_mean_and_their_spread():
    """Static camera, two frames: u (one colour, powers of two, so the history interpolates exactly: see above) and then w, any value
    per pixel.  n = 1 + 1 = 2 and a = k = 0.5 exactly, so with eps = 2^-24 (half an ulp, relative)
        m1 = fl(u / 2 + w / 2)              = M (1 + d1),               M = (u + w) / 2             one rounding, the products are exact
        m2 = fl(u^2 / 2 + fl(w^2) / 2)      = (u^2 + w^2 (1 + d2)) / 2 (1 + d3)                     two roundings
        var = fl(m2 - fl(m1 m1))            = (m2 - M^2 (1 + d1)^2 (1 + d4)) (1 + d5)               two roundings
    with every |d| <= eps.  Against V = ((u - w) / 2)^2 = (u^2 + w^2) / 2 - M^2 the error is therefore at most
        B = eps (w^2 / 2 + (u^2 + w^2) / 2 + 3 M^2)   from d2, d3 and (2 d1 + d4), to first order; x (1 + 4 eps) covers the higher orders
        |var - V| <= B (1 + 4 eps) + eps (V + B)      d5 on the difference itself."""
    W, H = 16, 12
    u = np.array([0.5, 2.0, 8.0], dtype=F)
    rng = np.random.default_rng(3)
    w = (rng.random((H, W, 3)) * 20).astype(F)
    out = static_chain([np.broadcast_to(u, (H, W, 3)), w], W, H)
    took, hist, m1, m2 = out[3], out[2], out[5], out[6]
    assert took.all() and (hist == F(2)).all()
    assert_bits(m1, (np.broadcast_to(u, (H, W, 3)) * F(0.5) + w * F(0.5)), "m1 = fl(u / 2 + w / 2)")
    u64, w64 = u.astype(np.float64), w.astype(np.float64)
    M, V = (u64 + w64) / 2, ((u64 - w64) / 2) ** 2
    assert (np.abs(m1 - M) <= 2.0 ** -24 * np.abs(M)).all()
    var, spatial = restated_estimate(m1, m2, hist, min_history=2)
    assert not spatial.any()
    eps = 2.0 ** -24
    B = eps * (w64 ** 2 / 2 + (u64 ** 2 + w64 ** 2) / 2 + 3 * M ** 2)
    bound = B * (1 + 4 * eps) + eps * (V + B)
    err = np.abs(var.astype(np.float64) - V)
    print("largest error / bound: %.3f; largest error in ulps of m2: %.2f" % ((err / bound).max(), (err / np.spacing(m2)).max()))
    assert (err <= bound).all() and V.max() > 50


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_restated_m1_is_the_unclamped_colour(seed):
    """With moment planes that go with the history (m1 = its colour), m1 has out_color's bits without a clamp -- the same taps, the same
    weights, the same blend -- and with a clamp that moves pixels it differs on exactly the pixels the clamp moved."""
    cur, cam, prev, pcam = T.synthetic(64, 48, seed)
    pm = moment_planes_of(prev)
    out = restated_moments(cur, cam, prev, pcam, pm)
    assert out[3].sum() >= 100 and not out[4].any()
    assert_bits(out[5], out[0], "m1 without a clamp")
    for clamp in ((1, 1.0), (2, 0.5), (3, 0.0)):
        color, _, _, took, clamped, m1, m2 = restated_moments(cur, cam, prev, pcam, pm, clamp=clamp)
        assert clamped.sum() >= 100
        differs = (color.view(np.uint32) != m1.view(np.uint32)).any(axis=2)
        assert np.array_equal(differs, clamped), (clamp, int(differs.sum()), int(clamped.sum()))
        assert_bits(m1, out[5], "m1 does not depend on the clamp")
        assert_bits(m2, out[6], "m2 does not depend on the clamp")
    # a reset pixel starts over: m1 = c, m2 = c * c
    reset = ~out[3]
    assert reset.sum() >= 100
    assert_bits(out[5][reset], cur["color"][reset], "m1 of reset pixels")
    assert_bits(out[6][reset], cur["color"][reset] * cur["color"][reset], "m2 of reset pixels")


def two_flat_sides(W=24, H=16):
    """left half m1 = 3, m2 = 13 (variance 4), right half m1 = 10, m2 = 101 (variance 1): small integers, so that every sum of the
    window is exact; the sides differ in normal and in depth"""
    left = np.zeros((H, W), dtype=bool)
    left[:, :W // 2] = True
    m1 = np.where(left[..., None], F(3), F(10)) * np.ones((H, W, 3), dtype=F)
    m2 = np.where(left[..., None], F(13), F(101)) * np.ones((H, W, 3), dtype=F)
    normal = np.where(left[..., None], np.array([0, 0, 1], dtype=F), np.array([1, 0, 0], dtype=F)).astype(F)
    depth = np.where(left, F(10), F(20)).astype(F)
    return left, m1.astype(F), m2.astype(F), normal, depth


def test_restated_spatial_estimate_on_flat_regions_and_across_a_step():
    """Equal normals and depths give e_n = e_d = +0 and w = exp(-0) = 1, so s1 = cnt m1, sw = cnt, mu = m1 and the estimate is
    (m2 - m1^2) fm / n, here exactly.  Across the step a tap has e_n = 2 / sigma_normal^2 or e_d = (0.5 / sigma_depth)^2: with small
    sigmas that is below -87, its weight is exactly 0 and the two sides do not mix; with the terms switched off they do."""
    left, m1, m2, normal, depth = two_flat_sides()
    H, W = left.shape
    hist = np.full((H, W), 2, dtype=F)
    hist[::3, ::2] = 1
    hist[1::3, 1::2] = 3
    assert float(O.math_fn("exp", np.array([-0.0], dtype=F))[0]) == 1.0 and float(O.math_fn("exp", np.array([-100.0], dtype=F))[0]) == 0.0
    e = np.where(left[..., None], F(4), F(1)) * np.ones((H, W, 3), dtype=F)
    for radius in (1, 2, 3):
        for guides in ({"normal": normal, "sigma_normal": 0.1}, {"depth": depth, "sigma_depth": 0.05}, {"normal": normal, "depth": depth}):
            var, spatial = restated_estimate(m1, m2, hist, min_history=4, radius=radius, **guides)
            assert spatial.all()
            assert_bits(var, e * (F(4) / hist)[..., None], "flat sides, radius %d, %r" % (radius, sorted(guides)))
            var1, _ = restated_estimate(m1, m2, hist, min_history=4, radius=radius, of_mean=1, **guides)
            assert_bits(var1, (e * (F(4) / hist)[..., None]) / hist[..., None], "flat sides of_mean, radius %d" % radius)
        mixed, _ = restated_estimate(m1, m2, hist, min_history=4, radius=radius, normal=normal, depth=depth, sigma_normal=INF, sigma_depth=INF)
        near = np.zeros((H, W), dtype=bool)
        near[:, W // 2 - radius:W // 2 + radius] = True
        assert_bits(mixed[~near], (e * (F(4) / hist)[..., None])[~near], "away from the step")
        assert (mixed[near] > (e * (F(4) / hist)[..., None])[near] * 2).all()       # (the two means are 7 apart: the window sees it)
    # one pixel at a time, in scalars: the vectorised statement on inputs that are not flat
    rng = np.random.default_rng(9)
    m1r = (rng.random((H, W, 3)) * 10).astype(F)
    m2r = (m1r * m1r + rng.random((H, W, 3)).astype(F) * 5).astype(F)
    nr = rng.normal(size=(H, W, 3)).astype(F)
    dr = (10 + rng.random((H, W))).astype(F)
    hr = rng.integers(1, 8, (H, W)).astype(F)
    for of_mean in (0, 1):
        kw = dict(min_history=4, radius=2, sigma_normal=2.0, sigma_depth=0.5, of_mean=of_mean, history_cap=5.0)
        var, spatial = restated_estimate(m1r, m2r, hr, normal=nr, depth=dr, **kw)
        assert spatial.sum() >= 50 and (~spatial).sum() >= 50
        for y, x in ((0, 0), (0, W - 1), (H - 1, 3), (5, 7), (6, 7), (7, 12), (H - 1, W - 1), (3, 0), (8, 8), (9, 20)):
            for ch in range(3):
                want = scalar_estimate(m1r, m2r, hr, nr, dr, x, y, ch, **kw)
                assert var[y, x, ch].view(np.uint32) == want.view(np.uint32), (y, x, ch, var[y, x, ch], want)


def test_moments_entry_points_and_defaults():
    lib = capi.lib()
    for name in ("crt_temporal_moments", "crt_temporal_moments_device", "crt_variance_estimate_defaults", "crt_variance_estimate",
                 "crt_variance_estimate_device"):
        assert name in capi.EXPORTS and getattr(lib, name)
    p = capi.VarianceEstimateParams()
    C.memset(C.byref(p), 0x7f, C.sizeof(p))
    assert lib.crt_variance_estimate_defaults(C.byref(p)) == capi.CRT_OK
    assert (p.width, p.height) == (0, 0)
    for name, v in ESTIMATE_DEFAULTS.items():
        assert F(getattr(p, name)) == F(v), name
    assert crt.variance_estimate_defaults() == {k: (float(F(v)) if isinstance(v, float) else v) for k, v in ESTIMATE_DEFAULTS.items()}
    assert lib.crt_variance_estimate_defaults(None) == capi.ERR_INVALID_ARG and lib.crt_last_error()
    assert lib.crt_abi_version() == 5
    assert C.sizeof(capi.TemporalMomentPlanes) == 16 and C.sizeof(capi.VarianceEstimateParams) == 32
    assert C.sizeof(capi.VarianceEstimateInputs) == 40 and C.sizeof(capi.VarianceEstimateInfo) == 16
    import inspect
    for f in (crt.temporal, crt.temporal_device):
        assert inspect.signature(f).parameters["moments"].default is None
    assert inspect.signature(crt.Render.run_view_temporal).parameters["variance"].default == "samples"
    for name in ("variance_estimate", "variance_estimate_device", "variance_estimate_defaults"):
        assert hasattr(crt, name)
    from cudaraytracing_amd import api
    assert api.ESTIMATE_OF_MEAN == 1                        # docs/experiments.md, "Variance from temporal moments": the rows that decided it
    assert api._estimate_params(8, 8, {}).of_mean == 1 and api._estimate_params(8, 8, {"of_mean": 0}).of_mean == 0
    frame = {"color": np.zeros((4, 4, 3), F), "depth": np.zeros((4, 4), F)}
    cam = (np.zeros(3), np.zeros(9), 1.0)
    for bad in (False, 1.0, {"m1": np.zeros((4, 4, 3), F)}, {"m1": np.zeros((4, 4, 3), F), "m2": np.zeros((4, 5, 3), F)}):
        with pytest.raises(ValueError):
            crt.temporal(frame, cam, prev=dict(frame, history=np.ones((4, 4), F)), prev_camera=cam, moments=bad)
    with pytest.raises(ValueError):          # planes without a history, and a history without planes
        crt.temporal(frame, cam, moments={"m1": np.zeros((4, 4, 3), F), "m2": np.zeros((4, 4, 3), F)})
    with pytest.raises(ValueError):
        crt.temporal(frame, cam, prev=dict(frame, history=np.ones((4, 4), F)), prev_camera=cam, moments=True)
    with pytest.raises(ValueError):
        crt.variance_estimate(np.zeros((4, 4, 3), F), np.zeros((4, 4, 3), F), np.ones((4, 4), F), sigma_color=1.0)
    with pytest.raises(ValueError):
        crt.variance_estimate(np.zeros((4, 4, 3), F), np.zeros((4, 5, 3), F), np.ones((4, 4), F))
    with pytest.raises(ValueError):
        crt.Render.run_view_temporal(None, None, None, None, variance="carried")
    with pytest.raises(NotImplementedError):
        crt.MultiRender.run_view_temporal(None, variance="moments")


def test_moments_arguments_are_checked_before_any_device_call():
    """Every invalid call of both forms of crt_temporal_moments returns its status also on a machine without a GPU.  The non-null
    buffers are dummies that must never be dereferenced."""
    lib = capi.lib()
    dummy = C.create_string_buffer(256)
    d = C.cast(dummy, C.c_void_p)

    def params(**over):
        p = capi.TemporalParams()
        assert lib.crt_temporal_defaults(C.byref(p)) == capi.CRT_OK
        p.width, p.height = 64, 48
        for k, v in over.items():
            setattr(p, k, v)
        return C.byref(p)

    def clamp(**over):
        c = capi.TemporalClamp()
        assert lib.crt_temporal_clamp_defaults(C.byref(c)) == capi.CRT_OK
        for k, v in over.items():
            setattr(c, k, v)
        return C.byref(c)

    def frame(**over):
        return C.byref(capi.TemporalFrame(**dict(dict(color=d, variance=d, depth=d, normal=d, id=d), **over)))

    def history(**over):
        return C.byref(capi.TemporalHistory(**dict(dict(color=d, variance=d, history=d, depth=d, normal=d, id=d), **over)))

    def planes(**over):
        return C.byref(capi.TemporalMomentPlanes(**dict(dict(m1=d, m2=d), **over)))

    AUTO = object()

    def both(prm, cl, cur, prev, pl=AUTO, color=d, var=d, hist=d, m1=d, m2=d, rgb=d, status=capi.ERR_INVALID_ARG, device=0):
        if pl is AUTO:
            pl = planes() if prev is not None else None
        r1 = lib.crt_temporal_moments(device, prm, cl, cur, prev, pl, color, var, hist, m1, m2, rgb, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_temporal_moments_device(device, prm, cl, cur, prev, pl, color, var, hist, m1, m2, rgb, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == status, (r1, r2, e1, e2)
        assert e1 and e2
        return e1

    for cl in (clamp(), clamp(gamma=INF), None):
        # the new ones
        for prev in (history(), None):
            assert b"out_m1" in both(params(), cl, frame(), prev, m1=None)
            assert b"out_m1" in both(params(), cl, frame(), prev, m2=None)
        assert b"go together" in both(params(), cl, frame(), history(), pl=None)
        assert b"go together" in both(params(), cl, frame(), None, pl=planes())
        assert b"m1 and m2" in both(params(), cl, frame(), history(), pl=planes(m1=None))
        assert b"m1 and m2" in both(params(), cl, frame(), history(), pl=planes(m2=None))
        # everything crt_temporal_clamped refuses
        assert b"null" in both(None, cl, frame(), history())
        assert b"null" in both(params(), cl, None, history())
        for prev in (history(), None):
            both(params(), cl, frame(color=None), prev)
            both(params(), cl, frame(depth=None), prev)
            both(params(), cl, frame(), prev, color=None)
            both(params(), cl, frame(), prev, hist=None)
            both(params(width=0), cl, frame(), prev)
            both(params(height=0), cl, frame(), prev)
            for name in ("depth_tolerance", "normal_tolerance"):
                for bad in (0.0, -1.0, NAN):
                    assert b"tolerance" in both(params(**{name: bad}), cl, frame(), prev), (name, bad)
            for bad in (0.0, 1.5, NAN):
                assert b"alpha_min" in both(params(alpha_min=bad), cl, frame(), prev), bad
            assert b"variance" in both(params(), cl, frame(variance=None), prev)
            assert b"variance" in both(params(), cl, frame(), prev, var=None)
        for missing in ("color", "history", "depth"):
            assert b"history" in both(params(), cl, frame(), history(**{missing: None})), missing
        assert b"variance" in both(params(), cl, frame(), history(variance=None))
        assert b"normals" in both(params(), cl, frame(normal=None), history())
        assert b"IDs" in both(params(), cl, frame(), history(id=None))
        both(params(width=(1 << 24) + 1), cl, frame(), history(), status=capi.ERR_UNSUPPORTED)
        both(params(width=1 << 24, height=1 << 24), cl, frame(), history(), status=capi.ERR_UNSUPPORTED)
        assert b"device index" in both(params(), cl, frame(), history(), device=-1)
        # neither variance: a valid call (one sample per pixel), the device index is what fails
        assert b"device index" in both(params(), cl, frame(variance=None), history(variance=None), var=None, device=-1)
    for prev in (history(), None):
        for radius in (0, 4, 2 ** 32 - 1):
            assert b"radius" in both(params(), clamp(radius=radius), frame(), prev), radius
        for gamma in (-1.0, NAN, -INF):
            assert b"gamma" in both(params(), clamp(gamma=gamma), frame(), prev), gamma


def test_estimate_arguments_are_checked_before_any_device_call():
    lib = capi.lib()
    dummy = C.create_string_buffer(256)
    d = C.cast(dummy, C.c_void_p)

    def params(**over):
        p = capi.VarianceEstimateParams()
        assert lib.crt_variance_estimate_defaults(C.byref(p)) == capi.CRT_OK
        p.width, p.height = 64, 48
        for k, v in over.items():
            setattr(p, k, v)
        return C.byref(p)

    def inputs(**over):
        return C.byref(capi.VarianceEstimateInputs(**dict(dict(m1=d, m2=d, history=d, normal=d, depth=d), **over)))

    def both(prm, inp, out=d, status=capi.ERR_INVALID_ARG, device=0):
        r1 = lib.crt_variance_estimate(device, prm, inp, out, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_variance_estimate_device(device, prm, inp, out, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == status, (r1, r2, e1, e2)
        assert e1 and e2
        return e1

    assert b"null" in both(None, inputs())
    assert b"null" in both(params(), None)
    assert b"output" in both(params(), inputs(), out=None)
    for missing in ("m1", "m2", "history"):
        assert b"required" in both(params(), inputs(**{missing: None})), missing
    both(params(width=0), inputs())
    both(params(height=0), inputs())
    assert b"min_history" in both(params(min_history=0), inputs())
    for radius in (0, 4, 2 ** 32 - 1):
        assert b"radius" in both(params(radius=radius), inputs()), radius
    for name in ("sigma_normal", "sigma_depth"):
        for bad in (0.0, -0.0, -1.0, NAN, -INF):
            assert b"sigma" in both(params(**{name: bad}), inputs()), (name, bad)
    for of_mean in (0, 1):
        for bad in (0.0, 0.5, -1.0, NAN, -INF):
            assert b"history_cap" in both(params(history_cap=bad, of_mean=of_mean), inputs()), bad
    both(params(width=(1 << 24) + 1), inputs(), status=capi.ERR_UNSUPPORTED)
    both(params(width=1 << 24, height=1 << 24), inputs(), status=capi.ERR_UNSUPPORTED)
    # valid calls: the guides are optional, +inf is allowed where the contract says so; the device index is what fails
    for ok in (params(), params(sigma_normal=INF, sigma_depth=INF), params(history_cap=INF, of_mean=1), params(history_cap=1.0),
               params(min_history=2 ** 32 - 1, radius=1)):
        for inp in (inputs(), inputs(normal=None), inputs(depth=None), inputs(normal=None, depth=None)):
            assert b"device index" in both(ok, inp, device=-1)


def test_cli_refuses_a_variance_source_without_a_sequence_or_with_a_malformed_value():
    from cudaraytracing_amd import build as b
    cli, cfg = b.build_cli(), util.SCENES["veach-mis"]
    for args in (["--temporal-variance", "moments"], ["--temporal-variance", "samples"], ["--temporal", "2", "--temporal-variance", "x"],
                 ["--temporal", "2", "--temporal-variance", "moments,0"], ["--temporal", "2", "--temporal-variance", "moments,"],
                 ["--temporal", "2", "--temporal-variance", "moments,-3"], ["--temporal", "2", "--temporal-variance", "moments,2x"],
                 ["--temporal", "2", "--temporal-variance", "moments,1,2"], ["--temporal", "2", "--temporal-variance", "samples,2"],
                 ["--temporal", "2", "--temporal-variance", "Moments"], ["--temporal", "2", "--temporal-variance"],
                 ["--temporal", "2", "--spp", "1", "--temporal-variance", "moments", "--temporal-denoise"]):          # (no --temporal-out)
        bad = subprocess.run([cli, cfg, "--base-dir", util.ROOT] + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "--temporal" in bad.stderr, (args, bad.stderr)
        if "--temporal-denoise" not in args and len(args) > 1:
            assert "--temporal-variance" in bad.stderr, (args, bad.stderr)


# ------------------------------------------------------------------------------------------------------------------ GPU --
# The frame of the rendered chains on which the estimate is checked, and its min_history, picked with the restatement on the CPU
# oracle's frames (the device's, bit for bit): with the library's clamp the last of the eight frames has 1012 (cornell-box) / 360
# (veach-mis) of its 3072 pixels in the spatial branch at min_history 4 -- background, newly seen and rejected pixels -- and the rest
# in the temporal one.  (At min_history 2 .. 5 the counts are 975 .. 1025 and 216 .. 390; frames 1 .. 3 have every pixel below 4.)
ESTIMATE_FRAME, ESTIMATE_MIN_HISTORY = 7, 4


def moments_chain(fr, variant, clamp, where, check=True, upto=None):
    """The frames of a moving camera accumulated by crt_temporal_moments, each output the next call's history; the last call's
    (cur, guides, results of check_moments or of crt.temporal)"""
    prev = pcam = pm = out = cur = g = None
    for f, (cur, _, g, cam) in enumerate(fr[:upto]):
        cur = T.subset(cur, variant)
        if check:
            out = check_moments(cur, cam, prev, pcam, pm, clamp, "%s frame %d" % (where, f))
        else:
            out = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, clamp=as_clamp(clamp), moments=pm if prev is not None else True)
        prev, pcam, pm = T.as_history(cur, out[1], out[2], out[3]), cam, {"m1": out[4], "m2": out[5]}
    return cur, g, out


def library_clamp():
    d = crt.temporal_clamp_defaults()
    return (d["radius"], d["gamma"])


@pytest.mark.gpu
@pytest.mark.parametrize("clamped", [False, True], ids=["no clamp", "clamp defaults"])
@pytest.mark.parametrize("variant", ["full", "no variance"])
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_moments_rendered_chains_match_restatement(renders, name, variant, clamped):
    """Eight chained frames of a moving camera (64 x 48, spp 4, seeds 100 .. 107): every output, the moments included, is the next
    frame's history.  After every frame colour, variance, history, m1, m2, RGB8 and both counts equal the restatement, and what the
    call shares with crt_temporal_clamped equals that call's own bits."""
    clamp = library_clamp() if clamped else None
    where = "%s 64x48 %s clamp %r" % (name, variant, clamp)
    fr = T.frames(renders, name, 64, 48, 8, 100)
    _, _, out = moments_chain(fr, variant, clamp, where)
    color, m1, took, moved = out[1], out[4], out[7], out[8]
    T.check_branches(T.subset(fr[-1][0], variant), took, where)
    differs = (color.view(np.uint32) != m1.view(np.uint32)).any(axis=2)
    if clamped:
        assert moved.sum() >= 100 and differs.sum() >= 100, where      # (m1 is not the clamped colour)
    else:
        assert not differs.any(), where                                 # clamp == NULL: the bits of out_m1 are the bits of out_color


_chains = {}


def chain_outputs(renders, name):
    """(guides, history, m1, m2) of frame ESTIMATE_FRAME of the chain with the library's clamp, made once per scene"""
    if name not in _chains:
        fr = T.frames(renders, name, 64, 48, 8, 100)
        _, g, out = moments_chain(fr, "full", library_clamp(), "", check=False, upto=ESTIMATE_FRAME + 1)
        _chains[name] = (g, out[3], out[4], out[5])
    return _chains[name]


@pytest.mark.gpu
@pytest.mark.parametrize("guides", [True, False], ids=["guides", "no guides"])
@pytest.mark.parametrize("of_mean", [0, 1])
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_estimate_on_rendered_chains_matches_restatement(renders, name, of_mean, guides):
    g, hist, m1, m2 = chain_outputs(renders, name)
    where = "%s estimate of_mean %d %s" % (name, of_mean, "guides" if guides else "no guides")
    var, spatial = check_estimate(m1, m2, hist, g["normal"] if guides else None, g["depth"] if guides else None, where,
                                  min_history=ESTIMATE_MIN_HISTORY, of_mean=of_mean)
    print("%s: %d pixels in the spatial branch, %d in the temporal one" % (where, spatial.sum(), (~spatial).sum()))
    assert spatial.sum() >= 100 and (~spatial).sum() >= 100, where
    assert np.isfinite(var).all() and (var >= 0).all() and (var > 0).sum() > var.size // 2


def synthetic_moments(w, h, seed):
    """temporal_restated.synthetic with moment planes for its history; on a frame too small for its blocks of misses, none"""
    cur, cam, prev, pcam = T.synthetic(w, h, seed)
    if w < 32 or h < 24:
        cur["depth"][:] = 40.0
        prev["depth"][:] = (F(40.0) * (F(0.97) + np.random.default_rng(seed).random((h, w)).astype(F) * F(0.06))).astype(F)
    return cur, cam, prev, pcam, moment_planes_of(prev)


def synthetic_estimate_inputs(w, h, seed, min_history=4):
    """moments, history lengths below, at and above min_history (whole numbers and fractions), normals and depths"""
    rng = np.random.default_rng(seed)
    cur = T.synthetic(w, h, seed)[0]
    m1 = (rng.random((h, w, 3)) * 100).astype(F)
    m2 = (m1 * m1 + (rng.random((h, w, 3)).astype(F) - F(0.1)) * F(300)).astype(F)        # (a tenth of them below m1^2: clamped at 0)
    hist = rng.integers(1, 2 * min_history + 1, (h, w)).astype(F)
    frac = rng.random((h, w)) < 0.3
    hist = np.where(frac, hist + rng.random((h, w)).astype(F), hist).astype(F)
    hist[0, :3] = [min_history - 1, min_history, min_history + 1]
    m2[0, 1] = 0.0                                                                          # (in the temporal branch, whatever the seed)
    depth = (cur["depth"] * (F(0.98) + rng.random((h, w)).astype(F) * F(0.04))).astype(F)   # (within the default sigma_depth, and the misses)
    return m1, m2, hist, cur["normal"], depth


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(130, 9), (61, 47), (5, 3)])
def test_moments_and_estimate_shapes_that_can_go_wrong(w, h):
    """130 x 9: three 64-wide blocks and three 4-row blocks, the last of each partial (two waves and two pixels per row), every window
    of radius 3 crossing a seam or a border; 61 x 47: one partial block across; 5 x 3: smaller than the 7 x 7 window on both axes."""
    cur, cam, prev, pcam, pm = synthetic_moments(w, h, 31)
    for clamp in (None, (3, 1.0), (1, 0.0)):
        for variant in ("full", "no variance"):
            where = "synthetic %dx%d clamp %r %s" % (w, h, clamp, variant)
            out = check_moments(T.subset(cur, variant), cam, T.subset(prev, variant), pcam, pm, clamp, where)
            took, moved = out[7], out[8]
            print("%s: %d took the history, %d clamped" % (where, took.sum(), moved.sum()))
            if w * h > 1000:
                assert took.sum() >= 100 and (~took).sum() >= 100, where
                if clamp is not None:
                    assert moved.sum() >= 50, where
            else:
                assert took.any(), where
    check_moments(cur, cam, None, None, None, (3, 1.0), "synthetic %dx%d, no history" % (w, h))
    m1, m2, hist, normal, depth = synthetic_estimate_inputs(w, h, 32)
    assert (hist < 4).any() and (hist == 4).any() and (hist > 4).any()
    for radius in (3, 1):
        for of_mean in (0, 1):
            for guides in ((normal, depth), (None, depth), (normal, None), (None, None)):
                where = "synthetic estimate %dx%d radius %d of_mean %d guides %r" % (w, h, radius, of_mean, [x is not None for x in guides])
                var, spatial = check_estimate(m1, m2, hist, guides[0], guides[1], where, radius=radius, of_mean=of_mean, history_cap=6.0)
                assert np.array_equal(spatial, hist < 4)
                assert (var == 0).any() and (var > 0).any()
    # every pixel in one branch: no wave enters the tap loop / every wave does
    _, spatial = check_estimate(m1, m2, hist, normal, depth, "all temporal", min_history=1)
    assert not spatial.any()
    _, spatial = check_estimate(m1, m2, hist, normal, depth, "all spatial", min_history=100, radius=2)
    assert spatial.all()


@pytest.mark.gpu
def test_moments_and_estimate_non_finite_values():
    """Non-finite values are not special-cased: NaN and +-inf in the history's moment planes and in the current colour go through the
    taps and the blends; in m1, m2, history (a NaN length takes the spatial branch), normal and depth through the estimate, with the
    terms on, off (sigma = +inf) and history_cap = +inf.  Bit for bit, NaN for NaN."""
    cur, cam, prev, pcam, pm = synthetic_moments(70, 45, 22)
    cur["color"][7, 9, 1] = np.inf
    cur["color"][30, 50, 0] = np.nan
    pm["m1"][12, 33, 2] = np.inf
    pm["m1"][25, 20, 0] = np.nan
    pm["m2"][26, 40, 1] = -np.inf
    pm["m2"][14, 35, 0] = np.nan
    prev["history"][20, 30] = np.inf
    for kw in ({}, {"depth_tolerance": INF, "normal_tolerance": INF}):
        for clamp in (None, (1, 1.0)):
            out = check_moments(cur, cam, prev, pcam, pm, clamp, "non-finite %r clamp %r" % (kw, clamp), **kw)
            assert np.isnan(out[4]).any() and np.isinf(out[4]).any() and np.isnan(out[5]).any() and np.isinf(out[5]).any()
            assert np.isfinite(out[4]).sum() > out[4].size // 2
    m1, m2, hist, normal, depth = synthetic_estimate_inputs(70, 45, 23)
    m1[5, 5, 0] = np.nan
    m1[6, 40, 1] = np.inf
    m1[30, 20, 2] = -np.inf
    m2[10, 10, 0] = np.nan
    m2[11, 50, 1] = np.inf
    m2[31, 21, 2] = -np.inf
    hist[3, 3] = np.nan
    hist[20, 20] = np.inf
    hist[21, 60] = -np.inf
    hist[40, 5] = 0.0
    hist[41, 6] = -2.0
    depth[8, 30] = np.nan
    depth[9, 31] = np.inf
    depth[25, 8] = -np.inf
    normal[12, 44, 1] = np.nan
    normal[13, 45, 0] = np.inf
    normal[33, 33, 2] = -np.inf
    for kw in ({}, {"sigma_normal": INF, "sigma_depth": INF}, {"of_mean": 1, "history_cap": INF}, {"of_mean": 1, "history_cap": 3.0, "radius": 1},
               {"sigma_depth": INF, "of_mean": 1}):
        var, spatial = check_estimate(m1, m2, hist, normal, depth, "non-finite estimate %r" % (kw,), **kw)
        assert spatial[3, 3] and not spatial[20, 20] and spatial[21, 60] and spatial[40, 5] and spatial[41, 6]
        assert np.isnan(var).any() and np.isfinite(var).sum() > var.size // 2
    check_estimate(m1, m2, hist, None, None, "non-finite estimate, no guides")


@pytest.mark.gpu
def test_moments_device_forms_on_a_stream_match_host_forms(renders):
    name, w, h = "veach-mis", 100, 70
    (c0, _, _, cam0), (c1, _, g1, cam1) = T.frames(renders, name, w, h, 2, 50)
    prev = T.as_history(c0, c0["color"], c0["variance"], np.full((h, w), 3, dtype=F))
    pm = moment_planes_of(prev)
    clamp = {"radius": 2, "gamma": 0.75}
    want_rgb, want_c, want_v, want_h, want_m1, want_m2, want_info = crt.temporal(c1, cam1, prev=prev, prev_camera=cam0, return_info=True, clamp=clamp,
                                                                                 moments=pm)
    assert 100 <= want_info["clamped"] < want_info["reprojected"] - 100
    est = dict(min_history=3, radius=2, of_mean=1, history_cap=3.5)
    want_e, want_einfo = crt.variance_estimate(want_m1, want_m2, want_h, normal=g1["normal"], depth=g1["depth"], return_info=True, **est)
    assert 100 <= want_einfo["spatial"] < w * h - 100
    host = {"cur_" + k: v for k, v in c1.items()}
    host.update({"prev_" + k: v for k, v in prev.items()})
    host.update({"prev_m1": pm["m1"], "prev_m2": pm["m2"]})
    outs = {"out_color": w * h * 12, "out_var": w * h * 12, "out_hist": w * h * 4, "out_rgb": w * h * 3, "out_m1": w * h * 12, "out_m2": w * h * 12,
            "out_est": w * h * 12}
    # (every output value must be written by the kernels: what is not uploaded is filled with 0x55)
    with DeviceBuffers({**host, **outs}, stream=True) as d:
        ptrs = d.ptrs

        def run(want_info, variance=True, out_rgb=True):
            cur_p = {k: ptrs["cur_" + k] for k in c1 if variance or k != "variance"}
            prev_p = {k: ptrs["prev_" + k] for k in prev if variance or k != "variance"}
            i1 = crt.temporal_device(w, h, cam1, cur_p, ptrs["out_color"], ptrs["out_hist"], out_variance_ptr=ptrs["out_var"] if variance else None,
                                     out_rgb_ptr=ptrs["out_rgb"] if out_rgb else None, prev_ptrs=prev_p, prev_camera=cam0, stream=d.stream,
                                     want_info=want_info, clamp=clamp,
                                     moments={"m1": ptrs["prev_m1"], "m2": ptrs["prev_m2"], "out_m1": ptrs["out_m1"], "out_m2": ptrs["out_m2"]})
            # the estimate reads what the call before it wrote, in stream order
            i2 = crt.variance_estimate_device(w, h, ptrs["out_m1"], ptrs["out_m2"], ptrs["out_hist"], ptrs["out_est"], normal_ptr=ptrs["cur_normal"],
                                              depth_ptr=ptrs["cur_depth"], stream=d.stream, want_info=want_info, **est)
            return i1, i2

        def fetch():
            return {n: d.download(n, size, np.uint8) if n == "out_rgb" else d.download(n, size // 4, F) for n, size in outs.items()}

        assert run(False) == (None, None)
        d.synchronize()
        got = fetch()
        for n, want in (("out_color", want_c), ("out_var", want_v), ("out_hist", want_h), ("out_m1", want_m1), ("out_m2", want_m2), ("out_est", want_e)):
            assert_bits(got[n].reshape(want.shape), want, "device form: " + n)
        assert np.array_equal(got["out_rgb"].reshape(h, w, 3), want_rgb)
        # without the variance pair and the RGB8, with the timers and the counts (each call synchronizes the stream)
        for n in outs:
            d.fill(n)
        i1, i2 = run(True, variance=False, out_rgb=False)
        assert i1["reprojected"] == want_info["reprojected"] and i1["clamped"] == want_info["clamped"] and i1["total_ms"] > 0, i1
        assert i2["spatial"] == want_einfo["spatial"] and i2["total_ms"] > 0, i2
        got = fetch()
        for n, want in (("out_color", want_c), ("out_hist", want_h), ("out_m1", want_m1), ("out_m2", want_m2), ("out_est", want_e)):
            assert_bits(got[n].reshape(want.shape), want, "device form, colour only: " + n)
        assert (got["out_rgb"] == 0x55).all() and (got["out_var"].view(np.uint32) == 0x55555555).all()


def render_frame_without_variance(r, cam, width, height, spp, seed):
    """A GPU render WITHOUT the variance flag (one sample per pixel has no per-sample variance) and its AOV pass"""
    return T.render_frame(r, cam, width, height, spp, seed, want_variance=False)


def by_hand_at_spp1(renders, name, w, h, n, seed0, clamp=None, **estimate):
    """n frames at one sample per pixel through the calls one by one: per frame (noisy rgb, rgb, colour, history, info, estimate, its
    info, guides)"""
    out, prev, pcam, pm = [], None, None, None
    for f in range(n):
        cam = T.camera_at(name, f)
        cur, noisy, g = render_frame_without_variance(renders[name], cam, w, h, 1, seed0 + f)
        rgb, color, var, hist, m1, m2, info = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, return_info=True, clamp=clamp,
                                                           moments=pm if prev is not None else True)
        assert var is None
        e, einfo = crt.variance_estimate(m1, m2, hist, normal=g["normal"], depth=g["depth"], return_info=True, **estimate)
        prev, pcam, pm = T.as_history(cur, color, None, hist), cam, {"m1": m1, "m2": m2}
        out.append((noisy, rgb, color, hist, info, e, einfo, g))
    return out


@pytest.mark.gpu
def test_run_view_temporal_with_moments_at_one_sample_per_pixel_equals_the_calls_by_hand(renders):
    name, w, h = "cornell-box", 64, 48
    r = renders[name]
    try:
        for clamp, estimate in ((None, {}), (True, {"min_history": 2, "of_mean": 0})):
            want = by_hand_at_spp1(renders, name, w, h, 3, 40, clamp=clamp, **estimate)
            r.set_spp(1)
            r.seed = 40
            r.reset_temporal()
            for f, (noisy, want_rgb, want_c, want_h, want_info, want_e, want_einfo, g) in enumerate(want):
                rgb, mean = r.run_view_temporal(*T.camera_at(name, f), width=w, height=h, variance="moments", denoise=(f == 2), clamp=clamp, **estimate)
                if f == 2:
                    want_rgb, want_mean = crt.denoise_var(want_c, want_e, **g)
                    assert r.denoise_info["passes"] == 3
                else:
                    want_mean = want_c
                assert_bits(mean, want_mean, "run_view_temporal(variance='moments') frame %d" % f)
                assert np.array_equal(rgb, want_rgb)
                assert_bits(r.variance_buffer, want_e, "variance_buffer")
                assert_bits(r.temporal_history_buffer, want_h, "temporal_history_buffer")
                assert r.temporal_info["reprojected"] == want_info["reprojected"] and r.temporal_info["clamped"] == want_info["clamped"]
                assert r.variance_estimate_info["spatial"] == want_einfo["spatial"] and r.seed == 40
                assert np.array_equal(r.frame_buffer, noisy)
            assert r.temporal_info["reprojected"] >= 100 and r.variance_estimate_info["spatial"] >= 100
            if estimate:                                     # (with min_history 4 every pixel of a third frame is in the spatial branch)
                assert r.variance_estimate_info["spatial"] <= w * h - 100
        # "samples" on the same object afterwards, by name (a change of `variance` starts a history; the seeds are given, since the
        # frames above count) and, after a reset, by default: the chain of plain crt.temporal calls, today's bits
        fr = T.frames(renders, name, w, h, 3, 40)
        r.set_spp(4)
        r.seed = 40
        for kw in ({"variance": "samples"}, {}):
            prev = pcam = None
            if not kw:
                r.reset_temporal()
            for f, (cur, noisy_rgb, g, cam) in enumerate(fr):
                if kw:
                    kw["seed"] = 40 + f
                want_rgb, want_c, want_v, want_h, want_info = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, return_info=True)
                prev, pcam = T.as_history(cur, want_c, want_v, want_h), cam
                rgb, mean = r.run_view_temporal(*cam, width=w, height=h, denoise=(f == 2), **kw)
                if f == 2:
                    want_rgb, want_c = crt.denoise_var(want_c, want_v, **g)
                assert_bits(mean, want_c, "run_view_temporal(%r) frame %d" % (kw, f))
                assert np.array_equal(rgb, want_rgb)
                assert_bits(r.variance_buffer, want_v, "variance_buffer")
                assert r.temporal_info["reprojected"] == want_info["reprojected"] and "clamped" not in r.temporal_info
    finally:
        r.seed = 0
        r.reset_temporal()


@pytest.mark.gpu
def test_cli_accumulates_a_sequence_at_one_sample_per_pixel(renders, tmp_path):
    from PIL import Image
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    name, w, h = "cornell-box", 64, 48
    base = [cli, util.SCENES[name], "--spp", "1", "--width", str(w), "--height", str(h), "--seed", "40", "--base-dir", util.ROOT,
            "--temporal", "3", "--temporal-step", ",".join(repr(float(v)) for v in T.MOVES[name][0]), "--temporal-denoise"]
    last = str(tmp_path / "last.png")
    for arg, estimate in (("moments", {}), ("moments,2", {"min_history": 2})):
        den = str(tmp_path / ("den_%s.png" % arg))
        res = subprocess.run(base + ["-o", last, "--temporal-out", den, "--temporal-variance", arg], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        want = by_hand_at_spp1(renders, name, w, h, 3, 40, of_mean=1, **estimate)
        noisy, _, color, _, _, e, einfo, g = want[-1]
        assert np.array_equal(np.asarray(Image.open(last)), noisy)
        assert np.array_equal(np.asarray(Image.open(den)), crt.denoise_var(color, e, **g)[0]), arg
        assert "from their neighbourhood" in res.stdout and ("variance of %d pixels" % einfo["spatial"]) in res.stdout
    # the Python path with its own defaults writes the same image
    r = renders[name]
    r.set_spp(1)
    r.seed = 40
    try:
        r.reset_temporal()
        for f in range(3):
            rgb, _ = r.run_view_temporal(*T.camera_at(name, f), width=w, height=h, variance="moments", denoise=(f == 2), min_history=2)
        assert np.array_equal(np.asarray(Image.open(den)), rgb)
    finally:
        r.seed = 0
        r.reset_temporal()
