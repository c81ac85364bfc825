"""The neighbourhood clamp of crt_temporal_clamped (include/crt.h) restated in numpy float32 on top of temporal_restated.restated, which
stays the statement of everything up to the blend: the interpolated history H = hc / ws is read out of it by a call whose blend is the
identity (see history_colour), and only the clamp's own lines are written here."""
import numpy as np

import cudaraytracing_amd as crt
import oracle_lib as O
import temporal_restated as T
from util import assert_bits

F = np.float32


def history_colour(cur, cam, prev, pcam, depth_tolerance, normal_tolerance):
    """H = hc / ws of the contract, from temporal_restated.restated itself: with a history length of 1e30 in every tap and alpha_min 0,
    n = 1e30, a = 1 / n = 1e-30 and k = 1 - a = 1 exactly, and with a current colour of -0.0 the blend H * k + color * a is
    H * 1 + (-0.0) = H for every H (NaN, infinities and both zeros included).  The taps that count depend on neither colour nor length."""
    shape = np.asarray(cur["color"]).shape
    c = {k: v for k, v in cur.items() if k != "variance"}
    c["color"] = np.full(shape, -0.0, dtype=F)
    p = {k: v for k, v in prev.items() if k != "variance"}
    p["history"] = np.full(shape[:2], 1e30, dtype=F)
    return T.restated(c, cam, p, pcam, depth_tolerance=depth_tolerance, normal_tolerance=normal_tolerance, alpha_min=0.0)[0]


def neighbourhood_box(color, radius, gamma):
    """(mu, lo, hi, cnt) of the contract: every ufunc is one IEEE fp32 operation per element, sums in tap order (dy outer, dx inner)"""
    H, W = color.shape[:2]
    g = F(gamma)
    yy, xx = np.mgrid[0:H, 0:W]
    s1, s2 = np.zeros((H, W, 3), dtype=F), np.zeros((H, W, 3), dtype=F)
    cnt = np.zeros((H, W), dtype=F)
    with np.errstate(all="ignore"):
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                ty, tx = yy + dy, xx + dx
                inside = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
                t = color[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)]
                s1 = np.where(inside[..., None], s1 + t, s1)
                s2 = np.where(inside[..., None], s2 + t * t, s2)
                cnt = np.where(inside, cnt + F(1), cnt)
        mu = s1 / cnt[..., None]
        e = s2 / cnt[..., None] - mu * mu
        e = np.where(e < F(0), F(0), e)
        w = g * np.sqrt(e)
        lo, hi = mu - w, mu + w
    assert lo.dtype == F and hi.dtype == F and cnt.dtype == F
    return mu, lo, hi, cnt


def restated_clamped(cur, cam, prev=None, pcam=None, clamp=None, depth_tolerance=0.05, normal_tolerance=0.5, alpha_min=0.05):
    """crt_temporal_clamped in numpy float32.  clamp: None or (radius, gamma).  Returns (color, variance or None, history, took, clamped):
    temporal_restated.restated's four and the mask of the pixels whose history the clamp moved."""
    out_c, out_v, out_h, took = T.restated(cur, cam, prev, pcam, depth_tolerance=depth_tolerance, normal_tolerance=normal_tolerance,
                                           alpha_min=alpha_min)
    clamped = np.zeros(took.shape, dtype=bool)
    if prev is None or clamp is None:
        return out_c, out_v, out_h, took, clamped
    radius, gamma = clamp
    color = np.ascontiguousarray(cur["color"], dtype=F)
    Hh = history_colour(cur, cam, prev, pcam, depth_tolerance, normal_tolerance)
    _, lo, hi, _ = neighbourhood_box(color, int(radius), gamma)
    with np.errstate(all="ignore"):
        a = F(1) / out_h                                    # out_history = n where the history was taken
        a = np.where(a < F(alpha_min), F(alpha_min), a)
        k = F(1) - a
        below = Hh < lo
        Hc = np.where(below, lo, Hh)
        above = Hc > hi
        Hc = np.where(above, hi, Hc)
        out_c = np.where(took[..., None], Hc * k[..., None] + color * a[..., None], color)
    assert out_c.dtype == F
    clamped = took & (below | above).any(axis=2)
    return out_c, out_v, out_h, took, clamped


def check_against_restatement(cur, cam, prev, pcam, clamp, where, **kw):
    """crt.temporal(clamp=...) against the restatement, bit for bit; returns (rgb, color, variance, history, info, took, clamped)"""
    rgb, color, var, hist, info = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, return_info=True,
                                               clamp={"radius": clamp[0], "gamma": clamp[1]}, **kw)
    want_c, want_v, want_h, took, clamped = restated_clamped(cur, cam, prev, pcam, clamp=clamp, **kw)
    assert_bits(color, want_c, where + ": colour")
    assert_bits(hist, want_h, where + ": history")
    if want_v is None:
        assert var is None
    else:
        assert_bits(var, want_v, where + ": variance")
    assert np.array_equal(rgb, O.tonemap(color)), where + ": rgb is not the tone map of the colour"
    assert info["reprojected"] == int(took.sum()), (where, info, int(took.sum()))
    assert info["clamped"] == int(clamped.sum()), (where, info, int(clamped.sum()))
    return rgb, color, var, hist, info, took, clamped


def chain(fr, variant, clamp, where, check=True):
    """The frames of a moving camera accumulated with the clamp, each output the next call's history; the last call's results"""
    prev = pcam = out = None
    for f, (cur, _, _, cam) in enumerate(fr):
        cur = T.subset(cur, variant)
        if check:
            out = check_against_restatement(cur, cam, prev, pcam, clamp, "%s frame %d" % (where, f))
        else:
            out = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, clamp=None if clamp is None else {"radius": clamp[0], "gamma": clamp[1]})
        prev, pcam = T.as_history(cur, out[1], out[2], out[3]), cam
    return out
