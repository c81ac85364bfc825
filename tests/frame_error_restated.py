"""The contracts of crt_frame_error and crt_render_until (include/crt.h) restated in numpy, one ufunc per IEEE operation, on the sums
of util.restated_sums: the criterion is variance_restated.variance_of_sums and the adaptive call's target, the two fp64 sums are added
in the contract's own order (tree_sum), the loop stops at the first check whose `above` is within max_above.
tests/test_frame_error.py checks the restatement on the CPU and the device against it."""
import numpy as np

from util import restated_sums
from variance_restated import variance_of_sums

F = np.float32
EDGES = tuple(np.ldexp(F(1.0), 2 * (j - 7)) for j in range(15))   # 4^(j - 7): exact powers of two, 2^-14 .. 2^14
FIELDS = ("samples_done", "spp", "pixels", "nan_pixels", "above", "hist", "sum_variance", "sum_mean")


def shard_slots_of(w, h, rank=0, world=1):
    """(j, i, valid) per pixel slot of shard `rank` of `world` of a w x h frame: slot s lies in tile (s // 64) * world + rank at
    (s % 8, s % 64 // 8); valid = the tile lies in the frame and the pixel in the tile's part of it"""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    nslots = (tx * ty + world - 1) // world * 64
    s = np.arange(nslots)
    tile, pix = (s // 64) * world + rank, s % 64
    i, j = (tile % tx) * 8 + pix % 8, (tile // tx) * 8 + pix // 8
    valid = (tile < tx * ty) & (i < w) & (j < h)
    return np.where(valid, j, 0), np.where(valid, i, 0), valid


def tree64(x):
    """The contract's step 2 on the last axis (64 long): for s = 32 .. 1, x[t] += x[t + s] for t < s; returns x[0]"""
    x = np.array(x, dtype=np.float64)
    assert x.shape[-1] == 64
    s = 32
    while s >= 1:
        x[..., :s] = x[..., :s] + x[..., s:2 * s]
        s //= 2
    return x[..., 0]


def tree_sum(values):
    """The fp64 sum of per-slot values (slot order) in the contract's order: blocks of 256 in groups of 64, the group tree,
    ((w0 + w1) + w2) + w3 per block, lane l of 64 adds partials l, l + 64, ... ascending from +0.0, the tree again"""
    v = np.asarray(values, dtype=np.float64)
    nb = max(1, (v.size + 255) // 256)
    x = np.zeros(nb * 256)
    x[:v.size] = v
    with np.errstate(all="ignore"):
        w = tree64(x.reshape(nb, 4, 64))
        P = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        rows = (nb + 63) // 64
        Pp = np.zeros(rows * 64)
        Pp[:nb] = P             # (a lane's sum starts at +0.0 and so never is -0.0: adding the +0.0 of a row it has no partial in changes nothing)
        lane = np.zeros(64)
        for r in range(rows):
            lane = lane + Pp[r * 64:(r + 1) * 64]
        return float(tree64(lane))


def criterion(c, q, S, n, threshold, mean_floor):
    """(v, tt, m) of the adaptive call's criterion per pixel from the sums c, q (..., 3) holding n of S samples"""
    thr, floor, fs, fn = F(threshold), F(mean_floor), F(S), F(n)
    with np.errstate(all="ignore"):
        r = fs / fn
        var = variance_of_sums(c, q, fn, r)
        p = c * r
        v = (var[..., 0] + var[..., 1]) + var[..., 2]
        m = (p[..., 0] + p[..., 1]) + p[..., 2]
        t = thr * (m + floor)
        tt = t * t
    for a in (v, m, tt):
        assert a.dtype == F
    return v, tt, m


def frame_error_of_sums(c, q, S, n, threshold, mean_floor, valid=None):
    """crt_frame_error_info as a dict from the sums per pixel slot (nslots, 3) and the slots' validity"""
    v, tt, m = criterion(c, q, S, n, threshold, mean_floor)
    valid = np.ones(v.shape, dtype=bool) if valid is None else valid
    with np.errstate(all="ignore"):
        nan = valid & (np.isnan(v) | np.isnan(tt))
        ok = valid & ~nan
        above = valid & ~(v <= tt)
        b = np.zeros(v.shape, dtype=np.int64)
        for e in EDGES:
            b += v > tt * e
    hist = [int((ok & (b == k)).sum()) for k in range(16)]
    return dict(samples_done=n, spp=S, pixels=int(valid.sum()), nan_pixels=int(nan.sum()), above=int(above.sum()), hist=hist,
                sum_variance=tree_sum(np.where(ok, v.astype(np.float64), 0.0)), sum_mean=tree_sum(np.where(ok, m.astype(np.float64), 0.0)))


def restated_frame_error(L, S, n, threshold, mean_floor, rank=0, world=1, sums=None):
    """crt_frame_error on the oracle's per-path radiance L (h, w, S, 3) after samples 0 .. n - 1, for shard `rank` of `world`"""
    c, q = restated_sums(L, S, n) if sums is None else sums
    j, i, valid = shard_slots_of(L.shape[1], L.shape[0], rank, world)
    return frame_error_of_sums(c[j, i], q[j, i], S, n, threshold, mean_floor, valid)


def restated_until(L, S, min_samples, step_samples, threshold, mean_floor, max_above, sample_begin=0, rank=0, world=1):
    """crt_render_until's loop: dict of samples_done, passes (ranges rendered), checks, above (per check), paths, last (the last summary)"""
    fs = F(S)
    c, q = restated_sums(L, S, sample_begin)
    have = sample_begin

    def advance(to):
        nonlocal c, q, have
        with np.errstate(all="ignore"):
            for k in range(have, to):
                x = L[:, :, k, :] / fs
                c = c + x
                q = q + x * x
        have = to

    n, passes, above = sample_begin, 0, []
    if n < min_samples:
        advance(min_samples)
        n, passes = min_samples, 1
    while True:
        E = restated_frame_error(L, S, n, threshold, mean_floor, rank, world, sums=(c, q))
        above.append(E["above"])
        if E["above"] <= max_above or n == S:
            break
        n += min(step_samples, S - n)
        advance(n)
        passes += 1
    return dict(samples_done=n, passes=passes, checks=len(above), above=above, paths=E["pixels"] * (n - sample_begin), last=E)
