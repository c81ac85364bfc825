"""The contracts of crt_pyramid_down and crt_pyramid_merge (include/crt.h) restated in numpy float32, operation by operation: every ufunc
below is one IEEE fp32 operation per element, every sum starts at +0.0f and runs in the contract's order, and a tap that is skipped adds
nothing.  tests/test_pyramid.py compares the device and the host-compiled kernel text with this, bit for bit."""
import numpy as np

F = np.float32


def low_size(w, h):
    return (w + 1) // 2, (h + 1) // 2


def _taps(plane):
    """[(values, taken)] of the four taps (2X, 2Y), (2X + 1, 2Y), (2X, 2Y + 1), (2X + 1, 2Y + 1) of every coarse pixel, in that order:
    values (H2, W2[, 3]) -- +0 where the tap lies outside the image --, taken (H2, W2[, 1]) bool"""
    plane = np.ascontiguousarray(plane, dtype=F)
    h, w = plane.shape[:2]
    w2, h2 = low_size(w, h)
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            v = np.zeros((h2, w2) + plane.shape[2:], dtype=F)
            taken = np.zeros((h2, w2) + (1,) * (plane.ndim - 2), dtype=bool)
            part = plane[dy::2, dx::2]
            v[:part.shape[0], :part.shape[1]] = part
            taken[:part.shape[0], :part.shape[1]] = True
            out.append((v, taken))
    return out


def down_plane(plane, kind="mean"):
    """One plane of crt_pyramid_down: kind "mean" (color, albedo, normal), "variance" or "depth" ((H, W), hits only)"""
    taps = _taps(plane)
    s = np.zeros_like(taps[0][0])
    n = np.zeros(taps[0][1].shape, dtype=F)
    with np.errstate(all="ignore"):
        for v, taken in taps:
            if kind == "depth":
                taken = taken & (v > F(0.0))          # (false for NaN)
            s = np.where(taken, s + v, s)
            n = np.where(taken, n + F(1.0), n)
        if kind == "depth":
            out = np.where(n > F(0.0), s / np.where(n > F(0.0), n, F(1.0)), F(0.0))
        elif kind == "variance":
            out = s / (n * n)
        else:
            out = s / n
    assert out.dtype == F
    return out


def down(color, variance=None, albedo=None, normal=None, depth=None):
    """crt_pyramid_down of the planes that are given, as a dict"""
    out = {"color": down_plane(color)}
    if variance is not None:
        out["variance"] = down_plane(variance, "variance")
    if albedo is not None:
        out["albedo"] = down_plane(albedo)
    if normal is not None:
        out["normal"] = down_plane(normal)
    if depth is not None:
        out["depth"] = down_plane(depth, "depth")
    return out


def _axis(n, n_low):
    """crt_upsample's lines along one axis at radius 1: (t0, u) -- the first tap's index and the position, per output pixel"""
    s = F(n_low) / F(n)
    u = (np.arange(n).astype(F) + F(0.5)) * s - F(0.5)
    assert u.dtype == F
    return np.floor(u).astype(np.int64), u


def merge(fine, coarse):
    """crt_pyramid_merge: out = fine + U(coarse - D(fine))"""
    fine, coarse = np.ascontiguousarray(fine, dtype=F), np.ascontiguousarray(coarse, dtype=F)
    h, w = fine.shape[:2]
    w2, h2 = low_size(w, h)
    assert coarse.shape == (h2, w2, 3)
    with np.errstate(all="ignore"):
        d = coarse - down_plane(fine)
        x0, u = _axis(w, w2)
        y0, v = _axis(h, h2)
        snum = np.zeros((h, w, 3), dtype=F)
        sden = np.zeros((h, w, 1), dtype=F)
        for oy in (0, 1):
            ty = y0 + oy
            wy = F(1.0) - np.abs(v - ty.astype(F)) / F(1.0)
            for ox in (0, 1):
                tx = x0 + ox
                wx = F(1.0) - np.abs(u - tx.astype(F)) / F(1.0)
                hw = (wy[:, None] * wx[None, :])[:, :, None]
                taken = (((ty >= 0) & (ty < h2))[:, None] & ((tx >= 0) & (tx < w2))[None, :])[:, :, None]
                q = d[np.clip(ty, 0, h2 - 1)[:, None], np.clip(tx, 0, w2 - 1)[None, :]]
                snum = np.where(taken, snum + q * hw, snum)
                sden = np.where(taken, sden + hw, sden)
        out = fine + snum / sden
    assert out.dtype == F and d.dtype == F
    return out
