"""The contract of crt_denoise_regress (include/crt.h) restated in numpy, operation by operation: every ufunc below is one IEEE operation
per element in `dtype`.  With dtype float32 and the oracle's det_expf (oracle_lib.math_fn("exp")) the result is what the device must give
bit for bit; with dtype float64 (and numpy's exp) it is the same definition evaluated finer, for the properties of the definition itself.
Per window offset o the pair terms d_o(t) are an image, a row sum is that image added along x in the contract's order, and D is the row
sums added along y: the numbers a per-pixel evaluation adds, in its order (as tests/test_denoise_nlm.py restates crt_denoise_nlm).
Used by tests/test_denoise_regress.py."""
import numpy as np

NORMAL, ALBEDO, DEPTH, POSITION = 1, 2, 4, 8
ALL = 15
DEFAULTS = {"radius": 5, "patch": 1, "k": 0.6, "alpha": 1.0, "sigma_normal": 0.5, "sigma_albedo": 0.1, "sigma_depth": 0.05, "sigma_position": 2.0,
            "ridge": 0.4, "features": ALL}
K3 = (0.25, 0.5, 0.25)


def shifted(a, dy, dx):
    """(a at (y + dy, x + dx), whether that pixel is inside the image); outside: some value that the caller masks"""
    h, w = a.shape[:2]
    ys, xs = np.arange(h) + dy, np.arange(w) + dx
    inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
    return a[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)], inside


def features_of(features, albedo, normal, depth):
    """the mask the Python layer hands the library: None = the default mask less the guides that are not given"""
    if features is not None:
        return int(features)
    return ALL & ~((ALBEDO if albedo is None else 0) | (NORMAL if normal is None else 0) | (DEPTH if depth is None else 0))


def restated(color, variance, albedo=None, normal=None, depth=None, weight_color=None, weight_variance=None, radius=5, patch=1, k=0.6, alpha=1.0,
             sigma_normal=0.5, sigma_albedo=0.1, sigma_depth=0.05, sigma_position=2.0, ridge=0.4, features=None, dtype=np.float32, exp=None):
    """Returns (out_mean (H, W, 3), fell_back (H, W) bool, S (H, W), Z (H, W, 3)) in `dtype`.  Settings are float32 values whatever the
    dtype (what the params struct holds).  exp: the exponential for float32 (oracle_lib.math_fn("exp", .)); float64 uses numpy's."""
    T = dtype
    val = lambda x: T(np.float32(x))
    img = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32).astype(T)
    c, wc, wv = img(color), img(color if weight_color is None else weight_color), img(variance if weight_variance is None else weight_variance)
    albedo, normal, depth = img(albedo), img(normal), img(depth)
    mask = features_of(features, albedo, normal, depth)
    assert not (mask & NORMAL and normal is None) and not (mask & ALBEDO and albedo is None) and not (mask & DEPTH and depth is None)
    if T is np.float32:
        assert exp is not None
    else:
        exp = np.exp
    h, w = c.shape[:2]
    sn, sa, sd, al, rg = val(sigma_normal), val(sigma_albedo), val(sigma_depth), val(alpha), val(ridge)
    k2 = val(k) * val(k)
    pos_den = val(sigma_position) * T(radius)
    zero, one = np.zeros((h, w), dtype=T), np.ones((h, w), dtype=T)

    def sq3(a, b):
        d = a - b
        return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]

    with np.errstate(all="ignore"):
        v = (wv[..., 0] + wv[..., 1]) + wv[..., 2]
        gn, gd = zero.copy(), zero.copy()
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                vt, inside = shifted(v, dy, dx)
                kk = T(K3[dy + 1]) * T(K3[dx + 1])
                gn = np.where(inside, gn + kk * vt, gn)
                gd = np.where(inside, gd + kk, gd)
        g = gn / gd
        F = (3 if mask & NORMAL else 0) + (3 if mask & ALBEDO else 0) + (1 if mask & DEPTH else 0) + (2 if mask & POSITION else 0)
        A = [[zero.copy() for _ in range(F + 1)] for _ in range(F + 1)]
        B = [[zero.copy() for _ in range(3)] for _ in range(F + 1)]
        for oy in range(-radius, radius + 1):
            for ox in range(-radius, radius + 1):
                # ---- e_p: crt_denoise_nlm's, on the weight pair ----
                cu, u_inside = shifted(wc, oy, ox)
                gu, _ = shifted(g, oy, ox)
                mn = np.where(gu < g, gu, g)
                d = (sq3(wc, cu) - al * (g + mn)) / (val(1e-10) + k2 * (g + gu))
                row = zero.copy()
                row_n = np.zeros((h, w), dtype=np.int64)
                for px in range(-patch, patch + 1):
                    dt, t_inside = shifted(d, 0, px)
                    ut, _ = shifted(u_inside, 0, px)
                    ok = t_inside & ut
                    row = np.where(ok, row + dt, row)
                    row_n += ok
                D = zero.copy()
                n = np.zeros((h, w), dtype=np.int64)
                for py in range(-patch, patch + 1):
                    rt, r_inside = shifted(row, py, 0)
                    nt, _ = shifted(row_n, py, 0)
                    D = D + np.where(r_inside, rt, T(0.0))
                    n += np.where(r_inside, nt, 0)
                Dm = D / n.astype(T)
                e_p = np.where(Dm < T(0.0), T(0.0), Dm)
                wgt = exp(-e_p)
                assert wgt.dtype == T and D.dtype == T and (n[u_inside] >= 1).all()
                # ---- the regressors, centred on p ----
                x = []
                if mask & NORMAL:
                    nq = shifted(normal, oy, ox)[0]
                    x += [(nq[..., ch] - normal[..., ch]) / sn for ch in range(3)]
                if mask & ALBEDO:
                    aq = shifted(albedo, oy, ox)[0]
                    x += [(aq[..., ch] - albedo[..., ch]) / sa for ch in range(3)]
                if mask & DEPTH:
                    dq = shifted(depth, oy, ox)[0]
                    m = np.where(depth > dq, depth, dq)
                    r = (dq - depth) / (sd * m)
                    x.append(np.where(m > 0, r, T(0.0)))
                if mask & POSITION:
                    x += [np.full((h, w), T(ox) / pos_den, dtype=T), np.full((h, w), T(oy) / pos_den, dtype=T)]
                x.append(one)
                assert len(x) == F + 1
                cq = shifted(c, oy, ox)[0]
                for i in range(F + 1):
                    wx = wgt * x[i]
                    for j in range(i, F + 1):
                        A[i][j] = np.where(u_inside, A[i][j] + wx * x[j], A[i][j])
                    for ch in range(3):
                        B[i][ch] = np.where(u_inside, B[i][ch] + wx * cq[..., ch], B[i][ch])
        S, Z = A[F][F], [B[F][ch] for ch in range(3)]
        for i in range(F):
            A[i][i] = A[i][i] + rg * S
        ok = np.ones((h, w), dtype=bool)
        for kk in range(F):
            d = A[kk][kk]
            ok &= d > 0
            for i in range(kk + 1, F + 1):
                f = A[kk][i] / d
                for j in range(i, F + 1):
                    A[i][j] = A[i][j] - f * A[kk][j]
                for ch in range(3):
                    B[i][ch] = B[i][ch] - f * B[kk][ch]
        d = A[F][F]
        ok &= d > 0
        out = np.stack([np.where(ok, B[F][ch] / d, Z[ch] / S) for ch in range(3)], axis=2)
    assert out.dtype == T and S.dtype == T
    return out, ~ok, S, np.stack(Z, axis=2)
