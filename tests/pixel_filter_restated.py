"""The pixel reconstruction filters of include/crt.h (CRT_FLAG_PIXEL_FILTER, crt_filtered_frame) restated in numpy float32, operation by
operation as the header states them, on the oracle's per-path radiance L (h, w, S, 3).  The jitter of every sample comes from a
vectorised numpy Philox4x32-10 with the draw addressing of csrc/crt_detmath.h; check_philox() holds it against oracle_lib.rng_draw.

    sums(L, S, n, kind, R, seed)               -> a (h, w, 3), W (h, w) after samples 0 .. n-1: float32, one ufunc per operation
    filtered(L, S, n, kind, R, seed)           -> (mean, rgb): the read-out
    sums64(L, S, n, kind, R, seed)             -> the float64 evaluation of the same sums, with what the error bound needs
"""
import numpy as np

import oracle_lib as O
from util import restated_sums

F = np.float32
U32 = np.uint32
U64 = np.uint64
BOX, TENT, MITCHELL = 0, 1, 2
KINDS = {"box": BOX, "tent": TENT, "mitchell": MITCHELL}


def philox4x32_10(c, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011) on uint32 arrays of one shape: c = four counter words, key (k0, k1); returns the four words"""
    c0, c1, c2, c3 = (np.asarray(v, dtype=U32) for v in c)
    k0, k1 = np.asarray(k0, dtype=U32).copy(), np.asarray(k1, dtype=U32).copy()
    m0, m1 = U64(0xD2511F53), U64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c0.astype(U64), m1 * c2.astype(U64)
        c0, c1, c2, c3 = (p1 >> U64(32)).astype(U32) ^ c1 ^ k0, p1.astype(U32), (p0 >> U64(32)).astype(U32) ^ c3 ^ k1, p0.astype(U32)
        k0 = (k0.astype(U64) + U64(0x9E3779B9)).astype(U32)
        k1 = (k1.astype(U64) + U64(0xBB67AE85)).astype(U32)
    return c0, c1, c2, c3


def uniform(x):
    """rng_uniform: curand_uniform's (0, 1] mapping, one conversion, one multiply, one add"""
    u = x.astype(F) * F(2.3283064365386963e-10) + F(1.1641532182693481e-10)
    assert u.dtype == F
    return u


def jitter(seed, w, h, k):
    """(ux, uy), (h, w) float32 each: rng_uniform of words x and y of rng_draw(seed, j * w + i, k, 0, RNG_JITTER, 0)"""
    pixel = np.arange(w * h, dtype=U32).reshape(h, w)
    zero = np.zeros_like(pixel)
    r = philox4x32_10((zero + U32(k), zero, zero, zero + U32(seed >> 32)), pixel, zero + U32(seed & 0xffffffff))
    return uniform(r[0]), uniform(r[1])


def check_philox(seeds=(0, 7, (5 << 32) | 9), w=13, h=9, ks=(0, 3)):
    """the numpy draws against the oracle's own rng_draw on a handful of pixels, samples and seeds (one above 2^32)"""
    for seed in seeds:
        for k in ks:
            ux, uy = jitter(seed, w, h, k)
            for i, j in ((0, 0), (w - 1, 0), (5, 4), (w - 1, h - 1)):
                u, f = O.rng_draw(seed, j * w + i, k, 0, 0, 0)
                got = np.array([ux[j, i], uy[j, i]], dtype=F)
                assert np.array_equal(got.view(U32), f[:2].view(U32)), (seed, k, i, j, got, f)
                assert (got > 0).all() and (got <= 1).all()


def reach_of(R):
    """ceil(R - 0.5), R - 0.5 in float32 (exact for the radii allowed)"""
    return int(np.ceil(F(R) - F(0.5)))


def weight(kind, R, d):
    """f(d) of the contract, elementwise"""
    R = F(R)
    x = np.abs(d)
    if kind == BOX:
        f = np.ones_like(d)
    elif kind == TENT:
        f = F(1) - x / R
    else:
        lo = ((((F(21) * x - F(36)) * x) * x) + F(16)) / F(18)
        hi = ((((F(-7) * x + F(36)) * x - F(60)) * x) + F(32)) / F(18)
        f = np.where(x < F(1), lo, hi)
    f = np.where((d > -R) & (d <= R), f, F(0))
    assert f.dtype == F
    return f


def _taps(L, S, n, kind, R, seed):
    """For every sample k < n and every (dj, di) in the contract's order: (output slices, w (float32), x of the tapped pixels (float32),
    mask of the taps that are not skipped)"""
    h, w = L.shape[:2]
    reach = reach_of(R)
    with np.errstate(all="ignore"):
        for k in range(n):
            ux, uy = jitter(seed, w, h, k)
            x = L[:, :, k, :] / F(S)
            for dj in range(-reach, reach + 1):
                j0, j1 = max(0, -dj), min(h, h - dj)
                for di in range(-reach, reach + 1):
                    i0, i1 = max(0, -di), min(w, w - di)
                    if j0 >= j1 or i0 >= i1:
                        continue
                    q = (slice(j0 + dj, j1 + dj), slice(i0 + di, i1 + di))      # the pixels tapped: inside the frame
                    p = (slice(j0, j1), slice(i0, i1))                          # the output pixels they are tapped for
                    dx = (F(di) + ux[q]) - F(0.5)
                    dy = (F(dj) + uy[q]) - F(0.5)
                    wt = weight(kind, R, dx) * weight(kind, R, dy)
                    assert wt.dtype == F
                    yield p, wt, x[q], wt != 0


def sums(L, S, n, kind, R, seed):
    h, w = L.shape[:2]
    a, W = np.zeros((h, w, 3), dtype=F), np.zeros((h, w), dtype=F)
    with np.errstate(all="ignore"):
        for p, wt, x, m in _taps(L, S, n, kind, R, seed):
            a[p] = np.where(m[..., None], a[p] + wt[..., None] * x, a[p])
            W[p] = np.where(m, W[p] + wt, W[p])
    return a, W


def resolve(a, W, c, S, n):
    """out_mean of the contract from the sums a, W and the frame's c after n of S samples"""
    with np.errstate(all="ignore"):
        r = F(S) / W
        out = np.where((W > 0)[..., None], a * r[..., None], c * (F(S) / F(n)))
    assert out.dtype == F
    return out


def filtered(L, S, n, kind, R, seed):
    """(out_mean, out_rgb) of crt_filtered_frame after samples 0 .. n-1 of S"""
    a, W = sums(L, S, n, kind, R, seed)
    mean = resolve(a, W, restated_sums(L, S, n)[0], S, n)
    return mean, O.tonemap(mean)


def sums64(L, S, n, kind, R, seed):
    """The same sums in float64 from the same float32 weights w and quotients x (both as the contract defines them): a64 = sum w x,
    W64 = sum w, and per pixel what the error bound takes: absum = sum |w x| (per channel), absw = sum |w|, taps = the taps added."""
    h, w = L.shape[:2]
    a, absum = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    W, absw, taps = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w), dtype=np.int64)
    for p, wt, x, m in _taps(L, S, n, kind, R, seed):
        t = np.where(m[..., None], wt[..., None].astype(np.float64) * x.astype(np.float64), 0.0)
        a[p] += t
        absum[p] += np.abs(t)
        W[p] += np.where(m, wt, 0).astype(np.float64)
        absw[p] += np.abs(np.where(m, wt, 0)).astype(np.float64)
        taps[p] += m
    return a, W, absum, absw, taps
