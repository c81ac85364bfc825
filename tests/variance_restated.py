"""The contracts of crt_variance and crt_render_adaptive (include/crt.h) restated in numpy float32, one ufunc per IEEE operation, on
the oracle's per-path radiance L (h, w, S, 3).  tests/test_variance.py and tests/test_adaptive.py check them against float64."""
import numpy as np

import oracle_lib as O
from util import restated_sums

F = np.float32


def restated_variance(L, S, n=None):
    n = S if n is None else n
    c, q = restated_sums(L, S, n)
    fn, fs = F(n), F(S)
    with np.errstate(all="ignore"):
        d = fn * q - c * c
        d = np.where(d < F(0.0), F(0.0), d)
        r = fs / fn
        var = ((r * r) * d) / (fn - F(1.0))
    assert var.dtype == F
    return var


def variance_of_sums(c, q, fn, r):
    """crt_variance's formula; fn, r: float32 scalars or (h, w, 1) arrays"""
    d = fn * q - c * c
    d = np.where(d < F(0.0), F(0.0), d)
    return ((r * r) * d) / (fn - F(1.0))


def restated_adaptive(L, S, min_samples, step_samples, threshold, mean_floor):
    """The contract of crt_render_adaptive on per-path radiance L (h, w, S, 3): dict of samples (h, w) uint32, mean, variance
    (h, w, 3) float32, rgb, pass_pixels, passes, paths."""
    thr, floor, fs = F(threshold), F(mean_floor), F(S)
    with np.errstate(all="ignore"):
        c, q = restated_sums(L, S, min_samples)
        n = min_samples
        nsamp = np.full(L.shape[:2], n, dtype=np.uint32)
        active = np.ones(L.shape[:2], dtype=bool)
        pass_pixels = []
        while n < S:
            fn = F(n)
            r = fs / fn
            var = variance_of_sums(c, q, fn, r)
            p = c * r
            v = (var[..., 0] + var[..., 1]) + var[..., 2]
            m = (p[..., 0] + p[..., 1]) + p[..., 2]
            t = thr * (m + floor)
            stop = v <= t * t
            active = active & ~stop
            if not active.any():
                break
            pass_pixels.append(int(active.sum()))
            ns = min(step_samples, S - n)
            a3 = active[..., None]
            for k in range(n, n + ns):
                x = L[:, :, k, :] / fs
                c = np.where(a3, c + x, c)
                q = np.where(a3, q + x * x, q)
            n += ns
            nsamp[active] = n
        fn = nsamp.astype(F)[..., None]
        r = fs / fn
        mean = c * r
        var = variance_of_sums(c, q, fn, r)
    for a in (c, q, mean, var, v):
        assert a.dtype == F
    return dict(samples=nsamp, mean=mean, variance=var, rgb=O.tonemap(mean), pass_pixels=pass_pixels, passes=1 + len(pass_pixels),
                paths=int(nsamp.astype(np.uint64).sum()), c=c)
