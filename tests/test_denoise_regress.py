"""First-order feature regression with non-local-means weights (crt_denoise_regress / crt_denoise_regress_device, include/crt.h;
denoise_regress, Render.run_view_denoised(regress=...) and the "reg" candidate of Render.run_view_selected in Python; crt_cli
--denoise-regress).

The contract of include/crt.h is restated in numpy, operation by operation, in tests/regress_restated.py, in float32 with the oracle's
det_expf and tone map and -- the same definition evaluated finer -- in float64.  The device result, and the host build of the kernel's own
text (tools/regress_host_check.cpp), must match the float32 restatement bit for bit: out_mean, out_rgb and fallback_pixels.  Comparisons
are on uint32 views; where the expected value is NaN the result must be NaN (payload not compared).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import host_program as HP
import oracle_lib as O
import regress_restated as RR
import util

F = np.float32
assert_bits = util.assert_bits
EXPORTS = ("crt_denoise_regress_defaults", "crt_denoise_regress_scratch_bytes", "crt_denoise_regress", "crt_denoise_regress_device")
NORMAL, ALBEDO, DEPTH, POSITION, ALL = RR.NORMAL, RR.ALBEDO, RR.DEPTH, RR.POSITION, RR.ALL
SETTINGS = ("radius", "patch", "k", "alpha", "sigma_normal", "sigma_albedo", "sigma_depth", "sigma_position", "ridge", "features")

# The largest relative deviation of the float32 restatement from the float64 evaluation of the same definition on the inputs of
# test_restatement_reproduces_an_affine_colour (two_planes(), radius 2, 3 and 5, the pixels and masks of AFFINE_CASES), measured on the
# CPU (docs/experiments.md, "The feature-regression filter"); the test's bound is 4 x this.
AFFINE_FP32_DEVIATION = 1.375e-5
AFFINE_BOUND = 4 * AFFINE_FP32_DEVIATION


def exp32(x):
    return O.math_fn("exp", x)


def restated(color, variance, **kw):
    """(mean, fell_back) of the float32 restatement"""
    mean, fell, _, _ = RR.restated(color, variance, exp=exp32, **kw)
    return mean, fell


# ------------------------------------------------------------------------------------------------------------------ inputs --

def synthetic(w, h, seed, special=False):
    """Random colours whose noise is small against the variance (weights between different pixels survive), fireflies whose patches match
    nothing (every weight but their own is 0: with ridge 0 they fall back), a block of zero variance, and guides that are noise on the
    left two thirds (well-conditioned systems) and plateaus with edges and a block of zero depth on the right (singular ones).
    special: NaN and +-inf scattered in colour, variance and guides."""
    rng = np.random.default_rng(seed)
    color = (F(10.0) + rng.random((h, w, 3)) * 4).astype(F)
    variance = (F(0.5) + rng.random((h, w, 3)) * 3).astype(F)
    n = rng.normal(size=(h, w, 3))
    normal = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(F)
    albedo = rng.random((h, w, 3)).astype(F)
    depth = (F(1.0) + rng.random((h, w)) * 49).astype(F)
    cut = (2 * w) // 3
    if w - cut >= 1 and w > 1:
        normal[:, cut:] = normal[0, 0]
        normal[h // 2:, cut:] = normal[0, min(1, w - 1)]
        albedo[:, cut:] = albedo[0, 0]
        albedo[:, cut + (w - cut) // 2:] = albedo[0, min(1, w - 1)]
        depth[:, cut:] = 7.0
        depth[h // 3:h // 3 + 3, cut:cut + 4] = 0.0
    variance[h // 4:h // 4 + 3, w // 5:w // 5 + 5] = 0.0
    for fy, fx in ((h // 2, w // 3), (h // 5, w // 2)):
        color[fy, fx] = 1e4
        variance[fy, fx] = 1e-3
    if special:
        values = np.array([np.nan, np.inf, -np.inf], dtype=F)
        for j, im in enumerate((color, variance, normal, albedo, depth)):
            flat = im.reshape(-1)
            idx = rng.permutation(flat.size)[:3]
            flat[idx] = values[(np.arange(idx.size) + j) % 3]
    return color, variance, {"albedo": albedo, "normal": normal, "depth": depth}


# the shapes of the issue: (w, h, radius, patch, features, ridge).  61 x 47: tiles cut by both far edges; 130 x 9: wider than two
# workgroups and lower than the window; 33 x 17 at the limits: window and patch reach past the image on all sides; 1 x 1 and 64 x 1.
# ridge 0, so that singular systems fall back; 64 x 1 has no second row for the position feature (its oy column is 0 everywhere).
SIZES = [(61, 47, 2, 1, ALL, 0.0), (130, 9, 3, 1, ALL, 0.0), (33, 17, 8, 3, NORMAL | DEPTH | POSITION, 0.0), (1, 1, 1, 1, ALL, 0.0),
         (64, 1, 2, 1, DEPTH, 0.0)]
# on 61 x 47: each single feature bit, the full mask (above), mask 0; two pairs; the full mask with a small ridge and with the default one
MASKS = [(NORMAL, 0.0), (ALBEDO, 0.0), (DEPTH, 0.0), (POSITION, 0.0), (0, 0.0), (NORMAL | POSITION, 0.0), (ALBEDO | DEPTH, 0.0), (ALL, 0.01), (ALL, RR.DEFAULTS["ridge"])]


def case_inputs(w, h):
    return synthetic(w, h, 50 + w)


@pytest.fixture(scope="module")
def cases():
    """{(w, h, radius, patch, features, ridge): (color, variance, guides, want_mean, fell_back)}: the restatement of every case, computed
    once, shared by the tests below, never written to.  Checked here: every case with a feature and ridge 0 has a fallback pixel, and
    in every case at least half of the pixels do not fall back (1 x 1: its one pixel does)."""
    out = {}
    for w, h, radius, patch, features, ridge in SIZES + [(61, 47, 2, 1, m, r) for m, r in MASKS]:
        color, variance, g = case_inputs(w, h)
        mean, fell = restated(color, variance, radius=radius, patch=patch, features=features, ridge=ridge, **g)
        if features and ridge == 0.0:
            assert fell.any(), (w, h, features)
        if w * h > 1:
            assert (~fell).mean() >= 0.5, (w, h, features, float((~fell).mean()))
        out[(w, h, radius, patch, features, ridge)] = (color, variance, g, mean, fell)
    return out


def check_device(color, variance, want_mean, want_fell, where, **kw):
    rgb, mean, info = crt.denoise_regress(color, variance, return_info=True, **kw)
    assert_bits(mean, want_mean, where + ": mean")
    assert np.array_equal(rgb, O.tonemap(want_mean)), where + ": rgb is not the tone map of the mean"
    assert info["fallback_pixels"] == int(want_fell.sum()), (where, info, int(want_fell.sum()))
    return mean


def two_planes(w=48, h=26):
    """Two planes that meet in a vertical crease at x = w / 2: per plane a linear depth ramp, a constant normal and a colour that is
    affine in the pixel position (another slope per plane, continuous across the crease); variance 0.01, no noise.
    Returns (color, variance, guides, crease)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    c = w // 2
    left = xx < c
    depth = np.where(left, 10.0 + 0.125 * xx + 0.0625 * yy, 10.0 + 0.125 * c + 0.375 * (xx - c) + 0.0625 * yy)
    normal = np.where(left[..., None], np.array([0.0, 0.6, 0.8]), np.array([0.6, 0.0, 0.8]))
    slopes = ((0.03125, 0.015625), (0.0625, -0.015625), (-0.015625, 0.03125))   # (d / dx, d / dy) per channel on the left; the right: twice d / dx
    color = np.stack([np.where(left, 4.0 + sx * xx + sy * yy, 4.0 + sx * c + 2 * sx * (xx - c) + sy * yy) for sx, sy in slopes], axis=2)
    assert (color > 1.0).all()
    return color.astype(F), np.full((h, w, 3), 0.01, dtype=F), {"normal": normal.astype(F), "depth": depth.astype(F)}, c


def off_crease(w, h, crease, radius):
    """the pixels whose window, cut by the image's border or not, lies in one plane"""
    xx = np.arange(w)[None, :] + np.zeros((h, 1), dtype=np.int64)
    return (xx + radius < crease) | (xx - radius >= crease)


def affine_deviations(radius, dtype, features, interior=False):
    """(the filtered two_planes(), which pixels fell back, the colour, the pixels to look at: those off the crease, with `interior` only
    the ones whose window the image's border does not cut either)"""
    color, variance, g, crease = two_planes()
    out, fell, _, _ = RR.restated(color, variance, radius=radius, patch=1, ridge=0.0, features=features, dtype=dtype, exp=exp32, **g)
    h, w = color.shape[:2]
    where = off_crease(w, h, crease, radius)
    if interior:
        where[:radius] = where[-radius:] = False
        where[:, :radius] = where[:, -radius:] = False
    return out, fell, color.astype(np.float64), where


# (features, interior): the position feature alone, at every pixel off the crease; with the depth feature, whose relative depth is all
# but collinear with the position on a linear ramp, where the window is whole (a cut window's system is too close to singular for fp32)
AFFINE_CASES = [(POSITION, False), (DEPTH | POSITION, True)]


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_regress_entry_points_are_exported():
    lib = capi.lib()
    for name in EXPORTS:
        assert name in capi.EXPORTS
        assert getattr(lib, name) is not None
    for name in ("denoise_regress", "denoise_regress_device", "denoise_regress_defaults", "denoise_regress_scratch_bytes"):
        assert name in crt.__all__ and callable(getattr(crt, name))
    assert lib.crt_abi_version() == 5 == capi.ABI_VERSION          # only entry points were added
    assert (crt.REGRESS_NORMAL, crt.REGRESS_ALBEDO, crt.REGRESS_DEPTH, crt.REGRESS_POSITION) == (1, 2, 4, 8)
    p = capi.RegressParams(7, 7, 99, 99, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, 99)
    assert lib.crt_denoise_regress_defaults(C.byref(p)) == capi.CRT_OK
    assert (p.width, p.height) == (0, 0)
    for name in SETTINGS:
        assert F(getattr(p, name)) == F(RR.DEFAULTS[name]), name
    assert crt.denoise_regress_defaults() == {k: (v if k in ("radius", "patch", "features") else float(F(v))) for k, v in RR.DEFAULTS.items()}
    assert lib.crt_denoise_regress_defaults(None) == capi.ERR_INVALID_ARG and lib.crt_last_error()
    assert crt.denoise_regress_scratch_bytes(100, 70) == 100 * 70 * 64
    n = C.c_uint64()
    for bad in ((0, 70, C.byref(n)), (100, 0, C.byref(n)), (100, 70, None)):
        assert lib.crt_denoise_regress_scratch_bytes(*bad) == capi.ERR_INVALID_ARG
    assert "reg" in crt.api._SELECT_CANDIDATES


def test_regress_arguments_are_checked_before_any_device_call():
    """Every refusal of the contract is CRT_ERR_INVALID_ARG with a message, from both entry points, also on a machine without a GPU.  The
    non-null buffers here are host memory that must never be dereferenced (a device call would fault on them)."""
    lib = capi.lib()
    buf = np.zeros(64, dtype=F)
    d = C.c_void_p((buf.ctypes.data + 15) & ~15)
    w, h = 64, 48
    need = crt.denoise_regress_scratch_bytes(w, h)
    inf, nan = float("inf"), float("nan")

    def params(**over):
        p = capi.RegressParams()
        assert lib.crt_denoise_regress_defaults(C.byref(p)) == capi.CRT_OK
        p.width, p.height = w, h
        for k, v in over.items():
            setattr(p, k, v)
        return C.byref(p)

    def inputs(**over):
        s = capi.RegressInputs(d, d, d, d, d, d, d)
        for k, v in over.items():
            setattr(s, k, v)
        return C.byref(s)

    def both(prm, inp, mean=d, rgb=d, want=capi.ERR_INVALID_ARG):
        r1 = lib.crt_denoise_regress(0, prm, inp, mean, rgb, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_denoise_regress_device(0, prm, inp, mean, rgb, d, need, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == want, (r1, r2, e1, e2)
        assert e1.startswith(b"crt_denoise_regress: ") and e2.startswith(b"crt_denoise_regress_device: ")
        return e1

    assert b"null" in both(None, inputs()) and b"null" in both(params(), None)
    assert b"colour" in both(params(), inputs(color=None))
    assert b"variance" in both(params(), inputs(variance=None))
    assert b"positive" in both(params(width=0), inputs()) and b"positive" in both(params(height=0), inputs())
    for bad in (0, 9, 1000):
        assert b"radius" in both(params(radius=bad), inputs())
    for bad in (4, 1000):
        assert b"patch" in both(params(patch=bad), inputs())
    for bad in (0.0, -0.0, -1.0, nan, inf, -inf):
        assert b"k must" in both(params(k=bad), inputs()), bad
    for bad in (-1e-3, -1.0, nan, inf, -inf):
        assert b"alpha" in both(params(alpha=bad), inputs()), bad
    for name in ("sigma_normal", "sigma_albedo", "sigma_depth", "sigma_position"):
        for bad in (0.0, -0.0, -1.0, nan, -inf):
            assert b"sigma" in both(params(**{name: bad}), inputs()), (name, bad)
    for bad in (-1e-3, -1.0, nan, inf, -inf):
        assert b"ridge" in both(params(ridge=bad), inputs()), bad
    assert b"features" in both(params(features=16), inputs()) and b"features" in both(params(features=1 << 31), inputs())
    for name, bit in (("normal", NORMAL), ("albedo", ALBEDO), ("depth", DEPTH)):
        assert name.encode() in both(params(features=bit), inputs(**{name: None}))
        assert name.encode() in both(params(), inputs(**{name: None}))
    assert b"no output" in both(params(), inputs(), mean=None, rgb=None)
    assert b"2^24" in both(params(width=(1 << 24) + 1), inputs(), want=capi.ERR_UNSUPPORTED)
    for scratch, size in ((None, need), (d, need - 1), (d, 0), (C.c_void_p(d.value + 4), need)):
        assert lib.crt_denoise_regress_device(0, params(), inputs(), d, d, scratch, size, None, None) == capi.ERR_INVALID_ARG
        assert b"scratch" in lib.crt_last_error()
    assert lib.crt_denoise_regress(-1, params(), inputs(), d, d, None) == capi.ERR_INVALID_ARG and b"device" in lib.crt_last_error()
    assert lib.crt_denoise_regress_device(-1, params(), inputs(), d, d, d, need, None, None) == capi.ERR_INVALID_ARG and b"device" in lib.crt_last_error()
    assert not buf.any()
    # the Python layer's own
    img = np.zeros((6, 8, 3), dtype=F)
    with pytest.raises(ValueError):
        crt.denoise_regress(img, None)
    with pytest.raises(ValueError):
        crt.denoise_regress(img, img, weight_color=np.zeros((6, 9, 3), dtype=F))
    with pytest.raises(ValueError):
        crt.denoise_regress(img, img, bandwidth=3)
    with pytest.raises(ValueError):
        crt.denoise_regress(img, img, radius=2.5)
    for bad in (dict(nlm=True), dict(variance_guided=True), dict(iterations=2), dict(sigma_color=3.0)):
        with pytest.raises(ValueError, match="regress"):
            crt.Render.run_view_denoised(_NoHandle(), None, None, None, regress=True, **bad)
    with pytest.raises(ValueError, match="regress"):
        crt.Render.run_view_denoised(_NoHandle(), None, None, None, regress={"sigma_color": 3.0})


class _NoHandle:
    """stands in for a Render whose argument checks are all that runs"""
    def _handle(self, who):
        pass


# (index into SIZES / MASKS, outputs: bit 0 mean, 1 rgb; weights: a weight pair of its own; guides: which are handed over)
HOST_JOBS = [("size", i, 3, False, 7) for i in range(len(SIZES))] + [("mask", i, 3, False, 7) for i in range(len(MASKS))] + \
            [("size", 0, 1, True, 7), ("size", 1, 2, True, 7), ("mask", 3, 3, False, 0), ("mask", 0, 3, True, 2)]


def host_job_case(job):
    kind, i, outputs, weights, guides = job
    w, h, radius, patch, features, ridge = SIZES[i] if kind == "size" else (61, 47, 2, 1) + MASKS[i]
    color, variance, g = case_inputs(w, h)
    wc, wv = synthetic(w, h, 900 + w)[:2] if weights else (None, None)
    return (w, h, radius, patch, features, ridge), color, variance, g, wc, wv


@pytest.fixture(scope="module")
def host_check_run(tmp_path_factory):
    """both builds of tools/regress_host_check.cpp run over HOST_JOBS: [(status, bytes, stderr) plain, sanitised]"""
    tmp = str(tmp_path_factory.mktemp("regress_host"))
    blob = [np.array([len(HOST_JOBS)], dtype="<u4").tobytes()]
    for job in HOST_JOBS:
        (w, h, radius, patch, features, ridge), color, variance, g, wc, wv = host_job_case(job)
        blob.append(np.array([w, h, radius, patch, features, job[2], int(job[3]), job[4]], dtype="<u4").tobytes())
        blob.append(np.array([RR.DEFAULTS[n] for n in ("k", "alpha", "sigma_normal", "sigma_albedo", "sigma_depth", "sigma_position")] + [ridge],
                             dtype="<f4").tobytes())
        images = [color, variance] + ([wc, wv] if job[3] else []) + [g[n] for bit, n in ((1, "albedo"), (2, "normal"), (4, "depth")) if job[4] & bit]
        blob += [np.ascontiguousarray(x, dtype="<f4").tobytes() for x in images]
    path = os.path.join(tmp, "in.bin")
    with open(path, "wb") as f:
        f.write(b"".join(blob))
    return HP.run_both_forms("regress_host_check.cpp", tmp, path)


def test_kernel_text_on_the_host_gives_the_restatement_bits(host_check_run):
    """csrc/crt_regress.h on crt_nlm.h as they are, compiled with g++ -ffp-contract=off, the kernel's body workgroup by workgroup: every
    output of every case against the restatement, bit for bit; an output that was not asked for is not written"""
    rc, raw, err = host_check_run[0]
    assert rc == 0, err
    off = 0
    for job in HOST_JOBS:
        (w, h, radius, patch, features, ridge), color, variance, g, wc, wv = host_job_case(job)
        want, fell = restated(color, variance, weight_color=wc, weight_variance=wv, radius=radius, patch=patch, features=features, ridge=ridge, **g)
        n = w * h
        got_mean = np.frombuffer(raw, dtype="<f4", count=n * 3, offset=off).reshape(h, w, 3); off += n * 12
        got_rgb = np.frombuffer(raw, dtype=np.uint8, count=n * 3, offset=off).reshape(h, w, 3); off += n * 3
        got_fell = int(np.frombuffer(raw[off:off + 8], dtype="<u8")[0]); off += 8
        where = "job %r" % (job,)
        if job[2] & 1:
            assert_bits(got_mean, want, where + " mean")
        else:
            assert (got_mean.view(np.uint32) == 0x5a5a5a5a).all(), where
        assert np.array_equal(got_rgb, O.tonemap(want)) if job[2] & 2 else (got_rgb == 0x5a).all(), where + " rgb"
        assert got_fell == int(fell.sum()), (where, got_fell, int(fell.sum()))
    assert off == len(raw)


def test_kernel_text_is_clean_under_the_sanitizers(host_check_run):
    """the same stand-alone program built with -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all: exit status 0
    and the same bytes -- no LDS, plane or image index outside its array (each has exactly its size)"""
    assert host_check_run[1][0] == 0, host_check_run[1][2]
    assert host_check_run[0][0] == 0 and host_check_run[1][1] == host_check_run[0][1] and len(host_check_run[0][1]) > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_without_features_is_the_weighted_mean(dtype):
    color, variance, g = synthetic(40, 21, 3)
    out, fell, S, Z = RR.restated(color, variance, radius=3, patch=1, features=0, ridge=0.0, dtype=dtype, exp=exp32, **g)
    assert not fell.any()
    with np.errstate(all="ignore"):
        assert np.array_equal(out, Z / S[..., None]) and np.isfinite(out).all()
    assert (S >= 1).all()           # the pixel itself has the weight exp(-0) = 1
    assert not np.array_equal(out, color.astype(dtype))


def test_restatement_reproduces_an_affine_colour():
    """ridge 0 on two_planes(): the colour is exactly affine in the position regressors (the depth regressor, where enabled, gets the
    coefficient 0), so the fit's value at the pixel is the colour, whatever the weights -- at the pixels of AFFINE_CASES, none of whose
    windows crosses the crease.  float64: to 1e-9; float32: within 4 x the measured deviation of the float32 from the float64
    evaluation (AFFINE_FP32_DEVIATION: the largest over these cases and radii).  The zero-order mask on the same input does not
    reproduce the ramp: where the image's border cuts the window its weighted mean is pulled inwards, by far more than the bound.  (Where
    the window is whole, the weights of a ramp are symmetric and a weighted mean does follow it: 4.6e-7 at radius 5.)  With the normal
    feature too every system is singular -- a plane's normal is constant -- and every pixel off the crease falls back."""
    assert AFFINE_BOUND > 0
    for radius in (2, 3, 5):
        for features, interior in AFFINE_CASES:
            out64, fell64, truth, where = affine_deviations(radius, np.float64, features, interior)
            out32, fell32, _, _ = affine_deviations(radius, np.float32, features, interior)
            assert where.sum() > 200 and not fell64[where].any() and not fell32[where].any()
            dev64 = float((np.abs(out64 - truth) / truth)[where].max())
            dev32 = float((np.abs(out32.astype(np.float64) - truth) / truth)[where].max())
            measured = float((np.abs(out32.astype(np.float64) - out64) / np.abs(out64))[where].max())
            print("radius %d features %d: deviation from the ramp float64 %.3g, float32 %.3g (float32 from float64: %.4g); bound %.3g"
                  % (radius, features, dev64, dev32, measured, AFFINE_BOUND))
            assert dev64 < 1e-9
            assert dev32 <= AFFINE_BOUND
        zero32, zfell, truth, where = affine_deviations(radius, np.float32, 0)
        devz = float((np.abs(zero32.astype(np.float64) - truth) / truth)[where].max())
        print("radius %d: the zero-order mask deviates by %.3g" % (radius, devz))
        assert devz > AFFINE_BOUND and not zfell.any()
    _, fell_n, _, where = affine_deviations(3, np.float32, NORMAL | DEPTH | POSITION)
    assert fell_n[where].all()


def test_restatement_falls_back_where_all_weights_are_on_one_pixel():
    """ridge 0, alpha 0 and a small k (a huge k-scaled distance).  (1) An image whose pixels all differ by far more than their variance:
    every weight but a pixel's own is exp(-huge) = 0, every regressor of that one tap is 0, so every feature pivot is 0 and every pixel
    falls back to Z / S = its own colour.  (2) A constant image with one outlier: the pixels whose patch holds the outlier match
    nothing but themselves and fall back likewise; the others have weights of 1 all round, and with the position feature alone a
    regular system that reproduces the constant."""
    h, w = 9, 11
    levels = (np.arange(h * w, dtype=np.float64).reshape(h, w, 1) * 1000.0 + np.array([1.0, 2.0, 3.0])).astype(F)
    variance = np.full((h, w, 3), 1e-3, dtype=F)
    g = {"normal": np.zeros((h, w, 3), dtype=F) + F(0.5), "albedo": np.zeros((h, w, 3), dtype=F) + F(0.25), "depth": np.full((h, w), 3.0, dtype=F)}
    for dtype in (np.float32, np.float64):
        for features in (POSITION, ALL):
            out, fell, S, Z = RR.restated(levels, variance, radius=3, patch=1, k=0.01, alpha=0.0, ridge=0.0, features=features, dtype=dtype, exp=exp32, **g)
            assert fell.all() and (S == 1).all()
            assert np.array_equal(out, Z / S[..., None]) and np.array_equal(out, levels.astype(dtype))
    const = np.full((h, w, 3), 2.0, dtype=F)
    const[4, 5] = 1e4
    out, fell = restated(const, variance, radius=3, patch=1, k=0.01, alpha=0.0, ridge=0.0, features=POSITION)
    near = np.zeros((h, w), dtype=bool)
    near[3:6, 4:7] = True
    assert np.array_equal(fell, near)
    assert_bits(out, const, "a constant with an outlier")


# ------------------------------------------------------------------------------------------------------------------ GPU --

@pytest.mark.gpu
@pytest.mark.parametrize("w,h,radius,patch,features,ridge", SIZES)
def test_regress_sizes_match_restatement(cases, w, h, radius, patch, features, ridge):
    color, variance, g, want, fell = cases[(w, h, radius, patch, features, ridge)]
    mean = check_device(color, variance, want, fell, "%dx%d r%d f%d mask %d" % (w, h, radius, patch, features), radius=radius, patch=patch,
                        features=features, ridge=ridge, **g)
    if w * h == 1:
        assert_bits(mean, color, "1x1")
        assert fell.all()
    else:
        assert not np.array_equal(mean, color)


@pytest.mark.gpu
@pytest.mark.parametrize("features,ridge", MASKS)
def test_regress_feature_masks_match_restatement(cases, features, ridge):
    """each single feature, pairs, no feature and the full mask with a ridge; and a disabled feature's buffer left out gives the
    same bits as handing it over"""
    color, variance, g, want, fell = cases[(61, 47, 2, 1, features, ridge)]
    check_device(color, variance, want, fell, "mask %d ridge %g" % (features, ridge), radius=2, patch=1, features=features, ridge=ridge, **g)
    enabled = {n: g[n] for n, bit in (("normal", NORMAL), ("albedo", ALBEDO), ("depth", DEPTH)) if features & bit}
    if len(enabled) < 3:
        check_device(color, variance, want, fell, "mask %d, the disabled guides NULL" % features, radius=2, patch=1, features=features, ridge=ridge, **enabled)
    if features == 0:
        assert not fell.any()


@pytest.mark.gpu
def test_regress_weights_from_another_image():
    w, h = 61, 47
    color, variance, g = case_inputs(w, h)
    wc, wv, _ = synthetic(w, h, 901)
    kw = dict(radius=2, patch=1, ridge=0.0, **g)
    both, fell = restated(color, variance, weight_color=wc, weight_variance=wv, **kw)
    check_device(color, variance, both, fell, "both weights", weight_color=wc, weight_variance=wv, **kw)
    only_c, fell_c = restated(color, variance, weight_color=wc, **kw)
    check_device(color, variance, only_c, fell_c, "weight_color only", weight_color=wc, **kw)
    only_v, fell_v = restated(color, variance, weight_variance=wv, **kw)
    check_device(color, variance, only_v, fell_v, "weight_variance only", weight_variance=wv, **kw)
    own, _ = restated(color, variance, **kw)
    assert not np.array_equal(both, own) and not np.array_equal(only_c, own) and not np.array_equal(only_v, own)
    # the pair given explicitly is the pair left out
    check_device(color, variance, own, restated(color, variance, **kw)[1], "the image as its own weights", weight_color=color, weight_variance=variance, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("ridge", [0.0, 0.01])
def test_regress_non_finite_pixels(ridge):
    """NaN and +-inf scattered in colour, variance and guides: the arithmetic defines the result; a NaN pivot falls back"""
    color, variance, g = synthetic(61, 47, 77, special=True)
    assert all(not np.isfinite(x).all() for x in (color, variance, g["normal"], g["albedo"], g["depth"]))
    want, fell = restated(color, variance, radius=2, patch=1, ridge=ridge, **g)
    mean = check_device(color, variance, want, fell, "non-finite inputs, ridge %g" % ridge, radius=2, patch=1, ridge=ridge, **g)
    assert fell.any() and (~fell).mean() >= 0.5
    assert np.isnan(mean).any() and np.isfinite(mean).any()


@pytest.mark.gpu
def test_regress_each_optional_output_may_be_left_out(cases):
    color, variance, g, want, fell = cases[SIZES[0]]
    kw = dict(radius=2, patch=1, features=ALL, ridge=0.0, **g)
    rgb, mean = crt.denoise_regress(color, variance, want_rgb=False, **kw)
    assert rgb is None
    assert_bits(mean, want, "without rgb")
    rgb, mean = crt.denoise_regress(color, variance, want_mean=False, **kw)
    assert mean is None and np.array_equal(rgb, O.tonemap(want))


@pytest.mark.gpu
def test_regress_device_form_on_a_stream(cases):
    w, h, radius, patch, features, ridge = SIZES[0]
    color, variance, g, want, fell = cases[SIZES[0]]
    wc = synthetic(w, h, 901)[0]
    want_w, fell_w = restated(color, variance, weight_color=wc, radius=radius, patch=patch, features=features, ridge=ridge, **g)
    scratch_bytes = crt.denoise_regress_scratch_bytes(w, h)
    host = {"color": color, "variance": variance, "wc": wc, "albedo": g["albedo"], "normal": g["normal"], "depth": g["depth"]}
    outs = {"out_mean": w * h * 12, "out_rgb": w * h * 3}
    # (every output value must be written by the filter: what is not uploaded is filled with 0x55)
    with DeviceBuffers({**host, **outs, "scratch": scratch_bytes}, stream=True) as d:
        ptrs = d.ptrs

        def run(want_info, out_mean=True, out_rgb=True, weight=None):
            return crt.denoise_regress_device(w, h, ptrs["color"], ptrs["variance"], ptrs["out_mean"] if out_mean else None,
                                              ptrs["out_rgb"] if out_rgb else None, ptrs["scratch"], scratch_bytes, albedo_ptr=ptrs["albedo"],
                                              normal_ptr=ptrs["normal"], depth_ptr=ptrs["depth"], weight_color_ptr=weight, stream=d.stream,
                                              want_info=want_info, radius=radius, patch=patch, features=features, ridge=ridge)

        assert run(False) is None
        d.synchronize()
        assert_bits(d.download("out_mean", (h, w, 3), F), want, "device form")
        assert np.array_equal(d.download("out_rgb", (h, w, 3), np.uint8), O.tonemap(want))
        # the mean only, with the info (the call synchronizes the stream), the weights from another image
        for n in outs:
            d.fill(n)
        info = run(True, out_rgb=False, weight=ptrs["wc"])
        assert info["fallback_pixels"] == int(fell_w.sum()) and info["total_ms"] > 0, info
        assert_bits(d.download("out_mean", (h, w, 3), F), want_w, "device form, mean only")
        assert (d.download("out_rgb", (h, w, 3), np.uint8) == 0x55).all()


@pytest.fixture(scope="module")
def cornell():
    t = util.task("cornell-box")
    r = crt.Render(util.host_scene("cornell-box"), 4, t.P_RR, t.light_sample_n)
    yield r
    r.free()


@pytest.mark.gpu
def test_run_view_denoised_regress_equals_the_calls_by_hand(cornell):
    name, w, h = "cornell-box", 48, 36
    r = cornell
    eye, iv, fov = util.camera(name)
    r.set_spp(4)
    rgb0 = r.run_view(eye, iv, fov, width=w, height=h, want_variance=True).copy()
    mean0, var0 = r.mean_buffer.copy(), r.variance_buffer.copy()
    g = r.run_view_aov(eye, iv, fov, want=("albedo", "normal", "depth"), width=w, height=h)
    want_rgb, want_mean, want_info = crt.denoise_regress(mean0, var0, return_info=True, **g)
    rgb, mean = r.run_view_denoised(eye, iv, fov, width=w, height=h, regress=True)
    assert_bits(mean, want_mean, "run_view_denoised(regress=True)")
    assert np.array_equal(rgb, want_rgb) and np.array_equal(r.frame_buffer, rgb0)
    assert r.denoise_info["fallback_pixels"] == want_info["fallback_pixels"]
    # ... which is the restatement's
    res_mean, res_fell = restated(mean0, var0, **g)
    assert_bits(want_mean, res_mean, "the defaults against the restatement")
    assert want_info["fallback_pixels"] == int(res_fell.sum())
    _, mean2 = r.run_view_denoised(eye, iv, fov, width=w, height=h, regress={"radius": 3, "patch": 0, "ridge": 0.1, "features": DEPTH | POSITION}, sigma_depth=0.1)
    assert_bits(mean2, crt.denoise_regress(mean0, var0, radius=3, patch=0, ridge=0.1, features=DEPTH | POSITION, sigma_depth=0.1, **g)[1], "with settings")
    # on irradiance: demodulate -> regress without the albedo feature -> modulate, by hand
    rgb3, mean3 = r.run_view_denoised(eye, iv, fov, width=w, height=h, regress=True, demodulate=True)
    sh = r.shading_buffers
    irr, ivar = crt.demodulate(mean0, sh["diffuse_albedo"], sh["emission"], variance=var0)
    filtered = crt.denoise_regress(irr, ivar, want_rgb=False, features=ALL & ~ALBEDO, **r.aov_buffers)[1]
    want_rgb3, want_mean3 = crt.modulate(filtered, sh["diffuse_albedo"], sh["emission"])
    assert_bits(mean3, want_mean3, "run_view_denoised(regress=True, demodulate=True)")
    assert np.array_equal(rgb3, want_rgb3)
    # the other forms are what they were
    _, mean4 = r.run_view_denoised(eye, iv, fov, width=w, height=h, nlm=True)
    assert_bits(mean4, crt.denoise_nlm(mean0, var0, **g)[1], "run_view_denoised(nlm=True)")


@pytest.mark.gpu
def test_run_view_selected_with_reg_is_its_pieces_called_by_hand(cornell):
    name, w, h = "cornell-box", 48, 36
    r = cornell
    eye, iv, fov = util.camera(name)
    r.set_spp(4)
    rgb, mean = r.run_view_selected(eye, iv, fov, candidates=("var", "reg"), width=w, height=h)
    info = r.select_info
    r.run_view(eye, iv, fov, width=w, height=h, want_halves=True)
    a, b, done = r.half_buffers(width=w, height=h)
    assert done == 4
    half_var = F(2.0) * r.variance(width=w, height=h)[0]
    g = r.run_view_aov(eye, iv, fov, want=("albedo", "normal", "depth"), width=w, height=h)
    fa = [crt.denoise_var(a, half_var, want_rgb=False, **g)[1], crt.denoise_regress(a, half_var, weight_color=b, weight_variance=half_var, want_rgb=False, **g)[1]]
    fb = [crt.denoise_var(b, half_var, want_rgb=False, **g)[1], crt.denoise_regress(b, half_var, weight_color=a, weight_variance=half_var, want_rgb=False, **g)[1]]
    rgb2, mean2, choice2, error2, info2 = crt.filter_select(a, b, half_var, fa, fb, return_info=True)
    assert np.array_equal(rgb, rgb2)
    assert_bits(mean, mean2, "run_view_selected mean")
    assert np.array_equal(r.select_buffers["choice"], choice2) and info["chosen"] == info2["chosen"] and sum(info["chosen"]) == w * h
    assert_bits(fa[1], restated(a, half_var, weight_color=b, weight_variance=half_var, **g)[0], "half A with half B's weights against the restatement")
    assert not np.array_equal(fa[1], crt.denoise_regress(a, half_var, want_rgb=False, **g)[1])      # the other half's weights are other weights
    with pytest.raises(ValueError):
        r.run_view_selected(eye, iv, fov, candidates=("none", "atrous", "var", "nlm", "reg"), width=w, height=h)


@pytest.mark.gpu
def test_cli_writes_the_regress_frame_and_selects_with_reg(cornell, tmp_path):
    from PIL import Image
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    name, w, h = "cornell-box", 48, 36
    base = [cli, util.SCENES[name], "--spp", "4", "--width", str(w), "--height", str(h), "--seed", "42", "--base-dir", util.ROOT]
    noisy, den, den2, sel = (str(tmp_path / n) for n in ("noisy.png", "den.png", "den2.png", "sel.png"))
    r = cornell
    eye, iv, fov = util.camera(name)
    r.set_spp(4)
    r.seed = 42
    try:
        rgb0 = r.run_view(eye, iv, fov, width=w, height=h, want_variance=True).copy()
        mean0, var0 = r.mean_buffer.copy(), r.variance_buffer.copy()
        g = r.run_view_aov(eye, iv, fov, want=("albedo", "normal", "depth"), width=w, height=h)
        want_sel, _ = r.run_view_selected(eye, iv, fov, candidates=("var", "reg"), width=w, height=h)
    finally:
        r.seed = 0
    res = subprocess.run(base + ["-o", noisy, "--denoise", den, "--denoise-regress"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert np.array_equal(np.asarray(Image.open(noisy)), rgb0)
    assert np.array_equal(np.asarray(Image.open(den)), crt.denoise_regress(mean0, var0, **g)[0])
    res = subprocess.run(base + ["-o", noisy, "--denoise", den2, "--denoise-regress", "--denoise-regress-params", "3,0,0.5,0.1", "--denoise-sigma", "77,0.25,0.2,0.1"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    want = crt.denoise_regress(mean0, var0, radius=3, patch=0, k=0.5, ridge=0.1, sigma_normal=0.25, sigma_albedo=0.2, sigma_depth=0.1, **g)[0]
    assert np.array_equal(np.asarray(Image.open(den2)), want)
    res = subprocess.run(base + ["-o", noisy, "--denoise", sel, "--denoise-select", "var+reg"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert np.array_equal(np.asarray(Image.open(sel)), want_sel)
    for extra in (["--denoise", den, "--denoise-regress", "--denoise-nlm"], ["--denoise", den, "--denoise-regress", "--denoise-variance"],
                  ["--denoise", den, "--denoise-regress", "--denoise-iterations", "2"], ["--denoise-regress"],
                  ["--denoise", den, "--denoise-regress-params", "3,0,0.5,0.1"], ["--denoise", den, "--denoise-regress", "--denoise-regress-params", "3,0,0.5"],
                  ["--gpus", "2", "--denoise-regress"]):
        bad = subprocess.run([cli, util.SCENES[name]] + extra, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "--denoise-" in bad.stderr, (extra, bad.stderr)
