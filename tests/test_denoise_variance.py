"""Variance-guided form of the a-trous denoiser (crt_denoise_var / crt_denoise_var_device, include/crt.h; denoise_var and
Render.run_view_denoised(variance_guided=True) in Python; crt_cli --denoise-variance).

The contract of include/crt.h is restated below in numpy float32, operation by operation, with the oracle's det_expf
(oracle_lib.math_fn("exp")) and tone map (oracle_lib.tonemap); the device result must match it bit for bit, the filtered variance
included.  Comparisons are on uint32 views; where the expected value is NaN the result must be NaN (payload not compared).  Two checks do
not use the restatement: one against crt_denoise, the kernel that is verified already, and one on an edge no weight crosses.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import oracle_lib as O
import util
from frames import GUIDES, gpu_frame, renders  # noqa: F401

DEFAULTS = {"iterations": 3, "sigma_color": 6.0, "sigma_normal": 0.5, "sigma_albedo": 0.1, "sigma_depth": 0.05}
H5 = np.array([1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16], dtype=np.float32)
K3 = np.array([1.0 / 4, 1.0 / 2, 1.0 / 4], dtype=np.float32)
F = np.float32
assert_bits = util.assert_bits


def restated(color, variance, albedo=None, normal=None, depth=None, iterations=3, sigma_color=6.0, sigma_normal=0.5, sigma_albedo=0.1,
             sigma_depth=0.05):
    """The contract, in numpy float32: every ufunc below is one IEEE fp32 operation per element.  Returns (c_iterations, v_iterations)."""
    c = np.ascontiguousarray(color, dtype=F)
    var3 = np.ascontiguousarray(variance, dtype=F)
    h, w = c.shape[:2]
    sc, sn, sa, sd = F(sigma_color), F(sigma_normal), F(sigma_albedo), F(sigma_depth)
    zero = np.zeros((h, w), dtype=F)

    def sq3(a, ys, xs):
        d = a - a[ys][:, xs]
        return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]

    def taps(d, s, n):
        q = np.arange(n) + d * s
        return (q >= 0) & (q < n), np.clip(q, 0, n - 1)

    with np.errstate(all="ignore"):
        v = (var3[..., 0] + var3[..., 1]) + var3[..., 2]
        for i in range(iterations):
            s = 1 << i
            gn, gd = np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=F)
            for dy in range(-1, 2):
                vy, ys = taps(dy, 1, h)
                for dx in range(-1, 2):
                    vx, xs = taps(dx, 1, w)
                    valid = vy[:, None] & vx[None, :]
                    k = K3[dy + 1] * K3[dx + 1]
                    gn = np.where(valid, gn + k * v[ys][:, xs], gn)
                    gd = np.where(valid, gd + k, gd)
            n_c = (sc * sc) * (gn / gd) + F(1e-10)
            assert n_c.dtype == F
            num = np.zeros((h, w, 3), dtype=F)
            den = np.zeros((h, w), dtype=F)
            vnum = np.zeros((h, w), dtype=F)
            for dy in range(-2, 3):
                vy, ys = taps(dy, s, h)
                for dx in range(-2, 3):
                    vx, xs = taps(dx, s, w)
                    valid = vy[:, None] & vx[None, :]
                    cq, vq = c[ys][:, xs], v[ys][:, xs]
                    e_c = sq3(c, ys, xs) / n_c
                    e_n = sq3(normal, ys, xs) / (sn * sn) if normal is not None else zero
                    e_a = sq3(albedo, ys, xs) / (sa * sa) if albedo is not None else zero
                    if depth is not None:
                        dq = depth[ys][:, xs]
                        m = np.where(depth > dq, depth, dq)
                        r = (depth - dq) / (sd * m)
                        e_d = np.where(m > 0, r * r, F(0.0))
                    else:
                        e_d = zero
                    wgt = (H5[dy + 2] * H5[dx + 2]) * O.math_fn("exp", -(((e_c + e_n) + e_a) + e_d))
                    assert wgt.dtype == F and e_c.dtype == F
                    num = np.where(valid[..., None], num + cq * wgt[..., None], num)
                    den = np.where(valid, den + wgt, den)
                    vnum = np.where(valid, vnum + vq * (wgt * wgt), vnum)
            c = num / den[..., None]
            v = vnum / (den * den)
    assert c.dtype == F and v.dtype == F
    return c, v


def check_against_restatement(color, variance, where, want_rgb=True, **kw):
    rgb, mean, var = crt.denoise_var(color, variance, want_rgb=want_rgb, want_variance=True, **kw)
    want_mean, want_var = restated(color, variance, **kw)
    assert_bits(mean, want_mean, where + ": mean")
    assert_bits(var, want_var, where + ": variance")
    if want_rgb:
        assert np.array_equal(rgb, O.tonemap(mean)), where + ": rgb is not the tone map of the mean"
    return rgb, mean, var


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_denoise_var_defaults():
    lib = capi.lib()
    p = capi.DenoiseParams(7, 7, 7, -1.0, -1.0, -1.0, -1.0)
    assert lib.crt_denoise_var_defaults(C.byref(p)) == capi.CRT_OK
    assert p.iterations == 3 and (p.width, p.height) == (0, 0)
    for name in ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"):
        assert F(getattr(p, name)) == F(DEFAULTS[name]), name
    assert crt.denoise_var_defaults() == {k: (v if k == "iterations" else float(F(v))) for k, v in DEFAULTS.items()}
    assert lib.crt_denoise_var_defaults(None) == capi.ERR_INVALID_ARG and lib.crt_last_error()
    assert crt.denoise_defaults()["sigma_color"] == 4.0       # the plain filter keeps its own


def test_denoise_var_arguments_are_checked_before_any_device_call():
    """Every invalid call is CRT_ERR_INVALID_ARG, also on a machine without a GPU: the arguments are checked first.  The non-null
    buffers here are dummies that must never be dereferenced."""
    lib = capi.lib()
    dummy = C.create_string_buffer(256)
    d = C.cast(dummy, C.c_void_p)
    w, h = 64, 48
    need = crt.denoise_scratch_bytes(w, h)

    def params(**over):
        p = capi.DenoiseParams()
        assert lib.crt_denoise_var_defaults(C.byref(p)) == capi.CRT_OK
        p.width, p.height = w, h
        for k, v in over.items():
            setattr(p, k, v)
        return C.byref(p)

    def inputs(color=d, variance=d):
        return C.byref(capi.DenoiseVarInputs(color, variance, d, d, d))

    def both(prm, inp, mean=d, rgb=d):
        r1 = lib.crt_denoise_var(0, prm, inp, mean, rgb, d, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_denoise_var_device(0, prm, inp, mean, rgb, d, d, need, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == capi.ERR_INVALID_ARG, (r1, r2, e1, e2)
        assert e1 and e2
        return e1

    assert b"null" in both(None, inputs())
    assert b"null" in both(params(), None)
    assert b"null" in both(params(), inputs(color=None))
    assert b"variance" in both(params(), inputs(variance=None))
    both(params(width=0), inputs())
    both(params(height=0), inputs())
    assert b"iterations" in both(params(iterations=0), inputs())
    assert b"iterations" in both(params(iterations=6), inputs())
    for name in ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"):
        for bad in (0.0, -0.0, -1.0, float("nan"), float("-inf")):
            assert b"sigma" in both(params(**{name: bad}), inputs()), (name, bad)
    assert b"sigma_color" in both(params(sigma_color=float("inf")), inputs())
    assert b"no output" in both(params(), inputs(), mean=None, rgb=None)
    for scratch, size in ((None, need), (d, need - 1), (d, 0), (C.c_void_p(d.value + 4), need)):
        assert lib.crt_denoise_var_device(0, params(), inputs(), d, d, d, scratch, size, None, None) == capi.ERR_INVALID_ARG
        assert b"scratch" in lib.crt_last_error()
    assert lib.crt_denoise_var(-1, params(), inputs(), d, d, d, None) == capi.ERR_INVALID_ARG


def test_restatement_reduces_to_a_gaussian_of_the_variance_where_nothing_stops_it():
    """The restated contract on an input whose weights are known in closed form (no device): constant colour and no guides make every
    weight h x h, so one pass leaves the colour and turns a constant variance V into V x sum(w^2) / sum(w)^2 = V x (35/128)^2 inside."""
    color = np.full((16, 16, 3), 2.0, dtype=F)
    variance = np.full((16, 16, 3), 1.0, dtype=F)
    mean, var = restated(color, variance, iterations=1)
    assert np.array_equal(mean, color)
    assert np.allclose(var[4:12, 4:12], 3.0 * (35.0 / 128.0) ** 2, rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------------ GPU --

def frame_and_guides(r, name, width, height, spp, seed=0):
    """(rgb, mean, variance, {albedo, normal, depth}) of a GPU render with the flag and its AOV pass"""
    f = gpu_frame(r, name, width, height, spp, seed=seed, want_variance=True, aov=GUIDES)
    return f["rgb"], f["mean"], f["variance"], {k: f[k] for k in GUIDES}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_denoise_var_rendered_frames_match_restatement(renders, name):
    """64 x 48: the spacing-16 taps of pass 4 leave the image from every pixel, so border skipping is exercised."""
    _, mean, var, g = frame_and_guides(renders[name], name, 64, 48, 4)
    assert (g["depth"] > 0).any() and (var > 0).any()
    for it in range(1, 6):
        check_against_restatement(mean, var, "%s 64x48 iterations %d" % (name, it), iterations=it, **g)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
@pytest.mark.parametrize("size", [(100, 70), (61, 47)])
def test_denoise_var_ragged_sizes_match_restatement(renders, name, size):
    _, mean, var, g = frame_and_guides(renders[name], name, size[0], size[1], 4)
    check_against_restatement(mean, var, "%s %dx%d" % (name, size[0], size[1]), iterations=3, **g)


def synthetic(w, h, seed):
    rng = np.random.default_rng(seed)
    color = (rng.random((h, w, 3)) * 100).astype(F)
    n = rng.normal(size=(h, w, 3))
    normal = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(F)
    albedo = rng.random((h, w, 3)).astype(F)
    depth = (F(50.0) - rng.random((h, w)).astype(F) * F(50.0)).astype(F)  # (0, 50]
    assert (depth > 0).all() and (depth <= 50).all()
    depth[h // 3:h // 3 + 9, w // 4:w // 4 + 13] = 0.0                     # a block of "miss" pixels
    # smooth regions too, so that not every weight underflows: a constant patch in every guide and the colour
    color[2:20, 3:30] = color[2, 3] + (rng.random((18, 27, 3)) * 2).astype(F)
    normal[0:24, 0:40] = normal[0, 0]
    albedo[0:24, 0:40] = albedo[0, 0]
    depth[0:10, 0:40] = depth[0, 0]
    variance = (rng.random((h, w, 3)) * 300).astype(F)
    variance[5:16, 8:22] = 0.0                                             # a block of zero variance inside the smooth patch
    variance[h - 8:, w - 11:] = 0.0                                        # ... and one in the noise, at the corner
    return color, variance, {"albedo": albedo, "normal": normal, "depth": depth}


@pytest.mark.gpu
@pytest.mark.parametrize("drop", [(), ("albedo",), ("normal",), ("depth",), ("albedo", "normal", "depth")])
def test_denoise_var_synthetic_inputs_with_null_guides(drop):
    color, variance, g = synthetic(70, 45, 11)
    assert (g["depth"] == 0).any() and (variance.sum(axis=2) == 0).any()
    kw = {k: v for k, v in g.items() if k not in drop}
    _, mean, var = check_against_restatement(color, variance, "synthetic without %r" % (drop,), iterations=4, **kw)
    assert np.isfinite(mean).all() and not np.array_equal(mean, color)
    assert np.isfinite(var).all() and (var >= 0).all()


@pytest.mark.gpu
def test_denoise_var_non_finite_pixels():
    color, variance, g = synthetic(70, 45, 12)
    bad_c, bad_v = color.copy(), variance.copy()
    bad_c[7, 9, 1] = np.inf
    bad_c[30, 50, 0] = np.nan
    _, m1, v1 = check_against_restatement(bad_c, variance, "inf and NaN colours", iterations=3, **g)
    assert np.isnan(m1).any() and np.isfinite(m1).any()
    bad_v[12, 40, 2] = np.inf
    bad_v[25, 20, 0] = np.nan
    bad_v[33, 60, 1] = -5.0
    _, m2, v2 = check_against_restatement(color, bad_v, "inf, NaN and negative variances", iterations=3, want_rgb=False, **g)
    assert np.isnan(v2).any() and np.isfinite(v2).any() and np.isfinite(m2).any()


@pytest.mark.gpu
def test_denoise_var_with_a_constant_variance_is_crt_denoise(renders):
    """Against the kernel that is verified already, one pass.  With variance (0.25, 0, 0) in every pixel g(p) is exactly 0.25 (the 3x3
    weights and their partial sums are multiples of 1/16: nothing rounds), n_c = 36 x 0.25 + 1e-10f rounds to 9 = 3 x 3, so
    crt_denoise_var(sigma_color 6) is crt_denoise(sigma_color 3) bit for bit; the filtered variance is 0.25 x sum(w^2) / sum(w)^2: at most
    0.25, and below it wherever a second tap has weight (in fp32: a weight that is not lost against the centre's)."""
    name = "cornell-box"
    _, mean, _, g = frame_and_guides(renders[name], name, 100, 70, 4)
    s_color, _, s_g = synthetic(70, 45, 13)
    for where, color, guides in (("rendered", mean, g), ("synthetic", s_color, s_g)):
        variance = np.zeros(color.shape, dtype=F)
        variance[..., 0] = 0.25
        rgb, got, var = crt.denoise_var(color, variance, iterations=1, sigma_color=6.0, want_variance=True, **guides)
        want_rgb, want = crt.denoise(color, iterations=1, sigma_color=3.0, **guides)
        assert_bits(got, want, where)
        assert np.array_equal(rgb, want_rgb)
        assert (var <= F(0.25)).all() and (var > 0).all(), where
        # "a second tap has weight", observed from outside: got - c = sum_i w_i (c_i - c) / sum(w), so a mean that moved by more than
        # 1e-3 x M, M the largest |colour| among the 25 taps, has more than 5e-4 of its weight on the other taps, and
        # sum(w^2) / sum(w)^2 <= f^2 + (1 - f)^2 with f < 1 - 5e-4 is below 1 by 1e-3: far beyond the rounding of 25 fp32 sums
        a = np.abs(color).max(axis=2)
        pad = np.pad(a, 2, mode="edge")
        M = np.max([pad[dy:dy + a.shape[0], dx:dx + a.shape[1]] for dy in range(5) for dx in range(5)], axis=0)
        moved = np.abs(got - color).max(axis=2) > F(1e-3) * M
        assert moved.sum() > moved.size // 10 and (var[moved] < F(0.25)).all(), where


@pytest.mark.gpu
def test_denoise_var_does_not_filter_across_a_normal_edge():
    """Independent of the restatement, one pass (from the second on g(p) reads the spacing-1 neighbours whatever their guides say):
    normals (1,0,0) | (-1,0,0) with sigma_normal 0.2 give e_n = 4 / 0.04 = 100 > 87, so the weight of every tap across the edge is
    exactly 0; with the same variance everywhere, the left half's mean and variance cannot depend on the right half's colours."""
    w, h = 64, 40
    rng = np.random.default_rng(3)
    color = (rng.random((h, w, 3)) * 100).astype(F)
    other = color.copy()
    other[:, w // 2:] = (rng.random((h, w // 2, 3)) * 100).astype(F)
    variance = (rng.random((h, w, 3)) * 300).astype(F)
    normal = np.zeros((h, w, 3), dtype=F)
    normal[:, :w // 2, 0], normal[:, w // 2:, 0] = 1.0, -1.0
    g = {"normal": normal, "albedo": np.full((h, w, 3), 0.5, dtype=F), "depth": np.full((h, w), 3.0, dtype=F)}
    kw = dict(iterations=1, sigma_normal=0.2, want_rgb=False, want_variance=True)
    _, a, va = crt.denoise_var(color, variance, **g, **kw)
    _, b, vb = crt.denoise_var(other, variance, **g, **kw)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    left = slice(0, w // 2)
    assert np.array_equal(a[:, left].view(np.uint32), b[:, left].view(np.uint32))
    assert np.array_equal(va[:, left].view(np.uint32), vb[:, left].view(np.uint32))
    assert not np.array_equal(a[:, w // 2:], b[:, w // 2:])
    assert not np.array_equal(a[:, left], color[:, left])          # ... and the halves are filtered within themselves


@pytest.mark.gpu
def test_denoise_var_device_form_on_a_stream_matches_host_form(renders):
    name, w, h, it = "veach-mis", 100, 70, 4
    _, mean, variance, g = frame_and_guides(renders[name], name, w, h, 4)
    want_rgb, want_mean, want_var = crt.denoise_var(mean, variance, iterations=it, want_variance=True, **g)
    scratch_bytes = crt.denoise_scratch_bytes(w, h)
    host = {"color": mean, "variance": variance, "albedo": g["albedo"], "normal": g["normal"], "depth": g["depth"]}
    outs = {"out_mean": w * h * 12, "out_rgb": w * h * 3, "out_var": w * h * 4}
    # (every output value must be written by the filter: what is not uploaded is filled with 0x55)
    with DeviceBuffers({**host, **outs, "scratch": scratch_bytes}, stream=True) as d:
        ptrs = d.ptrs

        def run(want_info, out_mean=True, out_rgb=True, out_var=True):
            return crt.denoise_var_device(w, h, ptrs["color"], ptrs["variance"], ptrs["out_mean"] if out_mean else None,
                                          ptrs["out_rgb"] if out_rgb else None, ptrs["out_var"] if out_var else None, ptrs["scratch"],
                                          scratch_bytes, albedo_ptr=ptrs["albedo"], normal_ptr=ptrs["normal"], depth_ptr=ptrs["depth"],
                                          iterations=it, stream=d.stream, want_info=want_info)

        def fetch():
            return d.download("out_mean", (h, w, 3), F), d.download("out_rgb", (h, w, 3), np.uint8), d.download("out_var", (h, w), F)

        assert run(False) is None
        d.synchronize()
        m, r, v = fetch()
        assert_bits(m, want_mean, "device form")
        assert_bits(v, want_var, "device form, variance")
        assert np.array_equal(r, want_rgb)
        # the mean only, with the timer (the call synchronizes the stream)
        for n in outs:
            d.fill(n)
        info = run(True, out_rgb=False, out_var=False)
        assert info["passes"] == it and info["total_ms"] > 0, info
        m, r, v = fetch()
        assert_bits(m, want_mean, "device form, mean only")
        assert (r == 0x55).all() and (v.view(np.uint32) == 0x55555555).all()


@pytest.mark.gpu
def test_run_view_denoised_variance_guided_equals_the_four_calls_by_hand(renders):
    name, w, h = "cornell-box", 96, 72
    r = renders[name]
    eye, iv, fov = util.camera(name)
    rgb0, mean0, var0, g = frame_and_guides(r, name, w, h, 4)
    want_rgb, want_mean = crt.denoise_var(mean0, var0, **g)
    r.set_spp(4)
    rgb, mean = r.run_view_denoised(eye, iv, fov, width=w, height=h, variance_guided=True)
    assert_bits(mean, want_mean, "run_view_denoised")
    assert np.array_equal(rgb, want_rgb)
    assert np.array_equal(r.frame_buffer, rgb0) and r.denoise_info["passes"] == 3
    assert_bits(r.variance_buffer, var0, "variance_buffer")
    rgb2, mean2 = r.run_view_denoised(eye, iv, fov, iterations=2, sigma_color=4.5, width=w, height=h, variance_guided=True)
    assert_bits(mean2, crt.denoise_var(mean0, var0, iterations=2, sigma_color=4.5, **g)[1], "run_view_denoised with overrides")
    # the plain form is what it was, and so is a following render
    rgb3, mean3 = r.run_view_denoised(eye, iv, fov, width=w, height=h)
    assert_bits(mean3, crt.denoise(mean0, **g)[1], "plain run_view_denoised")
    assert r.variance_buffer is None
    assert np.array_equal(r.run_view(eye, iv, fov, width=w, height=h), rgb0)
    assert np.array_equal(r.mean_buffer.view(np.uint32), mean0.view(np.uint32))


@pytest.mark.gpu
def test_cli_writes_the_variance_guided_frame(renders, tmp_path):
    from PIL import Image
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    cfg = util.SCENES["veach-mis"]
    base = [cli, cfg, "--spp", "4", "--width", "96", "--height", "72", "--seed", "42", "--base-dir", util.ROOT]
    noisy, den, den2, plain = (str(tmp_path / n) for n in ("noisy.png", "den.png", "den2.png", "plain.png"))
    res = subprocess.run(base + ["-o", noisy, "--denoise", den, "--denoise-variance"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    rgb, mean, var, g = frame_and_guides(renders["veach-mis"], "veach-mis", 96, 72, 4, seed=42)
    assert np.array_equal(np.asarray(Image.open(noisy)), rgb)
    assert np.array_equal(np.asarray(Image.open(den)), crt.denoise_var(mean, var, **g)[0])
    res = subprocess.run(base + ["-o", noisy, "--denoise", den2, "--denoise-variance", "--denoise-iterations", "2", "--denoise-sigma", "5,0.25,0.2,0.1"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    want = crt.denoise_var(mean, var, iterations=2, sigma_color=5, sigma_normal=0.25, sigma_albedo=0.2, sigma_depth=0.1, **g)[0]
    assert np.array_equal(np.asarray(Image.open(den2)), want)
    # without the switch --denoise is the plain filter with its own defaults
    res = subprocess.run(base + ["-o", noisy, "--denoise", plain], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert np.array_equal(np.asarray(Image.open(plain)), crt.denoise(mean, **g)[0])
    bad = subprocess.run([cli, cfg, "--devices", "0,0", "--gather", "copy", "--denoise-variance"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--denoise-variance" in bad.stderr
    bad = subprocess.run([cli, cfg, "--gpus", "2", "--denoise-variance"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--denoise-variance" in bad.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_variance_guided_defaults_beat_the_plain_defaults_against_a_converged_frame(renders, name):
    """160 x 120: N = spp 8, seed 0; R = spp 256, seed 7; mse on the RGB8 tone maps, as test_denoise_reduces_the_error_against_a_converged_frame.
    The variance-guided defaults must give a strictly smaller error than crt_denoise's defaults on the same frame.  The numpy prototype
    of the two contracts measured, noisy / plain / variance-guided: cornell-box 964.5 / 169.3 / 159.9, veach-mis 351.5 / 149.6 / 112.1."""
    r = renders[name]
    noisy_rgb, noisy_mean, noisy_var, g = frame_and_guides(r, name, 160, 120, 8, seed=0)
    ref_rgb = frame_and_guides(r, name, 160, 120, 256, seed=7)[0]
    plain_rgb, _ = crt.denoise(noisy_mean, **g)
    var_rgb, _ = crt.denoise_var(noisy_mean, noisy_var, **g)

    def mse(x):
        d = x.astype(np.float64) - ref_rgb.astype(np.float64)
        return float(np.mean(d * d))

    print("%s: mse noisy %.1f, crt_denoise defaults %.1f, crt_denoise_var defaults %.1f" % (name, mse(noisy_rgb), mse(plain_rgb), mse(var_rgb)))
    assert mse(var_rgb) < mse(plain_rgb)
