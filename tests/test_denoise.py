"""AOV-guided edge-avoiding a-trous denoiser (crt_denoise / crt_denoise_device, include/crt.h; denoise and Render.run_view_denoised
in Python; crt_cli --denoise).

The contract of include/crt.h is restated below in numpy float32, operation by operation, with the oracle's det_expf
(oracle_lib.math_fn("exp")) and tone map (oracle_lib.tonemap); the device result must match it bit for bit.  Comparisons are on uint32
views; where the expected value is NaN the result must be NaN (payload not compared).
"""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import oracle_lib as O
import util
from frames import GUIDES, gpu_frame, renders  # noqa: F401

DENOISE_EXPORTS = ("crt_denoise_defaults", "crt_denoise_scratch_bytes", "crt_denoise", "crt_denoise_device")
DEFAULTS = {"iterations": 3, "sigma_color": 4.0, "sigma_normal": 0.5, "sigma_albedo": 0.1, "sigma_depth": 0.05}
H5 = np.array([1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16], dtype=np.float32)
F = np.float32
assert_bits = util.assert_bits


def restated(color, albedo=None, normal=None, depth=None, iterations=3, sigma_color=4.0, sigma_normal=0.5, sigma_albedo=0.1,
             sigma_depth=0.05):
    """The contract, in numpy float32: every ufunc below is one IEEE fp32 operation per element."""
    c = np.ascontiguousarray(color, dtype=F)
    h, w = c.shape[:2]
    sn, sa, sd = F(sigma_normal), F(sigma_albedo), F(sigma_depth)
    zero = np.zeros((h, w), dtype=F)

    def sq3(a, ys, xs):
        d = a - a[ys][:, xs]
        return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]

    with np.errstate(all="ignore"):
        for i in range(iterations):
            s = 1 << i
            sig = F(sigma_color) / F(1 << i)
            num = np.zeros((h, w, 3), dtype=F)
            den = np.zeros((h, w), dtype=F)
            for dy in range(-2, 3):
                yq = np.arange(h) + dy * s
                vy = (yq >= 0) & (yq < h)
                ys = np.clip(yq, 0, h - 1)
                for dx in range(-2, 3):
                    xq = np.arange(w) + dx * s
                    vx = (xq >= 0) & (xq < w)
                    xs = np.clip(xq, 0, w - 1)
                    valid = vy[:, None] & vx[None, :]
                    cq = c[ys][:, xs]
                    e_c = sq3(c, ys, xs) / (sig * sig)
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
            c = num / den[..., None]
    assert c.dtype == F
    return c


def check_against_restatement(color, where, want_rgb=True, **kw):
    rgb, mean = crt.denoise(color, want_rgb=want_rgb, **kw)
    want = restated(color, **kw)
    assert_bits(mean, want, where)
    if want_rgb:
        assert np.array_equal(rgb, O.tonemap(mean)), where + ": rgb is not the tone map of the mean"
    return rgb, mean


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_denoise_entry_points_are_exported():
    lib = capi.lib()
    for name in DENOISE_EXPORTS:
        assert name in capi.EXPORTS
        getattr(lib, name)
    lib.crt_abi_version.restype = C.c_int
    assert lib.crt_abi_version() == 5 == capi.ABI_VERSION
    for name in ("denoise", "denoise_device", "denoise_defaults", "denoise_scratch_bytes"):
        assert hasattr(crt, name)
    assert hasattr(crt.Render, "run_view_denoised")


def test_denoise_defaults_and_scratch_size():
    lib = capi.lib()
    p = capi.DenoiseParams(7, 7, 7, -1.0, -1.0, -1.0, -1.0)
    assert lib.crt_denoise_defaults(C.byref(p)) == capi.CRT_OK
    assert p.iterations == 3 and (p.width, p.height) == (0, 0)
    for name in ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"):
        assert F(getattr(p, name)) == F(DEFAULTS[name]), name
    assert crt.denoise_defaults() == {k: (v if k == "iterations" else float(F(v))) for k, v in DEFAULTS.items()}
    assert lib.crt_denoise_defaults(None) == capi.ERR_INVALID_ARG
    sizes = [crt.denoise_scratch_bytes(w, h) for w, h in ((1, 1), (61, 47), (64, 48), (800, 600), (3840, 2160))]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert all(b >= 16 * w * h for b, (w, h) in zip(sizes, ((1, 1), (61, 47), (64, 48), (800, 600), (3840, 2160))))
    n = C.c_uint64()
    assert lib.crt_denoise_scratch_bytes(0, 4, C.byref(n)) == capi.ERR_INVALID_ARG
    assert lib.crt_denoise_scratch_bytes(4, 0, C.byref(n)) == capi.ERR_INVALID_ARG
    assert lib.crt_denoise_scratch_bytes(4, 4, None) == capi.ERR_INVALID_ARG


def test_denoise_arguments_are_checked_before_any_device_call():
    """Every invalid call is CRT_ERR_INVALID_ARG, also on a machine without a GPU: the arguments are checked first.  The non-null
    buffers here are dummies that must never be dereferenced."""
    lib = capi.lib()
    dummy = C.create_string_buffer(256)
    d = C.cast(dummy, C.c_void_p)
    w, h = 64, 48
    need = crt.denoise_scratch_bytes(w, h)

    def params(**over):
        p = capi.DenoiseParams()
        assert lib.crt_denoise_defaults(C.byref(p)) == capi.CRT_OK
        p.width, p.height = w, h
        for k, v in over.items():
            setattr(p, k, v)
        return C.byref(p)

    def inputs(color=d):
        return C.byref(capi.DenoiseInputs(color, d, d, d))

    def both(prm, inp, mean=d, rgb=d):
        r1 = lib.crt_denoise(0, prm, inp, mean, rgb, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_denoise_device(0, prm, inp, mean, rgb, d, need, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == capi.ERR_INVALID_ARG, (r1, r2, e1, e2)
        assert e1 and e2
        return e1

    assert b"null" in both(None, inputs())
    assert b"null" in both(params(), None)
    assert b"null" in both(params(), inputs(color=None))
    both(params(width=0), inputs())
    both(params(height=0), inputs())
    assert b"iterations" in both(params(iterations=0), inputs())
    assert b"iterations" in both(params(iterations=6), inputs())
    for name in ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"):
        for bad in (0.0, -0.0, -1.0, float("nan"), float("-inf")):
            assert b"sigma" in both(params(**{name: bad}), inputs()), (name, bad)
    assert b"no output" in both(params(), inputs(), mean=None, rgb=None)
    # the device form's scratch buffer: missing, one byte short, misaligned
    for scratch, size in ((None, need), (d, need - 1), (d, 0), (C.c_void_p(d.value + 4), need)):
        assert lib.crt_denoise_device(0, params(), inputs(), d, d, scratch, size, None, None) == capi.ERR_INVALID_ARG
        assert b"scratch" in lib.crt_last_error()


# ------------------------------------------------------------------------------------------------------------------ GPU --

def frame_and_guides(r, name, width, height, spp, seed=0):
    """(rgb, mean, {albedo, normal, depth}) of a GPU render and its AOV pass"""
    f = gpu_frame(r, name, width, height, spp, seed=seed, aov=GUIDES)
    return f["rgb"], f["mean"], {k: f[k] for k in GUIDES}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_denoise_rendered_frames_match_restatement(renders, name):
    """64 x 48: the spacing-16 taps of pass 4 leave the image from every pixel, so border skipping is exercised."""
    _, mean, g = frame_and_guides(renders[name], name, 64, 48, 4)
    assert (g["depth"] > 0).any()
    for it in range(1, 6):
        check_against_restatement(mean, "%s 64x48 iterations %d" % (name, it), iterations=it, **g)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
@pytest.mark.parametrize("size", [(100, 70), (61, 47)])
def test_denoise_ragged_sizes_match_restatement(renders, name, size):
    _, mean, g = frame_and_guides(renders[name], name, size[0], size[1], 4)
    check_against_restatement(mean, "%s %dx%d" % (name, size[0], size[1]), iterations=3, **g)


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
    return color, {"albedo": albedo, "normal": normal, "depth": depth}


@pytest.mark.gpu
@pytest.mark.parametrize("drop", [(), ("albedo",), ("normal",), ("depth",), ("albedo", "normal", "depth")])
def test_denoise_synthetic_inputs_with_null_guides(drop):
    color, g = synthetic(70, 45, 11)
    kw = {k: v for k, v in g.items() if k not in drop}
    _, mean = check_against_restatement(color, "synthetic without %r" % (drop,), iterations=4, **kw)
    assert np.isfinite(mean).all() and not np.array_equal(mean, color)


@pytest.mark.gpu
def test_denoise_infinite_colour_sigma_and_non_finite_pixels():
    color, g = synthetic(70, 45, 12)
    _, mean = check_against_restatement(color, "sigma_color inf", iterations=3, sigma_color=math.inf, **g)
    assert np.isfinite(mean).all()
    _, m2 = check_against_restatement(color, "all sigmas inf", iterations=2, sigma_color=math.inf, sigma_normal=math.inf,
                                      sigma_albedo=math.inf, sigma_depth=math.inf, want_rgb=False, **g)
    assert np.isfinite(m2).all()
    bad = color.copy()
    bad[7, 9, 1] = np.inf
    bad[30, 50, 0] = np.nan
    _, m3 = check_against_restatement(bad, "inf and NaN pixels", iterations=3, **g)
    assert np.isnan(m3).any() and np.isfinite(m3).any()


@pytest.mark.gpu
@pytest.mark.parametrize("sigma_color", [None, 1e6])
def test_denoise_does_not_filter_across_a_normal_edge(sigma_color):
    """Independent of the restatement: normals (1,0,0) | (-1,0,0) with sigma_normal 0.2 give e_n = 4 / 0.04 = 100 > 87, so the weight of
    every tap across the edge is exactly 0 and the left half's result cannot depend on the right half's colours.  With the default
    sigma_color, and with one so wide that the colour term stops nothing."""
    w, h = 64, 40
    rng = np.random.default_rng(3)
    color = (rng.random((h, w, 3)) * 100).astype(F)
    other = color.copy()
    other[:, w // 2:] = (rng.random((h, w // 2, 3)) * 100).astype(F)
    normal = np.zeros((h, w, 3), dtype=F)
    normal[:, :w // 2, 0], normal[:, w // 2:, 0] = 1.0, -1.0
    g = {"normal": normal, "albedo": np.full((h, w, 3), 0.5, dtype=F), "depth": np.full((h, w), 3.0, dtype=F)}
    kw = dict(iterations=5, sigma_normal=0.2, sigma_color=sigma_color, want_rgb=False)
    _, a = crt.denoise(color, **g, **kw)
    _, b = crt.denoise(other, **g, **kw)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert np.array_equal(a[:, :w // 2].view(np.uint32), b[:, :w // 2].view(np.uint32))
    assert not np.array_equal(a[:, w // 2:], b[:, w // 2:])
    assert not np.array_equal(a[:, :w // 2], color[:, :w // 2])   # ... and the halves are filtered within themselves


@pytest.mark.gpu
def test_denoise_device_form_on_a_stream_matches_host_form(renders):
    name, w, h, it = "veach-mis", 100, 70, 4
    _, mean, g = frame_and_guides(renders[name], name, w, h, 4)
    want_rgb, want_mean = crt.denoise(mean, iterations=it, **g)
    scratch_bytes = crt.denoise_scratch_bytes(w, h)
    host = {"color": mean, "albedo": g["albedo"], "normal": g["normal"], "depth": g["depth"]}
    # (every output value must be written by the filter: what is not uploaded is filled with 0x55)
    with DeviceBuffers({**host, "out_mean": w * h * 12, "out_rgb": w * h * 3, "scratch": scratch_bytes}, stream=True) as d:
        ptrs = d.ptrs

        def run(want_info, out_mean=True, out_rgb=True):
            return crt.denoise_device(w, h, ptrs["color"], ptrs["out_mean"] if out_mean else None, ptrs["out_rgb"] if out_rgb else None,
                                      ptrs["scratch"], scratch_bytes, albedo_ptr=ptrs["albedo"], normal_ptr=ptrs["normal"],
                                      depth_ptr=ptrs["depth"], iterations=it, stream=d.stream, want_info=want_info)

        def fetch():
            return d.download("out_mean", (h, w, 3), F), d.download("out_rgb", (h, w, 3), np.uint8)

        assert run(False) is None
        d.synchronize()
        m, r = fetch()
        assert_bits(m, want_mean, "device form")
        assert np.array_equal(r, want_rgb)
        # one output only, with the timer (the call synchronizes the stream)
        d.fill("out_mean")
        d.fill("out_rgb")
        info = run(True, out_rgb=False)
        assert info["passes"] == it and info["total_ms"] > 0, info
        m, r = fetch()
        assert_bits(m, want_mean, "device form, mean only")
        assert (r == 0x55).all()


@pytest.mark.gpu
def test_run_view_denoised_equals_the_three_calls_by_hand(renders):
    name, w, h = "cornell-box", 96, 72
    r = renders[name]
    eye, iv, fov = util.camera(name)
    rgb0, mean0, g = frame_and_guides(r, name, w, h, 4)
    want_rgb, want_mean = crt.denoise(mean0, **g)
    r.set_spp(4)
    rgb, mean = r.run_view_denoised(eye, iv, fov, width=w, height=h)
    assert_bits(mean, want_mean, "run_view_denoised")
    assert np.array_equal(rgb, want_rgb)
    assert np.array_equal(r.frame_buffer, rgb0) and r.denoise_info["passes"] == 3
    rgb2, mean2 = r.run_view_denoised(eye, iv, fov, iterations=2, sigma_color=1.5, width=w, height=h)
    assert_bits(mean2, crt.denoise(mean0, iterations=2, sigma_color=1.5, **g)[1], "run_view_denoised with overrides")
    # a following render is what it was
    assert np.array_equal(r.run_view(eye, iv, fov, width=w, height=h), rgb0)
    assert np.array_equal(r.mean_buffer.view(np.uint32), mean0.view(np.uint32))


@pytest.mark.gpu
def test_cli_writes_the_denoised_frame(renders, tmp_path):
    from PIL import Image
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    cfg = util.SCENES["veach-mis"]
    base = [cli, cfg, "--spp", "2", "--width", "96", "--height", "72", "--seed", "42", "--base-dir", util.ROOT]
    plain, noisy, den, den2 = (str(tmp_path / n) for n in ("plain.png", "noisy.png", "den.png", "den2.png"))
    res = subprocess.run(base + ["-o", plain], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    res = subprocess.run(base + ["-o", noisy, "--denoise", den], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert open(plain, "rb").read() == open(noisy, "rb").read()
    _, mean, g = frame_and_guides(renders["veach-mis"], "veach-mis", 96, 72, 2, seed=42)
    assert np.array_equal(np.asarray(Image.open(den)), crt.denoise(mean, **g)[0])
    res = subprocess.run(base + ["-o", noisy, "--denoise", den2, "--denoise-iterations", "2", "--denoise-sigma", "2,0.25,0.2,0.1"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    want = crt.denoise(mean, iterations=2, sigma_color=2, sigma_normal=0.25, sigma_albedo=0.2, sigma_depth=0.1, **g)[0]
    assert np.array_equal(np.asarray(Image.open(den2)), want)
    bad = subprocess.run([cli, cfg, "--devices", "0,0", "--gather", "copy", "--denoise", den], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--denoise" in bad.stderr
    bad = subprocess.run(base + ["--denoise", den, "--denoise-sigma", "1,2,3"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--denoise-sigma" in bad.stderr


@pytest.mark.gpu
def test_multi_render_has_no_denoiser():
    m = crt.MultiRender(util.host_scene("cornell-box"), 2, devices=(0,), gather=crt.GATHER_COPY)
    try:
        eye, iv, fov = util.camera("cornell-box")
        with pytest.raises(NotImplementedError):
            m.run_view_denoised(eye, iv, fov)
    finally:
        m.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name,bound", [("cornell-box", 0.25), ("veach-mis", 0.5)])
def test_denoise_reduces_the_error_against_a_converged_frame(renders, name, bound):
    """160 x 120: N = spp 8, seed 0; R = spp 256, seed 7; D = N filtered with the defaults and N's guides.  mse on the RGB8 tone maps.
    The numpy prototype of the contract measured mse(D) / mse(N) = 0.1756 (964.5 -> 169.3) on cornell-box and 0.4255 (351.5 -> 149.6) on
    veach-mis, whose glossy plates hold it there: the guides see the plate, not its reflection."""
    r = renders[name]
    noisy_rgb, noisy_mean, g = frame_and_guides(r, name, 160, 120, 8, seed=0)
    ref_rgb, _, _ = frame_and_guides(r, name, 160, 120, 256, seed=7)
    den_rgb, _ = crt.denoise(noisy_mean, **g)

    def mse(x):
        d = x.astype(np.float64) - ref_rgb.astype(np.float64)
        return float(np.mean(d * d))

    print("%s: mse noisy %.1f, denoised %.1f, ratio %.4f (bound %.2f)" % (name, mse(noisy_rgb), mse(den_rgb), mse(den_rgb) / mse(noisy_rgb), bound))
    assert mse(den_rgb) <= bound * mse(noisy_rgb)
