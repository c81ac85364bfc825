"""Temporal accumulation with reprojection (crt_temporal / crt_temporal_device, include/crt.h; temporal, temporal_device and
Render.run_view_temporal in Python; crt_cli --temporal).

The contract of include/crt.h is restated in temporal_restated.py in numpy float32, operation by operation, with the oracle's det_tanf
(oracle_lib.math_fn("tan")) for the two camera scales and its tone map (oracle_lib.tonemap); the device result must match it bit for
bit: colour, variance and history length on uint32 views (where the expected value is NaN the result must be NaN).  The restatement
itself is checked against plain geometry on the CPU, and four GPU checks do not use it at all.
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
from frames import renders  # noqa: F401
from temporal_restated import MOVES, as_history, check_branches, frames, plane_colour, plane_setup, restated, subset, synthetic
from util import assert_bits

F = np.float32
DEFAULTS = {"depth_tolerance": 0.05, "normal_tolerance": 0.5, "alpha_min": 0.05}


def check_against_restatement(cur, cam, prev, pcam, where, **kw):
    """crt.temporal against the restatement, bit for bit; returns (rgb, color, variance, history, info, took)"""
    rgb, color, var, hist, info = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, return_info=True, **kw)
    want_c, want_v, want_h, took = restated(cur, cam, prev, pcam, **kw)
    assert_bits(color, want_c, where + ": colour")
    assert_bits(hist, want_h, where + ": history")
    if want_v is None:
        assert var is None
    else:
        assert_bits(var, want_v, where + ": variance")
    assert np.array_equal(rgb, O.tonemap(color)), where + ": rgb is not the tone map of the colour"
    assert info["reprojected"] == int(took.sum()), (where, info, int(took.sum()))
    return rgb, color, var, hist, info, took


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_temporal_entry_points_and_defaults():
    lib = capi.lib()
    for name in ("crt_temporal_defaults", "crt_temporal", "crt_temporal_device"):
        assert name in capi.EXPORTS and getattr(lib, name)
    p = capi.TemporalParams()
    C.memset(C.byref(p), 0x7f, C.sizeof(p))
    assert lib.crt_temporal_defaults(C.byref(p)) == capi.CRT_OK
    assert (p.width, p.height) == (0, 0)
    for cam in (p.cur, p.prev):
        assert list(cam.eye) == [0.0] * 3 and list(cam.inv_view) == [0.0] * 9 and cam.fov_y == 0.0
    for name, v in DEFAULTS.items():
        assert F(getattr(p, name)) == F(v), name
    assert crt.temporal_defaults() == {k: float(F(v)) for k, v in DEFAULTS.items()}
    assert lib.crt_temporal_defaults(None) == capi.ERR_INVALID_ARG and lib.crt_last_error()
    assert lib.crt_abi_version() == 5
    with pytest.raises(NotImplementedError):
        crt.MultiRender.run_view_temporal(None)


def test_temporal_arguments_are_checked_before_any_device_call():
    """Every invalid call of both forms is CRT_ERR_INVALID_ARG, also on a machine without a GPU: the arguments are checked first.  The
    non-null buffers here are dummies that must never be dereferenced."""
    lib = capi.lib()
    dummy = C.create_string_buffer(256)
    d = C.cast(dummy, C.c_void_p)
    w, h = 64, 48

    def params(**over):
        p = capi.TemporalParams()
        assert lib.crt_temporal_defaults(C.byref(p)) == capi.CRT_OK
        p.width, p.height = w, h
        for k, v in over.items():
            setattr(p, k, v)
        return C.byref(p)

    def frame(**over):
        f = dict(color=d, variance=d, depth=d, normal=d, id=d)
        f.update(over)
        return C.byref(capi.TemporalFrame(**f))

    def history(**over):
        f = dict(color=d, variance=d, history=d, depth=d, normal=d, id=d)
        f.update(over)
        return C.byref(capi.TemporalHistory(**f))

    def both(prm, cur, prev, color=d, var=d, hist=d, rgb=d, status=capi.ERR_INVALID_ARG):
        r1 = lib.crt_temporal(0, prm, cur, prev, color, var, hist, rgb, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_temporal_device(0, prm, cur, prev, color, var, hist, rgb, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == status, (r1, r2, e1, e2)
        assert e1 and e2
        return e1

    assert b"null" in both(None, frame(), history())
    assert b"null" in both(params(), None, history())
    for prev in (history(), None):
        both(params(), frame(color=None), prev)
        both(params(), frame(depth=None), prev)
        both(params(), frame(), prev, color=None)
        both(params(), frame(), prev, hist=None)
        both(params(width=0), frame(), prev)
        both(params(height=0), frame(), prev)
        for name in ("depth_tolerance", "normal_tolerance"):
            for bad in (0.0, -0.0, -1.0, float("nan"), float("-inf")):
                assert b"tolerance" in both(params(**{name: bad}), frame(), prev), (name, bad)
        for bad in (0.0, -0.5, 1.5, float("nan"), float("inf")):
            assert b"alpha_min" in both(params(alpha_min=bad), frame(), prev), bad
        assert b"variance" in both(params(), frame(variance=None), prev)            # out_variance without the current variance
        assert b"variance" in both(params(), frame(), prev, var=None)               # ... and the other way round
    for missing in ("color", "history", "depth"):
        assert b"history" in both(params(), frame(), history(**{missing: None})), missing
    assert b"variance" in both(params(), frame(), history(variance=None))
    assert b"normals" in both(params(), frame(normal=None), history())
    assert b"normals" in both(params(), frame(), history(normal=None))
    assert b"IDs" in both(params(), frame(id=None), history())
    assert b"IDs" in both(params(), frame(), history(id=None))
    # sizes the launch cannot cover: the denoiser's answer
    both(params(width=(1 << 24) + 1), frame(), history(), status=capi.ERR_UNSUPPORTED)
    both(params(width=1 << 24, height=1 << 24), frame(), history(), status=capi.ERR_UNSUPPORTED)
    assert lib.crt_temporal(-1, params(), frame(), history(), d, d, d, d, None) == capi.ERR_INVALID_ARG
    assert lib.crt_temporal_device(-1, params(), frame(), history(), d, d, d, d, None, None) == capi.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        crt.temporal({"color": np.zeros((4, 4, 3), F), "depth": np.zeros((4, 5), F)}, (np.zeros(3), np.zeros(9), 1.0))


@pytest.mark.parametrize("size", [(64, 48), (61, 47)])
@pytest.mark.parametrize("move", [(10, 0, 0), (7.3, -4.1, 0), (3, 2, 15), (0, 0, -20)])
def test_restatement_reprojects_a_plane(size, move):
    """The restated contract against geometry (no device).  A colour that is linear in world x and y on a plane parallel to the image
    plane is linear in the previous frame's pixel coordinates, so its bilinear interpolation at the reprojected point is the colour of
    the pixel's own world point.  History length 10^6 with alpha_min 2^-20 and a current colour of 0: output = history x k with k within
    2^-24 of 1 - 2^-20.  Bound 1e-5 relative; measured at most 2.9e-7 with the prototype of the contract."""
    W, H = size
    pcam, pdepth, pP = plane_setup(W, H, (0, 0, 0))
    cam, depth, P = plane_setup(W, H, move)
    prev = {"color": plane_colour(pP).astype(F), "history": np.full((H, W), 1e6, dtype=F), "depth": pdepth.astype(F)}
    cur = {"color": np.zeros((H, W, 3), dtype=F), "depth": depth.astype(F)}
    out, var, hist, took = restated(cur, cam, prev, pcam, alpha_min=2.0 ** -20)
    assert var is None
    # where the point lands in the previous frame, in float64 and from the world point alone
    scale = np.tan(np.float64(pcam[2]) / 2)
    c = (P - pcam[0].astype(np.float64)) @ pcam[1].astype(np.float64).reshape(3, 3).T      # (cx: inv_view'[0..2] . v, ...)
    fx = ((-c[..., 0] / c[..., 2]) / (scale * W / H) + 1) * W / 2 - 0.5
    fy = (1 - (c[..., 1] / c[..., 2]) / scale) * H / 2 - 0.5
    eps = 1e-4                                          # (off the frame by more than the fp32 rounding of fx and fy)
    inside = (fx >= 0) & (fx <= W - 1) & (fy >= 0) & (fy <= H - 1)
    off = (fx < -1 - eps) | (fx > W + eps) | (fy < -1 - eps) | (fy > H + eps)
    assert inside.sum() > W * H // 4
    assert took[inside].all() and (np.abs(hist[inside] - 1e6) < 2).all()       # (the weighted mean of 10^6s, to rounding, + 1)
    want = plane_colour(P)
    rel = np.abs(out.astype(np.float64) / (1 - 2.0 ** -20) - want) / np.abs(want)
    print("%dx%d move %r: %d pixels inside, largest relative error %.3g; %d off the frame" % (W, H, move, inside.sum(), rel[inside].max(), off.sum()))
    assert rel[inside].max() < 1e-5
    if move != (3, 2, 15):                              # (moving forward, every pixel stays in the previous frame)
        assert off.sum() >= H
    assert not took[off].any()
    assert np.array_equal(out[off].view(np.uint32), cur["color"][off].view(np.uint32)) and (hist[off] == F(1)).all()


def test_cli_refuses_temporal_options_it_cannot_combine():
    """Exit status 1 and a message that names the option, before any device is touched."""
    from cudaraytracing_amd import build as b
    cli, cfg = b.build_cli(), util.SCENES["veach-mis"]
    for extra in (["--gpus", "2"], ["--devices", "0,0", "--gather", "copy"], ["--adaptive", "0.05"]):
        bad = subprocess.run([cli, cfg, "--base-dir", util.ROOT, "--temporal", "2"] + extra, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "--temporal" in bad.stderr and extra[0][:6] in bad.stderr, (extra, bad.stderr)
    for args in (["--temporal-out", "x.png"], ["--temporal-step", "1,0,0"], ["--temporal-denoise"], ["--temporal", "2", "--temporal-denoise"],
                 ["--temporal", "0"], ["--temporal", "2", "--temporal-step", "1,2"]):
        bad = subprocess.run([cli, cfg, "--base-dir", util.ROOT] + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "--temporal" in bad.stderr, (args, bad.stderr)


# ------------------------------------------------------------------------------------------------------------------ GPU --


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["full", "no guides", "no variance"])
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_temporal_rendered_frames_match_restatement(renders, name, variant):
    """Three chained frames of a moving camera: the third frame's history is itself an output."""
    fr = frames(renders, name, 64, 48, 3, 40)
    prev = pcam = None
    for f, (cur, _, _, cam) in enumerate(fr):
        cur = subset(cur, variant)
        where = "%s 64x48 %s frame %d" % (name, variant, f)
        _, color, var, hist, _, took = check_against_restatement(cur, cam, prev, pcam, where)
        if f:
            check_branches(cur, took, where)
            assert abs(hist.max() - (f + 1)) < 1e-4
        else:
            assert not took.any() and (hist == 1).all()
        prev, pcam = as_history(cur, color, var, hist), cam


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(61, 47), (100, 70)])
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_temporal_ragged_sizes_match_restatement(renders, name, size):
    (c0, _, _, cam0), (c1, _, _, cam1) = frames(renders, name, size[0], size[1], 2, 50)
    prev = as_history(c0, c0["color"], c0["variance"], np.ones(c0["depth"].shape, dtype=F))
    took = check_against_restatement(c1, cam1, prev, cam0, "%s %dx%d" % (name, size[0], size[1]))[5]
    assert took.sum() >= 100


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["full", "no guides", "no variance"])
def test_temporal_synthetic_inputs(variant):
    cur, cam, prev, pcam = synthetic(70, 45, 21)
    cur, prev = subset(cur, variant), subset(prev, variant)
    _, color, var, hist, _, took = check_against_restatement(cur, cam, prev, pcam, "synthetic " + variant)
    check_branches(cur, took, "synthetic " + variant)
    assert not took[cur["depth"] == 0].any()
    assert not took[:, :2].any() or not took[:, -2:].any()                 # a band of pixels leaves the frame on one side
    assert np.isfinite(color).all() and (hist[took] > 1).all()
    # the tolerances switched off: every pixel that lands in the frame on a hit takes the history
    inf = float("inf")
    took2 = check_against_restatement(cur, cam, prev, pcam, "synthetic, no tests, " + variant, depth_tolerance=inf, normal_tolerance=inf,
                                      alpha_min=1.0)[5]
    assert took2.sum() > took.sum()


@pytest.mark.gpu
def test_temporal_non_finite_pixels():
    cur, cam, prev, pcam = synthetic(70, 45, 22)
    cur["color"][7, 9, 1] = np.inf
    cur["color"][30, 50, 0] = np.nan
    prev["color"][12, 33, 2] = np.inf
    prev["color"][25, 20, 0] = np.nan
    cur["depth"][20, 40] = np.inf
    cur["depth"][21, 44] = np.nan
    prev["depth"][10, 20] = np.inf
    prev["depth"][35, 50] = np.nan
    prev["variance"][18, 28, 1] = np.inf
    prev["variance"][31, 41, 0] = np.nan
    prev["variance"][5, 60, 2] = -5.0
    inf = float("inf")
    for kw in ({}, {"depth_tolerance": inf, "normal_tolerance": inf}):      # (with the tests off, every planted tap counts)
        _, color, var, hist, _, took = check_against_restatement(cur, cam, prev, pcam, "non-finite %r" % (kw,), **kw)
        assert not took[20, 40] and not took[21, 44]
        assert np.isnan(color).any() and np.isfinite(color).any() and np.isfinite(hist).all()
    assert np.isnan(var).any() and np.isinf(color).any()


def assert_is_current_frame(out, cur, where):
    rgb, color, var, hist, info = out
    assert np.array_equal(color.view(np.uint32), cur["color"].view(np.uint32)), where
    assert np.array_equal(var.view(np.uint32), cur["variance"].view(np.uint32)), where
    assert (hist == F(1)).all() and info["reprojected"] == 0, where
    assert np.array_equal(rgb, O.tonemap(cur["color"])), where


@pytest.mark.gpu
def test_temporal_without_a_usable_history_returns_the_current_frame():
    """Independent of the restatement: a previous camera that looks the opposite way (every point of the frame is behind it) and no
    history at all both give the current frame's bits, history 1, nothing reprojected."""
    cur, cam, prev, _ = synthetic(70, 45, 23)
    eye = cam[0]
    back = (eye, crt.get_inverse_view_matrix(eye, eye + np.array([0.0, 0.0, -1.0], dtype=F), [0.0, 1.0, 0.0]), cam[2])
    inf = float("inf")
    out = crt.temporal(cur, cam, prev=prev, prev_camera=back, depth_tolerance=inf, normal_tolerance=inf, return_info=True)
    assert_is_current_frame(out, cur, "camera turned round")
    assert_is_current_frame(crt.temporal(cur, cam, return_info=True), cur, "no history")


@pytest.mark.gpu
def test_temporal_rejects_the_history_where_the_depth_disagrees():
    """Independent of the restatement: identical cameras and guides, so a pixel reprojects onto itself (to rounding: the other taps lie
    in its 3x3 neighbourhood and weigh next to nothing).  With the previous depth x 1.5 inside a rectangle, a pixel whose 3x3
    neighbourhood lies in the rectangle has no tap within 5 % and is reset; a pixel two or more away from it keeps its history."""
    w, h = 70, 45
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:h, 0:w]
    depth = (30 + 3 * np.sin(xx / 9.0) + 2 * np.cos(yy / 7.0)).astype(F)      # smooth: neighbours within 2 %
    normal = np.zeros((h, w, 3), dtype=F)
    normal[..., 2] = 1.0
    cur = {"color": (rng.random((h, w, 3)) * 100).astype(F), "variance": (rng.random((h, w, 3)) * 300).astype(F), "depth": depth,
           "normal": normal, "id": np.zeros((h, w), dtype=np.int32)}
    prev = dict(cur, color=(rng.random((h, w, 3)) * 100).astype(F), history=np.full((h, w), 5, dtype=F), depth=depth.copy())
    x0, x1, y0, y1 = 20, 41, 10, 29
    prev["depth"][y0:y1, x0:x1] *= F(1.5)
    eye = np.array([1.0, 2.0, 3.0], dtype=F)
    cam = (eye, crt.get_inverse_view_matrix(eye, eye + np.array([0.3, 0.1, 1.0], dtype=F), [0.0, 1.0, 0.0]), F(0.7))
    _, color, var, hist, info = crt.temporal(cur, cam, prev=prev, prev_camera=cam, return_info=True)
    core = np.zeros((h, w), dtype=bool)
    core[y0 + 1:y1 - 1, x0 + 1:x1 - 1] = True
    far = np.ones((h, w), dtype=bool)
    far[y0 - 2:y1 + 2, x0 - 2:x1 + 2] = False
    far[0, :] = far[-1, :] = far[:, 0] = far[:, -1] = False
    assert (hist[core] == F(1)).all()
    assert np.array_equal(color[core].view(np.uint32), cur["color"][core].view(np.uint32))
    assert (np.abs(hist[far] - F(6)) < 1e-5).all()        # (the weighted mean of fives, to rounding)
    assert not np.array_equal(color[far], cur["color"][far])
    assert core.sum() <= w * h - info["reprojected"] <= (~far).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("static", [True, False], ids=["static", "moving"])
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_temporal_accumulation_reduces_the_error_against_a_converged_frame(renders, name, static):
    """64 x 48, spp 4, 8 frames with seeds 100 .. 107, defaults; R = spp 256, seed 7 at the last camera; mse on the RGB8 tone maps.
    The numpy prototype of the contract (threshold 1/100 instead of 1/64) measured, last frame alone / accumulated: cornell-box static
    1479.5 / 531.5, moving (20, 0, 10) per frame 1648.6 / 694.7; veach-mis static 670.3 / 235.1, moving (0, 0.1, 0.3) 719.8 / 361.0.
    The restatement above on the CPU oracle's frames (the device's frames, bit for bit): 1479.5 / 561.9, 1648.6 / 536.3, 670.3 / 264.6,
    722.6 / 367.9."""
    fr = frames(renders, name, 64, 48, 8, 100, static)
    prev = pcam = None
    for cur, noisy_rgb, _, cam in fr:
        rgb, color, var, hist = crt.temporal(cur, cam, prev=prev, prev_camera=pcam)
        prev, pcam = as_history(cur, color, var, hist), cam
    r = renders[name]
    r.set_spp(256)
    r.seed = 7
    try:
        ref_rgb = r.run_view(*pcam, width=64, height=48).copy()
    finally:
        r.seed = 0

    def mse(x):
        d = x.astype(np.float64) - ref_rgb.astype(np.float64)
        return float(np.mean(d * d))

    print("%s %s: mse of the last frame alone %.1f, accumulated %.1f (longest history %d)" % (name, "static" if static else "moving", mse(noisy_rgb),
                                                                                            mse(rgb), hist.max()))
    assert mse(rgb) < mse(noisy_rgb)


@pytest.mark.gpu
def test_temporal_device_form_on_a_stream_matches_host_form(renders):
    name, w, h = "veach-mis", 100, 70
    (c0, _, _, cam0), (c1, _, _, cam1) = frames(renders, name, w, h, 2, 50)
    prev = as_history(c0, c0["color"], c0["variance"], np.full((h, w), 3, dtype=F))
    want_rgb, want_c, want_v, want_h, want_info = crt.temporal(c1, cam1, prev=prev, prev_camera=cam0, return_info=True)
    assert 100 <= want_info["reprojected"] < w * h
    host = {"cur_" + k: v for k, v in c1.items()}
    host.update({"prev_" + k: v for k, v in prev.items()})
    outs = {"out_color": w * h * 12, "out_var": w * h * 12, "out_hist": w * h * 4, "out_rgb": w * h * 3}
    # (every output value must be written by the kernel: what is not uploaded is filled with 0x55)
    with DeviceBuffers({**host, **outs}, stream=True) as d:
        ptrs = d.ptrs

        def run(want_info, variance=True, out_rgb=True):
            cur_p = {k: ptrs["cur_" + k] for k in c1 if variance or k != "variance"}
            prev_p = {k: ptrs["prev_" + k] for k in prev if variance or k != "variance"}
            return crt.temporal_device(w, h, cam1, cur_p, ptrs["out_color"], ptrs["out_hist"], out_variance_ptr=ptrs["out_var"] if variance else None,
                                       out_rgb_ptr=ptrs["out_rgb"] if out_rgb else None, prev_ptrs=prev_p, prev_camera=cam0, stream=d.stream,
                                       want_info=want_info)

        def fetch():
            return (d.download("out_color", (h, w, 3), F), d.download("out_var", (h, w, 3), F), d.download("out_hist", (h, w), F),
                    d.download("out_rgb", (h, w, 3), np.uint8))

        assert run(False) is None
        d.synchronize()
        c, v, hh, r = fetch()
        assert_bits(c, want_c, "device form")
        assert_bits(v, want_v, "device form, variance")
        assert_bits(hh, want_h, "device form, history")
        assert np.array_equal(r, want_rgb)
        # colour and history only, with the timer and the count (the call synchronizes the stream)
        for n in outs:
            d.fill(n)
        info = run(True, variance=False, out_rgb=False)
        assert info["reprojected"] == want_info["reprojected"] and info["total_ms"] > 0, info
        c, v, hh, r = fetch()
        assert_bits(c, want_c, "device form, colour only")
        assert_bits(hh, want_h, "device form, colour only: history")
        assert (r == 0x55).all() and (v.view(np.uint32) == 0x55555555).all()


@pytest.mark.gpu
def test_run_view_temporal_equals_the_calls_by_hand(renders):
    name, w, h = "cornell-box", 64, 48
    r = renders[name]
    fr = frames(renders, name, w, h, 3, 40)                  # seeds 40, 41, 42: self.seed + the frames since the reset
    r.set_spp(4)
    r.seed = 40
    try:
        r.reset_temporal()
        prev = pcam = None
        for f, (cur, noisy_rgb, g, cam) in enumerate(fr):
            want_rgb, want_c, want_v, want_h, want_info = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, return_info=True)
            prev, pcam = as_history(cur, want_c, want_v, want_h), cam
            rgb, mean = r.run_view_temporal(*cam, width=w, height=h, denoise=(f == 2))
            if f == 2:
                want_rgb, want_mean = crt.denoise_var(want_c, want_v, **g)
                assert r.denoise_info["passes"] == 3
            else:
                want_mean = want_c
            assert_bits(mean, want_mean, "run_view_temporal frame %d" % f)
            assert np.array_equal(rgb, want_rgb)
            assert_bits(r.variance_buffer, want_v, "variance_buffer")
            assert_bits(r.temporal_history_buffer, want_h, "temporal_history_buffer")
            assert r.temporal_info["reprojected"] == want_info["reprojected"] and r.seed == 40
            assert np.array_equal(r.frame_buffer, noisy_rgb) and np.array_equal(r.mean_buffer.view(np.uint32), cur["color"].view(np.uint32))
        assert r.temporal_info["reprojected"] >= 100
        # the filtered frame did not become the history: a fourth call with an explicit seed continues the unfiltered one
        cur3, _, _, cam3 = fr[1]
        want = crt.temporal(cur3, cam3, prev=prev, prev_camera=pcam)
        rgb, mean = r.run_view_temporal(*cam3, seed=41, width=w, height=h)
        assert_bits(mean, want[1], "fourth frame")
        # a change of size drops the history, and so does reset_temporal(): first frames, rendered with self.seed again
        r.run_view_temporal(*fr[0][3], width=w - 3, height=h)
        assert (r.temporal_history_buffer == 1).all() and r.temporal_info["reprojected"] == 0
        r.reset_temporal()
        rgb, mean = r.run_view_temporal(*fr[0][3], width=w, height=h)
        assert (r.temporal_history_buffer == 1).all() and r.temporal_info["reprojected"] == 0
        assert_bits(mean, fr[0][0]["color"], "first frame after the reset")
        assert np.array_equal(rgb, fr[0][1])
        # a following run_view gives the frame it gave before
        assert np.array_equal(r.run_view(*fr[0][3], width=w, height=h), fr[0][1])
        assert np.array_equal(r.mean_buffer.view(np.uint32), fr[0][0]["color"].view(np.uint32)) and r.variance_buffer is None
    finally:
        r.seed = 0
        r.reset_temporal()


@pytest.mark.gpu
def test_cli_accumulates_a_moving_sequence(renders, tmp_path):
    from PIL import Image
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    name, w, h = "cornell-box", 64, 48
    cfg = util.SCENES[name]
    base = [cli, cfg, "--spp", "4", "--width", str(w), "--height", str(h), "--seed", "40", "--base-dir", util.ROOT]
    step = ["--temporal", "3", "--temporal-step", ",".join(repr(float(v)) for v in MOVES[name][0])]
    last, acc, den = (str(tmp_path / n) for n in ("last.png", "acc.png", "den.png"))
    res = subprocess.run(base + step + ["-o", last, "--temporal-out", acc], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    res2 = subprocess.run(base + step + ["-o", last, "--temporal-out", den, "--temporal-denoise"], capture_output=True, text=True, timeout=120)
    assert res2.returncode == 0, res2.stderr
    prev = pcam = None
    for cur, noisy_rgb, g, cam in frames(renders, name, w, h, 3, 40):
        rgb, color, var, hist = crt.temporal(cur, cam, prev=prev, prev_camera=pcam)
        prev, pcam = as_history(cur, color, var, hist), cam
    assert np.array_equal(np.asarray(Image.open(last)), noisy_rgb)
    assert np.array_equal(np.asarray(Image.open(acc)), rgb)
    assert np.array_equal(np.asarray(Image.open(den)), crt.denoise_var(color, var, **g)[0])
