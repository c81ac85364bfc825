"""Per-pixel variance buffer (CRT_FLAG_VARIANCE, crt_variance / crt_variance_device, include/crt.h; Render.run_view(want_variance=True),
Render.variance in Python; crt_cli --variance).

The expected values come from the oracle's per-path radiance (OracleScene.render(want_L=True) -> (h, w, spp, 3)): the contract of
include/crt.h is restated in variance_restated.py in numpy float32, operation by operation -- first the frame's own sum, which must reproduce the oracle's
mean bit for bit, then the same loop with the sum of squares -- and the device result must match it on uint32 views (NaN matches NaN).
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import frames
import util
from frames import oracle_frame, renders  # noqa: F401
from util import assert_bits
from variance_restated import restated_variance

F = np.float32
VARIANCE_EXPORTS = ("crt_variance", "crt_variance_device", "crt_denoise_var_defaults", "crt_denoise_var", "crt_denoise_var_device")


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_variance_entry_points_are_exported():
    lib = capi.lib()
    for name in VARIANCE_EXPORTS:
        assert name in capi.EXPORTS
        getattr(lib, name)
    lib.crt_abi_version.restype = C.c_int
    assert lib.crt_abi_version() == 5 == capi.ABI_VERSION
    assert capi.FLAG_VARIANCE == 32 == crt.FLAG_VARIANCE
    for name in ("denoise_var", "denoise_var_device", "denoise_var_defaults"):
        assert hasattr(crt, name)
    for name in ("variance", "run_view_denoised"):
        assert hasattr(crt.Render, name)
    import inspect
    assert "want_variance" in inspect.signature(crt.Render.run_view).parameters
    assert "want_variance" in inspect.signature(crt.Render.run_view_range).parameters
    assert "variance_guided" in inspect.signature(crt.Render.run_view_denoised).parameters


def test_variance_null_arguments_are_refused_before_any_device_call():
    lib = capi.lib()
    buf = np.zeros(16, dtype=F)
    done = C.c_uint32(77)
    assert lib.crt_variance(None, capi.ptr(buf), C.byref(done)) == capi.ERR_INVALID_ARG
    assert b"null" in lib.crt_last_error()
    assert lib.crt_variance_device(None, capi.ptr(buf), None, None) == capi.ERR_INVALID_ARG
    assert b"null" in lib.crt_last_error()
    assert done.value == 77 and not buf.any()


def test_restatement_is_the_sample_variance_of_the_mean():
    """The restated contract against numpy's float64 sample variance on made-up samples (no oracle, no device): full frames and a
    partial range, whose r = S / n rescales the sums of L / S to sums of L / n.  The difference n q - c^2 cancels: its rounding error is
    a few 2^-24 of n q, so the variance of the mean is off by up to a few 2^-24 x mean^2 whatever its own size (two of these uniform
    samples can be arbitrarily close) -- allowed for below with 1e-5 x mean^2 beside the relative 1e-4."""
    rng = np.random.default_rng(5)
    L = (rng.random((6, 7, 8, 3)) * 10).astype(F)
    for n in (8, 5, 2):
        L64 = L[:, :, :n].astype(np.float64)
        want = L64.var(axis=2, ddof=1) / n
        got = restated_variance(L, 8, n)
        assert (np.abs(got - want) <= 1e-4 * want + 1e-5 * L64.mean(axis=2) ** 2).all(), n
    zero = np.zeros((2, 2, 4, 3), dtype=F)
    assert np.array_equal(restated_variance(zero, 4).view(np.uint32), np.zeros((2, 2, 3), dtype=np.uint32))


# ------------------------------------------------------------------------------------------------------------------ GPU --

def gpu_frame(r, name, w, h, spp, want_variance=True, **kw):
    """(rgb, mean, variance or None) of a GPU render"""
    f = frames.gpu_frame(r, name, w, h, spp, want_variance=want_variance, **kw)
    return f["rgb"], f["mean"], f["variance"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
@pytest.mark.parametrize("w,h,spp", [(64, 48, 4), (64, 48, 8), (61, 47, 4)])
def test_variance_matches_restatement_on_the_oracles_radiance(renders, name, w, h, spp):
    orgb, omean, L = oracle_frame(name, w, h, spp)
    want = restated_variance(L, spp)
    assert (want > 0).any()
    rgb, mean, var = gpu_frame(renders[name], name, w, h, spp)
    assert np.array_equal(rgb, orgb) and np.array_equal(mean.view(np.uint32), omean.view(np.uint32))
    assert_bits(var, want, "%s %dx%d spp %d" % (name, w, h, spp))
    v2, done = renders[name].variance(width=w, height=h)   # readable until the next render call, as often as one likes
    assert done == spp
    assert_bits(v2, want, "second read")
    for mode in (crt.TRAVERSAL_REFERENCE, crt.TRAVERSAL_FAST):
        assert_bits(gpu_frame(renders[name], name, w, h, spp, traversal=mode)[2], want, "%s traversal %d" % (name, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_frame_with_the_flag_is_the_frame_without_it(renders, name):
    r = renders[name]
    rgb0, mean0, none = gpu_frame(r, name, 100, 70, 6, seed=3, want_variance=False)
    assert none is None
    rgb1, mean1, var = gpu_frame(r, name, 100, 70, 6, seed=3)
    assert np.array_equal(rgb0, rgb1) and np.array_equal(mean0.view(np.uint32), mean1.view(np.uint32))
    assert var.shape == (70, 100, 3) and (var > 0).any() and not (var < 0).any()
    rgb2, mean2, _ = gpu_frame(r, name, 100, 70, 6, seed=3, want_variance=False)   # ... and a render without it afterwards is what it was
    assert np.array_equal(rgb0, rgb2) and np.array_equal(mean0.view(np.uint32), mean2.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_variance_is_the_same_through_every_path_of_the_frame_logic(renders, name, monkeypatch):
    r = renders[name]
    w, h, spp = 64, 48, 8
    _, _, L = oracle_frame(name, w, h, spp)
    want = restated_variance(L, spp)
    rgb0, mean0, var0 = gpu_frame(r, name, w, h, spp)
    assert_bits(var0, want, "one chunk")

    def check(where, **kw):
        rgb, mean, var = gpu_frame(r, name, w, h, spp, **kw)
        assert np.array_equal(rgb, rgb0) and np.array_equal(mean.view(np.uint32), mean0.view(np.uint32)), where
        assert_bits(var, want, where)

    # 3 072 pixel slots: chunks of 2^13 paths hold two samples, so the sums cross three chunk borders
    with monkeypatch.context() as m:
        m.setenv("CRT_CHUNK_LOG2", "13")
        check("small chunks")
        assert r.stats["kernel_launches"] == 4
        m.setenv("CRT_PIPELINE", "2")
        check("small chunks, wavefront pipeline")
    with monkeypatch.context() as m:
        m.setenv("CRT_PIPELINE", "2")
        check("wavefront pipeline")
    check("stats", stats=True)
    # the commit ring keeps no per-path radiance: the flag switches it off for the call
    with monkeypatch.context() as m:
        m.setenv("CRT_COMMIT_RING_LOG2", "2")
        gpu_frame(r, name, w, h, spp, want_variance=False, flags=crt.FLAG_BOUNDED_RADIANCE)
        assert r.radiance_storage()[1] == 4, "the forced ring did not engage: the check below would show nothing"
        check("forced ring and FLAG_BOUNDED_RADIANCE", flags=crt.FLAG_BOUNDED_RADIANCE)
        assert r.radiance_storage()[1] == 0
        check("forced ring", flags=0)
        assert r.radiance_storage()[1] == 0
    check("FLAG_BOUNDED_RADIANCE", flags=crt.FLAG_BOUNDED_RADIANCE)
    assert r.radiance_storage()[1] == 0


def variance_error(r, w, h):
    with pytest.raises(crt.CrtError) as e:
        r.variance(width=w, height=h)
    assert "crt_variance" in str(e.value)
    return str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["4", "2"])
def test_variance_of_a_progressive_render(pipeline, monkeypatch):
    monkeypatch.setenv("CRT_PIPELINE", pipeline)
    name, w, h, spp = "cornell-box", 64, 48, 8
    t = util.task(name)
    r = crt.Render(util.host_scene(name), spp, t.P_RR, t.light_sample_n)   # a fresh handle: no flagged render on it yet
    try:
        eye, iv, fov = util.camera(name)
        orgb, omean, L = oracle_frame(name, w, h, spp)
        variance_error(r, w, h)                                             # before any flagged render
        kw = dict(width=w, height=h)
        assert r.run_view_range(eye, iv, fov, 0, 3, want_variance=True, **kw) is None
        v3, done = r.variance(**kw)
        assert done == 3
        assert_bits(v3, restated_variance(L, spp, 3), "after [0, 3)")
        aov = r.run_view_aov(eye, iv, fov, **kw)
        assert r.run_view_range(eye, iv, fov, 3, 2, want_variance=True, **kw) is None
        prev_rgb, prev_mean, pdone = r.preview(want_mean=True, **kw)
        assert pdone == 5
        v5, done = r.variance(**kw)
        assert done == 5
        assert_bits(v5, restated_variance(L, spp, 5), "after [3, 5)")
        r.run_view_aov(eye, iv, fov, width=32, height=24)
        assert_bits(r.variance(**kw)[0], v5, "read again after an AOV pass and a preview")
        rgb = r.run_view_range(eye, iv, fov, 5, 3, want_variance=True, **kw)
        assert np.array_equal(rgb, orgb) and np.array_equal(r.mean_buffer.view(np.uint32), omean.view(np.uint32))
        v8, done = r.variance(**kw)
        assert done == spp
        assert_bits(v8, restated_variance(L, spp), "after [5, 8): the one-shot result")
        r.set_spp(spp)
        rgb1 = r.run_view(eye, iv, fov, want_variance=True, **kw)
        assert np.array_equal(rgb1, orgb)
        assert_bits(r.variance_buffer, v8, "one shot")
        assert np.array_equal(r.run_view_aov(eye, iv, fov, **kw)["depth"].view(np.uint32), aov["depth"].view(np.uint32))
        # errors: after an unflagged render
        r.run_view(eye, iv, fov, **kw)
        assert "CRT_FLAG_VARIANCE" in variance_error(r, w, h)
        # a first range of one sample
        assert r.run_view_range(eye, iv, fov, 0, 1, want_variance=True, **kw) is None
        assert "2 samples" in variance_error(r, w, h)
        # a frame whose second range dropped the flag, and stays dropped although the third has it again
        assert r.run_view_range(eye, iv, fov, 1, 4, **kw) is None
        variance_error(r, w, h)
        rgb = r.run_view_range(eye, iv, fov, 5, 3, want_variance=True, **kw)
        assert np.array_equal(rgb, orgb)
        variance_error(r, w, h)
        # a finished frame of one sample
        r.set_spp(1)
        r.run_view(eye, iv, fov, **kw)
        with pytest.raises(crt.CrtError):
            r.run_view(eye, iv, fov, want_variance=True, **kw)
        assert "2 samples" in variance_error(r, w, h)
    finally:
        r.free()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_variance_tiled_shards_deinterleave_to_row_major(renders, world):
    from cudaraytracing_amd.distributed import untile_numpy
    name, w, h, spp = "veach-mis", 100, 70, 4
    r = renders[name]
    _, _, full = gpu_frame(r, name, w, h, spp)
    eye, iv, fov = util.camera(name)
    cam = r._cam(eye, iv, fov)
    r.set_spp(spp)
    shards = []
    for rank in range(world):
        slots = crt.shard_slots(w, h, rank, world)
        rgb = np.zeros((slots, 3), dtype=np.uint8)
        prm = r._params(rank=rank, world=world, flags=capi.FLAG_TILED_OUTPUT | capi.FLAG_VARIANCE, width=w, height=h)
        capi.check(capi.lib().crt_render(r._h, C.byref(cam), C.byref(prm), capi.ptr(rgb), None, None), "crt_render")
        var = np.full((slots, 3), 7, dtype=F)   # (padding slots must come back as +0)
        done = C.c_uint32()
        capi.check(capi.lib().crt_variance(r._h, capi.ptr(var), C.byref(done)), "crt_variance")
        assert done.value == spp
        shards.append(var)
    g = np.stack(shards)
    assert_bits(untile_numpy(g, w, h), full, "tiled, world %d" % world)
    tx, ty = (w + 7) // 8, (h + 7) // 8
    padding = 0
    for rank in range(world):
        for s in range(g.shape[1]):
            tile = (s // 64) * world + rank
            i, j = (tile % tx) * 8 + (s % 64) % 8, (tile // tx) * 8 + (s % 64) // 8
            if tile >= tx * ty or i >= w or j >= h:
                padding += 1
                assert np.all(g[rank, s].view(np.uint32) == 0), (rank, s)
    assert padding > 0


@pytest.mark.gpu
def test_variance_device_form_on_a_stream_matches_host_form(renders):
    name, w, h, spp = "cornell-box", 100, 70, 4
    r = renders[name]
    rgb0, mean0, var0 = gpu_frame(r, name, w, h, spp)
    eye, iv, fov = util.camera(name)
    # (every output value must be written: the buffers are filled with 0x55)
    with DeviceBuffers({"rgb": w * h * 3, "mean": w * h * 12, "var": w * h * 12}, stream=True) as d:
        r.set_spp(spp)
        r.extra_flags = capi.FLAG_VARIANCE
        try:
            r.run_view_device(eye, iv, fov, d.ptrs["rgb"], d.ptrs["mean"], stream=d.stream, want_stats=False, width=w, height=h)
        finally:
            r.extra_flags = 0
        done = C.c_uint32()
        capi.check(capi.lib().crt_variance_device(r._h, C.c_void_p(d.ptrs["var"]), C.c_void_p(d.stream), C.byref(done)), "crt_variance_device")
        assert done.value == spp
        d.synchronize()
        rgb, mean, var = d.download("rgb", (h, w, 3), np.uint8), d.download("mean", (h, w, 3), F), d.download("var", (h, w, 3), F)
        assert np.array_equal(rgb, rgb0) and np.array_equal(mean.view(np.uint32), mean0.view(np.uint32))
        assert_bits(var, var0, "device form")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
@pytest.mark.parametrize("w,h,spp", [(64, 48, 8), (32, 24, 512)])
def test_variance_precision_against_float64(renders, name, w, h, spp):
    """crt_variance against the float64 sample variance (ddof = 1, divided by n) of the oracle's radiance, over the values whose float64
    variance is positive.  Bound 1e-4: the numpy restatement, which the device reproduces bit for bit, measured a largest relative error
    of 3.44e-6 / 2.75e-6 at spp 8 and 2.68e-6 / 3.46e-6 at spp 512 (cornell-box / veach-mis) on these inputs -- about thirty times below
    the bound, room for the next power of spp."""
    _, _, L = oracle_frame(name, w, h, spp)
    _, _, var = gpu_frame(renders[name], name, w, h, spp)
    assert_bits(var, restated_variance(L, spp), "%s spp %d" % (name, spp))
    L64 = L.astype(np.float64)
    want = L64.var(axis=2, ddof=1) / spp
    pos = want > 0
    assert pos.any()
    rel = np.abs(var.astype(np.float64)[pos] - want[pos]) / want[pos]
    print("%s %dx%d spp %d: largest relative error %.3e, 99th percentile %.3e, smallest variance / mean^2 %.3e"
          % (name, w, h, spp, rel.max(), np.percentile(rel, 99), (want[pos] / np.maximum(L64.mean(axis=2)[pos] ** 2, 1e-300)).min()))
    assert not (var < 0).any() and not np.isnan(var).any()
    assert rel.max() <= 1e-4
    assert (var[~pos].view(np.uint32) == 0).all()           # float64 variance 0: exactly +0
    dark = (L == 0).all(axis=(2, 3))
    assert (var[dark].view(np.uint32) == 0).all()           # a pixel whose samples are all +0


@pytest.mark.gpu
def test_cli_writes_the_variance_buffer(renders, tmp_path):
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    cfg = util.SCENES["veach-mis"]
    base = [cli, cfg, "--spp", "4", "--width", "96", "--height", "72", "--seed", "42", "--base-dir", util.ROOT]
    plain, flagged, pfm = (str(tmp_path / n) for n in ("plain.png", "flagged.png", "var.pfm"))
    res = subprocess.run(base + ["-o", plain], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    res = subprocess.run(base + ["-o", flagged, "--variance", pfm], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert open(plain, "rb").read() == open(flagged, "rb").read()
    _, _, var = gpu_frame(renders["veach-mis"], "veach-mis", 96, 72, 4, seed=42)
    assert_bits(util.read_pfm(pfm)[1], var, "--variance")
    bad = subprocess.run([cli, cfg, "--devices", "0,0", "--gather", "copy", "--variance", pfm], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--variance" in bad.stderr
    bad = subprocess.run([cli, cfg, "--gpus", "2", "--variance", pfm], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--variance" in bad.stderr


@pytest.mark.gpu
def test_multi_render_has_no_variance_buffer():
    name = "cornell-box"
    t = util.task(name)
    m = crt.MultiRender(util.host_scene(name), 2, t.P_RR, t.light_sample_n, devices=(0,), gather=crt.GATHER_COPY)
    try:
        eye, iv, fov = util.camera(name)
        with pytest.raises(NotImplementedError):
            m.run_view(eye, iv, fov, want_variance=True)
        with pytest.raises(NotImplementedError):
            m.variance()
        with pytest.raises(NotImplementedError):
            m.run_view_denoised(eye, iv, fov, variance_guided=True)
        # crt_multi_render clears the flag: the frame is the single-device frame
        m.extra_flags = crt.FLAG_VARIANCE
        rgb = m.run_view(eye, iv, fov, width=64, height=48)
        orgb, _, _ = oracle_frame(name, 64, 48, 2)
        assert np.array_equal(rgb, orgb)
    finally:
        m.free()
