"""GPU tests of the gathered buffers of a multi-device frame: crt_multi_render_buffers / crt_multi_buffers_device (include/crt.h),
MultiRender.run_view_gathered, gathered_device and the filtered forms on them, crt::Render::run_view_gathered through crt_cli --gathered.

The GPU box has ONE MI355X: several ranks share device 0 (CRT_GATHER_COPY), which runs everything but the collective itself; RCCL runs
with a one-rank communicator (as tests/test_multi_gpu.py).  Whatever the number of ranks, every plane must be the one the single-device
call it is named after produces on the same scene, seed and size: run_view(want_variance / want_halves), variance(), half_buffers() and
run_view_aov_shading(first=all six).  Every comparison is on bits: float32 on its uint32 view, the integer planes as they are."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import util

pytestmark = pytest.mark.gpu

SPP = 4
ALL = tuple(capi.MULTI_BUFFERS)
# scene, width, height, ranks: ragged on both edges with 4 tiles on 3 ranks (unequal tile counts, a width that is a multiple of neither 8
# nor 4); test_multi_gpu's two odd cases; a width that is a multiple of 4 but not of 8.  Never more ranks than tiles.
CASES = [("cornell-box", 13, 9, 3), ("veach-mis", 100, 75, 3), ("cornell-box", 64, 40, 8), ("cornell-box", 12, 16, 2)]


def padded_plane_bytes(name, w, h, world):
    """the bytes of plane `name` in one rank's block: the shard's slots x the pixel's bytes, to the next 16-byte boundary"""
    ch, dt = capi.MULTI_BUFFERS[name]
    return (crt.shard_slots(w, h, 0, world) * ch * np.dtype(dt).itemsize + 15) // 16 * 16


@pytest.fixture(scope="module")
def single():
    """single-device Renders and, made once per (scene, size, seed), every plane as the single-device calls give it: reference(...)"""
    renders, frames = {}, {}

    def reference(name, w, h, seed=0):
        key = (name, w, h, seed)
        if key not in frames:
            if name not in renders:
                t = util.task(name)
                renders[name] = crt.Render(util.host_scene(name), SPP, t.P_RR, t.light_sample_n, device=0)
            one = renders[name]
            eye, iv, fov = util.camera(name)
            one.set_spp(SPP)
            one.seed = seed
            one.traversal = crt.TRAVERSAL_EXACT
            f = {"rgb": one.run_view(eye, iv, fov, width=w, height=h, want_halves=True).copy(), "mean": one.mean_buffer.copy()}
            f["variance"] = one.variance(width=w, height=h)[0]
            f["half_a"], f["half_b"] = one.half_buffers(width=w, height=h)[:2]
            assert np.array_equal(util.bits(f["variance"]), util.bits(one.variance_buffer))
            # ... and the flags leave the frame alone: want_variance alone and no flag give the same frame and the same variance
            assert np.array_equal(one.run_view(eye, iv, fov, width=w, height=h, want_variance=True), f["rgb"])
            assert np.array_equal(util.bits(one.mean_buffer), util.bits(f["mean"])) and np.array_equal(util.bits(one.variance_buffer), util.bits(f["variance"]))
            f["rays"] = one.stats["rays"]
            f.update(one.run_view_aov_shading(eye, iv, fov, first=tuple(capi.AOV_BUFFERS), width=w, height=h))
            assert sorted(f) == sorted(ALL + ("rays",))
            for a in f.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            frames[key] = f
        return frames[key]

    yield reference
    for r in renders.values():
        r.free()


def multi(name, devices, gather=crt.GATHER_COPY, spp=SPP):
    t = util.task(name)
    return crt.MultiRender(util.host_scene(name), spp, t.P_RR, t.light_sample_n, devices=devices, gather=gather)


def assert_planes(got, want, names, where):
    assert sorted(got) == sorted(names), (where, sorted(got))
    util.assert_same(got, want, names, where)


@pytest.mark.parametrize("name,w,h,ranks", CASES)
def test_every_plane_equals_the_single_device_plane(single, name, w, h, ranks):
    want = single(name, w, h)
    eye, iv, fov = util.camera(name)
    m = multi(name, [0] * ranks)
    try:
        got = m.run_view_gathered(eye, iv, fov, want=ALL, width=w, height=h)
        assert_planes(got, want, ALL, "%s %dx%d on %d ranks" % (name, w, h, ranks))
        for n in ("tri", "material"):
            assert got[n].dtype == np.int32
        assert got["rgb"].dtype == np.uint8
        # the attributes Render fills
        assert m.frame_buffer is got["rgb"] and m.mean_buffer is got["mean"] and m.variance_buffer is got["variance"]
        assert m.half_a_buffer is got["half_a"] and m.half_b_buffer is got["half_b"]
        assert sorted(m.aov_buffers) == sorted(capi.AOV_BUFFERS) and all(m.aov_buffers[k] is got[k] for k in capi.AOV_BUFFERS)
        assert sorted(m.shading_buffers) == sorted(capi.AOV_SHADING_BUFFERS) and all(m.shading_buffers[k] is got[k] for k in capi.AOV_SHADING_BUFFERS)
        assert m.info["n_ranks"] == ranks and m.info["gather"] == crt.GATHER_COPY and m.info["rccl_ranks"] == 0
        assert m.info["bytes_per_rank"] == sum(padded_plane_bytes(n, w, h, ranks) for n in ALL)
        assert m.info["rays"] == want["rays"] == sum(s["rays"] for s in m.rank_stats) == m.stats["rays"]
        assert m.info["paths"] == w * h * SPP
        ptrs, dev = m.gathered_device()
        assert dev == 0 and all(ptrs[n] for n in ALL)
    finally:
        m.free()


@pytest.mark.parametrize("names", [("variance",), ("depth", "tri"), ("emission",)], ids=["variance", "depth-tri", "emission"])
def test_a_subset_yields_exactly_its_planes(single, names):
    """the variance alone (no AOV trace), depth and tri alone (no shading pass), the emission alone (the shading pass with `first` NULL)"""
    name, w, h, ranks = CASES[0]
    want = single(name, w, h)
    eye, iv, fov = util.camera(name)
    m = multi(name, [0] * ranks)
    try:
        got = m.run_view_gathered(eye, iv, fov, want=names, width=w, height=h)
        assert_planes(got, want, names, "subset %r" % (names,))
        assert m.info["bytes_per_rank"] == sum(padded_plane_bytes(n, w, h, ranks) for n in names)
        ptrs, dev = m.gathered_device()
        assert dev == 0
        for n in ALL:
            assert bool(ptrs[n]) == (n in names), n
        assert m.frame_buffer is None and m.mean_buffer is None
        # the frame device call reports what that frame made: neither RGB nor the mean
        d_rgb, d_mean = C.c_void_p(), C.c_void_p()
        capi.check(capi.lib().crt_multi_frame_device(m._mh, C.byref(d_rgb), C.byref(d_mean), None), "crt_multi_frame_device")
        assert not d_rgb.value and not d_mean.value
    finally:
        m.free()


def test_rccl_all_gather_carries_every_plane_on_a_one_rank_communicator(single):
    name, w, h = "cornell-box", 64, 40
    want = single(name, w, h)
    eye, iv, fov = util.camera(name)
    m = multi(name, [0], gather=crt.GATHER_RCCL)
    try:
        got = m.run_view_gathered(eye, iv, fov, want=ALL, width=w, height=h)
        assert m.info["gather"] == crt.GATHER_RCCL and m.info["rccl_ranks"] == 1 and m.info["rccl_version"] > 0
        assert m.info["bytes_per_rank"] == sum(padded_plane_bytes(n, w, h, 1) for n in ALL)
        assert_planes(got, want, ALL, "rccl")
    finally:
        m.free()


def test_refusals_leave_the_handle_usable_and_crt_multi_render_as_it_was(single):
    name, w, h, ranks = CASES[0]
    want = single(name, w, h)
    eye, iv, fov = util.camera(name)
    lib = capi.lib()
    m = multi(name, [0] * ranks)
    try:
        cam = m._cam(eye, iv, fov)
        prm = m._params(width=w, height=h)
        info = capi.MultiInfo()

        def call(mh, cam_, prm_, mask):
            return lib.crt_multi_render_buffers(mh, cam_, prm_, mask, None, None, C.byref(info))

        assert call(None, C.byref(cam), C.byref(prm), capi.MULTI_ALL) == capi.ERR_INVALID_ARG
        assert call(m._mh, None, C.byref(prm), capi.MULTI_ALL) == capi.ERR_INVALID_ARG
        assert call(m._mh, C.byref(cam), None, capi.MULTI_ALL) == capi.ERR_INVALID_ARG
        assert call(m._mh, C.byref(cam), C.byref(prm), 0) == capi.ERR_INVALID_ARG and b"want" in lib.crt_last_error()
        assert call(m._mh, C.byref(cam), C.byref(prm), capi.MULTI_ALL + 1) == capi.ERR_INVALID_ARG and b"want" in lib.crt_last_error()
        assert call(m._mh, C.byref(cam), C.byref(prm), capi.MULTI_BITS["rgb"] | (1 << 31)) == capi.ERR_INVALID_ARG
        one_sample = m._params(width=w, height=h)
        one_sample.spp = 1
        for n in ("variance", "half_a", "half_b"):
            assert call(m._mh, C.byref(cam), C.byref(one_sample), capi.MULTI_BITS[n]) == capi.ERR_INVALID_ARG and b"spp" in lib.crt_last_error(), n
        zero = m._params(width=w, height=h)
        zero.width = 0
        assert call(m._mh, C.byref(cam), C.byref(zero), capi.MULTI_ALL) == capi.ERR_INVALID_ARG
        assert lib.crt_multi_buffers_device(None, None, None) == capi.ERR_INVALID_ARG
        with pytest.raises(ValueError):
            m.run_view_gathered(eye, iv, fov, want=("rgb", "specular"), width=w, height=h)
        m.set_spp(1)
        with pytest.raises(crt.CrtError):
            m.run_view_gathered(eye, iv, fov, want=("variance",), width=w, height=h)
        # a refused call made no plane ...
        ptrs, _ = m.gathered_device()
        assert not any(ptrs.values())
        # ... and the next one gives the right frame
        m.set_spp(SPP)
        names = ("rgb", "mean", "variance", "normal", "material")
        assert_planes(m.run_view_gathered(eye, iv, fov, want=names, width=w, height=h), want, names, "after the refusals")
        # crt_multi_render afterwards: its frame, its mean, its block of RGB8 and the mean, and the planes it reports
        rgb = m.run_view(eye, iv, fov, width=w, height=h)
        assert np.array_equal(rgb, want["rgb"]) and np.array_equal(util.bits(m.mean_buffer), util.bits(want["mean"]))
        slots = crt.shard_slots(w, h, 0, ranks)
        assert m.info["bytes_per_rank"] == (slots * 3 + 15) // 16 * 16 + slots * 12
        ptrs, _ = m.gathered_device()
        assert [n for n in ALL if ptrs[n]] == ["rgb", "mean"]
        d_rgb, d_mean = C.c_void_p(), C.c_void_p()
        capi.check(lib.crt_multi_frame_device(m._mh, C.byref(d_rgb), C.byref(d_mean), None), "crt_multi_frame_device")
        assert d_rgb.value == ptrs["rgb"] and d_mean.value == ptrs["mean"]
        m.run_view(eye, iv, fov, width=w, height=h, want_mean=False)
        assert m.info["bytes_per_rank"] == (slots * 3 + 15) // 16 * 16
        # the refusals of the single-device interfaces stand
        for call_ in (lambda: m.run_view(eye, iv, fov, want_variance=True), lambda: m.variance(), lambda: m.run_view_aov(eye, iv, fov),
                      lambda: m.run_view_denoised(eye, iv, fov), lambda: m.run_view_selected(eye, iv, fov)):
            with pytest.raises(NotImplementedError):
                call_()
    finally:
        m.free()


def test_the_device_pointers_feed_a_device_filter_without_a_host_round_trip(single):
    name, w, h, ranks = "veach-mis", 100, 75, 3
    want = single(name, w, h)
    eye, iv, fov = util.camera(name)
    guides = {k: want[k] for k in ("albedo", "normal", "depth")}
    want_rgb, want_mean, want_var = crt.denoise_var(want["mean"], want["variance"], want_variance=True, **guides)
    m = multi(name, [0] * ranks)
    try:
        assert m.run_view_gathered(eye, iv, fov, want=("mean", "variance", "albedo", "normal", "depth"), width=w, height=h, to_host=False) is None
        assert m.mean_buffer is None and m.variance_buffer is None and m.aov_buffers is None
        p, dev = m.gathered_device()
        assert dev == 0
        scratch_bytes = crt.denoise_scratch_bytes(w, h)
        with DeviceBuffers({"out_mean": w * h * 12, "out_rgb": w * h * 3, "out_var": w * h * 4, "scratch": scratch_bytes}, stream=True) as d:
            info = crt.denoise_var_device(w, h, p["mean"], p["variance"], d.ptrs["out_mean"], d.ptrs["out_rgb"], d.ptrs["out_var"], d.ptrs["scratch"], scratch_bytes,
                                          albedo_ptr=p["albedo"], normal_ptr=p["normal"], depth_ptr=p["depth"], device=dev, stream=d.stream, want_info=True)
            assert info["passes"] > 0
            assert np.array_equal(d.download("out_rgb", (h, w, 3), np.uint8), want_rgb)
            assert np.array_equal(util.bits(d.download("out_mean", (h, w, 3))), util.bits(want_mean))
            assert np.array_equal(util.bits(d.download("out_var", (h, w))), util.bits(want_var))
    finally:
        m.free()


@pytest.fixture(scope="module")
def filtered():
    """one single-device Render and one MultiRender of three ranks on device 0 for the filtered forms at 64 x 40"""
    name = "cornell-box"
    t = util.task(name)
    one = crt.Render(util.host_scene(name), SPP, t.P_RR, t.light_sample_n, device=0)
    m = multi(name, [0, 0, 0])
    yield one, m, util.camera(name)
    one.free()
    m.free()


@pytest.mark.parametrize("settings", [dict(variance_guided=True), dict(nlm=True, demodulate=True), dict(regress=True, scales=2)],
                         ids=["variance-guided", "nlm-demodulated", "regress-two-scales"])
def test_gathered_denoised_equals_run_view_denoised(filtered, settings):
    one, m, (eye, iv, fov) = filtered
    want_rgb, want_mean = one.run_view_denoised(eye, iv, fov, width=64, height=40, **settings)
    rgb, mean = m.run_view_gathered_denoised(eye, iv, fov, width=64, height=40, **settings)
    assert np.array_equal(rgb, want_rgb) and np.array_equal(util.bits(mean), util.bits(want_mean))
    assert np.array_equal(m.frame_buffer, one.frame_buffer) and np.array_equal(util.bits(m.mean_buffer), util.bits(one.mean_buffer))
    assert np.array_equal(util.bits(m.variance_buffer), util.bits(one.variance_buffer))
    util.assert_same(m.aov_buffers, one.aov_buffers, ("albedo", "normal", "depth"), "guides")
    if settings.get("demodulate"):
        util.assert_same(m.shading_buffers, one.shading_buffers, tuple(capi.AOV_SHADING_BUFFERS), "shading")
    assert m.denoise_info is not None


def test_gathered_selected_equals_run_view_selected(filtered):
    one, m, (eye, iv, fov) = filtered
    want_rgb, want_mean = one.run_view_selected(eye, iv, fov, width=64, height=40)
    rgb, mean = m.run_view_gathered_selected(eye, iv, fov, width=64, height=40)
    assert np.array_equal(rgb, want_rgb) and np.array_equal(util.bits(mean), util.bits(want_mean))
    assert np.array_equal(m.select_buffers["choice"], one.select_buffers["choice"])
    assert np.array_equal(util.bits(m.select_buffers["error"]), util.bits(one.select_buffers["error"]))
    assert m.select_info["chosen"] == one.select_info["chosen"]
    with pytest.raises(ValueError):
        m.run_view_gathered_selected(eye, iv, fov, candidates=("median",), width=64, height=40)


def test_cli_gathered_files_are_the_single_device_files(tmp_path):
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    cfg = util.SCENES["veach-mis"]
    base = [cli, cfg, "--spp", "4", "--width", "96", "--height", "72", "--seed", "42", "--base-dir", util.ROOT]
    one, many = str(tmp_path / "one"), str(tmp_path / "many")
    r = subprocess.run(base + ["-o", one + ".png", "--variance", one + ".variance.pfm", "--aov", one, "--aov-shading", one], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(base + ["-o", many + ".png", "--devices", "0,0,0", "--gather", "copy", "--gathered", many + ",variance,depth,emission,diffuse_albedo"],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    assert "ranks: 3, gather: copy" in r.stdout

    def data(path):
        with open(path, "rb") as f:
            return f.read()

    assert data(many + ".png") == data(one + ".png")
    for got, want in ((".variance.pfm", ".variance.pfm"), (".depth.pfm", "_depth.pfm"), (".emission.pfm", ".emission.pfm"), (".diffuse_albedo.pfm", ".diffuse_albedo.pfm")):
        assert data(many + got) == data(one + want), got
        assert (many + got) in r.stdout
    # the default planes
    r = subprocess.run(base + ["-o", many + ".png", "--devices", "0,0,0", "--gather", "copy", "--gathered", many + "_d"], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.glob("many_d.*")) == ["many_d.%s.pfm" % n for n in ("albedo", "depth", "mean", "normal", "variance")]
    assert data(many + "_d.variance.pfm") == data(one + ".variance.pfm") and data(many + "_d.depth.pfm") == data(one + "_depth.pfm")
    # refused: on one device, with a name that is no float plane; the refusals of the single-device options stand
    bad = subprocess.run(base + ["-o", many + ".png", "--gathered", many], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--gathered" in bad.stderr and "--gpus / --devices" in bad.stderr
    bad = subprocess.run(base + ["--devices", "0,0", "--gather", "copy", "--gathered", many + ",tri"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--gathered" in bad.stderr
    bad = subprocess.run(base + ["--devices", "0,0", "--gather", "copy", "--gathered", many, "--variance", many + ".v.pfm"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--variance reads one device's buffer (not with --gpus / --devices)" in bad.stderr
