"""First-hit AOV pass (crt_render_aov / crt_render_aov_device, include/crt.h; Render.run_view_aov in Python; crt_cli --aov) and the
PFM writer.

The expected buffers come from the oracle (aov_expected.py): orc_render with p_rr = 0 under the ray log; the closest-hit rays that leave the eye are
the primary rays of the frame's paths, logged pixel by pixel, sample by sample.  Their hits are folded in numpy float32 exactly as
the contract says (a = a + kd / S over the hits in sample order, ...), and every buffer must match bit for bit.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import util
from aov_expected import NAMES, expected_aov, primary_rays, run_aov
from frames import renders  # noqa: F401

AOV_EXPORTS = ("crt_render_aov", "crt_render_aov_device", "crt_write_pfm")


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_aov_entry_points_are_exported():
    lib = capi.lib()
    for name in AOV_EXPORTS:
        assert name in capi.EXPORTS
        getattr(lib, name)
    assert hasattr(crt, "write_pfm")


def test_aov_arguments_are_checked_before_any_device_call():
    """Every invalid call is CRT_ERR_INVALID_ARG, also on a machine without a GPU: the arguments are checked first.  A non-null
    scene here is a dummy that must never be dereferenced."""
    lib = capi.lib()
    dummy = C.create_string_buffer(256)
    sc = C.cast(dummy, C.c_void_p)
    cam = capi.Camera()
    good = capi.Params(64, 48, 4, 0.6, 1, 0, 0, 1, capi.TRAVERSAL_EXACT, 0)
    buf = np.zeros(64 * 48 * 3, dtype=np.float32)
    bufs = capi.AovBuffers()
    bufs.albedo = buf.ctypes.data
    none = capi.AovBuffers()

    def both(scene, camera, prm, b):
        r1 = lib.crt_render_aov(scene, camera, prm, b, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_render_aov_device(scene, camera, prm, b, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == capi.ERR_INVALID_ARG, (r1, r2, e1, e2)
        return e1

    assert b"null" in both(None, C.byref(cam), C.byref(good), C.byref(bufs))
    assert b"null" in both(sc, None, C.byref(good), C.byref(bufs))
    assert b"null" in both(sc, C.byref(cam), None, C.byref(bufs))
    assert b"null" in both(sc, C.byref(cam), C.byref(good), None)
    assert b"no output" in both(sc, C.byref(cam), C.byref(good), C.byref(none))
    for field, value in (("spp", 0), ("width", 0), ("height", 0)):
        p = capi.Params(64, 48, 4, 0.6, 1, 0, 0, 1, capi.TRAVERSAL_EXACT, 0)
        setattr(p, field, value)
        both(sc, C.byref(cam), C.byref(p), C.byref(bufs))
    bad_shard = capi.Params(64, 48, 4, 0.6, 1, 0, 3, 3, capi.TRAVERSAL_EXACT, capi.FLAG_TILED_OUTPUT)
    both(sc, C.byref(cam), C.byref(bad_shard), C.byref(bufs))
    untiled = capi.Params(64, 48, 4, 0.6, 1, 0, 1, 3, capi.TRAVERSAL_EXACT, 0)
    both(sc, C.byref(cam), C.byref(untiled), C.byref(bufs))
    bad_mode = capi.Params(64, 48, 4, 0.6, 1, 0, 0, 1, 7, 0)
    both(sc, C.byref(cam), C.byref(bad_mode), C.byref(bufs))


def test_every_aov_entry_point_refuses_the_shared_bad_inputs():
    """The six entry points share one argument check: each bad input is CRT_ERR_INVALID_ARG from every one of them, before any device
    call, and the message begins with the entry's base name.  The scene is a dummy that must never be dereferenced."""
    lib = capi.lib()
    dummy = C.create_string_buffer(256)
    sc, cam, sp = C.cast(dummy, C.c_void_p), capi.Camera(), capi.AovSpecularParams(2)
    buf = np.zeros(64 * 48 * 3, dtype=np.float32)
    first, shading, specular = capi.AovBuffers(), capi.AovShadingBuffers(), capi.AovSpecularBuffers()
    first.albedo = shading.emission = specular.guide_albedo = buf.ctypes.data

    def params(**fields):
        p = capi.Params(64, 48, 4, 0.6, 1, 0, 0, 1, capi.TRAVERSAL_EXACT, 0)
        for k, v in fields.items():
            setattr(p, k, v)
        return C.byref(p)

    bad = {"null scene": (None, C.byref(cam), params()), "null camera": (sc, None, params()), "null params": (sc, C.byref(cam), None),
           "spp 0": (sc, C.byref(cam), params(spp=0)), "width 0": (sc, C.byref(cam), params(width=0)), "height 0": (sc, C.byref(cam), params(height=0)),
           "rank >= world": (sc, C.byref(cam), params(rank=3, world=3, flags=capi.FLAG_TILED_OUTPUT)),
           "world > 1, not tiled": (sc, C.byref(cam), params(rank=1, world=3)), "unknown traversal": (sc, C.byref(cam), params(traversal=7))}
    # what each form takes between the params and (the device form's stream and) the info
    own = {"crt_render_aov": (C.byref(first),), "crt_render_aov_shading": (None, C.byref(shading)),
           "crt_render_aov_specular": (C.byref(sp), C.byref(specular))}
    for base, args in own.items():
        for fn, tail in ((base, (None,)), (base + "_device", (None, None))):
            for what, head in bad.items():
                rc = getattr(lib, fn)(*head, *args, *tail)
                err = lib.crt_last_error()
                assert rc == capi.ERR_INVALID_ARG and err.startswith(base.encode() + b": "), (fn, what, rc, err)


def test_write_pfm_round_trips(tmp_path):
    rng = np.random.default_rng(5)
    one = (rng.normal(size=(5, 7)) * 1e3).astype(np.float32)
    one[0, 0], one[4, 6], one[2, 3] = np.inf, -0.0, np.float32(1e-42)
    three = rng.normal(size=(4, 6, 3)).astype(np.float32)
    lib = capi.lib()
    for a, kind in ((one, b"Pf"), (three, b"PF")):
        path = str(tmp_path / ("x%s.pfm" % kind.decode()))
        ch = 1 if a.ndim == 2 else 3
        capi.check(lib.crt_write_pfm(path.encode(), a.shape[1], a.shape[0], ch, capi.ptr(a)), "crt_write_pfm")
        raw = open(path, "rb").read()
        assert raw.startswith(kind + b"\n%d %d\n-1.0\n" % (a.shape[1], a.shape[0]))
        hdr, back = util.read_pfm(path)
        assert hdr == (kind, b"%d %d" % (a.shape[1], a.shape[0]), b"-1.0")
        assert np.array_equal(back.view(np.uint32), a.view(np.uint32))
        # bottom-up rows: the file's first row is the image's last
        first = np.frombuffer(raw[len(raw) - a.nbytes:][:a.shape[1] * ch * 4], dtype="<f4")
        assert np.array_equal(first.view(np.uint32), a[-1].reshape(-1).view(np.uint32))
        path2 = str(tmp_path / "api.pfm")
        crt.write_pfm(path2, a)
        assert open(path2, "rb").read() == raw
    assert lib.crt_write_pfm(str(tmp_path / "y.pfm").encode(), 7, 5, 2, capi.ptr(one)) == capi.ERR_INVALID_ARG
    assert lib.crt_write_pfm(str(tmp_path / "y.pfm").encode(), 0, 5, 1, capi.ptr(one)) == capi.ERR_INVALID_ARG
    assert lib.crt_write_pfm(None, 7, 5, 1, capi.ptr(one)) == capi.ERR_INVALID_ARG
    assert lib.crt_write_pfm(str(tmp_path / "no" / "such" / "dir.pfm").encode(), 7, 5, 1, capi.ptr(one)) == -5


# ------------------------------------------------------------------------------------------------------------------ GPU --

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_aov_small_frames_match_oracle(renders, name):
    got = run_aov(renders[name], name, 4, 64, 48)
    assert renders[name].aov_info["chunks"] == 1 and renders[name].aov_info["rays"] == 64 * 48 * 4
    want = expected_aov(name, 64, 48, 4)
    util.assert_same(got, want, NAMES, name)
    assert (got["tri"] >= 0).any() and (got["coverage"] > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name,x0,y0", [("cornell-box", 388, 0), ("veach-mis", 400, 40)])
def test_aov_crop_of_full_camera_in_chunks(renders, name, x0, y0):
    """800 x 600 at spp 160: 7.7e7 camera rays, more than the 2^25-ray budget of a chunk, so the running sums cross chunks."""
    spp = 160
    got = run_aov(renders[name], name, spp)
    info = renders[name].aov_info
    assert info["chunks"] >= 2 and info["rays"] == 800 * 600 * spp, info
    want = expected_aov(name, 800, 600, spp, crop=(x0, y0, 24, 16))
    crop = {n: got[n][y0:y0 + 16, x0:x0 + 24] for n in NAMES}
    util.assert_same(crop, want, NAMES, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_aov_spp1_equals_intersect_on_the_logged_primary_rays(renders, name):
    r = renders[name]
    got = run_aov(r, name, 1, 64, 48)
    o, d, _, _, _ = primary_rays(name, 64, 48, 1)
    tri, t = r.intersect(o.reshape(-1, 3), d.reshape(-1, 3), traversal=crt.TRAVERSAL_EXACT | crt.INTERSECT_RAW_DIRECTIONS)
    assert np.array_equal(got["tri"].reshape(-1), tri)
    depth = np.where(tri >= 0, t, np.float32(0.0)).astype(np.float32)
    assert np.array_equal(got["depth"].reshape(-1).view(np.uint32), depth.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_aov_traversal_modes_agree(renders, name):
    base = run_aov(renders[name], name, 4, 64, 48, seed=3)
    for mode in (crt.TRAVERSAL_REFERENCE, crt.TRAVERSAL_FAST):
        util.assert_same(run_aov(renders[name], name, 4, 64, 48, traversal=mode, seed=3), base, NAMES, "%s mode %d" % (name, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("var,value", [("CRT_PIPELINE", "2"), ("CRT_DEC", "0"), ("CRT_IMPL", "0"), ("CRT_REF16", "0")])
def test_aov_kernel_variants_agree(renders, var, value, monkeypatch):
    base = {n: run_aov(renders[n], n, 4, 64, 48) for n in renders}
    monkeypatch.setenv(var, value)
    for n in renders:
        util.assert_same(run_aov(renders[n], n, 4, 64, 48), base[n], NAMES, "%s %s=%s" % (n, var, value))


@pytest.mark.gpu
def test_aov_tiled_shards_deinterleave_to_row_major(renders):
    from cudaraytracing_amd.distributed import untile_numpy
    name, w, h, world, spp = "veach-mis", 100, 70, 3, 2
    r = renders[name]
    full = run_aov(r, name, spp, w, h)
    eye, iv, fov = util.camera(name)
    cam = r._cam(eye, iv, fov)
    shards = {n: [] for n in NAMES}
    for rank in range(world):
        slots = crt.shard_slots(w, h, rank, world)
        bufs, arrs = capi.AovBuffers(), {}
        for n in NAMES:
            ch, dt = capi.AOV_BUFFERS[n]
            arrs[n] = np.full((slots, ch), 7, dtype=dt)  # (padding slots must come back as 0 / -1)
            setattr(bufs, n, arrs[n].ctypes.data)
        prm = r._params(rank=rank, world=world, flags=capi.FLAG_TILED_OUTPUT, width=w, height=h)
        info = capi.AovInfo()
        capi.check(capi.lib().crt_render_aov(r._h, C.byref(cam), C.byref(prm), C.byref(bufs), C.byref(info)), "crt_render_aov")
        assert info.rays == slots * spp and info.chunks == 1
        for n in NAMES:
            shards[n].append(arrs[n])
    for n in NAMES:
        img = untile_numpy(np.stack(shards[n]), w, h)
        img = img if capi.AOV_BUFFERS[n][0] == 3 else img[:, :, 0]
        util.assert_same({n: img}, full, (n,), "tiled")
        # padding slots: every slot of the gathered tiles that is no pixel
        tx, ty = (w + 7) // 8, (h + 7) // 8
        g = np.stack(shards[n])
        lt = g.shape[1] // 64
        for rank in range(world):
            for s in range(g.shape[1]):
                tile = (s // 64) * world + rank
                i, j = (tile % tx) * 8 + (s % 64) % 8, (tile // tx) * 8 + (s % 64) // 8
                if tile >= tx * ty or i >= w or j >= h:
                    assert np.all(g[rank, s] == (-1 if n in ("tri", "material") else 0)), (n, rank, s)
        assert lt * world >= tx * ty


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["4", "2"])
def test_aov_calls_between_progressive_ranges(renders, pipeline, monkeypatch):
    monkeypatch.setenv("CRT_PIPELINE", pipeline)
    name = "cornell-box"
    r = renders[name]
    eye, iv, fov = util.camera(name)
    r.set_spp(4)
    one = r.run_view(eye, iv, fov, width=64, height=48).copy()
    one_mean = r.mean_buffer.copy()
    aov = r.run_view_aov(eye, iv, fov, width=64, height=48)
    assert r.run_view_range(eye, iv, fov, 0, 1, width=64, height=48) is None
    util.assert_same(r.run_view_aov(eye, iv, fov, width=64, height=48), aov, NAMES, "after range 0")
    _, _, done = r.preview(width=64, height=48)
    assert done == 1
    assert r.run_view_range(eye, iv, fov, 1, 2, width=64, height=48) is None
    r.run_view_aov(eye, iv, fov, width=32, height=24)  # another size in between
    rgb = r.run_view_range(eye, iv, fov, 3, 1, width=64, height=48)
    assert np.array_equal(rgb, one)
    assert np.array_equal(r.mean_buffer.view(np.uint32), one_mean.view(np.uint32))


@pytest.mark.gpu
def test_aov_device_form_on_a_stream_matches_host_form(renders):
    name, w, h = "veach-mis", 80, 56
    r = renders[name]
    want = run_aov(r, name, 3, w, h)
    eye, iv, fov = util.camera(name)
    with DeviceBuffers.image({n: capi.AOV_BUFFERS[n] for n in NAMES}, w, h) as d:
        assert r.run_view_aov_device(eye, iv, fov, d.ptrs, stream=d.stream, want_info=False, width=w, height=h) is None
        d.synchronize()
        util.assert_same(d.fetch(NAMES), want, NAMES, "device form")
        # a subset of the buffers, with the pass's timer (the call synchronizes the stream)
        d.fill("depth", 0)
        info = r.run_view_aov_device(eye, iv, fov, {"depth": d.ptrs["depth"]}, stream=d.stream, width=w, height=h)
        assert info["chunks"] == 1 and info["rays"] == w * h * 3 and info["total_ms"] > 0
        util.assert_same(d.fetch(["depth"]), want, ("depth",), "subset")


def to_u8(v):
    v = np.asarray(v, dtype=np.float32)
    out = np.where(np.isnan(v) | (v <= 0), 0, np.where(v >= 255, 255, np.trunc(np.nan_to_num(v))))
    return out.astype(np.uint8)


@pytest.mark.gpu
def test_cli_writes_aov_files(renders, tmp_path):
    from PIL import Image
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    prefix = str(tmp_path / "veach")
    cfg = util.SCENES["veach-mis"]
    res = subprocess.run([cli, cfg, "-o", prefix + ".png", "--spp", "2", "--width", "96", "--height", "72", "--seed", "42", "--base-dir", util.ROOT,
                          "--aov", prefix], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    got = run_aov(renders["veach-mis"], "veach-mis", 2, 96, 72, seed=42)
    one, two = np.float32(1.0), np.float32(2.0)
    alb = to_u8(np.float32(255.0) * np.clip(got["albedo"], np.float32(0), np.float32(1)))
    nrm = to_u8(np.float32(255.0) * np.clip((got["normal"] + one) / two, np.float32(0), np.float32(1)))
    assert np.array_equal(np.asarray(Image.open(prefix + "_albedo.png")), alb)
    assert np.array_equal(np.asarray(Image.open(prefix + "_normal.png")), nrm)
    hdr, depth = util.read_pfm(prefix + "_depth.pfm")
    assert hdr[0] == b"Pf" and hdr[2] == b"-1.0"
    assert np.array_equal(depth.view(np.uint32), got["depth"].view(np.uint32))
    bad = subprocess.run([cli, cfg, "--devices", "0,0", "--gather", "copy", "--aov", prefix], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--aov" in bad.stderr


@pytest.mark.gpu
def test_multi_render_has_no_aov_pass():
    m = crt.MultiRender(util.host_scene("cornell-box"), 2, devices=(0,), gather=crt.GATHER_COPY)
    try:
        eye, iv, fov = util.camera("cornell-box")
        with pytest.raises(NotImplementedError):
            m.run_view_aov(eye, iv, fov)
        with pytest.raises(NotImplementedError):
            m.run_view_aov_device(eye, iv, fov, {})
    finally:
        m.free()
