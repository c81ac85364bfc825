"""Half-frame buffers (CRT_FLAG_HALF_BUFFERS, crt_half_buffers / crt_half_buffers_device, include/crt.h; Render.run_view(want_halves=True),
Render.run_view_range(want_halves=True) and Render.half_buffers in Python).

The expected values come from the oracle's per-path radiance (OracleScene.render(want_L=True) -> (h, w, spp, 3)): the contract of
include/crt.h is restated below in numpy float32, operation by operation, in the style of util.restated_sums, and the device result must
match it on uint32 views.  37 x 21 is ragged against the 8 x 8 tiles in both directions (15 tiles, 960 pixel slots).
"""
import ctypes as C
import inspect

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import util
from frames import gpu_frame, oracle_frame, renders  # noqa: F401
from util import assert_bits

F = np.float32
W, H = 37, 21
SCENES = ("cornell-box", "veach-mis")


def restated_half_sums(L, S, n):
    """h0 and h1 of the crt_half_buffers contract after samples 0 .. n-1 of S: the quotient the frame adds, into the sum of its parity"""
    fs = F(S)
    h = [np.zeros(L.shape[:2] + (3,), dtype=F), np.zeros(L.shape[:2] + (3,), dtype=F)]
    with np.errstate(all="ignore"):
        for k in range(n):
            h[k & 1] = h[k & 1] + L[:, :, k, :] / fs
    assert h[0].dtype == F and h[1].dtype == F
    return h[0], h[1]


def restated_halves(L, S, n=None):
    """(out_a, out_b) of crt_half_buffers with n samples done"""
    n = S if n is None else n
    h0, h1 = restated_half_sums(L, S, n)
    with np.errstate(all="ignore"):
        a = h0 * (F(S) / F((n + 1) // 2))
        b = h1 * (F(S) / F(n // 2))
    assert a.dtype == F and b.dtype == F
    return a, b


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_half_buffer_entry_points_are_exported():
    lib = capi.lib()
    for name in ("crt_half_buffers", "crt_half_buffers_device"):
        assert name in capi.EXPORTS
        getattr(lib, name)
    lib.crt_abi_version.restype = C.c_int
    assert lib.crt_abi_version() == 5 == capi.ABI_VERSION
    assert capi.FLAG_HALF_BUFFERS == 64 == crt.FLAG_HALF_BUFFERS and "FLAG_HALF_BUFFERS" in crt.__all__
    assert hasattr(crt.Render, "half_buffers")
    assert "want_halves" in inspect.signature(crt.Render.run_view).parameters
    assert "want_halves" in inspect.signature(crt.Render.run_view_range).parameters
    for name in ("half_buffers", "run_view_selected"):
        with pytest.raises(NotImplementedError):
            getattr(crt.MultiRender, name)(None)


def test_half_buffers_null_and_unrendered_handles_are_refused_before_any_device_call():
    lib = capi.lib()
    buf = np.zeros(16, dtype=F)
    done = C.c_uint32(77)
    for call in (lambda: lib.crt_half_buffers(None, capi.ptr(buf), capi.ptr(buf), C.byref(done)),
                 lambda: lib.crt_half_buffers_device(None, capi.ptr(buf), capi.ptr(buf), None, C.byref(done))):
        assert call() == capi.ERR_INVALID_ARG
        assert lib.crt_last_error().startswith(b"crt_half_buffers: ") and b"null" in lib.crt_last_error()
    # a handle nothing has been rendered on: created from the host scene without a device call of ours; both-null and not-yet-rendered
    # are refused from the handle's marks alone
    sc = util.host_scene("veach-mis")
    h = C.c_void_p()
    if lib.crt_scene_create(C.byref(sc.desc()), 0, C.byref(h)) == capi.CRT_OK:  # (needs a device: on a machine without one the null checks above stand alone)
        try:
            assert lib.crt_half_buffers(h, None, None, C.byref(done)) == capi.ERR_INVALID_ARG and b"null" in lib.crt_last_error()
            assert lib.crt_half_buffers(h, capi.ptr(buf), None, C.byref(done)) == capi.ERR_INVALID_ARG
            assert b"CRT_FLAG_HALF_BUFFERS" in lib.crt_last_error()
        finally:
            lib.crt_scene_destroy(h)
    assert done.value == 77 and not buf.any()


def test_restated_halves_are_the_float64_half_means():
    """The restated contract against float64 means of the even and of the odd samples on made-up samples (no oracle, no device): a full
    frame, an odd count (n_a != n_b) and the smallest one.  Sums of at most 4 positive fp32 terms and one scale: 1e-6 relative is six
    roundings of 2^-24 with room.  The halves weighted by their counts are the frame's mean to the same bound."""
    rng = np.random.default_rng(11)
    L = (rng.random((5, 6, 8, 3)) * 10).astype(F)
    for n in (8, 7, 2):
        a, b = restated_halves(L, 8, n)
        L64 = L[:, :, :n].astype(np.float64)
        want_a, want_b = L64[:, :, 0::2].mean(axis=2), L64[:, :, 1::2].mean(axis=2)
        assert np.abs(a - want_a).max() <= 1e-6 * want_a.max() and np.abs(b - want_b).max() <= 1e-6 * want_b.max(), n
        n_a, n_b = (n + 1) // 2, n // 2
        both = (n_a * a.astype(np.float64) + n_b * b.astype(np.float64)) / n
        assert np.abs(both - L64.mean(axis=2)).max() <= 1e-6 * L64.mean(axis=2).max(), n
    a2, b2 = restated_halves(L, 8, 2)   # one sample each: the sample itself, to the rounding of x / S * (S / 1)
    assert np.allclose(a2, L[:, :, 0], rtol=3e-7, atol=0) and np.allclose(b2, L[:, :, 1], rtol=3e-7, atol=0)


# ------------------------------------------------------------------------------------------------------------------ GPU --

def gpu_halves(r, name, spp, want_halves=True, want_variance=False):
    f = gpu_frame(r, name, W, H, spp, want_halves=want_halves, want_variance=want_variance)
    return f["rgb"], f["mean"], f["variance"], f["half_a"], f["half_b"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("spp", [8, 7, 2])
def test_halves_match_the_restatement_on_the_oracles_radiance(renders, name, spp):
    orgb, omean, L = oracle_frame(name, W, H, spp)
    want_a, want_b = restated_halves(L, spp)
    assert (want_a > 0).any() and (want_b > 0).any() and not np.array_equal(want_a, want_b)
    rgb, mean, var, a, b = gpu_halves(renders[name], name, spp)
    assert np.array_equal(rgb, orgb) and np.array_equal(mean.view(np.uint32), omean.view(np.uint32))
    where = "%s spp %d" % (name, spp)
    assert_bits(a, want_a, where + " half a")
    assert_bits(b, want_b, where + " half b")
    a2, b2, done = renders[name].half_buffers(width=W, height=H)   # readable until the next render call
    assert done == spp
    assert_bits(a2, want_a, where + " second read a")
    assert_bits(b2, want_b, where + " second read b")
    # either output alone
    lib, only = capi.lib(), np.full((H, W, 3), 7, dtype=F)
    capi.check(lib.crt_half_buffers(renders[name]._h, None, capi.ptr(only), None), "crt_half_buffers")
    assert_bits(only, want_b, where + " b alone")
    capi.check(lib.crt_half_buffers(renders[name]._h, capi.ptr(only), None, None), "crt_half_buffers")
    assert_bits(only, want_a, where + " a alone")


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["4", "2"])
def test_halves_of_a_progressive_render_keep_the_frames_parity(pipeline, monkeypatch):
    """Ranges (0, 3), (3, 2), (5, 2) of spp 7, read out after every range: the second range starts on an odd sample, where a parity
    counted from the chunk's start would swap the halves."""
    monkeypatch.setenv("CRT_PIPELINE", pipeline)
    name, spp = "cornell-box", 7
    t = util.task(name)
    r = crt.Render(util.host_scene(name), spp, t.P_RR, t.light_sample_n)   # a fresh handle
    try:
        eye, iv, fov = util.camera(name)
        orgb, omean, L = oracle_frame(name, W, H, spp)
        kw = dict(width=W, height=H)
        with pytest.raises(crt.CrtError) as e:
            r.half_buffers(**kw)                                            # no render with the flag yet
        assert "CRT_FLAG_HALF_BUFFERS" in str(e.value)
        rgb = None
        for s0, ns in ((0, 3), (3, 2), (5, 2)):
            rgb = r.run_view_range(eye, iv, fov, s0, ns, want_halves=True, **kw)
            a, b, done = r.half_buffers(**kw)
            assert done == s0 + ns
            want_a, want_b = restated_halves(L, spp, s0 + ns)
            assert_bits(a, want_a, "after [%d, %d) half a" % (s0, s0 + ns))
            assert_bits(b, want_b, "after [%d, %d) half b" % (s0, s0 + ns))
            v, vdone = r.variance(**kw)                                     # the flag implies CRT_FLAG_VARIANCE
            assert vdone == s0 + ns
        assert np.array_equal(rgb, orgb) and np.array_equal(r.mean_buffer.view(np.uint32), omean.view(np.uint32))
        # a first range of one sample; a frame whose second range dropped the flag
        assert r.run_view_range(eye, iv, fov, 0, 1, want_halves=True, **kw) is None
        with pytest.raises(crt.CrtError) as e:
            r.half_buffers(**kw)
        assert "2 samples" in str(e.value)
        assert r.run_view_range(eye, iv, fov, 1, 3, want_variance=True, **kw) is None
        with pytest.raises(crt.CrtError):
            r.half_buffers(**kw)
        r.variance(**kw)                                                    # (the variance sums went on)
        assert r.run_view_range(eye, iv, fov, 4, 3, want_halves=True, **kw) is not None
        with pytest.raises(crt.CrtError):
            r.half_buffers(**kw)
    finally:
        r.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_halves_are_the_same_across_chunks_and_pipelines(renders, name, monkeypatch):
    spp = 7
    orgb, omean, L = oracle_frame(name, W, H, spp)
    want_a, want_b = restated_halves(L, spp)

    def check(where):
        rgb, mean, var, a, b = gpu_halves(renders[name], name, spp)
        assert np.array_equal(rgb, orgb) and np.array_equal(mean.view(np.uint32), omean.view(np.uint32)), where
        assert_bits(a, want_a, where + " half a")
        assert_bits(b, want_b, where + " half b")

    # 960 pixel slots: a chunk of 2^10 paths holds one sample, so every second chunk starts on an odd sample
    with monkeypatch.context() as m:
        m.setenv("CRT_CHUNK_LOG2", "10")
        check("one sample per chunk")
        m.setenv("CRT_PIPELINE", "2")
        check("one sample per chunk, wavefront pipeline")
    with monkeypatch.context() as m:
        m.setenv("CRT_CHUNK_LOG2", "12")                                    # four samples per chunk, then three
        check("four samples per chunk")
    with monkeypatch.context() as m:
        m.setenv("CRT_PIPELINE", "2")
        check("wavefront pipeline")


@pytest.mark.gpu
def test_halves_of_a_tiled_shard(renders):
    """Rank 1 of 3 with CRT_FLAG_TILED_OUTPUT: the shard's compact tiles, padding slots +0"""
    name, spp, rank, world = "veach-mis", 7, 1, 3
    r = renders[name]
    _, _, L = oracle_frame(name, W, H, spp)
    want = restated_halves(L, spp)
    eye, iv, fov = util.camera(name)
    cam = r._cam(eye, iv, fov)
    r.set_spp(spp)
    slots = crt.shard_slots(W, H, rank, world)
    rgb = np.zeros((slots, 3), dtype=np.uint8)
    prm = r._params(rank=rank, world=world, flags=capi.FLAG_TILED_OUTPUT | capi.FLAG_HALF_BUFFERS, width=W, height=H)
    capi.check(capi.lib().crt_render(r._h, C.byref(cam), C.byref(prm), capi.ptr(rgb), None, None), "crt_render")
    got = [np.full((slots, 3), 7, dtype=F), np.full((slots, 3), 7, dtype=F)]
    done = C.c_uint32()
    capi.check(capi.lib().crt_half_buffers(r._h, capi.ptr(got[0]), capi.ptr(got[1]), C.byref(done)), "crt_half_buffers")
    assert done.value == spp
    tx, ty = (W + 7) // 8, (H + 7) // 8
    expect = [np.zeros((slots, 3), dtype=F), np.zeros((slots, 3), dtype=F)]
    padding = 0
    for s in range(slots):
        tile = (s // 64) * world + rank
        i, j = (tile % tx) * 8 + (s % 64) % 8, (tile // tx) * 8 + (s % 64) // 8
        if tile >= tx * ty or i >= W or j >= H:
            padding += 1
            continue
        expect[0][s], expect[1][s] = want[0][j, i], want[1][j, i]
    assert padding > 0
    assert_bits(got[0], expect[0], "tiled half a")
    assert_bits(got[1], expect[1], "tiled half b")


@pytest.mark.gpu
def test_halves_device_form_on_a_stream(renders):
    name, spp = "cornell-box", 7
    r = renders[name]
    orgb, omean, L = oracle_frame(name, W, H, spp)
    want_a, want_b = restated_halves(L, spp)
    eye, iv, fov = util.camera(name)
    table = {"rgb": (3, np.uint8), "mean": (3, F), "a": (3, F), "b": (3, F)}
    with DeviceBuffers.image(table, W, H) as d:
        r.set_spp(spp)
        r.extra_flags = capi.FLAG_HALF_BUFFERS
        try:
            r.run_view_device(eye, iv, fov, d.ptrs["rgb"], d.ptrs["mean"], stream=d.stream, want_stats=False, width=W, height=H)
        finally:
            r.extra_flags = 0
        done = C.c_uint32()
        capi.check(capi.lib().crt_half_buffers_device(r._h, C.c_void_p(d.ptrs["a"]), C.c_void_p(d.ptrs["b"]), C.c_void_p(d.stream), C.byref(done)),
                   "crt_half_buffers_device")
        assert done.value == spp
        d.synchronize()
        got = d.fetch(("mean", "a", "b"))
    assert np.array_equal(got["mean"].view(np.uint32), omean.view(np.uint32))
    assert_bits(got["a"], want_a, "device form half a")
    assert_bits(got["b"], want_b, "device form half b")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_frame_and_variance_with_the_flag_are_those_of_the_variance_flag(renders, name):
    spp = 7
    rgb0, mean0, var0, a0, b0 = gpu_halves(renders[name], name, spp, want_halves=False, want_variance=True)
    assert a0 is None and b0 is None
    rgb1, mean1, var1, a, b = gpu_halves(renders[name], name, spp)
    assert np.array_equal(rgb0, rgb1) and np.array_equal(mean0.view(np.uint32), mean1.view(np.uint32))
    assert_bits(var1, var0, "variance with the half buffers")
    # the halves weighted by their counts against the frame's mean: the sums differ in order by design, so to rounding only -- seven
    # fp32 additions on either side, 1e-5 of the pixel's largest channel sum
    n_a, n_b = (spp + 1) // 2, spp // 2
    both = (n_a * a.astype(np.float64) + n_b * b.astype(np.float64)) / spp
    assert (np.abs(both - mean1) <= 1e-5 * np.abs(mean1)).all()
    rgb2, mean2, var2, _, _ = gpu_halves(renders[name], name, spp, want_halves=False, want_variance=True)   # ... and afterwards it is what it was
    assert np.array_equal(rgb0, rgb2) and np.array_equal(var0.view(np.uint32), var2.view(np.uint32))


@pytest.mark.gpu
def test_halves_are_refused_after_renders_that_keep_none(renders):
    name, spp = "veach-mis", 4
    r = renders[name]
    eye, iv, fov = util.camera(name)
    kw = dict(width=W, height=H)

    def refused():
        with pytest.raises(crt.CrtError) as e:
            r.half_buffers(**kw)
        assert e.value.status == capi.ERR_INVALID_ARG and "crt_half_buffers" in str(e.value)

    gpu_halves(r, name, spp)
    r.half_buffers(**kw)
    r.run_view(eye, iv, fov, want_variance=True, **kw)          # a render without the flag
    refused()
    gpu_halves(r, name, spp)
    r.half_buffers(**kw)
    r.extra_flags = capi.FLAG_HALF_BUFFERS                      # a sparse frame keeps no halves, whatever the flags say
    try:
        r.run_view_map(eye, iv, fov, np.full((H, W), 2, dtype=np.uint32), **kw)
    finally:
        r.extra_flags = 0
    refused()
