"""The progressive layer -- crt_render_range / crt_render_range_device, the accumulator on the scene handle, crt_preview /
crt_preview_device (include/crt.h) -- against the oracle, bit for bit.

The expected values come from the oracle's per-path radiance (OracleScene.render(want_L=True) -> (h, w, S, 3)), restated in numpy
float32 operation by operation as the header states the contract:
    c_n   = the loop c = c + L_k / F(S) for k < n          (util.restated_sums; c_S must be the oracle's own mean)
    p_n   = c_n * (F(S) / F(n))                            (one division for the scale, one multiply per channel)
    rgb_n = the oracle's tone map of p_n
Every comparison is on uint32 views (NaN matches NaN) or on the RGB bytes.
"""
import ctypes as C

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import oracle_lib as O
import util
from frames import fresh_render, oracle_frame, renders  # noqa: F401
from scene_files import _write_scaled_soup_scene
from util import assert_bits, restated_sums

F = np.float32
SCENES = ["cornell-box", "veach-mis"]


def restated_preview(L, S, n):
    """(c_n, p_n, rgb_n) of the contract after samples 0 .. n-1 of S"""
    c, _ = restated_sums(L, S, n)
    with np.errstate(all="ignore"):
        p = c * (F(S) / F(n))
    assert p.dtype == F
    return c, p, O.tonemap(p)


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_preview_null_arguments_are_refused_before_any_device_call():
    lib = capi.lib()
    rgb = np.full(48, 9, dtype=np.uint8)
    mean = np.full(48, 9, dtype=F)
    done = C.c_uint32(77)
    not_a_scene = np.zeros(1 << 18, dtype=np.uint8)   # (a non-null handle for the null-buffer case: the check comes before any use of it)
    for form in ("crt_preview", "crt_preview_device"):
        tail = (C.byref(done),) if form == "crt_preview" else (None, C.byref(done))
        assert getattr(lib, form)(None, capi.ptr(rgb), capi.ptr(mean), *tail) == capi.ERR_INVALID_ARG, form
        assert b"null" in lib.crt_last_error(), form
        assert getattr(lib, form)(capi.ptr(not_a_scene), None, capi.ptr(mean), *tail) == capi.ERR_INVALID_ARG, form
        assert b"null" in lib.crt_last_error(), form
    assert done.value == 77 and (rgb == 9).all() and (mean == 9).all() and not not_a_scene.any()


def test_restatement_is_the_mean_of_the_samples_so_far():
    """p_n of the restatement against the float64 mean of the first n of S = 7 made-up non-negative samples (no oracle, no device).
    Bound on the relative error, (n + 3) x 2^-23: n additions, one division per sample, one division and one multiply for the scale,
    each within 2^-24 of a non-negative partial result -- (n + 3) x 2^-24 to first order -- doubled."""
    rng = np.random.default_rng(11)
    S = 7
    L = (rng.random((5, 6, S, 3)) * 10).astype(F)
    L[0, 0] = 0                                            # a pixel whose samples are all +0: exactly +0
    L[0, 1, ::2] = 0
    for n in (1, 3, 6):
        _, p, _ = restated_preview(L, S, n)
        want = L[:, :, :n].astype(np.float64).mean(axis=2)
        err = np.abs(p.astype(np.float64) - want)
        print("n = %d: largest relative error %.3e, bound %.3e" % (n, (err[want > 0] / want[want > 0]).max(), (n + 3) * 2.0 ** -23))
        assert (err <= (n + 3) * 2.0 ** -23 * want).all(), n
        assert (p[0, 0].view(np.uint32) == 0).all()


# ------------------------------------------------------------------------------------------------------------------ GPU --


def check_preview(r, L, S, n, w, h, where, times=1):
    """crt_preview (host form, row-major) against p_n / rgb_n; returns the preview's mean"""
    _, p, rgb = restated_preview(L, S, n)
    for t in range(times):
        got_rgb, got_mean, done = r.preview(want_mean=True, width=w, height=h)
        assert done == n, (where, t)
        assert_bits(got_mean, p, "%s: mean of preview %d after %d of %d samples" % (where, t, n, S))
        assert np.array_equal(got_rgb, rgb), "%s: RGB of preview %d after %d of %d samples" % (where, t, n, S)
    return got_mean


def check_final(r, out, orgb, omean, where):
    assert out is not None and np.array_equal(out, orgb), where
    assert_bits(r.mean_buffer, omean, where + ": final mean")


def run_ranges(r, name, w, h, S, ranges, where, hook=None, **kw):
    """Submits the ranges in turn; after each one that does not end the frame compares a preview with the restatement, after the
    last one the frame with the oracle's.  hook(i, r): called after range i, before its preview."""
    orgb, omean, L = oracle_frame(name, w, h, S)
    eye, iv, fov = util.camera(name)
    r.set_spp(S)
    out = None
    for i, (b, c) in enumerate(ranges):
        out = r.run_view_range(eye, iv, fov, b, c, width=w, height=h, **kw)
        if hook:
            hook(i, r)
        if b + c < S:
            assert out is None
            check_preview(r, L, S, b + c, w, h, "%s, after [%d, %d)" % (where, b, b + c))
    assert ranges[-1][0] + ranges[-1][1] == S
    check_final(r, out, orgb, omean, where)


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["4", "2"])
@pytest.mark.parametrize("name", SCENES)
def test_preview_bits_with_inexact_scales(renders, name, pipeline, monkeypatch):
    """61 x 47 (ragged tiles), S = 7: the scales 7 / 1, 7 / 3 and 7 / 6 after the first three ranges; 7 / 3 and 7 / 6 are rounded, so
    (a * S) / n, an FMA or a reciprocal multiply would show.  Each preview twice: reading must not feed back."""
    monkeypatch.setenv("CRT_PIPELINE", pipeline)
    w, h, S = 61, 47, 7
    orgb, omean, L = oracle_frame(name, w, h, S)
    eye, iv, fov = util.camera(name)
    r = renders[name]
    r.set_spp(S)
    out = None
    for b, c in ((0, 1), (1, 2), (3, 3), (6, 1)):
        out = r.run_view_range(eye, iv, fov, b, c, width=w, height=h)
        if b + c < S:
            assert out is None
            check_preview(r, L, S, b + c, w, h, "%s pipeline %s" % (name, pipeline), times=2)
    check_final(r, out, orgb, omean, "%s pipeline %s" % (name, pipeline))
    with pytest.raises(crt.CrtError):
        r.preview(width=w, height=h)                      # nothing in flight after the range that ends the frame


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["4", "2"])
@pytest.mark.parametrize("name", SCENES)
def test_accumulator_bits_mid_flight(renders, name, pipeline, monkeypatch):
    """64 x 48, S = 8: after 2 and 4 samples the scales are 4 and 2, powers of two, so the preview's mean divided by the scale IS the
    accumulator (finite values far from overflow): c_n itself, whatever the scale's rounding."""
    monkeypatch.setenv("CRT_PIPELINE", pipeline)
    w, h, S = 64, 48, 8
    orgb, omean, L = oracle_frame(name, w, h, S)
    assert np.isfinite(L).all() and L.max() < 1e30
    eye, iv, fov = util.camera(name)
    r = renders[name]
    r.set_spp(S)
    out = None
    for b, c in ((0, 2), (2, 2), (4, 4)):
        out = r.run_view_range(eye, iv, fov, b, c, width=w, height=h)
        n = b + c
        if n < S:
            mean = check_preview(r, L, S, n, w, h, "%s pipeline %s" % (name, pipeline))
            assert F(S) / F(n) in (F(4), F(2))
            assert_bits(mean / (F(S) / F(n)), restated_sums(L, S, n)[0], "accumulator after %d samples" % n)
    check_final(r, out, orgb, omean, "%s pipeline %s" % (name, pipeline))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_previews_through_every_path_of_the_frame_logic(renders, name, monkeypatch):
    w, h = 64, 48
    r = renders[name]
    # 3 072 pixel slots: chunks of 2^13 paths hold two samples, so both ranges straddle chunk borders
    with monkeypatch.context() as m:
        m.setenv("CRT_CHUNK_LOG2", "13")
        launches = []
        run_ranges(r, name, w, h, 8, ((0, 3), (3, 5)), "small chunks", hook=lambda i, r: launches.append(r.stats["kernel_launches"]))
        assert launches == [2, 3]
        m.setenv("CRT_PIPELINE", "2")
        run_ranges(r, name, w, h, 8, ((0, 3), (3, 5)), "small chunks, wavefront pipeline")
    run_ranges(r, name, w, h, 8, ((0, 3), (3, 5)), "stats", stats=True)
    with monkeypatch.context() as m:
        m.setenv("CRT_PIPELINE", "2")
        run_ranges(r, name, w, h, 8, ((0, 3), (3, 5)), "stats, wavefront pipeline", stats=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_previews_between_ranges_with_and_without_the_commit_ring(name, monkeypatch):
    """A forced ring of 4 samples (CRT_COMMIT_RING_LOG2 = 2), S = 16: the ring launches sum inside the launch, the launches without
    it after the launch -- the accumulator between them must be c_n either way."""
    monkeypatch.delenv("CRT_PIPELINE", raising=False)
    w, h, S = 64, 48, 16
    r = fresh_render(name, S)                              # a fresh handle, as test_commit_ring.py uses
    try:
        monkeypatch.setenv("CRT_COMMIT_RING_LOG2", "2")
        rings = []
        run_ranges(r, name, w, h, S, ((0, 6), (6, 6), (12, 4)), "ring, ring, no ring", hook=lambda i, r: rings.append(r.radiance_storage()[1]))
        assert rings == [4, 4, 0], "the forced ring did not engage for the first two ranges: the check shows nothing"   # (the last range is not longer than the ring)

        def switch(i, r):
            rings.append(r.radiance_storage()[1])
            if i == 0:
                monkeypatch.delenv("CRT_COMMIT_RING_LOG2")
            else:
                monkeypatch.setenv("CRT_COMMIT_RING_LOG2", "2")
        del rings[:]
        run_ranges(r, name, w, h, S, ((0, 6), (6, 4), (10, 6)), "ring, no ring, ring", hook=switch)
        assert rings == [4, 0, 4]
    finally:
        r.free()


def shard_of(img, w, h, rank, world):
    """The compact-tile shard (slots, 3) of a row-major (h, w, 3) image: 8 x 8 tiles dealt round-robin to the ranks, 64 slots per tile
    in row-major order; padding slots (tiles beyond the frame, pixels beyond its right / bottom edge) 0.  Returns (shard, padding mask)."""
    slots = crt.shard_slots(w, h, rank, world)
    tx, ty = (w + 7) // 8, (h + 7) // 8
    s = np.arange(slots)
    tile = (s // 64) * world + rank
    i, j = (tile % tx) * 8 + (s % 64) % 8, (tile // tx) * 8 + (s % 64) // 8
    pad = (tile >= tx * ty) | (i >= w) | (j >= h)
    out = np.zeros((slots, 3), dtype=img.dtype)
    out[~pad] = img[j[~pad], i[~pad]]
    return out, pad


def range_call(r, name, w, h, rank, world, begin, count, rgb=None, mean=None):
    """crt_render_range on r's handle for a tiled shard, through the C ABI"""
    eye, iv, fov = util.camera(name)
    cam = r._cam(eye, iv, fov)
    prm = r._params(rank=rank, world=world, flags=capi.FLAG_TILED_OUTPUT, width=w, height=h)
    st = capi.Stats()
    return capi.lib().crt_render_range(r._h, C.byref(cam), C.byref(prm), begin, count, capi.ptr(rgb), capi.ptr(mean), C.byref(st))


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", SCENES)
def test_preview_of_tiled_shards(renders, name, world):
    from cudaraytracing_amd.distributed import untile_numpy
    w, h, S, n = 100, 70, 5, 2
    _, _, L = oracle_frame(name, w, h, S)
    _, p, prgb = restated_preview(L, S, n)
    r = renders[name]
    r.set_spp(S)
    rgbs, means, padding = [], [], 0
    for rank in range(world):
        capi.check(range_call(r, name, w, h, rank, world, 0, n), "crt_render_range")
        slots = crt.shard_slots(w, h, rank, world)
        rgb = np.full((slots, 3), 7, dtype=np.uint8)       # (every slot must be written, padding included)
        mean = np.full((slots, 3), 7, dtype=F)
        done = C.c_uint32()
        capi.check(capi.lib().crt_preview(r._h, capi.ptr(rgb), capi.ptr(mean), C.byref(done)), "crt_preview")
        assert done.value == n
        want_mean, pad = shard_of(p, w, h, rank, world)
        want_rgb, _ = shard_of(prgb, w, h, rank, world)
        assert_bits(mean, want_mean, "rank %d of %d" % (rank, world))
        assert np.array_equal(rgb, want_rgb), (rank, world)
        assert (rgb[pad] == 0).all() and (mean[pad].view(np.uint32) == 0).all(), (rank, world)
        padding += int(pad.sum())
        rgbs.append(rgb)
        means.append(mean)
    assert padding > 0
    assert_bits(untile_numpy(np.stack(means), w, h), p, "tiled, world %d" % world)
    assert np.array_equal(untile_numpy(np.stack(rgbs), w, h), prgb)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_device_forms_on_a_stream(renders, name):
    """crt_render_range_device and crt_preview_device on a caller's stream, rank 1 of 3: the device form has no host-side clearing of
    its buffers, so the 0x55 fill shows any slot -- a padding slot above all -- that the kernel does not write."""
    w, h, S, rank, world = 100, 70, 5, 1, 3
    orgb, omean, L = oracle_frame(name, w, h, S)
    _, p, prgb = restated_preview(L, S, 3)
    r = renders[name]
    r.set_spp(S)
    lib = capi.lib()
    eye, iv, fov = util.camera(name)
    cam = r._cam(eye, iv, fov)
    prm = r._params(rank=rank, world=world, flags=capi.FLAG_TILED_OUTPUT, width=w, height=h)
    slots = crt.shard_slots(w, h, rank, world)
    with DeviceBuffers({"rgb": slots * 3, "mean": slots * 12}, stream=True) as d:
        ptrs, stream = d.ptrs, C.c_void_p(d.stream)

        def fill():
            d.fill("rgb")
            d.fill("mean")

        def fetch():
            d.synchronize()
            return d.download("rgb", (slots, 3), np.uint8), d.download("mean", (slots, 3), F)

        capi.check(lib.crt_render_range_device(r._h, C.byref(cam), C.byref(prm), 0, 3, None, None, stream, None), "crt_render_range_device")
        done = C.c_uint32()
        capi.check(lib.crt_preview_device(r._h, C.c_void_p(ptrs["rgb"]), C.c_void_p(ptrs["mean"]), stream, C.byref(done)), "crt_preview_device")
        assert done.value == 3
        rgb, mean = fetch()
        # the host form of the same shard
        hrgb, hmean = np.full((slots, 3), 7, dtype=np.uint8), np.full((slots, 3), 7, dtype=F)
        capi.check(lib.crt_preview(r._h, capi.ptr(hrgb), capi.ptr(hmean), C.byref(done)), "crt_preview")
        assert done.value == 3
        assert_bits(mean, hmean, "device form against host form")
        assert np.array_equal(rgb, hrgb)
        # ... and both are the restatement's shard, padding slots RGB 0 and +0.0f
        want_mean, pad = shard_of(p, w, h, rank, world)
        want_rgb, _ = shard_of(prgb, w, h, rank, world)
        assert pad.any()
        assert_bits(mean, want_mean, "device form against the restatement")
        assert np.array_equal(rgb, want_rgb)
        assert (rgb[pad] == 0).all() and (mean[pad].view(np.uint32) == 0).all()
        # without a mean buffer: the same RGB, the mean buffer not touched
        fill()
        capi.check(lib.crt_preview_device(r._h, C.c_void_p(ptrs["rgb"]), None, stream, C.byref(done)), "crt_preview_device")
        rgb2, mean2 = fetch()
        assert np.array_equal(rgb2, rgb)
        assert (mean2.view(np.uint8) == 0x55).all()
        # the range that ends the frame, into the device buffers: the one-shot shard
        fill()
        capi.check(lib.crt_render_range_device(r._h, C.byref(cam), C.byref(prm), 3, 2, C.c_void_p(ptrs["rgb"]), C.c_void_p(ptrs["mean"]), stream, None),
                   "crt_render_range_device")
        rgb3, mean3 = fetch()
        one_rgb, one_mean = np.full((slots, 3), 7, dtype=np.uint8), np.full((slots, 3), 7, dtype=F)
        capi.check(lib.crt_render(r._h, C.byref(cam), C.byref(prm), capi.ptr(one_rgb), capi.ptr(one_mean), None), "crt_render")
        assert_bits(mean3, one_mean, "last range against one shot")
        assert np.array_equal(rgb3, one_rgb)
        assert_bits(mean3, shard_of(omean, w, h, rank, world)[0], "last range against the oracle")
        assert np.array_equal(rgb3, shard_of(orgb, w, h, rank, world)[0])


SOUP = dict(scale=1e12, w=48, h=36, S=4, n=2, seed=5, p_rr=0.6, lsn=2)


def soup_scene(d):
    obj, mtl = _write_scaled_soup_scene(str(d), SOUP["scale"])
    eye = (np.array([5.0, 5.0, 0.5]) * SOUP["scale"]).astype(F)
    iv = crt.get_inverse_view_matrix(eye, (np.array([5.0, 4.5, 9.0]) * SOUP["scale"]).astype(F), [0.0, 1.0, 0.0])
    return obj, mtl, eye, iv, crt.fov_to_radians(75.0)


@pytest.mark.gpu
def test_preview_of_non_finite_sums(tmp_path):
    """The soup scene of test_extreme_coordinate_scales scaled by 1e12 (48 x 36, S = 4, seed 5, p_rr 0.6, light_sample_n 2): products
    overflow and NaNs appear in the radiance.  Preview after samples [0, 2) against p_2 / rgb_2: NaN sums and finite sums go through
    the scale and the tone map side by side.
    The condition on the inputs, asserted below on the oracle's values alone: p_2 holds at least one NaN and at least one finite
    value.  It was meant to be "at least one finite NON-ZERO value"; the oracle cannot give that in this scene.  Checked on the CPU:
    with seed 5 and n = 2, p_2 has 984 NaNs among its 5 184 values and every other value is 0; the same holds for seeds 0 .. 11 at
    n = 1, 2, 3, because no sample of L is finite and non-zero at all.  The switch is global: up to a coordinate scale of 2.12e9 the
    scene has no NaN, from 2.15e9 on every finite radiance is exactly 0 (the light's own terms overflow), so no seed, n or scale of
    this scene has both.  Seed and n therefore stay as given; finite non-zero sums are what every other test of this file previews."""
    w, h, S, n = SOUP["w"], SOUP["h"], SOUP["S"], SOUP["n"]
    obj, mtl, eye, iv, fov = soup_scene(tmp_path)
    osc = O.OracleScene([(obj, mtl)], 2)
    orgb, omean, L, _ = osc.render(eye, iv, fov, w, h, S, SOUP["p_rr"], SOUP["lsn"], seed=SOUP["seed"], want_L=True)
    assert np.array_equal(restated_sums(L, S, S)[0].view(np.uint32), omean.view(np.uint32))
    _, p, prgb = restated_preview(L, S, n)
    assert np.isnan(p).any() and np.isfinite(p).any()
    scene = crt.Scene(w, h)
    scene.add_obj(obj, mtl)
    scene.set_BVH(2)
    r = crt.Render(scene, S, SOUP["p_rr"], SOUP["lsn"])
    r.seed = SOUP["seed"]
    try:
        assert r.run_view_range(eye, iv, fov, 0, n) is None
        rgb, mean, done = r.preview(want_mean=True)
        assert done == n
        assert_bits(mean, p, "preview of the 1e12 soup")
        assert np.array_equal(rgb, prgb)
        out = r.run_view_range(eye, iv, fov, n, S - n)
        check_final(r, out, orgb, omean, "1e12 soup")
    finally:
        r.free()


def refused(call):
    """call() raises CrtError / CRT_ERR_INVALID_ARG, and the library's own message names crt_render_range and what it expected"""
    with pytest.raises(crt.CrtError) as e:
        call()
    assert e.value.status == capi.ERR_INVALID_ARG
    msg = capi.lib().crt_last_error().decode()
    assert "crt_render_range" in msg and "expected" in msg, msg
    assert msg in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_a_range_that_does_not_continue_the_frame_in_flight_is_refused(name):
    w, h, S = 32, 24, 6
    orgb, omean, L = oracle_frame(name, w, h, S)
    eye, iv, fov = util.camera(name)
    r = fresh_render(name, S)
    kw = dict(width=w, height=h)

    def rng(b, c, **over):
        return r.run_view_range(eye, iv, fov, b, c, **dict(kw, **over))

    def still_in_flight_then_finish(n, where):
        """after a refusal: the frame in flight is as it was -- previewed, then continued to the oracle's frame"""
        check_preview(r, L, S, n, w, h, where)
        check_final(r, rng(n, S - n), orgb, omean, where)

    def other_spp():
        r.set_spp(7)
        try:
            rng(2, 2)
        finally:
            r.set_spp(S)

    try:
        refused(lambda: rng(2, 2))                                            # on a fresh handle
        with pytest.raises(crt.CrtError):
            r.preview(**kw)
        assert rng(0, 2) is None
        refused(lambda: rng(3, 1))                                            # a gap
        still_in_flight_then_finish(2, "after a gap")
        assert rng(0, 3) is None
        refused(lambda: rng(2, 2))                                            # an overlap
        still_in_flight_then_finish(3, "after an overlap")
        assert rng(0, 2) is None
        refused(lambda: rng(2, 2, width=40))                                  # another size
        still_in_flight_then_finish(2, "after another size")
        assert rng(0, 2) is None
        refused(other_spp)                                                    # another spp
        still_in_flight_then_finish(2, "after another spp")
        assert rng(0, 2) is None
        refused(lambda: capi.check(range_call(r, name, w, h, 0, 2, 2, 2), "crt_render_range"))   # another shard and layout
        still_in_flight_then_finish(2, "after another shard")
        assert np.array_equal(r.run_view(eye, iv, fov, **kw), orgb)
        refused(lambda: rng(2, 2))                                            # after a finished frame
        with pytest.raises(crt.CrtError):
            r.preview(**kw)
        # legal: a restart ...
        assert rng(0, 2) is None and rng(0, 2) is None
        still_in_flight_then_finish(2, "after a restart")
        # ... and a call that does not touch the accumulator, at another size, between two ranges
        assert rng(0, 2) is None
        r.run_view_aov(eye, iv, fov, width=16, height=12)
        still_in_flight_then_finish(2, "after an AOV pass at another size")
    finally:
        r.free()
