"""The per-path radiance between the render kernel and the fold: 12 bytes per work item (include/crt.h), written by
k_mega3's render form and by the wavefront pipeline's k_logic, read by fold_samples (k_accumulate, k_accumulate_var, the adaptive
accumulate), and per entry of the commit ring.  crt_intersect's answers keep their 16-byte entries, and the event pairs of a timed
frame are read after its one synchronisation.  None of this may change a result: every frame below is the oracle's, bit for bit -- float32 mean,
RGB8, ray counts -- at the smallest shapes where an entry addressed with the wrong stride, a slot of a ragged tile or a sum carried
between chunks would show.

The frame: cornell-box 44 x 20 (6 x 3 tiles of 8 x 8, ragged in both directions: 1 152 pixel slots for 880 pixels) at spp 5.
"""
import ctypes as C

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
import util
from frames import oracle_render
from util import assert_bits
from variance_restated import restated_adaptive, restated_variance

F = np.float32
NAME, W, H, SPP = "cornell-box", 44, 20, 5
NSLOTS = 6 * 3 * 64
COUNTERS = ("paths", "rays", "shadow_rays", "probe_rays")
MODES = [crt.TRAVERSAL_EXACT, crt.TRAVERSAL_REFERENCE]
PIPELINES = ["4", "2"]   # CRT_PIPELINE: the megakernel, the wavefront fallback


@pytest.fixture(scope="module")
def render():
    t = util.task(NAME)
    r = crt.Render(util.host_scene(NAME), SPP, t.P_RR, t.light_sample_n)
    yield r
    r.free()


@pytest.fixture(autouse=True)
def default_settings(request):
    """Every test leaves the shared handle's settings as it found them"""
    yield
    if "render" in request.fixturenames:
        r = request.getfixturevalue("render")
        r.set_spp(SPP)
        r.seed, r.traversal, r.extra_flags = 0, crt.TRAVERSAL_EXACT, 0


def frame(r, stats=False, want_variance=False, w=W, h=H):
    eye, iv, fov = util.camera(NAME)
    rgb = r.run_view(eye, iv, fov, stats=stats, width=w, height=h, want_variance=want_variance).copy()
    return rgb, r.mean_buffer.copy(), dict(r.stats)


def check_frame(rgb, mean, where, want=None):
    orgb, omean = (want or oracle_render(NAME, W, H, SPP))[:2]
    assert_bits(mean, omean, where + ": mean")
    assert np.array_equal(rgb, orgb), where + ": RGB8"


def check_counters(st, where, want=None):
    ost = want or oracle_render(NAME, W, H, SPP)[3]
    for k in COUNTERS:
        assert st[k] == ost[k], (where, k, st[k], ost[k])


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("mode", MODES)
def test_ragged_frame_whole_and_as_a_shard(render, mode, pipeline, monkeypatch):
    monkeypatch.setenv("CRT_PIPELINE", pipeline)
    r = render
    r.traversal = mode
    where = "traversal %d, pipeline %s" % (mode, pipeline)
    rgb, mean, st = frame(r)
    check_frame(rgb, mean, where)
    check_counters(st, where)
    # rank 1 of 3, tiled: local tile lt is tile 3 lt + 1 of the frame's 18; every slot against the oracle's pixel, padding slots +0 / 0
    orgb, omean = oracle_render(NAME, W, H, SPP)[:2]
    eye, iv, fov = util.camera(NAME)
    rank, world = 1, 3
    slots = crt.shard_slots(W, H, rank, world)
    assert slots == 6 * 64
    srgb = np.full((slots, 3), 9, dtype=np.uint8)
    smean = np.full((slots, 3), 9, dtype=F)
    cam = r._cam(eye, iv, fov)
    prm = r._params(rank=rank, world=world, flags=capi.FLAG_TILED_OUTPUT, width=W, height=H)
    sst = capi.Stats()
    capi.check(capi.lib().crt_render(r._h, C.byref(cam), C.byref(prm), capi.ptr(srgb), capi.ptr(smean), C.byref(sst)), "crt_render")
    want_rgb, want_mean = np.zeros_like(srgb), np.zeros_like(smean)
    pixels = 0
    for s in range(slots):
        tile = (s // 64) * world + rank
        i, j = (tile % 6) * 8 + (s % 64) % 8, (tile // 6) * 8 + (s % 64) // 8
        if tile < 18 and i < W and j < H:
            want_rgb[s], want_mean[s] = orgb[j, i], omean[j, i]
            pixels += 1
    assert 0 < pixels < slots
    assert_bits(smean, want_mean, where + ", rank 1 of 3: mean")
    assert np.array_equal(srgb, want_rgb), where + ", rank 1 of 3: RGB8"
    assert sst.as_dict()["paths"] == pixels * SPP


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_progressive_ranges_carry_the_sum_across_chunks(render, pipeline, monkeypatch):
    """(0, 2) then (2, 3): the first chunk starts the sums, the last one adds to what the first left and writes the frame"""
    monkeypatch.setenv("CRT_PIPELINE", pipeline)
    r = render
    eye, iv, fov = util.camera(NAME)
    one_rgb, one_mean, _ = frame(r)
    assert r.run_view_range(eye, iv, fov, 0, 2, width=W, height=H) is None
    paths = r.stats["paths"]
    rgb = r.run_view_range(eye, iv, fov, 2, 3, width=W, height=H)
    assert paths == W * H * 2 and r.stats["paths"] == W * H * 3
    check_frame(rgb, r.mean_buffer, "ranges (0, 2), (2, 3), pipeline " + pipeline)
    check_frame(one_rgb, one_mean, "one shot, pipeline " + pipeline)
    # ... and one call in chunks of one sample (2^11 work items hold one sample's 1 152): five launches, four carried sums
    monkeypatch.setenv("CRT_CHUNK_LOG2", "11")
    rgb, mean, st = frame(r)
    check_frame(rgb, mean, "chunks of one sample, pipeline " + pipeline)
    check_counters(st, "chunks of one sample, pipeline " + pipeline)
    if pipeline == "4":
        assert st["kernel_launches"] == 5


@pytest.mark.gpu
def test_variance_sums_and_an_adaptive_pass(render, monkeypatch):
    """fold_samples' VAR arm (k_accumulate_var, the adaptive accumulate): expected values restated in numpy float32 on the oracle's
    per-path radiance, as tests/test_variance.py and tests/test_adaptive.py do"""
    r = render
    L = oracle_render(NAME, W, H, SPP)[2]
    want_var = restated_variance(L, SPP)
    assert (want_var > 0).any()
    for chunk_log2 in (None, "11"):
        with monkeypatch.context() as m:
            if chunk_log2:
                m.setenv("CRT_CHUNK_LOG2", chunk_log2)
            where = "FLAG_VARIANCE, chunk log2 %s" % chunk_log2
            rgb, mean, _ = frame(r, want_variance=True)
            check_frame(rgb, mean, where)
            assert_bits(r.variance_buffer, want_var, where)
    # one adaptive pass: 2 samples for every pixel, then 3 more for the 239 pixels the criterion leaves active (a sparse pass: not a
    # multiple of 64, its work items go through the item list)
    ad = dict(min_samples=2, step_samples=3, threshold=0.2, mean_floor=0.01)
    want = restated_adaptive(L, SPP, **ad)
    assert want["pass_pixels"] == [239] and want["passes"] == 2
    eye, iv, fov = util.camera(NAME)
    rgb = r.run_view_adaptive(eye, iv, fov, want_variance=True, width=W, height=H, **ad)
    assert np.array_equal(r.samples_buffer, want["samples"])
    assert_bits(r.mean_buffer, want["mean"], "adaptive: mean")
    assert np.array_equal(rgb, want["rgb"])
    assert_bits(r.variance_buffer, want["variance"], "adaptive: variance")
    assert r.adaptive_info["pass_pixels"] == want["pass_pixels"]
    assert r.adaptive_info["passes"] == 2 and r.adaptive_info["paths"] == want["paths"]
    rgb, mean, _ = frame(r)   # a plain frame afterwards
    check_frame(rgb, mean, "after the adaptive frame")


@pytest.mark.gpu
def test_commit_ring_gives_the_same_frame(render, monkeypatch):
    r = render
    monkeypatch.setenv("CRT_COMMIT_RING_LOG2", "1")   # a ring of two samples for the frame's five
    r.extra_flags = crt.FLAG_BOUNDED_RADIANCE
    rgb, mean, st = frame(r)
    nbytes, ring_samples = r.radiance_storage()
    assert ring_samples == 2, "the ring did not engage"
    assert nbytes == 12 * 2 * 64 * 64   # 64 cursor shards of 64 pixel slots (1 152 / 64 = 18, up to a whole tile) per ring sample
    check_frame(rgb, mean, "forced ring with the flag")
    check_counters(st, "forced ring with the flag")
    r.extra_flags = 0
    rgb, mean, _ = frame(r)
    assert r.radiance_storage()[1] == 2
    check_frame(rgb, mean, "forced ring")
    monkeypatch.delenv("CRT_COMMIT_RING_LOG2")
    rgb, mean, _ = frame(r)
    assert r.radiance_storage() == (12 * NSLOTS * SPP, 0)
    check_frame(rgb, mean, "without the ring again")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_render_intersect_render_on_one_handle(mode):
    """The render's 12-byte entries and crt_intersect's 16-byte answers live in one allocation that grows to the larger use: a tiny
    frame (64 entries), 512 rays (the answers need more), the frame (its radiance needs more still), the rays again (they fit)"""
    t = util.task(NAME)
    r = crt.Render(util.host_scene(NAME), SPP, t.P_RR, t.light_sample_n)   # a fresh handle: nothing allocated yet
    try:
        r.traversal = mode
        o, d = util.random_rays(NAME, 512, seed=23)
        otri, ot, _ = util.oracle_scene(NAME).intersect(o, d)
        assert 100 < (otri >= 0).sum()

        def rays(where):
            tri, tt = r.intersect(o, d, traversal=mode)
            assert np.array_equal(tri, otri), where
            assert np.array_equal(util.bits(tt), util.bits(ot)), where

        r.set_spp(1)
        rgb, mean, _ = frame(r, w=8, h=8)
        check_frame(rgb, mean, "8 x 8 spp 1", want=oracle_render(NAME, 8, 8, 1))
        assert r.radiance_storage()[0] == 12 * 64
        rays("after the tiny frame")
        r.set_spp(SPP)
        rgb, mean, st = frame(r)
        check_frame(rgb, mean, "after crt_intersect")
        check_counters(st, "after crt_intersect")
        rays("after the frame")
        rgb, mean, _ = frame(r)
        check_frame(rgb, mean, "after crt_intersect again")
    finally:
        r.free()


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_radiance_storage_is_12_bytes_per_path_of_a_chunk(render, pipeline, monkeypatch):
    monkeypatch.setenv("CRT_PIPELINE", pipeline)
    frame(render)
    assert render.radiance_storage() == (12 * NSLOTS * SPP, 0)
    monkeypatch.setenv("CRT_CHUNK_LOG2", "12")   # 2^12 work items: three samples of 1 152 slots
    frame(render)
    assert render.radiance_storage() == (12 * NSLOTS * 3, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_deep_paths_through_specular_vertices(mode):
    """veach-mis, the crop (368, 268) 32 x 24 of the 800 x 600 frame at spp 8: paths that go on from SPECULAR vertices (the oracle counts
    1 748 probe rays in the crop), so the backward recursion reads cosines and the records of the incoming directions together"""
    name, spp, crop = "veach-mis", 8, (368, 268, 32, 24)
    t = util.task(name)
    orgb, omean, _, ost = oracle_render(name, t.width, t.height, spp, crop=crop)
    assert ost["probe_rays"] > 1000 and ost["rays"] > 7 * ost["paths"]
    eye, iv, fov = util.camera(name)
    r = crt.Render(util.host_scene(name), spp, t.P_RR, t.light_sample_n)
    try:
        r.traversal = mode
        for pipeline in PIPELINES:
            with pytest.MonkeyPatch.context() as m:
                m.setenv("CRT_PIPELINE", pipeline)
                rgb = r.run_view(eye, iv, fov)
            x0, y0, cw, ch = crop
            assert_bits(r.mean_buffer[y0:y0 + ch, x0:x0 + cw], omean, "pipeline %s: mean" % pipeline)
            assert np.array_equal(rgb[y0:y0 + ch, x0:x0 + cw], orgb), pipeline
            assert r.stats["paths"] == t.width * t.height * spp
    finally:
        r.free()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_stats_of_a_frame_in_two_launches(render, mode, monkeypatch):
    """The timed frame enqueues every launch and fold without waiting and reads its event pairs at the end: launches and ray counters with
    CRT_FLAG_STATS are those without it, and the oracle's"""
    monkeypatch.setenv("CRT_CHUNK_LOG2", "12")   # three samples per launch: (0, 3), (3, 2)
    r = render
    r.traversal = mode
    rgb0, mean0, st0 = frame(r, stats=False)
    rgb1, mean1, st1 = frame(r, stats=True)
    assert st0["kernel_launches"] == 2 == st1["kernel_launches"]
    for k in COUNTERS:
        assert st0[k] == st1[k], k
    check_counters(st1, "stats on")
    check_frame(rgb0, mean0, "stats off")
    check_frame(rgb1, mean1, "stats on")
    for st in (st0, st1):
        assert 0 < st["kernel_ms"] <= st["total_ms"]
    assert r.last_launch_ms()[1] == 2
