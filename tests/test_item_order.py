"""GPU tests of the order in which k_mega3 is handed the last work items of a launch (k_order_items, csrc/crt_item_order.h: the end of
every cursor shard sorted into classes of descending roulette length) and of the list's reuse from launch to launch (crt_item_order,
include/crt.h).  The order of the work items cannot change a result -- every path writes its own L[item] -- so every frame here must be,
bit for bit (f32 means and RGB8) and counter for counter, the frame handed out in cursor order (CRT_ITEM_ORDER=0); a work item that an
order loses or lists twice changes `paths`.  The code reads the environment at every frame, so one process switches between the orders.

Sizes.  A launch without the commit ring has 64 cursor shards of roundup64(ceil(slots x spp / 64)) work items, ordered in spans of 1 024:
  cornell-box 52 x 44   7 x 6 tiles of 8 x 8 (ragged in both directions: padding slots) = 2 688 slots; spp 40: 107 520 items, 1 680 per shard
                        -> 1 728 = one span and 704 items; shard 62 holds the last 384 items, shard 63 none
  veach-mis 48 x 40     6 x 5 tiles = 1 920 slots (SPECULAR probes); spp 40: 76 800 items, 1 200 per shard -> 1 216 = one span and 192 items
  rank 3 of 8, 52 x 44  tiles 3, 11, .., 43 of 42 (the last one beyond the frame) = 384 slots; spp 200: 76 800 items -> 1 216 per shard
  the commit ring       CRT_FLAG_BOUNDED_RADIANCE picks a ring of 1 024 samples for 2 688 slots, so spp 1 100 (more than the ring) takes it:
                        64 shards of 64 slots x 1 100 samples = 70 400 items = 68 spans and 768 items, 22 of them beyond the frame's slots;
                        the window is at most half the ring, 512 x 64 items
CRT_ORDER_WINDOW=1000 is smaller than every one of these shards and no whole number of spans; 1 << 20 is larger than all of them."""
import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd.hipmem import DeviceBuffers
import util

pytestmark = pytest.mark.gpu

ORDERS = {"none": {"CRT_ITEM_ORDER": "0"}, "default": {}, "window 1000": {"CRT_ORDER_WINDOW": "1000"}, "whole shards": {"CRT_ORDER_WINDOW": str(1 << 20)},
          "two classes": {"CRT_ORDER_CLASSES": "2"}, "eight classes": {"CRT_ORDER_CLASSES": "2,3,4,5,7,9,13"}}
CLASSES = {"none": 0, "two classes": 2, "eight classes": 8}  # what crt_item_order reports for them
COUNTERS = ("rays", "paths", "shadow_rays", "rays_untraced")


def _set_order(monkeypatch, env):
    for k in ("CRT_ITEM_ORDER", "CRT_ORDER_WINDOW", "CRT_ORDER_CLASSES", "CRT_COMMIT_RING_LOG2"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _render(name, spp):
    t = util.task(name)
    return crt.Render(util.host_scene(name), spp, t.P_RR, t.light_sample_n, device=0)


def _frame(r, name, w, h):
    """(rgb, bits of the f32 mean, counters) of a whole frame"""
    eye, iv, fov = util.camera(name)
    rgb = r.run_view(eye, iv, fov, width=w, height=h).copy()
    return rgb, util.bits(r.mean_buffer).copy(), {k: r.stats[k] for k in COUNTERS}


def _shard_frame(r, name, w, h, rank, world):
    """the same for the compact tiles of rank / world, outputs in device memory (run_view_device; with stats the call synchronizes)"""
    eye, iv, fov = util.camera(name)
    slots = crt.shard_slots(w, h, rank, world)
    with DeviceBuffers({"rgb": slots * 3, "mean": slots * 12}) as d:
        st = r.run_view_device(eye, iv, fov, d.ptrs["rgb"], d.ptrs["mean"], None, rank=rank, world=world, tiled=True, want_stats=True, width=w, height=h)
        rgb, mean = d.download("rgb", (slots, 3), np.uint8), d.download("mean", (slots, 3), np.float32)   # (after the null stream's work)
    return rgb, util.bits(mean), {k: st[k] for k in COUNTERS}


def _assert_same(got, ref, where):
    assert np.array_equal(got[1], ref[1]), "%s: %d of %d floats of the mean differ" % (where, int((got[1] != ref[1]).sum()), ref[1].size)
    assert np.array_equal(got[0], ref[0]), "%s: the RGB8 frames differ" % where
    assert got[2] == ref[2], "%s: counters %r, in cursor order %r" % (where, got[2], ref[2])


def _under_every_order(monkeypatch, r, render, expect_window):
    """renders under every entry of ORDERS on the handle r, compares with the frame in cursor order; expect_window(name) -> the window
    crt_item_order must report"""
    frames = {}
    for order, env in ORDERS.items():
        _set_order(monkeypatch, env)
        frames[order] = render()
        info = r.item_order()
        want = expect_window(order)
        assert info["window"] == want, (order, info, want)
        if order in CLASSES:
            assert info["classes"] == CLASSES[order], (order, info)
        else:  # the default classes: chosen by measurement, at most eight
            assert 2 <= info["classes"] <= 8, (order, info)
    ref = frames["none"]
    assert ref[2]["paths"] > 0 and ref[0].std() > 5
    for order in ORDERS:
        _assert_same(frames[order], ref, order)


@pytest.mark.parametrize("name,w,h,spp,per_shard", [("cornell-box", 52, 44, 40, 1728), ("veach-mis", 48, 40, 40, 1216)])
def test_frame_and_counters_under_every_order(monkeypatch, name, w, h, spp, per_shard):
    slots = ((w + 7) // 8) * ((h + 7) // 8) * 64
    assert ((slots * spp + 63) // 64 + 63) // 64 * 64 == per_shard and per_shard > 1024 and per_shard % 1024  # (the arithmetic of the docstring)
    r = _render(name, spp)
    try:
        _under_every_order(monkeypatch, r, lambda: _frame(r, name, w, h),
                           lambda order: {"none": 0, "window 1000": 1000}.get(order, per_shard))
        assert r.stats["paths"] == w * h * spp
    finally:
        r.free()


def test_rank_3_of_8_under_every_order(monkeypatch):
    name, w, h, spp, per_shard = "cornell-box", 52, 44, 200, 1216
    assert crt.shard_slots(w, h, 3, 8) == 384 and ((384 * spp + 63) // 64 + 63) // 64 * 64 == per_shard
    r = _render(name, spp)
    try:
        _under_every_order(monkeypatch, r, lambda: _shard_frame(r, name, w, h, 3, 8),
                           lambda order: {"none": 0, "window 1000": 1000}.get(order, per_shard))
    finally:
        r.free()


def test_the_commit_ring_under_every_order(monkeypatch):
    name, w, h, spp = "cornell-box", 52, 44, 1100
    r = _render(name, spp)
    try:
        r.extra_flags = crt.FLAG_BOUNDED_RADIANCE

        def render():
            f = _frame(r, name, w, h)
            assert r.radiance_storage()[1] == 1024 and r.stats["kernel_launches"] == 1  # the ring, one launch
            return f
        # 64 slots x 1 100 samples per shard; the window may span half the ring
        _under_every_order(monkeypatch, r, render, lambda order: {"none": 0, "window 1000": 1000}.get(order, min(64 * spp, 512 * 64)))
        # ... and the frame is the one without the ring
        _set_order(monkeypatch, {})
        r.extra_flags = 0
        plain = _frame(r, name, w, h)
        assert r.radiance_storage()[1] == 0
        r.extra_flags = crt.FLAG_BOUNDED_RADIANCE
        ring = _frame(r, name, w, h)
        assert np.array_equal(ring[1], plain[1]) and np.array_equal(ring[0], plain[0])
    finally:
        r.free()


def test_the_list_is_built_once_per_key(monkeypatch):
    """One handle through a sequence of launches: the list is built again for every change of what it depends on and taken as it is when
    nothing changed (the camera is not part of that); every frame is the frame of a fresh handle."""
    name, w, h, spp = "cornell-box", 52, 44, 40
    eye, iv, fov = util.camera(name)
    _set_order(monkeypatch, {})

    def fresh(seed, spp_, shot):
        f = _render(name, spp_)
        try:
            f.seed = seed
            return shot(f)
        finally:
            f.free()

    def whole(q):
        return _frame(q, name, w, h)

    def two_ranges(q):  # samples [0, 24) and [24, spp): two launches with different first samples
        q.run_view_range(eye, iv, fov, 0, 24, width=w, height=h)
        rgb = q.run_view_range(eye, iv, fov, 24, q.spp - 24, width=w, height=h).copy()
        return rgb, util.bits(q.mean_buffer).copy(), None

    def shard(q):
        return _shard_frame(q, name, w, h, 1, 3)

    r = _render(name, spp)
    try:
        built = reused = 0

        def step(what, seed, spp_, shot, builds, reuses):
            nonlocal built, reused
            r.seed = seed
            r.set_spp(spp_)
            got = shot(r)
            info = r.item_order()
            built, reused = built + builds, reused + reuses
            assert (info["lists_built"], info["lists_reused"]) == (built, reused), (what, info, built, reused)
            want = fresh(seed, spp_, shot)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]) and got[2] == want[2], what

        step("seed 1", 1, spp, whole, 1, 0)
        step("seed 1 again", 1, spp, whole, 0, 1)
        step("seed 2", 2, spp, whole, 1, 0)
        step("seed 1 after seed 2", 1, spp, whole, 1, 0)          # (one list per handle)
        step("after set_spp", 1, 56, whole, 1, 0)
        step("the same again", 1, 56, whole, 0, 1)
        step("two sample ranges", 1, 56, two_ranges, 2, 0)
        step("the two ranges again", 1, 56, two_ranges, 2, 0)     # (each range displaces the other's list)
        step("rank 1 of 3", 1, 56, shard, 1, 0)
        step("rank 1 of 3 again", 1, 56, shard, 0, 1)
        step("the whole frame", 1, 56, whole, 1, 0)
        # another camera is the same key ...
        r.run_view((eye[0] + 0.1, eye[1], eye[2]), iv, fov, width=w, height=h)
        assert r.item_order()["lists_reused"] == reused + 1 and r.item_order()["lists_built"] == built
        reused += 1
        # ... another window or class setting is not, and neither is coming back from no order at all
        for env in ({"CRT_ORDER_WINDOW": "1000"}, {"CRT_ORDER_WINDOW": "1000", "CRT_ORDER_CLASSES": "2"}, {"CRT_ORDER_CLASSES": "2"}, {}):
            _set_order(monkeypatch, env)
            step("order %r" % (env,), 1, 56, whole, 1, 0)
        _set_order(monkeypatch, {"CRT_ITEM_ORDER": "0"})
        step("no order", 1, 56, whole, 0, 0)
        assert r.item_order()["window"] == 0 and r.item_order()["classes"] == 0
        _set_order(monkeypatch, {})
        step("the default after no order", 1, 56, whole, 0, 1)  # (the list on the handle is still the one of this key)
    finally:
        r.free()
