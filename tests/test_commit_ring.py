"""GPU tests of the commit ring (CRT_FLAG_BOUNDED_RADIANCE, csrc/crt_path.h: ring_publish / ring_commit): the frame's sum
c += L_k / spp (reference: Render.cuh:348) made in sample order INSIDE the launch with radiance storage for a window of samples.
The ring changes where and when the additions happen, never their order: every frame here must be, bit for bit (f32 sums and RGB8),
the frame of the default path, which keeps one radiance per path and sums after the launch."""
import os

import numpy as np
import pytest

import cudaraytracing_amd as crt
import parity_cases as PC
import util
from parity_cases import _render

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,w,h,spp,ring_log2", [("cornell-box", 128, 96, 64, 2), ("cornell-box", 128, 96, 64, 3), ("cornell-box", 203, 149, 48, 2),
                                                    ("veach-mis", 160, 120, 40, 2), ("cornell-box", 64, 64, 200, 4), ("cornell-box", 37, 21, 70, 1)])
def test_tiny_rings_reproduce_the_frame(name, w, h, spp, ring_log2):
    PC.tiny_ring_reproduces_the_frame(name, w, h, spp, ring_log2)


def test_the_flag_picks_a_ring_and_one_launch():
    PC.flag_picks_a_ring_and_one_launch()


def test_a_shard_of_the_frame_through_the_ring():
    PC.shard_through_the_ring_is_the_shard_without_it()


def test_progressive_ranges_with_and_without_the_ring():
    """Sample ranges submitted one after the other (crt_render_range): a ring launch continues the accumulator a launch without
    the ring left, and the other way round."""
    name, w, h, spp = "cornell-box", 96, 64, 96
    ref = _render(name, w, h, spp)
    old = os.environ.pop("CRT_COMMIT_RING_LOG2", None)
    try:
        t = util.task(name)
        eye, iv, fov = util.camera(name)
        r = crt.Render(util.host_scene(name), spp, t.P_RR, t.light_sample_n, device=0)
        try:
            os.environ["CRT_COMMIT_RING_LOG2"] = "2"
            r.run_view_range(eye, iv, fov, 0, 40, width=w, height=h)       # ring (4 samples)
            os.environ.pop("CRT_COMMIT_RING_LOG2")
            r.run_view_range(eye, iv, fov, 40, 16, width=w, height=h)      # one radiance per path
            os.environ["CRT_COMMIT_RING_LOG2"] = "3"
            rgb = r.run_view_range(eye, iv, fov, 56, 40, width=w, height=h).copy()   # ring (8 samples), ends the frame
            bad = util.bits(r.mean_buffer) != util.bits(ref[1])
            assert not bad.any(), "%d of %d floats differ, first at %s: %r vs %r" % (
                int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), r.mean_buffer[bad][:4].tolist(), ref[1][bad][:4].tolist())
            assert np.array_equal(rgb, ref[0])
        finally:
            r.free()
    finally:
        os.environ.pop("CRT_COMMIT_RING_LOG2", None)
        if old is not None:
            os.environ["CRT_COMMIT_RING_LOG2"] = old


def test_cli_flag_for_the_ring(tmp_path):
    """crt_cli --bounded-radiance (crt::Render::set_flags): the same PNG as without it (320 samples: more than the 256-sample ring a
    160 x 120 frame gets, so the ring is really used)."""
    import subprocess
    from PIL import Image
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    cfg = util.SCENES["cornell-box"]
    outs = []
    for extra in ([], ["--bounded-radiance"]):
        out = str(tmp_path / ("c%d.png" % len(extra)))
        r = subprocess.run([cli, cfg, "-o", out, "--spp", "320", "--width", "160", "--height", "120", "--seed", "7", "--base-dir", util.ROOT] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append(np.asarray(Image.open(out)).copy())
    assert np.array_equal(outs[0], outs[1]) and outs[0].std() > 10


def test_ring_under_the_multi_device_entry():
    """crt_multi_render with three ranks on the one device and CRT_FLAG_BOUNDED_RADIANCE passed through: every rank's scene handle
    renders its shard with its own ring (ranks sharing a device never wait for one another: a commit only needs work that resident
    waves of the same launch already hold); the gathered frame is the single-device frame."""
    name, w, h, spp = "cornell-box", 120, 88, 300
    t = util.task(name)
    eye, iv, fov = util.camera(name)
    ref = _render(name, w, h, spp)
    m = crt.MultiRender(util.host_scene(name), spp, t.P_RR, t.light_sample_n, devices=[0, 0, 0], gather=crt.GATHER_COPY)
    old = os.environ.pop("CRT_COMMIT_RING_LOG2", None)
    os.environ["CRT_COMMIT_RING_LOG2"] = "3"   # (a share of 3 520 pixel slots would get a ring longer than the 300 samples: 8 samples forced)
    try:
        m.extra_flags = crt.FLAG_BOUNDED_RADIANCE
        got = m.run_view(eye, iv, fov, width=w, height=h)
        assert np.array_equal(got, ref[0]) and np.array_equal(util.bits(m.mean_buffer), util.bits(ref[1]))
        assert m.info["paths"] == w * h * spp
    finally:
        os.environ.pop("CRT_COMMIT_RING_LOG2", None)
        if old is not None:
            os.environ["CRT_COMMIT_RING_LOG2"] = old
        m.free()
