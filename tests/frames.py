"""Frames for the tests, stated once: the module-scoped `renders` fixture (one crt.Render per shipped scene), the oracle's frame with
its per-path radiance, and a GPU frame with its buffers and guides.  A test file takes the fixture with
`from frames import renders  # noqa: F401` among its imports."""
import functools

import numpy as np
import pytest

import cudaraytracing_amd as crt
import oracle_lib as O
import util

SCENES = ("cornell-box", "veach-mis")
GUIDES = ("albedo", "normal", "depth")


def fresh_render(name, spp=None):
    """A handle of its own on a shipped scene, with the scene's P_RR and light_sample_n (spp: the scene's unless given)"""
    t = util.task(name)
    return crt.Render(util.host_scene(name), t.spp if spp is None else spp, t.P_RR, t.light_sample_n)


def scene_renders(names=SCENES, spp=None):
    """The generator behind `renders`: {name: Render} with the scene's own spp (or `spp`), every handle freed afterwards"""
    out = {}
    for name in names:
        out[name] = fresh_render(name, spp)
    yield out
    for r in out.values():
        r.free()


@pytest.fixture(scope="module")
def renders(request):
    """One Render per shipped scene for the importing module; a module that states RENDER_SPP gets handles created with that spp."""
    yield from scene_renders(spp=getattr(request.module, "RENDER_SPP", None))


@functools.lru_cache(maxsize=None)
def oracle_render(name, w, h, spp, seed=0, crop=None):
    """(rgb, mean, L (h, w, spp, 3), stats) of the oracle at the scene's own camera, P_RR and light_sample_n, computed once, the arrays
    read-only; of a crop (x0, y0, w, h) without L.  The inputs are checked before any test relies on them: summing L / S as the
    contracts do gives the oracle's own mean bit for bit, and its tone map the oracle's RGB."""
    t = util.task(name)
    eye, iv, fov = util.camera(name)
    rgb, mean, L, st = util.oracle_scene(name).render(eye, iv, fov, w, h, spp, t.P_RR, t.light_sample_n, seed=seed, crop=crop, want_L=crop is None)
    if L is not None:
        c, _ = util.restated_sums(L, spp, spp)
        assert np.array_equal(c.view(np.uint32), mean.view(np.uint32)), "summing L / S in numpy does not give the oracle's own mean"
        assert np.array_equal(O.tonemap(c), rgb)
        L.flags.writeable = False
    rgb.flags.writeable = mean.flags.writeable = False
    return rgb, mean, L, st


def oracle_frame(name, w, h, spp, seed=0):
    """(rgb, mean, L) of oracle_render"""
    return oracle_render(name, w, h, spp, seed)[:3]


def gpu_frame(r, name, width, height, spp, seed=0, cam=None, traversal=crt.TRAVERSAL_EXACT, flags=0, want_variance=False, want_halves=False,
              stats=False, render=True, aov=None, shading=None):
    """A GPU frame on the handle r at the camera of scene `name` (or `cam`), then the guides from the same settings: aov = the `want`
    of run_view_aov, shading = the `first` of run_view_aov_shading.  Returns {rgb, mean, variance, half_a, half_b} (copies; None where
    the handle holds none after the render; nothing with render=False) plus the guide buffers by name.  seed, traversal and extra_flags are the handle's defaults
    again afterwards, whatever happened."""
    cam = util.camera(name) if cam is None else cam
    r.set_spp(spp)
    r.seed, r.traversal, r.extra_flags = seed, traversal, flags
    out = {}
    try:
        if render:
            rgb = r.run_view(*cam, width=width, height=height, want_variance=want_variance, want_halves=want_halves, stats=stats)
            out = {"rgb": rgb, "mean": r.mean_buffer.copy(), "variance": r.variance_buffer, "half_a": r.half_a_buffer, "half_b": r.half_b_buffer}
            out = {k: (v.copy() if v is not None else None) for k, v in out.items()}
        if aov is not None:
            out.update(r.run_view_aov(*cam, want=aov, width=width, height=height))
        if shading is not None:
            out.update(r.run_view_aov_shading(*cam, first=shading, width=width, height=height))
    finally:
        r.seed, r.traversal, r.extra_flags = 0, crt.TRAVERSAL_EXACT, 0
    return out


_frames = {}


def cached_frame(renders, name, width, height, spp, seed=0, cam=None, **kw):
    """gpu_frame on renders[name], rendered once per process for each set of arguments: a frame is a function of them, not of the
    handle that drew it."""
    key = (name, width, height, spp, seed, None if cam is None else tuple(np.concatenate([np.ravel(c) for c in cam]).tolist()),
           tuple(sorted(kw.items())))
    if key not in _frames:
        _frames[key] = gpu_frame(renders[name], name, width, height, spp, seed=seed, cam=cam, **kw)
    return _frames[key]
