"""The ambient-occlusion AOV pass (crt_render_aov_ao / crt_render_aov_ao_device, include/crt.h; Render.run_view_aov_ao in Python; crt_cli
--aov-ao): per first hit, ao_samples rays of at most max_distance over the hemisphere of the facing normal.

The expected buffers come from aov_ao_restated: the contract in numpy float32 on the oracle's primary rays, draws, samplers, vector
functions and closest hit.  The CPU tests anchor that restatement -- exactly on scenes whose answer is known, statistically on one with
an analytic answer -- and run the kernel text on the host against a second, plain restatement (tools/aov_ao_host_check.cpp).  On the GPU
every buffer must match bit for bit.
Unless stated a case is cornell-box at 40 x 30, spp 3, ao_samples 2, the scene's default max_distance, seed 7.
"""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import aov_ao_restated as R
import host_program as HP
import oracle_lib as O
import scene_files
import util
from frames import renders  # noqa: F401

F = np.float32
NAMES = R.NAMES
SCENE_NAMES = ("cornell-box", "veach-mis")
W, H, SPP, AOS, SEED = 40, 30, 3, 2, 7


@functools.lru_cache(maxsize=None)
def default_distance(name):
    return float(R.default_max_distance(util.oracle_scene(name)))


@functools.lru_cache(maxsize=None)
def expected(name="cornell-box", w=W, h=H, spp=SPP, ao_samples=AOS, max_distance=None, seed=SEED):
    want = R.expected(name, w, h, spp, ao_samples, default_distance(name) if max_distance is None else max_distance, seed)
    for a in want.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return want


def slots_of(w, h, world=1):
    return ((((w + 7) // 8) * ((h + 7) // 8) + world - 1) // world) * 64


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_ao_entry_points_are_exported():
    lib = capi.lib()
    for name in ("crt_aov_ao_defaults", "crt_render_aov_ao", "crt_render_aov_ao_device"):
        assert name in capi.EXPORTS
        getattr(lib, name)
    assert tuple(capi.AOV_AO_BUFFERS) == NAMES
    assert [f for f, _ in capi.AovAoBuffers._fields_] == list(NAMES)
    assert [f for f, _ in capi.AovAoParams._fields_] == ["ao_samples", "max_distance"]
    for method in ("run_view_aov_ao", "run_view_aov_ao_device", "aov_ao_defaults"):
        assert hasattr(crt.Render, method)
        with pytest.raises(NotImplementedError):
            getattr(crt.MultiRender, method)(None)


def test_ao_arguments_are_checked_before_any_device_call():
    """No buffer named, null arguments, ao_samples and max_distance out of range and what crt_render_aov refuses: CRT_ERR_INVALID_ARG from
    both forms, also on a machine without a GPU.  A non-null scene here is a dummy that must never be dereferenced."""
    lib = capi.lib()
    dummy = C.create_string_buffer(1024)
    sc = C.cast(dummy, C.c_void_p)
    cam = capi.Camera()
    buf = np.zeros(64 * 48 * 3, dtype=np.float32)
    out, none = capi.AovAoBuffers(), capi.AovAoBuffers()
    out.bent_normal = buf.ctypes.data
    ao = capi.AovAoParams(4, 1.5)

    def params(**kw):
        p = capi.Params(64, 48, 4, 0.6, 1, 0, 0, 1, capi.TRAVERSAL_EXACT, 0)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def both(scene, camera, prm, a, o):
        r1 = lib.crt_render_aov_ao(scene, camera, prm, a, o, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_render_aov_ao_device(scene, camera, prm, a, o, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == capi.ERR_INVALID_ARG, (r1, r2, e1, e2)
        return e1

    good = params()
    assert b"null" in both(None, C.byref(cam), C.byref(good), C.byref(ao), C.byref(out))
    assert b"null" in both(sc, None, C.byref(good), C.byref(ao), C.byref(out))
    assert b"null" in both(sc, C.byref(cam), None, C.byref(ao), C.byref(out))
    assert b"null" in both(sc, C.byref(cam), C.byref(good), None, C.byref(out))
    assert b"null" in both(sc, C.byref(cam), C.byref(good), C.byref(ao), None)
    assert b"no output" in both(sc, C.byref(cam), C.byref(good), C.byref(ao), C.byref(none))
    for n in (0, 257):
        assert b"ao_samples" in both(sc, C.byref(cam), C.byref(good), C.byref(capi.AovAoParams(n, 1.5)), C.byref(out))
    for dist in (0.0, -1.0, float("inf"), float("nan")):
        assert b"max_distance" in both(sc, C.byref(cam), C.byref(good), C.byref(capi.AovAoParams(4, dist)), C.byref(out))
    for field in ("spp", "width", "height"):
        both(sc, C.byref(cam), C.byref(params(**{field: 0})), C.byref(ao), C.byref(out))
    both(sc, C.byref(cam), C.byref(params(rank=3, world=3, flags=capi.FLAG_TILED_OUTPUT)), C.byref(ao), C.byref(out))
    both(sc, C.byref(cam), C.byref(params(rank=1, world=3)), C.byref(ao), C.byref(out))
    both(sc, C.byref(cam), C.byref(params(traversal=7)), C.byref(ao), C.byref(out))
    # light_sample_n and p_rr are not read
    assert lib.crt_render_aov_ao(None, C.byref(cam), C.byref(params(light_sample_n=-1)), C.byref(ao), C.byref(out), None) == capi.ERR_INVALID_ARG
    assert b"null" in lib.crt_last_error()
    assert lib.crt_aov_ao_defaults(None, C.byref(ao)) == capi.ERR_INVALID_ARG and lib.crt_aov_ao_defaults(sc, None) == capi.ERR_INVALID_ARG


def _write_scene(d, quads, name="anchor"):
    """quads: (four corners, material) -- `grey` or `light`; the file pair for OracleScene / crt.Scene.add_obj"""
    with open(os.path.join(d, name + ".mtl"), "w") as m:
        m.write("newmtl grey\nKd 0.6 0.6 0.6\nNs 1\nnewmtl light\nKe 20 20 20\nKd 0 0 0\nNs 1\n")
    with open(os.path.join(d, name + ".obj"), "w") as o:
        o.write("mtllib %s.mtl\n" % name)
        nv = 0
        for corners, mtl in quads:
            o.write("usemtl %s\n" % mtl)
            for p in corners:
                o.write("v %.9g %.9g %.9g\nvn 0 1 0\nvt 0 0\n" % tuple(p))
            for a, b, c in ((1, 2, 3), (1, 3, 4)):
                o.write("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % ((nv + a,) * 3 + (nv + b,) * 3 + (nv + c,) * 3))
            nv += 4
    return os.path.join(d, name + ".obj"), d


def _view(eye, lookat, up, fov_degrees):
    return eye, crt.get_inverse_view_matrix(eye, lookat, up), crt.fov_to_radians(fov_degrees)


# a light that no camera ray sees and no occlusion ray reaches: below every surface of the anchor scenes, facing down
_HIDDEN_LIGHT = ([(-1, -5, -1), (1, -5, -1), (1, -5, 1), (-1, -5, 1)], "light")


def test_restatement_on_an_open_plane_is_fully_open(tmp_path):
    """A single large quad seen from above: no ray of the upper hemisphere can hit anything, so ao == 1.0f, openness == 1.0f and
    bent_normal == the normalized sum of all directions at every pixel, all of which hit.
    The eye is 2^-10 above the quad: pos = o + t * d is rounded, so a vertex may lie below the quad by up to an ulp of the eye's height, and
    a ray from there meets the quad again at t = |pos.y| / dir.y -- a hit that blocked() counts once t exceeds EPSILON, as in the
    reference's own shadow rays.  At this height that needs dir.y < 2^-34 / 1e-5 = 6e-6; the test states that no ray is that flat."""
    obj, mtl = _write_scene(str(tmp_path), [([(-50, 0, -50), (-50, 0, 50), (50, 0, 50), (50, 0, -50)], "grey"), _HIDDEN_LIGHT])
    osc = O.OracleScene([(obj, mtl)], 2)
    s = 2.0 ** -10
    eye, iv, fov = _view((10.0 + 0.5 * s, s, -3.0 - 0.25 * s), (10.0, 0.0, -3.0), (0.0, 0.0, 1.0), 40.0)   # (away from the quad's diagonal)
    w, h, spp, n_q = 12, 9, 2, 3
    S = R.samples(osc, eye, iv, fov, w, h, spp, n_q, 25.0, seed=3)
    got = R.fold(S, w, h, spp)
    assert S["vertex"].all()
    assert (S["w"] * R.EPSILON > np.abs(S["pos"][:, 1])[:, None]).all()      # no ray is flat enough to meet the quad again beyond EPSILON
    assert not S["blocked"].any()
    assert (got["ao"] == 1).all() and (got["openness"] == 1).all() and got["rays"] == w * h * spp * n_q
    total = np.zeros((w * h, 3), dtype=F)
    dirs = S["dir"].reshape(w * h, spp * n_q, 3)
    for i in range(spp * n_q):
        total = total + dirs[:, i]
    util.assert_bits(got["bent_normal"].reshape(-1, 3), O.fn("normalized", total).view(F), "bent normal of an open plane")
    assert (got["bent_normal"][:, :, 1] > 0).all()                      # it points up
    assert (S["dir"][:, :, 1] >= 0).all() and (S["w"] == S["dir"][:, :, 1]).all()   # nf = (0, 1, 0): the cosine is the y component
    assert np.abs(np.linalg.norm(S["dir"].astype(np.float64), axis=2) - 1).max() < 1e-6


def test_restatement_inside_a_closed_box_is_fully_closed(tmp_path):
    """A closed room seen from inside with max_distance beyond its diagonal: every ray is blocked, so ao == 0, openness == 0 and
    bent_normal == +0 exactly, at every pixel."""
    obj, mtl = scene_files._write_box_scene(str(tmp_path), n_side=3)
    osc = O.OracleScene([(obj, mtl)], 4)
    eye, iv, fov = _view((5.0, 5.0, 1.0), (5.2, 4.6, 9.0), (0.0, 1.0, 0.0), 50.0)
    w, h, spp, n_q = 12, 9, 2, 3
    S = R.samples(osc, eye, iv, fov, w, h, spp, n_q, 40.0, seed=3)
    got = R.fold(S, w, h, spp)
    assert S["vertex"].all() and S["blocked"].all()
    assert (util.bits(got["ao"]) == 0).all() and (util.bits(got["openness"]) == 0).all() and (util.bits(got["bent_normal"]) == 0).all()
    assert (got["A"] > 0).all() and (util.bits(got["V"]) == 0).all()
    # the same rays with a limit that reaches nothing (a hit counts from t > EPSILON on, and limit - t > EPSILON blocks): all open
    near = R.fold(R.samples(osc, eye, iv, fov, w, h, spp, n_q, 1e-5, seed=3), w, h, spp)
    assert (near["ao"] == 1).all() and (near["openness"] == 1).all()


def test_restatement_beside_a_wall_has_the_analytic_open_fraction(tmp_path):
    """A floor and, at a right angle, a wall of height h = 1 that is 2000 long, max_distance 100: at a floor point at distance x from the
    wall the cosine-weighted open fraction is (1 + x / sqrt(x^2 + h^2)) / 2 (the form factor of an infinite perpendicular strip).  One
    pixel, spp 16 x ao_samples 256 = 4096 rays; the tolerance 5 x 0.5 / sqrt(4096) = 0.04 is five standard deviations of a binomial
    fraction at its widest, derived and not measured (the pixel's footprint, 0.02 wide, moves the answer by less than 0.005)."""
    L, hgt = 1000.0, 1.0
    quads = [([(-L, 0, -L), (-L, 0, L), (L, 0, L), (L, 0, -L)], "grey"),
             ([(0, 0, -L), (0, 0, L), (0, hgt, L), (0, hgt, -L)], "grey"), _HIDDEN_LIGHT]
    obj, mtl = _write_scene(str(tmp_path), quads)
    osc = O.OracleScene([(obj, mtl)], 2)
    for x in (0.5, 1.5):
        eye, iv, fov = _view((x, 5.0, 0.3), (x, 0.0, 0.3), (0.0, 0.0, 1.0), 0.25)
        spp, n_q = 16, 256
        S = R.samples(osc, eye, iv, fov, 1, 1, spp, n_q, 100.0, seed=11)
        got = R.fold(S, 1, 1, spp)
        assert got["rays"] == spp * n_q == 4096 and np.abs(S["pos"][:, 0] - x).max() < 0.02 and np.abs(S["pos"][:, 1]).max() < 1e-5
        want = (1.0 + x / math.sqrt(x * x + hgt * hgt)) / 2.0
        print("x = %.1f: ao %.4f, analytic %.4f, openness %.4f" % (x, got["ao"][0, 0], want, got["openness"][0, 0]))
        assert abs(float(got["ao"][0, 0]) - want) <= 5 * 0.5 / math.sqrt(4096)
        assert got["bent_normal"][0, 0, 0] > 0 and got["bent_normal"][0, 0, 1] > 0   # it leans away from the wall


def test_kernel_text_on_the_host_matches_its_plain_restatement(tmp_path):
    """tools/aov_ao_host_check.cpp under AddressSanitizer and UBSan, a stand-alone program: set-up and resolve of crt_aov_ao.h against the
    restatement inside the program on buffers of exactly their size -- NaN and infinite normals and positions, open == 0, A == 0,
    sub-batch borders inside a sample, tiled shards with padding slots, null outputs."""
    exe = HP.build("aov_ao_host_check.cpp", str(tmp_path / "aov_ao_host_check"), HP.SANITISED)
    rc, out, err = HP.run(exe)
    assert rc == 0, out[-2000:] + err
    assert out.splitlines()[-1] == "12 cases, 0 failures", out[-2000:]


# ------------------------------------------------------------------------------------------------------------------ GPU --

def run_ao(r, name, spp=SPP, w=W, h=H, ao_samples=AOS, max_distance=None, seed=SEED, traversal=crt.TRAVERSAL_EXACT, **kw):
    eye, iv, fov = util.camera(name)
    old = r.spp
    r.set_spp(spp)
    r.seed, r.traversal = seed, traversal
    try:
        return r.run_view_aov_ao(eye, iv, fov, ao_samples=ao_samples, max_distance=max_distance, width=w, height=h, **kw)
    finally:
        r.seed, r.traversal = 0, crt.TRAVERSAL_EXACT
        r.set_spp(old)


def check_bits(r, name, traversal=crt.TRAVERSAL_EXACT, **case):
    want = expected(name, **case)
    got = run_ao(r, name, traversal=traversal, **case)
    util.assert_same(got, want, NAMES, name)
    w, h, spp = case.get("w", W), case.get("h", H), case.get("spp", SPP)
    assert r.aov_ao_info["rays"] == slots_of(w, h) * spp + want["rays"], (r.aov_ao_info, want["rays"])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_ao_defaults_are_four_rays_and_a_quarter_of_the_root_box(renders, name):
    d = renders[name].aov_ao_defaults()
    assert d["ao_samples"] == 4
    assert F(d["max_distance"]) == R.default_max_distance(util.oracle_scene(name)) and 0 < d["max_distance"] < float("inf")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENE_NAMES)
@pytest.mark.parametrize("size", [(40, 30), (61, 47)], ids=["40x30", "61x47"])
def test_ao_bits_match_the_restatement(renders, name, size):
    got = check_bits(renders[name], name, w=size[0], h=size[1])
    assert renders[name].aov_ao_info["chunks"] == 1
    want = expected(name, w=size[0], h=size[1])
    assert (want["open_per_pixel"] > 0).any() and (want["open_per_pixel"] < want["rays_per_pixel"]).any()   # both answers occur
    assert (got["ao"] >= 0).all() and (got["ao"] <= 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ao_samples", [1, 5])
def test_ao_bits_with_other_ray_counts(renders, ao_samples):
    check_bits(renders["cornell-box"], "cornell-box", ao_samples=ao_samples)


@pytest.mark.gpu
def test_ao_with_a_tiny_and_a_large_max_distance(renders):
    """A limit that reaches nothing: ao and openness are exactly 1.0f wherever the camera ray hits; one beyond the scene's size: the
    restatement's bits, with more blocked rays than at the default."""
    name = "cornell-box"
    tiny = check_bits(renders[name], name, max_distance=1e-5)   # (a hit counts from t > 1e-5 on, and limit - t > 1e-5 blocks)
    assert (tiny["ao"] == 1).all() and (tiny["openness"] == 1).all()
    assert expected(name, max_distance=1e-5)["open_per_pixel"].sum() == expected(name, max_distance=1e-5)["rays"] > 0
    check_bits(renders[name], name, max_distance=1e4)
    assert expected(name, max_distance=1e4)["open_per_pixel"].sum() < expected(name)["open_per_pixel"].sum()


@pytest.mark.gpu
@pytest.mark.parametrize("traversal", [crt.TRAVERSAL_REFERENCE, crt.TRAVERSAL_FAST], ids=["reference", "fast"])
def test_ao_bits_with_the_other_traversals(renders, traversal):
    check_bits(renders["veach-mis"], "veach-mis", traversal=traversal)


@pytest.mark.gpu
def test_ao_on_the_fallback_pipeline(renders, monkeypatch):
    monkeypatch.setenv("CRT_PIPELINE", "2")
    check_bits(renders["cornell-box"], "cornell-box")


@pytest.mark.gpu
@pytest.mark.parametrize("entries", [3, 1])
def test_ao_sub_batch_borders_change_no_bit(renders, monkeypatch, entries):
    """CRT_AOV_AO_BATCH = 3 x nslots and 1 x nslots with ao_samples 5: sub-batches that begin and end inside a sample"""
    name = "cornell-box"
    whole = run_ao(renders[name], name, ao_samples=5)
    assert renders[name].aov_ao_info["chunks"] == 1
    rays = renders[name].aov_ao_info["rays"]
    monkeypatch.setenv("CRT_AOV_AO_BATCH", str(entries * slots_of(W, H)))
    got = run_ao(renders[name], name, ao_samples=5)
    info = renders[name].aov_ao_info
    assert info["chunks"] == -(-SPP * 5 // entries) > 1 and info["rays"] == rays, info
    util.assert_same(got, whole, NAMES, "sub-batches of %d" % entries)
    util.assert_same(got, expected(name, ao_samples=5), NAMES, name)


@pytest.mark.gpu
def test_ao_tiled_shard_of_rank_1_of_world_3(renders):
    """The tiled shard of rank 1 of world 3: its pixels carry the full frame's bits; padding slots get ao 1.0f, openness 1.0f, bent_normal +0"""
    name, world, rank = "cornell-box", 3, 1
    r = renders[name]
    want = expected(name)
    eye, iv, fov = util.camera(name)
    old = r.spp
    r.set_spp(SPP)
    r.seed = SEED
    tx, ty = (W + 7) // 8, (H + 7) // 8
    try:
        slots = crt.shard_slots(W, H, rank, world)
        assert slots == slots_of(W, H, world)
        bufs, arrs = capi.AovAoBuffers(), {}
        for n in NAMES:
            arrs[n] = np.full((slots, capi.AOV_AO_BUFFERS[n][0]), 7, dtype=F)
            setattr(bufs, n, arrs[n].ctypes.data)
        cam = r._cam(eye, iv, fov)
        prm = r._params(rank=rank, world=world, flags=capi.FLAG_TILED_OUTPUT, width=W, height=H)
        ao = capi.AovAoParams(AOS, default_distance(name))
        info = capi.AovInfo()
        capi.check(capi.lib().crt_render_aov_ao(r._h, C.byref(cam), C.byref(prm), C.byref(ao), C.byref(bufs), C.byref(info)), "crt_render_aov_ao")
    finally:
        r.seed = 0
        r.set_spp(old)
    pixels = padding = rays = 0
    for s in range(slots):
        tile = (s // 64) * world + rank
        i, j = (tile % tx) * 8 + (s % 64) % 8, (tile // tx) * 8 + (s % 64) // 8
        if tile < tx * ty and i < W and j < H:
            pixels += 1
            rays += int(want["rays_per_pixel"][j, i])
            for n in NAMES:
                assert (util.bits(arrs[n][s]) == util.bits(want[n][j, i]).reshape(-1)).all(), (n, s)
        else:
            padding += 1
            assert arrs["ao"][s, 0] == 1 and arrs["openness"][s, 0] == 1 and (util.bits(arrs["bent_normal"][s]) == 0).all(), s
    assert pixels > 0 and padding > 0 and info.rays == slots * SPP + rays


@pytest.mark.gpu
def test_ao_device_form_on_a_stream_and_null_outputs(renders):
    """The device form on a stream of its own gives the host form's bits; with any output left out the others keep theirs and the buffer
    that is not named is not written."""
    name = "veach-mis"
    r = renders[name]
    want = run_ao(r, name)
    util.assert_same(want, expected(name), NAMES, name)
    eye, iv, fov = util.camera(name)
    old = r.spp
    r.set_spp(SPP)
    r.seed = SEED
    try:
        with DeviceBuffers.image(dict(capi.AOV_AO_BUFFERS), W, H) as d:
            assert d.stream
            assert r.run_view_aov_ao_device(eye, iv, fov, dict(d.ptrs), ao_samples=AOS, stream=d.stream, want_info=False, width=W, height=H) is None
            d.synchronize()
            util.assert_same(d.fetch(want), want, NAMES, "device form")
            for left_out in NAMES:
                for n in NAMES:
                    d.fill(n, 0x5a)
                marked = d.fetch([left_out])[left_out].copy()
                ptrs = {n: d.ptrs[n] for n in NAMES if n != left_out}
                info = r.run_view_aov_ao_device(eye, iv, fov, ptrs, ao_samples=AOS, stream=d.stream, width=W, height=H)
                assert info["chunks"] == 1 and info["rays"] == slots_of(W, H) * SPP + expected(name)["rays"] and info["total_ms"] > 0
                util.assert_same(d.fetch(list(ptrs)), want, tuple(ptrs), "without " + left_out)
                util.assert_same(d.fetch([left_out]), {left_out: marked}, (left_out,), left_out + " is not written")
            with pytest.raises(ValueError):
                r.run_view_aov_ao_device(eye, iv, fov, {"albedo": d.ptrs["ao"]}, width=W, height=H)
    finally:
        r.seed = 0
        r.set_spp(old)
    for left_out in NAMES:   # the host form
        names = tuple(n for n in NAMES if n != left_out)
        util.assert_same(run_ao(r, name, want=names), want, names, "host form without " + left_out)


@pytest.mark.gpu
def test_ao_refusals_leave_the_frame_in_flight_and_the_pass_leaves_the_final_frame(renders):
    """Between two progressive ranges: a refused call changes nothing -- a preview after it has the bits of the one before --, the pass
    itself leaves the accumulator alone, and the frame the ranges complete is the one-shot frame."""
    name = "cornell-box"
    r = renders[name]
    eye, iv, fov = util.camera(name)
    old = r.spp
    r.set_spp(4)
    r.seed = SEED
    try:
        r.run_view_range(eye, iv, fov, 0, 2, width=W, height=H)
        rgb0, mean0, done0 = r.preview(want_mean=True, width=W, height=H)
        for kw in (dict(want=()), dict(ao_samples=0), dict(ao_samples=257), dict(max_distance=0.0), dict(max_distance=-1.0),
                   dict(max_distance=float("inf")), dict(max_distance=float("nan"))):
            with pytest.raises(crt.CrtError) as e:
                r.run_view_aov_ao(eye, iv, fov, width=W, height=H, **{"ao_samples": AOS, **kw})
            assert e.value.status == capi.ERR_INVALID_ARG, kw
            rgb1, mean1, done1 = r.preview(want_mean=True, width=W, height=H)
            assert done1 == done0 == 2 and np.array_equal(rgb0, rgb1), kw
            util.assert_bits(mean1, mean0, "preview after a refusal")
        got = r.run_view_aov_ao(eye, iv, fov, ao_samples=AOS, width=W, height=H)
        rgb1, mean1, done1 = r.preview(want_mean=True, width=W, height=H)
        assert done1 == 2 and np.array_equal(rgb0, rgb1)
        util.assert_bits(mean1, mean0, "preview after the pass")
        r.run_view_range(eye, iv, fov, 2, 2, width=W, height=H)
        ranged = r.mean_buffer.copy()
        r.run_view(eye, iv, fov, width=W, height=H)
        util.assert_bits(ranged, r.mean_buffer, "ranges with the pass in between against the one-shot frame")
    finally:
        r.seed = 0
        r.set_spp(old)
    util.assert_same(got, expected(name, spp=4), NAMES, name)


@pytest.mark.gpu
def test_cli_writes_the_ao_files(renders, tmp_path):
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    name = "veach-mis"
    prefix = str(tmp_path / "veach")
    res = subprocess.run([cli, util.SCENES[name], "-o", prefix + ".png", "--spp", "2", "--width", "48", "--height", "36", "--seed", "42", "--base-dir", util.ROOT,
                          "--aov-ao", prefix + ",3,2.5"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    got = run_ao(renders[name], name, spp=2, w=48, h=36, ao_samples=3, max_distance=2.5, seed=42)
    assert (got["ao"] < 1).any() and (got["bent_normal"] != 0).any()
    for n, suffix in zip(NAMES, ("ao", "openness", "bent")):
        hdr, a = util.read_pfm("%s_%s.pfm" % (prefix, suffix))
        assert hdr[0] == (b"PF" if n == "bent_normal" else b"Pf") and hdr[2] == b"-1.0"
        assert (util.bits(a) == util.bits(got[n])).all(), n
    plain = subprocess.run([cli, util.SCENES[name], "-o", prefix + ".png", "--spp", "1", "--width", "16", "--height", "16", "--seed", "5", "--base-dir", util.ROOT,
                            "--aov-ao", prefix + "_d"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    dflt = run_ao(renders[name], name, spp=1, w=16, h=16, ao_samples=None, seed=5)
    assert (util.bits(util.read_pfm(prefix + "_d_ao.pfm")[1]) == util.bits(dflt["ao"])).all()
    for bad_arg in (prefix + ",0", prefix + ",4,0", ",4"):
        bad = subprocess.run([cli, util.SCENES[name], "--aov-ao", bad_arg], capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "--aov-ao" in bad.stderr, bad_arg
    bad = subprocess.run([cli, util.SCENES[name], "--devices", "0,0", "--gather", "copy", "--aov-ao", prefix], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--aov-ao" in bad.stderr
