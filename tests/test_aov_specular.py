"""The AOV pass that follows perfect-mirror bounces (crt_render_aov_specular / _device, include/crt.h; Render.run_view_aov_specular and
run_view_denoised(specular_guides=True) in Python; crt_cli --aov-specular / --denoise-specular).

The expected buffers are the contract of include/crt.h restated in numpy float32: the oracle's primary rays (its ray log, as
tests/test_aov.py takes them: util.primary_rays_of), the bounces through OracleScene.intersect -- which normalises a raw direction as
Ray's constructor does -- and kd, ke, normal and mode from OracleScene.tris().  Every buffer must match bit for bit.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import oracle_lib as O
import util
from frames import renders  # noqa: F401

F = np.float32
NAMES = ("guide_albedo", "last_normal", "path_depth", "bounces", "last_tri")
EXPORTS = ("crt_aov_specular_defaults", "crt_render_aov_specular", "crt_render_aov_specular_device")
SPECULAR = 1  # crt_material.mode / the oracle's mode of a SPECULAR material (the loader: Ns > 1)


# -------------------------------------------------------------------------------------------------------- restatement --

def unit_rows(v):
    """Ray's constructor: v / sqrt(x x + (y y + z z)) per component, v itself if the sum is not positive"""
    z = v[:, 0] * v[:, 0] + (v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    s = np.sqrt(z)
    return np.where((z > 0)[:, None], v / s[:, None], v).astype(F)


def chains(osc, o, d, t, tri, max_bounces):
    """Per sample, the chain of the contract: (hit, D, B, thr, tri_L or -1)."""
    tris = osc.tris()
    n = tri.shape[0]
    hit = tri >= 0
    length = np.zeros(n, dtype=F)
    B = np.zeros(n, dtype=np.int32)
    thr = np.zeros((n, 3), dtype=F)
    last = np.full(n, -1, dtype=np.int32)
    act = np.nonzero(hit)[0]
    co, cd, ct, ctri = o[act].astype(F), d[act].astype(F), t[act].astype(F), tri[act]
    with np.errstate(all="ignore"):
        while act.size:
            length[act] = length[act] + ct
            go = (tris["mode"][ctri] == SPECULAR) & (B[act] < max_bounces)
            last[act[~go]] = ctri[~go]
            g = act[go]
            kd = tris["kd"][ctri[go]].astype(F)
            thr[g] = np.where((B[g] == 0)[:, None], kd, thr[g] * kd)
            nrm = tris["normal"][ctri[go]].astype(F)
            dd, tt = cd[go], ct[go]
            P = co[go] + dd * tt[:, None]
            c = dd[:, 0] * nrm[:, 0] + (dd[:, 1] * nrm[:, 1] + dd[:, 2] * nrm[:, 2])
            c2 = c + c
            r = dd - nrm * c2[:, None]
            assert P.dtype == F and r.dtype == F
            B[g] += 1
            if g.size == 0:
                break
            ntri, nt, _ = osc.intersect(P, r)
            more = ntri >= 0
            act, co, cd, ct, ctri = g[more], P[more], unit_rows(r)[more], nt[more].astype(F), ntri[more]
    return hit, length, B, thr, last


def restated(osc, rays, spp, max_bounces):
    """The five buffers of the contract from the primary rays `rays` of util.primary_rays_of, and the per-sample chains."""
    o, d, t, tri, (ch, cw) = rays
    tris = osc.tris()
    hit, length, B, thr, last = chains(osc, o, d, t, tri, max_bounces)
    p = ch * cw
    li = np.maximum(last, 0)
    kd, ke = tris["kd"][li].astype(F), tris["ke"][li].astype(F)
    with np.errstate(all="ignore"):
        e = np.where(ke < 1, ke, F(1.0)).astype(F)
        G = np.where((B == 0)[:, None], kd, thr * (kd + e)).astype(F)
        N = tris["normal"][li].astype(F)
        has = last >= 0
        sh = lambda a: a.reshape((p, spp) + a.shape[1:])
        G, N, has, hit_, D, Bf = sh(G), sh(N), sh(has), sh(hit), sh(length), sh(B.astype(F))
        a = np.zeros((p, 3), dtype=F)
        nr = np.zeros((p, 3), dtype=F)
        ds = np.zeros(p, dtype=F)
        bs = np.zeros(p, dtype=F)
        hits = np.zeros(p, dtype=np.int64)
        fs = F(spp)
        for k in range(spp):
            a = np.where(has[:, k, None], a + G[:, k] / fs, a)
            nr = np.where(has[:, k, None], nr + N[:, k] / fs, nr)
            ds = np.where(hit_[:, k], ds + D[:, k], ds)
            bs = np.where(hit_[:, k], bs + Bf[:, k], bs)
            hits += hit_[:, k]
        fh = hits.astype(F)
        depth = np.where(hits > 0, ds / fh, F(0.0)).astype(F)
        bounces = np.where(hits > 0, bs / fh, F(0.0)).astype(F)
    assert a.dtype == F and nr.dtype == F
    out = {"guide_albedo": a.reshape(ch, cw, 3), "last_normal": nr.reshape(ch, cw, 3), "path_depth": depth.reshape(ch, cw),
           "bounces": bounces.reshape(ch, cw), "last_tri": sh(last)[:, 0].reshape(ch, cw)}
    return out, {"hit": hit, "B": B, "last": last}


@functools.lru_cache(maxsize=None)
def expected(name, width, height, spp, max_bounces, crop=None, seed=0):
    osc, t = util.oracle_scene(name), util.task(name)
    eye, iv, fov = util.camera(name)
    return restated(osc, util.primary_rays_of(osc, eye, iv, fov, t.light_sample_n, width, height, spp, crop, seed), spp, max_bounces)


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_aov_specular_entry_points_are_exported():
    lib = capi.lib()
    for name in EXPORTS:
        assert name in capi.EXPORTS
        getattr(lib, name)
    assert crt.aov_specular_defaults() == {"max_bounces": 2}
    for name in ("run_view_aov_specular", "run_view_aov_specular_device"):
        assert hasattr(crt.Render, name)
    assert lib.crt_aov_specular_defaults(None) == capi.ERR_INVALID_ARG


def test_aov_specular_arguments_are_checked_before_any_device_call():
    """Every invalid call is CRT_ERR_INVALID_ARG, also on a machine without a GPU.  A non-null scene here is a dummy that must never be
    dereferenced."""
    lib = capi.lib()
    dummy = C.create_string_buffer(256)
    sc = C.cast(dummy, C.c_void_p)
    cam = capi.Camera()
    good = capi.Params(64, 48, 4, 0.6, 1, 0, 0, 1, capi.TRAVERSAL_EXACT, 0)
    buf = np.zeros(64 * 48 * 3, dtype=np.float32)
    bufs = capi.AovSpecularBuffers()
    bufs.guide_albedo = buf.ctypes.data
    none = capi.AovSpecularBuffers()
    sp = capi.AovSpecularParams(2)

    def both(scene, camera, prm, s, b):
        r1 = lib.crt_render_aov_specular(scene, camera, prm, s, b, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_render_aov_specular_device(scene, camera, prm, s, b, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == capi.ERR_INVALID_ARG, (r1, r2, e1, e2)
        return e1

    assert b"null" in both(None, C.byref(cam), C.byref(good), C.byref(sp), C.byref(bufs))
    assert b"null" in both(sc, None, C.byref(good), C.byref(sp), C.byref(bufs))
    assert b"null" in both(sc, C.byref(cam), None, C.byref(sp), C.byref(bufs))
    assert b"null" in both(sc, C.byref(cam), C.byref(good), None, C.byref(bufs))
    assert b"null" in both(sc, C.byref(cam), C.byref(good), C.byref(sp), None)
    assert b"no output" in both(sc, C.byref(cam), C.byref(good), C.byref(sp), C.byref(none))
    for bad in (0, 9, 0xffffffff):
        assert b"max_bounces" in both(sc, C.byref(cam), C.byref(good), C.byref(capi.AovSpecularParams(bad)), C.byref(bufs))
    for field, value in (("spp", 0), ("width", 0), ("height", 0)):
        p = capi.Params(64, 48, 4, 0.6, 1, 0, 0, 1, capi.TRAVERSAL_EXACT, 0)
        setattr(p, field, value)
        both(sc, C.byref(cam), C.byref(p), C.byref(sp), C.byref(bufs))
    both(sc, C.byref(cam), C.byref(capi.Params(64, 48, 4, 0.6, 1, 0, 3, 3, capi.TRAVERSAL_EXACT, capi.FLAG_TILED_OUTPUT)), C.byref(sp), C.byref(bufs))
    both(sc, C.byref(cam), C.byref(capi.Params(64, 48, 4, 0.6, 1, 0, 1, 3, capi.TRAVERSAL_EXACT, 0)), C.byref(sp), C.byref(bufs))
    both(sc, C.byref(cam), C.byref(capi.Params(64, 48, 4, 0.6, 1, 0, 0, 1, 7, 0)), C.byref(sp), C.byref(bufs))


# a scene with mirror-to-mirror chains: two facing mirrors (x = -1 and x = 1, z in [0, 3]) over a diffuse floor, an emitter that closes a
# part of the far end, everything else open; the camera looks into the corridor at a slant
MIRROR_MTL = ("newmtl left\nKd 0.9 0.8 0.7\nNs 100\nnewmtl right\nKd 0.6 0.9 0.8\nNs 50\nnewmtl floor\nKd 0.5 0.6 0.7\nNs 1\n"
              "newmtl light\nKe 20 15 0.5\nKd 0 0 0\nNs 1\n")
MIRROR_QUADS = [("left", [(-1, 0, 0), (-1, 2, 0), (-1, 2, 3), (-1, 0, 3)]),
                ("right", [(1, 0, 0), (1, 0, 3), (1, 2, 3), (1, 2, 0)]),
                ("floor", [(-1, 0, -1), (-1, 0, 3), (1, 0, 3), (1, 0, -1)]),
                ("light", [(-1, 0.5, 3), (-1, 1.5, 3), (1, 1.5, 3), (1, 0.5, 3)])]
MIRROR_EYE, MIRROR_LOOKAT, MIRROR_UP, MIRROR_FOV = (0.9, 1.0, -0.5), (-1.0, 0.9, 0.5), (0.0, 1.0, 0.0), 60.0
MIRROR_W, MIRROR_H, MIRROR_SPP, MIRROR_THRESH = 33, 17, 3, 2


def write_mirror_scene(d):
    """Two triangles (a, b, c), (a, c, e) per quad; the stored normal is cross(e1, e2)."""
    d = str(d)
    with open(os.path.join(d, "mirrors.mtl"), "w") as f:
        f.write(MIRROR_MTL)
    with open(os.path.join(d, "mirrors.obj"), "w") as f:
        f.write("mtllib mirrors.mtl\n")
        i = 0
        for m, corners in MIRROR_QUADS:
            for p in corners:
                f.write("v %.9g %.9g %.9g\nvn 0 1 0\nvt 0 0\n" % tuple(p))
            f.write("usemtl %s\n" % m)
            for a, b, c in ((i + 1, i + 2, i + 3), (i + 1, i + 3, i + 4)):
                f.write("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % (a, a, a, b, b, b, c, c, c))
            i += 4
    return os.path.join(d, "mirrors.obj"), d


def mirror_camera():
    return MIRROR_EYE, crt.get_inverse_view_matrix(MIRROR_EYE, MIRROR_LOOKAT, MIRROR_UP), crt.fov_to_radians(MIRROR_FOV)


def mirror_expected(d):
    obj, mtl = write_mirror_scene(d)
    osc = O.OracleScene([(obj, mtl)], MIRROR_THRESH)
    eye, iv, fov = mirror_camera()
    rays = util.primary_rays_of(osc, eye, iv, fov, 1, MIRROR_W, MIRROR_H, MIRROR_SPP)
    return {mb: restated(osc, rays, MIRROR_SPP, mb) for mb in (1, 2, 8)}


def test_mirror_scene_has_every_kind_of_chain(tmp_path):
    """The restatement on the scene of test_aov_specular_mirror_to_mirror_chains: the cases that test is about are there."""
    want = mirror_expected(tmp_path)
    c1, c2, c8 = want[1][1], want[2][1], want[8][1]
    assert (~c8["hit"]).any() and (c8["hit"] & (c8["B"] == 0)).any()              # camera rays that miss, and that stay on the floor
    assert (c8["B"] == 1).any() and (c8["B"] >= 2).any() and (c8["B"] >= 3).any()
    assert (c8["hit"] & (c8["last"] < 0)).any()                                    # chains that end in a miss
    assert (c8["B"] < 8).all()                                                     # none cut by the cap of 8 ...
    tris = O.OracleScene([write_mirror_scene(tmp_path)], MIRROR_THRESH).tris()
    for c, cap in ((c1, 1), (c2, 2)):                                              # ... some by the caps of 1 and 2: they end ON a mirror
        cut = (c["B"] == cap) & (c["last"] >= 0) & (tris["mode"][np.maximum(c["last"], 0)] == SPECULAR)
        assert cut.any(), cap
    lit = (c8["last"] >= 0) & (c8["B"] >= 1) & (tris["has_emit"][np.maximum(c8["last"], 0)] != 0)
    assert lit.any()                                                               # and some end at the emitter
    assert not np.array_equal(want[1][0]["guide_albedo"], want[2][0]["guide_albedo"])
    assert not np.array_equal(want[2][0]["guide_albedo"], want[8][0]["guide_albedo"])


# ------------------------------------------------------------------------------------------------------------------ GPU --


def run_spec(r, name, spp, width=None, height=None, max_bounces=None, traversal=crt.TRAVERSAL_EXACT, seed=0, want=NAMES):
    eye, iv, fov = util.camera(name)
    r.set_spp(spp)
    r.seed = seed
    r.traversal = traversal
    try:
        return r.run_view_aov_specular(eye, iv, fov, max_bounces=max_bounces, want=want, width=width, height=height)
    finally:
        r.traversal = crt.TRAVERSAL_EXACT
        r.seed = 0


@pytest.mark.gpu
@pytest.mark.parametrize("max_bounces", [1, 2])
def test_aov_specular_veach_matches_restatement(renders, max_bounces):
    r = renders["veach-mis"]
    got = run_spec(r, "veach-mis", 4, 64, 48, max_bounces)
    want, ch = expected("veach-mis", 64, 48, 4, max_bounces)
    util.assert_same(got, want, NAMES, "veach-mis max_bounces %d" % max_bounces)
    assert (got["bounces"] > 0).any() and (got["bounces"] == 0).any()
    tris = util.oracle_scene("veach-mis").tris()
    assert ((ch["B"] >= 1) & (ch["last"] >= 0) & (tris["has_emit"][np.maximum(ch["last"], 0)] != 0)).any()  # a chain ends at an emitter
    info = r.aov_specular_info
    assert info["chunks"] == 1 and info["rays"] == 64 * 48 * 4 + int(ch["B"].sum()), info


@pytest.mark.gpu
def test_aov_specular_changes_nothing_on_cornell_box(renders):
    """No SPECULAR triangle: the first-hit buffers bit for bit, and no ray beyond the camera rays."""
    r = renders["cornell-box"]
    assert not (util.oracle_scene("cornell-box").tris()["mode"] == SPECULAR).any()
    got = run_spec(r, "cornell-box", 4, 64, 48)
    assert r.aov_specular_info["rays"] == 64 * 48 * 4 and r.aov_specular_info["chunks"] == 1
    eye, iv, fov = util.camera("cornell-box")
    aov = r.run_view_aov(eye, iv, fov, width=64, height=48)
    util.assert_same(got, {"guide_albedo": aov["albedo"], "last_normal": aov["normal"], "path_depth": aov["depth"], "last_tri": aov["tri"]},
                     ("guide_albedo", "last_normal", "path_depth", "last_tri"), "cornell-box")
    assert not got["bounces"].any() and (got["last_tri"] >= 0).any()
    util.assert_same(got, expected("cornell-box", 64, 48, 4, 2)[0], NAMES, "cornell-box")


@pytest.mark.gpu
def test_aov_specular_invariant_on_veach_pixels_without_a_specular_hit(renders):
    r = renders["veach-mis"]
    got = run_spec(r, "veach-mis", 4, 64, 48, 2)
    eye, iv, fov = util.camera("veach-mis")
    r.set_spp(4)
    aov = r.run_view_aov(eye, iv, fov, width=64, height=48)
    _, _, _, tri, _ = util.primary_rays_of(util.oracle_scene("veach-mis"), eye, iv, fov, util.task("veach-mis").light_sample_n, 64, 48, 4)
    mode = util.oracle_scene("veach-mis").tris()["mode"]
    plain = ~((tri >= 0) & (mode[np.maximum(tri, 0)] == SPECULAR)).reshape(48, 64, 4).any(axis=2)
    assert plain.any() and (~plain).any()
    for a, b in (("guide_albedo", "albedo"), ("last_normal", "normal"), ("path_depth", "depth"), ("last_tri", "tri")):
        assert np.array_equal(got[a][plain].view(np.uint32), aov[b][plain].view(np.uint32)), a
    assert not got["bounces"][plain].any()


@pytest.mark.gpu
def test_aov_specular_mirror_to_mirror_chains(tmp_path):
    want = mirror_expected(tmp_path)
    obj, mtl = write_mirror_scene(tmp_path)
    scene = crt.Scene(MIRROR_W, MIRROR_H)
    scene.add_obj(obj, mtl)
    scene.set_BVH(MIRROR_THRESH)
    r = crt.Render(scene, MIRROR_SPP, 0.0, 1)
    try:
        eye, iv, fov = mirror_camera()
        for mb in (1, 2, 8):
            got = r.run_view_aov_specular(eye, iv, fov, max_bounces=mb)
            util.assert_same(got, want[mb][0], NAMES, "mirrors max_bounces %d" % mb)
            # the camera rays of every slot, padding included (33 x 17 is ragged), and the reflected rays of the pixels alone
            assert r.aov_specular_info["rays"] == crt.shard_slots(MIRROR_W, MIRROR_H, 0, 1) * MIRROR_SPP + int(want[mb][1]["B"].sum())
    finally:
        r.free()
        scene.free()


PLATE_CROP = (330, 310, 16, 8)  # inside a plate of veach-mis at 800 x 600


@pytest.mark.gpu
def test_aov_specular_crop_of_full_camera_in_chunks(renders):
    """800 x 600 at spp 72: 2^25 / 480 000 = 69 samples per chunk, so two chunks, and the running sums and the chain state cross them."""
    spp = 72
    r = renders["veach-mis"]
    got = run_spec(r, "veach-mis", spp)
    assert r.aov_specular_info["chunks"] == 2 and r.aov_specular_info["rays"] > 800 * 600 * spp, r.aov_specular_info
    x0, y0, cw, ch = PLATE_CROP
    want, chain = expected("veach-mis", 800, 600, spp, 2, crop=PLATE_CROP)
    assert (chain["B"] > 0).mean() > 0.5
    util.assert_same({n: got[n][y0:y0 + ch, x0:x0 + cw] for n in NAMES}, want, NAMES, "chunks")


@pytest.mark.gpu
def test_aov_specular_traversal_modes_agree(renders):
    base = run_spec(renders["veach-mis"], "veach-mis", 4, 64, 48, 2, seed=3)
    assert (base["bounces"] > 0).any()
    for mode in (crt.TRAVERSAL_REFERENCE, crt.TRAVERSAL_FAST):
        util.assert_same(run_spec(renders["veach-mis"], "veach-mis", 4, 64, 48, 2, traversal=mode, seed=3), base, NAMES, "mode %d" % mode)


@pytest.mark.gpu
@pytest.mark.parametrize("var,value", [("CRT_PIPELINE", "2"), ("CRT_DEC", "0"), ("CRT_REF16", "0")])
def test_aov_specular_kernel_variants_agree(renders, var, value, monkeypatch):
    base = {n: run_spec(renders[n], n, 4, 64, 48, 2) for n in renders}
    monkeypatch.setenv(var, value)
    for n in renders:
        util.assert_same(run_spec(renders[n], n, 4, 64, 48, 2), base[n], NAMES, "%s %s=%s" % (n, var, value))


@pytest.mark.gpu
def test_aov_specular_tiled_shards_deinterleave_to_row_major(renders):
    from cudaraytracing_amd.distributed import untile_numpy
    name, w, h, world, spp = "veach-mis", 70, 45, 3, 2
    r = renders[name]
    full = run_spec(r, name, spp, w, h, 2)
    assert (full["bounces"] > 0).any()
    eye, iv, fov = util.camera(name)
    cam = r._cam(eye, iv, fov)
    sp = capi.AovSpecularParams(2)
    shards = {n: [] for n in NAMES}
    for rank in range(world):
        slots = crt.shard_slots(w, h, rank, world)
        bufs, arrs = capi.AovSpecularBuffers(), {}
        for n in NAMES:
            ch, dt = capi.AOV_SPECULAR_BUFFERS[n]
            arrs[n] = np.full((slots, ch), 7, dtype=dt)  # (padding slots must come back as 0 / -1)
            setattr(bufs, n, arrs[n].ctypes.data)
        prm = r._params(rank=rank, world=world, flags=capi.FLAG_TILED_OUTPUT, width=w, height=h)
        info = capi.AovInfo()
        capi.check(capi.lib().crt_render_aov_specular(r._h, C.byref(cam), C.byref(prm), C.byref(sp), C.byref(bufs), C.byref(info)), "crt_render_aov_specular")
        assert info.rays >= slots * spp and info.chunks == 1
        for n in NAMES:
            shards[n].append(arrs[n])
    tx, ty = (w + 7) // 8, (h + 7) // 8
    for n in NAMES:
        g = np.stack(shards[n])
        img = untile_numpy(g, w, h)
        img = img if capi.AOV_SPECULAR_BUFFERS[n][0] == 3 else img[:, :, 0]
        util.assert_same({n: img}, full, (n,), "tiled")
        for rank in range(world):
            for s in range(g.shape[1]):
                tile = (s // 64) * world + rank
                i, j = (tile % tx) * 8 + (s % 64) % 8, (tile // tx) * 8 + (s % 64) // 8
                if tile >= tx * ty or i >= w or j >= h:
                    assert np.all(g[rank, s] == (-1 if n == "last_tri" else 0)), (n, rank, s)


@pytest.mark.gpu
def test_aov_specular_device_form_on_a_stream_between_progressive_ranges(renders):
    """The device form on a stream of its own equals the host form, and a progressive frame in flight is left alone: ranges with the
    call in between give the one-shot frame."""
    name, w, h = "veach-mis", 80, 56
    r = renders[name]
    eye, iv, fov = util.camera(name)
    want = run_spec(r, name, 3, w, h, 2)
    r.set_spp(3)
    one = r.run_view(eye, iv, fov, width=w, height=h).copy()
    one_mean = r.mean_buffer.copy()
    with DeviceBuffers.image({n: capi.AOV_SPECULAR_BUFFERS[n] for n in NAMES}, w, h) as d:
        assert r.run_view_range(eye, iv, fov, 0, 2, width=w, height=h) is None
        assert r.run_view_aov_specular_device(eye, iv, fov, d.ptrs, max_bounces=2, stream=d.stream, want_info=False, width=w, height=h) is None
        d.synchronize()
        util.assert_same(d.fetch(NAMES), want, NAMES, "device form")
        _, _, done = r.preview(width=w, height=h)
        assert done == 2
        rgb = r.run_view_range(eye, iv, fov, 2, 1, width=w, height=h)
        assert np.array_equal(rgb, one)
        assert np.array_equal(r.mean_buffer.view(np.uint32), one_mean.view(np.uint32))
        # a subset of the buffers, with the pass's timer
        d.fill("bounces", 0)
        info = r.run_view_aov_specular_device(eye, iv, fov, {"bounces": d.ptrs["bounces"]}, max_bounces=2, stream=d.stream, width=w, height=h)
        assert info["chunks"] == 1 and info["rays"] > w * h * 3 and info["total_ms"] > 0
        util.assert_same(d.fetch(["bounces"]), want, ("bounces",), "subset")


@pytest.mark.gpu
@pytest.mark.parametrize("variance_guided", [False, True])
def test_run_view_denoised_with_specular_guides_equals_the_calls_by_hand(renders, variance_guided):
    name, w, h = "veach-mis", 96, 72
    r = renders[name]
    eye, iv, fov = util.camera(name)
    r.set_spp(4)
    r.run_view(eye, iv, fov, width=w, height=h, want_variance=variance_guided)
    mean0 = r.mean_buffer.copy()
    var0 = r.variance_buffer.copy() if variance_guided else None
    g = r.run_view_aov(eye, iv, fov, want=("albedo", "normal", "depth"), width=w, height=h)
    first_hit = g["albedo"]
    g["albedo"] = r.run_view_aov_specular(eye, iv, fov, want=("guide_albedo",), width=w, height=h)["guide_albedo"]
    assert not np.array_equal(g["albedo"], first_hit)
    if variance_guided:
        want_rgb, want_mean = crt.denoise_var(mean0, var0, **g)
    else:
        want_rgb, want_mean = crt.denoise(mean0, **g)
    rgb, mean = r.run_view_denoised(eye, iv, fov, width=w, height=h, variance_guided=variance_guided, specular_guides=True)
    util.assert_bits(mean, want_mean, "run_view_denoised(specular_guides=True)")
    assert np.array_equal(rgb, want_rgb)
    assert np.array_equal(r.aov_buffers["albedo"].view(np.uint32), g["albedo"].view(np.uint32))
    # the default is the first-hit albedo, and max_bounces reaches the pass
    r.run_view_denoised(eye, iv, fov, width=w, height=h, variance_guided=variance_guided)
    assert np.array_equal(r.aov_buffers["albedo"].view(np.uint32), first_hit.view(np.uint32))
    r.run_view_denoised(eye, iv, fov, width=w, height=h, variance_guided=variance_guided, specular_guides=True, max_bounces=1)
    one = r.run_view_aov_specular(eye, iv, fov, max_bounces=1, want=("guide_albedo",), width=w, height=h)["guide_albedo"]
    assert np.array_equal(r.aov_buffers["albedo"].view(np.uint32), one.view(np.uint32))


@pytest.mark.gpu
def test_cli_writes_specular_aov_files_and_the_denoised_frame(renders, tmp_path):
    from PIL import Image
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    prefix, den, den0 = str(tmp_path / "veach"), str(tmp_path / "den.png"), str(tmp_path / "den0.png")
    cfg = util.SCENES["veach-mis"]
    base = [cli, cfg, "-o", prefix + ".png", "--spp", "2", "--width", "96", "--height", "72", "--seed", "42", "--base-dir", util.ROOT]
    res = subprocess.run(base + ["--aov-specular", prefix + ",1", "--denoise", den, "--denoise-specular"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    r = renders["veach-mis"]
    got = run_spec(r, "veach-mis", 2, 96, 72, 1, seed=42)
    for n in ("guide_albedo", "last_normal", "path_depth", "bounces"):
        hdr, a = util.read_pfm("%s_%s.pfm" % (prefix, n))
        assert hdr[2] == b"-1.0" and np.array_equal(a.view(np.uint32), got[n].view(np.uint32)), n
    eye, iv, fov = util.camera("veach-mis")
    r.set_spp(2)
    r.seed = 42
    try:
        rgb, _ = r.run_view_denoised(eye, iv, fov, width=96, height=72, specular_guides=True, max_bounces=1)
        rgb0, _ = r.run_view_denoised(eye, iv, fov, width=96, height=72)
    finally:
        r.seed = 0
    assert np.array_equal(np.asarray(Image.open(den)), rgb)
    res = subprocess.run(base + ["--denoise", den0], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert np.array_equal(np.asarray(Image.open(den0)), rgb0) and not np.array_equal(rgb, rgb0)
    bad = subprocess.run([cli, cfg, "--devices", "0,0", "--gather", "copy", "--aov-specular", prefix], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--aov-specular" in bad.stderr
    bad = subprocess.run(base + ["--aov-specular", prefix + ",9"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "MAX_BOUNCES" in bad.stderr
    bad = subprocess.run(base + ["--denoise-specular"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--denoise-specular" in bad.stderr


@pytest.mark.gpu
def test_multi_render_has_no_specular_aov_pass():
    m = crt.MultiRender(util.host_scene("cornell-box"), 2, devices=(0,), gather=crt.GATHER_COPY)
    try:
        eye, iv, fov = util.camera("cornell-box")
        with pytest.raises(NotImplementedError):
            m.run_view_aov_specular(eye, iv, fov)
        with pytest.raises(NotImplementedError):
            m.run_view_aov_specular_device(eye, iv, fov, {})
        with pytest.raises(NotImplementedError):
            m.run_view_denoised(eye, iv, fov, specular_guides=True)
    finally:
        m.free()


@pytest.mark.gpu
def test_specular_albedo_guide_lowers_the_denoised_error_on_veach(renders):
    """veach-mis 64 x 48, N = spp 8 seed 0, R = spp 256 seed 999, crt_denoise with its defaults; mse on the RGB8 tone maps against R.
    The numpy restatements of the final contract (the oracle's frames, tests/test_denoise.py::restated, this file's restated with
    max_bounces 2) gave 365.6 with the first-hit albedo and 250.5 with guide_albedo (noisy frame 479.5); seeds 1 and 2 of N: 328.3 ->
    231.4 and 318.0 -> 211.8."""
    name, w, h = "veach-mis", 64, 48
    r = renders[name]
    eye, iv, fov = util.camera(name)

    def frame(spp, seed):
        r.set_spp(spp)
        r.seed = seed
        try:
            rgb = r.run_view(eye, iv, fov, width=w, height=h).copy()
            return rgb, r.mean_buffer.copy()
        finally:
            r.seed = 0

    ref_rgb, _ = frame(256, 999)
    _, noisy = frame(8, 0)
    r.set_spp(8)
    g = r.run_view_aov(eye, iv, fov, want=("albedo", "normal", "depth"), width=w, height=h)
    guide = r.run_view_aov_specular(eye, iv, fov, want=("guide_albedo",), width=w, height=h)["guide_albedo"]

    def mse(x):
        d = x.astype(np.float64) - ref_rgb.astype(np.float64)
        return float(np.mean(d * d))

    first = mse(crt.denoise(noisy, **g)[0])
    spec = mse(crt.denoise(noisy, albedo=guide, normal=g["normal"], depth=g["depth"])[0])
    msg = "mse against spp 256: first-hit albedo %.1f, guide_albedo %.1f" % (first, spec)
    print(msg)
    assert spec < first, msg
