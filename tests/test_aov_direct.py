"""The direct-light AOV pass (crt_render_aov_direct / crt_render_aov_direct_device, include/crt.h; Render.run_view_aov_direct in Python;
crt_cli --aov-direct; run_view_denoised(split_direct=True)): the first-vertex next-event term of the frame's own paths.

The expected buffers come from aov_direct_restated: the contract in numpy float32 on the oracle's primary rays, draws, light triangles,
vector functions and closest hit.  The CPU tests pin that restatement to the oracle itself -- at p_rr = 0 the oracle ends every path at
its first vertex, so its per-path radiance is that vertex's L_dir -- and run the kernel text on the host against a second, plain
restatement (tools/aov_direct_host_check.cpp).  On the GPU every buffer must match bit for bit.
Unless stated a case is 40 x 30, spp 4, light_sample_n 2, seed 7.
"""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import aov_direct_restated as R
import aov_expected as aov
import host_program as HP
import util
from frames import renders  # noqa: F401

F = np.float32
NAMES = R.NAMES
SCENE_NAMES = ("cornell-box", "veach-mis")
W, H, SPP, LSN, SEED = 40, 30, 4, 2, 7


@functools.lru_cache(maxsize=None)
def samples_of(name, w=W, h=H, spp=SPP, lsn=LSN, seed=SEED):
    return R.samples(name, w, h, spp, lsn, seed)


@functools.lru_cache(maxsize=None)
def expected(name, w=W, h=H, spp=SPP, lsn=LSN, seed=SEED):
    want = R.fold(samples_of(name, w, h, spp, lsn, seed), w, h, spp)
    for a in want.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return want


def slots_of(w, h, world=1):
    return ((((w + 7) // 8) * ((h + 7) // 8) + world - 1) // world) * 64


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_direct_entry_points_are_exported():
    lib = capi.lib()
    for name in ("crt_render_aov_direct", "crt_render_aov_direct_device"):
        assert name in capi.EXPORTS
        getattr(lib, name)
    assert tuple(capi.AOV_DIRECT_BUFFERS) == NAMES
    assert [f for f, _ in capi.AovDirectBuffers._fields_] == list(NAMES)
    assert hasattr(crt.Render, "run_view_aov_direct") and hasattr(crt.Render, "run_view_aov_direct_device")
    for method in ("run_view_aov_direct", "run_view_aov_direct_device"):
        with pytest.raises(NotImplementedError):
            getattr(crt.MultiRender, method)(None)


def test_direct_arguments_are_checked_before_any_device_call():
    """No buffer named, null arguments, light_sample_n out of range and what crt_render_aov refuses: CRT_ERR_INVALID_ARG from both forms,
    also on a machine without a GPU.  A non-null scene here is a dummy that must never be dereferenced."""
    lib = capi.lib()
    dummy = C.create_string_buffer(256)
    sc = C.cast(dummy, C.c_void_p)
    cam = capi.Camera()
    buf = np.zeros(64 * 48 * 3, dtype=np.float32)
    out, none = capi.AovDirectBuffers(), capi.AovDirectBuffers()
    out.direct = buf.ctypes.data

    def params(**kw):
        p = capi.Params(64, 48, 4, 0.6, 1, 0, 0, 1, capi.TRAVERSAL_EXACT, 0)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def both(scene, camera, prm, o):
        r1 = lib.crt_render_aov_direct(scene, camera, prm, o, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_render_aov_direct_device(scene, camera, prm, o, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == capi.ERR_INVALID_ARG, (r1, r2, e1, e2)
        return e1

    good = params()
    assert b"null" in both(None, C.byref(cam), C.byref(good), C.byref(out))
    assert b"null" in both(sc, None, C.byref(good), C.byref(out))
    assert b"null" in both(sc, C.byref(cam), None, C.byref(out))
    assert b"null" in both(sc, C.byref(cam), C.byref(good), None)
    assert b"no output" in both(sc, C.byref(cam), C.byref(good), C.byref(none))
    for lsn in (-1, 4097):
        assert b"light_sample_n" in both(sc, C.byref(cam), C.byref(params(light_sample_n=lsn)), C.byref(out))
    for field in ("spp", "width", "height"):
        both(sc, C.byref(cam), C.byref(params(**{field: 0})), C.byref(out))
    both(sc, C.byref(cam), C.byref(params(rank=3, world=3, flags=capi.FLAG_TILED_OUTPUT)), C.byref(out))
    both(sc, C.byref(cam), C.byref(params(rank=1, world=3)), C.byref(out))
    both(sc, C.byref(cam), C.byref(params(traversal=7)), C.byref(out))


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_restatement_is_the_oracles_first_vertex_direct_light(name):
    """At p_rr = 0 the oracle's per-path radiance is the first vertex's L_dir: the restated Ld_k has its bits on every path whose camera
    ray does not hit an emitter, the restated limits and blocked flags are those of the oracle's ray log (limit - t > EPSILON), and the
    counts are the ones the frame's description states."""
    S = samples_of(name)
    Ld, _ = R.sample_sums(S)
    tris = S["tris"]
    emitter = (S["tri"] >= 0) & (tris["has_emit"][np.maximum(S["tri"], 0)] != 0)
    assert emitter.any() and S["vertex"].any()
    util.assert_bits(Ld[~emitter], S["L"][~emitter], "%s: Ld_k against the oracle's L" % name)
    util.assert_bits(S["L"][emitter], tris["ke"][S["tri"][emitter]], "%s: the paths left out carry ke" % name)
    shadow = S["log"][~S["prim"]]
    n_shadow = {"cornell-box": 6672, "veach-mis": 37872}[name]
    assert shadow.shape[0] == n_shadow == int(S["vertex"].sum()) * S["n_q"]
    with np.errstate(all="ignore"):
        log_blocked = (shadow[:, 8] - shadow[:, 6]) > R.EPSILON
    assert np.array_equal(log_blocked, S["blocked"][S["vertex"]].reshape(-1))
    util.assert_bits(S["tl"][S["vertex"]].reshape(-1), shadow[:, 8], "%s: limits" % name)
    util.assert_bits(S["pos"][S["vertex"]].repeat(S["n_q"], axis=0), shadow[:, 0:3], "%s: vertices" % name)
    print("%s: %d shadow rays, %.1f %% blocked, %.1f %% of the traced ones" % (name, n_shadow, 100 * log_blocked.mean(),
                                                                                100 * S["blocked"][S["traced"]].mean()))
    assert 0.2 < log_blocked.mean() < 0.8   # (both answers are well represented)
    emitter_pixels = int(emitter.reshape(W * H, SPP).any(axis=1).sum())
    assert emitter_pixels == {"cornell-box": 10, "veach-mis": 25}[name]
    # the fold: a pixel without emitter samples has the oracle's mean in `direct`; every kind of sample is there
    want = expected(name)
    quiet = ~emitter.reshape(H, W, SPP).any(axis=2)
    util.assert_bits(want["direct"][quiet], S["mean"][quiet], "%s: direct against the oracle's mean" % name)
    assert 0 < want["traced"] < n_shadow and (~S["traced"][S["vertex"]]).any()
    assert (want["visibility"] == 1).any() and (want["visibility"] < 1).any() and (want["visibility"] >= 0).all()
    assert (util.bits(want["unshadowed"]) != util.bits(want["direct"])).any()
    assert np.isfinite(want["direct_variance"]).all() and (want["direct_variance"] > 0).any()


def test_kernel_text_on_the_host_matches_its_plain_restatement(tmp_path):
    """tools/aov_direct_host_check.cpp, plain and sanitised (a wave is 64 host threads: CRT_HOST_WAVES): the kernels of crt_aov_direct.h
    against the restatement inside the program -- outputs and traced count equal in every case --, and both builds write the same bytes."""
    res = []
    for form, mode in (("plain", HP.PLAIN), ("sanitised", HP.SANITISED)):
        exe = HP.build("aov_direct_host_check.cpp", str(tmp_path / ("aov_direct_host_check_" + form)), mode, ["-pthread"])
        outp = str(tmp_path / (form + ".bin"))
        rc, out, err = HP.run(exe, ["job", outp])
        assert rc == 0, out[-2000:] + err
        assert out.splitlines()[-1] == "11 cases, 0 failures", out[-2000:]
        res.append(open(outp, "rb").read())
    assert len(res[0]) > 1000 and res[0] == res[1]


# ------------------------------------------------------------------------------------------------------------------ GPU --

def run_direct(r, name, spp=SPP, w=W, h=H, lsn=LSN, seed=SEED, traversal=crt.TRAVERSAL_EXACT, p_rr=None, **kw):
    eye, iv, fov = util.camera(name)
    old = (r.spp, r.light_sample_n, r.P_RR)
    r.set_spp(spp)
    r.set_light_sample_n(lsn)
    if p_rr is not None:
        r.set_P_RR(p_rr)
    r.seed, r.traversal = seed, traversal
    try:
        return r.run_view_aov_direct(eye, iv, fov, width=w, height=h, **kw)
    finally:
        r.seed, r.traversal = 0, crt.TRAVERSAL_EXACT
        r.set_spp(old[0]); r.set_light_sample_n(old[1]); r.set_P_RR(old[2])


def check_bits(r, name, traversal=crt.TRAVERSAL_EXACT, **case):
    want = expected(name, **case)
    got = run_direct(r, name, traversal=traversal, **case)
    util.assert_same(got, want, NAMES, name)
    w, h, spp = case.get("w", W), case.get("h", H), case.get("spp", SPP)
    assert r.aov_direct_info["rays"] == slots_of(w, h) * spp + want["traced"], (r.aov_direct_info, want["traced"])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_direct_bits_match_the_restatement(renders, name):
    check_bits(renders[name], name)
    assert renders[name].aov_direct_info["chunks"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("traversal", [crt.TRAVERSAL_REFERENCE, crt.TRAVERSAL_FAST], ids=["reference", "fast"])
def test_direct_bits_with_the_other_traversals(renders, traversal):
    check_bits(renders["cornell-box"], "cornell-box", traversal=traversal)


@pytest.mark.gpu
def test_direct_on_the_fallback_pipeline(renders, monkeypatch):
    monkeypatch.setenv("CRT_PIPELINE", "2")
    check_bits(renders["cornell-box"], "cornell-box")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_direct_is_the_frame_of_the_render_kernel_at_p_rr_0(renders, name):
    """run_view at p_rr = 0 ends every path at its first vertex: mean == direct bit for bit on every pixel whose emission AOV is zero
    (the oracle leaves out 0.8 % and 2.1 % of the pixels; at most 5 % may be left out)."""
    r = renders[name]
    eye, iv, fov = util.camera(name)
    old = (r.spp, r.light_sample_n, r.P_RR)
    r.set_spp(SPP); r.set_light_sample_n(LSN); r.set_P_RR(0.0)
    r.seed = SEED
    try:
        r.run_view(eye, iv, fov, width=W, height=H)
        mean = r.mean_buffer.copy()
        direct = r.run_view_aov_direct(eye, iv, fov, want=("direct",), width=W, height=H)["direct"]
        emission = r.run_view_aov_shading(eye, iv, fov, want=("emission",), width=W, height=H)["emission"]
    finally:
        r.seed = 0
        r.set_spp(old[0]); r.set_light_sample_n(old[1]); r.set_P_RR(old[2])
    keep = (emission == 0).all(axis=2)
    left_out = 1.0 - keep.mean()
    print("%s: %.2f %% of the pixels left out" % (name, 100 * left_out))
    assert left_out <= 0.05
    util.assert_bits(direct[keep], mean[keep], "%s: direct against the frame's mean" % name)
    assert (direct[keep] != 0).any()


@pytest.mark.gpu
def test_direct_does_not_depend_on_p_rr(renders):
    name = "veach-mis"
    a = run_direct(renders[name], name, p_rr=0.0)
    b = run_direct(renders[name], name, p_rr=0.8)
    util.assert_same(a, b, NAMES, "p_rr 0 against 0.8")
    util.assert_same(a, expected(name), NAMES, name)


@pytest.mark.gpu
def test_direct_ragged_tiles_and_the_division_by_light_sample_n(renders):
    """veach-mis at 37 x 19, spp 3, light_sample_n 3: 12 samples per vertex, ragged tiles in both directions, c / 3 a division"""
    check_bits(renders["veach-mis"], "veach-mis", w=37, h=19, spp=3, lsn=3)


@pytest.mark.gpu
@pytest.mark.parametrize("entries", [5, 1])
def test_direct_sub_batch_borders_change_no_bit(renders, monkeypatch, entries):
    """CRT_AOV_DIRECT_BATCH = 5 x nslots and 1 x nslots: sub-batches that begin and end inside a sample (n_q = 8 on veach-mis)"""
    name = "veach-mis"
    whole = run_direct(renders[name], name)
    assert renders[name].aov_direct_info["chunks"] == 1
    rays = renders[name].aov_direct_info["rays"]
    monkeypatch.setenv("CRT_AOV_DIRECT_BATCH", str(entries * slots_of(W, H)))
    got = run_direct(renders[name], name)
    info = renders[name].aov_direct_info
    assert info["chunks"] == -(-SPP * 8 // entries) > 1 and info["rays"] == rays, info
    util.assert_same(got, whole, NAMES, "sub-batches of %d" % entries)
    util.assert_same(got, expected(name), NAMES, name)


@pytest.mark.gpu
def test_direct_sparse_cases_one_sample_and_no_light_samples(renders):
    name = "cornell-box"
    got = check_bits(renders[name], name, spp=1)
    assert (util.bits(got["direct_variance"]) == 0).all()   # one sample has no variance
    got = check_bits(renders[name], name, lsn=0)
    for n in NAMES[:3]:
        assert (util.bits(got[n]) == 0).all(), n
    assert (got["visibility"] == 1).all()
    assert renders[name].aov_direct_info["rays"] == slots_of(W, H) * SPP


@pytest.mark.gpu
def test_direct_tiled_shards_hold_the_full_frames_pixels(renders):
    """Tiled shards at world 2, ranks 0 and 1: every pixel of the full frame once, padding slots 0"""
    name, world = "cornell-box", 2
    r = renders[name]
    want = expected(name)
    eye, iv, fov = util.camera(name)
    old = (r.spp, r.light_sample_n)
    r.set_spp(SPP); r.set_light_sample_n(LSN)
    r.seed = SEED
    tx, ty = (W + 7) // 8, (H + 7) // 8
    seen = np.zeros((H, W), dtype=int)
    traced = 0
    try:
        for rank in range(world):
            slots = crt.shard_slots(W, H, rank, world)
            assert slots == slots_of(W, H, world)
            bufs, arrs = capi.AovDirectBuffers(), {}
            for n in NAMES:
                arrs[n] = np.full((slots, capi.AOV_DIRECT_BUFFERS[n][0]), 7, dtype=F)
                setattr(bufs, n, arrs[n].ctypes.data)
            cam = r._cam(eye, iv, fov)
            prm = r._params(rank=rank, world=world, flags=capi.FLAG_TILED_OUTPUT, width=W, height=H)
            info = capi.AovInfo()
            capi.check(capi.lib().crt_render_aov_direct(r._h, C.byref(cam), C.byref(prm), C.byref(bufs), C.byref(info)), "crt_render_aov_direct")
            traced += info.rays - slots * SPP
            for s in range(slots):
                tile = (s // 64) * world + rank
                i, j = (tile % tx) * 8 + (s % 64) % 8, (tile // tx) * 8 + (s % 64) // 8
                if tile < tx * ty and i < W and j < H:
                    seen[j, i] += 1
                    for n in NAMES:
                        assert (util.bits(arrs[n][s]) == util.bits(want[n][j, i]).reshape(-1)).all(), (n, rank, s)
                else:
                    for n in NAMES:
                        assert (util.bits(arrs[n][s]) == 0).all(), (n, rank, s)
    finally:
        r.seed = 0
        r.set_spp(old[0]); r.set_light_sample_n(old[1])
    assert (seen == 1).all() and traced == want["traced"]


@pytest.mark.gpu
def test_direct_device_form_on_a_stream_matches_host_form(renders):
    name = "veach-mis"
    r = renders[name]
    want = run_direct(r, name)
    eye, iv, fov = util.camera(name)
    old = (r.spp, r.light_sample_n)
    r.set_spp(SPP); r.set_light_sample_n(LSN)
    r.seed = SEED
    try:
        with DeviceBuffers.image(dict(capi.AOV_DIRECT_BUFFERS), W, H) as d:
            assert d.stream
            assert r.run_view_aov_direct_device(eye, iv, fov, dict(d.ptrs), stream=d.stream, want_info=False, width=W, height=H) is None
            d.synchronize()
            util.assert_same(d.fetch(want), want, NAMES, "device form")
            d.fill("visibility", 0)
            info = r.run_view_aov_direct_device(eye, iv, fov, {"visibility": d.ptrs["visibility"]}, stream=d.stream, width=W, height=H)
            assert info["chunks"] == 1 and info["rays"] == slots_of(W, H) * SPP + expected(name)["traced"] and info["total_ms"] > 0
            util.assert_same(d.fetch(["visibility"]), want, ("visibility",), "subset")
            with pytest.raises(ValueError):
                r.run_view_aov_direct_device(eye, iv, fov, {"albedo": d.ptrs["direct"]}, width=W, height=H)
    finally:
        r.seed = 0
        r.set_spp(old[0]); r.set_light_sample_n(old[1])
    util.assert_same(want, expected(name), NAMES, name)


@pytest.mark.gpu
def test_direct_leaves_the_handles_other_state_alone(renders):
    """A progressive frame in flight is untouched -- preview gives the same bits before and after the pass -- and crt_render_aov and
    crt_render_aov_shading, which share the query pool, return their usual bits after it."""
    name = "cornell-box"
    r = renders[name]
    eye, iv, fov = util.camera(name)
    first_before = aov.run_aov(r, name, SPP, W, H, seed=SEED)
    old = (r.spp, r.light_sample_n)
    r.set_spp(SPP); r.set_light_sample_n(LSN)
    r.seed = SEED
    try:
        r.run_view_range(eye, iv, fov, 0, 2, width=W, height=H)
        rgb0, mean0, done0 = r.preview(want_mean=True, width=W, height=H)
        got = r.run_view_aov_direct(eye, iv, fov, width=W, height=H)
        rgb1, mean1, done1 = r.preview(want_mean=True, width=W, height=H)
        assert done0 == done1 == 2 and np.array_equal(rgb0, rgb1)
        util.assert_bits(mean1, mean0, "preview after the pass")
        r.run_view_range(eye, iv, fov, 2, 2, width=W, height=H)
        ranged = r.mean_buffer.copy()
        r.run_view(eye, iv, fov, width=W, height=H)
        util.assert_bits(ranged, r.mean_buffer, "ranges with the pass in between against the one-shot frame")
        shading = r.run_view_aov_shading(eye, iv, fov, first=aov.NAMES, width=W, height=H)
    finally:
        r.seed = 0
        r.set_spp(old[0]); r.set_light_sample_n(old[1])
    util.assert_same(got, expected(name), NAMES, name)
    util.assert_same(aov.run_aov(r, name, SPP, W, H, seed=SEED), first_before, aov.NAMES, "crt_render_aov after the pass")
    util.assert_same(shading, first_before, aov.NAMES, "crt_render_aov_shading after the pass")
    util.assert_same(first_before, aov.expected_aov(name, W, H, SPP, seed=SEED), aov.NAMES, "crt_render_aov against the oracle")


@pytest.mark.gpu
def test_cli_writes_the_direct_files(renders, tmp_path):
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    name = "veach-mis"
    prefix = str(tmp_path / "veach")
    t = util.task(name)
    res = subprocess.run([cli, util.SCENES[name], "-o", prefix + ".png", "--spp", "2", "--width", "48", "--height", "36", "--seed", "42", "--base-dir", util.ROOT,
                          "--aov-direct", prefix], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    got = run_direct(renders[name], name, spp=2, w=48, h=36, lsn=t.light_sample_n, seed=42)
    assert (got["direct"] != 0).any()
    for n in NAMES:
        hdr, a = util.read_pfm("%s_%s.pfm" % (prefix, n))
        assert hdr[0] == (b"Pf" if n == "visibility" else b"PF") and hdr[2] == b"-1.0"
        assert (util.bits(a) == util.bits(got[n])).all(), n
    bad = subprocess.run([cli, util.SCENES[name], "--devices", "0,0", "--gather", "copy", "--aov-direct", prefix], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "--aov-direct" in bad.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("variance_guided", [False, True], ids=["plain", "variance-guided"])
def test_split_direct_is_the_composition_of_the_public_calls(renders, variance_guided):
    """run_view_denoised(split_direct=True): direct (with direct_variance) and mean - direct (with the frame's variance) filtered
    separately with the same settings, added, and tone-mapped with the frame's operator -- the same made by hand from the public calls."""
    name = "cornell-box"
    r = renders[name]
    eye, iv, fov = util.camera(name)
    old = (r.spp, r.light_sample_n)
    r.set_spp(SPP); r.set_light_sample_n(LSN)
    r.seed = SEED
    try:
        rgb, mean = r.run_view_denoised(eye, iv, fov, width=W, height=H, variance_guided=variance_guided, split_direct=True)
        unsplit_rgb, unsplit = r.run_view_denoised(eye, iv, fov, width=W, height=H, variance_guided=variance_guided)
        r.run_view(eye, iv, fov, width=W, height=H, want_variance=True)
        frame, var = r.mean_buffer.copy(), r.variance_buffer.copy()
        guides = r.run_view_aov(eye, iv, fov, want=("albedo", "normal", "depth"), width=W, height=H)
        d = r.run_view_aov_direct(eye, iv, fov, want=("direct", "direct_variance"), width=W, height=H)
    finally:
        r.seed = 0
        r.set_spp(old[0]); r.set_light_sample_n(old[1])
    rest = frame - d["direct"]
    assert rest.dtype == F
    if variance_guided:
        a = crt.denoise_var(d["direct"], d["direct_variance"], guides["albedo"], guides["normal"], guides["depth"])[1]
        b = crt.denoise_var(rest, var, guides["albedo"], guides["normal"], guides["depth"])[1]
    else:
        a = crt.denoise(d["direct"], guides["albedo"], guides["normal"], guides["depth"])[1]
        b = crt.denoise(rest, guides["albedo"], guides["normal"], guides["depth"])[1]
    want = a + b
    assert want.dtype == F
    util.assert_bits(mean, want, "split_direct")
    assert np.array_equal(rgb, crt.modulate(a, np.zeros_like(a), b)[0])   # (a zero albedo passes a through: a + b and the frame's tone map)
    assert not np.array_equal(rgb, unsplit_rgb)
    assert (util.bits(mean) != util.bits(unsplit)).any()
