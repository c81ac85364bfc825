"""Dual reprojection of the temporal history (crt_temporal_dual / crt_temporal_dual_device, include/crt.h; dual= of temporal and
temporal_device, specular= of Render.run_view_temporal in Python; crt::Render::run_temporal_specular; crt_cli --temporal-specular).

The contract is restated in numpy float32 in tests/temporal_dual_restated.py, on the restatements of crt_temporal and
crt_temporal_clamped; the device result must match it bit for bit: colour, variance, history length, RGB8 and all four counts.  The
restatement itself is checked against plain geometry on the CPU -- a mirror, and behind the camera a plane it reflects -- and the
kernel's text also runs on the host (tools/temporal_host_check.cpp), plain and under the sanitizers, as a stand-alone program.
"""
import ctypes as C
import inspect
import subprocess

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import host_program as HP
import oracle_lib as O
import temporal_dual_restated as D
import temporal_clamp_restated as TC
import temporal_restated as T
import util
from frames import renders  # noqa: F401
from util import assert_bits

F = np.float32
INF = float("inf")
EXPORTS = ("crt_temporal_dual_defaults", "crt_temporal_dual", "crt_temporal_dual_device")
HOST_CHECK_SUMMARY = "91 cases, 0 failures"
SPEC_NAMES = ("path_depth", "bounces", "last_normal")


def dual_dict(dual):
    return None if dual is None else {"radius": dual[0], "min_bounces": dual[1]}


def clamp_dict(clamp):
    return None if clamp is None else {"radius": clamp[0], "gamma": clamp[1]}


def check_against_restatement(cur, cam, prev, pcam, clamp, dual, where, **kw):
    """crt.temporal(dual=...) against the restatement, bit for bit; returns (rgb, color, variance, history, info, masks)"""
    rgb, color, var, hist, info = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, return_info=True, clamp=clamp_dict(clamp),
                                               dual=True if dual is None else dual_dict(dual), **kw)
    want_c, want_v, want_h, masks = D.restated_dual(cur, cam, prev, pcam, clamp=clamp, dual=dual, **kw)
    assert_bits(color, want_c, where + ": colour")
    assert_bits(hist, want_h, where + ": history")
    if want_v is None:
        assert var is None
    else:
        assert_bits(var, want_v, where + ": variance")
    assert np.array_equal(rgb, O.tonemap(color)), where + ": rgb is not the tone map of the colour"
    got = {k: info[k] for k in ("reprojected", "clamped", "virtual_tried", "virtual_taken")}
    assert got == D.counts(masks), (where, info, D.counts(masks))
    return rgb, color, var, hist, info, masks


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_dual_entry_points_and_defaults():
    lib = capi.lib()
    for name in EXPORTS:
        assert name in capi.EXPORTS and getattr(lib, name)
    d = capi.TemporalDual()
    C.memset(C.byref(d), 0x7f, C.sizeof(d))
    assert lib.crt_temporal_dual_defaults(C.byref(d)) == capi.CRT_OK
    assert (d.radius, d.min_bounces) == (1, 0.5)             # include/crt.h: tuned on nothing
    assert crt.temporal_dual_defaults() == {"radius": 1, "min_bounces": 0.5} == D.DEFAULTS
    assert lib.crt_temporal_dual_defaults(None) == capi.ERR_INVALID_ARG and lib.crt_last_error()
    assert lib.crt_abi_version() == 5
    assert C.sizeof(capi.TemporalDual) == 8 and C.sizeof(capi.TemporalSpecularPlanes) == 24 and C.sizeof(capi.TemporalDualInfo) == 40
    for f in (crt.temporal, crt.temporal_device):
        assert inspect.signature(f).parameters["dual"].default is None
    assert inspect.signature(crt.Render.run_view_temporal).parameters["specular"].default is False
    frame = {"color": np.zeros((4, 4, 3), F), "depth": np.zeros((4, 4), F), "path_depth": np.zeros((4, 4), F), "bounces": np.zeros((4, 4), F)}
    camera = (np.zeros(3), np.zeros(9), 1.0)
    for bad in (False, 1.0, {"gamma": 1.0}, {"radius": 1.5}):
        with pytest.raises(ValueError):
            crt.temporal(frame, camera, dual=bad)
    with pytest.raises(ValueError, match="moments"):
        crt.temporal(frame, camera, dual=True, moments=True)
    with pytest.raises(ValueError, match="moments"):
        crt.temporal_device(4, 4, camera, {}, 1, 1, dual=True, moments={"out_m1": 1, "out_m2": 1})
    with pytest.raises(ValueError, match="moments"):          # (refused before the handle is looked at)
        crt.Render.run_view_temporal(None, np.zeros(3), np.zeros(9), 1.0, specular=True, variance="moments")
    for bad in (None, 1, {"gamma": 1.0}):
        with pytest.raises(ValueError, match="specular"):
            crt.Render.run_view_temporal(None, np.zeros(3), np.zeros(9), 1.0, specular=bad)
    with pytest.raises(NotImplementedError):
        crt.MultiRender.run_view_temporal(None)


def test_dual_arguments_are_checked_before_any_device_call():
    """Every invalid call of both forms is CRT_ERR_INVALID_ARG, also on a machine without a GPU.  The non-null buffers are dummies that
    must never be dereferenced."""
    lib = capi.lib()
    dummy = C.create_string_buffer(256)
    d = C.cast(dummy, C.c_void_p)

    def params(**over):
        p = capi.TemporalParams()
        assert lib.crt_temporal_defaults(C.byref(p)) == capi.CRT_OK
        p.width, p.height = 64, 48
        for k, v in over.items():
            setattr(p, k, v)
        return C.byref(p)

    def clamp(**over):
        c = capi.TemporalClamp()
        assert lib.crt_temporal_clamp_defaults(C.byref(c)) == capi.CRT_OK
        for k, v in over.items():
            setattr(c, k, v)
        return C.byref(c)

    def dual(**over):
        c = capi.TemporalDual()
        assert lib.crt_temporal_dual_defaults(C.byref(c)) == capi.CRT_OK
        for k, v in over.items():
            setattr(c, k, v)
        return C.byref(c)

    def frame(**over):
        return C.byref(capi.TemporalFrame(**dict(dict(color=d, variance=d, depth=d, normal=d, id=d), **over)))

    def history(**over):
        return C.byref(capi.TemporalHistory(**dict(dict(color=d, variance=d, history=d, depth=d, normal=d, id=d), **over)))

    def spec(**over):
        return C.byref(capi.TemporalSpecularPlanes(**dict(dict(path_depth=d, bounces=d, last_normal=d), **over)))

    def both(prm, cl, du, cur, cspec, prev, pspec, color=d, var=d, hist=d, rgb=d, status=capi.ERR_INVALID_ARG, device=0):
        r1 = lib.crt_temporal_dual(device, prm, cl, du, cur, cspec, prev, pspec, color, var, hist, rgb, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_temporal_dual_device(device, prm, cl, du, cur, cspec, prev, pspec, color, var, hist, rgb, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == status, (r1, r2, e1, e2)
        assert e1 and e2 and e1.replace(b"_device", b"") == e2.replace(b"_device", b"")
        return e1

    for cl in (clamp(), None):
        for prev, pspec in ((history(), spec()), (None, None)):
            # what this call refuses itself
            assert b"null" in both(params(), cl, None, frame(), spec(), prev, pspec)
            assert b"null" in both(params(), cl, dual(), frame(), None, prev, pspec)
            for radius in (0, 4, 2 ** 32 - 1):
                assert b"radius must be 1 .. 3" in both(params(), cl, dual(radius=radius), frame(), spec(), prev, pspec), radius
            for bad in (0.0, -0.0, -1.0, float("nan"), -INF):
                assert b"min_bounces" in both(params(), cl, dual(min_bounces=bad), frame(), spec(), prev, pspec), bad
            for missing in ("path_depth", "bounces"):
                assert b"path_depth and bounces" in both(params(), cl, dual(), frame(), spec(**{missing: None}), prev, pspec), missing
        for missing in ("path_depth", "bounces"):
            assert b"path_depth and bounces" in both(params(), cl, dual(), frame(), spec(), history(), spec(**{missing: None})), missing
        assert b"last normals" in both(params(), cl, dual(), frame(), spec(last_normal=None), history(), spec())
        assert b"last normals" in both(params(), cl, dual(), frame(), spec(), history(), spec(last_normal=None))
        assert b"go together" in both(params(), cl, dual(), frame(), spec(), history(), None)
        assert b"go together" in both(params(), cl, dual(), frame(), spec(), None, spec())
        # everything crt_temporal_clamped refuses
        assert b"null" in both(None, cl, dual(), frame(), spec(), history(), spec())
        assert b"null" in both(params(), cl, dual(), None, spec(), history(), spec())
        for prev, pspec in ((history(), spec()), (None, None)):
            both(params(), cl, dual(), frame(color=None), spec(), prev, pspec)
            both(params(), cl, dual(), frame(depth=None), spec(), prev, pspec)
            both(params(), cl, dual(), frame(), spec(), prev, pspec, color=None)
            both(params(), cl, dual(), frame(), spec(), prev, pspec, hist=None)
            both(params(width=0), cl, dual(), frame(), spec(), prev, pspec)
            both(params(height=0), cl, dual(), frame(), spec(), prev, pspec)
            for name in ("depth_tolerance", "normal_tolerance"):
                for bad in (0.0, -1.0, float("nan")):
                    assert b"tolerance" in both(params(**{name: bad}), cl, dual(), frame(), spec(), prev, pspec), (name, bad)
            for bad in (0.0, 1.5, float("nan")):
                assert b"alpha_min" in both(params(alpha_min=bad), cl, dual(), frame(), spec(), prev, pspec), bad
            assert b"variance" in both(params(), cl, dual(), frame(variance=None), spec(), prev, pspec)
            assert b"variance" in both(params(), cl, dual(), frame(), spec(), prev, pspec, var=None)
        for missing in ("color", "history", "depth"):
            assert b"history" in both(params(), cl, dual(), frame(), spec(), history(**{missing: None}), spec()), missing
        assert b"variance" in both(params(), cl, dual(), frame(), spec(), history(variance=None), spec())
        assert b"normals" in both(params(), cl, dual(), frame(normal=None), spec(), history(), spec())
        assert b"IDs" in both(params(), cl, dual(), frame(), spec(), history(id=None), spec())
        both(params(width=(1 << 24) + 1), cl, dual(), frame(), spec(), history(), spec(), status=capi.ERR_UNSUPPORTED)
        assert b"device index" in both(params(), cl, dual(), frame(), spec(), history(), spec(), device=-1)
        # +inf is a min_bounces, and last normals may be left out of both frames: the device index is what fails
        assert b"device index" in both(params(), cl, dual(min_bounces=INF, radius=3), frame(), spec(last_normal=None), history(), spec(last_normal=None), device=-1)
    for radius in (0, 4):
        assert b"clamp's radius" in both(params(), clamp(radius=radius), dual(), frame(), spec(), history(), spec())
    assert b"gamma" in both(params(), clamp(gamma=-1.0), dual(), frame(), spec(), history(), spec())


def test_cli_refuses_temporal_specular_it_cannot_run():
    from cudaraytracing_amd import build as b
    cli, cfg = b.build_cli(), util.SCENES["veach-mis"]
    for args in (["--temporal-specular"], ["--temporal-specular", "0.5"], ["--temporal", "2", "--temporal-specular", "x"],
                 ["--temporal", "2", "--temporal-specular", "0"], ["--temporal", "2", "--temporal-specular", "-1"],
                 ["--temporal", "2", "--temporal-specular", "nan"], ["--temporal", "2", "--temporal-specular", "0.5,0"],
                 ["--temporal", "2", "--temporal-specular", "0.5,4"], ["--temporal", "2", "--temporal-specular", "0.5,1,0"],
                 ["--temporal", "2", "--temporal-specular", "0.5,1,9"], ["--temporal", "2", "--temporal-specular", "0.5,1,2,3"],
                 ["--temporal", "2", "--temporal-specular", "0.5,"], ["--temporal", "2", "--temporal-specular", "0.5x"]):
        bad = subprocess.run([cli, cfg, "--base-dir", util.ROOT] + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "--temporal" in bad.stderr and "--temporal-specular" in bad.stderr, (args, bad.stderr)
    for args in (["--temporal", "2", "--temporal-specular", "--temporal-variance", "moments"],
                 ["--temporal", "2", "--temporal-variance", "moments,2", "--temporal-specular", "0.25,2"]):
        bad = subprocess.run([cli, cfg, "--base-dir", util.ROOT] + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "--temporal-specular" in bad.stderr and "--temporal-variance moments" in bad.stderr, (args, bad.stderr)


@pytest.mark.parametrize("size", [(64, 48), (61, 47)])
@pytest.mark.parametrize("move", [(10, 0, 0), (7.3, -4.1, 0), (3, 2, 15), (0, 0, -20)])
def test_restatement_reprojects_a_mirror_image(size, move):
    """The restated contract against geometry (no device, and no line of the contract on the expected side).  A camera looks along +z at a
    mirror in the plane z = 100; behind it lies the plane z = -50, coloured linearly in world x and y, which every pixel sees in the
    mirror.  First-hit depth and id are the mirror's and do not change when the camera moves; path_depth runs on to the reflected plane.
    The reflected point has the x and y of the virtual point on the pixel's straight ray, in the plane z = 250, and that point moves rigidly:
    seen from the previous camera the colour is linear in the pixel coordinates, so its bilinear interpolation where the virtual point
    lands is the colour the pixel shows now -- exact up to a few dozen fp32 roundings; bound 1e-5 relative, test_restatement_reprojects_a_plane's
    for its reason.  The history is read out of the restatement before the blend (want_history_colour), the current colour is what the pixel shows.
    crt_temporal's own reprojection follows the mirror's surface instead: under the sideways moves the history it fetches shows a point
    1.5 x the move away (|eye.x| (zm - zq) / zm): in every pixel at least 5 % of its worst channel, more than 100 times the bound.
    Pixels whose taps are all inside: the four bilinear taps in the previous frame and the 3 x 3 taps of the choice in the current one.  On
    the image's border the mean over the clipped neighbourhood of an affine colour lies half a pixel's gradient from the pixel's own colour,
    so a surface history that errs by less than a pixel's gradient can lie nearer to it and is kept by the contract's rule; measured: the
    three pixels (12 .. 14, 0) of the 64 x 48 frame and three of the 61 x 47 one under the move (3, 2, 15), error 1.1e-2, none elsewhere."""
    W, H = size
    pcam, pframe, _ = D.mirror_scene(W, H, (0, 0, 0))
    cam, frame, Pv = D.mirror_scene(W, H, move)
    prev = dict(D.as_float32(pframe), history=np.full((H, W), 1e6, dtype=F))
    cur = D.as_float32(frame)
    out, var, hist, masks, Hh = D.restated_dual(cur, cam, prev, pcam, alpha_min=2.0 ** -20, want_history_colour=True)
    assert var is None
    # where the virtual point lands in the previous frame, in float64 and from the point alone
    scale = np.tan(np.float64(pcam[2]) / 2)
    c = (Pv - pcam[0].astype(np.float64)) @ pcam[1].astype(np.float64).reshape(3, 3).T
    fx = ((-c[..., 0] / c[..., 2]) / (scale * W / H) + 1) * W / 2 - 0.5
    fy = (1 - (c[..., 1] / c[..., 2]) / scale) * H / 2 - 0.5
    inside = (fx >= 0) & (fx <= W - 1) & (fy >= 0) & (fy <= H - 1)
    inside[0, :] = inside[-1, :] = inside[:, 0] = inside[:, -1] = False
    assert inside.sum() > W * H // 4
    # (where the camera moves along its axis both candidates land on the same point in the middle of the frame, and S is kept when its
    # colour is as near: the bound below holds for whichever candidate was taken)
    assert masks["tried"].all() and masks["took"][inside].all() and masks["took_V"][inside].sum() > inside.sum() * 3 // 4
    want = T.plane_colour(Pv)
    rel = np.abs(Hh.astype(np.float64) - want) / np.abs(want)
    surface = TC.history_colour(D.surface_inputs(cur), cam, D.surface_inputs(prev), pcam, 0.05, 0.5)
    took_S = T.restated(D.surface_inputs(cur), cam, D.surface_inputs(prev), pcam)[3]
    rel_S = np.abs(surface.astype(np.float64) - want) / np.abs(want)
    print("%dx%d move %r: %d pixels inside, largest relative error of the dual history %.3g, of crt_temporal's %.3g (smallest over the pixels' worst channel %.3g)"
          % (W, H, move, inside.sum(), rel[inside].max(), rel_S[inside & took_S].max(), rel_S[inside & took_S].max(axis=1).min()))
    assert rel[inside].max() < 1e-5
    assert np.abs(hist[inside] - 1e6).max() < 2
    if move[2] == 0:                                        # the sideways moves: the defect, without a renderer
        both = inside & took_S                              # (the mirror is nearer than the virtual image: its reprojection leaves the frame sooner)
        assert both.sum() > W * H // 4
        assert rel_S[both].max() > 100 * 1e-5
        assert rel_S[both].max(axis=1).min() > 100 * 1e-5   # ... in every pixel


@pytest.mark.parametrize("seed", [21, 22])
def test_restatement_that_never_tries_is_crt_temporal_clampeds(seed):
    cur, cam, prev, pcam = D.synthetic(64, 48, seed)
    zero = dict(cur, bounces=np.zeros((48, 64), dtype=F))
    for clamp in (None, (1, 1.0), (2, 0.5)):
        want = TC.restated_clamped(D.surface_inputs(cur), cam, D.surface_inputs(prev), pcam, clamp=clamp)
        assert want[3].sum() >= 100
        for c, dual in ((cur, (1, INF)), (cur, (3, INF)), (zero, (1, 0.5)), (zero, (2, 1e-30))):
            got = D.restated_dual(c, cam, prev, pcam, clamp=clamp, dual=dual)
            for g, w, what in zip(got[:3], want[:3], ("colour", "variance", "history")):
                assert_bits(g, w, "clamp %r dual %r: %s" % (clamp, dual, what))
            m = got[3]
            assert np.array_equal(m["took"], want[3]) and np.array_equal(m["clamped"], want[4]) and not m["tried"].any() and not m["took_V"].any()
        # ... and with the defaults it is something else: every branch of the choice is taken on these inputs
        m = D.restated_dual(cur, cam, prev, pcam, clamp=clamp)[3]
        assert (m["took_V"] & want[3]).sum() >= 50 and (m["took_V"] & ~want[3]).sum() >= 50 and (m["tried"] & ~m["took_V"] & m["took"]).sum() >= 50


@pytest.fixture(scope="module")
def host_check_run(tmp_path_factory):
    """both builds of tools/temporal_host_check.cpp, each run as `program - out`: [(status, bytes, printed) plain, sanitised]"""
    return HP.run_both_forms("temporal_host_check.cpp", str(tmp_path_factory.mktemp("temporal_host")), "-")


def test_kernel_text_on_the_host_passes_its_checks(host_check_run):
    """csrc/crt_temporal.h as it is -- the per-pixel text of k_temporal_dual and of the four k_temporal kernels -- compiled with g++
    -ffp-contract=off, against the program's own scalar restatement of the contract: 70 x 19, 5 x 3 and 1 x 1; radius 1 and 3; with and without a clamp; min_bounces 0.5 and +inf; finite inputs, NaN and +-inf in the
    colours, path_depth and bounces, and frames without variance, normals and ids; no history; then the mirror scene of
    test_restatement_reprojects_a_mirror_image with its bounds.  The summary line carries the case count."""
    rc, raw, printed = host_check_run[0]
    assert rc == 0, printed
    assert HOST_CHECK_SUMMARY in printed.splitlines(), printed
    assert len(raw) > 0


def test_kernel_text_is_clean_under_the_sanitizers(host_check_run):
    """the same stand-alone program built with -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all (nothing is
    preloaded): exit status 0, the same summary and the same bytes -- no tap outside its image (each has exactly its size)"""
    rc, raw, printed = host_check_run[1]
    assert rc == 0, printed
    assert HOST_CHECK_SUMMARY in printed.splitlines(), printed
    assert raw == host_check_run[0][1]


# ------------------------------------------------------------------------------------------------------------------ GPU --

@pytest.mark.gpu
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("w,h", [(130, 9), (61, 47)])
def test_dual_shapes_that_can_go_wrong(w, h, radius):
    """130 x 9: three 64-wide blocks and three 4-row blocks, the last of each partial; 61 x 47: one partial block across.  Cameras that
    differ by a translation, a rotation and in fov_y; holes in either frame's depth and path_depth; bounces of 0, 0.25, 0.5 (== min_bounces),
    0.75 and 1; a black history (an exact tie: both candidates 0) and a block where the virtual point is the surface point (the same
    taps); blocks where only V's taps can count and where only S's can.  With and without a clamp (its radius equal to the choice's and
    not), with and without last normals, a min_bounces below every positive bounces value; then no history at all."""
    cur, cam, prev, pcam = D.synthetic(w, h, 31 + radius)
    for clamp in (None, (radius, 1.0), (1 + radius % 3, 0.5)):
        where = "synthetic %dx%d radius %d clamp %r" % (w, h, radius, clamp)
        m = check_against_restatement(cur, cam, prev, pcam, clamp, (radius, 0.5), where)[5]
        took_S = T.restated(D.surface_inputs(cur), cam, D.surface_inputs(prev), pcam)[3]
        assert (m["took_V"] & took_S).sum() >= 30 and (m["took_V"] & ~took_S).sum() >= 30, where       # V against S, and V alone
        assert (m["tried"] & ~m["took_V"] & m["took"]).sum() >= 30 and (~m["tried"] & m["took"]).sum() >= 30, where     # S kept, and S alone
        assert (m["tried"] & ~m["took"]).sum() >= 1 and ((cur["bounces"] == F(0.5)) & m["tried"]).sum() >= 30, where
        if clamp is not None:
            assert m["clamped"].sum() >= 30 and (clamp[1] != 1.0 or m["took"].sum() - m["clamped"].sum() >= 30), where
    drop = lambda f: {k: v for k, v in f.items() if k != "last_normal"}
    check_against_restatement(drop(cur), cam, drop(prev), pcam, (radius, 1.0), (radius, 0.2), "no last normals %dx%d" % (w, h))
    none = check_against_restatement(cur, cam, None, None, (radius, 1.0), (radius, 0.5), "no history %dx%d" % (w, h))
    assert none[4]["reprojected"] == none[4]["virtual_tried"] == 0 and (none[3] == 1).all()


@pytest.mark.gpu
def test_dual_ties_keep_the_surface_history():
    """the planted ties of the synthetic frames, counted on the restatement: where both candidates are valid and their distances are
    equal to the bit, the output is the surface candidate's -- the bits crt_temporal_clamped writes there"""
    cur, cam, prev, pcam = D.synthetic(61, 47, 40)
    _, color, _, hist, _, m = check_against_restatement(cur, cam, prev, pcam, None, (1, 0.5), "ties")
    cs, ps = D.surface_inputs(cur), D.surface_inputs(prev)
    H_S = TC.history_colour(cs, cam, ps, pcam, 0.05, 0.5)
    H_V = TC.history_colour(D.virtual_inputs(cur, 0.5, False), cam, D.virtual_inputs(prev, 0.5, True), pcam, 0.05, 0.5)
    mu = D.mean_colour(cur["color"], 1)
    plain = T.restated(cs, cam, ps, pcam)
    valid_V = m["tried"] & T.restated(D.virtual_inputs(cur, 0.5, False), cam, D.virtual_inputs(prev, 0.5, True), pcam)[3]
    tie = valid_V & plain[3] & (D.distance(H_S, mu) == D.distance(H_V, mu))
    assert tie.sum() >= 30 and not m["took_V"][tie].any()
    assert_bits(color[tie], plain[0][tie], "ties: colour")
    assert_bits(hist[tie], plain[2][tie], "ties: history")


@pytest.mark.gpu
def test_dual_non_finite_pixels():
    """NaN and +-inf in every plane of both frames: in the colours (a NaN distance keeps S; a NaN mean keeps S in every neighbourhood it
    lies in), in path_depth and depth (no projection, or no tap), in bounces (a NaN is no mirror; +inf is one), in the history length and
    the variance -- bit for bit, with the tests on and off"""
    cur, cam, prev, pcam = D.synthetic(70, 45, 22)
    rng = np.random.default_rng(5)
    bad = (np.nan, np.inf, -np.inf)
    for f in (cur, prev):
        for name, plane in f.items():
            if name == "id":
                continue
            flat = plane.reshape(-1)
            at = rng.choice(flat.size, 12, replace=False)
            flat[at] = np.resize(np.array(bad, dtype=F), 12)
    for kw in ({}, {"depth_tolerance": INF, "normal_tolerance": INF}):
        for clamp, dual in ((None, (1, 0.5)), ((2, 1.0), (2, 0.5)), ((1, 0.0), (3, 0.75)), ((3, INF), (1, INF))):
            where = "non-finite clamp %r dual %r %r" % (clamp, dual, kw)
            _, color, var, hist, info, m = check_against_restatement(cur, cam, prev, pcam, clamp, dual, where, **kw)
            assert np.isnan(color).any() and np.isinf(color).any() and np.isfinite(color).any()
            if dual[1] != INF:
                assert m["took_V"].sum() >= 100, where
            else:
                assert m["tried"].sum() == int(((cur["bounces"] == np.inf) & (cur["path_depth"] > 0)).sum()), where


def spec_frames(renders, name, width, height, n, seed0, cameras=None):
    """temporal_restated.frames with the three specular planes of each frame in its dict (the pass runs with the frame's spp and seed)"""
    fr = T.frames(renders, name, width, height, n, seed0) if cameras is None else [
        T.render_frame(renders[name], cam, width, height, 4, seed0 + f) + (cam,) for f, cam in enumerate(cameras)]
    out = []
    r = renders[name]
    for f, (cur, rgb, g, cam) in enumerate(fr):
        r.set_spp(4)
        r.seed = seed0 + f
        try:
            spec = r.run_view_aov_specular(*cam, want=SPEC_NAMES, width=width, height=height)
        finally:
            r.seed = 0
        out.append((dict(cur, **spec), rgb, g, cam))
    return out


def chain(fr, clamp, dual, where, check=True):
    """The frames accumulated with the dual pass, each output the next call's history; the last call's results"""
    prev = pcam = out = None
    for f, (cur, _, _, cam) in enumerate(fr):
        if check:
            out = check_against_restatement(cur, cam, prev, pcam, clamp, dual, "%s frame %d" % (where, f))
        else:
            out = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, clamp=clamp_dict(clamp), dual=True if dual is None else dual_dict(dual),
                               return_info=True)
        prev, pcam = T.as_history(cur, out[1], out[2], out[3]), cam
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("clamp", [None, (1, 1.0)], ids=["no clamp", "the clamp's defaults"])
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_dual_rendered_chains_match_restatement(renders, name, clamp):
    """Four chained frames of a moving camera (64 x 48, spp 4, seeds 100 .. 103, temporal_restated's moves): an output is the next frame's
    history, compared after every frame.  On the CPU oracle's frames (the device's, bit for bit) through the restatements, with the
    clamp's defaults, the last call on veach-mis tries V on 1055 pixels and takes it on 327 of the 3072 (10.6 %; the plates cover a
    third of the view); cornell-box has no mirror, tries nothing, and writes crt_temporal_clamped's bits."""
    where = "%s 64x48 clamp %r" % (name, clamp)
    fr = spec_frames(renders, name, 64, 48, 8, 100)[:4]
    _, color, var, hist, info, m = chain(fr, clamp, None, where)
    print("%s: tried %d, taken %d of %d" % (where, info["virtual_tried"], info["virtual_taken"], 64 * 48))
    if name == "veach-mis":
        assert info["virtual_taken"] >= 0.01 * 64 * 48
    else:
        assert info["virtual_tried"] == 0
        plain = TC.chain([(D.surface_inputs(c), a, b, cam) for c, a, b, cam in fr], "full", clamp, "", check=False)
        assert_bits(color, plain[1], where + ": colour against crt_temporal_clamped")
        assert_bits(var, plain[2], where + ": variance against crt_temporal_clamped")
        assert_bits(hist, plain[3], where + ": history against crt_temporal_clamped")
        assert np.array_equal(fr[-1][0]["bounces"], np.zeros((48, 64), dtype=F))


def run_device(cur, cam, prev, pcam, clamp, dual, stream=False, variance=True, out_rgb=True, want_info=True):
    """crt.temporal_device on uploaded copies, with dual= or without: (color, variance, history, rgb, info); what the call does not
    write keeps its fill (0x55)"""
    h, w = cur["color"].shape[:2]
    host = {"cur_" + k: v for k, v in cur.items()}
    host.update({"prev_" + k: v for k, v in prev.items()})
    outs = {"out_color": w * h * 12, "out_var": w * h * 12, "out_hist": w * h * 4, "out_rgb": w * h * 3}
    with DeviceBuffers({**host, **outs}, stream=stream) as d:
        ptrs = d.ptrs
        for n in outs:
            d.fill(n)
        keep = lambda f, pre: {k: ptrs[pre + k] for k in f if (variance or k != "variance") and (dual is not None or k not in SPEC_NAMES)}
        info = crt.temporal_device(w, h, cam, keep(cur, "cur_"), ptrs["out_color"], ptrs["out_hist"], out_variance_ptr=ptrs["out_var"] if variance else None,
                                   out_rgb_ptr=ptrs["out_rgb"] if out_rgb else None, prev_ptrs=keep(prev, "prev_"), prev_camera=pcam,
                                   stream=d.stream if stream else None, want_info=want_info, clamp=clamp_dict(clamp), dual=dual_dict(dual))
        d.synchronize()
        return (d.download("out_color", (h, w, 3), F), d.download("out_var", (h, w, 3), F), d.download("out_hist", (h, w), F),
                d.download("out_rgb", (h, w, 3), np.uint8), info)


@pytest.mark.gpu
def test_dual_that_never_tries_is_crt_temporal_clamped_device(renders):
    """min_bounces = +inf, and bounces zero everywhere, each against crt_temporal_clamped_device with the same clamp and against
    crt_temporal_device for a NULL clamp: colour, variance, history, RGB8 and the counts"""
    name, w, h = "veach-mis", 100, 70
    (c0, _, _, cam0), (c1, _, _, cam1) = spec_frames(renders, name, w, h, 2, 50)
    prev = T.as_history(c0, c0["color"], c0["variance"], np.full((h, w), 3, dtype=F))
    zero = dict(c1, bounces=np.zeros((h, w), dtype=F))
    assert (c1["bounces"] >= 0.5).sum() >= 100 and np.isfinite(c1["bounces"]).all()
    for clamp in (None, (1, 1.0), (2, 0.5)):
        want = run_device(c1, cam1, prev, cam0, clamp, None)
        assert 100 <= want[4]["reprojected"] < w * h
        for cur, dual in ((c1, (1, INF)), (c1, (3, INF)), (zero, (1, 0.5)), (zero, (2, 0.25))):
            got = run_device(cur, cam1, prev, cam0, clamp, dual)
            where = "clamp %r dual %r" % (clamp, dual)
            for g, wnt, what in zip(got[:3], want[:3], ("colour", "variance", "history")):
                assert_bits(g, wnt, where + ": " + what)
            assert np.array_equal(got[3], want[3]), where
            assert got[4]["reprojected"] == want[4]["reprojected"] and got[4]["clamped"] == want[4].get("clamped", 0), (where, got[4], want[4])
            assert got[4]["virtual_tried"] == got[4]["virtual_taken"] == 0, (where, got[4])
        # ... and with the defaults the call is something else
        some = run_device(c1, cam1, prev, cam0, clamp, (1, 0.5))
        assert some[4]["virtual_taken"] >= 100 and not np.array_equal(some[0], want[0])


@pytest.mark.gpu
def test_dual_device_form_on_a_stream_matches_host_form(renders):
    name, w, h = "veach-mis", 100, 70
    (c0, _, _, cam0), (c1, _, _, cam1) = spec_frames(renders, name, w, h, 2, 50)
    prev = T.as_history(c0, c0["color"], c0["variance"], np.full((h, w), 3, dtype=F))
    clamp, dual = (2, 0.75), (2, 0.25)
    want_rgb, want_c, want_v, want_h, want_info = crt.temporal(c1, cam1, prev=prev, prev_camera=cam0, return_info=True, clamp=clamp_dict(clamp),
                                                               dual=dual_dict(dual))
    assert want_info["virtual_taken"] >= 100 and 100 <= want_info["clamped"] < want_info["reprojected"] - 100
    c, v, hh, r, info = run_device(c1, cam1, prev, cam0, clamp, dual, stream=True, want_info=False)
    assert info is None
    assert_bits(c, want_c, "device form")
    assert_bits(v, want_v, "device form, variance")
    assert_bits(hh, want_h, "device form, history")
    assert np.array_equal(r, want_rgb)
    # colour and history only, with the timer and the counts (the call synchronizes the stream)
    c, v, hh, r, info = run_device(c1, cam1, prev, cam0, clamp, dual, stream=True, variance=False, out_rgb=False)
    assert {k: info[k] for k in want_info if k != "total_ms"} == {k: want_info[k] for k in want_info if k != "total_ms"} and info["total_ms"] > 0, info
    assert_bits(c, want_c, "device form, colour only")
    assert_bits(hh, want_h, "device form, colour only: history")
    assert (r == 0x55).all() and (v.view(np.uint32) == 0x55555555).all()


@pytest.mark.gpu
def test_run_view_temporal_with_specular_equals_the_calls_by_hand(renders):
    name, w, h = "veach-mis", 64, 48
    r = renders[name]
    fr = spec_frames(renders, name, w, h, 3, 40)             # seeds 40, 41, 42: self.seed + the frames since the reset
    one = fr
    r.set_spp(4)
    r.seed = 40
    try:
        for specular, clamp, dual in ((True, True, None), ({"radius": 2, "min_bounces": 0.25}, None, (2, 0.25)), (False, True, None)):
            r.reset_temporal()
            prev = pcam = None
            for f, (cur, noisy_rgb, g, cam) in enumerate(one):
                if specular is False:
                    cur = D.surface_inputs(cur)
                    want = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, return_info=True, clamp=clamp)
                else:
                    want = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, return_info=True, clamp=clamp, dual=True if dual is None else dual_dict(dual))
                want_rgb, want_c, want_v, want_h, want_info = want
                prev, pcam = T.as_history(cur, want_c, want_v, want_h), cam
                rgb, mean = r.run_view_temporal(*cam, width=w, height=h, clamp=clamp, specular=specular)
                where = "run_view_temporal(specular=%r) frame %d" % (specular, f)
                assert_bits(mean, want_c, where)
                assert np.array_equal(rgb, want_rgb), where
                assert_bits(r.variance_buffer, want_v, where + ": variance_buffer")
                assert_bits(r.temporal_history_buffer, want_h, where + ": temporal_history_buffer")
                assert {k: v for k, v in r.temporal_info.items() if k != "total_ms"} == {k: v for k, v in want_info.items() if k != "total_ms"}, where
                assert np.array_equal(r.frame_buffer, noisy_rgb), where
            if specular is False:
                assert "virtual_tried" not in r.temporal_info
                # today's method, bit for bit: the chain of clamped calls
                plain = TC.chain([(D.surface_inputs(c), a, b, cam) for c, a, b, cam in fr], "full", (1, 1.0), "", check=False)
                assert_bits(mean, plain[1], "run_view_temporal(specular=False)")
            else:
                assert r.temporal_info["virtual_taken"] >= 30, r.temporal_info
        # a history without specular planes is not continued with them
        r.run_view_temporal(*one[0][3], width=w, height=h, specular=True)
        assert r.temporal_info["reprojected"] == 0
        # it composes with denoise and demodulate
        r.reset_temporal()
        for f in range(2):
            rgb, mean = r.run_view_temporal(*one[f][3], width=w, height=h, specular=True, clamp=True, denoise=True, demodulate=True)
        assert r.temporal_info["virtual_tried"] >= 100 and rgb.shape == (h, w, 3) and np.isfinite(mean).all()
    finally:
        r.seed = 0
        r.reset_temporal()


@pytest.mark.gpu
def test_render_class_temporal_specular_step(tmp_path):
    """tools/temporal_specular_host_check.cpp: crt::Render::run_temporal_specular against crt_render, crt_variance, crt_render_aov,
    crt_render_aov_specular and crt_temporal_dual called directly on a second handle, bit for bit and count for count, and no history
    carried between it and run_temporal"""
    from cudaraytracing_amd import build as b
    exe = b.build_temporal_specular_check()
    r = subprocess.run([exe, util.SCENES["veach-mis"], util.ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert r.stdout.splitlines()[-1] == "temporal_specular_host_check: ok"


@pytest.mark.gpu
def test_cli_accumulates_a_sequence_with_temporal_specular(renders, tmp_path):
    """veach-mis, the camera and its lookat point moving sideways past the plates (along z: the camera looks down -x) by 0.25 per frame (crt_cli moves both)"""
    from PIL import Image
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    name, w, h, step = "veach-mis", 64, 48, (0.0, 0.0, 0.25)
    t = util.task(name)
    cams = []
    for f in range(3):
        s = F(f) * np.asarray(step, dtype=F)
        cams.append((t.eye_pos + s, crt.get_inverse_view_matrix(t.eye_pos + s, t.lookat + s, t.up), crt.fov_to_radians(t.fov_y)))
    fr = spec_frames(renders, name, w, h, 3, 40, cameras=cams)
    base = [cli, util.SCENES[name], "--spp", "4", "--width", str(w), "--height", str(h), "--seed", "40", "--base-dir", util.ROOT,
            "--temporal", "3", "--temporal-step", ",".join(repr(float(v)) for v in step)]
    last = str(tmp_path / "last.png")
    results = []
    for i, (args, clamp, dual, max_bounces) in enumerate(((["--temporal-specular"], None, None, None),
                                                           (["--temporal-specular", "0.25,2", "--temporal-clamp", "1.5"], (1, 1.5), (2, 0.25), None),
                                                           (["--temporal-specular", "0.5,1,1"], None, (1, 0.5), 1))):
        acc = str(tmp_path / ("acc%d.png" % i))
        res = subprocess.run(base + ["-o", last, "--temporal-out", acc] + args, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        frames = fr
        if max_bounces is not None:
            r = renders[name]
            frames = []
            for f, (cur, rgb, g, cam) in enumerate(fr):
                r.set_spp(4)
                r.seed = 40 + f
                try:
                    frames.append((dict(cur, **r.run_view_aov_specular(*cam, max_bounces=max_bounces, want=SPEC_NAMES, width=w, height=h)), rgb, g, cam))
                finally:
                    r.seed = 0
        want = chain(frames, clamp, dual, "", check=False)
        assert np.array_equal(np.asarray(Image.open(acc)), want[0]), args
        assert np.array_equal(np.asarray(Image.open(last)), fr[-1][1])
        assert "%d pixels tried their virtual image, %d took it" % (want[4]["virtual_tried"], want[4]["virtual_taken"]) in res.stdout, res.stdout
        assert want[4]["virtual_taken"] >= 30
        results.append(want[0])
    plain = TC.chain([(D.surface_inputs(c), a, b, cam) for c, a, b, cam in fr], "full", None, "", check=False)
    assert not np.array_equal(results[0], plain[0])
