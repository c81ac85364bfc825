"""The neighbourhood clamp of the temporal history (crt_temporal_clamped / crt_temporal_clamped_device, include/crt.h; clamp= of
temporal, temporal_device and Render.run_view_temporal in Python; crt_cli --temporal-clamp).

The contract is restated in numpy float32 in temporal_clamp_restated.py, on top of temporal_restated.restated, which stays the statement
of everything up to the blend.  The device result must match bit for bit: colour, variance, history length, RGB8 and both counts.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import temporal_restated as T
import util
from frames import renders  # noqa: F401
from temporal_clamp_restated import chain, check_against_restatement, neighbourhood_box, restated_clamped
from util import assert_bits

F = np.float32
INF = float("inf")


def settings():
    """(the library's defaults, a tight box): the two settings of the rendered chains"""
    d = crt.temporal_clamp_defaults()
    return [(d["radius"], d["gamma"]), (1, 0.5)]


def check_both_branches(took, clamped, where, least=100):
    free = took & ~clamped
    print("%s: %d histories clamped, %d taken as they are" % (where, clamped.sum(), free.sum()))
    assert clamped.sum() >= least and free.sum() >= least, where


# ------------------------------------------------------------------------------------------------------------------ CPU --

@pytest.mark.parametrize("seed", [21, 22, 23])
def test_restatement_without_a_clamp_or_with_an_infinite_box_is_crt_temporals(seed):
    cur, cam, prev, pcam = T.synthetic(64, 48, seed)
    want = T.restated(cur, cam, prev, pcam)
    assert want[3].sum() >= 100
    for clamp in (None, (1, INF), (2, INF), (3, INF)):
        got = restated_clamped(cur, cam, prev, pcam, clamp=clamp)
        for g, w, what in zip(got[:3], want[:3], ("colour", "variance", "history")):
            assert_bits(g, w, "clamp %r: %s" % (clamp, what))
        assert np.array_equal(got[3], want[3]) and not got[4].any(), clamp
    # ... and the history colour read out of temporal_restated.restated is finite here, so a finite box does clamp it
    assert restated_clamped(cur, cam, prev, pcam, clamp=(1, 1.0))[4].sum() >= 100


def scalar_box(color, x, y, radius, gamma):
    """mu, hi and cnt of one pixel and one channel at a time, in numpy float32 scalars and plain loops: the contract's lines without the
    masks and clipped gathers of neighbourhood_box"""
    H, W = color.shape[:2]
    mu, hi = np.zeros(3, dtype=F), np.zeros(3, dtype=F)
    n = 0
    for ch in range(3):
        s1, s2, cnt = F(0), F(0), F(0)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                if 0 <= y + dy < H and 0 <= x + dx < W:
                    t = color[y + dy, x + dx, ch]
                    s1, s2, cnt = s1 + t, s2 + t * t, cnt + F(1)
        m = s1 / cnt
        e = s2 / cnt - m * m
        e = F(0) if e < 0 else e
        mu[ch], hi[ch], n = m, m + F(gamma) * np.sqrt(e), int(cnt)
    return mu, hi, n


def test_restatement_clamps_a_bright_history_to_the_top_of_the_box():
    """Static camera on a plane, so that every pixel reprojects onto itself; current colour 1 +- a known pattern (at most 0.5), history
    colour 10 and history length 8 everywhere.  8 b is exact, so hn / ws = 8, n = 9, a = 1/9, k = 1 - a in every pixel; the history lies
    above every box (hi <= 1.5 + 0.5), so the output is hi k + c a whatever the rounding of its interpolation -- and mu k + c a with
    gamma 0, where the box is the mean alone and every reprojected pixel counts as clamped."""
    W, H = 16, 12
    cam, depth, _ = T.plane_setup(W, H, (0, 0, 0))
    yy, xx = np.mgrid[0:H, 0:W]
    pattern = ((xx * 5 + yy * 3) % 9 - 4) / 8.0                      # -0.5 .. 0.5, a different slope per channel below
    color = np.stack([1 + pattern, 1 - pattern, 1 + pattern * ((xx + yy) % 2)], axis=-1).astype(F)
    cur = {"color": color, "depth": depth.astype(F)}
    prev = {"color": np.full((H, W, 3), 10, dtype=F), "history": np.full((H, W), 8, dtype=F), "depth": depth.astype(F)}
    a = F(1) / F(9)
    k = F(1) - a
    _, _, _, cnt = neighbourhood_box(color, 1, 1.0)
    assert (cnt[1:-1, 1:-1] == 9).all() and (cnt[0, 1:-1] == 6).all() and (cnt[-1, 1:-1] == 6).all() and (cnt[1:-1, 0] == 6).all()
    assert (cnt[1:-1, -1] == 6).all() and [cnt[0, 0], cnt[0, -1], cnt[-1, 0], cnt[-1, -1]] == [4, 4, 4, 4]
    for gamma in (1.0, 0.0):
        out, var, hist, took, clamped = restated_clamped(cur, cam, prev, cam, clamp=(1, gamma))
        assert var is None and took.all() and (hist == F(9)).all()
        assert np.array_equal(clamped, took)
        for y in range(H):
            for x in range(W):
                mu, hi, n = scalar_box(color, x, y, 1, gamma)
                assert n == (3 if 0 < y < H - 1 else 2) * (3 if 0 < x < W - 1 else 2)
                top = hi if gamma else mu
                want = top * k + color[y, x] * a
                assert np.array_equal(out[y, x].view(np.uint32), want.astype(F).view(np.uint32)), (gamma, x, y, out[y, x], want)
    # a history of 1 lies inside every box of 100 deviations (|mu - 1| <= 0.5, and no 3x3 block of the pattern is flat to 0.005): it is
    # left alone, crt_temporal's bits
    prev["color"] = np.ones((H, W, 3), dtype=F)
    out, _, _, took, clamped = restated_clamped(cur, cam, prev, cam, clamp=(1, 100.0))
    assert took.all() and not clamped.any()
    assert_bits(out, T.restated(cur, cam, prev, cam)[0], "wide box")


def test_clamp_entry_points_and_defaults():
    lib = capi.lib()
    for name in ("crt_temporal_clamp_defaults", "crt_temporal_clamped", "crt_temporal_clamped_device"):
        assert name in capi.EXPORTS and getattr(lib, name)
    c = capi.TemporalClamp()
    C.memset(C.byref(c), 0x7f, C.sizeof(c))
    assert lib.crt_temporal_clamp_defaults(C.byref(c)) == capi.CRT_OK
    assert (c.radius, c.gamma) == (1, 1.0)                 # docs/experiments.md, "The neighbourhood clamp": the sweep's minimum
    assert crt.temporal_clamp_defaults() == {"radius": 1, "gamma": 1.0}
    assert lib.crt_temporal_clamp_defaults(None) == capi.ERR_INVALID_ARG and lib.crt_last_error()
    assert lib.crt_abi_version() == 5
    assert C.sizeof(capi.TemporalClamp) == 8 and C.sizeof(capi.TemporalClampInfo) == 24
    import inspect
    for f in (crt.temporal, crt.temporal_device, crt.Render.run_view_temporal):
        assert inspect.signature(f).parameters["clamp"].default is None
    for bad in (False, 1.0, {"sigma": 1.0}, {"radius": 1.5}):
        with pytest.raises(ValueError):
            crt.temporal({"color": np.zeros((4, 4, 3), F), "depth": np.zeros((4, 4), F)}, (np.zeros(3), np.zeros(9), 1.0), clamp=bad)


def test_clamp_arguments_are_checked_before_any_device_call():
    """Every invalid call of both clamped forms is CRT_ERR_INVALID_ARG, also on a machine without a GPU.  The non-null buffers are
    dummies that must never be dereferenced."""
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

    def frame(**over):
        return C.byref(capi.TemporalFrame(**dict(dict(color=d, variance=d, depth=d, normal=d, id=d), **over)))

    def history(**over):
        return C.byref(capi.TemporalHistory(**dict(dict(color=d, variance=d, history=d, depth=d, normal=d, id=d), **over)))

    def both(prm, cl, cur, prev, color=d, var=d, hist=d, rgb=d, status=capi.ERR_INVALID_ARG, device=0):
        r1 = lib.crt_temporal_clamped(device, prm, cl, cur, prev, color, var, hist, rgb, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_temporal_clamped_device(device, prm, cl, cur, prev, color, var, hist, rgb, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == status, (r1, r2, e1, e2)
        assert e1 and e2
        return e1

    for prev in (history(), None):
        for radius in (0, 4, 2 ** 32 - 1):
            assert b"radius" in both(params(), clamp(radius=radius), frame(), prev), radius
        for gamma in (-1.0, float("nan"), -INF, -1e-30):
            assert b"gamma" in both(params(), clamp(gamma=gamma), frame(), prev), gamma
    # everything crt_temporal refuses, with a valid clamp and with none (a NULL clamp is accepted: the device index is what fails below)
    for cl in (clamp(), clamp(gamma=INF), clamp(gamma=0.0, radius=3), None):
        assert b"null" in both(None, cl, frame(), history())
        assert b"null" in both(params(), cl, None, history())
        for prev in (history(), None):
            both(params(), cl, frame(color=None), prev)
            both(params(), cl, frame(depth=None), prev)
            both(params(), cl, frame(), prev, color=None)
            both(params(), cl, frame(), prev, hist=None)
            both(params(width=0), cl, frame(), prev)
            both(params(height=0), cl, frame(), prev)
            for name in ("depth_tolerance", "normal_tolerance"):
                for bad in (0.0, -1.0, float("nan")):
                    assert b"tolerance" in both(params(**{name: bad}), cl, frame(), prev), (name, bad)
            for bad in (0.0, 1.5, float("nan")):
                assert b"alpha_min" in both(params(alpha_min=bad), cl, frame(), prev), bad
            assert b"variance" in both(params(), cl, frame(variance=None), prev)
            assert b"variance" in both(params(), cl, frame(), prev, var=None)
        for missing in ("color", "history", "depth"):
            assert b"history" in both(params(), cl, frame(), history(**{missing: None})), missing
        assert b"variance" in both(params(), cl, frame(), history(variance=None))
        assert b"normals" in both(params(), cl, frame(normal=None), history())
        assert b"IDs" in both(params(), cl, frame(), history(id=None))
        both(params(width=(1 << 24) + 1), cl, frame(), history(), status=capi.ERR_UNSUPPORTED)
        assert b"device index" in both(params(), cl, frame(), history(), device=-1)
    # the clamp is looked at before the sizes the launch cannot cover
    both(params(width=(1 << 24) + 1), clamp(radius=0), frame(), history())


def test_cli_refuses_a_clamp_without_a_sequence_or_with_a_malformed_value():
    from cudaraytracing_amd import build as b
    cli, cfg = b.build_cli(), util.SCENES["veach-mis"]
    for args in (["--temporal-clamp", "1.0"], ["--temporal-clamp", "1.0,2"], ["--temporal", "2", "--temporal-clamp", "x"],
                 ["--temporal", "2", "--temporal-clamp", "-1"], ["--temporal", "2", "--temporal-clamp", "nan"],
                 ["--temporal", "2", "--temporal-clamp", "1,0"], ["--temporal", "2", "--temporal-clamp", "1,4"],
                 ["--temporal", "2", "--temporal-clamp", "1,2,3"], ["--temporal", "2", "--temporal-clamp", "1,"],
                 ["--temporal", "2", "--temporal-clamp", "1.0x"], ["--temporal", "2", "--temporal-clamp"]):
        bad = subprocess.run([cli, cfg, "--base-dir", util.ROOT] + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "--temporal" in bad.stderr, (args, bad.stderr)
        if len(args) > 1:
            assert "--temporal-clamp" in bad.stderr, (args, bad.stderr)


# ------------------------------------------------------------------------------------------------------------------ GPU --

@pytest.mark.gpu
@pytest.mark.parametrize("setting", [0, 1], ids=["defaults", "radius 1, gamma 0.5"])
@pytest.mark.parametrize("variant", ["full", "no variance"])
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_clamped_rendered_chains_match_restatement(renders, name, variant, setting):
    """Four chained frames of a moving camera (64 x 48, spp 4, seeds 100 .. 103): a clamped output is the next frame's history.  On the
    CPU oracle's frames the last call clamps 404 (cornell-box) / 365 (veach-mis) histories with the defaults (1, 1) and 1221 / 1173 with
    (1, 0.5), and takes 1881 / 2466 and 1064 / 1658 as they are."""
    clamp = settings()[setting]
    where = "%s 64x48 %s clamp %r" % (name, variant, clamp)
    fr = T.frames(renders, name, 64, 48, 8, 100)[:4]       # (the eight frames of the effect tests, here and in test_temporal)
    _, _, _, _, _, took, clamped = chain(fr, variant, clamp, where)
    check_both_branches(took, clamped, where)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,radius", [(130, 9, 3), (61, 47, 2)])
def test_clamped_shapes_that_can_go_wrong(w, h, radius):
    """130 x 9 with radius 3: three 64-wide blocks and three 4-row blocks, the last of each partial, every neighbourhood of the middle
    rows crossing a block seam and those of the outer three rows and columns an image border; 61 x 47 with radius 2: one partial block
    across.  Random colours under a previous camera turned by 8 degrees; three box widths, the two ends included."""
    cur, cam, prev, pcam = T.synthetic(w, h, 31)
    for gamma in (1.0, 0.0, INF):
        where = "synthetic %dx%d radius %d gamma %r" % (w, h, radius, gamma)
        took, clamped = check_against_restatement(cur, cam, prev, pcam, (radius, gamma), where)[5:]
        if gamma == 1.0:
            check_both_branches(took, clamped, where, least=50)
            edge = np.ones((h, w), dtype=bool)
            edge[radius:h - radius, radius:w - radius] = False
            assert (took & edge).sum() >= 50 and (clamped & edge).sum() >= 10, where
        elif gamma == 0.0:
            assert took.sum() - clamped.sum() <= 2         # (a history that IS the mean, to the bit, is not moved)
        else:
            assert not clamped.any()


@pytest.mark.gpu
def test_clamped_non_finite_pixels():
    """NaN and +-inf in the current colour -- at p and inside neighbourhoods, where they make the box NaN (inf - inf) -- and in the
    history colour: both comparisons are false and the interpolated history passes through, bit for bit."""
    cur, cam, prev, pcam = T.synthetic(70, 45, 22)
    cur["color"][7, 9, 1] = np.inf
    cur["color"][30, 50, 0] = np.nan
    cur["color"][22, 12, 2] = -np.inf
    cur["color"][0, 0, 0] = np.nan                           # corners and a border: cnt = 4 and 6
    cur["color"][44, 69, 1] = np.inf
    cur["color"][44, 30, 2] = -np.inf
    prev["color"][12, 33, 2] = np.inf
    prev["color"][25, 20, 0] = np.nan
    prev["color"][26, 40, 1] = -np.inf
    prev["variance"][18, 28, 1] = np.inf
    inf = float("inf")
    planted = ((7, 9, 1), (30, 50, 0), (22, 12, 2))          # (y, x, channel) of the interior ones
    for kw in ({}, {"depth_tolerance": inf, "normal_tolerance": inf}):      # (with the tests off, every planted tap counts)
        plain = T.restated(cur, cam, prev, pcam, **kw)[0]
        for clamp in ((1, 1.0), (3, 0.5), (2, 0.0), (2, INF)):
            where = "non-finite clamp %r %r" % (clamp, kw)
            _, color, var, hist, _, took, clamped = check_against_restatement(cur, cam, prev, pcam, clamp, where, **kw)
            assert np.isnan(color).any() and np.isinf(color).any() and np.isfinite(color).any() and np.isfinite(hist).all()
            # a planted value makes the box of its channel NaN (mean +-inf, inf - inf) in every neighbourhood it lies in: there that
            # channel of the history passes through, the unclamped call's bits, while the clamp works around it
            r = clamp[0]
            for y, x, ch in planted:
                near = np.zeros((45, 70), dtype=bool)
                near[y - r:y + r + 1, x - r:x + r + 1] = True
                near &= took
                assert_bits(color[near][:, ch], plain[near][:, ch], where + ": next to a planted value")
                if kw:
                    assert near.sum() >= 9, where
            if clamp[1] != INF:
                assert clamped.sum() >= 100, where


def raw_clamped(cur, cam, prev, pcam, clamp_ptr):
    """crt_temporal_clamped through ctypes, so that the clamp can be NULL: (rgb, color, variance, history, info)"""
    from cudaraytracing_amd import api
    h, w = cur["color"].shape[:2]
    keep = []
    fc = api._temporal_struct(capi.TemporalFrame(), cur, h, w, keep)
    fp = api._temporal_struct(capi.TemporalHistory(), prev, h, w, keep)
    prm = api._temporal_params(w, h, cam, pcam, None, None, None)
    color, var, hist = np.zeros((h, w, 3), dtype=F), np.zeros((h, w, 3), dtype=F), np.zeros((h, w), dtype=F)
    rgb = np.zeros((h, w, 3), dtype=np.uint8)
    info = capi.TemporalClampInfo()
    capi.check(capi.lib().crt_temporal_clamped(0, C.byref(prm), clamp_ptr, C.byref(fc), C.byref(fp), capi.ptr(color), capi.ptr(var),
                                               capi.ptr(hist), capi.ptr(rgb), C.byref(info)), "crt_temporal_clamped")
    return rgb, color, var, hist, info.as_dict()


@pytest.mark.gpu
def test_clamped_with_an_infinite_box_or_a_null_clamp_is_crt_temporal(renders):
    name, w, h = "veach-mis", 100, 70
    (c0, _, _, cam0), (c1, _, _, cam1) = T.frames(renders, name, w, h, 2, 50)
    prev = T.as_history(c0, c0["color"], c0["variance"], np.full((h, w), 3, dtype=F))
    want = crt.temporal(c1, cam1, prev=prev, prev_camera=cam0, return_info=True)
    assert 100 <= want[4]["reprojected"] < w * h
    for radius in (1, 2, 3):
        inf_box = capi.TemporalClamp(radius, INF)
        got = raw_clamped(c1, cam1, prev, cam0, C.byref(inf_box))
        for g, wnt, what in zip(got[1:4], want[1:4], ("colour", "variance", "history")):
            assert_bits(g, wnt, "infinite box, radius %d: %s" % (radius, what))
        assert np.array_equal(got[0], want[0]) and got[4]["reprojected"] == want[4]["reprojected"] and got[4]["clamped"] == 0
    got = raw_clamped(c1, cam1, prev, cam0, None)
    for g, wnt, what in zip(got[1:4], want[1:4], ("colour", "variance", "history")):
        assert_bits(g, wnt, "null clamp: " + what)
    assert np.array_equal(got[0], want[0]) and got[4]["reprojected"] == want[4]["reprojected"] and got[4]["clamped"] == 0
    # ... and a finite box is something else
    some = crt.temporal(c1, cam1, prev=prev, prev_camera=cam0, return_info=True, clamp=True)
    assert some[4]["clamped"] >= 100 and not np.array_equal(some[1], want[1])


@pytest.mark.gpu
def test_clamped_device_form_on_a_stream_matches_host_form(renders):
    name, w, h = "veach-mis", 100, 70
    (c0, _, _, cam0), (c1, _, _, cam1) = T.frames(renders, name, w, h, 2, 50)
    prev = T.as_history(c0, c0["color"], c0["variance"], np.full((h, w), 3, dtype=F))
    clamp = {"radius": 2, "gamma": 0.75}
    want_rgb, want_c, want_v, want_h, want_info = crt.temporal(c1, cam1, prev=prev, prev_camera=cam0, return_info=True, clamp=clamp)
    assert 100 <= want_info["clamped"] < want_info["reprojected"] - 100
    host = {"cur_" + k: v for k, v in c1.items()}
    host.update({"prev_" + k: v for k, v in prev.items()})
    outs = {"out_color": w * h * 12, "out_var": w * h * 12, "out_hist": w * h * 4, "out_rgb": w * h * 3}
    # (every output value must be written by the kernel: what is not uploaded is filled with 0x55)
    with DeviceBuffers({**host, **outs}, stream=True) as d:
        ptrs = d.ptrs

        def run(want_info, variance=True, out_rgb=True):
            cur_p = {k: ptrs["cur_" + k] for k in c1 if variance or k != "variance"}
            prev_p = {k: ptrs["prev_" + k] for k in prev if variance or k != "variance"}
            return crt.temporal_device(w, h, cam1, cur_p, ptrs["out_color"], ptrs["out_hist"], out_variance_ptr=ptrs["out_var"] if variance else None,
                                       out_rgb_ptr=ptrs["out_rgb"] if out_rgb else None, prev_ptrs=prev_p, prev_camera=cam0, stream=d.stream,
                                       want_info=want_info, clamp=clamp)

        def fetch():
            return (d.download("out_color", (h, w, 3), F), d.download("out_var", (h, w, 3), F), d.download("out_hist", (h, w), F),
                    d.download("out_rgb", (h, w, 3), np.uint8))

        assert run(False) is None
        d.synchronize()
        c, v, hh, r = fetch()
        assert_bits(c, want_c, "device form")
        assert_bits(v, want_v, "device form, variance")
        assert_bits(hh, want_h, "device form, history")
        assert np.array_equal(r, want_rgb)
        # colour and history only, with the timer and the counts (the call synchronizes the stream)
        for n in outs:
            d.fill(n)
        info = run(True, variance=False, out_rgb=False)
        assert info["reprojected"] == want_info["reprojected"] and info["clamped"] == want_info["clamped"] and info["total_ms"] > 0, info
        c, v, hh, r = fetch()
        assert_bits(c, want_c, "device form, colour only")
        assert_bits(hh, want_h, "device form, colour only: history")
        assert (r == 0x55).all() and (v.view(np.uint32) == 0x55555555).all()


@pytest.mark.gpu
def test_run_view_temporal_with_a_clamp_equals_the_calls_by_hand(renders):
    name, w, h = "cornell-box", 64, 48
    r = renders[name]
    fr = T.frames(renders, name, w, h, 3, 40)                # seeds 40, 41, 42: self.seed + the frames since the reset
    r.set_spp(4)
    r.seed = 40
    try:
        for clamp in (True, None):
            r.reset_temporal()
            prev = pcam = None
            for f, (cur, noisy_rgb, g, cam) in enumerate(fr):
                want_rgb, want_c, want_v, want_h, want_info = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, return_info=True, clamp=clamp)
                prev, pcam = T.as_history(cur, want_c, want_v, want_h), cam
                rgb, mean = r.run_view_temporal(*cam, width=w, height=h, clamp=clamp)
                assert_bits(mean, want_c, "run_view_temporal(clamp=%r) frame %d" % (clamp, f))
                assert np.array_equal(rgb, want_rgb)
                assert_bits(r.variance_buffer, want_v, "variance_buffer")
                assert_bits(r.temporal_history_buffer, want_h, "temporal_history_buffer")
                assert r.temporal_info["reprojected"] == want_info["reprojected"]
                assert r.temporal_info.get("clamped") == want_info.get("clamped")
                assert np.array_equal(r.frame_buffer, noisy_rgb)
            if clamp:
                assert r.temporal_info["clamped"] >= 100
                clamped_mean = mean
            else:
                assert "clamped" not in r.temporal_info and not np.array_equal(mean, clamped_mean)
                # today's bits: the chain of plain crt.temporal calls
                plain = chain(fr, "full", None, "", check=False)
                assert_bits(mean, plain[1], "run_view_temporal(clamp=None)")
    finally:
        r.seed = 0
        r.reset_temporal()


@pytest.mark.gpu
def test_cli_accumulates_a_clamped_sequence(renders, tmp_path):
    from PIL import Image
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    name, w, h = "cornell-box", 64, 48
    base = [cli, util.SCENES[name], "--spp", "4", "--width", str(w), "--height", str(h), "--seed", "40", "--base-dir", util.ROOT,
            "--temporal", "3", "--temporal-step", ",".join(repr(float(v)) for v in T.MOVES[name][0])]
    fr = T.frames(renders, name, w, h, 3, 40)
    last = str(tmp_path / "last.png")
    for arg, clamp in (("0.5,2", (2, 0.5)), ("1.5", (crt.temporal_clamp_defaults()["radius"], 1.5))):
        acc = str(tmp_path / ("acc%s.png" % arg))
        res = subprocess.run(base + ["-o", last, "--temporal-out", acc, "--temporal-clamp", arg], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        want = chain(fr, "full", clamp, "", check=False)
        assert np.array_equal(np.asarray(Image.open(acc)), want[0]), arg
        assert np.array_equal(np.asarray(Image.open(last)), fr[-1][1])
        assert "histories clamped" in res.stdout
    assert not np.array_equal(want[0], chain(fr, "full", None, "", check=False)[0])


@pytest.mark.gpu
def test_clamp_defaults_lower_the_error_of_a_moving_camera_on_veach_mis(renders):
    """64 x 48, spp 4, 8 frames with seeds 100 .. 107, camera moving by (0, 0.1, 0.3) per frame; R = spp 256, seed 7 at the last camera;
    mse on the RGB8 tone maps.  The restatements on the CPU oracle's frames (the device's, bit for bit) measured 367.9 without the clamp
    and 339.3 with the defaults (radius 1, gamma 1); the direction is what is pinned."""
    name = "veach-mis"
    fr = T.frames(renders, name, 64, 48, 8, 100)
    plain = chain(fr, "full", None, "", check=False)
    d = crt.temporal_clamp_defaults()
    clamped = chain(fr, "full", (d["radius"], d["gamma"]), "", check=False)
    r = renders[name]
    r.set_spp(256)
    r.seed = 7
    try:
        ref_rgb = r.run_view(*fr[-1][3], width=64, height=48).copy()
    finally:
        r.seed = 0

    def mse(x):
        e = x.astype(np.float64) - ref_rgb.astype(np.float64)
        return float(np.mean(e * e))

    print("%s moving: mse accumulated %.1f, with the clamp's defaults %.1f" % (name, mse(plain[0]), mse(clamped[0])))
    assert mse(clamped[0]) < mse(plain[0])
