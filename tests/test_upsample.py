"""Guide-driven upsampling (crt_upsample / crt_upsample_device, include/crt.h; upsample, upsample_device and
Render.run_view_upsampled in Python; crt_cli --upsample).

The contract of include/crt.h is restated below in numpy float32, one ufunc per operation, with the oracle's det_expf
(oracle_lib.math_fn("exp")) and tone map (oracle_lib.tonemap); the device result must match it bit for bit (uint32 views; where the
expected value is NaN the result must be NaN).
"""
import ctypes as C
import subprocess
import types

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import oracle_lib as O
import util
from frames import GUIDES, cached_frame, renders  # noqa: F401

F = np.float32
UPSAMPLE_EXPORTS = ("crt_upsample_defaults", "crt_upsample", "crt_upsample_device")
DEFAULTS = {"radius": 1, "min_weight": 1.0 / 64, "sigma_normal": 0.5, "sigma_albedo": 0.1, "sigma_depth": 0.05}
assert_bits = util.assert_bits


def restated(low, width, height, guides=None, radius=1, min_weight=1.0 / 64, sigma_normal=0.5, sigma_albedo=0.1, sigma_depth=0.05):
    """The contract: (color, variance or None, guided (height, width) bool).  Every ufunc is one IEEE fp32 operation per element."""
    c = np.ascontiguousarray(low["color"], dtype=F)
    var = low.get("variance")
    lh, lw = c.shape[:2]
    g = guides if guides is not None else {}
    use = {k: g.get(k) is not None for k in GUIDES}
    for k in GUIDES:
        assert guides is None or use[k] == (low.get(k) is not None), k
    sn, sa, sd, fr = F(sigma_normal), F(sigma_albedo), F(sigma_depth), F(radius)
    zero = np.zeros((height, width), dtype=F)

    def sq3(p, q):
        d = p - q
        return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]

    with np.errstate(all="ignore"):
        sx, sy = F(lw) / F(width), F(lh) / F(height)
        u = (np.arange(width, dtype=F) + F(0.5)) * sx - F(0.5)
        v = (np.arange(height, dtype=F) + F(0.5)) * sy - F(0.5)
        assert u.dtype == F and v.dtype == F
        x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
        num, snum = np.zeros((height, width, 3), dtype=F), np.zeros((height, width, 3), dtype=F)
        vnum, svnum = np.zeros((height, width, 3), dtype=F), np.zeros((height, width, 3), dtype=F)
        den, sden = zero.copy(), zero.copy()
        taps_inside = np.zeros((height, width), dtype=np.int64)
        for j in range(-radius + 1, radius + 1):
            ty = y0 + j
            vy = (ty >= 0) & (ty < lh)
            ys = np.clip(ty, 0, lh - 1)
            wy = F(1.0) - np.abs(v - ty.astype(F)) / fr
            for i in range(-radius + 1, radius + 1):
                tx = x0 + i
                vx = (tx >= 0) & (tx < lw)
                xs = np.clip(tx, 0, lw - 1)
                wx = F(1.0) - np.abs(u - tx.astype(F)) / fr
                valid = vy[:, None] & vx[None, :]
                hw = wy[:, None] * wx[None, :]
                e_n = sq3(g["normal"], low["normal"][ys][:, xs]) / (sn * sn) if use["normal"] else zero
                e_a = sq3(g["albedo"], low["albedo"][ys][:, xs]) / (sa * sa) if use["albedo"] else zero
                if use["depth"]:
                    pd, qd = g["depth"], low["depth"][ys][:, xs]
                    m = np.where(pd > qd, pd, qd)
                    r = (pd - qd) / (sd * m)
                    e_d = np.where(m > 0, r * r, F(0.0))
                else:
                    e_d = zero
                w = hw * O.math_fn("exp", -((e_n + e_a) + e_d))
                assert w.dtype == F and hw.dtype == F
                cq = c[ys][:, xs]
                num = np.where(valid[..., None], num + cq * w[..., None], num)
                den = np.where(valid, den + w, den)
                snum = np.where(valid[..., None], snum + cq * hw[..., None], snum)
                sden = np.where(valid, sden + hw, sden)
                if var is not None:
                    vq = var[ys][:, xs]
                    vnum = np.where(valid[..., None], vnum + vq * (w * w)[..., None], vnum)
                    svnum = np.where(valid[..., None], svnum + vq * (hw * hw)[..., None], svnum)
                taps_inside += valid
        assert (taps_inside >= 1).all()
        guided = den > F(min_weight) * sden
        out = np.where(guided[..., None], num / den[..., None], snum / sden[..., None])
        out_var = None
        if var is not None:
            out_var = np.where(guided[..., None], vnum / (den * den)[..., None], svnum / (sden * sden)[..., None])
    assert out.dtype == F
    return out, out_var, guided


def check(low, width, height, guides, where, **settings):
    """crt.upsample against the restatement: colour, variance, RGB and the count; returns (rgb, color, variance, info, guided)"""
    want_c, want_v, guided = restated(low, width, height, guides, **settings)
    got = crt.upsample(low, width, height, guides=guides, return_info=True, **settings)
    rgb, color, info = got[0], got[1], got[-1]
    assert_bits(color, want_c, where + " colour")
    var = None
    if want_v is not None:
        var = got[2]
        assert_bits(var, want_v, where + " variance")
    else:
        assert len(got) == 3
    assert np.array_equal(rgb, O.tonemap(want_c)), where + " rgb"
    assert info["fallback_pixels"] == int((~guided).sum()), (where, info, int((~guided).sum()))
    return rgb, color, var, info, guided


def synthetic(w, h, seed, special=True):
    """colour, variance, albedo, normal (h, w, 3) and depth (h, w) of a w x h image, with every special value the contract lets through
    sprinkled into every buffer"""
    rng = np.random.default_rng(seed)
    n = h * w
    out = {"color": (rng.random(n * 3) * 40).astype(F), "variance": (rng.random(n * 3) * 3).astype(F),
           "albedo": (rng.random(n * 3) * 0.2 + 0.4).astype(F), "normal": (rng.random(n * 3) * 0.4).astype(F),
           "depth": (rng.random(n) * 0.3 + 5).astype(F)}
    values = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e30, 1e-30, -0.5], dtype=F)
    if special:
        for k, a in enumerate(out.values()):
            idx = rng.permutation(a.size)[:min(max(values.size, a.size // 12), a.size // 3)]  # (a 1 x 1 image keeps finite values)
            a[idx] = values[(np.arange(idx.size) + k) % values.size]
    return {k: a.reshape((h, w, 3) if a.size == n * 3 else (h, w)) for k, a in out.items()}


def two_sizes(w, h, lw, lh, seed, special=True):
    """(low dict with colour, variance and guides at lw x lh; guides dict at w x h)"""
    low, full = synthetic(lw, lh, seed, special), synthetic(w, h, seed + 1, special)
    return low, {k: full[k] for k in GUIDES}


def without(d, names):
    return {k: a for k, a in d.items() if k not in names}


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_upsample_entry_points_are_exported():
    lib = capi.lib()
    for name in UPSAMPLE_EXPORTS:
        assert name in capi.EXPORTS
        getattr(lib, name)
    lib.crt_abi_version.restype = C.c_int
    assert lib.crt_abi_version() == 5 == capi.ABI_VERSION
    for name in ("upsample", "upsample_device", "upsample_defaults"):
        assert hasattr(crt, name) and name in crt.__all__
    assert hasattr(crt.Render, "run_view_upsampled")


def test_upsample_defaults():
    lib = capi.lib()
    p = capi.UpsampleParams(7, 7, 7, 7, 7, -1.0, -1.0, -1.0, -1.0)
    assert lib.crt_upsample_defaults(C.byref(p)) == capi.CRT_OK
    assert (p.width, p.height, p.low_width, p.low_height) == (0, 0, 0, 0) and p.radius == 1
    for name in ("min_weight", "sigma_normal", "sigma_albedo", "sigma_depth"):
        assert F(getattr(p, name)) == F(DEFAULTS[name]), name
    d = crt.upsample_defaults()
    assert set(d) == set(DEFAULTS) and all(F(d[k]) == F(DEFAULTS[k]) for k in DEFAULTS)
    assert lib.crt_upsample_defaults(None) == capi.ERR_INVALID_ARG and lib.crt_last_error()


def test_upsample_arguments_are_checked_before_any_device_call():
    """Every refusal of the contract is CRT_ERR_INVALID_ARG from both forms, also on a machine without a GPU: the arguments are checked
    first (the pointers here are host memory that a device call would fault on)."""
    lib = capi.lib()
    buf = np.zeros(8 * 6 * 3, dtype=F)
    d = buf.ctypes.data

    def params(**over):
        p = capi.UpsampleParams()
        assert lib.crt_upsample_defaults(C.byref(p)) == capi.CRT_OK
        p.width, p.height, p.low_width, p.low_height = 8, 6, 4, 3
        for k, v in over.items():
            setattr(p, k, v)
        return C.byref(p)

    def low(**over):
        s = capi.UpsampleLow(d, d, d, d, d)
        for k, v in over.items():
            setattr(s, k, v)
        return C.byref(s)

    def guides(**over):
        s = capi.UpsampleGuides(d, d, d)
        for k, v in over.items():
            setattr(s, k, v)
        return C.byref(s)

    def both(prm, lo, gd, color=d, var=d, rgb=d):
        r1 = lib.crt_upsample(0, prm, lo, gd, color, var, rgb, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_upsample_device(0, prm, lo, gd, color, var, rgb, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == capi.ERR_INVALID_ARG, (r1, r2, e1, e2)
        assert e1.startswith(b"crt_upsample: ") and e2.startswith(b"crt_upsample_device: ") and e1[len("crt_upsample: "):] == e2[len("crt_upsample_device: "):]
        return e1

    assert b"null" in both(None, low(), guides())
    assert b"null" in both(params(), None, guides())
    assert b"null" in both(params(), low(color=None), guides())
    for side in ("width", "height", "low_width", "low_height"):
        assert b"positive" in both(params(**{side: 0}), low(), guides())
    assert b"larger" in both(params(low_width=9), low(), guides())
    assert b"larger" in both(params(low_height=7), low(), guides())
    for radius in (0, 5, 2 ** 32 - 1):
        assert b"radius" in both(params(radius=radius), low(), guides())
    for mw in (-0.25, float("nan"), float("inf"), float("-inf")):
        assert b"min_weight" in both(params(min_weight=mw), low(), guides())
    for name in ("sigma_normal", "sigma_albedo", "sigma_depth"):
        for bad in (0.0, -1.0, float("nan")):
            assert b"sigma" in both(params(**{name: bad}), low(), guides())
    for name in GUIDES:  # one of a pair without the other, either way
        assert b"both resolutions" in both(params(), low(**{name: None}), guides())
        assert b"both resolutions" in both(params(), low(), guides(**{name: None}))
    assert b"together" in both(params(), low(variance=None), guides())
    assert b"together" in both(params(), low(), guides(), var=None)
    assert b"no output" in both(params(), low(), guides(), color=None, rgb=None)
    # the order: the first fault decides the message
    assert b"positive" in both(params(width=0, radius=9), low(), guides())
    assert b"radius" in both(params(radius=9, min_weight=-1.0), low(), guides(), color=None, rgb=None)
    # a negative device index, after the argument checks
    assert lib.crt_upsample(-1, params(), low(), guides(), d, d, d, None) == capi.ERR_INVALID_ARG and b"device" in lib.crt_last_error()
    assert lib.crt_upsample_device(-1, params(), low(), guides(), d, d, d, None, None) == capi.ERR_INVALID_ARG and b"device" in lib.crt_last_error()
    # an image the launch cannot cover
    for prm in (params(width=2 ** 24 + 1), params(width=2 ** 24, height=2 ** 24)):
        assert lib.crt_upsample(0, prm, low(), guides(), d, d, d, None) == capi.ERR_UNSUPPORTED
        assert lib.crt_upsample_device(0, prm, low(), guides(), d, d, d, None, None) == capi.ERR_UNSUPPORTED


def test_python_validates_shapes_and_names():
    low, guides = two_sizes(8, 6, 4, 3, 1, special=False)
    with pytest.raises(ValueError):
        crt.upsample({"color": np.zeros((3, 4), dtype=F)}, 8, 6)
    with pytest.raises(ValueError):
        crt.upsample(without(low, ("color",)), 8, 6)
    with pytest.raises(ValueError):
        crt.upsample(dict(low, albedo=np.zeros((3, 5, 3), dtype=F)), 8, 6, guides=guides)
    with pytest.raises(ValueError):
        crt.upsample(low, 8, 6, guides=dict(guides, depth=np.zeros((3, 4), dtype=F)))
    with pytest.raises(ValueError):
        crt.upsample(dict(low, history=low["depth"]), 8, 6)
    with pytest.raises(ValueError):
        crt.upsample(low, 8, 6, guides=dict(guides, color=guides["albedo"]))
    with pytest.raises(ValueError):
        crt.upsample(low, 8, 6, guides=guides, sigma_color=1.0)
    with pytest.raises(ValueError):
        crt.upsample(low, 8, 6, guides=guides, radius=1.5)


def test_run_view_upsampled_refuses_a_size_the_factor_does_not_divide():
    """before anything is rendered: no handle is looked at"""
    stub = types.SimpleNamespace(scene=types.SimpleNamespace(width=64, height=48))
    eye, iv, fov = (0, 0, 0), np.eye(3, dtype=F), 0.5
    for kw in (dict(factor=5), dict(factor=3, width=66, height=50), dict(factor=2, width=63, height=48), dict(factor=4, width=64, height=50)):
        with pytest.raises(ValueError, match="divisible"):
            crt.Render.run_view_upsampled(stub, eye, iv, fov, **kw)
    for factor in (1, 9, 2.5):
        with pytest.raises(ValueError, match="factor"):
            crt.Render.run_view_upsampled(stub, eye, iv, fov, factor=factor)


def test_multi_render_refuses_upsampling():
    with pytest.raises(NotImplementedError):
        crt.MultiRender.run_view_upsampled(None)


def test_restated_identity_and_tent():
    """What the restatement itself promises, without a device: equal sizes, radius 1 and no guides give the input's bits (w = hw = 1 for
    the centre tap and 0 for the other), and every pixel has a tap inside the low image (restated asserts it) at the sizes the device
    tests use."""
    rng = np.random.default_rng(3)
    c = (rng.random((9, 13, 3)) * 40 + 0.5).astype(F)
    out, _, guided = restated({"color": c}, 13, 9)
    assert_bits(out, c, "identity")
    assert guided.all()
    for w, h, lw, lh, radius in SIZES:
        low, guides = two_sizes(w, h, lw, lh, 0, special=False)
        out, var, guided = restated(low, w, h, guides, radius=radius)
        assert np.isfinite(out).all() and np.isfinite(var).all() and out.shape == (h, w, 3) and guided.shape == (h, w)


SIZES = [(61, 47, 31, 24, 1), (130, 9, 33, 3, 2), (65, 5, 17, 2, 4), (7, 5, 1, 1, 3)]
DROPS = [(), ("albedo",), ("normal",), ("depth",), GUIDES]


# ------------------------------------------------------------------------------------------------------------------ GPU --

def frame_of(renders, name, width, height, spp, seed=0, variance=True):
    """A GPU render (with its variance) and the shading pass with the guides from the same trace, rendered once"""
    return cached_frame(renders, name, width, height, spp, seed=seed, render=variance, want_variance=variance, shading=GUIDES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_rendered_frames_match_restatement(renders, name):
    """64 x 48 from 32 x 24, spp 4, all guides, all outputs: the radiance itself and its variance"""
    lo, hi = frame_of(renders, name, 32, 24, 4), frame_of(renders, name, 64, 48, 4, variance=False)
    low = dict({k: lo[k] for k in GUIDES}, color=lo["mean"], variance=lo["variance"])
    guides = {k: hi[k] for k in GUIDES}
    _, color, _, info, guided = check(low, 64, 48, guides, name)
    assert guided.any() and np.isfinite(color).all()
    check(low, 64, 48, guides, name + " radius 2", radius=2)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d<-%dx%d r%d" % s for s in SIZES])
@pytest.mark.parametrize("drop", DROPS, ids=["all guides", "no albedo", "no normal", "no depth", "no guides"])
def test_synthetic_inputs_match_restatement(size, drop):
    """a ratio that is no integer with ragged blocks; a low image shorter than the tap window and three waves per row; one pixel in a
    second wave; a single tap.  NaN, +-inf, -0, 1e30, 1e-30 and negative values in every buffer."""
    w, h, lw, lh, radius = size
    low, guides = two_sizes(w, h, lw, lh, w * h + radius)
    for group in (low, guides):
        every = np.concatenate([a.reshape(-1) for a in group.values()])
        assert np.isnan(every).any() and np.isinf(every).any()
    where = "%dx%d<-%dx%d r%d without %r" % (w, h, lw, lh, radius, drop)
    if drop == GUIDES:
        _, color, var, _, guided = check(low, w, h, None, where, radius=radius)
        # guides == NULL: the tent interpolation, whatever `low` holds
        tent_c, tent_v, _ = restated(without(low, GUIDES), w, h, None, radius=radius)
        assert_bits(color, tent_c, where + " tent")
        assert_bits(var, tent_v, where + " tent variance")
    else:
        check(without(low, drop), w, h, without(guides, drop), where, radius=radius)
    # without a variance, and one output at a time
    lo2, g2 = without(low, drop + ("variance",)), (without(guides, drop) if drop != GUIDES else None)
    want = restated(lo2, w, h, g2, radius=radius)[0]
    rgb, color = crt.upsample(lo2, w, h, guides=g2, radius=radius)
    assert_bits(color, want, where + " no variance")
    assert np.array_equal(rgb, O.tonemap(want))
    assert crt.upsample(lo2, w, h, guides=g2, radius=radius, want_rgb=False)[0] is None


@pytest.mark.gpu
def test_equal_sizes_without_guides_are_the_identity():
    rng = np.random.default_rng(3)
    c = (rng.random((9, 13, 3)) * 40 + 0.5).astype(F)
    v = (rng.random((9, 13, 3)) * 3).astype(F)
    rgb, color, var, info = crt.upsample({"color": c, "variance": v}, 13, 9, return_info=True)
    assert_bits(color, c, "identity")
    assert_bits(var, v, "identity variance")
    assert np.array_equal(rgb, O.tonemap(c)) and info["fallback_pixels"] == 0


def surfaces(w, h, edge, column=None):
    """The full-resolution truth of two surfaces that meet at column `edge` -- left: colour 1, normal (1, 0, 0), albedo 0.2, depth 10;
    right: colour 5, normal (0, 0, 1), albedo 0.7, depth 14 -- and, `column`, a one-pixel-wide strip unlike both"""
    right = (np.arange(w) >= edge)[None, :, None] & np.ones((h, 1, 1), dtype=bool)
    out = {"color": np.where(right, F(5), F(1)) * np.ones((h, w, 3), dtype=F),
           "normal": np.where(right, np.array([0, 0, 1], dtype=F), np.array([1, 0, 0], dtype=F)) * np.ones((h, w, 3), dtype=F),
           "albedo": np.where(right, F(0.7), F(0.2)) * np.ones((h, w, 3), dtype=F),
           "depth": np.where(right[..., 0], F(14), F(10)) * np.ones((h, w), dtype=F)}
    if column is not None:
        out["color"][:, column] = 9
        out["normal"][:, column] = (0, 1, 0)
        out["albedo"][:, column] = 0.95
        out["depth"][:, column] = 30
    return {k: a.astype(F) for k, a in out.items()}


def cell_means(full, f):
    """the low-resolution buffers: the mean of every f x f cell"""
    out = {}
    for k, a in full.items():
        h, w = a.shape[:2]
        b = a.astype(np.float64).reshape((h // f, f, w // f, f) + a.shape[2:])
        out[k] = b.mean(axis=(1, 3)).astype(F)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("edge,factor,radius", [(32, 2, 1), (33, 2, 1), (32, 4, 2)])
def test_guides_keep_an_edge_that_interpolation_smears(edge, factor, radius):
    """With the guides every output pixel takes its colour from low-resolution pixels of its own surface: the error against the
    full-resolution truth is at most 1e-5 (the restatement gives 0.0: the weight of a tap across the edge underflows against one
    on the pixel's side).  The tent interpolation alone is off by 0.9 or more next to the edge (the restatement gives 1.0 and more).
    Edge 33 lies inside a low-resolution cell of factor 2, whose mean belongs to neither surface.  (At factor 4 a cell that is three
    quarters one surface is not rejected outright by the default sigmas -- the restatement leaves 1.6e-3 there: no case of this test.)"""
    w, h = 64, 48
    truth = surfaces(w, h, edge)
    low = cell_means(truth, factor)
    guides = {k: truth[k] for k in GUIDES}
    _, color, _, info, _ = check(low, w, h, guides, "edge %d" % edge, radius=radius)
    err = float(np.abs(color - truth["color"]).max())
    _, plain = crt.upsample(without(low, GUIDES), w, h, radius=radius)
    err_plain = float(np.abs(plain - truth["color"]).max())
    print("edge at %d, factor %d, radius %d: max error %g with guides, %g without; %d fallback pixels" % (edge, factor, radius, err, err_plain, info["fallback_pixels"]))
    assert err <= 1e-5
    assert err_plain >= 0.9
    assert info["fallback_pixels"] == 0


@pytest.mark.gpu
def test_a_feature_thinner_than_a_low_pixel_falls_back():
    """A one-pixel-wide column (x = 21) whose normal, albedo and depth are unlike everything around it: no low-resolution pixel agrees
    with it, so exactly its 48 pixels are counted and get the tent interpolation's bits; every other pixel is within 1e-5 of the truth."""
    w, h, col = 64, 48, 21
    truth = surfaces(w, h, 32, column=col)
    low = cell_means(truth, 2)
    guides = {k: truth[k] for k in GUIDES}
    _, color, _, info, guided = check(low, w, h, guides, "column")
    assert info["fallback_pixels"] == h
    assert (~guided[:, col]).all() and guided[:, :col].all() and guided[:, col + 1:].all()
    tent = restated(without(low, GUIDES), w, h)[0]
    assert_bits(color[:, col], tent[:, col], "the column")
    others = np.arange(w) != col
    err = float(np.abs(color[:, others] - truth["color"][:, others]).max())
    print("max error off the column: %g" % err)
    assert err <= 1e-5
    # min_weight 0: a pixel falls back only when its guided weight is 0 or NaN (here it is: every exponent is below -87)
    _, _, _, info0, guided0 = check(low, w, h, guides, "column, min_weight 0", min_weight=0.0)
    assert info0["fallback_pixels"] == int((~guided0).sum())


@pytest.mark.gpu
def test_device_form_on_a_stream():
    """Everything in device memory on a non-default stream: the host form's bits; without an info nothing synchronizes; one output at
    a time; nothing is written past an output's end."""
    w, h, lw, lh = 61, 47, 31, 24
    low, guides = two_sizes(w, h, lw, lh, 9)
    want_rgb, want_c, want_v, want_info = crt.upsample(low, w, h, guides=guides, radius=2, return_info=True)
    low_table = {"color": (3, F), "variance": (3, F), "albedo": (3, F), "normal": (3, F), "depth": (1, F)}
    # (rgb: 3 bytes per pixel in a buffer of 12: what lies behind them must stay as it was)
    full_table = {"albedo": (3, F), "normal": (3, F), "depth": (1, F), "out_color": (3, F), "out_variance": (3, F), "out_rgb": (3, np.uint32)}
    with DeviceBuffers.image(low_table, lw, lh) as dl, DeviceBuffers.image(full_table, w, h) as dh:
        for d, src in ((dl, low), (dh, guides)):
            for k, a in src.items():
                d.upload(k, a)
        guide_ptrs = {k: dh.ptrs[k] for k in GUIDES}

        def run(want_info, color=True, variance=True, rgb=True):
            for k in ("out_color", "out_variance", "out_rgb"):
                dh.fill(k, 0x55)
            lp = dict(dl.ptrs) if variance else without(dl.ptrs, ("variance",))
            info = crt.upsample_device(w, h, lw, lh, lp, dh.ptrs["out_color"] if color else None, out_variance_ptr=dh.ptrs["out_variance"] if variance else None,
                                       out_rgb_ptr=dh.ptrs["out_rgb"] if rgb else None, guide_ptrs=guide_ptrs, stream=dh.stream, want_info=want_info, radius=2)
            if not want_info:
                assert info is None
                dh.synchronize()
            got = dh.fetch(("out_color", "out_variance", "out_rgb"))
            raw = got["out_rgb"].view(np.uint8).reshape(-1)
            assert (raw[w * h * 3:] == 0x55).all()
            return info, got["out_color"], got["out_variance"], raw[:w * h * 3].reshape(h, w, 3)

        untouched = np.full((h, w, 3), 0x55555555, dtype=np.uint32)
        _, c, v, rgb = run(False)
        assert_bits(c, want_c, "device colour")
        assert_bits(v, want_v, "device variance")
        assert np.array_equal(rgb, want_rgb)
        info, c, v, rgb = run(True, variance=False, rgb=False)
        assert info["total_ms"] > 0 and info["fallback_pixels"] == want_info["fallback_pixels"]
        assert_bits(c, want_c, "colour alone")
        assert np.array_equal(v.view(np.uint32), untouched) and (rgb == 0x55).all()
        _, c, v, rgb = run(False, color=False, variance=False)
        assert np.array_equal(rgb, want_rgb)
        assert np.array_equal(c.view(np.uint32), untouched) and np.array_equal(v.view(np.uint32), untouched)
        # no guides: the tent interpolation
        for k in ("out_color", "out_variance", "out_rgb"):
            dh.fill(k, 0x55)
        assert crt.upsample_device(w, h, lw, lh, dl.ptrs, dh.ptrs["out_color"], out_variance_ptr=dh.ptrs["out_variance"], stream=dh.stream, want_info=False) is None
        dh.synchronize()
        tent_c, tent_v, _ = restated(without(low, GUIDES), w, h)
        got = dh.fetch(("out_color", "out_variance"))
        assert_bits(got["out_color"], tent_c, "device tent")
        assert_bits(got["out_variance"], tent_v, "device tent variance")
        with pytest.raises(ValueError):
            crt.upsample_device(w, h, lw, lh, {"colour": dl.ptrs["color"]}, dh.ptrs["out_color"])


# ---- the chain ----

@pytest.mark.gpu
@pytest.mark.parametrize("demodulate,filter_low", [(True, False), (False, False), (True, True)], ids=["demodulated", "radiance", "filtered low frame"])
def test_run_view_upsampled_equals_the_calls_by_hand(renders, demodulate, filter_low):
    name, w, h, f = "cornell-box", 64, 48, 2
    r = renders[name]
    lo, hi = frame_of(renders, name, w // f, h // f, 4), frame_of(renders, name, w, h, 1, variance=False)  # the guides with 1 sample
    color, var = lo["mean"], lo["variance"]
    if demodulate:
        color, var = crt.demodulate(color, lo["diffuse_albedo"], lo["emission"], variance=var)
    low_guides = {k: lo[k] for k in GUIDES}
    if filter_low:
        color = crt.denoise_var(color, var, want_rgb=False, **low_guides)[1]
    want_rgb, want_mean, want_var, want_info = crt.upsample(dict(low_guides, color=color, variance=var), w, h, guides={k: hi[k] for k in GUIDES}, return_info=True)
    if demodulate:
        want_rgb, want_mean = crt.modulate(want_mean, hi["diffuse_albedo"], hi["emission"])
    r.set_spp(4)
    rgb, mean = r.run_view_upsampled(*util.camera(name), factor=f, width=w, height=h, guide_spp=1, demodulate=demodulate, filter_low=filter_low)
    assert r.spp == 4
    assert_bits(mean, want_mean, "run_view_upsampled")
    assert np.array_equal(rgb, want_rgb)
    assert_bits(r.upsampled_variance, want_var, "upsampled_variance")
    assert r.upsample_info["fallback_pixels"] == want_info["fallback_pixels"] and r.upsample_info["total_ms"] > 0
    assert np.array_equal(r.low_frame["rgb"], lo["rgb"])
    for k in ("mean", "variance", "emission", "diffuse_albedo") + GUIDES:
        assert_bits(r.low_frame[k], lo[k], "low_frame " + k)
    for k in GUIDES:
        assert_bits(r.aov_buffers[k], hi[k], k)
    for k in ("emission", "diffuse_albedo"):
        assert_bits(r.shading_buffers[k], hi[k], k)
    # the settings reach the operation, and the sample count comes back when the call fails
    rgb2, _ = r.run_view_upsampled(*util.camera(name), factor=f, width=w, height=h, guide_spp=1, demodulate=demodulate, filter_low=filter_low,
                                   sigma_albedo=float("inf"), radius=2)
    assert not np.array_equal(rgb2, rgb)
    with pytest.raises(capi.CrtError):
        r.run_view_upsampled(*util.camera(name), factor=f, width=w, height=h, guide_spp=1, radius=7)
    assert r.spp == 4
    with pytest.raises(ValueError):
        r.run_view_upsampled(*util.camera(name), factor=f, width=w, height=h, guide_spp=1, sigma_color=1.0)


@pytest.mark.gpu
def test_cli_writes_the_upsampled_frame(renders, tmp_path):
    from PIL import Image
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    name = "cornell-box"
    base = [cli, util.SCENES[name], "--spp", "4", "--width", "64", "--height", "48", "--seed", "42", "--base-dir", util.ROOT]
    plain, noisy, up, up2 = (str(tmp_path / n) for n in ("plain.png", "noisy.png", "up.png", "up2.png"))
    res = subprocess.run(base + ["-o", plain], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    res = subprocess.run(base + ["-o", noisy, "--upsample", "2", "--upsample-out", up], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert "upsample: factor 2, radius 1" in res.stdout
    assert open(plain, "rb").read() == open(noisy, "rb").read()  # -o stays the plain frame at full size
    r = renders[name]
    r.set_spp(4)
    r.seed = 42
    try:
        want, _ = r.run_view_upsampled(*util.camera(name), factor=2, width=64, height=48)
        want2, _ = r.run_view_upsampled(*util.camera(name), factor=4, width=64, height=48, radius=2, guide_spp=1)
    finally:
        r.seed = 0
    assert np.array_equal(np.asarray(Image.open(up)), want)
    res = subprocess.run(base + ["-o", noisy, "--upsample", "4,2", "--upsample-out", up2, "--upsample-guide-spp", "1"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert np.array_equal(np.asarray(Image.open(up2)), want2)
    for bad_args in (["--devices", "0,0", "--gather", "copy", "--upsample", "2", "--upsample-out", up], ["--upsample", "5", "--upsample-out", up],
                     ["--upsample", "2"], ["--upsample", "9", "--upsample-out", up], ["--upsample", "2,5", "--upsample-out", up], ["--upsample-out", up]):
        bad = subprocess.run(base + bad_args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "--upsample" in bad.stderr, (bad_args, bad.stderr)


@pytest.mark.gpu
def test_multi_render_has_no_upsampling():
    m = crt.MultiRender(util.host_scene("cornell-box"), 2, devices=(0,), gather=crt.GATHER_COPY)
    try:
        eye, iv, fov = util.camera("cornell-box")
        with pytest.raises(NotImplementedError):
            m.run_view_upsampled(eye, iv, fov)
    finally:
        m.free()
