"""Pixel reconstruction filters -- crt_set_pixel_filter, CRT_FLAG_PIXEL_FILTER, crt_filtered_frame (include/crt.h) -- against the numpy
float32 restatement of tests/pixel_filter_restated.py on the oracle's per-path radiance, bit for bit; the kernel text on the host
(tools/pixel_filter_host_check.cpp) against the same restatement under the sanitizers; Render.set_pixel_filter / filtered in Python,
crt_cli --pixel-filter.  Comparisons are on uint32 views (NaN matches NaN) or on the RGB bytes."""
import ctypes as C
import inspect
import os
import struct
import subprocess

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import host_program as HP
import oracle_lib as O
import pixel_filter_restated as PF
import util
from frames import oracle_frame, renders  # noqa: F401
from util import assert_bits, restated_sums

F = np.float32
SCENES = ["cornell-box", "veach-mis"]
EXPORTS = ("crt_pixel_filter_defaults", "crt_set_pixel_filter", "crt_filtered_frame", "crt_filtered_frame_device")
# the filters of the issue: (kind, radius); reach 0, 1, 1, 1, 2, 2
FILTERS = [("box", 0.5), ("box", 1.5), ("tent", 1.0), ("tent", 1.5), ("tent", 2.0), ("mitchell", 2.0)]
SIZES = [(61, 47, 7), (13, 9, 3), (5, 3, 2)]          # ragged tiles / two ragged tile columns, reach 2 across tile corners / one partial tile
BIG_SEED = (5 << 32) | 9                              # the draw's c.w word is not 0
U = 2.0 ** -24


def spec(kind, radius):
    return dict(kind=kind, radius=radius)


_restated = {}


def restated(name, w, h, S, n, kind, radius, seed):
    """(mean, rgb) of the restatement, computed once per set of arguments"""
    key = (name, w, h, S, n, kind, radius, seed)
    if key not in _restated:
        _restated[key] = PF.filtered(oracle_frame(name, w, h, S, seed)[2], S, n, PF.KINDS[kind], radius, seed)
    return _restated[key]


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_entry_points_flag_and_abi_version_are_exported():
    lib = capi.lib()
    for name in EXPORTS:
        assert name in capi.EXPORTS and getattr(lib, name)
    lib.crt_abi_version.restype = C.c_int
    assert lib.crt_abi_version() == 5 == capi.ABI_VERSION
    assert capi.FLAG_PIXEL_FILTER == 128 == crt.FLAG_PIXEL_FILTER
    assert (capi.PIXEL_FILTER_BOX, capi.PIXEL_FILTER_TENT, capi.PIXEL_FILTER_MITCHELL) == (0, 1, 2)
    assert crt.pixel_filter_defaults() == {"kind": "tent", "radius": 1.0}
    for name in ("set_pixel_filter", "filtered"):
        assert hasattr(crt.Render, name)
    assert "pixel_filter" in inspect.signature(crt.Render.run_view).parameters
    assert "pixel_filter" in inspect.signature(crt.Render.run_view_range).parameters
    header = open(os.path.join(util.ROOT, "include", "crt.h")).read()
    assert "CRT_FLAG_PIXEL_FILTER = 128u" in header and "#define CRT_ABI_VERSION 5" in header


def fake_scene():
    """A non-null handle of zeroes for the checks that come before any use of the device: no filter set, no sums on it"""
    return np.zeros(1 << 18, dtype=np.uint8)


def test_refusals_come_before_any_device_call():
    """On a machine without a device every call here would fail with CRT_ERR_HIP if it reached one."""
    lib = capi.lib()
    sc = fake_scene()
    h_ = capi.ptr(sc)
    cam = capi.Camera()
    rgb, mean = np.full(48 * 3, 9, dtype=np.uint8), np.full(48 * 3, 9, dtype=F)
    done = C.c_uint32(77)

    def params(flags, world=1):
        return capi.Params(4, 4, 2, 0.8, 1, 0, 0, world, capi.TRAVERSAL_EXACT, flags)

    def renders_refused(status, word, prm):
        calls = (lambda: lib.crt_render(h_, C.byref(cam), C.byref(prm), capi.ptr(rgb), capi.ptr(mean), None),
                 lambda: lib.crt_render_device(h_, C.byref(cam), C.byref(prm), capi.ptr(rgb), capi.ptr(mean), None, None),
                 lambda: lib.crt_render_range(h_, C.byref(cam), C.byref(prm), 0, 1, None, None, None),
                 lambda: lib.crt_render_range_device(h_, C.byref(cam), C.byref(prm), 0, 1, None, None, None, None))
        for i, call in enumerate(calls):
            assert call() == status, i
            msg = lib.crt_last_error()
            assert word in msg and b"crt_render" in msg, (i, msg)

    # the flag with no filter set
    renders_refused(capi.ERR_INVALID_ARG, b"no filter", params(capi.FLAG_PIXEL_FILTER))
    # bad settings: refused, and still no filter on the handle
    for kind, radius in ((0, 0.49), (0, 2.5), (1, 0.5), (1, 0.99), (1, 2.01), (2, 1.0), (2, 1.9999), (3, 1.0), (7, 2.0), (0, float("nan")), (1, float("nan")),
                         (2, float("nan")), (1, float("inf")), (0, -1.0)):
        assert lib.crt_set_pixel_filter(h_, C.byref(capi.PixelFilter(kind, radius))) == capi.ERR_INVALID_ARG, (kind, radius)
        assert b"crt_set_pixel_filter" in lib.crt_last_error()
    renders_refused(capi.ERR_INVALID_ARG, b"no filter", params(capi.FLAG_PIXEL_FILTER))
    assert lib.crt_set_pixel_filter(None, C.byref(capi.PixelFilter(1, 1.0))) == capi.ERR_INVALID_ARG
    # every allowed setting is taken; with a filter set, a shard is refused as unsupported
    for kind, radius in ((0, 0.5), (0, 2.0), (1, 1.0), (1, 2.0), (2, 2.0), (1, 1.25)):
        assert lib.crt_set_pixel_filter(h_, C.byref(capi.PixelFilter(kind, radius))) == capi.CRT_OK, (kind, radius)
    renders_refused(capi.ERR_UNSUPPORTED, b"world > 1", params(capi.FLAG_PIXEL_FILTER | capi.FLAG_TILED_OUTPUT, world=2))
    # a bad setting keeps the old filter: the shard is still refused for being a shard, not for a missing filter
    assert lib.crt_set_pixel_filter(h_, C.byref(capi.PixelFilter(1, 0.25))) == capi.ERR_INVALID_ARG
    renders_refused(capi.ERR_UNSUPPORTED, b"world > 1", params(capi.FLAG_PIXEL_FILTER | capi.FLAG_TILED_OUTPUT, world=2))
    # NULL takes the filter off
    assert lib.crt_set_pixel_filter(h_, None) == capi.CRT_OK
    renders_refused(capi.ERR_INVALID_ARG, b"no filter", params(capi.FLAG_PIXEL_FILTER))
    # crt_filtered_frame: null scene, both outputs null, no render with the flag on the handle
    for form in ("crt_filtered_frame", "crt_filtered_frame_device"):
        tail = (C.byref(done),) if form == "crt_filtered_frame" else (None, C.byref(done))
        assert getattr(lib, form)(None, capi.ptr(rgb), capi.ptr(mean), *tail) == capi.ERR_INVALID_ARG, form
        assert b"crt_filtered_frame" in lib.crt_last_error() and b"null" in lib.crt_last_error()
        assert getattr(lib, form)(h_, None, None, *tail) == capi.ERR_INVALID_ARG, form
        assert b"crt_filtered_frame" in lib.crt_last_error() and b"null" in lib.crt_last_error()
        assert getattr(lib, form)(h_, capi.ptr(rgb), capi.ptr(mean), *tail) == capi.ERR_INVALID_ARG, form
        assert b"crt_filtered_frame" in lib.crt_last_error() and b"CRT_FLAG_PIXEL_FILTER" in lib.crt_last_error()
    assert done.value == 77 and (rgb == 9).all() and (mean == 9).all()
    crt_defaults = capi.PixelFilter()
    assert lib.crt_pixel_filter_defaults(None) == capi.ERR_INVALID_ARG
    assert lib.crt_pixel_filter_defaults(C.byref(crt_defaults)) == capi.CRT_OK and (crt_defaults.kind, crt_defaults.radius) == (1, 1.0)


def test_python_filter_specs():
    from cudaraytracing_amd.api import _pixel_filter
    assert [(p.kind, p.radius) for p in (_pixel_filter("box"), _pixel_filter("tent"), _pixel_filter("mitchell"))] == [(0, 0.5), (1, 1.0), (2, 2.0)]
    p = _pixel_filter(dict(kind="tent", radius=1.5))
    assert (p.kind, p.radius) == (1, 1.5)
    assert _pixel_filter(dict(kind=capi.PIXEL_FILTER_BOX, radius=2)).radius == 2.0
    for bad in ("gauss", dict(radius=1.0), dict(kind="tent", width=2)):
        with pytest.raises(ValueError):
            _pixel_filter(bad)


def test_numpy_philox_is_the_oracles():
    PF.check_philox()
    assert [PF.reach_of(r) for r in (0.5, 0.75, 1.0, 1.5, 1.51, 2.0)] == [0, 1, 1, 1, 2, 2]


def error_bound(L, S, n, kind, radius, seed):
    """out_mean of the restatement, its float64 evaluation, and the bound on their difference.
    The float64 evaluation takes the contract's own float32 weights w, quotients x = L / S and W, and evaluates a = sum w x and
    out = a S / W without rounding.  Against it the float32 result has, per channel of a pixel with T taps added: one rounding per
    product w x and T - 1 additions (the first adds to +0 exactly) -- T roundings at most on any term's way into a, each within 2^-24
    of a partial sum that is at most sum |w x| (for recursive sums and dot products T x 2^-24 holds without higher-order terms:
    Jeannerod and Rump 2013) --, one for S / W and one for the last product: (T + 2) x 2^-24 x sum |w x| x S / W.  A product that
    underflows adds at most 2^-150 each, allowed for with (T + 2) x 2^-149 x S / W."""
    a, W = PF.sums(L, S, n, kind, radius, seed)
    c = restated_sums(L, S, n)[0]
    out = PF.resolve(a, W, c, S, n)
    a64, W64, absum, absw, taps = PF.sums64(L, S, n, kind, radius, seed)
    assert (W > 0).all() and (taps >= n).all()             # every pixel takes at least its own samples
    scale = S / W.astype(np.float64)
    want = a64 * scale[..., None]
    bound = (taps + 2)[..., None] * U * absum * scale[..., None] + ((taps + 2) * 2.0 ** -149 * scale)[..., None]
    # W itself: T - 1 additions, each within 2^-24 of a partial sum of at most sum |w|
    assert (np.abs(W.astype(np.float64) - W64) <= (taps - 1) * U * absw).all()
    return out, want, bound


@pytest.mark.parametrize("w,h,S", SIZES[:2])
@pytest.mark.parametrize("name", SCENES)
def test_restatement_on_the_oracles_radiance(name, w, h, S):
    orgb, omean, L = oracle_frame(name, w, h, S)
    # BOX with R = 0.5 is the frame's own filter: the oracle's mean and RGB, bit for bit; mid-frame crt_preview's value
    mean, rgb = PF.filtered(L, S, S, PF.BOX, 0.5, 0)
    assert_bits(mean, omean, "box 0.5 against the oracle's mean")
    assert np.array_equal(rgb, orgb)
    n = S - 1
    with np.errstate(all="ignore"):
        assert_bits(PF.filtered(L, S, n, PF.BOX, 0.5, 0)[0], restated_sums(L, S, n)[0] * (F(S) / F(n)), "box 0.5 mid-frame against crt_preview's value")
    # every filter against the float64 evaluation of the same sums
    for kind, radius in FILTERS:
        for n in (S, 1):
            out, want, bound = error_bound(L, S, n, PF.KINDS[kind], radius, 0)
            err = np.abs(out.astype(np.float64) - want)
            print("%s %dx%d n %d %s %g: largest error / bound %.3f" % (name, w, h, n, kind, radius, float((err / np.maximum(bound, 1e-300)).max())))
            assert (err <= bound).all(), (kind, radius, n)


@pytest.mark.parametrize("kind,radius", FILTERS)
def test_a_constant_radiance_comes_back_constant(kind, radius):
    """L = 0.7 everywhere, S = 7, 13 x 9: in exact arithmetic every filter returns 0.7 x sum w / W = 0.7.  Held to error_bound's bound,
    where sum |w x| S / W = 0.7 sum |w| / W.  (The float64 evaluation there divides by the float32 W; against the constant itself W's own
    rounding -- at most (T - 1) x 2^-24 sum |w| / W more -- comes on top in the worst case.  The roundings of a and of W are those of
    nearly the same sum, and the figure printed here stays far below 1.)"""
    w, h, S = 13, 9, 7
    L = np.full((h, w, S, 3), 0.7, dtype=F)
    for seed in (0, BIG_SEED):
        out, want, bound = error_bound(L, S, S, PF.KINDS[kind], radius, seed)
        assert (np.abs(out.astype(np.float64) - want) <= bound).all()
        err = np.abs(out.astype(np.float64) - float(F(0.7)))
        print("%s %g seed %d: largest |out - 0.7| / bound %.3f" % (kind, radius, seed, float((err / bound).max())))
        assert (err <= bound).all()
    if kind == "box" and radius == 0.5:
        assert_bits(out, restated_sums(L, S, S)[0], "box 0.5 of a constant")


# ---- the kernel text on the host, under the sanitizers ----

def host_job(frames, resolves, taps):
    b = [struct.pack("<I", len(frames))]
    for (w, h, S, n, chunk, kind, radius, seed, L) in frames:
        assert L.shape == (h, w, S, 3) and L.dtype == F
        b += [struct.pack("<IIIIIIfQ", w, h, S, n, chunk, kind, radius, seed), np.ascontiguousarray(L).tobytes()]
    b.append(struct.pack("<I", len(resolves)))
    for (a, W, c, S, n) in resolves:
        b.append(np.array(list(a) + [W] + list(c), dtype=F).tobytes() + struct.pack("<II", S, n))
    b.append(struct.pack("<I", len(taps)))
    for (kind, radius, di, dj, ux, uy, x, s) in taps:
        b.append(struct.pack("<Ifii", kind, radius, di, dj) + np.array([ux, uy] + list(x) + list(s), dtype=F).tobytes())
    return b"".join(b)


def restated_tap(kind, radius, di, dj, ux, uy, x, s):
    """one tap of the contract on made-up values, numpy float32 scalars"""
    with np.errstate(all="ignore"):
        dx, dy = (F(di) + F(ux)) - F(0.5), (F(dj) + F(uy)) - F(0.5)
        wt = PF.weight(kind, radius, np.array([dx, dy], dtype=F))
        wv = wt[0] * wt[1]
        s = np.array(s, dtype=F)
        if wv == 0:
            return s
        return np.array([s[0] + wv * F(x[0]), s[1] + wv * F(x[1]), s[2] + wv * F(x[2]), s[3] + wv], dtype=F)


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tools/pixel_filter_host_check.cpp built with the sanitizers and run on the job below: (job, status, output bytes, printed)"""
    tmp = str(tmp_path_factory.mktemp("pixel_filter_host"))
    rng = np.random.default_rng(3)
    inf, nan = float("inf"), float("nan")
    w, h, S = 13, 9, 3
    L = (rng.random((h, w, S, 3)) * 4).astype(F)
    # NaN / +-inf radiance in single samples: (j, i, sample) -> value
    L[4, 6, 1] = nan
    L[0, 0, 0, 1] = inf
    L[8, 12, 2] = -inf
    L[3, 11, 0, 2] = nan
    frames = []
    for kind, radius in FILTERS:
        for chunk in (S, 1):
            frames.append((w, h, S, S, chunk, PF.KINDS[kind], radius, BIG_SEED, L))
    frames.append((w, h, S, 2, 2, PF.TENT, 1.0, 0, L))                       # a frame in flight: n < S
    frames.append((5, 3, 2, 2, 2, PF.MITCHELL, 2.0, 7, (rng.random((3, 5, 2, 3)) * 4).astype(F)))   # one partial tile
    frames.append((37, 10, 2, 2, 1, PF.TENT, 2.0, 0, (rng.random((10, 37, 2, 3)) * 4).astype(F)))   # a second, partial workgroup in x, two tile rows
    a, c = (1.0, 2.0, 3.0), (0.25, 0.5, 0.75)
    resolves = [(a, W, c, 7, 3) for W in (0.0, -0.0, -1.0, nan, inf, -inf, 1e-38, 1e-45, 0.5, 3.0)]
    resolves += [((nan, inf, -1.0), 2.0, c, 7, 3), (a, nan, (nan, inf, 0.0), 5, 5)]
    taps = []
    s0 = (0.5, 0.25, 0.125, 1.5)
    x = (1.0, 2.0, 3.0)
    for kind, radius in FILTERS + [("box", 1.0), ("box", 2.0), ("tent", 1.25)]:
        k = PF.KINDS[kind]
        reach = PF.reach_of(radius)
        for di in range(-reach, reach + 1):
            # ux = 1 exactly, the smallest and the largest jitter below it, the middle, and the values that put d on +-R where there are any
            for ux in (1.0, float(F(1.1641532182693481e-10)), float(np.nextafter(F(1), F(0))), 0.5, radius + 0.5 - di, -radius + 0.5 - di,
                       float(np.nextafter(F(radius + 0.5 - di), F(9))), float(np.nextafter(F(-radius + 0.5 - di), F(9)))):
                taps.append((k, radius, di, 0, ux, 0.5, x, s0))
                taps.append((k, radius, 0, di, 0.5, ux, x, s0))
        taps.append((k, radius, 0, 0, 0.5, 0.5, (nan, inf, -inf), s0))
        taps.append((k, radius, reach, reach, 1.0, 1.0, (nan, 1.0, 2.0), s0))  # outside the support unless R reaches reach + 0.5: a NaN that must not count
    job = os.path.join(tmp, "job.bin")
    with open(job, "wb") as f:
        f.write(host_job(frames, resolves, taps))
    exe = HP.build("pixel_filter_host_check.cpp", os.path.join(tmp, "pixel_filter_host_check"), HP.SANITISED)
    out = os.path.join(tmp, "out.bin")
    rc, printed, err = HP.run(exe, [job, out])
    return (frames, resolves, taps), rc, open(out, "rb").read() if os.path.exists(out) else b"", printed + err


def test_kernel_text_on_the_host_is_clean_under_the_sanitizers(host_check):
    _, rc, _, printed = host_check
    assert rc == 0, printed
    assert "runtime error" not in printed and "Sanitizer" not in printed, printed


def test_kernel_text_on_the_host_gives_the_restatement_bits(host_check):
    (frames, resolves, taps), rc, data, printed = host_check
    assert rc == 0, printed
    at = 0

    def take(count, dtype):
        nonlocal at
        v = np.frombuffer(data, dtype=dtype, count=count, offset=at)
        at += v.nbytes
        return v

    for (w, h, S, n, chunk, kind, radius, seed, L) in frames:
        a, W = PF.sums(L, S, n, kind, radius, seed)
        mean = PF.resolve(a, W, restated_sums(L, S, n)[0], S, n)
        rgb = O.tonemap(mean)
        where = "%dx%d S %d n %d chunk %d kind %d radius %g" % (w, h, S, n, chunk, kind, radius)
        for form in ("direct", "staged"):
            assert_bits(take(h * w * 3, F).reshape(h, w, 3), a, "%s, %s: a" % (where, form))
            assert_bits(take(h * w, F).reshape(h, w), W, "%s, %s: W" % (where, form))
            assert_bits(take(h * w * 3, F).reshape(h, w, 3), mean, "%s, %s: out_mean" % (where, form))
            assert np.array_equal(take(h * w * 3, np.uint8).reshape(h, w, 3), rgb), (where, form)
    # NaN / inf radiance poisons exactly the pixels whose support holds the sample: where the float32 sums of the finite rest differ
    w, h, S, n, chunk, kind, radius, seed, L = frames[4]                      # tent 1, one chunk
    assert (kind, radius) == (PF.TENT, 1.0) and not np.isfinite(L).all()
    clean = np.where(np.isfinite(L), L, F(0))
    marked = np.where(np.isfinite(L), F(0), F(1))
    hit = PF.sums(marked, S, n, kind, radius, seed)[0] > 0                   # the channels some non-finite sample reaches with w != 0
    got = PF.filtered(L, S, n, kind, radius, seed)[0]
    assert hit.any() and not hit.all()
    assert (~np.isfinite(got) == hit).all()
    assert_bits(got[~hit], PF.filtered(clean, S, n, kind, radius, seed)[0][~hit], "the pixels no non-finite sample reaches")
    # pixel_filter_resolve on made-up sums
    for (a, W, c, S, n) in resolves:
        with np.errstate(all="ignore"):
            want = PF.resolve(np.array(a, dtype=F)[None, None], np.array([[W]], dtype=F), np.array(c, dtype=F)[None, None], S, n)[0, 0]
            fallback = np.array(c, dtype=F) * (F(S) / F(n))
        got = take(3, F)
        assert_bits(got, want, "resolve W = %r" % (W,))
        if not (W > 0):
            assert_bits(got, fallback, "the fallback at W = %r" % (W,))
    # pixel_filter_tap on made-up jitters: ux = 1, the support's borders
    counted = 0
    for t in taps:
        got, want = take(4, F), restated_tap(*t)
        assert_bits(got, want, "tap %r" % (t,))
        counted += int(got[3] != F(t[7][3]))
    assert 0 < counted < len(taps)
    assert at == len(data)
    # the borders themselves: d = R counts, d = -R does not (BOX, whose f is 1 inside: the weight says which side)
    s0 = (0.0, 0.0, 0.0, 0.0)
    assert restated_tap(PF.BOX, 0.5, 0, 0, 1.0, 0.5, (1, 1, 1), s0)[3] == 1     # d = +0.5
    assert restated_tap(PF.BOX, 0.5, 0, 0, 0.0, 0.5, (1, 1, 1), s0)[3] == 0     # d = -0.5 (no real jitter is 0)
    assert restated_tap(PF.BOX, 1.5, 1, 0, 1.0, 0.5, (1, 1, 1), s0)[3] == 1     # d = +1.5
    assert restated_tap(PF.BOX, 1.5, -2, 0, 1.0, 0.5, (1, 1, 1), s0)[3] == 0    # d = -1.5


# ------------------------------------------------------------------------------------------------------------------ GPU --

def filtered_frame(r, name, w, h, S, kind, radius, seed=0, **kw):
    """(frame rgb, frame mean, filtered rgb, filtered mean) of a one-shot render with the flag"""
    r.set_spp(S)
    r.seed = seed
    try:
        r.set_pixel_filter(spec(kind, radius))
        rgb = r.run_view(*util.camera(name), width=w, height=h, pixel_filter=True, **kw).copy()
        return rgb, r.mean_buffer.copy(), r.filtered_rgb, r.filtered_mean
    finally:
        r.seed = 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, BIG_SEED])
@pytest.mark.parametrize("w,h,S", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_device_matches_the_restatement(renders, name, w, h, S, seed, monkeypatch):
    orgb, omean, L = oracle_frame(name, w, h, S, seed)
    r = renders[name]
    for kind, radius in FILTERS:
        want_mean, want_rgb = restated(name, w, h, S, S, kind, radius, seed)
        for form in ("direct", "staged"):
            monkeypatch.setenv("CRT_PIXEL_FILTER_FORM", form)
            where = "%s %dx%d spp %d seed %d, %s %g, %s" % (name, w, h, S, seed, kind, radius, form)
            rgb, mean, frgb, fmean = filtered_frame(r, name, w, h, S, kind, radius, seed)
            assert np.array_equal(rgb, orgb), where
            assert_bits(mean, omean, where + ": the frame")
            assert_bits(fmean, want_mean, where + ": out_mean")
            assert np.array_equal(frgb, want_rgb), where
            frgb2, fmean2, done = r.filtered(width=w, height=h)       # readable until the next render call, as often as one likes
            assert done == S
            assert_bits(fmean2, want_mean, where + ": second read")
            assert np.array_equal(frgb2, want_rgb), where
            if (kind, radius) == ("box", 0.5):                        # the frame's own filter: the same call's frame
                assert_bits(fmean, mean, where + ": box 0.5 against the frame")
                assert np.array_equal(frgb, rgb), where
            else:
                assert not np.array_equal(fmean, mean), where


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_the_flag_changes_nothing_else(renders, name, monkeypatch):
    """The frame, c (crt_preview mid-frame), the variance and the halves with the flag are the bits without it."""
    w, h, S = 61, 47, 7
    r = renders[name]
    cam = util.camera(name)
    r.set_spp(S)
    r.set_pixel_filter(spec("mitchell", 2.0))

    def run(flag):
        out = {}
        assert r.run_view_range(*cam, 0, 3, width=w, height=h, want_halves=True, pixel_filter=flag) is None
        out["preview"] = r.preview(want_mean=True, width=w, height=h)[1]
        out["rgb"] = r.run_view_range(*cam, 3, 4, width=w, height=h, want_halves=True, pixel_filter=flag).copy()
        out["mean"] = r.mean_buffer.copy()
        out["variance"] = r.variance(width=w, height=h)[0]
        out["half_a"], out["half_b"] = r.half_buffers(width=w, height=h)[:2]
        return out

    plain, flagged = run(False), run(True)
    for k in plain:
        if k == "rgb":
            assert np.array_equal(plain[k], flagged[k])
        else:
            assert_bits(flagged[k], plain[k], k)
    assert_bits(r.filtered(width=w, height=h)[1], restated(name, w, h, S, S, "mitchell", 2.0, 0)[0], "the filtered frame beside the halves")
    # without the variance: the frame of a one-shot render, and the commit ring (here forced to 2 samples) is off for the call
    orgb, omean, _ = oracle_frame(name, w, h, S)
    monkeypatch.delenv("CRT_PIPELINE", raising=False)
    monkeypatch.setenv("CRT_COMMIT_RING_LOG2", "1")
    r.run_view(*cam, width=w, height=h)
    assert r.radiance_storage()[1] == 2, "the forced ring did not engage without the flag: the check shows nothing"
    rgb = r.run_view(*cam, width=w, height=h, pixel_filter=True)
    assert r.radiance_storage()[1] == 0
    assert np.array_equal(rgb, orgb)
    assert_bits(r.mean_buffer, omean, "the frame with the flag alone")
    assert_bits(r.filtered_mean, restated(name, w, h, S, S, "mitchell", 2.0, 0)[0], "the filtered frame of the flag alone")


def tiled(img, w, h):
    """img (h, w, k) in the compact tile order of an unsharded frame: (slots, k), padding slots 0"""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    out = np.zeros((tx * ty * 64,) + img.shape[2:], dtype=img.dtype)
    for j in range(h):
        for i in range(w):
            out[((j // 8) * tx + i // 8) * 64 + (j % 8) * 8 + i % 8] = img[j, i]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["4", "2"])
@pytest.mark.parametrize("name", SCENES)
def test_chunk_borders_and_progressive_ranges(renders, name, pipeline, monkeypatch):
    """61 x 47 spp 7 in chunks of one sample (3 072 pixel slots, chunks of 2^12 paths), ranges split at 0 | 3 | 7: crt_filtered_frame
    after each range is the restatement with n samples; a range that changes the filter mid-frame is refused and the frame in flight
    survives; the device form on a stream, with the tiled layout."""
    monkeypatch.setenv("CRT_PIPELINE", pipeline)
    monkeypatch.setenv("CRT_CHUNK_LOG2", "12")
    w, h, S = 61, 47, 7
    orgb, omean, L = oracle_frame(name, w, h, S)
    r = renders[name]
    cam = util.camera(name)
    r.set_spp(S)
    lib = capi.lib()
    for kind, radius in (("tent", 1.0), ("mitchell", 2.0)):
        for form in ("direct", "staged"):
            monkeypatch.setenv("CRT_PIXEL_FILTER_FORM", form)
            where = "%s pipeline %s %s %g %s" % (name, pipeline, kind, radius, form)
            r.set_pixel_filter(spec(kind, radius))
            assert r.run_view_range(*cam, 0, 3, width=w, height=h, pixel_filter=True, stats=True) is None
            assert pipeline == "2" or r.stats["kernel_launches"] == 3, where
            m3, rgb3 = restated(name, w, h, S, 3, kind, radius, 0)
            frgb, fmean, done = r.filtered(width=w, height=h)
            assert done == 3
            assert_bits(fmean, m3, where + ": after 3 samples")
            assert np.array_equal(frgb, rgb3), where
            # another filter mid-frame: refused, nothing touched
            r.set_pixel_filter(spec("box", 1.5))
            with pytest.raises(crt.CrtError) as e:
                r.run_view_range(*cam, 3, 4, width=w, height=h, pixel_filter=True)
            assert e.value.status == capi.ERR_INVALID_ARG and "crt_render_range" in str(e.value) and "filter" in str(e.value)
            assert_bits(r.filtered(width=w, height=h)[1], m3, where + ": after the refused range")
            assert r.preview(width=w, height=h)[2] == 3
            # a setting the library does not allow keeps the old filter; the frame's own filter goes back on and the frame completes
            with pytest.raises(crt.CrtError):
                r.set_pixel_filter(dict(kind="tent", radius=0.5))
            r.set_pixel_filter(spec(kind, radius))
            rgb = r.run_view_range(*cam, 3, 4, width=w, height=h, pixel_filter=True)
            assert np.array_equal(rgb, orgb), where
            assert_bits(r.mean_buffer, omean, where + ": the frame")
            m7, rgb7 = restated(name, w, h, S, S, kind, radius, 0)
            frgb, fmean, done = r.filtered(width=w, height=h)
            assert done == S
            assert_bits(fmean, m7, where + ": after the last range")
            assert np.array_equal(frgb, rgb7), where
    # the device forms on a stream of the caller's, tiled layout (world == 1): every slot is written, padding slots RGB 0 and +0
    kind, radius = "mitchell", 2.0
    m3, rgb3 = restated(name, w, h, S, 3, kind, radius, 0)
    want_mean, want_rgb = tiled(m3, w, h), tiled(rgb3, w, h)
    slots = crt.shard_slots(w, h, 0, 1)
    assert slots == want_mean.shape[0]
    c_cam = r._cam(*cam)
    prm = r._params(flags=capi.FLAG_TILED_OUTPUT | capi.FLAG_PIXEL_FILTER, width=w, height=h)
    with DeviceBuffers({"rgb": slots * 3, "mean": slots * 12}, stream=True) as d:
        stream = C.c_void_p(d.stream)
        d.fill("rgb")
        d.fill("mean")
        capi.check(lib.crt_render_range_device(r._h, C.byref(c_cam), C.byref(prm), 0, 3, None, None, stream, None), "crt_render_range_device")
        done = C.c_uint32()
        capi.check(lib.crt_filtered_frame_device(r._h, C.c_void_p(d.ptrs["rgb"]), C.c_void_p(d.ptrs["mean"]), stream, C.byref(done)), "crt_filtered_frame_device")
        d.synchronize()
        assert done.value == 3
        assert_bits(d.download("mean", (slots, 3), F), want_mean, "device form, tiled")
        assert np.array_equal(d.download("rgb", (slots, 3), np.uint8), want_rgb)
        # one output at a time
        d.fill("rgb")
        d.fill("mean")
        capi.check(lib.crt_filtered_frame_device(r._h, None, C.c_void_p(d.ptrs["mean"]), stream, None), "crt_filtered_frame_device")
        d.synchronize()
        assert_bits(d.download("mean", (slots, 3), F), want_mean, "device form, the mean alone")
        assert (d.download("rgb", (slots, 3), np.uint8) == 0x55).all()
        hrgb = np.full((slots, 3), 7, dtype=np.uint8)
        capi.check(lib.crt_filtered_frame(r._h, capi.ptr(hrgb), None, None), "crt_filtered_frame")
        assert np.array_equal(hrgb, want_rgb)


@pytest.mark.gpu
def test_filtered_frame_is_refused_without_the_sums(renders):
    name, w, h, S = "cornell-box", 13, 9, 3
    r = renders[name]
    cam = util.camera(name)
    r.set_spp(S)
    r.set_pixel_filter("tent")

    def refused():
        with pytest.raises(crt.CrtError) as e:
            r.filtered(width=w, height=h)
        assert e.value.status == capi.ERR_INVALID_ARG and "crt_filtered_frame" in str(e.value)

    r.run_view(*cam, width=w, height=h)                                        # the last render went without the flag
    refused()
    r.run_view_range(*cam, 0, 1, width=w, height=h, pixel_filter=True)
    assert r.filtered(width=w, height=h)[2] == 1
    r.run_view_range(*cam, 1, 1, width=w, height=h)                            # a range of the frame without the flag
    refused()
    r.run_view_range(*cam, 2, 1, width=w, height=h, pixel_filter=True)         # ... and the sums stay refused for the rest of the frame
    refused()
    r.run_view(*cam, width=w, height=h, pixel_filter=True)
    assert r.filtered(width=w, height=h)[2] == S
    r.extra_flags = capi.FLAG_PIXEL_FILTER                                     # the sparse frames ignore the flag
    try:
        r.run_view_adaptive(*cam, min_samples=2, width=w, height=h)
        refused()
        r.run_view(*cam, width=w, height=h, pixel_filter=True)
        r.run_view_map(*cam, np.full((h, w), 2, dtype=np.uint32), width=w, height=h)
        refused()
        r.run_view(*cam, width=w, height=h, pixel_filter=True)
        r.run_view_planned(*cam, min_samples=2, width=w, height=h)
        refused()
    finally:
        r.extra_flags = 0
    r.set_pixel_filter(None)
    with pytest.raises(crt.CrtError) as e:
        r.run_view(*cam, width=w, height=h, pixel_filter=True)
    assert e.value.status == capi.ERR_INVALID_ARG and "no filter" in str(e.value)


@pytest.mark.gpu
def test_multi_device_frames_clear_the_flag():
    """crt_multi_render and crt_multi_render_buffers clear the flag (a shard keeps no filter sums): left on, every rank would refuse the
    call for want of a filter on its handle.  Two ranks on one device."""
    name, w, h, S = "veach-mis", 61, 47, 7                 # (the smaller scene: two handles are made; the oracle's frame is the other tests')
    orgb, omean, _ = oracle_frame(name, w, h, S)
    t = util.task(name)
    m = crt.MultiRender(util.host_scene(name), S, t.P_RR, t.light_sample_n, devices=(0, 0), gather=crt.GATHER_COPY)
    try:
        m.extra_flags = capi.FLAG_PIXEL_FILTER
        rgb = m.run_view(*util.camera(name), width=w, height=h)
        assert np.array_equal(rgb, orgb)
        assert_bits(m.mean_buffer, omean, "crt_multi_render with the flag")
        out = m.run_view_gathered(*util.camera(name), want=("rgb", "mean"), width=w, height=h)
        assert np.array_equal(out["rgb"], orgb)
        assert_bits(out["mean"], omean, "crt_multi_render_buffers with the flag")
    finally:
        m.free()


@pytest.mark.gpu
def test_cli_writes_the_filtered_frame(tmp_path):
    from PIL import Image
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    name, w, h, S, seed = "cornell-box", 32, 24, 4, 42
    orgb, omean, L = oracle_frame(name, w, h, S, seed)
    base = [cli, util.SCENES[name], "--spp", str(S), "--width", str(w), "--height", str(h), "--seed", str(seed), "--base-dir", util.ROOT]
    plain, png, pfm = (str(tmp_path / n) for n in ("plain.png", "filtered.png", "filtered.pfm"))
    res = subprocess.run(base + ["-o", plain, "--pixel-filter", "tent,1.5", "--pixel-filter-out", png], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    want_mean, want_rgb = restated(name, w, h, S, S, "tent", 1.5, seed)
    assert np.array_equal(np.asarray(Image.open(plain)), orgb)
    assert np.array_equal(np.asarray(Image.open(png)), want_rgb)
    res = subprocess.run(base + ["-o", plain, "--pixel-filter", "mitchell", "--pixel-filter-out", pfm], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert_bits(util.read_pfm(pfm)[1], restated(name, w, h, S, S, "mitchell", 2.0, seed)[0], "the PFM of the Mitchell frame")
    for extra in (["--pixel-filter", "tent"], ["--pixel-filter-out", png], ["--pixel-filter", "gauss", "--pixel-filter-out", png],
                  ["--pixel-filter", "tent,wide", "--pixel-filter-out", png], ["--pixel-filter", "tent,0.5", "--pixel-filter-out", png],
                  ["--pixel-filter", "tent", "--pixel-filter-out", png, "--adaptive", "0.05"]):
        bad = subprocess.run(base + ["-o", plain] + extra, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "ixel" in bad.stderr, (extra, bad.stderr)
