"""The error of the frame in flight and rendering to an error target: crt_frame_error / crt_frame_error_device /
crt_frame_error_defaults and crt_render_until / crt_render_until_device / crt_until_defaults (include/crt.h), Render.frame_error,
Render.run_view_until and until_defaults in Python, crt::Render::frame_error / run_view_until, crt_cli --until.

The expected values come from the oracle's per-path radiance (frames.oracle_render): frame_error_restated.py restates both contracts
in numpy -- the sums of util.restated_sums, the criterion on variance_restated.variance_of_sums, the two fp64 sums in the contract's own
order -- and the device must give every count exactly and both sums bit for bit.

The until frames are 64 x 48 at spp 32, min_samples 4, step 4, mean_floor 0.01 and threshold 0.3.  The threshold was picked on the CPU
so that the restated sequence of `above` at n = 4, 8, 12 falls strictly on both scenes (cornell-box 1364, 1160, 1007; veach-mis 864, 374,
252): with max_above = the third check's value the restated call stops at n = 12, inside (4, 32).  until_case asserts that of its inputs."""
import ctypes as C
import functools
import inspect
import math
import struct
import subprocess

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import host_program as HP
import oracle_lib as O
import util
from frame_error_restated import (FIELDS, criterion, frame_error_of_sums, restated_frame_error, restated_until, shard_slots_of, tree64, tree_sum)
from frames import fresh_render, oracle_frame, renders  # noqa: F401
from util import assert_bits, restated_sums
from variance_restated import restated_variance

F = np.float32
EXPORTS = ("crt_frame_error_defaults", "crt_frame_error", "crt_frame_error_device", "crt_until_defaults", "crt_render_until", "crt_render_until_device")
S = 8                      # the frames of the crt_frame_error tests: mid-flight after range(0, 3), and finished
MID = 3
SHAPES = [(1, 1), (9, 7), (8, 8), (13, 5), (17, 15), (16, 16), (257, 1), (64, 48)]   # 63, 64, 65, 255, 256 pixels; 33 tiles in a row; 12 blocks
UW, UH, US = 64, 48, 32    # the frames of the crt_render_until tests
UNTIL = dict(min_samples=4, step_samples=4, threshold=0.3, mean_floor=0.01)
RENDER_SPP = S             # (what frames.renders creates the handles with)


def bits64(x):
    return struct.pack("<d", x)


def check_summary(got, want, where):
    """Every field of a crt_frame_error_info (dicts): the counts exactly, the two sums bit for bit"""
    for f in FIELDS:
        if f.startswith("sum_"):
            assert bits64(got[f]) == bits64(want[f]), "%s: %s is %r (%s), expected %r (%s)" % (where, f, got[f], float(got[f]).hex(), want[f], float(want[f]).hex())
        else:
            assert got[f] == want[f], "%s: %s is %r, expected %r" % (where, f, got[f], want[f])
    assert sum(got["hist"]) + got["nan_pixels"] == got["pixels"] and sum(got["hist"][8:]) + got["nan_pixels"] == got["above"], where


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_entry_points_are_exported_and_the_abi_version_stays():
    lib = capi.lib()
    for name in EXPORTS:
        assert name in capi.EXPORTS
        getattr(lib, name)
    lib.crt_abi_version.restype = C.c_int
    assert lib.crt_abi_version() == 5 == capi.ABI_VERSION
    for name in ("until_defaults", "frame_error_defaults", "FrameError"):
        assert hasattr(crt, name)
    sig = inspect.signature(crt.Render.run_view_until).parameters
    for name in ("min_samples", "step_samples", "threshold", "mean_floor", "max_above", "sample_begin", "want_variance", "width", "height"):
        assert name in sig
    assert set(inspect.signature(crt.Render.frame_error).parameters) == {"self", "threshold", "mean_floor"}
    for method in ("frame_error", "run_view_until"):
        with pytest.raises(NotImplementedError):       # (like its siblings: no handle is looked at)
            getattr(crt.MultiRender, method)(None)
    assert C.sizeof(capi.FrameErrorInfo) == 4 + 4 + 3 * 8 + 16 * 8 + 2 * 8 and capi.FrameErrorInfo.above.offset == 24
    assert C.sizeof(capi.UntilParams) == 24 and capi.UntilParams.max_above.offset == 16
    assert C.sizeof(capi.UntilInfo) == 16 + 64 * 8 + 8 + 4 + 4 + C.sizeof(capi.FrameErrorInfo) and capi.UntilInfo.last.offset == 544


def test_defaults_are_the_adaptive_calls():
    d, a = crt.until_defaults(), crt.adaptive_defaults()
    assert set(d) == {"min_samples", "step_samples", "threshold", "mean_floor", "max_above"}
    assert all(d[k] == a[k] for k in a) and d["max_above"] == 0
    assert (d["min_samples"], d["step_samples"]) == (16, 64) and F(d["threshold"]) == F(0.05) and F(d["mean_floor"]) == F(0.01)
    e = crt.frame_error_defaults()
    assert e == {"threshold": a["threshold"], "mean_floor": a["mean_floor"]}
    lib = capi.lib()
    assert lib.crt_until_defaults(None) == capi.ERR_INVALID_ARG and lib.crt_last_error().decode().startswith("crt_until_defaults")
    assert lib.crt_frame_error_defaults(None, None) == capi.ERR_INVALID_ARG and lib.crt_last_error().decode().startswith("crt_frame_error_defaults")


def test_refusals_come_before_any_device_call():
    """Every refusal that needs no handle, with a null scene (there is no device call to make): CRT_ERR_INVALID_ARG, the outputs
    untouched, and crt_last_error starts with the entry point's name and names the argument.  (What the handle holds: the GPU tests.)"""
    lib = capi.lib()
    info = capi.FrameErrorInfo()
    info.pixels = 77
    nan, inf = float("nan"), float("inf")

    def fe(form, thr=0.05, floor=0.01, out=True):
        if form == "crt_frame_error":
            rc = lib.crt_frame_error(None, thr, floor, C.byref(info) if out else None)
        else:
            rc = lib.crt_frame_error_device(None, thr, floor, C.c_void_p(C.addressof(info)) if out else None, None)
        return rc, lib.crt_last_error().decode()

    for form in ("crt_frame_error", "crt_frame_error_device"):
        for kw, word in ((dict(), "null argument"), (dict(out=False), "null output"), (dict(thr=-0.5), "threshold"), (dict(thr=nan), "threshold"),
                         (dict(floor=-1.0), "mean_floor"), (dict(floor=inf), "mean_floor"), (dict(floor=nan), "mean_floor")):
            rc, err = fe(form, **kw)
            assert rc == capi.ERR_INVALID_ARG and err.startswith("crt_frame_error: ") and word in err, (form, kw, rc, err)
        for kw in (dict(thr=inf), dict(thr=0.0, floor=0.0)):      # accepted values are not what is refused
            rc, err = fe(form, **kw)
            assert rc == capi.ERR_INVALID_ARG and "null argument" in err, (form, kw, err)
    assert info.pixels == 77

    n = 8 * 8
    rgb, mean, var = np.full(n * 3, 9, dtype=np.uint8), np.full(n * 3, 9, dtype=F), np.full(n * 3, 9, dtype=F)
    ui = capi.UntilInfo()
    ui.passes = 77
    cam = capi.Camera()

    def until(form, cam_=cam, prm=None, up=None, out_rgb=rgb, no_prm=False, no_up=False, begin=0):
        p = capi.Params(8, 8, 16, 0.8, 1, 0, 0, 1, capi.TRAVERSAL_EXACT, 0)
        for k, v_ in (prm or {}).items():
            setattr(p, k, v_)
        u = capi.UntilParams(4, 2, 0.1, 0.01, 0)
        for k, v_ in (up or {}).items():
            setattr(u, k, v_)
        tail = (C.byref(ui),) if form == "crt_render_until" else (None, C.byref(ui))
        rc = getattr(lib, form)(None, C.byref(cam_) if cam_ is not None else None, None if no_prm else C.byref(p), None if no_up else C.byref(u), begin,
                                capi.ptr(out_rgb), capi.ptr(mean), capi.ptr(var), *tail)
        return rc, lib.crt_last_error().decode()

    cases = [(dict(), "scene"), (dict(cam_=None), "camera"), (dict(no_prm=True), "params"), (dict(no_up=True), "until params"), (dict(out_rgb=None), "out_rgb"),
             (dict(up=dict(min_samples=1)), "min_samples"), (dict(up=dict(min_samples=0)), "min_samples"), (dict(up=dict(min_samples=17)), "min_samples"),
             (dict(up=dict(step_samples=0)), "step_samples"), (dict(up=dict(threshold=-0.5)), "threshold"), (dict(up=dict(threshold=nan)), "threshold"),
             (dict(up=dict(mean_floor=-1.0)), "mean_floor"), (dict(up=dict(mean_floor=inf)), "mean_floor"), (dict(up=dict(mean_floor=nan)), "mean_floor")]
    render_cases = [(dict(prm=dict(width=0)), "width"), (dict(prm=dict(world=0)), "rank < world"), (dict(prm=dict(rank=1)), "rank < world"),
                    (dict(prm=dict(world=2)), "CRT_FLAG_TILED_OUTPUT"), (dict(prm=dict(light_sample_n=-1)), "light_sample_n"), (dict(prm=dict(traversal=7)), "traversal")]
    for form in ("crt_render_until", "crt_render_until_device"):
        for kw, word in cases:
            rc, err = until(form, **kw)
            assert rc == capi.ERR_INVALID_ARG and err.startswith("crt_render_until: ") and word in err, (form, kw, rc, err)
        for kw, word in render_cases:                                  # what crt_render_range refuses, as it refuses it
            rc, err = until(form, **kw)
            assert rc == capi.ERR_INVALID_ARG and err.startswith("crt_render: ") and word in err, (form, kw, rc, err)
        for kw in (dict(up=dict(threshold=inf)), dict(up=dict(threshold=0.0, mean_floor=0.0)), dict(up=dict(min_samples=16)), dict(up=dict(max_above=2 ** 40)),
                   dict(begin=5)):
            rc, err = until(form, **kw)
            assert rc == capi.ERR_INVALID_ARG and "null scene" in err, (form, kw, err)
    assert (rgb == 9).all() and (mean == 9).all() and (var == 9).all() and ui.passes == 77


def synthetic_sums(n_pix, seed, specials):
    rng = np.random.default_rng(seed)
    x = (rng.random((n_pix, 5, 3)) * rng.random((n_pix, 1, 1)) ** 4 * 4).astype(F) / F(8)
    c, q = x.sum(axis=1, dtype=F), (x * x).sum(axis=1, dtype=F)
    if specials:
        c[::17, 0], c[5::29, 1], q[3::23, 2], q[7::31, 0], c[11::37, 2] = np.nan, np.inf, np.inf, -np.inf, 0.0
    return c, q


def test_restated_counts_are_consistent_and_the_tree_sum_is_a_sum_in_its_own_order():
    rng = np.random.default_rng(5)
    for n_pix in (1, 63, 64, 65, 255, 256, 257, 64 * 256 - 1, 64 * 256, 64 * 256 + 300):
        c, q = synthetic_sums(n_pix, n_pix, specials=True)
        valid = rng.random(n_pix) < 0.9
        for thr in (0.0, 0.05, 0.5, np.inf):
            E = frame_error_of_sums(c, q, 8, 5, thr, 0.01, valid)
            assert E["pixels"] == valid.sum() and sum(E["hist"]) + E["nan_pixels"] == E["pixels"], (n_pix, thr)
            assert sum(E["hist"][8:]) + E["nan_pixels"] == E["above"], (n_pix, thr)
            if n_pix > 64:
                assert E["nan_pixels"] > 0
            v, tt, m = criterion(c, q, 8, 5, thr, 0.01)
            assert E["above"] == int((valid & ~(v <= tt)).sum())                    # the adaptive call's own decision
        assert frame_error_of_sums(c, q, 8, 5, np.inf, 0.01, valid)["above"] == frame_error_of_sums(c, q, 8, 5, np.inf, 0.01, valid)["nan_pixels"]
        # several bins are in use: the histogram says something
        c, q = synthetic_sums(n_pix, n_pix, specials=False)
        if n_pix >= 255:
            assert sum(1 for k in frame_error_of_sums(c, q, 8, 5, 0.3, 0.01)["hist"] if k) >= 4
    # the tree against the exact sum and against another order
    differs = []
    for n_pix in (1, 64, 65, 257, 64 * 256 + 300, 160 * 120, 30000, 50000):
        v = rng.random(n_pix) ** 8 * 1e3
        exact, got = math.fsum(v), tree_sum(v)
        assert abs(got - exact) <= 64 * np.spacing(exact), n_pix                    # (a tree of depth < 32 over n_pix positive values)
        if n_pix > 1000:
            running = 0.0
            for x in v:
                running += x
            assert abs(running - exact) <= 1e-11 * exact
            differs.append(bits64(running) != bits64(got))
    assert any(differs), "every running sum has the tree's bits: the test could not tell the orders apart"
    x = np.arange(64, dtype=np.float64)
    assert tree64(x) == 63 * 32 and tree_sum(np.full(300, -0.0)) == 0.0 and not math.copysign(1.0, tree_sum(np.full(300, -0.0))) < 0


def test_restated_until_stops_at_the_first_check_within_max_above():
    rng = np.random.default_rng(9)
    S_, h, w = 24, 12, 14
    L = (rng.random((h, w, S_, 3)) * rng.random((h, w, 1, 1)) * 4).astype(F)
    A = {n: restated_frame_error(L, S_, n, 0.2, 0.02)["above"] for n in range(3, S_ + 1)}
    for mn, st, begin in ((3, 5, 0), (4, 1, 0), (6, 4, 2), (3, 5, 8), (3, 7, 3)):
        checks = [max(mn, begin)]
        while checks[-1] < S_:
            checks.append(min(checks[-1] + st, S_))
        for max_above in sorted(set(A.values()) | {0, h * w}):
            got = restated_until(L, S_, mn, st, 0.2, 0.02, max_above, sample_begin=begin)
            stop = next((n for n in checks if A[n] <= max_above), S_)
            assert got["samples_done"] == stop, (mn, st, begin, max_above)
            k = checks.index(stop)
            assert got["above"] == [A[n] for n in checks[:k + 1]] and got["checks"] == k + 1
            assert got["passes"] == k + (1 if begin < mn else 0) and got["paths"] == h * w * (stop - begin)
            assert got["last"] == restated_frame_error(L, S_, stop, 0.2, 0.02)
    assert restated_until(L, S_, 3, 5, np.inf, 0.02, 0)["samples_done"] == 3
    assert restated_until(L, S_, 3, 5, 0.0, 0.02, 0)["samples_done"] == S_


def test_host_check_passes_plain_and_sanitised_with_the_same_bytes(tmp_path):
    """tools/frame_error_host_check.cpp: the kernel text on the host against a plain restatement in the program; nothing is preloaded"""
    out = []
    for name, mode in (("plain", HP.PLAIN), ("sanitised", HP.SANITISED)):
        exe = HP.build("frame_error_host_check.cpp", str(tmp_path / ("frame_error_host_check_" + name)), mode, ["-pthread"])
        path = str(tmp_path / (name + ".bin"))
        rc, stdout, err = HP.run(exe, [path], timeout=600)
        assert rc == 0, stdout[-2000:] + err
        assert stdout.splitlines()[-1] == "53 cases, 0 failures", stdout[-2000:]
        out.append(open(path, "rb").read())
    assert out[0] == out[1] and len(out[0]) == 53 * C.sizeof(capi.FrameErrorInfo)


# ------------------------------------------------------------------------------------------------------------------ GPU --

def progressive_checks(r, name, w, h, spp, mid, traversal=crt.TRAVERSAL_EXACT, settings=((None, None), (0.3, 0.0))):
    """A frame in two ranges on handle r with a summary after each, against the restatement; the summary in between changes no bit of
    what follows (the preview's and the final frame's bits are the oracle's)"""
    orgb, omean, L = oracle_frame(name, w, h, spp)
    cam = util.camera(name)
    d = crt.frame_error_defaults()
    r.set_spp(spp)
    r.traversal = traversal
    try:
        kw = dict(width=w, height=h, want_variance=True)
        assert r.run_view_range(*cam, 0, mid, **kw) is None
        for n in (mid, spp):
            if n == spp:
                rgb = r.run_view_range(*cam, mid, spp - mid, **kw)
                assert np.array_equal(rgb, orgb), "the final frame after a summary in between"
                assert_bits(r.mean_buffer, omean, "the final mean after a summary in between")
                assert_bits(r.variance(width=w, height=h)[0], restated_variance(L, spp), "the final variance")
            for thr, floor in settings:
                got = r.frame_error(threshold=thr, mean_floor=floor)
                want = restated_frame_error(L, spp, n, d["threshold"] if thr is None else thr, d["mean_floor"] if floor is None else floor)
                check_summary(got.as_dict(), want, "%s %dx%d n %d threshold %r" % (name, w, h, n, thr))
                assert got.pixels == w * h and got.fraction_above == want["above"] / (w * h)
            if n == mid:
                pm = r.preview(want_mean=True, width=w, height=h)[1]
                c, _ = restated_sums(L, spp, mid)
                assert_bits(pm, c * (F(spp) / F(mid)), "the preview after a summary")
    finally:
        r.traversal = crt.TRAVERSAL_EXACT


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_frame_error_matches_restatement_on_the_oracles_radiance(renders, shape):
    progressive_checks(renders["cornell-box"], "cornell-box", shape[0], shape[1], S, MID)


@pytest.mark.gpu
def test_frame_error_with_two_partials_per_finishing_lane(renders):
    progressive_checks(renders["cornell-box"], "cornell-box", 160, 120, 4, 2, settings=((None, None),))   # 75 blocks


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", ["4", "2"])
@pytest.mark.parametrize("traversal", [crt.TRAVERSAL_EXACT, crt.TRAVERSAL_REFERENCE])
def test_frame_error_on_both_scenes_traversals_and_pipelines(renders, traversal, pipeline, monkeypatch):
    monkeypatch.setenv("CRT_PIPELINE", pipeline)
    progressive_checks(renders["veach-mis"], "veach-mis", 17, 15, S, MID, traversal=traversal, settings=((None, None),))


def tiled_range(r, name, prm, begin, count, slots):
    """crt_render_range of a tiled shard; (rgb, mean) of the range that ends at spp"""
    cam = r._cam(*util.camera(name))
    last = begin + count == prm.spp
    rgb, mean = (np.zeros((slots, 3), dtype=np.uint8), np.zeros((slots, 3), dtype=F)) if last else (None, None)
    capi.check(capi.lib().crt_render_range(r._h, C.byref(cam), C.byref(prm), begin, count, capi.ptr(rgb), capi.ptr(mean), None), "crt_render_range")
    return rgb, mean


@pytest.mark.gpu
def test_frame_error_of_a_tiled_shard_leaves_the_padding_out(renders):
    name, w, h, rank, world = "cornell-box", 61, 47, 1, 3
    r = renders[name]
    _, omean, L = oracle_frame(name, w, h, S)
    j, i, valid = shard_slots_of(w, h, rank, world)
    assert 0 < valid.sum() < valid.size and valid.size == crt.shard_slots(w, h, rank, world)
    r.set_spp(S)
    prm = r._params(rank=rank, world=world, flags=capi.FLAG_TILED_OUTPUT | capi.FLAG_VARIANCE, width=w, height=h)
    tiled_range(r, name, prm, 0, MID, valid.size)
    check_summary(r.frame_error().as_dict(), restated_frame_error(L, S, MID, 0.05, 0.01, rank, world), "mid-flight")
    _, mean = tiled_range(r, name, prm, MID, S - MID, valid.size)
    assert_bits(mean[valid], omean[j[valid], i[valid]], "the shard's final mean")
    got = r.frame_error(threshold=0.3)
    check_summary(got.as_dict(), restated_frame_error(L, S, S, 0.3, 0.01, rank, world), "finished")
    assert got.pixels == valid.sum() == crt.api.shard_pixels(w, h, rank, world)


@pytest.mark.gpu
def test_frame_error_device_form_on_a_stream_matches_host_form(renders):
    name, w, h = "veach-mis", 64, 48
    r = renders[name]
    cam = util.camera(name)
    r.set_spp(S)
    assert r.run_view_range(*cam, 0, MID, width=w, height=h, want_variance=True) is None
    host = r.frame_error(threshold=0.2).as_dict()
    with DeviceBuffers({"info": C.sizeof(capi.FrameErrorInfo)}, stream=True) as d:
        r.frame_error_device(d.ptrs["info"], threshold=0.2, stream=d.stream)
        d.synchronize()
        raw = d.download("info", (C.sizeof(capi.FrameErrorInfo),), np.uint8)
    dev = capi.FrameErrorInfo.from_buffer_copy(raw.tobytes()).as_dict()
    check_summary(dev, {k: host[k] for k in FIELDS}, "device form")
    _, _, L = oracle_frame(name, w, h, S)
    check_summary(dev, restated_frame_error(L, S, MID, 0.2, 0.01), "device form against the restatement")
    # what a caller reads from it
    e = r.frame_error(threshold=0.2)
    assert e.rel_rmse == math.sqrt(e.sum_variance / e.pixels) / (e.sum_mean / e.pixels + e.mean_floor) and 0 < e.rel_rmse < 10
    cum = np.cumsum(e.hist)
    for p in (0, 10, 50, 90, 100):
        k = int(np.argmax(cum >= math.ceil(e.pixels * p / 100.0))) if cum[-1] >= math.ceil(e.pixels * p / 100.0) else 15
        assert e.percentile_ratio(p) == (4.0 ** (k - 7) if k < 15 else math.inf), p
    assert e.percentile_ratio(0) == 4.0 ** -7
    assert r.run_view_range(*cam, MID, S - MID, width=w, height=h, want_variance=True) is not None


@pytest.mark.gpu
def test_frame_error_refuses_what_crt_variance_refuses():
    name, w, h = "cornell-box", 9, 7
    r = fresh_render(name, S)
    try:
        cam = util.camera(name)

        def refused(word):
            with pytest.raises(crt.CrtError) as e:
                r.frame_error()
            assert e.value.status == capi.ERR_INVALID_ARG and str(e.value).count("crt_frame_error: ") == 1 and word in str(e.value), str(e.value)
        refused("CRT_FLAG_VARIANCE")                                  # nothing rendered yet
        r.run_view(*cam, width=w, height=h)
        refused("CRT_FLAG_VARIANCE")                                  # a frame without the flag
        r.run_view_range(*cam, 0, 1, width=w, height=h, want_variance=True)
        refused("fewer than 2 samples")
        r.run_view_range(*cam, 1, 1, width=w, height=h, want_variance=True)
        assert r.frame_error().samples_done == 2
        r.run_view_range(*cam, 2, 1, width=w, height=h)              # a range without the flag ends the sums' validity
        refused("CRT_FLAG_VARIANCE")
        assert r.preview(width=w, height=h)[2] == 3                   # and the refusals left the frame in flight
    finally:
        r.free()


@functools.lru_cache(maxsize=None)
def until_case(name, rank=0, world=1):
    """(L, max_above, the restated call) of the until frame of a scene: max_above is the restated `above` at the third check, and the
    restated call must then stop inside (4, 32) -- a condition on the inputs, asserted here"""
    _, _, L = oracle_frame(name, UW, UH, US)
    seq = restated_until(L, US, max_above=0, rank=rank, world=world, **dict(UNTIL, threshold=UNTIL["threshold"]))["above"]
    max_above = seq[2]
    want = restated_until(L, US, max_above=max_above, rank=rank, world=world, **UNTIL)
    assert 4 < want["samples_done"] < US, (name, seq)
    assert want["above"] == seq[:want["checks"]]
    return L, max_above, want


def check_until_info(info, want, where):
    for f in ("samples_done", "passes", "checks", "above", "paths"):
        assert info[f] == want[f], "%s: %s is %r, expected %r" % (where, f, info[f], want[f])
    check_summary(info["last"].as_dict(), want["last"], where + ": the last summary")
    assert info["total_ms"] > 0 and 0 <= info["kernel_ms"] <= info["total_ms"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_until_stops_where_the_restatement_stops_and_leaves_the_frame_in_flight(renders, name):
    L, max_above, want = until_case(name)
    orgb, omean, _ = oracle_frame(name, UW, UH, US)
    r = renders[name]
    cam = util.camera(name)
    kw = dict(width=UW, height=UH)
    r.set_spp(US)
    rgb = r.run_view_until(*cam, max_above=max_above, want_variance=True, **UNTIL, **kw)
    n = want["samples_done"]
    check_until_info(r.until_info, want, name)
    assert r.until_info["kernel_ms"] > 0
    mean, var = r.mean_buffer.copy(), r.variance_buffer.copy()
    # the outputs: crt_preview's and crt_variance's of a separate handle ranged to n
    r2 = fresh_render(name, US)
    try:
        assert r2.run_view_range(*cam, 0, n, want_variance=True, **kw) is None
        prgb, pmean, done = r2.preview(want_mean=True, **kw)
        assert done == n and np.array_equal(rgb, prgb)
        assert_bits(mean, pmean, "out_mean against crt_preview")
        assert_bits(var, r2.variance(**kw)[0], "out_variance against crt_variance")
    finally:
        r2.free()
    assert_bits(var, restated_variance(L, US, n), "out_variance against the restatement")
    # the handle still previews, and a fraction is a pixel count
    prgb, _, done = r.preview(**kw)
    assert done == n and np.array_equal(prgb, rgb)
    again = r.run_view_until(*cam, max_above=(max_above + 0.5) / (UW * UH), sample_begin=n, **UNTIL, **kw)   # met already: one check, nothing rendered
    assert np.array_equal(again, rgb) and r.until_info["passes"] == 0 and r.until_info["above"] == [want["above"][-1]] and r.until_info["samples_done"] == n
    # a stricter target continues the frame: threshold 0 runs to S, and the frame is crt_render's
    rgb = r.run_view_until(*cam, sample_begin=n, max_above=0, want_variance=True, **dict(UNTIL, threshold=0.0), **kw)
    info = r.until_info
    assert info["samples_done"] == US and info["passes"] == (US - n) // 4 and info["checks"] == info["passes"] + 1 and info["paths"] == UW * UH * (US - n)
    assert np.array_equal(rgb, orgb)
    assert_bits(r.mean_buffer, omean, "run to S: crt_render's mean")
    assert_bits(r.variance_buffer, restated_variance(L, US), "run to S: crt_variance")
    check_summary(info["last"].as_dict(), restated_frame_error(L, US, US, 0.0, 0.01), "run to S: the last summary")
    with pytest.raises(crt.CrtError):                                  # the frame is finished
        r.preview(**kw)


@pytest.mark.gpu
def test_until_limits_and_refusals(renders):
    name = "cornell-box"
    L, max_above, want = until_case(name)
    r = renders[name]
    cam = util.camera(name)
    kw = dict(width=UW, height=UH)
    r.set_spp(US)
    # threshold +inf: the first check passes
    rgb = r.run_view_until(*cam, **dict(UNTIL, threshold=np.inf), **kw)
    info = r.until_info
    assert info["samples_done"] == 4 and info["passes"] == 1 and info["above"] == [0] and info["paths"] == UW * UH * 4
    c, _ = restated_sums(L, US, 4)
    assert_bits(r.mean_buffer, c * (F(US) / F(4)), "threshold +inf: crt_preview's mean at min_samples")
    assert np.array_equal(rgb, O.tonemap(r.mean_buffer))
    # a sample_begin below min_samples renders up to it first
    r.run_view_range(*cam, 0, 2, want_variance=True, **kw)
    r.run_view_until(*cam, sample_begin=2, max_above=max_above, **UNTIL, **kw)
    assert r.until_info["samples_done"] == want["samples_done"] and r.until_info["above"] == want["above"]
    assert r.until_info["paths"] == UW * UH * (want["samples_done"] - 2) and r.until_info["passes"] == want["passes"]
    # refused: a sample_begin that is not the frame's, sums without the flag -- and the handle is as it was
    n = want["samples_done"]
    for begin in (n - 1, n + 1):
        with pytest.raises(crt.CrtError) as e:
            r.run_view_until(*cam, sample_begin=begin, **UNTIL, **kw)
        assert e.value.status == capi.ERR_INVALID_ARG and "crt_render_until: sample_begin" in str(e.value)
    with pytest.raises(crt.CrtError):
        r.run_view_until(*cam, sample_begin=n, **dict(UNTIL, min_samples=1), **kw)
    assert r.preview(**kw)[2] == n and r.frame_error().samples_done == n
    r.run_view_range(*cam, n, 1, **kw)                                 # a range without the flag
    with pytest.raises(crt.CrtError) as e:
        r.run_view_until(*cam, sample_begin=n + 1, **UNTIL, **kw)
    assert "without valid variance sums" in str(e.value) and r.preview(**kw)[2] == n + 1
    # min_samples == spp: the uniform frame in one range, one check
    orgb, omean, _ = oracle_frame(name, UW, UH, US)
    rgb = r.run_view_until(*cam, **dict(UNTIL, min_samples=US), **kw)
    assert np.array_equal(rgb, orgb) and r.until_info["passes"] == 1 and r.until_info["checks"] == 1 and r.until_info["samples_done"] == US
    assert_bits(r.mean_buffer, omean, "min_samples == spp")


@pytest.mark.gpu
def test_until_on_a_tiled_shard(renders):
    name, rank, world = "veach-mis", 1, 3
    L, max_above, want = until_case(name, rank, world)
    r = renders[name]
    r.set_spp(US)
    j, i, valid = shard_slots_of(UW, UH, rank, world)
    slots = valid.size
    rgb, mean, var = np.full((slots, 3), 7, dtype=np.uint8), np.full((slots, 3), 7, dtype=F), np.full((slots, 3), 7, dtype=F)
    cam = r._cam(*util.camera(name))
    prm = r._params(rank=rank, world=world, flags=capi.FLAG_TILED_OUTPUT, width=UW, height=UH)
    up = capi.UntilParams(UNTIL["min_samples"], UNTIL["step_samples"], UNTIL["threshold"], UNTIL["mean_floor"], max_above)
    info = capi.UntilInfo()
    capi.check(capi.lib().crt_render_until(r._h, C.byref(cam), C.byref(prm), C.byref(up), 0, capi.ptr(rgb), capi.ptr(mean), capi.ptr(var), C.byref(info)),
               "crt_render_until")
    got = crt.api._until_info(info, up)
    check_until_info(got, want, "rank 1 of 3")
    n = want["samples_done"]
    c, _ = restated_sums(L, US, n)
    assert_bits(mean, (c * (F(US) / F(n)))[j, i], "the shard's mean: crt_preview's")
    assert np.array_equal(rgb, O.tonemap(mean))
    assert_bits(var, restated_variance(L, US, n)[j, i], "the shard's variance")
    assert r.frame_error(threshold=UNTIL["threshold"]).above == want["above"][-1]


@pytest.mark.gpu
def test_until_device_form_on_a_stream_and_half_buffers(renders):
    name = "veach-mis"
    L, max_above, want = until_case(name)
    r = renders[name]
    cam = util.camera(name)
    kw = dict(width=UW, height=UH)
    r.set_spp(US)
    host_rgb = r.run_view_until(*cam, max_above=max_above, want_variance=True, want_halves=True, **UNTIL, **kw).copy()
    host_mean, host_var = r.mean_buffer.copy(), r.variance_buffer.copy()
    check_until_info(r.until_info, want, "with the half buffers")
    n = want["samples_done"]
    a, b, done = r.half_buffers(**kw)
    assert done == n
    r2 = fresh_render(name, US)
    try:
        for s0 in range(0, n, 4):
            r2.run_view_range(*cam, s0, 4, want_halves=True, **kw)
        a2, b2, done2 = r2.half_buffers(**kw)
        assert done2 == n
        assert_bits(a, a2, "half A against plain ranges")
        assert_bits(b, b2, "half B against plain ranges")
    finally:
        r2.free()
    with DeviceBuffers({"rgb": UW * UH * 3, "mean": UW * UH * 12, "variance": UW * UH * 12}, stream=True) as d:
        info = r.run_view_until_device(*cam, d.ptrs, max_above=max_above, stream=d.stream, **UNTIL, **kw)
        d.synchronize()
        check_until_info(info, want, "device form")
        assert np.array_equal(d.download("rgb", (UH, UW, 3), np.uint8), host_rgb)
        assert_bits(d.download("mean", (UH, UW, 3)), host_mean, "device form: mean")
        assert_bits(d.download("variance", (UH, UW, 3)), host_var, "device form: variance")
        # without info and without the optional outputs
        d.fill("rgb")
        assert r.run_view_until_device(*cam, {"rgb": d.ptrs["rgb"]}, max_above=max_above, stream=d.stream, want_info=False, **UNTIL, **kw) is None
        d.synchronize()
        assert np.array_equal(d.download("rgb", (UH, UW, 3), np.uint8), host_rgb)
        assert r.preview(**kw)[2] == n


@pytest.mark.gpu
def test_cli_and_cpp_render_to_the_target_with_the_librarys_n_and_bytes(renders, tmp_path):
    """crt_cli --until and crt::Render::run_view_until / frame_error (tools/until_host_check.cpp, a stand-alone program beside crt_cli)
    against Render.run_view_until: the same samples done, the same frame and mean."""
    from cudaraytracing_amd import build as b
    name = "cornell-box"
    L, max_above, want = until_case(name)
    r = renders[name]
    cam = util.camera(name)
    r.set_spp(US)
    rgb = r.run_view_until(*cam, max_above=max_above, want_variance=True, width=UW, height=UH, **UNTIL).copy()
    mean, var, n = r.mean_buffer.copy(), r.variance_buffer.copy(), r.until_info["samples_done"]
    assert n == want["samples_done"]
    ref = str(tmp_path / "python.png")
    r.save_frame_buffer(ref)
    # the C++ class
    out = str(tmp_path / "until.bin")
    res = subprocess.run([b.build_until_check(), util.SCENES[name], util.ROOT, repr(UNTIL["threshold"]), str(max_above), str(UNTIL["min_samples"]),
                          str(UNTIL["step_samples"]), out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.stdout + res.stderr)[-2000:]
    assert res.stdout.strip() == "until_host_check: ok, %d samples" % n
    raw = open(out, "rb").read()
    assert len(raw) == 4 + UW * UH * 15 and struct.unpack("<I", raw[:4])[0] == n
    assert np.array_equal(np.frombuffer(raw, np.uint8, UW * UH * 3, 4).reshape(UH, UW, 3), rgb)
    assert_bits(np.frombuffer(raw, "<f4", UW * UH * 3, 4 + UW * UH * 3).reshape(UH, UW, 3), mean, "crt::Render::run_view_until: mean")
    # the command line: a fraction of the pixels, to more digits than a pixel needs
    cli = b.build_cli()
    png, vpfm = str(tmp_path / "until.png"), str(tmp_path / "var.pfm")
    base = [cli, util.SCENES[name], "--spp", str(US), "--width", str(UW), "--height", str(UH), "--seed", "0", "--base-dir", util.ROOT]
    spec = "%r,%.9f,%d,%d" % (UNTIL["threshold"], (max_above + 0.5) / (UW * UH), UNTIL["min_samples"], UNTIL["step_samples"])
    res = subprocess.run(base + ["-o", png, "--until", spec, "--variance", vpfm], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert "until: %d of %d samples in %d ranges, %d checks" % (n, US, want["passes"], want["checks"]) in res.stdout, res.stdout
    assert "until: %d of %d pixels above the target (%d allowed, 0 NaN)" % (want["above"][-1], UW * UH, max_above) in res.stdout, res.stdout
    assert "until: hist " + " ".join(str(k) for k in want["last"]["hist"]) in res.stdout, res.stdout
    assert open(png, "rb").read() == open(ref, "rb").read()
    assert_bits(util.read_pfm(vpfm)[1], var, "--variance of the frame in flight")
    for extra, word in ((["--until", "x"], "--until"), (["--until", "0.1,1.5"], "--until"), (["--until", "0.1", "--adaptive", "0.1"], "--until"),
                        (["--until", "0.1", "--devices", "0,0", "--gather", "copy"], "--until")):
        bad = subprocess.run([cli, util.SCENES[name]] + extra, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and word in bad.stderr, (extra, bad.stderr)
