"""Multi-scale denoising: crt_pyramid_down / crt_pyramid_merge and their _device forms (contract: include/crt.h), pyramid_down,
pyramid_merge, denoise_multiscale and Render.run_view_denoised(scales=...) in Python, crt_cli --denoise-scales.

The two contracts are restated in numpy float32, operation by operation, in tests/pyramid_restated.py; the device result must match it
bit for bit from both forms of the merge kernel (CRT_PYRAMID_FORM=direct|staged).  Comparisons are on uint32 views; where the expected
value is NaN the result must be NaN (payload not compared).  The kernels' text also runs on the host (tools/pyramid_host_check.cpp), plain
and under the sanitizers, as a stand-alone program.
"""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import host_program as HP
import oracle_lib as O
import pyramid_restated as PR
import util

F = np.float32
assert_bits = util.assert_bits
EXPORTS = ("crt_pyramid_size", "crt_pyramid_down", "crt_pyramid_down_device", "crt_pyramid_merge", "crt_pyramid_merge_device")
PYTHON_CALLS = ("pyramid_size", "pyramid_down", "pyramid_down_device", "pyramid_merge", "pyramid_merge_device", "denoise_multiscale")
FORMS = ("direct", "staged")
PLANES = ("variance", "albedo", "normal", "depth")
# 1 x 1 and 2 x 2; 3 x 5: odd in both directions; 33 x 9: one column and one row past a 32 x 8 merge tile, odd; 65 x 17: two tile
# borders, coarse sizes 33 x 9; 70 x 19
SIZES = [(1, 1), (2, 2), (3, 5), (33, 9), (65, 17), (70, 19)]
HOST_CHECK_SUMMARY = "336 cases, 0 failures; the largest tile: 1296 bytes of LDS"


# ------------------------------------------------------------------------------------------------------------------ inputs --

def synthetic(w, h, seed, special=False):
    """Random colour, variance and guides; a fifth of the depth plane are misses (0), with whole 2 x 2 groups among them.
    special: NaN, +-inf, +-1e30 and -0 scattered in every buffer."""
    rng = np.random.default_rng(seed)
    color = (rng.random((h, w, 3)) * 40).astype(F)
    variance = (rng.random((h, w, 3)) * 3).astype(F)
    n = rng.normal(size=(h, w, 3))
    normal = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(F)
    albedo = rng.random((h, w, 3)).astype(F)
    depth = (F(1.0) + rng.random((h, w)) * 49).astype(F)
    depth[rng.random((h, w)) < 0.2] = 0.0
    depth[:2, :2] = 0.0
    if special:
        values = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0], dtype=F)
        for j, im in enumerate((color, variance, albedo, normal, depth)):
            flat = im.reshape(-1)
            idx = rng.permutation(flat.size)[:max(6, flat.size // 10)]
            flat[idx] = values[(np.arange(idx.size) + j) % values.size]
    return {"color": color, "variance": variance, "albedo": albedo, "normal": normal, "depth": depth}


@pytest.fixture(scope="module")
def cases():
    """{(w, h): (planes, RR.down of all of them, a coarse image, RR.merge(colour, coarse))}: each restatement computed once"""
    out = {}
    for w, h in SIZES:
        planes = synthetic(w, h, 100 + w)
        w2, h2 = PR.low_size(w, h)
        coarse = synthetic(w2, h2, 200 + w)["color"]
        out[(w, h)] = (planes, PR.down(**planes), coarse, PR.merge(planes["color"], coarse))
    return out


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_pyramid_entry_points_are_exported():
    lib = capi.lib()
    for name in EXPORTS:
        assert name in capi.EXPORTS
        assert getattr(lib, name) is not None
    for name in PYTHON_CALLS:
        assert name in crt.__all__ and callable(getattr(crt, name))
    assert lib.crt_abi_version() == 5 == capi.ABI_VERSION          # only entry points were added
    for (w, h), want in (((1, 1), (1, 1)), ((2, 2), (1, 1)), ((3, 5), (2, 3)), ((800, 600), (400, 300)), ((1 << 24, 7), (1 << 23, 4))):
        assert crt.pyramid_size(w, h) == want == PR.low_size(w, h)
    a, b = C.c_uint32(), C.c_uint32()
    for bad in ((0, 7, C.byref(a), C.byref(b)), (7, 0, C.byref(a), C.byref(b)), (7, 7, None, C.byref(b)), (7, 7, C.byref(a), None)):
        assert lib.crt_pyramid_size(*bad) == capi.ERR_INVALID_ARG and lib.crt_last_error().startswith(b"crt_pyramid_size: ")
    assert "scales" in crt.Render.run_view_denoised.__code__.co_varnames


class _NoHandle:
    """stands in for a Render whose argument checks are all that runs"""
    def _handle(self, who):
        pass


def test_pyramid_arguments_are_checked_before_any_device_call():
    """Every refusal of the contract is CRT_ERR_INVALID_ARG with a message that starts with the entry point's name, from all four entry
    points, also on a machine without a GPU.  The non-null buffers here are host memory that must never be dereferenced (a device call
    would fault on them)."""
    lib = capi.lib()
    buf = np.zeros(64, dtype=F)
    d = C.c_void_p((buf.ctypes.data + 15) & ~15)
    w, h = 65, 17

    def params(**over):
        p = capi.PyramidParams(w, h, 33, 9)
        for k, v in over.items():
            setattr(p, k, v)
        return C.byref(p)

    def planes(**over):
        s = capi.PyramidPlanes(d, d, d, d, d)
        for k, v in over.items():
            setattr(s, k, v)
        return C.byref(s)

    def down(prm, inp, out, device=0, want=capi.ERR_INVALID_ARG):
        r1 = lib.crt_pyramid_down(device, prm, inp, out, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_pyramid_down_device(device, prm, inp, out, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == want, (r1, r2, e1, e2)
        assert e1.startswith(b"crt_pyramid_down: ") and e2.startswith(b"crt_pyramid_down_device: "), (e1, e2)
        return e1

    def merge(prm, fine=d, coarse=d, color=d, rgb=d, device=0, want=capi.ERR_INVALID_ARG):
        r1 = lib.crt_pyramid_merge(device, prm, fine, coarse, color, rgb, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_pyramid_merge_device(device, prm, fine, coarse, color, rgb, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == want, (r1, r2, e1, e2)
        assert e1.startswith(b"crt_pyramid_merge: ") and e2.startswith(b"crt_pyramid_merge_device: "), (e1, e2)
        return e1

    assert b"null" in down(None, planes(), planes()) and b"null" in down(params(), None, planes()) and b"null" in down(params(), planes(), None)
    assert b"colour" in down(params(), planes(color=None), planes()) and b"colour" in down(params(), planes(), planes(color=None))
    assert b"null" in merge(None) and b"null" in merge(params(), fine=None) and b"null" in merge(params(), coarse=None)
    for bad in (dict(width=0), dict(height=0)):
        assert b"positive" in down(params(**bad), planes(), planes()) and b"positive" in merge(params(**bad))
    for bad in (dict(low_width=32), dict(low_width=34), dict(low_height=8), dict(low_height=10), dict(low_width=0), dict(low_width=65, low_height=17)):
        assert b"coarse size" in down(params(**bad), planes(), planes()), bad
        assert b"coarse size" in merge(params(**bad)), bad
    for name in PLANES:
        assert b"plane" in down(params(), planes(**{name: None}), planes())
        assert b"plane" in down(params(), planes(), planes(**{name: None}))
    assert b"no output" in merge(params(), color=None, rgb=None)
    big = dict(width=(1 << 24) + 1, low_width=(1 << 23) + 1)
    assert b"2^24" in down(params(**big), planes(), planes(), want=capi.ERR_UNSUPPORTED) and b"2^24" in merge(params(**big), want=capi.ERR_UNSUPPORTED)
    assert b"device" in down(params(), planes(), planes(), device=-1) and b"device" in merge(params(), device=-1)
    assert not buf.any()
    # the Python layer's own
    img = np.zeros((6, 8, 3), dtype=F)
    with pytest.raises(ValueError):
        crt.pyramid_down(np.zeros((6, 8), dtype=F))
    with pytest.raises(ValueError):
        crt.pyramid_down(img, depth=np.zeros((6, 9), dtype=F))
    with pytest.raises(ValueError):
        crt.pyramid_merge(img, np.zeros((3, 5, 3), dtype=F))
    with pytest.raises(ValueError):
        crt.pyramid_down_device(8, 6, {"colour": 1}, {"color": 1})
    with pytest.raises(ValueError, match="variance"):
        crt.denoise_multiscale(img, None)
    with pytest.raises(ValueError, match="filter"):
        crt.denoise_multiscale(img, img, filter="atrous")
    for bad in (0, 5, 2.5, True, -1):
        with pytest.raises(ValueError, match="scales"):
            crt.denoise_multiscale(img, img, scales=bad)
        with pytest.raises(ValueError, match="scales"):
            crt.Render.run_view_denoised(_NoHandle(), None, None, None, nlm=True, scales=bad)
    for scales in (2, 3, 4):
        with pytest.raises(ValueError, match="scales needs"):
            crt.Render.run_view_denoised(_NoHandle(), None, None, None, scales=scales)


@pytest.mark.parametrize("w,h", SIZES)
def test_restated_merge_of_the_reduced_image_is_the_image(w, h):
    """coarse = D(fine): every detail is +-0, so the merge returns fine's values"""
    fine = synthetic(w, h, 7)["color"]
    assert np.array_equal(PR.merge(fine, PR.down_plane(fine)), fine)


@pytest.mark.parametrize("w,h", SIZES)
def test_restatement_keeps_a_constant_image_constant(w, h):
    c = np.full((h, w, 3), 0.7, dtype=F) * np.array([1, 2, 3], dtype=F)
    low = PR.down_plane(c)
    w2, h2 = PR.low_size(w, h)
    assert low.shape == (h2, w2, 3) and np.array_equal(low, np.broadcast_to(c[0, 0], low.shape))   # (x + x) / 2 and ((x + x) + x + x) / 4 are exact
    assert np.array_equal(PR.merge(c, low), c)
    # a constant correction is added as it is: the tent weights sum to sden, and (d * a + d * b) / (a + b) stays within rounding of d
    shifted = PR.merge(c, low + F(0.25))
    assert np.abs(shifted - (c + F(0.25))).max() <= 4 * np.spacing(F(2.35))


def test_restated_variance_of_a_constant_variance_image():
    """v / n with n = 4 / 2 / 1 at the interior / an edge / the corner of an odd-sized image"""
    v = F(0.6)
    low = PR.down_plane(np.full((5, 7, 3), v, dtype=F), "variance")
    assert low.shape == (3, 4, 3)
    assert (low[:2, :3] == v / F(4)).all() and (low[2, :3] == v / F(2)).all() and (low[:2, 3] == v / F(2)).all() and (low[2, 3] == v).all()
    assert np.array_equal(PR.down_plane(np.full((4, 6, 3), v, dtype=F), "variance"), np.full((2, 3, 3), v / F(4), dtype=F))


def test_restated_depth_is_the_mean_of_the_hits():
    depth = np.array([[2, 0, 0, 0, 5],
                      [4, 6, 0, 0, 0],
                      [0, 3, np.nan, 8, 0]], dtype=F)
    low = PR.down_plane(depth, "depth")
    assert_bits(low, np.array([[4, 0, 5], [3, 8, 0]], dtype=F), "depth")     # (2 + 4 + 6) / 3; no hit: 0; NaN is no hit
    assert not np.signbit(low).any()


@pytest.fixture(scope="module")
def host_check_run(tmp_path_factory):
    """both builds of tools/pyramid_host_check.cpp, each run as `program - out`: [(status, bytes, printed) plain, sanitised]"""
    return HP.run_both_forms("pyramid_host_check.cpp", str(tmp_path_factory.mktemp("pyramid_host")), "-")


def test_kernel_text_on_the_host_passes_its_checks(host_check_run):
    """csrc/crt_pyramid.h on crt_upsample.h as they are, compiled with g++ -ffp-contract=off: down with every combination of planes, both
    forms of the merge, against the program's own plain restatement; the summary line carries the case count"""
    rc, raw, printed = host_check_run[0]
    assert rc == 0, printed
    assert printed.splitlines()[-1] == HOST_CHECK_SUMMARY, printed
    assert len(raw) > 0


def test_kernel_text_is_clean_under_the_sanitizers(host_check_run):
    """the same stand-alone program built with -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all (nothing is
    preloaded): exit status 0, the same summary and the same bytes -- no LDS or image index outside its array (each has exactly its size)"""
    rc, raw, printed = host_check_run[1]
    assert rc == 0, printed
    assert printed.splitlines()[-1] == HOST_CHECK_SUMMARY, printed
    assert raw == host_check_run[0][1]


# ------------------------------------------------------------------------------------------------------------------ GPU --

def check_down(planes, want, where):
    got = crt.pyramid_down(**planes)
    assert sorted(got) == sorted(want), where
    for name in want:
        assert_bits(got[name], want[name], "%s: %s" % (where, name))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_down_matches_restatement_with_every_combination_of_planes(cases, w, h):
    planes, want, _, _ = cases[(w, h)]
    for r in range(len(PLANES) + 1):
        for given in itertools.combinations(PLANES, r):
            names = ("color",) + given
            check_down({n: planes[n] for n in names}, {n: want[n] for n in names}, "%dx%d %r" % (w, h, given))


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("w,h", SIZES)
def test_merge_forms_match_restatement(cases, monkeypatch, form, w, h):
    """CRT_PYRAMID_FORM is read per call: each form against the restatement, so the two against each other"""
    planes, _, coarse, want = cases[(w, h)]
    monkeypatch.setenv("CRT_PYRAMID_FORM", form)
    rgb, mean = crt.pyramid_merge(planes["color"], coarse)
    assert_bits(mean, want, "%s %dx%d" % (form, w, h))
    assert np.array_equal(rgb, O.tonemap(want))
    rgb, mean = crt.pyramid_merge(planes["color"], coarse, want_mean=False)
    assert mean is None and np.array_equal(rgb, O.tonemap(want))
    rgb, mean = crt.pyramid_merge(planes["color"], coarse, want_rgb=False)
    assert rgb is None
    assert_bits(mean, want, "%s %dx%d without rgb" % (form, w, h))
    # coarse = D(fine): fine's values come back
    _, same = crt.pyramid_merge(planes["color"], crt.pyramid_down(planes["color"])["color"], want_rgb=False)
    assert np.array_equal(same, planes["color"])


@pytest.mark.gpu
def test_an_unknown_form_is_refused(cases, monkeypatch):
    planes, _, coarse, _ = cases[(3, 5)]
    monkeypatch.setenv("CRT_PYRAMID_FORM", "neither")
    with pytest.raises(Exception, match="CRT_PYRAMID_FORM"):
        crt.pyramid_merge(planes["color"], coarse)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("w,h", [(3, 5), (33, 9), (70, 19)])
def test_non_finite_values_in_every_buffer(monkeypatch, form, w, h):
    """NaN, +-inf, +-1e30 and -0 scattered in every buffer: the arithmetic defines the result"""
    monkeypatch.setenv("CRT_PYRAMID_FORM", form)
    planes = synthetic(w, h, 300 + w, special=True)
    assert all(not np.isfinite(x).all() for x in planes.values())
    check_down(planes, PR.down(**planes), "non-finite %dx%d" % (w, h))
    w2, h2 = PR.low_size(w, h)
    coarse = synthetic(w2, h2, 400 + w, special=True)["color"]
    want = PR.merge(planes["color"], coarse)
    rgb, mean = crt.pyramid_merge(planes["color"], coarse)
    assert_bits(mean, want, "non-finite merge %s %dx%d" % (form, w, h))
    assert np.array_equal(rgb, O.tonemap(want))
    assert np.isnan(want).any() and np.isfinite(want).any()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(70, 19), (131, 9)])
def test_depth_misses_on_tile_borders(w, h):
    """A workgroup reduces 64 x 4 coarse pixels (128 x 8 fine ones): misses along the fine rows and columns on either side of those
    borders, as whole lines, as single pixels of a 2 x 2 group and as whole groups"""
    planes = synthetic(w, h, 500 + w)
    depth = (F(1.0) + np.random.default_rng(w).random((h, w)) * 9).astype(F)
    depth[7:9, :] = 0.0                      # the fine rows on either side of the first row border
    depth[15 % h, ::2] = 0.0                # (row 6 of the 9-row image)
    depth[16 % h, 1::2] = 0.0
    for x in (126, 127, 128, 129, 63, 64):   # the column border (131 wide), and the middle of a tile
        if x < w:
            depth[::3, x] = 0.0
    depth[0:2, 0:2] = 0.0
    depth[h - 1, w - 1] = 0.0               # the corner pixel of an odd-sized image: its only tap
    planes["depth"] = depth
    want = PR.down(**planes)
    assert (want["depth"] == 0).any() and (want["depth"] > 0).any()
    check_down(planes, want, "depth misses %dx%d" % (w, h))
    check_down({"color": planes["color"], "depth": depth}, {"color": want["color"], "depth": want["depth"]}, "depth alone %dx%d" % (w, h))


def textured_scene(tmp, w, h):
    sys.path.insert(0, os.path.join(util.ROOT, "scenes"))
    import gen_cornell_box
    obj, mtl_dir, _ = gen_cornell_box.write_textured_variant(tmp, 12)
    sc = crt.Scene(w, h)
    sc.add_obj(obj, mtl_dir)
    sc.set_BVH(util.task("cornell-box").bvh_thresh_n)
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis", "cornell-box-textured"])
def test_rendered_frame_with_its_guides(tmp_path, name):
    """one rendered 37 x 21 frame of each scene: its colour, variance and first-hit guides reduced, and the variance-guided filter's
    results at both sizes merged"""
    w, h = 37, 21
    base = "cornell-box" if name == "cornell-box-textured" else name
    t = util.task(base)
    eye, iv, fov = util.camera(base)
    scene = textured_scene(str(tmp_path), w, h) if name == "cornell-box-textured" else util.host_scene(name)
    r = crt.Render(scene, 4, t.P_RR, t.light_sample_n)
    try:
        r.run_view(eye, iv, fov, width=w, height=h, want_variance=True)
        planes = {"color": r.mean_buffer.copy(), "variance": r.variance_buffer.copy()}
        planes.update(r.run_view_aov(eye, iv, fov, want=("albedo", "normal", "depth"), width=w, height=h))
    finally:
        r.free()
    want = PR.down(**planes)
    check_down(planes, want, name)
    assert (want["variance"] > 0).any() and (want["depth"] > 0).any()
    fine = crt.denoise_var(want_rgb=False, **planes)[1]
    coarse = crt.denoise_var(want_rgb=False, **want)[1]
    merged = PR.merge(fine, coarse)
    rgb, mean = crt.pyramid_merge(fine, coarse)
    assert_bits(mean, merged, name + ": merge")
    assert np.array_equal(rgb, O.tonemap(merged))
    assert not np.array_equal(merged, fine)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_device_forms_on_a_stream(cases, monkeypatch, form):
    monkeypatch.setenv("CRT_PYRAMID_FORM", form)
    w, h = 65, 17
    w2, h2 = PR.low_size(w, h)
    planes, want, coarse, want_merge = cases[(w, h)]
    host = dict(planes, coarse=coarse)
    outs = {"out_" + n: w2 * h2 * (4 if n == "depth" else 12) for n in planes}
    outs.update(merged=w * h * 12, merged_rgb=w * h * 3)
    # (every output value must be written by the kernels: what is not uploaded is filled with 0x55)
    with DeviceBuffers({**host, **outs}, stream=True) as d:
        ptrs = d.ptrs
        assert crt.pyramid_down_device(w, h, {n: ptrs[n] for n in planes}, {n: ptrs["out_" + n] for n in planes}, stream=d.stream, want_info=False) is None
        assert crt.pyramid_merge_device(w, h, ptrs["color"], ptrs["coarse"], ptrs["merged"], ptrs["merged_rgb"], stream=d.stream, want_info=False) is None
        d.synchronize()
        for n in planes:
            assert_bits(d.download("out_" + n, (h2, w2) if n == "depth" else (h2, w2, 3), F), want[n], "device form: " + n)
        assert_bits(d.download("merged", (h, w, 3), F), want_merge, "device form: merge")
        assert np.array_equal(d.download("merged_rgb", (h, w, 3), np.uint8), O.tonemap(want_merge))
        # the colour alone and the RGB alone, with the info (the call synchronizes the stream)
        for n in outs:
            d.fill(n)
        info = crt.pyramid_down_device(w, h, {"color": ptrs["color"]}, {"color": ptrs["out_color"]}, stream=d.stream)
        assert info["total_ms"] > 0, info
        assert_bits(d.download("out_color", (h2, w2, 3), F), want["color"], "device form: colour alone")
        assert (d.download("out_depth", (h2, w2), np.uint32) == 0x55555555).all()
        info = crt.pyramid_merge_device(w, h, ptrs["color"], ptrs["coarse"], None, ptrs["merged_rgb"], stream=d.stream)
        assert info["total_ms"] > 0, info
        assert np.array_equal(d.download("merged_rgb", (h, w, 3), np.uint8), O.tonemap(want_merge))
        assert (d.download("merged", (h, w, 3), np.uint32) == 0x55555555).all()


def filter_call(name):
    return {"var": crt.denoise_var, "nlm": crt.denoise_nlm, "reg": crt.denoise_regress}[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["var", "nlm", "reg"])
def test_one_scale_is_the_single_filter(cases, name):
    planes, _, _, _ = cases[(33, 9)]
    want_rgb, want_mean = filter_call(name)(**planes)[:2]
    rgb, mean, info = crt.denoise_multiscale(filter=name, scales=1, return_info=True, **planes)
    assert_bits(mean, want_mean, name)
    assert np.array_equal(rgb, want_rgb)
    assert [c[:3] for c in info["calls"]] == [("denoise_" + name, 33, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,settings", [("var", {}), ("nlm", {"radius": 3}), ("reg", {"radius": 2, "ridge": 0.1})])
def test_three_scales_equal_the_calls_by_hand(cases, name, settings):
    """33 x 9 -> 17 x 5 -> 9 x 3: reduce twice, filter the three scales with the same settings, merge twice from the coarsest up"""
    l0, _, _, _ = cases[(33, 9)]
    call = filter_call(name)
    l1 = crt.pyramid_down(**l0)
    l2 = crt.pyramid_down(**l1)
    assert l2["color"].shape == (3, 9, 3)
    for got, want in ((l1, PR.down(**l0)), (l2, PR.down(**l1))):
        for n in want:
            assert_bits(got[n], want[n], n)
    f0, f1, f2 = (call(want_rgb=False, **settings, **l)[1] for l in (l0, l1, l2))
    m1 = crt.pyramid_merge(f1, f2, want_rgb=False)[1]
    want_rgb, want_mean = crt.pyramid_merge(f0, m1)
    assert_bits(want_mean, PR.merge(f0, PR.merge(f1, f2)), "the merges against the restatement")
    rgb, mean, info = crt.denoise_multiscale(filter=name, scales=3, return_info=True, **settings, **l0)
    assert_bits(mean, want_mean, name)
    assert np.array_equal(rgb, want_rgb) and np.array_equal(rgb, O.tonemap(want_mean))
    assert [c[:3] for c in info["calls"]] == [("pyramid_down", 33, 9), ("pyramid_down", 17, 5), ("denoise_" + name, 9, 3), ("denoise_" + name, 17, 5),
                                              ("pyramid_merge", 17, 5), ("denoise_" + name, 33, 9), ("pyramid_merge", 33, 9)]


@pytest.mark.gpu
def test_four_scales_reach_one_pixel():
    """8 x 5 -> 4 x 3 -> 2 x 2 -> 1 x 1: a scale may be as small as one pixel"""
    planes = synthetic(8, 5, 9)
    rgb, mean, info = crt.denoise_multiscale(filter="var", scales=4, return_info=True, **planes)
    assert [c[1:3] for c in info["calls"] if c[0] == "denoise_var"] == [(1, 1), (2, 2), (4, 3), (8, 5)]
    levels = [planes]
    for _ in range(3):
        levels.append(PR.down(**levels[-1]))
    result = None
    for l in reversed(levels):
        f = crt.denoise_var(want_rgb=False, **l)[1]
        result = f if result is None else PR.merge(f, result)
    assert_bits(mean, result, "four scales")


@pytest.fixture(scope="module")
def cornell():
    t = util.task("cornell-box")
    r = crt.Render(util.host_scene("cornell-box"), 4, t.P_RR, t.light_sample_n)
    yield r
    r.free()


@pytest.mark.gpu
def test_run_view_denoised_with_scales_equals_the_calls_by_hand(cornell):
    name, w, h = "cornell-box", 48, 36
    r = cornell
    eye, iv, fov = util.camera(name)
    r.set_spp(4)
    rgb0 = r.run_view(eye, iv, fov, width=w, height=h, want_variance=True).copy()
    mean0, var0 = r.mean_buffer.copy(), r.variance_buffer.copy()
    g = r.run_view_aov(eye, iv, fov, want=("albedo", "normal", "depth"), width=w, height=h)
    low = crt.pyramid_down(mean0, variance=var0, **g)
    f0 = crt.denoise_nlm(mean0, var0, want_rgb=False, **g)[1]
    f1 = crt.denoise_nlm(low["color"], low["variance"], want_rgb=False, albedo=low["albedo"], normal=low["normal"], depth=low["depth"])[1]
    want_rgb, want_mean = crt.pyramid_merge(f0, f1)
    rgb, mean = r.run_view_denoised(eye, iv, fov, width=w, height=h, nlm=True, scales=2)
    assert_bits(mean, want_mean, "run_view_denoised(nlm=True, scales=2)")
    assert np.array_equal(rgb, want_rgb) and np.array_equal(r.frame_buffer, rgb0)
    assert_bits(want_mean, PR.merge(f0, f1), "the merge against the restatement")
    assert [c[0] for c in r.denoise_info["calls"]] == ["pyramid_down", "denoise_nlm", "denoise_nlm", "pyramid_merge"]
    # None and 1 are the single call
    for scales in (None, 1):
        assert_bits(r.run_view_denoised(eye, iv, fov, width=w, height=h, nlm=True, scales=scales)[1], f0, "scales=%r" % scales)
    # the other two filters, with settings
    _, mean2 = r.run_view_denoised(eye, iv, fov, width=w, height=h, variance_guided=True, iterations=2, scales=2)
    assert_bits(mean2, crt.denoise_multiscale(mean0, var0, filter="var", scales=2, iterations=2, **g)[1], "variance_guided, scales=2")
    _, mean3 = r.run_view_denoised(eye, iv, fov, width=w, height=h, regress={"radius": 3}, scales=3)
    assert_bits(mean3, crt.denoise_multiscale(mean0, var0, filter="reg", scales=3, radius=3, **g)[1], "regress, scales=3")
    # on irradiance: demodulate -> the pyramid -> modulate, by hand
    rgb4, mean4 = r.run_view_denoised(eye, iv, fov, width=w, height=h, nlm=True, scales=2, demodulate=True)
    sh = r.shading_buffers
    irr, ivar = crt.demodulate(mean0, sh["diffuse_albedo"], sh["emission"], variance=var0)
    filtered = crt.denoise_multiscale(irr, ivar, filter="nlm", scales=2, want_rgb=False, **r.aov_buffers)[1]
    want_rgb4, want_mean4 = crt.modulate(filtered, sh["diffuse_albedo"], sh["emission"])
    assert_bits(mean4, want_mean4, "run_view_denoised(nlm=True, scales=2, demodulate=True)")
    assert np.array_equal(rgb4, want_rgb4)


@pytest.mark.gpu
def test_cli_writes_the_multiscale_frame(cornell, tmp_path):
    from PIL import Image
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    name, w, h = "cornell-box", 48, 36
    base = [cli, util.SCENES[name], "--spp", "4", "--width", str(w), "--height", str(h), "--seed", "42", "--base-dir", util.ROOT]
    noisy, den, den2, den3 = (str(tmp_path / n) for n in ("noisy.png", "den.png", "den2.png", "den3.png"))
    r = cornell
    eye, iv, fov = util.camera(name)
    r.set_spp(4)
    r.seed = 42
    try:
        rgb0 = r.run_view(eye, iv, fov, width=w, height=h, want_variance=True).copy()
        mean0, var0 = r.mean_buffer.copy(), r.variance_buffer.copy()
        g = r.run_view_aov(eye, iv, fov, want=("albedo", "normal", "depth"), width=w, height=h)
        want_demodulated = r.run_view_denoised(eye, iv, fov, width=w, height=h, regress=True, scales=2, demodulate=True)[0]
    finally:
        r.seed = 0
    res = subprocess.run(base + ["-o", noisy, "--denoise", den, "--denoise-nlm", "--denoise-scales", "2"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert np.array_equal(np.asarray(Image.open(noisy)), rgb0)
    assert np.array_equal(np.asarray(Image.open(den)), crt.denoise_multiscale(mean0, var0, filter="nlm", scales=2, **g)[0])
    res = subprocess.run(base + ["-o", noisy, "--denoise", den2, "--denoise-variance", "--denoise-scales", "3", "--denoise-iterations", "2"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert np.array_equal(np.asarray(Image.open(den2)), crt.denoise_multiscale(mean0, var0, filter="var", scales=3, iterations=2, **g)[0])
    res = subprocess.run(base + ["-o", noisy, "--denoise", den3, "--denoise-regress", "--denoise-scales", "2", "--demodulate"], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr
    assert np.array_equal(np.asarray(Image.open(den3)), want_demodulated)
    for extra in (["--denoise", den, "--denoise-scales", "2"], ["--denoise", den, "--denoise-select", "var+nlm", "--denoise-scales", "2"],
                  ["--denoise", den, "--denoise-nlm", "--denoise-scales", "0"], ["--denoise", den, "--denoise-nlm", "--denoise-scales", "5"],
                  ["--denoise", den, "--denoise-nlm", "--denoise-scales", "two"], ["--denoise-scales", "2"]):
        bad = subprocess.run([cli, util.SCENES[name]] + extra, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "--denoise-scales" in bad.stderr, (extra, bad.stderr)


# ------------------------------------------------------------------------------------------------------------------ error --

def mse_rgb8(a, b):
    return float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.gpu
def test_two_scales_do_not_lose_on_veach_mis_at_spp_8():
    """The issue's condition: on the 160 x 120 veach-mis frame at spp 8, crt_denoise_nlm at 2 scales must not have a higher error (RGB8
    mean squared error against spp 256, seed 7) than at 1 scale plus 5 %.  The CPU prototype has 107.5 against 113.4.  No gain is asserted."""
    name, w, h = "veach-mis", 160, 120
    t = util.task(name)
    eye, iv, fov = util.camera(name)
    r = crt.Render(util.host_scene(name), 8, t.P_RR, t.light_sample_n)
    try:
        r.seed = 7
        r.set_spp(256)
        ref = r.run_view(eye, iv, fov, width=w, height=h).copy()
        r.seed = 0
        r.set_spp(8)
        one = r.run_view_denoised(eye, iv, fov, width=w, height=h, nlm=True)[0]
        two = r.run_view_denoised(eye, iv, fov, width=w, height=h, nlm=True, scales=2)[0]
        noisy = r.frame_buffer.copy()
    finally:
        r.free()
    e0, e1, e2 = mse_rgb8(noisy, ref), mse_rgb8(one, ref), mse_rgb8(two, ref)
    print("veach-mis 160x120 spp 8: noisy %.1f, nlm at 1 scale %.1f, at 2 scales %.1f" % (e0, e1, e2))
    assert e2 <= 1.05 * e1, (e0, e1, e2)
