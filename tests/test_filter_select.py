"""Error-estimated filter selection (crt_filter_select / crt_filter_select_device, include/crt.h; filter_select, filter_select_device and
Render.run_view_selected in Python).

The contract of include/crt.h is restated below in numpy float32, one ufunc per operation, with the oracle's tone map
(oracle_lib.tonemap); the device result -- and the host build of the kernels' own text, tools/select_host_check.cpp -- must match it bit
for bit (uint32 views; where the expected value is NaN the result must be NaN).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
from cudaraytracing_amd.hipmem import DeviceBuffers
import host_program as HP
import oracle_lib as O
import util

F = np.float32
ROOT = util.ROOT
SELECT_EXPORTS = ("crt_filter_select_defaults", "crt_filter_select_scratch_bytes", "crt_filter_select", "crt_filter_select_device")
assert_bits = util.assert_bits


def _window_sum(e, r, axis):
    """sum over d = -r .. r ascending of e shifted by d along `axis`, in-image taps only, from +0.0f; and the taps inside per position"""
    n = e.shape[axis]
    acc = np.zeros_like(e)
    pos = np.arange(n)
    taps = np.zeros(n, dtype=np.int64)
    for d in range(-r, r + 1):
        src = pos + d
        valid = (src >= 0) & (src < n)
        shifted = np.take(e, np.clip(src, 0, n - 1), axis=axis)
        mask = valid[None, :] if axis == 1 else valid[:, None]
        acc = np.where(mask, acc + shifted, acc)
        taps += valid
    return acc, taps


def restated(a, b, v, fa, fb, r=3, s=1):
    """The contract: (mean (H, W, 3), choice (H, W) uint8, error (H, W), chosen [4]).  Every ufunc is one IEEE fp32 operation per element."""
    a, b, v = (np.ascontiguousarray(x, dtype=F) for x in (a, b, v))
    fa, fb = [np.ascontiguousarray(x, dtype=F) for x in fa], [np.ascontiguousarray(x, dtype=F) for x in fb]
    K = len(fa)
    h, w = a.shape[:2]
    with np.errstate(all="ignore"):
        E = []
        for k in range(K):
            da, db = fa[k] - b, fb[k] - a
            t = (da * da - v) + (db * db - v)
            e = ((t[..., 0] + t[..., 1]) + t[..., 2]) / F(6.0)
            e = np.where(np.isfinite(e), e, F(np.inf))
            hs, nx = _window_sum(e, r, 1)
            vs, ny = _window_sum(hs, r, 0)
            E.append(vs / (ny[:, None] * nx[None, :]).astype(F))
            assert E[-1].dtype == F
        best, ebest = np.zeros((h, w), dtype=np.int64), E[0]
        for k in range(1, K):
            less = E[k] < ebest
            best, ebest = np.where(less, k, best), np.where(less, E[k], ebest)
        m = []
        for k in range(K):
            mk = (best == k).astype(np.int64)
            mk = _window_sum(_window_sum(mk, s, 1)[0], s, 0)[0]
            m.append(mk)
        total = sum(m)
        o = np.zeros((h, w, 3), dtype=F)
        for k in range(K):
            wk = m[k].astype(F) / total.astype(F)
            term = wk[..., None] * ((fa[k] + fb[k]) * F(0.5))
            o = np.where((m[k] > 0)[..., None], o + term, o)
        assert o.dtype == F and ebest.dtype == F
    chosen = [int((best == k).sum()) for k in range(4)]
    return o, best.astype(np.uint8), ebest, chosen


def box_blur(img, radius=2):
    """(2 radius + 1)^2 clamped box blur, float32"""
    h, w = img.shape[:2]
    ys, xs = np.arange(h), np.arange(w)
    acc = np.zeros_like(img)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            acc = acc + img[np.clip(ys + dy, 0, h - 1)][:, np.clip(xs + dx, 0, w - 1)]
    return (acc / F((2 * radius + 1) ** 2)).astype(F)


def flat_and_checkerboard(seed):
    """64 x 32: truth 0.5 for x < 32, a per-pixel 0.2 / 0.8 checkerboard to the right; halves = truth + N(0, 0.1^2); variance 0.01"""
    h, w = 32, 64
    yy, xx = np.mgrid[0:h, 0:w]
    t1 = np.where(xx < 32, 0.5, np.where((xx + yy) % 2 == 0, 0.2, 0.8))
    truth = np.repeat(t1[..., None], 3, axis=2).astype(F)
    rng = np.random.default_rng(seed)
    a = (truth + rng.normal(0.0, 0.1, truth.shape)).astype(F)
    b = (truth + rng.normal(0.0, 0.1, truth.shape)).astype(F)
    v = np.full(truth.shape, 0.01, dtype=F)
    return truth, a, b, v


def synthetic(w, h, K, seed, special=False):
    """halves, variance and K candidate pairs of a w x h image; special: NaN, +-inf and other awkward values sprinkled into every buffer's
    left third"""
    rng = np.random.default_rng(seed)
    base = rng.random((h, w, 3)) * 2
    imgs = [(base + rng.normal(0, 0.2, base.shape)).astype(F) for _ in range(2)]
    imgs.append((rng.random((h, w, 3)) * 0.05).astype(F))
    band = (np.arange(w) * K) // w                       # candidate k is the quiet one in the k-th vertical band: every candidate wins somewhere
    for k in range(2 * K):
        sigma = np.where(band == k % K, 0.05, 0.4)[None, :, None]
        imgs.append((base + rng.normal(0, 1, base.shape) * sigma).astype(F))
    if special:
        values = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30, 1e-30], dtype=F)
        cols = max(1, w // 3)                             # in the left third only: to the right of it and its window the errors stay finite
        for j, im in enumerate(imgs):
            idx = rng.permutation(h * cols * 3)[:max(values.size, h * cols * 3 // 16)]
            im[idx // (cols * 3), (idx // 3) % cols, idx % 3] = values[(np.arange(idx.size) + j) % values.size]
    return imgs[0], imgs[1], imgs[2], imgs[3:3 + K], imgs[3 + K:]


# the shapes of the issue: 70 x 19 (three tiles across, ragged; three down) at the widest, the default and no windows; a window larger
# than the image; one pixel.  (w, h, K, r, s, special)
CASES = [(70, 19, 4, 8, 4, False), (70, 19, 2, 3, 1, False), (70, 19, 4, 0, 0, False), (5, 3, 2, 8, 1, False), (1, 1, 1, 3, 1, False), (1, 1, 4, 8, 4, False),
         (70, 19, 1, 3, 1, False), (70, 19, 4, 3, 1, True), (33, 9, 3, 8, 4, True), (5, 3, 4, 8, 4, True)]


def case_inputs(i):
    w, h, K, r, s, special = CASES[i]
    return synthetic(w, h, K, 100 + i, special) + (r, s)


# ------------------------------------------------------------------------------------------------------------------ CPU --

def test_select_entry_points_are_exported():
    lib = capi.lib()
    for name in SELECT_EXPORTS:
        assert name in capi.EXPORTS
        getattr(lib, name)
    lib.crt_abi_version.restype = C.c_int
    assert lib.crt_abi_version() == 5 == capi.ABI_VERSION
    for name in ("filter_select", "filter_select_device", "filter_select_defaults", "filter_select_scratch_bytes"):
        assert hasattr(crt, name) and name in crt.__all__
    assert hasattr(crt.Render, "run_view_selected")
    p = capi.FilterSelectParams(7, 7, 7, 7, 7)
    assert lib.crt_filter_select_defaults(C.byref(p)) == capi.CRT_OK
    assert (p.width, p.height, p.n_candidates, p.error_radius, p.blend_radius) == (0, 0, 2, 3, 1)
    assert crt.filter_select_defaults() == {"error_radius": 3, "blend_radius": 1}
    assert lib.crt_filter_select_defaults(None) == capi.ERR_INVALID_ARG
    assert crt.filter_select_scratch_bytes(70, 19) >= 70 * 19 and crt.filter_select_scratch_bytes(70, 19) % 16 == 0


def test_select_arguments_are_checked_before_any_device_call():
    """Every refusal of the contract is CRT_ERR_INVALID_ARG from both forms, also on a machine without a GPU (the pointers here are host
    memory that a device call would fault on)."""
    lib = capi.lib()
    buf = np.zeros(8 * 6 * 3 + 64, dtype=F)
    d = (buf.ctypes.data + 15) & ~15

    def params(**over):
        p = capi.FilterSelectParams(8, 6, 2, 3, 1)
        for k, v in over.items():
            setattr(p, k, v)
        return C.byref(p)

    def inputs(**over):
        s = capi.FilterSelectInputs(d, d, d)
        for k in range(4):
            s.filtered_a[k], s.filtered_b[k] = d, d
        for k, v in over.items():
            if k in ("fa1", "fb0"):
                (s.filtered_a if k == "fa1" else s.filtered_b)[1 if k == "fa1" else 0] = v
            else:
                setattr(s, k, v)
        return C.byref(s)

    def both(prm, inp, mean=d, rgb=d, want=capi.ERR_INVALID_ARG):
        r1 = lib.crt_filter_select(0, prm, inp, mean, rgb, d, d, None)
        e1 = lib.crt_last_error()
        r2 = lib.crt_filter_select_device(0, prm, inp, mean, rgb, d, d, d, 1 << 20, None, None)
        e2 = lib.crt_last_error()
        assert r1 == r2 == want, (r1, r2, e1, e2)
        assert e1.startswith(b"crt_filter_select: ") and e2.startswith(b"crt_filter_select_device: ")
        assert e1[len("crt_filter_select: "):] == e2[len("crt_filter_select_device: "):]
        return e1

    assert b"null" in both(None, inputs()) and b"null" in both(params(), None)
    assert b"positive" in both(params(width=0), inputs()) and b"positive" in both(params(height=0), inputs())
    assert b"n_candidates" in both(params(n_candidates=0), inputs()) and b"n_candidates" in both(params(n_candidates=5), inputs())
    assert b"error_radius" in both(params(error_radius=9), inputs())
    assert b"blend_radius" in both(params(blend_radius=5), inputs())
    assert b"half" in both(params(), inputs(half_a=None)) and b"half" in both(params(), inputs(half_b=None))
    assert b"half_variance" in both(params(), inputs(half_variance=None))
    assert b"candidate 1" in both(params(), inputs(fa1=None)) and b"candidate 0" in both(params(), inputs(fb0=None))
    assert b"no output" in both(params(), inputs(), mean=None, rgb=None)
    assert b"2^24" in both(params(width=(1 << 24) + 1), inputs(), want=capi.ERR_UNSUPPORTED)
    # the scratch of the device form
    for scratch, size, what in ((None, 1 << 20, b"null scratch"), (d, 47, b"too small"), (d + 4, 1 << 20, b"aligned")):
        assert lib.crt_filter_select_device(0, params(), inputs(), d, d, d, d, scratch, size, None, None) == capi.ERR_INVALID_ARG
        assert what in lib.crt_last_error()
    assert lib.crt_filter_select_device(-1, params(), inputs(), d, d, d, d, d, 1 << 20, None, None) == capi.ERR_INVALID_ARG
    assert lib.crt_filter_select_scratch_bytes(8, 6, None) == capi.ERR_INVALID_ARG
    assert not buf.any()
    # the Python layer's own
    img = np.zeros((6, 8, 3), dtype=F)
    with pytest.raises(ValueError):
        crt.filter_select(img, img, img, [img], [img, img])
    with pytest.raises(ValueError):
        crt.filter_select(img, img, img, [img] * 5, [img] * 5)
    with pytest.raises(ValueError):
        crt.filter_select(img, img, img, [], [])
    with pytest.raises(ValueError):
        crt.filter_select(img, img, np.zeros((6, 8), dtype=F), [img], [img])
    with pytest.raises(ValueError):
        crt.filter_select(img, img, img, [img], [img], error_radius=1.5)
    with pytest.raises(ValueError):
        crt.Render.run_view_selected(None, None, None, None, candidates=("var", "median"))
    with pytest.raises(ValueError):
        crt.Render.run_view_selected(None, None, None, None, candidates=())


@pytest.mark.parametrize("s", [0, 1])
def test_restatement_picks_the_blur_on_the_flat_half_and_the_identity_on_the_checkerboard(s):
    """The contract alone, no device: identity against a 5 x 5 box blur.  On the flat half the blur removes noise and adds no bias; on
    the checkerboard it averages 0.2 and 0.8 to 0.5, a squared bias of 0.09 against the identity's noise of 0.01.  The bands x < 27 and
    x >= 37 keep error_radius 3 + the blur's 2 away from the border between the two."""
    for seed in range(5):
        truth, a, b, v = flat_and_checkerboard(seed)
        fa, fb = [a, box_blur(a)], [b, box_blur(b)]
        mean, choice, error, chosen = restated(a, b, v, fa, fb, r=3, s=s)
        assert (choice[:, :27] == 1).mean() >= 0.95, (seed, (choice[:, :27] == 1).mean())
        assert (choice[:, 37:] == 0).mean() >= 0.95, (seed, (choice[:, 37:] == 0).mean())
        assert chosen[0] + chosen[1] == truth.shape[0] * truth.shape[1] and chosen[2] == chosen[3] == 0

        def mse(x):
            return float(((x.astype(np.float64) - truth) ** 2).mean())
        candidates = [mse((fa[k] + fb[k]) * F(0.5)) for k in range(2)]
        print("seed %d s %d: blur on the left %.3f, identity on the right %.3f, MSE selected %.4f identity %.4f blur %.4f"
              % (seed, s, (choice[:, :27] == 1).mean(), (choice[:, 37:] == 0).mean(), mse(mean), candidates[0], candidates[1]))
        assert mse(mean) < min(candidates), (seed, mse(mean), candidates)


@pytest.fixture(scope="module")
def host_check_run(tmp_path_factory):
    """both builds of tools/select_host_check.cpp run over CASES, each with every output and with one output at a time:
    (jobs [(case index, outputs)], [(status, bytes, stderr) plain, sanitised])"""
    tmp = str(tmp_path_factory.mktemp("select_host"))
    jobs = [(i, 15) for i in range(len(CASES))] + [(1, 1), (1, 2), (7, 1 | 4), (7, 2 | 8)]
    blob = [np.array([len(jobs)], dtype="<u4").tobytes()]
    for i, outputs in jobs:
        w, h, K, r, s, _ = CASES[i]
        a, b, v, fa, fb, _, _ = case_inputs(i)
        blob.append(np.array([w, h, K, r, s, outputs], dtype="<u4").tobytes())
        blob += [x.tobytes() for x in [a, b, v] + fa + fb]
    job = os.path.join(tmp, "in.bin")
    with open(job, "wb") as f:
        f.write(b"".join(blob))
    return jobs, HP.run_both_forms("select_host_check.cpp", tmp, job)


def test_kernel_text_on_the_host_gives_the_restatement_bits(host_check_run):
    """csrc/crt_select.h as it is, compiled with g++ -ffp-contract=off, both kernels' bodies workgroup by workgroup: every output of
    every case against the restatement, bit for bit; an output that was not asked for is not written"""
    jobs, res = host_check_run
    rc, raw, err = res[0]
    assert rc == 0, err
    off = 0
    for i, outputs in jobs:
        w, h, K, r, s, _ = CASES[i]
        a, b, v, fa, fb, _, _ = case_inputs(i)
        mean, choice, error, chosen = restated(a, b, v, fa, fb, r, s)
        n = w * h
        got_mean = np.frombuffer(raw, dtype="<f4", count=n * 3, offset=off).reshape(h, w, 3); off += n * 12
        got_rgb = np.frombuffer(raw, dtype=np.uint8, count=n * 3, offset=off).reshape(h, w, 3); off += n * 3
        got_choice = np.frombuffer(raw, dtype=np.uint8, count=n, offset=off).reshape(h, w); off += n
        got_error = np.frombuffer(raw[off:off + n * 4], dtype="<f4").reshape(h, w); off += n * 4
        got_chosen = np.frombuffer(raw[off:off + 32], dtype="<u8"); off += 32
        where = "case %d %r outputs %d" % (i, CASES[i], outputs)
        untouched = np.frombuffer(b"\x5a" * 4, dtype="<f4")[0]
        if outputs & 1:
            assert_bits(got_mean, mean, where + " mean")
        else:
            assert (got_mean.view(np.uint32) == untouched.view(np.uint32)).all(), where
        assert np.array_equal(got_rgb, O.tonemap(mean)) if outputs & 2 else (got_rgb == 0x5a).all(), where + " rgb"
        assert np.array_equal(got_choice, choice) if outputs & 4 else (got_choice == 0x5a).all(), where + " choice"
        if outputs & 8:
            assert_bits(got_error, error, where + " error")
        else:
            assert (got_error.view(np.uint32) == untouched.view(np.uint32)).all(), where
        assert [int(x) for x in got_chosen] == chosen, where
    assert off == len(raw)


def test_kernel_text_is_clean_under_the_sanitizers(host_check_run):
    """the same stand-alone program built with -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all: exit status
    0 and the same bytes -- no LDS, image or scratch index outside its array (each has exactly its size)"""
    _, res = host_check_run
    assert res[1][0] == 0, res[1][2]
    assert res[0][0] == 0 and res[1][1] == res[0][1]


# ------------------------------------------------------------------------------------------------------------------ GPU --

def check_device(a, b, v, fa, fb, r, s, where):
    mean, choice, error, chosen = restated(a, b, v, fa, fb, r, s)
    rgb, gmean, gchoice, gerror, info = crt.filter_select(a, b, v, fa, fb, error_radius=r, blend_radius=s, return_info=True)
    assert_bits(gmean, mean, where + " mean")
    assert np.array_equal(rgb, O.tonemap(mean)), where + " rgb"
    assert np.array_equal(gchoice, choice), where + " choice"
    assert_bits(gerror, error, where + " error")
    assert info["chosen"] == chosen, (where, info, chosen)
    return mean, choice, error, chosen


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)))
def test_device_matches_the_restatement(i):
    a, b, v, fa, fb, r, s = case_inputs(i)
    mean, choice, error, chosen = check_device(a, b, v, fa, fb, r, s, "case %d %r" % (i, CASES[i]))
    K, special = CASES[i][2], CASES[i][5]
    if special:
        assert np.isinf(error).any() and np.isnan(mean).any(), "the special values reached nothing"
    if K > 1 and CASES[i][0] > 5:
        assert sum(c > 0 for c in chosen) >= 2, "one candidate everywhere: the case shows little"


@pytest.mark.gpu
def test_ties_and_all_infinite_errors_stay_with_the_lower_index():
    a, b, v, fa, fb, r, s = case_inputs(1)
    same = [fa[0], fa[0].copy(), fa[0].copy()], [fb[0], fb[0].copy(), fb[0].copy()]
    mean, choice, error, chosen = check_device(a, b, v, same[0], same[1], r, s, "identical candidates")
    assert not choice.any() and chosen == [a.shape[0] * a.shape[1], 0, 0, 0]
    nan_v = np.full_like(v, np.nan)
    mean, choice, error, chosen = check_device(a, b, nan_v, fa, fb, r, s, "NaN variance")
    assert not choice.any() and np.isinf(error).all()


@pytest.mark.gpu
def test_each_optional_output_may_be_left_out():
    a, b, v, fa, fb, r, s = case_inputs(1)
    mean, choice, error, chosen = restated(a, b, v, fa, fb, r, s)
    for drop in ("rgb", "mean", "choice", "error"):
        kw = {"want_" + k: k != drop for k in ("rgb", "mean", "choice", "error")}
        got = dict(zip(("rgb", "mean", "choice", "error"), crt.filter_select(a, b, v, fa, fb, error_radius=r, blend_radius=s, **kw)))
        assert got[drop] is None
        if drop != "mean":
            assert_bits(got["mean"], mean, "without " + drop)
        if drop != "rgb":
            assert np.array_equal(got["rgb"], O.tonemap(mean))
        if drop != "choice":
            assert np.array_equal(got["choice"], choice)
        if drop != "error":
            assert_bits(got["error"], error, "without " + drop)


@pytest.mark.gpu
def test_device_form_on_a_stream():
    i = 7
    w, h, K, r, s, _ = CASES[i]
    a, b, v, fa, fb, _, _ = case_inputs(i)
    mean, choice, error, chosen = restated(a, b, v, fa, fb, r, s)
    names = ["a", "b", "v"] + ["fa%d" % k for k in range(K)] + ["fb%d" % k for k in range(K)]
    table = {n: (3, F) for n in names}
    table.update({"mean": (3, F), "rgb": (3, np.uint8), "error": (1, F), "choice": (1, np.uint8), "scratch": (1, F)})
    with DeviceBuffers.image(table, w, h) as d:
        for n, x in zip(names, [a, b, v] + fa + fb):
            d.upload(n, x)
        assert crt.filter_select_scratch_bytes(w, h) <= d.nbytes("scratch")
        args = (w, h, d.ptrs["a"], d.ptrs["b"], d.ptrs["v"], [d.ptrs["fa%d" % k] for k in range(K)], [d.ptrs["fb%d" % k] for k in range(K)])
        none = crt.filter_select_device(*args, d.ptrs["mean"], d.ptrs["rgb"], d.ptrs["scratch"], d.nbytes("scratch"), out_choice_ptr=d.ptrs["choice"],
                                        out_error_ptr=d.ptrs["error"], error_radius=r, blend_radius=s, stream=d.stream, want_info=False)
        assert none is None
        d.synchronize()
        got = d.fetch(("mean", "error", "rgb", "choice"))
        info = crt.filter_select_device(*args, None, d.ptrs["rgb"], d.ptrs["scratch"], d.nbytes("scratch"), error_radius=r, blend_radius=s, stream=d.stream)
    assert_bits(got["mean"], mean, "device form mean")
    assert_bits(got["error"], error, "device form error")
    assert np.array_equal(got["rgb"], O.tonemap(mean)) and np.array_equal(got["choice"], choice)
    assert info["chosen"] == chosen and info["total_ms"] > 0


@pytest.mark.gpu
def test_run_view_selected_is_its_pieces_called_by_hand():
    name, w, h, spp = "veach-mis", 48, 32, 8
    t = util.task(name)
    r = crt.Render(util.host_scene(name), spp, t.P_RR, t.light_sample_n)
    try:
        eye, iv, fov = util.camera(name)
        rgb, mean = r.run_view_selected(eye, iv, fov, candidates=("var", "nlm"), width=w, height=h)
        sel, info = r.select_buffers, r.select_info
        noisy = r.mean_buffer.copy()
        # by hand
        r.run_view(eye, iv, fov, width=w, height=h, want_halves=True)
        assert np.array_equal(r.mean_buffer.view(np.uint32), noisy.view(np.uint32))
        a, b, done = r.half_buffers(width=w, height=h)
        assert done == spp
        half_var = F(2.0) * r.variance(width=w, height=h)[0]
        g = r.run_view_aov(eye, iv, fov, want=("albedo", "normal", "depth"), width=w, height=h)
        fa = [crt.denoise_var(a, half_var, want_rgb=False, **g)[1], crt.denoise_nlm(a, half_var, want_rgb=False, **g)[1]]
        fb = [crt.denoise_var(b, half_var, want_rgb=False, **g)[1], crt.denoise_nlm(b, half_var, want_rgb=False, **g)[1]]
        rgb2, mean2, choice2, error2, info2 = crt.filter_select(a, b, half_var, fa, fb, return_info=True)
        assert np.array_equal(rgb, rgb2)
        assert_bits(mean, mean2, "run_view_selected mean")
        assert np.array_equal(sel["choice"], choice2)
        assert_bits(sel["error"], error2, "run_view_selected error")
        assert info["chosen"] == info2["chosen"] and sum(info["chosen"]) == w * h
        # ... and those are the restatement's
        want_mean, want_choice, _, _ = restated(a, b, half_var, fa, fb)
        assert_bits(mean2, want_mean, "against the restatement")
        assert np.array_equal(choice2, want_choice)
        with pytest.raises(ValueError):
            r.run_view_selected(eye, iv, fov, candidates=("var", "bilateral"), width=w, height=h)
    finally:
        r.free()


@pytest.mark.gpu
def test_cli_writes_the_selected_frame_and_the_choice_map(tmp_path):
    from PIL import Image
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    name, w, h, spp = "veach-mis", 48, 32, 8
    base = [cli, util.SCENES[name], "--spp", str(spp), "--width", str(w), "--height", str(h), "--seed", "42", "--base-dir", util.ROOT]
    plain, sel, choice = (str(tmp_path / n) for n in ("plain.png", "selected.png", "choice.png"))
    res = subprocess.run(base + ["-o", plain, "--denoise", sel, "--denoise-select", "none+var+nlm,2,0", "--denoise-choice", choice], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr
    assert "denoise-select: error radius 2, blend radius 0" in res.stdout
    t = util.task(name)
    r = crt.Render(util.host_scene(name), spp, t.P_RR, t.light_sample_n)
    try:
        r.seed = 42
        want, _ = r.run_view_selected(*util.camera(name), candidates=("none", "var", "nlm"), error_radius=2, blend_radius=0, width=w, height=h)
        assert np.array_equal(np.asarray(Image.open(plain)), r.frame_buffer)   # -o stays the plain frame
        assert np.array_equal(np.asarray(Image.open(sel)), want)
        grey = np.asarray(Image.open(choice))
        assert np.array_equal(grey[..., 0], (255 * r.select_buffers["choice"].astype(np.int64) // 2).astype(np.uint8))
    finally:
        r.free()
    for bad_args in (["--denoise-select", "var+nlm"], ["--denoise", sel, "--denoise-choice", choice], ["--denoise", sel, "--denoise-select", "var+median"],
                     ["--denoise", sel, "--denoise-select", "var,9"], ["--denoise", sel, "--denoise-select", "var,3,5"],
                     ["--denoise", sel, "--denoise-select", "none+atrous+var+nlm+var"], ["--denoise", sel, "--denoise-select", "var", "--denoise-nlm"],
                     ["--denoise", sel, "--denoise-select", "var", "--adaptive", "0.1"]):
        bad = subprocess.run(base + bad_args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 1 and "--denoise-" in bad.stderr, (bad_args, bad.stderr)
