"""The device's deterministic math, short divisions, samplers and per-vertex path formulas, value by value (crt_device_fn, include/crt.h).

Every frame result rests on the device evaluating csrc/crt_detmath.h, the vector helpers of crt_device.h, the samplers of crt_trace.h
and the formulas of crt_path.h bit for bit as the oracle does.  The frame tests check that through two scenes; here each function is
called on the device with chosen inputs (tests/device_fn_sets.py: the whole exponent range with denormals, infinities and NaNs, each
function's own borders, whole waves inside and outside the short division's guard, the ties and axes of to_world, both sides of
sample_lobe's 1e-5 test, shininess far beyond the shipped five values) and compared on uint32 views.  Where the expectation is NaN the
result must be NaN; the payload is not compared.

Expectations: the oracle (O.math_fn, O.fn) for the math and the samplers; numpy float32, one IEEE operation per ufunc, for the vector
helpers and the path formulas (device_fn_sets.py cites Render.cuh); the reference's OWN to_world, get_cuda_random_sphere_vector and
get_cuda_random_specular_sphere_vector (Global.h:35-94) through tests/golden/reference_pin/samplers.npz.

CPU tests: the entry point's argument checks; csrc/crt_detmath.h compiled for the host (tools/detmath_host_check.cpp, plain and with
-fsanitize=address,undefined,float-cast-overflow) against the oracle; the oracle against the fixture (and the live probe against the
fixture where oracle/_ref/path_probe exists); and anchors of the oracle against numpy float64, so that "the device equals the oracle"
means something."""
import os

import numpy as np
import pytest

import cudaraytracing_amd as crt
import device_fn_sets as DS
import host_program as HP
import oracle_lib as O
import reference_pin as RP
from cudaraytracing_amd import _capi as capi

F, U = np.float32, np.uint32
gpu = pytest.mark.gpu
live = pytest.mark.skipif(not RP.have_probe(), reason="oracle/_ref/path_probe is not built (needs the reference tree: make -C oracle)")

FN_WORDS = {"sin": (1, 1), "cos": (1, 1), "tan": (1, 1), "asin": (1, 1), "acos": (1, 1), "atan": (1, 1), "exp": (1, 1), "log": (1, 1),
            "log10": (1, 1), "uniform": (1, 1), "sincos": (1, 2), "atan2": (2, 1), "pow": (2, 1), "dot3": (6, 1), "cross3": (6, 3),
            "norm3": (3, 1), "unit3": (3, 3), "div3": (4, 3), "make_ray": (3, 6), "to_world": (6, 3), "sample_hemisphere": (5, 3),
            "sample_lobe": (7, 3), "bounce_dir": (5, 3), "cos_to_next": (9, 1), "roulette": (6, 5), "probe_dir": (12, 3),
            "probe_term": (17, 3), "indirect_step": (11, 3), "seed_direct": (3, 3), "seed_emitter": (4, 3), "tonemap": (1, 1)}
MAX_CALL = 1 << 20


def dev(name, records):
    """crt.device_fn on (n, input words) bits, in calls of at most 2^20 elements cut at multiples of 64 (whole waves stay whole)"""
    r = np.ascontiguousarray(records)
    r = (r if r.dtype == U else DS.bits(r)).reshape(len(r), -1)
    assert r.shape[1] == FN_WORDS[name][0], (name, r.shape)
    return np.concatenate([crt.device_fn(name, r[i:i + MAX_CALL], FN_WORDS[name][1]) for i in range(0, len(r), MAX_CALL)])


def assert_same(got, want, records=None, what=""):
    want = np.ascontiguousarray(want)
    want = (want if want.dtype == U else DS.bits(want)).reshape(len(got), -1)
    ok = DS.same(got, want).all(axis=1)
    if not ok.all():
        i = np.nonzero(~ok)[0]
        rec = None if records is None else np.asarray(records).reshape(len(got), -1)[i[:4]]
        raise AssertionError("%s: %d of %d differ; first at %s: inputs %s got %s want %s" % (what, len(i), len(ok), i[:4], rec, got[i[:4]], want[i[:4]]))


# ================================================================================================ CPU: the entry point's argument checks
def test_device_fn_argument_checks_need_no_device():
    L = capi.lib()
    assert "crt_device_fn" in capi.EXPORTS
    buf = np.zeros(32, dtype=U)
    out = np.zeros(32, dtype=U)
    p, q = capi.ptr(buf), capi.ptr(out)

    def status(*a):
        s = L.crt_device_fn(*a)
        return s, L.crt_last_error().decode()
    s, msg = status(0, b"no_such_function", 1, p, 1, q, 1)
    assert s == capi.ERR_INVALID_ARG and "no_such_function" in msg
    for bad in ((0, None, 1, p, 1, q, 1), (0, b"sin", 1, None, 1, q, 1), (0, b"sin", 1, p, 1, None, 1)):
        s, msg = status(*bad)
        assert s == capi.ERR_INVALID_ARG and "null" in msg
    for name, (iw, ow) in FN_WORDS.items():
        for bad_iw, bad_ow in ((iw + 1, ow), (iw, ow + 1), (0, ow), (iw, 0)):
            s, msg = status(0, name.encode(), 1, p, bad_iw, q, bad_ow)
            assert s == capi.ERR_INVALID_ARG and name in msg and "words" in msg, (name, bad_iw, bad_ow, s, msg)
        assert L.crt_device_fn(0, name.encode(), 0, p, iw, q, ow) == capi.CRT_OK     # n == 0: nothing to do, no device call
    s, msg = status(-1, b"sin", 1, p, 1, q, 1)
    assert s == capi.ERR_INVALID_ARG and "device" in msg
    with pytest.raises(crt.CrtError):
        crt.device_fn("sin", np.zeros((4, 2), dtype=F), 1)
    with pytest.raises(TypeError):
        crt.device_fn("sin", np.zeros((4, 1), dtype=np.float64), 1)
    assert crt.device_fn("sin", np.zeros((0, 1), dtype=F), 1).shape == (0, 1)


# ================================================================================================ CPU: crt_detmath.h on the host
HOST_FNS = ("sin", "cos", "tan", "asin", "acos", "atan", "exp", "log", "log10", "sincos.s", "sincos.c", "uniform")


@pytest.fixture(scope="module")
def host_check_run(tmp_path_factory):
    """both builds of tools/detmath_host_check.cpp run on X + borders and the pairs: (x, a, b, bytes plain, status and bytes sanitised)"""
    tmp = str(tmp_path_factory.mktemp("detmath_host"))
    x = DS.all_scalars()
    a, b = DS.pow_pairs()
    job = os.path.join(tmp, "in.bin")
    with open(job, "wb") as f:
        f.write(np.array([x.size], dtype="<u4").tobytes() + x.tobytes() + np.array([a.size], dtype="<u4").tobytes() + a.tobytes() + b.tobytes())
    return x, a, b, HP.run_both_forms("detmath_host_check.cpp", tmp, job)


def test_detmath_header_on_the_host_gives_the_oracle_bits(host_check_run):
    """csrc/crt_detmath.h as it is, compiled with g++ -ffp-contract=off: every function over X, every border and the pair grids against
    O.math_fn, bit for bit.  (What the device build of the same text gives is test_device_math_over_the_whole_range.)"""
    x, a, b, res = host_check_run
    rc, raw, err = res[0]
    assert rc == 0, err
    got = np.frombuffer(raw, dtype="<u4")
    assert got.size == len(HOST_FNS) * x.size + 2 * a.size
    for i, fn in enumerate(HOST_FNS):
        g = got[i * x.size:(i + 1) * x.size]
        want = DS.bits(DS.uniform(DS.bits(x))) if fn == "uniform" else DS.bits(O.math_fn({"sincos.s": "sin", "sincos.c": "cos"}.get(fn, fn), x))
        assert_same(g.reshape(-1, 1), want, x, "host " + fn)
    base = len(HOST_FNS) * x.size
    assert_same(got[base:base + a.size].reshape(-1, 1), O.math_fn("atan2", a, b), np.column_stack([a, b]), "host atan2")
    assert_same(got[base + a.size:].reshape(-1, 1), O.math_fn("pow", a, b), np.column_stack([a, b]), "host pow")


def test_detmath_header_is_clean_under_the_sanitizers(host_check_run):
    """the same stand-alone program built with -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all: the same
    inputs, exit status 0, the same bytes (no conversion of an out-of-range float, no signed overflow, no shift of a negative exponent)"""
    _, _, _, res = host_check_run
    assert res[1][0] == 0, res[1][2]
    assert res[0][0] == 0 and res[1][1] == res[0][1]


# ================================================================================================ CPU: the reference's own samplers
@pytest.fixture(scope="module")
def samplers_gold():
    return RP.load("samplers")


def test_sampler_fixture_holds_the_recorded_sets(samplers_gold):
    recs, meta = DS.sampler_records(), RP.load_meta()["samplers"]
    for k in RP.SAMPLER_FNS:
        assert np.array_equal(samplers_gold["in_" + k], recs[k]) and meta[k] == len(recs[k])
        assert samplers_gold["out_" + k].shape == (len(recs[k]), 3)
    # the branches the shipped scenes rarely reach are in it
    n = DS.fl(recs["to_world"][:, 3:6])
    assert (np.abs(n[:, 0]) == np.abs(n[:, 1])).sum() >= 30 and np.isnan(n).any() and (np.abs(n) > 1e38).any()
    ox = DS.fl(recs["sample_lobe"][:, 0])
    assert ((np.abs(ox).astype(np.float64) < 1e-5) & (ox != 0)).sum() >= 8 and (np.abs(ox).astype(np.float64) >= 1e-5).sum() > 3000


@pytest.mark.parametrize("fn", RP.SAMPLER_FNS)
def test_oracle_reproduces_the_reference_samplers(samplers_gold, fn):
    """O.fn (the oracle's to_world / sample_hemisphere / sample_lobe) against what the reference's Global.h:35-94 computed at the same records"""
    rec, out = samplers_gold["in_" + fn], samplers_gold["out_" + fn]
    assert_same(O.fn(fn, rec), out, rec, "oracle " + fn)
    # the ordinary records (the 3000 random unit vectors; for the lobe those whose angles stay below 8192 rad) hold no NaN: no comparison
    # above is carried by NaN == NaN alone
    ordinary = np.arange(len(rec)) < len(DS.random_units())
    if fn == "sample_lobe":
        with np.errstate(invalid="ignore"):
            ordinary &= np.abs(DS.fl(rec[:, 4])) < 8000
        assert ordinary.sum() > 1500
    assert not np.isnan(DS.fl(out[ordinary])).any()


def test_oracle_single_calls_agree_with_the_vectorised_form(samplers_gold):
    """orc_fn calls the same functions as the per-element entry points the older tests use"""
    rh, rl = samplers_gold["in_sample_hemisphere"][::97], samplers_gold["in_sample_lobe"][::97]
    one = np.array([DS.bits(O.sample_hemisphere(DS.fl(r[:3]), DS.uniform(r[3:4])[0], DS.uniform(r[4:5])[0])) for r in rh])
    assert_same(O.fn("sample_hemisphere", rh), one)
    one = np.array([DS.bits(O.sample_lobe(DS.fl(r[:3]), DS.fl(r[3:4])[0], DS.fl(r[4:5])[0], DS.uniform(r[5:6])[0], DS.uniform(r[6:7])[0])) for r in rl])
    assert_same(O.fn("sample_lobe", rl), one)
    v = samplers_gold["in_to_world"][::53]
    assert_same(O.fn("normalized", v[:, :3]), np.array([O.vec_op("normalized", r[:3]) for r in v]))
    assert_same(O.fn("dot", v), np.array([O.vec_op("dot", r) for r in v]))
    assert_same(O.fn("cross", v), np.array([O.vec_op("cross", r) for r in v]))
    assert_same(O.fn("norm", v[:, :3]), np.array([O.vec_op("norm", r[:3]) for r in v]))
    assert_same(O.fn("bounce_dir", rh), O.fn("normalized", O.fn("sample_hemisphere", rh)))


@live
def test_live_probe_reproduces_the_sampler_fixture(samplers_gold, tmp_path):
    RP.rebuild_probe()
    res = RP.probe_samplers({k: samplers_gold["in_" + k] for k in RP.SAMPLER_FNS}, tmp_path)
    for k in RP.SAMPLER_FNS:
        assert_same(res[k], samplers_gold["out_" + k], samplers_gold["in_" + k], "live " + k)


# ================================================================================================ CPU: the vector sets are what they claim
def test_division_sets_lie_where_they_claim():
    """the wave-ordered sets of unit3 / div3 / make_ray against the restated guard of quot3_exact: >= 4 whole waves inside, every reason to
    be outside as whole waves of its own with the offending numerator in x, in y and in z, and a mix that has both kinds in one wave"""
    for (recs, st), inside_of in ((DS.div3_set(), lambda r: DS.quot_guard(r[:, :3], r[:, 3], False)), (DS.unit3_set(), DS.unit3_inside)):
        inside = inside_of(np.asarray(recs))
        names = [s[0] for s in st]
        assert len(recs) % 64 == 0 and len(recs) <= MAX_CALL
        for name, lo, hi, want in st:
            assert lo % 64 == 0 and hi % 64 == 0
            if want is True:
                assert hi - lo >= 256 and inside[lo:hi].all(), name
            elif want is False:
                assert hi - lo >= 128 and not inside[lo:hi].any(), name
            else:
                w = inside[lo:hi].reshape(-1, 64).sum(axis=1)
                assert ((w > 0) & (w < 64)).mean() > 0.9, name     # waves of the mix diverge at the guard
        for c in "xyz":
            assert "numerator %s in (0, 2^-64)" % c in names and "numerator %s non-finite" % c in names
        assert sum(hi - lo for _, lo, hi, w in st if w is False) >= 256
    names = [s[0] for s in DS.div3_set()[1]]
    assert all("numerator %s >= 2^62" % c in names for c in "xyz")
    assert {"divisor < 2^-62", "divisor >= 2^60", "divisor zero / negative / non-finite"} <= set(names)
    # in an "outside because of one numerator" stretch the other two numerators and the divisor are ordinary: alone they would be inside
    recs, st = DS.div3_set()
    for name, lo, hi, want in st:
        if name.startswith("numerator"):
            c = "xyz".index(name.split()[1])
            r = np.array(recs[lo:hi])
            r[:, c] = 1.0
            assert DS.quot_guard(r[:, :3], r[:, 3], False).all(), name


# ================================================================================================ CPU: the oracle against float64
def _ulps(got, exact):
    """|got - exact| in units of the float32 spacing at |exact|"""
    exact = np.asarray(exact, dtype=np.float64)
    with np.errstate(all="ignore"):
        near = exact.astype(F)
        e = np.frexp(np.minimum(np.abs(near), np.finfo(F).max).astype(np.float64))[1]   # |x| = m 2^e, m in [0.5, 1)
        u = np.abs(got.astype(np.float64) - exact) / np.ldexp(1.0, np.maximum(e - 24, -149))
        return np.where(np.isinf(near) & (got == near), 0.0, u)   # (an exact value that rounds to infinity: infinity is the right answer)


def _measure_anchors():
    """the worst error of the oracle against numpy float64 on the sets of device_fn_sets.py: {name: figure}"""
    fig = {}
    with np.errstate(all="ignore"):
        x = DS.scalar_set("sin")
        x = x[np.abs(x) < 8192]
        for fn, ref in (("sin", np.sin), ("cos", np.cos)):
            g, e = O.math_fn(fn, x), ref(x.astype(np.float64))
            fig[fn + " abs"] = float(np.abs(g.astype(np.float64) - e).max())
            fig[fn + " ulp"] = float(_ulps(g, e).max())
        x = DS.scalar_set("exp")
        x = x[(x >= -87) & (x <= F(88.72283905206835))]
        fig["exp ulp"] = float(_ulps(O.math_fn("exp", x), np.exp(x.astype(np.float64))).max())
        x = DS.scalar_set("log")
        x = x[(x > 0) & np.isfinite(x)]
        fig["log ulp"] = float(_ulps(O.math_fn("log", x), np.log(x.astype(np.float64))).max())
        fig["log10 ulp"] = float(_ulps(O.math_fn("log10", x), np.log10(x.astype(np.float64))).max())
        x = DS.scalar_set("acos")
        x = x[np.abs(x) <= 1]
        fig["acos ulp"] = float(_ulps(O.math_fn("acos", x), np.arccos(x.astype(np.float64))).max())
        fig["asin ulp"] = float(_ulps(O.math_fn("asin", x), np.arcsin(x.astype(np.float64))).max())
        x = DS.scalar_set("atan")
        x = x[np.isfinite(x)]
        fig["atan ulp"] = float(_ulps(O.math_fn("atan", x), np.arctan(x.astype(np.float64))).max())
        a, b = DS.pair_grid()
        k = np.isfinite(a) & np.isfinite(b) & (a != 0)   # (a zero y: Cephes ignores its sign, atan2(-0, x < 0) is +pi -- the same angle as libm's -pi)
        a, b = a[k], b[k]
        fig["atan2 ulp"] = float(_ulps(O.math_fn("atan2", a, b), np.arctan2(a.astype(np.float64), b.astype(np.float64))).max())
        x = DS.whole_range()
        x = x[(x > 0) & (x <= 1)]
        e = np.full_like(x, 0.6)
        fig["pow 0.6 ulp"] = float(_ulps(O.math_fn("pow", x, e), x.astype(np.float64) ** np.float64(F(0.6))).max())
        # ---- samplers with unit normals and finite inputs, against the same formulas in float64
        recs = DS.sampler_records(4)
        r = recs["sample_hemisphere"]
        N = DS.fl(r[:, :3])
        unit = np.abs(np.sqrt(DS.sqnorm(N.astype(np.float64))) - 1) < 1e-6
        r, N = r[unit], N[unit].astype(np.float64)
        v = DS.fl(O.fn("sample_hemisphere", r)).astype(np.float64)
        fig["hemisphere n"] = int(len(r))
        fig["hemisphere | |v| - 1 |"] = float(np.abs(np.sqrt((v * v).sum(axis=1)) - 1).max())
        fig["hemisphere -min v.N"] = float(max(0.0, -(v * N).sum(axis=1).min()))
        x1, x2 = DS.uniform(r[:, 3]).astype(np.float64), DS.uniform(r[:, 4]).astype(np.float64)
        z = np.abs(1 - 2 * x1)
        rr, phi = np.sqrt(1 - z * z), 2 * DS.PI * x2
        loc = np.column_stack([rr * np.cos(phi), rr * np.sin(phi), z])
        big = np.abs(N[:, 0]) > np.abs(N[:, 1])
        il = 1 / np.sqrt(np.where(big, N[:, 0] ** 2, N[:, 1] ** 2) + N[:, 2] ** 2)
        Cv = np.where(big[:, None], np.column_stack([N[:, 2] * il, 0 * il, -N[:, 0] * il]), np.column_stack([0 * il, N[:, 2] * il, -N[:, 1] * il]))
        Bv = np.cross(Cv, N)
        w = loc[:, 0:1] * Bv + loc[:, 1:2] * Cv + loc[:, 2:3] * N
        fig["hemisphere vs float64"] = float(np.abs(v - w).max())
        r = recs["sample_lobe"]
        o, dth, dph = DS.fl(r[:, :3]).astype(np.float64), DS.fl(r[:, 3]).astype(np.float64), DS.fl(r[:, 4]).astype(np.float64)
        e1, e2 = 2 * DS.uniform(r[:, 5]).astype(np.float64) - 1, 2 * DS.uniform(r[:, 6]).astype(np.float64) - 1
        nrm = np.sqrt((o * o).sum(axis=1))
        th0 = np.arccos(np.clip(o[:, 2] / nrm, -1, 1))
        ph0 = np.where(np.abs(o[:, 0]) < 1e-5, np.where(o[:, 1] > 0, DS.PI / 2, -DS.PI / 2), np.arctan2(o[:, 1], o[:, 0]))
        th, ph = th0 + e1 * dth, ph0 + e2 * dph
        k = np.isfinite(o).all(axis=1) & (nrm > 0.1) & (nrm < 10) & (np.abs(th) <= 16) & (np.abs(ph) <= 16)
        v = DS.fl(O.fn("sample_lobe", r[k])).astype(np.float64)
        w = np.column_stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])[k]
        fig["lobe n"] = int(k.sum())
        fig["lobe | |v| - 1 |"] = float(np.abs(np.sqrt((v * v).sum(axis=1)) - 1).max())
        fig["lobe vs float64"] = float(np.abs(v - w).max())
    return fig


@pytest.fixture(scope="module")
def anchors():
    fig = _measure_anchors()
    print("measured anchors:", {k: (v if isinstance(v, int) else float("%.3g" % v)) for k, v in fig.items()})
    return fig


# name: the worst error measured with the sets of device_fn_sets.py; the bound asserted is twice that
ANCHORS = {
    "sin abs": 6.297e-08, "sin ulp": 1.391, "cos abs": 6.553e-08, "cos ulp": 1.242,   # |x| < 8192 of X and the borders
    "exp ulp": 0.9091,                                                                # [-87, 88.7228] of X and the exp borders
    "log ulp": 0.709, "log10 ulp": 1.989,                                             # every positive finite input, denormals included
    "acos ulp": 1.129, "asin ulp": 1.879,                                             # [-1, 1]
    "atan ulp": 2.46,                                                                 # every finite input
    "atan2 ulp": 2.534,                                                               # finite pairs of the grid with y != 0
    "pow 0.6 ulp": 67.76,                                                             # every x of X in (0, 1] (worst at tiny bases)
    "hemisphere | |v| - 1 |": 2.21e-07, "hemisphere -min v.N": 1.583e-08, "hemisphere vs float64": 3.738e-05,
    "lobe | |v| - 1 |": 8.986e-08, "lobe vs float64": 2e-05,
}


@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_oracle_is_anchored_to_float64(anchors, name):
    """The oracle is the expectation of every device comparison below, so it is itself held to numpy float64 -- an independent
    evaluation -- on the domains where the Cephes float algorithms are accurate.  The tolerances are measured, not chosen: the worst
    error over the sets of device_fn_sets.py is recorded in ANCHORS and asserted at twice that figure (the margin covers numpy's float64
    functions on another libm, which are not correctly rounded).  Measured -> bound:
      sin / cos, |x| < 8192        6.30e-8 / 6.55e-8 absolute -> 1.26e-7 / 1.31e-7;  1.39 / 1.24 ulp -> 2.78 / 2.48 ulp
      exp on [-87, 88.7228]        0.909 ulp -> 1.82 ulp
      log, log10, x > 0 finite     0.709 / 1.99 ulp -> 1.42 / 3.98 ulp (denormal inputs included)
      acos, asin on [-1, 1]        1.13 / 1.88 ulp -> 2.26 / 3.76 ulp
      atan (finite), atan2 (finite pairs, y != 0)   2.46 / 2.53 ulp -> 4.92 / 5.07 ulp
      pow(x, 0.6), x in (0, 1]     67.8 ulp -> 136 ulp (worst at tiny bases: the error of log x times 0.6 |log x|)
      hemisphere, unit normals     | |v| - 1 | 2.21e-7 -> 4.42e-7;  v . N >= -1.58e-8 -> -3.17e-8;  against float64 3.74e-5 -> 7.48e-5
                                   (cancellation of 1 - z^2 near the pole, inherent to Global.h:62)
      lobe, |out| in (0.1, 10), |theta|, |phi| <= 16   | |v| - 1 | 8.99e-8 -> 1.80e-7;  against float64 2.0e-5 -> 4.0e-5
    (an ulp is the float32 spacing at the exact value).  Outside these domains the Cephes reduction is not accurate by design (sin / cos
    beyond 8192 lose the low bits of the argument, beyond 1e30 they return NaN), exp returns 0 below -87 where the exact value is still a
    denormal, and atan2 ignores the sign of a zero y: there only the bit comparisons of this file apply."""
    measured = ANCHORS[name]
    print("%s: %.4g now, %.4g recorded, bound %.4g" % (name, anchors[name], measured, 2 * measured))
    assert anchors[name] <= 2 * measured


def test_anchor_sets_are_not_empty(anchors):
    assert anchors["hemisphere n"] >= 10000 and anchors["lobe n"] >= 5000


# ================================================================================================ GPU: the math
ONE_ARG = ("sin", "cos", "tan", "asin", "acos", "atan", "exp", "log", "log10")


@gpu
@pytest.mark.parametrize("fn", ONE_ARG)
def test_device_math_over_the_whole_range(fn):
    """every sign x exponent x 512 mantissas (denormals, infinities and NaNs included) and the function's own borders with their
    neighbours (for exp: the cut-offs and every x whose exponent n is -126, 127 or 128), against the oracle"""
    x = DS.scalar_set(fn)
    assert x.size >= 262144 and x.size <= MAX_CALL
    assert_same(dev(fn, x), O.math_fn(fn, x), x, fn)


@gpu
def test_device_sincos_is_sin_and_cos():
    x = DS.scalar_set("sincos")
    got = dev("sincos", x)
    assert_same(got[:, 0:1], O.math_fn("sin", x), x, "sincos.s")
    assert_same(got[:, 1:2], O.math_fn("cos", x), x, "sincos.c")


@gpu
def test_device_atan2_and_pow_over_the_pair_grid():
    a, b = DS.pair_grid()
    assert_same(dev("atan2", np.column_stack([a, b])), O.math_fn("atan2", a, b), np.column_stack([a, b]), "atan2")
    a, b = DS.pow_pairs()
    assert a.size > 850000
    assert_same(dev("pow", np.column_stack([a, b])), O.math_fn("pow", a, b), np.column_stack([a, b]), "pow")


@gpu
def test_device_uniform_and_tonemap():
    w = np.concatenate([DS.EDGE_WORDS, DS.draw_words(np.random.default_rng(5), 100000), np.arange(0xffffff00, 0x100000000, dtype=np.uint64).astype(U)])
    got = dev("uniform", w)
    assert_same(got, DS.uniform(w), w, "uniform")
    assert DS.fl(got).min() > 0.0 and DS.fl(got).max() <= 1.0
    u, f = O.rng_draw(9, 8, 7, 6, 1, 0)                  # (the oracle's own mapping of a draw's words is the same one)
    assert np.array_equal(DS.bits(DS.uniform(u)), DS.bits(f))
    x = np.concatenate([DS.whole_range(), DS.around([0.0, 1.0, 0.5, 1.0 / 255.0]), np.linspace(0, 1, 4097).astype(F)])
    got = dev("tonemap", x)
    assert got.max() <= 255
    assert np.array_equal(got.reshape(-1).astype(np.uint8), O.tonemap(x)), "tonemap"


# ================================================================================================ GPU: vectors and the short division
def _wide_vectors(seed, m):
    """random vectors over a wide exponent range, the special ones, zeros of both signs"""
    rng = np.random.default_rng(seed)
    v = np.column_stack([DS._log_uniform(rng, m, -70, 70) for _ in range(3)])
    v[:len(DS.special_vectors())] = DS.special_vectors()
    v[100:110] = DS.fl(DS.draw_words(rng, 30)).reshape(10, 3)   # any bits
    v[110] = [0.0, -0.0, 0.0]
    return v


@gpu
def test_device_dot_cross_norm():
    a, b = _wide_vectors(21, 65536 + 37), _wide_vectors(22, 65536 + 37)
    b[:21] = b[:21][::-1]
    ab = np.column_stack([a, b])
    with np.errstate(all="ignore"):
        assert_same(dev("dot3", ab), DS.dot(a, b), ab, "dot3")
        cr = np.column_stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]])
        assert_same(dev("cross3", ab), cr, ab, "cross3")
        assert_same(dev("norm3", a), np.sqrt(DS.sqnorm(a)), a, "norm3")
    assert_same(dev("dot3", ab), O.fn("dot", DS.bits(ab)), ab, "dot3 against the oracle")
    assert_same(dev("cross3", ab), O.fn("cross", DS.bits(ab)), ab, "cross3 against the oracle")


@gpu
def test_device_short_division_wave_by_wave():
    """unit3 / div3 / make_ray over whole waves inside quot3_exact's guard, whole waves outside it for each reason (the offending
    numerator in x, in y, in z: the guard is the min / max of three numerators behind a wave-uniform branch) and a shuffled mix,
    against numpy float32 /, sqrt and the Eigen order x x + (y y + z z).  test_division_sets_lie_where_they_claim checks the sets."""
    recs, _ = DS.div3_set()
    with np.errstate(all="ignore"):
        assert_same(dev("div3", recs), recs[:, :3] / recs[:, 3:4], recs, "div3")
    recs, _ = DS.unit3_set()
    want = DS.normalized(recs)
    assert_same(dev("unit3", recs), want, recs, "unit3")
    assert_same(dev("unit3", recs), O.fn("normalized", DS.bits(recs)), recs, "unit3 against the oracle")
    with np.errstate(all="ignore"):
        assert_same(dev("make_ray", recs), np.column_stack([want, F(1) / want]), recs, "make_ray")


# ================================================================================================ GPU: the samplers
@gpu
@pytest.mark.parametrize("fn", RP.SAMPLER_FNS)
def test_device_samplers_give_the_reference_bits(samplers_gold, fn):
    """against what the reference's own Global.h:35-94 computed (the fixture), then against the oracle on four times as many draws"""
    assert_same(dev(fn, samplers_gold["in_" + fn]), samplers_gold["out_" + fn], samplers_gold["in_" + fn], fn + " against the reference")
    r = DS.sampler_records(4)[fn]
    assert len(r) >= 12000
    assert_same(dev(fn, r), O.fn(fn, r), r, fn + " against the oracle")


@gpu
def test_device_bounce_dir_is_the_normalized_hemisphere_sample():
    r = DS.sampler_records(4)["sample_hemisphere"]
    assert_same(dev("bounce_dir", r), O.fn("normalized", O.fn("sample_hemisphere", r)), r, "bounce_dir")


# ================================================================================================ GPU: the per-vertex path formulas
def _no_nan(bits_):
    return not np.isnan(DS.fl(bits_)).any()


@gpu
def test_device_cos_to_next():
    rng = np.random.default_rng(31)
    m = 8192
    frm, to = rng.uniform(-10, 10, (m, 3)).astype(F), rng.uniform(-10, 10, (m, 3)).astype(F)
    n = np.tile(DS.random_units(), (3, 1))[:m].copy()
    ordinary = slice(64, m)
    to[0:16] = frm[0:16]                                                   # to == from: the zero vector is not normalised, the cosine is 0
    to[16:32] = frm[16:32] + DS.fl(DS.bits(frm[16:32]) & U(0x7f800000)) * F(2.0 ** -23)   # one ulp apart
    frm[32:40, 0], to[40:48, 1], n[48:56, 2] = np.nan, np.inf, np.nan
    frm[56:64] *= F(1e30)
    want = DS.cos_to_next(frm, to, n)
    assert _no_nan(DS.bits(want)) and (want[0:16] == 0).all() and (want[ordinary] > 0).sum() > 3000 and (want[ordinary] == 0).sum() > 3000
    rec = np.column_stack([frm, to, n])
    assert_same(dev("cos_to_next", rec), want, rec, "cos_to_next")


@gpu
def test_device_roulette():
    rng = np.random.default_rng(32)
    p = np.array([0, 0.6, 0.8, 1, np.nextafter(F(1), F(0)), np.nan], dtype=F)
    depth = np.array([0, 1, 62, 63], dtype=U)
    reps = 96
    pp, dd = np.meshgrid(p, depth, indexing="ij")
    pp, dd = np.tile(pp.reshape(-1), reps), np.tile(dd.reshape(-1), reps)
    m = len(pp)
    seed = rng.integers(0, 1 << 64, m, dtype=np.uint64)
    seed[:4] = [0, 1, 0xffffffffffffffff, 0x100000000]
    pixel, k = DS.draw_words(rng, m) >> U(8), DS.draw_words(rng, m) >> U(20)
    want = DS.roulette(seed, pixel, k, dd, pp)
    full = dd == 63
    assert (want[full, 0] == 1).all() and (want[full, 1:] == 0).all()        # depth 63: stop, no draw, rb = 0
    assert (want[~full & (pp == 0), 0] == 1).all() and (want[~full & (pp == 1), 0] == 0).all() and (want[~full & np.isnan(pp), 0] == 0).all()
    mid = ~full & (pp == F(0.6))
    assert 0.3 < want[mid, 0].mean() < 0.5
    rec = np.column_stack([(seed & np.uint64(0xffffffff)).astype(U), (seed >> np.uint64(32)).astype(U), pixel, k, dd, DS.bits(pp)])
    assert_same(dev("roulette", rec), want, rec, "roulette")


def _path_ids(rng, m):
    seed = rng.integers(0, 1 << 64, m, dtype=np.uint64)
    return seed, DS.draw_words(rng, m) >> U(8), DS.draw_words(rng, m) >> U(20), rng.integers(0, 63, m).astype(U)


@gpu
def test_device_probe_dir_over_shininess():
    """Render.cuh:297-300 at 2000 shininess values between 1e-3 and 1e6, the shipped five, the ns at which 25 / ns crosses exp's cut-offs,
    and 0, -1, denormal, inf and NaN: det_expf(25 / ns) and the double chains around it, the reflection, the lobe and Ray's normalisation"""
    rng = np.random.default_rng(33)
    ns = np.tile(DS.shininess(), 2)
    m = len(ns)
    seed, pixel, k, depth = _path_ids(rng, m)
    arrived = (DS.normalized(rng.standard_normal((m, 3)).astype(F)) * rng.uniform(0.2, 30, (m, 1)).astype(F)).astype(F)
    n = np.tile(DS.random_units(), (2, 1))[:m].copy()
    sp = DS.special_vectors()
    n[:len(sp)] = sp                                        # (with ns of the grid's low end)
    arrived[len(sp):2 * len(sp)] = sp
    want = DS.probe_dir(seed, pixel, k, depth, ns, arrived, n)
    # the ordinary part: finite unit vectors and ns >= 3, where the lobe's angles (delta_phi = 120 deg x (e^(25 / ns) - 1) / (e - 1)) stay
    # below 8192 rad, the range in which det_sinf / det_cosf are accurate.  Below that -- the shipped Ns = 1 gives 9e10 rad -- the
    # reduction returns what its float arithmetic returns (beyond 1e20 rad NaN as well): deterministic, compared on bits, not a direction
    ordinary = (ns >= 3) & np.isfinite(ns) & (np.arange(m) >= 2 * len(sp))
    assert ordinary.sum() > 2400 and _no_nan(want[ordinary])
    assert np.abs(np.sqrt(DS.sqnorm(DS.fl(want[ordinary]).astype(np.float64))) - 1).max() < 1e-6
    rec = np.column_stack([(seed & np.uint64(0xffffffff)).astype(U), (seed >> np.uint64(32)).astype(U), pixel, k, depth, DS.bits(ns), DS.bits(arrived), DS.bits(n)])
    assert_same(dev("probe_dir", rec), want, rec, "probe_dir")


@gpu
def test_device_probe_term_over_shininess():
    """Render.cuh:306-311: det_log10f(ns) (its denormal branch included) and (double)log * 0.5 + 1, the hit position, the clamped cosine"""
    rng = np.random.default_rng(34)
    ns = np.tile(DS.shininess(), 2)
    m = len(ns)
    n, d = np.tile(DS.random_units(), (2, 1))[:m].copy(), DS.random_units(m, 302).copy()
    kd, ke = rng.uniform(0, 1, (m, 3)).astype(F), rng.uniform(0, 30, (m, 3)).astype(F)
    o, t = rng.uniform(-10, 10, (m, 3)).astype(F), rng.uniform(1e-3, 30, m).astype(F)
    t[:8] = [0.0, -0.0, 1e-30, -1.0, np.inf, np.nan, 1e-45, 3e38]
    ke[8:12] = 0.0
    kd[12:16, 1] = [np.nan, np.inf, -0.0, 1e-40]
    want = DS.probe_term(n, kd, ke, o, d, t, ns)
    ordinary = (ns > 0) & np.isfinite(ns) & (np.arange(m) >= 16)
    assert ordinary.sum() > 4000 and _no_nan(DS.bits(want[ordinary])) and (want[ordinary] > 0).any() and (want[ordinary] == 0).any()
    rec = np.column_stack([n, kd, ke, o, d, t, ns])
    assert_same(dev("probe_term", rec), want, rec, "probe_term")


@gpu
def test_device_indirect_step_and_seeds():
    """Render.cuh:293, :323 with the division by P_RR as whole waves inside the short division's guard, whole waves with p_rr = 0, and a
    mix; L of negative zeros; then the two seeds of the backward recursion"""
    rng = np.random.default_rng(35)
    m = 4096
    L, f_r = rng.uniform(0, 50, (m, 3)).astype(F), (rng.uniform(0, 1, (m, 3)) / np.pi).astype(F)
    cos, L_dir = rng.uniform(0, 1, m).astype(F), rng.uniform(0, 20, (m, 3)).astype(F)
    p = rng.choice(np.array([0.6, 0.8, 0.95, 1.0, np.nextafter(F(1), F(0))], dtype=F), m)
    ordinary = np.ones(m, dtype=bool)
    ordinary[256:1024] = False
    p[256:512] = 0.0                                     # four whole waves: x / 0 = inf, 0 / 0 = NaN
    L[256:320] = 0.0
    L[512:576] = -0.0                                    # a negative-zero L (and, below, L_dir): -0 / p + -0 = -0
    L_dir[512:544] = -0.0
    p[576:640] = [np.nan, np.inf, -0.6, 0.0] * 16
    cos[640:704] = 0.0
    L[704:768] *= F(1e36)                                # the product overflows: inf / p
    L[768:832] *= F(1e-40)                               # denormal numerators: outside the guard
    p[832:1024] = np.where(rng.random(192) < 0.5, F(0), p[832:1024])   # waves that diverge at the guard
    want = DS.indirect_step(L, f_r, cos, p, L_dir)
    assert _no_nan(DS.bits(want[ordinary])) and np.isnan(want[256:320]).all() and (DS.bits(want[512:544]) == 0x80000000).all()
    rec = np.column_stack([L, f_r, cos, p, L_dir])
    assert_same(dev("indirect_step", rec), want, rec, "indirect_step")
    v = _wide_vectors(36, 4096)
    v[200:204] = [[-0.0, -0.0, -0.0], [0.0, -0.0, 1.0], [np.nan, 1, 2], [np.inf, -np.inf, 0]]
    with np.errstate(invalid="ignore"):
        zero_plus = F(0) + v                                                             # 0 + L_dir (Render.cuh:237, :323): -0 becomes +0
    assert_same(dev("seed_direct", v), zero_plus, v, "seed_direct")
    deepest = np.resize(np.array([0, 1, 2, 63, 0xffffffff, 0], dtype=U), len(v))
    want = np.where((deepest == 0)[:, None], zero_plus, F(0)).astype(F)                  # Render.cuh:249-255
    rec = np.column_stack([deepest, DS.bits(v)])
    assert_same(dev("seed_emitter", rec), want, rec, "seed_emitter")
