"""GPU parity tests proper: the HIP path, called through the C ABI, against the CPU oracle.

Bar: bit-exact on the float mean-radiance buffer (the north star allows 1e-5; the
design makes it exact, so the tests assert exact and report max |delta|), exact RGB8.
"""
import os

import numpy as np
import pytest

import cudaraytracing_amd as crt
import oracle_lib as O
import parity_cases as PC
import util
from frames import renders  # noqa: F401
from parity_cases import _compare_room

pytestmark = pytest.mark.gpu

TOL = 1e-5  # north-star tolerance on the float radiance buffer


def test_device_present():
    assert crt.device_count() >= 1


@pytest.mark.parametrize("fn,lo,hi", [("sin", -50, 50), ("cos", -50, 50), ("tan", -1.5, 1.5), ("acos", -1, 1),
                                      ("exp", -30, 30), ("log10", 1e-6, 1e5), ("sincos_s", -50, 50),
                                      ("sincos_c", -50, 50)])
def test_device_math_matches_oracle(fn, lo, hi):
    rng = np.random.default_rng(7)
    x = rng.uniform(lo, hi, 200000).astype(np.float32)
    x[:8] = [0.0, -0.0, lo, hi, 1.0, -1.0, 0.5, -0.5]
    got = crt.device_math(fn, x)
    ref = O.math_fn({"sincos_s": "sin", "sincos_c": "cos"}.get(fn, fn), x)
    assert np.array_equal(util.bits(got), util.bits(ref))


def test_device_math_two_arg_and_uniform():
    rng = np.random.default_rng(8)
    y = rng.normal(size=100000).astype(np.float32)
    x = rng.normal(size=100000).astype(np.float32)
    x[:4] = 0.0
    assert np.array_equal(util.bits(crt.device_math("atan2", y, x)), util.bits(O.math_fn("atan2", y, x)))
    c = rng.uniform(0, 1, 100000).astype(np.float32)
    c[:3] = [0.0, 1.0, 0.5]
    e = np.full_like(c, 0.6)
    assert np.array_equal(util.bits(crt.device_math("pow", c, e)), util.bits(O.math_fn("pow", c, e)))
    u = rng.integers(0, 2**32, 100000, dtype=np.uint64).astype(np.uint32)
    u[:3] = [0, 0xFFFFFFFF, 0x80000000]
    got = crt.device_math("uniform", u.view(np.float32))
    ref = (u.astype(np.float32) * np.float32(2.3283064365386963e-10) + np.float32(1.1641532182693481e-10)).astype(np.float32)
    assert np.array_equal(util.bits(got), util.bits(ref))
    assert got.min() > 0.0 and got.max() <= 1.0


def test_short_reciprocal_is_the_division_for_every_input():
    # the kernels compute 1/det and 1/direction as v_rcp_f32 + one Newton step in FMA; inside the guarded exponent range the
    # bits must equal those of the IEEE division for ALL inputs (outside it the kernels take the division itself)
    inside, outside = crt.device_rcp_check()
    assert inside == 0
    assert outside > 0  # (zero / denormal / huge / infinite inputs do differ: the guard is not vacuous)


def test_short_division_is_the_ieee_quotient():
    """unit3 / div3 of the kernels divide three numerators by one positive divisor as an exact reciprocal plus Markstein's correction
    (crt_device.h: quot3_exact; all 2^46 mantissa pairs were checked on gfx950 by tools/exhaustive/div_pair_check.hip) inside an
    exponent guard, the IEEE division outside it.  Here: the entry point against numpy's float32 division, bit for bit, on random
    operands over the whole exponent range, on the guard's borders, zeros of both signs, denormals, infinities and NaNs."""
    rng = np.random.default_rng(11)
    def bits(u):
        return np.asarray(u, dtype=np.uint32).view(np.float32)
    a = [bits(rng.integers(0, 2**32, 400000, dtype=np.uint64).astype(np.uint32)),            # anything, incl. NaN / inf / denormals
         (rng.standard_normal(400000) * np.exp2(rng.integers(-70, 70, 400000))).astype(np.float32)]
    b = [bits(rng.integers(0, 2**32, 400000, dtype=np.uint64).astype(np.uint32)),
         np.abs(rng.standard_normal(400000) * np.exp2(rng.integers(-70, 70, 400000))).astype(np.float32)]
    edge = np.array([0.0, -0.0, 1.0, -1.0, 2.0**-64, np.nextafter(np.float32(2.0**-64), np.float32(0)), 2.0**62, np.nextafter(np.float32(2.0**62), np.float32(0)),
                     2.0**-62, 2.0**60, 1e-45, -1e-45, 1e-38, 3.4e38, np.inf, -np.inf, np.nan, 0.6, 1.0 / 3.0, 16777215.0], dtype=np.float32)
    ea, eb = np.meshgrid(edge, edge)
    a.append(ea.reshape(-1).copy()); b.append(eb.reshape(-1).copy())
    a, b = np.concatenate(a), np.concatenate(b)
    with np.errstate(all="ignore"):
        ref = (a / b).astype(np.float32)
    for fn in ("div_short", "div_short_bounded"):
        aa, bb, rr = a, b, ref
        if fn == "div_short_bounded":   # the form unit3 uses relies on |numerator| <= divisor (a component of v over |v|)
            keep = ~(np.abs(a) > np.abs(b))
            aa, bb, rr = a[keep], b[keep], ref[keep]
        got = crt.device_math(fn, aa, bb)
        same = (got.view(np.uint32) == rr.view(np.uint32)) | (np.isnan(got) & np.isnan(rr))
        assert same.all(), (fn, aa[~same][:5], bb[~same][:5], got[~same][:5], rr[~same][:5])
        assert len(aa) > 300000


def test_device_philox_matches_oracle_and_kat():
    ctr = np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]], dtype=np.uint32)
    key = np.array([[0, 0], [0xFFFFFFFF] * 2, [0xA4093822, 0x299F31D0]], dtype=np.uint32)
    got = crt.device_philox(ctr, key)
    kat = np.array([[0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD],
                    [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]], dtype=np.uint32)
    assert np.array_equal(got, kat)
    rng = np.random.default_rng(3)
    c = rng.integers(0, 2**32, (4096, 4), dtype=np.uint64).astype(np.uint32)
    k = rng.integers(0, 2**32, (4096, 2), dtype=np.uint64).astype(np.uint32)
    got = crt.device_philox(c, k)
    ref = np.stack([O.philox(c[i], k[i]) for i in range(0, 4096, 37)])
    assert np.array_equal(got[::37], ref)


@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
@pytest.mark.parametrize("mode", [crt.TRAVERSAL_REFERENCE, crt.TRAVERSAL_FAST, crt.TRAVERSAL_EXACT])
def test_intersect_matches_oracle(renders, name, mode):
    o, d = util.random_rays(name, 4096, seed=11)
    tri, t = renders[name].intersect(o, d, traversal=mode)
    otri, ot, _ = util.oracle_scene(name).intersect(o, d)
    assert np.array_equal(tri, otri)
    assert np.array_equal(util.bits(t), util.bits(ot))
    assert (tri >= 0).sum() > 1000


CROPS = {"cornell-box": [(368, 268, 64, 48), (0, 0, 32, 24), (768, 576, 32, 24), (150, 330, 48, 32)],
         "veach-mis": [(368, 268, 64, 48), (250, 150, 48, 32), (100, 400, 48, 32)]}


@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
@pytest.mark.parametrize("mode", [crt.TRAVERSAL_REFERENCE, crt.TRAVERSAL_FAST, crt.TRAVERSAL_EXACT])
def test_render_crops_match_oracle(renders, name, mode):
    """800x600 at the scene's own config (C1 for cornell): crops against the oracle."""
    t = util.task(name)
    eye, iv, fov = util.camera(name)
    r = renders[name]
    r.traversal = mode
    r.set_spp(4)
    rgb = r.run_view(eye, iv, fov)
    mean = r.mean_buffer
    assert r.stats["paths"] == 800 * 600 * 4
    osc = util.oracle_scene(name)
    for (x0, y0, cw, ch) in CROPS[name]:
        orgb, omean, _, st = osc.render(eye, iv, fov, t.width, t.height, 4, t.P_RR, t.light_sample_n, seed=0,
                                        crop=(x0, y0, cw, ch))
        g = mean[y0:y0 + ch, x0:x0 + cw]
        delta = np.abs(g.astype(np.float64) - omean.astype(np.float64))
        n_bad = int((~(delta <= TOL)).any(axis=2).sum())
        assert n_bad == 0, "%s crop %s: %d pixels beyond %g (max %g)" % (name, (x0, y0, cw, ch), n_bad, TOL, np.nanmax(delta))
        assert np.array_equal(util.bits(g), util.bits(omean)), "float buffer not bit-identical"
        assert np.array_equal(rgb[y0:y0 + ch, x0:x0 + cw], orgb)


@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_small_full_frame_matches_oracle_with_counters(renders, name, monkeypatch):
    """Whole 96x72 frame incl. ragged 8x8 tiles, ray counters against the oracle's."""
    t = util.task(name)
    eye, iv, fov = util.camera(name)
    r = renders[name]
    r.traversal = crt.TRAVERSAL_REFERENCE
    r.set_spp(3)
    w, h = 100, 75  # not multiples of 8
    rgb = r.run_view(eye, iv, fov, stats=True, width=w, height=h)
    orgb, omean, _, st = util.oracle_scene(name).render(eye, iv, fov, w, h, 3, t.P_RR, t.light_sample_n)
    assert np.array_equal(util.bits(r.mean_buffer), util.bits(omean))
    assert np.array_equal(rgb, orgb)
    for k in ("paths", "rays", "shadow_rays", "probe_rays", "inner_pops", "leaf_pops", "tri_tests", "hits"):
        assert r.stats[k] == st[k], k
    for mode in (crt.TRAVERSAL_FAST, crt.TRAVERSAL_EXACT):
        r.traversal = mode
        rgb2 = r.run_view(eye, iv, fov, stats=True, width=w, height=h)
        assert np.array_equal(util.bits(r.mean_buffer), util.bits(omean))
        assert np.array_equal(rgb2, orgb)
        assert r.stats["rays"] == st["rays"]
        if mode == crt.TRAVERSAL_EXACT:
            exact_visits = (r.stats["inner_pops"], r.stats["leaf_pops"])
        else:
            fast_visits = (r.stats["inner_pops"], r.stats["leaf_pops"])
    # pruning only ever removes visits -- between two walks in the same order: with the leaves decoupled (EXACT's default form) an any-hit
    # ray meets its leaves in another order than FAST's and may stop earlier, so the comparison is with EXACT in the coupled form
    if os.environ.get("CRT_DEC") != "1":
        monkeypatch.setenv("CRT_DEC", "0")
        r.traversal = crt.TRAVERSAL_EXACT
        rgb3 = r.run_view(eye, iv, fov, stats=True, width=w, height=h)
        assert np.array_equal(rgb3, orgb) and r.stats["rays"] == st["rays"]
        assert r.stats["inner_pops"] >= fast_visits[0] and r.stats["leaf_pops"] >= fast_visits[1]
        monkeypatch.delenv("CRT_DEC")


@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_fast_equals_reference_full_frame(renders, name):
    """Full 800x600 frame: pruned/any-hit traversal is bit-identical to the exhaustive one."""
    eye, iv, fov = util.camera(name)
    r = renders[name]
    r.set_spp(8)
    r.traversal = crt.TRAVERSAL_REFERENCE
    r.run_view(eye, iv, fov)
    ref = r.mean_buffer.copy()
    ref_rays = r.stats["rays"]
    for mode in (crt.TRAVERSAL_FAST, crt.TRAVERSAL_EXACT):  # (EXACT: the fast traversal without its pruning rule, provably identical)
        r.traversal = mode
        r.run_view(eye, iv, fov)
        assert np.array_equal(util.bits(ref), util.bits(r.mean_buffer)), mode
        assert r.stats["rays"] == ref_rays


def test_seed_changes_image_and_is_reproducible(renders):
    eye, iv, fov = util.camera("cornell-box")
    r = renders["cornell-box"]
    r.traversal = crt.TRAVERSAL_EXACT
    r.set_spp(2)
    a = r.run_view(eye, iv, fov, width=160, height=120).copy()
    b = r.run_view(eye, iv, fov, width=160, height=120).copy()
    r.seed = 1234567890123
    c = r.run_view(eye, iv, fov, width=160, height=120).copy()
    orgb, omean, _, _ = util.oracle_scene("cornell-box").render(eye, iv, fov, 160, 120, 2, 0.6, 2, seed=1234567890123)
    r.seed = 0
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)
    assert np.array_equal(c, orgb)


def test_sharded_render_reassembles(renders):
    """world=3 tile shards written in compact tile order reassemble to the single-GPU image."""
    import ctypes as C
    from cudaraytracing_amd import _capi as capi
    from cudaraytracing_amd.distributed import untile_numpy
    eye, iv, fov = util.camera("veach-mis")
    r = renders["veach-mis"]
    r.traversal = crt.TRAVERSAL_EXACT
    r.set_spp(2)
    w, h = 200, 150
    full = r.run_view(eye, iv, fov, width=w, height=h).copy()
    world = 3
    shards = []
    for rank in range(world):
        slots = crt.shard_slots(w, h, rank, world)
        buf = np.zeros((slots, 3), dtype=np.uint8)
        prm = r._params(rank=rank, world=world, flags=capi.FLAG_TILED_OUTPUT, width=w, height=h)
        cam = r._cam(eye, iv, fov)
        capi.check(capi.lib().crt_render(r._h, C.byref(cam), C.byref(prm), capi.ptr(buf), None, None), "crt_render")
        shards.append(buf)
    img = untile_numpy(np.stack(shards), w, h)
    assert np.array_equal(img, full)


def test_cli_renders_config_to_png(tmp_path):
    """Headless replacement of the reference's GUI shell: config.json -> PNG, identical to the oracle."""
    import subprocess
    from PIL import Image
    from cudaraytracing_amd import build as b
    cli = b.build_cli()
    out = str(tmp_path / "veach.png")
    cfg = util.SCENES["veach-mis"]
    r = subprocess.run([cli, cfg, "-o", out, "--spp", "2", "--width", "96", "--height", "72", "--seed", "42", "--base-dir", util.ROOT],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "render cost:" in r.stdout
    t = util.task("veach-mis")
    eye, iv, fov = util.camera("veach-mis")
    orgb, _, _, _ = util.oracle_scene("veach-mis").render(eye, iv, fov, 96, 72, 2, t.P_RR, t.light_sample_n, seed=42)
    assert np.array_equal(np.asarray(Image.open(out)), orgb)
    bad = subprocess.run([cli, str(tmp_path / "missing.json")], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and "unable to open config" in bad.stderr


def test_bench_with_two_ranks_on_one_device(renders, tmp_path):
    """The N > 1 path of bench.py -- one process per rank, sharded render, all-gather, max-over-ranks timing, rank 0's JSON
    line -- with both ranks on this box's one GPU over gloo (CRT_BENCH_ONE_DEVICE: RCCL refuses two ranks on a device).
    The ranks' ray counts must add up to the whole frame's, and the gathered image must be the one-GPU image."""
    import json
    import subprocess
    import sys
    from PIL import Image
    png = str(tmp_path / "two.png")
    env = dict(os.environ, CRT_BENCH_ONE_DEVICE="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29641", os.path.join(util.ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--spp", "4",
           "--width", "200", "--height", "152", "--no-cpu-baseline", "--save-png", png]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=util.ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["steps"] == 1 and line["scaling"] == "strong"
    name = "cornell-box"
    eye, iv, fov = util.camera(name)
    one = renders[name]
    one.set_spp(4)
    one.traversal = crt.TRAVERSAL_EXACT
    rgb = one.run_view(eye, iv, fov, width=200, height=152)
    assert line["rays_per_frame"] == one.stats["rays"]
    assert np.array_equal(np.asarray(Image.open(png)), rgb)


def test_errors_are_reported_not_printed(renders):
    import ctypes as C
    from cudaraytracing_amd import _capi as capi
    r = renders["cornell-box"]
    eye, iv, fov = util.camera("cornell-box")
    cam = r._cam(eye, iv, fov)
    buf = np.zeros((8, 8, 3), dtype=np.uint8)
    prm = r._params(width=8, height=8)
    prm.spp = 0
    assert capi.lib().crt_render(r._h, C.byref(cam), C.byref(prm), capi.ptr(buf), None, None) == -1
    prm = r._params(rank=1, world=2, width=8, height=8)  # world > 1 needs the tiled layout
    assert capi.lib().crt_render(r._h, C.byref(cam), C.byref(prm), capi.ptr(buf), None, None) == -1
    with pytest.raises(crt.CrtError):
        crt.Render(util.host_scene("cornell-box"), device=99)


# ----------------------------------------------------------------------------------------------
# Edge cases the reference's data model allows: other leaf sizes (bvh_thresh_n), no / several NEE
# samples, paths that run into the 64-vertex bounce cap, one-leaf trees, every pipeline variant.
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thresh", [1, 2, 3, 5, 20, 200])
def test_other_leaf_sizes(tmp_path, thresh):
    PC.room_matches_oracle_at_leaf_size(tmp_path, thresh)


def test_leaf_of_300_triangles(tmp_path):
    PC.room_that_is_one_leaf_of_300_triangles_matches_oracle(tmp_path)


def test_room_of_180000_triangles(tmp_path):
    PC.room_of_180000_triangles_matches_oracle(tmp_path)


@pytest.mark.parametrize("thresh", [1, 2, 4])
def test_triangle_soup_with_ties_and_degenerate_triangles(tmp_path, thresh):
    PC.soup_with_ties_and_degenerate_triangles_matches_oracle(tmp_path, thresh)


@pytest.mark.parametrize("scale", [1e-12, 1e12, 1e17])
def test_extreme_coordinate_scales(tmp_path, scale):
    PC.scaled_soup_matches_oracle(tmp_path, scale)


@pytest.mark.parametrize("specular", [False, True])
def test_rays_with_non_finite_operands_take_the_reference_arithmetic(tmp_path, specular):
    PC.room_with_every_ray_on_the_reference_arithmetic_matches_oracle(tmp_path, specular)


def test_scene_without_emitters(tmp_path):
    """No light object at all (DeviceLights with ln = 0): every vertex has zero next-event samples; the frame is black."""
    st = _compare_room(tmp_path, 2, lsn=2, p_rr=0.7, spp=2, light=False)
    assert st["shadow_rays"] == 0 and st["rays"] > 3000


@pytest.mark.parametrize("lsn", [0, 1, 3])
def test_light_sample_counts(tmp_path, lsn):
    st = _compare_room(tmp_path, 2, lsn=lsn, p_rr=0.6, spp=3)
    assert (st["shadow_rays"] == 0) == (lsn == 0)


def test_paths_hit_the_bounce_stack_cap(tmp_path):
    """P_RR = 1 never terminates a path by roulette: closed room -> every path runs to the 64-vertex cap
    (DeviceStack overflow semantics, Render.cuh:210) unless it finds the light first."""
    st = _compare_room(tmp_path, 2, lsn=1, p_rr=1.0, spp=1, w=24, h=18)
    assert st["max_depth"] == 63


def test_specular_probe_rays(tmp_path):
    st = _compare_room(tmp_path, 2, lsn=2, p_rr=0.8, spp=4, specular=True)
    assert st["probe_rays"] > 0


@pytest.mark.parametrize("pipeline", ["2", "4"])
def test_all_pipeline_variants_agree(renders, pipeline, monkeypatch):
    """CRT_PIPELINE selects k_mega3 (4, default) or the wavefront rounds (2: k_logic + k_trace, scalar box / triangle tests)."""
    monkeypatch.setenv("CRT_PIPELINE", pipeline)
    for name in ("cornell-box", "veach-mis"):
        t = util.task(name)
        eye, iv, fov = util.camera(name)
        r = renders[name]
        r.traversal = crt.TRAVERSAL_EXACT
        r.set_spp(2)
        rgb = r.run_view(eye, iv, fov, width=128, height=96)
        orgb, omean, _, st = util.oracle_scene(name).render(eye, iv, fov, 128, 96, 2, t.P_RR, t.light_sample_n)
        assert np.array_equal(util.bits(r.mean_buffer), util.bits(omean))
        assert np.array_equal(rgb, orgb) and r.stats["rays"] == st["rays"]


@pytest.mark.parametrize("pipeline", ["2", "4"])
def test_progressive_ranges_equal_one_shot(renders, pipeline, monkeypatch):
    """crt_render_range: samples rendered in ascending ranges accumulate in the reference's order (Render.cuh:348), so the
    frame after the last range is the one-shot frame, bit for bit; ray counts add up."""
    monkeypatch.setenv("CRT_PIPELINE", pipeline)
    name = "veach-mis"
    eye, iv, fov = util.camera(name)
    r = renders[name]
    r.traversal = crt.TRAVERSAL_EXACT
    r.set_spp(7)
    ref = r.run_view(eye, iv, fov, width=96, height=72).copy()
    ref_mean, ref_rays = r.mean_buffer.copy(), r.stats["rays"]
    rays, out = 0, None
    for b, c in ((0, 2), (2, 1), (3, 4)):
        out = r.run_view_range(eye, iv, fov, b, c, width=96, height=72)
        rays += r.stats["rays"]
        assert (out is None) == (b + c < 7)
    assert np.array_equal(out, ref) and np.array_equal(util.bits(r.mean_buffer), util.bits(ref_mean)) and rays == ref_rays
    with pytest.raises(crt.CrtError):
        r.run_view_range(eye, iv, fov, 5, 3, width=96, height=72)   # beyond spp


@pytest.mark.parametrize("pipeline", ["2", "4"])
def test_previews_of_a_progressive_render(renders, pipeline, monkeypatch):
    """crt_preview (the viewer half of SURVEY 8(f) row 4; the reference shows nothing until all spp are done,
    src/main.cu:368-377): after `done` samples the preview is the estimate from those samples -- the frame a render with
    spp = done produces, up to the rounding of (sum L_k / spp) * spp / done -- and taking previews, any number of them,
    leaves the final frame's bits untouched."""
    monkeypatch.setenv("CRT_PIPELINE", pipeline)
    name = "cornell-box"
    eye, iv, fov = util.camera(name)
    r = renders[name]
    r.traversal = crt.TRAVERSAL_EXACT
    w, h, spp = 96, 72, 12
    r.set_spp(spp)
    ref = r.run_view(eye, iv, fov, width=w, height=h).copy()
    ref_mean = r.mean_buffer.copy()
    with pytest.raises(crt.CrtError):
        r.preview(width=w, height=h)  # nothing in flight after a complete frame
    done_at = []
    out = None
    for b, c in ((0, 1), (1, 4), (5, 3), (8, 4)):
        out = r.run_view_range(eye, iv, fov, b, c, width=w, height=h)
        if b + c < spp:
            for _ in range(2):  # twice: a preview must not feed back into the accumulator
                rgb, mean, done = r.preview(want_mean=True, width=w, height=h)
            assert done == b + c
            done_at.append((done, rgb.copy(), mean.copy()))
    assert np.array_equal(out, ref) and np.array_equal(util.bits(r.mean_buffer), util.bits(ref_mean))
    with pytest.raises(crt.CrtError):
        r.preview(width=w, height=h)
    for done, rgb, mean in done_at:  # against a one-shot render of the same samples
        r.set_spp(done)
        one = r.run_view(eye, iv, fov, width=w, height=h).astype(np.int32)
        om = r.mean_buffer
        assert np.allclose(mean, om, rtol=2e-5, atol=1e-6), done
        assert np.abs(rgb.astype(np.int32) - one).max() <= 1, done
    r.set_spp(2)


@pytest.mark.parametrize("pipeline", ["2", "4"])
def test_samples_rendered_in_chunks_equal_one_launch(renders, pipeline, monkeypatch):
    """Frames with more work items than the per-item radiance buffer holds are rendered in chunks of samples (one launch each)
    that accumulate in sample order: forced here with a tiny buffer (7 samples -> 4 launches)."""
    monkeypatch.setenv("CRT_PIPELINE", pipeline)
    name = "cornell-box"
    eye, iv, fov = util.camera(name)
    r = renders[name]
    r.set_spp(7)
    r.traversal = crt.TRAVERSAL_EXACT
    one = r.run_view(eye, iv, fov, width=64, height=48).copy()
    mean_one = r.mean_buffer.copy()
    launches_one = r.stats["kernel_launches"]
    monkeypatch.setenv("CRT_CHUNK_LOG2", "13")  # 8192 items: two samples of 64 x 48 pixels per launch
    many = r.run_view(eye, iv, fov, width=64, height=48)
    assert np.array_equal(util.bits(r.mean_buffer), util.bits(mean_one))
    assert np.array_equal(many, one)
    if pipeline == "4":
        assert launches_one == 1 and r.stats["kernel_launches"] == 4


def test_zero_contribution_samples_are_answered_without_traversal(renders):
    """The default mode (CRT_TRAVERSAL_EXACT) and FAST answer next-event samples whose contribution is exactly zero without tracing
    them (adding +0 cannot change L_dir): same frame, same reference ray counts, with and without CRT_FLAG_TRACE_ALL; REFERENCE
    traces everything."""
    for name in ("cornell-box", "veach-mis"):
        t = util.task(name)
        eye, iv, fov = util.camera(name)
        r = renders[name]
        r.set_spp(3)
        out = {}
        for key, trav, flags in (("exact", crt.TRAVERSAL_EXACT, 0), ("exact_all", crt.TRAVERSAL_EXACT, crt.FLAG_TRACE_ALL), ("fast", crt.TRAVERSAL_FAST, 0),
                                 ("fast_all", crt.TRAVERSAL_FAST, crt.FLAG_TRACE_ALL), ("ref", crt.TRAVERSAL_REFERENCE, 0)):
            r.traversal, r.extra_flags = trav, flags
            rgb = r.run_view(eye, iv, fov, width=160, height=120)
            out[key] = (rgb.copy(), r.mean_buffer.copy(), dict(r.stats))
        r.traversal, r.extra_flags = crt.TRAVERSAL_EXACT, 0
        for key in ("exact_all", "fast", "fast_all", "ref"):
            assert np.array_equal(out[key][0], out["exact"][0]) and np.array_equal(util.bits(out[key][1]), util.bits(out["exact"][1])), key
            assert out[key][2]["rays"] == out["exact"][2]["rays"] and out[key][2]["shadow_rays"] == out["exact"][2]["shadow_rays"], key
        for key in ("exact_all", "fast_all", "ref"):
            assert out[key][2]["rays_untraced"] == 0, key
        un = out["exact"][2]["rays_untraced"]
        assert 0 < un < out["exact"][2]["shadow_rays"] and un == out["fast"][2]["rays_untraced"]
        orgb, omean, _, st = util.oracle_scene(name).render(eye, iv, fov, 160, 120, 3, t.P_RR, t.light_sample_n)
        assert np.array_equal(util.bits(out["exact"][1]), util.bits(omean)) and out["exact"][2]["rays"] == st["rays"]


def test_baseline_size_frame_properties(renders):
    """BASELINE configuration C2 at full size (cornell-box 800x600 spp 512, 1.1 G rays) in the DEFAULT mode (CRT_TRAVERSAL_EXACT, the
    mode the benchmark number is quoted in): the same mode with every sample traced, FAST with and without that, the exhaustive
    REFERENCE traversal and a render split into progressive ranges give the same frame -- float bits of the mean buffer -- and the
    same ray counts."""
    name = "cornell-box"
    eye, iv, fov = util.camera(name)
    r = renders[name]
    r.set_spp(512)
    r.traversal, r.extra_flags = crt.TRAVERSAL_EXACT, 0
    rgb = r.run_view(eye, iv, fov).copy()
    mean, st = r.mean_buffer.copy(), dict(r.stats)
    assert st["paths"] == 800 * 600 * 512 and st["rays"] > 10 ** 9 and 0 < st["rays_untraced"] < st["shadow_rays"]
    for trav, flags in ((crt.TRAVERSAL_EXACT, crt.FLAG_TRACE_ALL), (crt.TRAVERSAL_FAST, 0), (crt.TRAVERSAL_FAST, crt.FLAG_TRACE_ALL), (crt.TRAVERSAL_REFERENCE, 0)):
        r.traversal, r.extra_flags = trav, flags
        rgb2 = r.run_view(eye, iv, fov)
        assert np.array_equal(rgb2, rgb) and np.array_equal(util.bits(r.mean_buffer), util.bits(mean)), (trav, flags)
        assert r.stats["rays"] == st["rays"] and r.stats["shadow_rays"] == st["shadow_rays"], (trav, flags)
        assert r.stats["rays_untraced"] == (st["rays_untraced"] if (trav, flags) == (crt.TRAVERSAL_FAST, 0) else 0), (trav, flags)
    r.traversal, r.extra_flags = crt.TRAVERSAL_EXACT, 0
    out = None
    for b, c in ((0, 100), (100, 156), (256, 256)):
        out = r.run_view_range(eye, iv, fov, b, c)
    assert np.array_equal(out, rgb) and np.array_equal(util.bits(r.mean_buffer), util.bits(mean))
    assert np.isfinite(mean).all() and mean.min() >= 0.0
