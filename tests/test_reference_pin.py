"""The oracle -- and through it k_mega3, the wavefront pipeline and crt_intersect -- pinned to the REFERENCE's own path code.

tests/golden/reference_pin/ holds what the reference's loader, BVH builder, DeviceBVH::intersect, blocked(), cast_ray_v2 and
view_render_kernel compute when they are compiled from where they lie and run on the CPU (oracle/ref_probe/path_probe.cpp), fed with
the oracle's random draws (a tape of raw 32-bit words in the order of the reference's sequential per-pixel stream) and the oracle's
transcendental functions (oracle/ref_probe/det_libm.cpp).  With those two inputs equal, the reference's own instructions have no
excuse to differ from the oracle in a single bit, so every comparison here is on bits: no tolerance, no allclose.

CPU tests: from the fixtures always -- first that the oracle regenerates the stored tapes, rays and flags bit for bit (the draw
order), then radiance, bytes, hits and trees; and live, when oracle/_ref/path_probe exists (`make -C oracle` on a machine with the
reference tree): the probe is brought up to date, re-run on the fixtures' inputs and must reproduce the fixtures' outputs.
GPU tests (fixtures only): crt_intersect against the reference's recorded hits and verdicts, Render.run_view against the reference's
recorded per-path radiance and bytes, in the default kernel, the wavefront pipeline and the coupled / 32-bit forms of k_mega3.

The one exclusion (docs/experiments.md "Pinned to the reference's own code"): Render.cuh:311-312 keeps an Eigen
expression in `auto` whose operands are temporaries, so what the optimised reference computes on a path that takes the emitter-probe
branch (Render.cuh:304-313) is not defined by the language.  The oracle flags those paths.  Where the fixtures record that the -O2
build disagrees on them (16 of 3072 and 16 of 1536 paths of two veach-mis cases), exactly the flagged paths, and the pixels that hold
one, are left out of the comparison with the -O2 outputs -- and are compared instead, every one, with the outputs of the same
program built with -O0 -fstack-reuse=none, where each temporary keeps its stack slot and the code computes what the text means.
Loader.h:89-103 has the same defect (kd of a map_Kd triangle): the textured scene is recorded from that unoptimised build, and the
comparison with the -O2 build is kept as a strict xfail."""
import numpy as np
import pytest

import cudaraytracing_amd as crt
import reference_pin as RP
import util
from blocked_restated import _oracle_blocked

META = RP.load_meta()
SCENE_IDS = [c[0] for c in RP.SCENE_CASES]
live = pytest.mark.skipif(not RP.have_probe(), reason="oracle/_ref/path_probe is not built (needs the reference tree: make -C oracle)")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("reference_pin"))


@pytest.fixture(scope="module")
def probe_ready():
    RP.rebuild_probe()


_specs, _frames, _gold = {}, {}, {}


def spec_of(name, tmp, thresh=None):
    key = (name, thresh)
    if key not in _specs:
        _specs[key] = RP.SceneSpec(name, tmp, thresh)
    return _specs[key]


def gold(name):
    if name not in _gold:
        _gold[name] = RP.load(name)
    return _gold[name]


def case_of(cid):
    return [c for c in RP.FRAME_CASES if c["id"] == cid][0]


def case_frame(cid, tmp):
    """the oracle's frame of a case with its draw log: computed once, shared, never changed"""
    if cid not in _frames:
        case = case_of(cid)
        _frames[cid] = RP.oracle_frame(spec_of(case["scene"], tmp), case)
    return _frames[cid]


def excluded_paths(cid):
    """exactly the flagged paths of a case whose fixtures record a disagreement of the -O2 build; nothing else, ever"""
    g, m = gold("frame_" + cid), META["frames"][cid]
    flagged = g["flags"] == 1
    assert int(flagged.sum()) == m["flagged_paths"]
    return flagged if not m["emitter_probe_paths_agree"] else np.zeros_like(flagged)


# ------------------------------------------------------------------------------------------------ the fixtures themselves
def test_the_cases_are_the_ones_recorded():
    assert sorted(META["frames"]) == sorted(RP.FRAME_IDS) and sorted(META["scenes"]) == sorted(SCENE_IDS)
    for case in RP.FRAME_CASES:
        assert {k: META["frames"][case["id"]][k] for k in case} == case
    assert META["emitter_probe_paths_agree"] == all(m["emitter_probe_paths_agree"] for m in META["frames"].values())


@pytest.mark.parametrize("cid", SCENE_IDS)
def test_scene_files_are_the_ones_the_reference_read(cid, tmp):
    _, name, thresh = [c for c in RP.SCENE_CASES if c[0] == cid][0]
    assert spec_of(name, tmp, thresh).file_hashes() == META["scenes"][cid]["files_sha1"]


@pytest.mark.parametrize("cid", RP.FRAME_IDS)
def test_flagged_paths_stay_within_their_bounds(cid):
    """cornell-box (all Ns 1): no path is flagged or excluded.  veach-mis: at most a quarter of a case's paths."""
    g, m = gold("frame_" + cid), META["frames"][cid]
    flagged = g["flags"] == 1
    if m["scene"] != "veach-mis":
        assert not flagged.any() and not excluded_paths(cid).any()
    assert flagged.mean() <= RP.MAX_FLAGGED
    assert excluded_paths(cid).sum() <= flagged.sum()
    if flagged.any():   # every flagged path has its record from the unoptimised build, and that build agreed with the oracle when recorded
        assert len(g["flagged_L_unopt"]) == flagged.sum() and m["emitter_probe_paths_agree_unoptimised"] is True
    print("%s: %d paths, %d flagged, %d excluded from the -O2 comparison" % (cid, flagged.size, flagged.sum(), excluded_paths(cid).sum()))


# ------------------------------------------------------------------------------------------------ draw order
@pytest.mark.parametrize("cid", RP.FRAME_IDS)
def test_oracle_regenerates_tapes_rays_and_flags(cid, tmp):
    """The tape is the reference's sequential stream: the two jitters, then per vertex RR and -- only if the path goes on -- x_1, x_2;
    on the way back per vertex the triangle pick, alpha, beta of every next-event sample and the probe's two uniforms.  The probe
    consumed exactly these words in exactly this order when the fixtures were made (it fails when a tape runs out, and the number it
    consumed is compared below), so an oracle that draws another number of words, or in another order, regenerates another tape."""
    g, of = gold("frame_" + cid), case_frame(cid, tmp)
    assert np.array_equal(of["lens"], g["lens"]), "words per path"
    assert np.array_equal(of["words"], g["words"]), "tape"
    assert np.array_equal(of["flags"], g["flags"]), "emitter-probe flags"
    assert same_bits(of["rays"], g["rays"]).all(), "camera rays"
    m = META["frames"][cid]
    assert (len(g["lens"]), len(g["words"]), of["stats"]["rays"], of["stats"]["max_depth"]) == (m["paths"], m["draws"], m["rays"], m["max_depth"])


def test_a_path_reaches_the_bounce_stack_cap(tmp):
    assert case_frame("room-cap-spp1-rr1-lsn1", tmp)["stats"]["max_depth"] == 63   # BOUNCE_STACK_SIZE - 1: the stack is full (Render.cuh:210)


# ------------------------------------------------------------------------------------------------ paths and frames
@pytest.mark.parametrize("cid", RP.FRAME_IDS)
def test_oracle_path_radiance_is_cast_ray_v2s(cid, tmp):
    g, of = gold("frame_" + cid), case_frame(cid, tmp)
    oL = of["L"].reshape(-1, 3)
    excl = excluded_paths(cid)
    same = same_bits(oL, g["L"]).all(axis=1)
    assert same[~excl].all(), "%d of %d unflagged paths differ from the reference (first: path %d)" % ((~same[~excl]).sum(), (~excl).sum(), np.nonzero(~same & ~excl)[0][0])
    # the words cast_ray_v2 consumed: the path's tape without the two jitters, exactly, on every path
    assert np.array_equal(g["used"], g["lens"] - 2) and np.array_equal(of["lens"] - 2, g["used"])
    flagged = g["flags"] == 1
    if flagged.any():   # every flagged path against the unoptimised build of the reference
        assert same_bits(oL[flagged], g["flagged_L_unopt"]).all()
    print("%s: %d paths compared with the -O2 reference, %d excluded; %d flagged paths compared with the unoptimised reference; %d draws" %
          (cid, (~excl).sum(), excl.sum(), flagged.sum(), len(g["words"])))


@pytest.mark.parametrize("cid", RP.FRAME_IDS)
def test_oracle_frame_bytes_are_view_render_kernels(cid, tmp):
    g, of, case = gold("frame_" + cid), case_frame(cid, tmp), case_of(cid)
    excl_px = excluded_paths(cid).reshape(-1, case["spp"]).any(axis=1).reshape(case["h"], case["w"])
    same = (of["rgb"] == g["rgb"]).all(axis=2)
    assert same[~excl_px].all(), "%d pixels differ from the reference" % (~same[~excl_px]).sum()
    # words view_render_kernel consumed per pixel: the tapes of its spp paths, jitter included, exactly, on every pixel
    assert np.array_equal(g["frame_used"], g["lens"].reshape(-1, case["spp"]).sum(axis=1))
    if "flagged_pixels" in g:
        px = g["flagged_pixels"]
        assert np.array_equal(np.nonzero((g["flags"] == 1).reshape(-1, case["spp"]).any(axis=1))[0], px)
        assert np.array_equal(of["rgb"].reshape(-1, 3)[px], g["flagged_rgb_unopt"])
    print("%s: %d pixels compared, %d excluded" % (cid, (~excl_px).sum(), excl_px.sum()))


# ------------------------------------------------------------------------------------------------ hits
@pytest.mark.parametrize("name", [c[0] for c in RP.INTERSECT_CASES])
def test_oracle_hits_are_device_bvh_intersects(name, tmp):
    """util.random_rays (axis-parallel directions, zero components, origins on box planes) plus the visibility queries of real
    next-event samples with their t_to_light = dist.x / dir.x: closest hit (triangle, t on its bits, pos, normal) and blocked()."""
    g = gold("intersect_" + name)
    seed = dict(RP.INTERSECT_CASES)[name]
    spec = spec_of(name, tmp)
    osc = util.oracle_scene(name)
    o, d, lim = RP.intersect_inputs(name, seed, spec, osc)
    assert same_bits(o, g["origin"]).all() and same_bits(d, g["dir"]).all() and same_bits(lim, g["limit"]).all(), "the rays are not the recorded ones"
    tri, t, _ = osc.intersect(o, d)
    hit = g["happend"] == 1
    assert np.array_equal(tri >= 0, hit)
    assert same_bits(t, g["t"]).all()
    assert np.array_equal(tri, g["tri"])
    nd = RP.ray_constructor(o, d)
    with np.errstate(all="ignore"):
        pos = o + t[:, None] * nd     # DeviceTriangle.cuh:50, one fp32 operation per ufunc
    blocked = _oracle_blocked(osc, o, d, lim)   # blocked() of Render.cuh:19-27 as the visibility tests of the kernels restate it
    assert pos.dtype == np.float32
    assert same_bits(pos[hit], g["pos"][hit]).all() and same_bits(osc.tris()["normal"][tri[hit]], g["normal"][hit]).all()
    assert not g["pos"][~hit].any() and not g["normal"][~hit].any()   # HitPayload() of a miss
    assert np.array_equal(blocked, g["blocked"] == 1)
    m = META["intersect"][name]
    assert (len(o), int(hit.sum()), int(blocked.sum())) == (m["rays"], m["hits"], m["blocked"])
    assert hit.sum() > 1000 and 0.2 < blocked.mean() < 0.8
    nee = slice(RP.N_RANDOM_RAYS, None)   # next-event queries: the hit on the light lies within rounding of the limit on many of them
    with np.errstate(all="ignore"):
        assert (np.abs(lim[nee] - t[nee]) < 1e-4).sum() > 100


# ------------------------------------------------------------------------------------------------ scenes
@pytest.mark.parametrize("cid", SCENE_IDS)
def test_oracle_scene_is_the_references(cid, tmp):
    """Loader, Object, Scene::set_BVH, DeviceBVH, DeviceLights: nodes (lc rc n it AA BB), root, triangles in BVH order, the lights'
    triangles in shape order -- every field on its bits (a digest per field; the dump itself where it is small)."""
    _, name, thresh = [c for c in RP.SCENE_CASES if c[0] == cid][0]
    m = META["scenes"][cid]
    dump = RP.oracle_scene_dump(spec_of(name, tmp, thresh).oracle())
    rec = RP.scene_record(dump)
    for k in ("n_nodes", "n_tris", "root", "lights"):
        assert rec[k] == m[k], k
    for part in ("nodes", "tris"):
        for f, digest in m[part].items():
            assert rec[part][f] == digest, "%s.%s differs from the reference's" % (part, f)
    assert rec["light_tris"] == m["light_tris"]
    if m["stored_whole"]:
        g = gold("scene_" + cid)
        assert dump["nodes"].tobytes() == g["nodes"].tobytes() and dump["tris"].tobytes() == g["tris"].tobytes()
        for i, l in enumerate(dump["lights"]):
            assert l.tobytes() == g["light%d" % i].tobytes()


@live
@pytest.mark.xfail(strict=True, reason="Loader.h:89,95,101 keep `Eigen::Vector3f(texels) / 255.` in `auto`: the operand is a temporary that is gone when "
                   "Loader.h:103 averages the three.  The compiled reference reads stale stack (kd = (9.7011074e+28, 1.2303007e+02, -4.0234160e-28) on the "
                   "first textured triangle in one run, other values in the next); the oracle evaluates the text eagerly (kd = (0.5124183, 0.7058824, "
                   "0.24313726) there), and so does the reference built with -O0 -fstack-reuse=none, which the textured case of the other tests records.")
def test_textured_kd_is_the_references(tmp, probe_ready):
    spec = spec_of("textured", tmp, 2)
    ref, mine = RP.probe_scene(spec, tmp, binary=RP.PROBE), RP.oracle_scene_dump(spec.oracle())
    assert same_bits(ref["tris"]["kd"], mine["tris"]["kd"]).all()


# ------------------------------------------------------------------------------------------------ live: the probe reproduces the fixtures
@live
@pytest.mark.parametrize("cid", SCENE_IDS)
def test_live_scene(cid, tmp, probe_ready):
    _, name, thresh = [c for c in RP.SCENE_CASES if c[0] == cid][0]
    rec, m = RP.scene_record(RP.probe_scene(spec_of(name, tmp, thresh), tmp)), META["scenes"][cid]
    assert {k: rec[k] for k in rec} == {k: m[k] for k in rec}


@live
@pytest.mark.parametrize("name", [c[0] for c in RP.INTERSECT_CASES])
def test_live_intersect(name, tmp, probe_ready):
    g = gold("intersect_" + name)
    hit = RP.probe_intersect(spec_of(name, tmp), g["origin"], g["dir"], g["limit"], tmp)
    assert np.array_equal(hit["happend"], g["happend"]) and np.array_equal(hit["tri"], g["tri"]) and np.array_equal(hit["blocked"], g["blocked"])
    assert same_bits(hit["t"], g["t"]).all() and same_bits(hit["pos"], g["pos"]).all() and same_bits(hit["normal"], g["normal"]).all()
    assert np.array_equal(hit["matches"], g["happend"])   # the triangle of every hit is the one triangle that reproduces it


@live
@pytest.mark.parametrize("cid", RP.FRAME_IDS)
def test_live_paths_and_frame(cid, tmp, probe_ready):
    g, case = gold("frame_" + cid), case_of(cid)
    spec = spec_of(case["scene"], tmp)
    excl = excluded_paths(cid)   # (what the -O2 build computes on them is stale stack: not recorded, not compared)
    excl_px = excl.reshape(-1, case["spp"]).any(axis=1)
    _, L, used, _ = RP.probe_paths(spec, case, g["rays"], g["lens"], g["words"], tmp)
    assert same_bits(L, g["L"])[~excl].all() and np.array_equal(used, g["used"])
    rgb, frame_used, _ = RP.probe_frame(spec, case, g["lens"], g["words"], tmp)
    assert np.array_equal(rgb[~excl_px], g["rgb"].reshape(-1, 3)[~excl_px]) and np.array_equal(frame_used, g["frame_used"])
    flagged = np.nonzero(g["flags"] == 1)[0]
    if len(flagged):
        lens, words = RP.path_tapes(g["lens"], g["words"], flagged)
        _, L0, used0, _ = RP.probe_paths(spec, case, g["rays"][flagged], lens, words, tmp, binary=RP.PROBE_O0)
        assert same_bits(L0, g["flagged_L_unopt"]).all() and np.array_equal(used0, g["used"][flagged])
        rgb0, _, _ = RP.probe_frame(spec, case, g["lens"], g["words"], tmp, pixels=g["flagged_pixels"], binary=RP.PROBE_O0)
        assert np.array_equal(rgb0, g["flagged_rgb_unopt"])


@live
def test_a_tape_one_word_short_fails_loudly(tmp, probe_ready):
    """The stand-in generator never hands out a silent zero: a path whose tape lacks its last word ends the probe with status 3."""
    cid = "veach-mis-spp2-rr0-lsn3"
    g, case = gold("frame_" + cid), case_of(cid)
    spec = spec_of(case["scene"], tmp)
    lens, words = RP.path_tapes(g["lens"], g["words"], np.arange(4))
    rc, L, used, err = RP.probe_paths(spec, case, g["rays"][:4], lens, words, tmp, check=False)
    assert rc == 0 and np.array_equal(used, lens - 2)
    short = lens.copy()
    short[3] -= 1
    rc, L, used, err = RP.probe_paths(spec, case, g["rays"][:4], short, words[:-1], tmp, check=False)
    assert rc == 3 and "tape ran out" in err and L is None


# ------------------------------------------------------------------------------------------------ GPU: the kernels against the recorded reference
KERNELS = {"default": {}, "wavefront": {"CRT_PIPELINE": "2"}, "coupled": {"CRT_DEC": "0"}, "decoupled-32": {"CRT_DEC": "1", "CRT_REF32": "1"}}
MODES = [crt.TRAVERSAL_REFERENCE, crt.TRAVERSAL_FAST, crt.TRAVERSAL_EXACT]


def _set_kernel(monkeypatch, kernel):
    for k in ("CRT_PIPELINE", "CRT_DEC", "CRT_REF16", "CRT_REF32", "CRT_IMPL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in KERNELS[kernel].items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def pinned_renders(tmp):
    out = {}
    for name in ("cornell-box", "veach-mis"):
        out[name] = crt.Render(util.host_scene(name), 1, 0.6, 1)
    spec = spec_of("room", tmp)
    out["room"] = crt.Render(spec.host_scene(4, 4), 1, 1.0, 1)
    yield out
    for r in out.values():
        r.free()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", [c[0] for c in RP.INTERSECT_CASES])
def test_gpu_intersect_gives_the_references_hits(pinned_renders, name, kernel, monkeypatch):
    """crt_intersect against DeviceBVH::intersect's recorded hit (triangle, t on its bits) and blocked()'s recorded verdict, in the
    three traversal modes"""
    g = gold("intersect_" + name)
    _set_kernel(monkeypatch, kernel)
    r = pinned_renders[name]
    for mode in MODES:
        tri, t = r.intersect(g["origin"], g["dir"], traversal=mode)
        assert np.array_equal(tri, g["tri"]), (kernel, mode)
        assert same_bits(t, g["t"]).all(), (kernel, mode)
        blk, _ = r.blocked(g["origin"], g["dir"], g["limit"], traversal=mode)
        assert np.array_equal(np.asarray(blk, dtype=bool), g["blocked"] == 1), (kernel, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("cid", RP.FRAME_IDS)
def test_gpu_frames_are_the_references(pinned_renders, cid, kernel, monkeypatch):
    """Render.run_view: mean_buffer against util.restated_sums of the reference's recorded per-path radiance, RGB against the
    reference's recorded bytes.  A flagged path takes its radiance, a pixel that holds one its bytes, from the unoptimised build's
    record (see the module docstring): every path and every pixel is compared."""
    g, case, m = gold("frame_" + cid), case_of(cid), META["frames"][cid]
    L, rgb_ref = g["L"].copy(), g["rgb"].copy()
    if not m["emitter_probe_paths_agree"]:
        L[g["flags"] == 1] = g["flagged_L_unopt"]
        rgb_ref.reshape(-1, 3)[g["flagged_pixels"]] = g["flagged_rgb_unopt"]
    want, _ = util.restated_sums(L.reshape(case["h"], case["w"], case["spp"], 3), case["spp"], case["spp"])
    _set_kernel(monkeypatch, kernel)
    r = pinned_renders[case["scene"]]
    r.set_spp(case["spp"]); r.set_P_RR(case["p_rr"]); r.set_light_sample_n(case["lsn"])
    r.seed = case["seed"]
    if case["scene"] == "room":
        eye, iv, fov = np.array([5.0, 5.0, 0.5], dtype=np.float32), crt.get_inverse_view_matrix([5.0, 5.0, 0.5], [5.0, 4.0, 9.0], [0.0, 1.0, 0.0]), crt.fov_to_radians(70.0)
    else:
        eye, iv, fov = util.camera(case["scene"])
    for mode in MODES:
        r.traversal = mode
        rgb = r.run_view(eye, iv, fov, width=case["w"], height=case["h"])
        util.assert_bits(r.mean_buffer, want, "%s %s mode %d" % (cid, kernel, mode))
        assert np.array_equal(rgb, rgb_ref), (cid, kernel, mode)
