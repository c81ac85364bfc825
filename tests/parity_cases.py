"""Case bodies that more than one test module runs: the room, soup and grazing-ray comparisons with the oracle of test_gpu_parity.py
and test_adversarial_traversal.py, and the commit-ring comparisons of test_commit_ring.py.  test_decoupled_leaves.py runs them again in
both forms of k_mega3's pool, test_first_frame.py as other work between first frames.  Each function is a whole case with its
assertions; the tests pass tmp_path and their parameters through."""
import os

import numpy as np

import cudaraytracing_amd as crt
import oracle_lib as O
import util
from blocked_restated import _oracle_blocked
from scene_files import _write_box_scene, _write_scaled_soup_scene, _write_soup_scene


def _compare_room(tmp_path, thresh, lsn, p_rr, spp, specular=False, w=48, h=36, seed=3, n_side=6, extra_flags=0, light=True):
    obj, mtl = _write_box_scene(str(tmp_path), n_side=n_side, specular=specular, light=light)
    scene = crt.Scene(w, h)
    scene.add_obj(obj, mtl)
    scene.set_BVH(thresh)
    osc = O.OracleScene([(obj, mtl)], thresh)
    assert scene.nodes().tobytes() == osc.nodes().tobytes()
    eye = np.array([5.0, 5.0, 0.5], dtype=np.float32)
    iv = crt.get_inverse_view_matrix(eye, [5.0, 4.0, 9.0], [0.0, 1.0, 0.0])
    fov = crt.fov_to_radians(70.0)
    r = crt.Render(scene, spp, p_rr, lsn)
    r.seed = seed
    r.extra_flags = extra_flags
    orgb, omean, _, st = osc.render(eye, iv, fov, w, h, spp, p_rr, lsn, seed=seed)
    try:
        for mode in (crt.TRAVERSAL_REFERENCE, crt.TRAVERSAL_FAST, crt.TRAVERSAL_EXACT):
            r.traversal = mode
            rgb = r.run_view(eye, iv, fov)
            assert np.array_equal(util.bits(r.mean_buffer), util.bits(omean)), (thresh, lsn, p_rr, mode)
            assert np.array_equal(rgb, orgb)
            assert r.stats["rays"] == st["rays"] and r.stats["probe_rays"] == st["probe_rays"]
    finally:
        r.free()
    return st


def room_matches_oracle_at_leaf_size(tmp_path, thresh):
    """bvh_thresh_n other than 2: leaves with 1, 3..5, more than 15 triangles, and a tree that is one leaf."""
    st = _compare_room(tmp_path, thresh, lsn=1, p_rr=0.6, spp=3)
    assert st["rays"] > 5000


def room_that_is_one_leaf_of_300_triangles_matches_oracle(tmp_path):
    """The whole 300-triangle room as ONE leaf (150 triangle-pair records, best-triangle offsets beyond 8 bits)."""
    st = _compare_room(tmp_path, 400, lsn=1, p_rr=0.6, spp=2, n_side=12)
    assert st["rays"] > 5000


def room_of_180000_triangles_matches_oracle(tmp_path):
    """A floor tessellated into 180 000 triangles (node / triangle indices beyond 16 bits, an 18-level reference tree,
    traversal stacks far beyond the three LDS levels)."""
    st = _compare_room(tmp_path, 2, lsn=1, p_rr=0.6, spp=1, n_side=300, w=40, h=30)
    assert st["rays"] > 3000


def soup_with_ties_and_degenerate_triangles_matches_oracle(tmp_path, thresh):
    obj, mtl = _write_soup_scene(str(tmp_path))
    w, h, spp = 64, 48, 2
    scene = crt.Scene(w, h)
    scene.add_obj(obj, mtl)
    scene.set_BVH(thresh)
    osc = O.OracleScene([(obj, mtl)], thresh)
    assert scene.nodes().tobytes() == osc.nodes().tobytes()
    eye = np.array([5.0, 5.0, 0.5], dtype=np.float32)
    iv = crt.get_inverse_view_matrix(eye, [5.0, 4.5, 9.0], [0.0, 1.0, 0.0])
    fov = crt.fov_to_radians(75.0)
    r = crt.Render(scene, spp, 0.6, 2)
    r.seed = 5
    orgb, omean, _, st = osc.render(eye, iv, fov, w, h, spp, 0.6, 2, seed=5)
    try:
        for mode in (crt.TRAVERSAL_REFERENCE, crt.TRAVERSAL_FAST, crt.TRAVERSAL_EXACT):
            r.traversal = mode
            rgb = r.run_view(eye, iv, fov)
            assert np.array_equal(util.bits(r.mean_buffer), util.bits(omean)), mode
            assert np.array_equal(rgb, orgb)
            assert r.stats["rays"] == st["rays"]
        # closest-hit queries straight at the duplicated / coplanar triangles: triangle ids must agree, not only distances
        n = 4096
        rng = np.random.RandomState(1)
        o = np.tile(eye, (n, 1)).astype(np.float32)
        dd = (rng.uniform([1.5, 1.5, 9.0], [8.5, 8.5, 9.0], (n, 3)) - eye).astype(np.float32)
        for mode in (crt.TRAVERSAL_REFERENCE, crt.TRAVERSAL_FAST, crt.TRAVERSAL_EXACT):
            tri, t = r.intersect(o, dd, traversal=mode)
            otri, ot, _ = osc.intersect(o, dd)
            assert np.array_equal(tri, otri) and np.array_equal(util.bits(t), util.bits(ot)), mode
    finally:
        r.free()


def scaled_soup_matches_oracle(tmp_path, scale):
    """The soup scene with every coordinate scaled: products underflow to denormals / overflow to inf, NaNs appear in the
    radiance (1e12) -- kernel and oracle must still agree bit for bit (the NaNs included), in both traversal modes."""
    obj, mtl = _write_scaled_soup_scene(str(tmp_path), scale)
    w, h, spp = 48, 36, 2
    scene = crt.Scene(w, h)
    scene.add_obj(obj, mtl)
    scene.set_BVH(2)
    osc = O.OracleScene([(obj, mtl)], 2)
    assert scene.nodes().tobytes() == osc.nodes().tobytes()
    eye = (np.array([5.0, 5.0, 0.5]) * scale).astype(np.float32)
    iv = crt.get_inverse_view_matrix(eye, (np.array([5.0, 4.5, 9.0]) * scale).astype(np.float32), [0.0, 1.0, 0.0])
    fov = crt.fov_to_radians(75.0)
    r = crt.Render(scene, spp, 0.6, 2)
    r.seed = 5
    orgb, omean, _, st = osc.render(eye, iv, fov, w, h, spp, 0.6, 2, seed=5)
    try:
        for mode in (crt.TRAVERSAL_REFERENCE, crt.TRAVERSAL_FAST, crt.TRAVERSAL_EXACT):
            r.traversal = mode
            rgb = r.run_view(eye, iv, fov)
            assert np.array_equal(util.bits(r.mean_buffer), util.bits(omean)), (scale, mode)
            assert np.array_equal(rgb, orgb)
            assert r.stats["rays"] == st["rays"]
    finally:
        r.free()


def room_with_every_ray_on_the_reference_arithmetic_matches_oracle(tmp_path, specular):
    """CRT_FLAG_FORCE_EXACT sends every ray of the FAST traversal down the path that rays with a zero / denormal direction
    component take: reference box arithmetic (sign-selected planes, NaN-aware comparisons) on the reference topology, still
    pruned and any-hit.  Nothing changes."""
    st = _compare_room(tmp_path, 2, lsn=2, p_rr=0.7, spp=3, specular=specular, extra_flags=crt.FLAG_FORCE_EXACT)
    assert st["rays"] > 5000


def _load(obj, mtl, thresh, w=48, h=36):
    scene = crt.Scene(w, h)
    scene.add_obj(obj, mtl)
    scene.set_BVH(thresh)
    osc = O.OracleScene([(obj, mtl)], thresh)
    assert scene.nodes().tobytes() == osc.nodes().tobytes()
    return scene, osc


def _check_rays(r, osc, o, d):
    otri, ot, _ = osc.intersect(o, d)
    out = {}
    for mode in (crt.TRAVERSAL_REFERENCE, crt.TRAVERSAL_FAST, crt.TRAVERSAL_EXACT):
        tri, t = r.intersect(o, d, traversal=mode)
        out[mode] = (tri, t)
        bad = np.nonzero((tri != otri) | (util.bits(t) != util.bits(ot)))[0]
        assert bad.size == 0, (mode, bad[:8], tri[bad[:8]], otri[bad[:8]], t[bad[:8]], ot[bad[:8]])
    return otri, ot


def _grazing_rays(tris, rng, n_per, angles):
    """Rays that cross triangle planes at the given (tiny) angles, aimed at a point inside the triangle, from both sides,
    from near and far; plus rays lying exactly in the plane (determinant exactly or nearly zero)."""
    o_list, d_list = [], []
    for v in tris:
        e1, e2 = v[1] - v[0], v[2] - v[0]
        n = np.cross(e1, e2)
        ln = np.linalg.norm(n)
        if ln == 0:
            continue
        n /= ln
        for _ in range(n_per):
            a, b = rng.uniform(0.05, 0.9), rng.uniform(0.05, 0.9)
            if a + b > 0.95:
                a, b = 0.3, 0.3
            p = v[0] + a * e1 + b * e2
            tdir = np.cos(rng.uniform(0, 2 * np.pi)) * e1 / np.linalg.norm(e1) + np.sin(rng.uniform(0, 2 * np.pi)) * np.cross(n, e1) / np.linalg.norm(e1)
            tdir /= np.linalg.norm(tdir)
            for th in angles:
                for sgn in (1.0, -1.0):
                    d = np.cos(th) * tdir + sgn * np.sin(th) * n
                    s = rng.choice([0.01, 0.5, 3.0, 40.0])
                    o_list.append(p - s * d)
                    d_list.append(d)
    return np.asarray(o_list, dtype=np.float32), np.asarray(d_list, dtype=np.float32)


def _soup_triangles(obj):
    vs, fs = [], []
    for line in open(obj):
        t = line.split()
        if not t:
            continue
        if t[0] == "v":
            vs.append([float(x) for x in t[1:4]])
        elif t[0] == "f":
            fs.append([int(x.split("/")[0]) - 1 for x in t[1:4]])
    vs = np.asarray(vs, dtype=np.float64)
    return [vs[f] for f in fs]


def rays_grazing_triangle_planes_match_oracle(tmp_path, thresh):
    obj, mtl = _write_soup_scene(str(tmp_path), n=300, dup=30, degenerate=10)
    scene, osc = _load(obj, mtl, thresh)
    r = crt.Render(scene, 1, 0.6, 1)
    try:
        rng = np.random.RandomState(7)
        tris = _soup_triangles(obj)
        pick = [tris[i] for i in rng.choice(len(tris), 160, replace=False)]
        o, d = _grazing_rays(pick, rng, 3, [0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2])
        otri, ot = _check_rays(r, osc, o, d)
        assert (otri >= 0).sum() > o.shape[0] // 4  # the probes do hit things
    finally:
        r.free()


def visibility_queries_match_blocked(name):
    """crt_intersect with CRT_INTERSECT_VISIBILITY is blocked() of the reference (Render.cuh:19-27, :272) in every traversal mode:
    rays from surface points towards points on other surfaces, limits around the true distance, and the limits the reference's
    t_to_light = dist.x / dir.x can produce (0, negative, infinite, NaN)."""
    t = util.task(name)
    osc = util.oracle_scene(name)
    r = crt.Render(util.host_scene(name), 1, t.P_RR, t.light_sample_n)
    try:
        rng = np.random.RandomState(11)
        tr = osc.tris()
        n = 20000
        def surface_points(k):
            i = rng.randint(0, tr["v1"].shape[0], k)
            a, b = rng.rand(k, 1).astype(np.float32), rng.rand(k, 1).astype(np.float32)
            flip = (a + b) > 1
            a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
            return (tr["v1"][i] + a * (tr["v2"][i] - tr["v1"][i]) + b * (tr["v3"][i] - tr["v1"][i])).astype(np.float32)
        o, p = surface_points(n), surface_points(n)
        d = p - o
        dist = np.linalg.norm(d, axis=1).astype(np.float32)
        lim = dist * rng.choice(np.array([1.0, 1.0, 0.5, 0.999999, 1.000001, 1.00001, 2.0, 1e-3], dtype=np.float32), n)
        lim[:64] = np.tile(np.array([0.0, -1.0, np.inf, -np.inf, np.nan, 3.0e38, 1.0e-5, 2.0e-5], dtype=np.float32), 8)
        ob = _oracle_blocked(osc, o, d, lim)
        assert 0.2 < ob.mean() < 0.95  # both answers are well represented
        for mode in (crt.TRAVERSAL_REFERENCE, crt.TRAVERSAL_FAST, crt.TRAVERSAL_FAST | crt.INTERSECT_FORCE_EXACT, crt.TRAVERSAL_EXACT,
                     crt.TRAVERSAL_EXACT | crt.INTERSECT_FORCE_EXACT):
            blk, tri = r.blocked(o, d, lim, traversal=mode)
            bad = np.nonzero(blk != ob)[0]
            assert bad.size == 0, (mode, bad[:8], lim[bad[:8]])
            assert np.all(tri[~blk] == -1)
            assert np.all(tri[blk & np.isfinite(lim)] >= 0)
    finally:
        r.free()


def _render(name, w, h, spp, ring_log2=None, flags=0, traversal=None, ranges=None):
    """(rgb, f32 sums, launches, (storage bytes, ring samples))"""
    old = os.environ.pop("CRT_COMMIT_RING_LOG2", None)
    if ring_log2 is not None:
        os.environ["CRT_COMMIT_RING_LOG2"] = str(ring_log2)   # (test hook: a ring of 2^n samples, far smaller than a render would choose)
    try:
        t = util.task(name)
        eye, iv, fov = util.camera(name)
        r = crt.Render(util.host_scene(name), spp, t.P_RR, t.light_sample_n, device=0)
        try:
            r.extra_flags = flags
            if traversal is not None:
                r.traversal = traversal
            launches = 0
            if ranges is None:
                rgb = r.run_view(eye, iv, fov, width=w, height=h).copy()
                launches = r.stats["kernel_launches"]
            else:
                rgb = None
                for (b, n) in ranges:
                    rgb = r.run_view_range(eye, iv, fov, b, n, width=w, height=h)
                rgb = rgb.copy()
            return rgb, r.mean_buffer.copy(), launches, r.radiance_storage()
        finally:
            r.free()
    finally:
        os.environ.pop("CRT_COMMIT_RING_LOG2", None)
        if old is not None:
            os.environ["CRT_COMMIT_RING_LOG2"] = old


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(util.bits(a[1]), util.bits(b[1]))


def tiny_ring_reproduces_the_frame(name, w, h, spp, ring_log2):
    """Rings of 2 - 16 samples under a pool that could hold every path of the frame at once: nearly every ray slot is handed a work
    item it may not start yet (ST_WAIT), every sample is committed by whichever wave completes it, ragged tiles (203 x 149, 37 x 21)
    leave cursor shards with fewer pixels than slots."""
    ref = _render(name, w, h, spp)
    got = _render(name, w, h, spp, ring_log2=ring_log2)
    assert ref[3][1] == 0 and got[3][1] == 1 << ring_log2 and got[2] == 1
    assert got[3][0] < ref[3][0]
    assert _same(ref, got)


def flag_picks_a_ring_and_one_launch():
    """CRT_FLAG_BOUNDED_RADIANCE at 256 x 192 spp 160: the ring the render chooses for itself (64 samples here), less storage, same bits;
    with every sample traced (CRT_FLAG_TRACE_ALL) and in the two other traversal modes too."""
    name, w, h, spp = "cornell-box", 256, 192, 160
    ref = _render(name, w, h, spp)
    got = _render(name, w, h, spp, flags=crt.FLAG_BOUNDED_RADIANCE)
    assert got[3][1] in (32, 64, 128) and got[3][0] * 2 <= ref[3][0] and got[2] == 1
    assert _same(ref, got)
    assert _same(ref, _render(name, w, h, spp, flags=crt.FLAG_BOUNDED_RADIANCE | crt.FLAG_TRACE_ALL))
    for mode in (crt.TRAVERSAL_FAST, crt.TRAVERSAL_REFERENCE):
        assert _same(_render(name, w, h, 48, traversal=mode), _render(name, w, h, 48, ring_log2=3, traversal=mode)), mode


def shard_through_the_ring_is_the_shard_without_it():
    """Rank 1 of 3 (interleaved tiles, compact output): the ring's cursor shards are ranges of THIS rank's pixel slots."""
    import ctypes as C
    from cudaraytracing_amd import _capi as capi
    name, w, h, spp = "cornell-box", 200, 120, 64
    t = util.task(name)
    eye, iv, fov = util.camera(name)
    r = crt.Render(util.host_scene(name), spp, t.P_RR, t.light_sample_n, device=0)
    old = os.environ.pop("CRT_COMMIT_RING_LOG2", None)
    try:
        out = []
        for ring in (None, "2"):
            if ring:
                os.environ["CRT_COMMIT_RING_LOG2"] = ring
            slots = crt.shard_slots(w, h, 1, 3)
            buf = np.zeros((slots, 3), dtype=np.uint8)
            mean = np.zeros((slots, 3), dtype=np.float32)
            prm = r._params(rank=1, world=3, flags=capi.FLAG_TILED_OUTPUT, width=w, height=h)
            cam = r._cam(eye, iv, fov)
            st = capi.Stats()
            capi.check(capi.lib().crt_render(r._h, C.byref(cam), C.byref(prm), capi.ptr(buf), capi.ptr(mean), C.byref(st)), "crt_render")
            out.append((buf.copy(), mean.copy(), r.radiance_storage()))
        assert out[0][2][1] == 0 and out[1][2][1] == 4
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(util.bits(out[0][1]), util.bits(out[1][1]))
    finally:
        os.environ.pop("CRT_COMMIT_RING_LOG2", None)
        if old is not None:
            os.environ["CRT_COMMIT_RING_LOG2"] = old
        r.free()
