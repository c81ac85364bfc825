"""The facts the exactness proof of EXACT / FAST assumes (csrc/crt_accel.h), checked on the arrays the kernel walks: every
reference leaf reached exactly once, leaf boxes the reference's bit for bit, inner boxes supersets, no NaN, the exact subtree the reference
BVH, the nodes4i decode, the leaf records, and the sizes taken from the tree (depths / stack_cap, layout_caps, coord_max).  The trees come
from device memory (Render.export_trees); tests/tree_check.py restates every layout in numpy.  Frames cannot show a structural fault that
only changes rays grazing a box edge; these checks do, on every scene below -- and the mutation test shows that they can fail."""
import copy
import os
import struct
import sys

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
import oracle_lib as O
import tree_check as TC
import util
from scene_files import _scene, _write_box_scene, _write_scaled_soup_scene, _write_soup_scene, write_signed_zero_scene

sys.path.insert(0, os.path.join(util.ROOT, "scenes"))
import gen_cornell_box  # noqa: E402

FLT_MAX = float(np.finfo(np.float32).max)


def _check(scene, render, stats=None):
    ex = render.export_trees()
    info = render.accel_info()
    v = TC.check_trees(ex, info, scene.nodes(), scene.root, scene.triangles(), stats)
    return ex, info, v


def _leaf_sizes(scene):
    n = scene.nodes()
    return n["n"][(n["lc"] < 0) & (n["rc"] < 0)]


def _tags(v):
    return {x.split(":")[0] for x in v}


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the checker on a hand-built tree (five one-triangle leaves; a four-wide root with one inner child)
# ---------------------------------------------------------------------------------------------------------------------------------
def _py_with_bits(f, chunk, up):
    m = struct.unpack("<I", struct.pack("<f", f))[0]
    neg, m = m >> 31, m & 0x7fffffff
    grow = (not up) if neg else up
    c = (m & ~0xfff) | chunk
    if grow and c < m:
        c += 0x1000
    elif not grow and c > m:
        if c < 0x1000:
            return struct.unpack("<f", struct.pack("<I", chunk | (0 if neg else 0x80000000)))[0]
        c -= 0x1000
    return struct.unpack("<f", struct.pack("<I", c | (0x80000000 if neg else 0)))[0]


def _toy():
    f32 = np.float32
    tris = np.zeros(5, capi.TRI_DTYPE)
    for k in range(5):
        tris[k]["v1"] = [k, -0.0 if k == 0 else 0.0, 0.0]
        tris[k]["v2"] = [k + 0.5, 1.0, 0.25]
        tris[k]["v3"] = [k + 0.25, 0.5, 1.0 + k / 3.0]
        tris[k]["normal"] = [0.0, 0.0, 1.0]
        tris[k]["material"] = k % 2
    lo = np.minimum(np.minimum(tris["v1"], tris["v2"]), tris["v3"]).astype(f32)
    hi = np.maximum(np.maximum(tris["v1"], tris["v2"]), tris["v3"]).astype(f32)
    # reference (post-order): n0 L0, n1 L1, n2 (n0, n1), n3 L2, n4 L3, n5 (n3, n4), n6 (n2, n5), n7 L4, n8 (n6, n7) = root
    nodes = np.zeros(9, capi.NODE_DTYPE)
    kids = {2: (0, 1), 5: (3, 4), 6: (2, 5), 8: (6, 7)}
    leaf_of = {0: 0, 1: 1, 3: 2, 4: 3, 7: 4}
    for i in range(9):
        if i in kids:
            a, b = kids[i]
            nodes[i]["lc"], nodes[i]["rc"] = a, b
            nodes[i]["aa"] = np.minimum(nodes[a]["aa"], nodes[b]["aa"])
            nodes[i]["bb"] = np.maximum(nodes[a]["bb"], nodes[b]["bb"])
        else:
            k = leaf_of[i]
            nodes[i]["lc"] = nodes[i]["rc"] = -1
            nodes[i]["it"], nodes[i]["n"], nodes[i]["aa"], nodes[i]["bb"] = k, 1, lo[k], hi[k]
    bfs = [8, 6, 2, 5]                                  # both binary trees: the reference topology, breadth first

    def bin_rows(base, leaf_ref, packed3):
        rows = np.zeros((16, 4), f32)
        for q, i in enumerate(bfs):
            refs, boxes = [], []
            for c in kids[i]:
                refs.append(base + bfs.index(c) if c in kids else leaf_ref(leaf_of[c]))
                boxes.append((nodes[c]["aa"], nodes[c]["bb"]))
            (la, lb), (ra, rb) = boxes
            r = rows[4 * q:4 * q + 4]
            if packed3:
                r[0] = [la[0], ra[0], la[1], ra[1]]; r[1] = [la[2], ra[2], lb[0], rb[0]]; r[2] = [lb[1], rb[1], lb[2], rb[2]]
                r[3, :2] = np.array(refs, np.int32).view(f32)
            else:
                r[0, :3], r[1, :3], r[2, :3], r[3, :3] = la, lb, ra, rb
                r[0, 3], r[1, 3] = np.array(refs, np.int32).view(f32)
        return rows

    nodes2 = np.concatenate([bin_rows(0, lambda k: ~((k << 4) | 1), False), bin_rows(4, lambda k: ~((k << 4) | 1), False)])
    nodes3 = np.concatenate([bin_rows(0, lambda k: ~k, True), bin_rows(4, lambda k: ~k, True)])
    # nodes4: node 0 = (inner node 1 = leaves 0, 1; leaf 2; leaf 3; leaf 4), node 1 = (leaf 0, leaf 1, empty, empty), node 2 = empty
    inf = np.inf
    box1 = (np.minimum(lo[0], lo[1]), np.maximum(hi[0], hi[1]))
    slots4 = [[(box1, 1), ((lo[2], hi[2]), ~2), ((lo[3], hi[3]), ~3), ((lo[4], hi[4]), ~4)],
              [((lo[0], hi[0]), ~0), ((lo[1], hi[1]), ~1), None, None], [None] * 4]
    n4 = np.zeros((24, 4), f32)
    for q, sl in enumerate(slots4):
        for s, e in enumerate(sl):
            (l, h), r = e if e else ((np.full(3, inf, f32), np.full(3, -inf, f32)), ~0x7ffffff0)
            for a in range(3):
                n4[8 * q + 2 * a, s], n4[8 * q + 2 * a + 1, s] = l[a], h[a]
            n4[8 * q + 6, s] = np.array([r], np.int32).view(f32)[0]
            r7 = r if r >= 0 or q == 2 else (0x80000000 | ((~r & 0x7fffff) << 8))   # (the empty node keeps the raw ref in row 7)
            n4[8 * q + 7, s] = np.array([r7 & 0xffffffff], np.uint32).view(f32)[0]
    # nodes4i: node 0 mixed (its fringe child node 1 first: ff = 1, n_m = 0, n_f = 1), node 1 fringe, node 2 empty
    chunk = [0, 1 << 3, 1 << 9]
    n4i = np.zeros((18, 4), f32)
    for q in range(3):
        for s in range(4):
            src = 8 * q
            for a in range(3):
                n4i[6 * q + 2 * a, s], n4i[6 * q + 2 * a + 1, s] = n4[src + 2 * a, s], n4[src + 2 * a + 1, s]
    for a in range(3):
        n4i[2 * a, 0] = _py_with_bits(float(n4i[2 * a, 0]), chunk[a], False)
        n4i[2 * a + 1, 0] = _py_with_bits(float(n4i[2 * a + 1, 0]), chunk[a], True)
    tri_geo = np.zeros((15, 4), f32)
    leaf_geo = np.zeros((25, 4), f32)
    v1, e1, e2 = tris["v1"].astype(f32), (tris["v2"] - tris["v1"]).astype(f32), (tris["v3"] - tris["v1"]).astype(f32)
    for k in range(5):
        tri_geo[3 * k:3 * k + 3] = [[*v1[k], e1[k, 0]], [e1[k, 1], e1[k, 2], e2[k, 0], e2[k, 1]], [e2[k, 2], 0.0, 0.0, 1.0]]
        g = leaf_geo[5 * k:5 * k + 5]
        g[0] = [v1[k, 0], v1[k, 0], v1[k, 1], v1[k, 1]]; g[1] = [v1[k, 2], v1[k, 2], e1[k, 0], e1[k, 0]]
        g[2] = [e1[k, 1], e1[k, 1], e1[k, 2], e1[k, 2]]; g[3] = [e2[k, 0], e2[k, 0], e2[k, 1], e2[k, 1]]
        g[4, :2] = e2[k, 2]
        g[4, 2:] = np.array([k, 1], np.int32).view(f32)
    rec_map = np.array([4, 5, 1, 2, 3], np.int32)
    lgi = np.zeros((60, 4), f32)
    for d, sp in enumerate(rec_map):
        lgi[5 * sp:5 * sp + 5] = leaf_geo[5 * d:5 * d + 5]
    tri_nm = np.zeros((5, 4), f32)
    tri_nm[:, 2] = 1.0
    tri_nm[:, 3] = tris["material"].astype(np.int32).view(f32)
    planes = np.concatenate([n4[:6].reshape(-1), n4[8:14, :2].reshape(-1), n4i[:6].reshape(-1)])
    ex = {"nodes": nodes2, "nodes3": nodes3, "nodes4": n4, "nodes4i": n4i, "leaf_geo": leaf_geo, "leaf_geo_i": lgi, "rec_map": rec_map,
          "tri_geo": tri_geo, "leaf_count": np.zeros(5, np.int32), "tri_nm": tri_nm, "root_fast": 0, "root_exact": 4, "root3_fast": 0,
          "root3_exact": 4, "root4": 0, "root4i": 0, "n_mixed4i": 1, "empty4_off": 2 * 128, "empty4i_off": 2 * 96,
          "coord_max": float(np.abs(planes).max()), "stack_cap": 11, "node4i_f4": 6}
    info = {"n_nodes4": 2, "depth2": 4, "depth4": 3, "layout_caps": 15}
    return ex, info, nodes, 8, tris


def test_checker_on_a_hand_built_tree():
    ex, info, nodes, root, tris = _toy()
    stats = {}
    assert TC.check_trees(ex, info, nodes, root, tris, stats) == []
    assert stats["nudged_planes"] > 0

    def broken(change):
        e, i = copy.deepcopy(ex), dict(info)
        change(e, i)
        return _tags(TC.check_trees(e, i, nodes, root, tris))

    def inner_inwards(e, i):        # node 0 slot 0 (inner) lo.x one ulp up
        e["nodes4"][0, 0] = np.nextafter(e["nodes4"][0, 0], np.float32(np.inf))

    def leaf_bit_exact(e, i):
        b = e["nodes4"][3:4, 1:2].view(np.uint32)
        b ^= np.uint32(1)

    def swap_records(e, i):
        g = e["leaf_geo"]
        g[0:5], g[5:10] = g[5:10].copy(), g[0:5].copy()

    def hi_chunk(e, i):
        e["nodes4i"][1:2, 0:1].view(np.uint32)[...] ^= np.uint32(2)

    def cmax(e, i):
        e["coord_max"] = float(np.nextafter(np.float32(e["coord_max"]), np.float32(0)))

    def dup_leaf(e, i):             # node 0's leaf 3 slot points at leaf 2 as well (rows 6 and 7)
        e["nodes4"][6:8, 2] = e["nodes4"][6:8, 1]

    def depth(e, i):
        i["depth4"] = 2

    def caps(e, i):
        i["layout_caps"] = 7

    def exact_order(e, i):          # the exact tree's root children swapped (boxes and refs): still a valid tree, not the reference's
        r = e["nodes"][16:20].copy()
        e["nodes"][16, :3], e["nodes"][18, :3] = r[2, :3], r[0, :3]
        e["nodes"][17, :3], e["nodes"][19, :3] = r[3, :3], r[1, :3]
        e["nodes"][16, 3], e["nodes"][17, 3] = r[1, 3], r[0, 3]

    assert "I3" in broken(inner_inwards)
    assert "I2" in broken(leaf_bit_exact)
    assert "I6" in broken(swap_records)
    assert "I5" in broken(hi_chunk)
    assert broken(cmax) == {"I9"}
    assert "I1" in broken(dup_leaf)
    assert broken(depth) == {"I7"}
    assert broken(caps) == {"I8"}
    assert broken(exact_order) == {"I4"}


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU: every tree of every scene below gives no violation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_trees_of_the_benchmark_scenes(name):
    t = util.task(name)
    scene = util.host_scene(name)
    r = crt.Render(scene, 2, t.P_RR, t.light_sample_n)
    try:
        ex, info, v = _check(scene, r)
        assert v == [], v
        assert info["layout_caps"] & 8 and len(ex["nodes4i"]) > 0
        if name == "veach-mis":
            assert info["index_splits"] > 0  # coincident leaves
    finally:
        r.free()


def _mutations(ex):
    """One real export broken in six ways; each must be reported (invariant expected, mutated export)."""
    f32 = np.float32
    n4 = ex["nodes4"].reshape(-1, 8, 4)
    refs = n4[:, 6].view(np.int32)
    out = []
    q, s = [int(x) for x in np.argwhere(refs[:-1] >= 0)[0]]
    e = copy.deepcopy(ex)
    e["nodes4"].reshape(-1, 8, 4)[q, 0, s] = np.nextafter(n4[q, 0, s], f32(np.inf))      # inner lo.x one ulp inwards
    out.append(("I3", "inner plane one ulp inwards", e))
    lq, ls = [int(x) for x in np.argwhere((refs[:-1] < 0) & (refs[:-1] != TC.EMPTY_REF))[0]]
    e = copy.deepcopy(ex)
    e["nodes4"].reshape(-1, 8, 4)[lq, 1:2, ls:ls + 1].view(np.uint32)[...] ^= np.uint32(1)  # leaf hi.x low bit
    out.append(("I2", "low bit of a leaf plane", e))
    e = copy.deepcopy(ex)
    g = e["leaf_geo"]
    g[0:5], g[5:10] = g[5:10].copy(), g[0:5].copy()
    out.append(("I6", "two leaf records swapped", e))
    e = copy.deepcopy(ex)
    e["nodes4i"][1:2, 0:1].view(np.uint32)[...] ^= np.uint32(1 << 5)                      # node 0 (mixed): one chunk bit of hi.x only
    out.append(("I5", "one chunk bit in a hi plane", e))
    e = copy.deepcopy(ex)
    e["coord_max"] = float(np.nextafter(f32(ex["coord_max"]), f32(0)))
    out.append(("I9", "coord_max one ulp down", e))
    e = copy.deepcopy(ex)
    m4 = e["nodes4"].reshape(-1, 8, 4)
    leaf_slots = np.argwhere((refs[:-1] < 0) & (refs[:-1] != TC.EMPTY_REF))
    (q1, s1), (q2, s2) = leaf_slots[0], leaf_slots[-1]
    m4[q2, 6:8, s2] = m4[q1, 6:8, s1]                                                      # one leaf ref twice
    out.append(("I1", "a leaf ref duplicated", e))
    return out


@pytest.mark.gpu
def test_trees_of_the_102412_triangle_mesh_and_every_mutation_is_reported(tmp_path):
    obj, mtl, n = gen_cornell_box.write_variant(str(tmp_path), (6, 5))
    assert n == 102412
    scene = _scene(obj, mtl, util.task("cornell-box").bvh_thresh_n)
    r = crt.Render(scene, 1, 0.6, 1)
    try:
        ex, info, v = _check(scene, r)
        assert v == [], v
        assert 16384 < info["n_nodes4"] <= 32768 and info["layout_caps"] & 8   # nodes4i ids use bit 14
        args = (info, scene.nodes(), scene.root, scene.triangles())
        for tag, what, e in _mutations(ex):
            got = TC.check_trees(e, *args)
            assert tag in _tags(got), (what, got)
    finally:
        r.free()


def _room_frame_stack(r, scene):
    eye = np.array([5.0, 5.0, 0.5], dtype=np.float32)
    iv = crt.get_inverse_view_matrix(eye, [5.0, 4.0, 9.0], [0.0, 1.0, 0.0])
    r.run_view(eye, iv, crt.fov_to_radians(70.0), stats=True)
    return r.stats["stack_max"]


@pytest.mark.gpu
def test_trees_of_the_room_of_180000_triangles(tmp_path):
    obj, mtl = _write_box_scene(str(tmp_path), n_side=300)
    scene = _scene(obj, mtl, 2, 40, 30)
    r = crt.Render(scene, 1, 0.6, 1)
    try:
        ex, info, v = _check(scene, r)
        assert v == [], v
        assert info["n_nodes4"] > 32768 and not info["layout_caps"] & 8 and len(ex["nodes4i"]) == 0
        assert _room_frame_stack(r, scene) <= ex["stack_cap"]
    finally:
        r.free()


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", [1, 2, 4, 20, 200])
def test_trees_of_the_soup_with_duplicates_and_degenerate_triangles(tmp_path, thresh):
    obj, mtl = _write_soup_scene(str(tmp_path))
    scene = _scene(obj, mtl, thresh)
    r = crt.Render(scene, 1, 0.6, 1)
    try:
        ex, info, v = _check(scene, r)
        assert v == [], v
        if thresh >= 4:
            assert _leaf_sizes(scene).max() > 2 and not info["layout_caps"] & 8   # multi-record leaves: no nodes4i
        if thresh == 1:
            assert _room_frame_stack(r, scene) <= ex["stack_cap"]
    finally:
        r.free()


@pytest.mark.gpu
def test_trees_of_a_room_that_is_one_leaf(tmp_path):
    obj, mtl = _write_box_scene(str(tmp_path), n_side=12)
    scene = _scene(obj, mtl, 400)
    assert len(scene.nodes()) == 1 and len(scene.triangles()) == 300
    r = crt.Render(scene, 1, 0.6, 1)
    try:
        ex, info, v = _check(scene, r)
        assert v == [], v
        assert ex["root_fast"] < 0 and ex["root4"] < 0 and len(ex["nodes"]) == 0
    finally:
        r.free()


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1e-12, 1e12, 1e17])
def test_trees_at_extreme_coordinate_scales(tmp_path, scale):
    obj, mtl = _write_scaled_soup_scene(str(tmp_path), scale)
    scene = _scene(obj, mtl, 2)
    r = crt.Render(scene, 1, 0.6, 1)
    try:
        ex, info, v = _check(scene, r)
        assert v == [], v
    finally:
        r.free()


@pytest.mark.gpu
def test_trees_with_planes_at_signed_zeros_and_denormals(tmp_path):
    obj, mtl = write_signed_zero_scene(str(tmp_path))
    scene = _scene(obj, mtl, 2)
    aa = scene.nodes()["aa"]
    assert (np.signbit(aa) & (aa == 0)).any() and (~np.signbit(aa) & (aa == 0)).any()
    assert ((np.abs(aa) > 0) & (np.abs(aa) < np.finfo(np.float32).tiny)).any()
    r = crt.Render(scene, 1, 0.6, 1)
    try:
        st = {}
        ex, info, v = _check(scene, r, st)
        assert v == [], v
        assert info["layout_caps"] & 8
        assert st["crossed_zero"] > 0, st   # a with_bits nudge crossed zero: the nodes4i plane's sign differs from the nodes4 plane's
    finally:
        r.free()


@pytest.mark.gpu
def test_with_bits_gives_up_next_to_flt_max(tmp_path):
    """Triangles with a vertex at x = FLT_MAX: every box that holds them has hi.x = FLT_MAX (low bits 0xfff), where no larger finite
    value with other low bits exists -- the nodes4i copy is not made, the frame still equals the oracle's."""
    obj, mtl = _write_box_scene(str(tmp_path), n_side=4)
    with open(obj) as f:
        nv = sum(1 for line in f if line.startswith("v "))
    rng = np.random.RandomState(2)
    with open(obj, "a") as o:
        o.write("usemtl floor\n")
        for _ in range(64):
            y, z = rng.uniform(0, 10, 2)
            for p in ((FLT_MAX, y, z), (FLT_MAX, y + 0.5, z), (1e38 * rng.uniform(1.0, 3.0), y, z + 0.5)):
                o.write("v %.9g %.9g %.9g\nvn 0 1 0\nvt 0 0\n" % p)
            o.write("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % (nv + 1, nv + 1, nv + 1, nv + 2, nv + 2, nv + 2, nv + 3, nv + 3, nv + 3))
            nv += 3
    w, h = 32, 24
    scene = _scene(obj, mtl, 2, w, h)
    r = crt.Render(scene, 1, 0.6, 1)
    try:
        ex, info, v = _check(scene, r)
        assert v == [], v
        # every other condition of the nodes4i copy holds (crt_scene_layout.h: one-record leaves, <= 32 768 nodes, finite planes) ...
        n4c = info["n_nodes4"]
        assert n4c < 4095 and _leaf_sizes(scene).max() <= 2 and ex["root4"] >= 0 and np.isfinite(ex["coord_max"])
        # ... and some node with an inner child has hi.x = FLT_MAX (low bits 0xfff) on EVERY inner child: whichever of them nodes4i puts in
        # slot 0, its hi.x must move up to carry fm & 0xfff (fm < 4095: not 0xfff), and no finite value above FLT_MAX exists
        n4 = ex["nodes4"].reshape(-1, 8, 4)[:n4c]
        inner = n4[:, 6].view(np.int32) >= 0
        at_max = n4[:, 1].view(np.uint32) == 0x7f7fffff
        assert (inner.any(1) & (at_max | ~inner).all(1)).any()
        assert not info["layout_caps"] & 8 and len(ex["nodes4i"]) == 0
        eye = np.array([5.0, 5.0, 0.5], dtype=np.float32)
        iv = crt.get_inverse_view_matrix(eye, [5.0, 4.0, 9.0], [0.0, 1.0, 0.0])
        fov = crt.fov_to_radians(70.0)
        rgb = r.run_view(eye, iv, fov)
        orgb, omean, _, st = O.OracleScene([(obj, mtl)], 2).render(eye, iv, fov, w, h, 1, 0.6, 1, seed=0)
        assert np.array_equal(util.bits(r.mean_buffer), util.bits(omean)) and np.array_equal(rgb, orgb)
    finally:
        r.free()
