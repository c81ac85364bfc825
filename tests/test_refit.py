"""crt_scene_refit: a scene handle's triangles move, every topology it holds stays (include/crt.h, "Refit").

The contract is exact: after the refit to B the handle is, byte for byte, what a fresh handle holds that was created from B' -- A's nodes
with the boxes of the numpy rule (tests/refit_restated.py) and B's triangles -- wherever topology does not enter, and renders what it
renders.  On the CPU tools/refit_host_check.cpp runs the kernel text of both forms (levels, walk) on the layout the library builds, plain
and under AddressSanitizer / UBSan; on the GPU the handle is compared with the fresh handle, with the tool's bytes and with itself after
refusals.

Scene B moves A in three ways at once: the triangles of one material are carried across the plane x = 0 (planes change sign, nudged
planes are rounded in both directions), those of an emitter are scaled by (1.5, 0.75, 1.25) about their centroid (area_of_obj and the
light triangles change), and those of a third material get a per-vertex displacement with the normals recomputed in numpy."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
import host_program as HP
import refit_restated as RR
import tree_check as TC
import util
from scene_files import _scene, _write_box_scene, _write_soup_scene, write_signed_zero_scene
from traversal_trees import _dump, build_dump_tool, set_layout

F = np.float32
FORMS = ("levels", "walk")
ARRAYS = tuple(crt.Render.EXPORT_ARRAYS) + ("ltri",)
SCALARS = [k for k, _ in capi.TreeScalars._fields_]
W, H = 48, 36


class Desc:
    """A scene description held in numpy arrays: what crt.Render needs of a scene (desc(), the arrays, root, width, height)"""

    def __init__(self, nodes, root, tris, ltris, mats, lights, width=W, height=H):
        self.a = [np.ascontiguousarray(x).copy() for x in (nodes, tris, mats, ltris, lights)]
        self.root, self.width, self.height = int(root), width, height

    @classmethod
    def of(cls, scene, **kw):
        return cls(scene.nodes(), scene.root, scene.triangles(), scene.light_triangles(), scene.materials(), scene.lights(), **kw)

    def nodes(self): return self.a[0]
    def triangles(self): return self.a[1]
    def materials(self): return self.a[2]
    def light_triangles(self): return self.a[3]
    def lights(self): return self.a[4]

    def desc(self):
        n, t, m, l, g = self.a
        d = capi.SceneDesc()
        d.nodes, d.n_nodes, d.root = n.ctypes.data_as(C.POINTER(capi.BvhNode)), len(n), self.root
        d.tris, d.n_tris = t.ctypes.data_as(C.POINTER(capi.Triangle)), len(t)
        d.materials, d.n_materials = m.ctypes.data_as(C.POINTER(capi.Material)), len(m)
        d.light_tris, d.n_light_tris = (l.ctypes.data_as(C.POINTER(capi.Triangle)) if len(l) else None), len(l)
        d.lights, d.n_lights = (g.ctypes.data_as(C.POINTER(capi.Light)) if len(g) else None), len(g)
        return d

    def with_triangles(self, tris, ltris):
        """B': the same nodes with the boxes of the rule for `tris`"""
        return Desc(RR.refit_nodes(self.nodes(), tris), self.root, tris, ltris, self.materials(), self.lights(), self.width, self.height)


def _vertex_key(t):
    return np.ascontiguousarray(np.concatenate([t["v1"], t["v2"], t["v3"]], axis=1), dtype=F).view(np.uint32)


def _renormal(t):
    """normal and area of the triangles from their vertices, in numpy (any values do: both sides get the same arrays)"""
    n = np.cross(t["v2"] - t["v1"], t["v3"] - t["v1"]).astype(F)
    ln = np.sqrt((n * n).sum(axis=1)).astype(F)
    t["normal"] = np.where(ln[:, None] > 0, n / np.where(ln > 0, ln, 1)[:, None], n).astype(F)
    t["area"] = (ln * F(0.5)).astype(F)


def moved(A, seed=3):
    """(tris, light_tris) of scene B from description A; light triangles follow the triangles they equal in A, vertex for vertex"""
    tris, ltris, mats = A.triangles().copy(), A.light_triangles().copy(), A.materials()
    rng = np.random.RandomState(seed)
    by_mat = [np.nonzero(tris["material"] == m)[0] for m in range(len(mats))]
    emit = [m for m in range(len(mats)) if mats["has_emit"][m] and len(by_mat[m])]
    plain = sorted((m for m in range(len(mats)) if not mats["has_emit"][m] and len(by_mat[m])), key=lambda m: len(by_mat[m]))
    V = ("v1", "v2", "v3")
    if plain:                                     # across the plane x = 0: the object's mirror position
        s = by_mat[plain[0]]
        xs = np.concatenate([tris[v][s, 0] for v in V])
        dx = F(-(xs.min() + xs.max()))
        for v in V:
            tris[v][s, 0] = tris[v][s, 0] + dx
    if emit:                                      # a non-uniform scale of an emitter about its centroid
        s = by_mat[emit[0]]
        c = np.mean(np.concatenate([tris[v][s] for v in V]), axis=0).astype(F)
        k = np.array([1.5, 0.75, 1.25], dtype=F)
        for v in V:
            tris[v][s] = (tris[v][s] - c) * k + c
    if len(plain) > 1:                            # a displacement per vertex
        s = by_mat[plain[-1]]
        ext = F(np.ptp(np.concatenate([tris[v][s] for v in V]), axis=0).max())
        for v in V:
            tris[v][s] = tris[v][s] + (rng.uniform(-0.01, 0.01, (len(s), 3)) * ext).astype(F)
    _renormal(tris)
    if len(ltris):
        key = {k.tobytes(): i for i, k in enumerate(_vertex_key(A.triangles()))}
        src = np.array([key[k.tobytes()] for k in _vertex_key(ltris)])
        for f in V + ("normal", "area"):
            ltris[f] = tris[f][src]
        for g in A.lights():                      # the light's area, as Object sums it
            r = slice(int(g["first_tri"]), int(g["first_tri"] + g["count"]))
            a = F(0)
            for x in ltris["area"][r]:
                a = F(a + x)
            ltris["area_of_obj"][r] = a
            tris["area_of_obj"][src[r]] = a
    assert tris.tobytes() != A.triangles().tobytes()
    return tris, ltris


# ---------------------------------------------------------------- the host program ----
@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("refit_tools"))
    extra = ["-pthread", "-fno-fast-math"]
    return {"dump": build_dump_tool(d),
            "plain": HP.build("refit_host_check.cpp", os.path.join(d, "refit_plain"), HP.PLAIN, extra),
            "sanitised": HP.build("refit_host_check.cpp", os.path.join(d, "refit_sanitised"), HP.SANITISED, extra)}


def _load(d):
    ex = {}
    for name in ARRAYS:
        dt = crt.Render.EXPORT_ARRAYS.get(name, np.float32)
        a = np.fromfile(os.path.join(d, name + ".bin"), dtype=dt)
        ex[name] = a.reshape(-1, 4) if dt is np.float32 else a
    with open(os.path.join(d, "scalars.bin"), "rb") as f:
        ex.update(capi.TreeScalars.from_buffer_copy(f.read()).as_dict())
    with open(os.path.join(d, "accel.bin"), "rb") as f:
        info = capi.AccelInfo.from_buffer_copy(f.read()).as_dict()
    ex["root_box"] = np.fromfile(os.path.join(d, "root.bin"), dtype=F)
    return ex, info


def run_tool(exe, tmp, A, form, moves, want_status=0):
    """The tool on description A with the refits `moves` [(tris, light_tris), ...] in order: (arrays and scalars, accel info)"""
    src, out = os.path.join(tmp, "src"), os.path.join(tmp, "out_%s_%s" % (os.path.basename(exe), form))
    os.makedirs(src, exist_ok=True)
    os.makedirs(out, exist_ok=True)
    for name, a in (("nodes", A.nodes()), ("tris", A.triangles()), ("light_tris", A.light_triangles()), ("materials", A.materials()), ("lights", A.lights())):
        a.tofile(os.path.join(src, "desc_%s.bin" % name))
    args = [src, str(A.root), form, out]
    for k, (t, l) in enumerate(moves):
        pt, pl = os.path.join(src, "move%d_tris.bin" % k), os.path.join(src, "move%d_ltris.bin" % k)
        t.tofile(pt)
        l.tofile(pl)
        args += [pt, pl]
    rc, so, se = HP.run(exe, args, timeout=300)
    assert rc == want_status, (rc, so, se)
    return _load(out)


def same_export(got, want, where, arrays=ARRAYS, scalars=SCALARS):
    for k in arrays:
        if k not in want:
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (where, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), (where, k, int((got[k].view(np.uint32) != want[k].view(np.uint32)).sum()))
    for k in scalars:
        assert F(got[k]).tobytes() == F(want[k]).tobytes() if k == "coord_max" else got[k] == want[k], (where, k, got[k], want[k])


def all_runs(tools, tmp, A, moves, want_status=0):
    """Both forms, plain and sanitised: one result, after all four gave the same bytes"""
    first = None
    for form in FORMS:
        for build in ("plain", "sanitised"):
            ex, info = run_tool(tools[build], tmp, A, form, moves, want_status)
            if first is None:
                first = (ex, info)
            else:
                same_export(ex, first[0], (form, build))
                assert ex["root_box"].tobytes() == first[0]["root_box"].tobytes(), (form, build)
    return first


def leaf_planes(ex, A):
    """{tree: (leaf node of the description, lo, hi)} for every leaf slot of nodes (both ranges), nodes4 and nodes4i"""
    nodes = A.nodes()
    leaf_of_it = {int(nodes["it"][i]): i for i in np.nonzero(RR.is_leaf(nodes))[0]}
    out = {}
    if len(ex["nodes"]):
        r = ex["nodes"].reshape(-1, 4, 4)
        refs = np.ascontiguousarray(r[:, :2, 3]).view(np.int32)                  # (n, 2)
        lo, hi = np.stack([r[:, 0, :3], r[:, 2, :3]], 1), np.stack([r[:, 1, :3], r[:, 3, :3]], 1)
        m = refs < 0
        out["nodes"] = ([leaf_of_it[(~int(x) & 0xffffffff) >> 4] for x in refs[m]], lo[m], hi[m])
    rec_it = np.ascontiguousarray(ex["leaf_geo"].reshape(-1, 5, 4)[:, 4, 2]).view(np.int32)
    if ex["root4"] >= 0:
        r = ex["nodes4"].reshape(-1, 8, 4)[:-1]
        refs = np.ascontiguousarray(r[:, 6, :]).view(np.int32)
        lo, hi = r[:, 0:6:2, :].transpose(0, 2, 1), r[:, 1:6:2, :].transpose(0, 2, 1)   # (n, slot, axis)
        m = (refs < 0) & (refs != TC.EMPTY_REF)
        out["nodes4"] = ([leaf_of_it[int(rec_it[~int(x)])] for x in refs[m]], lo[m], hi[m])
        if len(ex["nodes4i"]):
            r = ex["nodes4i"].reshape(-1, 6, 4)[:-1]
            lo, hi = r[:, 0:6:2, :].transpose(0, 2, 1), r[:, 1:6:2, :].transpose(0, 2, 1)
            sparse = ex["rec_map"]
            out["nodes4i"] = ([leaf_of_it[int(rec_it[d])] for d in range(len(sparse))], lo.reshape(-1, 3)[sparse], hi.reshape(-1, 3)[sparse])
    return out


def check_against(ex, info, Bp, where, stats=None):
    """The four checks of a refit to B on an export: every tree invariant against B', the rows, ltri, the leaf planes"""
    v = TC.check_trees(ex, info, Bp.nodes(), Bp.root, Bp.triangles(), stats)
    assert v == [], (where, v)
    util.assert_bits(ex["tri_geo"], RR.tri_geo_rows(Bp.triangles()), "%s tri_geo" % (where,))
    util.assert_bits(ex["tri_nm"], RR.tri_nm_rows(Bp.triangles(), Bp.materials()), "%s tri_nm" % (where,))
    util.assert_bits(ex["leaf_geo"], RR.leaf_geo_rows(Bp.nodes(), Bp.triangles()), "%s leaf_geo" % (where,))
    if "ltri" in ex:
        util.assert_bits(ex["ltri"], RR.ltri_rows(Bp.light_triangles(), Bp.materials()), "%s ltri" % (where,))
    for tree, (leaves, lo, hi) in leaf_planes(ex, Bp).items():
        util.assert_bits(lo, Bp.nodes()["aa"][leaves], "%s %s leaf lo" % (where, tree))
        util.assert_bits(hi, Bp.nodes()["bb"][leaves], "%s %s leaf hi" % (where, tree))
    if "root_box" in ex:
        util.assert_bits(ex["root_box"], np.concatenate([Bp.nodes()["aa"][Bp.root], Bp.nodes()["bb"][Bp.root]]), "%s root box" % (where,))


# ---------------------------------------------------------------- CPU: the kernel text on the host ----
@pytest.mark.parametrize("name", ["veach-mis", "cornell-box"])
def test_refitting_a_scene_with_its_own_triangles_reproduces_the_layout(tools, tmp_path, name):
    """Identity: every array and scalar of the layout tool's dump of A, byte for byte, from both forms, plain and sanitised -- the
    unions, the nudges, the record lanes and coord_max against the code that builds them at crt_scene_create."""
    scene = util.host_scene(name)
    A = Desc.of(scene)
    want, want_info = _dump(tools["dump"], scene, str(tmp_path))
    got, info = all_runs(tools, str(tmp_path), A, [(A.triangles(), A.light_triangles())])
    same_export(got, want, name)
    assert info == want_info or {k: info[k] for k in info if not k.endswith("_ms")} == {k: want_info[k] for k in want_info if not k.endswith("_ms")}
    util.assert_bits(got["root_box"], np.concatenate([A.nodes()["aa"][A.root], A.nodes()["bb"][A.root]]), "root box")
    util.assert_bits(got["ltri"], RR.ltri_rows(A.light_triangles(), A.materials()), "ltri")


def test_a_moved_scene_and_the_way_back(tools, tmp_path):
    """B: the four checks against B'.  A -> B -> A: the dump of A again, byte for byte."""
    scene = util.host_scene("veach-mis")
    A = Desc.of(scene)
    tb, lb = moved(A)
    Bp = A.with_triangles(tb, lb)
    st = {}
    ex, info = all_runs(tools, str(tmp_path), A, [(tb, lb)])
    check_against(ex, info, Bp, "B", st)
    assert st["nudged_planes"] > 0
    assert (tb["v1"][:, 0] < 0).any() and (tb["v1"][:, 0] > 0).any()
    assert lb.tobytes() != A.light_triangles().tobytes() and not np.array_equal(lb["area_of_obj"], A.light_triangles()["area_of_obj"])
    want, _ = _dump(tools["dump"], scene, str(tmp_path))
    back, _ = all_runs(tools, str(tmp_path), A, [(tb, lb), (A.triangles(), A.light_triangles())])
    same_export(back, want, "A -> B -> A")


def test_the_forms_take_turns_on_one_layout(tools, tmp_path):
    """CRT_REFIT_FORM is read per call: refits of one handle in levels, walk, levels, walk -- and walk, walk, levels, walk -- leave what a
    single form leaves.  (The walk's counters advance in walk calls only; a count of ALL calls would let a walk after a levels call wait
    for arrivals that never come and leave every inner box above the lowest as it was.)"""
    A = Desc.of(util.host_scene("veach-mis"))
    tb, lb = moved(A)
    a, b = (A.triangles(), A.light_triangles()), (tb, lb)
    want_b, _ = run_tool(tools["plain"], str(tmp_path), A, "levels", [b])
    want_a, _ = run_tool(tools["plain"], str(tmp_path), A, "levels", [b, a])
    for forms in ("levels,walk,levels,walk", "walk,walk,levels,walk", "levels,levels,walk"):
        n = len(forms.split(","))
        for build in ("plain", "sanitised") if forms.startswith("levels,walk") else ("plain",):
            for last, want in ((b, want_b), (a, want_a)):
                moves = ([a, b] * n)[:n - 1] + [last]              # the last refit, in the list's last form, decides what is left
                got, _ = run_tool(tools[build], str(tmp_path), A, forms, moves)
                same_export(got, want, (forms, build))
                assert got["root_box"].tobytes() == want["root_box"].tobytes(), (forms, build)


def _two_triangles(d):
    with open(os.path.join(d, "two.mtl"), "w") as m:
        m.write("newmtl grey\nKd 0.6 0.6 0.6\nNs 1\nnewmtl light\nKe 20 20 20\nKd 0 0 0\nNs 1\n")
    with open(os.path.join(d, "two.obj"), "w") as o:
        o.write("mtllib two.mtl\n")
        for p in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 2), (1, 0, 2), (0, 1, 2.5)):
            o.write("v %g %g %g\nvn 0 1 0\nvt 0 0\n" % p)
        o.write("usemtl grey\nf 1/1/1 2/2/2 3/3/3\nusemtl light\nf 4/4/4 5/5/5 6/6/6\n")
    return os.path.join(d, "two.obj"), d


def write_row_scene(d, E, ratio=1.2):
    """A row of triangles in geometric progression along x, from 2^-E up to 2^E (the generator of tests/test_deep_trees.py, restated): at
    position x the triangle (x, 0, 0), (x + s, s, 0), (x, 0, s) with s = x (ratio - 1) / 2, then x *= ratio.  The SAH builder peels such
    a row a few leaves at a time, so the trees are about as deep as the row is long.  All grey but the last, which is the light."""
    tris, x = [], 2.0 ** -E
    while x < 2.0 ** E:
        w = x * (ratio - 1.0) / 2.0
        tris.append(((x, 0.0, 0.0), (x + w, w, 0.0), (x, 0.0, w)))
        x *= ratio
    with open(os.path.join(d, "row.mtl"), "w") as m:
        m.write("newmtl grey\nKd 0.6 0.6 0.6\nNs 1\nnewmtl light\nKe 20 20 20\nKd 0 0 0\nNs 1\n")
    with open(os.path.join(d, "row.obj"), "w") as o:
        o.write("mtllib row.mtl\nusemtl grey\n")
        for i, t in enumerate(tris):
            if i == len(tris) - 1:
                o.write("usemtl light\n")
            for q in t:
                o.write("v %.9g %.9g %.9g\nvn 0 1 0\nvt 0 0\n" % q)
            o.write("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % ((3 * i + 1,) * 3 + (3 * i + 2,) * 3 + (3 * i + 3,) * 3))
    return os.path.join(d, "row.obj"), d


def _small(name, d):
    if name == "one-leaf":
        return _scene(*_write_box_scene(d, n_side=12), 400)
    if name == "two-leaves":
        return _scene(*_two_triangles(d), 1)
    if name.startswith("soup"):
        return _scene(*_write_soup_scene(d), int(name[4:]))
    if name == "chain":
        return _scene(*write_row_scene(d, 30), 1)
    return _scene(*write_signed_zero_scene(d), 2)


def _jitter(A, seed):
    """every vertex displaced a little, normals recomputed; light triangles follow"""
    t, l = A.triangles().copy(), A.light_triangles().copy()
    rng = np.random.RandomState(seed)
    for v in ("v1", "v2", "v3"):
        t[v] = (t[v] * (1 + rng.uniform(-0.02, 0.02, t[v].shape))).astype(F)
    _renormal(t)
    if len(l):
        key = {k.tobytes(): i for i, k in enumerate(_vertex_key(A.triangles()))}
        src = np.array([key[k.tobytes()] for k in _vertex_key(l)])
        for f in ("v1", "v2", "v3", "normal", "area"):
            l[f] = t[f][src]
    return t, l


@pytest.mark.parametrize("name", ["one-leaf", "two-leaves", "soup1", "soup2", "soup8", "chain"])
def test_the_smallest_shapes(tools, tmp_path, name):
    """One leaf (no nodes, no nodes4), two leaves, bvh_thresh_n 1, 2 and 8 (at 8: leaves of more than two triangles, odd tails, no nodes4i
    set), and a row in geometric progression whose four-wide tree is at least 40 levels deep: the four checks, and the way back."""
    scene = _small(name, str(tmp_path))
    A = Desc.of(scene)
    want, want_info = _dump(tools["dump"], scene, str(tmp_path))
    n = A.nodes()
    leaves = n["n"][RR.is_leaf(n)]
    if name == "one-leaf":
        assert len(leaves) == 1 and want["root4"] < 0 and len(want["nodes"]) == 0
    if name == "two-leaves":
        assert len(leaves) == 2
    if name == "soup8":
        assert leaves.max() > 2 and (leaves % 2 == 1).any() and len(want["nodes4i"]) == 0
    if name == "chain":
        assert want_info["depth4"] >= 40
    tb, lb = _jitter(A, 5)
    Bp = A.with_triangles(tb, lb)
    ex, info = all_runs(tools, str(tmp_path), A, [(tb, lb)])
    check_against(ex, info, Bp, name)
    # the way back: A by the rule (the builder's own boxes may differ from the rule's in the sign of a zero plane only)
    back, binfo = all_runs(tools, str(tmp_path), A, [(tb, lb), (A.triangles(), A.light_triangles())])
    check_against(back, binfo, A.with_triangles(A.triangles(), A.light_triangles()), name + " back")
    once, _ = run_tool(tools["plain"], str(tmp_path), A, "levels", [(A.triangles(), A.light_triangles())])
    same_export(back, once, name + " A -> B -> A against A -> A")


def test_planes_at_zero_minus_zero_and_denormals(tools, tmp_path):
    """Mixed nodes whose child-0 planes are +0, -0 and denormals: the coordinates of the signed-zero scene with the sign of every x
    flipped (+0 <-> -0, denormals change side), and back."""
    scene = _small("zeros", str(tmp_path))
    A = Desc.of(scene)
    t, l = A.triangles().copy(), A.light_triangles().copy()
    for v in ("v1", "v2", "v3"):
        t[v][:, 0] = -t[v][:, 0]
    _renormal(t)
    zeros = np.concatenate([t[v].ravel() for v in ("v1", "v2", "v3")])
    assert (zeros.view(np.uint32) == 0x80000000).any() and (zeros.view(np.uint32) == 0).any() and ((zeros != 0) & (np.abs(zeros) < TC.FLT_MIN)).any()
    for moves, B, where in (([(t, l)], (t, l), "flipped"), ([(t, l), (A.triangles(), A.light_triangles())], (A.triangles(), A.light_triangles()), "back")):
        st = {}
        ex, info = all_runs(tools, str(tmp_path), A, moves)
        check_against(ex, info, A.with_triangles(*B), where, st)
        assert st["crossed_zero"] > 0, st


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 2.0 ** 127])
def test_a_refused_coordinate_leaves_every_array(tools, tmp_path, bad):
    scene = util.host_scene("veach-mis")
    A = Desc.of(scene)
    want, _ = _dump(tools["dump"], scene, str(tmp_path))
    t = A.triangles().copy()
    t["v3"][len(t) // 2, 1] = bad
    for form in FORMS:
        got, _ = run_tool(tools["plain"], str(tmp_path), A, form, [(t, A.light_triangles())], want_status=3)
        same_export(got, want, (form, bad))
    ok = A.triangles().copy()
    ok["v3"][len(t) // 2, 1] = 2.0 ** 126          # the largest magnitude a refit takes
    run_tool(tools["plain"], str(tmp_path), A, "walk", [(ok, A.light_triangles())])


# ---------------------------------------------------------------- CPU: the host layer ----
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]


def _fresh_host_scene(name="veach-mis"):
    return crt.Scene.from_task(util.task(name))


def test_transform_object_identity_keeps_the_description():
    s = _fresh_host_scene()
    before = Desc.of(s)
    for i in range(len(s.objects())):
        s.transform_object(i, IDENTITY)
    after = Desc.of(s)
    for a, b in zip(before.a, after.a):
        assert a.tobytes() == b.tobytes()
    with pytest.raises(capi.CrtError):
        s.transform_object(len(s.objects()), IDENTITY)
    s.free()


def test_transform_object_moves_one_object_and_refits_the_boxes():
    s = _fresh_host_scene()
    before = Desc.of(s)
    objs = s.objects()
    idx = next(i for i, o in enumerate(objs) if o[0])            # a light: its light triangles move with it
    s.transform_object(idx, [1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 2.0])
    after = Desc.of(s)
    assert after.nodes().tobytes() == RR.refit_nodes(before.nodes(), after.triangles()).tobytes()
    for f in ("lc", "rc", "n", "it"):
        assert np.array_equal(before.nodes()[f], after.nodes()[f])
    t0, t1 = before.triangles(), after.triangles()
    changed = np.array([t0[i].tobytes() != t1[i].tobytes() for i in range(len(t0))])
    assert changed.sum() == objs[idx][2]
    d = np.array([0.5, -0.25, 2.0], dtype=F)
    for v in ("v1", "v2", "v3"):
        util.assert_bits(t1[v][changed], t0[v][changed] + d, v)
    l0, l1 = before.light_triangles(), after.light_triangles()
    lchanged = np.array([l0[i].tobytes() != l1[i].tobytes() for i in range(len(l0))])
    assert lchanged.sum() == objs[idx][2]
    assert np.array_equal(t0["material"], t1["material"]) and before.materials().tobytes() == after.materials().tobytes()
    s.set_BVH(util.task("veach-mis").bvh_thresh_n)              # a rebuild afterwards works as before
    assert len(s.nodes()) > 0
    s.free()


def test_entry_points_are_exported_and_the_abi_version_stays():
    lib = capi.lib()
    for name in ("crt_scene_refit", "crt_scene_refit_device", "crt_host_scene_transform_object"):
        assert name in capi.EXPORTS
        getattr(lib, name)
    assert lib.crt_abi_version() == 5 == capi.ABI_VERSION          # only entry points were added
    assert "ltri" not in crt.Render.EXPORT_ARRAYS
    assert lib.crt_scene_refit(None, None, 0, None, 0, None) == capi.ERR_INVALID_ARG
    assert lib.crt_scene_refit_device(None, None, 0, None, 0, None, None) == capi.ERR_INVALID_ARG


# ---------------------------------------------------------------- GPU ----
def _export(r):
    ex = r.export_trees()
    ex["ltri"] = r.export_array("ltri")
    return ex


def _frame(r, cam, **kw):
    rgb = r.run_view(*cam, **kw).copy()
    return rgb, r.mean_buffer.copy(), (r.stats["rays"], r.stats["shadow_rays"])


def _same_frame(a, b, where):
    assert np.array_equal(a[0], b[0]), where
    util.assert_bits(a[1], b[1], str(where))
    assert a[2] == b[2], (where, a[2], b[2])


@pytest.fixture(scope="module")
def veach():
    scene = util.host_scene("veach-mis")
    A = Desc.of(scene)
    tb, lb = moved(A)
    return A, tb, lb, A.with_triangles(tb, lb), util.camera("veach-mis")


def _clear(monkeypatch):
    for k in ("CRT_REFIT_FORM", "CRT_PIPELINE", "CRT_SAH_HOST", "CRT_DEC", "CRT_REF16", "CRT_REF32", "CRT_IMPL"):
        monkeypatch.delenv(k, raising=False)


FRAME_CASES = [("exact", capi.TRAVERSAL_EXACT, "default", None, 1), ("reference", capi.TRAVERSAL_REFERENCE, "default", None, 1),
               ("fast", capi.TRAVERSAL_FAST, "default", None, 4), ("wavefront", capi.TRAVERSAL_EXACT, "default", "2", 1),
               ("coupled-16", capi.TRAVERSAL_EXACT, "coupled-16", None, 4), ("decoupled-16", capi.TRAVERSAL_EXACT, "decoupled-16", None, 1),
               ("decoupled-16, rows of refs", capi.TRAVERSAL_FAST, "decoupled-16, rows of refs", None, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_the_refitted_handle_renders_the_fresh_handles_frame(veach, monkeypatch, case, form):
    """rgb, mean, rays and shadow rays after the refit to B equal those of a fresh handle created from B'"""
    A, tb, lb, Bp, cam = veach
    _, traversal, layout, pipeline, lsn = case
    _clear(monkeypatch)
    set_layout(monkeypatch, layout)
    if pipeline:
        monkeypatch.setenv("CRT_PIPELINE", pipeline)
    monkeypatch.setenv("CRT_REFIT_FORM", form)
    r, f = crt.Render(A, 4, 0.6, lsn), crt.Render(Bp, 4, 0.6, lsn)
    try:
        r.traversal = f.traversal = traversal
        r.seed = f.seed = 11
        _frame(r, cam, stats=True)                                   # a frame of A first: nothing of it may stay
        info = r.refit(tb, lb)
        assert info["form"] == FORMS.index(form) and info["n_tris"] == len(tb) and info["leaves"] == int(RR.is_leaf(A.nodes()).sum())
        _same_frame(_frame(r, cam, stats=True), _frame(f, cam, stats=True), case[0])
    finally:
        r.free()
        f.free()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_exports_after_a_refit(veach, tools, tmp_path, monkeypatch, form):
    """The exported trees pass every invariant against B'; with the host SAH builder on both sides every exported array, ltri and the
    scalars are the host program's bytes; identity and A -> B -> A are a fresh handle of A; accel_info() does not move."""
    A, tb, lb, Bp, cam = veach
    _clear(monkeypatch)
    monkeypatch.setenv("CRT_SAH_HOST", "1")
    monkeypatch.setenv("CRT_REFIT_FORM", form)
    r, fresh = crt.Render(A, 4, 0.6, 1), crt.Render(A, 4, 0.6, 1)
    try:
        counts = {k: v for k, v in r.accel_info().items() if not k.endswith("_ms")}
        want_a = _export(fresh)
        info = r.refit(A.triangles(), A.light_triangles())
        assert info["prepare_ms"] > 0
        same_export(_export(r), want_a, "identity")
        info = r.refit(tb, lb)
        assert info["prepare_ms"] == 0
        ex = _export(r)
        check_against(ex, r.accel_info(), Bp, "B")
        tool, _ = run_tool(tools["plain"], str(tmp_path), A, form, [(tb, lb)])
        same_export(ex, tool, "against the host program")
        util.assert_bits(np.array(info["root_aa"] + info["root_bb"], dtype=F), tool["root_box"], "root box")
        assert F(info["coord_max"]).tobytes() == F(tool["coord_max"]).tobytes()
        r.refit(A.triangles(), A.light_triangles())
        same_export(_export(r), want_a, "A -> B -> A")
        assert {k: v for k, v in r.accel_info().items() if not k.endswith("_ms")} == counts
    finally:
        r.free()
        fresh.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one-leaf", "soup8", "chain", "zeros"])
def test_small_shapes_on_the_device(tools, tmp_path, monkeypatch, name):
    """The shapes of the CPU tests whose code paths differ -- no tree at all, no nodes4i set and odd tails, a deep tree (one launch per
    height; long walks), nudges across zero -- both forms against the host program's bytes"""
    _clear(monkeypatch)
    monkeypatch.setenv("CRT_SAH_HOST", "1")
    scene = _small(name, str(tmp_path))
    A = Desc.of(scene, width=32, height=24)
    tb, lb = _jitter(A, 5)
    tool, _ = run_tool(tools["plain"], str(tmp_path), A, "levels", [(tb, lb)])
    for form in FORMS:
        monkeypatch.setenv("CRT_REFIT_FORM", form)
        r = crt.Render(A, 1, 0.6, 1)
        try:
            r.refit(tb, lb)
            same_export(_export(r), tool, (name, form))
            r.refit(tb, lb)                                          # the walk's counters carry on from the call before
            same_export(_export(r), tool, (name, form, "again"))
        finally:
            r.free()


@pytest.mark.gpu
def test_the_device_form_on_a_stream(veach, monkeypatch):
    """The triangle arrays in device memory, the work on a stream of its own: the host form's bytes.  (The buffers and the stream are
    made on the HIP runtime the library itself calls, cudaraytracing_amd.hipmem: a torch tensor's pointer or stream belongs to the runtime
    torch bundles and is a foreign handle to the library's.)"""
    from cudaraytracing_amd import hipmem
    A, tb, lb, Bp, cam = veach
    _clear(monkeypatch)
    monkeypatch.setenv("CRT_SAH_HOST", "1")
    r, h = crt.Render(A, 4, 0.6, 1), crt.Render(A, 4, 0.6, 1)
    try:
        h.refit(tb, lb)
        with hipmem.DeviceBuffers({"tris": tb.view(np.uint8).reshape(-1), "ltris": lb.view(np.uint8).reshape(-1)}, stream=True) as d:
            info = r.refit_device(d.ptrs["tris"], d.ptrs["ltris"], stream=d.stream, n_tris=len(tb), n_light_tris=len(lb))
            assert info["device_ms"] > 0
            same_export(_export(r), _export(h), "device form")
            assert r.refit_info["coord_max"] == h.refit_info["coord_max"] and r.refit_info["root_aa"] == h.refit_info["root_aa"]
            _same_frame(_frame(r, cam, stats=True), _frame(h, cam, stats=True), "device form")
    finally:
        r.free()
        h.free()


@pytest.mark.gpu
def test_a_refit_ends_the_frame_in_flight(veach, monkeypatch):
    A, tb, lb, Bp, cam = veach
    _clear(monkeypatch)
    r = crt.Render(A, 4, 0.6, 1)
    try:
        r.run_view_range(*cam, 0, 2, want_variance=True)
        r.variance()
        r.refit(tb, lb)
        with pytest.raises(capi.CrtError) as e:
            r.run_view_range(*cam, 2, 2, want_variance=True)
        assert e.value.status == capi.ERR_INVALID_ARG
        with pytest.raises(capi.CrtError) as e:
            r.variance()
        assert e.value.status == capi.ERR_INVALID_ARG
        r.run_view_range(*cam, 0, 2, want_variance=True)
        assert r.run_view_range(*cam, 2, 2, want_variance=True) is not None
    finally:
        r.free()


@pytest.mark.gpu
def test_side_passes_after_a_refit(veach, monkeypatch):
    A, tb, lb, Bp, cam = veach
    _clear(monkeypatch)
    r, f = crt.Render(A, 4, 0.6, 1), crt.Render(Bp, 4, 0.6, 1)
    try:
        r.refit(tb, lb)
        assert r.aov_ao_defaults() == f.aov_ao_defaults()
        a, b = r.run_view_aov(*cam), f.run_view_aov(*cam)
        util.assert_same(a, b, list(b), "aov")
        a, b = r.run_view_aov_ao(*cam, ao_samples=4), f.run_view_aov_ao(*cam, ao_samples=4)
        util.assert_same(a, b, list(b), "aov_ao")
    finally:
        r.free()
        f.free()


@pytest.mark.gpu
def test_refusals_leave_the_handle_as_it_was(veach, monkeypatch):
    A, tb, lb, Bp, cam = veach
    _clear(monkeypatch)
    r = crt.Render(A, 4, 0.6, 1)
    try:
        r.refit(tb, lb)                                              # (tables made: a refusal after the first refit, and the state it left)
        before = _export(r)
        t, l = tb.copy(), lb.copy()

        def refused(tris, ltris, where):
            with pytest.raises(capi.CrtError) as e:
                r.refit(tris, ltris)
            assert e.value.status == capi.ERR_INVALID_ARG, where
            same_export(_export(r), before, where)

        refused(t[:-1], l, "one triangle short")
        refused(t, l[:-1], "one light triangle short")
        for bad in (np.nan, np.inf, 2.0 ** 127):
            x = t.copy()
            x["v2"][7, 2] = bad
            refused(x, l, bad)
            y = l.copy()
            y["v1"][0, 0] = bad
            refused(t, y, ("light", bad))
        x = t.copy()
        x["material"][3] = (x["material"][3] + 1) % len(A.materials())
        refused(x, l, "material")
        monkeypatch.setenv("CRT_REFIT_FORM", "neither")
        refused(t, l, "form")
        monkeypatch.delenv("CRT_REFIT_FORM")
        r.refit(t, l)
        same_export(_export(r), before, "and the same refit again")
    finally:
        r.free()


@pytest.mark.gpu
def test_the_cli_moves_an_object_as_the_library_does(tmp_path, monkeypatch):
    """crt_cli --move-object (crt::Scene::transform_object, crt::Render::refit) against Scene.transform_object and Render.refit: the
    same PNG."""
    from PIL import Image
    _clear(monkeypatch)
    t = util.task("veach-mis")
    s = _fresh_host_scene()
    idx = next(i for i, o in enumerate(s.objects()) if o[0])
    png = str(tmp_path / "moved.png")
    cli = os.path.join(os.path.dirname(capi.lib_path()), "crt_cli")
    subprocess.run([cli, util.SCENES["veach-mis"], "--base-dir", util.ROOT, "-o", png, "--spp", "4", "--seed", "5", "--width", str(W), "--height", str(H),
                    "--move-object", "%d,0.5,-0.25,0.125" % idx, "--move-object", "0,0.25,0,0"], check=True, timeout=120)
    s.width, s.height = W, H
    r = crt.Render(s, 4, t.P_RR, t.light_sample_n)  # (the task's own settings, as the CLI takes them)
    try:
        r.seed = 5
        s.transform_object(idx, [1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 0.125])
        r.refit()
        s.transform_object(0, [1, 0, 0, 0.25, 0, 1, 0, 0, 0, 0, 1, 0])
        r.refit()
        rgb = r.run_view(*util.camera("veach-mis"), width=W, height=H)
        assert np.array_equal(np.asarray(Image.open(png)), rgb)
    finally:
        r.free()
        s.free()


@pytest.mark.gpu
def test_the_forms_take_turns_on_one_handle(veach, monkeypatch):
    """One handle, the form changing from call to call: after every refit the arrays are those a handle holds that was refitted once"""
    A, tb, lb, Bp, cam = veach
    _clear(monkeypatch)
    monkeypatch.setenv("CRT_SAH_HOST", "1")
    a, b = (A.triangles(), A.light_triangles()), (tb, lb)
    r, ha, hb = crt.Render(A, 4, 0.6, 1), crt.Render(A, 4, 0.6, 1), crt.Render(A, 4, 0.6, 1)
    try:
        monkeypatch.setenv("CRT_REFIT_FORM", "levels")
        ha.refit(*a)
        hb.refit(*b)
        want = {"a": _export(ha), "b": _export(hb)}
        frame_b = _frame(hb, cam, stats=True)
        for k, (form, to) in enumerate([("levels", "b"), ("walk", "a"), ("levels", "b"), ("walk", "b"), ("walk", "a"), ("levels", "a"), ("walk", "b")]):
            monkeypatch.setenv("CRT_REFIT_FORM", form)
            info = r.refit(*(a if to == "a" else b))
            assert info["form"] == FORMS.index(form)
            same_export(_export(r), want[to], (k, form, to))
        _same_frame(_frame(r, cam, stats=True), frame_b, "after the last walk")
    finally:
        for h in (r, ha, hb):
            h.free()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_the_cornell_box_renders_the_fresh_handles_frame(monkeypatch, form):
    """The second scene A of the suite, 40 972 triangles: more mixed nodes, other depths, thousands of tasks per height"""
    _clear(monkeypatch)
    monkeypatch.setenv("CRT_REFIT_FORM", form)
    A = Desc.of(util.host_scene("cornell-box"))
    tb, lb = moved(A)
    Bp, cam = A.with_triangles(tb, lb), util.camera("cornell-box")
    r, f = crt.Render(A, 4, 0.6, 1), crt.Render(Bp, 4, 0.6, 1)
    try:
        r.seed = f.seed = 7
        r.refit(tb, lb)
        for traversal in (capi.TRAVERSAL_EXACT, capi.TRAVERSAL_REFERENCE):
            r.traversal = f.traversal = traversal
            _same_frame(_frame(r, cam, stats=True), _frame(f, cam, stats=True), ("cornell-box", form, traversal))
        ex = _export(r)
        for tree, (leaves, lo, hi) in leaf_planes(ex, Bp).items():
            util.assert_bits(lo, Bp.nodes()["aa"][leaves], "%s leaf lo" % tree)
            util.assert_bits(hi, Bp.nodes()["bb"][leaves], "%s leaf hi" % tree)
    finally:
        r.free()
        f.free()


TORCH_CHILD = """
import sys
import torch                                     # first: the library then shares torch's HIP runtime
sys.path[:0] = [%(root)r, %(tests)r]
import numpy as np
import cudaraytracing_amd as crt
from cudaraytracing_amd import distributed
import util
tb, lb = np.load(%(tris)r), np.load(%(ltris)r)
scene, cam = util.host_scene("veach-mis"), util.camera("veach-mis")
r, h = crt.Render(scene, 4, 0.6, 1), crt.Render(scene, 4, 0.6, 1)
distributed._check_single_hip_runtime()          # raises if two runtimes are mapped: nothing of torch's is handed over then
h.refit(tb, lb)
dt = torch.from_numpy(tb.view(np.uint8).reshape(-1).copy()).cuda()
dl = torch.from_numpy(lb.view(np.uint8).reshape(-1).copy()).cuda()
st = torch.cuda.Stream()
st.wait_stream(torch.cuda.current_stream())
info = r.refit_device(dt.data_ptr(), dl.data_ptr(), stream=st.cuda_stream, n_tris=len(tb), n_light_tris=len(lb))
assert info["device_ms"] > 0 and info["n_tris"] == len(tb)
ea, eb = r.export_trees(), h.export_trees()
for k in list(crt.Render.EXPORT_ARRAYS) + ["coord_max"]:
    assert np.asarray(ea[k]).tobytes() == np.asarray(eb[k]).tobytes(), k
assert r.export_array("ltri").tobytes() == h.export_array("ltri").tobytes()
fa, fb = r.run_view(*cam, width=48, height=36).copy(), h.run_view(*cam, width=48, height=36).copy()
assert np.array_equal(fa, fb) and np.array_equal(r.mean_buffer.view(np.uint32), h.mean_buffer.view(np.uint32))
r.free(); h.free()
print("refit-from-torch-tensors-ok")
"""


@pytest.mark.gpu
def test_the_device_form_takes_torch_tensors(veach, tmp_path):
    """The triangle arrays in torch tensors, the work on a torch stream: the host form's bytes and frame.  In a process of its own that
    imports torch first, so that the library and torch share one HIP runtime."""
    A, tb, lb, Bp, cam = veach
    np.save(str(tmp_path / "tris.npy"), tb)
    np.save(str(tmp_path / "ltris.npy"), lb)
    code = TORCH_CHILD % {"root": util.ROOT, "tests": os.path.join(util.ROOT, "tests"), "tris": str(tmp_path / "tris.npy"), "ltris": str(tmp_path / "ltris.npy")}
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180, cwd=util.ROOT)
    assert p.returncode == 0 and "refit-from-torch-tensors-ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
