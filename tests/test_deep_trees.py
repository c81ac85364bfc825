"""Traversal on deep trees: stacks that spill far beyond their LDS levels, and k_mega3's 8-bit stack depth without a test hook.

Every traversal form keeps the first levels of a ray's stack in LDS (eight 16-bit or four 32-bit levels in the coupled pool, six or three
in the decoupled one, CRT_STACK_LDS = 8 in k_trace) and spills deeper levels to a global area of (stack_cap - LDS levels) x lanes entries
(csrc/crt_render.hip: plan_mega3, make_trace_setup); in the 16-bit layouts a ray on the reference-arithmetic path keeps its whole stack
there.  The other scenes of the suite have a stack_cap of about 40 and reach a few spilled levels at most.  The scenes here are rows of
triangles in geometric progression (scene_files.write_geometric_chain_scene), which the SAH builder peels a few leaves at a time:

    scene                    triangles  depth2  depth4  stack_cap  coord_max     (tools/scene_layout_dump.cpp, host builder, default
    geo(20, 1.2)                   153      42      33        101    1.1e6        environment, bvh_thresh_n 1; index_splits 0 and
    geo(20, 1.2), row = 4          612      44      32         98    1.1e6        layout_caps 15 everywhere, tree_check: no violation)
    geo(48, 1.2)                   365      95      82        248    2.6e14
    geo(50, 1.2)                   381      99      85        257    1.2e15

geo(48) and geo(50) lie on either side of CRT_MEGA3_MAX_STACK = 255: the first renders with k_mega3, the second with the wavefront pipeline.

The frames' camera stands at the small end, (0, h, h) with h = 4 x 2^-E, and looks along (1, 0.04, 0.04) through 6 degrees: its rays run
from the small end towards the large one inside nearly every leaf box, so the nearest child of a chain node is its inner child and the
leaves beside it stay pending.  The numpy walk of the exported nodes4 (traversal_trees.pending_entries) predicts 80 pending entries with
leaves on the stack and 28 with inner nodes only on geo(20), 75 / 74 on its row = 4 variant, 227 / 68 on geo(48) and 236 / 71 on geo(50);
stats["stack_max"] of the frames on an MI355X is exactly that: 80 / 28, 75 / 74 and 227 / 68 in k_mega3's coupled / decoupled pool, and
89 and 93 in k_trace, which walks the two-wide tree, on geo(48) and geo(50) (docs/experiments.md has the table).
The light of these scenes is their last and largest triangle and faces away from the row, so the frames are black: what the frame
comparison pins is the ray count (every bounce and every next-event sample depends on a closest hit); the hits themselves are compared
value by value through crt_intersect, in front of and behind the closest hit through the visibility form."""
import numpy as np
import pytest

import cudaraytracing_amd as crt
import oracle_lib as O
import tree_check as TC
import util
from aov_expected import NAMES, expected_aov_of
from blocked_restated import _oracle_blocked
from scene_files import _scene, geometric_chain_rays, write_geometric_chain_scene
from traversal_trees import LAYOUTS, LDS_LEVELS, _checked_export, _dump, _same_trees, build_dump_tool, pending_entries, set_layout

SCENES = {"geo20": (20, 1), "geo20-row4": (20, 4), "geo48": (48, 1), "geo50": (50, 1)}   # (E, row) at ratio 1.2
W, H, SPP, P_RR, LSN, SEED = 48, 36, 3, 0.6, 1, 3
MEGA3_MAX_STACK = 255          # CRT_MEGA3_MAX_STACK (csrc/crt_mega3.h): the stack depth has 8 bits of word D
TRACE_LDS_LEVELS = 8           # CRT_STACK_LDS (csrc/crt_render.hip: make_trace_setup)
PIPELINE_HOOKS = ("CRT_TEST_MAX_STACK", "CRT_PIPELINE", "CRT_DEC", "CRT_REF16", "CRT_REF32", "CRT_IMPL", "CRT_SAH_HOST", "CRT_STACK_LDS")
FRAME_MODES = ((crt.TRAVERSAL_FAST, 0), (crt.TRAVERSAL_EXACT, 0), (crt.TRAVERSAL_REFERENCE, 0), (crt.TRAVERSAL_FAST, crt.FLAG_FORCE_EXACT),
               (crt.TRAVERSAL_EXACT, crt.FLAG_FORCE_EXACT))
QUERY_MODES = (crt.TRAVERSAL_FAST, crt.TRAVERSAL_EXACT, crt.TRAVERSAL_REFERENCE, crt.TRAVERSAL_FAST | crt.INTERSECT_FORCE_EXACT,
               crt.TRAVERSAL_EXACT | crt.INTERSECT_FORCE_EXACT)


class Chain:
    """One scene of the family with everything the tests compare against, each computed once: the files, the host and oracle scenes,
    the camera, the layout tool's dump, the oracle's frame, and the ray set with the oracle's answers."""

    def __init__(self, name, d, tool):
        self.name, self.dir, self.tool = name, str(d), tool
        self.E, self.row = SCENES[name]
        self.obj, self.mtl = write_geometric_chain_scene(self.dir, self.E, 1.2, self.row)
        self.scene = _scene(self.obj, self.mtl, 1, W, H)
        eye = np.array([0.0, 4.0 * 2.0 ** -self.E, 4.0 * 2.0 ** -self.E], dtype=np.float32)
        look = (eye.astype(np.float64) + np.array([1.0, 0.04, 0.04])).astype(np.float32)
        self.view = (eye, crt.get_inverse_view_matrix(eye, look, [0.0, 1.0, 0.0]), crt.fov_to_radians(6.0))
        self._memo = {}

    def _once(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    @property
    def osc(self):
        def make():
            osc = O.OracleScene([(self.obj, self.mtl)], 1)
            assert self.scene.nodes().tobytes() == osc.nodes().tobytes()
            return osc
        return self._once("osc", make)

    @property
    def dump(self):
        return self._once("dump", lambda: _dump(self.tool, self.scene, self.dir))

    @property
    def frame(self):
        """(rgb, mean, stats) of the oracle's frame"""
        def make():
            rgb, mean, _, st = self.osc.render(*self.view, W, H, SPP, P_RR, LSN, seed=SEED)
            return rgb, mean, st
        return self._once("frame", make)

    @property
    def rays(self):
        """(origins, directions, the +-x group, the oracle's triangles and distances, visibility limits, the oracle's blocked())"""
        def make():
            o, d, along_x = geometric_chain_rays(self.E, 1.2, self.row)
            otri, ot, _ = self.osc.intersect(o, d)
            rng = np.random.RandomState(4)
            n = len(o)
            # limits on both sides of the closest hit, and the degenerate ones
            lim = np.where(ot < np.float32(3.0e38), ot, np.float32(5.0)) * rng.choice(np.array([0.5, 0.99999, 1.0, 1.00001, 1.5], dtype=np.float32), n)
            lim[:40] = np.tile(np.array([0.0, -1.0, np.inf, -np.inf, np.nan, 3.0e38, 1.0e-5, 2.0e-5], dtype=np.float32), 5)
            return o, d, along_x, otri, ot, lim, _oracle_blocked(self.osc, o, d, lim)
        return self._once("rays", make)


@pytest.fixture(scope="module")
def chains(tmp_path_factory):
    tool = build_dump_tool(tmp_path_factory.mktemp("layout_tool"))
    made = {}

    def get(name):
        if name not in made:
            made[name] = Chain(name, tmp_path_factory.mktemp(name), tool)
        return made[name]
    return get


def _clear(monkeypatch):
    for k in PIPELINE_HOOKS:
        monkeypatch.delenv(k, raising=False)


def _check_frame(r, c, mode, flags, stats, where):
    """One frame in this mode: the oracle's mean bits, RGB and ray count; returns the stats"""
    orgb, omean, ost = c.frame
    r.traversal, r.extra_flags, r.seed = mode, flags, SEED
    rgb = r.run_view(*c.view, stats=stats)
    assert np.array_equal(util.bits(r.mean_buffer), util.bits(omean)), where
    assert np.array_equal(rgb, orgb) and r.stats["rays"] == ost["rays"], (where, r.stats["rays"], ost["rays"])
    return r.stats


def _check_queries(r, c, modes, where):
    """crt_intersect and its visibility form on the scene's ray set in these modes: the oracle's answers bit for bit"""
    o, d, _, otri, ot, lim, ob = c.rays
    for mode in modes:
        tri, t = r.intersect(o, d, traversal=mode)
        bad = np.nonzero((tri != otri) | (util.bits(t) != util.bits(ot)))[0]
        assert bad.size == 0, (where, mode, bad.size, bad[:8], tri[bad[:8]], otri[bad[:8]], t[bad[:8]], ot[bad[:8]])
        blk, _ = r.blocked(o, d, lim, traversal=mode)
        bad = np.nonzero(blk != ob)[0]
        assert bad.size == 0, (where, mode, bad.size, bad[:8], lim[bad[:8]], ot[bad[:8]])


# ------------------------------------------------------------------------------------------------------------------ CPU --

@pytest.mark.parametrize("name", list(SCENES))
def test_the_chain_scenes_are_deep_and_keep_every_tree_invariant(chains, name):
    """The layout built on the CPU: no violation of tests/tree_check.py, no range split by index, depth4 >= 30 on the two E = 20 scenes,
    and geo(48) / geo(50) on either side of the 255 entries that k_mega3's word D can count (figures: the table above)."""
    c = chains(name)
    ex, info = c.dump
    v = TC.check_trees(ex, info, c.scene.nodes(), c.scene.root, c.scene.triangles())
    print(name, len(c.scene.triangles()), {k: info[k] for k in ("depth2", "depth4", "index_splits", "layout_caps")}, ex["stack_cap"], ex["coord_max"])
    assert v == [], v
    assert info["index_splits"] == 0 and info["sah_on_device"] == 0
    assert ex["stack_cap"] >= max(info["depth2"] + 2, 3 * info["depth4"] + 2)
    if c.E == 20:
        assert info["depth4"] >= 30
    elif name == "geo48":
        assert 200 <= ex["stack_cap"] <= MEGA3_MAX_STACK
    else:
        assert ex["stack_cap"] > MEGA3_MAX_STACK
    assert ex["coord_max"] < 1e17   # (the scales the extreme-scale tests cover)


@pytest.mark.parametrize("name", list(SCENES))
def test_the_ray_set_hits_the_chain(chains, name):
    """The condition on the ray set, against the oracle: at least half of the 4096 rays hit a triangle, the +-x group at least 20
    different ones."""
    o, d, along_x, otri, ot, lim, ob = chains(name).rays
    assert len(o) == 4096 and along_x.stop - along_x.start == 4096 // 3
    assert (otri >= 0).sum() * 2 >= len(o), (otri >= 0).mean()
    assert len(np.unique(otri[along_x][otri[along_x] >= 0])) >= 20
    assert 0.1 < ob[40:].mean() < 0.9   # both answers of the visibility form


@pytest.mark.parametrize("name,leaves,inner", [("geo20", 16, 10), ("geo20-row4", 16, 10), ("geo48", 128, 10), ("geo50", 128, 10)])
def test_the_walk_sends_the_frames_rays_deep(chains, name, leaves, inner):
    """How the camera was chosen (nothing here runs the device): on the oracle's camera rays of the frame, an unpruned nearest-first walk
    of the dumped nodes4 leaves at least `leaves` entries pending with leaves on the stack -- 8 LDS levels + 8 on the E = 20 scenes, beyond
    7 bits on the two scenes around the 8-bit limit -- and `inner` with inner nodes only (6 LDS levels + 4), never more than stack_cap."""
    c = chains(name)
    o, d, _, _, _ = util.primary_rays_of(c.osc, *c.view, LSN, W, H, 1)
    p = pending_entries(c.dump[0], o[::7], d[::7]).max(axis=0)
    print(name, "pending entries, with leaves / inner nodes only:", p, "stack_cap", c.dump[0]["stack_cap"])
    assert leaves <= p[0] <= c.dump[0]["stack_cap"] and inner <= p[1] <= c.dump[0]["stack_cap"], p


# ------------------------------------------------------------------------------------------------------------------ GPU --

@pytest.mark.gpu
def test_closest_hits_on_geo20_in_the_default_layout(chains, monkeypatch):
    """The narrowest case, first: crt_intersect on geo(20), default layout, CRT_TRAVERSAL_EXACT."""
    _clear(monkeypatch)
    c = chains("geo20")
    r = crt.Render(c.scene, SPP, P_RR, LSN)
    try:
        o, d, _, otri, ot, _, _ = c.rays
        tri, t = r.intersect(o, d, traversal=crt.TRAVERSAL_EXACT)
        bad = np.nonzero((tri != otri) | (util.bits(t) != util.bits(ot)))[0]
        assert bad.size == 0, (bad.size, bad[:8], tri[bad[:8]], otri[bad[:8]], t[bad[:8]], ot[bad[:8]])
    finally:
        r.free()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", ["geo20", "geo20-row4"])
def test_every_pool_layout_on_a_deep_tree(chains, monkeypatch, name, layout):
    """Each form of k_mega3's pool on a tree of 33 four-wide levels: the oracle's frame and ray count in FAST, EXACT and REFERENCE and
    with every ray on the reference-arithmetic path, without and with the counters; the oracle's closest hits and visibility answers on
    the ray set in the five query modes.  The spilled levels are really used: the deepest stack of the frame is at least the form's LDS
    levels + 8 in the coupled pool (leaves on the stack) and + 4 in the decoupled one (inner nodes only), and never above stack_cap."""
    _clear(monkeypatch)
    c = chains(name)
    set_layout(monkeypatch, layout)
    r = crt.Render(c.scene, SPP, P_RR, LSN)
    try:
        cap = r.export_trees()["stack_cap"]
        assert cap == c.dump[0]["stack_cap"]
        assert r.accel_info()["depth4"] >= 30
        for mode, flags in FRAME_MODES:
            _check_frame(r, c, mode, flags, False, (name, layout, mode, flags))
            st = _check_frame(r, c, mode, flags, True, (name, layout, mode, flags, "stats"))
            assert st["kernel_launches"] == 1   # k_mega3
            print("stack_max", name, "|", layout, "| mode", mode, "flags", flags, ":", st["stack_max"], "of", cap)
            assert 0 < st["stack_max"] <= cap, (name, layout, mode, flags, st["stack_max"], cap)
            if flags == 0 and mode != crt.TRAVERSAL_REFERENCE:
                form, lv = LDS_LEVELS[layout][1 if mode == crt.TRAVERSAL_EXACT else 0]
                floor = lv + (8 if form == "coupled" else 4)
                assert st["stack_max"] >= floor, (name, layout, mode, form, st["stack_max"], floor)
        r.extra_flags = 0
        _check_queries(r, c, QUERY_MODES, (name, layout))
    finally:
        r.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["geo48", "geo50"])
def test_the_depth_limit_without_a_hook(chains, monkeypatch, name):
    """No test hook set: geo(48), stack_cap 248, renders with k_mega3 (one launch) and geo(50), stack_cap 257, with the wavefront
    pipeline (choose_pipeline: a deeper stack would spill into the flag bits of word D).  On both, in the three traversal modes, the
    oracle's frame, ray count, closest hits and visibility answers -- and stacks that need the eighth bit of the depth.  geo(48) under
    CRT_PIPELINE=2 as well: k_trace far beyond CRT_STACK_LDS."""
    _clear(monkeypatch)
    c = chains(name)
    cap = c.dump[0]["stack_cap"]
    assert (cap <= MEGA3_MAX_STACK) == (name == "geo48")
    r = crt.Render(c.scene, SPP, P_RR, LSN)
    try:
        assert r.export_trees()["stack_cap"] == cap
        modes = (crt.TRAVERSAL_FAST, crt.TRAVERSAL_EXACT, crt.TRAVERSAL_REFERENCE)
        for pipeline in (None, "2") if name == "geo48" else (None,):
            if pipeline:
                monkeypatch.setenv("CRT_PIPELINE", pipeline)
            mega3 = name == "geo48" and pipeline is None
            for mode in modes:
                st = _check_frame(r, c, mode, 0, False, (name, pipeline, mode))
                assert (st["kernel_launches"] == 1) if mega3 else (st["kernel_launches"] > 1), (name, pipeline, mode, st["kernel_launches"])
                st = _check_frame(r, c, mode, 0, True, (name, pipeline, mode, "stats"))
                print("stack_max", name, "| pipeline", pipeline, "| mode", mode, ":", st["stack_max"], "of", cap)
                assert st["stack_max"] <= cap, (name, pipeline, mode, st["stack_max"], cap)
                if mode == crt.TRAVERSAL_FAST:
                    # k_mega3's coupled pool walks the four-wide tree with its leaves on the stack: beyond 7 bits of the depth byte.  k_trace
                    # walks the two-wide tree, one pending sibling per level of its 95 / 99: far beyond CRT_STACK_LDS all the same
                    floor = 128 if mega3 else TRACE_LDS_LEVELS + 8
                    assert st["stack_max"] >= floor, (name, pipeline, mode, st["stack_max"], floor)
                elif mode == crt.TRAVERSAL_EXACT:
                    # (k_mega3: the decoupled pool, inner nodes only -- the walk says 68 on this scene, the deepest of the family)
                    floor = 6 + 4 if mega3 else TRACE_LDS_LEVELS + 8
                    assert st["stack_max"] >= floor, (name, pipeline, mode, st["stack_max"], floor)
            _check_queries(r, c, modes, (name, pipeline))
    finally:
        r.free()


@pytest.mark.gpu
def test_the_device_sah_builder_on_a_hundred_levels(chains, monkeypatch):
    """build_sah_device launches k_sah_level once per level: on geo(48), depth2 95, the tree is the host builder's, byte for byte."""
    _clear(monkeypatch)
    c = chains("geo48")
    dev = crt.Render(c.scene, 1, P_RR, LSN)
    monkeypatch.setenv("CRT_SAH_HOST", "1")
    host = crt.Render(c.scene, 1, P_RR, LSN)
    monkeypatch.delenv("CRT_SAH_HOST", raising=False)
    try:
        a, b = dev.accel_info(), host.accel_info()
        assert a["sah_on_device"] == 1 and b["sah_on_device"] == 0
        for k in ("n_leaves", "n_nodes2", "n_nodes4", "depth2", "depth4", "index_splits"):
            assert a[k] == b[k] == c.dump[1][k], (k, a[k], b[k], c.dump[1][k])
        assert a["depth2"] >= 90
        _same_trees(_checked_export(dev, c.scene), _checked_export(host, c.scene))
    finally:
        dev.free()
        host.free()


@pytest.mark.gpu
def test_the_aov_pass_on_a_deep_tree(chains, monkeypatch):
    """The query form behind crt_render_aov (work item = ray) on geo(20): the oracle's primary rays folded as the contract says."""
    _clear(monkeypatch)
    c = chains("geo20")
    want = expected_aov_of(c.osc, c.scene, c.view, LSN, W, H, SPP, seed=SEED)
    assert (want["tri"] >= 0).mean() > 0.25 and len(np.unique(want["tri"])) >= 20
    r = crt.Render(c.scene, SPP, P_RR, LSN)
    try:
        r.seed = SEED
        for mode in (crt.TRAVERSAL_EXACT, crt.TRAVERSAL_FAST, crt.TRAVERSAL_REFERENCE):
            r.traversal = mode
            got = r.run_view_aov(*c.view)
            assert r.aov_info["rays"] == crt.shard_slots(W, H, 0, 1) * SPP   # (the padding slots of the ragged tiles included)
            util.assert_same(got, want, NAMES, "geo20 mode %d" % mode)
    finally:
        r.free()
