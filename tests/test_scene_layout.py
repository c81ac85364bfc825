"""The scene layout without a GPU, and the upload that adds nothing to it.  csrc/crt_scene_layout.h builds every array the kernels walk in
plain C++; tools/scene_layout_dump.cpp, compiled here with g++ and the library's host flags, runs it on a scene description and writes the
arrays of crt_scene_export.  On the CPU the invariants of the exactness proof (tests/tree_check.py, I1-I9) hold on the dump of every scene
below; on the GPU the arrays read back from device memory (Render.export_trees) equal the dump byte for byte."""
import numpy as np
import pytest

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
import tree_check as TC
import util
from scene_files import _scene, _write_box_scene, _write_soup_scene, write_signed_zero_scene
from traversal_trees import _dump, build_dump_tool

COUNTS = ["n_leaves", "n_nodes2", "n_nodes4", "depth2", "depth4", "index_splits", "layout_caps"]   # crt_accel_info without its clocks


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return build_dump_tool(tmp_path_factory.mktemp("layout_tool"))


def _make(name, d):
    if name in util.SCENES:
        return util.host_scene(name)
    if name.startswith("soup"):
        return _scene(*_write_soup_scene(d), int(name[4:]))
    if name == "one-leaf":
        return _scene(*_write_box_scene(d, n_side=12), 400)
    return _scene(*write_signed_zero_scene(d), 2)


@pytest.mark.parametrize("name", ["veach-mis", "cornell-box", "soup2", "soup5", "one-leaf", "zeros"])
def test_the_layout_built_on_the_cpu_keeps_every_tree_invariant(tool, tmp_path, name):
    scene = _make(name, str(tmp_path))
    ex, info = _dump(tool, scene, str(tmp_path))
    st = {}
    v = TC.check_trees(ex, info, scene.nodes(), scene.root, scene.triangles(), st)
    assert v == [], v
    assert info["sah_on_device"] == 0
    leaves = scene.nodes()
    leaves = leaves["n"][(leaves["lc"] < 0) & (leaves["rc"] < 0)]
    if name == "soup5":
        assert leaves.max() > 2 and not info["layout_caps"] & 8 and len(ex["nodes4i"]) == 0 and len(ex["rec_map"]) == 0
    elif name == "one-leaf":
        assert len(leaves) == 1 and ex["root_fast"] < 0 and ex["root4"] < 0 and len(ex["nodes"]) == 0 and len(ex["nodes3"]) == 0
    else:
        assert leaves.max() <= 2 and info["layout_caps"] & 8 and len(ex["nodes4i"]) == (info["n_nodes4"] + 1) * ex["node4i_f4"]
    if name == "zeros":
        assert st["crossed_zero"] > 0, st
    if name == "cornell-box":
        assert 0 < ex["n_mixed4i"] < info["n_nodes4"]      # both classes of nodes: mixed and fringe


@pytest.mark.gpu
@pytest.mark.parametrize("name,env", [("veach-mis", {"CRT_SAH_HOST": "1"}), ("soup5", {"CRT_SAH_HOST": "1"}), ("one-leaf", {"CRT_SAH_HOST": "1"}),
                                      ("zeros", {"CRT_SAH_HOST": "1"}), ("zeros", {}), ("veach-mis", {"CRT_SAH_HOST": "1", "CRT_COLLAPSE": "greedy"})],
                         ids=["veach-mis", "soup5", "one-leaf", "zeros", "zeros-device-builder", "veach-mis-greedy"])
def test_the_upload_adds_nothing_to_the_layout(tool, tmp_path, monkeypatch, name, env):
    """What crt_scene_export reads back from device memory is the tool's dump, byte for byte: all ten arrays, every crt_tree_scalars field
    and every count of crt_accel_info.  With the default (device) SAH builder on the signed-zero scene too: no range of it is split by
    index (index_splits == 0), where alone the two builders may differ (tests/test_accel_device.py)."""
    monkeypatch.delenv("CRT_SAH_HOST", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene = _make(name, str(tmp_path))
    want, want_info = _dump(tool, scene, str(tmp_path))
    r = crt.Render(scene, 1, 0.6, 1)
    try:
        got, info = r.export_trees(), r.accel_info()
    finally:
        r.free()
    for k in crt.Render.EXPORT_ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), k
    for k, _ in capi.TreeScalars._fields_:
        assert np.float32(got[k]).tobytes() == np.float32(want[k]).tobytes() if k == "coord_max" else got[k] == want[k], (k, got[k], want[k])
    for k in COUNTS:
        assert info[k] == want_info[k], (k, info[k], want_info[k])
    if "CRT_SAH_HOST" in env:
        assert info["sah_on_device"] == 0
    else:
        assert info["index_splits"] == 0
