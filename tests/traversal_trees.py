"""What the tree tests share: the environment of each form of k_mega3's pool with the stack levels it keeps in LDS, the comparison of two
handles' exported trees, the scene-layout tool's dump (tools/scene_layout_dump.cpp: the layout built on the CPU), and a numpy walk of an
exported nodes4 that counts the stack entries a ray leaves pending -- it chooses inputs for the deep-tree tests and asserts nothing about
the device."""
import os
import subprocess

import numpy as np

import cudaraytracing_amd as crt
from cudaraytracing_amd import _capi as capi
import host_program as HP
import tree_check as TC

LAYOUTS = {  # environment of each form of k_mega3's pool (csrc/crt_render.hip: use_dec, use_ref16, use_impl)
    "coupled-16": {"CRT_DEC": "0"},
    "coupled-32": {"CRT_DEC": "0", "CRT_REF16": "0"},
    "decoupled-16": {"CRT_DEC": "1"},                       # (on the tree without its rows of refs where the scene offers it: both shipped scenes do)
    "decoupled-16, rows of refs": {"CRT_DEC": "1", "CRT_IMPL": "0"},
    "decoupled-32": {"CRT_DEC": "1", "CRT_REF32": "1"},
    "default": {},  # decoupled-16 for CRT_TRAVERSAL_EXACT on a scene of up to about 160 000 triangles, coupled-16 for the other modes
    "default, leaf records beyond 16 bits": {"CRT_REF16": "0"},  # a scene of 50 000 - 160 000 triangles: coupled-32 for the other modes
}
LAYOUT_HOOKS = ("CRT_DEC", "CRT_REF16", "CRT_REF32", "CRT_IMPL")

# (form, stack levels in LDS) of each layout for CRT_TRAVERSAL_FAST / _REFERENCE and for CRT_TRAVERSAL_EXACT on a scene whose refs fit 16
# bits (csrc/crt_mega3.h: eight 16-bit or four 32-bit levels in the coupled pool, six or three in the decoupled one)
LDS_LEVELS = {
    "coupled-16": (("coupled", 8), ("coupled", 8)),
    "coupled-32": (("coupled", 4), ("coupled", 4)),
    "decoupled-16": (("decoupled", 6), ("decoupled", 6)),
    "decoupled-16, rows of refs": (("decoupled", 6), ("decoupled", 6)),
    "decoupled-32": (("decoupled", 3), ("decoupled", 3)),
    "default": (("coupled", 8), ("decoupled", 6)),
    "default, leaf records beyond 16 bits": (("coupled", 4), ("decoupled", 6)),
}

TREE_ARRAYS = ("nodes", "nodes3", "nodes4", "nodes4i", "leaf_geo_i", "rec_map")


def set_layout(monkeypatch, layout):
    for k in LAYOUT_HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in LAYOUTS[layout].items():
        monkeypatch.setenv(k, v)


def _checked_export(r, scene):
    """The trees of a handle (Render.export_trees), after tests/tree_check.py found no violation in them."""
    ex = r.export_trees()
    v = TC.check_trees(ex, r.accel_info(), scene.nodes(), scene.root, scene.triangles())
    assert v == [], v
    return ex


def _same_trees(a, b):
    for k in TREE_ARRAYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ("root4", "root4i", "n_mixed4i", "coord_max", "stack_cap"):
        assert a[k] == b[k], k


def build_dump_tool(d):
    return HP.build("scene_layout_dump.cpp", os.path.join(str(d), "scene_layout_dump"), extra=["-pthread", "-fno-fast-math"])


def _dump(tool, scene, d):
    """The tool's arrays and scalars in the dict shape of Render.export_trees(), and its crt_accel_info as accel_info() gives it."""
    for name, a in (("nodes", scene.nodes()), ("tris", scene.triangles()), ("light_tris", scene.light_triangles()),
                    ("materials", scene.materials()), ("lights", scene.lights())):
        a.tofile(os.path.join(d, "desc_%s.bin" % name))
    subprocess.run([tool, d, str(scene.root)], check=True, timeout=300)
    ex = {}
    for name, dt in crt.Render.EXPORT_ARRAYS.items():
        a = np.fromfile(os.path.join(d, name + ".bin"), dtype=dt)
        ex[name] = a.reshape(-1, 4) if dt is np.float32 else a
    with open(os.path.join(d, "scalars.bin"), "rb") as f:
        ex.update(capi.TreeScalars.from_buffer_copy(f.read()).as_dict())
    with open(os.path.join(d, "accel.bin"), "rb") as f:
        info = capi.AccelInfo.from_buffer_copy(f.read()).as_dict()
    return ex, info


def pending_entries(ex, o, d):
    """Walks each ray (o, d: (n, 3)) through the exported nodes4 as an unpruned traversal does -- the nearest child that the slab test
    enters next, the others pushed -- and returns the largest number of pending stack entries per ray, once with leaves on the stack (the
    coupled pool) and once with inner nodes only (the decoupled pool).  float64 slabs, no leaf tests: a prediction of which rays go deep."""
    n4 = ex["nodes4"].reshape(-1, 8, 4).astype(np.float64)
    refs = np.ascontiguousarray(ex["nodes4"]).reshape(-1, 8, 4)[:, 6, :].view(np.int32)
    root = int(ex["root4"])
    o = np.asarray(o, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    out = np.zeros((len(o), 2), dtype=np.int64)
    if root < 0:
        return out
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        for i in range(len(o)):
            for with_leaves in (True, False):
                stack, deepest, node = [], 0, root
                while True:
                    if node >= 0:
                        b = n4[node]
                        t0 = (b[0::2][:3] - o[i][:, None]) * inv[i][:, None]
                        t1 = (b[1::2][:3] - o[i][:, None]) * inv[i][:, None]
                        near = np.fmax.reduce(np.minimum(t0, t1), axis=0)
                        far = np.fmin.reduce(np.maximum(t0, t1), axis=0)
                        hit = (near <= far) & (far >= 0) & (refs[node] != TC.EMPTY_REF)
                        kids = [(near[k], int(refs[node][k])) for k in range(4) if hit[k] and (with_leaves or refs[node][k] >= 0)]
                        kids.sort(key=lambda e: -e[0])             # farthest first; the nearest is visited next
                        nxt = kids.pop()[1] if kids else None
                        stack.extend(r for _, r in kids)
                        deepest = max(deepest, len(stack))
                        if nxt is not None:
                            node = nxt
                            continue
                    if not stack:
                        break
                    node = stack.pop()
                out[i, 0 if with_leaves else 1] = deepest
    return out
