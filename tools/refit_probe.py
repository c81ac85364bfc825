#!/usr/bin/env python3
"""Measurements of crt_scene_refit on one GPU (docs/experiments.md, "Refitting a scene").

  time     per scene and form (CRT_REFIT_FORM=levels|walk): the device form by its HIP events (crt_refit_info.device_ms) and the host
           form by the host clock, the median of --repeat refits alternating between two positions of one object; the first refit's
           prepare_ms; the bytes a refit writes; and what a rebuild pays: crt_scene_destroy + crt_scene_create + the first frame at spp 1
           against refit + the same frame.
  quality  one object translated by 0.1, 1 and 4 times its extent: the frame (--width x --height, --spp) and the inner visits per ray
           (CRT_FLAG_STATS) on the refitted handle against a handle built from the moved scene.

Scenes: cornell-box, cornell-box-102k (scenes/gen_cornell_box.py --detail 6,5, written to a temporary directory), veach-mis, and
chain (a row of triangles in geometric progression: a deep tree).  Prints one JSON object per line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cudaraytracing_amd as crt  # noqa: E402


def translation(d):
    return [1, 0, 0, d[0], 0, 1, 0, d[1], 0, 0, 1, d[2]]


def chain_obj(d, E=40, ratio=1.2):
    """The row of tests/scene_files.py (write_geometric_chain_scene), restated: triangles from 2^-E to 2^E along x, the last one the light"""
    tris, x = [], 2.0 ** -E
    while x < 2.0 ** E:
        s = x * (ratio - 1.0) / 2.0
        tris.append(((x, 0.0, 0.0), (x + s, s, 0.0), (x, 0.0, s)))
        x *= ratio
    with open(os.path.join(d, "chain.mtl"), "w") as m:
        m.write("newmtl grey\nKd 0.6 0.6 0.6\nNs 1\nnewmtl light\nKe 20 20 20\nKd 0 0 0\nNs 1\n")
    with open(os.path.join(d, "chain.obj"), "w") as o:
        o.write("mtllib chain.mtl\nusemtl grey\n")
        for i, t in enumerate(tris):
            if i == len(tris) - 1:
                o.write("usemtl light\n")
            for p in t:
                o.write("v %.9g %.9g %.9g\nvn 0 1 0\nvt 0 0\n" % p)
            o.write("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % ((3 * i + 1,) * 3 + (3 * i + 2,) * 3 + (3 * i + 3,) * 3))
    return os.path.join(d, "chain.obj")


class Case:
    def __init__(self, name, tmp, width, height):
        self.name = name
        base = "veach-mis" if name == "veach-mis" else "cornell-box"
        self.task = crt.Task(os.path.join(ROOT, "scenes", base, "config.json"), base_dir=ROOT)
        self.thresh = self.task.bvh_thresh_n
        self.objs = list(self.task.OBJ_paths)
        if name == "cornell-box-102k":
            obj = os.path.join(tmp, "cornell-box-102k.obj")
            subprocess.run([sys.executable, os.path.join(ROOT, "scenes", "gen_cornell_box.py"), obj, "--detail", "6,5"], check=True, stdout=subprocess.DEVNULL)
            self.objs = [(obj, self.objs[0][1])]
        elif name == "chain":
            self.objs, self.thresh = [(chain_obj(tmp), tmp)], 1
        self.width, self.height = width, height
        self.cam = (self.task.eye_pos, crt.get_inverse_view_matrix(self.task.eye_pos, self.task.lookat, self.task.up), crt.fov_to_radians(self.task.fov_y))

    def scene(self):
        s = crt.Scene(self.width, self.height)
        for obj, mtl in self.objs:
            s.add_obj(obj, mtl)
        s.set_BVH(self.thresh)
        return s


def object_to_move(scene):
    """(index, extent) of the non-light object with the most triangles that is not the largest (the room)"""
    objs = scene.objects()
    order = sorted((i for i, o in enumerate(objs) if not o[0]), key=lambda i: -objs[i][2])
    idx = order[1] if len(order) > 1 else order[0]
    return idx


def extent_of(scene, idx, before):
    """the largest side of the box of the triangles that object idx's move changes"""
    scene.transform_object(idx, translation((1.0, 0.0, 0.0)))
    after = scene.triangles()
    scene.transform_object(idx, translation((-1.0, 0.0, 0.0)))
    m = np.array([before[i].tobytes() != after[i].tobytes() for i in range(len(before))])
    v = np.concatenate([before[k][m] for k in ("v1", "v2", "v3")])
    return float(np.ptp(v, axis=0).max()), int(m.sum())


def bytes_written(r, info):
    """What a refit stores: the rows, the planes of every tree (three of four rows of nodes3, six of eight of nodes4) and the box array"""
    ex = r.export_trees()
    n = sum(ex[k].nbytes for k in ("tri_geo", "tri_nm", "leaf_geo", "leaf_geo_i", "nodes", "nodes4i")) + r.export_array("ltri").nbytes
    n += ex["nodes3"].nbytes * 3 // 4 + ex["nodes4"].nbytes * 3 // 4
    n += (info["leaves"] + len(ex["nodes"]) // 4 + len(ex["nodes4"]) // 8 + len(ex["nodes4i"]) // 6) * 32
    return n


def part_time(case, repeat):
    from cudaraytracing_amd import hipmem
    for form in ("levels", "walk"):
        os.environ["CRT_REFIT_FORM"] = form
        s = case.scene()
        a = (s.triangles(), s.light_triangles())
        idx = object_to_move(s)
        ext, moved = extent_of(s, idx, a[0])
        s.transform_object(idx, translation((0.1 * ext, 0.0, 0.0)))
        b = (s.triangles(), s.light_triangles())
        s.transform_object(idx, translation((-0.1 * ext, 0.0, 0.0)))
        r = crt.Render(s, 1, 0.6, 1)
        first = r.refit(*b)
        dev = hipmem.DeviceBuffers({str(i): x.view(np.uint8).reshape(-1) for i, x in enumerate(a + b) if len(x)}, stream=True)  # (the library's own HIP runtime)
        ptr = [dev.ptrs.get(str(i)) for i in range(4)]
        d_ms, h_ms = [], []
        for k in range(repeat):
            which = k % 2
            info = r.refit_device(ptr[2 * which], ptr[2 * which + 1], stream=dev.stream, n_tris=len(a[0]), n_light_tris=len(a[1]))
            d_ms.append(info["device_ms"])
        for k in range(repeat):
            t0 = time.perf_counter()
            info = r.refit(*(a if k % 2 == 0 else b))
            h_ms.append((time.perf_counter() - t0) * 1e3)
        dev.free()
        nbytes = bytes_written(r, info)
        # what a rebuild pays against a refit: the next frame at spp 1 included
        def frame(h):
            h.run_view(*case.cam, want_mean=False)
        rebuild, refit = [], []
        for k in range(5):
            s.transform_object(idx, translation(((0.1 if k % 2 == 0 else -0.1) * ext, 0.0, 0.0)))
            t0 = time.perf_counter()
            r.refit()
            frame(r)
            refit.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            r.free()
            r = crt.Render(s, 1, 0.6, 1)
            frame(r)
            rebuild.append((time.perf_counter() - t0) * 1e3)
        acc = r.accel_info()
        med = statistics.median(d_ms)
        print(json.dumps({"part": "time", "scene": case.name, "form": form, "triangles": len(a[0]), "moved_triangles": moved, "leaves": info["leaves"],
                          "n_nodes2": acc["n_nodes2"], "n_nodes4": acc["n_nodes4"], "depth2": acc["depth2"], "depth4": acc["depth4"], "launches": info["launches"],
                          "prepare_ms": round(first["prepare_ms"], 3), "device_ms_median": round(med, 4), "device_ms_min": round(min(d_ms), 4),
                          "host_form_ms_median": round(statistics.median(h_ms), 4), "bytes_written": nbytes, "gb_per_s": round(nbytes / med / 1e6, 2),
                          "refit_plus_frame_ms": round(statistics.median(refit), 3), "rebuild_plus_frame_ms": round(statistics.median(rebuild), 3),
                          "sah_ms": round(acc["sah_ms"], 3)}), flush=True)
        r.free()
        s.free()
    os.environ.pop("CRT_REFIT_FORM", None)


def part_quality(case, spp):
    s = case.scene()
    idx = object_to_move(s)
    ext, _ = extent_of(s, idx, s.triangles())
    r = crt.Render(s, spp, 0.6, 1)
    r.seed = 1
    at = 0.0
    for f in (0.0, 0.1, 1.0, 4.0):
        s.transform_object(idx, translation(((f - at) * ext, 0.0, 0.0)))
        at = f
        if f:
            r.refit()
        fresh_scene = case.scene()
        fresh_scene.transform_object(idx, translation((f * ext, 0.0, 0.0)))
        fresh_scene.set_BVH(case.thresh)
        fr = crt.Render(fresh_scene, spp, 0.6, 1)
        fr.seed = 1
        row = {"part": "quality", "scene": case.name, "moved_by_extents": f, "extent": ext}
        # the rebuilt side's tree is the median-split tree over the moved triangles, with other leaves than the refitted handle's:
        # pixel slots whose mean differs in any bit (a ray that grazes a triangle may miss one of the two trees' leaf boxes)
        means = []
        for h in (r, fr):
            h.run_view(*case.cam)
            means.append(h.mean_buffer.copy())
        row["pixels"] = int(means[0].shape[0] * means[0].shape[1])
        row["pixels_differ"] = int((means[0].view(np.uint32) != means[1].view(np.uint32)).any(axis=2).sum())
        for name, h in (("refit", r), ("rebuilt", fr)):
            ms = []
            for _ in range(3):
                h.run_view(*case.cam, want_mean=False)
                ms.append(h.stats["kernel_ms"])
            h.run_view(*case.cam, stats=True, want_mean=False)
            row[name + "_kernel_ms"] = round(statistics.median(ms), 3)
            row[name + "_inner_per_ray"] = round(h.stats["inner_pops"] / max(1, h.stats["rays"] + h.stats["shadow_rays"] - h.stats["rays_untraced"]), 4)
            row[name + "_leaf_per_ray"] = round(h.stats["leaf_pops"] / max(1, h.stats["rays"] + h.stats["shadow_rays"] - h.stats["rays_untraced"]), 4)
        print(json.dumps(row), flush=True)
        fr.free()
        fresh_scene.free()
    r.free()
    s.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell-box,cornell-box-102k,veach-mis,chain")
    ap.add_argument("--parts", default="time,quality")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--spp", type=int, default=64)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.scenes.split(","):
            case = Case(name, tmp, a.width, a.height)
            if "time" in a.parts:
                part_time(case, a.repeat)
            if "quality" in a.parts and name != "chain":
                part_quality(case, a.spp)


if __name__ == "__main__":
    main()
