#!/usr/bin/env python3
"""Writes tests/golden/reference_pin/: what the REFERENCE's own path code computes at the cases of tests/reference_pin.py, recorded
from oracle/_ref/path_probe (built by `make -C oracle` on a machine that has the reference tree; oracle/ref_probe/path_probe.cpp).

Per frame case: the tape of raw 32-bit draws and the camera rays (the oracle's draw log, the probe's INPUT), the flags of the paths
that take the emitter-probe branch (Render.cuh:304-313), and the probe's outputs -- cast_ray_v2's radiance per path with the number
of words it consumed, view_render_kernel's bytes per pixel with the number of words it consumed.  Per intersect case: the rays, the
visibility limits, and DeviceBVH::intersect's hit / blocked()'s verdict per ray.  Per scene case: a digest of every field of the
reference's BVH nodes, triangles and light triangles (the dump itself where it is small), and the SHA-1 of every scene file read.
samplers.npz: the records of tests/device_fn_sets.py's sampler_records() and what the reference's to_world,
get_cuda_random_sphere_vector and get_cuda_random_specular_sphere_vector (Global.h:35-94) return for them.
Data only; a second run reproduces every file byte for byte."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import reference_pin as RP  # noqa: E402

LIMIT = os.path.getsize(os.path.join(HERE, "eigen_ops.json"))   # no fixture larger than the largest one there was

if not RP.have_probe():
    sys.exit("oracle/_ref/path_probe is missing: run `make -C oracle` on a machine with the reference tree")
os.makedirs(RP.GOLD, exist_ok=True)
tmp = tempfile.mkdtemp()
meta = {"scenes": {}, "intersect": {}, "frames": {}}
sizes = {}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


for cid, name, thresh in RP.SCENE_CASES:
    spec = RP.SceneSpec(name, tmp, thresh)
    dump = RP.probe_scene(spec, tmp)
    rec = RP.scene_record(dump)
    rec.update(scene=name, unoptimised_build=name in RP.UNOPTIMISED_SCENES, bvh_thresh_n=int(spec.thresh), files_sha1=spec.file_hashes())
    raw = dump["nodes"].nbytes + dump["tris"].nbytes
    rec["stored_whole"] = bool(raw <= RP.SMALL_SCENE_BYTES)
    if rec["stored_whole"]:
        arrays = {"nodes": dump["nodes"], "tris": dump["tris"]}
        arrays.update({"light%d" % i: l for i, l in enumerate(dump["lights"])})
        sizes["scene_" + cid] = RP.save("scene_" + cid, arrays)
    meta["scenes"][cid] = rec

for name, seed in RP.INTERSECT_CASES:
    spec = RP.SceneSpec(name, tmp)
    o, d, lim = RP.intersect_inputs(name, seed, spec, spec.oracle())
    hit = RP.probe_intersect(spec, o, d, lim, tmp)
    happend = hit["happend"] == 1
    # the triangle of a hit is the one triangle whose own get_intersection reproduces it
    assert np.all(hit["matches"][happend] == 1) and np.all(hit["matches"][~happend] == 0), "ambiguous hit triangle: choose other rays"
    sizes["intersect_" + name] = RP.save("intersect_" + name, {
        "origin": o, "dir": d, "limit": lim, "happend": happend.astype(np.uint8), "t": hit["t"], "pos": hit["pos"], "normal": hit["normal"],
        "tri": hit["tri"], "blocked": (hit["blocked"] == 1).astype(np.uint8)})
    meta["intersect"][name] = {"seed": seed, "rays": int(len(o)), "random_rays": RP.N_RANDOM_RAYS, "next_event_rays": RP.N_NEE_RAYS,
                               "hits": int(happend.sum()), "blocked": int((hit["blocked"] == 1).sum()), "files_sha1": spec.file_hashes()}

agree_everywhere = True
for case in RP.FRAME_CASES:
    spec = RP.SceneSpec(case["scene"], tmp)
    of = RP.oracle_frame(spec, case)
    _, L, used, _ = RP.probe_paths(spec, case, of["rays"], of["lens"], of["words"], tmp)
    rgb, frame_used, _ = RP.probe_frame(spec, case, of["lens"], of["words"], tmp)
    flagged = of["flags"] == 1
    # the one undefined spot of the reference (Render.cuh:311-312).  How many paths may reach it is a property
    # of the case, checked here on the CPU; whether the compiled reference agrees with the oracle on them is recorded, not required.
    if case["scene"] == "cornell-box":
        assert not flagged.any(), "a cornell-box path took the emitter-probe branch"
    assert flagged.mean() <= RP.MAX_FLAGGED, "%s: %d of %d paths take the emitter-probe branch: move the camera" % (case["id"], flagged.sum(), flagged.size)
    oL = of["L"].reshape(-1, 3)
    agree = bool(same_bits(L, oL)[flagged].all())
    agree_everywhere = agree_everywhere and agree
    if not agree:
        # what the -O2 build computes on a flagged path is stale stack, not a result: it is not recorded (zeros stand in its place)
        L[flagged] = 0
        rgb[np.unique(np.nonzero(flagged)[0] // case["spp"])] = 0
    arrays = {"words": of["words"], "lens": of["lens"], "flags": of["flags"], "rays": of["rays"], "L": L, "used": used,
              "rgb": rgb.reshape(case["h"], case["w"], 3), "frame_used": frame_used.astype(np.uint32)}
    agree_unopt = None
    if flagged.any():
        # the flagged paths, and the pixels that hold one, once more through the unoptimised build of the same program
        idx = np.nonzero(flagged)[0]
        sub_lens, sub_words = RP.path_tapes(of["lens"], of["words"], idx)
        _, L0, used0, _ = RP.probe_paths(spec, case, of["rays"][idx], sub_lens, sub_words, tmp, binary=RP.PROBE_O0)
        pixels = np.unique(idx // case["spp"]).astype(np.uint32)
        rgb0, frame_used0, per_pixel0 = RP.probe_frame(spec, case, of["lens"], of["words"], tmp, pixels=pixels, binary=RP.PROBE_O0)
        assert np.array_equal(used0, used[idx]) and np.array_equal(frame_used0, per_pixel0)
        agree_unopt = bool(same_bits(L0, oL[idx]).all())
        arrays.update(flagged_L_unopt=L0, flagged_pixels=pixels, flagged_rgb_unopt=rgb0)
    sizes["frame_" + case["id"]] = RP.save("frame_" + case["id"], arrays)
    m = dict(case)
    m.update(paths=int(len(L)), rays=int(of["stats"]["rays"]), draws=int(len(of["words"])), flagged_paths=int(flagged.sum()),
             emitter_probe_paths_agree=agree, emitter_probe_paths_agree_unoptimised=agree_unopt, max_depth=int(of["stats"]["max_depth"]), files_sha1=spec.file_hashes())
    meta["frames"][case["id"]] = m
meta["emitter_probe_paths_agree"] = agree_everywhere

# the reference's own to_world / get_cuda_random_sphere_vector / get_cuda_random_specular_sphere_vector (Global.h:35-94) at chosen inputs
import device_fn_sets as DS  # noqa: E402
recs = DS.sampler_records()
res = RP.probe_samplers(recs, tmp)
arrays = {"in_" + k: recs[k] for k in RP.SAMPLER_FNS}
arrays.update({"out_" + k: res[k] for k in RP.SAMPLER_FNS})
sizes["samplers"] = RP.save("samplers", arrays)
meta["samplers"] = {k: int(len(recs[k])) for k in RP.SAMPLER_FNS}

with open(os.path.join(RP.GOLD, "meta.json"), "w") as f:
    json.dump(meta, f, indent=1, sort_keys=True)
    f.write("\n")
for k, v in sorted(sizes.items()):
    print("%-40s %7d bytes" % (k, v))
    assert v <= LIMIT, (k, v, LIMIT)
print("emitter_probe_paths_agree:", agree_everywhere)
