#!/usr/bin/env python3
"""Cost of the first-hit AOV pass next to the frame: for each scene and spp, the host-clock time of crt_render_aov_device (all six
buffers) and of crt_render_device at the same camera and params, each around the device call plus a synchronize, after a warm-up
call; best of --reps.  Prints one JSON line.  Device buffers come from cudaraytracing_amd/hipmem.py.

  python tools/aov_probe.py [--spp 16,64,512] [--scenes cornell-box,veach-mis] [--reps 3]

--specular instead times the pass that follows mirror bounces (crt_render_aov_specular_device, all five buffers, --bounces) beside
crt_render_aov_device in one process, the two taking turns: the HIP-event time of each call (its info) and the host-clock time around
it, median and best of --reps, at --spp (default 64).  The specular call synchronizes its stream once per bounce and chunk to read how
many rays go on; `syncs` is that count and `sync_us` the host-clock time of one 4-byte device-to-host copy on the idle device, which is
what one such round trip costs at least.

  python tools/aov_probe.py --specular [--spp 64] [--bounces 1,2] [--reps 20]

--shading times the pass with the shading AOVs (crt_render_aov_shading_device, the six first-hit buffers and its two) beside
crt_render_aov_device in one process, the two taking turns: the HIP-event time of each call, median and best of --reps, at --spp
(default 64).

  python tools/aov_probe.py --shading [--spp 64] [--reps 20]

--direct times the direct-light pass (crt_render_aov_direct_device, its four buffers) beside crt_render_aov_device and beside a frame at
p_rr = 0 -- which traces the same camera and shadow rays inside the render kernel -- in one process, the three taking turns: the
host-clock time around each call plus a synchronize, median and best of --reps, at --spp (default 64).  Also the pass's rays (camera,
traced shadow rays, samples not traced), its sub-batches = host synchronizations per call, and the frame's own counts from one call with
statistics.

  python tools/aov_probe.py --direct [--spp 64] [--reps 20]

--ao times the ambient-occlusion pass (crt_render_aov_ao_device, its three buffers, crt_aov_ao_defaults' settings) beside
crt_render_aov_device and crt_render_aov_direct_device in one process, the three taking turns: the HIP-event time of each call (its
info), median and best of --reps, at --spp (default 64), and each call's rays -- so also the time per occlusion ray beside the direct
pass's time per shadow ray, both with the time of crt_render_aov, which traces the same camera rays, taken off.

  python tools/aov_probe.py --ao [--spp 64] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cudaraytracing_amd as crt  # noqa: E402
from cudaraytracing_amd import _capi as capi  # noqa: E402
from cudaraytracing_amd import hipmem  # noqa: E402


def image_buffers(a, table):
    return hipmem.DeviceBuffers.image(table, a.width, a.height, stream=False)


def specular(a):
    """The two AOV passes side by side (see the module's text)."""
    w, h = a.width, a.height
    first, second = image_buffers(a, capi.AOV_BUFFERS), image_buffers(a, capi.AOV_SPECULAR_BUFFERS)
    ptrs, sptrs = first.ptrs, second.ptrs
    word = np.zeros(1, dtype=np.uint32)
    us = []
    for _ in range(200):
        hipmem.device_synchronize()
        t0 = time.perf_counter()
        first.download("depth", out=word, offset=0)
        us.append((time.perf_counter() - t0) * 1e6)
    out = {"width": w, "height": h, "reps": a.reps, "sync_us": round(statistics.median(us[20:]), 2), "runs": []}
    spps = [int(s) for s in a.spp.split(",")] if a.spp is not None else [64]
    for name in a.scenes.split(","):
        t = crt.Task(os.path.join(ROOT, "scenes", name, "config.json"), base_dir=ROOT)
        sc = crt.Scene.from_task(t, w, h)
        r = crt.Render(sc, 1, t.P_RR, t.light_sample_n)
        iv = crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up)
        fov = crt.fov_to_radians(t.fov_y)
        for spp in spps:
            r.set_spp(spp)
            for mb in [int(v) for v in a.bounces.split(",")]:
                ev = {"aov": [], "spec": []}
                host = {"aov": [], "spec": []}
                for i in range(a.reps + 2):  # (the first two rounds warm up: allocations, code objects)
                    for key, fn in (("aov", lambda: r.run_view_aov_device(t.eye_pos, iv, fov, ptrs)),
                                    ("spec", lambda: r.run_view_aov_specular_device(t.eye_pos, iv, fov, sptrs, max_bounces=mb))):
                        hipmem.device_synchronize()
                        t0 = time.perf_counter()
                        info = fn()
                        dt = (time.perf_counter() - t0) * 1e3
                        if i >= 2:
                            ev[key].append(info["total_ms"])
                            host[key].append(dt)
                info = r.aov_specular_info
                camera_rays = r.aov_info["rays"]
                # one synchronization after every bounce kernel but the one at the cap; a chunk whose count comes back 0 stops there
                run = {"scene": name, "spp": spp, "max_bounces": mb, "chunks": info["chunks"], "camera_rays": camera_rays,
                       "reflected_rays": info["rays"] - camera_rays,
                       "aov_event_ms": round(statistics.median(ev["aov"]), 4), "aov_event_ms_best": round(min(ev["aov"]), 4),
                       "specular_event_ms": round(statistics.median(ev["spec"]), 4), "specular_event_ms_best": round(min(ev["spec"]), 4),
                       "aov_host_ms": round(statistics.median(host["aov"]), 4), "specular_host_ms": round(statistics.median(host["spec"]), 4),
                       "specular_over_aov": round(statistics.median(ev["spec"]) / statistics.median(ev["aov"]), 3)}
                out["runs"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
        r.free()
    first.free()
    second.free()
    print(json.dumps(out), flush=True)


def shading(a):
    """--shading: crt_render_aov_shading_device (all eight buffers) beside crt_render_aov_device (its six), the two taking turns: the
    HIP-event time of each call, median and best of --reps.  One trace serves both structs, so the difference is the resolve's."""
    w, h = a.width, a.height
    first, second = image_buffers(a, capi.AOV_BUFFERS), image_buffers(a, capi.AOV_SHADING_BUFFERS)
    ptrs, sptrs = first.ptrs, second.ptrs
    out = {"width": w, "height": h, "reps": a.reps, "runs": []}
    spps = [int(s) for s in a.spp.split(",")] if a.spp is not None else [64]
    for name in a.scenes.split(","):
        t = crt.Task(os.path.join(ROOT, "scenes", name, "config.json"), base_dir=ROOT)
        r = crt.Render(crt.Scene.from_task(t, w, h), 1, t.P_RR, t.light_sample_n)
        iv = crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up)
        fov = crt.fov_to_radians(t.fov_y)
        for spp in spps:
            r.set_spp(spp)
            ev = {"aov": [], "shading": []}
            for i in range(a.reps + 2):  # (the first two rounds warm up: allocations, code objects)
                for key, fn in (("aov", lambda: r.run_view_aov_device(t.eye_pos, iv, fov, ptrs)),
                                ("shading", lambda: r.run_view_aov_shading_device(t.eye_pos, iv, fov, sptrs, first_ptrs=ptrs))):
                    hipmem.device_synchronize()
                    info = fn()
                    if i >= 2:
                        ev[key].append(info["total_ms"])
            med = {k: statistics.median(v) for k, v in ev.items()}
            run = {"scene": name, "spp": spp, "chunks": r.aov_info["chunks"], "rays": r.aov_info["rays"],
                   "aov_event_ms": round(med["aov"], 4), "aov_event_ms_best": round(min(ev["aov"]), 4),
                   "shading_event_ms": round(med["shading"], 4), "shading_event_ms_best": round(min(ev["shading"]), 4),
                   "shading_over_aov": round(med["shading"] / med["aov"], 4)}
            out["runs"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
        r.free()
    first.free()
    second.free()
    print(json.dumps(out), flush=True)


def direct(a):
    """--direct: see the module's text."""
    w, h = a.width, a.height
    first, second, frame = image_buffers(a, capi.AOV_BUFFERS), image_buffers(a, capi.AOV_DIRECT_BUFFERS), hipmem.DeviceBuffers({"rgb": w * h * 3})
    out = {"width": w, "height": h, "reps": a.reps, "runs": []}
    spps = [int(s) for s in a.spp.split(",")] if a.spp is not None else [64]
    for name in a.scenes.split(","):
        t = crt.Task(os.path.join(ROOT, "scenes", name, "config.json"), base_dir=ROOT)
        r = crt.Render(crt.Scene.from_task(t, w, h), 1, 0.0, t.light_sample_n)  # (p_rr = 0: every path of the frame ends at its first vertex)
        iv = crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up)
        fov = crt.fov_to_radians(t.fov_y)
        calls = (("aov", lambda: r.run_view_aov_device(t.eye_pos, iv, fov, first.ptrs, want_info=False)),
                 ("direct", lambda: r.run_view_aov_direct_device(t.eye_pos, iv, fov, second.ptrs, want_info=False)),
                 ("frame", lambda: r.run_view_device(t.eye_pos, iv, fov, frame.ptrs["rgb"], want_stats=False)))
        for spp in spps:
            r.set_spp(spp)
            ms = {k: [] for k, _ in calls}
            for i in range(a.reps + 2):  # (the first two rounds warm up: allocations, code objects)
                for key, fn in calls:
                    hipmem.device_synchronize()
                    t0 = time.perf_counter()
                    fn()
                    hipmem.device_synchronize()
                    if i >= 2:
                        ms[key].append((time.perf_counter() - t0) * 1e3)
            info = r.run_view_aov_direct_device(t.eye_pos, iv, fov, second.ptrs)
            camera_rays = r.run_view_aov_device(t.eye_pos, iv, fov, first.ptrs)["rays"]
            st = r.run_view_device(t.eye_pos, iv, fov, frame.ptrs["rgb"], want_stats=True)
            med = {k: statistics.median(v) for k, v in ms.items()}
            run = {"scene": name, "spp": spp, "light_sample_n": t.light_sample_n, "sub_batches": info["chunks"], "syncs_per_call": info["chunks"],
                   "camera_rays": camera_rays, "shadow_rays_traced": info["rays"] - camera_rays, "direct_event_ms": round(info["total_ms"], 4),
                   "frame_rays": st["rays"], "frame_shadow_rays": st["shadow_rays"], "frame_rays_untraced": st["rays_untraced"],
                   "aov_ms": round(med["aov"], 4), "aov_ms_best": round(min(ms["aov"]), 4),
                   "direct_ms": round(med["direct"], 4), "direct_ms_best": round(min(ms["direct"]), 4),
                   "frame_p_rr_0_ms": round(med["frame"], 4), "frame_p_rr_0_ms_best": round(min(ms["frame"]), 4),
                   "direct_over_frame": round(med["direct"] / med["frame"], 4), "direct_over_aov": round(med["direct"] / med["aov"], 4)}
            out["runs"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
        r.free()
    for b in (first, second, frame):
        b.free()
    print(json.dumps(out), flush=True)


def ao(a):
    """--ao: see the module's text."""
    w, h = a.width, a.height
    first, second, third = image_buffers(a, capi.AOV_BUFFERS), image_buffers(a, capi.AOV_DIRECT_BUFFERS), image_buffers(a, capi.AOV_AO_BUFFERS)
    out = {"width": w, "height": h, "reps": a.reps, "runs": []}
    spps = [int(s) for s in a.spp.split(",")] if a.spp is not None else [64]
    for name in a.scenes.split(","):
        t = crt.Task(os.path.join(ROOT, "scenes", name, "config.json"), base_dir=ROOT)
        r = crt.Render(crt.Scene.from_task(t, w, h), 1, t.P_RR, t.light_sample_n)
        iv = crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up)
        fov = crt.fov_to_radians(t.fov_y)
        calls = (("aov", lambda: r.run_view_aov_device(t.eye_pos, iv, fov, first.ptrs)),
                 ("direct", lambda: r.run_view_aov_direct_device(t.eye_pos, iv, fov, second.ptrs)),
                 ("ao", lambda: r.run_view_aov_ao_device(t.eye_pos, iv, fov, third.ptrs)))
        for spp in spps:
            r.set_spp(spp)
            ms = {k: [] for k, _ in calls}
            info = {}
            for i in range(a.reps + 2):  # (the first two rounds warm up: allocations, code objects)
                for key, fn in calls:
                    info[key] = dict(fn())
                    if i >= 2:
                        ms[key].append(info[key]["total_ms"])
            med = {k: statistics.median(v) for k, v in ms.items()}
            camera_rays = info["aov"]["rays"]
            shadow_rays, ao_rays = info["direct"]["rays"] - camera_rays, info["ao"]["rays"] - camera_rays
            ns_shadow = (med["direct"] - med["aov"]) * 1e6 / max(1, shadow_rays)
            ns_ao = (med["ao"] - med["aov"]) * 1e6 / max(1, ao_rays)
            run = {"scene": name, "spp": spp, **r.aov_ao_defaults(), "camera_rays": camera_rays, "shadow_rays": shadow_rays, "ao_rays": ao_rays,
                   "ao_sub_batches": info["ao"]["chunks"], "direct_sub_batches": info["direct"]["chunks"],
                   "aov_ms": round(med["aov"], 4), "aov_ms_best": round(min(ms["aov"]), 4),
                   "direct_ms": round(med["direct"], 4), "direct_ms_best": round(min(ms["direct"]), 4),
                   "ao_ms": round(med["ao"], 4), "ao_ms_best": round(min(ms["ao"]), 4),
                   "ns_per_shadow_ray": round(ns_shadow, 4), "ns_per_ao_ray": round(ns_ao, 4), "ao_over_direct_per_ray": round(ns_ao / ns_shadow, 3) if ns_shadow > 0 else None}
            out["runs"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
        r.free()
    for b in (first, second, third):
        b.free()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", default=None, help="comma-separated; default 16,64,512, with --specular / --shading / --direct / --ao 64")
    ap.add_argument("--scenes", default="cornell-box,veach-mis")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--specular", action="store_true", help="time crt_render_aov_specular_device beside crt_render_aov_device")
    ap.add_argument("--bounces", default="1,2", help="--specular: the max_bounces values")
    ap.add_argument("--shading", action="store_true", help="time crt_render_aov_shading_device beside crt_render_aov_device")
    ap.add_argument("--direct", action="store_true", help="time crt_render_aov_direct_device beside crt_render_aov_device and a frame at p_rr = 0")
    ap.add_argument("--ao", action="store_true", help="time crt_render_aov_ao_device beside crt_render_aov_device and crt_render_aov_direct_device")
    a = ap.parse_args()
    w, h = a.width, a.height
    if a.ao:
        return ao(a)
    if a.specular:
        return specular(a)
    if a.shading:
        return shading(a)
    if a.direct:
        return direct(a)
    frame, aovs = hipmem.DeviceBuffers({"rgb": w * h * 3}), image_buffers(a, capi.AOV_BUFFERS)
    rgb, ptrs = frame.ptrs["rgb"], aovs.ptrs
    out = {"width": w, "height": h, "reps": a.reps, "runs": []}
    for name in a.scenes.split(","):
        t = crt.Task(os.path.join(ROOT, "scenes", name, "config.json"), base_dir=ROOT)
        sc = crt.Scene.from_task(t, w, h)
        r = crt.Render(sc, 1, t.P_RR, t.light_sample_n)
        iv = crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up)
        fov = crt.fov_to_radians(t.fov_y)

        def timed(fn):
            best = None
            for i in range(a.reps + 1):  # (the first call warms up: allocations, code objects)
                hipmem.device_synchronize()
                t0 = time.perf_counter()
                fn()
                hipmem.device_synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if i > 0:
                    best = dt if best is None else min(best, dt)
            return best

        for spp in [int(s) for s in (a.spp or "16,64,512").split(",")]:
            r.set_spp(spp)
            aov_ms = timed(lambda: r.run_view_aov_device(t.eye_pos, iv, fov, ptrs, want_info=False))
            frame_ms = timed(lambda: r.run_view_device(t.eye_pos, iv, fov, rgb, want_stats=False))
            info = r.run_view_aov_device(t.eye_pos, iv, fov, ptrs)  # (HIP-event time of the pass, chunks)
            rays = info["rays"]
            out["runs"].append({"scene": name, "spp": spp, "aov_ms": round(aov_ms, 3), "frame_ms": round(frame_ms, 3),
                                "ratio": round(aov_ms / frame_ms, 4), "aov_event_ms": round(info["total_ms"], 3), "chunks": info["chunks"],
                                "rays": rays, "primary_Grays_per_s": round(rays / aov_ms / 1e6, 3)})
            print(json.dumps(out["runs"][-1]), file=sys.stderr, flush=True)
        r.free()
    frame.free()
    aovs.free()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
