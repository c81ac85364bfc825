#!/usr/bin/env python3
"""Cost of the first-hit AOV pass next to the frame: for each scene and spp, the host-clock time of crt_render_aov_device (all six
buffers) and of crt_render_device at the same camera and params, each around the device call plus a synchronize, after a warm-up
call; best of --reps.  Prints one JSON line.  Device buffers come from the HIP runtime libcrt.so is linked against (ctypes).

  python tools/aov_probe.py [--spp 16,64,512] [--scenes cornell-box,veach-mis] [--reps 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cudaraytracing_amd as crt  # noqa: E402
from cudaraytracing_amd import _capi as capi  # noqa: E402


def hip_runtime():
    capi.lib()
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    H = C.CDLL(path)
    H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    H.hipFree.argtypes = [C.c_void_p]
    return H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", default="16,64,512")
    ap.add_argument("--scenes", default="cornell-box,veach-mis")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    w, h = a.width, a.height
    H = hip_runtime()

    def dev_alloc(nbytes):
        p = C.c_void_p()
        if H.hipMalloc(C.byref(p), nbytes) != 0:
            raise RuntimeError("hipMalloc of %d bytes failed" % nbytes)
        return p.value

    rgb = dev_alloc(w * h * 3)
    ptrs = {n: dev_alloc(w * h * ch * 4) for n, (ch, _) in capi.AOV_BUFFERS.items()}
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
                H.hipDeviceSynchronize()
                t0 = time.perf_counter()
                fn()
                H.hipDeviceSynchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if i > 0:
                    best = dt if best is None else min(best, dt)
            return best

        for spp in [int(s) for s in a.spp.split(",")]:
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
    for p in [rgb] + list(ptrs.values()):
        H.hipFree(C.c_void_p(p))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
