#!/usr/bin/env python3
"""Cost of CRT_FLAG_VARIANCE: frames of one scene with and without the flag in ONE process, taking turns, after a warm-up frame of each.
Per frame: the host clock around crt_render_device plus a synchronize, and from crt_stats the HIP-event time of the whole device
pipeline (total_ms) and of the render kernel (kernel_ms); total_ms - kernel_ms is k_order_items plus k_accumulate, the only kernel the
flag changes.  Prints the medians, the differences and the time of crt_variance_device itself.  One JSON line.

  python tools/variance_probe.py [--scene cornell-box] [--width 800] [--height 600] [--spp 512] [--frames 7]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cudaraytracing_amd as crt  # noqa: E402
from cudaraytracing_amd import _capi as capi  # noqa: E402
from cudaraytracing_amd import hipmem  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell-box")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--frames", type=int, default=7)
    a = ap.parse_args()
    if crt.device_count() < 1:
        raise SystemExit("variance_probe: no HIP device")
    w, h = a.width, a.height
    dev = hipmem.DeviceBuffers({"rgb": w * h * 3, "mean": w * h * 12, "var": w * h * 12})
    bufs = dev.ptrs
    t = crt.Task(os.path.join(ROOT, "scenes", a.scene, "config.json"), base_dir=ROOT)
    r = crt.Render(crt.Scene.from_task(t, w, h), a.spp, t.P_RR, t.light_sample_n)
    iv = crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up)
    fov = crt.fov_to_radians(t.fov_y)

    def frame(flag):
        r.extra_flags = capi.FLAG_VARIANCE if flag else 0
        hipmem.device_synchronize()
        t0 = time.perf_counter()
        st = r.run_view_device(t.eye_pos, iv, fov, bufs["rgb"], bufs["mean"])
        hipmem.device_synchronize()
        return {"wall_ms": (time.perf_counter() - t0) * 1e3, "total_ms": st["total_ms"], "kernel_ms": st["kernel_ms"],
                "rest_ms": st["total_ms"] - st["kernel_ms"]}

    runs = {False: [], True: []}
    read_ms = []
    for i in range(a.frames + 1):          # (the first frame of each kind warms up: allocations, code objects)
        for flag in (False, True):
            f = frame(flag)
            if flag:
                hipmem.device_synchronize()
                t0 = time.perf_counter()
                capi.check(capi.lib().crt_variance_device(r._h, C.c_void_p(bufs["var"]), None, None), "crt_variance_device")
                hipmem.device_synchronize()
                f["read_ms"] = (time.perf_counter() - t0) * 1e3
            if i > 0:
                runs[flag].append(f)
                if flag:
                    read_ms.append(f["read_ms"])
    out = {"scene": a.scene, "width": w, "height": h, "spp": a.spp, "frames": a.frames}
    for key in ("wall_ms", "total_ms", "kernel_ms", "rest_ms"):
        plain = statistics.median(f[key] for f in runs[False])
        var = statistics.median(f[key] for f in runs[True])
        out[key] = {"plain": round(plain, 3), "variance": round(var, 3), "difference": round(var - plain, 3),
                    "plain_min_max": [round(min(f[key] for f in runs[False]), 3), round(max(f[key] for f in runs[False]), 3)]}
    out["crt_variance_device_wall_ms"] = round(statistics.median(read_ms), 3)
    r.free()
    dev.free()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
