#!/usr/bin/env python3
"""Cost and error of the pixel reconstruction filters (CRT_FLAG_PIXEL_FILTER, crt_filtered_frame).

Cost (the default): frames of one scene in ONE process, the variants taking turns after a warm-up frame of each -- the plain frame,
the frame with CRT_FLAG_VARIANCE (k_accumulate_var), and the frame with CRT_FLAG_PIXEL_FILTER from either form of the chunk kernel
(CRT_PIXEL_FILTER_FORM=direct|staged) at reach 0, 1 and 2 (box 0.5, tent 1, mitchell 2).  Per frame, from crt_stats: the HIP-event
time of the whole device pipeline (total_ms) and of the render kernel's launches, one event pair per chunk (kernel_ms);
rest_ms = total_ms - kernel_ms is what runs after each chunk's render kernel -- k_order_items, the accumulate kernel and, with the flag,
the filter's chunk kernel (and one k_preview) -- so a variant's rest_ms minus the plain frame's is the cost of what the variant adds.
Prints the medians and one JSON line.

  python tools/pixel_filter_probe.py [--scene cornell-box] [--width 800] [--height 600] [--spp 512] [--frames 20]

--error: RGB8 mean squared error of the box-filtered frame and of the tent 1, tent 1.5 and Mitchell frames of the same paths at --spp
samples (seed 0), against a frame of --truth-spp samples with seed 7: against its box-filtered frame and against its frame under
the same filter.

  python tools/pixel_filter_probe.py --error [--scene veach-mis] [--width 160] [--height 120] [--spp 8] [--truth-spp 2048]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import cudaraytracing_amd as crt  # noqa: E402
from cudaraytracing_amd import _capi as capi  # noqa: E402
from cudaraytracing_amd import hipmem  # noqa: E402

REACHES = (("box", 0.5), ("tent", 1.0), ("mitchell", 2.0))
ERROR_FILTERS = (("tent", 1.0), ("tent", 1.5), ("mitchell", 2.0))


def cost(a, r, view):
    w, h = a.width, a.height
    dev = hipmem.DeviceBuffers({"rgb": w * h * 3, "mean": w * h * 12})
    variants = [("plain", 0, None, None), ("variance", capi.FLAG_VARIANCE, None, None)]
    for kind, radius in REACHES:
        for form in ("direct", "staged"):
            variants.append(("%s %g %s" % (kind, radius, form), capi.FLAG_PIXEL_FILTER, dict(kind=kind, radius=radius), form))

    def frame(flags, spec, form):
        r.extra_flags = flags
        if spec:
            r.set_pixel_filter(spec)
            os.environ["CRT_PIXEL_FILTER_FORM"] = form
        hipmem.device_synchronize()
        st = r.run_view_device(*view, dev.ptrs["rgb"], dev.ptrs["mean"])
        hipmem.device_synchronize()
        return {"total_ms": st["total_ms"], "kernel_ms": st["kernel_ms"], "rest_ms": st["total_ms"] - st["kernel_ms"], "launches": st["kernel_launches"]}

    runs = {v[0]: [] for v in variants}
    for i in range(a.frames + 1):          # (the first frame of each kind warms up: allocations, code objects)
        for name, flags, spec, form in variants:
            f = frame(flags, spec, form)
            if i > 0:
                runs[name].append(f)
    out = {"scene": a.scene, "width": w, "height": h, "spp": a.spp, "frames": a.frames, "chunks": runs["plain"][0]["launches"], "variants": {}}
    plain = statistics.median(f["rest_ms"] for f in runs["plain"])
    paths = w * h * a.spp
    for name, _, _, _ in variants:
        rest = [f["rest_ms"] for f in runs[name]]
        med = statistics.median(rest)
        out["variants"][name] = {"rest_ms": round(med, 3), "rest_min_max": [round(min(rest), 3), round(max(rest), 3)], "added_ms": round(med - plain, 3),
                                 "kernel_ms": round(statistics.median(f["kernel_ms"] for f in runs[name]), 3),
                                 "added_GBps_at_12B_per_path": round(12 * paths / max(med - plain, 1e-6) / 1e6, 1) if name != "plain" else None}
        print("%-22s rest %8.3f ms (%.3f .. %.3f), added %8.3f ms" % (name, med, min(rest), max(rest), med - plain))
    dev.free()
    print(json.dumps(out), flush=True)


def mse(x, y):
    return float(np.mean((x.astype(np.float64) - y.astype(np.float64)) ** 2))


def error(a, r, view):
    w, h = a.width, a.height

    def frames(spp, seed):
        """the box-filtered frame and the frame under each of ERROR_FILTERS, RGB8, of the same paths"""
        r.set_spp(spp)
        r.seed = seed
        out = {}
        for kind, radius in ERROR_FILTERS:
            r.set_pixel_filter(dict(kind=kind, radius=radius))
            out["box"] = r.run_view(*view, width=w, height=h, pixel_filter=True).copy()
            out["%s %g" % (kind, radius)] = r.filtered_rgb
        return out

    truth = frames(a.truth_spp, 7)
    got = frames(a.spp, 0)
    out = {"scene": a.scene, "width": w, "height": h, "spp": a.spp, "truth_spp": a.truth_spp, "box": round(mse(got["box"], truth["box"]), 1)}
    for kind, radius in ERROR_FILTERS:
        k = "%s %g" % (kind, radius)
        out[k] = {"against_box_truth": round(mse(got[k], truth["box"]), 1), "against_same_filter_truth": round(mse(got[k], truth[k]), 1)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell-box")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--error", action="store_true")
    ap.add_argument("--truth-spp", type=int, default=2048)
    a = ap.parse_args()
    if crt.device_count() < 1:
        raise SystemExit("pixel_filter_probe: no HIP device")
    t = crt.Task(os.path.join(ROOT, "scenes", a.scene, "config.json"), base_dir=ROOT)
    r = crt.Render(crt.Scene.from_task(t, a.width, a.height), a.spp, t.P_RR, t.light_sample_n)
    view = (t.eye_pos, crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up), crt.fov_to_radians(t.fov_y))
    try:
        (error if a.error else cost)(a, r, view)
    finally:
        r.free()


if __name__ == "__main__":
    main()
