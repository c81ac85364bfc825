#!/usr/bin/env python3
"""What the frame's error summary (crt_frame_error) and rendering to an error target (crt_render_until) cost and buy, on one GPU, in one
process, the calls of a comparison taking turns.  One JSON line per row on stdout and, with --out, in a file.

  summary   crt_frame_error_device beside crt_variance_device (which reads the same 24 B per pixel slot and is the yardstick) on the
            sums of a frame in flight, at every --summary-sizes: HIP events on a stream around each call, the median of --repeat
  check     one check of crt_render_until (a call that continues the frame in flight with a target already met: one summary, one 8-byte
            copy, the preview) against what a caller pays without it: crt_variance and crt_preview to the host and the numpy reduction.
            Host clock, both ending with the data on the host
  overhead  crt_render_until with a target nothing meets (threshold 0) against crt_render_range in the same steps, cap --spp: the
            difference is the price of the checks
  quality   per scene and threshold of --thresholds, at --fractions of the pixels allowed above the target: time, samples done and the
            RGB8 mean squared error against a uniform frame of --ref-spp samples -- beside the rows of crt_render_adaptive and
            crt_render_planned (tools/adaptive_probe.py, docs/experiments.md) at the same threshold.  A frame of crt_render_until IS the
            uniform frame of its samples: the row says where the target stops it

    python tools/until_probe.py --out until_probe.jsonl
"""
import argparse
import ctypes as C
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

SCENES = {n: os.path.join(ROOT, "scenes", n, "config.json") for n in ("cornell-box", "veach-mis")}
F = np.float32


class Events:
    """A pair of HIP events on the runtime the library calls"""

    def __init__(self):
        self.H = hipmem.runtime()
        self.H.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.H.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.H.hipEventSynchronize.argtypes = [C.c_void_p]
        self.H.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.H.hipEventDestroy.argtypes = [C.c_void_p]
        self.e = [C.c_void_p(), C.c_void_p()]
        for e in self.e:
            assert self.H.hipEventCreate(C.byref(e)) == 0

    def time(self, stream, fn):
        assert self.H.hipEventRecord(self.e[0], stream) == 0
        fn()
        assert self.H.hipEventRecord(self.e[1], stream) == 0 and self.H.hipEventSynchronize(self.e[1]) == 0
        ms = C.c_float()
        assert self.H.hipEventElapsedTime(C.byref(ms), self.e[0], self.e[1]) == 0
        return float(ms.value)

    def free(self):
        for e in self.e:
            self.H.hipEventDestroy(e)


def spread(ms):
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def wall(fn):
    hipmem.device_synchronize()
    t0 = time.perf_counter()
    fn()
    hipmem.device_synchronize()
    return (time.perf_counter() - t0) * 1e3


def mse(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float((d * d).mean())


def host_reduction(var, mean, threshold, mean_floor):
    """What a caller computes today from crt_variance and crt_preview on the host: the pixels above the target"""
    v = (var[..., 0] + var[..., 1]) + var[..., 2]
    m = (mean[..., 0] + mean[..., 1]) + mean[..., 2]
    t = F(threshold) * (m + F(mean_floor))
    return int((~(v <= t * t)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell-box,veach-mis")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--min", type=int, default=16)
    ap.add_argument("--step", type=int, default=64)
    ap.add_argument("--thresholds", default="0.1,0.05,0.02")
    ap.add_argument("--fractions", default="0,0.05")
    ap.add_argument("--summary-sizes", default="800x600,3840x2160")
    ap.add_argument("--repeat", type=int, default=50)
    ap.add_argument("--frames", type=int, default=5, help="repetitions of the whole-frame comparisons")
    ap.add_argument("--parts", default="summary,check,overhead,quality")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if crt.device_count() < 1:
        raise SystemExit("until_probe: no HIP device")
    out = open(a.out, "w") if a.out else None
    parts = a.parts.split(",")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    w, h = a.width, a.height
    ev = Events()
    for name in a.scenes.split(","):
        t = crt.Task(SCENES[name], base_dir=ROOT)
        cam = (t.eye_pos, crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up), crt.fov_to_radians(t.fov_y))
        r = crt.Render(crt.Scene.from_task(t), a.spp, t.P_RR, t.light_sample_n)
        first = name == a.scenes.split(",")[0]
        if "summary" in parts and first:
            for size in a.summary_sizes.split(","):
                sw, sh = (int(x) for x in size.split("x"))
                r.set_spp(8)
                r.run_view_range(*cam, 0, 4, width=sw, height=sh, want_variance=True)
                with hipmem.DeviceBuffers({"info": C.sizeof(capi.FrameErrorInfo), "var": sw * sh * 12}, stream=True) as d:
                    st = C.c_void_p(d.stream)
                    calls = {"frame_error": lambda: r.frame_error_device(d.ptrs["info"], stream=d.stream),
                             "variance": lambda: capi.check(capi.lib().crt_variance_device(r._h, C.c_void_p(d.ptrs["var"]), st, None), "crt_variance_device")}
                    ms = {k: [] for k in calls}
                    for i in range(a.repeat + 3):            # (the first three of each warm up)
                        for k, fn in calls.items():
                            x = ev.time(st, fn)
                            if i >= 3:
                                ms[k].append(x)
                emit(dict(part="summary", scene=name, width=sw, height=sh, slots=crt.shard_slots(sw, sh, 0, 1), repeat=a.repeat,
                          frame_error_device_ms=spread(ms["frame_error"]), variance_device_ms=spread(ms["variance"]),
                          ratio=round(statistics.median(ms["frame_error"]) / statistics.median(ms["variance"]), 3)))
        if "check" in parts and first:
            r.set_spp(a.spp)
            r.run_view_range(*cam, 0, a.min, width=w, height=h, want_variance=True)
            d = crt.frame_error_defaults()
            above = []

            def today():
                var = r.variance(width=w, height=h)[0]
                mean = r.preview(want_mean=True, width=w, height=h)[1]
                above.append(host_reduction(var, mean, d["threshold"], d["mean_floor"]))

            def check():
                r.run_view_until(*cam, min_samples=a.min, threshold=np.inf, sample_begin=a.min, want_mean=False, width=w, height=h)

            def summary():
                above.append(r.frame_error().above)

            ms = {"today": [], "until_check": [], "frame_error": []}
            for i in range(a.repeat + 3):
                for k, fn in (("today", today), ("until_check", check), ("frame_error", summary)):
                    x = wall(fn)
                    if i >= 3:
                        ms[k].append(x)
            assert len(set(above)) == 1, "the host reduction and crt_frame_error disagree on the pixels above the target"
            emit(dict(part="check", scene=name, width=w, height=h, samples=a.min, repeat=a.repeat, above=above[0],
                      today_variance_preview_numpy_wall_ms=spread(ms["today"]), until_check_with_rgb_preview_wall_ms=spread(ms["until_check"]),
                      frame_error_host_form_wall_ms=spread(ms["frame_error"])))
        if "overhead" in parts:
            r.set_spp(a.spp)

            def ranges():
                n = 0
                for ns in [a.min] + [a.step] * ((a.spp - a.min + a.step - 1) // a.step):
                    ns = min(ns, a.spp - n)
                    r.run_view_range(*cam, n, ns, width=w, height=h, want_variance=True, want_mean=False)
                    n += ns

            def until():
                r.run_view_until(*cam, min_samples=a.min, step_samples=a.step, threshold=0.0, max_above=0, want_mean=False, width=w, height=h)

            ms = {"ranges": [], "until": []}
            for i in range(a.frames + 1):
                for k, fn in (("ranges", ranges), ("until", until)):
                    x = wall(fn)
                    if i >= 1:
                        ms[k].append(x)
            info = r.until_info
            assert info["samples_done"] == a.spp
            emit(dict(part="overhead", scene=name, width=w, height=h, spp=a.spp, min_samples=a.min, step_samples=a.step, frames=a.frames, checks=info["checks"],
                      ranges_wall_ms=spread(ms["ranges"]), until_wall_ms=spread(ms["until"]),
                      difference_ms=round(statistics.median(ms["until"]) - statistics.median(ms["ranges"]), 3),
                      per_check_ms=round((statistics.median(ms["until"]) - statistics.median(ms["ranges"])) / info["checks"], 4)))
        if "quality" in parts:
            r.extra_flags = crt.FLAG_BOUNDED_RADIANCE   # (the reference frame: same bits from a ring of samples instead of 12 B per path)
            r.set_spp(a.ref_spp)
            ref = r.run_view(*cam, width=w, height=h, want_mean=False).copy()
            r.extra_flags = 0
            r.set_spp(a.spp)
            r.run_view(*cam, width=w, height=h, want_mean=False)
            emit(dict(part="quality", scene=name, kind="uniform_cap", spp=a.spp, total_ms=r.stats["total_ms"], mse_vs_ref=mse(r.frame_buffer, ref), ref_spp=a.ref_spp))
            for thr in (float(x) for x in a.thresholds.split(",")):
                for frac in (float(x) for x in a.fractions.split(",")):
                    ms = []
                    for i in range(a.frames + 1):
                        r.run_view_until(*cam, min_samples=a.min, step_samples=a.step, threshold=thr, max_above=frac if frac > 0 else 0, want_mean=False,
                                         width=w, height=h)
                        if i >= 1:
                            ms.append(r.until_info["total_ms"])
                    info, e = r.until_info, r.until_info["last"]
                    emit(dict(part="quality", scene=name, kind="until", threshold=thr, fraction=frac, samples_done=info["samples_done"], checks=info["checks"],
                              above=info["above"], total_ms=spread(ms), kernel_ms=info["kernel_ms"], paths=info["paths"], mse_vs_ref=mse(r.frame_buffer, ref),
                              fraction_above=e.fraction_above, rel_rmse=e.rel_rmse, within_2x=e.percentile_ratio(95.0)))
        r.free()
    ev.free()
    if out:
        out.close()


if __name__ == "__main__":
    main()
