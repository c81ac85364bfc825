"""What adaptive sampling (crt_render_adaptive) costs and buys against the uniform frame, on one GPU, in one process.

For each scene at --width x --height with a cap of --spp samples:
  * the uniform frame (crt_render): HIP-event time of the call (crt_stats.total_ms), paths;
  * the adaptive frame at every --thresholds x --steps (warm-up --min): HIP-event time of the call (crt_adaptive_info.total_ms: every
    pass, the selection kernels and the per-pass synchronisation included), the render kernel's share (kernel_ms), paths, passes, the
    pixels active per pass, ms per million paths of each against the uniform frame's;
  * the RGB8 mean squared error against a uniform frame of --ref-spp samples, for the adaptive frame and for the uniform frame of the
    same number of paths (spp = paths / pixels, rounded).
With --planned the three frames take turns in one process -- per threshold: crt_render_adaptive at the first of --steps, then
crt_render_planned (crt_map_info.total_ms: the warm-up, the plan, the histogram's synchronisation, the list, fold and resolve kernels
included) -- and each planned row also carries the uniform frame of equal TIME (spp = cap x planned ms / uniform ms, rounded), how far
the plan over- or undershoots the iterative call's paths, and the parent's recorded row (PARENT_ROWS: docs/experiments.md, "Adaptive
sampling") beside it.  A last row per scene is crt_render_map with a map of the cap everywhere against crt_render: what the prepare,
list and fold kernels and the synchronisation cost on top of the same paths (total - kernel ms = everything but the render kernel).
Every timed call is warmed up (--warmup calls) and repeated (--repeat); the figure is the median, the spread (min .. max) is printed
beside it.  One JSON line per row on stdout and, with --out, in a file.

    python tools/adaptive_probe.py --out adaptive_probe.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cudaraytracing_amd as crt  # noqa: E402

SCENES = {n: os.path.join(ROOT, "scenes", n, "config.json") for n in ("cornell-box", "veach-mis")}


# (scene, threshold) -> the parent's row at step 64: passes, paths (M), total ms, kernel ms, ms / Mpath x uniform, MSE, and the uniform
# frame of equal paths (spp, ms, MSE); the parent's uniform frames: 72.74 / 140.00 ms, MSE 36.67 / 5.42
PARENT_ROWS = {("cornell-box", 0.1): (9, 93.9, 52.91, 51.01, 1.90, 78.84, (196, 29.60, 91.19)),
               ("cornell-box", 0.05): (9, 158.5, 80.44, 78.02, 1.71, 52.60, (330, 47.93, 57.51)),
               ("cornell-box", 0.02): (9, 172.5, 86.31, 84.08, 1.69, 48.97, (359, 52.21, 53.05)),
               ("veach-mis", 0.1): (9, 41.1, 38.70, 37.53, 1.65, 35.55, (86, 25.27, 33.79)),
               ("veach-mis", 0.05): (9, 98.2, 73.09, 70.88, 1.31, 13.52, (205, 57.22, 14.72)),
               ("veach-mis", 0.02): (9, 221.2, 148.60, 146.27, 1.18, 6.69, (461, 126.39, 6.15))}


def mse(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float((d * d).mean())


def timed(fn, warmup, repeat):
    """fn() -> device ms of one call; (median, min, max) over `repeat` calls after `warmup`"""
    for _ in range(warmup):
        fn()
    ms = [fn() for _ in range(repeat)]
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell-box,veach-mis")
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--min", type=int, default=16)
    ap.add_argument("--steps", default="64")
    ap.add_argument("--thresholds", default="0.1,0.05,0.02")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--planned", action="store_true", help="also crt_render_planned at every threshold, and crt_render_map at the cap")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    w, h = a.width, a.height
    for name in a.scenes.split(","):
        t = crt.Task(SCENES[name], base_dir=ROOT)
        scene = crt.Scene.from_task(t)
        eye, iv, fov = t.eye_pos, crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up), crt.fov_to_radians(t.fov_y)
        r = crt.Render(scene, a.spp, t.P_RR, t.light_sample_n)

        def uniform(spp):
            r.set_spp(spp)
            r.run_view(eye, iv, fov, width=w, height=h, want_mean=False)
            return r.stats["total_ms"]

        r.extra_flags = crt.FLAG_BOUNDED_RADIANCE   # (the reference frame: same bits from a ring of samples instead of 16 B per path)
        uniform(a.ref_spp)
        r.extra_flags = 0
        ref = r.frame_buffer.copy()
        u_ms, u_lo, u_hi = timed(lambda: uniform(a.spp), a.warmup, a.repeat)
        u_paths = w * h * a.spp
        u_rate = u_ms / (u_paths / 1e6)
        emit(dict(scene=name, kind="uniform", width=w, height=h, spp=a.spp, total_ms=u_ms, total_ms_min=u_lo, total_ms_max=u_hi, paths=u_paths,
                  ms_per_mpath=u_rate, mse_vs_ref=mse(r.frame_buffer, ref), ref_spp=a.ref_spp))
        for step in (int(s) for s in a.steps.split(",")):
            for thr in (float(x) for x in a.thresholds.split(",")):
                def adaptive():
                    r.set_spp(a.spp)
                    r.run_view_adaptive(eye, iv, fov, min_samples=a.min, step_samples=step, threshold=thr, width=w, height=h)
                    return r.adaptive_info["total_ms"]

                ms, lo, hi = timed(adaptive, a.warmup, a.repeat)
                info = r.adaptive_info
                frame = r.frame_buffer.copy()
                spp_eq = max(1, int(round(info["paths"] / float(w * h))))
                uniform(spp_eq)
                rate = ms / (info["paths"] / 1e6)
                emit(dict(scene=name, kind="adaptive", threshold=thr, min_samples=a.min, step_samples=step, total_ms=ms, total_ms_min=lo, total_ms_max=hi,
                          kernel_ms=info["kernel_ms"], passes=info["passes"], paths=info["paths"], paths_share=info["paths"] / float(u_paths),
                          ms_per_mpath=rate, ms_per_mpath_vs_uniform=rate / u_rate, time_vs_uniform=ms / u_ms,
                          mse_vs_ref=mse(frame, ref), uniform_equal_paths_spp=spp_eq, uniform_equal_paths_ms=r.stats["total_ms"],
                          uniform_equal_paths_mse=mse(r.frame_buffer, ref), samples_mean=float(r.samples_buffer.mean()),
                          pass_pixels=info["pass_pixels"]))
                if not a.planned or step != int(a.steps.split(",")[0]):
                    continue
                ad_paths, ad_ms, ad_mse = info["paths"], ms, mse(frame, ref)

                def planned():
                    r.set_spp(a.spp)
                    r.run_view_planned(eye, iv, fov, min_samples=a.min, threshold=thr, width=w, height=h)
                    return r.map_info["total_ms"]

                ms, lo, hi = timed(planned, a.warmup, a.repeat)
                info = r.map_info
                frame = r.frame_buffer.copy()
                spp_eq = max(1, int(round(info["paths"] / float(w * h))))
                uniform(spp_eq)
                eq_ms, eq_mse = r.stats["total_ms"], mse(r.frame_buffer, ref)
                spp_t = max(1, min(a.spp, int(round(a.spp * ms / u_ms))))
                uniform(spp_t)
                rate = ms / (info["paths"] / 1e6)
                emit(dict(scene=name, kind="planned", threshold=thr, min_samples=a.min, total_ms=ms, total_ms_min=lo, total_ms_max=hi,
                          kernel_ms=info["kernel_ms"], launches=info["launches"], max_samples=info["max_samples"], paths=info["paths"],
                          paths_share=info["paths"] / float(u_paths), ms_per_mpath=rate, ms_per_mpath_vs_uniform=rate / u_rate,
                          time_vs_uniform=ms / u_ms, mse_vs_ref=mse(frame, ref), uniform_equal_paths_spp=spp_eq, uniform_equal_paths_ms=eq_ms,
                          uniform_equal_paths_mse=eq_mse, uniform_equal_time_spp=spp_t, uniform_equal_time_ms=r.stats["total_ms"],
                          uniform_equal_time_mse=mse(r.frame_buffer, ref), paths_vs_adaptive=info["paths"] / float(ad_paths),
                          time_vs_adaptive=ms / ad_ms, adaptive_mse=ad_mse, samples_mean=float(r.samples_buffer.mean()),
                          parent_row=PARENT_ROWS.get((name, thr))))
        if a.planned:
            full = np.full((h, w), a.spp, dtype=np.uint32)

            def mapped():
                r.set_spp(a.spp)
                r.run_view_map(eye, iv, fov, full, width=w, height=h)
                return r.map_info["total_ms"]

            ms, lo, hi = timed(mapped, a.warmup, a.repeat)
            info = r.map_info
            u2_ms, u2_lo, u2_hi = timed(lambda: uniform(a.spp), a.warmup, a.repeat)
            emit(dict(scene=name, kind="map_at_cap", total_ms=ms, total_ms_min=lo, total_ms_max=hi, kernel_ms=info["kernel_ms"],
                      outside_render_kernel_ms=ms - info["kernel_ms"], launches=info["launches"], paths=info["paths"],
                      uniform_total_ms=u2_ms, uniform_total_ms_min=u2_lo, uniform_total_ms_max=u2_hi, uniform_kernel_ms=r.stats["kernel_ms"],
                      time_vs_uniform=ms / u2_ms))
        r.free()
    if out:
        out.close()


if __name__ == "__main__":
    main()
