#!/usr/bin/env python3
"""Cost and effect of guide-driven upsampling (crt_upsample, include/crt.h; Render.run_view_upsampled).

Cost: for each size pair of --pairs, the HIP-event time of crt_upsample_device (crt_upsample_info.total_ms: its one kernel on the
stream, with the counter of fallback pixels) over --calls calls after --warmup warm-up calls, on a cornell-box frame of --spp samples
rendered here at the low size with its variance and AOVs and the AOVs at the full size; all guides, the variance and all three outputs.
In the same process, the calls taking turns, the a-trous denoiser's time per pass at the full size (crt_denoise_device, 3 iterations, as
tools/denoise_probe.py measures it).  Prints the median, best and worst ms per call, the medians of the two halves of the calls (the
spread of one form: what a difference has to exceed), the fallback share and the rate of the compulsory bytes -- 28 B of guides read
and 27 B written per output pixel, 52 B read per low-resolution pixel -- over the median time.  (The A/B against a form that stages the
low-resolution tile in LDS is tools/upsample_ab.hip.)

Effect: at --size and --spp-full samples, per scene (the two shipped ones and cornell-box-textured: cornell-box with a map_Kd texture on
its walls, scenes/gen_cornell_box.py, --cells per side, generated into a temporary directory), the mean squared error of the RGB8 tone
map against a --ref-spp, --ref-seed frame at the full size, and the device time -- the path kernel's, the AOV passes' and the filters'
own timers added up; demodulate / modulate and the host copies in between are not in it -- of
  (a) the full-resolution frame at --spp-full;
  (b) run_view_upsampled at --factor and --spp-full, with and without filter_low, with guide_spp --spp-full and --guide-spp, and
      with demodulate=False;
  (c) the full-resolution frame at --spp-full / factor^2 -- the paths of (b) -- filtered with crt_denoise_var (plain and demodulated).
Sweep: (b) unfiltered with radius 1 and 2 and sigma_albedo of --sigma-albedo, per scene.

One JSON line per figure on stderr, one JSON document on stdout.

  python tools/upsample_probe.py [--pairs 800x600:400x300,3840x2160:1920x1080,3840x2160:960x540] [--calls 50] [--warmup 5] [--spp 4]
                                 [--size 800x600] [--factor 2] [--spp-full 64] [--guide-spp 4] [--ref-spp 2048] [--ref-seed 7] [--cells 12]
                                 [--sigma-albedo 0.05,0.1,0.2,inf] [--skip-cost] [--skip-effect]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cudaraytracing_amd as crt  # noqa: E402
from cudaraytracing_amd import hipmem  # noqa: E402

F = np.float32
GUIDES = ("albedo", "normal", "depth")
OUT_BYTES, GUIDE_BYTES, LOW_BYTES = 27, 28, 52


def cost(a, out):
    scene = "cornell-box"
    t = crt.Task(os.path.join(ROOT, "scenes", scene, "config.json"), base_dir=ROOT)
    cam = (t.eye_pos, crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up), crt.fov_to_radians(t.fov_y))
    for pair in a.pairs.split(","):
        (w, h), (lw, lh) = (tuple(int(v) for v in s.split("x")) for s in pair.split(":"))
        r = crt.Render(crt.Scene.from_task(t, w, h), a.spp, t.P_RR, t.light_sample_n)
        r.run_view(*cam, width=lw, height=lh, want_variance=True)
        low = dict(r.run_view_aov(*cam, want=GUIDES, width=lw, height=lh), color=r.mean_buffer.copy(), variance=r.variance_buffer.copy())
        full = r.run_view_aov(*cam, want=GUIDES)
        r.free()
        host = {"low_" + k: v for k, v in low.items()}
        host.update({"full_" + k: v for k, v in full.items()})
        host["full_color"] = np.zeros((h, w, 3), dtype=F)  # what the denoiser pass filters: its time does not depend on the values
        scratch_bytes = crt.denoise_scratch_bytes(w, h)
        dev = hipmem.DeviceBuffers({**host, "out_color": w * h * 12, "out_var": w * h * 12, "out_rgb": w * h * 3,
                                    "scratch": scratch_bytes})
        ptrs = dev.ptrs

        def call_upsample(radius):
            return crt.upsample_device(w, h, lw, lh, {k: ptrs["low_" + k] for k in low}, ptrs["out_color"], out_variance_ptr=ptrs["out_var"],
                                       out_rgb_ptr=ptrs["out_rgb"], guide_ptrs={k: ptrs["full_" + k] for k in GUIDES}, radius=radius)

        def call_denoise():
            return crt.denoise_device(w, h, ptrs["full_color"], ptrs["out_color"], ptrs["out_rgb"], ptrs["scratch"], scratch_bytes,
                                      albedo_ptr=ptrs["full_albedo"], normal_ptr=ptrs["full_normal"], depth_ptr=ptrs["full_depth"], iterations=3)["total_ms"]

        radii = (1, 2)
        ms, ms_dn, info = {k: [] for k in radii}, [], {}
        for _ in range(a.warmup + a.calls):
            for k in radii:
                info[k] = call_upsample(k)
                ms[k].append(info[k]["total_ms"])
            ms_dn.append(call_denoise())
        ms_dn = ms_dn[a.warmup:]
        dn_pass = statistics.median(ms_dn) / 3
        for k in radii:
            m = ms[k][a.warmup:]
            med = statistics.median(m)
            run = {"width": w, "height": h, "low_width": lw, "low_height": lh, "radius": k, "upsample_ms_median": round(med, 4),
                   "upsample_ms_best": round(min(m), 4), "upsample_ms_worst": round(max(m), 4),
                   "upsample_ms_halves": [round(statistics.median(m[:len(m) // 2]), 4), round(statistics.median(m[len(m) // 2:]), 4)],
                   "fallback_fraction": round(info[k]["fallback_pixels"] / (w * h), 5),
                   "compulsory_bytes_per_output_pixel": round(OUT_BYTES + GUIDE_BYTES + LOW_BYTES * lw * lh / (w * h), 2),
                   "compulsory_TB_per_s": round(((OUT_BYTES + GUIDE_BYTES) * w * h + LOW_BYTES * lw * lh) / (med * 1e-3) / 1e12, 4),
                   "denoise_ms_per_pass_median": round(dn_pass, 4), "upsample_over_denoise_pass": round(med / dn_pass, 4)}
            out["cost"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
        dev.free()


def mse(x, ref):
    d = x.astype(np.float64) - ref.astype(np.float64)
    return float(np.mean(d * d))


def load_scene(name, w, h, cells):
    """(task, Scene) of a shipped scene or of cornell-box-textured"""
    textured = name == "cornell-box-textured"
    t = crt.Task(os.path.join(ROOT, "scenes", "cornell-box" if textured else name, "config.json"), base_dir=ROOT)
    if not textured:
        return t, crt.Scene.from_task(t, w, h)
    sys.path.insert(0, os.path.join(ROOT, "scenes"))
    import gen_cornell_box
    with tempfile.TemporaryDirectory(prefix="crt_textured_") as d:  # (the loader reads the files in add_obj and keeps nothing of them open)
        obj, mtl_dir, _ = gen_cornell_box.write_textured_variant(d, cells)
        scene = crt.Scene(w, h)
        scene.add_obj(obj, mtl_dir)
        scene.set_BVH(t.bvh_thresh_n)
    return t, scene


def effect(a, out):
    w, h = (int(v) for v in a.size.split("x"))
    f = a.factor
    for name in a.scenes.split(","):
        t, scene = load_scene(name, w, h, a.cells)
        cam = (t.eye_pos, crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up), crt.fov_to_radians(t.fov_y))
        r = crt.Render(scene, a.spp_full, t.P_RR, t.light_sample_n)
        r.set_spp(a.ref_spp)
        r.seed = a.ref_seed
        ref = r.run_view(*cam).copy()
        r.seed = 0

        def row(kind, rgb, render_ms, aov_ms, filter_ms, **more):
            run = dict({"scene": name, "width": w, "height": h, "kind": kind, "mse": round(mse(rgb, ref), 2), "render_ms": round(render_ms, 3),
                        "aov_ms": round(aov_ms, 3), "filter_ms": round(filter_ms, 3), "device_ms": round(render_ms + aov_ms + filter_ms, 3)}, **more)
            out["effect"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
            return run

        # (a) the full-resolution frame
        r.set_spp(a.spp_full)
        rgb = r.run_view(*cam).copy()
        row("full spp %d" % a.spp_full, rgb, r.stats["total_ms"], 0.0, 0.0)

        # (c) the paths of (b) at full resolution, filtered
        spp_c = max(2, a.spp_full // (f * f))
        r.set_spp(spp_c)
        for demodulate in (False, True):
            rgb, _ = r.run_view_denoised(*cam, variance_guided=True, demodulate=demodulate)
            row("full spp %d + denoise_var%s" % (spp_c, ", demodulated" if demodulate else ""), rgb, r.stats["total_ms"], r.aov_info["total_ms"],
                r.denoise_info["total_ms"])
        row("full spp %d" % spp_c, r.frame_buffer, r.stats["total_ms"], 0.0, 0.0)

        # (b) the upsampled frame: the timers of its stages are read from the same calls made one by one
        r.set_spp(a.spp_full)
        r.run_view(*cam, width=w // f, height=h // f, want_variance=True)
        low_ms = r.stats["total_ms"]
        r.run_view_aov_shading(*cam, first=GUIDES, width=w // f, height=h // f)
        low_aov_ms = r.aov_info["total_ms"]
        aov_ms = {}
        for g in sorted({a.spp_full, a.guide_spp}):
            r.set_spp(g)
            r.run_view_aov_shading(*cam, first=GUIDES)
            aov_ms[g] = r.aov_info["total_ms"]
        r.set_spp(a.spp_full)
        for demodulate, filter_low, g in ((True, False, a.spp_full), (True, False, a.guide_spp), (True, True, a.spp_full), (True, True, a.guide_spp),
                                          (False, False, a.spp_full)):
            rgb, _ = r.run_view_upsampled(*cam, factor=f, guide_spp=g, demodulate=demodulate, filter_low=filter_low)
            dn_ms = 0.0
            if filter_low:  # the same filter call by hand, for its timer
                lo = r.low_frame
                c, v = (crt.demodulate(lo["mean"], lo["diffuse_albedo"], lo["emission"], variance=lo["variance"]) if demodulate else (lo["mean"], lo["variance"]))
                dn_ms = crt.denoise_var(c, v, want_rgb=False, return_info=True, **{k: lo[k] for k in GUIDES})[2]["total_ms"]
            row("upsampled x%d spp %d, guide spp %d%s%s" % (f, a.spp_full, g, ", filtered low frame" if filter_low else "", "" if demodulate else ", radiance"),
                rgb, low_ms, low_aov_ms + aov_ms[g], r.upsample_info["total_ms"] + dn_ms, fallback_fraction=round(r.upsample_info["fallback_pixels"] / (w * h), 5))

        # the sweep: radius and sigma_albedo, unfiltered, guides at the frame's sample count
        for radius in (1, 2):
            for sa in [float(v) for v in a.sigma_albedo.split(",")]:
                rgb, _ = r.run_view_upsampled(*cam, factor=f, radius=radius, sigma_albedo=sa)
                run = {"scene": name, "factor": f, "radius": radius, "sigma_albedo": sa, "mse": round(mse(rgb, ref), 2),
                       "fallback_fraction": round(r.upsample_info["fallback_pixels"] / (w * h), 5), "upsample_ms": round(r.upsample_info["total_ms"], 4)}
                out["sweep"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
        r.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="800x600:400x300,3840x2160:1920x1080,3840x2160:960x540")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--size", default="800x600")
    ap.add_argument("--scenes", default="cornell-box,veach-mis,cornell-box-textured")
    ap.add_argument("--factor", type=int, default=2)
    ap.add_argument("--spp-full", type=int, default=64)
    ap.add_argument("--guide-spp", type=int, default=4)
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--ref-seed", type=int, default=7)
    ap.add_argument("--cells", type=int, default=12)
    ap.add_argument("--sigma-albedo", default="0.05,0.1,0.2,inf")
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-effect", action="store_true")
    a = ap.parse_args()
    if crt.device_count() < 1:
        raise SystemExit("upsample_probe: no HIP device")
    out = {"calls": a.calls, "warmup": a.warmup, "spp": a.spp, "cost": [], "effect": [], "sweep": []}
    if not a.skip_cost:
        cost(a, out)
    if not a.skip_effect:
        effect(a, out)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
