#!/usr/bin/env python3
"""Cost of the a-trous denoiser (crt_denoise_device): for each size and iteration count, the HIP-event time of the call
(crt_denoise_info.total_ms: the pack kernel and the filter passes on the stream) over --calls calls after --warmup warm-up calls.
Inputs: a cornell-box frame of --spp samples and its AOVs at that size, rendered here.  Prints ms per call (median and best), ms per
pass (the call's time over its passes: the pack kernel is in it), and the cache-side byte rate -- (25 taps x 40 B + 12 B) per pixel and
pass over the time -- next to the rate of the compulsory 52 B per pixel and pass.  One JSON line per figure on stderr, one JSON document on stdout.
--variance also times the variance-guided form (crt_denoise_var_device, with the frame's crt_variance buffer and the filtered variance
written) in the same run, the two forms' calls taking turns, and prints its figures and the ratio to the plain form.

  python tools/denoise_probe.py [--sizes 800x600,3840x2160] [--iterations 3,5] [--calls 50] [--warmup 5] [--spp 4] [--variance]

--error measures what the filters leave instead of what they cost: per scene (--scenes), a frame of --error-spp samples (seed 0) at
--error-size, filtered by crt_denoise and by crt_denoise_var (their defaults) with the first-hit albedo and with guide_albedo of
crt_render_aov_specular (--bounces) as the albedo guide -- normal and depth first-hit throughout -- and the mean squared error of each
RGB8 result against a frame of --ref-spp samples (seed 999).  --sigma-albedo also lists the error for other values of that one sigma.

  python tools/denoise_probe.py --error [--scenes cornell-box,veach-mis] [--error-size 160x120] [--error-spp 8] [--ref-spp 256]
                                [--bounces 1,2] [--sigma-albedo 0.05,0.1,0.2,0.4]

--demodulate times crt_demodulate_device (with variance) and crt_modulate_device (both outputs) at --sizes beside one filter pass in
the same process; with --error it lists, per scene, albedo guide, --sigma-color and sigma_albedo (default, +inf), the error of both
filters on radiance and on irradiance (demodulate, filter, modulate) against the converged frame of --ref-seed; --sigma-albedo adds
values between the two.  The scene name cornell-box-textured stands for cornell-box with a map_Kd texture on its walls (--cells per
side, scenes/gen_cornell_box.py), generated into a temporary directory.

  python tools/denoise_probe.py --demodulate [--sizes 800x600,3840x2160] [--calls 50] [--warmup 5]
  python tools/denoise_probe.py --error --demodulate [--sigma-color 4,6,8,16] [--ref-seed 7] [--bounces 2]

--nlm times crt_denoise_nlm_device (--nlm-params RADIUS,PATCH,K, default: the filter's) at --sizes beside crt_denoise_var_device's 3
iterations in one process: the variance-guided call and the two forms of the non-local-means kernel (CRT_NLM_FORM=direct|shared, read
per call) taking turns, HIP events, the median of --calls calls.  With --error it lists, per scene, the error of the unfiltered frame,
of crt_denoise, crt_denoise_var and crt_denoise_nlm (their defaults, first-hit guides) at spp 8 and spp 32 against --ref-spp samples of
--ref-seed (give --ref-seed 7 for the frames of docs/experiments.md).

  python tools/denoise_probe.py --nlm [--sizes 800x600,3840x2160] [--calls 50] [--warmup 5] [--nlm-params 5,1,0.7]
  python tools/denoise_probe.py --nlm --error --ref-seed 7

--regress times crt_denoise_regress_device (its defaults or --regress-params RADIUS,PATCH,K,RIDGE; the full mask, the position feature
alone and no feature) at --sizes beside one a-trous pass (crt_denoise_device, 1 iteration) and crt_denoise_nlm_device in one process, the
calls taking turns, HIP events, the median of --calls calls.  With --error it lists, per scene (cornell-box-textured as above) at spp 8
and spp 32, the error of the unfiltered frame, of crt_denoise_var, crt_denoise_nlm and crt_denoise_regress on radiance and on irradiance,
and of the selection among {var, nlm}, {var, nlm, reg} and {var, reg} (Render.run_view_selected, radiance).  --sweep lists the error of
crt_denoise_regress for every combination of the --sweep-* values instead, by its sum relative to crt_denoise_var's defaults.

  python tools/denoise_probe.py --regress [--sizes 800x600,3840x2160] [--calls 50] [--warmup 5] [--regress-params 5,1,0.6,0.4]
  python tools/denoise_probe.py --regress --error --ref-seed 7 --scenes cornell-box,veach-mis,cornell-box-textured
  python tools/denoise_probe.py --regress --error --sweep --ref-seed 7 --scenes cornell-box,veach-mis,cornell-box-textured

--scales times the two operations of the pyramid (crt_pyramid_down_device with every plane; crt_pyramid_merge_device in both forms,
CRT_PYRAMID_FORM=direct|staged, read per call) at --sizes beside one a-trous pass, and, per filter (var, nlm, reg, their defaults), the
single call and the whole chain of denoise_multiscale at 2 and 3 scales made of the *_device calls: all in one process, the calls
taking turns, HIP events (a chain: the sum of its calls' timers), the median of --calls calls.  With --error it lists, per scene
(cornell-box-textured as above) and --error-spps, the error of the unfiltered frame and of var, nlm, reg and nlm at radius 3 at 1 ..
--max-scales scales (denoise_multiscale) against --ref-spp samples of --ref-seed, at --error-size.

  python tools/denoise_probe.py --scales [--sizes 800x600,3840x2160] [--calls 50] [--warmup 5]
  python tools/denoise_probe.py --scales --error --ref-seed 7 --scenes cornell-box,veach-mis,cornell-box-textured
  python tools/denoise_probe.py --scales --error --ref-seed 7 --error-size 800x600 --ref-spp 2048 --error-spps 8 --max-scales 4

--error --split-direct lists, per scene and --error-spps, the error of crt_denoise and crt_denoise_var on the frame beside the same filters
on direct and indirect light separately (Render.run_view_denoised(split_direct=True): crt_render_aov_direct supplies the split), on the
whole frame and on the pixels in shadow.

  python tools/denoise_probe.py --error --split-direct --ref-seed 7 --scenes cornell-box,veach-mis,cornell-box-textured
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cudaraytracing_amd as crt  # noqa: E402
from cudaraytracing_amd import hipmem  # noqa: E402

CACHE_SIDE_BYTES = 25 * 40 + 12   # per pixel and pass: 10 floats per tap, 3 floats written
COMPULSORY_BYTES = 40 + 12


def demodulated_error_table(a):
    """--error --demodulate: per scene, albedo guide, sigma_color and sigma_albedo (the filter's default, +inf), the error of crt_denoise
    and crt_denoise_var on radiance and on irradiance (demodulate, filter, modulate)"""
    import numpy as np
    w, h = (int(v) for v in a.error_size.split("x"))
    out = {"width": w, "height": h, "spp": a.error_spp, "ref_spp": a.ref_spp, "ref_seed": a.ref_seed, "runs": []}
    sigma_albedos = [None] + [float(v) for v in a.sigma_albedo.split(",") if v] + [float("inf")]
    for name in a.scenes.split(","):
        textured = name == "cornell-box-textured"  # cornell-box with a map_Kd texture on its walls, generated here
        t = crt.Task(os.path.join(ROOT, "scenes", "cornell-box" if textured else name, "config.json"), base_dir=ROOT)
        iv = crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up)
        fov = crt.fov_to_radians(t.fov_y)
        if textured:
            import tempfile
            sys.path.insert(0, os.path.join(ROOT, "scenes"))
            import gen_cornell_box
            with tempfile.TemporaryDirectory(prefix="crt_textured_") as d:  # (the loader reads the files in add_obj and keeps nothing of them open)
                obj, mtl_dir, _ = gen_cornell_box.write_textured_variant(d, a.cells)
                scene = crt.Scene(w, h)
                scene.add_obj(obj, mtl_dir)
                scene.set_BVH(t.bvh_thresh_n)
        else:
            scene = crt.Scene.from_task(t, w, h)
        r = crt.Render(scene, a.ref_spp, t.P_RR, t.light_sample_n)
        r.seed = a.ref_seed
        ref = r.run_view(t.eye_pos, iv, fov).astype(np.float64)
        r.seed = 0
        r.set_spp(a.error_spp)
        noisy_rgb = r.run_view(t.eye_pos, iv, fov, want_variance=True).copy()
        mean, var = r.mean_buffer.copy(), r.variance_buffer.copy()
        g = r.run_view_aov_shading(t.eye_pos, iv, fov, first=("albedo", "normal", "depth"))
        E, A = g["emission"], g["diffuse_albedo"]
        guides = {"first-hit": g["albedo"]}
        for mb in [int(v) for v in a.bounces.split(",") if v]:
            guides["guide_albedo, max_bounces %d" % mb] = r.run_view_aov_specular(t.eye_pos, iv, fov, max_bounces=mb, want=("guide_albedo",))["guide_albedo"]
        r.free()
        irr, ivar = crt.demodulate(mean, A, E, var)

        def mse(x):
            return round(float(np.mean((x.astype(np.float64) - ref) ** 2)), 1)

        run = {"scene": name, "unfiltered": mse(noisy_rgb), "rows": []}
        for label, alb in guides.items():
            for sc in [float(v) for v in a.sigma_color.split(",")]:
                for sa in sigma_albedos:
                    k = dict(albedo=alb, normal=g["normal"], depth=g["depth"], sigma_color=sc, sigma_albedo=sa)
                    row = {"albedo_guide": label, "sigma_color": sc, "sigma_albedo": "default" if sa is None else repr(sa),
                           "denoise": mse(crt.denoise(mean, **k)[0]), "denoise_var": mse(crt.denoise_var(mean, var, **k)[0]),
                           "demodulated_denoise": mse(crt.modulate(crt.denoise(irr, want_rgb=False, **k)[1], A, E)[0]),
                           "demodulated_denoise_var": mse(crt.modulate(crt.denoise_var(irr, ivar, want_rgb=False, **k)[1], A, E)[0])}
                    run["rows"].append(row)
                    print(json.dumps(dict(row, scene=name)), file=sys.stderr, flush=True)
        out["runs"].append(run)
    print(json.dumps(out), flush=True)


def modulate_times(a):
    """--demodulate: crt_demodulate_device (with variance) and crt_modulate_device (both outputs) beside ONE filter pass -- the
    difference of crt_denoise_device with two iterations and with one -- the four calls taking turns, on synthetic images.  The byte
    rate is that of the compulsory traffic: 72 B per pixel for demodulate with variance (four planes read, two written), 39 B for
    modulate with both outputs (three read, 12 + 3 B written)."""
    import numpy as np
    out = {"calls": a.calls, "warmup": a.warmup, "runs": []}
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        n = w * h
        rng = np.random.default_rng(1)
        host = {"color": (rng.random((h, w, 3)) * 20).astype(np.float32), "albedo": (rng.random((h, w, 3)) * 0.9 + 0.05).astype(np.float32),
                "emission": np.where(rng.random((h, w, 3)) < 0.05, 100.0, 0.0).astype(np.float32), "variance": rng.random((h, w, 3)).astype(np.float32),
                "normal": rng.random((h, w, 3)).astype(np.float32), "depth": (rng.random((h, w)) + 1).astype(np.float32)}
        scratch_bytes = crt.denoise_scratch_bytes(w, h)
        dev = hipmem.DeviceBuffers({**host, "irr": n * 12, "ivar": n * 12, "out_mean": n * 12, "out_rgb": n * 3,
                                    "scratch": scratch_bytes})
        ptrs = dev.ptrs
        calls = {
            "demodulate": lambda: crt.demodulate_device(w, h, ptrs["color"], ptrs["albedo"], ptrs["irr"], emission_ptr=ptrs["emission"],
                                                        variance_ptr=ptrs["variance"], out_variance_ptr=ptrs["ivar"])["total_ms"],
            "modulate": lambda: crt.modulate_device(w, h, ptrs["irr"], ptrs["albedo"], ptrs["out_mean"], out_rgb_ptr=ptrs["out_rgb"],
                                                    emission_ptr=ptrs["emission"])["total_ms"],
            "denoise_1": lambda: crt.denoise_device(w, h, ptrs["irr"], ptrs["out_mean"], ptrs["out_rgb"], ptrs["scratch"], scratch_bytes, albedo_ptr=ptrs["albedo"],
                                                    normal_ptr=ptrs["normal"], depth_ptr=ptrs["depth"], iterations=1)["total_ms"],
            "denoise_2": lambda: crt.denoise_device(w, h, ptrs["irr"], ptrs["out_mean"], ptrs["out_rgb"], ptrs["scratch"], scratch_bytes, albedo_ptr=ptrs["albedo"],
                                                    normal_ptr=ptrs["normal"], depth_ptr=ptrs["depth"], iterations=2)["total_ms"]}
        ms = {k: [] for k in calls}
        for _ in range(a.warmup + a.calls):
            for k, f in calls.items():
                ms[k].append(f())
        med = {k: statistics.median(v[a.warmup:]) for k, v in ms.items()}
        run = {"width": w, "height": h, "demodulate_ms": round(med["demodulate"], 4), "modulate_ms": round(med["modulate"], 4),
               "denoise_pass_ms": round(med["denoise_2"] - med["denoise_1"], 4), "denoise_1_iteration_ms": round(med["denoise_1"], 4),
               "demodulate_best_ms": round(min(ms["demodulate"][a.warmup:]), 4), "modulate_best_ms": round(min(ms["modulate"][a.warmup:]), 4),
               "demodulate_TB_per_s": round(72 * n / (med["demodulate"] * 1e-3) / 1e12, 3),
               "modulate_TB_per_s": round(39 * n / (med["modulate"] * 1e-3) / 1e12, 3)}
        out["runs"].append(run)
        print(json.dumps(run), file=sys.stderr, flush=True)
        dev.free()
    print(json.dumps(out), flush=True)


def nlm_settings(a):
    if not a.nlm_params:
        return {}
    radius, patch, k = a.nlm_params.split(",")
    return {"radius": int(radius), "patch": int(patch), "k": float(k)}


def nlm_error_table(a):
    """--nlm --error: the four rows of docs/experiments.md, "The non-local-means filter", on the device"""
    import numpy as np
    w, h = (int(v) for v in a.error_size.split("x"))
    out = {"width": w, "height": h, "ref_spp": a.ref_spp, "ref_seed": a.ref_seed, "nlm": nlm_settings(a) or crt.denoise_nlm_defaults(), "rows": []}
    for name in a.scenes.split(","):
        t = crt.Task(os.path.join(ROOT, "scenes", name, "config.json"), base_dir=ROOT)
        iv = crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up)
        fov = crt.fov_to_radians(t.fov_y)
        r = crt.Render(crt.Scene.from_task(t, w, h), a.ref_spp, t.P_RR, t.light_sample_n)
        r.seed = a.ref_seed
        ref = r.run_view(t.eye_pos, iv, fov).astype(np.float64)
        r.seed = 0

        def mse(x):
            return round(float(np.mean((x.astype(np.float64) - ref) ** 2)), 1)

        for spp in (8, 32):
            r.set_spp(spp)
            noisy_rgb = r.run_view(t.eye_pos, iv, fov, want_variance=True).copy()
            mean, var = r.mean_buffer.copy(), r.variance_buffer.copy()
            g = r.run_view_aov(t.eye_pos, iv, fov, want=("albedo", "normal", "depth"))
            row = {"scene": name, "spp": spp, "unfiltered": mse(noisy_rgb), "denoise": mse(crt.denoise(mean, **g)[0]),
                   "denoise_var": mse(crt.denoise_var(mean, var, **g)[0]), "denoise_nlm": mse(crt.denoise_nlm(mean, var, **nlm_settings(a), **g)[0]),
                   "denoise_nlm_no_guides": mse(crt.denoise_nlm(mean, var, **nlm_settings(a))[0])}
            out["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        r.free()
    print(json.dumps(out), flush=True)


def nlm_times(a):
    """--nlm: crt_denoise_var_device (3 iterations) and the two forms of crt_denoise_nlm_device, the three calls taking turns"""
    t = crt.Task(os.path.join(ROOT, "scenes", a.scene, "config.json"), base_dir=ROOT)
    iv = crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up)
    fov = crt.fov_to_radians(t.fov_y)
    out = {"scene": a.scene, "spp": a.spp, "calls": a.calls, "warmup": a.warmup, "nlm": nlm_settings(a) or crt.denoise_nlm_defaults(), "runs": []}
    before = os.environ.get("CRT_NLM_FORM")
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        r = crt.Render(crt.Scene.from_task(t, w, h), a.spp, t.P_RR, t.light_sample_n)
        r.run_view(t.eye_pos, iv, fov, want_variance=True)
        host = dict(r.run_view_aov(t.eye_pos, iv, fov, want=("albedo", "normal", "depth")), color=r.mean_buffer, variance=r.variance_buffer)
        r.free()
        scratch_bytes = max(crt.denoise_scratch_bytes(w, h), crt.denoise_nlm_scratch_bytes(w, h))
        dev = hipmem.DeviceBuffers({**host, "out_mean": w * h * 12, "out_rgb": w * h * 3, "out_var": w * h * 4,
                                    "scratch": scratch_bytes})
        ptrs = dev.ptrs
        common = dict(albedo_ptr=ptrs["albedo"], normal_ptr=ptrs["normal"], depth_ptr=ptrs["depth"])
        args = (w, h, ptrs["color"], ptrs["variance"], ptrs["out_mean"], ptrs["out_rgb"], ptrs["out_var"], ptrs["scratch"], scratch_bytes)

        def call_nlm(form):
            os.environ["CRT_NLM_FORM"] = form
            return crt.denoise_nlm_device(*args, **common, **nlm_settings(a))["total_ms"]

        calls = {"denoise_var_3": lambda: crt.denoise_var_device(*args, iterations=3, **common)["total_ms"],
                 "nlm_direct": lambda: call_nlm("direct"), "nlm_shared": lambda: call_nlm("shared")}
        ms = {k: [] for k in calls}
        for _ in range(a.warmup + a.calls):
            for k, f in calls.items():
                ms[k].append(f())
        run = {"width": w, "height": h}
        for k, v in ms.items():
            run[k + "_ms_median"] = round(statistics.median(v[a.warmup:]), 4)
            run[k + "_ms_best"] = round(min(v[a.warmup:]), 4)
        run["shared_over_direct"] = round(run["nlm_shared_ms_median"] / run["nlm_direct_ms_median"], 4)
        out["runs"].append(run)
        print(json.dumps(run), file=sys.stderr, flush=True)
        dev.free()
    if before is None:
        os.environ.pop("CRT_NLM_FORM", None)
    else:
        os.environ["CRT_NLM_FORM"] = before
    print(json.dumps(out), flush=True)


def regress_settings(a):
    if not a.regress_params:
        return {}
    radius, patch, k, ridge = a.regress_params.split(",")
    return {"radius": int(radius), "patch": int(patch), "k": float(k), "ridge": float(ridge)}


def regress_times(a):
    """--regress: one a-trous pass (crt_denoise_device, 1 iteration), crt_denoise_nlm_device (its default form) and
    crt_denoise_regress_device at the full mask, with the position feature alone and with no feature, the five calls taking turns"""
    t = crt.Task(os.path.join(ROOT, "scenes", a.scene, "config.json"), base_dir=ROOT)
    iv = crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up)
    fov = crt.fov_to_radians(t.fov_y)
    out = {"scene": a.scene, "spp": a.spp, "calls": a.calls, "warmup": a.warmup, "regress": dict(crt.denoise_regress_defaults(), **regress_settings(a)), "runs": []}
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        r = crt.Render(crt.Scene.from_task(t, w, h), a.spp, t.P_RR, t.light_sample_n)
        r.run_view(t.eye_pos, iv, fov, want_variance=True)
        host = dict(r.run_view_aov(t.eye_pos, iv, fov, want=("albedo", "normal", "depth")), color=r.mean_buffer, variance=r.variance_buffer)
        r.free()
        scratch_bytes = max(crt.denoise_scratch_bytes(w, h), crt.denoise_nlm_scratch_bytes(w, h), crt.denoise_regress_scratch_bytes(w, h))
        dev = hipmem.DeviceBuffers({**host, "out_mean": w * h * 12, "out_rgb": w * h * 3, "out_var": w * h * 4, "scratch": scratch_bytes})
        ptrs = dev.ptrs
        common = dict(albedo_ptr=ptrs["albedo"], normal_ptr=ptrs["normal"], depth_ptr=ptrs["depth"])
        args = (w, h, ptrs["color"], ptrs["variance"], ptrs["out_mean"], ptrs["out_rgb"])

        def call_regress(features):
            return crt.denoise_regress_device(*args, ptrs["scratch"], scratch_bytes, features=features, **common, **regress_settings(a))["total_ms"]

        calls = {"atrous_1_pass": lambda: crt.denoise_device(w, h, ptrs["color"], ptrs["out_mean"], ptrs["out_rgb"], ptrs["scratch"], scratch_bytes, iterations=1,
                                                             **common)["total_ms"],
                 "nlm": lambda: crt.denoise_nlm_device(*args, ptrs["out_var"], ptrs["scratch"], scratch_bytes, **common)["total_ms"],
                 "regress_all": lambda: call_regress(15), "regress_position": lambda: call_regress(crt.REGRESS_POSITION), "regress_none": lambda: call_regress(0)}
        ms = {k: [] for k in calls}
        for _ in range(a.warmup + a.calls):
            for k, f in calls.items():
                ms[k].append(f())
        run = {"width": w, "height": h}
        for k, v in ms.items():
            run[k + "_ms_median"] = round(statistics.median(v[a.warmup:]), 4)
            run[k + "_ms_best"] = round(min(v[a.warmup:]), 4)
        run["regress_over_nlm"] = round(run["regress_all_ms_median"] / run["nlm_ms_median"], 3)
        run["regress_over_atrous_pass"] = round(run["regress_all_ms_median"] / run["atrous_1_pass_ms_median"], 3)
        out["runs"].append(run)
        print(json.dumps(run), file=sys.stderr, flush=True)
        dev.free()
    print(json.dumps(out), flush=True)


def regress_error_table(a):
    """--regress --error: per scene (cornell-box-textured as in --demodulate), spp 8 and 32, on radiance and on irradiance: the error of
    the unfiltered frame, of crt_denoise_var, crt_denoise_nlm and crt_denoise_regress (their defaults, or --regress-params), and on radiance
    of the selection among {var, nlm} and among {var, nlm, reg} (Render.run_view_selected), against --ref-spp samples of --ref-seed.
    --sweep instead lists, for every combination of --sweep-* values, the error of crt_denoise_regress on the six radiance frames and
    their sum relative to crt_denoise_var's defaults, the smallest sum first."""
    import itertools
    import numpy as np
    w, h = (int(v) for v in a.error_size.split("x"))
    out = {"width": w, "height": h, "ref_spp": a.ref_spp, "ref_seed": a.ref_seed, "regress": dict(crt.denoise_regress_defaults(), **regress_settings(a)), "rows": []}
    frames = []
    for name in a.scenes.split(","):
        textured = name == "cornell-box-textured"
        t = crt.Task(os.path.join(ROOT, "scenes", "cornell-box" if textured else name, "config.json"), base_dir=ROOT)
        view = (t.eye_pos, crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up), crt.fov_to_radians(t.fov_y))
        if textured:
            import tempfile
            sys.path.insert(0, os.path.join(ROOT, "scenes"))
            import gen_cornell_box
            with tempfile.TemporaryDirectory(prefix="crt_textured_") as d:
                obj, mtl_dir, _ = gen_cornell_box.write_textured_variant(d, a.cells)
                scene = crt.Scene(w, h)
                scene.add_obj(obj, mtl_dir)
                scene.set_BVH(t.bvh_thresh_n)
        else:
            scene = crt.Scene.from_task(t, w, h)
        r = crt.Render(scene, a.ref_spp, t.P_RR, t.light_sample_n)
        r.seed = a.ref_seed
        ref = r.run_view(*view).astype(np.float64)
        r.seed = 0

        def mse(x, ref=ref):
            return round(float(np.mean((x.astype(np.float64) - ref) ** 2)), 1)

        for spp in (8, 32):
            r.set_spp(spp)
            noisy_rgb = r.run_view(*view, want_variance=True).copy()
            mean, var = r.mean_buffer.copy(), r.variance_buffer.copy()
            g = r.run_view_aov_shading(*view, first=("albedo", "normal", "depth"))
            E, A = g["emission"], g["diffuse_albedo"]
            guides = {k: g[k] for k in ("albedo", "normal", "depth")}
            irr, ivar = crt.demodulate(mean, A, E, var)
            frames.append({"scene": name, "spp": spp, "mse": mse, "mean": mean, "var": var, "guides": guides, "irr": irr, "ivar": ivar, "A": A, "E": E,
                           "var_default": mse(crt.denoise_var(mean, var, **guides)[0])})
            if a.sweep:
                continue
            no_albedo = crt.denoise_regress_defaults()["features"] & ~crt.REGRESS_ALBEDO
            row = {"scene": name, "spp": spp, "unfiltered": mse(noisy_rgb), "var": frames[-1]["var_default"], "nlm": mse(crt.denoise_nlm(mean, var, **guides)[0]),
                   "reg": mse(crt.denoise_regress(mean, var, **regress_settings(a), **guides)[0]),
                   "selected_var_nlm": mse(r.run_view_selected(*view, candidates=("var", "nlm"))[0]),
                   "selected_var_nlm_reg": mse(r.run_view_selected(*view, candidates=("var", "nlm", "reg"))[0]),
                   "selected_var_reg": mse(r.run_view_selected(*view, candidates=("var", "reg"))[0]),
                   "demodulated_var": mse(crt.modulate(crt.denoise_var(irr, ivar, want_rgb=False, **guides)[1], A, E)[0]),
                   "demodulated_nlm": mse(crt.modulate(crt.denoise_nlm(irr, ivar, want_rgb=False, **guides)[1], A, E)[0]),
                   "demodulated_reg": mse(crt.modulate(crt.denoise_regress(irr, ivar, want_rgb=False, features=no_albedo, **regress_settings(a), **guides)[1], A, E)[0])}
            info = crt.denoise_regress(mean, var, return_info=True, **regress_settings(a), **guides)[2]
            row["reg_fallback_pixels"] = info["fallback_pixels"]
            out["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        r.free()
    if a.sweep:
        grid = {"radius": [int(v) for v in a.sweep_radius.split(",")], "patch": [int(v) for v in a.sweep_patch.split(",")],
                "k": [float(v) for v in a.sweep_k.split(",")], "ridge": [float(v) for v in a.sweep_ridge.split(",")],
                "sigma_position": [float(v) for v in a.sweep_sigma_position.split(",")], "features": [int(v) for v in a.sweep_features.split(",")]}
        for combo in itertools.product(*grid.values()):
            s = dict(zip(grid.keys(), combo))
            errs = [f["mse"](crt.denoise_regress(f["mean"], f["var"], **s, **f["guides"])[0]) for f in frames]
            rel = sum(e / f["var_default"] for e, f in zip(errs, frames))
            out["rows"].append(dict(s, errors=errs, relative_sum=round(rel, 4)))
        out["rows"].sort(key=lambda row: row["relative_sum"])
        out["frames"] = [{"scene": f["scene"], "spp": f["spp"], "var": f["var_default"]} for f in frames]
        for row in out["rows"][:20]:
            print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


def _probe_scene(name, w, h, cells):
    """(task, view, scene) of a scene name of --scenes; cornell-box-textured is generated into a temporary directory"""
    textured = name == "cornell-box-textured"
    t = crt.Task(os.path.join(ROOT, "scenes", "cornell-box" if textured else name, "config.json"), base_dir=ROOT)
    view = (t.eye_pos, crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up), crt.fov_to_radians(t.fov_y))
    if not textured:
        return t, view, crt.Scene.from_task(t, w, h)
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "scenes"))
    import gen_cornell_box
    with tempfile.TemporaryDirectory(prefix="crt_textured_") as d:  # (the loader reads the files in add_obj and keeps nothing of them open)
        obj, mtl_dir, _ = gen_cornell_box.write_textured_variant(d, cells)
        scene = crt.Scene(w, h)
        scene.add_obj(obj, mtl_dir)
        scene.set_BVH(t.bvh_thresh_n)
    return t, view, scene


SCALE_FILTERS = (("var", "var", {}), ("nlm", "nlm", {}), ("reg", "reg", {}), ("nlm_r3", "nlm", {"radius": 3}))


def scales_error_table(a):
    """--scales --error: per scene and sample count, every filter of SCALE_FILTERS at 1 .. --max-scales scales"""
    import numpy as np
    w, h = (int(v) for v in a.error_size.split("x"))
    out = {"width": w, "height": h, "ref_spp": a.ref_spp, "ref_seed": a.ref_seed, "rows": []}
    for name in a.scenes.split(","):
        t, view, scene = _probe_scene(name, w, h, a.cells)
        r = crt.Render(scene, a.ref_spp, t.P_RR, t.light_sample_n)
        r.seed = a.ref_seed
        ref = r.run_view(*view).astype(np.float64)
        r.seed = 0
        for spp in [int(v) for v in a.error_spps.split(",")]:
            r.set_spp(spp)
            noisy_rgb = r.run_view(*view, want_variance=True).copy()
            mean, var = r.mean_buffer.copy(), r.variance_buffer.copy()
            g = r.run_view_aov(*view, want=("albedo", "normal", "depth"))
            row = {"scene": name, "spp": spp, "unfiltered": round(float(np.mean((noisy_rgb.astype(np.float64) - ref) ** 2)), 1)}
            for label, filt, settings in SCALE_FILTERS:
                row[label] = [round(float(np.mean((crt.denoise_multiscale(mean, var, filter=filt, scales=n, **settings, **g)[0].astype(np.float64) - ref) ** 2)), 1)
                              for n in range(1, a.max_scales + 1)]
            out["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        r.free()
    print(json.dumps(out), flush=True)


def split_direct_error_table(a):
    """--error --split-direct: per scene (cornell-box-textured as in --demodulate) and --error-spps, the error of the unfiltered frame, of
    crt_denoise and crt_denoise_var on the frame, and of the same two with direct and indirect light filtered separately
    (Render.run_view_denoised(split_direct=True)), against --ref-spp samples of --ref-seed at --error-size; and the same errors on the
    shadowed pixels alone -- those whose visibility AOV is below 1 -- where the split has something to keep."""
    import numpy as np
    w, h = (int(v) for v in a.error_size.split("x"))
    out = {"width": w, "height": h, "ref_spp": a.ref_spp, "ref_seed": a.ref_seed, "rows": []}
    for name in a.scenes.split(","):
        t, view, scene = _probe_scene(name, w, h, a.cells)
        r = crt.Render(scene, a.ref_spp, t.P_RR, t.light_sample_n)
        r.seed = a.ref_seed
        ref = r.run_view(*view).astype(np.float64)
        r.seed = 0
        for spp in [int(v) for v in a.error_spps.split(",")]:
            r.set_spp(spp)
            shadowed = r.run_view_aov_direct(*view, want=("visibility",))["visibility"] < 1

            def mse(x, mask=None):
                d = (x.astype(np.float64) - ref) ** 2
                return round(float(np.mean(d if mask is None else d[mask])), 1)

            row = {"scene": name, "spp": spp, "shadowed_pixels": int(shadowed.sum()), "unfiltered": mse(r.run_view(*view))}
            for label, vg in (("atrous", False), ("var", True)):
                whole = r.run_view_denoised(*view, variance_guided=vg)[0]
                split = r.run_view_denoised(*view, variance_guided=vg, split_direct=True)[0]
                row.update({label: mse(whole), label + "_split": mse(split), label + "_shadowed": mse(whole, shadowed), label + "_split_shadowed": mse(split, shadowed)})
            out["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        r.free()
    print(json.dumps(out), flush=True)


def scales_times(a):
    """--scales: the pyramid's two operations, one a-trous pass, and per filter the single call and the chains at 2 and 3 scales"""
    t = crt.Task(os.path.join(ROOT, "scenes", a.scene, "config.json"), base_dir=ROOT)
    view = (t.eye_pos, crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up), crt.fov_to_radians(t.fov_y))
    out = {"scene": a.scene, "spp": a.spp, "calls": a.calls, "warmup": a.warmup, "runs": []}
    before = os.environ.get("CRT_PYRAMID_FORM")
    planes = (("color", 12), ("variance", 12), ("albedo", 12), ("normal", 12), ("depth", 4))
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        r = crt.Render(crt.Scene.from_task(t, w, h), a.spp, t.P_RR, t.light_sample_n)
        r.run_view(*view, want_variance=True)
        host = dict(r.run_view_aov(*view, want=("albedo", "normal", "depth")), color=r.mean_buffer, variance=r.variance_buffer)
        r.free()
        sizes = [(w, h)]
        for _ in range(2):
            sizes.append(crt.pyramid_size(*sizes[-1]))
        scratch_bytes = max(crt.denoise_scratch_bytes(w, h), crt.denoise_nlm_scratch_bytes(w, h), crt.denoise_regress_scratch_bytes(w, h))
        buffers = {n + "0": host[n] for n, _ in planes}
        for k, (lw, lh) in enumerate(sizes):
            if k:
                buffers.update({n + str(k): lw * lh * b for n, b in planes})
            buffers.update({"f%d" % k: lw * lh * 12, "m%d" % k: lw * lh * 12})
        buffers.update(out_rgb=w * h * 3, out_var=w * h * 4, scratch=scratch_bytes)
        dev = hipmem.DeviceBuffers(buffers)
        ptrs = dev.ptrs

        def level(k):
            return {n: ptrs[n + str(k)] for n, _ in planes}

        def down(k):  # level k - 1 -> level k
            return crt.pyramid_down_device(*sizes[k - 1], level(k - 1), level(k))["total_ms"]

        def merge(k, coarse, rgb, form=None):  # f<k> and the coarser result -> m<k>
            if form is None:
                os.environ.pop("CRT_PYRAMID_FORM", None)
            else:
                os.environ["CRT_PYRAMID_FORM"] = form
            return crt.pyramid_merge_device(*sizes[k], ptrs["f%d" % k], coarse, ptrs["m%d" % k], ptrs["out_rgb"] if rgb else None)["total_ms"]

        def filt(name, k, rgb):  # level k -> f<k>
            lw, lh = sizes[k]
            p = level(k)
            guides = dict(albedo_ptr=p["albedo"], normal_ptr=p["normal"], depth_ptr=p["depth"])
            rgb_ptr = ptrs["out_rgb"] if rgb else None
            if name == "reg":
                return crt.denoise_regress_device(lw, lh, p["color"], p["variance"], ptrs["f%d" % k], rgb_ptr, ptrs["scratch"], scratch_bytes, **guides)["total_ms"]
            call = crt.denoise_var_device if name == "var" else crt.denoise_nlm_device
            return call(lw, lh, p["color"], p["variance"], ptrs["f%d" % k], rgb_ptr, None, ptrs["scratch"], scratch_bytes, **guides)["total_ms"]

        def chain(name, scales):
            ms = sum(down(k) for k in range(1, scales))
            result = None
            for k in range(scales - 1, -1, -1):
                ms += filt(name, k, rgb=scales == 1)
                if result is None:
                    result = ptrs["f%d" % k]
                else:
                    ms += merge(k, result, rgb=k == 0)
                    result = ptrs["m%d" % k]
            return ms

        down(1)  # (level 1 holds a reduced frame for the merges timed alone)
        calls = {"atrous_1": lambda: crt.denoise_device(w, h, ptrs["color0"], ptrs["f0"], ptrs["out_rgb"], ptrs["scratch"], scratch_bytes, albedo_ptr=ptrs["albedo0"],
                                                        normal_ptr=ptrs["normal0"], depth_ptr=ptrs["depth0"], iterations=1)["total_ms"],
                 "pyramid_down": lambda: down(1),
                 "pyramid_merge_direct": lambda: merge(0, ptrs["color1"], True, "direct"),
                 "pyramid_merge_staged": lambda: merge(0, ptrs["color1"], True, "staged")}
        for name in ("var", "nlm", "reg"):
            for scales in (1, 2, 3):
                calls["%s_%d" % (name, scales)] = lambda name=name, scales=scales: chain(name, scales)
        ms = {k: [] for k in calls}
        for _ in range(a.warmup + a.calls):
            for k, f in calls.items():
                ms[k].append(f())
        run = {"width": w, "height": h}
        for k, v in ms.items():
            run[k + "_ms_median"] = round(statistics.median(v[a.warmup:]), 4)
            run[k + "_ms_best"] = round(min(v[a.warmup:]), 4)
        run["staged_over_direct"] = round(run["pyramid_merge_staged_ms_median"] / run["pyramid_merge_direct_ms_median"], 4)
        for name in ("var", "nlm", "reg"):
            for scales in (2, 3):
                run["%s_%d_over_1" % (name, scales)] = round(run["%s_%d_ms_median" % (name, scales)] / run[name + "_1_ms_median"], 4)
        out["runs"].append(run)
        print(json.dumps(run), file=sys.stderr, flush=True)
        dev.free()
    if before is None:
        os.environ.pop("CRT_PYRAMID_FORM", None)
    else:
        os.environ["CRT_PYRAMID_FORM"] = before
    print(json.dumps(out), flush=True)


def error_table(a):
    import numpy as np
    w, h = (int(v) for v in a.error_size.split("x"))
    out = {"width": w, "height": h, "spp": a.error_spp, "ref_spp": a.ref_spp, "runs": []}
    sigmas = [None] + [float(v) for v in a.sigma_albedo.split(",") if v]
    for name in a.scenes.split(","):
        t = crt.Task(os.path.join(ROOT, "scenes", name, "config.json"), base_dir=ROOT)
        iv = crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up)
        fov = crt.fov_to_radians(t.fov_y)
        r = crt.Render(crt.Scene.from_task(t, w, h), a.ref_spp, t.P_RR, t.light_sample_n)
        r.seed = 999
        ref = r.run_view(t.eye_pos, iv, fov).astype(np.float64)
        r.seed = 0
        r.set_spp(a.error_spp)
        noisy_rgb = r.run_view(t.eye_pos, iv, fov, want_variance=True).copy()
        mean, var = r.mean_buffer.copy(), r.variance_buffer.copy()
        g = r.run_view_aov(t.eye_pos, iv, fov, want=("albedo", "normal", "depth"))
        guides = {"first-hit": g["albedo"]}
        for mb in [int(v) for v in a.bounces.split(",")]:
            guides["guide_albedo, max_bounces %d" % mb] = r.run_view_aov_specular(t.eye_pos, iv, fov, max_bounces=mb, want=("guide_albedo",))["guide_albedo"]
        r.free()

        def mse(x):
            return round(float(np.mean((x.astype(np.float64) - ref) ** 2)), 1)

        run = {"scene": name, "unfiltered": mse(noisy_rgb), "rows": []}
        for label, alb in guides.items():
            for sa in sigmas:
                row = {"albedo_guide": label, "sigma_albedo": sa,
                       "denoise": mse(crt.denoise(mean, albedo=alb, normal=g["normal"], depth=g["depth"], sigma_albedo=sa)[0]),
                       "denoise_var": mse(crt.denoise_var(mean, var, albedo=alb, normal=g["normal"], depth=g["depth"], sigma_albedo=sa)[0])}
                run["rows"].append(row)
                print(json.dumps(dict(row, scene=name)), file=sys.stderr, flush=True)
        out["runs"].append(run)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="800x600,3840x2160")
    ap.add_argument("--iterations", default="3,5")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--scene", default="cornell-box")
    ap.add_argument("--variance", action="store_true", help="time crt_denoise_var_device beside crt_denoise_device")
    ap.add_argument("--error", action="store_true", help="the error the filters leave, with the first-hit and the specular albedo guide")
    ap.add_argument("--scenes", default="cornell-box,veach-mis")
    ap.add_argument("--error-size", default="160x120")
    ap.add_argument("--error-spp", type=int, default=8)
    ap.add_argument("--ref-spp", type=int, default=256)
    ap.add_argument("--bounces", default="1,2")
    ap.add_argument("--sigma-albedo", default="")
    ap.add_argument("--demodulate", action="store_true", help="time crt_demodulate_device / crt_modulate_device beside one filter pass; with --error: the filters on irradiance")
    ap.add_argument("--sigma-color", default="4,6,8,16", help="--error --demodulate: the colour sigmas of the table")
    ap.add_argument("--cells", type=int, default=12, help="--error --demodulate with the scene cornell-box-textured: cells per wall side")
    ap.add_argument("--ref-seed", type=int, default=999, help="--error --demodulate: the seed of the converged frame")
    ap.add_argument("--nlm", action="store_true", help="time crt_denoise_nlm_device (both forms) beside crt_denoise_var_device; with --error: the error rows at spp 8 and 32")
    ap.add_argument("--nlm-params", default="", help="--nlm: RADIUS,PATCH,K instead of the filter's defaults")
    ap.add_argument("--regress", action="store_true", help="time crt_denoise_regress_device beside crt_denoise_nlm_device and one a-trous pass; with --error: the error rows")
    ap.add_argument("--regress-params", default="", help="--regress: RADIUS,PATCH,K,RIDGE instead of the filter's defaults")
    ap.add_argument("--sweep", action="store_true", help="--regress --error: the error for every combination of the --sweep-* values")
    ap.add_argument("--sweep-radius", default="3,5,7")
    ap.add_argument("--sweep-patch", default="1,2")
    ap.add_argument("--sweep-k", default="0.5,0.7,1.0")
    ap.add_argument("--sweep-ridge", default="0.001,0.01,0.1")
    ap.add_argument("--sweep-sigma-position", default="0.5,1,2")
    ap.add_argument("--sweep-features", default="15,13,12,8,7", help="masks of the REGRESS_* bits (normal 1, albedo 2, depth 4, position 8)")
    ap.add_argument("--scales", action="store_true", help="time crt_pyramid_down_device / crt_pyramid_merge_device and the multi-scale chains; with --error: the error rows")
    ap.add_argument("--max-scales", type=int, default=3, help="--scales --error: the most scales of a row (1 .. 4)")
    ap.add_argument("--error-spps", default="8,32", help="--scales --error: the sample counts of the rows")
    ap.add_argument("--split-direct", action="store_true", help="--error: direct and indirect light filtered separately beside the unsplit filters")
    a = ap.parse_args()
    if crt.device_count() < 1:
        raise SystemExit("denoise_probe: no HIP device")
    if a.error and a.split_direct:
        return split_direct_error_table(a)
    if a.scales:
        return scales_error_table(a) if a.error else scales_times(a)
    if a.regress:
        return regress_error_table(a) if a.error else regress_times(a)
    if a.error:
        return nlm_error_table(a) if a.nlm else demodulated_error_table(a) if a.demodulate else error_table(a)
    if a.nlm:
        return nlm_times(a)
    if a.demodulate:
        return modulate_times(a)
    t = crt.Task(os.path.join(ROOT, "scenes", a.scene, "config.json"), base_dir=ROOT)
    iv = crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up)
    fov = crt.fov_to_radians(t.fov_y)
    out = {"scene": a.scene, "spp": a.spp, "calls": a.calls, "warmup": a.warmup, "runs": []}
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        r = crt.Render(crt.Scene.from_task(t, w, h), a.spp, t.P_RR, t.light_sample_n)
        r.run_view(t.eye_pos, iv, fov, want_variance=a.variance)
        host = dict(r.run_view_aov(t.eye_pos, iv, fov, want=("albedo", "normal", "depth")), color=r.mean_buffer)
        if a.variance:
            host["variance"] = r.variance_buffer
        r.free()
        scratch_bytes = crt.denoise_scratch_bytes(w, h)
        dev = hipmem.DeviceBuffers({**host, "out_mean": w * h * 12, "out_rgb": w * h * 3, "out_var": w * h * 4,
                                    "scratch": scratch_bytes})
        ptrs = dev.ptrs

        def call(iterations):
            return crt.denoise_device(w, h, ptrs["color"], ptrs["out_mean"], ptrs["out_rgb"], ptrs["scratch"], scratch_bytes,
                                      albedo_ptr=ptrs["albedo"], normal_ptr=ptrs["normal"], depth_ptr=ptrs["depth"],
                                      iterations=iterations)["total_ms"]

        def call_var(iterations):
            return crt.denoise_var_device(w, h, ptrs["color"], ptrs["variance"], ptrs["out_mean"], ptrs["out_rgb"], ptrs["out_var"], ptrs["scratch"],
                                          scratch_bytes, albedo_ptr=ptrs["albedo"], normal_ptr=ptrs["normal"], depth_ptr=ptrs["depth"],
                                          iterations=iterations)["total_ms"]

        for it in [int(v) for v in a.iterations.split(",")]:
            ms, ms_var = [], []
            for _ in range(a.warmup + a.calls):
                ms.append(call(it))
                if a.variance:
                    ms_var.append(call_var(it))
            ms, ms_var = ms[a.warmup:], ms_var[a.warmup:]
            med, best = statistics.median(ms), min(ms)
            per_pass = med / it
            run = {"width": w, "height": h, "iterations": it, "ms_per_call_median": round(med, 4), "ms_per_call_best": round(best, 4),
                   "ms_per_pass": round(per_pass, 4),
                   "cache_side_TB_per_s": round(CACHE_SIDE_BYTES * w * h / (per_pass * 1e-3) / 1e12, 3),
                   "compulsory_TB_per_s": round(COMPULSORY_BYTES * w * h / (per_pass * 1e-3) / 1e12, 4)}
            if a.variance:
                med_var = statistics.median(ms_var)
                run.update({"var_ms_per_call_median": round(med_var, 4), "var_ms_per_call_best": round(min(ms_var), 4),
                            "var_ms_per_pass": round(med_var / it, 4), "var_over_plain": round(med_var / med, 4)})
            out["runs"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
        dev.free()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
