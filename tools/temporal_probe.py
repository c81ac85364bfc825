#!/usr/bin/env python3
"""Cost and effect of temporal accumulation (crt_temporal, include/crt.h).

Cost: for each size, the HIP-event time of crt_temporal_device (crt_temporal_info.total_ms: its one kernel on the stream) over --calls
calls after --warmup warm-up calls, on two cornell-box frames of --spp samples one camera step apart, rendered here with their variance
and AOVs; all buffers given (variance, normals, IDs, RGB8 out).  In the same process, the calls taking turns, the a-trous denoiser's
time per pass (crt_denoise_device, 3 iterations, as tools/denoise_probe.py measures it).  Prints the median and best ms per call, the
fraction of pixels that took the history and the rate of the compulsory bytes -- 44 B read per current pixel, 48 B per history pixel,
31 B written -- over the median time.

Effect: at --error-size, spp 8, 8 frames with seeds 100 .. 107, per scene with a static and a moving camera and for each alpha_min of
--alpha-min: the mean squared error of the RGB8 tone map against an spp 256, seed 7 frame of the last camera for the last frame alone,
its variance-guided denoise (crt_denoise_var), the accumulated frame, and the variance-guided denoise of the accumulated frame with
its accumulated variance.

--clamp: the neighbourhood clamp (crt_temporal_clamped).  Cost: at each size the clamped call at radius 1, 2 and 3 (gamma: the
default) takes turns with the unclamped call in the same loop; median ms of each, its ratio to the unclamped median of this run, the
share of pixels clamped and the (2 radius + 1)^2 x 12 cached bytes a pixel's neighbourhood reads.  Effect: the sequences above with the
default alpha_min, for every radius of 1, 2, 3 and gamma of --clamp-gammas: the accumulated error, that of its variance-guided denoise,
and the share of pixels clamped in the last frame; then the setting with the smallest sum over the sequences of clamped / unclamped
accumulated error.

--moments: variance from temporal moments (crt_temporal_moments, crt_variance_estimate).  Cost: at each size, taking turns in one loop,
crt_temporal_clamped_device and crt_temporal_moments_device with the default clamp, the two without a clamp, crt_variance_estimate_device
on what the moments call wrote -- with min_history 1 (every pixel in the temporal branch), the default 4 on a two-frame history (every
pixel in the spatial branch, radius 3) and 2 (the reset pixels only) -- and the denoiser.  Effect: the four sequences, unclamped and
with the default clamp, each accumulated frame under crt_denoise_var fed with (a) the carried variance, (b) the moment estimate with
of_mean 0, (c) with of_mean 1; then the same at one sample per pixel, where only (b) and (c) exist and the comparison is the last frame
under crt_denoise.

--demodulate: albedo demodulation (crt_demodulate / crt_modulate).  Effect only: the four sequences, unclamped and with the default
clamp, accumulated as radiance and as irradiance; per combination the accumulated error and that of its variance-guided filter (with
the filter's sigma_albedo and with +inf), which on irradiance runs before the accumulated frame is modulated.

--specular: dual reprojection (crt_temporal_dual).  Cost: at each size, on veach-mis inputs (a third of the pixels try their virtual
image) and on cornell-box inputs (none does), crt_temporal_dual_device and crt_temporal_clamped_device with the default clamp, and the
two without a clamp, taking turns in one loop; medians, spreads, ratios, the shares of pixels that tried and took V.  Effect: the four
sequences and a fifth, veach-mis with eye and lookat point moving sideways past the plates by (0, 0, 0.5) per frame: the accumulated
error plain / with the default clamp / dual / dual + clamp, the same four under crt_denoise_var, the shares of tried and taken pixels
in the last frame; then min_bounces 0.25 / 0.5 / 1 x radius 1 / 2 on the two moving veach-mis sequences.

One JSON line per figure on stderr, one JSON document on stdout.

  python tools/temporal_probe.py [--sizes 800x600,3840x2160] [--calls 50] [--warmup 5] [--spp 4] [--error-size 160x120] [--alpha-min 0.05,0.1,0.2]
                                 [--clamp] [--clamp-gammas 0.5,1,1.5,2,3,inf] [--moments] [--demodulate] [--specular]
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
from cudaraytracing_amd import hipmem  # noqa: E402

F = np.float32
COMPULSORY_BYTES = 44 + 48 + 31
# per-frame camera moves: (step, the lookat point moves along)
MOVES = {"cornell-box": ((20.0, 0.0, 10.0), True), "veach-mis": ((0.0, 0.1, 0.3), False)}


def camera_at(t, scene, f):
    step, with_lookat = MOVES[scene]
    s = F(f) * np.asarray(step, dtype=F)
    eye = t.eye_pos + s
    return eye, crt.get_inverse_view_matrix(eye, t.lookat + s if with_lookat else t.lookat, t.up), crt.fov_to_radians(t.fov_y)


SPECULAR_PLANES = ("path_depth", "bounces", "last_normal")
# --specular: the fifth sequence, eye and lookat point moving by this per frame (the camera looks down -x: sideways past the plates)
SIDEWAYS = (0.0, 0.0, 0.5)


def render_frame(r, cam, spp, seed, variance=True, specular=False):
    """(the dict crt.temporal takes as `cur`, rgb, {albedo, normal, depth}); variance=False: rendered without the flag (spp 1);
    specular: the dict also has the three planes crt_temporal_dual takes"""
    r.set_spp(spp)
    r.seed = seed
    rgb = r.run_view(*cam, want_variance=variance).copy()
    g = r.run_view_aov(*cam, want=("albedo", "normal", "depth", "material"))
    cur = {"color": r.mean_buffer.copy(), "depth": g["depth"], "normal": g["normal"], "id": g["material"]}
    if variance:
        cur["variance"] = r.variance_buffer.copy()
    if specular:
        cur.update(r.run_view_aov_specular(*cam, want=SPECULAR_PLANES))
    return cur, rgb, {k: g[k] for k in ("albedo", "normal", "depth")}


def cost(a, out):
    scene = "cornell-box"
    t = crt.Task(os.path.join(ROOT, "scenes", scene, "config.json"), base_dir=ROOT)
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        r = crt.Render(crt.Scene.from_task(t, w, h), a.spp, t.P_RR, t.light_sample_n)
        cams = [camera_at(t, scene, f) for f in (0, 1)]
        (c0, _, _), (c1, _, g1) = (render_frame(r, cams[f], a.spp, f) for f in (0, 1))
        r.free()
        prev = dict(c0, history=np.ones((h, w), dtype=F))
        host = {"cur_" + k: v for k, v in c1.items()}
        host.update({"prev_" + k: v for k, v in prev.items()})
        host["albedo"] = g1["albedo"]
        scratch_bytes = crt.denoise_scratch_bytes(w, h)
        dev = hipmem.DeviceBuffers({**host, "out_color": w * h * 12, "out_var": w * h * 12, "out_hist": w * h * 4,
                                    "out_rgb": w * h * 3, "scratch": scratch_bytes})
        ptrs = dev.ptrs

        def call_temporal(clamp=None):
            return crt.temporal_device(w, h, cams[1], {k: ptrs["cur_" + k] for k in c1}, ptrs["out_color"], ptrs["out_hist"],
                                       out_variance_ptr=ptrs["out_var"], out_rgb_ptr=ptrs["out_rgb"], prev_ptrs={k: ptrs["prev_" + k] for k in prev},
                                       prev_camera=cams[0], clamp=clamp)

        def call_denoise():
            return crt.denoise_device(w, h, ptrs["cur_color"], ptrs["out_color"], ptrs["out_rgb"], ptrs["scratch"], scratch_bytes,
                                      albedo_ptr=ptrs["albedo"], normal_ptr=ptrs["cur_normal"], depth_ptr=ptrs["cur_depth"], iterations=3)["total_ms"]

        ms, ms_dn, info = [], [], None
        radii = (1, 2, 3) if a.clamp else ()
        ms_cl, info_cl = {r: [] for r in radii}, {}
        for _ in range(a.warmup + a.calls):
            info = call_temporal()
            ms.append(info["total_ms"])
            for r in radii:
                info_cl[r] = call_temporal({"radius": r})
                ms_cl[r].append(info_cl[r]["total_ms"])
            ms_dn.append(call_denoise())
        ms, ms_dn = ms[a.warmup:], ms_dn[a.warmup:]
        med = statistics.median(ms)
        run = {"width": w, "height": h, "temporal_ms_median": round(med, 4), "temporal_ms_best": round(min(ms), 4),
               "temporal_ms_worst": round(max(ms), 4), "reprojected_fraction": round(info["reprojected"] / (w * h), 4),
               "compulsory_TB_per_s": round(COMPULSORY_BYTES * w * h / (med * 1e-3) / 1e12, 4),
               "denoise_ms_per_pass_median": round(statistics.median(ms_dn) / 3, 4),
               "temporal_over_denoise_pass": round(med / (statistics.median(ms_dn) / 3), 4)}
        out["cost"].append(run)
        print(json.dumps(run), file=sys.stderr, flush=True)
        for r in radii:
            m = statistics.median(ms_cl[r][a.warmup:])
            run = {"width": w, "height": h, "clamp_radius": r, "clamp_gamma": crt.temporal_clamp_defaults()["gamma"], "clamped_ms_median": round(m, 4),
                   "clamped_ms_best": round(min(ms_cl[r][a.warmup:]), 4), "clamped_ms_worst": round(max(ms_cl[r][a.warmup:]), 4),
                   "unclamped_ms_median": round(med, 4), "clamped_over_unclamped": round(m / med, 4),
                   "clamped_fraction": round(info_cl[r]["clamped"] / (w * h), 4), "reprojected_fraction": round(info_cl[r]["reprojected"] / (w * h), 4),
                   "neighbourhood_bytes_per_pixel": (2 * r + 1) ** 2 * 12}
            out["clamp_cost"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
        dev.free()


def mse(x, ref):
    d = x.astype(np.float64) - ref.astype(np.float64)
    return float(np.mean(d * d))


def effect(a, out):
    w, h = (int(v) for v in a.error_size.split("x"))
    for scene in ("cornell-box", "veach-mis"):
        t = crt.Task(os.path.join(ROOT, "scenes", scene, "config.json"), base_dir=ROOT)
        r = crt.Render(crt.Scene.from_task(t, w, h), 8, t.P_RR, t.light_sample_n)
        for moving in (False, True):
            frames = []
            for f in range(8):
                cam = camera_at(t, scene, f if moving else 0)
                frames.append(render_frame(r, cam, 8, 100 + f) + (cam,))
            r.set_spp(256)
            r.seed = 7
            ref = r.run_view(*frames[-1][3]).copy()
            cur, noisy_rgb, g, _ = frames[-1]
            base = {"scene": scene, "camera": "moving" if moving else "static", "width": w, "height": h,
                    "mse_last_frame": round(mse(noisy_rgb, ref), 1),
                    "mse_last_frame_denoise_var": round(mse(crt.denoise_var(cur["color"], cur["variance"], **g)[0], ref), 1)}
            for alpha_min in [float(v) for v in a.alpha_min.split(",")]:
                prev = pcam = None
                for cur, _, g, cam in frames:
                    rgb, color, var, hist, info = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, alpha_min=alpha_min, return_info=True)
                    prev, pcam = dict(cur, color=color, variance=var, history=hist), cam
                run = dict(base, alpha_min=alpha_min, mse_accumulated=round(mse(rgb, ref), 1),
                           mse_accumulated_denoise_var=round(mse(crt.denoise_var(color, var, **g)[0], ref), 1),
                           reprojected_fraction_last=round(info["reprojected"] / (w * h), 4), mean_history=round(float(hist.mean()), 2))
                out["effect"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
            if not a.clamp:
                continue
            for radius in (1, 2, 3):
                for gamma in [float(v) for v in a.clamp_gammas.split(",")]:
                    prev = pcam = None
                    for cur, _, g, cam in frames:
                        rgb, color, var, hist, info = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, return_info=True,
                                                                   clamp={"radius": radius, "gamma": gamma})
                        prev, pcam = dict(cur, color=color, variance=var, history=hist), cam
                    run = dict(base, clamp_radius=radius, clamp_gamma=repr(gamma), mse_accumulated=round(mse(rgb, ref), 1),
                               mse_accumulated_denoise_var=round(mse(crt.denoise_var(color, var, **g)[0], ref), 1),
                               clamped_fraction_last=round(info["clamped"] / (w * h), 4))
                    out["clamp_effect"].append(run)
                    print(json.dumps(run), file=sys.stderr, flush=True)
        r.free()
    if a.clamp:
        # the sum over the sequences of clamped / unclamped accumulated error (the unclamped one: gamma = inf), per setting
        rows = out["clamp_effect"]
        plain = {(x["scene"], x["camera"]): x["mse_accumulated"] for x in rows if x["clamp_gamma"] == "inf" and x["clamp_radius"] == 1}
        sums = {}
        for x in rows:
            key = (x["clamp_radius"], x["clamp_gamma"])
            sums[key] = sums.get(key, 0.0) + x["mse_accumulated"] / plain[(x["scene"], x["camera"])]
        best = min(sums, key=sums.get)
        out["clamp_ratio_sums"] = [{"clamp_radius": k[0], "clamp_gamma": k[1], "ratio_sum": round(v, 3)} for k, v in sorted(sums.items())]
        out["clamp_best"] = {"clamp_radius": best[0], "clamp_gamma": best[1], "ratio_sum": round(sums[best], 3), "defaults": crt.temporal_clamp_defaults()}
        print(json.dumps(out["clamp_best"]), file=sys.stderr, flush=True)


def moments_cost(a, out):
    scene = "cornell-box"
    t = crt.Task(os.path.join(ROOT, "scenes", scene, "config.json"), base_dir=ROOT)
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        r = crt.Render(crt.Scene.from_task(t, w, h), a.spp, t.P_RR, t.light_sample_n)
        cams = [camera_at(t, scene, f) for f in (0, 1)]
        (c0, _, _), (c1, _, g1) = (render_frame(r, cams[f], a.spp, f) for f in (0, 1))
        r.free()
        prev = dict(c0, history=np.ones((h, w), dtype=F))
        host = {"cur_" + k: v for k, v in c1.items()}
        host.update({"prev_" + k: v for k, v in prev.items()})
        host.update({"prev_m1": c0["color"], "prev_m2": (c0["color"] * c0["color"]).astype(F), "albedo": g1["albedo"]})
        scratch_bytes = crt.denoise_scratch_bytes(w, h)
        dev = hipmem.DeviceBuffers({**host, "out_color": w * h * 12, "out_var": w * h * 12, "out_hist": w * h * 4,
                                    "out_rgb": w * h * 3, "out_m1": w * h * 12, "out_m2": w * h * 12,
                                    "out_est": w * h * 12, "scratch": scratch_bytes})
        ptrs = dev.ptrs
        planes = {"m1": ptrs["prev_m1"], "m2": ptrs["prev_m2"], "out_m1": ptrs["out_m1"], "out_m2": ptrs["out_m2"]}

        def call_temporal(clamp, moments):
            return crt.temporal_device(w, h, cams[1], {k: ptrs["cur_" + k] for k in c1}, ptrs["out_color"], ptrs["out_hist"],
                                       out_variance_ptr=ptrs["out_var"], out_rgb_ptr=ptrs["out_rgb"], prev_ptrs={k: ptrs["prev_" + k] for k in prev},
                                       prev_camera=cams[0], clamp=clamp, moments=planes if moments else None)

        def call_estimate(min_history):
            return crt.variance_estimate_device(w, h, ptrs["out_m1"], ptrs["out_m2"], ptrs["out_hist"], ptrs["out_est"], normal_ptr=ptrs["cur_normal"],
                                                depth_ptr=ptrs["cur_depth"], min_history=min_history)

        def call_denoise():
            return crt.denoise_device(w, h, ptrs["cur_color"], ptrs["out_color"], ptrs["out_rgb"], ptrs["scratch"], scratch_bytes,
                                      albedo_ptr=ptrs["albedo"], normal_ptr=ptrs["cur_normal"], depth_ptr=ptrs["cur_depth"], iterations=3)["total_ms"]

        ms = {k: [] for k in ("clamped", "clamped_moments", "plain", "plain_moments", "estimate_temporal", "estimate_spatial", "estimate_mixed", "denoise3")}
        info = {}
        for _ in range(a.warmup + a.calls):
            for key, clamp, moments in (("clamped", True, False), ("clamped_moments", True, True), ("plain", None, False), ("plain_moments", None, True)):
                info[key] = call_temporal(clamp, moments)
                ms[key].append(info[key]["total_ms"])
            for key, m in (("estimate_temporal", 1), ("estimate_spatial", 4), ("estimate_mixed", 2)):     # (after a moments call: its outputs)
                info[key] = call_estimate(m)
                ms[key].append(info[key]["total_ms"])
            ms["denoise3"].append(call_denoise())
        med = {k: statistics.median(v[a.warmup:]) for k, v in ms.items()}
        run = {"width": w, "height": h}
        run.update({k + "_ms_median": round(v, 4) for k, v in med.items()})
        run.update({k + "_ms_best_worst": [round(min(ms[k][a.warmup:]), 4), round(max(ms[k][a.warmup:]), 4)] for k in ("clamped_moments", "plain_moments",
                                                                                                                   "estimate_spatial")})
        pass_ms = med["denoise3"] / 3
        run.update({"clamped_moments_over_clamped": round(med["clamped_moments"] / med["clamped"], 4),
                    "plain_moments_over_plain": round(med["plain_moments"] / med["plain"], 4), "denoise_ms_per_pass_median": round(pass_ms, 4),
                    "estimate_temporal_over_denoise_pass": round(med["estimate_temporal"] / pass_ms, 4),
                    "estimate_spatial_over_denoise_pass": round(med["estimate_spatial"] / pass_ms, 4),
                    "estimate_mixed_over_denoise_pass": round(med["estimate_mixed"] / pass_ms, 4),
                    "reprojected_fraction": round(info["plain_moments"]["reprojected"] / (w * h), 4),
                    "spatial_fraction_temporal_spatial_mixed": [round(info[k]["spatial"] / (w * h), 4) for k in ("estimate_temporal", "estimate_spatial",
                                                                                                                 "estimate_mixed")]})
        out["moments_cost"].append(run)
        print(json.dumps(run), file=sys.stderr, flush=True)
        dev.free()


def moments_effect(a, out):
    w, h = (int(v) for v in a.error_size.split("x"))
    for scene in ("cornell-box", "veach-mis"):
        t = crt.Task(os.path.join(ROOT, "scenes", scene, "config.json"), base_dir=ROOT)
        r = crt.Render(crt.Scene.from_task(t, w, h), 8, t.P_RR, t.light_sample_n)
        for moving in (False, True):
            cams = [camera_at(t, scene, f if moving else 0) for f in range(8)]
            r.set_spp(256)
            r.seed = 7
            ref = r.run_view(*cams[-1]).copy()
            for spp in (8, 1):
                frames = [render_frame(r, cams[f], spp, 100 + f, variance=spp > 1) + (cams[f],) for f in range(8)]
                cur, noisy_rgb, g, _ = frames[-1]
                run = {"scene": scene, "camera": "moving" if moving else "static", "width": w, "height": h, "spp": spp,
                       "mse_last_frame": round(mse(noisy_rgb, ref), 1), "mse_last_frame_denoise": round(mse(crt.denoise(cur["color"], **g)[0], ref), 1)}
                if spp > 1:
                    run["mse_last_frame_denoise_var"] = round(mse(crt.denoise_var(cur["color"], cur["variance"], **g)[0], ref), 1)
                for tag, clamp in (("plain", None), ("clamp", True)):
                    prev = pcam = pm = None
                    for cur, _, g, cam in frames:
                        rgb, color, var, hist, m1, m2 = crt.temporal(cur, cam, prev=prev, prev_camera=pcam, clamp=clamp, moments=pm if prev is not None else True)
                        prev, pcam, pm = dict(cur, color=color, history=hist), cam, {"m1": m1, "m2": m2}
                        if var is not None:
                            prev["variance"] = var
                    run[tag + "_mse_accumulated"] = round(mse(rgb, ref), 1)
                    if var is not None:
                        run[tag + "_mse_denoise_var_carried"] = round(mse(crt.denoise_var(color, var, **g)[0], ref), 1)
                    for of_mean in (0, 1):
                        e, einfo = crt.variance_estimate(m1, m2, hist, normal=g["normal"], depth=g["depth"], of_mean=of_mean, return_info=True)
                        run[tag + "_mse_denoise_var_moments_of_mean%d" % of_mean] = round(mse(crt.denoise_var(color, e, **g)[0], ref), 1)
                    run[tag + "_spatial_last"] = einfo["spatial"]
                out["moments_effect"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
        r.free()


def demodulate_effect(a, out):
    """--demodulate: the four sequences, unclamped and with the default clamp, accumulated as radiance and as irradiance (each frame
    through demodulate with its own shading AOVs, the accumulated frame through modulate with the last frame's): the accumulated
    error and that of its variance-guided filter -- on irradiance, the filter runs before modulate."""
    w, h = (int(v) for v in a.error_size.split("x"))
    for scene in ("cornell-box", "veach-mis"):
        t = crt.Task(os.path.join(ROOT, "scenes", scene, "config.json"), base_dir=ROOT)
        r = crt.Render(crt.Scene.from_task(t, w, h), 8, t.P_RR, t.light_sample_n)
        for moving in (False, True):
            cams = [camera_at(t, scene, f if moving else 0) for f in range(8)]
            r.set_spp(256)
            r.seed = 7
            ref = r.run_view(*cams[-1]).copy()
            frames = []
            for f in range(8):
                cur, rgb, g = render_frame(r, cams[f], 8, 100 + f)
                sh = r.run_view_aov_shading(*cams[f])
                irr, ivar = crt.demodulate(cur["color"], sh["diffuse_albedo"], sh["emission"], cur["variance"])
                frames.append((cur, dict(cur, color=irr, variance=ivar), sh, g, cams[f]))
            run = {"scene": scene, "camera": "moving" if moving else "static", "width": w, "height": h}
            for tag, clamp in (("plain", None), ("clamp", True)):
                for kind in ("radiance", "irradiance"):
                    prev = pcam = None
                    for cur, dcur, sh, g, cam in frames:
                        c = dcur if kind == "irradiance" else cur
                        rgb, color, var, hist = crt.temporal(c, cam, prev=prev, prev_camera=pcam, clamp=clamp)
                        prev, pcam = dict(c, color=color, variance=var, history=hist), cam
                    if kind == "irradiance":
                        E, A = sh["emission"], sh["diffuse_albedo"]
                        rgb = crt.modulate(color, A, E)[0]
                        den = crt.modulate(crt.denoise_var(color, var, want_rgb=False, **g)[1], A, E)[0]
                        den_inf = crt.modulate(crt.denoise_var(color, var, want_rgb=False, sigma_albedo=float("inf"), **g)[1], A, E)[0]
                    else:
                        den = crt.denoise_var(color, var, **g)[0]
                        den_inf = crt.denoise_var(color, var, sigma_albedo=float("inf"), **g)[0]
                    run["%s_%s_mse_accumulated" % (tag, kind)] = round(mse(rgb, ref), 1)
                    run["%s_%s_mse_accumulated_denoise_var" % (tag, kind)] = round(mse(den, ref), 1)
                    run["%s_%s_mse_accumulated_denoise_var_sigma_albedo_inf" % (tag, kind)] = round(mse(den_inf, ref), 1)
            out["demodulate_effect"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
        r.free()


def specular_cost(a, out):
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        for scene in ("veach-mis", "cornell-box"):
            t = crt.Task(os.path.join(ROOT, "scenes", scene, "config.json"), base_dir=ROOT)
            r = crt.Render(crt.Scene.from_task(t, w, h), a.spp, t.P_RR, t.light_sample_n)
            cams = [camera_at(t, scene, f) for f in (0, 1)]
            (c0, _, _), (c1, _, _) = (render_frame(r, cams[f], a.spp, f, specular=True) for f in (0, 1))
            r.free()
            prev = dict(c0, history=np.ones((h, w), dtype=F))
            host = {"cur_" + k: v for k, v in c1.items()}
            host.update({"prev_" + k: v for k, v in prev.items()})
            dev = hipmem.DeviceBuffers({**host, "out_color": w * h * 12, "out_var": w * h * 12, "out_hist": w * h * 4, "out_rgb": w * h * 3})
            ptrs = dev.ptrs

            def call(clamp, dual):
                keep = lambda f, pre: {k: ptrs[pre + k] for k in f if dual or k not in SPECULAR_PLANES}
                return crt.temporal_device(w, h, cams[1], keep(c1, "cur_"), ptrs["out_color"], ptrs["out_hist"], out_variance_ptr=ptrs["out_var"],
                                           out_rgb_ptr=ptrs["out_rgb"], prev_ptrs=keep(prev, "prev_"), prev_camera=cams[0], clamp=clamp, dual=dual)

            kinds = (("clamped", True, None), ("dual_clamped", True, True), ("plain", None, None), ("dual", None, True))
            ms, info = {k: [] for k, _, _ in kinds}, {}
            for _ in range(a.warmup + a.calls):
                for key, clamp, dual in kinds:
                    info[key] = call(clamp, dual)
                    ms[key].append(info[key]["total_ms"])
            run = {"scene": scene, "width": w, "height": h}
            for key, _, _ in kinds:
                v = ms[key][a.warmup:]
                run[key + "_ms_median_best_worst"] = [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]
            med = {k: statistics.median(v[a.warmup:]) for k, v in ms.items()}
            run.update({"dual_clamped_over_clamped": round(med["dual_clamped"] / med["clamped"], 4), "dual_over_plain": round(med["dual"] / med["plain"], 4),
                        "tried_fraction": round(info["dual"]["virtual_tried"] / (w * h), 4), "taken_fraction": round(info["dual"]["virtual_taken"] / (w * h), 4),
                        "reprojected_fraction": round(info["dual"]["reprojected"] / (w * h), 4)})
            out["specular_cost"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
            dev.free()


def specular_effect(a, out):
    w, h = (int(v) for v in a.error_size.split("x"))
    for scene in ("cornell-box", "veach-mis"):
        t = crt.Task(os.path.join(ROOT, "scenes", scene, "config.json"), base_dir=ROOT)
        r = crt.Render(crt.Scene.from_task(t, w, h), 8, t.P_RR, t.light_sample_n)
        for camera in ("static", "moving") + (("sideways",) if scene == "veach-mis" else ()):
            if camera == "sideways":
                cams = []
                for f in range(8):
                    s = F(f) * np.asarray(SIDEWAYS, dtype=F)
                    cams.append((t.eye_pos + s, crt.get_inverse_view_matrix(t.eye_pos + s, t.lookat + s, t.up), crt.fov_to_radians(t.fov_y)))
            else:
                cams = [camera_at(t, scene, f if camera == "moving" else 0) for f in range(8)]
            frames = [render_frame(r, cams[f], 8, 100 + f, specular=True) + (cams[f],) for f in range(8)]
            r.set_spp(256)
            r.seed = 7
            ref = r.run_view(*cams[-1]).copy()
            cur, noisy_rgb, g, _ = frames[-1]
            run = {"scene": scene, "camera": camera, "width": w, "height": h, "mse_last_frame": round(mse(noisy_rgb, ref), 1),
                   "mse_last_frame_denoise_var": round(mse(crt.denoise_var(cur["color"], cur["variance"], **g)[0], ref), 1)}

            def accumulate(clamp, dual):
                prev = pcam = None
                for cur, _, g, cam in frames:
                    c = cur if dual is not None else {k: v for k, v in cur.items() if k not in SPECULAR_PLANES}
                    rgb, color, var, hist, info = crt.temporal(c, cam, prev=prev, prev_camera=pcam, return_info=True, clamp=clamp, dual=dual)
                    prev, pcam = dict(c, color=color, variance=var, history=hist), cam
                return round(mse(rgb, ref), 1), round(mse(crt.denoise_var(color, var, **g)[0], ref), 1), info

            for tag, clamp, dual in (("plain", None, None), ("clamp", True, None), ("dual", None, True), ("dual_clamp", True, True)):
                run[tag + "_mse_accumulated"], run[tag + "_mse_accumulated_denoise_var"], info = accumulate(clamp, dual)
                if dual:
                    run[tag + "_tried_taken_last"] = [round(info["virtual_tried"] / (w * h), 4), round(info["virtual_taken"] / (w * h), 4)]
            out["specular_effect"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
            if scene != "veach-mis" or camera == "static":
                continue
            for min_bounces in (0.25, 0.5, 1.0):
                for radius in (1, 2):
                    row = {"scene": scene, "camera": camera, "min_bounces": min_bounces, "radius": radius}
                    for tag, clamp in (("dual", None), ("dual_clamp", True)):
                        row[tag + "_mse_accumulated"], row[tag + "_mse_accumulated_denoise_var"], info = accumulate(clamp, {"radius": radius, "min_bounces": min_bounces})
                        row[tag + "_tried_taken_last"] = [round(info["virtual_tried"] / (w * h), 4), round(info["virtual_taken"] / (w * h), 4)]
                    out["specular_sweep"].append(row)
                    print(json.dumps(row), file=sys.stderr, flush=True)
        r.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="800x600,3840x2160")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--error-size", default="160x120")
    ap.add_argument("--alpha-min", default="0.05,0.1,0.2")
    ap.add_argument("--clamp", action="store_true")
    ap.add_argument("--clamp-gammas", default="0.5,1,1.5,2,3,inf")
    ap.add_argument("--moments", action="store_true")
    ap.add_argument("--demodulate", action="store_true", help="the sequences accumulated as irradiance beside radiance")
    ap.add_argument("--specular", action="store_true", help="dual reprojection (crt_temporal_dual): its cost beside the clamped call, and the sequences with it")
    ap.add_argument("--skip-cost", action="store_true")
    ap.add_argument("--skip-effect", action="store_true")
    a = ap.parse_args()
    if crt.device_count() < 1:
        raise SystemExit("temporal_probe: no HIP device")
    out = {"calls": a.calls, "warmup": a.warmup, "spp": a.spp, "cost": [], "effect": [], "clamp_cost": [], "clamp_effect": [], "moments_cost": [],
           "moments_effect": []}
    if a.specular:                                           # (its own tables only)
        out.update({"specular_cost": [], "specular_effect": [], "specular_sweep": []})
        if not a.skip_cost:
            specular_cost(a, out)
        if not a.skip_effect:
            specular_effect(a, out)
        print(json.dumps(out), flush=True)
        return
    if a.demodulate:                                         # (its own table only)
        out["demodulate_effect"] = []
        demodulate_effect(a, out)
        print(json.dumps(out), flush=True)
        return
    if a.moments:                                            # (its own tables only: the others are the earlier sections')
        if not a.skip_cost:
            moments_cost(a, out)
        if not a.skip_effect:
            moments_effect(a, out)
        print(json.dumps(out), flush=True)
        return
    if not a.skip_cost:
        cost(a, out)
    if not a.skip_effect:
        effect(a, out)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
