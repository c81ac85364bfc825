#!/usr/bin/env python3
"""Cost and effect of the half buffers and of error-estimated filter selection (CRT_FLAG_HALF_BUFFERS, crt_half_buffers,
crt_filter_select, include/crt.h; Render.run_view_selected).  Three parts, one per invocation, so that each runs under a time limit of
its own:

  --part time    per size of --sizes: the HIP-event time of crt_filter_select_device (its two kernels on the stream, with the counters)
                 with K = 2 (var, nlm) and K = 4 (none, atrous, var, nlm) at the default radii, and of ONE a-trous pass
                 (crt_denoise_device, iterations 1), taking turns in one process: --calls calls after --warmup, on a cornell-box frame of
                 --spp samples rendered here with its halves, variance and guides.  Median, best, worst, the medians of the two halves
                 of the calls, and the compulsory bytes per pixel (36 B of halves and variance and 24 B per candidate read, 20 B written)
                 over the median time.
  --part flag    the --flag-size frame at --flag-spp samples with CRT_FLAG_HALF_BUFFERS, with CRT_FLAG_VARIANCE and with neither, taking
                 turns in one process (tools/variance_probe.py's method): crt_stats' total_ms, kernel_ms and their difference, which is
                 k_order_items plus the accumulate kernel, the only kernel the flags change; and the time of crt_half_buffers_device.
  --part effect  per scene and spp of --effect-spp at --effect-size: the mean squared error of the RGB8 tone map against a frame of
                 --ref-spp samples of --ref-seed of: the noisy frame; crt_denoise_var and crt_denoise_nlm of the full frame; the
                 selection among {var, nlm} and among {none, var, nlm}; and the same selections made with the TRUE error -- per pixel and
                 candidate the squared difference of the candidate's mean of its two half results to the reference's mean, averaged
                 over the channels, smoothed over the same window, blended the same way: what a perfect estimate would reach with these
                 candidates.  With --sweep also the selection among {var, nlm} for (error_radius, blend_radius) in {1, 3, 5} x {0, 1, 2}.

One JSON line per figure on stderr, one JSON document on stdout.

  python tools/select_probe.py --part time [--sizes 800x600,3840x2160] [--calls 50] [--warmup 5] [--spp 2]
  python tools/select_probe.py --part flag [--flag-size 800x600] [--flag-spp 512] [--frames 5]
  python tools/select_probe.py --part effect [--scenes cornell-box,veach-mis] [--effect-size 160x120] [--effect-spp 8,32] [--ref-spp 256]
                                             [--ref-seed 7] [--sweep]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cudaraytracing_amd as crt  # noqa: E402
from cudaraytracing_amd import _capi as capi  # noqa: E402
from cudaraytracing_amd import hipmem  # noqa: E402
from cudaraytracing_amd.api import _select_candidate as candidate  # noqa: E402  (run_view_selected's: name, half, half variance, guides, device)

F = np.float32
GUIDES = ("albedo", "normal", "depth")


def emit(out, key, run):
    out[key].append(run)
    print(json.dumps(run), file=sys.stderr, flush=True)


def scene_view(name, w, h):
    t = crt.Task(os.path.join(ROOT, "scenes", name, "config.json"), base_dir=ROOT)
    return t, crt.Scene.from_task(t, w, h), (t.eye_pos, crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up), crt.fov_to_radians(t.fov_y))


def part_time(a, out):
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        t, scene, cam = scene_view("cornell-box", w, h)
        r = crt.Render(scene, a.spp, t.P_RR, t.light_sample_n)
        r.run_view(*cam, want_halves=True)
        half = {"a": r.half_a_buffer, "b": r.half_b_buffer}
        hv = F(2.0) * r.variance_buffer
        guides = r.run_view_aov(*cam, want=GUIDES)
        r.free()
        names = ("none", "atrous", "var", "nlm")
        host = {"a": half["a"], "b": half["b"], "v": hv}
        host.update({g: guides[g] for g in GUIDES})
        for side in ("a", "b"):
            for n in names[1:]:
                host["f%s_%s" % (side, n)] = candidate(n, half[side], hv, guides, 0)
        sel_scratch, dn_scratch = crt.filter_select_scratch_bytes(w, h), crt.denoise_scratch_bytes(w, h)
        dev = hipmem.DeviceBuffers({**host, "mean": w * h * 12, "rgb": w * h * 3, "choice": w * h, "error": w * h * 4,
                                    "sel_scratch": sel_scratch, "dn_scratch": dn_scratch})
        ptrs = dev.ptrs

        def fptr(side, n):
            return ptrs[side] if n == "none" else ptrs["f%s_%s" % (side, n)]

        def call_select(cands):
            return crt.filter_select_device(w, h, ptrs["a"], ptrs["b"], ptrs["v"], [fptr("a", n) for n in cands], [fptr("b", n) for n in cands], ptrs["mean"],
                                            ptrs["rgb"], ptrs["sel_scratch"], sel_scratch, out_choice_ptr=ptrs["choice"], out_error_ptr=ptrs["error"])

        def call_pass():
            return crt.denoise_device(w, h, ptrs["a"], ptrs["mean"], ptrs["rgb"], ptrs["dn_scratch"], dn_scratch, albedo_ptr=ptrs["albedo"],
                                      normal_ptr=ptrs["normal"], depth_ptr=ptrs["depth"], iterations=1)["total_ms"]

        sets = {2: ("var", "nlm"), 4: names}
        ms, ms_pass, info = {k: [] for k in sets}, [], {}
        for _ in range(a.warmup + a.calls):
            for k, cands in sets.items():
                info[k] = call_select(cands)
                ms[k].append(info[k]["total_ms"])
            ms_pass.append(call_pass())
        one_pass = statistics.median(ms_pass[a.warmup:])
        for k in sets:
            m = ms[k][a.warmup:]
            med = statistics.median(m)
            compulsory = 36 + 24 * k + 20
            emit(out, "time", {"width": w, "height": h, "candidates": k, "select_ms_median": round(med, 4), "select_ms_best": round(min(m), 4),
                               "select_ms_worst": round(max(m), 4),
                               "select_ms_halves": [round(statistics.median(m[:len(m) // 2]), 4), round(statistics.median(m[len(m) // 2:]), 4)],
                               "chosen": info[k]["chosen"], "compulsory_bytes_per_pixel": compulsory,
                               "compulsory_TB_per_s": round(compulsory * w * h / (med * 1e-3) / 1e12, 4), "atrous_pass_ms_median": round(one_pass, 4),
                               "select_over_atrous_pass": round(med / one_pass, 3)})
        dev.free()


def part_flag(a, out):
    w, h = (int(v) for v in a.flag_size.split("x"))
    t, scene, cam = scene_view("cornell-box", w, h)
    r = crt.Render(scene, a.flag_spp, t.P_RR, t.light_sample_n)
    dev = hipmem.DeviceBuffers({"rgb": w * h * 3, "mean": w * h * 12, "a": w * h * 12, "b": w * h * 12})
    bufs = dev.ptrs
    kinds = {"plain": 0, "variance": capi.FLAG_VARIANCE, "half_buffers": capi.FLAG_HALF_BUFFERS}
    runs, read_ms = {k: [] for k in kinds}, []
    import time
    for i in range(a.frames + 1):              # (the first frame of each kind warms up: allocations, code objects)
        for kind, flags in kinds.items():
            r.extra_flags = flags
            st = r.run_view_device(*cam, bufs["rgb"], bufs["mean"])
            hipmem.device_synchronize()
            if kind == "half_buffers":
                t0 = time.perf_counter()
                capi.check(capi.lib().crt_half_buffers_device(r._h, C.c_void_p(bufs["a"]), C.c_void_p(bufs["b"]), None, None), "crt_half_buffers_device")
                hipmem.device_synchronize()
                if i > 0:
                    read_ms.append((time.perf_counter() - t0) * 1e3)
            if i > 0:
                runs[kind].append({"total_ms": st["total_ms"], "kernel_ms": st["kernel_ms"], "rest_ms": st["total_ms"] - st["kernel_ms"]})
    r.extra_flags = 0
    run = {"width": w, "height": h, "spp": a.flag_spp, "frames": a.frames}
    for key in ("total_ms", "kernel_ms", "rest_ms"):
        run[key] = {k: {"median": round(statistics.median(f[key] for f in runs[k]), 3),
                        "min_max": [round(min(f[key] for f in runs[k]), 3), round(max(f[key] for f in runs[k]), 3)]} for k in kinds}
    run["crt_half_buffers_device_wall_ms"] = round(statistics.median(read_ms), 3)
    emit(out, "flag", run)
    r.free()
    dev.free()


def window_mean(e, r):
    """the mean of e over the in-image part of the (2 r + 1)^2 window (float64)"""
    h, w = e.shape
    pad = np.zeros((h + 2 * r, w + 2 * r))
    cnt = np.zeros_like(pad)
    pad[r:r + h, r:r + w] = e
    cnt[r:r + h, r:r + w] = 1
    s, c = np.zeros((h, w)), np.zeros((h, w))
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            s += pad[dy:dy + h, dx:dx + w]
            c += cnt[dy:dy + h, dx:dx + w]
    return s / c


def select_with(errors, cands, s):
    """the contract's choice and blend from given per-pixel errors (already smoothed): the blended mean (float32)"""
    best = np.argmin(np.stack(errors), axis=0)
    o = np.zeros_like(cands[0], dtype=np.float64)
    total = window_mean(np.ones(best.shape), s)  # (1 everywhere: the weights below are shares of the window's pixels)
    for k, c in enumerate(cands):
        o += (window_mean((best == k).astype(np.float64), s) / total)[..., None] * c
    return o.astype(F)


def tone_map(mean):
    """the frame's tone map of a mean, by the device: a selection among one candidate is that candidate ((x + x) * 0.5 = x)"""
    zero = np.zeros_like(mean)
    return crt.filter_select(zero, zero, zero, [mean], [mean], error_radius=0, blend_radius=0, want_mean=False, want_choice=False, want_error=False)[0]


def part_effect(a, out):
    w, h = (int(v) for v in a.effect_size.split("x"))
    for name in a.scenes.split(","):
        t, scene, cam = scene_view(name, w, h)
        r = crt.Render(scene, a.ref_spp, t.P_RR, t.light_sample_n)
        r.seed = a.ref_seed
        ref = r.run_view(*cam).astype(np.float64)
        ref_mean = r.mean_buffer.astype(np.float64)
        r.seed = 0

        def mse(x):
            return round(float(np.mean((x.astype(np.float64) - ref) ** 2)), 1)

        for spp in (int(v) for v in a.effect_spp.split(",")):
            r.set_spp(spp)
            rgb = r.run_view(*cam, want_halves=True).copy()
            mean, var, ha, hb = r.mean_buffer.copy(), r.variance_buffer, r.half_a_buffer, r.half_b_buffer
            hv = F(2.0) * var
            g = r.run_view_aov(*cam, want=GUIDES)
            row = {"scene": name, "spp": spp, "noisy": mse(rgb), "var": mse(crt.denoise_var(mean, var, **g)[0]), "nlm": mse(crt.denoise_nlm(mean, var, **g)[0])}
            fa = {n: candidate(n, ha, hv, g, 0) for n in ("none", "var", "nlm")}
            fb = {n: candidate(n, hb, hv, g, 0) for n in ("none", "var", "nlm")}
            d = crt.filter_select_defaults()
            for names in (("var", "nlm"), ("none", "var", "nlm")):
                key = "+".join(names)
                sel = crt.filter_select(ha, hb, hv, [fa[n] for n in names], [fb[n] for n in names], return_info=True)
                row["selected " + key] = mse(sel[0])
                row["chosen " + key] = sel[4]["chosen"][:len(names)]
                cands = [(fa[n].astype(np.float64) + fb[n]) * 0.5 for n in names]
                row["halves averaged " + key] = [mse(tone_map(c.astype(F))) for c in cands]
                true = [window_mean(((c - ref_mean) ** 2).mean(axis=2), d["error_radius"]) for c in cands]
                row["true-error selection " + key] = mse(tone_map(select_with(true, cands, d["blend_radius"])))
                true0 = [((c - ref_mean) ** 2).mean(axis=2) for c in cands]
                row["true-error selection, no windows " + key] = mse(tone_map(select_with(true0, cands, 0)))
            emit(out, "effect", row)
            if a.sweep:
                for er in (1, 3, 5):
                    for br in (0, 1, 2):
                        sel = crt.filter_select(ha, hb, hv, [fa["var"], fa["nlm"]], [fb["var"], fb["nlm"]], error_radius=er, blend_radius=br)
                        emit(out, "sweep", {"scene": name, "spp": spp, "error_radius": er, "blend_radius": br, "selected var+nlm": mse(sel[0])})
        r.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("time", "flag", "effect"), required=True)
    ap.add_argument("--sizes", default="800x600,3840x2160")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--flag-size", default="800x600")
    ap.add_argument("--flag-spp", type=int, default=512)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--scenes", default="cornell-box,veach-mis")
    ap.add_argument("--effect-size", default="160x120")
    ap.add_argument("--effect-spp", default="8,32")
    ap.add_argument("--ref-spp", type=int, default=256)
    ap.add_argument("--ref-seed", type=int, default=7)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    if crt.device_count() < 1:
        raise SystemExit("select_probe: no HIP device")
    out = {"time": [], "flag": [], "effect": [], "sweep": []}
    {"time": part_time, "flag": part_flag, "effect": part_effect}[a.part](a, out)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
