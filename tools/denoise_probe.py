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
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cudaraytracing_amd as crt  # noqa: E402
from cudaraytracing_amd import _capi as capi  # noqa: E402

CACHE_SIDE_BYTES = 25 * 40 + 12   # per pixel and pass: 10 floats per tap, 3 floats written
COMPULSORY_BYTES = 40 + 12


def hip_runtime():
    capi.lib()
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    H = C.CDLL(path)
    H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    H.hipFree.argtypes = [C.c_void_p]
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return H


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
    a = ap.parse_args()
    if crt.device_count() < 1:
        raise SystemExit("denoise_probe: no HIP device")
    if a.error:
        return error_table(a)
    H = hip_runtime()
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
        ptrs = {}
        for name, nbytes in [(n, v.nbytes) for n, v in host.items()] + [("out_mean", w * h * 12), ("out_rgb", w * h * 3), ("out_var", w * h * 4),
                                                                                    ("scratch", scratch_bytes)]:
            p = C.c_void_p()
            if H.hipMalloc(C.byref(p), nbytes) != 0:
                raise RuntimeError("hipMalloc of %d bytes failed" % nbytes)
            ptrs[name] = p.value
        for name, v in host.items():
            if H.hipMemcpy(C.c_void_p(ptrs[name]), v.ctypes.data, v.nbytes, 1) != 0:  # hipMemcpyHostToDevice
                raise RuntimeError("hipMemcpy failed")

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
        for p in ptrs.values():
            H.hipFree(C.c_void_p(p))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
