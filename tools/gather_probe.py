#!/usr/bin/env python3
"""What gathering a multi-device frame's buffers costs (crt_multi_render_buffers, include/crt.h; csrc/crt_untile.h): ONE process with
--ranks ranks on ONE device, so the exchange is the peer copies of CRT_GATHER_COPY on that device -- no exchange over two or more distinct
devices is measured here.  Run by hand, one part per invocation, each under a time limit of its own:

  --part masks   per size of --sizes and per request mask of MASKS: the medians over --frames frames (after --warmup) of
                 crt_multi_info's render_ms and gather_ms, the block's bytes_per_rank, and the HIP-event time of the de-interleave kernel
                 alone (crt_multi_untile_time: --calls launches on the last frame's blocks) with the bytes it moves over that time.
  --part frame   crt_multi_render (RGB8 and the mean) as MultiRender.run_view calls it: frame_ms, render_ms and gather_ms of --frames
                 frames after --warmup, per size.  It uses nothing this commit adds, so --root may name a built checkout of another
                 commit (its package, its library, its scenes): this tree's bindings refuse a library without the new entry points, so
                 CRT_LIB_PATH alone cannot put the parent's library under them.
  --part ab      --part frame in child processes taking turns, --rounds times each: this tree and the built checkout of the parent
                 commit that --parent-root names.  Per size and tree the median over all frames and the medians of the rounds; the
                 parent's spread is the range of its rounds' medians.  This process itself opens no device.

One JSON line per figure on stderr, one JSON document on stdout.

  python tools/gather_probe.py --part masks [--sizes 800x600,3840x2160] [--ranks 4] [--spp 2] [--frames 5] [--warmup 1] [--calls 20]
  python tools/gather_probe.py --part ab --parent-root DIR [--rounds 4] [--frames 5] [--warmup 2]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # (main: --root replaces it)

MASKS = {"rgb+mean": ("rgb", "mean"),
         "denoise": ("rgb", "mean", "variance", "albedo", "normal", "depth"),
         "denoise demodulated": ("rgb", "mean", "variance", "albedo", "normal", "depth", "emission", "diffuse_albedo"),
         "select": ("rgb", "mean", "variance", "half_a", "half_b", "albedo", "normal", "depth"),
         "all": None}


def emit(out, key, run):
    out[key].append(run)
    print(json.dumps(run), file=sys.stderr, flush=True)


def multi_render(a, w, h):
    import cudaraytracing_amd as crt
    t = crt.Task(os.path.join(ROOT, "scenes", "cornell-box", "config.json"), base_dir=ROOT)
    cam = (t.eye_pos, crt.get_inverse_view_matrix(t.eye_pos, t.lookat, t.up), crt.fov_to_radians(t.fov_y))
    return crt.MultiRender(crt.Scene.from_task(t, w, h), a.spp, t.P_RR, t.light_sample_n, devices=[0] * a.ranks, gather=crt.GATHER_COPY), cam


def sizes(a):
    return [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]


def part_masks(a, out):
    from cudaraytracing_amd import _capi as capi
    for w, h in sizes(a):
        m, cam = multi_render(a, w, h)
        for label, names in MASKS.items():
            names = tuple(capi.MULTI_BUFFERS) if names is None else names
            infos = []
            for _ in range(a.warmup + a.frames):
                m.run_view_gathered(*cam, want=names, to_host=False)
                infos.append(m.info)
            infos = infos[a.warmup:]
            ms = (C.c_float * a.calls)()
            capi.check(capi.lib().crt_multi_untile_time(m._mh, a.calls, ms), "crt_multi_untile_time")
            untile = statistics.median(ms)
            moved = 2 * sum(w * h * ch * dt().itemsize for ch, dt in (capi.MULTI_BUFFERS[n] for n in names))   # read once, written once
            emit(out, "masks", {"width": w, "height": h, "ranks": a.ranks, "spp": a.spp, "mask": label, "planes": len(names),
                                "bytes_per_rank": infos[-1]["bytes_per_rank"], "render_ms": round(statistics.median(i["render_ms"] for i in infos), 3),
                                "gather_ms": round(statistics.median(i["gather_ms"] for i in infos), 3), "untile_ms_median": round(untile, 4),
                                "untile_ms_min_max": [round(min(ms), 4), round(max(ms), 4)], "untile_bytes": moved,
                                "untile_TB_per_s": round(moved / (untile * 1e-3) / 1e12, 3)})
        m.free()


def part_frame(a, out):
    for w, h in sizes(a):
        m, cam = multi_render(a, w, h)
        infos = []
        for _ in range(a.warmup + a.frames):
            m.run_view(*cam)
            infos.append(m.info)
        m.free()
        emit(out, "frame", {"width": w, "height": h, "ranks": a.ranks, "spp": a.spp, "bytes_per_rank": infos[-1]["bytes_per_rank"],
                            "frame_ms": [round(i["frame_ms"], 3) for i in infos[a.warmup:]], "render_ms": [round(i["render_ms"], 3) for i in infos[a.warmup:]],
                            "gather_ms": [round(i["gather_ms"], 3) for i in infos[a.warmup:]]})


def part_ab(a, out):
    libs = {"parent": os.path.abspath(a.parent_root), "this": ROOT}
    runs = {k: [] for k in libs}
    for _ in range(a.rounds):
        for which, root in libs.items():
            env = dict(os.environ)
            env.pop("CRT_LIB_PATH", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", "frame", "--root", root, "--sizes", a.sizes, "--ranks", str(a.ranks), "--spp", str(a.spp),
                                "--frames", str(a.frames), "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, timeout=a.child_timeout)
            if p.returncode != 0:   # (a child that failed ends the probe: nothing more is started)
                raise SystemExit("gather_probe: the %s tree's run ended with status %d\n%s" % (which, p.returncode, p.stderr[-3000:]))
            runs[which].append(json.loads(p.stdout)["frame"])
    for k, (w, h) in enumerate(sizes(a)):
        row = {"width": w, "height": h, "ranks": a.ranks, "spp": a.spp, "rounds": a.rounds, "frames_per_round": a.frames}
        for which in libs:
            for key in ("frame_ms", "gather_ms"):
                rounds = [r[k][key] for r in runs[which]]
                meds = [statistics.median(r) for r in rounds]
                row["%s %s" % (which, key)] = {"median": round(statistics.median(v for r in rounds for v in r), 3), "round_medians": [round(v, 3) for v in meds],
                                               "round_spread": round(max(meds) - min(meds), 3)}
        emit(out, "ab", row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("masks", "frame", "ab"), required=True)
    ap.add_argument("--sizes", default="800x600,3840x2160")
    ap.add_argument("--ranks", type=int, default=4)
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent-root")
    ap.add_argument("--root")
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    global ROOT
    ROOT = os.path.abspath(a.root) if a.root else ROOT
    sys.path.insert(0, ROOT)
    out = {"masks": [], "frame": [], "ab": []}
    if a.part == "ab":
        if not a.parent_root:
            raise SystemExit("gather_probe: --part ab needs --parent-root DIR")
        part_ab(a, out)
    else:
        import cudaraytracing_amd as crt
        if crt.device_count() < 1:
            raise SystemExit("gather_probe: no HIP device")
        {"masks": part_masks, "frame": part_frame}[a.part](a, out)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
