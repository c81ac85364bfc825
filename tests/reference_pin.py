"""Shared by tests/test_reference_pin.py and tests/golden/make_reference_golden.py: the cases at which the oracle (and, through it,
the kernels) are pinned to the reference's own path code, the jobs of oracle/_ref/path_probe (oracle/ref_probe/path_probe.cpp: the
reference's loader, BVH builder, traversal, integrator and pixel kernel compiled from where they lie and run on the CPU, fed with the
oracle's random draws and the oracle's transcendental functions), and the oracle's side of every comparison.

Nothing here tolerates a difference: every comparison downstream is on bits."""
import hashlib
import io
import json
import os
import shutil
import struct
import subprocess
import zipfile

import numpy as np

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "oracle", "_ref", "path_probe")
# The same program built with -O0 -fstack-reuse=none, for the two spots where the reference keeps an Eigen expression in `auto` whose
# operands are temporaries: the paths that reach Render.cuh:311-312, and the loader of a map_Kd texture (Loader.h:89-103).  What the -O2
# build reads there is stale stack (for the texture other values in every run); this build keeps every temporary's slot intact.
PROBE_O0 = PROBE + "_O0"
UNOPTIMISED_SCENES = ("textured",)
GOLD = os.path.join(ROOT, "tests", "golden", "reference_pin")
W, H = 32, 24

# (id, scene, bvh_thresh_n or None for the scene's own)
SCENE_CASES = [("cornell-box", "cornell-box", None), ("veach-mis", "veach-mis", None), ("veach-mis-thresh1", "veach-mis", 1),
               ("veach-mis-thresh5", "veach-mis", 5), ("textured", "textured", 2), ("room", "room", 2)]
INTERSECT_CASES = [("cornell-box", 11), ("veach-mis", 12)]           # (scene, seed of util.random_rays)
N_RANDOM_RAYS, N_NEE_RAYS = 4096, 1024
# full frames; the first four at W x H with the scene's own camera, the last one the closed room whose paths run into BOUNCE_STACK_SIZE
FRAME_CASES = [
    dict(id="veach-mis-spp4-rr0.6-lsn1", scene="veach-mis", w=W, h=H, spp=4, p_rr=0.6, lsn=1, seed=1),    # the specular probe, four Ns values
    dict(id="veach-mis-spp2-rr0.95-lsn2", scene="veach-mis", w=W, h=H, spp=2, p_rr=0.95, lsn=2, seed=2),  # long paths
    dict(id="cornell-box-spp4-rr0.8-lsn1", scene="cornell-box", w=W, h=H, spp=4, p_rr=0.8, lsn=1, seed=3),
    dict(id="veach-mis-spp2-rr0-lsn3", scene="veach-mis", w=W, h=H, spp=2, p_rr=0.0, lsn=3, seed=4),      # direct light only
    dict(id="room-cap-spp1-rr1-lsn1", scene="room", w=4, h=4, spp=1, p_rr=1.0, lsn=1, seed=3),            # BOUNCE_STACK_SIZE reached
]
FRAME_IDS = [c["id"] for c in FRAME_CASES]
MAX_FLAGGED = 0.25   # of a veach-mis case's paths may take the emitter-probe branch (Render.cuh:304-313); cornell-box: none


def sha1(path):
    return hashlib.sha1(open(path, "rb").read()).hexdigest()


# ------------------------------------------------------------------------------------------------ scenes
def write_textured_scene(d):
    """An OBJ with a map_Kd texture from tests/golden/textures (13 x 7: Loader.h:58 swaps width and height), uv beyond [0, 1) and
    negative (the modff chain of Loader.h:86-87), triangles wholly below y = 0.1 (the loader's normal override, Loader.h:108-111),
    above it and across it, and a light.  Random vertices: no two centroids are equal, so std::sort has no ties to break."""
    rng = np.random.default_rng(2024)
    shutil.copy(os.path.join(ROOT, "tests", "golden", "textures", "png_rgb8.png"), os.path.join(d, "tex.png"))
    v, vt, f = [], [], []
    for k in range(48):
        c = rng.uniform(0.0, 8.0, 3)
        c[1] = (0.02, 0.09, 1.5)[k % 3] if k % 4 else rng.uniform(0.0, 3.0)
        for _ in range(3):
            p = c + rng.uniform(-0.6, 0.6, 3) * (1.0, 0.05 if k % 3 < 2 else 0.8, 1.0)
            v.append(tuple(float(np.float32(x)) for x in p))
            vt.append((float(np.float32(rng.uniform(-2.5, 3.5))), float(np.float32(rng.uniform(-2.5, 3.5)))))
        f.append(("tex" if k % 5 else "plain", 3 * k + 1, 3 * k + 2, 3 * k + 3))
    b = len(v)
    for p in ((2.0, 5.0, 2.25), (6.0, 5.0, 2.0), (6.25, 5.0, 6.0), (2.0, 5.0, 6.5)):
        v.append(p)
        vt.append((0.5, 0.5))
    f.append(("light", b + 1, b + 2, b + 3))
    f.append(("light", b + 1, b + 3, b + 4))
    with open(os.path.join(d, "t.mtl"), "w") as m:
        m.write("newmtl tex\nKd 0.3 0.3 0.3\nmap_Kd tex.png\nNs 1\nnewmtl plain\nKd 0.2 0.5 0.7\nNs 40\n"
                "newmtl light\nKe 20 18 16\nKd 0 0 0\nNs 1\n")
    with open(os.path.join(d, "t.obj"), "w") as o:
        o.write("mtllib t.mtl\n")
        for p, t in zip(v, vt):
            o.write("v %r %r %r\nvn 0 1 0\nvt %r %r\n" % (p[0], p[1], p[2], t[0], t[1]))
        cur = None
        for mtl, a, bb, c in f:
            if mtl != cur:
                o.write("usemtl %s\n" % mtl)
                cur = mtl
            o.write("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % (a, a, a, bb, bb, bb, c, c, c))
    return [os.path.join(d, n) for n in ("t.obj", "t.mtl", "tex.png")]


class SceneSpec:
    """obj_paths [(obj, mtl_dir)], bvh_thresh_n, the camera (eye, inv_view, fov_y in radians) and the files read (for their SHA-1)."""

    def __init__(self, name, tmpdir, thresh=None):
        import cudaraytracing_amd as crt
        import util
        self.name = name
        if name in util.SCENES:
            t = util.task(name)
            self.obj_paths = [(str(o), str(m)) for o, m in t.OBJ_paths]
            self.thresh = t.bvh_thresh_n if thresh is None else thresh
            self.eye, self.iv, self.fov = util.camera(name)
            self.files = []
            for o, m in self.obj_paths:
                self.files.append(o)
                self.files += [os.path.join(m, ln.split()[1]) for ln in open(o) if ln.split()[:1] == ["mtllib"]]
        else:
            d = os.path.join(str(tmpdir), name)
            os.makedirs(d, exist_ok=True)
            if name == "textured":
                self.files = write_textured_scene(d)
                self.obj_paths = [(self.files[0], d)]
                eye, lookat, fov = [4.0, 2.5, -6.0], [4.0, 1.0, 4.0], 60.0
            elif name == "room":
                from scene_files import _write_box_scene
                obj, mtl = _write_box_scene(d)
                self.files = [obj, os.path.join(d, "room.mtl")]
                self.obj_paths = [(obj, mtl)]
                eye, lookat, fov = [5.0, 5.0, 0.5], [5.0, 4.0, 9.0], 70.0
            else:
                raise KeyError(name)
            self.thresh = 2 if thresh is None else thresh
            self.eye = np.array(eye, dtype=np.float32)
            self.iv = crt.get_inverse_view_matrix(self.eye, lookat, [0.0, 1.0, 0.0])
            self.fov = crt.fov_to_radians(fov)

    def file_hashes(self):
        return {os.path.basename(p): sha1(p) for p in self.files}

    def oracle(self):
        return O.OracleScene(self.obj_paths, self.thresh)

    def host_scene(self, w, h):
        import cudaraytracing_amd as crt
        sc = crt.Scene(w, h)
        for o, m in self.obj_paths:
            sc.add_obj(o, m)
        sc.set_BVH(self.thresh)
        return sc

    def job_head(self):
        b = struct.pack("<I", len(self.obj_paths))
        for o, m in self.obj_paths:
            for s in (o, m):   # the very strings the oracle's loader is given (the probe runs from the repository root)
                b += struct.pack("<I", len(s.encode())) + s.encode()
        return b + struct.pack("<I", self.thresh)


# ------------------------------------------------------------------------------------------------ the probe
def have_probe():
    return os.path.exists(PROBE)


def rebuild_probe():
    """Brings oracle/_ref/path_probe up to date where the reference tree it is compiled from is present (make decides)."""
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    ref = [ln.split("?=")[1].strip() for ln in mk.splitlines() if ln.startswith("REF ?=")][0]
    ref = os.environ.get("REF", ref)
    if os.path.isdir(os.path.join(ref, "include", "Eigen")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/path_probe"], stdout=subprocess.DEVNULL)


def run_probe(mode, job, tmpdir, check=True, binary=None):
    """Runs the probe on a job; returns (exit status, output bytes, stderr text)."""
    jp, op = os.path.join(str(tmpdir), "job_%s.bin" % mode), os.path.join(str(tmpdir), "out_%s.bin" % mode)
    with open(jp, "wb") as f:
        f.write(job)
    if os.path.exists(op):
        os.remove(op)
    p = subprocess.run([binary or PROBE, mode, jp, op], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, cwd=ROOT)
    if check and p.returncode != 0:
        raise RuntimeError("path_probe %s failed (%d): %s" % (mode, p.returncode, p.stderr.decode()[-400:]))
    return p.returncode, (open(op, "rb").read() if os.path.exists(op) else b""), p.stderr.decode()


def probe_scene(spec, tmpdir, binary=None):
    """the reference's scene dump; a scene of UNOPTIMISED_SCENES through the unoptimised build unless a binary is named"""
    binary = binary or (PROBE_O0 if spec.name in UNOPTIMISED_SCENES else PROBE)
    _, out, _ = run_probe("scene", spec.job_head(), tmpdir, binary=binary)
    n_nodes, root, n_tris, n_lights = struct.unpack_from("<IiII", out, 0)
    pos = 16
    nodes = np.frombuffer(out, dtype=O.NODE_DTYPE, count=n_nodes, offset=pos).copy()
    pos += n_nodes * O.NODE_DTYPE.itemsize
    tris = np.frombuffer(out, dtype=O.TRI_DTYPE, count=n_tris, offset=pos).copy()
    pos += n_tris * O.TRI_DTYPE.itemsize
    lights = []
    for _ in range(n_lights):
        (n,) = struct.unpack_from("<I", out, pos)
        lights.append(np.frombuffer(out, dtype=O.TRI_DTYPE, count=n, offset=pos + 4).copy())
        pos += 4 + n * O.TRI_DTYPE.itemsize
    assert pos == len(out)
    return {"root": root, "nodes": nodes, "tris": tris, "lights": lights}


HIT_DTYPE = np.dtype([("happend", "<i4"), ("t", "<f4"), ("pos", "<f4", 3), ("normal", "<f4", 3), ("tri", "<i4"), ("blocked", "<i4"),
                      ("matches", "<i4")])


def probe_intersect(spec, o, d, lim, tmpdir):
    o, d, lim = (np.ascontiguousarray(a, dtype=np.float32) for a in (o, d, lim))
    job = spec.job_head() + struct.pack("<I", len(o)) + o.tobytes() + d.tobytes() + lim.tobytes()
    _, out, _ = run_probe("intersect", job, tmpdir)
    return np.frombuffer(out, dtype=HIT_DTYPE).copy()


def paths_job(spec, case, rays, lens, words):
    """cast_ray_v2 for every logged camera ray, each with its own tape AFTER the two jitter words"""
    off = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))]).astype(np.uint64)
    keep = np.ones(len(words), dtype=bool)
    keep[off[:-1]] = False
    keep[off[:-1] + np.uint64(1)] = False
    off2 = (off - np.uint64(2) * np.arange(len(off), dtype=np.uint64)).astype(np.uint64)
    return spec.job_head() + struct.pack("<Ifi", len(rays), case["p_rr"], case["lsn"]) + np.ascontiguousarray(rays, dtype=np.float32).tobytes() + \
        off2.tobytes() + np.ascontiguousarray(words[keep], dtype=np.uint32).tobytes()


def probe_paths(spec, case, rays, lens, words, tmpdir, check=True, binary=None):
    rc, out, err = run_probe("paths", paths_job(spec, case, rays, lens, words), tmpdir, check=check, binary=binary)
    if rc != 0:
        return rc, None, None, err
    a = np.frombuffer(out, dtype=np.dtype([("L", "<f4", 3), ("used", "<u4")]))
    return rc, a["L"].copy(), a["used"].copy(), err


def pixel_tapes(case, lens, words, pixels):
    """the concatenated tapes of the spp paths of each listed pixel, jitter included: (words per pixel, the words)"""
    off = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    spp = case["spp"]
    per_pixel = np.array([off[(p + 1) * spp] - off[p * spp] for p in pixels], dtype=np.uint64)
    sel = np.concatenate([words[off[p * spp]:off[(p + 1) * spp]] for p in pixels]) if len(pixels) else np.zeros(0, dtype=np.uint32)
    return per_pixel, sel


def path_tapes(lens, words, paths):
    """the tapes (jitter included) of the listed paths alone: (words per path, the words)"""
    off = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    sel = np.concatenate([words[off[p]:off[p + 1]] for p in paths]) if len(paths) else np.zeros(0, dtype=np.uint32)
    return lens[paths], sel


def probe_frame(spec, case, lens, words, tmpdir, pixels=None, binary=None):
    """view_render_kernel for the listed pixels (default: every pixel, row by row), each with the tapes of its spp paths; returns the
    bytes (n, 3), the words each pixel consumed and the words its tape holds"""
    pixels = np.arange(case["w"] * case["h"], dtype=np.uint32) if pixels is None else np.asarray(pixels, dtype=np.uint32)
    per_pixel, sel = pixel_tapes(case, lens, words, pixels)
    off = np.concatenate([[0], np.cumsum(per_pixel)]).astype(np.uint64)
    job = spec.job_head() + struct.pack("<IIIfi", case["w"], case["h"], case["spp"], case["p_rr"], case["lsn"]) + \
        np.asarray(spec.eye, dtype=np.float32).tobytes() + np.asarray(spec.iv, dtype=np.float32).reshape(9).tobytes() + \
        struct.pack("<fI", float(np.float32(spec.fov)), len(pixels)) + pixels.tobytes() + off.tobytes() + \
        np.ascontiguousarray(sel, dtype=np.uint32).tobytes()
    _, out, _ = run_probe("frame", job, tmpdir, binary=binary)
    rgb = np.frombuffer(out, dtype=np.uint8, count=len(pixels) * 3).reshape(len(pixels), 3).copy()
    used = np.frombuffer(out, dtype="<u8", offset=len(pixels) * 3).copy()
    return rgb, used, per_pixel


SAMPLER_FNS = ("to_world", "sample_hemisphere", "sample_lobe")   # Global.h:35-94: to_world, get_cuda_random_sphere_vector, get_cuda_random_specular_sphere_vector


def samplers_job(recs):
    """The records of tests/device_fn_sets.py's sampler_records() (uint32 bits: (a, N), (N, two tape words), (out, delta_theta,
    delta_phi, two tape words)) as a job of the probe's `samplers` mode, which needs no scene"""
    tw, sh, sl = (np.ascontiguousarray(recs[k], dtype=np.uint32) for k in SAMPLER_FNS)
    assert tw.shape[1] == 6 and sh.shape[1] == 5 and sl.shape[1] == 7
    return struct.pack("<I", len(tw)) + np.ascontiguousarray(tw[:, 0:3]).tobytes() + np.ascontiguousarray(tw[:, 3:6]).tobytes() + \
        struct.pack("<I", len(sh)) + np.ascontiguousarray(sh[:, 0:3]).tobytes() + np.ascontiguousarray(sh[:, 3:5]).tobytes() + \
        struct.pack("<I", len(sl)) + np.ascontiguousarray(sl[:, 0:5]).tobytes() + np.ascontiguousarray(sl[:, 5:7]).tobytes()


def probe_samplers(recs, tmpdir):
    """the reference's own three sampler functions at the records: {name: (n, 3) uint32 bits of the result vector}"""
    _, out, _ = run_probe("samplers", samplers_job(recs), tmpdir)
    res, pos = {}, 0
    for k in SAMPLER_FNS:
        n = len(recs[k])
        res[k] = np.frombuffer(out, dtype="<u4", count=3 * n, offset=pos).reshape(n, 3).copy()
        pos += 12 * n
    assert pos == len(out)
    return res


# ------------------------------------------------------------------------------------------------ the oracle's side
def oracle_frame(spec, case, osc=None):
    """The oracle's frame of a case with its draw log: rgb, per-path L (h, w, spp, 3), tape words, words per path, flags, camera rays."""
    osc = osc or spec.oracle()
    O.draw_log_begin()
    rgb, mean, L, st = osc.render(spec.eye, spec.iv, spec.fov, case["w"], case["h"], case["spp"], case["p_rr"], case["lsn"], seed=case["seed"],
                                  want_L=True)
    log = O.draw_log_end()
    lens = np.diff(log["off"]).astype(np.uint32)
    assert len(lens) == case["w"] * case["h"] * case["spp"] == st["paths"]
    return {"rgb": rgb, "mean": mean, "L": L, "words": log["words"], "lens": lens, "flags": log["flags"], "rays": log["rays"], "stats": st}


def nee_rays(spec, osc, n):
    """Visibility queries the oracle's integrator really asks (Render.cuh:268-272): origin, direction and t_to_light = dist.x / dir.x of
    the first n next-event rays of a small frame, from the oracle's ray log.  On an unoccluded sample the hit on the light lies within
    rounding of the limit, so `t_to_light - t > 1e-5` is decided in the last bits."""
    O.ray_log_begin()
    osc.render(spec.eye, spec.iv, spec.fov, W, H, 1, 0.6, 2, seed=9)
    log = O.ray_log_end()
    nee = log[~np.isnan(log[:, 8])]
    assert len(nee) >= n
    nee = nee[:: len(nee) // n][:n]
    return nee[:, 0:3].copy(), nee[:, 3:6].copy(), nee[:, 8].copy()


def intersect_inputs(name, seed, spec, osc):
    import util
    o, d = util.random_rays(name, N_RANDOM_RAYS, seed)
    nodes = osc.nodes()
    root = nodes[osc.root]
    diag = float(np.linalg.norm(root["bb"] - root["aa"]))
    lim = (np.random.default_rng(seed).random(N_RANDOM_RAYS) * diag).astype(np.float32)
    lim[:8] = np.array([0.0, -1.0, np.inf, -np.inf, np.nan, 3.0e38, 1.0e-5, 2.0e-5], dtype=np.float32)
    no, nd, nl = nee_rays(spec, osc, N_NEE_RAYS)
    return np.concatenate([o, no]).astype(np.float32), np.concatenate([d, nd]).astype(np.float32), np.concatenate([lim, nl]).astype(np.float32)


def ray_constructor(o, d):
    """Ray's constructor (Ray.cuh:12-15) in one IEEE fp32 operation per ufunc: Eigen's normalized() (z = x*x + (y*y + z*z); v / sqrt(z) if z > 0)"""
    F = np.float32
    d = np.ascontiguousarray(d, dtype=F)
    with np.errstate(all="ignore"):
        z = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        n = np.where((z > 0)[:, None], d / np.sqrt(z)[:, None], d)
    assert n.dtype == F
    return n


# ------------------------------------------------------------------------------------------------ fixtures
SMALL_SCENE_BYTES = 1 << 16   # a scene dump up to this size is stored whole beside its digests


def field_digests(a):
    """SHA-256 of every field of a structured array (its little-endian bytes in row order): equal digests <=> equal bits, and a
    mismatch names the field"""
    return {f: hashlib.sha256(np.ascontiguousarray(a[f]).tobytes()).hexdigest() for f in a.dtype.names}


def scene_record(dump):
    """What the fixtures keep of a scene dump (the reference's or the oracle's): counts, root, and a digest of every field of the nodes,
    of the triangles in BVH order and of each light's triangles in shape order"""
    return {"n_nodes": int(len(dump["nodes"])), "n_tris": int(len(dump["tris"])), "root": int(dump["root"]),
            "lights": [int(len(l)) for l in dump["lights"]], "nodes": field_digests(dump["nodes"]), "tris": field_digests(dump["tris"]),
            "light_tris": [field_digests(l) for l in dump["lights"]]}


def oracle_scene_dump(osc):
    return {"root": osc.root, "nodes": osc.nodes(), "tris": osc.tris(), "lights": [osc.light_tris(i) for i in range(osc.num_lights)]}


def save(name, arrays):
    """A .npz whose bytes depend on its contents alone (numpy.savez stamps the time of day into the archive)"""
    path = os.path.join(GOLD, name + ".npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), version=(1, 0))
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue(), compresslevel=9)
    return os.path.getsize(path)


def load_meta():
    return json.load(open(os.path.join(GOLD, "meta.json")))


def load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return {k: z[k] for k in z.files}
