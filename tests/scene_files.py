"""The scene files that more than one test module writes into its tmp_path (a tessellated room, triangle soups with ties and degenerate
triangles, coordinates at signed zeros and denormals), and the loader that goes with them."""
import os

import numpy as np

import cudaraytracing_amd as crt


def _write_box_scene(d, n_side=6, specular=False, light=True):
    """A small closed room with an emissive quad and a tessellated floor (2 * n_side^2 + 12 triangles)."""
    import os
    v, f = [], []

    def quad(a, b, c, e, mtl):
        i = len(v)
        v.extend([a, b, c, e])
        f.append((mtl, i + 1, i + 2, i + 3))
        f.append((mtl, i + 1, i + 3, i + 4))
    S = 10.0
    step = S / n_side
    for i in range(n_side):
        for j in range(n_side):
            x0, z0 = i * step, j * step
            quad((x0, 0, z0), (x0, 0, z0 + step), (x0 + step, 0, z0 + step), (x0 + step, 0, z0), "floor")
    quad((0, S, 0), (S, S, 0), (S, S, S), (0, S, S), "wall")             # ceiling (faces down)
    quad((0, 0, S), (0, S, S), (S, S, S), (S, 0, S), "wall")             # back wall, faces -z
    quad((0, 0, 0), (S, 0, 0), (S, S, 0), (0, S, 0), "wall")             # front wall behind the camera, faces +z
    quad((0, 0, 0), (0, S, 0), (0, S, S), (0, 0, S), "wall")             # x = 0, faces +x
    quad((S, 0, 0), (S, 0, S), (S, S, S), (S, S, 0), "plate" if specular else "wall")  # x = S, faces -x
    if light:
        quad((4, S - 0.01, 4), (6, S - 0.01, 4), (6, S - 0.01, 6), (4, S - 0.01, 6), "light")
    with open(os.path.join(d, "room.mtl"), "w") as m:
        m.write("newmtl floor\nKd 0.7 0.6 0.5\nNs 1\nnewmtl wall\nKd 0.5 0.5 0.7\nNs 1\n"
                "newmtl plate\nKd 0.1 0.2 0.3\nNs 500\nnewmtl light\nKe 30 25 20\nKd 0 0 0\nNs 1\n")
    with open(os.path.join(d, "room.obj"), "w") as o:
        o.write("mtllib room.mtl\n")
        for p in v:
            o.write("v %g %g %g\nvn 0 1 0\nvt 0 0\n" % p)
        cur = None
        for mtl, a, b, c in f:
            if mtl != cur:
                o.write("usemtl %s\n" % mtl)
                cur = mtl
            o.write("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % (a, a, a, b, b, b, c, c, c))
    return os.path.join(d, "room.obj"), d


def _write_soup_scene(d, n=400, dup=60, degenerate=20, seed=11):
    """A closed room with a light and, inside it, a soup of random triangles: `dup` of them twice with identical vertices (equal
    hit distances in different leaves: the reference's tie rule), `degenerate` with zero area (determinant 0: the division by it
    is the IEEE one, not the short reciprocal), and coplanar overlapping quads."""
    import os
    rng = np.random.RandomState(seed)
    obj, mtl = _write_box_scene(d, n_side=4)
    tris = []
    for _ in range(n):
        c = rng.uniform(1.5, 8.5, 3)
        tris.append(c + rng.uniform(-0.9, 0.9, (3, 3)))
    for i in rng.choice(n, dup, replace=False):
        tris.append(tris[i].copy())                       # exact duplicates
    for _ in range(degenerate):
        p, q = rng.uniform(2, 8, 3), rng.uniform(2, 8, 3)
        tris.append(np.stack([p, q, p + 0.5 * (q - p)]))  # collinear vertices
    for z in (3.0, 3.0, 6.0):                             # coplanar overlapping quads (two of them in the same plane)
        x0, y0 = rng.uniform(2, 5, 2)
        tris.append(np.array([[x0, y0, z], [x0 + 3, y0, z], [x0 + 3, y0 + 3, z]]))
        tris.append(np.array([[x0, y0, z], [x0 + 3, y0 + 3, z], [x0, y0 + 3, z]]))
    with open(obj) as f:
        nv = sum(1 for line in f if line.startswith("v "))
    with open(obj, "a") as o:
        o.write("usemtl floor\n")
        for t in tris:
            for v in t.astype(np.float32):
                o.write("v %.9g %.9g %.9g\nvn 0 1 0\nvt 0 0\n" % tuple(v))
            o.write("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % (nv + 1, nv + 1, nv + 1, nv + 2, nv + 2, nv + 2, nv + 3, nv + 3, nv + 3))
            nv += 3
    return obj, mtl


def _write_scaled_soup_scene(d, scale):
    """The smaller soup scene with every vertex coordinate multiplied by `scale` (rounded to float32)"""
    obj, mtl = _write_soup_scene(d, n=200, dup=20, degenerate=10)
    lines = open(obj).read().split("\n")
    with open(obj, "w") as f:
        for line in lines:
            if line.startswith("v "):
                x, y, z = (np.float32(float(v) * scale) for v in line.split()[1:4])
                line = "v %.9g %.9g %.9g" % (x, y, z)
            f.write(line + "\n")
    return obj, mtl


def geometric_chain_triangles(E, ratio=1.2, row=1):
    """The triangles of write_geometric_chain_scene as an (n, 3, 3) float64 array, in file order (position by position, then along y)"""
    tris = []
    x = 2.0 ** -E
    while x < 2.0 ** E:
        s = x * (ratio - 1.0) / 2.0
        w = s / row
        for k in range(row):
            tris.append([[x, k * w, 0.0], [x + s, (k + 1) * w, 0.0], [x, k * w, s]])
        x *= ratio
    return np.array(tris, dtype=np.float64)


def write_geometric_chain_scene(d, E, ratio=1.2, row=1):
    """geo(E, ratio): a row of triangles in geometric progression along x, from 2^-E up to 2^E -- at position x the triangle (x, 0, 0),
    (x + s, s, 0), (x, 0, s) with s = x (ratio - 1) / 2, then x *= ratio.  The SAH builder's 32 centroid bins peel such a row a few
    leaves at a time, so the tree is a chain about as deep as the row is long (the re-insertion pass and the 4-wide collapse keep it).
    row > 1: `row` triangles side by side in y at each position, each 1 / row of the width -- an inner subtree hangs off every position
    of the chain.  All grey but the last, which is the light."""
    tris = geometric_chain_triangles(E, ratio, row)
    with open(os.path.join(d, "chain.mtl"), "w") as m:
        m.write("newmtl grey\nKd 0.6 0.6 0.6\nNs 1\nnewmtl light\nKe 20 20 20\nKd 0 0 0\nNs 1\n")
    with open(os.path.join(d, "chain.obj"), "w") as o:
        o.write("mtllib chain.mtl\nusemtl grey\n")
        for i, t in enumerate(tris):
            if i == len(tris) - 1:
                o.write("usemtl light\n")
            for p in t:
                o.write("v %.9g %.9g %.9g\nvn 0 1 0\nvt 0 0\n" % tuple(p))
            o.write("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % ((3 * i + 1,) * 3 + (3 * i + 2,) * 3 + (3 * i + 3,) * 3))
    return os.path.join(d, "chain.obj"), d


def geometric_chain_rays(E, ratio=1.2, row=1, n=4096, seed=7):
    """Rays for geo(E, ratio): (origins, directions, the slice of the first group), a third of the n rays in each of three groups.
    Along +-x with y = z drawn log-uniformly over the scene's scales, from before the small end and from beyond the large end (from the
    small end towards the large one the inner child is the nearest and its siblings are still ahead: the stack grows); from
    log-uniform points towards random points on random triangles; random origins and directions."""
    rng = np.random.RandomState(seed)
    tris = geometric_chain_triangles(E, ratio, row)
    lo, hi = -float(E), float(E)
    k = n // 3

    def log_uniform(shape):
        return 2.0 ** rng.uniform(lo, hi, shape)

    o = np.zeros((n, 3))
    d = np.zeros((n, 3))
    # the width at position x is s = 0.1 x for ratio 1.2: y = z = c lies inside the triangles from x = 2 c / (ratio - 1) * 2 on
    c = log_uniform(k) * (ratio - 1.0) / 8.0
    fwd = rng.rand(k) < 0.75
    o[:k, 0] = np.where(fwd, -(2.0 ** -E), 2.0 ** (E + 1))
    o[:k, 1] = c / row
    o[:k, 2] = c
    d[:k, 0] = np.where(fwd, 1.0, -1.0)
    # aimed: from a log-uniform point (either sign per coordinate) at a random point of a random triangle
    t = tris[rng.randint(0, len(tris), k)]
    a, b = rng.rand(k, 1), rng.rand(k, 1)
    flip = (a + b) > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    p = t[:, 0] + a * (t[:, 1] - t[:, 0]) + b * (t[:, 2] - t[:, 0])
    o[k:2 * k] = log_uniform((k, 3)) * rng.choice([-1.0, 1.0], (k, 3))
    d[k:2 * k] = p - o[k:2 * k]
    # random
    o[2 * k:] = log_uniform((n - 2 * k, 3)) * rng.choice([-1.0, 1.0], (n - 2 * k, 3))
    d[2 * k:] = rng.normal(size=(n - 2 * k, 3))
    return o.astype(np.float32), d.astype(np.float32), slice(0, k)


def _scene(obj, mtl, thresh, w=32, h=24):
    s = crt.Scene(w, h)
    s.add_obj(obj, mtl)
    s.set_BVH(thresh)
    return s


def write_signed_zero_scene(d, n=240, seed=5, denormals=True):
    """Triangles whose coordinates are +0.0, -0.0, denormals and small normals (and, per triangle, two coordinates from [2, 3], so that
    no two leaves share a centroid): box planes at both zeros and at denormals, unions over +-0 (the sign the builders give them), and
    nodes4i nudges that cross zero."""
    rng = np.random.RandomState(seed)
    vals = [0.0, -0.0, 0.25, 0.5, 1.0] + ([1e-45, 3e-42, 1e-39, 1.1754944e-38] if denormals else [])   # (lo planes at +0.0 nudged down cross zero)
    vals = np.array(vals, np.float32)
    with open(os.path.join(d, "zeros.mtl"), "w") as m:
        m.write("newmtl floor\nKd 0.7 0.6 0.5\nNs 1\n")
    with open(os.path.join(d, "zeros.obj"), "w") as o:
        o.write("mtllib zeros.mtl\nusemtl floor\n")
        for i in range(n):
            t = vals[rng.randint(0, len(vals), (3, 3))]
            t[1, rng.randint(0, 3)] = np.float32(rng.uniform(2.0, 3.0))
            t[2, rng.randint(0, 3)] = np.float32(rng.uniform(2.0, 3.0))
            for p in t:
                o.write("v %.9g %.9g %.9g\nvn 0 1 0\nvt 0 0\n" % tuple(float(c) for c in p))
            o.write("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % ((3 * i + 1,) * 3 + (3 * i + 2,) * 3 + (3 * i + 3,) * 3))
    return os.path.join(d, "zeros.obj"), d
