"""The contract of crt_temporal_dual (include/crt.h) restated in numpy float32 on the restatements that exist: temporal_restated.restated
is the statement of a candidate's taps, temporal_clamp_restated.restated_clamped of the clamp and the blend, temporal_clamp_restated.history_colour
reads H = hc / ws out of the former.  What is written here is what the dual pass adds:

  candidate V is candidate S of other inputs -- the pixel's path_depth in the place of its depth, its last normal in the place of its normal,
    and as the previous frame's depth its path_depth where its bounces reach min_bounces and 0 (no tap: crt_temporal skips a depth that is
    not > 0) elsewhere; the first-hit ids stay.  A pixel whose own bounces do not reach min_bounces does not try V at all;
  the choice -- mu, the two distances e, V iff !valid_S || e_V < e_S;
  the counts.

The blend of the chosen candidate is restated_clamped's of that candidate's inputs, so the output is a per-pixel selection between two of
its results.  Every ufunc below is one IEEE fp32 operation per element."""
import numpy as np

import temporal_clamp_restated as TC
import temporal_restated as T

F = np.float32
SPECULAR = ("path_depth", "bounces", "last_normal")
DEFAULTS = {"radius": 1, "min_bounces": 0.5}


def surface_inputs(frame):
    """a frame's dict without the specular planes: what crt_temporal takes"""
    return None if frame is None else {k: v for k, v in frame.items() if k not in SPECULAR}


def virtual_inputs(frame, min_bounces, is_history):
    """The frame as candidate V's crt_temporal sees it (see the module's text).  The current frame's bounces are not applied here: they
    decide whether V is tried, not whether a tap counts."""
    out = surface_inputs(frame)
    out.pop("normal", None)
    pd = np.ascontiguousarray(frame["path_depth"], dtype=F)
    if is_history:
        with np.errstate(invalid="ignore"):
            mirror = np.ascontiguousarray(frame["bounces"], dtype=F) >= F(min_bounces)         # (a NaN: false)
        pd = np.where(mirror, pd, F(0))
    out["depth"] = pd
    if frame.get("last_normal") is not None:
        out["normal"] = frame["last_normal"]
    return out


def mean_colour(color, radius):
    """mu of the contract's step 3: the clamp's s1 / cnt"""
    return TC.neighbourhood_box(np.ascontiguousarray(color, dtype=F), int(radius), 0.0)[0]


def distance(Hh, mu):
    with np.errstate(all="ignore"):
        d = Hh - mu
        e = d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    assert e.dtype == F
    return e


def restated_dual(cur, cam, prev=None, pcam=None, clamp=None, dual=None, depth_tolerance=0.05, normal_tolerance=0.5, alpha_min=0.05,
                  want_history_colour=False):
    """crt_temporal_dual in numpy float32.  cur / prev: the dicts crt.temporal(dual=...) takes; clamp: None or (radius, gamma); dual: None
    (the defaults) or (radius, min_bounces).  Returns (color, variance or None, history, masks): masks = dict of took, clamped, tried,
    took_V (bool, per pixel).  want_history_colour: also H = hc / ws of the chosen candidate (meaningful where took)."""
    radius, min_bounces = (DEFAULTS["radius"], DEFAULTS["min_bounces"]) if dual is None else dual
    kw = dict(depth_tolerance=depth_tolerance, normal_tolerance=normal_tolerance, alpha_min=alpha_min)
    cs, ps = surface_inputs(cur), surface_inputs(prev)
    out_c, out_v, out_h, took_S, clamped_S = TC.restated_clamped(cs, cam, ps, pcam, clamp=clamp, **kw)
    none = np.zeros(took_S.shape, dtype=bool)
    if prev is None:
        res = (out_c, out_v, out_h, {"took": none, "clamped": none, "tried": none, "took_V": none})
        return res + (np.zeros_like(out_c),) if want_history_colour else res
    with np.errstate(invalid="ignore"):
        tried = (np.ascontiguousarray(cur["bounces"], dtype=F) >= F(min_bounces)) & (np.ascontiguousarray(cur["path_depth"], dtype=F) > 0)
    cv, pv = virtual_inputs(cur, min_bounces, False), virtual_inputs(prev, min_bounces, True)
    v_c, v_v, v_h, took_V, clamped_V = TC.restated_clamped(cv, cam, pv, pcam, clamp=clamp, **kw)
    valid_S, valid_V = took_S, tried & took_V
    tol = dict(depth_tolerance=depth_tolerance, normal_tolerance=normal_tolerance)
    H_S, H_V = TC.history_colour(cs, cam, ps, pcam, **tol), TC.history_colour(cv, cam, pv, pcam, **tol)
    mu = mean_colour(cur["color"], radius)
    with np.errstate(invalid="ignore"):
        take_V = valid_V & (~valid_S | (distance(H_V, mu) < distance(H_S, mu)))               # a tie or a NaN keeps S
    color = np.where(take_V[..., None], v_c, out_c)
    var = None if out_v is None else np.where(take_V[..., None], v_v, out_v)
    hist = np.where(take_V, v_h, out_h)
    masks = {"took": valid_S | take_V, "clamped": np.where(take_V, clamped_V, clamped_S), "tried": tried, "took_V": take_V}
    res = (color, var, hist, masks)
    return res + (np.where(take_V[..., None], H_V, H_S),) if want_history_colour else res


def counts(masks):
    return {"reprojected": int(masks["took"].sum()), "clamped": int(masks["clamped"].sum()), "virtual_tried": int(masks["tried"].sum()),
            "virtual_taken": int(masks["took_V"].sum())}


# ---- inputs ----

def mirror_scene(W, H, eye, zm=100.0, zq=-50.0):
    """A camera at `eye` looking along +z at a mirror in the plane z = zm (temporal_restated.plane_setup's plane); behind the camera the plane
    z = zq, parallel to it, coloured by temporal_restated.plane_colour of world x and y.  A pixel shows the point of that plane its
    reflected ray reaches: the point of the virtual plane z = 2 zm - zq on the straight pixel ray, mirrored in z -- the same x and y.
    Returns (camera, the frame's dict in float64 -- depth to the mirror, path_depth = that + the way on to the plane, bounces 1, one id,
    the colour of the reflected point --, the virtual points)."""
    cam, depth, P = T.plane_setup(W, H, eye)
    e = np.asarray(eye, dtype=np.float64)
    path = depth * ((2 * zm - zq) - e[2]) / (zm - e[2])
    Pv = e + (P - e) / depth[..., None] * path[..., None]
    frame = {"color": T.plane_colour(Pv), "depth": depth, "path_depth": path, "bounces": np.ones((H, W)), "id": np.full((H, W), 5, dtype=np.int32)}
    return cam, frame, Pv


def as_float32(frame):
    return {k: (v if v.dtype == np.int32 else v.astype(F)) for k, v in frame.items()}


def synthetic(w, h, seed, last_normal=True):
    """Two frames of random colours on random surfaces, seen by cameras that differ by a translation, a rotation and in fov_y, so that the
    first hit (depth about 40) and the virtual point (path_depth about 70) of a pixel land on different taps.  Planted: holes in either
    frame (depth 0, path_depth 0, independently), bounces on both sides of 0.5 and exactly 0.5, blocks of differing ids and of last
    normals that fail the test, a block where the history is black (H_S == H_V == 0: a tie), a block where path_depth == depth in both
    frames under equal normals (V projects where S does), a block where only V's taps can count (previous depth 0) and one where only
    S's can (previous path_depth 0).  Returns (cur, cam, prev, pcam)."""
    rng = np.random.default_rng(seed)

    def unit(n):
        return (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(F)

    def frame():
        n = np.array([0.0, 0.0, 1.0]) + rng.normal(size=(h, w, 3)) * 0.25
        m = np.array([0.0, 1.0, 0.0]) + rng.normal(size=(h, w, 3)) * 0.25
        f = {"color": (rng.random((h, w, 3)) * 100).astype(F), "variance": (rng.random((h, w, 3)) * 300).astype(F),
             "depth": (F(40.0) * (F(0.94) + rng.random((h, w)).astype(F) * F(0.12))).astype(F),
             "normal": unit(n), "id": np.full((h, w), 3, dtype=np.int32),
             "path_depth": (F(70.0) * (F(0.94) + rng.random((h, w)).astype(F) * F(0.12))).astype(F),
             "bounces": rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], dtype=F), size=(h, w))}
        if last_normal:
            f["last_normal"] = unit(m)
        return f

    cur, prev = frame(), frame()
    prev["history"] = (1 + rng.integers(0, 40, (h, w))).astype(F)

    def block(y0, y1, x0, x1):
        return (slice(min(y0, h - 1), min(y1, h)), slice(min(x0, w - 1), min(x1, w)))

    cur["depth"][block(h // 3, h // 3 + 5, w // 4, w // 4 + 9)] = 0.0
    prev["depth"][block(h // 2, h // 2 + 5, w // 2, w // 2 + 11)] = 0.0              # only V's taps can count here
    cur["path_depth"][block(2, 6, 3 * w // 4, 3 * w // 4 + 8)] = 0.0
    prev["path_depth"][block(h // 4, h // 4 + 6, w // 8, w // 8 + 10)] = 0.0         # only S's
    prev["id"][block(1, 5, w // 2, w // 2 + 9)] = 7
    cur["id"][block(2 * h // 3, 2 * h // 3 + 4, 5, 20)] = 9
    prev["color"][block(3 * h // 4, h, 0, w // 3)] = 0.0                             # black history: both H are 0, a tie
    same = block(0, h // 5 + 1, 0, w // 5 + 1)                                       # V projects where S does
    for f in (cur, prev):
        f["path_depth"][same] = f["depth"][same]
        f["bounces"][same] = 1.0
        if last_normal:
            f["last_normal"][same] = f["normal"][same]
    if last_normal:
        prev["last_normal"][block(h // 2, h // 2 + 4, 0, 12)] = np.array([1.0, 0.0, 0.0], dtype=F)
    eye = np.array([1.0, 2.0, 3.0], dtype=F)
    up = [0.0, 1.0, 0.0]
    import cudaraytracing_amd as crt
    cam = (eye, crt.get_inverse_view_matrix(eye, eye + np.array([0.0, 0.0, 1.0], dtype=F), up), F(0.7))
    t = np.radians(3.0)
    peye = eye + np.array([1.5, -0.75, 0.5], dtype=F)
    pcam = (peye, crt.get_inverse_view_matrix(peye, peye + np.array([np.sin(t), 0.02, np.cos(t)], dtype=F), up), F(0.75))
    return cur, cam, prev, pcam
