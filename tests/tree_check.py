"""Structural checker of the traversal trees a scene handle holds (Render.export_trees), in plain numpy.

The exactness proof of EXACT / FAST (csrc/crt_accel.h) rests on facts about the arrays the kernel walks, not on frames:
every reference leaf is reached exactly once, a leaf's own box is the reference's bit for bit, an inner box contains every box below
it, no plane is NaN.  This module restates every layout from the comments that define it (csrc/crt_device.h, csrc/crt_scene_layout.h:
build_scene_layout) and the kernel's nodes4i decode (csrc/crt_mega3_decoupled.h: visit_front) without calling product code; the single
source of truth is the reference BVH of the host layer (Scene.nodes(), Scene.triangles()).

check_trees() returns a list of violations, each a string that starts with the invariant it breaks ("I1: ...").  I1 every leaf
exactly once, I2 leaf box exact, I3 supersets / no NaN / empty slots, I4 the exact subtree is the reference tree, I5 the nodes4i
decode rebuilds nodes4, I6 leaf records and triangles, I7 depths and stack_cap, I8 layout_caps, I9 coord_max."""
import numpy as np

EMPTY_REF = np.int32(~0x7ffffff0)     # ref of an empty slot of nodes4 (never followed)
PINF, NINF = np.uint32(0x7f800000), np.uint32(0xff800000)
FLT_MIN = np.float32(2.0 ** -126)


def _u(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class Ref:
    """The reference BVH: leaves numbered in node-array order, their boxes and their first leaf_geo record."""

    def __init__(self, nodes, root, tris):
        self.nodes, self.root, self.tris = nodes, int(root), tris
        is_leaf = (nodes["lc"] < 0) & (nodes["rc"] < 0)
        self.is_leaf = is_leaf
        self.leaf_nodes = np.nonzero(is_leaf)[0]
        self.n_leaves = len(self.leaf_nodes)
        self.leaf_of_node = np.full(len(nodes), -1, dtype=np.int64)
        self.leaf_of_node[self.leaf_nodes] = np.arange(self.n_leaves)
        self.it = nodes["it"][self.leaf_nodes].astype(np.int64)
        self.n = nodes["n"][self.leaf_nodes].astype(np.int64)
        self.lo = nodes["aa"][self.leaf_nodes].astype(np.float32)
        self.hi = nodes["bb"][self.leaf_nodes].astype(np.float32)
        self.leaf_of_it = np.full(max(len(tris), 1), -1, dtype=np.int64)
        self.leaf_of_it[self.it] = np.arange(self.n_leaves)
        nrec = (self.n + 1) // 2                                  # records of a leaf: two triangles each, in node-array order
        self.rec_first = np.concatenate([[0], np.cumsum(nrec)[:-1]]).astype(np.int64)
        self.n_records = int(nrec.sum())
        self.leaf_of_first_rec = np.full(self.n_records, -1, dtype=np.int64)
        self.leaf_of_first_rec[self.rec_first] = np.arange(self.n_leaves)

    def leaf_of_rec(self, rec):
        rec = np.asarray(rec, dtype=np.int64)
        ok = (rec >= 0) & (rec < self.n_records)
        out = np.full(rec.shape, -1, dtype=np.int64)
        out[ok] = self.leaf_of_first_rec[rec[ok]]
        return out


class Wide:
    """A tree in one form: per node W slots with box (lo, hi: (n, W, 3)), kind (0 empty, 1 inner, 2 leaf, -1 undecodable) and target
    (inner: node index, leaf: reference leaf number)."""

    def __init__(self, name, lo, hi, kind, tgt, root_kind, root_tgt):
        self.name, self.lo, self.hi, self.kind, self.tgt = name, lo, hi, kind, tgt
        self.root_kind, self.root_tgt = root_kind, root_tgt
        self.n = lo.shape[0]


def _binary(name, rows, decode_leaf, root):
    """nodes (crt_device.h): [0] = (L.lo, ref L) [1] = (L.hi, ref R) [2] = (R.lo, 0) [3] = (R.hi, 0)."""
    r = rows.reshape(-1, 4, 4)
    lo = np.stack([r[:, 0, :3], r[:, 2, :3]], axis=1)
    hi = np.stack([r[:, 1, :3], r[:, 3, :3]], axis=1)
    refs = np.stack([_i(r[:, 0, 3]), _i(r[:, 1, 3])], axis=1).astype(np.int64)
    return _wide_from_refs(name, lo, hi, refs, decode_leaf, root, empty=False)


def _binary3(name, rows, decode_leaf, root):
    """nodes3 (crt_device.h): [0] = (lo.x L, lo.x R, lo.y L, lo.y R) [1] = (lo.z L, lo.z R, hi.x L, hi.x R)
    [2] = (hi.y L, hi.y R, hi.z L, hi.z R) [3] = (ref L, ref R, 0, 0)."""
    r = rows.reshape(-1, 4, 4)
    lo = np.stack([np.stack([r[:, 0, 0], r[:, 0, 2], r[:, 1, 0]], -1), np.stack([r[:, 0, 1], r[:, 0, 3], r[:, 1, 1]], -1)], axis=1)
    hi = np.stack([np.stack([r[:, 1, 2], r[:, 2, 0], r[:, 2, 2]], -1), np.stack([r[:, 1, 3], r[:, 2, 1], r[:, 2, 3]], -1)], axis=1)
    refs = np.stack([_i(r[:, 3, 0]), _i(r[:, 3, 1])], axis=1).astype(np.int64)
    return _wide_from_refs(name, lo, hi, refs, decode_leaf, root, empty=False)


def _wide_from_refs(name, lo, hi, refs, decode_leaf, root, empty):
    kind = np.where(refs >= 0, 1, 2)
    if empty:
        kind = np.where(refs == EMPTY_REF, 0, kind)
    tgt = np.where(refs >= 0, refs, -1)
    leaf = kind == 2
    tgt[leaf] = decode_leaf(refs[leaf])
    kind = np.where((kind == 2) & (tgt < 0), -1, kind)
    kind = np.where((kind == 1) & (tgt >= lo.shape[0]), -1, kind)
    if root >= 0:
        return Wide(name, lo, hi, kind, tgt, 1 if root < lo.shape[0] else -1, root)
    t = int(decode_leaf(np.array([root], dtype=np.int64))[0])
    return Wide(name, lo, hi, kind, tgt, 2 if t >= 0 else -1, t)


def _walk(w, v):
    """Breadth-first walk from the root: (reached inner nodes in order, depth of each, leaf targets reached, tree depth)."""
    if w.root_kind == 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.array([w.root_tgt]), 1
    if w.root_kind != 1:
        v.append("I1: %s: root %d cannot be decoded" % (w.name, w.root_tgt))
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    order, depths, leaves = [], [], []
    front, d, seen = np.array([w.root_tgt], dtype=np.int64), 1, np.zeros(w.n, dtype=bool)
    depth = 1
    while len(front):
        if seen[front].any() or len(np.unique(front)) != len(front):
            v.append("I1: %s: an inner node is reached twice (depth %d)" % (w.name, d))
            front = np.unique(front[~seen[front]])
            if not len(front):
                break
        seen[front] = True
        order.append(front)
        depths.append(np.full(len(front), d))
        k, t = w.kind[front], w.tgt[front]
        if (k == -1).any():
            v.append("I1: %s: %d child refs cannot be decoded" % (w.name, int((k == -1).sum())))
        if (k != 0).any():
            depth = d + 1
        leaves.append(t[k == 2])
        front = t[k == 1]
        d += 1
    return np.concatenate(order), np.concatenate(depths), np.concatenate(leaves) if leaves else np.zeros(0, np.int64), depth


def _leaf_unions(w, ref, nodes, depths):
    """The exact union of the reference leaf boxes below each reached inner node (deepest level first)."""
    ulo = np.full((w.n, 3), np.inf, np.float32)
    uhi = np.full((w.n, 3), -np.inf, np.float32)
    for d in range(int(depths.max()), 0, -1):
        q = nodes[depths == d]
        k, t = w.kind[q], w.tgt[q]
        slo = np.full(k.shape + (3,), np.inf, np.float32)
        shi = np.full(k.shape + (3,), -np.inf, np.float32)
        lf, inn = k == 2, k == 1
        slo[lf], shi[lf] = ref.lo[t[lf]], ref.hi[t[lf]]
        slo[inn], shi[inn] = ulo[t[inn]], uhi[t[inn]]
        ulo[q], uhi[q] = slo.min(1), shi.max(1)
    return ulo, uhi


def check_tree(w, ref, v, empty_slots, direct=True):
    """I1 - I3 on one tree; returns (reached inner nodes, depth).  direct: an inner slot must contain every used slot box of its child
    (nodes, nodes3, nodes4: inner boxes are exact unions); otherwise (nodes4i, whose inner children's planes are nudged outwards, so that a
    child's box may stick out of its parent's slot) every leaf box below it -- what the proof needs (crt_accel.h: a leaf is entered iff
    every ancestor box passes, and a box that contains the leaf's own passes whenever the leaf's does)."""
    nodes, depths, leaves, depth = _walk(w, v)
    cnt = np.bincount(leaves.astype(np.int64), minlength=ref.n_leaves) if len(leaves) else np.zeros(ref.n_leaves, np.int64)
    if (cnt == 0).any():
        v.append("I1: %s: %d reference leaves are not reached (first: leaf %d)" % (w.name, int((cnt == 0).sum()), int(np.argmin(cnt))))
    if (cnt > 1).any():
        v.append("I1: %s: %d reference leaves are reached more than once (first: leaf %d)" % (w.name, int((cnt > 1).sum()), int(np.argmax(cnt > 1))))
    if w.root_kind == 2 or not len(nodes):
        return nodes, depth
    k, t = w.kind[nodes], w.tgt[nodes]
    lo, hi = w.lo[nodes], w.hi[nodes]
    # I2: a leaf slot's six planes are the reference leaf's box, bit for bit
    m = k == 2
    if m.any():
        bad = (_u(lo[m]) != _u(ref.lo[t[m]])).any(-1) | (_u(hi[m]) != _u(ref.hi[t[m]])).any(-1)
        if bad.any():
            v.append("I2: %s: %d leaf slots whose box is not the reference leaf's bit for bit" % (w.name, int(bad.sum())))
    # I3: no NaN in a used slot; empty slots are exactly (+inf, -inf); an inner slot contains every used slot of its child
    used = k != 0
    if (np.isnan(lo[used]).any() or np.isnan(hi[used]).any()):
        v.append("I3: %s: NaN plane in a used slot" % w.name)
    e = k == 0
    if e.any():
        if not empty_slots:
            v.append("I3: %s: empty slot in a binary tree" % w.name)
        elif (_u(lo[e]) != PINF).any() or (_u(hi[e]) != NINF).any():
            v.append("I3: %s: %d empty slots are not exactly (+inf, -inf)" % (w.name, int(e.sum())))
    qi, si = np.nonzero(k == 1)
    if len(qi):
        c = t[qi, si]
        plo, phi = lo[qi, si][:, None, :], hi[qi, si][:, None, :]
        if direct:
            clo, chi, cu = w.lo[c], w.hi[c], w.kind[c] != 0
        else:
            ulo, uhi = _leaf_unions(w, ref, nodes, depths)
            clo, chi, cu = ulo[c][:, None, :], uhi[c][:, None, :], np.ones((len(c), 1), bool)
        with np.errstate(invalid="ignore"):
            out = ((clo < plo) | (chi > phi)).any(-1) & cu
        if out.any():
            v.append("I3: %s: %d inner slots do not contain %s" % (w.name, int(out.any(-1).sum()), "their child's boxes" if direct else "the leaf boxes below them"))
    return nodes, depth


def check_exact(w, ref, v):
    """I4: the subtree of the exact root is the reference BVH: same topology, child order and boxes bit for bit."""
    N = ref.nodes
    if ref.is_leaf[ref.root]:
        if not (w.root_kind == 2 and w.root_tgt == ref.leaf_of_node[ref.root]):
            v.append("I4: %s: the reference root is a leaf, the exact root is not that leaf" % w.name)
        return
    if w.root_kind != 1:
        v.append("I4: %s: the exact root is not an inner node" % w.name)
        return
    rf, ex = np.array([ref.root]), np.array([w.root_tgt], dtype=np.int64)
    while len(rf):
        nxt_r, nxt_e = [], []
        for s, side in enumerate(("lc", "rc")):
            rc = N[side][rf].astype(np.int64)
            k, t = w.kind[ex, s], w.tgt[ex, s]
            bad = (_u(w.lo[ex, s]) != _u(N["aa"][rc])).any(-1) | (_u(w.hi[ex, s]) != _u(N["bb"][rc])).any(-1)
            if bad.any():
                v.append("I4: %s: %d exact-tree slots whose box is not the reference child's" % (w.name, int(bad.sum())))
            rl = ref.is_leaf[rc]
            if ((k == 2) != rl).any() or (rl & (t != ref.leaf_of_node[rc])).any():
                v.append("I4: %s: exact-tree topology or child order differs from the reference" % w.name)
                return
            nxt_r.append(rc[~rl]); nxt_e.append(t[~rl])
        rf, ex = np.concatenate(nxt_r), np.concatenate(nxt_e)


def _empty_node_ok(rows):
    return (_u(rows[0::2]) == PINF).all() and (_u(rows[1::2]) == NINF).all()


def decode_nodes4i(ex, ref, n4i_rows, v):
    """The kernel's decode of nodes4i (crt_mega3.hip): child 0's planes of a mixed node carry (fm, ff, n_m, n_f) in their low 12 bits --
    cx from lo.x, cy from lo.y, cz from lo.z; fm = cx | (cy & 7) << 12, ff = cy >> 3 | (cz & 63) << 9, n_m = cz >> 6 & 7,
    n_f = cz >> 9.  Slot i < n_m: node fm + i; n_m <= i < n_m + n_f: node ff + i - n_m; else leaf record 4 n + i of leaf_geo_i (or an
    empty slot).  A node numbered from n_mixed4i on is fringe: no bits, leaves only."""
    F = int(ex["node4i_f4"])
    n_all = len(n4i_rows) // F
    r = n4i_rows.reshape(n_all, F, 4)[:, :6]
    lo = np.stack([r[:, 0], r[:, 2], r[:, 4]], -1)   # (n, 4 slots, 3)
    hi = np.stack([r[:, 1], r[:, 3], r[:, 5]], -1)
    n4 = n_all - 1
    nm = int(ex["n_mixed4i"])
    lo, hi = lo[:n4], hi[:n4]
    ids = np.arange(n4)
    clo, chi = _u(lo[:, 0, :]) & 0xfff, _u(hi[:, 0, :]) & 0xfff
    mixed = ids < nm
    if (clo[mixed] != chi[mixed]).any():
        v.append("I5: nodes4i: %d mixed nodes whose lo and hi planes of child 0 carry different bits" % int((clo[mixed] != chi[mixed]).any(-1).sum()))
    cx, cy, cz = clo[:, 0].astype(np.int64), clo[:, 1].astype(np.int64), clo[:, 2].astype(np.int64)
    fm = cx | ((cy & 7) << 12)
    ff = (cy >> 3) | ((cz & 63) << 9)
    cm = np.where(mixed, (cz >> 6) & 7, 0)
    ci = np.where(mixed, cm + (cz >> 9), 0)
    kind = np.zeros((n4, 4), np.int64)
    tgt = np.full((n4, 4), -1, np.int64)
    lgi_recs = len(ex["leaf_geo_i"]) // 5
    inv = np.full(lgi_recs, -1, np.int64)
    rm = ex["rec_map"].astype(np.int64)
    okm = (rm >= 0) & (rm < lgi_recs)
    inv[rm[okm]] = np.arange(len(rm))[okm]
    empty = (_u(lo) == PINF).all(-1) & (_u(hi) == NINF).all(-1)
    for i in range(4):
        inner = i < ci
        child = np.where(i < cm, fm + i, ff + i - cm)
        kind[:, i] = np.where(inner, 1, np.where(empty[:, i], 0, 2))
        tgt[:, i] = np.where(inner, child, -1)
        bad_inner = inner & ((child < 0) | (child >= n4) | ((i < cm) & (child >= nm)) | ((i >= cm) & (child < nm)))
        kind[bad_inner, i] = -1
        leaf = kind[:, i] == 2
        sp = ids[leaf] * 4 + i
        dense = np.where(sp < lgi_recs, inv[np.minimum(sp, lgi_recs - 1)], -1)
        tgt[leaf, i] = ref.leaf_of_rec(dense)
        kind[leaf, i] = np.where(tgt[leaf, i] >= 0, 2, -1)
    # classes in slot order: inner, leaves, empty (no leaf after an empty slot)
    seen_empty = np.logical_or.accumulate(kind == 0, axis=1)
    if ((kind == 2) & seen_empty).any():
        v.append("I5: nodes4i: a leaf slot after an empty slot")
    if not _empty_node_ok(r[n4, :6]) or int(ex["empty4i_off"]) != n4 * F * 16:
        v.append("I3: nodes4i: the empty node at empty4i_off is not four (+inf, -inf) slots behind the tree")
    rk = int(ex["root4i"])
    w = Wide("nodes4i", lo, hi, kind, tgt, 1 if 0 <= rk < n4 else -1, rk)
    return w, mixed


def _min_leaf(w, order):
    """Smallest reference leaf below each reached inner node (the subtrees' leaf sets are disjoint: it names a subtree)."""
    ml = np.full(w.n, np.iinfo(np.int64).max, np.int64)
    big = np.iinfo(np.int64).max
    for q in order[::-1]:
        k, t = w.kind[q], w.tgt[q]
        vals = [int(t[s]) if k[s] == 2 else (int(ml[t[s]]) if k[s] == 1 else big) for s in range(len(k))]
        ml[q] = min(vals)
    return ml


def check_nodes4i_against_nodes4(w4, wi, mixed, v, order4, orderi, stats):
    """I5: the decoded nodes4i is nodes4 with children reordered (mixed, fringe, leaf, empty) and child 0's planes of a mixed node moved
    outwards only -- by at most 2^-11 of the coordinate, or across zero by a denormal."""
    ml4, mli = _min_leaf(w4, order4), _min_leaf(wi, orderi)
    if w4.root_kind != 1 or wi.root_kind != 1:
        return
    todo = [(w4.root_tgt, wi.root_tgt)]
    stats["nudged_planes"], stats["crossed_zero"] = 0, 0
    while todo:
        q, n = todo.pop()
        a = {}
        for s in range(4):
            if w4.kind[q, s] == 1:
                a[("i", int(ml4[w4.tgt[q, s]]))] = s
            elif w4.kind[q, s] == 2:
                a[("l", int(w4.tgt[q, s]))] = s
        b = {}
        for s in range(4):
            if wi.kind[n, s] == 1:
                b[("i", int(mli[wi.tgt[n, s]]))] = s
            elif wi.kind[n, s] == 2:
                b[("l", int(wi.tgt[n, s]))] = s
        if set(a) != set(b):
            v.append("I5: nodes4i node %d does not hold the children of nodes4 node %d" % (n, q))
            continue
        for key, s4 in a.items():
            si = b[key]
            l4, h4, li, hi_ = w4.lo[q, s4], w4.hi[q, s4], wi.lo[n, si], wi.hi[n, si]
            if key[0] == "i":
                c4, ci = int(w4.tgt[q, s4]), int(wi.tgt[n, si])
                child_mixed = (w4.kind[c4] == 1).any()
                if child_mixed != bool(mixed[ci]):
                    v.append("I5: nodes4i node %d is numbered as %s but is not" % (ci, "mixed" if mixed[ci] else "fringe"))
                todo.append((c4, ci))
            if key[0] == "i" and si == 0 and mixed[n]:
                stats["nudged_planes"] += int((_u(l4) != _u(li)).sum() + (_u(h4) != _u(hi_)).sum())
                stats["crossed_zero"] += int((np.signbit(l4) != np.signbit(li)).sum() + (np.signbit(h4) != np.signbit(hi_)).sum())
                if not _nudge_ok(l4, li, down=True) or not _nudge_ok(h4, hi_, down=False):
                    v.append("I5: nodes4i node %d: child 0's planes moved inwards or too far" % n)
            elif (_u(l4) != _u(li)).any() or (_u(h4) != _u(hi_)).any():
                v.append("I5: nodes4i node %d slot %d: box differs from nodes4's" % (n, si))


def _nudge_ok(old, new, down):
    old64, new64 = old.astype(np.float64), new.astype(np.float64)
    out = (new64 <= old64) if down else (new64 >= old64)
    small = np.abs(new64 - old64) <= 2.0 ** -11 * np.abs(old64)
    denorm = (np.abs(old64) < float(FLT_MIN)) & (np.abs(new64) < float(FLT_MIN))
    fin = np.isfinite(new64)
    return bool((out & (small | denorm) & fin).all())


def check_records(ex, ref, v):
    """I6: leaf_geo records restated from crt_device.h: record j of a leaf (it, n) holds triangles a = it + 2j, b = a + 1 (a again for an
    odd tail) as (v1.x a, v1.x b, v1.y a, v1.y b) (v1.z, e1.x) (e1.y, e1.z) (e2.x, e2.y) (e2.z, index of a, n - 2j); e1 = v2 - v1,
    e2 = v3 - v1 in fp32 (DeviceTriangle.cuh:27-28).  Also tri_geo, tri_nm's normals, leaf_count and the sparse copy leaf_geo_i."""
    tris = ref.tris
    v1, v2, v3 = tris["v1"].astype(np.float32), tris["v2"].astype(np.float32), tris["v3"].astype(np.float32)
    e1, e2 = (v2 - v1).astype(np.float32), (v3 - v1).astype(np.float32)
    lg = ex["leaf_geo"]
    if len(lg) != 5 * ref.n_records:
        v.append("I6: leaf_geo holds %d records, the reference leaves need %d" % (len(lg) // 5, ref.n_records))
        return
    rec_leaf = np.repeat(np.arange(ref.n_leaves), (ref.n + 1) // 2)
    j = np.arange(ref.n_records) - ref.rec_first[rec_leaf]
    a = ref.it[rec_leaf] + 2 * j
    b = np.where(2 * j + 1 < ref.n[rec_leaf], a + 1, a)
    want = np.zeros((ref.n_records, 5, 4), np.float32)
    want[:, 0] = np.stack([v1[a, 0], v1[b, 0], v1[a, 1], v1[b, 1]], -1)
    want[:, 1] = np.stack([v1[a, 2], v1[b, 2], e1[a, 0], e1[b, 0]], -1)
    want[:, 2] = np.stack([e1[a, 1], e1[b, 1], e1[a, 2], e1[b, 2]], -1)
    want[:, 3] = np.stack([e2[a, 0], e2[b, 0], e2[a, 1], e2[b, 1]], -1)
    want[:, 4, 0], want[:, 4, 1] = e2[a, 2], e2[b, 2]
    wb = _u(want)
    wb[:, 4, 2] = a.astype(np.uint32)
    wb[:, 4, 3] = (ref.n[rec_leaf] - 2 * j).astype(np.uint32)
    bad = (_u(lg).reshape(-1, 5, 4) != wb).any((1, 2))
    if bad.any():
        v.append("I6: %d leaf_geo records differ from the reference triangles (first: record %d)" % (int(bad.sum()), int(np.argmax(bad))))
    tg = ex["tri_geo"].reshape(-1, 3, 4)
    if len(tg) != len(tris):
        v.append("I6: tri_geo holds %d triangles, the scene %d" % (len(tg), len(tris)))
    else:
        wt = np.zeros_like(tg)
        wt[:, 0, :3], wt[:, 0, 3] = v1, e1[:, 0]
        wt[:, 1] = np.stack([e1[:, 1], e1[:, 2], e2[:, 0], e2[:, 1]], -1)
        wt[:, 2, 0], wt[:, 2, 1:] = e2[:, 2], tris["normal"]
        if (_u(tg) != _u(wt)).any():
            v.append("I6: tri_geo differs from the reference triangles")
    nm = ex["tri_nm"]
    if len(nm) != len(tris) or (_u(nm[:, :3]) != _u(tris["normal"].astype(np.float32))).any() \
            or ((_u(nm[:, 3]) & 0x3fffffff) != tris["material"].astype(np.uint32)).any():
        v.append("I6: tri_nm differs from the triangles' normals / materials")
    big = ref.n > 15
    if big.any() and (ex["leaf_count"][ref.it[big]] != ref.n[big]).any():
        v.append("I6: leaf_count does not hold the size of a leaf of more than 15 triangles")
    if len(ex["nodes4i"]):
        lgi, rm = ex["leaf_geo_i"].reshape(-1, 5, 4), ex["rec_map"].astype(np.int64)
        if len(rm) != ref.n_records or (rm < 0).any() or (rm >= len(lgi)).any() or len(np.unique(rm)) != len(rm):
            v.append("I6: rec_map is not a one-to-one map of the records into leaf_geo_i")
        elif (_u(lgi[rm]) != _u(lg).reshape(-1, 5, 4)).any():
            v.append("I6: leaf_geo_i[rec_map[d]] != leaf_geo[d]")


def check_trees(ex, info, ref_nodes, ref_root, tris, stats=None):
    """All invariants on every tree of an export (Render.export_trees()) with its accel_info(); returns the violations.  `stats`
    (a dict, optional) receives counts of what was seen: nudged_planes / crossed_zero (nodes4i planes that differ from nodes4's /
    whose sign does)."""
    v = []
    stats = {} if stats is None else stats
    ref = Ref(ref_nodes, ref_root, tris)
    check_records(ex, ref, v)

    def dec_bin(r):        # nodes: ~ref = it << 4 | cnt, cnt 0: leaf_count[it]
        x = ~r
        it, cnt = x >> 4, x & 15
        ok = (x >= 0) & (it < len(ref.leaf_of_it))
        lf = np.where(ok, ref.leaf_of_it[np.where(ok, it, 0)], -1)
        n = np.where(lf >= 0, ref.n[np.maximum(lf, 0)], 0)
        good = (lf >= 0) & (np.where(n <= 15, cnt == n, (cnt == 0) & (ex["leaf_count"][np.where(ok, it, 0)] == n)))
        return np.where(good, lf, -1)

    def dec_rec(r):        # nodes3 / nodes4: ~ref = the leaf's first record in leaf_geo
        return ref.leaf_of_rec(~r)

    depth2 = 0
    for rows, make, dec, root, nm, exact in ((ex["nodes"], _binary, dec_bin, ex["root_fast"], "nodes/fast", False),
                                             (ex["nodes"], _binary, dec_bin, ex["root_exact"], "nodes/exact", True),
                                             (ex["nodes3"], _binary3, dec_rec, ex["root3_fast"], "nodes3/fast", False),
                                             (ex["nodes3"], _binary3, dec_rec, ex["root3_exact"], "nodes3/exact", True)):
        if root >= 0 and len(rows) == 0:
            v.append("I1: %s: inner root but no nodes exported" % nm)
            continue
        w = make(nm, rows if len(rows) else np.zeros((4, 4), np.float32), dec, int(root))
        _, d = check_tree(w, ref, v, empty_slots=False)
        if exact:
            check_exact(w, ref, v)
        if nm.startswith("nodes/"):
            depth2 = max(depth2, d)

    # nodes4: [2a] / [2a + 1] = lo / hi of axis a of the four children, [6] = refs, [7] = refs for the decoupled-leaves step:
    # a leaf as 0x80000000 | record << 8
    n4 = int(info["n_nodes4"])
    r4 = ex["nodes4"].reshape(-1, 8, 4)
    if len(r4) != n4 + 1:
        v.append("I3: nodes4 holds %d nodes, accel_info says %d (+ the empty node)" % (len(r4), n4))
    if int(ex["empty4_off"]) != n4 * 128 or len(r4) <= n4 or not _empty_node_ok(r4[n4, :6]) \
            or (_i(r4[n4, 6:]) != EMPTY_REF).any():
        v.append("I3: nodes4: the empty node at empty4_off is not four (+inf, -inf) slots behind the tree")
    t4 = r4[:n4]
    lo4 = np.stack([t4[:, 0], t4[:, 2], t4[:, 4]], -1)
    hi4 = np.stack([t4[:, 1], t4[:, 3], t4[:, 5]], -1)
    refs6 = _i(t4[:, 6]).astype(np.int64)
    row7 = _u(t4[:, 7]).astype(np.int64)
    want7 = np.where(refs6 >= 0, refs6, 0x80000000 | (((~refs6) & 0x7fffff) << 8))
    if (row7 != want7).any():
        v.append("I1: nodes4: %d row-7 refs differ from row 6" % int((row7 != want7).sum()))
    if int(info["layout_caps"]) & 4:   # the decoupled-leaves step reads row 7: decode the leaves from there
        refs = np.where(row7 & 0x80000000, np.where(refs6 == EMPTY_REF, EMPTY_REF, ~((row7 >> 8) & 0x7fffff)), row7)
    else:
        refs = refs6
    w4 = _wide_from_refs("nodes4", lo4, hi4, refs, dec_rec, int(ex["root4"]), empty=True)
    order4, depth4 = check_tree(w4, ref, v, empty_slots=True)

    planes = [lo4[w4.kind[:n4] != 0], hi4[w4.kind[:n4] != 0]]
    has_i = len(ex["nodes4i"]) > 0
    if has_i:
        wi, mixed = decode_nodes4i(ex, ref, ex["nodes4i"], v)
        orderi, depthi = check_tree(wi, ref, v, empty_slots=True, direct=False)
        if depthi != depth4:
            v.append("I5: nodes4i depth %d, nodes4 depth %d" % (depthi, depth4))
        check_nodes4i_against_nodes4(w4, wi, mixed, v, order4, orderi, stats)
        planes += [wi.lo[wi.kind != 0], wi.hi[wi.kind != 0]]

    # I7: depths as crt_scene_layout.h counts them (root 1, the leaf level counts) and the stack they size
    if depth2 != int(info["depth2"]) or depth4 != int(info["depth4"]):
        v.append("I7: measured depths (%d, %d), accel_info (%d, %d)" % (depth2, depth4, info["depth2"], info["depth4"]))
    if int(ex["stack_cap"]) < max(depth2 + 2, 3 * depth4 + 2):
        v.append("I7: stack_cap %d < max(depth2 + 2, 3 depth4 + 2) = %d" % (ex["stack_cap"], max(depth2 + 2, 3 * depth4 + 2)))

    # I8: layout_caps against the data
    recs, caps = ref.n_records, int(info["layout_caps"])
    want = (1 if n4 <= 32768 and recs <= 32768 else 0) | (2 if n4 <= 32768 else 0) | (4 if recs <= 1 << 23 else 0) | (8 if has_i else 0)
    if caps != want:
        v.append("I8: layout_caps %#x, the data says %#x" % (caps, want))
    if has_i and (ref.n.max() > 2 or n4 > 32768):
        v.append("I8: nodes4i exists with leaves of several records or more than 32 768 nodes")

    # I9: coord_max bounds every used plane of nodes4 and nodes4i (+inf if one is not finite)
    p = np.concatenate([x.reshape(-1) for x in planes]) if planes else np.zeros(0, np.float32)
    cmax = np.float32(ex["coord_max"])
    if len(p):
        if not np.isfinite(p).all():
            if not (np.isinf(cmax) and cmax > 0):
                v.append("I9: a used plane is not finite and coord_max is %r" % float(cmax))
        elif not cmax >= np.abs(p).max():
            v.append("I9: coord_max %r < largest |plane| %r" % (float(cmax), float(np.abs(p).max())))
    return v
