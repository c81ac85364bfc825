"""Input sets and numpy restatements shared by tests/test_device_fn.py and tests/golden/make_reference_golden.py: the values at which
the device's math, short divisions, samplers and per-vertex path formulas (crt_device_fn, include/crt.h) are compared with the oracle,
with numpy float32 and with the reference's own samplers (tests/golden/reference_pin/samplers.npz).  Everything is built from fixed
seeds; floats travel as uint32 bits.  Every restatement is one IEEE operation per ufunc, float32 where the reference's text is float
and float64 exactly where Render.cuh:297-311 promotes to double."""
import functools

import numpy as np

import oracle_lib as O

F = np.float32
U = np.uint32
PI = 3.14159265358979323846
M_E = 2.71828182845904523536
RNG_BOUNCE, RNG_PROBE = 1, 3   # csrc/crt_detmath.h
BOUNCE_STACK_SIZE = 64         # Global.h:18

EDGE_WORDS = np.array([0, 1, 0x3fffffff, 0x40000000, 0x7fffffff, 0x80000000, 0x80000001, 0xc0000000, 0xffffffff], dtype=U)
EDGE_MANTISSAS = [0, 1, 2, 3, 0x3fffff, 0x400000, 0x400001, 0x7ffffe, 0x7fffff]


def fl(bits):
    return np.ascontiguousarray(bits, dtype=U).view(F)


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(U)


def same(got_bits, want_bits):
    """uint32 views equal, or both NaN (payload not compared)"""
    g, w = np.ascontiguousarray(got_bits, dtype=U), np.ascontiguousarray(want_bits, dtype=U)
    assert g.shape == w.shape, (g.shape, w.shape)
    return (g == w) | (np.isnan(g.view(F)) & np.isnan(w.view(F)))


def around(values):
    """each value with its nextafter neighbours on both sides"""
    v = np.asarray(values, dtype=F)
    return np.concatenate([np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]).astype(F)


# ------------------------------------------------------------------------------------------------ scalars
@functools.lru_cache(maxsize=None)
def whole_range():
    """X: every sign x every exponent x 512 mantissas (the nine edge ones and 503 random): 262 144 values with +-0, every denormal
    magnitude, +-inf and NaNs"""
    rng = np.random.default_rng(101)
    man = np.concatenate([EDGE_MANTISSAS, rng.integers(0, 1 << 23, 503)]).astype(U)
    e = (np.arange(256, dtype=U) << U(23))
    s = np.array([0, 0x80000000], dtype=U)
    x = fl((s[:, None, None] | e[None, :, None] | man[None, None, :]).reshape(-1))
    assert x.size == 262144
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def exp_borders():
    """-87, 88.72283905206835 and every x whose floor(1.4427 x + 0.5), in the float arithmetic of det_expf, is -126, 127 or 128"""
    lo, hi = (int(v) for v in bits(np.array([86.0, 90.0], dtype=F)))
    mag = np.arange(lo, hi + 1, dtype=U)
    x = np.concatenate([fl(mag), fl(mag | U(0x80000000))])
    zf = np.floor(F(1.44269504088896341) * x + F(0.5))
    assert zf.dtype == F
    return np.concatenate([around([-87.0, 88.72283905206835]), x[(zf == -126) | (zf == 127) | (zf == 128)]]).astype(F)


@functools.lru_cache(maxsize=None)
def scalar_set(fn):
    """X and the function's own borders with their neighbours"""
    extra = {
        "sin": around([1e30, -1e30, 8192.0, -8192.0]), "cos": around([1e30, -1e30, 8192.0, -8192.0]), "tan": around([1e30, -1e30, 8192.0, -8192.0]),
        "sincos": around([1e30, -1e30, 8192.0, -8192.0]),
        "asin": around([1, -1, 0.5, -0.5, 1e-4, -1e-4]), "acos": around([1, -1, 0.5, -0.5, 1e-4, -1e-4]),
        "atan": around([0.41421357, 2.4142137, -0.41421357, -2.4142137]),
        "log": around(np.concatenate([[2.0 ** -126], F(0.70710678) * np.exp2(np.arange(-126, 128)).astype(F)])),
    }
    extra["log10"] = extra["log"]
    e = exp_borders() if fn == "exp" else extra.get(fn, np.zeros(0, dtype=F))
    x = np.concatenate([whole_range(), e.astype(F)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def all_scalars():
    """the union of every function's set, once (the host check program evaluates every function on all of it)"""
    x = np.concatenate([whole_range()] + [scalar_set(f)[whole_range().size:] for f in ("sin", "asin", "atan", "exp", "log")])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def pair_grid():
    """atan2 / pow: a thinned X with itself, >= 500 000 pairs, both signs of zero, inf and NaN on both sides"""
    x = whole_range()
    must = fl(np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 1, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000,
                        0x80800000, 0x3f800000, 0xbf800000, 0x7f7fffff, 0xff7fffff, 0x3f000000, 0x40000000, 0x3f19999a], dtype=U))
    t = np.concatenate([must, x[181::367]])
    a, b = np.meshgrid(t, t, indexing="ij")
    a, b = a.reshape(-1).copy(), b.reshape(-1).copy()
    assert a.size >= 500000
    return a, b


@functools.lru_cache(maxsize=None)
def pow_pairs():
    """the grid, and every base of X in [0, 1] with the exponents 0.6, 1, 2, 0.25, 0, -1"""
    a, b = pair_grid()
    x = whole_range()
    base = x[(x >= 0) & (x <= 1)]
    ex = np.array([0.6, 1, 2, 0.25, 0, -1], dtype=F)
    return np.concatenate([a, np.repeat(base, ex.size)]), np.concatenate([b, np.tile(ex, base.size)])


# ------------------------------------------------------------------------------------------------ vectors by wave
def quot_guard(a, n, bounded):
    """quot3_exact's guard restated (crt_device.h): 2^-62 <= n < 2^60; every numerator zero or 2^-64 <= |a| < 2^62 (`bounded`, the form
    unit3 uses: the upper test is on the divisor alone).  a: (m, 3), n: (m,).  False for NaN anywhere."""
    a, n = np.asarray(a, dtype=F), np.asarray(n, dtype=F)
    with np.errstate(invalid="ignore"):
        aa = np.abs(a)
        ok = (n >= F(2.0 ** -62)) & (n < F(2.0 ** 60)) & np.all((aa == 0) | (aa >= F(2.0 ** -64)), axis=1)
        if not bounded:
            ok &= np.all((aa == 0) | (aa < F(2.0 ** 62)), axis=1)
    return ok


def sqnorm(a):
    """Eigen order: x x + (y y + z z)"""
    return a[:, 0] * a[:, 0] + (a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])


def dot(a, b):
    return a[:, 0] * b[:, 0] + (a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2])


def normalized(a):
    """Eigen's normalized(): z = squaredNorm; z > 0 ? v / sqrt(z) : v"""
    a = np.ascontiguousarray(a, dtype=F)
    with np.errstate(all="ignore"):
        z = sqnorm(a)
        r = np.where((z > 0)[:, None], a / np.sqrt(z)[:, None], a)
    assert r.dtype == F
    return r


def unit3_inside(a):
    """an element of unit3 takes the short quotient: z > 0 and the guard holds for the divisor sqrt(z)"""
    a = np.ascontiguousarray(a, dtype=F)
    with np.errstate(all="ignore"):
        z = sqnorm(a)
        return (z > 0) & quot_guard(a, np.sqrt(z), True)


STRETCH = 128   # two whole waves


def _log_uniform(rng, m, lo_exp, hi_exp, signed=True):
    v = (rng.uniform(1.0, 2.0, m) * np.exp2(rng.integers(lo_exp, hi_exp, m))).astype(F)
    return v * rng.choice(np.array([-1, 1], dtype=F), m) if signed else v


@functools.lru_cache(maxsize=None)
def div3_set():
    """(records (m, 4) = a.xyz, s; stretches [(name, start, stop, inside)]): 256 elements inside the guard, then per reason to be outside
    a stretch of two whole waves -- the numerator reasons once with the offender in x, in y and in z, the other two ordinary -- then a
    shuffled mix (inside None).  Every stretch starts at a multiple of 64."""
    rng = np.random.default_rng(202)
    recs, st = [], []

    def add(name, a, s, inside):
        start = sum(len(r) for r in recs)
        assert start % 64 == 0 and len(a) % 64 == 0
        recs.append(np.column_stack([a, s]).astype(F))
        st.append((name, start, start + len(a), inside))

    def ordinary(m):
        return np.column_stack([_log_uniform(rng, m, -20, 20) for _ in range(3)]), _log_uniform(rng, m, -20, 20, signed=False)

    a, s = ordinary(256)
    a[:8, 0] = [0.0, -0.0, 2.0 ** -64, -2.0 ** -64, np.nextafter(F(2.0 ** 62), F(0)), 1.0, 0.0, -0.0]
    a[6:8, 1:] = 0.0
    s[8:12] = [2.0 ** -62, np.nextafter(F(2.0 ** 60), F(0)), 1.0, 3.0]
    add("inside", a, s, True)
    a, s = ordinary(STRETCH)
    s = _log_uniform(rng, STRETCH, -149, -62, signed=False)
    s[:2] = [np.nextafter(F(2.0 ** -62), F(0)), 1e-45]
    add("divisor < 2^-62", a, s, False)
    a, s = ordinary(STRETCH)
    s = _log_uniform(rng, STRETCH, 60, 127, signed=False)
    s[:2] = [2.0 ** 60, 3.4e38]
    add("divisor >= 2^60", a, s, False)
    a, s = ordinary(STRETCH)
    s = -s
    s[:8] = [0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -2.0 ** -70, -2.0 ** 70]
    add("divisor zero / negative / non-finite", a, s, False)
    for c in range(3):
        a, s = ordinary(STRETCH)
        a[:, c] = _log_uniform(rng, STRETCH, -149, -64)
        a[:2, c] = [np.nextafter(F(2.0 ** -64), F(0)), -1e-45]
        add("numerator %s in (0, 2^-64)" % "xyz"[c], a, s, False)
    for c in range(3):
        a, s = ordinary(STRETCH)
        a[:, c] = _log_uniform(rng, STRETCH, 62, 127)
        a[:2, c] = [2.0 ** 62, -3.4e38]
        add("numerator %s >= 2^62" % "xyz"[c], a, s, False)
    for c in range(3):
        a, s = ordinary(STRETCH)
        a[:, c] = np.resize(np.array([np.inf, -np.inf, np.nan], dtype=F), STRETCH)
        add("numerator %s non-finite" % "xyz"[c], a, s, False)
    # the mix: everything above shuffled together with operands over the whole exponent range
    m = 8192
    a = np.column_stack([_log_uniform(rng, m, -80, 80) for _ in range(3)])
    s = _log_uniform(rng, m, -80, 80, signed=False)
    prev = np.concatenate(recs)
    a = np.concatenate([a, prev[:, :3]])
    s = np.concatenate([s, prev[:, 3]])
    pad = (-len(a)) % 64
    a, s = np.concatenate([a, a[:pad]]), np.concatenate([s, s[:pad]])
    p = rng.permutation(len(a))
    add("mix", a[p], s[p], None)
    r = np.concatenate(recs)
    r.setflags(write=False)
    return r, st


@functools.lru_cache(maxsize=None)
def unit3_set():
    """the same for unit3 / make_ray, whose divisor is |a| (records (m, 3)): the reasons that a vector alone can produce"""
    rng = np.random.default_rng(203)
    recs, st = [], []

    def add(name, a, inside):
        start = sum(len(r) for r in recs)
        assert start % 64 == 0 and len(a) % 64 == 0
        recs.append(np.asarray(a, dtype=F))
        st.append((name, start, start + len(a), inside))

    def ordinary(m, lo=-20, hi=20):
        return np.column_stack([_log_uniform(rng, m, lo, hi) for _ in range(3)])

    a = ordinary(256)
    a[:6] = [[1, 0, 0], [0, -1, 0], [0, 0, 1], [0.6, 0.0, -0.8], [2.0 ** -60, 0, 0], [2.0 ** 59, 2.0 ** 30, -0.0]]
    add("inside", a, True)
    a = ordinary(STRETCH, -149, -63)   # |a| < 2^-62 (denormal squares: z may be 0, then unit3 returns a)
    add("divisor < 2^-62", a, False)
    a = ordinary(STRETCH, 60, 127)     # (z overflows beyond 2^64: the divisor is +inf)
    a[:2] = [[2.0 ** 60, 0, 0], [0, 2.0 ** 60, 2.0 ** 60]]
    add("divisor >= 2^60", a, False)
    a = np.zeros((STRETCH, 3), dtype=F)
    a[1::2] = -0.0
    a[2, 0] = 1e-30   # z underflows to 0
    add("divisor zero", a, False)
    for c in range(3):
        a = ordinary(STRETCH)
        a[:, c] = _log_uniform(rng, STRETCH, -149, -64)
        a[:2, c] = [np.nextafter(F(2.0 ** -64), F(0)), -1e-45]
        add("numerator %s in (0, 2^-64)" % "xyz"[c], a, False)
    for c in range(3):
        a = ordinary(STRETCH)
        a[:, c] = np.resize(np.array([np.inf, -np.inf, np.nan], dtype=F), STRETCH)
        add("numerator %s non-finite" % "xyz"[c], a, False)
    m = 8192
    prev = np.concatenate(recs)
    a = np.concatenate([ordinary(m, -80, 80), prev])
    a = np.concatenate([a, a[:(-len(a)) % 64]])
    add("mix", a[rng.permutation(len(a))], None)
    r = np.concatenate(recs)
    r.setflags(write=False)
    return r, st


# ------------------------------------------------------------------------------------------------ normals, directions, draws, Ns
S = F(np.sqrt(0.5))


@functools.lru_cache(maxsize=None)
def random_units(n=3000, seed=301):
    rng = np.random.default_rng(seed)
    v = normalized(rng.standard_normal((n, 3)).astype(F))
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def special_vectors():
    """the six axes, the |N.x| > |N.y| ties, nearly-axis vectors, the zero vector, a NaN and an inf component, very long and very short"""
    v = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
         [S, S, 0], [S, -S, 0], [-S, S, 0], [-S, -S, 0], [S, 0, S], [0, S, S],
         [1e-20, 1, 0], [1, 1e-20, 0], [0, 0, 0], [np.nan, 0.6, 0.8], [0.6, np.inf, 0.8],
         [3e38, 0, 0], [1.7e38, 1.7e38, 1.7e38], [1e-30, 0, 0], [6e-31, 6e-31, 5e-31]]
    v = np.array(v, dtype=F)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def lobe_specials():
    """out.x on both sides of the (double)|out.x| < 1e-5 test with out.y of both signs and zero; out on the z axis; out = (-1, +-0, 0)"""
    e = F(1e-5)
    xs = [F(0), e, -e, np.nextafter(e, F(1)), -np.nextafter(e, F(1)), np.nextafter(e, F(0)), -np.nextafter(e, F(0))]
    v = [[x, y, 0.5] for x in xs for y in (0.7, -0.7, 0.0, -0.0)]
    v += [[0, 0, 1], [0, 0, -1], [0, 0, 2.5], [0, 0, -1e-3], [-1, 0.0, 0], [-1, -0.0, 0]]
    v = np.array(v, dtype=F)
    v.setflags(write=False)
    return v


def draw_words(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U)


def uniform(words):
    """curand_uniform's (0, 1] mapping as the kernels and the oracle state it"""
    return (np.asarray(words, dtype=U).astype(F) * F(2.3283064365386963e-10) + F(1.1641532182693481e-10)).astype(F)


@functools.lru_cache(maxsize=None)
def shininess():
    """Ns: a log grid 1e-3 .. 1e6, the shipped five, 0, -1, denormals, inf, NaN, and the ns at which 25 / ns crosses det_expf's cut-offs
    (88.7228 and, for negative ns, -87) with their neighbours"""
    grid = np.exp(np.linspace(np.log(1e-3), np.log(1e6), 2000)).astype(F)
    shipped = np.array([1, 100, 500, 1000, 5000], dtype=F)
    cross = []
    for lim in (88.72283905206835, -87.0):
        c = F(25) / F(lim)
        v = c
        for _ in range(3):
            v = np.nextafter(v, F(-np.inf))
        for _ in range(7):
            cross.append(v)
            v = np.nextafter(v, F(np.inf))
    border = np.array([0.0, -0.0, -1.0, 1e-45, -1e-45, 1e-39, np.inf, -np.inf, np.nan], dtype=F)
    ns = np.concatenate([grid, shipped, np.array(cross, dtype=F), border]).astype(F)
    ns.setflags(write=False)
    return ns


# ------------------------------------------------------------------------------------------------ sampler records
def _cross_words(vecs, words_a, words_b):
    """every vector with every (word_a, word_b)"""
    wa, wb = np.meshgrid(words_a, words_b, indexing="ij")
    wa, wb = wa.reshape(-1), wb.reshape(-1)
    v = np.repeat(bits(vecs), wa.size, axis=0)
    return v, np.tile(wa, len(vecs)), np.tile(wb, len(vecs))


def lobe_deltas(ns):
    """delta_theta, delta_phi of a probe at shininess ns: Render.cuh:297, :300 with Global.h:20-21 (delta_coeff * 30 * M_PI / 180: a float
    product, then double)"""
    with np.errstate(all="ignore"):
        dc = delta_coeff(ns)
        return ((dc * F(30)).astype(np.float64) * PI / 180).astype(F), ((dc * F(120)).astype(np.float64) * PI / 180).astype(F)


def delta_coeff(ns):
    with np.errstate(all="ignore"):
        e = O.math_fn("exp", F(25) / np.asarray(ns, dtype=F))          # exp(25 / ns), float (Render.cuh:297)
        return ((e - F(1)).astype(np.float64) / (M_E - 1)).astype(F)   # (float - 1) / (M_E - 1): double, narrowed by the assignment


@functools.lru_cache(maxsize=None)
def sampler_records(scale=1):
    """{"to_world": (m, 6), "sample_hemisphere": (m, 5), "sample_lobe": (m, 7)} as uint32 bits.  scale 1: the records of the committed
    fixture (what the reference's own functions were run on); larger: more random draws per vector, for the comparison with the oracle."""
    rng = np.random.default_rng(400 + scale)
    units, sp, ls = random_units(), special_vectors(), lobe_specials()
    nu = len(units)
    # to_world: a local vector per normal (random in the unit ball, then axes and zero), every special normal with a few locals
    reps = scale
    a = rng.uniform(-1, 1, (nu * reps, 3)).astype(F)
    tw = [np.column_stack([bits(a), np.tile(bits(units), (reps, 1))])]
    loc = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0], [-0.0, -0.0, -0.0], [0.3, -0.4, 0.5], [np.inf, 0, 0], [0, np.nan, 1]], dtype=F)
    tw.append(np.column_stack([np.tile(bits(loc), (len(sp), 1)), np.repeat(bits(sp), len(loc), axis=0)]))
    # sample_hemisphere: every random normal with random words (the first ones with the edge words), every special normal with every pair of edge words
    w1, w2 = draw_words(rng, nu * reps), draw_words(rng, nu * reps)
    ea, eb = np.meshgrid(EDGE_WORDS, EDGE_WORDS, indexing="ij")
    w1[:81], w2[:81] = ea.reshape(-1), eb.reshape(-1)
    sh = [np.column_stack([np.tile(bits(units), (reps, 1)), w1, w2])]
    v, wa, wb = _cross_words(sp, EDGE_WORDS, EDGE_WORDS)
    sh.append(np.column_stack([v, wa, wb]))
    # sample_lobe: random directions (not unit: the probe's `out` is a reflection) with the deltas of a shininess of the grid and random
    # words; the specials with the deltas of Ns 100 and every pair of three edge words; a few deltas that are no shininess's
    ns = shininess()
    dth, dph = lobe_deltas(ns)
    pick = rng.integers(0, len(ns), nu * reps)
    out = np.tile(units, (reps, 1)) * rng.uniform(0.5, 2.0, (nu * reps, 1)).astype(F)
    w1, w2 = draw_words(rng, nu * reps), draw_words(rng, nu * reps)
    w1[:81], w2[:81] = ea.reshape(-1), eb.reshape(-1)
    sl = [np.column_stack([bits(out), bits(dth[pick]), bits(dph[pick]), w1, w2])]
    few = EDGE_WORDS[[0, 4, 8]]
    d100 = lobe_deltas(np.array([100], dtype=F))
    for vecs in (ls, sp):
        v, wa, wb = _cross_words(vecs, few, few)
        sl.append(np.column_stack([v, np.full(len(v), bits(d100[0])[0]), np.full(len(v), bits(d100[1])[0]), wa, wb]))
    odd = np.array([[0, 0], [-0.0, 4.0], [100.0, -100.0], [np.inf, 1], [1, np.nan], [1e30, 1e-30], [2e30, 8192.0]], dtype=F)
    sl.append(np.column_stack([np.tile(bits(ls[:8]), (len(odd), 1)), np.repeat(bits(odd), 8, axis=0), np.full(8 * len(odd), EDGE_WORDS[3]), np.full(8 * len(odd), EDGE_WORDS[6])]))
    r = {"to_world": np.concatenate(tw).astype(U), "sample_hemisphere": np.concatenate(sh).astype(U), "sample_lobe": np.concatenate(sl).astype(U)}
    for a in r.values():
        a.setflags(write=False)
    return r


# ------------------------------------------------------------------------------------------------ path formulas in numpy
def clamp0(c):
    """c > 0 ? c : 0 (Render.cuh:292, :310): a NaN becomes 0"""
    with np.errstate(invalid="ignore"):
        return np.where(c > 0, c, F(0)).astype(F)


def cos_to_next(frm, to, n):
    """Render.cuh:291-292: (pre_hit.pos - pos).normalized().dot(normal), clamped"""
    with np.errstate(all="ignore"):
        return clamp0(dot(normalized(to - frm), n))


def draws(seed, pixel, k, depth, purpose):
    """the raw words of rng_draw(seed, pixel, k, depth, purpose, 0), one row per element"""
    out = np.zeros((len(pixel), 4), dtype=U)
    for i in range(len(pixel)):
        out[i] = O.rng_draw(int(seed[i]), int(pixel[i]), int(k[i]), int(depth[i]), purpose, 0)[0]
    return out


def roulette(seed, pixel, k, depth, p_rr):
    """Render.cuh:210-218: stop when the bounce stack is full (no draw, rb = 0), else when the draw's uniform exceeds P_RR"""
    rb = draws(seed, pixel, k, depth, RNG_BOUNCE)
    full = np.asarray(depth) == BOUNCE_STACK_SIZE - 1
    rb[full] = 0
    with np.errstate(invalid="ignore"):
        stop = full | (uniform(rb[:, 0]) > np.asarray(p_rr, dtype=F))
    return np.column_stack([stop.astype(U), rb])


def probe_dir(seed, pixel, k, depth, ns, arrived, n):
    """Render.cuh:297-300: the direction handed to Ray's constructor"""
    with np.errstate(all="ignore"):
        inn = normalized(arrived)                                            # :298
        out = inn - n * (F(2) * dot(inn, n))[:, None]                        # :299
        dth, dph = lobe_deltas(ns)                                           # :297, :300
        rp = draws(seed, pixel, k, depth, RNG_PROBE)
        lobe = O.fn("sample_lobe", np.column_stack([bits(out), bits(dth), bits(dph), rp[:, 0], rp[:, 1]]))
        return bits(normalized(fl(lobe)))


def probe_term(n, kd, ke, o, d, t, ns):
    """Render.cuh:306-311, evaluated eagerly, with the hit position of DeviceTriangle.cuh:50 (o + t * d)"""
    with np.errstate(all="ignore"):
        sc = (O.math_fn("log10", ns).astype(np.float64) * 0.5 + 1).astype(F)   # :306-307
        ip = F(F(2.0 * PI) / F(8))                                             # :308 (Global.h:98)
        hit = o + t[:, None] * d
        ct = cos_to_next(o, hit, n)                                            # :309-310
        return ((sc[:, None] * (ke * kd)) * ct[:, None]) * ip                  # :311


def indirect_step(L, f_r, cos_next, p_rr, L_dir):
    """Render.cuh:293, :323"""
    with np.errstate(all="ignore"):
        ind = (((L * f_r) * cos_next[:, None]) * F(2.0 * PI)) / p_rr[:, None]
        return ind + L_dir

