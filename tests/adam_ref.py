"""Host statement of mm3dgs_adam (csrc/fused.hip: fused_adam_kernel; the element is adam_elem of csrc/mm3dgs_math.h): the float32 scalars as
include/mm3dgs.h defines them, one step in float64, derived error bars, two honest float32 evaluations, and the inputs the tests run.  numpy
(and nothing of the product): tests/test_adam_ref.py checks this file on the CPU, tests/test_gpu_adam.py holds the kernel to it.

The statement (float32 inputs and scalars, evaluated in float64):
    m* = m + (g - m) o1        v* = v b2 + g g o2        q* = sqrt(v*) / c + e        r* = m* / q*        p* = p - s r*

The bars, per element and to first order, u = 2^-24 (one float32 rounding is at most u relative):
    Bm = 3 u (|m| + |g|)                       three roundings (g - m, the product, the sum) of quantities no larger than |m| + |g|
    Bv = 4 u v*                                four roundings (g g, times o2, v b2, the sum) of non-negative terms no larger than v*
    Bp = u |p*| + |s| (Bm / q* + 8 u |r*|)     q carries 5 u relative (v*'s 4 u halved by the root, the root, the division by c, the sum),
                                               then the division, the product with s and the final subtraction
The device's division and sqrtf are the IEEE sequences (the gfx950 ISA of fused_adam_kernel shows v_div_fixup and a fixed-up v_sqrt), so
one rounding each is what they cost.  A test holds the kernel to TWICE these bounds: the factor covers the second-order terms and
whichever a * b + c the compiler contracts into one FMA (a contraction removes a rounding, it never adds one).  `worst` returns
error / (2 B), so a passing result is <= 1.  Where a bar is 0 (an element with g = m = v = 0) the result must be exact.

Every input stays in the normal float32 range (gradients 5e-9 .. 1.5e3, so g g o2 >= 2.5e-20): no decision depends on flush-to-zero."""
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15          # what the product passes: torch.optim.Adam's betas, the map's eps

Scalars = namedtuple("Scalars", "o1 b2 o2 c e s")


def scalars(step, beta1=BETA1, beta2=BETA2, eps=EPS, lr=1e-3):
    """The six float32 scalars of one call and group: each formed in double and rounded once."""
    step = float(step)
    return Scalars(o1=np.float32(1.0 - beta1), b2=np.float32(beta2), o2=np.float32(1.0 - beta2),
                   c=np.float32(np.sqrt(1.0 - beta2 ** step)), e=np.float32(eps), s=np.float32(lr / (1.0 - beta1 ** step)))


def scalars64(step, beta1=BETA1, beta2=BETA2, eps=EPS, lr=1e-3):
    """The same six in double (what torch.optim.Adam computes with on float64 tensors)."""
    step = float(step)
    return Scalars(1.0 - beta1, beta2, 1.0 - beta2, np.sqrt(1.0 - beta2 ** step), eps, lr / (1.0 - beta1 ** step))


def _f64(*a):
    return tuple(np.asarray(x, np.float64) for x in a)


def step64(p, m, v, g, sc):
    """(p*, m*, v*) in float64."""
    p, m, v, g = _f64(p, m, v, g)
    o1, b2, o2, c, e, s = (float(x) for x in sc)
    with np.errstate(invalid="ignore"):
        m1 = m + (g - m) * o1
        v1 = v * b2 + g * g * o2
        q = np.sqrt(v1) / c + e
        return p - s * (m1 / q), m1, v1


def bars(p, m, v, g, sc):
    """(Bp, Bm, Bv): the derived bounds of the module docstring (NaN where the statement is NaN)."""
    p, m, v, g = _f64(p, m, v, g)
    p1, m1, v1 = step64(p, m, v, g, sc)
    with np.errstate(invalid="ignore"):
        q = np.sqrt(v1) / float(sc.c) + float(sc.e)
        bm = 3.0 * U * (np.abs(m) + np.abs(g))
        bv = 4.0 * U * v1
        bp = U * np.abs(p1) + abs(float(sc.s)) * (bm / q + 8.0 * U * np.abs(m1 / q))
    return bp, bm, bv


def worst(got, want, bar):
    """max over the elements of |got - want| / (2 bar); inf where the statement is NaN and `got` is not (or the reverse), or where the bar
    is 0 and `got` is not exact."""
    got, want, bar = _f64(got, want, bar)
    if not got.size:
        return 0.0
    nan = np.isnan(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - want)
        ratio = np.where(bar > 0, err / (2.0 * bar), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(nan, np.where(np.isnan(got), 0.0, np.inf), np.where(np.isnan(got), np.inf, ratio))
    return float(ratio.max())


def ratios(got_p, got_m, got_v, p, m, v, g, sc):
    """(worst p, worst m, worst v) of one step's results against the statement from the state (p, m, v) and gradient g."""
    want, bar = step64(p, m, v, g, sc), bars(p, m, v, g, sc)
    return tuple(worst(a, w, b) for a, w, b in zip((got_p, got_m, got_v), want, bar))


def broken(got, want, bar):
    """The elements (bool) at which `got` misses the 2 x bar (NaN elements: never)."""
    got, want, bar = _f64(got, want, bar)
    with np.errstate(invalid="ignore"):
        return np.abs(got - want) > 2.0 * bar


# ---- float32 ----------------------------------------------------------------------------------------------------------------------
def _f32(*a):
    return tuple(np.asarray(x, np.float32) for x in a)


def step32(p, m, v, g, sc):
    """One step, operation by operation in float32 (no contraction): (p, m, v) as float32."""
    p, m, v, g = _f32(p, m, v, g)
    o1, b2, o2, c, e, s = sc
    with np.errstate(invalid="ignore"):
        m1 = m + (g - m) * o1
        v1 = v * b2 + g * g * o2
        return p - s * (m1 / (np.sqrt(v1) / c + e)), m1, v1


def _fma(a, b, c):
    """a * b + c rounded once (the float32 product is exact in float64; the sum's rounding to 53 bits before the one to 24 is the
    double rounding an evaluation through float64 has: it differs from the true FMA in about one case in 2^29)."""
    a, b, c = _f64(a, b, c)
    return (a * b + c).astype(np.float32)


def step32_fma(p, m, v, g, sc):
    """One step in float32 with every a * b + c contracted: (p, m, v) as float32."""
    p, m, v, g = _f32(p, m, v, g)
    o1, b2, o2, c, e, s = sc
    with np.errstate(invalid="ignore"):
        m1 = _fma(g - m, o1, m)
        v1 = _fma(v, b2, g * g * o2)
        return _fma(-s, m1 / (np.sqrt(v1) / c + e), p), m1, v1


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "p m v g unseen decay nan")


def make_case(n, seed):
    """n elements of Adam state and a gradient.  Every element has a gradient magnitude of its own, 10^U(-8, 3); its moments are what 0 to 5
    steps (drawn per element) of the statement leave from zero moments over gradients of that magnitude, cast to float32; parameters are
    +-10^U(-3, 1).  Hand-placed from n >= 8: element 1 unseen (g = m = v = 0), element 2 decay only (g = 0, live moments), element 5 a NaN
    gradient (its float4 neighbours 4, 6, 7 are ordinary); from n >= 64 the same three classes again at n - 1, n - 2 and n - 7 (the last
    float4, or the scalar tail)."""
    rng = np.random.default_rng(1000003 * seed + n)
    mag = 10.0 ** rng.uniform(-8.0, 3.0, n)

    def grad():
        return (mag * rng.uniform(0.5, 1.5, n) * rng.choice((-1.0, 1.0), n)).astype(np.float32)
    hist = rng.integers(0, 6, n)
    m, v = np.zeros(n), np.zeros(n)
    for t in range(5):
        _, m1, v1 = step64(np.zeros(n), m.astype(np.float32), v.astype(np.float32), grad(), scalars(t + 1))
        on = hist > t
        m, v = np.where(on, m1, m), np.where(on, v1, v)
    g = grad()
    p = (10.0 ** rng.uniform(-3.0, 1.0, n) * rng.choice((-1.0, 1.0), n)).astype(np.float32)
    m, v = m.astype(np.float32), v.astype(np.float32)
    unseen, decay, nan = [], [], []
    if n >= 8:
        unseen, decay, nan = [1], [2], [5]
    if n >= 64:
        unseen, decay, nan = unseen + [n - 1], decay + [n - 2], nan + [n - 7]
    for i in unseen:
        g[i] = m[i] = v[i] = 0.0
    for i in decay:
        g[i] = 0.0
        if v[i] == 0.0:       # (an element that drew no history: give it one step's worth)
            m[i], v[i] = np.float32(0.1 * mag[i]), np.float32(1e-3 * mag[i] * mag[i])
    for i in nan:
        g[i] = np.nan
    fin = np.isfinite(g) & (g != 0)
    tiny = np.finfo(np.float32).tiny
    assert (np.abs(g[fin]) >= 5e-9).all() and (v[v != 0] >= 1e3 * tiny).all() and (np.abs(m[m != 0]) >= 1e3 * tiny).all()
    ix = lambda a: np.asarray(a, np.int64)
    return Case(p, m, v, g, ix(unseen), ix(decay), ix(nan))


LRS = (1.6e-4, 2.5e-3, 5e-2, 1e-3, 1e-3, 1.25e-4)       # the map's six groups: xyz, f_dc, opacity, scaling, rotation, f_rest

# one group of each n, once per body: 2048 workgroups x 256 lanes x float4 = 2097152 floats is one trip of the capped grid
SIZES = (1, 3, 4, 5, 63, 64, 65, 1020, 1024, 1028, 1029, 2097152, 2097156, 2098181)


def size_case(n):
    """(Case, step, lr) of the sizes test."""
    return make_case(n, 1), 1 + n % 4, LRS[n % 6]


PATTERN_N = 1028                  # the sixteen alignment patterns
PATTERN_STEP, PATTERN_LR = 3, 2.5e-3

# the group table test: (n, words past a 16-byte boundary, lr); n = 0 entries are NULL.  The largest group (70000, scalar body: four trips
# of the 69-workgroup grid it sizes) is the fourth; 64 / 1024 / 4096 run the float4 body, 1029 (aligned) and 3 the scalar one
TABLE_GROUPS = ((64, 0, 1.6e-4), (0, 0, 1e-3), (1029, 0, 2.5e-3), (70000, 1, 5e-2), (0, 0, 1e-3), (4096, 0, 0.0), (3, 1, 1e-3), (1024, 0, 1e-3))
TABLE_STEP = 2

SHARD_P, SHARD_W, SHARD_WORLD = (257, 1000, 6001), (14, 38), (2, 3, 8)
SHARD_STEP = 4
FLAT_GROUPS = ((0, 3), (3, 6), (6, 7), (7, 10), (10, 14))       # the engine's flat layout in units of P; f_rest is (14, W)


def flat_ranges(P, W):
    """[(a, b, lr)]: the groups' element ranges in the flat layout [0, W P)."""
    cols = FLAT_GROUPS + (((14, W),) if W > 14 else ())
    return [(a * P, b * P, LRS[i]) for i, (a, b) in enumerate(cols)]


def shard_bounds(rank, world, n):
    """WindowParallel.shard_bounds restated: (S, lo, hi), S = ceil(n / world) rounded up to a multiple of 4."""
    S = (-(-n // world) + 3) // 4 * 4
    lo = min(rank * S, n)
    return S, lo, min(lo + S, n)


POSE_STEPS = (1, 2, 3, 20000)
POSE_LRS = (5e-4, 2e-3)           # cam_q_lr (elements 0:4, the float4 body), cam_t_lr (4:7, the scalar body)


def pose_case(step):
    return make_case(7, 7000 + step)


def cpu_cases():
    """(name, p, m, v, g, Scalars) of every input tests/test_gpu_adam.py feeds to mm3dgs_adam from this file -- the sizes, the pattern case,
    the table's groups, the flat arrays of the sharded step per group, the pose groups (from the built state: the device test continues
    from the device's own)."""
    for n in SIZES:
        c, step, lr = size_case(n)
        yield f"size {n}", c.p, c.m, c.v, c.g, scalars(step, lr=lr)
    c = make_case(PATTERN_N, 2)
    yield "patterns", c.p, c.m, c.v, c.g, scalars(PATTERN_STEP, lr=PATTERN_LR)
    for i, (n, _, lr) in enumerate(TABLE_GROUPS):
        if n:
            c = make_case(n, 30 + i)
            yield f"table group {i}", c.p, c.m, c.v, c.g, scalars(TABLE_STEP, lr=lr)
    for P in SHARD_P:
        for W in SHARD_W:
            c = make_case(W * P, 40)
            for a, b, lr in flat_ranges(P, W):
                yield f"shard P {P} W {W} [{a}, {b})", c.p[a:b], c.m[a:b], c.v[a:b], c.g[a:b], scalars(SHARD_STEP, lr=lr)
    for step in POSE_STEPS:
        c = pose_case(step)
        for (a, b), lr in zip(((0, 4), (4, 7)), POSE_LRS):
            yield f"pose step {step} [{a}:{b}]", c.p[a:b], c.m[a:b], c.v[a:b], c.g[a:b], scalars(step, lr=lr)
