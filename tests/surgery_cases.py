"""TEST INFRASTRUCTURE: the inputs of tests/test_gpu_surgery.py (and of tests/test_surgery_ref.py, which checks on the CPU that every
generator here leaves fewer than 1 % of its elements within surgery_ref.MARGIN of a threshold).  Seeded numpy only; float32 arrays as
the kernels read them.  `placed` marks the elements put on purpose where a drawn one must not be (NaN, exactly on a threshold): the
margin rule leaves them alone."""
import numpy as np

from tests import surgery_ref as ref

# row counts: one element, a wave and its neighbours, a workgroup and its neighbours, exactly 1024 workgroups, and 1025 (the second round
# of the 1024-wide scan of the per-workgroup counts)
SIZES = [1, 63, 64, 65, 255, 256, 257, 262144, 262145]
LARGE = 262144
MIN_OPACITY, MAX_SCALE, MAX_SCREEN = 0.005, 0.13, 100.0
MAX_GRAD, MAX_CLONE_SCALE = 0.5, 0.05
NAN = np.float32(np.nan)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


# ---- prune ------------------------------------------------------------------------------------------------------------------------
# (scale row, opacity logit, radius) placed by hand
PRUNE_PLACED = [
    ((NAN, 5.0, 0.0), 1.0, 10.0),           # a NaN scale in each position: the scale clause is false, the row stays
    ((5.0, NAN, 0.0), 1.0, 10.0),
    ((0.0, 1.0, NAN), 1.0, 10.0),
    ((NAN, NAN, NAN), 1.0, 10.0),
    ((-5.0, -5.0, -5.0), NAN, 10.0),        # a NaN opacity: the opacity clause is false, the row stays
    ((5.0, -5.0, -5.0), NAN, 10.0),         # ... but the scale clause still prunes
    ((-5.0, -5.0, -5.0), 1.0, NAN),         # a NaN radius: the screen clause is false
    ((NAN, -5.0, -5.0), -9.0, 10.0),        # a NaN scale does not shield a transparent row
    ((-5.0, -5.0, -5.0), 1.0, MAX_SCREEN),  # a radius exactly on the threshold is not larger than it
    ((-5.0, -5.0, -5.0), 1.0, float(np.nextafter(np.float32(MAX_SCREEN), np.float32(1e9)))),      # ... the next float32 is
]


def prune_rows(n, seed=0):
    """(opacity [n,1], log_scales [n,3], radii [n], placed bool [n]).  Healthy rows, with each clause firing on its own random fifth of
    them; from 63 rows on the hand-placed rows stand at rows 5.. and the (0, 1, NaN) one again in the last row."""
    g = _rng(1, n, seed)
    opacity = g.uniform(-2.0, 4.0, (n, 1)).astype(np.float32)
    scales = g.uniform(-6.0, -3.0, (n, 3)).astype(np.float32)
    radii = g.uniform(1.0, 90.0, n).astype(np.float32)
    fire = g.random((3, n)) < 0.2
    if n < 8:
        fire = np.array([[i % 4 == k for i in range(n)] for k in range(3)])
    opacity[fire[0], 0] = g.uniform(-9.0, -6.0, int(fire[0].sum())).astype(np.float32)
    scales[fire[1], g.integers(0, 3, int(fire[1].sum()))] = g.uniform(-1.5, 1.0, int(fire[1].sum())).astype(np.float32)
    radii[fire[2]] = g.uniform(110.0, 200.0, int(fire[2].sum())).astype(np.float32)
    placed = np.zeros(n, bool)
    if n >= 63:
        for k, (s, o, r) in enumerate(PRUNE_PLACED + [PRUNE_PLACED[2]]):
            i = 5 + k if k < len(PRUNE_PLACED) else n - 1
            scales[i], opacity[i, 0], radii[i], placed[i] = s, o, r, True
    return opacity, scales, radii, placed


# ---- compaction -------------------------------------------------------------------------------------------------------------------
KEEP_PATTERNS = ["all", "none", "first", "last", "alternating", "bytes", "hole", "random"]


def keep_bytes(n, pattern, seed=0):
    g = _rng(2, n, seed)
    i = np.arange(n)
    if pattern == "all":
        return np.ones(n, np.uint8)
    if pattern == "none":
        return np.zeros(n, np.uint8)
    if pattern == "first":
        return (i == 0).astype(np.uint8)
    if pattern == "last":
        return (i == n - 1).astype(np.uint8)
    if pattern == "alternating":
        return (i % 2).astype(np.uint8)
    if pattern == "bytes":          # any non-zero byte keeps
        return np.where(g.random(n) < 0.5, g.choice(np.array([0x80, 0xFF, 0x02, 0x01], np.uint8), n), 0).astype(np.uint8)
    if pattern == "hole":           # every second workgroup of 256 is empty, the others are full
        return ((i // 256) % 2 == 0).astype(np.uint8)
    assert pattern == "random"
    return (g.random(n) < 0.5).astype(np.uint8)


def row_arrays(n, widths, seed=0):
    g = _rng(3, n, seed)
    return [g.standard_normal((n, w)).astype(np.float32) for w in widths]


# ---- seeding ----------------------------------------------------------------------------------------------------------------------
SEED_SHAPES = [(1, 1), (16, 16), (15, 17), (1, 257), (257, 1), (513, 512)]       # the last: 1026 workgroups of pixels


def seed_case(H, W, seed=0):
    """dict: color [3,H,W], depth [H,W], keep uint8 [H W], pose (unnormalised quaternion), fx != fy, cx, cy."""
    g = _rng(4, H, W, seed)
    keep = (g.random(H * W) < (0.3 if H * W > 4096 else 0.6)).astype(np.uint8)
    keep[0] = keep[-1] = 1
    pose = np.array([0.9, 0.1, -0.2, 0.15, 0.3, -0.2, 0.5], np.float32)
    pose[:4] *= 1.7
    return dict(H=H, W=W, color=g.random((3, H, W)).astype(np.float32), depth=g.uniform(0.5, 4.0, (H, W)).astype(np.float32), keep=keep,
                pose=pose, fx=1.1 * W + 20.0, fy=0.9 * W + 25.0, cx=W / 2 - 0.3, cy=H / 2 + 0.2)


# ---- densification ----------------------------------------------------------------------------------------------------------------
DENSIFY_MIXES = ["none", "all_clone", "all_split", "mix", "split_last"]


def densify_rows(P, mix, seed=0, n_rest=2):
    """(arrays {group: float32 [P, width]}, grad_accum [P], denom [P], placed bool [P]).  Gradients are at least a fifth away from
    MAX_GRAD and scales at least a third away from MAX_CLONE_SCALE, except the rows placed by hand (mix `mix`, from 63 rows on)."""
    g = _rng(5, P, DENSIFY_MIXES.index(mix), seed)
    arrays = dict(xyz=g.standard_normal((P, 3)) * 3.0, f_dc=g.standard_normal((P, 3)), f_rest=g.standard_normal((P, 3 * n_rest)),
                  opacity=g.standard_normal((P, 1)), scaling=g.uniform(-6.0, -3.5, (P, 3)), rgb=g.random((P, 3)))
    q = g.standard_normal((P, 4))
    arrays["rotation"] = (q / np.linalg.norm(q, axis=1, keepdims=True)) * g.uniform(0.5, 2.0, (P, 1))      # unnormalised, never near zero
    arrays = {k: v.astype(np.float32) for k, v in arrays.items()}
    i = np.arange(P)
    if mix == "none":
        cls = np.zeros(P, int)
    elif mix == "all_clone":
        cls = np.full(P, ref.CLONE)
    elif mix == "all_split":
        cls = np.full(P, ref.SPLIT)
    elif mix == "mix":
        cls = g.integers(0, 3, P)
    else:                                   # split rows only in the last workgroup of 256 (the last row among them)
        cls = g.integers(0, 2, P)
        last = i >= 256 * ((P - 1) // 256)
        cls[last & (g.random(P) < 0.5)] = ref.SPLIT
        cls[-1] = ref.SPLIT
    denom = g.integers(1, 6, P).astype(np.float32)
    grad = np.where(cls == ref.KEEP, g.uniform(0.0, 0.4, P), g.uniform(0.6, 2.0, P))
    big = g.random(P) < 0.5                 # kept rows are large or small: the gradient alone keeps them
    wide = (cls == ref.SPLIT) | ((cls == ref.KEEP) & big)
    arrays["scaling"][wide, g.integers(0, 3, int(wide.sum()))] = g.uniform(-2.5, -1.0, int(wide.sum())).astype(np.float32)
    grad_accum = (grad * denom).astype(np.float32)
    never = (cls == ref.KEEP) & (g.random(P) < 0.2)      # rows never seen: 0 / 0
    grad_accum[never], denom[never] = 0.0, 0.0
    placed = np.zeros(P, bool)
    if mix == "mix" and P >= 63:
        hand = [((NAN, -1.0, -5.0), 1.0, 1.0),                  # selected by the gradient, NaN scale: neither clone nor split
                ((-5.0, NAN, -5.0), 0.1, 1.0),
                ((-5.0, -5.0, -5.0), MAX_GRAD, 1.0),            # a gradient exactly on the threshold is selected (>=): clone
                ((-1.0, -5.0, -5.0), 2.0 * MAX_GRAD, 4.0),      # half of MAX_GRAD after the division: a large row that stays
                ((-1.0, -5.0, -5.0), 4.0 * MAX_GRAD, 4.0),      # exactly MAX_GRAD after an exact division: split
                ((-5.0, -5.0, -5.0), 1.0, 0.0)]                 # x / 0 = inf: selected
        for k, (s, a, d) in enumerate(hand):
            arrays["scaling"][7 + k], grad_accum[7 + k], denom[7 + k], placed[7 + k] = s, a, d, True
    return arrays, grad_accum, denom, placed


def densify_moments(arrays, groups, seed=0):
    g = _rng(6, arrays["xyz"].shape[0], seed)
    return {k: (g.standard_normal(arrays[k].shape).astype(np.float32) * 1e-3, g.random(arrays[k].shape).astype(np.float32) * 1e-6) for k in groups}


# ---- covisibility -----------------------------------------------------------------------------------------------------------------
COVIS_SHAPES = [(1, 1), (15, 17), (16, 16), (1, 257), (128, 128), (113, 145)]       # 16384 pixels = the 64-workgroup grid; 16385: a second trip
COVIS_VIEWS = ["keeps_all", "loses_half", "behind"]


def covis_case(H, W, view, seed=0, plain=False):
    """dict: depth, sil [H,W], kf_pose, cur_pose, intrinsics, placed bool [H,W].  The keyframe sees a bumpy surface 1.5 - 2.5 m away.
    Unless `plain`: rows of silhouette 0.5, pixels of zero and of negative depth, and one surface point placed at the world origin (the
    keyframe's translation is that pixel's camera-space point, so p_w = R^T (x_c - t) vanishes up to rounding).
    Views: the camera steps back (every point stays inside), steps sideways by about half the frustum and a little back and down (about half the points leave; a pure side step
    would put every pixel of image row 0 on vv = 0 itself),
    steps far forward (every point behind it: zc <= 0)."""
    g = _rng(7, H, W, COVIS_VIEWS.index(view), seed)
    fx, fy, cx, cy = 1.1 * W + 20.0, 0.9 * W + 25.0, W / 2 - 0.3, H / 2 + 0.2
    depth = g.uniform(1.5, 2.5, (H, W)).astype(np.float32)
    sil = g.uniform(0.995, 1.0, (H, W)).astype(np.float32)
    placed = np.zeros((H, W), bool)
    v0, u0 = H // 2, W // 3
    z0 = float(depth[v0, u0])
    q = np.array([0.95, 0.05, -0.1, 0.08], np.float32) * np.float32(1.3)          # unnormalised
    t = np.array([(u0 - cx) / fx * z0, (v0 - cy) / fy * z0, z0], np.float32)
    if plain:
        t = t + np.float32(0.25)
    elif H * W > 1:
        sil[::5, :] = 0.5
        sil[v0, :] = 0.999
        flat = g.permutation(H * W)[:max(2, H * W // 16)]
        flat = flat[flat != v0 * W + u0]
        depth.reshape(-1)[flat[0::2]] = 0.0
        depth.reshape(-1)[flat[1::2]] = -1.0
        placed[v0, u0] = True
    delta = dict(keeps_all=(0.0, 0.0, 0.25), loses_half=(W / fx, 0.1 * H / fy, 0.1), behind=(0.0, 0.0, -6.0))[view]
    cur = np.concatenate([q * np.float32(0.8), t + np.array(delta, np.float32)]).astype(np.float32)
    return dict(H=H, W=W, depth=depth, sil=sil, kf_pose=np.concatenate([q, t]).astype(np.float32), cur_pose=cur, fx=fx, fy=fy, cx=cx, cy=cy,
                placed=placed)


def densify_run(P, mix):
    """The variation a (P, mix) run of the GPU test takes, so that every one occurs at small and at large sizes without a full cross:
    N in 1..3, f_rest two coefficients wide or of width zero, Adam state on every group or on xyz and opacity alone (the others hand NULL
    moment pointers), the parent array given or NULL.  The two large sizes use the narrow forms."""
    si, mi = SIZES.index(P), DENSIFY_MIXES.index(mix)
    large = P >= LARGE
    return dict(N=1 + (si + mi) % 3, n_rest=0 if large or si % 2 else 2,
                moment_groups=("xyz", "opacity") if large or (si + mi) % 2 else ref.GROUPS, with_parent=(si + mi) % 2 == 0)


DENSIFY_RUNS = [(P, mix, densify_run(P, mix)["N"]) for P in SIZES for mix in DENSIFY_MIXES]
DENSIFY_RUNS += [(257, mix, N) for mix in DENSIFY_MIXES for N in (1, 2, 3) if N != densify_run(257, mix)["N"]]
DENSIFY_SEED = 0x9E3779B9
