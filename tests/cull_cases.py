"""Inputs of the culling tests (tests/test_cull.py on the host, tests/test_gpu_cull.py on the device): analytic scenes whose answer is known
by construction, random scenes that straddle the frustum, and the set shapes (all kept, none kept, only skipped, empty).

Why equality, and why no case can flip.  ``cull.cull_host`` and ``cull_mark_kernel`` perform the same sequence of IEEE-754 double operations
on the same widened float32 inputs: the quaternion's four squares, their sum left to right and one square root, four divisions, the
rotation's products and sums as written, per row three products and three sums per camera axis, one product, one division and two sums per
pixel coordinate, floor, and comparisons; with a depth image one widening and one sum.  Multiplication, addition, division and square
root are correctly rounded on both sides and neither side contracts a product into a sum (numpy has separate ufuncs, the kernel is
compiled with contraction off), so every intermediate is the same double and every comparison sees the same two numbers -- a point placed
exactly on a bound, or one ulp beside it, lands on the same side on both.  The float32 tests of the depth pixel compare inputs, not
computed values.  The analytic scenes use an identity pose (R = I and t = 0 exactly, so p_c is the point itself) and powers of two or
small dyadic numbers, so the quantity under test is exact and its distance to the bound is the one stated; each scene asserts that.

A scene is a dict: H, W, fx, fy, cx, cy, near, far, eps, depth_max, views [(depth or None, pose)], rows [n,4] int32 and, for the analytic
ones, want_frustum / want_occlusion (bool [n]: seen by the one view) and why (one string per row)."""
import numpy as np

IDENTITY = np.array([1, 0, 0, 0, 0, 0, 0], dtype=np.float32)
SIZES = (1, 255, 256, 257, 1000)
SECOND_ROUND = 262145      # 1025 blocks of 256: the second round of the 1024-wide scan


def rows_of(xyz, rgba=None):
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    rows = np.empty((len(xyz), 4), dtype=np.int32)
    rows[:, :3] = xyz.view(np.int32)
    rows[:, 3] = (np.arange(len(xyz), dtype=np.uint32) * np.uint32(2654435761) | np.uint32(0xff000000)).view(np.int32) if rgba is None else rgba
    return rows


def frustum_only(scene):
    """The scene with its depth images removed (mode frustum)."""
    return dict(scene, views=[(None, p) for _, p in scene["views"]])


def options(scene):
    return {k: scene[k] for k in ("H", "W", "fx", "fy", "cx", "cy", "near", "far", "eps", "depth_max")}


def _analytic(name, K, near, far, eps, depth, depth_max, table):
    xyz = [t[0] for t in table]
    return dict(name=name, H=12, W=16, fx=K[0], fy=K[1], cx=K[2], cy=K[3], near=near, far=far, eps=eps, depth_max=depth_max,
                views=[(depth, IDENTITY.copy())], rows=rows_of(xyz), want_frustum=np.array([t[1] for t in table], dtype=bool),
                want_occlusion=np.array([t[2] for t in table], dtype=bool), why=[t[3] for t in table])


def _depth_image():
    """12 x 16, 2.0 everywhere; (v 0, u 3) = 4.0; row v = 1: u 7 = 0, u 8 = NaN, u 9 = +Inf, u 10 = 10.0 (above depth_max = 8)."""
    d = np.full((12, 16), 2.0, dtype=np.float32)
    d[0, 3] = 4.0
    d[1, 7], d[1, 8], d[1, 9], d[1, 10] = 0.0, np.nan, np.inf, 10.0
    return d


def exact_scene():
    """fx = fy = 1, cx = cy = 0, near 0.5, far 4, eps 0.25: every quantity under test sits exactly ON its bound."""
    nan, inf = float("nan"), float("inf")
    table = [
        ((-0.5, 0.0, 1.0), True, True, "fx x / z + cx = -0.5 exactly: floor(0) = 0, inside; z = 1 <= 2 + 0.25"),
        ((15.5, 0.0, 1.0), False, False, "fx x / z + cx = W - 0.5 exactly: floor(16) = 16, outside"),
        ((0.0, -0.5, 1.0), True, True, "fy y / z + cy = -0.5 exactly: inside"),
        ((0.0, 11.5, 1.0), False, False, "fy y / z + cy = H - 0.5 exactly: outside"),
        ((0.0, 0.0, 0.5), False, False, "z_c = near exactly: z_c > near fails"),
        ((12.0, 0.0, 4.0), True, True, "z_c = far exactly: z_c <= far holds; pixel (0, 3) holds 4.0"),
        ((11.25, 0.0, 2.25), True, True, "z_c = d + eps = 2.25 exactly at pixel (0, 5): seen"),
        ((0.0, 0.0, -1.0), False, False, "behind the camera"),
        ((0.0, 0.0, 0.0), False, False, "z_c = 0: in the camera plane"),
        ((nan, 0.0, 1.0), False, False, "NaN coordinate: skipped"),
        ((0.0, inf, 1.0), False, False, "+Inf coordinate: skipped"),
        ((0.0, 0.0, -inf), False, False, "-Inf coordinate: skipped"),
        ((7.0, 1.0, 1.0), True, False, "depth pixel 0: a hole sees nothing"),
        ((8.0, 1.0, 1.0), True, False, "depth pixel NaN"),
        ((9.0, 1.0, 1.0), True, False, "depth pixel +Inf"),
        ((10.0, 1.0, 1.0), True, False, "depth pixel 10 above depth_max 8"),
        ((2.0, 2.0, 1.0), True, True, "plainly inside, in front of the surface"),
        ((6.0, 6.0, 3.0), True, False, "inside the frustum, 0.75 behind the surface of 2.0"),
    ]
    return _analytic("on the bounds", (1.0, 1.0, 0.0, 0.0), 0.5, 4.0, 0.25, _depth_image(), 8.0, table)


def ulp_scene():
    """The same points one ulp on the other side of each bound.  The rows are float32, so the ulp comes from the double parameters:
    fx = 1 - 2^-53 and cx = -1.5 2^-53 put x = -0.5 at -0.5 - 2^-53 (the next double below -0.5) and x = 15.5 at 15.5 - 2^-49 (the next
    below 15.5); near and far are the next doubles below 0.5 and 4, so z_c = 0.5 and z_c = 4 are the next doubles above them; eps = 0.25 -
    2^-51 makes d + eps = 2.25 - 2^-51, so z_c = 2.25 is the next double above it."""
    fx, cx = 1.0 - 2.0 ** -53, -1.5 * 2.0 ** -53
    near, far, eps = float(np.nextafter(0.5, 0.0)), float(np.nextafter(4.0, 0.0)), 0.25 - 2.0 ** -51
    # the claims of the docstring, in the statement's own operation order
    assert fx * -0.5 / 1.0 + cx == np.nextafter(-0.5, -np.inf) and fx * 15.5 / 1.0 + cx == np.nextafter(15.5, 0.0)
    assert np.nextafter(near, np.inf) == 0.5 and np.nextafter(far, np.inf) == 4.0 and np.nextafter(2.0 + eps, np.inf) == 2.25
    table = [
        ((-0.5, 0.0, 1.0), False, False, "fx x / z + cx = the next double below -0.5: floor(-2^-53) = -1, outside"),
        ((15.5, 0.0, 1.0), True, True, "fx x / z + cx = the next double below W - 0.5: floor(16 - 2^-49) = 15, inside"),
        ((0.0, 0.0, 0.5), True, True, "z_c = the next double above near: inside"),
        ((12.0, 0.0, 4.0), False, False, "z_c = the next double above far: outside"),
        ((11.25, 0.0, 2.25), True, False, "z_c = the next double above d + eps: not seen"),
    ]
    return _analytic("one ulp beside the bounds", (fx, 1.0, cx, 0.0), near, far, eps, _depth_image(), 8.0, table)


def analytic_scenes():
    return [exact_scene(), ulp_scene()]


def _poses(n_views, rng):
    """World->camera poses near the identity: a rotation of up to about 20 degrees, a translation of up to 0.5, the quaternion not normalised."""
    out = []
    for _ in range(n_views):
        q = np.array([1.0, 0, 0, 0]) + rng.uniform(-0.18, 0.18, 4) * np.array([0.3, 1, 1, 1])
        out.append(np.concatenate([q * rng.uniform(0.7, 1.4), rng.uniform(-0.5, 0.5, 3)]).astype(np.float32))
    return out


def _depth(H, W, rng):
    """A wavy surface between 1.5 and 4.5 with a tenth of the pixels holes (0, NaN, Inf) or beyond depth_max."""
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = (3.0 + 1.5 * np.sin(u * 0.9 + rng.uniform(0, 6)) * np.cos(v * 0.7 + rng.uniform(0, 6))).astype(np.float32)
    holes = rng.uniform(size=(H, W))
    d[holes < 0.025] = 0.0
    d[(holes >= 0.025) & (holes < 0.05)] = np.nan
    d[(holes >= 0.05) & (holes < 0.075)] = np.inf
    d[(holes >= 0.075) & (holes < 0.1)] = 9.0
    return d


def random_scene(n, H=12, W=16, n_views=3, seed=0, analytic_rows=True):
    """n rows, about half of them inside some frustum: uniform in a box around the viewing cone of the poses of `_poses` (focal length W,
    so the cone's half-width at depth z is z / 2), with the analytic scenes' rows and not-finite rows mixed in while they fit."""
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-2.5, 2.5, n), rng.uniform(-1.0, 6.5, n)], 1).astype(np.float32)
    if analytic_rows:
        extra = np.concatenate([s["rows"][:, :3].view(np.float32) for s in analytic_scenes()])
        k = min(len(extra), n // 4)
        xyz[rng.choice(n, k, replace=False)] = extra[:k]
    views = [(_depth(H, W, rng), p) for p in _poses(n_views, rng)]
    return dict(name=f"random {n} rows, {n_views} view(s), {H} x {W}", H=H, W=W, fx=float(W), fy=float(W), cx=0.5 * (W - 1), cy=0.5 * (H - 1), near=0.25,
                far=6.0, eps=0.05, depth_max=8.0, views=views, rows=rows_of(xyz))


def shape_scenes():
    """all kept / none kept / only skipped rows / no row, one identity-pose view of 12 x 16 (fx = fy = 16, the principal point in the middle)."""
    base = dict(H=12, W=16, fx=16.0, fy=16.0, cx=7.5, cy=5.5, near=0.0, far=0.0, eps=0.0, depth_max=0.0, views=[(None, IDENTITY.copy())])
    rng = np.random.default_rng(5)
    front = np.stack([rng.uniform(-0.2, 0.2, 300), rng.uniform(-0.2, 0.2, 300), rng.uniform(1.0, 2.0, 300)], 1)
    return [dict(base, name="all kept", rows=rows_of(front), kept=300, skipped=0),
            dict(base, name="none kept", rows=rows_of(front * np.array([1, 1, -1.0])), kept=0, skipped=0),
            dict(base, name="only skipped rows", rows=rows_of(np.full((300, 3), np.nan)), kept=0, skipped=300),
            dict(base, name="no row", rows=np.zeros((0, 4), dtype=np.int32), kept=0, skipped=0)]


def brute_force(scene, min_views=1):
    """(seen uint32 [n], index uint32 [k], counters int64 [8]) by a loop over the points with Python / numpy float64 scalars: an independent
    statement of the rule of cull.py's docstring (its own quaternion -> rotation, its own projection)."""
    H, W = scene["H"], scene["W"]
    fx, fy, cx, cy = (np.float64(scene[k]) for k in ("fx", "fy", "cx", "cy"))
    near, far, eps, dmax = np.float64(scene["near"]), np.float64(scene["far"]), np.float64(scene["eps"]), np.float32(scene["depth_max"])
    xyz = np.ascontiguousarray(scene["rows"][:, :3]).view(np.float32)
    seen = np.zeros(len(xyz), dtype=np.uint32)
    finite = np.zeros(len(xyz), dtype=bool)
    cams = []
    for depth, pose in scene["views"]:
        w, x, y, z = (np.float64(v) for v in np.asarray(pose, dtype=np.float32)[:4])
        nrm = np.sqrt(w * w + x * x + y * y + z * z)
        w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
        R = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
             [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
             [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]
        cams.append((depth, R, [np.float64(v) for v in np.asarray(pose, dtype=np.float32)[4:]]))
    with np.errstate(all="ignore"):
        for i, p in enumerate(xyz):
            if not (np.isfinite(p[0]) and np.isfinite(p[1]) and np.isfinite(p[2])):
                continue
            finite[i] = True
            px, py, pz = np.float64(p[0]), np.float64(p[1]), np.float64(p[2])
            for depth, R, t in cams:
                c = [R[k][0] * px + R[k][1] * py + R[k][2] * pz + t[k] for k in range(3)]
                if not c[2] > near:
                    continue
                if far > 0 and not c[2] <= far:
                    continue
                fu, fv = np.floor(fx * c[0] / c[2] + cx + 0.5), np.floor(fy * c[1] / c[2] + cy + 0.5)
                if not (0 <= fu < W and 0 <= fv < H):
                    continue
                if depth is not None:
                    d = np.float32(depth[int(fv), int(fu)])
                    if not (d > np.float32(0) and d < np.float32(np.inf) and (not dmax > 0 or d <= dmax)):
                        continue
                    if not c[2] <= np.float64(d) + eps:
                        continue
                seen[i] += 1
    index = np.flatnonzero(finite & (seen >= min_views)).astype(np.uint32)
    counters = np.array([len(cams), int(seen.sum()), len(index), len(index), 0, int((~finite).sum()), 0, 0], dtype=np.int64)
    return seen, index, counters
