"""A triangle mesh rendered to a depth image from a camera, and the depth L1 of two such renderings: the 2D figure of the published mesh
evaluations (NICE-SLAM's ``eval_recon``, Co-SLAM, ESLAM: both meshes rendered from the same cameras, the mean absolute depth difference
over the pixels) and the depth image that culls by occlusion against a reference mesh (``geometry.cull_depth: reference``).  On a GPU one
view is one ``mm3dgs_mesh_depth_render`` call and one comparison one ``mm3dgs_depth_compare`` call (``csrc/meshdepth.hip``, ``MeshDepth``);
``render_host`` and ``compare_rows_host`` are the float64 numpy statement of the same rules: the yardstick of the kernels, bit for bit, and
the path of ``device: cpu``.

**Inputs.**  Vertex rows ``[V,4] int32 = {float32 x, y, z; rgba}`` and triangles ``int32 [T,3]`` (``mesh.read_surface_ply``, the extraction);
a view ``H, W, fx, fy, cx, cy`` with a world->camera pose ``[7]`` as in ``cull.py`` (``cull.check_camera``); ``near >= 0`` and ``far >= 0``
(``far = 0``: no limit).

**The rule.**  Every operation is in double from the widened float32 inputs, without contraction, in exactly this order.

* *Camera-space corner*: ``p_c[k] = R[k][0] x + R[k][1] y + R[k][2] z + t[k]``, summed left to right; ``R, t`` from
  ``pointcloud.pose_rotation`` (``rigid_from_pose`` on the device).
* *A triangle* is, first match wins, *invalid*: an index outside ``[0, V)`` or a corner with a coordinate that is not finite (tested on
  ``p_c``: with a finite pose a component of ``p_c`` is not finite exactly when a coordinate of the row is not); *behind*: no corner has
  ``z_c > near``; otherwise *drawn*.
* *Per drawn triangle* with corners a, b, c: ``n0 = b x c``, ``n1 = c x a``, ``n2 = a x b``, each component ``p q - r s`` (two products,
  one subtraction: ``(u x w).x = u.y w.z - u.z w.y``, ``.y = u.z w.x - u.x w.z``, ``.z = u.x w.y - u.y w.x``), and ``det = a.x n0.x + a.y n0.y
  + a.z n0.z``, summed left to right.
* *Per pixel* with integer centre ``(u, v)``: ``dx = (u - cx) / fx``, ``dy = (v - cy) / fy``; ``E_i = n_i.x dx + n_i.y dy + n_i.z`` and
  ``S = E0 + E1 + E2``, both summed left to right.  The pixel is *inside* when ``E0, E1, E2 >= 0 and S > 0`` or ``E0, E1, E2 <= 0 and S <
  0`` (two-sided: no back-face culling), and a *hit* when inside and ``z = det / S`` is finite, ``z > near`` and, with ``far > 0``, ``z <=
  far``.
* *Per pixel result*: the hit with the smallest double ``z``, on an exact tie the lowest triangle index: ``depth[v,u] = float32(z)``,
  rounded once, ``tri[v,u]`` that index; no hit gives ``0.0f`` and ``-1``.

This is homogeneous rasterization (the pixel's ray against the triangle's plane, from the camera-space corners): a triangle that crosses
the camera plane needs no clipping.  Along an edge shared by two triangles the two edge normals are exact negatives of each other, so a
pixel centre is never outside both: a tessellated surface has no cracks.

**The rectangle** of a drawn triangle may only ever be a superset of its hits: when all three ``z_c > 0`` and the projections ``px = fx x /
z + cx``, ``py = fy y / z + cy`` (left to right) are finite it is ``floor(min px) - 1 .. ceil(max px) + 1`` by ``floor(min py) - 1 ..
ceil(max py) + 1``, clamped to the image in double (empty when nothing is left); otherwise it is the whole image.  The kernel bins a
triangle into the 16 x 16-pixel tiles its rectangle touches; ``render_host`` evaluates a triangle on its rectangle only, and with
``full=True`` on every pixel.

**Counters** (int64 [8], accumulating over calls): [0] views, [1] drawn triangles, [2] invalid triangles, [3] triangles behind, [4] (tile,
triangle) pairs, [5] pairs dropped for lack of room, [6] hit pixels, [7] 0.  ``render_host`` fills [4] from the same rectangle rule (the
tiles every drawn triangle's rectangle touches; with ``max_pairs`` the part beyond it goes to [5]) and leaves [4] and [5] 0 with
``full=True``.

**A comparison** of two depth images a (estimate) and b (reference) ``[H,W]`` float32: a pixel is valid in an image when ``d > 0 and d <
inf`` (strict float32 tests, a NaN fails).  One row of eight float64 values: [0] n, the pixels valid in both, [1] mean ``|a - b|``, [2]
rms, [3] max, [4] pixels valid only in b, [5] only in a, [6] in neither, [7] 0; the differences in double from the widened values, the four
figures 0 when n is 0.  ``sum_order="kernel"`` adds in the device's fixed order (``geometry.kernel_order_sum`` over the pixels in raster
order, 0.0 for a pixel that is not valid in both)."""
from __future__ import annotations

import numpy as np
import torch

from . import cull as cl
from .pointcloud import as_np, pose_rotation, rows_xyz

COUNTER_NAMES = ("views", "drawn", "invalid", "behind", "pairs", "dropped", "hits", "reserved7")
ROW_NAMES = ("n", "mean", "rms", "max", "only_reference", "only_estimate", "neither", "reserved")
TILE = 16
MAX_ROWS = 1 << 30
MAX_PAIRS = 1 << 31


def check_range(near, far):
    near, far = float(near), float(far)
    for name, v in (("near", near), ("far", far)):
        if not (np.isfinite(v) and v >= 0):
            raise ValueError(f"mesh depth {name} = {v} (must be finite and not negative)")
    return near, far


def _mesh(rows, triangles):
    rows = as_np(rows, np.int32).reshape(-1, 4)
    tris = as_np(triangles, np.int32).reshape(-1, 3)
    if len(rows) > MAX_ROWS or len(tris) > MAX_ROWS:
        raise ValueError(f"mesh of {len(rows)} vertices and {len(tris)} triangles (each at most 2^30)")
    return rows, tris


def _cross(u, w):
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)


def setup_host(rows, triangles, pose, H, W, fx, fy, cx, cy, near=0.0):
    """Per triangle, by the rule of the module docstring: dict(cls int8 [T]: 0 drawn, 1 invalid, 2 behind; n float64 [T,3,3]: n0, n1, n2;
    det float64 [T]; rect int64 [T,4]: x0, y0, x1, y1 inclusive, x1 < x0 when empty or not drawn)."""
    rows, tris = _mesh(rows, triangles)
    V, T = len(rows), len(tris)
    R, t = pose_rotation(pose)
    p = rows_xyz(rows).astype(np.float64) if V else np.zeros((0, 3))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pc = np.stack([R[k, 0] * p[:, 0] + R[k, 1] * p[:, 1] + R[k, 2] * p[:, 2] + t[k] for k in range(3)], 1)
        ti = tris.astype(np.int64)
        ok = ((ti >= 0) & (ti < V)).all(1)
        safe = np.where(ok[:, None], ti, 0)
        a, b, c = (pc[safe[:, k]] if V else np.full((T, 3), np.nan) for k in range(3))
        ok &= np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1)
        front = (a[:, 2] > near) | (b[:, 2] > near) | (c[:, 2] > near)
        cls = np.where(~ok, 1, np.where(front, 0, 2)).astype(np.int8)
        n0, n1, n2 = _cross(b, c), _cross(c, a), _cross(a, b)
        det = a[:, 0] * n0[:, 0] + a[:, 1] * n0[:, 1] + a[:, 2] * n0[:, 2]
        z = np.stack([a[:, 2], b[:, 2], c[:, 2]], 1)
        px = float(fx) * np.stack([a[:, 0], b[:, 0], c[:, 0]], 1) / z + float(cx)
        py = float(fy) * np.stack([a[:, 1], b[:, 1], c[:, 1]], 1) / z + float(cy)
        tight = (z > 0).all(1) & np.isfinite(px).all(1) & np.isfinite(py).all(1)
        px, py = np.where(tight[:, None], px, 0.0), np.where(tight[:, None], py, 0.0)
        x0 = np.clip(np.floor(px.min(1)) - 1.0, 0.0, float(W))      # (clamped in double: a projection may lie beyond any integer)
        x1 = np.clip(np.ceil(px.max(1)) + 1.0, -1.0, float(W - 1))
        y0 = np.clip(np.floor(py.min(1)) - 1.0, 0.0, float(H))
        y1 = np.clip(np.ceil(py.max(1)) + 1.0, -1.0, float(H - 1))
    rect = np.stack([x0, y0, x1, y1], 1).astype(np.int64)
    rect[~tight] = (0, 0, W - 1, H - 1)
    rect[(cls != 0) | (rect[:, 0] > rect[:, 2]) | (rect[:, 1] > rect[:, 3])] = (0, 0, -1, -1)
    return {"cls": cls, "n": np.stack([n0, n1, n2], 1), "det": det, "rect": rect}


def tile_pairs(rect):
    """The (tile, triangle) pairs of the rectangles [T,4] (x1 < x0: none): the 16 x 16-pixel tiles each one touches."""
    r = np.asarray(rect, dtype=np.int64).reshape(-1, 4)
    live = r[:, 2] >= r[:, 0]
    return int((((r[:, 2] >> 4) - (r[:, 0] >> 4) + 1) * ((r[:, 3] >> 4) - (r[:, 1] >> 4) + 1))[live].sum())


def render_host(rows, triangles, pose, H, W, fx, fy, cx, cy, near=0.0, far=0.0, full=False, max_pairs=None):
    """(depth float32 [H,W], tri int32 [H,W], counters int64 [8]) of one view by the rule of the module docstring.  Each drawn triangle
    is evaluated on its rectangle; with `full` on every pixel of the image (counters [4], [5] then stay 0)."""
    H, W, fx, fy, cx, cy = cl.check_camera(H, W, fx, fy, cx, cy)
    near, far = check_range(near, far)
    s = setup_host(rows, triangles, pose, H, W, fx, fy, cx, cy, near)
    dx, dy = (np.arange(W, dtype=np.float64) - cx) / fx, (np.arange(H, dtype=np.float64) - cy) / fy
    best = np.full((H, W), np.inf)
    tri = np.full((H, W), -1, dtype=np.int32)
    for t in np.flatnonzero(s["cls"] == 0):
        x0, y0, x1, y1 = (0, 0, W - 1, H - 1) if full else s["rect"][t]
        if x1 < x0:
            continue
        n, ex, ey = s["n"][t], dx[None, x0:x1 + 1], dy[y0:y1 + 1, None]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            E0, E1, E2 = (n[i, 0] * ex + n[i, 1] * ey + n[i, 2] for i in range(3))
            S = E0 + E1 + E2
            inside = ((E0 >= 0) & (E1 >= 0) & (E2 >= 0) & (S > 0)) | ((E0 <= 0) & (E1 <= 0) & (E2 <= 0) & (S < 0))
            z = s["det"][t] / S
            hit = inside & np.isfinite(z) & (z > near)
            if far > 0:
                hit &= z <= far
        b, k = best[y0:y1 + 1, x0:x1 + 1], tri[y0:y1 + 1, x0:x1 + 1]
        win = hit & (z < b)      # (triangles come in index order: a tie keeps the lower index)
        b[win] = z[win]
        k[win] = t
    with np.errstate(over="ignore"):
        depth = np.where(tri >= 0, best, 0.0).astype(np.float32)
    need = 0 if full else tile_pairs(s["rect"])
    pairs = need if max_pairs is None else min(need, int(max_pairs))
    counters = np.array([1, int((s["cls"] == 0).sum()), int((s["cls"] == 1).sum()), int((s["cls"] == 2).sum()), pairs, need - pairs, int((tri >= 0).sum()), 0],
                        dtype=np.int64)
    return depth, tri, counters


def _valid(d):
    with np.errstate(invalid="ignore"):
        return (d > 0) & (d < np.float32(np.inf))


def compare_rows_host(a, b, sum_order="numpy"):
    """The table float64 [n,8] of the comparison of the module docstring for depth images a (estimate) and b (reference), [H,W] (n = 1)
    or [n,H,W] each.  `sum_order` "kernel": the sums in mm3dgs_depth_compare's order, so that a device table can be held to this one bit
    for bit; "numpy" (the default) differs from it in the last bits."""
    from .geometry import kernel_order_sum
    a, b = as_np(a, np.float32), as_np(b, np.float32)
    if a.shape != b.shape or a.ndim not in (2, 3):
        raise ValueError(f"depth comparison of {a.shape} against {b.shape} (two [H,W] or two [n,H,W] stacks of one shape)")
    a, b = a.reshape((-1,) + a.shape[-2:]), b.reshape((-1,) + b.shape[-2:])
    table = np.zeros((len(a), 8), dtype=np.float64)
    for row, x, y in zip(table, a, b):
        va, vb = _valid(x), _valid(y)
        both = va & vb
        d = np.abs(np.where(both, x, np.float32(0)).astype(np.float64) - np.where(both, y, np.float32(0)).astype(np.float64)).reshape(-1)
        n = int(both.sum())
        row[0], row[4], row[5], row[6] = n, int((vb & ~va).sum()), int((va & ~vb).sum()), int((~va & ~vb).sum())
        if n:
            s1, s2 = (kernel_order_sum(d), kernel_order_sum(d * d)) if sum_order == "kernel" else (d.sum(), (d * d).sum())
            row[1], row[2], row[3] = s1 / n, np.sqrt(s2 / n), d.max()
    return table


# ---- the device side -------------------------------------------------------------------------------------------------------------------
class MeshDepth:
    """The device side of one mesh: owns the vertex rows and triangles, the work buffer (the camera-space corners, the setup records, the
    tile lists with room for `max_pairs` (tile, triangle) pairs) and the eight counters.  ``render(pose)`` is one mm3dgs_mesh_depth_render
    call on the current stream: (depth float32 [H,W], tri int32 [H,W]) on the device, no read-back; ``finish()`` the one read-back, of the
    counters (int64 [8] as numpy), and raises RuntimeError when pairs were dropped for lack of room."""

    def __init__(self, rows, triangles, H, W, fx, fy, cx, cy, near=0.0, far=0.0, max_pairs=1 << 25, device="cuda:0"):
        from . import _lib
        if not str(device).startswith("cuda"):
            raise ValueError("MeshDepth needs a CUDA device (the host path is render_host)")
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = cl.check_camera(H, W, fx, fy, cx, cy)
        self.near, self.far = check_range(near, far)
        self.device, self.lib, self.max_pairs = device, _lib.load(), int(max_pairs)
        self.rows = torch.as_tensor(rows, device=device).to(torch.int32).reshape(-1, 4).contiguous()
        self.triangles = torch.as_tensor(triangles, device=device).to(torch.int32).reshape(-1, 3).contiguous()
        self.V, self.T = int(self.rows.shape[0]), int(self.triangles.shape[0])
        nbytes = int(self.lib.mm3dgs_mesh_depth_work_bytes(self.V, self.T, self.H, self.W, self.max_pairs)) if 0 <= self.max_pairs <= MAX_PAIRS else 0
        if nbytes == 0:
            raise ValueError(f"mesh depth of {self.V} vertices and {self.T} triangles with room for {self.max_pairs} pairs (at most 2^30, 2^30 and 2^31)")
        self.work = torch.empty(nbytes // 8, dtype=torch.int64, device=device)
        self.counters = torch.zeros(8, dtype=torch.int64, device=device)

    def render(self, pose, depth=None, tri=None, want_tri=True):
        from . import _lib
        from .rasterizer import _stream
        pose_c = torch.as_tensor(pose, device=self.device).detach().float().contiguous().reshape(7)
        depth = torch.empty(self.H, self.W, dtype=torch.float32, device=self.device) if depth is None else depth
        if tri is None and want_tri:
            tri = torch.empty(self.H, self.W, dtype=torch.int32, device=self.device)
        P = _lib.ptr
        _lib.check(self.lib.mm3dgs_mesh_depth_render(self.H, self.W, self.fx, self.fy, self.cx, self.cy, P(pose_c), self.near, self.far, self.V,
                                                     P(self.rows) if self.V else None, self.T, P(self.triangles) if self.T else None, self.max_pairs, P(depth),
                                                     P(tri), P(self.work), P(self.counters), _stream()))
        return depth, tri

    def finish(self):
        c = self.counters.cpu().numpy().copy()      # the one read-back
        if c[5]:
            raise RuntimeError(f"mesh depth: {int(c[5])} (tile, triangle) pairs of {int(c[4] + c[5])} over {int(c[0])} views dropped for lack of room; raise "
                               f"geometry.depth_max_pairs (now {self.max_pairs} per view)")
        return c


def compare_device(a, b, table, view):
    """Row `view` of the device table float64 [n,8] = the comparison of the device images a, b [H,W] float32: one mm3dgs_depth_compare call on
    the current stream, no read-back."""
    from . import _lib
    from .rasterizer import _stream
    lib, P = _lib.load(), _lib.ptr
    H, W = (int(v) for v in a.shape)
    work = torch.empty(int(lib.mm3dgs_depth_compare_work_bytes(H, W)) // 8, dtype=torch.int64, device=a.device)
    _lib.check(lib.mm3dgs_depth_compare(H, W, P(a), P(b), P(work), P(table[view]), _stream()))


def summarise(table, counters_estimate, counters_reference):
    """The summary of a per-view table [n,8]: views, empty_views (n = 0; left out of `mean`), mean (of the per-view means, as NICE-SLAM
    averages), the pooled mean / rmse / max, coverage = sum n / sum (n + only-reference), and both sides' counters."""
    t = np.asarray(table, dtype=np.float64).reshape(-1, 8)
    n = t[:, 0]
    scored, total = n > 0, float(n.sum())
    seen = total + float(t[:, 4].sum())
    name = lambda c: {k: int(v) for k, v in zip(COUNTER_NAMES[:7], c)}
    return {"views": int(len(t)), "empty_views": int((~scored).sum()), "mean": float(t[scored, 1].mean()) if scored.any() else 0.0,
            "pooled": float((t[:, 1] * n).sum() / total) if total else 0.0, "rmse": float(np.sqrt((t[:, 2] * t[:, 2] * n).sum() / total)) if total else 0.0,
            "max": float(t[:, 3].max()) if len(t) else 0.0, "coverage": total / seen if seen else 0.0,
            "counters": {"estimate": name(counters_estimate), "reference": name(counters_reference)}}


def depth_l1(estimate, reference, poses, H, W, cam, near=0.0, far=0.0, device="cpu", max_pairs=1 << 25, sum_order="numpy"):
    """(table float64 [n,8], summary) of the depth L1 of two meshes, each (vertex rows, triangles), over any list of world->camera poses:
    both rendered at every pose, the renderings compared view by view.  HIP on a CUDA device (one MeshDepth per mesh, one
    mm3dgs_depth_compare per view, the table and the counters read back once), the host statements otherwise (`sum_order` as in
    ``compare_rows_host``; the device adds in the kernel's order)."""
    poses = list(poses)
    if str(device).startswith("cuda"):
        kw = dict(H=H, W=W, fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], near=near, far=far, max_pairs=max_pairs, device=device)
        est, ref = MeshDepth(estimate[0], estimate[1], **kw), MeshDepth(reference[0], reference[1], **kw)
        table = torch.zeros(max(len(poses), 1), 8, dtype=torch.float64, device=device)
        a = b = None
        for k, pose in enumerate(poses):
            a, b = est.render(pose, a, want_tri=False)[0], ref.render(pose, b, want_tri=False)[0]      # (ordered on the stream: the images are reused)
            compare_device(a, b, table, k)
        ce, cr = est.finish(), ref.finish()
        t = table.cpu().numpy()[:len(poses)]
    else:
        kw = dict(H=H, W=W, fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], near=near, far=far)
        ce, cr, rows = np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64), []
        for pose in poses:
            a, _, c1 = render_host(as_np(estimate[0], np.int32), as_np(estimate[1], np.int32), pose, **kw)
            b, _, c2 = render_host(as_np(reference[0], np.int32), as_np(reference[1], np.int32), pose, **kw)
            ce, cr = ce + c1, cr + c2
            rows.append(compare_rows_host(a, b, sum_order)[0])
        t = np.stack(rows) if rows else np.zeros((0, 8))
    return t, summarise(t, ce, cr)
