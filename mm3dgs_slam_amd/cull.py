"""Visibility culling of a point set against the views of a run: what no camera could have seen is removed from both sides of the geometry
evaluation before it is scored, as the published protocols do (NICE-SLAM's and Co-SLAM's mesh culling and their descendants) -- a
ground-truth mesh covers the whole scene, a run sees part of it.  On a GPU one view is one ``mm3dgs_cull_mark_view`` call and the selection
one ``mm3dgs_cull_select`` call (``csrc/cull.hip``, ``Culler``); ``cull_host`` is the float64 numpy statement of the same rule: the yardstick
of the kernels, bit for bit, and the path of ``device: cpu``.

**A view** is the intrinsics ``fx, fy, cx, cy`` with ``H, W``, a world->camera pose ``[7]`` (qw,qx,qy,qz,tx,ty,tz; the quaternion is
normalised here, ``pointcloud.pose_rotation``) and optionally a depth image ``[H,W]`` float32: ``(depth or None, pose)``.  Views without a
depth image test the frustum only (mode ``frustum``), views with one also test occlusion (mode ``occlusion``).

**A row** ``{float32 x, y, z; rgba}`` **is seen by a view** when all of the following hold, in this order; every operation is in double from
the widened float32 inputs, without contraction, and ``p_c[k] = R[k][0] x + R[k][1] y + R[k][2] z + t[k]`` is summed left to right, as
``tsdf_integrate_kernel`` sums it:

1. its three coordinates are finite -- a row that fails is *skipped*: it is seen by no view and counted once, at the select step;
2. ``z_c > near`` (``near >= 0``; written so that a NaN fails);
3. if ``far > 0``: ``z_c <= far``;
4. ``fu = floor(fx x_c / z_c + cx + 0.5)`` and ``fv = floor(fy y_c / z_c + cy + 0.5)`` with ``0 <= fu < W`` and ``0 <= fv < H`` (pixel
   centres at integer coordinates, the projection rule of the mesh export);
5. only when the view carries a depth image: the pixel ``d = depth[fv, fu]`` passes the point cloud's validity test without a silhouette
   (``d > 0``, ``d < inf``, ``d <= depth_max`` when ``depth_max > 0``; strict float32 tests, a NaN fails) and ``z_c <= (double)d + eps`` --
   a hole in the depth image sees nothing.

``seen[i]`` is the number of views that see row i, as a uint32.  A row is *kept* when ``seen[i] >= min_views`` (``min_views >= 1``).  Kept
rows keep their relative order; ``index[k]`` is the original row of kept row k.

**Counters** (int64 [8]): [0] views, [1] (row, view) sightings, [2] kept rows, [3] rows written = min(kept, cap), [4] kept rows dropped for
lack of room, [5] skipped rows, [6] [7] 0."""
from __future__ import annotations

import numpy as np
import torch

from .pointcloud import as_np, pose_rotation, rows_xyz, valid_mask

COUNTER_NAMES = ("views", "sightings", "kept", "written", "dropped", "skipped", "reserved6", "reserved7")
MODES = ("none", "frustum", "occlusion")
MAX_ROWS = 1 << 30


def check_options(near, far, eps, min_views):
    """(near, far, eps, min_views) as floats / int, validated as the entry points validate them."""
    near, far, eps = float(near), float(far), float(eps)
    for name, v in (("near", near), ("far", far), ("eps", eps)):
        if not (np.isfinite(v) and v >= 0):
            raise ValueError(f"cull {name} = {v} (must be finite and not negative)")
    if int(min_views) != min_views or int(min_views) < 1:
        raise ValueError(f"cull min_views = {min_views} (an integer, at least 1)")
    return near, far, eps, int(min_views)


def check_camera(H, W, fx, fy, cx, cy):
    H, W, fx, fy, cx, cy = int(H), int(W), float(fx), float(fy), float(cx), float(cy)
    if H <= 0 or W <= 0 or H * W > 1 << 28:
        raise ValueError(f"cull view of {H} x {W} (both positive, at most 2^28 pixels)")
    if not (np.isfinite([fx, fy, cx, cy]).all() and fx != 0 and fy != 0):
        raise ValueError(f"cull intrinsics fx = {fx}, fy = {fy}, cx = {cx}, cy = {cy} (finite, fx and fy not 0)")
    return H, W, fx, fy, cx, cy


def mode_of(views):
    """"occlusion" when the views carry depth images, "frustum" when none does (a mix is an error)."""
    with_depth = [d is not None for d, _ in views]
    if any(with_depth) and not all(with_depth):
        raise ValueError("cull views: either every view carries a depth image or none does")
    return "occlusion" if any(with_depth) else "frustum"


def seen_by_view_host(rows, depth, pose, H, W, fx, fy, cx, cy, near=0.0, far=0.0, eps=0.0, depth_max=0.0):
    """bool [n]: the rows one view sees, by the rule of the module docstring in float64."""
    xyz = rows_xyz(as_np(rows, np.int32).reshape(-1, 4))
    fin = np.isfinite(xyz).all(1)
    p = np.where(fin[:, None], xyz, np.float32(0)).astype(np.float64)
    R, t = pose_rotation(pose)
    x, y, z = (R[a, 0] * p[:, 0] + R[a, 1] * p[:, 1] + R[a, 2] * p[:, 2] + t[a] for a in range(3))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        hit = fin & (z > float(near))
        if float(far) > 0:
            hit &= z <= float(far)
        fu = np.floor(float(fx) * x / z + float(cx) + 0.5)
        fv = np.floor(float(fy) * y / z + float(cy) + 0.5)
        hit &= (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
    if depth is not None:
        d = as_np(depth, np.float32).reshape(H, W)
        ui, vi = np.where(hit, fu, 0).astype(np.int64), np.where(hit, fv, 0).astype(np.int64)
        dz = d[vi, ui]
        with np.errstate(invalid="ignore", over="ignore"):
            hit &= valid_mask(d, None, 0.0, depth_max)[vi, ui] & (z <= np.where(hit, dz, np.float32(0)).astype(np.float64) + float(eps))
    return hit


def cull_host(rows, views, H, W, fx, fy, cx, cy, near=0.0, far=0.0, eps=0.0, min_views=1, depth_max=0.0, cap=None):
    """(kept_rows [k,4] int32, index uint32 [k], seen uint32 [n], counters int64 [8]) of the rows [n,4] int32 against the views
    [(depth [H,W] or None, pose [7])], by the rule of the module docstring; at most `cap` kept rows are returned, the rest counted as
    dropped."""
    H, W, fx, fy, cx, cy = check_camera(H, W, fx, fy, cx, cy)
    near, far, eps, min_views = check_options(near, far, eps, min_views)
    rows = as_np(rows, np.int32).reshape(-1, 4)
    n = len(rows)
    if n > MAX_ROWS:
        raise ValueError(f"cull of {n} rows (at most 2^30)")
    views = list(views)
    mode_of(views)
    seen = np.zeros(n, dtype=np.uint32)
    for depth, pose in views:
        seen += seen_by_view_host(rows, depth, pose, H, W, fx, fy, cx, cy, near, far, eps, depth_max).astype(np.uint32)
    fin = np.isfinite(rows_xyz(rows)).all(1)
    index = np.flatnonzero(fin & (seen >= min_views)).astype(np.uint32)
    kept = len(index)
    written = kept if cap is None else min(kept, int(cap))
    counters = np.array([len(views), int(seen.sum(dtype=np.uint64)), kept, written, kept - written, int((~fin).sum()), 0, 0], dtype=np.int64)
    index = index[:written]
    return rows[index.astype(np.int64)].copy(), index, seen, counters


class Culler:
    """The device side of one point set: owns ``seen`` (uint32 per row, as int32 storage), the eight counters and the work buffer.
    ``add_view(depth or None, pose)`` is one mm3dgs_cull_mark_view call on the current stream; ``finish()`` one mm3dgs_cull_select call and
    the one read-back, of the counters: (kept rows [k,4] int32, index [k] int32 storage of uint32, counters int64 [8] as numpy), tensors on
    the device."""

    def __init__(self, rows, H, W, fx, fy, cx, cy, near=0.0, far=0.0, eps=0.0, min_views=1, depth_max=0.0, device="cuda:0"):
        from . import _lib
        if not str(device).startswith("cuda"):
            raise ValueError("Culler needs a CUDA device (the host path is cull_host)")
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = check_camera(H, W, fx, fy, cx, cy)
        self.near, self.far, self.eps, self.min_views = check_options(near, far, eps, min_views)
        self.depth_max, self.device = float(depth_max), device
        self.lib = _lib.load()
        self.rows = torch.as_tensor(rows, device=device).to(torch.int32).reshape(-1, 4).contiguous()
        self.n = int(self.rows.shape[0])
        nbytes = int(self.lib.mm3dgs_cull_work_bytes(self.n))
        if nbytes == 0:
            raise ValueError(f"cull of {self.n} rows (at most 2^30)")
        self.seen = torch.zeros(max(self.n, 1), dtype=torch.int32, device=device)
        self.counters = torch.zeros(8, dtype=torch.int64, device=device)
        self.work = torch.empty(nbytes // 8, dtype=torch.int64, device=device)
        self.with_depth = None

    def add_view(self, depth, pose):
        from . import _lib
        from .rasterizer import _stream
        if self.with_depth is not None and self.with_depth != (depth is not None):
            raise ValueError("cull views: either every view carries a depth image or none does")
        self.with_depth = depth is not None
        prep = lambda t: torch.as_tensor(t, device=self.device).detach().float().contiguous()
        pose_c = prep(pose).reshape(7)
        depth_c = None
        if depth is not None:
            depth_c = prep(depth)
            if tuple(depth_c.shape) != (self.H, self.W):
                raise ValueError(f"Culler.add_view: depth [{self.H},{self.W}]; got {tuple(depth_c.shape)}")
        P = _lib.ptr
        _lib.check(self.lib.mm3dgs_cull_mark_view(self.H, self.W, self.fx, self.fy, self.cx, self.cy, P(pose_c), P(depth_c), self.depth_max, self.near, self.far,
                                                  self.eps, self.n, P(self.rows), P(self.seen), P(self.counters), _stream()))

    def finish(self, cap=None):
        from . import _lib
        from .rasterizer import _stream
        P = _lib.ptr
        cap = self.n if cap is None else int(cap)
        out = torch.empty(max(cap, 1), 4, dtype=torch.int32, device=self.device)
        index = torch.empty(max(cap, 1), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.mm3dgs_cull_select(self.n, P(self.rows), P(self.seen), self.min_views, P(out), cap, P(index), P(self.work), P(self.counters), _stream()))
        c = self.counters.cpu().numpy().copy()      # the one read-back
        written = int(c[3])
        return out[:written], index[:written], c


# ---- the geometry evaluation's argument -----------------------------------------------------------------------------------------------
def spec(views, H, W, cam, near=0.0, far=0.0, eps=0.0, min_views=1, depth_max=0.0):
    """The ``cull=`` argument of ``geometry.compare``: the views [(depth or None, pose)] plus the options, validated."""
    views = list(views)
    H, W, fx, fy, cx, cy = check_camera(H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    near, far, eps, min_views = check_options(near, far, eps, min_views)
    return {"views": views, "mode": mode_of(views), "H": H, "W": W, "fx": fx, "fy": fy, "cx": cx, "cy": cy, "near": near, "far": far, "eps": eps,
            "min_views": min_views, "depth_max": float(depth_max)}


def _camera_and_options(s):
    return dict(H=s["H"], W=s["W"], fx=s["fx"], fy=s["fy"], cx=s["cx"], cy=s["cy"], near=s["near"], far=s["far"], eps=s["eps"], min_views=s["min_views"],
                depth_max=s["depth_max"])


def side_counts(n, counters):
    return {"rows": int(n), "kept": int(counters[2]), "skipped": int(counters[5]), "sightings": int(counters[1])}


def apply_host(rows, s):
    """(kept rows, index, counts) of one side of a comparison on the host."""
    kept, index, _, c = cull_host(rows, s["views"], **_camera_and_options(s))
    return kept, index, side_counts(len(rows), c)


def device_views(s, device):
    """The views of a spec as device tensors, made once for both sides."""
    on = lambda t: None if t is None else torch.as_tensor(t, device=device).detach().float().contiguous()
    return [(on(d), on(p)) for d, p in s["views"]]


def apply_device(rows, s, views, device):
    """(kept rows, index, counts) of one side on the device; `views`: ``device_views(s, device)``."""
    c = Culler(rows, device=device, **_camera_and_options(s))
    for depth, pose in views:
        c.add_view(depth, pose)
    kept, index, counters = c.finish()
    return kept, index, side_counts(c.n, counters)


def summary(s, estimate, reference):
    """The ``cull`` entry of a comparison and block of metrics.json."""
    return {"mode": s["mode"], "eps": s["eps"], "near": s["near"], "far": s["far"], "min_views": s["min_views"], "depth_max": s["depth_max"],
            "views": len(s["views"]), "estimate": estimate, "reference": reference}
