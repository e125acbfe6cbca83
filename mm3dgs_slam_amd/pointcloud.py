"""The reconstruction as a fused coloured point cloud (the computational core of the reference's ``scripts/visualizer.py``): the RGB-D
image of every exported view -- the map rendered at the estimated pose, or the frame itself -- is lifted pixel by pixel to world points
(``rgbd2pcd``, ``visualizer.py:69-112``), and of all the points that fall into one voxel the first in stream order (view, then raster) is
kept.  The cloud goes to a binary PLY file that MeshLab, CloudCompare or any PLY reader opens (``float x y z; uchar red green blue
alpha``), the camera path to a second one (vertices = camera centres, one ``edge`` element joining consecutive poses, the reference's
``cool`` colour ramp, ``visualizer.py:188-201``).  The interactive window, open3d and matplotlib stay out of scope.

A row is 16 bytes, ``{float32 x, y, z; uint32 rgba}`` (red in the low byte), held as ``[n,4] int32``.  On a GPU one view is one
``mm3dgs_pointcloud_add_view`` call (``csrc/pointcloud.hip``, ``PointCloudBuilder``); ``backproject_host`` / ``voxel_select_host`` are the
float64 statement of the same rules: the yardstick of the kernels and the path of ``device: cpu`` (``HostPointCloudBuilder``)."""
from __future__ import annotations

import numpy as np
import torch

COUNTER_NAMES = ("rows", "valid", "merged", "out_of_range", "probe_fail", "capacity_dropped", "views")
CELL_LIMIT = 1 << 20      # cells on either side of the origin per axis


def as_np(t, dtype):
    """A tensor (any device) or array as a contiguous numpy array of `dtype`; None stays None."""
    if t is None:
        return None
    return np.ascontiguousarray((t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(dtype, copy=False))


def pose_rotation(pose):
    """(R, t) of the world->camera 7-vector (qw,qx,qy,qz,tx,ty,tz) in float64; the quaternion is normalised here."""
    p = as_np(pose, np.float32).astype(np.float64).reshape(7)
    w, x, y, z = p[:4] / np.sqrt((p[:4] * p[:4]).sum())
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return R, p[4:]


def quantise_colour(c):
    """uint8 of a float32 channel: (uint8)(min(max(c, 0), 1) * 255.0f + 0.5f) in float32, NaN -> 0."""
    c = np.asarray(c, dtype=np.float32)
    c = np.where(c > 0, c, np.float32(0))
    c = np.where(c < 1, c, np.float32(1)).astype(np.float32)
    return (c * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)


def valid_mask(depth, sil, sil_min, depth_max):
    """The valid pixels [H,W]: strict float32 comparisons on the inputs, a NaN fails."""
    d = as_np(depth, np.float32)
    with np.errstate(invalid="ignore"):
        ok = (d > 0) & (d < np.float32(np.inf))
        if float(np.float32(depth_max)) > 0:
            ok &= d <= np.float32(depth_max)
        if sil is not None:
            ok &= as_np(sil, np.float32) > np.float32(sil_min)
    return ok


def backproject_host(color, depth, sil, pose, fx, fy, cx, cy, sil_min=0.0, depth_max=0.0, full=False):
    """One view in float64: color [3,H,W], depth [H,W], sil [H,W] or None, pose 7 floats (world->camera).  The valid pixels in raster
    order as rows [n,4] int32 = {float32 x, y, z bits; rgba}: p_c = ((u - cx) / fx z, (v - cy) / fy z, z) with integer pixel indices,
    p_w = R^T (p_c - t), rounded once to float32; the colour rule of ``quantise_colour``, alpha 255.  With ``full`` also the float64
    positions [n,3], scale = |R|^T (|p_c| + |t|) componentwise (what a float32 evaluation's error is measured against) and the pixel
    indices [n]."""
    col = as_np(color, np.float32)
    d = as_np(depth, np.float32)
    H, W = d.shape
    idx = np.flatnonzero(valid_mask(d, sil, sil_min, depth_max).reshape(-1))
    z = d.reshape(-1)[idx].astype(np.float64)
    u, v = (idx % W).astype(np.float64), (idx // W).astype(np.float64)
    R, t = pose_rotation(pose)
    pc = np.stack([(u - float(cx)) / float(fx) * z, (v - float(cy)) / float(fy) * z, z], 1)
    xyz = (pc - t) @ R                                   # rows: R^T (p_c - t)
    rows = np.empty((len(idx), 4), dtype=np.int32)
    rows[:, :3] = xyz.astype(np.float32).view(np.int32)
    q = quantise_colour(col.reshape(3, -1)[:, idx]).astype(np.uint32)
    rows[:, 3] = (q[0] | (q[1] << 8) | (q[2] << 16) | np.uint32(0xff000000)).view(np.int32)
    if not full:
        return rows
    scale = (np.abs(pc) + np.abs(t)) @ np.abs(R)
    return rows, xyz, scale, idx


def rows_xyz(rows):
    """The float32 positions [n,3] of rows [n,4] int32."""
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32)[:, :3]).view(np.float32)


def rows_rgba(rows):
    """The colour bytes [n,4] (r, g, b, a) of rows [n,4] int32."""
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32)[:, 3:4]).view(np.uint8)


def voxel_keys(xyz_f32, voxel):
    """(keys int64 [n], in_range bool [n]): cell = floor((double)x_f32 / voxel) per axis; out of range when some |cell| >= 2^20 or the
    position is not a number; with the cells (i, j, k): key = (i + 2^20) << 42 | (j + 2^20) << 21 | (k + 2^20)."""
    x = np.asarray(xyz_f32, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor(x / float(voxel))
        ok = (np.abs(c) < CELL_LIMIT).all(1)
    ci = np.where(ok[:, None], c, 0.0).astype(np.int64) + CELL_LIMIT
    return (ci[:, 0] << 42) | (ci[:, 1] << 21) | ci[:, 2], ok


def voxel_select_host(xyz_f32, voxel, seen=None):
    """Indices (ascending) of the points that are the first to reach their voxel: first occurrence of every in-range key that is not in
    ``seen``; ``seen`` (a set, updated in place) carries the keys across views."""
    keys, ok = voxel_keys(xyz_f32, voxel)
    idx = np.flatnonzero(ok)
    uniq, first = np.unique(keys[idx], return_index=True)
    if seen is not None:
        fresh = np.fromiter((int(k) not in seen for k in uniq), dtype=bool, count=len(uniq))
        seen.update(int(k) for k in uniq[fresh])
        first = first[fresh]
    return np.sort(idx[first])


def _counters_dict(c):
    out = {name: int(c[k]) for k, name in enumerate(COUNTER_NAMES)}
    assert out["valid"] == out["rows"] + out["merged"] + out["out_of_range"] + out["probe_fail"] + out["capacity_dropped"], out
    return out


def _overflow_error(c):
    return RuntimeError(f"point cloud export dropped points: {c['capacity_dropped']} did not fit into pointcloud.max_points rows and "
                        f"{c['probe_fail']} found no slot in the voxel table (sized from pointcloud.max_points); raise "
                        f"pointcloud.max_points or pointcloud.voxel")


class HostPointCloudBuilder:
    """The builder of ``device: cpu``: the host statement, view by view."""

    def __init__(self, H, W, cam, voxel=0.01, max_points=1 << 24, sil_min=0.99, depth_max=0.0, device=None):
        self.H, self.W, self.cam = int(H), int(W), cam
        self.voxel, self.cap, self.sil_min, self.depth_max = float(voxel), int(max_points), float(sil_min), float(depth_max)
        self.seen, self.parts, self.c = set(), [], [0] * 8

    def add(self, color, depth, sil, pose):
        rows = backproject_host(color, depth, sil, pose, self.cam["fx"], self.cam["fy"], self.cam["cx"], self.cam["cy"], self.sil_min, self.depth_max)
        n_valid, n_oor = len(rows), 0
        if self.voxel > 0:
            n_oor = int((~voxel_keys(rows_xyz(rows), self.voxel)[1]).sum())
            rows = rows[voxel_select_host(rows_xyz(rows), self.voxel, self.seen)]
        keep = min(len(rows), self.cap - self.c[0])
        self.parts.append(rows[:keep])
        c = self.c
        c[0] += keep; c[1] += n_valid; c[2] += n_valid - n_oor - len(rows); c[3] += n_oor; c[5] += len(rows) - keep; c[6] += 1

    def finish(self):
        c = _counters_dict(self.c)
        if c["probe_fail"] or c["capacity_dropped"]:
            raise _overflow_error(c)
        return c

    def rows(self):
        return np.concatenate(self.parts) if self.parts else np.empty((0, 4), dtype=np.int32)


def device_view(who, H, W, color, depth, sil, pose, method="add"):
    """One view as the device builders (`who`: PointCloudBuilder, TsdfVolume, SparseTsdfVolume; `method`: the one that was called) take it:
    device tensors color [3,H,W] (None where the method reads none), depth and sil (or None) [H,W], pose 7 values, returned as contiguous
    float32 (color, depth, sil, pose [7]); such a tensor is not copied."""
    shape = lambda t: None if t is None else tuple(t.shape)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in (color, depth, pose, sil) if t is not None):
        raise RuntimeError(f"{who}.{method} needs device tensors (the host path is Host{who})")
    if shape(color) not in (None, (3, H, W)) or shape(depth) != (H, W) or shape(sil) not in (None, (H, W)):
        raise ValueError(f"{who}.{method}: color [3,{H},{W}], depth and sil [{H},{W}]; got {shape(color)}, {shape(depth)}, {shape(sil)}")
    prep = lambda t: None if t is None else t.detach().float().contiguous()
    return prep(color), prep(depth), prep(sil), prep(pose).reshape(7)


def cam_args(cam):
    """(fx, fy, cx, cy) of a camera dict as the C ABI's four doubles."""
    return tuple(float(cam[k]) for k in ("fx", "fy", "cx", "cy"))


class PointCloudBuilder:
    """The device builder: owns the rows [max_points,4] int32, the voxel table (slots = the power of two >= 2 max_points, 16 bytes each;
    none with voxel == 0), the eight counters and the work buffer; ``add`` is one mm3dgs_pointcloud_add_view call on the current stream."""

    def __init__(self, H, W, cam, voxel=0.01, max_points=1 << 24, sil_min=0.99, depth_max=0.0, device="cuda:0"):
        from . import _lib
        from .rasterizer import _stream
        self.H, self.W, self.cam = int(H), int(W), cam
        self.voxel, self.cap, self.sil_min, self.depth_max = float(voxel), int(max_points), float(sil_min), float(depth_max)
        if self.cap < 1:
            raise ValueError(f"pointcloud.max_points = {max_points} (must be positive)")
        if not str(device).startswith("cuda"):
            raise ValueError("PointCloudBuilder needs a CUDA device (the host path is HostPointCloudBuilder)")
        self.lib = _lib.load()
        nbytes = int(self.lib.mm3dgs_pointcloud_work_bytes(self.H, self.W))
        if nbytes == 0:
            raise ValueError(f"point cloud of {H} x {W} views: both sizes must be positive and H W at most 2^28")
        self.slots = 0
        self.table = None
        if self.voxel > 0:
            self.slots = 64
            while self.slots < 2 * self.cap:
                self.slots *= 2
            self.table = torch.empty(self.slots, 2, dtype=torch.int64, device=device)
        self.buf = torch.empty(self.cap, 4, dtype=torch.int32, device=device)
        self.counters = torch.empty(8, dtype=torch.int64, device=device)
        self.work = torch.empty(nbytes // 8, dtype=torch.int64, device=device)
        self.view = 0
        self._read = None
        _lib.check(self.lib.mm3dgs_pointcloud_reset(_lib.ptr(self.table), self.slots, _lib.ptr(self.counters), _stream()))

    def add(self, color, depth, sil, pose):
        from . import _lib
        from .rasterizer import _stream
        color_c, depth_c, sil_c, pose_c = device_view("PointCloudBuilder", self.H, self.W, color, depth, sil, pose)
        P = _lib.ptr
        _lib.check(self.lib.mm3dgs_pointcloud_add_view(self.H, self.W, *cam_args(self.cam), P(pose_c), P(color_c), P(depth_c), P(sil_c), self.sil_min, self.depth_max,
                                                       self.voxel, self.view, P(self.buf), self.cap, P(self.table), self.slots, P(self.counters), P(self.work), _stream()))
        self.view += 1
        self._read = None

    def read_counters(self):
        if self._read is None:
            self._read = self.counters.cpu().numpy().copy()      # the one read-back
        return _counters_dict(self._read)

    def finish(self):
        c = self.read_counters()
        if c["probe_fail"] or c["capacity_dropped"]:
            raise _overflow_error(c)
        return c

    def rows(self):
        """The filled prefix of the row buffer (a view, on the device)."""
        return self.buf[:self.read_counters()["rows"]]


# ---- files ----------------------------------------------------------------------------------------------------------------------
CLOUD_PROPERTIES = "property float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"


def cloud_header(n):
    return "ply\nformat binary_little_endian 1.0\n" + f"element vertex {int(n)}\n" + CLOUD_PROPERTIES + "end_header\n"


def write_ply(path, rows):
    """Binary little-endian PLY, ``float x y z; uchar red green blue alpha``: the body is the row buffer's bytes as they are."""
    rows = as_np(rows, np.int32).reshape(-1, 4)
    with open(path, "wb") as fh:
        fh.write(cloud_header(len(rows)).encode("ascii"))
        fh.write(rows.astype("<i4", copy=False).tobytes())
    return path


def read_header(fh):
    """[(element name, count, [(type, property name)])] of a PLY header, the stream left at the body."""
    elements = []
    if fh.readline().strip() != b"ply":
        raise ValueError("not a PLY file")
    while True:
        line = fh.readline()
        if not line:
            raise ValueError("PLY header without end_header")
        words = line.decode("ascii").split()
        if words[:1] == ["element"]:
            elements.append((words[1], int(words[2]), []))
        elif words[:1] == ["property"]:
            elements[-1][2].append((words[1], words[2]))
        elif words[:1] == ["format"] and words[1] != "binary_little_endian":
            raise ValueError(f"PLY format {words[1]} (binary_little_endian is what this package writes)")
        elif words[:1] == ["end_header"]:
            return elements


def read_ply(path):
    """The rows [n,4] int32 of a file written by ``write_ply``."""
    with open(path, "rb") as fh:
        elements = read_header(fh)
        if len(elements) != 1 or [p for _, p in elements[0][2]] != ["x", "y", "z", "red", "green", "blue", "alpha"]:
            raise ValueError(f"{path}: not a point cloud of write_ply")
        n = elements[0][1]
        body = fh.read(16 * n)
    if len(body) != 16 * n:
        raise ValueError(f"{path}: {len(body)} body bytes for {n} vertices")
    return np.frombuffer(body, dtype="<i4").reshape(n, 4).copy()


def trajectory_colors(n):
    """The reference's ramp for the camera path: cool(0.5 + 0.5 i / n), cool(x) = (x, 1 - x, 1), as uint8 [n,3] (rounded)."""
    x = 0.5 + 0.5 * np.arange(n, dtype=np.float64) / max(n, 1)
    return np.floor(np.stack([x, 1.0 - x, np.ones_like(x)], 1) * 255.0 + 0.5).astype(np.uint8)


_TRAJ_VERTEX = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)])


def write_trajectory_ply(path, poses):
    """The camera path of world->camera 7-vectors [n,7]: vertices = the camera centres (eval_utils.camera_centers) with the ramp colours,
    one polyline as n - 1 ``edge`` elements (vertex1, vertex2) joining consecutive poses."""
    from .eval_utils import camera_centers
    poses = np.asarray(poses.detach().cpu() if isinstance(poses, torch.Tensor) else poses, dtype=np.float64).reshape(-1, 7)
    n = len(poses)
    vert = np.zeros(n, dtype=_TRAJ_VERTEX)
    if n:
        vert["xyz"] = camera_centers(poses)[:, 4:].numpy().astype(np.float32)
    vert["rgb"] = trajectory_colors(n)
    edges = np.stack([np.arange(max(n - 1, 0)), np.arange(1, max(n, 1))], 1).astype("<i4")
    header = ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {n}\n" + "property float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n" + f"element edge {len(edges)}\n"
              "property int vertex1\nproperty int vertex2\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(edges.tobytes())
    return path


def read_trajectory_ply(path):
    """(xyz float32 [n,3], rgb uint8 [n,3], edges int32 [m,2]) of a file written by ``write_trajectory_ply``."""
    with open(path, "rb") as fh:
        elements = read_header(fh)
        if [e[0] for e in elements] != ["vertex", "edge"]:
            raise ValueError(f"{path}: not a trajectory of write_trajectory_ply")
        vert = np.frombuffer(fh.read(_TRAJ_VERTEX.itemsize * elements[0][1]), dtype=_TRAJ_VERTEX)
        edges = np.frombuffer(fh.read(8 * elements[1][1]), dtype="<i4").reshape(-1, 2)
    return vert["xyz"].copy(), vert["rgb"].copy(), edges.copy()
