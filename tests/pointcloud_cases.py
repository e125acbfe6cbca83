"""Inputs shared by tests/test_pointcloud.py (CPU) and tests/test_gpu_pointcloud.py: seeded views at the shapes where the count / scan /
scatter compaction of csrc/pointcloud.hip can break, with the validity patterns of its pixel test, and planted planes for the voxel
selection.  Everything is numpy on the host; the GPU tests move it over once."""
import numpy as np

SHAPES = ((1, 1), (16, 16), (17, 33), (520, 520))      # one pixel; exactly one workgroup; a partial last one; 1057 workgroups: two rounds of the 1024-wide scan
PATTERNS = ("all", "none", "checker", "last", "planted", "sil_edge", "depth_max_edge")
SIL_MIN = 0.99
DEPTH_MAX_EDGE = 2.75      # exactly representable: depth == depth_max passes, the next float32 above does not


def camera(H, W):
    f = 1.25 * max(W, 8)
    return {"fx": f + 0.37, "fy": f - 0.21, "cx": 0.5 * W - 0.85, "cy": 0.5 * H + 0.4}


def view_faults(pose_ptr):
    """The faults of the posed pinhole view itself -- H, W, fx, fy, cx, cy, pose -- as overrides of a driver's arguments: the one list every
    call that takes a view must reject (pointcloud_add_view, the three tsdf calls, cull_mark_view, mesh_depth_render).  pose_ptr: the
    device address of the good pose."""
    nan, inf = float("nan"), float("inf")
    return {"H = 0": dict(H=0), "W < 0": dict(W=-3), "more than 2^28 pixels": dict(H=1 << 14, W=(1 << 14) + 1), "fx NaN": dict(fx=nan), "fx = 0": dict(fx=0.0),
            "fy = 0": dict(fy=0.0), "fy inf": dict(fy=inf), "cx NaN": dict(cx=nan), "cy inf": dict(cy=inf), "NULL pose": dict(pose=None),
            "misaligned pose": dict(pose=pose_ptr + 2)}


def view_fault_texts(who, H, W, pose_ptr, misaligned):
    """(overrides, mm3dgs_last_error() text) of five single faults of a view for the call named `who`: both size faults, both intrinsics
    faults and the misaligned pose, whose text (`misaligned`) names the call's other pointers.  The texts are the ones api.hip had before its
    view checks were stated once: they are part of the C ABI's behaviour."""
    return [(dict(H=0, W=W), f"{who}: H = 0, W = {W} (both must be positive)"),
            (dict(H=1 << 14, W=(1 << 14) + 1), f"{who}: 16384 x 16385 has more than 2^28 pixels"),
            (dict(fx=0.0, fy=2.5), f"{who}: fx = 0, fy = 2.5 (finite, not 0)"),
            (dict(cx=1.5, cy=float("inf")), f"{who}: cx = 1.5, cy = inf (must be finite)"),
            (dict(pose=pose_ptr + 2), f"{who}: {misaligned}")]


def pose(k=0, shift=(0.0, 0.0, 0.0)):
    """A world->camera pose with a non-unit quaternion (the kernel normalises) whose world points all have positive coordinates for depths
    below ~4 m (t = -5 on every axis puts the camera centre near (+5, +5, +5) R)."""
    q = np.array([0.93, 0.08 + 0.01 * k, -0.06, 0.05]) * 1.7
    t = np.array([-5.0 + shift[0], -5.2 + shift[1], -4.9 + shift[2]])
    return np.concatenate([q, t]).astype(np.float32)


def view(H, W, pattern, seed=0):
    """dict(color [3,H,W], depth [H,W], sil [H,W] or None, pose [7], cam, sil_min, depth_max) of one validity pattern."""
    rng = np.random.default_rng(1000 * H + W + 7 * seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    color = (rng.random((3, H, W), dtype=np.float32) * 1.4 - 0.2).astype(np.float32)      # below 0 and above 1 too
    color.reshape(-1)[::7] = np.float32(np.nan)      # NaN quantises to 0
    color.reshape(-1)[3::11] = 0.5
    depth = (1.2 + 1.1 * rng.random((H, W), dtype=np.float32) + 0.3 * xx / max(W, 1)).astype(np.float32)
    sil, depth_max = None, 0.0
    if pattern == "none":
        depth[:] = 0.0
    elif pattern == "checker":
        depth[((xx + yy) % 2) == 1] = 0.0
    elif pattern == "last":
        keep = depth[-1, -1]
        depth[:] = -1.0
        depth[-1, -1] = keep
    elif pattern == "planted":
        flat = depth.reshape(-1)
        for k, bad in enumerate((np.nan, np.inf, 0.0, -0.0, -1.5, -np.inf)):
            flat[(5 * k + 1) % flat.size::37] = bad
    elif pattern == "sil_edge":
        s = np.float32(SIL_MIN)
        sil = rng.choice(np.array([s, np.nextafter(s, np.float32(2)), np.nextafter(s, np.float32(0)), 1.0, 0.0, np.nan], dtype=np.float32), size=(H, W))
        sil = np.ascontiguousarray(sil, dtype=np.float32)
    elif pattern == "depth_max_edge":
        e = np.float32(DEPTH_MAX_EDGE)
        depth.reshape(-1)[::3] = e
        depth.reshape(-1)[1::3] = np.nextafter(e, np.float32(10))
        depth.reshape(-1)[2::5] = np.nextafter(e, np.float32(0))
        depth_max = DEPTH_MAX_EDGE
    return {"color": color, "depth": depth, "sil": sil, "pose": pose(), "cam": camera(H, W), "sil_min": SIL_MIN, "depth_max": depth_max}


def plane_view(H, W, k=0, shift=(0.0, 0.0, 0.0), seed=0):
    """A tilted plane z = 2 + 0.3 x_n - 0.2 y_n seen from pose k shifted by `shift`: neighbouring pixels are ~2 / f apart, so a voxel of
    a few pixel footprints merges some and not others."""
    rng = np.random.default_rng(77 + seed + 13 * k)
    cam = camera(H, W)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = (2.0 + 0.3 * (xx - cam["cx"]) / cam["fx"] - 0.2 * (yy - cam["cy"]) / cam["fy"]).astype(np.float32)
    depth.reshape(-1)[4::29] = 0.0      # a few holes
    color = rng.random((3, H, W), dtype=np.float32)
    return {"color": color, "depth": depth, "sil": None, "pose": pose(k, shift), "cam": cam, "sil_min": SIL_MIN, "depth_max": 0.0}


def footprint(v):
    """Distance of neighbouring pixels' points on a surface ~2 m away."""
    return 2.0 / v["cam"]["fx"]
