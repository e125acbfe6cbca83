"""Inputs shared by tests/test_mesh_sparse.py (CPU) and tests/test_gpu_mesh_sparse.py: ray-cast views of a sphere fixed in the world (with
an invalid background or a wall behind it), analytic volumes cut into voxel blocks, and helpers that build the dense volume a voxel-block
volume is compared with.  Everything is numpy on the host; the GPU tests move it over once."""
import numpy as np

from mm3dgs_slam_amd import mesh as ms
from mm3dgs_slam_amd.pointcloud import pose_rotation
from tests import mesh_cases as cases
from tests import pointcloud_cases as pcases

SPHERE_RADIUS = 0.45
SPHERE_DEPTH = 2.0      # in front of pose(0)
WALL_DEPTH = 3.0        # the plane z = 3 of pose(0)'s camera frame


def sphere_view(H, W, k=0, wall=False):
    """A view of tests/pointcloud_cases.py's kind: the sphere seen from pose(k, shift=(0.15 k, -0.1 k, 0.05 k)); depth along the optical
    axis, 0 (invalid) where the ray meets nothing; the colour a smooth function of the world point."""
    cam = pcases.camera(H, W)
    R0, t0 = pose_rotation(pcases.pose(0))
    pose = pcases.pose(k, shift=(0.15 * k, -0.1 * k, 0.05 * k))
    R, t = pose_rotation(pose)
    centre = R @ ((np.array([0.0, 0.0, SPHERE_DEPTH]) - t0) @ R0) + t      # the sphere's centre in this camera's frame
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([(u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"], np.ones_like(u)], -1)      # the ray, z = 1 per unit of depth
    a, b, c = (d * d).sum(-1), -2.0 * (d @ centre), centre @ centre - SPHERE_RADIUS ** 2
    disc = b * b - 4 * a * c
    with np.errstate(invalid="ignore"):
        depth = np.where(disc > 0, (-b - np.sqrt(disc)) / (2 * a), 0.0)
    depth = np.where(depth > 0, depth, 0.0)
    if wall:
        # z0 = (R0 R^T (lambda d - t) + t0)_z = 3
        M = R0 @ R.T
        lam = (WALL_DEPTH - t0[2] + (M @ t)[2]) / (d @ M[2])
        depth = np.where((depth == 0) & (lam > 0), lam, depth)
    pw = (d * depth[..., None] - t) @ R
    color = np.stack([0.5 + 0.5 * np.sin(3.0 * pw[..., 0]), 0.5 + 0.5 * np.cos(2.0 * pw[..., 1]), 0.5 + 0.4 * np.sin(pw[..., 2] + pw[..., 0])]).astype(np.float32)
    return {"color": color, "depth": depth.astype(np.float32), "sil": None, "pose": pose, "cam": cam, "sil_min": pcases.SIL_MIN, "depth_max": 0.0}


def sphere_case(voxel=0.02, wall=False, n_views=3, hw=(48, 64), anchor=(0.0, 0.0, 0.0)):
    """dict(views, voxel, trunc = 4 voxel, anchor) of `n_views` sphere views."""
    return {"views": [sphere_view(hw[0], hw[1], k, wall) for k in range(n_views)], "voxel": float(voxel), "trunc": 4.0 * float(voxel),
            "anchor": np.asarray(anchor, dtype=np.float64)}


def scattered_case(hw, pattern, n_views, voxel=0.05, anchor=(0.0, 0.0, 0.0)):
    """The scattered-depth views of tests/mesh_cases.integrate_case as a voxel-block case."""
    c = cases.integrate_case((17, 9, 6), hw[0], hw[1], pattern, n_views)
    return {"views": c["views"], "voxel": float(voxel), "trunc": 4.0 * float(voxel), "anchor": np.asarray(anchor, dtype=np.float64)}


def reserve_all(case, clip=None, full=False):
    """(keys ascending, [views, valid, pairs, blocks, 0, out of range], near) of a case's views by the host statement."""
    keys, c, near, clean = np.zeros(0, dtype=np.int64), [0] * 6, 0, np.zeros(0, dtype=np.int64)
    for v in case["views"]:
        k, info = ms.reserve_host(v["depth"], v["sil"], v["pose"], **v["cam"], voxel=case["voxel"], trunc=case["trunc"], anchor=case["anchor"],
                                  sil_min=v["sil_min"], depth_max=v["depth_max"], clip=clip, full=True)
        keys = np.union1d(keys, k)
        clean = np.union1d(clean, info["keys_without_near"])
        c[0] += 1; c[1] += info["valid"]; c[2] += info["pairs"]; c[5] += info["out_of_range"]
        near += info["near"]
    c[3] = len(keys)
    return (keys, c, near, clean) if full else (keys, c, near)


def host_volume(case, cls=ms.HostSparseTsdfVolume, **kw):
    """A HostSparseTsdfVolume (or another class of its interface) over a case: reserved, frozen, integrated."""
    v0 = case["views"][0]
    H, W = v0["depth"].shape
    vol = cls(case["voxel"], case["trunc"], H, W, v0["cam"], sil_min=v0["sil_min"], depth_max=v0["depth_max"], anchor=case["anchor"], **kw)
    for v in case["views"]:
        vol.reserve(v["depth"], v["sil"], v["pose"])
    vol.freeze()
    for v in case["views"]:
        vol.add(v["color"], v["depth"], v["sil"], v["pose"])
    return vol


def dense_over(case, first, dims, mask=None, excluded=False):
    """(tsdf_w, rgb_w, counters [3]) of the host statement over the lattice `dims` whose first sample has the lattice index `first`; with
    `mask` [nz,ny,nx] the samples outside it are zeroed after every view and the counts are those inside it.  `excluded`: also the samples
    tests/mesh_cases.integrate_all leaves out (a pixel coordinate within 1e-9 of a rounding boundary or an sdf within 1e-9 trunc of +-trunc
    in some view)."""
    tsdf_w, rgb_w = ms.empty_volume(*dims)
    c = [0, 0, 0]
    out = np.zeros(tsdf_w.shape[:3], dtype=bool)
    for v in case["views"]:
        _, g = ms.integrate_host(tsdf_w, rgb_w, v["color"], v["depth"], v["sil"], v["pose"], **v["cam"], origin=case["anchor"], voxel=case["voxel"],
                                 trunc=case["trunc"], sil_min=v["sil_min"], depth_max=v["depth_max"], full=True, first=first)
        keep = np.ones(g["upd"].shape, dtype=bool) if mask is None else mask
        if mask is not None:
            tsdf_w[~mask] = 0
            rgb_w[~mask] = 0
        c[0] += 1; c[1] += int((g["upd"] & keep).sum()); c[2] += int((g["col"] & keep).sum())
        with np.errstate(invalid="ignore"):
            for f in (g["fu"], g["fv"]):
                frac = f - np.floor(f)
                out |= (g["z"] > 0) & ((frac < 1e-9) | (frac > 1 - 1e-9))
            out |= g["seen"] & ((np.abs(g["sdf"] - case["trunc"]) < 1e-9 * case["trunc"]) | (np.abs(g["sdf"] + case["trunc"]) < 1e-9 * case["trunc"]))
    return (tsdf_w, rgb_w, c, out) if excluded else (tsdf_w, rgb_w, c)


def analytic_blocks(kind, drop_third=False):
    """The analytic volume of tests/mesh_cases.py at (65, 65, 65), padded to 72^3 with weight 0, as 9^3 blocks with block coordinates from
    0: dict(tsdf_w, rgb_w [72,72,72,.] -- with `drop_third` every third block (in key order) zeroed --, blocks [n,3] in ascending key
    order, keys, first, dims, origin, voxel)."""
    vol = cases.analytic_volume(kind, (65, 65, 65))
    tsdf_w, rgb_w = ms.empty_volume(72, 72, 72)
    tsdf_w[:65, :65, :65], rgb_w[:65, :65, :65] = vol["tsdf_w"], vol["rgb_w"]
    bz, by, bx = np.meshgrid(np.arange(9), np.arange(9), np.arange(9), indexing="ij")
    blocks = np.stack([bx, by, bz], -1).reshape(-1, 3)      # z-major raster: ascending keys
    if drop_third:
        gone = blocks[1::3]
        for b in gone:
            tsdf_w[8 * b[2]:8 * b[2] + 8, 8 * b[1]:8 * b[1] + 8, 8 * b[0]:8 * b[0] + 8] = 0
            rgb_w[8 * b[2]:8 * b[2] + 8, 8 * b[1]:8 * b[1] + 8, 8 * b[0]:8 * b[0] + 8] = 0
        blocks = np.delete(blocks, np.arange(1, len(blocks), 3), axis=0)
    keys = ms.block_keys(blocks)
    assert bool((np.diff(keys) > 0).all())
    return {"tsdf_w": tsdf_w, "rgb_w": rgb_w, "blocks": blocks, "keys": keys, "first": np.zeros(3, dtype=np.int64), "dims": [72, 72, 72], "origin": vol["origin"],
            "voxel": vol["voxel"], "kind": kind}


def to_pool(tsdf_w, rgb_w, blocks, first, dims):
    """(tsdf_w [n,512,2], rgb_w [n,512,4]) of the blocks of a dense lattice."""
    nx, ny, nz = dims
    s = ms.pool_index(blocks, first, dims, np.arange(nx * ny * nz))
    at = np.argsort(s, kind="stable")[int((s < 0).sum()):]
    return np.ascontiguousarray(tsdf_w.reshape(-1, 2)[at].reshape(-1, 512, 2)), np.ascontiguousarray(rgb_w.reshape(-1, 4)[at].reshape(-1, 512, 4))


def neighbours_host(keys):
    """int32 [n,27]: the rank of the block at offset (dx, dy, dz) at entry (dz + 1) 9 + (dy + 1) 3 + (dx + 1), -1 for none."""
    keys = np.asarray(keys, dtype=np.int64)
    b = ms.key_blocks(keys)
    out = np.full((len(keys), 27), -1, dtype=np.int32)
    for j in range(27):
        nb = b + np.array([j % 3 - 1, (j // 3) % 3 - 1, j // 9 - 1])[None, :]
        ok = (np.abs(nb) < ms.BLOCK_BIAS).all(1)
        k = ms.block_keys(np.where(ok[:, None], nb, 0))
        at = np.searchsorted(keys, k)
        hit = ok & (at < len(keys)) & (keys[np.minimum(at, len(keys) - 1)] == k)
        out[hit, j] = at[hit]
    return out


def mesh_sets(rows, tris):
    """A mesh as order-free sets: the vertices as (position bytes, colour) rows and the triangles as sorted rows of those vertices."""
    rows = np.asarray(rows, dtype=np.int32).reshape(-1, 4)
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    t = inv.reshape(-1)[np.asarray(tris, dtype=np.int64).reshape(-1, 3)]
    return uniq, (np.unique(t, axis=0) if len(t) else t.reshape(0, 3)), len(uniq) == len(rows)
