"""Inputs shared by tests/test_mesh.py (CPU) and tests/test_gpu_mesh.py: analytic distance fields sampled straight into a volume (sphere,
torus, tilted plane; off-lattice centres, so no sample is exactly 0), and posed views over small lattices for the integration, with the
validity patterns of tests/pointcloud_cases.py.  Everything is numpy on the host; the GPU tests move it over once."""
import numpy as np

from mm3dgs_slam_amd import mesh as ms
from mm3dgs_slam_amd.pointcloud import pose_rotation
from tests import pointcloud_cases as pcases

# one cube; a few cubes; 918 samples: a partial last workgroup; 274 625 samples: 1073 workgroups, the second round of the 1024-wide scan
MESH_SHAPES = ((2, 2, 2), (5, 4, 3), (17, 9, 6), (65, 65, 65))
KINDS = ("sphere", "torus", "plane")
INTEGRATE_SHAPES = ((2, 2, 2), (5, 4, 3), (17, 9, 6), (65, 33, 5), (6, 5, 19))      # the last: three 8-slice steps of a workgroup along z, the third partial
VIEW_SHAPES = ((17, 33), (48, 64))
ORIGIN = np.array([-1.3, 0.7, 2.1])
VOXEL = 0.05
OFF = np.array([0.037, -0.039, 0.083])      # the centre's offset from the lattice's middle, in voxels: no sample on the surface


def distance(kind, dims, p):
    """The true signed distance (negative inside) of points p [..., 3] to the surface of `kind` in the lattice `dims` = (nx, ny, nz)."""
    n = np.asarray(dims, dtype=np.float64)
    c = ORIGIN + VOXEL * (0.5 * (n - 1) + OFF)
    m = VOXEL * (n.min() - 1)
    q = np.asarray(p, dtype=np.float64) - c
    if kind == "sphere":
        return np.sqrt((q * q).sum(-1)) - 0.31 * m
    if kind == "torus":
        mm = VOXEL * (min(dims[0], dims[1]) - 1)
        return np.sqrt((np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - 0.29 * mm) ** 2 + q[..., 2] ** 2) - 0.11 * min(m, mm)
    nrm = np.array([0.31, -0.22, 0.92])
    return q @ (nrm / np.sqrt(nrm @ nrm))      # the half space below the tilted plane is inside


def radii(kind, dims):
    m = VOXEL * (min(dims) - 1)
    return {"sphere": 0.31 * m, "torus": (0.29 * m, 0.11 * m)}[kind]


def analytic_volume(kind, dims, half_known=False):
    """dict(tsdf_w [nz,ny,nx,2], rgb_w [nz,ny,nx,4], origin, voxel, trunc): the distance field of `kind`, truncated at 4 voxels, weight 1
    everywhere (`half_known`: 0 in the upper half of x), smooth colours that leave [0, 1] on both sides."""
    nx, ny, nz = dims
    trunc = 4 * VOXEL
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = ORIGIN + VOXEL * np.stack([i, j, k], -1).astype(np.float64)
    tsdf_w, rgb_w = ms.empty_volume(nx, ny, nz)
    tsdf_w[..., 0] = np.clip(distance(kind, dims, p) / trunc, -1.0, 1.0)
    tsdf_w[..., 1] = 1.0
    if half_known:
        tsdf_w[:, :, nx // 2:, 1] = 0.0
    assert not (tsdf_w[..., 0] == 0).any()
    rgb_w[..., 0] = 1.3 * i / (nx - 1) - 0.15
    rgb_w[..., 1] = 0.5 + 0.6 * np.sin(0.7 * j + 0.3 * k)
    rgb_w[..., 2] = (k + 0.5 * j) / (nz + 0.5 * ny)
    rgb_w[..., 3] = 1.0
    return {"tsdf_w": tsdf_w, "rgb_w": rgb_w, "origin": ORIGIN.copy(), "voxel": VOXEL, "trunc": trunc, "dims": tuple(dims), "kind": kind}


def integrate_case(dims, H, W, pattern, n_views=1):
    """dict(views: [pointcloud_cases.view ...] from `n_views` poses, origin, voxel, trunc, dims): a lattice around the world point of the
    central pixel at 1.9 m, about 1.5 m wide (the views' depths scatter over 1.2 .. 2.9 m, so with trunc = 4 voxel some samples lie behind
    -trunc, some beyond +trunc and some in the band; the lattice is wider than the frustum, so some project outside the image)."""
    nx, ny, nz = dims
    views = []
    for k in range(n_views):
        v = pcases.view(H, W, pattern, seed=k)
        v["pose"] = pcases.pose(k, shift=(0.05 * k, -0.03 * k, 0.02 * k))
        views.append(v)
    cam = views[0]["cam"]
    R, t = pose_rotation(views[0]["pose"])
    centre = (np.array([(0.5 * W - cam["cx"]) / cam["fx"] * 1.9, (0.5 * H - cam["cy"]) / cam["fy"] * 1.9, 1.9]) - t) @ R
    voxel = 1.5 / max(nx, ny) * 1.0371      # (no lattice plane through a pixel boundary by construction of round numbers)
    origin = centre - voxel * 0.5 * (np.array([nx, ny, nz], dtype=np.float64) - 1) + voxel * OFF
    return {"views": views, "origin": origin, "voxel": voxel, "trunc": 4 * voxel, "dims": tuple(dims)}


def integrate_all(case):
    """The host statement over a case's views: (tsdf_w, rgb_w, counters [3], excluded [nz,ny,nx] bool).  A sample is excluded when in some
    view its pixel coordinate is within 1e-9 of a rounding boundary or its sdf within 1e-9 trunc of +-trunc: there the float64 roundoff of
    another evaluation order may decide differently."""
    nx, ny, nz = case["dims"]
    tsdf_w, rgb_w = ms.empty_volume(nx, ny, nz)
    counters = [0, 0, 0]
    excluded = np.zeros((nz, ny, nx), dtype=bool)
    for v in case["views"]:
        n, g = ms.integrate_host(tsdf_w, rgb_w, v["color"], v["depth"], v["sil"], v["pose"], **v["cam"], origin=case["origin"], voxel=case["voxel"],
                                 trunc=case["trunc"], sil_min=v["sil_min"], depth_max=v["depth_max"], full=True)
        counters[0] += 1; counters[1] += n[0]; counters[2] += n[1]
        with np.errstate(invalid="ignore"):
            front = g["z"] > 0
            for f in (g["fu"], g["fv"]):
                frac = f - np.floor(f)
                excluded |= front & ((frac < 1e-9) | (frac > 1 - 1e-9))
            excluded |= g["seen"] & ((np.abs(g["sdf"] - case["trunc"]) < 1e-9 * case["trunc"]) | (np.abs(g["sdf"] + case["trunc"]) < 1e-9 * case["trunc"]))
    return tsdf_w, rgb_w, counters, excluded
