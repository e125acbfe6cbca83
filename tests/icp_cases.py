"""Scenes and helpers of the ICP tests (tests/test_icp.py on the host, tests/test_gpu_icp.py on the device): the corner scene with its three
true motions, the sets for the rare branches, and the stand-in `device: cpu` run of tests/test_geometry.py re-stated."""
import random

import numpy as np
import torch

from mm3dgs_slam_amd import geometry as geo
from tests.geometry_cases import rows_of

CELL, MAX_DIST, ITERS, REL = 0.05, 0.1, 30, 1e-6      # the scoring cell's default (the threshold), NICE-SLAM's distance, Open3D's criteria
STEP = 0.04
# (angle in degrees about (1, 2, 3), t_true in metres)
MOTIONS = ((2.0, (0.015, -0.010, 0.008)), (5.0, (0.03, -0.02, 0.02)), (8.0, (0.04, -0.03, 0.03)))
BOUND = 1e-5      # rotation (rad) and translation (m): the bound tests/test_geometry.py holds `horn` / `umeyama` to under the identity


def rotation(deg, axis=(1.0, 2.0, 3.0)):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    r = np.deg2rad(deg)
    return np.eye(3) + np.sin(r) * K + (1.0 - np.cos(r)) * (K @ K)


def corner_reference():
    """The 1483 points of the corner (float64 [n,3], already rounded to float32): a floor and two walls on a 0.04 m lattice, jittered."""
    lattice = lambda ni, nj: np.stack(np.meshgrid(np.arange(ni) * STEP, np.arange(nj) * STEP, indexing="ij"), -1).reshape(-1, 2)
    f, a, b = lattice(31, 21), lattice(21, 16), lattice(31, 16)
    pts = np.concatenate([np.stack([f[:, 0], f[:, 1], np.zeros(len(f))], 1),
                          np.stack([np.zeros(len(a)), a[:, 0], a[:, 1] + STEP], 1),
                          np.stack([b[:, 0] + STEP, np.zeros(len(b)), b[:, 1] + STEP], 1)])
    k = np.arange(len(pts), dtype=np.uint32)
    jitter = np.stack([geo.mix32(np.uint32(3) * k + np.uint32(s)).astype(np.float64) / 2.0 ** 32 - 0.5 for s in (1, 2, 3)], 1) * np.array([0.02, 0.02, 0.01])
    return (pts + jitter).astype(np.float32).astype(np.float64)


def corner_case(motion, every=1):
    """dict(ref, src: rows [n,4] int32; R, t: the true motion with ref = R src + t) of MOTIONS[motion], with every `every`-th source row."""
    deg, t = MOTIONS[motion]
    R, t = rotation(deg), np.asarray(t, dtype=np.float64)
    ref = corner_reference()
    src = ((ref - t) @ R).astype(np.float32)      # R^T (ref - t) per row
    return {"name": f"corner {deg:g} deg every {every}", "ref": rows_of(ref), "src": rows_of(src[::every], rgba=np.arange(len(src[::every]), dtype=np.int32)), "R": R, "t": t}


def corner_cases():
    return [corner_case(m, every) for m in range(len(MOTIONS)) for every in (1, 3)]


def motion_errors(T, R, t):
    """(rotation error in rad, translation error in m) of T [3,4] against the true motion."""
    T = np.asarray(T, dtype=np.float64).reshape(3, 4)
    D = T[:, :3] @ R.T      # (its angle from the skew part: arccos of the trace has no resolution near 0)
    sin = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(sin, (np.trace(D) - 1.0) / 2.0)), float(np.linalg.norm(T[:, 3] - t))


def run_host(case, sum_order="numpy", **kw):
    args = dict(cell=CELL, max_dist=MAX_DIST, iters=ITERS, rel_fitness=REL, rel_rmse=REL)
    args.update(kw)
    return geo.icp_host(case["src"], case["ref"], sum_order=sum_order, **args)


def tiled_case(copies=257, rows=256):
    """256 x 257 source rows, so that the finish over the partial rows takes its second round: the first 256 rows of the 5 degree corner
    source, tiled, every copy with a hash jitter of at most 1 mm per axis."""
    c = corner_case(1)
    base = geo.rows_xyz(c["src"])[:rows].astype(np.float64)
    n = copies * rows
    k = np.arange(n, dtype=np.uint32)
    jitter = np.stack([geo.mix32(np.uint32(3) * k + np.uint32(s) + np.uint32(0x51ed)).astype(np.float64) / 2.0 ** 32 - 0.5 for s in (1, 2, 3)], 1) * 0.002
    return dict(c, name="second round of the finish", src=rows_of((np.tile(base, (copies, 1)) + jitter).astype(np.float32)))


def rare_case():
    """The rare branches in one set, on the 2 degree corner: three source rows that are not finite; source rows outside the reference grid
    by more than max_dist (no correspondence) and by less; a reference with exact duplicates of its first rows appended FIRST (so the
    smaller row of a tie is not the one a cell happens to hold first) and with rows that are not finite."""
    c = corner_case(0)
    ref, src = geo.rows_xyz(c["ref"]).copy(), geo.rows_xyz(c["src"]).copy()
    ref = np.concatenate([ref[:40], [[np.nan, 0, 0], [0, np.inf, 0]], ref, ref[100:140]]).astype(np.float32)
    far = np.array([[3.0, 3.0, 3.0], [-2.0, 0.5, 0.5], [0.5, 0.5, 5.0]], dtype=np.float32)                  # beyond the grid by more than max_dist
    near = np.array([[1.25, 0.4, -0.06], [0.6, -0.05, 0.3], [-0.07, 0.5, 0.4], [1.30, 0.4, 0.0]], dtype=np.float32)      # outside the jittered lattice, some within reach
    bad = np.array([[np.nan, 0.1, 0.1], [0.1, -np.inf, 0.1], [0.1, 0.1, np.nan]], dtype=np.float32)
    src = np.concatenate([bad[:1], src[:700], far, bad[1:2], near, src[700:], bad[2:]]).astype(np.float32)
    return dict(c, name="rare branches", ref=rows_of(ref), src=rows_of(src))


def box_mesh(lo=(0.0, 0.0, 0.0), hi=(1.2, 0.8, 0.6)):
    """A box of 8 vertices and 12 triangles (vertex rows [8,4] int32, triangles int32 [12,3])."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[x, y, z] for z in (lo[2], hi[2]) for y in (lo[1], hi[1]) for x in (lo[0], hi[0])], dtype=np.float32)
    quads = ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3))
    tris = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int32)
    return rows_of(v, rgba=np.arange(8, dtype=np.int32)), tris


def cpu_slam(tmp, geometry, mesh, tracking=None):
    """The stand-in run of `device: cpu` of tests/test_geometry.py (32 x 48, 3 frames, the oracle rasterizer injected), run to its end."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.renderer import Renderer
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from oracle.raster_ref import RefRasterizer
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device="cpu", height=32, width=48, tracking=dict({"iters": 2}, **(tracking or {})), mapping={"iters": 3, "kf_every": 2},
                         outputdir=str(tmp), mesh=mesh, geometry=geometry)
    seq = SyntheticSequence(cfg, 3, 600, seed=2, renderer=Renderer(cfg, rasterizer_cls=RefRasterizer))
    slam = SLAM(cfg, seq, rasterizer_cls=RefRasterizer)
    slam.run()
    return slam, seq, cfg
