"""The post-run stage (mm3dgs_slam_amd/export.py) and the rules it shares with their host statements: `mesh.view_bounds` against
`pointcloud.backproject_host`, `mesh.lattice_for` against its arithmetic written out, `geometry.align_rows` under the identity alignment,
`export.options`, the isolation and order of `export.run_post`, and the view contract `pointcloud.device_view`.  CPU only."""
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import export, geometry as geo, mesh as ms, pointcloud as pc
from mm3dgs_slam_amd.config import _TUM, default_config

CAM = {"fx": 41.5, "fy": 40.25, "cx": 2.25, "cy": 0.75}
POSE = torch.tensor([0.9, -0.3, 0.5, 0.2, 0.31, -0.27, 0.64])      # the quaternion is not normalised (norm ~1.09)
SIL_MIN, DEPTH_MAX = 0.6, 4.0


def _view(H, W, with_sil=True):
    """depth [H,W] in (1, 3), silhouette all 1 (or None); 3 x 5: one pixel each of 0, NaN, +inf, above DEPTH_MAX, silhouette below SIL_MIN"""
    g = torch.Generator().manual_seed(H * 100 + W)
    depth = 1.0 + 2.0 * torch.rand(H, W, generator=g)
    sil = torch.ones(H, W) if with_sil else None
    if (H, W) == (3, 5):
        depth[0, 1], depth[1, 0], depth[1, 3], depth[2, 2] = 0.0, float("nan"), float("inf"), DEPTH_MAX + 0.5
        if with_sil:
            sil[2, 4] = SIL_MIN - 0.1
    return depth, sil


@pytest.mark.parametrize("H,W,with_sil,n_valid", [(1, 1, True, 1), (3, 5, True, 10), (3, 5, False, 11)])
def test_view_bounds_is_the_box_of_the_host_statements_points(H, W, with_sil, n_valid):
    """Both sides are float64 evaluations of one formula in different operation orders: 64 x 2^-52 x the largest `scale` component of
    `backproject_host(full=True)` (a few roundings per operation over about ten operations)."""
    depth, sil = _view(H, W, with_sil)
    lo, hi = ms.view_bounds(depth, sil, POSE, CAM, SIL_MIN, DEPTH_MAX)
    rows, xyz, scale, idx = pc.backproject_host(torch.zeros(3, H, W), depth, sil, POSE, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], SIL_MIN, DEPTH_MAX, full=True)
    assert len(idx) == n_valid and lo.dtype == hi.dtype == torch.float64 and lo.device == depth.device
    bound = 64 * 2.0 ** -52 * float(scale.max())
    err = max(np.abs(lo.numpy() - xyz.min(0)).max(), np.abs(hi.numpy() - xyz.max(0)).max())
    print(f"EXPORTERR view_bounds {H} x {W}, sil {with_sil}: {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_view_without_a_valid_pixel_is_the_empty_box_and_the_driver_names_it():
    depth = torch.tensor([[0.0, float("nan")], [float("inf"), DEPTH_MAX + 1.0]])
    lo, hi = ms.view_bounds(depth, None, POSE, CAM, SIL_MIN, DEPTH_MAX)
    assert (lo == float("inf")).all() and (hi == -float("inf")).all()
    cfg = {"cam": CAM, "mapping": {"kf_every": 1}, "mesh": {"max_depth": DEPTH_MAX}}
    slam = SimpleNamespace(cfg=cfg, seq=[(torch.zeros(3, 2, 2), depth, POSE)], estimate_pose_list=[POSE])
    with pytest.raises(ValueError, match="no view has a valid pixel"):
        export.mesh_bounds(slam, export.options(cfg, "mesh", source="sensor"))


def test_lattice_for_is_the_snap_down_and_ceil_plus_one_rule():
    voxel = 0.1
    box = np.array([-1.37, 0.26, 0.5, 0.91, 0.29, 0.5])      # y flatter than one voxel, z flat
    origin, dims = ms.lattice_for(box, voxel, 1 << 28)
    want_origin = np.array([np.floor(-1.37 / voxel) * voxel, np.floor(0.26 / voxel) * voxel, np.floor(0.5 / voxel) * voxel])
    want_dims = [max(int(np.ceil((0.91 - want_origin[0]) / voxel)) + 1, 2), max(int(np.ceil((0.29 - want_origin[1]) / voxel)) + 1, 2),
                 max(int(np.ceil((0.5 - want_origin[2]) / voxel)) + 1, 2)]
    assert np.array_equal(origin, want_origin) and list(dims) == want_dims
    assert (origin <= box[:3]).all() and abs(origin[0] + 1.4) < 1e-12 and list(dims) == [25, 2, 2]      # -1.4 .. 0.91: 24 cells, 25 samples
    n = dims[0] * dims[1] * dims[2]
    assert ms.lattice_for(box, voxel, n)[1] == dims
    with pytest.raises(ValueError, match=rf"is a lattice of {dims[0]} x 2 x 2 samples, more than mesh\.max_voxels = {n - 1} \(at most 2\^30\)"):
        ms.lattice_for(box, voxel, n - 1)


@pytest.mark.parametrize("method", ["horn", "umeyama"])
def test_align_rows_under_the_identity_keeps_colours_and_positions(method):
    """est_poses == gt_poses: the float64 transform is the identity up to float64 rounding, then one rounding to float32."""
    poses = [torch.tensor(p) for p in ([1.0, 0, 0, 0, 0.0, 0.0, 0.0], [0.98, 0.1, -0.15, 0.05, 0.4, -0.1, 0.2], [0.95, -0.2, 0.1, 0.2, -0.3, 0.5, 0.1])]
    rng = np.random.default_rng(3)
    rows = np.empty((257, 4), dtype=np.int32)
    rows[:, :3] = (rng.uniform(-5, 5, (257, 3)).astype(np.float32)).view(np.int32)
    rows[:, 3] = rng.integers(-2 ** 31, 2 ** 31, 257, dtype=np.int64).astype(np.int32)
    out = geo.align_rows(rows, poses + [None], poses + [None], method).numpy()
    assert np.array_equal(out[:, 3], rows[:, 3])
    a, b = pc.rows_xyz(rows), pc.rows_xyz(out)
    err, tol = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()), 2.0 * float(np.spacing(np.abs(a).max()))
    print(f"EXPORTERR align_rows {method}: {err:.3e} (2 ulp of the largest coordinate {tol:.3e})")
    assert err <= tol


def test_options_merges_resolves_and_validates():
    cfg = default_config(device="cpu")
    for block in ("pointcloud", "mesh"):
        opt = export.options(cfg, block)
        assert opt["every"] == cfg["mapping"]["kf_every"] and opt["voxel"] == _TUM[block]["voxel"] and opt["source"] == "render"
        assert all(opt[k] == v for k, v in _TUM[block].items() if k not in ("every", "trunc"))
    assert export.options(cfg, "mesh")["trunc"] == 4 * _TUM["mesh"]["voxel"] and "trunc" not in export.options(cfg, "pointcloud")
    cfg["mesh"] = {"voxel": 0.05, "every": 3, "trunc": 0.3, "source": "sensor"}
    opt = export.options(cfg, "mesh")
    assert (opt["every"], opt["voxel"], opt["trunc"], opt["source"], opt["min_weight"]) == (3, 0.05, 0.3, "sensor", 1)
    opt = export.options(cfg, "mesh", every=None, voxel=0.25, source="render")      # an override wins over the block; None is no override
    assert (opt["every"], opt["voxel"], opt["trunc"], opt["source"]) == (3, 0.25, 0.3, "render")
    cfg["mesh"]["trunc"] = 0
    assert export.options(cfg, "mesh", voxel=0.25)["trunc"] == 1.0
    geo_opt = export.options(cfg, "geometry", estimate="pointcloud")
    assert (geo_opt["estimate"], geo_opt["reference"], geo_opt["align"], geo_opt["threshold"]) == ("pointcloud", "sensor", "none", 0.05)
    for block, over, text in (("mesh", {"source": "lidar"}, r"mesh\.source = 'lidar' \(render / sensor\)"), ("pointcloud", {"every": 0}, r"pointcloud\.every = 0 \(must be positive\)"),
                              ("mesh", {"voxel": 0.0}, r"mesh\.voxel = 0\.0 \(must be positive\)"), ("geometry", {"estimate": "volume"}, "mesh / pointcloud")):
        with pytest.raises(ValueError, match=text):
            export.options(cfg, block, **over)
    assert export.options(cfg, "pointcloud", voxel=0.0)["voxel"] == 0.0      # no thinning: allowed


def test_run_post_reports_a_failed_stage_and_runs_the_next(tmp_path, capsys):
    """`pointcloud.max_points: 1`: the point cloud export raises its overflow error; the run does not, and the mesh is still exported after it."""
    from mm3dgs_slam_amd.renderer import Renderer
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from oracle.raster_ref import RefRasterizer
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device="cpu", height=24, width=32, tracking={"iters": 1, "use_gt_pose": True}, mapping={"iters": 1, "kf_every": 1}, outputdir=str(tmp_path),
                         pointcloud={"export": True, "max_points": 1, "source": "sensor"}, mesh={"export": True, "voxel": 0.25, "source": "sensor"})
    seq = SyntheticSequence(cfg, 2, 300, seed=2, renderer=Renderer(cfg, rasterizer_cls=RefRasterizer))
    slam = SLAM(cfg, seq, rasterizer_cls=RefRasterizer)
    slam.run()
    out = capsys.readouterr().out
    assert [row[:2] for row in export.POST] == [("pointcloud", "export"), ("mesh", "export"), ("geometry", "eval")]
    assert "(point cloud export: RuntimeError('point cloud export dropped points" in out and "\nMesh: " in out
    assert out.index("(point cloud export: ") < out.index("\nMesh: ") and "Geometry (" not in out
    assert slam.pointcloud_export is None and slam.mesh_export is not None and slam.geometry_eval is None
    rows, tris = ms.read_surface_ply(str(tmp_path / "mesh" / "mesh.ply"))
    assert slam.mesh_export["mesh"] == str(tmp_path / "mesh" / "mesh.ply") and len(rows) == slam.mesh_export["counters"]["vertices"] > 0 and len(tris) > 0
    assert not (tmp_path / "pointcloud" / "cloud.ply").exists()


def test_device_view_wants_device_tensors_and_names_its_caller():
    color, depth, pose = torch.zeros(3, 2, 3), torch.ones(2, 3), torch.tensor([1.0, 0, 0, 0, 0, 0, 0])
    for who in ("PointCloudBuilder", "TsdfVolume"):
        with pytest.raises(RuntimeError, match=rf"{who}\.add needs device tensors \(the host path is Host{who}\)"):
            pc.device_view(who, 2, 3, color, depth, None, pose)
