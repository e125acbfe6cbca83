#!/usr/bin/env python
"""Entry point with the reference's command line (`python slam_top.py --config X.yml`, reference slam_top.py:30-42).

The YAML schema is the reference's (configs/TUM.yml, configs/UTMM.yml).  A config with a non-empty `inputdir` and `dataset: tum` or
`utmm` is read from disk (`mm3dgs_slam_amd.dataset.RecordedSequence`: TUM-format / UT-MM-format directory `inputdir/scene`, all
frames or `--frames N` of them; `ingest_on_device` and `prefetch` choose how a frame gets to the device; `est_depth_dir` names the folder
of per-frame monocular depth estimates).  Every other config -- the
default `dataset: synthetic`, and the two configs the reference ships, whose `inputdir:` is empty -- runs on the in-memory synthetic
RGB-D sequence (10 frames unless `--frames` says otherwise) with the config's hot-path settings (iteration budgets, learning rates,
pipeline flags, intrinsics); Replica, EXR depth, colour undistortion and the monocular depth network itself stay out of scope.  On the
synthetic sequence `use_gt_depth: false` (what configs/TUM.yml ships) and `tracking.dynamics_model: imu` are honoured: the
sequence provides a stand-in for the monocular estimate (`SyntheticSequence.est`, aligned per frame like slam/SLAM.py:411-448) and
synthetic IMU rows (`SyntheticSequence.imu`).  A recorded sequence honours `use_gt_depth: false` when the config names `est_depth_dir`, a
folder in `inputdir/scene` with the network's raw output per colour frame (`<stem>.npy` float32 / float16, or a 16-bit `<stem>.png`):
the estimate is resampled to the frame size as the reference's MiDaS.estimate_depth does and aligned per frame; without the key a
recorded sequence has no estimate and the sensor depth is used.  Only `niqe_kf` is forced off (it needs a downloaded network).

Outputs in `outputdir`, in the reference's formats (slam/SLAM.py:286-373,488-500): `point_cloud/iteration_<n>/point_cloud.ply` for
every frame index in `save_iterations` and for the final map (attribute layout of slam/gaussian_model.py:205-257), `results.npz`
with the reference's keys (pose_est, pose_gt, keyframes, ate_rmse, psnr_list, ssim_list, lpips_list [empty: LPIPS needs a downloaded
network], avg_tracking_it_time / avg_mapping_it_time with debug.get_runtime_stats).  A config that carries `iteration: <n>` resumes
from that checkpoint (map, poses, keyframes, covisibility graph), like the reference.  `debug.create_video: true` adds `debug_video/`
(one PNG per frame of the reference's debug video: after tracking and after mapping; INTEGRATION.md has the ffmpeg line that makes the
video), `debug.save_keyframes: true` adds `keyframes/<idx>.png`, and `--render` adds `render/render<idx>.png` + `render/gt<idx>.png` for
every 50th frame (the reference's `SLAM.render()`).  None of them changes a pose.  `eval_on_device: true` scores the evaluated frames on
the device (`mm3dgs_eval_image`: PSNR, SSIM and the depth L1 against the sensor depth, one read-back) and adds `eval_table`, `eval_frames` and
`depth_l1_list` to `results.npz`.  `--pointcloud` (or `pointcloud.export: true`) adds `pointcloud/cloud.ply`, the reconstruction as a fused coloured
point cloud (the map rendered at every `pointcloud.every`-th estimated pose, lifted to world points, one point per `pointcloud.voxel`; binary PLY, `float x y z;
uchar red green blue alpha`), and `pointcloud/trajectory.ply`, the camera path -- the computational core of the reference's scripts/visualizer.py, for MeshLab or
CloudCompare; `--pointcloud --eval` writes the two files from the checkpoint without running a frame.  `--mesh` (or `mesh.export: true`) adds `mesh/mesh.ply`,
the same views fused into a truncated signed distance volume and meshed by marching tetrahedra (a coloured triangle mesh, binary PLY); `--mesh --eval` likewise
from the checkpoint.  `--geometry` (or `geometry.eval: true`) adds `geometry/metrics.json`, `accuracy.ply` and `completion.ply`: the exported mesh or cloud scored
against a reference surface (the same frames' sensor depth at the ground-truth poses, or a PLY file) -- accuracy, completion, completion ratio, F-score, Chamfer
distance; `--geometry --eval` likewise from the checkpoint.  `--mesh-clean small|largest` (or `mesh.clean`) removes the mesh's small disconnected pieces behind
the extraction, for `--mesh` and for the meshes `--geometry` scores (`mesh.clean_min_triangles`; mesh_clean.py).  `--mesh-volume sparse` (or `mesh.volume`)
holds the fusion volume in hashed 8 x 8 x 8-sample blocks along the surface instead of one dense lattice (`mesh.max_blocks`).  `--mesh-normals` (or
`mesh.normals: true`) writes area-weighted vertex normals into `mesh.ply`; `--geometry-normals` (or `geometry.normals: true`) adds normal consistency to
the geometry scores (`estimate: mesh` against a mesh); `--geometry-icp` (or `geometry.icp: point`) registers the estimate to the reference by
point-to-point ICP before it is scored (NICE-SLAM's protocol; `icp` block of `metrics.json`, `geometry/icp.npz`).

`--eval [--iteration N]` runs no frame: it builds the same sequence (give the run's `--frames` / `--gaussians`), resumes the checkpoint
`outputdir/point_cloud/iteration_<N>` (default: the config's `iteration`, else the largest on disk) with the poses of `results.npz`, and
prints mean PSNR and SSIM (depth L1 with `eval_on_device`), `ATE RMSE` and `ATE RMSE c2w` -- the reference's scripts/eval_image.py and the
printing part of scripts/eval_traj.py; plots stay out of scope.  It writes nothing.
"""
import argparse
import os
import sys
import random
import time

import numpy as np
import torch


def seed_everything(seed=0):
    """Same sources of randomness as the reference seeds (slam_top.py:13-27)."""
    random.seed(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def sequence_source(cfg):
    """"recorded" when the merged config names a sequence on disk (non-empty `inputdir`, `dataset` tum / utmm), else "synthetic"."""
    from mm3dgs_slam_amd.dataset import is_recorded
    return "recorded" if is_recorded(cfg) else "synthetic"


def build_sequence(cfg, frames=None, gaussians=150000):
    """The frame source of a run: the directory `inputdir/scene` (all frames, or the first `frames`), or `frames` (default 10) synthetic
    frames.  A recorded sequence writes its scaled intrinsics into `cfg["cam"]`: build it before the SLAM object."""
    if sequence_source(cfg) == "recorded":
        from mm3dgs_slam_amd.dataset import RecordedSequence
        return RecordedSequence(cfg, frames=frames)
    from mm3dgs_slam_amd.slam import SyntheticSequence
    return SyntheticSequence(cfg, 10 if frames is None else frames, gaussians, seed=0)


def resume_checkpoint(cfg, seq, iteration=None):
    """A SLAM object resumed from `outputdir/point_cloud/iteration_<n>` (`iteration`, else the config's `iteration`, else the largest one on
    disk) with the poses and keyframes of `outputdir/results.npz`; runs no frame.  Returns it with the iteration."""
    import copy
    from mm3dgs_slam_amd.slam import SLAM
    cfg = copy.deepcopy(cfg)
    if iteration is None:
        iteration = cfg.get("iteration")
    if iteration is None:
        names = os.listdir(os.path.join(cfg["outputdir"], "point_cloud"))
        iteration = max(int(n[len("iteration_"):]) for n in names if n.startswith("iteration_"))
    cfg["iteration"] = int(iteration)
    return SLAM(cfg, seq), int(iteration)


def evaluate_checkpoint(cfg, seq, iteration=None):
    """`--eval`: score a finished run from its checkpoint (the reference's scripts/eval_image.py and the printing part of scripts/eval_traj.py).
    Resumes the map `outputdir/point_cloud/iteration_<n>` (`iteration`, else the config's `iteration`, else the largest one on disk) and the
    poses of `outputdir/results.npz`, runs no frame, renders and scores frame 0 and every `eval_every`-th frame of `seq` at the stored poses
    (`SLAM.evaluate_images`; on the device with `eval_on_device`) and aligns the stored trajectories.  Prints the means and returns them with
    the lists; writes nothing: results.npz and the map stay as they are."""
    from mm3dgs_slam_amd.eval_utils import camera_centers, evaluate_ate_rmse
    from mm3dgs_slam_amd.slam import print_image_metrics
    outdir = cfg["outputdir"]
    slam, iteration = resume_checkpoint(cfg, seq, iteration)
    stored = np.load(os.path.join(outdir, "results.npz"), allow_pickle=True)
    est, gt = stored["pose_est"], stored["pose_gt"]
    last_idx = min(len(est), len(seq))
    with torch.no_grad():
        psnr_list, ssim_list, _ = slam.evaluate_images(last_idx)
    out = {"iteration": int(iteration), "psnr_list": psnr_list, "ssim_list": ssim_list, "eval_table": slam.eval_table, "eval_frames": slam.eval_frames,
           "depth_l1_list": None if slam.eval_table is None else [np.asarray(v) for v in slam.eval_table[:, 2]]}
    _, out["ate_rmse"] = evaluate_ate_rmse(est, gt, method="umeyama")
    _, out["ate_rmse_c2w"] = evaluate_ate_rmse(camera_centers(est).numpy(), camera_centers(gt).numpy(), method="umeyama")
    print(f"Evaluation of {outdir} at iteration {iteration}: {len(psnr_list)} of {last_idx} frames")
    print_image_metrics(psnr_list, ssim_list, out["depth_l1_list"])
    print(f"  ATE RMSE : {out['ate_rmse']} m")
    print(f"  ATE RMSE c2w : {out['ate_rmse_c2w']} m")
    return out


def export_pointcloud_checkpoint(cfg, seq, iteration=None):
    """`--pointcloud --eval`: the fused point cloud of a finished run from its checkpoint, without running a frame (the offline part of the
    reference's scripts/visualizer.py): resumes like `evaluate_checkpoint` and calls `SLAM.export_pointcloud` with the config's
    `pointcloud` block.  Adds `outputdir/pointcloud/` (cloud.ply, trajectory.ply) and touches nothing else.  Returns what the export returns."""
    slam, iteration = resume_checkpoint(cfg, seq, iteration)
    out = slam.export_pointcloud()
    out["iteration"] = iteration
    return out


def export_mesh_checkpoint(cfg, seq, iteration=None):
    """`--mesh --eval`: the coloured triangle mesh of a finished run from its checkpoint, without running a frame: resumes like
    `evaluate_checkpoint` and calls `SLAM.export_mesh` with the config's `mesh` block.  Adds `outputdir/mesh/` (mesh.ply) and touches nothing
    else.  Returns what the export returns."""
    slam, iteration = resume_checkpoint(cfg, seq, iteration)
    out = slam.export_mesh()
    out["iteration"] = iteration
    return out


def evaluate_geometry_checkpoint(cfg, seq, iteration=None):
    """`--geometry --eval`: the geometry scores of a finished run from its checkpoint, without running a frame: resumes like
    `evaluate_checkpoint` and calls `SLAM.evaluate_geometry` with the config's `geometry` block (the ground-truth poses of a "sensor"
    reference come from results.npz).  Adds `outputdir/geometry/` (metrics.json, accuracy.ply, completion.ply) and touches nothing else.
    Returns what the evaluation returns."""
    slam, iteration = resume_checkpoint(cfg, seq, iteration)
    out = slam.evaluate_geometry()
    out["iteration"] = iteration
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, default=None, help="YAML config in the reference's schema")
    ap.add_argument("--frames", type=int, default=None, help="frames to run (default: 10 synthetic frames, or the whole recorded sequence)")
    ap.add_argument("--gaussians", type=int, default=150000, help="size of the synthetic ground-truth scene")
    ap.add_argument("--render", action="store_true", help="after the run, write render / ground-truth image pairs of every 50th frame to outputdir/render")
    ap.add_argument("--eval", action="store_true", help="run no frame: score the finished run in outputdir from its checkpoint (PSNR, SSIM, depth L1 with eval_on_device, ATE RMSE)")
    ap.add_argument("--pointcloud", action="store_true", help="after the run (or, with --eval, from the checkpoint without running a frame) write the fused coloured point cloud and the camera path to outputdir/pointcloud (the config's `pointcloud` block)")
    ap.add_argument("--mesh", action="store_true", help="after the run (or, with --eval, from the checkpoint without running a frame) write the reconstruction as a coloured triangle mesh to outputdir/mesh/mesh.ply (the config's `mesh` block)")
    ap.add_argument("--geometry", action="store_true", help="after the run (or, with --eval, from the checkpoint without running a frame) score the exported geometry against a reference surface into outputdir/geometry (the config's `geometry` block)")
    ap.add_argument("--mesh-clean", choices=("small", "largest"), default=None, help="with --mesh / --geometry: remove the mesh's small disconnected pieces (overrides the `mesh` block's `clean`; small: components below mesh.clean_min_triangles triangles, largest: all but the largest component)")
    ap.add_argument("--mesh-volume", choices=("dense", "sparse"), default=None, help="with --mesh / --geometry: how the fusion volume is held (overrides the `mesh` block's `volume`; dense: one lattice over the box of the views, sparse: hashed 8 x 8 x 8-sample blocks along the surface, mesh.max_blocks)")
    ap.add_argument("--mesh-normals", action="store_true", help="with --mesh: write area-weighted vertex normals into mesh.ply (`float nx ny nz` behind the position; sets the `mesh` block's `normals`)")
    ap.add_argument("--geometry-normals", action="store_true", help="with --geometry: also score normal consistency (needs `estimate: mesh` and a mesh as the reference; sets the `geometry` block's `normals`)")
    ap.add_argument("--geometry-icp", action="store_true", help="with --geometry: register the estimate to the reference by point-to-point ICP before it is scored, as NICE-SLAM's eval_recon does (sets the `geometry` block's `icp` to point; icp_max_dist, icp_iters, icp_rel_fitness, icp_rel_rmse)")
    ap.add_argument("--iteration", type=int, default=None, help="with --eval: the checkpoint to score (default: the config's `iteration`, else the largest one in outputdir/point_cloud)")
    args = ap.parse_args()
    from mm3dgs_slam_amd.config import default_config, load_config
    from mm3dgs_slam_amd.slam import SLAM
    seed_everything(0)
    cfg = default_config()
    if args.config:
        user = load_config(args.config)
        for k, v in user.items():
            if isinstance(v, dict) and isinstance(cfg.get(k), dict):
                cfg[k].update(v)
            else:
                cfg[k] = v
    cfg["mapping"]["niqe_kf"] = False
    dbg = dict(cfg.get("debug") or {})
    cfg["debug"] = {"get_runtime_stats": bool(dbg.get("get_runtime_stats", False)), "create_video": bool(dbg.get("create_video", False)),
                    "save_keyframes": bool(dbg.get("save_keyframes", False))}
    cfg.setdefault("outputdir", "output/" + (str(cfg.get("scene") or "recorded") if sequence_source(cfg) == "recorded" else "synthetic"))
    outdir = cfg["outputdir"]
    if args.mesh_clean:
        cfg["mesh"] = dict(cfg.get("mesh") or {}, clean=args.mesh_clean)
    if args.mesh_volume:
        cfg["mesh"] = dict(cfg.get("mesh") or {}, volume=args.mesh_volume)
    if args.mesh_normals:
        cfg["mesh"] = dict(cfg.get("mesh") or {}, normals=True)
    if args.geometry_normals:
        cfg["geometry"] = dict(cfg.get("geometry") or {}, normals=True)
    if args.geometry_icp:
        cfg["geometry"] = dict(cfg.get("geometry") or {}, icp="point")
    if args.eval:
        seq = build_sequence(cfg, args.frames, args.gaussians)
        if args.pointcloud:
            export_pointcloud_checkpoint(cfg, seq, args.iteration)
        if args.mesh:
            export_mesh_checkpoint(cfg, seq, args.iteration)
        if args.geometry:
            evaluate_geometry_checkpoint(cfg, seq, args.iteration)
        if not (args.pointcloud or args.mesh or args.geometry):
            evaluate_checkpoint(cfg, seq, args.iteration)
        return
    if args.geometry:
        cfg["geometry"] = dict(cfg.get("geometry") or {}, eval=True)
    if args.pointcloud:
        cfg["pointcloud"] = dict(cfg.get("pointcloud") or {}, export=True)
    if args.mesh:
        cfg["mesh"] = dict(cfg.get("mesh") or {}, export=True)
    os.makedirs(outdir, exist_ok=True)
    seq = build_sequence(cfg, args.frames, args.gaussians)
    slam = SLAM(cfg, seq)
    times, t_last = [], [time.perf_counter()]

    def progress(i):
        torch.cuda.synchronize()
        now = time.perf_counter()
        times.append(now - t_last[0]); t_last[0] = now
        err = slam.pose_errors()[-1]
        print(f"frame {i:4d}  {times[-1] * 1e3:8.1f} ms  gaussians {slam.gaussians.get_xyz.shape[0]:7d}  pose error {err * 100:.2f} cm")

    slam.run(progress, reraise=False)          # (the reference's behaviour on a failed frame: print, save, carry on -- reported by the exit code below); checkpoints, the final map and results.npz are written inside (reference formats)
    res = np.load(os.path.join(outdir, "results.npz"), allow_pickle=True)
    print(f"Average Trajectory Error RMSE: {float(res['ate_rmse'])} m; {1.0 / np.mean(times[1:]):.2f} frames/s after frame 0; outputs in {outdir}")
    if args.render:
        print(f"{len(slam.render())} images in {os.path.join(outdir, 'render')}")
    if slam.failure is not None:      # (the reference prints the exception and saves what it has, slam/SLAM.py:494-503; the exit code says so too)
        sys.exit(1)


if __name__ == "__main__":
    main()
