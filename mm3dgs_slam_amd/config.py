"""YAML config loader with the reference's schema (``configs/config.py:4-18``, keys as in ``configs/TUM.yml`` /
``configs/UTMM.yml``) plus ``default_config`` -- the TUM.yml hot-path settings as a dict for synthetic runs."""
import copy

import yaml


def load_config(path):
    with open(path, "r") as f:
        return yaml.safe_load(f)


_TUM = {
    "dataset": "synthetic", "device": "cuda:0", "method": "vigs", "use_gt_depth": True,
    # use_gt_depth false: the per-frame least-squares fit of the monocular estimate to the map from mm3dgs_align_depth (two launches,
    # sums and solve in double) instead of the torch operator graph; opt-in, it also records every frame's fit (results.npz: depth_align)
    "depth_align_on_device": False, "white_background": False,
    # the evaluation at the end of a run (PSNR, SSIM, and the depth L1 the host chain does not have) from mm3dgs_eval_image: two launches per
    # frame into a table on the device, one read-back per evaluation; opt-in (results.npz: eval_table, eval_frames, depth_l1_list)
    "eval_on_device": False,
    # after the run, the reconstruction as a fused coloured point cloud (outputdir/pointcloud/cloud.ply + trajectory.ply; pointcloud.py,
    # mm3dgs_pointcloud_add_view): every `every`-th frame (None: mapping.kf_every) lifted to world points -- source "render": the map
    # rendered at the estimated pose where the silhouette exceeds sil_min, "sensor": the frame's own colour and depth --, depths beyond
    # max_depth dropped (0: no limit), one point per `voxel`-sized cell (0: no thinning), at most max_points rows; opt-in, changes no pose
    "pointcloud": {"export": False, "every": None, "voxel": 0.01, "source": "render", "sil_min": 0.99, "max_depth": 0, "max_points": 16777216},
    # after the run, the reconstruction as a coloured triangle mesh (outputdir/mesh/mesh.ply; mesh.py, mm3dgs_tsdf_integrate +
    # mm3dgs_tsdf_mesh_plan / _emit): the same views as the point cloud fused into a dense truncated signed distance volume of `voxel`-sized
    # cells (trunc 0: 4 voxel) over `bounds` ([xmin, ymin, zmin, xmax, ymax, zmax]; None: the box of the views' lifted valid points, grown by
    # trunc + voxel), then marching tetrahedra over the samples seen at least min_weight times; a lattice above max_voxels samples is an
    # error; opt-in, changes no pose (further keys of the block, with their defaults: MESH_CLEAN below)
    "mesh": {"export": False, "every": None, "voxel": 0.02, "trunc": 0, "source": "render", "sil_min": 0.99, "max_depth": 0, "min_weight": 1,
             "bounds": None, "max_voxels": 1 << 28},
    # after the run, the exported geometry scored against a reference surface (outputdir/geometry/metrics.json + accuracy.ply +
    # completion.ply; geometry.py, mm3dgs_nn_grid_build / mm3dgs_nn_query / mm3dgs_mesh_sample_*): `estimate` mesh / pointcloud = what the
    # `mesh` / `pointcloud` block exports (its every, source and sizes); `reference` "sensor" = the same frames' colour and sensor depth
    # fused by the same builder at the ground-truth poses, or the path of a PLY cloud or mesh; accuracy, completion, completion ratio /
    # precision / recall / F-score at `threshold`, Chamfer distance, from nearest-neighbour distances truncated at max_dist through a grid of
    # `cell`-sized cells (0: threshold); meshes sampled at `density` points per m^2 (`seed`, at most max_samples); `align` none / horn /
    # umeyama moves the estimate by the trajectory alignment first; opt-in, changes no pose and no other output
    "geometry": {"eval": False, "estimate": "mesh", "reference": "sensor", "threshold": 0.05, "max_dist": 1.0,
                 "density": 10000.0, "cell": 0, "seed": 0, "align": "none", "max_samples": 16777216},
    # (further keys of the block, with their defaults: GEOMETRY_CULL and GEOMETRY_DEPTH below)
    "scene_radius_depth_ratio": 2, "desired_height": 480, "desired_width": 640,
    "debug": {"get_runtime_stats": False, "create_video": False, "save_keyframes": False},
    "pipeline": {"convert_SHs_python": False, "compute_cov3D_python": False, "transform_means_python": True,
                 "force_isotropic": False, "use_rgb": False},
    "tracking": {"iters": 100, "use_gt_pose": False, "dynamics_model": "const_velocity", "use_imu_loss": False,
                 "imu_T_weight": 0.0, "imu_q_weight": 0.0, "use_depth_estimate_loss": False, "pearson_weight": 0.05,
                 "position_lr": 0.001, "rotation_lr": 0.003,
                 # dynamics_model imu: the start pose from mm3dgs_propagate_imu (one double-precision lane, no pose read-back) instead of
                 # the float32 torch chain on the host; opt-in, the two differ in the last bits
                 "imu_on_device": False},
    "mapping": {"iters": 150, "kf_every": 5, "niqe_kf": False, "niqe_window_size": 5, "kf_window_size": 25,
                "covisibility_level": 1, "min_covisibility": 0.95, "kf_covisibility": 0.1, "do_BA": False,
                "use_depth_estimate_loss": True, "pearson_weight": 0.05, "sh_degree": 0, "cam_t_lr": 0.001,
                "cam_q_lr": 0.003, "position_lr_init": 0.0001, "position_lr_final": 0.0000016,
                "position_lr_delay_mult": 0.01, "position_lr_max_steps": 30000, "feature_lr": 0.0025, "opacity_lr": 0.05,
                "scaling_lr": 0.001, "rotation_lr": 0.001, "rgb_lr": 0.0025, "spatial_lr_scale": 1, "percent_dense": 0.01,
                "lambda_dssim": 0.2, "min_opacity": 0.005, "densification_interval": 50, "pruning_interval": 50,
                "size_threshold": 100, "opacity_reset_interval": 500, "densify_from_iter": 0, "densify_until_iter": 50,
                "densify_grad_threshold": 0.0002},
    "cam": {"image_height": 480, "image_width": 640, "fx": 517.3, "fy": 516.5, "cx": 318.6, "cy": 255.3,
            "crop_edge": 8, "png_depth_scale": 5000.0, "fps": 30},
}


# Optional keys of the `geometry` block and their defaults (export.options merges them under the block; they are kept out of the default
# block itself, whose exact contents a test pins): before scoring, both surfaces are culled to what the cameras of the run saw (cull.py,
# mm3dgs_cull_mark_view / mm3dgs_cull_select) -- the views are the frames the scored export uses, at their ground-truth poses.  `cull`
# none / frustum (inside some view's image and depth range) / occlusion (also not behind the frame's sensor depth by more than cull_eps;
# 0: the block's `threshold` -- a point farther behind the measured surface than the score's own threshold cannot count as within it
# anyway); cull_near / cull_far: the depth range in metres (far 0: no limit); a point is kept when at least cull_min_views views see it
GEOMETRY_CULL = {"cull": "none", "cull_eps": 0, "cull_near": 0, "cull_far": 0, "cull_min_views": 1}


# Further optional keys of the `geometry` block (merged the same way, kept apart for the same reason): what needs a mesh rendered to a depth
# image from a camera (mesh_depth.py, mm3dgs_mesh_depth_render / mm3dgs_depth_compare).  `depth_l1`: after the 3D scores, the estimate
# mesh and the reference mesh are rendered at the views the culling uses (the frames the scored export takes, at their ground-truth poses;
# cull_near / cull_far are the depth range) and the mean absolute depth difference goes to metrics.json (`depth_l1`) and
# outputdir/geometry/depth_l1.npz -- needs `estimate: mesh` and a mesh as the reference.  `cull_depth` sensor / reference: what
# `cull: occlusion` tests against, the frame's sensor depth or the reference mesh rendered at the view (no frame needs sensor depth then).
# depth_max_pairs: the room of one view's tile lists in (tile, triangle) pairs; 2^25 (128 MB of uint32 pairs) is a placeholder, not a
# measured default: the need grows with the triangles and with the image, and a view that exceeds it raises
GEOMETRY_DEPTH = {"depth_l1": False, "cull_depth": "sensor", "depth_max_pairs": 1 << 25}


# Optional keys of the `mesh` block and their defaults (export.options merges them under the block; kept out of the default block for the
# same reason): after the extraction, the mesh's small disconnected pieces are removed (mesh_clean.py, mm3dgs_mesh_components /
# mm3dgs_mesh_clean_plan / _emit) -- from mesh.ply and from both meshes of the geometry evaluation, which share the block.  `clean` none /
# small (drop the components -- vertices joined through triangles -- of fewer than clean_min_triangles triangles) / largest (keep the one
# component with the most triangles).  clean_min_triangles: 100 is a placeholder, not a measured default: the right value depends on
# mesh.voxel (a piece of a given size has more triangles at a finer voxel)
MESH_CLEAN = {"clean": "none", "clean_min_triangles": 100}

# Further optional keys of the `mesh` block (merged the same way): `volume` dense / sparse.  dense (the default) is the lattice over the
# box of everything the cameras saw, 24 bytes per sample, capped by max_voxels.  sparse allocates 8 x 8 x 8-sample blocks only where a depth
# pixel puts the truncation band (mesh.SparseTsdfVolume, mm3dgs_tsdf_blocks_*): a reservation pass over the views replaces the bounds
# pass, max_voxels is not consulted, the lattice is anchored at the world origin, trunc may be at most 16 voxel, and at most max_blocks
# blocks (1 .. 2^21; 12 KiB each) are held -- more is an error that names the key.  max_blocks: 2^18 (3 GiB of pool when all are used) is a
# placeholder, not a measured default
MESH_VOLUME = {"volume": "dense", "max_blocks": 1 << 18}

# Normals (geometry.py: the face cross product, mm3dgs_normal_consistency / mm3dgs_mesh_vertex_normals), two more opt-in keys merged the
# same way and kept apart for the same reason.  `geometry.normals`: the evaluation also scores normal consistency -- the mean |dot| of the
# face normal under a sample and the face normal under its nearest sample of the other surface, both directions -- into the `normals`
# block of metrics.json and outputdir/geometry/normals.npz; needs `estimate: mesh` and a mesh as the reference.  `mesh.normals`: mesh.ply
# carries area-weighted vertex normals of the final (cleaned) mesh, `float nx ny nz` behind the position
GEOMETRY_NORMALS = {"normals": False}
MESH_NORMALS = {"normals": False}

# Registration (geometry.py: icp_host / register, mm3dgs_icp_point / mm3dgs_rows_move), five more opt-in keys of the `geometry` block merged
# the same way and kept apart for the same reason.  `icp` none / point: after `align` and before culling and scoring, the estimate is
# registered to the reference by point-to-point ICP, as NICE-SLAM's eval_recon does before it measures (metrics.json gains an `icp` block,
# outputdir/geometry/icp.npz the transform and the per-pass log).  icp_max_dist: the correspondence distance in metres; icp_iters: at most
# this many solves; icp_rel_fitness / icp_rel_rmse: the loop stops when both figures change by less between two passes.  The four numbers
# are Open3D's registration_icp defaults (30, 1e-6, 1e-6) and NICE-SLAM's 0.1 m threshold, not measured defaults of ours
GEOMETRY_ICP = {"icp": "none", "icp_max_dist": 0.1, "icp_iters": 30, "icp_rel_fitness": 1e-6, "icp_rel_rmse": 1e-6}

# configs/UTMM.yml's hot-path settings that differ from TUM.yml (BASELINE.json configs[2]: RGB-D + IMU): 640x330, intrinsics of the
# 1280x660 sensor scaled by 1/2 (gradslam_datasets/datautils.py:73-118), isotropic Gaussians, IMU dead-reckoning for the pose
# prediction, Pearson term in tracking, 0.002 pose learning rates, size threshold 200.
_UTMM_DELTA = {
    "desired_height": 330, "desired_width": 640,
    "pipeline": {"force_isotropic": True},
    "tracking": {"dynamics_model": "imu", "use_depth_estimate_loss": True, "pearson_weight": 0.001, "position_lr": 0.002, "rotation_lr": 0.002},
    "mapping": {"pearson_weight": 0.001, "cam_t_lr": 0.002, "cam_q_lr": 0.002, "size_threshold": 200},
    "cam": {"image_height": 330, "image_width": 640, "fx": 642.6510620117188 / 2, "fy": 641.807373046875 / 2, "cx": 654.4762573242188 / 2,
            "cy": 359.5939025878906 / 2, "png_depth_scale": 1000.0, "fps": 30},
}


def utmm_config(device="cuda:0", **overrides):
    """configs/UTMM.yml's hot-path settings on the synthetic sequence (ground-truth depth, NIQE filter off)."""
    cfg = copy.deepcopy(_TUM)
    cfg["device"] = device
    for k, v in _UTMM_DELTA.items():
        if isinstance(v, dict):
            cfg[k].update(v)
        else:
            cfg[k] = v
    for k, v in overrides.items():
        if isinstance(v, dict):
            cfg[k].update(v)
        else:
            cfg[k] = v
    return cfg


def default_config(device="cuda:0", height=480, width=640, **overrides):
    """configs/TUM.yml's hot-path settings (iteration budgets, learning rates, pipeline flags) with ground-truth depth
    (no monocular network offline) and the NIQE keyframe filter off.  Intrinsics scale with the image size."""
    cfg = copy.deepcopy(_TUM)
    cfg["device"] = device
    sx, sy = width / 640.0, height / 480.0
    cfg["desired_height"], cfg["desired_width"] = height, width
    for k, s in (("fx", sx), ("cx", sx), ("fy", sy), ("cy", sy)):
        cfg["cam"][k] = _TUM["cam"][k] * s
    for k, v in overrides.items():
        if isinstance(v, dict):
            cfg[k].update(v)
        else:
            cfg[k] = v
    return cfg
