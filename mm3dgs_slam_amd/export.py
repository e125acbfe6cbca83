"""The post-run stage of a SLAM object: what is made of the finished map and trajectory, after ``results.npz``, which it does not touch --
``pointcloud.export`` / ``export_pointcloud`` (``pointcloud.py``), ``mesh.export`` / ``export_mesh`` (``mesh.py``) and ``geometry.eval`` /
``evaluate_geometry`` (``geometry.py``).  Plain functions of the ``SLAM`` object, which keeps the three drivers as methods; ``options`` is
the one place a config block is resolved, ``run_post`` what ``SLAM.run`` ends in."""
import os

import numpy as np
import torch

from . import cull as cl, geometry as geo, mesh as ms, mesh_clean as mc, mesh_depth as md, pointcloud as pc
from .config import _TUM, GEOMETRY_CULL, GEOMETRY_DEPTH, GEOMETRY_ICP, GEOMETRY_NORMALS, MESH_CLEAN, MESH_NORMALS, MESH_VOLUME


def _flag(key, value):
    if value is None:
        return False
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"{key} = {value!r} (true / false)")
    return bool(value)


def options(cfg, block, **overrides):
    """The `pointcloud`, `mesh` or `geometry` block of `cfg` merged over the defaults, an override that is not None over both, resolved
    and validated: `every` (None: `mapping.kf_every`), `voxel`, `source` and the mesh's `trunc` (0: 4 voxel), `clean` and
    `clean_min_triangles` of an export; `estimate`, `reference`, `align` and the `icp` keys of the evaluation."""
    opt = dict(_TUM[block], **(cfg.get(block) or {}))
    if block == "geometry":
        opt = dict(GEOMETRY_ICP, **dict(GEOMETRY_NORMALS, **dict(GEOMETRY_DEPTH, **dict(GEOMETRY_CULL, **opt))))
        opt.update((k, v) for k, v in overrides.items() if v is not None)
        opt.update(estimate=str(opt["estimate"]), reference=str(opt["reference"]), align=str(opt["align"] or "none").lower(),
                   cull=str(opt["cull"] or "none").lower())
        if opt["estimate"] not in ("mesh", "pointcloud"):
            raise ValueError(f"geometry.estimate = {opt['estimate']!r} (mesh / pointcloud)")
        if opt["align"] not in ("none", "horn", "umeyama"):
            raise ValueError(f"geometry.align = {opt['align']!r} (none / horn / umeyama)")
        if opt["cull"] not in cl.MODES:
            raise ValueError(f"geometry.cull = {opt['cull']!r} (none / frustum / occlusion)")
        try:
            near, far, eps, min_views = cl.check_options(opt["cull_near"] or 0, opt["cull_far"] or 0, opt["cull_eps"] or 0, opt["cull_min_views"])
        except (TypeError, ValueError) as e:
            raise ValueError(f"geometry.cull_near / cull_far / cull_eps / cull_min_views: {e}") from None
        opt.update(cull_near=near, cull_far=far, cull_eps=eps if eps > 0 else float(opt["threshold"]), cull_min_views=min_views)
        opt.update(depth_l1=bool(opt["depth_l1"]), cull_depth=str(opt["cull_depth"] or "sensor").lower())
        if opt["cull_depth"] not in ("sensor", "reference"):
            raise ValueError(f"geometry.cull_depth = {opt['cull_depth']!r} (sensor / reference)")
        pairs = opt["depth_max_pairs"]
        if isinstance(pairs, bool) or not isinstance(pairs, (int, np.integer)) or not 1 <= int(pairs) <= md.MAX_PAIRS:
            raise ValueError(f"geometry.depth_max_pairs = {pairs!r} (an integer, 1 .. 2^31)")
        opt["depth_max_pairs"] = int(pairs)
        opt["normals"] = _flag("geometry.normals", opt["normals"])
        opt["icp"] = str(opt["icp"] or "none").lower()
        if opt["icp"] not in ("none", "point"):
            raise ValueError(f"geometry.icp = {opt['icp']!r} (none / point)")
        for key in ("icp_max_dist", "icp_iters", "icp_rel_fitness", "icp_rel_rmse"):
            if isinstance(opt[key], bool) or not isinstance(opt[key], (int, float, np.integer, np.floating)):
                raise ValueError(f"geometry.{key} = {opt[key]!r} (a number)")
        try:
            opt["icp_max_dist"], opt["icp_iters"], opt["icp_rel_fitness"], opt["icp_rel_rmse"] = geo._check_icp(opt["icp_max_dist"], opt["icp_iters"],
                                                                                                             opt["icp_rel_fitness"], opt["icp_rel_rmse"])
        except ValueError as e:
            raise ValueError(f"geometry.{e}") from None
        cell = float(opt["cell"]) if opt["cell"] and float(opt["cell"]) > 0 else float(opt["threshold"])
        if not float(np.ceil(opt["icp_max_dist"] / cell)) <= geo.MAX_RINGS:
            raise ValueError(f"geometry.icp_max_dist = {opt['icp_max_dist']} over a cell of {cell} (at most 2^20 rings)")
        return opt
    if block == "mesh":
        opt = dict(MESH_NORMALS, **dict(MESH_VOLUME, **dict(MESH_CLEAN, **opt)))
    opt["every"] = opt["every"] or cfg["mapping"]["kf_every"]
    opt.update((k, v) for k, v in overrides.items() if v is not None)
    every, voxel, source = int(opt["every"]), float(opt["voxel"]), str(opt["source"])
    opt.update(every=every, voxel=voxel, source=source)
    if source not in ("render", "sensor"):
        raise ValueError(f"{block}.source = {source!r} (render / sensor)")
    if every < 1:
        raise ValueError(f"{block}.every = {every} (must be positive)")
    if block == "mesh":
        if not (np.isfinite(voxel) and voxel > 0):
            raise ValueError(f"{block}.voxel = {voxel} (must be positive)")
        opt["trunc"] = float(opt["trunc"]) if float(opt["trunc"] or 0) > 0 else 4.0 * voxel
        opt["clean"] = str(opt["clean"] or "none").lower()
        if opt["clean"] not in mc.MODES:
            raise ValueError(f"mesh.clean = {opt['clean']!r} (none / small / largest)")
        try:
            opt["clean_min_triangles"] = mc.check_options("small", opt["clean_min_triangles"])[1]
        except (TypeError, ValueError):
            raise ValueError(f"mesh.clean_min_triangles = {opt['clean_min_triangles']!r} (an integer, at least 1)") from None
        opt["normals"] = _flag("mesh.normals", opt["normals"])
        opt["volume"] = str(opt["volume"] or "dense").lower()
        if opt["volume"] not in ("dense", "sparse"):
            raise ValueError(f"mesh.volume = {opt['volume']!r} (dense / sparse)")
        blocks = opt["max_blocks"]
        if isinstance(blocks, bool) or not isinstance(blocks, (int, np.integer)) or not 1 <= int(blocks) <= ms.MAX_BLOCKS:
            raise ValueError(f"mesh.max_blocks = {blocks!r} (an integer, 1 .. 2^21)")
        opt["max_blocks"] = int(blocks)
        if opt["volume"] == "sparse" and not opt["trunc"] <= ms.MAX_TRUNC_VOXELS * voxel:
            raise ValueError(f"mesh.trunc = {opt['trunc']} with mesh.volume: sparse (at most {ms.MAX_TRUNC_VOXELS} mesh.voxel = {ms.MAX_TRUNC_VOXELS * voxel})")
    return opt


def views(slam, every, source, block, poses=None):
    """The views of an export (`pointcloud`, `mesh`), one (color [3,H,W], depth [H,W], silhouette [H,W] or None, pose [7]) per frame with
    `idx % every == 0` that has an estimated pose: `source` "render": the map rendered at that pose with its rendered silhouette;
    "sensor": the frame's own colour and sensor depth.  `poses` (one per frame, None: the estimated ones) replaces the pose of every
    view -- the geometry evaluation's reference places the same frames at their ground-truth poses."""
    for idx in range(len(slam.seq)):
        pose = slam.estimate_pose_list[idx]
        if pose is None or idx % every != 0:
            continue
        if poses is not None:
            pose = poses[idx]
        if source == "render":
            result = slam.renderer.render(slam.gaussians, camera_pose=pose)
            yield result["render"], result["depth"][0], result["depth"][1], pose
        else:
            color, depth, _ = slam.seq[idx]
            if depth is None:
                raise ValueError(f'{block}.source "sensor": frame {idx} has no sensor depth')
            yield color, depth, None, pose


def gt_poses(slam):
    """One ground-truth pose per frame for the geometry evaluation's reference: `gt_pose_list` as the run filled it, else (a resumed
    checkpoint, which ran no frame) `pose_gt` of `outputdir/results.npz`."""
    poses = list(slam.gt_pose_list)
    if any(p is None for p, e in zip(poses, slam.estimate_pose_list) if e is not None) and "outputdir" in slam.cfg:
        stored = os.path.join(slam.cfg["outputdir"], "results.npz")
        if os.path.exists(stored):
            for i, p in enumerate(np.load(stored, allow_pickle=True)["pose_gt"][:len(poses)]):
                if poses[i] is None:
                    poses[i] = torch.tensor(p, device=slam.cfg["device"])
    missing = [i for i, (p, e) in enumerate(zip(poses, slam.estimate_pose_list)) if e is not None and p is None]
    if missing:
        raise ValueError(f'geometry.reference "sensor": no ground-truth pose for frame(s) {missing[:8]} (neither from the run nor in results.npz)')
    return poses


def scored_frames(slam, block):
    """The frames the scored export uses: `idx % every == 0` with an estimated pose."""
    return [idx for idx in range(len(slam.seq)) if slam.estimate_pose_list[idx] is not None and idx % block["every"] == 0]


def mesh_renderer(slam, opt, mesh):
    """pose -> the depth image [H,W] of the mesh (rows, triangles) at that pose over cull_near .. cull_far (mesh_depth.py): a device tensor
    from one mm3dgs_mesh_depth_render call on a GPU, the host statement on `device: cpu`; and `finish()`, which raises when a view's
    tile lists lacked room (`geometry.depth_max_pairs`)."""
    cfg, cam = slam.cfg, slam.cfg["cam"]
    H, W = int(cfg["desired_height"]), int(cfg["desired_width"])
    if str(cfg["device"]).startswith("cuda"):
        r = md.MeshDepth(mesh[0], mesh[1], H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"], opt["cull_near"], opt["cull_far"], opt["depth_max_pairs"], cfg["device"])
        return (lambda pose: r.render(pose, want_tri=False)[0]), r.finish
    rows, tris = pc.as_np(mesh[0], np.int32), pc.as_np(mesh[1], np.int32)
    return (lambda pose: md.render_host(rows, tris, pose, H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"], opt["cull_near"], opt["cull_far"])[0]), (lambda: None)


def cull_views(slam, opt, block, reference=None):
    """The ``cull=`` argument of the geometry evaluation (None with `cull: none`): one view per frame the scored export uses (`idx % every
    == 0` with an estimated pose), placed at its ground-truth pose -- the reference lives in the ground-truth frame, and the estimate has
    been moved there by `geometry.align`.  "occlusion": each view carries the frame's sensor depth (ValueError naming the frame without
    one; depths beyond the export block's `max_depth` see nothing), or with `cull_depth: reference` the depth of the `reference` mesh
    (rows, triangles) rendered at the view (ValueError when the reference is not a mesh; no frame is read); "frustum": no frame is read.
    `opt`, `block`: `options` of the `geometry` block and of the estimate's."""
    if opt["cull"] == "none":
        return None
    poses, out = gt_poses(slam), []
    render = finish = None
    if opt["cull"] == "occlusion" and opt["cull_depth"] == "reference":
        if not geo._is_mesh(reference):
            raise ValueError('geometry.cull_depth "reference": the reference is not a mesh (`reference: sensor` with `estimate: mesh`, or a PLY file with faces)')
        render, finish = mesh_renderer(slam, opt, reference)
    for idx in scored_frames(slam, block):
        depth = None
        if render is not None:
            depth = render(poses[idx].detach())
        elif opt["cull"] == "occlusion":
            depth = slam.seq[idx][1]
            if depth is None:
                raise ValueError(f'geometry.cull "occlusion": frame {idx} has no sensor depth')
        out.append((depth, poses[idx].detach()))
    if finish is not None:
        finish()
    return cl.spec(out, int(slam.cfg["desired_height"]), int(slam.cfg["desired_width"]), slam.cfg["cam"], near=opt["cull_near"], far=opt["cull_far"],
                   eps=opt["cull_eps"], min_views=opt["cull_min_views"], depth_max=float(block["max_depth"]))


def cloud_geometry(slam, opt, poses=None):
    """The views of an export lifted and thinned (what `export_pointcloud` writes and `evaluate_geometry` scores): the finished builder
    (its `rows()`: device tensor on a GPU) and its counters.  `opt`: `options` of the `pointcloud` block; `poses` as in `views`."""
    Builder = pc.PointCloudBuilder if str(slam.cfg["device"]).startswith("cuda") else pc.HostPointCloudBuilder
    builder = Builder(int(slam.cfg["desired_height"]), int(slam.cfg["desired_width"]), slam.cfg["cam"], voxel=opt["voxel"], max_points=int(opt["max_points"]), sil_min=float(opt["sil_min"]),
                      depth_max=float(opt["max_depth"]), device=slam.cfg["device"])
    with torch.no_grad():
        for view in views(slam, opt["every"], opt["source"], "pointcloud", poses):
            builder.add(*view)
    return builder, builder.finish()


def mesh_bounds(slam, opt, poses=None):
    """The box [xmin, ymin, zmin, xmax, ymax, zmax] of the lifted valid points of an export's views (`mesh.view_bounds`, view by view); its
    six numbers are read back once, after the last view."""
    lo = hi = None
    for color, depth, sil, pose in views(slam, opt["every"], opt["source"], "mesh", poses):
        a, b = ms.view_bounds(depth, sil, pose, slam.cfg["cam"], float(opt["sil_min"]), float(opt["max_depth"]))
        lo, hi = (a, b) if lo is None else (torch.minimum(lo, a), torch.maximum(hi, b))
    if lo is None:
        raise ValueError("mesh export: no frame has an estimated pose")
    box = torch.cat([lo, hi]).cpu().numpy()          # the one read-back
    if not np.isfinite(box).all():
        raise ValueError("mesh export: no view has a valid pixel (mesh.sil_min, mesh.max_depth)")
    return box


def _extract_clean(volume, opt, device):
    """(rows, triangles, counters) of a filled volume, with `mesh.clean` small / largest cleaned behind the extraction."""
    rows, triangles, counters = volume.extract()
    if opt.get("clean", "none") != "none":
        rows, triangles, _, info = mc.clean(rows, triangles, opt["clean"], opt["clean_min_triangles"], device=device)
        counters = dict(counters, clean=dict(info, mode=opt["clean"], min_triangles=opt["clean_min_triangles"], vertices=int(rows.shape[0]), triangles=int(triangles.shape[0])))
    return rows, triangles, counters


def mesh_geometry(slam, opt, poses=None):
    """The views of an export fused and meshed (what `export_mesh` writes and `evaluate_geometry` scores): (rows, triangles, counters,
    lattice sizes, origin); device tensors on a GPU.  `opt`: `options` of the `mesh` block; `poses` as in `views`.  With `mesh.clean`
    small / largest the mesh is cleaned behind the extraction (mesh_clean.py) and the counters -- which stay those of the extraction --
    carry the cleaning's figures under `clean`."""
    voxel, trunc, cfg = opt["voxel"], opt["trunc"], slam.cfg
    if opt.get("volume", "dense") == "sparse":
        return sparse_mesh_geometry(slam, opt, poses)
    with torch.no_grad():
        if opt["bounds"] is None:
            box = mesh_bounds(slam, opt, poses)
            box[:3] -= trunc + voxel
            box[3:] += trunc + voxel
        else:
            box = np.asarray(opt["bounds"], dtype=np.float64).reshape(6)
        origin, dims = ms.lattice_for(box, voxel, opt["max_voxels"])
        Volume = ms.TsdfVolume if str(cfg["device"]).startswith("cuda") else ms.HostTsdfVolume
        volume = Volume(dims, origin, voxel, trunc, int(cfg["desired_height"]), int(cfg["desired_width"]), cfg["cam"], sil_min=float(opt["sil_min"]),
                        depth_max=float(opt["max_depth"]), min_weight=float(opt["min_weight"]), device=cfg["device"])
        for view in views(slam, opt["every"], opt["source"], "mesh", poses):
            volume.add(*view)
        return _extract_clean(volume, opt, cfg["device"]) + (dims, origin)


def sparse_mesh_geometry(slam, opt, poses=None):
    """`mesh_geometry` with `mesh.volume: sparse`: no bounds pass and no `mesh.max_voxels`; a reservation pass over the views decides which
    8 x 8 x 8-sample blocks exist (`mesh.reserve_host`, mm3dgs_tsdf_blocks_reserve), the set is frozen, and a second pass over the same views
    integrates them.  The same five values; the lattice sizes and the origin describe the block set's bounding lattice, and the counters
    gain `blocks`, `pairs` and `volume_bytes`."""
    cfg = slam.cfg
    Volume = ms.SparseTsdfVolume if str(cfg["device"]).startswith("cuda") else ms.HostSparseTsdfVolume
    with torch.no_grad():
        volume = Volume(opt["voxel"], opt["trunc"], int(cfg["desired_height"]), int(cfg["desired_width"]), cfg["cam"], sil_min=float(opt["sil_min"]),
                        depth_max=float(opt["max_depth"]), min_weight=float(opt["min_weight"]), max_blocks=opt["max_blocks"], bounds=opt["bounds"], device=cfg["device"])
        n = 0
        for _, depth, sil, pose in views(slam, opt["every"], opt["source"], "mesh", poses):
            volume.reserve(depth, sil, pose)
            n += 1
        if n == 0:
            raise ValueError("mesh export: no frame has an estimated pose")
        volume.freeze()
        for view in views(slam, opt["every"], opt["source"], "mesh", poses):
            volume.add(*view)
        return _extract_clean(volume, opt, cfg["device"]) + (volume.dims, volume.origin)


def export_pointcloud(slam, path=None, every=None, voxel=None, source=None):
    """The reconstruction as a fused coloured point cloud (pointcloud.py; the core of the reference's scripts/visualizer.py): for every
    frame with `idx % every == 0` that has an estimated pose one view at that pose -- `source` "render": the map rendered there, with
    the rendered silhouette as the surface test (> `pointcloud.sil_min`, the reference's 0.99); "sensor": the frame's own colour and
    sensor depth -- is lifted to world points, and the first point of every `voxel`-sized cell is kept.  Writes `path/cloud.ply` and
    `path/trajectory.ply` (default `outputdir/pointcloud`); arguments left None come from the `pointcloud` config block.  One
    mm3dgs_pointcloud_add_view call per view on a GPU, the host statement on `device: cpu`.  Returns the two paths and the counters;
    raises RuntimeError when points were dropped for lack of room (`pointcloud.max_points`)."""
    opt = options(slam.cfg, "pointcloud", every=every, voxel=voxel, source=source)
    path = os.path.join(slam.cfg["outputdir"], "pointcloud") if path is None else path
    builder, counters = cloud_geometry(slam, opt)
    poses = [pose.detach() for pose in slam.estimate_pose_list[:len(slam.seq)] if pose is not None]
    os.makedirs(path, exist_ok=True)
    out = {"cloud": pc.write_ply(os.path.join(path, "cloud.ply"), builder.rows()),
           "trajectory": pc.write_trajectory_ply(os.path.join(path, "trajectory.ply"), torch.stack(poses) if poses else np.zeros((0, 7))),
           "counters": counters}
    slam.pointcloud_export = out      # what the last export wrote (run_post calls this without a caller to hand it to)
    print(f"Point cloud: {counters['rows']} points from {counters['views']} views ({counters['valid']} valid pixels, voxel {opt['voxel']} m) in {out['cloud']}")
    return out


def export_mesh(slam, path=None, every=None, voxel=None, source=None):
    """The reconstruction as a coloured triangle mesh (mesh.py): the views of `export_pointcloud` (`every`, `source`) fused into a dense
    truncated signed distance volume of `mesh.voxel`-sized cells (`mesh.trunc`, 0: 4 voxel) over `mesh.bounds` -- None: a first pass
    over the same views takes the box of their lifted valid points, which is grown by trunc + voxel, the origin snapped down to a
    multiple of voxel --, then marching tetrahedra over the samples seen at least `mesh.min_weight` times, and with `mesh.clean` small /
    largest the removal of the small disconnected pieces (mesh_clean.py; the returned dict gains `clean`).  Writes `path/mesh.ply`
    (default `outputdir/mesh`; the format: `mesh.write_mesh_ply`; with `mesh.normals: true` the file carries the area-weighted vertex
    normals of the final mesh, `geometry.vertex_normals`, and the returned dict gains `normals`: its counters).  One mm3dgs_tsdf_integrate call per view and one mm3dgs_tsdf_mesh_plan /
    _emit pair on a GPU, the host statement on `device: cpu`.  Returns the path, the counters and the lattice; raises ValueError when the
    lattice exceeds `mesh.max_voxels`.  With `mesh.volume: sparse` the volume is held in 8 x 8 x 8-sample blocks only where a view's
    truncation band reaches (`sparse_mesh_geometry`): neither the bounds pass nor `mesh.max_voxels`; the returned dict gains `volume`,
    `blocks`, `pairs` and `volume_bytes`; raises ValueError when more than `mesh.max_blocks` blocks are needed."""
    opt = options(slam.cfg, "mesh", every=every, voxel=voxel, source=source)
    path = os.path.join(slam.cfg["outputdir"], "mesh") if path is None else path
    rows, triangles, counters, dims, origin = mesh_geometry(slam, opt)
    os.makedirs(path, exist_ok=True)
    normals = nc = None
    if opt["normals"]:      # of the final mesh: behind mesh.clean
        normals, nc = geo.vertex_normals(rows, triangles, slam.cfg["device"])
    out = {"mesh": ms.write_mesh_ply(os.path.join(path, "mesh.ply"), rows, triangles, normals), "counters": counters, "lattice": tuple(dims),
           "origin": origin.tolist(), "voxel": opt["voxel"], "trunc": opt["trunc"]}
    cleaned = ""
    if nc is not None:
        out["normals"] = nc
    if opt["volume"] == "sparse":
        out.update(volume="sparse", blocks=counters["blocks"], pairs=counters["pairs"], volume_bytes=counters["volume_bytes"])
        cleaned = f"; sparse volume: {counters['blocks']} blocks from {counters['pairs']} (pixel, block) pairs, {counters['volume_bytes']} bytes"
    if "clean" in counters:
        out["clean"] = counters["clean"]
        cleaned = f"; {mc.summary(opt['clean'], opt['clean_min_triangles'], counters['clean'])}"
    slam.mesh_export = out      # what the last export wrote
    print(f"Mesh: {counters['vertices']} vertices, {counters['triangles']} triangles from {counters['views']} views "
          f"(lattice {dims[0]} x {dims[1]} x {dims[2]}, voxel {opt['voxel']} m){cleaned} in {out['mesh']}")
    if nc is not None:
        print(f"Mesh normals: {nc['vertices'] - nc['without_normal']} of {nc['vertices']} vertices ({nc['rejected_triangles']} triangles without an area)")
    return out


def evaluate_geometry(slam, path=None, estimate=None, reference=None):
    """The exported geometry scored against a reference surface (the figures of geometry.py).  `estimate` "mesh" / "pointcloud": what `export_mesh` / `export_pointcloud` produce (their blocks' `every`, `source` and sizes), from their rows in memory.
    `reference` "sensor": the same frames' own colour and sensor depth fused by the same builder at the GROUND-TRUTH poses -- what a
    perfect tracker and map would have exported (ValueError without sensor depth) --, or the path of a PLY file: a point cloud or, with a
    face element, a mesh (`mesh.read_surface_ply`).  Meshes on either side are sampled at `geometry.density` samples per m^2;
    `geometry.align` none / horn / umeyama moves the estimate by the trajectory alignment first; `geometry.icp: point` then registers it to
    the reference by point-to-point ICP (`geometry.register`; metrics.json gains an `icp` block, `path/icp.npz` holds T, log and status;
    fewer than 3 correspondences leave the estimate where it was, and the block says so); `geometry.cull` frustum / occlusion then
    removes from both point sets what no camera of the run could have seen (`cull_views`, cull.py; metrics.json gains a `cull` block;
    `geometry.cull_depth: reference` tests occlusion against the reference mesh rendered at each view instead of the sensor depth).
    `geometry.depth_l1: true` (needs `estimate: mesh` and a mesh as the reference) also renders both meshes -- the unculled ones, the
    estimate after `geometry.align` -- to depth images at the same views over `cull_near` .. `cull_far` (mesh_depth.py) and writes their
    depth L1 as the `depth_l1` block of metrics.json and the per-view table and frame indices to `path/depth_l1.npz`.
    With `mesh.clean` small / largest the estimate mesh and the `reference: sensor` mesh come cleaned from their builder (a reference
    file is left as it is) and metrics.json gains a `mesh_clean` block.  Writes `path/metrics.json`,
    `accuracy.ply` and `completion.ply` (default `outputdir/geometry`); `geometry.normals: true` (the same two needs as `depth_l1`) adds
    normal consistency: the `normals` block of metrics.json and `path/normals.npz`; arguments left None come from the `geometry` config block.  HIP
    kernels and one read-back of the [2,8] table on a GPU, the host statement on `device: cpu`.  Touches no pose and no other output.
    Returns the comparison with the paths."""
    opt = options(slam.cfg, "geometry", estimate=estimate, reference=reference)
    estimate, reference, align = opt["estimate"], opt["reference"], opt["align"]
    block = options(slam.cfg, estimate)

    cleaned = {}

    def build(block, poses, side):
        if estimate == "mesh":
            rows, triangles, counters = mesh_geometry(slam, block, poses)[:3]
            if "clean" in counters:
                cleaned[side] = counters["clean"]
            return rows, triangles
        return cloud_geometry(slam, block, poses)[0].rows()

    est = build(block, None, "estimate")
    if align != "none":
        move = lambda rows: geo.align_rows(rows, slam.estimate_pose_list[:len(slam.seq)], gt_poses(slam), align)
        est = (move(est[0]), est[1]) if estimate == "mesh" else move(est)
    ref = build(dict(block, source="sensor"), gt_poses(slam), "reference") if reference == "sensor" else ms.read_surface_ply(reference)
    if opt["depth_l1"] and not (estimate == "mesh" and geo._is_mesh(ref)):
        raise ValueError("geometry.depth_l1 needs `estimate: mesh` and a mesh as the reference (`reference: sensor`, or a PLY file with faces)")
    if opt["normals"] and not (estimate == "mesh" and geo._is_mesh(ref)):
        raise ValueError("geometry.normals needs `estimate: mesh` and a mesh as the reference (`reference: sensor`, or a PLY file with faces)")
    icp = None
    if opt["icp"] == "point":      # behind `align`, in front of everything that looks at the estimate
        est, icp = geo.register(est, ref, device=slam.cfg["device"], threshold=float(opt["threshold"]), cell=float(opt["cell"] or 0), density=float(opt["density"]),
                                seed=int(opt["seed"]), max_samples=int(opt["max_samples"]), max_dist=opt["icp_max_dist"], iters=opt["icp_iters"],
                                rel_fitness=opt["icp_rel_fitness"], rel_rmse=opt["icp_rel_rmse"])
    culled = {} if opt["cull"] == "none" else {"cull": cull_views(slam, opt, block, ref)}
    if opt["normals"]:
        culled["normals"] = True
    result = geo.compare(est, ref, device=slam.cfg["device"], threshold=float(opt["threshold"]), max_dist=float(opt["max_dist"]),
                         cell=float(opt["cell"] or 0), density=float(opt["density"]), seed=int(opt["seed"]), max_samples=int(opt["max_samples"]), **culled)
    if "cull" in culled and culled["cull"]["mode"] == "occlusion" and opt["cull_depth"] == "reference":
        result["cull"] = dict(result["cull"], depth="reference")
    path = os.path.join(slam.cfg["outputdir"], "geometry") if path is None else path
    extra = {"estimate": estimate, "reference": reference, "align": align, "density": float(opt["density"]), "seed": int(opt["seed"])}
    if cleaned:
        result["mesh_clean"] = extra["mesh_clean"] = dict(cleaned, mode=block["clean"], min_triangles=block["clean_min_triangles"])
    if icp is not None:
        result["icp"] = extra["icp"] = dict({k: v for k, v in icp.items() if k not in ("T", "log")}, T=np.asarray(icp["T"]).tolist(), status_name=geo.ICP_STATUS[icp["status"]],
                                            moved=icp["status"] != 2, max_dist=opt["icp_max_dist"], iters=opt["icp_iters"], rel_fitness=opt["icp_rel_fitness"],
                                            rel_rmse=opt["icp_rel_rmse"])
    if opt["depth_l1"]:
        frames, poses = scored_frames(slam, block), gt_poses(slam)
        table, summary = md.depth_l1(est, ref, [poses[i].detach() for i in frames], int(slam.cfg["desired_height"]), int(slam.cfg["desired_width"]), slam.cfg["cam"],
                                     near=opt["cull_near"], far=opt["cull_far"], device=slam.cfg["device"], max_pairs=opt["depth_max_pairs"])
        result["depth_l1"] = extra["depth_l1"] = dict(summary, near=opt["cull_near"], far=opt["cull_far"])
        result["depth_l1_table"] = table
    result["files"] = geo.write_outputs(path, result, extra)
    if opt["depth_l1"]:
        result["files"]["depth_l1"] = os.path.join(path, "depth_l1.npz")
        np.savez(result["files"]["depth_l1"], table=table, frames=np.asarray(frames, dtype=np.int64))
    if icp is not None:
        result["files"]["icp"] = os.path.join(path, "icp.npz")
        np.savez(result["files"]["icp"], T=np.asarray(icp["T"], dtype=np.float64), log=np.asarray(icp["log"], dtype=np.float64), status=np.int64(icp["status"]))
    slam.geometry_eval = result      # what the last evaluation found
    t = result["table"]
    print(f"Geometry ({estimate} against {reference}): accuracy {result['accuracy'] * 100:.3f} cm, completion {result['completion'] * 100:.3f} cm, "
          f"completion ratio {result['completion_ratio'] * 100:.2f} % at {float(opt['threshold']) * 100:g} cm, F-score {result['fscore']:.4f}, Chamfer "
          f"{result['chamfer'] * 100:.3f} cm ({result['n_estimate']} / {result['n_reference']} points, clamped {int(t[0, 5])} / {int(t[1, 5])}) in "
          f"{result['files']['metrics']}")
    if icp is not None:
        print(f"ICP ({geo.ICP_STATUS[icp['status']]} after {icp['passes']} passes{'' if icp['status'] != 2 else '; the estimate is left where it was'}): fitness "
              f"{icp['fitness_start']:.4f} -> {icp['fitness']:.4f}, rmse {icp['rmse_start'] * 100:.3f} -> {icp['rmse'] * 100:.3f} cm over {icp['n_source']} / "
              f"{icp['n_reference']} points within {opt['icp_max_dist']} m in {result['files']['icp']}")
    if opt["normals"]:
        nf = result["normals"]
        print(f"Normal consistency: {nf['normal_consistency']:.4f} (normal accuracy {nf['normal_accuracy']:.4f}, normal completion {nf['normal_completion']:.4f}; "
              f"mean |dot| over {int(result['normal_table'][0, 0])} / {int(result['normal_table'][1, 0])} points) in {result['files']['normals']}")
    if opt["depth_l1"]:
        d = result["depth_l1"]
        print(f"Depth L1 ({d['views']} views, {d['empty_views']} empty): {d['mean'] * 100:.3f} cm (pooled {d['pooled'] * 100:.3f} cm, rmse {d['rmse'] * 100:.3f} cm, max "
              f"{d['max'] * 100:.3f} cm, coverage {d['coverage'] * 100:.2f} %) in {result['files']['depth_l1']}")
    return result


# (config block, its switch, the stage, how a failure is reported), in the order they run
POST = (("pointcloud", "export", export_pointcloud, "point cloud export"),
        ("mesh", "export", export_mesh, "mesh export"),
        ("geometry", "eval", evaluate_geometry, "geometry evaluation"))


def run_post(slam):
    """The stages whose block is switched on, each reported and never raised: one that fails takes neither the run nor the next one down."""
    for block, switch, stage, label in POST:
        if (slam.cfg.get(block) or {}).get(switch, False):
            try:
                stage(slam)
            except Exception as e:      # noqa: BLE001
                print(f"({label}: {e!r})")
