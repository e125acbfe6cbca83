#!/usr/bin/env python
"""A/B of the registration step (point-to-point ICP for the geometry scores) on the sensor meshes of tools/mesh_ab.py at the shapes of the
bench workloads (640x480 and 1200x680): the export's views fused into a 256^3 volume and meshed.  The reference is that mesh sampled at
`--density`, the source the same samples moved by 1 degree about (1, 2, 3) and 1 cm.  Needs the GPU; there is no fall-back.

    python tools/icp_ab.py [--calls 200] [--untimed 20] [--frames 30] [--repeats 3] [--out profiles/r22_icp.jsonl]

Every device timing is taken between device events around every single call, the two sides alternating in the same process: the median,
p10 and p90 of `--calls` calls after `--untimed` calls of each side.

(a) One mm3dgs_icp_point call to convergence (GeometryScorer.icp: the zeroing launch and 2 (iters + 1) launches, no read-back), and that
    time over the passes that ran; against
(b) the same loop as a chain: per pass mm3dgs_rows_move, mm3dgs_nn_query_index, a torch gather and the sums, one read-back and
    eval_utils.align_horn on the host, with the same stop rule.
(c) A host ICP with scipy.spatial.cKDTree (float64 numpy, an SVD per pass, the same stop rule), `--repeats` times, host clock.
(d) mm3dgs_rows_move against geometry.align_rows' torch chain (float64 matmul, one rounding, cat).
(e) A whole SLAM.evaluate_geometry (`estimate: mesh` against the mesh file moved by the same motion) with `geometry.icp` point against
    none, `--repeats` times each after one untimed pass; host clock, device synchronised at both ends."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ab          # noqa: E402  (start, lattice, stat: the same scenes and the same statistics)
import normals_ab       # noqa: E402  (timed, ratio, sensor_mesh, whole_stage)

DEV = mesh_ab.DEV
MAX_DIST, ITERS, REL = 0.1, 30, 1e-6


def motion(deg=1.0, shift=0.01):
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    r = np.deg2rad(deg)
    return np.concatenate([np.eye(3) + np.sin(r) * K + (1.0 - np.cos(r)) * (K @ K), shift * a[:, None]], 1)


def torch_move(rows, A, b):
    """geometry.align_rows' chain."""
    xyz = rows[:, :3].contiguous().view(torch.float32).double() @ A.T + b
    return torch.cat([xyz.float().view(torch.int32), rows[:, 3:]], 1).contiguous()


def stopped(k, n, fit, rmse, before):
    if before is not None and abs(fit - before[0]) < REL and abs(rmse - before[1]) < REL:
        return 0
    return 2 if n < 3 else (1 if k == ITERS else -1)


def chain_icp(geo, scorer, src, ref_xyz):
    """(b): returns (T, passes)."""
    from mm3dgs_slam_amd.eval_utils import align_horn
    nq = int(src.shape[0])
    dist, row, index = torch.empty(nq, dtype=torch.float32, device=DEV), torch.zeros(8, dtype=torch.float64, device=DEV), torch.empty(nq, dtype=torch.int32, device=DEV)
    p_all = src[:, :3].contiguous().view(torch.float32).double()
    T, before = np.eye(3, 4), None
    for k in range(ITERS + 1):
        moved = geo.move_rows(src, torch.from_numpy(T.reshape(12)).to(DEV), DEV)
        scorer.query(moved, dist=dist, row=row, index=index)
        has = index >= 0
        q = ref_xyz[index.clamp(min=0).long()]
        w = has.double()[:, None]
        p, q = p_all * w, q * w
        d = (moved[:, :3].contiguous().view(torch.float32).double() - q) * w
        s = torch.cat([has.sum().double().reshape(1), p.sum(0), q.sum(0), (p[:, :, None] * q[:, None, :]).sum(0).reshape(9), (d * d).sum().reshape(1)]).cpu().numpy()      # the read-back
        n = s[0]
        fit, rmse = (n / nq, float(np.sqrt(s[16] / n))) if n > 0 else (0.0, 0.0)
        if stopped(k, n, fit, rmse, before) >= 0:
            return T, k + 1
        before = (fit, rmse)
        hp, hq = p[has].cpu().numpy(), q[has].cpu().numpy()      # align_horn takes the pairs
        R, t, _ = align_horn(hp.T, hq.T)
        T = np.concatenate([R, t.reshape(3, 1)], 1)
    return T, ITERS + 1


def tree_icp(src_xyz, ref_xyz):
    """(c): returns (T, passes)."""
    from scipy.spatial import cKDTree
    from mm3dgs_slam_amd.eval_utils import align_horn
    tree = cKDTree(ref_xyz)
    T, before = np.eye(3, 4), None
    for k in range(ITERS + 1):
        moved = (src_xyz @ T[:, :3].T + T[:, 3]).astype(np.float32).astype(np.float64)
        d, j = tree.query(moved, distance_upper_bound=MAX_DIST)
        has = np.isfinite(d)
        n = int(has.sum())
        fit, rmse = (n / len(src_xyz), float(np.sqrt((d[has] ** 2).sum() / n))) if n else (0.0, 0.0)
        if stopped(k, n, fit, rmse, before) >= 0:
            return T, k + 1
        before = (fit, rmse)
        R, t, _ = align_horn(src_xyz[has].T, ref_xyz[j[has]].T)
        T = np.concatenate([R, t.reshape(3, 1)], 1)
    return T, ITERS + 1


def kernel_parts(args, emit, shape, ref_mesh):
    from mm3dgs_slam_amd import geometry as geo
    T_true = motion()
    inverse = np.concatenate([T_true[:, :3].T, -(T_true[:, :3].T @ T_true[:, 3:])], 1)
    ref, _ = geo.sample_mesh_device(ref_mesh[0], ref_mesh[1], args.density, 0, 1 << 26, DEV)
    src = geo.move_rows(ref, inverse, DEV)      # reference = T_true source
    ref_xyz = ref[:, :3].contiguous().view(torch.float32).double()
    scorer = geo.GeometryScorer(ref, 0.05, MAX_DIST, 0.05, DEV)
    nq = int(src.shape[0])
    sizes = dict(shape=shape, source_rows=nq, reference_rows=int(ref.shape[0]), density=args.density, max_dist=MAX_DIST, iters=ITERS, rel=REL, calls=args.calls, untimed=args.untimed)
    out = scorer.icp(src, MAX_DIST, ITERS, REL, REL)
    state, log = out["state"].cpu().numpy(), out["log"].cpu().numpy()
    passes = int(state[12])
    Tc, chain_passes = chain_icp(geo, scorer, src, ref_xyz)
    us = normals_ab.timed((("device", lambda: scorer.icp(src, MAX_DIST, ITERS, REL, REL)), ("chain", lambda: chain_icp(geo, scorer, src, ref_xyz))), args.calls, args.untimed)
    emit(dict(sizes, part="a+b", device_us=mesh_ab.stat(us["device"]), device_us_per_pass=round(statistics.median(us["device"]) / passes, 2), device_passes=passes,
              device_status=int(state[13]), fitness=[float(log[0, 3]), float(log[passes - 1, 3])], rmse=[float(log[0, 4]), float(log[passes - 1, 4])],
              chain_us=mesh_ab.stat(us["chain"]), chain_us_per_pass=round(statistics.median(us["chain"]) / chain_passes, 2), chain_passes=chain_passes,
              chain_over_device_median=normals_ab.ratio(us, "chain", "device"), max_T_error_device=float(np.abs(state[:12].reshape(3, 4) - T_true).max()),
              max_T_error_chain=float(np.abs(Tc - T_true).max())))
    src_xyz, ref_np = src[:, :3].contiguous().view(torch.float32).double().cpu().numpy(), ref_xyz.cpu().numpy()
    ms_ = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        Tt, tree_passes = tree_icp(src_xyz, ref_np)
        ms_.append((time.perf_counter() - t0) * 1e3)
    emit(dict(sizes, part="c", tree_ms=dict(median=round(statistics.median(ms_), 3), min=round(min(ms_), 3), max=round(max(ms_), 3)), tree_passes=tree_passes,
              repeats=args.repeats, max_T_error_tree=float(np.abs(Tt - T_true).max())))
    Td = torch.from_numpy(T_true.reshape(12)).to(DEV)
    A, b = torch.from_numpy(T_true[:, :3].copy()).to(DEV), torch.from_numpy(T_true[:, 3].copy()).to(DEV)
    us = normals_ab.timed((("torch", lambda: torch_move(src, A, b)), ("device", lambda: geo.move_rows(src, Td, DEV))), args.calls, args.untimed)
    emit(dict(sizes, part="d", torch_us=mesh_ab.stat(us["torch"]), device_us=mesh_ab.stat(us["device"]), torch_over_device_median=normals_ab.ratio(us, "torch", "device"),
              words_that_differ=int((torch_move(src, A, b) != geo.move_rows(src, Td, DEV)).sum())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--untimed", type=int, default=20)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--density", type=float, default=10000.0, help="surface samples per m^2 (the `geometry` block's default)")
    ap.add_argument("--gaussians", type=int, default=150000, help="size of the synthetic ground-truth scene (bench.py's default)")
    ap.add_argument("--out", default="", help="append the lines to this file as well")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"

    def emit(d):
        d = dict(d, device=torch.cuda.get_device_name(0))
        print(json.dumps(d), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    from mm3dgs_slam_amd import geometry as geo, mesh as ms
    with tempfile.TemporaryDirectory() as tmp:
        for H, W in mesh_ab.SHAPES:
            shape = f"{W}x{H}"
            slam, seq = mesh_ab.start(args, H, W, tmp)
            for i in range(args.frames):
                slam.gt_pose_list[i] = seq[i][2].clone()
            origin, voxel, trunc, box = mesh_ab.lattice(slam, 1, "sensor")
            with torch.no_grad():
                ref = normals_ab.sensor_mesh(slam, voxel, box)
            kernel_parts(args, emit, shape, ref)
            pad = 5.0 * voxel
            mesh_block = dict(slam.cfg.get("mesh") or {}, bounds=[float(v) for v in np.concatenate([box[:3] - pad, box[3:] + pad])], voxel=voxel, every=1, source="sensor")
            moved_file = ms.write_mesh_ply(os.path.join(tmp, f"reference_{shape}.ply"), geo.move_rows(ref[0], motion(), DEV), ref[1])

            def evaluate(on):
                slam.cfg["mesh"] = dict(mesh_block)
                slam.cfg["geometry"] = dict(slam.cfg.get("geometry") or {}, eval=False, estimate="mesh", reference=moved_file, density=args.density, icp="point" if on else "none")
                return slam.evaluate_geometry(path=os.path.join(tmp, "geometry"))

            normals_ab.whole_stage(args, emit, "e", shape, slam, evaluate, "geometry.icp",
                                   lambda out: dict(points=[out["n_estimate"], out["n_reference"]], accuracy=out["accuracy"], completion=out["completion"],
                                                    icp={k: v for k, v in out["icp"].items() if k != "T"}))
            del slam, seq
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
