#!/usr/bin/env python
"""A/B of the point cloud export at the shapes of the bench workloads (640x480 and 1200x680): one view through
PointCloudBuilder.add (mm3dgs_pointcloud_add_view: three launches without a voxel size, four with one) against the torch chain that does the
same job -- the operator sequence of the reference's rgbd2pcd (scripts/visualizer.py:69-112: index grids, back-projection, a 4x4 inverse and
a matrix product in float32), the surface mask, the colour bytes, and with a voxel size the keys and `torch.unique` over the keys so far.
Needs the GPU; there is no fall-back.

    python tools/pointcloud_ab.py [--calls 200] [--untimed 20] [--frames 30] [--repeats 3] [--out profiles/r14_pointcloud.jsonl]

(a) One view, timed between device events around every single call, torch chain and device call alternating in the same process: the median,
p10 and p90 of `--calls` calls after `--untimed` calls of each side, at voxel 0 and 0.01.  The inputs are the workload's own: the map seeded
and mapped on frame 0, rendered at the poses of two later frames.  With a voxel size both sides add the second view to a cloud that holds the
first: before every timed device call the builder is reset and given the first view (untimed); the torch chain's `torch.unique` runs over the
first view's unique keys and the second view's keys.

(b) A whole SLAM.export_pointcloud over `--frames` views (every 1, voxel 0.01, the default 16.7 M-point buffers: one render and one add per
view, the counters' read-back and the two files) from the same state, `--repeats` times after one untimed pass; host clock, device
synchronised at both ends.  No host-side counterpart was timed."""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
SHAPES = [(480, 640), (680, 1200)]
VOXELS = [0.0, 0.01]
MAX_POINTS = 1 << 21      # part (a): rows 32 MiB, table 64 MiB -- a reset per timed call stays cheap


def start(args, H, W, outdir):
    """The sequence and a SLAM object after frame 0, every later frame at its ground-truth pose (nothing of this is timed)."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    frac = min(1.0, args.gaussians / (0.95 * H * W))      # bench.py's seeding fraction
    cfg = default_config(device=DEV, height=H, width=W, mapping={"seed_fraction": frac}, outputdir=outdir)
    seq = SyntheticSequence(cfg, args.frames, args.gaussians, seed=0)
    slam = SLAM(cfg, seq)
    slam.step(0)
    for i in range(1, args.frames):
        slam.estimate_pose_list[i] = seq[i][2].clone()
    torch.cuda.synchronize()
    return slam, seq


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def torch_keys(pts, voxel):
    cell = torch.floor(pts.double() / voxel).long() + (1 << 20)
    return (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]


def torch_view(color, depth, sil, pose, cam, sil_min):
    """The operator sequence of rgbd2pcd in float32 torch, then the surface mask and the colour bytes: (points [n,3], rgba [n,3] uint8)."""
    from mm3dgs_slam_amd.pose_utils import get_camera_from_tensor
    H, W = depth.shape
    n = H * W
    # the same operators in the same order: two integer index grids, subtract / divide / multiply per axis, a stack, a column of ones,
    # the 4x4 inverse, one [4,4] x [4,n] product, a slice; then the permuted colour image
    col_index = torch.arange(W, device=DEV).tile((H,))
    row_index = torch.arange(H, device=DEV).repeat_interleave(W)
    z = depth.reshape(n)
    ray_x, ray_y = (col_index - cam["cx"]) / cam["fx"], (row_index - cam["cy"]) / cam["fy"]
    homogeneous = torch.cat([torch.stack([ray_x * z, ray_y * z, z], dim=-1), torch.ones(n, 1, device=DEV)], dim=1)
    cam_to_world = torch.inverse(get_camera_from_tensor(pose).float())
    world = (cam_to_world @ homogeneous.T).T[:, :3]
    rgb = color.permute(1, 2, 0).reshape(n, 3)
    surface = (z > 0) & (sil.reshape(n) > sil_min)
    return world[surface], (rgb[surface].clamp(0, 1) * 255.0 + 0.5).to(torch.uint8)


def call_times(slam, args, emit, H, W, voxel):
    """(a): us per added view"""
    from mm3dgs_slam_amd import pointcloud as pc
    cam, sil_min = slam.cfg["cam"], 0.99
    ia, ib = min(5, args.frames - 1), min(6, args.frames - 1)
    with torch.no_grad():
        ra = slam.renderer.render(slam.gaussians, camera_pose=slam.estimate_pose_list[ia])
        rb = slam.renderer.render(slam.gaussians, camera_pose=slam.estimate_pose_list[ib])
    va = (ra["render"].contiguous(), ra["depth"][0].contiguous(), ra["depth"][1].contiguous(), slam.estimate_pose_list[ia])
    vb = (rb["render"].contiguous(), rb["depth"][0].contiguous(), rb["depth"][1].contiguous(), slam.estimate_pose_list[ib])
    builder = pc.PointCloudBuilder(H, W, cam, voxel=voxel, max_points=MAX_POINTS, sil_min=sil_min, depth_max=0.0, device=DEV)
    seen = torch.unique(torch_keys(torch_view(*va, cam, sil_min)[0], voxel)) if voxel > 0 else None

    def prepare():      # untimed: a cloud that holds the first view
        from mm3dgs_slam_amd import _lib
        from mm3dgs_slam_amd.rasterizer import _stream
        _lib.check(builder.lib.mm3dgs_pointcloud_reset(_lib.ptr(builder.table), builder.slots, _lib.ptr(builder.counters), _stream()))
        builder.view, builder._read = 0, None
        if voxel > 0:
            builder.add(*va)

    def device():
        builder.add(*vb)

    def host():
        pts, rgba = torch_view(*vb, cam, sil_min)
        if voxel > 0:
            uniq, inverse = torch.unique(torch.cat([seen, torch_keys(pts, voxel)]), return_inverse=True)
            return uniq, inverse, rgba
        return pts, rgba

    with torch.no_grad():
        for _ in range(args.untimed):
            prepare(); device(); host()
        torch.cuda.synchronize()
        us = {"host": [], "device": []}
        for _ in range(args.calls):
            for side, fn in (("host", host), ("device", device)):
                if side == "device":
                    prepare()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                us[side].append(e0.elapsed_time(e1) * 1e3)
        prepare()
        first = builder.read_counters()      # the cloud before the timed view: empty, or the first view
        device()
        c = builder.read_counters()
        out = host()
    n_host = int(out[0].numel() - seen.numel()) if voxel > 0 else int(out[0].shape[0])
    stat = lambda v: dict(median=round(statistics.median(v), 2), p10=round(pct(v, 0.1), 2), p90=round(pct(v, 0.9), 2))
    emit(dict(part="a", shape=f"{W}x{H}", voxel=voxel, calls=args.calls, untimed=args.untimed, torch_us_per_view=stat(us["host"]),
              device_us_per_view=stat(us["device"]), torch_over_device_median=round(statistics.median(us["host"]) / statistics.median(us["device"]), 3),
              device_faster=bool(statistics.median(us["device"]) < statistics.median(us["host"])), valid_pixels=c["valid"] - first["valid"],
              rows_added_device=c["rows"] - first["rows"], rows_added_torch=n_host, counters=c))


def export_times(slam, args, emit, H, W):
    """(b): ms per export_pointcloud over all frames"""
    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = slam.export_pointcloud(every=1, voxel=0.01, source="render")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    run()
    ms = []
    for _ in range(args.repeats):
        t, out = run()
        ms.append(t)
    emit(dict(part="b", shape=f"{W}x{H}", frames=args.frames, repeats=args.repeats, voxel=0.01, gaussians=int(slam.gaussians.get_xyz.shape[0]),
              ms_export=dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3), max=round(max(ms), 3)),
              ms_per_view=round(statistics.median(ms) / args.frames, 4), cloud_bytes=os.path.getsize(out["cloud"]), counters=out["counters"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--untimed", type=int, default=20)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
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

    with tempfile.TemporaryDirectory() as tmp:
        for H, W in SHAPES:
            slam, seq = start(args, H, W, tmp)
            for voxel in VOXELS:
                call_times(slam, args, emit, H, W, voxel)
            export_times(slam, args, emit, H, W)
            del slam, seq
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
