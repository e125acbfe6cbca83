#!/usr/bin/env python
"""A/B of the mesh export at the shapes of the bench workloads (640x480 and 1200x680) over a 256^3 volume: one view through
TsdfVolume.add (mm3dgs_tsdf_integrate: one launch) against the torch-operator chain that does the same dense update over the whole lattice
(sample grid, rigid transform, projection, a gather of depth, silhouette and colour, the truncation tests, the two running means through
`torch.where`, in float32); marching tetrahedra (mm3dgs_tsdf_mesh_plan + mm3dgs_tsdf_mesh_emit) on that volume; and a whole
SLAM.export_mesh.  Needs the GPU; there is no fall-back.

    python tools/mesh_ab.py [--calls 200] [--untimed 20] [--frames 30] [--repeats 3] [--out profiles/r15_mesh.jsonl]

(a) One view, timed between device events around every single call, torch chain and device call alternating in the same process: the median,
p10 and p90 of `--calls` calls after `--untimed` calls of each side.  The inputs are the workload's own: the map seeded and mapped on frame
0, rendered at the pose of a later frame (source "render": the surface pixels are those with silhouette > 0.99, few of them after one
mapped frame at 1200x680), or that frame's own colour and sensor depth (source "sensor": every pixel valid, the most work a view can be);
the lattice is the box of the export's views at 256 samples along its longest side, padded to 256^3.  Both sides keep integrating the same view into their own volume (the weights grow, the work per call does not change).

(b) plan + emit on the device volume after every view of the export went in, `--calls` times between device events, the rows and triangles
allocated once from the first plan's totals.  No torch counterpart exists (no marching-cubes operator), none was timed.

(c) A whole SLAM.export_mesh over `--frames` views (every 1, the same box and voxel size: the bounds pass is skipped, one render and one
integrate per view, plan, the totals' read-back, emit, the file) from the same state, `--repeats` times after one untimed pass; host clock,
device synchronised at both ends."""
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
SIDE = 256


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


def stat(v):
    return dict(median=round(statistics.median(v), 2), p10=round(pct(v, 0.1), 2), p90=round(pct(v, 0.9), 2))


class TorchVolume:
    """The dense update with torch operators, float32, over the whole lattice."""

    def __init__(self, dims, origin, voxel, trunc, cam, sil_min):
        nx, ny, nz = dims
        self.T = torch.zeros(nz, ny, nx, device=DEV)
        self.W = torch.zeros(nz, ny, nx, device=DEV)
        self.C = torch.zeros(3, nz, ny, nx, device=DEV)
        self.CW = torch.zeros(nz, ny, nx, device=DEV)
        self.dims, self.origin, self.voxel, self.trunc, self.cam, self.sil_min = dims, [float(v) for v in origin], float(voxel), float(trunc), cam, sil_min

    def add(self, color, depth, sil, pose):
        from mm3dgs_slam_amd.pose_utils import get_camera_from_tensor
        nx, ny, nz = self.dims
        H, W = depth.shape
        w2c = get_camera_from_tensor(pose).float()
        gx = self.origin[0] + self.voxel * torch.arange(nx, device=DEV, dtype=torch.float32)[None, None, :]
        gy = self.origin[1] + self.voxel * torch.arange(ny, device=DEV, dtype=torch.float32)[None, :, None]
        gz = self.origin[2] + self.voxel * torch.arange(nz, device=DEV, dtype=torch.float32)[:, None, None]
        x, y, z = (w2c[a, 0] * gx + w2c[a, 1] * gy + w2c[a, 2] * gz + w2c[a, 3] for a in range(3))
        u = torch.floor(self.cam["fx"] * x / z + self.cam["cx"] + 0.5)
        v = torch.floor(self.cam["fy"] * y / z + self.cam["cy"] + 0.5)
        seen = (z > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        pix = (v.clamp(0, H - 1).long() * W + u.clamp(0, W - 1).long()).reshape(-1)
        d = depth.reshape(-1)[pix].reshape(nz, ny, nx)
        sdf = d - z
        upd = seen & (d > 0) & torch.isfinite(d) & (sdf >= -self.trunc)
        if sil is not None:
            upd &= sil.reshape(-1)[pix].reshape(nz, ny, nx) > self.sil_min
        cup = upd & (sdf <= self.trunc)
        self.T = torch.where(upd, (self.T * self.W + (sdf / self.trunc).clamp(max=1.0)) / (self.W + 1), self.T)
        self.W = torch.where(upd, self.W + 1, self.W)
        col = color.reshape(3, -1)[:, pix].reshape(3, nz, ny, nx)
        self.C = torch.where(cup[None], (self.C * self.CW[None] + col) / (self.CW[None] + 1), self.C)
        self.CW = torch.where(cup, self.CW + 1, self.CW)


def lattice(slam, every, source):
    """The export's box at SIDE samples along its longest side: (origin, voxel, trunc, bounds)."""
    from mm3dgs_slam_amd import export
    with torch.no_grad():
        box = export.mesh_bounds(slam, export.options(slam.cfg, "mesh", every=every, source=source, sil_min=0.99, max_depth=0.0))
    voxel = float((box[3:] - box[:3]).max()) / (SIDE - 10)      # room for trunc + voxel on both sides
    trunc = 4.0 * voxel
    origin = np.floor((box[:3] - trunc - voxel) / voxel) * voxel
    return origin, voxel, trunc, box


def integrate_times(slam, args, emit, H, W, source, origin, voxel, trunc):
    """(a): us per integrated view"""
    from mm3dgs_slam_amd import export, mesh as ms
    cam, sil_min = slam.cfg["cam"], 0.99
    i = min(5, args.frames - 1)
    with torch.no_grad():
        view = [v for k, v in enumerate(export.views(slam, 1, source, "mesh")) if k == i][0]
    view = tuple(None if t is None else t.detach().float().contiguous() for t in view)
    dims = (SIDE, SIDE, SIDE)
    dev = ms.TsdfVolume(dims, origin, voxel, trunc, H, W, cam, sil_min=sil_min, device=DEV)
    host = TorchVolume(dims, origin, voxel, trunc, cam, sil_min)
    sides = (("host", lambda: host.add(*view)), ("device", lambda: dev.add(*view)))
    with torch.no_grad():
        for _ in range(args.untimed):
            for _, fn in sides:
                fn()
        torch.cuda.synchronize()
        us = {"host": [], "device": []}
        for _ in range(args.calls):
            for side, fn in sides:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                us[side].append(e0.elapsed_time(e1) * 1e3)
    c = dev.counters.cpu().numpy()
    n = args.untimed + args.calls
    agree = int(((host.W > 0) == (dev.tsdf_w[..., 1] > 0)).sum())
    emit(dict(part="a", shape=f"{W}x{H}", source=source, lattice=list(dims), voxel=round(voxel, 6), calls=args.calls, untimed=args.untimed, torch_us_per_view=stat(us["host"]),
              device_us_per_view=stat(us["device"]), torch_over_device_median=round(statistics.median(us["host"]) / statistics.median(us["device"]), 3),
              device_faster=bool(statistics.median(us["device"]) < statistics.median(us["host"])), dist_updates_per_view=int(c[1]) // n,
              colour_updates_per_view=int(c[2]) // n, samples=SIDE ** 3, samples_where_both_sides_agree_on_seen=agree))


def mesh_times(slam, args, emit, H, W, source, origin, voxel, trunc):
    """(b): us per plan + emit on the volume of all views"""
    from mm3dgs_slam_amd import _lib, export, mesh as ms
    from mm3dgs_slam_amd.rasterizer import _stream
    P = _lib.ptr
    vol = ms.TsdfVolume((SIDE, SIDE, SIDE), origin, voxel, trunc, H, W, slam.cfg["cam"], sil_min=0.99, device=DEV)
    with torch.no_grad():
        for view in export.views(slam, 1, source, "mesh"):
            vol.add(*view)
    rows, tris, c = vol.extract()
    V, T = c["vertices"], c["triangles"]
    work = torch.empty(int(vol.lib.mm3dgs_tsdf_mesh_work_bytes(SIDE, SIDE, SIDE)) // 8, dtype=torch.int64, device=DEV)
    mc = torch.empty(8, dtype=torch.int64, device=DEV)
    rows, tris = torch.empty(max(V, 1), 4, dtype=torch.int32, device=DEV), torch.empty(max(T, 1), 3, dtype=torch.int32, device=DEV)

    def plan():
        _lib.check(vol.lib.mm3dgs_tsdf_mesh_plan(SIDE, SIDE, SIDE, P(vol.tsdf_w), 1.0, P(work), P(mc), _stream()))

    def emit_():
        _lib.check(vol.lib.mm3dgs_tsdf_mesh_emit(SIDE, SIDE, SIDE, P(vol.tsdf_w), P(vol.rgb_w), ms.double3(vol.origin), voxel, P(work), P(rows), V, P(tris), T, P(mc), _stream()))

    for _ in range(args.untimed):
        plan(); emit_()
    torch.cuda.synchronize()
    us = {"plan": [], "emit": []}
    for _ in range(args.calls):
        for name, fn in (("plan", plan), ("emit", emit_)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3)
    emit(dict(part="b", shape=f"{W}x{H}", source=source, lattice=[SIDE] * 3, views=c["views"], vertices=V, triangles=T, calls=args.calls, plan_us=stat(us["plan"]),
              emit_us=stat(us["emit"]), plan_plus_emit_us_median=round(statistics.median(us["plan"]) + statistics.median(us["emit"]), 2),
              counters_after_emit=mc.cpu().tolist()))


def export_times(slam, args, emit, H, W, source, voxel, box):
    """(c): ms per export_mesh over all frames"""
    pad = 5.0 * voxel      # trunc + voxel, what the export adds to a box it finds itself
    slam.cfg["mesh"] = dict(slam.cfg.get("mesh") or {}, bounds=[float(v) for v in np.concatenate([box[:3] - pad, box[3:] + pad])], voxel=voxel, every=1,
                            source=source)

    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = slam.export_mesh()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    run()
    ms_ = []
    for _ in range(args.repeats):
        t, out = run()
        ms_.append(t)
    emit(dict(part="c", shape=f"{W}x{H}", source=source, frames=args.frames, repeats=args.repeats, voxel=round(voxel, 6), lattice=list(out["lattice"]),
              gaussians=int(slam.gaussians.get_xyz.shape[0]), ms_export=dict(median=round(statistics.median(ms_), 3), min=round(min(ms_), 3), max=round(max(ms_), 3)),
              ms_per_view=round(statistics.median(ms_) / args.frames, 4), mesh_bytes=os.path.getsize(out["mesh"]), counters=out["counters"]))


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
            for source in ("render", "sensor"):
                origin, voxel, trunc, box = lattice(slam, 1, source)
                integrate_times(slam, args, emit, H, W, source, origin, voxel, trunc)
                mesh_times(slam, args, emit, H, W, source, origin, voxel, trunc)
                export_times(slam, args, emit, H, W, source, voxel, box)
            del slam, seq
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
