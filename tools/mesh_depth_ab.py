#!/usr/bin/env python
"""A/B of the mesh depth renderer and the depth comparison (mm3dgs_slam_amd/mesh_depth.py, csrc/meshdepth.hip) against a chunked float64
torch broadcast of the same rule on the device, at 640x480 and 1200x680.  Needs the GPU; there is no fall-back.

    python tools/mesh_depth_ab.py [--calls 200] [--untimed 20] [--frames 6] [--repeats 3] [--out profiles/r19_mesh_depth.jsonl]

(a) One view of the sensor mesh of tools/mesh_ab.py (the frames' own colour and sensor depth fused at the ground-truth poses over a lattice
of 256 samples along the box's longest side, marching tetrahedra): one mm3dgs_mesh_depth_render between device events around every single
call, the median, p10 and p90 of `--calls` calls after `--untimed` untimed ones.  The torch broadcast evaluates every triangle on every
pixel (`--chunk` triangles at a time), which at a mesh of this size is minutes per view: it is timed, `--baseline-calls` times, on the
first `--baseline-triangles` triangles, and so is the kernel on the same sub-mesh -- the ratio is of those two; each line says whether
the two images are equal.
(b) A room of 12 triangles (a 6 x 4 x 6 m box around the camera: wall-sized triangles, every tile in every list): the kernel against the
torch broadcast over the whole mesh, `--calls` calls each.
(c) One mm3dgs_depth_compare of two renderings against the torch chain (masks, a float64 difference, sum / square sum / max / counts).
(d) A whole SLAM.evaluate_geometry (`estimate: mesh`, `reference: sensor`) over `--frames` views with `geometry.depth_l1` on against off,
`--repeats` times after one untimed pass each; host clock, device synchronised at both ends."""
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
DEV = "cuda:0"
SHAPES = [(480, 640), (680, 1200)]


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def stat(v):
    return dict(median=round(statistics.median(v), 2), p10=round(pct(v, 0.1), 2), p90=round(pct(v, 0.9), 2))


def timed(fn, calls, untimed):
    """us per call between device events"""
    us = []
    for k in range(untimed + calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if k >= untimed:
            us.append(e0.elapsed_time(e1) * 1e3)
    return us


def torch_render(xyz64, tris, R, t, H, W, fx, fy, cx, cy, near, far, chunk):
    """The rule of mesh_depth.py as float64 torch operators, every triangle on every pixel, `chunk` triangles at a time: (depth, tri)."""
    pc = torch.stack([R[k, 0] * xyz64[:, 0] + R[k, 1] * xyz64[:, 1] + R[k, 2] * xyz64[:, 2] + t[k] for k in range(3)], 1)
    V = xyz64.shape[0]
    ok = ((tris >= 0) & (tris < V)).all(1)
    safe = torch.where(ok[:, None], tris, torch.zeros_like(tris)).long()
    a, b, c = pc[safe[:, 0]], pc[safe[:, 1]], pc[safe[:, 2]]
    ok &= torch.isfinite(a).all(1) & torch.isfinite(b).all(1) & torch.isfinite(c).all(1)
    ok &= (a[:, 2] > near) | (b[:, 2] > near) | (c[:, 2] > near)
    cross = lambda u, w: torch.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    n = (cross(b, c), cross(c, a), cross(a, b))
    det = a[:, 0] * n[0][:, 0] + a[:, 1] * n[0][:, 1] + a[:, 2] * n[0][:, 2]
    dx = ((torch.arange(W, device=DEV, dtype=torch.float64) - cx) / fx).repeat(H)
    dy = ((torch.arange(H, device=DEV, dtype=torch.float64) - cy) / fy).repeat_interleave(W)
    inf = torch.tensor(float("inf"), device=DEV, dtype=torch.float64)
    best = torch.full((H * W,), float("inf"), device=DEV, dtype=torch.float64)
    tri = torch.full((H * W,), -1, device=DEV, dtype=torch.int64)
    for lo in range(0, tris.shape[0], chunk):
        s = slice(lo, lo + chunk)
        E = [m[s, 0, None] * dx + m[s, 1, None] * dy + m[s, 2, None] for m in n]
        S = E[0] + E[1] + E[2]
        inside = ((E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0) & (S > 0)) | ((E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0) & (S < 0))
        z = det[s, None] / S
        hit = inside & ok[s, None] & torch.isfinite(z) & (z > near)
        if far > 0:
            hit &= z <= far
        z = torch.where(hit, z, inf)
        zc, k = z.min(0)      # (the first minimum along the chunk: the lowest index of a tie on this device's reduction is not promised)
        win = zc < best
        best = torch.where(win, zc, best)
        tri = torch.where(win, k + lo, tri)
    return torch.where(tri >= 0, best, torch.zeros_like(best)).float().reshape(H, W), tri.reshape(H, W)


def torch_compare(a, b):
    va, vb = (a > 0) & (a < float("inf")), (b > 0) & (b < float("inf"))
    both = va & vb
    d = torch.where(both, (a.double() - b.double()).abs(), torch.zeros((), device=a.device, dtype=torch.float64))
    n = both.sum().double()
    return torch.stack([n, d.sum() / n.clamp(min=1), (d * d).sum().div(n.clamp(min=1)).sqrt(), d.max(), (vb & ~va).sum().double(), (va & ~vb).sum().double(),
                        (~va & ~vb).sum().double(), n * 0])


def room():
    """12 triangles: the box x in [-3, 3], y in [-2, 2], z in [-3, 3] around a camera at the origin."""
    xyz = np.array([[x, y, z] for z in (-3.0, 3.0) for y in (-2.0, 2.0) for x in (-3.0, 3.0)], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)]
    tris = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], dtype=np.int32)
    rows = np.empty((8, 4), dtype=np.int32)
    rows[:, :3] = xyz.view(np.int32)
    rows[:, 3] = -1
    return rows, tris


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--untimed", type=int, default=20)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--baseline-calls", type=int, default=5)
    ap.add_argument("--baseline-triangles", type=int, default=4096)
    ap.add_argument("--gaussians", type=int, default=150000, help="size of the synthetic ground-truth scene (bench.py's default)")
    ap.add_argument("--out", default="", help="append the lines to this file as well")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from mm3dgs_slam_amd import export as ex, mesh_depth as md
    from mm3dgs_slam_amd.pointcloud import pose_rotation
    from tools.mesh_ab import lattice, start

    def emit(d):
        d = dict(d, device=torch.cuda.get_device_name(0))
        print(json.dumps(d), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    def one_view(part, rows, tris, pose, H, W, cam, calls, base_calls, extra):
        m = md.MeshDepth(rows, tris, H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"], near=0.05, far=0.0, device=DEV)
        depth, tri = m.render(pose)
        us = timed(lambda: m.render(pose, depth, tri), calls, args.untimed)
        c = m.finish()
        n_calls = int(c[0])
        R_h, t_h = pose_rotation(pose)
        R, t = torch.from_numpy(R_h).to(DEV), torch.from_numpy(t_h).to(DEV)
        xyz64 = m.rows[:, :3].contiguous().view(torch.float32).double()
        chain = lambda: torch_render(xyz64, m.triangles, R, t, H, W, float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"]), 0.05, 0.0, args.chunk)
        us_t = timed(chain, base_calls, 1)
        td, tt = chain()
        emit(dict(part=part, H=H, W=W, vertices=m.V, triangles=m.T, calls=calls, baseline_calls=base_calls, kernel_us=stat(us), torch_broadcast_us=stat(us_t),
                  torch_over_kernel_median=round(statistics.median(us_t) / statistics.median(us), 2), pairs_per_view=int(c[4]) // n_calls, drawn_per_view=int(c[1]) // n_calls,
                  hit_pixels=int(c[6]) // n_calls, depth_equals_torch_broadcast=bool(torch.equal(depth, td)), **extra))
        return depth

    with tempfile.TemporaryDirectory() as tmp:
        for H, W in SHAPES:
            slam, seq = start(args, H, W, tmp)
            for i in range(1, args.frames):      # (start ran frame 0 only: the later frames' ground-truth poses, as a run would have kept them)
                slam.gt_pose_list[i] = seq[i][2].detach().clone()
            cam = slam.cfg["cam"]
            origin, voxel, trunc, box = lattice(slam, 1, "sensor")
            pad = 5.0 * voxel
            slam.cfg["mesh"] = dict(slam.cfg.get("mesh") or {}, bounds=[float(v) for v in np.concatenate([box[:3] - pad, box[3:] + pad])], voxel=voxel, every=1, source="sensor")
            block = ex.options(slam.cfg, "mesh")
            gt = ex.gt_poses(slam)
            rows, tris = ex.mesh_geometry(slam, block, gt)[:2]
            pose = gt[args.frames // 2].detach().cpu().numpy()
            # (a) the whole sensor mesh: the kernel alone; then kernel and broadcast on its first triangles
            m = md.MeshDepth(rows, tris, H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"], near=0.05, far=0.0, device=DEV)
            depth, tri = m.render(pose)
            us = timed(lambda: m.render(pose, depth, tri), args.calls, args.untimed)
            c = m.finish()
            emit(dict(part="a", mesh="sensor", H=H, W=W, vertices=m.V, triangles=m.T, voxel=round(voxel, 6), calls=args.calls, kernel_us=stat(us),
                      pairs_per_view=int(c[4]) // int(c[0]), drawn_per_view=int(c[1]) // int(c[0]), hit_pixels=int(c[6]) // int(c[0]), torch_broadcast_us="not measured (whole mesh)"))
            full = depth.clone()
            one_view("a_subset", rows, tris[:args.baseline_triangles], pose, H, W, cam, args.calls, args.baseline_calls, dict(mesh="sensor, first triangles"))
            # (b) the room
            rrows, rtris = room()
            rdepth = one_view("b", rrows, rtris, np.array([0.98, 0.05, 0.17, 0.02, 0.1, -0.2, 0.3], dtype=np.float32), H, W, cam, args.calls, args.calls, dict(mesh="room"))
            # (c) one comparison
            table = torch.zeros(1, 8, dtype=torch.float64, device=DEV)
            us = timed(lambda: md.compare_device(full, rdepth, table, 0), args.calls, args.untimed)
            us_t = timed(lambda: torch_compare(full, rdepth), args.calls, args.untimed)
            want = md.compare_rows_host(full, rdepth, "kernel")
            emit(dict(part="c", H=H, W=W, calls=args.calls, kernel_us=stat(us), torch_chain_us=stat(us_t), torch_over_kernel_median=round(statistics.median(us_t) / statistics.median(us), 2),
                      n=int(want[0, 0]), row_equals_host_statement=bool(table.cpu().numpy().tobytes() == want.tobytes())))
            # (d) the whole evaluation, the key on against off
            ms = {}
            for key in (False, True):
                slam.cfg["geometry"] = dict(slam.cfg.get("geometry") or {}, eval=False, estimate="mesh", reference="sensor", density=2000.0, depth_l1=key)
                runs = []
                for k in range(args.repeats + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = slam.evaluate_geometry(path=os.path.join(tmp, f"geometry_{H}_{int(key)}"))
                    torch.cuda.synchronize()
                    if k:
                        runs.append((time.perf_counter() - t0) * 1e3)
                ms[key] = runs
            emit(dict(part="d", H=H, W=W, frames=args.frames, repeats=args.repeats, triangles=int(tris.shape[0]),
                      ms_off=dict(median=round(statistics.median(ms[False]), 3), min=round(min(ms[False]), 3), max=round(max(ms[False]), 3)),
                      ms_on=dict(median=round(statistics.median(ms[True]), 3), min=round(min(ms[True]), 3), max=round(max(ms[True]), 3)),
                      ms_added_per_view=round((statistics.median(ms[True]) - statistics.median(ms[False])) / args.frames, 4), depth_l1=out["depth_l1"]))
            del slam, seq, m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
