#!/usr/bin/env python
"""A/B of the visibility culling (mm3dgs_slam_amd/cull.py, csrc/cull.hip) against a torch operator chain of the same rule, at `--rows` rows
(10^6: a scene-sized reference sampled at 10^4 points per m^2) and views of 640x480 and 1200x680.  Needs the GPU; there is no fall-back.

    python tools/cull_ab.py [--calls 200] [--untimed 20] [--rows 1000000] [--out profiles/r17_cull.jsonl]

The rows are uniform in a 6 x 4 x 6 m box around and in front of the camera (about a third inside the frustum); the depth image is a wavy
surface 2 - 4 m away with a few holes.  Between device events around every single call, the median, p10 and p90 of `--calls` calls after
`--untimed` untimed ones: one mm3dgs_cull_mark_view in each mode (seen is zeroed outside the timed region), one mm3dgs_cull_select, and the
torch chain (float64 operators: the pose applied, the projection, the masks, a gather of the depth, `seen += hit`; and for select
`rows[mask]` with `nonzero`).  Each line says whether the kernel's `seen` equals the chain's."""
import argparse
import json
import os
import statistics
import sys

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


def timed(fn, calls, untimed, before=None):
    """us per call between device events; `before` runs outside the timed region"""
    us = []
    for k in range(untimed + calls):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if k >= untimed:
            us.append(e0.elapsed_time(e1) * 1e3)
    return us


def torch_mark(xyz64, fin, R, t, fx, fy, cx, cy, H, W, near, far, eps, depth, depth_max, seen):
    pc = xyz64 @ R.T + t
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    hit = fin & (z > near) & (z <= far)
    fu, fv = torch.floor(fx * x / z + cx + 0.5), torch.floor(fy * y / z + cy + 0.5)
    hit &= (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
    if depth is not None:
        pix = torch.where(hit, fv * W + fu, torch.zeros_like(fu)).long()
        d = depth.reshape(-1)[pix]
        hit &= (d > 0) & torch.isfinite(d) & (d <= depth_max) & (z <= d.double() + eps)
    seen += hit.to(seen.dtype)
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--untimed", type=int, default=20)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--out", default="", help="append the lines to this file as well")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from mm3dgs_slam_amd import _lib, cull as cl
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.pointcloud import pose_rotation
    from mm3dgs_slam_amd.rasterizer import _stream
    lib, P = _lib.load(), _lib.ptr

    def emit(d):
        d = dict(d, device=torch.cuda.get_device_name(0))
        print(json.dumps(d), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    rng = np.random.default_rng(0)
    n = args.rows
    xyz = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(-1, 5, n)], 1).astype(np.float32)
    rows_h = np.empty((n, 4), dtype=np.int32)
    rows_h[:, :3] = xyz.view(np.int32)
    rows_h[:, 3] = -1
    rows = torch.from_numpy(rows_h).to(DEV)
    pose_h = np.array([0.995, 0.02, -0.05, 0.01, 0.1, -0.05, 0.2], dtype=np.float32)
    pose = torch.from_numpy(pose_h).to(DEV)
    near, far, eps, depth_max = 0.1, 6.0, 0.05, 8.0
    for H, W in SHAPES:
        cam = default_config(device=DEV, height=H, width=W)["cam"]
        fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
        v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        depth_h = (3.0 + np.sin(u * 0.02) * np.cos(v * 0.03)).astype(np.float32)
        depth_h[rng.uniform(size=(H, W)) < 0.02] = 0.0
        depth = torch.from_numpy(depth_h).to(DEV)
        seen = torch.zeros(n, dtype=torch.int32, device=DEV)
        counters = torch.zeros(8, dtype=torch.int64, device=DEV)
        work = torch.empty(int(lib.mm3dgs_cull_work_bytes(n)) // 8, dtype=torch.int64, device=DEV)
        out = torch.empty(n, 4, dtype=torch.int32, device=DEV)
        index = torch.empty(n, dtype=torch.int32, device=DEV)
        mark = lambda d: _lib.check(lib.mm3dgs_cull_mark_view(H, W, fx, fy, cx, cy, P(pose), P(d), depth_max, near, far, eps, n, P(rows), P(seen), P(counters), _stream()))
        select = lambda: _lib.check(lib.mm3dgs_cull_select(n, P(rows), P(seen), 1, P(out), n, P(index), P(work), P(counters), _stream()))
        R_h, t_h = pose_rotation(pose_h)
        R, t = torch.from_numpy(R_h).to(DEV), torch.from_numpy(t_h).to(DEV)
        xyz64 = rows[:, :3].contiguous().view(torch.float32).double()
        fin = torch.isfinite(xyz64).all(1)
        tseen = torch.zeros(n, dtype=torch.int32, device=DEV)
        for mode, d in (("frustum", None), ("occlusion", depth)):
            us = timed(lambda: mark(d), args.calls, args.untimed, before=seen.zero_)
            chain = lambda: torch_mark(xyz64, fin, R, t, fx, fy, cx, cy, H, W, near, far, eps, d, depth_max, tseen)
            us_t = timed(chain, args.calls, args.untimed, before=tseen.zero_)
            host_seen = cl.seen_by_view_host(rows_h, None if d is None else depth_h, pose_h, H, W, fx, fy, cx, cy, near, far, eps, depth_max)
            emit(dict(part="mark_view", mode=mode, rows=n, H=H, W=W, calls=args.calls, seen_rows=int(seen.sum()), kernel_us=stat(us), torch_chain_us=stat(us_t),
                      torch_over_kernel_median=round(statistics.median(us_t) / statistics.median(us), 2),
                      bytes_per_call=16 * n + 8 * int(seen.sum()), gb_per_s_at_median=round((16 * n + 8 * int(seen.sum())) / statistics.median(us) * 1e-3, 1),
                      seen_equals_torch_chain=bool(torch.equal(seen, tseen)), seen_equals_host_statement=bool(np.array_equal(seen.cpu().numpy().astype(bool), host_seen))))
        us = timed(select, args.calls, args.untimed)
        kept = int(counters.cpu()[2])
        chain = lambda: (rows[tseen >= 1], torch.nonzero(tseen >= 1))
        us_t = timed(chain, args.calls, args.untimed)
        emit(dict(part="select", rows=n, H=H, W=W, calls=args.calls, kept=kept, kernel_us=stat(us), torch_chain_us=stat(us_t),
                  torch_over_kernel_median=round(statistics.median(us_t) / statistics.median(us), 2),
                  kept_equals_torch_chain=bool(torch.equal(out[:kept], rows[tseen >= 1]))))


if __name__ == "__main__":
    main()
