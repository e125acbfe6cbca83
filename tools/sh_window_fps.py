#!/usr/bin/env python
"""Frames/s of a resumed SH-2 map under a mapping WINDOW (WindowParallel: the multi-GPU orchestration on one GPU), in the three SH viewing-
direction modes, at bench.py's headline workload (BASELINE.json configs[1]: 640x480, ~150 k Gaussians, 100 tracking + 150 mapping iterations
per frame).  Since ABI 212 such a window runs on the native loops; before, FusedMapper handed it to the torch-graph loop -- the line's
`torch_graph_map_calls` says which one ran.  Needs the GPU; the forced-collective windows run over backend "nccl" with world size 1.

    python tools/sh_window_fps.py [--frames 2] [--warmup 1] [--modes default,python_sh,world_means] [--windows allreduce,reduce_scatter,batch2] [--two-launch]

windows: allreduce / reduce_scatter -- WindowParallel(0, 1, always_reduce=True, optimizer=...); batch2 -- WindowParallel(0, 1, batch=2).
One JSON line per (mode, window)."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MODES = {"default": {}, "python_sh": {"convert_SHs_python": True}, "world_means": {"transform_means_python": False}}


def _window(name):
    from mm3dgs_slam_amd.window_parallel import WindowParallel
    if name == "batch2":
        return WindowParallel(0, 1, batch=2)
    return WindowParallel(0, 1, always_reduce=True, optimizer=name)


def run(mode, window, args):
    from mm3dgs_slam_amd import mapper
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    dev = "cuda:0"
    frac = min(1.0, args.gaussians / (0.95 * args.height * args.width))
    cfg = default_config(device=dev, height=args.height, width=args.width, pipeline=dict(MODES[mode]), tracking={"iters": args.track_iters},
                         mapping={"iters": args.map_iters, "seed_fraction": frac, "sh_degree": 2})
    graph_calls = []
    real = mapper.Mapper.optimize_map

    def counted(self, *a, **k):
        graph_calls.append(1)
        return real(self, *a, **k)
    mapper.Mapper.optimize_map = counted
    try:
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        n = 1 + args.warmup + args.frames
        seq = SyntheticSequence(cfg, n + 1, args.gaussians, seed=0)
        slam = SLAM(cfg, seq, window=_window(window))
        slam.gaussians.active_sh_degree = 2
        slam.step(0)
        for i in range(1, 1 + args.warmup):
            slam.step(i)
        torch.cuda.synchronize()
        graph_calls.clear()
        t0 = time.perf_counter()
        for i in range(1 + args.warmup, n):
            slam.step(i)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
    finally:
        mapper.Mapper.optimize_map = real
    return dict(mode=mode, pipeline=MODES[mode], window=window, torch_graph_map_calls=len(graph_calls), active_sh_degree=int(slam.gaussians.active_sh_degree),
                gaussians=int(slam.gaussians.get_xyz.shape[0]), frames=args.frames, two_launch=args.two_launch, seconds=round(sec, 3), fps=round(args.frames / sec, 3),
                pose_errors=[float(e) for e in slam.pose_errors()][:3], label=args.label, device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--modes", default="default,python_sh,world_means")
    ap.add_argument("--windows", default="allreduce,reduce_scatter,batch2")
    ap.add_argument("--gaussians", type=int, default=150000)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--track-iters", type=int, default=100)
    ap.add_argument("--map-iters", type=int, default=150)
    ap.add_argument("--label", default="", help="free text copied into every line (which build ran)")
    ap.add_argument("--two-launch", action="store_true", help="FusedMapper.fuse_adam_project = False: mm3dgs_adam + the projecting map call")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    if args.two_launch:
        from mm3dgs_slam_amd.fused import FusedMapper
        FusedMapper.fuse_adam_project = False
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29517")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        for mode in args.modes.split(","):
            for window in args.windows.split(","):
                print(json.dumps(run(mode, window, args)), flush=True)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
