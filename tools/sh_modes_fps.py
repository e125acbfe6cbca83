#!/usr/bin/env python
"""Frames/s of a resumed SH-2 map in the two viewing-direction modes that became native with ABI 211, native loops against the torch-graph
loops (native_loops=False), at bench.py's headline workload (BASELINE.json configs[1]: 640x480, ~150 k Gaussians, 100 tracking + 150 mapping
iterations per frame).  Needs the GPU.

    python tools/sh_modes_fps.py [--frames 4] [--warmup 1] [--modes A,B] [--paths native,torch]

mode A: transform_means_python: true, convert_SHs_python: true   (SH on the world mean about the origin, evaluated in Python by the reference)
mode B: transform_means_python: false                            (SH on the world mean seen from the camera centre)
The map is seeded from frame 0 at max_sh_degree 2 and its active degree raised to 2 right away, as load_ply leaves a resumed checkpoint.
One JSON line per (mode, path)."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MODES = {"A": {"transform_means_python": True, "convert_SHs_python": True}, "B": {"transform_means_python": False, "convert_SHs_python": False}}


def run(mode, native, args):
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.fused import FusedEngine
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    dev = "cuda:0"
    frac = min(1.0, args.gaussians / (0.95 * args.height * args.width))
    cfg = default_config(device=dev, height=args.height, width=args.width, pipeline=dict(MODES[mode]), tracking={"iters": args.track_iters},
                         mapping={"iters": args.map_iters, "seed_fraction": frac, "sh_degree": 2})
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    n = 1 + args.warmup + args.frames
    seq = SyntheticSequence(cfg, n + 1, args.gaussians, seed=0)
    slam = SLAM(cfg, seq, native_loops=native)
    slam.gaussians.active_sh_degree = 2
    slam.step(0)
    for i in range(1, 1 + args.warmup):
        slam.step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(1 + args.warmup, n):
        slam.step(i)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    return dict(mode=mode, pipeline=MODES[mode], path="native" if native else "torch-graph", eligible=bool(FusedEngine.eligible(cfg, slam.gaussians)),
                active_sh_degree=int(slam.gaussians.active_sh_degree), gaussians=int(slam.gaussians.get_xyz.shape[0]), frames=args.frames,
                seconds=round(sec, 3), fps=round(args.frames / sec, 3), pose_errors=[float(e) for e in slam.pose_errors()][:3],
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--modes", default="A,B")
    ap.add_argument("--paths", default="native,torch")
    ap.add_argument("--gaussians", type=int, default=150000)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--track-iters", type=int, default=100)
    ap.add_argument("--map-iters", type=int, default=150)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    for mode in args.modes.split(","):
        for path in args.paths.split(","):
            print(json.dumps(run(mode, path == "native", args)), flush=True)


if __name__ == "__main__":
    main()
