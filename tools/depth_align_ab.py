#!/usr/bin/env python
"""A/B of depth_align_on_device at bench.py's `mono_depth` workload (640x480, the default map, use_gt_depth: false, 100 tracking + 150
mapping iterations per frame, seed 0).  Key off = the host fit (depth_utils.get_scale_shift_LS: ~30 torch launches, float64 copies of the
image); key on = mm3dgs_align_depth (two launches).  Needs the GPU.

    python tools/depth_align_ab.py [--calls 100] [--steps 20] [--warmup 2] [--repeats 3] [--out profiles/r10_depth_align.jsonl]

(a) One alignment call -- scale_depth_estimate on a later frame with the render already made: mask, fit and apply -- timed with device
events around `--calls` back-to-back calls, host path and device path alternating, `--repeats` times after an untimed round of each.
The inputs are a frame of the workload itself: the monocular estimate of the first timed frame and the map rendered at the last
tracked pose.  The summary holds the claim the key's documentation makes: the device call is faster than the host call by more than
the spread (max - min) of the host call's repeats; it says so when that does not hold.

(b) Frames/s of `--steps` SLAM frames with the key off and on, alternating, `--repeats` times after one untimed pass of each; every run
is a fresh SLAM object from the same seeds, the key applies to the timed frames only, so both settings enter the timed region from the
same map, keyframes and poses; timed like bench.py (host clock, device synchronised at both ends).  Reported as a pair, without a bar,
next to the largest pose difference between the two settings over the timed frames and the same figure between two key-off runs."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"


def config(args):
    from mm3dgs_slam_amd.config import default_config
    frac = min(1.0, args.gaussians / (0.95 * args.height * args.width))      # bench.py's seeding fraction
    return default_config(device=DEV, height=args.height, width=args.width, use_gt_depth=False, tracking={"iters": args.track_iters},
                          mapping={"iters": args.map_iters, "seed_fraction": frac})


def start(seq, args):
    """frame 0 and the warm-up frames with the key off (untimed)"""
    from mm3dgs_slam_amd.slam import SLAM
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    slam = SLAM(config(args), seq)
    slam.step(0)
    torch.cuda.synchronize()
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    for i in range(1, 1 + args.warmup):
        slam.step(i)
    torch.cuda.synchronize()
    return slam


def run(seq, args, key, steps):
    slam = start(seq, args)
    first = 1 + args.warmup
    slam.cfg["depth_align_on_device"] = key
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(first, first + steps):
        slam.step(i)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    poses = torch.stack([slam.estimate_pose_list[i].detach() for i in range(first, first + steps)]).cpu()
    line = dict(part="b", depth_align_on_device=key, steps=steps, seconds=round(sec, 4), fps=round(steps / sec, 3), ms_per_frame=round(sec / steps * 1e3, 3),
                gaussians=int(slam.gaussians.get_xyz.shape[0]), keyframes=len(slam.mapper.keyframes))
    if key:
        fits = torch.stack(slam.depth_fits)[:, :4].cpu()
        line.update(fits_ok=int(fits[:, 2].sum()), fits=len(slam.depth_fits), n_valid_min=float(fits[:, 3].min()))
    return line, poses


def call_times(seq, args, emit):
    """(a): us per alignment call, host and device path alternating"""
    from mm3dgs_slam_amd.depth_utils import scale_depth_estimate
    slam = start(seq, args)
    idx = 1 + args.warmup
    est, gt = seq.est(idx), seq[idx][1]
    d, s = slam.mapper._render_depth_sil(slam.estimate_pose_list[idx - 1])
    d, s = d.clone(), s.clone()
    render = lambda: (d, s)
    one = {False: lambda: scale_depth_estimate(slam.cfg, idx, est, gt, render),
           True: lambda: scale_depth_estimate(slam.cfg, idx, est, gt, render, on_device=True)}
    host, dev = one[False](), one[True]()
    fin = torch.isfinite(host) & torch.isfinite(dev)
    agree = dict(max_abs_diff_scaled=float((host - dev)[fin].abs().max()), bit_identical_pixels=int((host.view(torch.int32) == dev.view(torch.int32)).sum()),
                 pixels=int(host.numel()))
    for key in (False, True):      # untimed round
        for _ in range(10):
            one[key]()
    torch.cuda.synchronize()
    us = {False: [], True: []}
    for r in range(args.repeats):
        for key in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                one[key]()
            e1.record()
            e1.synchronize()
            us[key].append(e0.elapsed_time(e1) / args.calls * 1e3)
            emit(dict(part="a", path="device" if key else "host", repeat=r, calls=args.calls, us_per_call=round(us[key][-1], 2)))
    del slam
    return us, agree


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--gaussians", type=int, default=150000, help="size of the synthetic ground-truth scene (bench.py's default)")
    ap.add_argument("--track-iters", type=int, default=100)
    ap.add_argument("--map-iters", type=int, default=150)
    ap.add_argument("--out", default="", help="append the lines to this file as well")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from mm3dgs_slam_amd.slam import SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    seq = SyntheticSequence(config(args), args.warmup + args.steps + 1, args.gaussians, seed=0)

    def emit(d):
        d = dict(d, device=torch.cuda.get_device_name(0))
        print(json.dumps(d), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    stat = lambda v: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
    us, agree = call_times(seq, args, emit)
    spread = max(us[False]) - min(us[False])
    gain = statistics.median(us[False]) - statistics.median(us[True])
    emit(dict(part="a", summary=True, workload=f"mono_depth ({args.width}x{args.height}, use_gt_depth: false)", calls=args.calls, repeats=args.repeats,
              host_us_per_call=stat(us[False]), device_us_per_call=stat(us[True]), host_spread_us=round(spread, 3), host_minus_device_us=round(gain, 3),
              device_faster_by_more_than_the_host_spread=bool(gain > spread), **agree))

    for key in (False, True):      # untimed pass of each setting
        run(seq, args, key, 2)
    fps, on_off, off_off, prev_off = {False: [], True: []}, 0.0, 0.0, None
    for r in range(args.repeats):
        poses = {}
        for key in (False, True):
            line, poses[key] = run(seq, args, key, args.steps)
            fps[key].append(line["fps"])
            emit(dict(line, repeat=r))
        on_off = max(on_off, float((poses[True] - poses[False]).abs().max()))
        if prev_off is not None:
            off_off = max(off_off, float((poses[False] - prev_off).abs().max()))
        prev_off = poses[False]
    emit(dict(part="b", summary=True, workload=f"mono_depth ({args.width}x{args.height}, use_gt_depth: false)", steps=args.steps, warmup=args.warmup,
              repeats=args.repeats, track_iters=args.track_iters, map_iters=args.map_iters, fps_key_off=stat(fps[False]), fps_key_on=stat(fps[True]),
              fps_ratio_on_over_off_median=round(statistics.median(fps[True]) / statistics.median(fps[False]), 4),
              max_pose_diff_on_vs_off_timed_frames=on_off, max_pose_diff_off_vs_off=off_off if args.repeats > 1 else None))


if __name__ == "__main__":
    main()
