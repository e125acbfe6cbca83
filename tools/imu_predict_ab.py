#!/usr/bin/env python
"""A/B of tracking.imu_on_device at bench.py's `c3` workload (BASELINE.json configs[2]: UT-MM-shaped 640x330 RGB-D + IMU, configs/UTMM.yml
settings, IMU residual in the tracking loss, the map grown by keyframes to its stated size on the wide sweep, 100 tracking + 150 mapping
iterations per frame, seed 0).  Key off = the host prediction (a pose read-back at the head of every frame, then pose_utils.propagate_imu as
float32 torch operators); key on = mm3dgs_propagate_imu.  Both settings run in one process on one shared synthetic sequence, alternating,
`--repeats` times after one untimed pass of each (operators, code objects, pinned allocator); every run is a fresh SLAM object from the
same seeds, timed like bench.py (host clock around `--steps` frames, device synchronised at both ends).  Needs the GPU.

    python tools/imu_predict_ab.py [--steps 10] [--warmup 2] [--repeats 3] [--grow-to 300000] [--whole-run] [--out profiles/r09_imu_predict.jsonl]

By default the key applies to the timed frames only: warm-up and growth run with the key off, so both settings enter the timed region from
the same map, keyframes and poses (a run is reproducible bit for bit, see `max_pose_diff_off_vs_off`) and time the same frames.
`--whole-run` applies it from frame 1: the last-bit difference of a start pose then has the whole growth phase to flip a keyframe or
pruning decision, after which the two settings time different maps (the lines carry `gaussians`, `keyframes`, `first_timed_frame`).

One JSON line per timed run, then a summary line: frames/s of both settings (median, min, max), the largest per-frame pose difference
between the key-on and the key-off run of a repeat over the timed frames both runs timed (and over every frame both runs tracked) -- next
to the same figure between two key-off runs, the run-to-run floor -- and the largest difference, over the timed frames of the key-on runs,
between the device prediction and the float32 host prediction from the same two estimated poses."""
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


def config(args, key):
    from mm3dgs_slam_amd.config import utmm_config
    return utmm_config(device=DEV, tracking={"iters": args.track_iters, "use_imu_loss": True, "imu_T_weight": 1.0, "imu_q_weight": 0.1, "imu_on_device": key},
                       mapping={"iters": args.map_iters, "seed_fraction": 1.0})


def run(seq, args, key, steps):
    """frame 0, warm-up frames, growth to the stated map size (all untimed), then `steps` timed frames; returns the line and the run."""
    from mm3dgs_slam_amd.slam import SLAM
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = config(args, key and args.whole_run)
    slam = SLAM(cfg, seq)
    slam.step(0)
    torch.cuda.synchronize()
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    for i in range(1, 1 + args.warmup):
        slam.step(i)
    grown = 0
    while args.grow_to and grown < args.grow_max_frames and int(slam.gaussians.get_xyz.shape[0]) < args.grow_to:
        slam.step(1 + args.warmup + grown)
        grown += 1
    first = 1 + args.warmup + grown
    cfg["tracking"]["imu_on_device"] = key
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(first, first + steps):
        slam.step(i)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    poses = torch.stack([slam.estimate_pose_list[i].detach() for i in range(first + steps)]).cpu()      # every tracked frame, by frame index
    line = dict(imu_on_device=key, steps=steps, seconds=round(sec, 4), fps=round(steps / sec, 3), ms_per_frame=round(sec / steps * 1e3, 3),
                first_timed_frame=first, grown_frames=grown, gaussians=int(slam.gaussians.get_xyz.shape[0]), keyframes=len(slam.mapper.keyframes),
                pose_error_max_m=float(max(slam.pose_errors()[first:first + steps])))
    return line, slam, poses, first


def prediction_gap(slam, seq, first, steps):
    """max |device prediction - float32 host prediction| over the timed frames, both from the run's own estimates of frames idx-1, idx-2"""
    from mm3dgs_slam_amd.pose_utils import propagate_imu
    worst = 0.0
    est = slam.estimate_pose_list
    for idx in range(first, first + steps):
        dev = slam.tracker.predict_pose(idx, seq.imu(idx)).cpu()
        host = propagate_imu(est[idx - 1].detach().cpu(), est[idx - 2].detach().cpu(), seq.imu(idx), seq.tf["c2i"], seq.tstamps[idx - 1] - seq.tstamps[idx - 2], 0.01)
        worst = max(worst, float((dev - host).abs().max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--gaussians", type=int, default=150000, help="size of the synthetic ground-truth scene (bench.py's default)")
    ap.add_argument("--track-iters", type=int, default=100)
    ap.add_argument("--map-iters", type=int, default=150)
    ap.add_argument("--grow-to", type=int, default=300000, help="map size at which the timed region starts (bench.py's c3 default; 0: right after the warm-up)")
    ap.add_argument("--grow-max-frames", type=int, default=160)
    ap.add_argument("--whole-run", action="store_true", help="the key applies from frame 1 (default: to the timed frames only)")
    ap.add_argument("--out", default="", help="append the lines to this file as well")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from mm3dgs_slam_amd.slam import SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    seq = SyntheticSequence(config(args, False), args.warmup + args.steps + 1 + args.grow_max_frames, args.gaussians, seed=0,
                            motion="desk_wide" if args.grow_to else "bounded")

    def emit(d):
        d = dict(d, device=torch.cuda.get_device_name(0))
        print(json.dumps(d), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    for key in (False, True):      # untimed pass of each setting
        run(seq, args, key, 2)
    fps = {False: [], True: []}
    on_off_timed, on_off_all, off_off, gap, prev_off = None, 0.0, 0.0, 0.0, None
    for r in range(args.repeats):
        poses, first = {}, {}
        for key in (False, True):
            line, slam, poses[key], first[key] = run(seq, args, key, args.steps)
            fps[key].append(line["fps"])
            if key:
                gap = max(gap, prediction_gap(slam, seq, first[key], args.steps))
            emit(dict(line, repeat=r, whole_run=args.whole_run))
            del slam
        n = min(poses[True].shape[0], poses[False].shape[0])
        diff = (poses[True][:n] - poses[False][:n]).abs().amax(1)
        on_off_all = max(on_off_all, float(diff.max()))
        if max(first.values()) < n:      # frames inside both timed regions
            on_off_timed = max(on_off_timed or 0.0, float(diff[max(first.values()):].max()))
        if prev_off is not None:
            off_off = max(off_off, float((poses[False] - prev_off).abs().max()))
        prev_off = poses[False]
    stat = lambda v: dict(median=round(statistics.median(v), 3), min=min(v), max=max(v))
    emit(dict(summary=True, workload="c3 (UT-MM-shaped 640x330 RGB-D + IMU)", steps=args.steps, warmup=args.warmup, repeats=args.repeats,
              track_iters=args.track_iters, map_iters=args.map_iters, fps_key_off=stat(fps[False]), fps_key_on=stat(fps[True]),
              fps_ratio_on_over_off_median=round(statistics.median(fps[True]) / statistics.median(fps[False]), 4),
              whole_run=args.whole_run, max_pose_diff_on_vs_off_timed_frames=on_off_timed, max_pose_diff_on_vs_off_all_frames=on_off_all,
              max_pose_diff_off_vs_off=off_off if args.repeats > 1 else None,
              max_device_vs_float32_host_prediction=gap))


if __name__ == "__main__":
    main()
