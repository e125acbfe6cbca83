#!/usr/bin/env python
"""A/B of eval_on_device at the shapes of the bench workloads (640x480 and 1200x680).  Key off = the host chain of SLAM.evaluate_images
(eval_utils.psnr + loss_utils.ssim in torch: five grouped 11x11 convolutions and the operators around them, and two `.cpu()` read-backs
per frame); key on = eval_utils.image_metrics_device (mm3dgs_eval_image: two launches into a row of a device table, which also holds the
depth L1 the host chain does not compute).  Needs the GPU; there is no fall-back.

    python tools/eval_ab.py [--calls 200] [--untimed 20] [--frames 30] [--repeats 5] [--out profiles/r13_eval.jsonl]

(a) One frame's scoring, timed between device events around every single call, host chain and device call alternating in the same process:
the median, p10 and p90 of `--calls` calls after `--untimed` calls of each side.  The inputs are a frame of the workload itself: the map
seeded and mapped on frame 0, rendered at the pose of a later frame, against that frame's colour and depth.

(b) A whole SLAM.evaluate_images over `--frames` frames (eval_every 1: one render and one scoring per frame) from the same state -- the
map after frame 0, every later frame at its ground-truth pose --, key off and on alternating, `--repeats` times after one untimed pass of
each; host clock, device synchronised at both ends.  Reported next to the largest difference of the two settings' PSNR and SSIM lists."""
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
SHAPES = [(480, 640), (680, 1200)]


def config(args, H, W):
    from mm3dgs_slam_amd.config import default_config
    frac = min(1.0, args.gaussians / (0.95 * H * W))      # bench.py's seeding fraction
    return default_config(device=DEV, height=H, width=W, eval_every=1, mapping={"seed_fraction": frac})


def start(args, H, W):
    """The sequence and a SLAM object after frame 0, every later frame at its ground-truth pose (nothing of this is timed)."""
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = config(args, H, W)
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


def call_times(slam, seq, args, emit, H, W):
    """(a): us per scoring of one frame"""
    from mm3dgs_slam_amd.eval_utils import image_metrics_device, image_metrics_host, psnr
    from mm3dgs_slam_amd.loss_utils import ssim
    idx = min(5, args.frames - 1)
    color, gt_depth = seq[idx][0], seq[idx][1]
    with torch.no_grad():
        result = slam.renderer.render(slam.gaussians, camera_pose=slam.estimate_pose_list[idx])
    image, depth = result["render"], result["depth"][0]
    table = torch.zeros(1, 16, dtype=torch.float64, device=DEV)

    def host():
        return psnr(image, color).mean().detach().cpu().numpy(), ssim(image, color).detach().cpu().numpy()

    def device():
        return image_metrics_device(image, color, depth, gt_depth, table[0])

    one = {"host": host, "device": device}
    with torch.no_grad():
        for side in one:
            for _ in range(args.untimed):
                one[side]()
        torch.cuda.synchronize()
        us = {"host": [], "device": []}
        for _ in range(args.calls):
            for side in one:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                one[side]()
                e1.record()
                e1.synchronize()
                us[side].append(e0.elapsed_time(e1) * 1e3)
        p, s = host()
        row = device().cpu().numpy()
        ref = image_metrics_host(image, color, depth, gt_depth).cpu().numpy()
    stat = lambda v: dict(median=round(statistics.median(v), 2), p10=round(pct(v, 0.1), 2), p90=round(pct(v, 0.9), 2))
    emit(dict(part="a", shape=f"{W}x{H}", calls=args.calls, untimed=args.untimed, host_us_per_call=stat(us["host"]), device_us_per_call=stat(us["device"]),
              host_over_device_median=round(statistics.median(us["host"]) / statistics.median(us["device"]), 3),
              device_faster=bool(statistics.median(us["device"]) < statistics.median(us["host"])),
              psnr_host=float(p), psnr_device=float(row[0]), psnr_float64=float(ref[0]), ssim_host=float(s), ssim_device=float(row[1]),
              ssim_float64=float(ref[1]), depth_l1_device=float(row[2]), depth_l1_float64=float(ref[2])))


def evaluation_times(slam, args, emit, H, W):
    """(b): seconds per evaluate_images over all frames"""
    def run(key):
        slam.cfg["eval_on_device"] = key
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lists = slam.evaluate_images(args.frames)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, lists

    for key in (False, True):
        run(key)
    ms, lists = {False: [], True: []}, {}
    for _ in range(args.repeats):
        for key in (False, True):
            sec, lists[key] = run(key)
            ms[key].append(sec * 1e3)
    slam.cfg["eval_on_device"] = False
    stat = lambda v: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
    d_psnr = max(abs(float(a) - float(b)) for a, b in zip(lists[True][0], lists[False][0]))
    d_ssim = max(abs(float(a) - float(b)) for a, b in zip(lists[True][1], lists[False][1]))
    emit(dict(part="b", shape=f"{W}x{H}", frames=args.frames, repeats=args.repeats, gaussians=int(slam.gaussians.get_xyz.shape[0]),
              ms_key_off=stat(ms[False]), ms_key_on=stat(ms[True]), off_over_on_median=round(statistics.median(ms[False]) / statistics.median(ms[True]), 3),
              ms_per_frame_key_off=round(statistics.median(ms[False]) / args.frames, 4), ms_per_frame_key_on=round(statistics.median(ms[True]) / args.frames, 4),
              max_psnr_diff_db=d_psnr, max_ssim_diff=d_ssim))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--untimed", type=int, default=20)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
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

    for H, W in SHAPES:
        slam, seq = start(args, H, W)
        call_times(slam, seq, args, emit, H, W)
        evaluation_times(slam, args, emit, H, W)
        del slam, seq
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
