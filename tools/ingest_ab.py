#!/usr/bin/env python
"""A/B of frame ingest for recorded sequences (mm3dgs_slam_amd/dataset.py): the host chain (`ingest_on_device: false`: float64 resize on
the CPU, upload of 16 bytes per pixel, permute, / 255) against mm3dgs_ingest_frame (`true`: pinned staging, upload of the raw 5 bytes per
source pixel, one launch).  Needs the GPU.

    python tools/ingest_ab.py [--fetches 200] [--steps 20] [--warmup 2] [--repeats 3] [--out profiles/r11_ingest.jsonl]

(a) Per-frame time of `seq[i]`, device synchronised, host clock, with the PNG decode EXCLUDED (the decoder hands out pre-decoded arrays;
the copy into the staging slot stays in: it is part of both paths); prefetch off; host and device path alternating fetch by fetch, median
of `--fetches` each after an untimed round; at 640x480 native (frames of the benchmark's synthetic sequence, quantised) and at
1280x660 -> 640x330 (UT-MM's exact 2x; synthetic RGB-D frames of that size).  The two paths' outputs are compared once per shape.
The summary says whether the device path's median is below the host path's at BOTH shapes -- the condition under which it is the default.

(b) PNG decode time per frame on its own (PIL, this host's CPU), at both sizes.

(c) Frames/s of a SLAM run over a recorded copy of the benchmark's synthetic sequence (bench.py's defaults: 640x480, 150 k Gaussians,
100 tracking + 150 mapping iterations, seed 0): the frames quantised to uint8 / uint16 and written as PNG to a temporary directory.
Every run is a fresh SLAM object from the same seeds: frame 0 and `--warmup` frames untimed, then `--steps` frames timed like bench.py
(host clock, device synchronised at both ends); the configurations alternate, `--repeats` times after one short untimed pass of each:
host ingest without prefetch, device ingest without prefetch, device ingest with prefetch, and -- the ceiling -- an in-memory sequence
built from the same quantised frames (what bench.py times: float32 frames already on the device).

(d) The monocular depth estimate of a recorded sequence (`est_depth_dir`): per-frame time of the host path (`ingest_est_host`: float64
bilinear on the CPU, upload of 4 bytes per output pixel) against the device path (pinned raw array up non-blocking, `mm3dgs_ingest_est`),
device synchronised, file decode excluded, alternating call by call, median of `--fetches` each after an untimed round; at 384x512
float16 -> 480x640 (the network's output) and at 480x640 float32 native.  The two outputs are compared once per shape.  The device path
stays governed by `ingest_on_device`; this part only reports."""
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


def config(args, **top):
    from mm3dgs_slam_amd.config import default_config
    frac = min(1.0, args.gaussians / (0.95 * args.height * args.width))      # bench.py's seeding fraction
    return default_config(device=DEV, height=args.height, width=args.width, tracking={"iters": args.track_iters},
                          mapping={"iters": args.map_iters, "seed_fraction": frac}, **top)


def recorded_config(args, root, scene, Hs, Ws, H, W, on_device, prefetch):
    cfg = config(args, dataset="tum", inputdir=root, scene=scene, ingest_on_device=on_device, prefetch=prefetch)
    cfg["desired_height"], cfg["desired_width"] = H, W
    cfg["cam"].update(image_height=Hs, image_width=Ws)
    return cfg


class MemorySequence:
    """The frames of a recorded sequence, ingested once and kept on the device."""

    def __init__(self, rec):
        self.frames = [tuple(t.clone() for t in rec[i][:2]) for i in range(len(rec))]
        self.poses, self.tstamps, self.tf = rec.poses, rec.tstamps, rec.tf

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return self.frames[i][0], self.frames[i][1], self.poses[i]


class CachedDecoder:
    """Pre-decoded frames by path: takes the PNG decode out of the timed fetch."""

    def __init__(self, rec, n):
        from mm3dgs_slam_amd.dataset import decode_png
        self.cache = {(rec.color_paths[i], rec.depth_paths[i]): decode_png(rec.color_paths[i], rec.depth_paths[i]) for i in range(n)}

    def __call__(self, color_path, depth_path):
        return self.cache[(color_path, depth_path)]


def fetch_times(args, root, scene, Hs, Ws, H, W, emit):
    from mm3dgs_slam_amd.dataset import RecordedSequence
    seqs = {}
    for on_device in (False, True):
        seqs[on_device] = RecordedSequence(recorded_config(args, root, scene, Hs, Ws, H, W, on_device, False), frames=args.distinct)
        seqs[on_device]._decoder = CachedDecoder(seqs[on_device], len(seqs[on_device]))
    n = len(seqs[True])
    h, d = seqs[False][1], seqs[True][1]
    torch.cuda.synchronize()
    agree = dict(color_bit_identical=bool(torch.equal(h[0], d[0])), depth_bit_identical=bool(torch.equal(h[1], d[1])),
                 color_max_abs_diff=float((h[0] - d[0]).abs().max()))
    for k in range(2 * n):      # untimed round
        for on_device in (False, True):
            seqs[on_device][k % n]
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for k in range(args.fetches):
        for on_device in (False, True):
            t0 = time.perf_counter()
            seqs[on_device][k % n]
            torch.cuda.synchronize()
            ms[on_device].append((time.perf_counter() - t0) * 1e3)
    for s in seqs.values():
        s.close()
    q = lambda v: dict(median=round(statistics.median(v), 4), p10=round(float(np.percentile(v, 10)), 4), p90=round(float(np.percentile(v, 90)), 4))
    line = dict(part="a", shape=f"{Ws}x{Hs} -> {W}x{H}", fetches=args.fetches, distinct_frames=n, host_ms_per_frame=q(ms[False]),
                device_ms_per_frame=q(ms[True]), device_median_below_host_median=bool(statistics.median(ms[True]) < statistics.median(ms[False])),
                upload_bytes_host=16 * H * W, upload_bytes_device=5 * Hs * Ws, **agree)
    emit(line)
    return line


def est_times(args, Hs, Ws, dtype, H, W, emit):
    from mm3dgs_slam_amd.dataset import ingest_est_device, ingest_est_host
    g = torch.Generator().manual_seed(5)
    raws = [(torch.rand(Hs, Ws, generator=g) * 3000.0).to(dtype) for _ in range(args.distinct)]
    pinned = [r.clone().pin_memory() for r in raws]
    dev = torch.empty(Hs, Ws, dtype=dtype, device=DEV)

    def host(k):
        return ingest_est_host(raws[k].numpy(), 1.0, H, W, DEV)

    def device(k):
        dev.copy_(pinned[k], non_blocking=True)
        return ingest_est_device(dev, 1.0, H, W)

    h, d = host(1), device(1)
    torch.cuda.synchronize()
    agree = dict(bit_identical=bool(torch.equal(h, d)), max_abs_diff=float((h - d).abs().max()))
    n = len(raws)
    for k in range(2 * n):      # untimed round
        host(k % n), device(k % n)
    torch.cuda.synchronize()
    ms = {"host": [], "device": []}
    for k in range(args.fetches):
        for name, fn in (("host", host), ("device", device)):
            t0 = time.perf_counter()
            fn(k % n)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    q = lambda v: dict(median=round(statistics.median(v), 4), p10=round(float(np.percentile(v, 10)), 4), p90=round(float(np.percentile(v, 90)), 4))
    emit(dict(part="d", what="monocular depth estimate, per frame, file decode excluded", shape=f"{Ws}x{Hs} {str(dtype).split('.')[-1]} -> {W}x{H}",
              fetches=args.fetches, host_ms_per_frame=q(ms["host"]), device_ms_per_frame=q(ms["device"]),
              upload_bytes_host=4 * H * W, upload_bytes_device=Hs * Ws * raws[0].element_size(), **agree))


def decode_times(rec_paths, label, emit):
    from mm3dgs_slam_amd.dataset import decode_png
    ms = []
    for _ in range(3):
        for c, d in rec_paths:
            t0 = time.perf_counter()
            decode_png(c, d)
            ms.append((time.perf_counter() - t0) * 1e3)
    emit(dict(part="b", what="PNG decode (colour + depth) with PIL, per frame", frames=label, decodes=len(ms), ms_median=round(statistics.median(ms), 3),
              ms_min=round(min(ms), 3), ms_max=round(max(ms), 3)))


def slam_run(args, make_seq, steps):
    from mm3dgs_slam_amd.slam import SLAM
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg, seq = make_seq()
    slam = SLAM(cfg, seq)
    slam.step(0)
    torch.cuda.synchronize()
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    for i in range(1, 1 + args.warmup):
        slam.step(i)
    torch.cuda.synchronize()
    first = 1 + args.warmup
    t0 = time.perf_counter()
    for i in range(first, first + steps):
        slam.step(i)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    poses = torch.stack([slam.estimate_pose_list[i].detach() for i in range(first, first + steps)]).cpu()
    if hasattr(seq, "close"):
        seq.close()
    return dict(steps=steps, seconds=round(sec, 4), fps=round(steps / sec, 3), ms_per_frame=round(sec / steps * 1e3, 3),
                gaussians=int(slam.gaussians.get_xyz.shape[0]), keyframes=len(slam.mapper.keyframes)), poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fetches", type=int, default=200)
    ap.add_argument("--distinct", type=int, default=8, help="distinct frames the timed fetches cycle through")
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
    from mm3dgs_slam_amd import dataset as ds
    from mm3dgs_slam_amd import synthetic
    from mm3dgs_slam_amd.slam import SyntheticSequence

    def emit(d):
        d = dict(d, device=torch.cuda.get_device_name(0))
        print(json.dumps(d), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    n_frames = args.warmup + args.steps + 1
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    src = SyntheticSequence(config(args), n_frames, args.gaussians, seed=0)
    scale = float(config(args)["cam"]["png_depth_scale"])
    with tempfile.TemporaryDirectory() as root:
        ds.write_tum_sequence(os.path.join(root, "bench"), [ds.quantise_frame(c, d, scale) for c, d in src.frames], src.poses,
                              [1000.0 + 0.1 * i for i in range(n_frames)])
        big = []
        for k in range(4):
            c, d = synthetic.rgbd_frame(660, 1280, seed=20 + k)
            big.append(ds.quantise_frame(c, d, 1000.0))
        ds.write_tum_sequence(os.path.join(root, "utmm_size"), big, src.poses[:4], [2000.0 + 0.1 * i for i in range(4)])
        del src
        torch.cuda.empty_cache()

        H, W = args.height, args.width
        a = [fetch_times(args, root, "bench", H, W, H, W, emit), fetch_times(args, root, "utmm_size", 660, 1280, 330, 640, emit)]
        emit(dict(part="a", summary=True, device_median_below_host_median_at_both_shapes=all(l["device_median_below_host_median"] for l in a),
                  note="seq[i] synchronised, PNG decode excluded, prefetch off, host and device path alternating"))

        paths = lambda scene, n: [(os.path.join(root, scene, "rgb", f"{i:04d}.png"), os.path.join(root, scene, "depth", f"{i:04d}.png")) for i in range(n)]
        decode_times(paths("bench", min(8, n_frames)), f"{W}x{H} (rendered synthetic frames)", emit)
        decode_times(paths("utmm_size", 4), "1280x660 (synthetic RGB-D frames)", emit)

        est_times(args, 384, 512, torch.float16, H, W, emit)
        est_times(args, H, W, torch.float32, H, W, emit)

        def recorded(on_device, prefetch):
            def make():
                cfg = recorded_config(args, root, "bench", H, W, H, W, on_device, prefetch)
                return cfg, ds.RecordedSequence(cfg)
            return make

        def memory():
            cfg = recorded_config(args, root, "bench", H, W, H, W, False, False)
            rec = ds.RecordedSequence(cfg)
            mem = MemorySequence(rec)
            rec.close()
            return cfg, mem

        configs = {"host_ingest_no_prefetch": recorded(False, False), "device_ingest_no_prefetch": recorded(True, False),
                   "device_ingest_prefetch": recorded(True, True), "in_memory_ceiling": memory}
        for make in configs.values():      # untimed pass of each configuration
            slam_run(args, make, 2)
        fps = {k: [] for k in configs}
        ref_poses, max_diff = None, 0.0
        for r in range(args.repeats):
            for name, make in configs.items():
                line, poses = slam_run(args, make, args.steps)
                fps[name].append(line["fps"])
                ref_poses = poses if ref_poses is None else ref_poses
                max_diff = max(max_diff, float((poses - ref_poses).abs().max()))
                emit(dict(line, part="c", configuration=name, repeat=r))
        stat = lambda v: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
        emit(dict(part="c", summary=True, workload=f"recorded copy of bench.py's synthetic sequence ({W}x{H}, {args.gaussians} Gaussians)", steps=args.steps,
                  warmup=args.warmup, repeats=args.repeats, track_iters=args.track_iters, map_iters=args.map_iters,
                  fps={k: stat(v) for k, v in fps.items()}, max_pose_diff_between_any_two_runs=max_diff))


if __name__ == "__main__":
    main()
