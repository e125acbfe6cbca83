#!/usr/bin/env python
"""What a debug-video frame costs (mm3dgs_slam_amd/debug_frames.py, csrc/mosaic.hip).  Needs the GPU.  Recorded, not gated: the feature is
opt-in and its two composers give the same bytes, so no threshold decides anything.

    python tools/video_frame_ab.py [--calls 200] [--host-calls 20] [--frames 30] [--repeats 2] [--out profiles/r12_video_frame.jsonl]

(a) The 2 x 3 mosaic of one frame at 480x640 and at 330x640, panels on the device (the render is a [6,H,W] tensor, as in a run):
    * `compose_device`: mm3dgs_mosaic, per call between two device events, median of `--calls` after 20 untimed calls; and the same
      followed by the copy of the finished frame to pinned host memory, host clock, device synchronised;
    * the reference's structure (slam/SLAM.py:233-276 with utils/depth_utils.py:14-34): every depth image to the host, normalised and
      looked up there (the committed table in place of the matplotlib call), the float64 colour image back to the device, torch.cat,
      `* 255`, `.to(uint8)` on the device and the frame to the host -- host clock, device synchronised, median of `--host-calls`.
    The two frames are compared once per shape.

(b) Frames/s of a synthetic run (bench.py's defaults: 640x480, 150 k Gaussians, 100 tracking + 150 mapping iterations, seed 0) of
    `--frames` frames with `debug.create_video` on against off: a fresh SLAM object from the same seeds each time, frame 0 untimed, the
    rest timed with a host clock, device synchronised at both ends and the PNG writer drained inside the timed window; off and on
    alternate, `--repeats` times after one short untimed pass of each.  The poses of all runs are compared.

(c) Where a video frame's time goes (a run writes two per frame): the device side -- the extra render, the mosaic and the copy of the frame to
    pinned host memory, device synchronised -- and the host side, the PNG encode of that frame by the writer thread."""
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


def panels_for(H, W, seed=0):
    from mm3dgs_slam_amd import debug_frames as df
    g = torch.Generator().manual_seed(seed)
    render6 = torch.rand(6, H, W, generator=g).to(DEV)
    render6[3] = 0.5 + 3.0 * render6[3]
    gt_color = torch.rand(3, H, W, generator=g).to(DEV)
    gt_depth = (0.5 + 3.0 * torch.rand(H, W, generator=g)).to(DEV)
    est = (0.4 + 3.2 * torch.rand(H, W, generator=g)).to(DEV)
    return [(df.COLOR, gt_color, None), (df.COLOR, render6[:3], None), (df.ABSDIFF, render6[:3], gt_color),
            (df.DEPTH, gt_depth, None), (df.DEPTH, render6[3], None), (df.DEPTH, est, None)]


def reference_structure(panels):
    """The reference's frame, transfer for transfer: three depth images down, three float64 colour images up, one uint8 frame down."""
    from mm3dgs_slam_amd import debug_frames as df
    top = torch.cat([panels[0][1], panels[1][1], torch.abs(panels[2][1] - panels[2][2])], dim=2)
    bottom = torch.cat([df.depth_to_rgb_host(p[1]).to(DEV) for p in panels[3:]], dim=2)
    vid = torch.cat([top, bottom], dim=1)
    return (vid * 255).to(torch.uint8).permute(1, 2, 0).cpu()


def compose_times(args, H, W, emit):
    from mm3dgs_slam_amd import debug_frames as df
    panels = panels_for(H, W)
    pinned = torch.empty(2 * H, 3 * W, 3, dtype=torch.uint8, pin_memory=True)
    dev_frame = df.compose_device(panels, 2, 3).cpu()
    same = bool(torch.equal(dev_frame, reference_structure(panels))) and bool(torch.equal(dev_frame, df.compose_host(panels, 2, 3)))
    for _ in range(20):
        df.compose_device(panels, 2, 3)
    torch.cuda.synchronize()
    kernel_ms, with_copy_ms, host_ms = [], [], []
    for _ in range(args.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        df.compose_device(panels, 2, 3)
        e1.record()
        e1.synchronize()
        kernel_ms.append(e0.elapsed_time(e1))
    for _ in range(args.calls):
        t0 = time.perf_counter()
        pinned.copy_(df.compose_device(panels, 2, 3), non_blocking=True)
        torch.cuda.synchronize()
        with_copy_ms.append((time.perf_counter() - t0) * 1e3)
    reference_structure(panels)
    for _ in range(args.host_calls):
        t0 = time.perf_counter()
        reference_structure(panels)
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    q = lambda v: dict(median=round(statistics.median(v), 4), p10=round(float(np.percentile(v, 10)), 4), p90=round(float(np.percentile(v, 90)), 4))
    emit(dict(part="a", shape=f"{W}x{H}", mosaic="2x3", calls=args.calls, host_calls=args.host_calls, compose_device_ms_events=q(kernel_ms),
              compose_device_plus_download_ms=q(with_copy_ms), reference_structure_ms=q(host_ms), same_bytes=same,
              bytes_in=int(4 * H * W * (3 + 3 + 6 + 3)), bytes_out=int(2 * H * 3 * W * 3)))


def slam_run(args, frames, video, outdir):
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    frac = min(1.0, args.gaussians / (0.95 * args.height * args.width))      # bench.py's seeding fraction
    cfg = default_config(device=DEV, height=args.height, width=args.width, tracking={"iters": args.track_iters},
                         mapping={"iters": args.map_iters, "seed_fraction": frac}, outputdir=outdir,
                         debug={"get_runtime_stats": False, "create_video": video, "save_keyframes": False})
    seq = SyntheticSequence(cfg, frames, args.gaussians, seed=0)
    slam = SLAM(cfg, seq)
    slam.step(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(1, frames):
        slam.step(i)
    if slam.frame_sink is not None:
        slam.frame_sink.close()
        slam.frame_sink = None
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    poses = torch.stack([p.detach() for p in slam.estimate_pose_list]).cpu()
    written = len(os.listdir(os.path.join(outdir, "debug_video"))) if video else 0
    return dict(frames_timed=frames - 1, seconds=round(sec, 4), fps=round((frames - 1) / sec, 3), ms_per_frame=round(sec / (frames - 1) * 1e3, 3),
                video_frames_written=written, gaussians=int(slam.gaussians.get_xyz.shape[0])), poses


def video_frame_parts(args, outdir, emit):
    """(c) where a video frame's time goes, on the map of a 3-frame run: the device side (render at the estimated pose, mosaic, copy to pinned
    host memory; host clock, device synchronised) and the host side (PNG encode of that frame with PIL, compress_level=1, this host's CPU)."""
    import io
    from PIL import Image
    from mm3dgs_slam_amd import debug_frames as df
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    frac = min(1.0, args.gaussians / (0.95 * args.height * args.width))
    cfg = default_config(device=DEV, height=args.height, width=args.width, tracking={"iters": args.track_iters},
                         mapping={"iters": args.map_iters, "seed_fraction": frac}, outputdir=outdir)
    seq = SyntheticSequence(cfg, 3, args.gaussians, seed=0)
    slam = SLAM(cfg, seq)
    for i in range(3):
        slam.step(i)
    color, depth, _ = seq[2]
    pinned = torch.empty(2 * args.height, 3 * args.width, 3, dtype=torch.uint8, pin_memory=True)

    def device_side():
        with torch.no_grad():
            r = slam.renderer.render(slam.gaussians, camera_pose=slam.estimate_pose_list[2])
            frame = df.compose_device([(df.COLOR, color, None), (df.COLOR, r["render"], None), (df.ABSDIFF, r["render"], color),
                                       (df.DEPTH, depth, None), (df.DEPTH, r["depth"][0], None), (df.DEPTH, depth, None)], 2, 3)
            pinned.copy_(frame, non_blocking=True)
        torch.cuda.synchronize()

    for _ in range(5):
        device_side()
    dev_ms, png_ms, size = [], [], 0
    for _ in range(50):
        t0 = time.perf_counter()
        device_side()
        dev_ms.append((time.perf_counter() - t0) * 1e3)
    for _ in range(10):
        buf = io.BytesIO()
        t0 = time.perf_counter()
        Image.fromarray(pinned.numpy()).save(buf, format="PNG", compress_level=1)
        png_ms.append((time.perf_counter() - t0) * 1e3)
        size = buf.tell()
    q = lambda v: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
    emit(dict(part="c", what="one video frame: render + mosaic + copy to pinned memory (device synchronised) | PNG encode on the host (PIL, compress_level=1)",
              shape=f"{3 * args.width}x{2 * args.height}", render_compose_download_ms=q(dev_ms), png_encode_ms=q(png_ms), png_bytes=size,
              gaussians=int(slam.gaussians.get_xyz.shape[0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--host-calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--gaussians", type=int, default=150000, help="size of the synthetic ground-truth scene (bench.py's default)")
    ap.add_argument("--track-iters", type=int, default=100)
    ap.add_argument("--map-iters", type=int, default=150)
    ap.add_argument("--out", default="", help="append the lines to this file as well")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"

    def emit(d):
        d = dict(d, device=torch.cuda.get_device_name(0))
        print(json.dumps(d), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    for H, W in ((480, 640), (330, 640)):
        compose_times(args, H, W, emit)

    with tempfile.TemporaryDirectory() as root:
        runs = 0

        def run(frames, video):
            nonlocal runs
            runs += 1
            return slam_run(args, frames, video, os.path.join(root, f"run{runs}"))

        for video in (False, True):      # untimed pass of each
            run(3, video)
        video_frame_parts(args, os.path.join(root, "parts"), emit)
        fps = {False: [], True: []}
        ref_poses, max_diff = None, 0.0
        for r in range(args.repeats):
            for video in (False, True):
                line, poses = run(args.frames, video)
                fps[video].append(line["fps"])
                ref_poses = poses if ref_poses is None else ref_poses
                max_diff = max(max_diff, float((poses - ref_poses).abs().max()))
                emit(dict(line, part="b", create_video=video, repeat=r))
        stat = lambda v: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))
        emit(dict(part="b", summary=True, workload=f"synthetic sequence ({args.width}x{args.height}, {args.gaussians} Gaussians)", frames=args.frames,
                  repeats=args.repeats, track_iters=args.track_iters, map_iters=args.map_iters, fps_video_off=stat(fps[False]), fps_video_on=stat(fps[True]),
                  max_pose_diff_between_any_two_runs=max_diff))


if __name__ == "__main__":
    main()
