#!/usr/bin/env python
"""A/B of the geometry scores (mm3dgs_slam_amd/geometry.py, csrc/geometry.hip) against the chain a user runs today, on the sets of the bench
workloads' exports (30 views at 640x480 and 1200x680: the sensor frames fused and meshed at poses 1 cm off the true ones against the same
frames at the true poses, both sampled at `--density` points per m^2), on two synthetic sets of about a million points each (a 6 x 4 x 3 m room's walls sampled with two
seeds, one copy moved by a centimetre), and of the surface sampler at a million samples.  Needs the GPU; there is no fall-back.

    python tools/geometry_ab.py [--calls 200] [--untimed 20] [--baseline-calls 2] [--frames 30] [--out profiles/r16_geometry.jsonl]

(a) Grid build and query, each direction, between device events around every single call: the median, p10 and p90 of `--calls` calls after
`--untimed` untimed ones.  The query is timed on the rows as they arrive (mesh samples in triangle order) and on the same rows sorted by
cell (the build, reused on the query set; its cost is the build line of the other direction).
(b) The same distances by chunked `torch.cdist(q, ref).min(1)` on the device (float32, chunks of at most 2^28 distances), `--baseline-calls`
passes between device events after one untimed pass, and by `scipy.spatial.cKDTree(ref).query(q)` on the host (build + query, host clock,
one pass) when scipy can be imported -- the line says so when it cannot.
(c) The sampler: mm3dgs_mesh_sample_plan + mm3dgs_mesh_sample_emit at about a million samples, `--calls` calls, against the torch chain
that does the same job on the device (areas, `torch.multinomial` over them, two `torch.rand` per sample, the barycentric blend)."""
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


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def stat(v):
    return dict(median=round(statistics.median(v), 2), p10=round(pct(v, 0.1), 2), p90=round(pct(v, 0.9), 2))


def timed(fn, calls, untimed):
    """us per call between device events"""
    for _ in range(untimed):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return us


def xyz_of(rows):
    return rows[:, :3].contiguous().view(torch.float32)


def cdist_min(q, ref):
    out = torch.empty(q.shape[0], device=DEV)
    chunk = max(1, (1 << 28) // max(int(ref.shape[0]), 1))
    for i in range(0, q.shape[0], chunk):
        out[i:i + chunk] = torch.cdist(q[i:i + chunk], ref).min(1).values
    return out


class Direction:
    """One direction query -> reference through the raw entry points, buffers allocated once."""

    def __init__(self, q_rows, ref_rows, cell, max_dist, threshold):
        from mm3dgs_slam_amd import geometry as geo
        self.scorer = geo.GeometryScorer(ref_rows, cell, max_dist, threshold, DEV)
        self.q = q_rows
        self.dist = torch.empty(q_rows.shape[0], dtype=torch.float32, device=DEV)
        self.row = torch.zeros(8, dtype=torch.float64, device=DEV)
        s = self.scorer
        self.gwork = torch.empty(int(s.lib.mm3dgs_nn_grid_work_bytes(s.n_ref, *s.dims)) // 8, dtype=torch.int64, device=DEV)

    def build(self):
        from mm3dgs_slam_amd import _lib
        from mm3dgs_slam_amd.rasterizer import _stream
        s, P = self.scorer, _lib.ptr
        _lib.check(s.lib.mm3dgs_nn_grid_build(s.n_ref, P(s.rows), s.cell, s._origin, *s.dims, P(s.cell_start), P(s.sorted), P(s.counters), P(self.gwork), _stream()))

    def query(self, rows=None):
        self.scorer.query(self.q if rows is None else rows, dist=self.dist, row=self.row)


def nn_lines(emit, args, name, est, ref, cell, max_dist, threshold):
    from mm3dgs_slam_amd import geometry as geo
    if min(int(est.shape[0]), int(ref.shape[0])) == 0:
        emit(dict(part="nn", set=name, n_estimate=int(est.shape[0]), n_reference=int(ref.shape[0]), note="an empty set: not measured"))
        return
    for tag, q, r in (("estimate->reference", est, ref), ("reference->estimate", ref, est)):
        d = Direction(q, r, cell, max_dist, threshold)
        own = geo.GeometryScorer(q, cell, max_dist, threshold, DEV)      # the query set in cell order: the build reused
        q_sorted = own.sorted[:int(own.counters.cpu()[0])].contiguous()
        build = timed(d.build, args.calls, args.untimed)
        plain = timed(d.query, args.calls, args.untimed)
        row_plain = d.row.cpu().numpy().copy()
        srt = timed(lambda: d.query(q_sorted), args.calls, args.untimed)
        row_sorted = d.row.cpu().numpy().copy()
        d.query()
        ours = d.dist.clone()
        qx, rx = xyz_of(q), xyz_of(r)
        cdist_min(qx, rx)
        base = timed(lambda: cdist_min(qx, rx), args.baseline_calls, 0)
        theirs = cdist_min(qx, rx).clamp(max=max_dist)
        line = dict(part="nn", set=name, direction=tag, n_query=int(q.shape[0]), n_reference=int(r.shape[0]), cell=d.scorer.cell, grid=d.scorer.dims, max_dist=max_dist,
                    calls=args.calls, build_us=stat(build), query_us=stat(plain), query_sorted_us=stat(srt),
                    sorted_over_plain_median=round(statistics.median(srt) / statistics.median(plain), 3), row=row_plain.tolist(),
                    row_sorted_equal_counts=bool((row_plain[[0, 4, 5, 6]] == row_sorted[[0, 4, 5, 6]]).all()), cdist_calls=args.baseline_calls, cdist_us=stat(base),
                    cdist_over_build_plus_query_median=round(statistics.median(base) / (statistics.median(build) + statistics.median(plain)), 2),
                    max_abs_difference_to_cdist_float32=float((ours - theirs).abs().max()))
        try:
            from scipy.spatial import cKDTree
            qh, rh = qx.cpu().numpy().astype(np.float64), rx.cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            tree = cKDTree(rh)
            t1 = time.perf_counter()
            dk = tree.query(qh, distance_upper_bound=max_dist)[0]
            t2 = time.perf_counter()
            line.update(ckdtree_build_ms=round((t1 - t0) * 1e3, 2), ckdtree_query_ms=round((t2 - t1) * 1e3, 2),
                        max_abs_difference_to_ckdtree=float(np.abs(np.minimum(dk, max_dist) - ours.cpu().numpy().astype(np.float64)).max()))
        except ImportError:
            line.update(ckdtree="scipy is not importable here: not measured")
        emit(line)
        del d, own
        torch.cuda.empty_cache()


def room_mesh(dx=0.0):
    """The six walls of a 6 x 4 x 3 m room as twelve wall-sized triangles (108 m^2)."""
    from mm3dgs_slam_amd.pointcloud import rows_xyz
    c = np.array([[x, y, z] for z in (0, 3) for y in (0, 4) for x in (0, 6)], dtype=np.float64) + dx
    quads = [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)]
    tris = np.array([t for a, b, cc, d in quads for t in ((a, b, cc), (a, cc, d))], dtype=np.int32)
    rows = np.empty((8, 4), dtype=np.int32)
    rows[:, :3] = c.astype(np.float32).view(np.int32)
    rows[:, 3] = -1
    return torch.from_numpy(rows).to(DEV), torch.from_numpy(tris).to(DEV)


def torch_sampler(v, tris, n):
    p = xyz_of(v)[tris.long()]
    a, e1, e2 = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    area = 0.5 * torch.linalg.cross(e1, e2).norm(dim=1)
    t = torch.multinomial(area / area.sum(), n, replacement=True)
    r = torch.rand(n, 2, device=DEV)
    flip = r.sum(1, keepdim=True) > 1
    r = torch.where(flip, 1 - r, r)
    return a[t] + r[:, :1] * e1[t] + r[:, 1:] * e2[t]


def sampler_line(emit, args):
    from mm3dgs_slam_amd import _lib, geometry as geo
    from mm3dgs_slam_amd.rasterizer import _stream
    lib, P = _lib.load(), _lib.ptr
    v, tris = room_mesh()
    density = 1e6 / 108.0
    rows, c = geo.sample_mesh_device(v, tris, density, seed=0, device=DEV)
    n, m = c["samples"], int(tris.shape[0])
    work = torch.empty(int(lib.mm3dgs_mesh_sample_work_bytes(m)) // 8, dtype=torch.int64, device=DEV)
    counters = torch.empty(8, dtype=torch.int64, device=DEV)
    out = torch.empty(n, 4, dtype=torch.int32, device=DEV)
    plan = lambda: _lib.check(lib.mm3dgs_mesh_sample_plan(8, P(v), m, P(tris), density, 0, P(work), P(counters), _stream()))
    emit_ = lambda: _lib.check(lib.mm3dgs_mesh_sample_emit(8, P(v), m, P(tris), density, 0, P(work), P(out), n, P(counters), _stream()))
    plan()
    us_plan, us_emit = timed(plan, args.calls, args.untimed), timed(emit_, args.calls, args.untimed)
    us_torch = timed(lambda: torch_sampler(v, tris, n), args.calls, args.untimed)
    emit(dict(part="sampler", triangles=m, samples=n, calls=args.calls, plan_us=stat(us_plan), emit_us=stat(us_emit), torch_chain_us=stat(us_torch),
              torch_over_plan_plus_emit_median=round(statistics.median(us_torch) / (statistics.median(us_plan) + statistics.median(us_emit)), 3),
              same_bytes_as_first_call=bool(torch.equal(out, rows))))


def export_sets(args, H, W, outdir):
    """The two sets of a 30-view export: the rendered map's mesh and the sensor mesh at the ground-truth poses, sampled."""
    from mm3dgs_slam_amd import export, geometry as geo
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    frac = min(1.0, args.gaussians / (0.95 * H * W))
    cfg = default_config(device=DEV, height=H, width=W, mapping={"seed_fraction": frac}, outputdir=outdir)
    seq = SyntheticSequence(cfg, args.frames, args.gaussians, seed=0)
    slam = SLAM(cfg, seq)
    slam.step(0)
    for i in range(1, args.frames):
        slam.estimate_pose_list[i] = seq[i][2].clone()
        slam.gt_pose_list[i] = seq[i][2].clone()
    with torch.no_grad():
        box = export.mesh_bounds(slam, export.options(slam.cfg, "mesh", every=1, source="sensor"))
    voxel = float((box[3:] - box[:3]).max()) / 246.0
    opt = export.options(slam.cfg, "mesh", every=1, source="sensor", voxel=voxel)
    # the estimate: the sensor frames fused at poses 1 cm off the true ones (a map after one mapped frame renders too few surface pixels
    # to be a set worth timing: 2 484 samples at 640x480, none at 1200x680); the reference: the same frames at the true poses
    gt = export.gt_poses(slam)
    off = [p.clone() for p in gt]
    for p in off:
        p[4:] += 0.01
    sets = []
    for poses in (off, gt):
        rows, tris = export.mesh_geometry(slam, opt, poses)[:2]
        sets.append(geo.sample_mesh_device(rows, tris, args.density, seed=0, max_samples=1 << 26, device=DEV)[0])
    del slam, seq
    torch.cuda.empty_cache()
    return sets, voxel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--untimed", type=int, default=20)
    ap.add_argument("--baseline-calls", type=int, default=2)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--density", type=float, default=10000.0)
    ap.add_argument("--gaussians", type=int, default=150000, help="size of the synthetic ground-truth scene (bench.py's default)")
    ap.add_argument("--skip-exports", action="store_true")
    ap.add_argument("--skip-room", action="store_true", help="leave out the sampler and the synthetic million-point sets")
    ap.add_argument("--out", default="", help="append the lines to this file as well")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from mm3dgs_slam_amd import geometry as geo

    def emit(d):
        d = dict(d, device=torch.cuda.get_device_name(0))
        print(json.dumps(d), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    if not args.skip_room:
        sampler_line(emit, args)
        v, tris = room_mesh()
        ref = geo.sample_mesh_device(v, tris, 1e6 / 108.0, seed=0, device=DEV)[0]
        v2, _ = room_mesh(0.01)
        est = geo.sample_mesh_device(v2, tris, 1e6 / 108.0, seed=1, device=DEV)[0]
        nn_lines(emit, args, "room 6x4x3, two seeds, 1 cm apart", est, ref, 0.05, 1.0, 0.05)
    if not args.skip_exports:
        with tempfile.TemporaryDirectory() as tmp:
            for H, W in SHAPES:
                (est, ref), voxel = export_sets(args, H, W, tmp)
                nn_lines(emit, args, f"{args.frames}-view export {W}x{H}, mesh voxel {voxel:.4f}", est, ref, 0.05, 1.0, 0.05)


if __name__ == "__main__":
    main()
