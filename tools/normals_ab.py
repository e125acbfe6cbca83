#!/usr/bin/env python
"""A/B of the normals (normal consistency for the geometry scores, vertex normals for mesh.ply) on the sensor meshes of tools/mesh_ab.py
at the shapes of the bench workloads (640x480 and 1200x680): the export's views fused into a 256^3 volume and meshed.  The reference is that
mesh, the estimate the same mesh moved by 5 mm along x.  Needs the GPU; there is no fall-back.

    python tools/normals_ab.py [--calls 200] [--untimed 20] [--frames 30] [--repeats 3] [--out profiles/r21_normals.jsonl]

Every device timing is taken between device events around every single call, the two sides alternating in the same process: the median,
p10 and p90 of `--calls` calls after `--untimed` calls of each side.

(a) mm3dgs_nn_query_index against the unchanged mm3dgs_nn_query on the same sets (the samples of the two meshes at `--density`): the cost
    of keeping the index.
(b) mm3dgs_normal_consistency against a torch chain of the same rule in float64 (gather of the corners, `torch.cross`, the norms, the dot,
    the clamp, the means).
(c) mm3dgs_mesh_vertex_normals against a float32 torch chain (`torch.cross`, three `index_add_`, normalise).
(d) mm3dgs_mesh_vertex_normals on a one-vertex fan of 2^16 triangles: every triangle's adds land on the same three words.  Nothing to
    compare against; it shows what contention on one word costs.
(e) A whole SLAM.evaluate_geometry (`estimate: mesh`, `reference: sensor`) with `geometry.normals` on against off, `--repeats` times each
    after one untimed pass; host clock, device synchronised at both ends.
(f) A whole SLAM.export_mesh over `--frames` views with `mesh.normals` on against off, the same way."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ab      # noqa: E402  (start, lattice, stat: the same scenes and the same statistics)

DEV = mesh_ab.DEV


def timed(sides, calls, untimed):
    """{name: [us per call]} of the callables in `sides`, alternating."""
    for _ in range(untimed):
        for _, fn in sides:
            fn()
    torch.cuda.synchronize()
    us = {name: [] for name, _ in sides}
    for _ in range(calls):
        for name, fn in sides:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3)
    return us


def ratio(us, a, b):
    return round(statistics.median(us[a]) / statistics.median(us[b]), 3)


def sensor_mesh(slam, voxel, box):
    from mm3dgs_slam_amd import export
    pad = 5.0 * voxel
    opt = export.options(slam.cfg, "mesh", every=1, voxel=voxel, source="sensor")
    opt["bounds"] = [float(v) for v in np.concatenate([box[:3] - pad, box[3:] + pad])]
    rows, tris = export.mesh_geometry(slam, opt)[:2]
    return rows.contiguous(), tris.contiguous()


def moved(rows, dx):
    xyz = rows[:, :3].contiguous().view(torch.float32).clone()
    xyz[:, 0] += dx
    return torch.cat([xyz.view(torch.int32), rows[:, 3:]], 1).contiguous()


def torch_consistency(tri_q, index, tri_r, mesh_q, mesh_r):
    def normals(mesh):
        p = mesh[0][:, :3].contiguous().view(torch.float32).double()
        t = mesh[1].long()
        return torch.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]], dim=1)
    found = index >= 0
    j = index.clamp(min=0).long()
    a, b = normals(mesh_q)[tri_q.long()], normals(mesh_r)[tri_r.long()[j]]
    dot = ((a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))).clamp(-1.0, 1.0).float()
    dot = torch.where(found, dot, torch.full_like(dot, float("nan")))
    d = dot[found].double()
    return dot, torch.stack([found.sum().double(), d.abs().mean(), d.mean(), d.abs().min()])


def torch_vertex_normals(rows, tris):
    p = rows[:, :3].contiguous().view(torch.float32)
    t = tris.long()
    c = torch.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]], dim=1)
    s = torch.zeros_like(p)
    for k in range(3):
        s.index_add_(0, t[:, k], c)
    return s / s.norm(dim=1, keepdim=True).clamp(min=1e-30)


def kernel_parts(args, emit, shape, est, ref):
    from mm3dgs_slam_amd import geometry as geo
    rows_e, ce, tri_e = geo.sample_mesh_device(est[0], est[1], args.density, 0, 1 << 26, DEV, want_tri=True)
    rows_r, cr, tri_r = geo.sample_mesh_device(ref[0], ref[1], args.density, 0, 1 << 26, DEV, want_tri=True)
    scorer = geo.GeometryScorer(rows_r, 0.05, 1.0, 0.05, DEV)
    nq = int(rows_e.shape[0])
    dist, row, index = torch.empty(nq, dtype=torch.float32, device=DEV), torch.zeros(8, dtype=torch.float64, device=DEV), torch.empty(nq, dtype=torch.int32, device=DEV)
    us = timed((("nn_query", lambda: scorer.query(rows_e, dist=dist, row=row)), ("nn_query_index", lambda: scorer.query(rows_e, dist=dist, row=row, index=index))),
               args.calls, args.untimed)
    sizes = dict(shape=shape, vertices=int(est[0].shape[0]), triangles=int(est[1].shape[0]), queries=nq, references=int(rows_r.shape[0]), density=args.density,
                 calls=args.calls, untimed=args.untimed)
    emit(dict(sizes, part="a", nn_query_us=mesh_ab.stat(us["nn_query"]), nn_query_index_us=mesh_ab.stat(us["nn_query_index"]),
              index_over_plain_median=ratio(us, "nn_query_index", "nn_query"), without_a_row=int((index < 0).sum())))
    dot, nrow = torch.empty(nq, dtype=torch.float32, device=DEV), torch.zeros(8, dtype=torch.float64, device=DEV)
    us = timed((("torch", lambda: torch_consistency(tri_e, index, tri_r, est, ref)),
                ("device", lambda: geo.normal_consistency_device(tri_e, index, tri_r, est, ref, dot=dot, row=nrow, device=DEV))), args.calls, args.untimed)
    tdot, trow = torch_consistency(tri_e, index, tri_r, est, ref)
    emit(dict(sizes, part="b", torch_us=mesh_ab.stat(us["torch"]), device_us=mesh_ab.stat(us["device"]), torch_over_device_median=ratio(us, "torch", "device"),
              row=nrow.cpu().tolist(), torch_row=trow.cpu().tolist(), max_dot_difference=float((dot - tdot)[index >= 0].abs().max())))
    us = timed((("torch", lambda: torch_vertex_normals(*est)), ("device", lambda: geo.vertex_normals_device(est[0], est[1], DEV))), args.calls, args.untimed)
    normals, counters = geo.vertex_normals_device(est[0], est[1], DEV)
    emit(dict(sizes, part="c", torch_us=mesh_ab.stat(us["torch"]), device_us=mesh_ab.stat(us["device"]), torch_over_device_median=ratio(us, "torch", "device"),
              counters=counters.cpu().tolist()[:3], max_component_difference=float((normals - torch_vertex_normals(*est)).abs().max())))


def fan_part(args, emit):
    from mm3dgs_slam_amd import geometry as geo
    m = 1 << 16
    a = 2.0 * np.pi * np.arange(m) / m
    p = np.concatenate([[[0.0, 0.0, 0.7]], np.stack([np.cos(a), np.sin(a), np.zeros(m)], 1)]).astype(np.float32)
    rows = torch.from_numpy(np.concatenate([p.view(np.int32), np.full((m + 1, 1), -1, dtype=np.int32)], 1)).to(DEV)
    k = np.arange(m)
    tris = torch.from_numpy(np.stack([np.zeros(m, dtype=np.int64), 1 + k, 1 + (k + 1) % m], 1).astype(np.int32)).to(DEV)
    spread = tris.clone()
    spread[:, 0] = tris[:, 1]      # the same number of triangles without the shared apex (degenerate: rejected, nothing is added)
    us = timed((("fan", lambda: geo.vertex_normals_device(rows, tris, DEV)), ("rejected", lambda: geo.vertex_normals_device(rows, spread, DEV))), args.calls, args.untimed)
    emit(dict(part="d", triangles=m, valence_of_vertex_0=m, calls=args.calls, fan_us=mesh_ab.stat(us["fan"]), same_size_all_rejected_us=mesh_ab.stat(us["rejected"]),
              apex_normal=geo.vertex_normals_device(rows, tris, DEV)[0][0].cpu().tolist()))


def whole_stage(args, emit, part, shape, slam, run, key, extra):
    ms_ = {False: [], True: []}
    for on in (False, True, False, True):      # one untimed pass of each side first
        run(on)
    for _ in range(args.repeats):
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run(on)
            torch.cuda.synchronize()
            ms_[on].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms_.items()}
    emit(dict(part=part, shape=shape, frames=args.frames, repeats=args.repeats, key=key, ms_off=dict(median=round(med[False], 3), min=round(min(ms_[False]), 3), max=round(max(ms_[False]), 3)),
              ms_on=dict(median=round(med[True], 3), min=round(min(ms_[True]), 3), max=round(max(ms_[True]), 3)), ms_added=round(med[True] - med[False], 3), **extra(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--untimed", type=int, default=20)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--density", type=float, default=10000.0, help="surface samples per m^2 (the `geometry` block's default)")
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

    fan_part(args, emit)
    with tempfile.TemporaryDirectory() as tmp:
        for H, W in mesh_ab.SHAPES:
            shape = f"{W}x{H}"
            slam, seq = mesh_ab.start(args, H, W, tmp)
            for i in range(args.frames):      # the evaluation's `reference: sensor` places the frames at their ground-truth poses
                slam.gt_pose_list[i] = seq[i][2].clone()
            origin, voxel, trunc, box = mesh_ab.lattice(slam, 1, "sensor")
            with torch.no_grad():
                ref = sensor_mesh(slam, voxel, box)
            est = (moved(ref[0], 0.005), ref[1])
            kernel_parts(args, emit, shape, est, ref)
            pad = 5.0 * voxel
            mesh_block = dict(slam.cfg.get("mesh") or {}, bounds=[float(v) for v in np.concatenate([box[:3] - pad, box[3:] + pad])], voxel=voxel, every=1, source="sensor")

            def evaluate(on):
                slam.cfg["mesh"] = dict(mesh_block)
                slam.cfg["geometry"] = dict(slam.cfg.get("geometry") or {}, eval=False, estimate="mesh", reference="sensor", density=args.density, normals=on)
                return slam.evaluate_geometry(path=os.path.join(tmp, "geometry"))

            def export(on):
                slam.cfg["mesh"] = dict(mesh_block, normals=on)
                return slam.export_mesh(path=os.path.join(tmp, "mesh"))

            whole_stage(args, emit, "e", shape, slam, evaluate, "geometry.normals",
                        lambda out: dict(points=[out["n_estimate"], out["n_reference"]], normals=out["normals"], chamfer=out["chamfer"]))
            whole_stage(args, emit, "f", shape, slam, export, "mesh.normals",
                        lambda out: dict(vertices=out["counters"]["vertices"], triangles=out["counters"]["triangles"], normals=out["normals"], mesh_bytes=os.path.getsize(out["mesh"])))
            del slam, seq
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
