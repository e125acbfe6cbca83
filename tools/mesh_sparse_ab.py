#!/usr/bin/env python
"""A/B of the mesh export's two volumes (`mesh.volume: sparse` against `dense`) on the views of tools/mesh_ab.py: 640x480 and 1200x680, the
default 150 k-Gaussian synthetic scene after frame 0, the box of the 30 views at 256 samples along its longest side (the dense side: a
256^3 lattice, the dense kernels as they are), sources `render` and `sensor`.  Needs the GPU; there is no fall-back.

    python tools/mesh_sparse_ab.py [--calls 200] [--untimed 20] [--frames 30] [--repeats 3] [--out profiles/r20_mesh_sparse.jsonl]

Every timing is taken between two device events around one call, the two sides alternating in the same process: median, p10 and p90 of
`--calls` calls after `--untimed` calls of each side.

(a) reserve, one view (mm3dgs_tsdf_blocks_reserve): into a table that already holds the view's blocks (every claim ends at its first load:
    what the views of an export mostly are after the first few) and into a freshly reset table (every block is claimed by atomicCAS; the
    reset is outside the events).
(b) integrate, one view: SparseTsdfVolume.add over the blocks of all `--frames` views against TsdfVolume.add over 256^3, the same view.
(c) plan + emit after every view went in: mm3dgs_tsdf_blocks_mesh_plan / _emit against mm3dgs_tsdf_mesh_plan / _emit; and whether the two
    meshes have the same numbers of vertices and triangles.
(d) memory: blocks, pool bytes (12 KiB per block), table bytes, keys and neighbour bytes, against 24 bytes x 256^3.
(e) a whole SLAM.export_mesh over `--frames` views (`every: 1`, no bounds given: two passes over the views on both sides -- bounds and
    integrate, or reserve and integrate), `--repeats` times after one untimed pass, the two volumes alternating; host clock, device
    synchronised at both ends."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mesh_ab import DEV, SHAPES, SIDE, lattice, start, stat      # noqa: E402  (the same workload, lattice and statistics)


def timed(sides, calls, untimed, before=None):
    """{name: [us per call]} of the callables `sides`, alternating; `before(name)` runs outside the events."""
    us = {name: [] for name, _ in sides}
    for k in range(untimed + calls):
        for name, fn in sides:
            if before is not None:
                before(name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if k >= untimed:
                us[name].append(e0.elapsed_time(e1) * 1e3)
    return us


def one_config(slam, args, emit, H, W, source):
    from mm3dgs_slam_amd import _lib, export, mesh as ms
    from mm3dgs_slam_amd.rasterizer import _stream
    P, cam = _lib.ptr, slam.cfg["cam"]
    origin, voxel, trunc, box = lattice(slam, 1, source)
    tag = dict(shape=f"{W}x{H}", source=source, voxel=round(voxel, 6), frames=args.frames)
    with torch.no_grad():
        views = [tuple(None if t is None else t.detach().float().contiguous() for t in v) for v in export.views(slam, 1, source, "mesh")]
    view = views[min(5, len(views) - 1)]
    dims = (SIDE, SIDE, SIDE)
    sparse = ms.SparseTsdfVolume(voxel, trunc, H, W, cam, sil_min=0.99, max_blocks=1 << 18, device=DEV)
    lib = sparse.lib

    def reset():
        _lib.check(lib.mm3dgs_tsdf_blocks_reset(P(sparse.table), sparse.max_blocks, P(sparse.rc), _stream()))

    # (a)
    us = timed((("fresh", lambda: sparse.reserve(view[1], view[2], view[3])),), args.calls, args.untimed, before=lambda name: reset())
    one_view = sparse.rc.cpu().numpy().copy()
    us.update(timed((("held", lambda: sparse.reserve(view[1], view[2], view[3])),), args.calls, args.untimed))
    emit(dict(tag, part="a", calls=args.calls, untimed=args.untimed, reserve_fresh_us_per_view=stat(us["fresh"]), reserve_held_us_per_view=stat(us["held"]),
              valid_pixels=int(one_view[1]), pairs=int(one_view[2]), blocks_of_the_view=int(one_view[3]), pairs_per_valid_pixel=round(int(one_view[2]) / max(int(one_view[1]), 1), 2)))
    # the block set of all views
    reset()
    for v in views:
        sparse.reserve(v[1], v[2], v[3])
    n = sparse.freeze()
    rc = sparse.rc.cpu().numpy()
    dense = ms.TsdfVolume(dims, origin, voxel, trunc, H, W, cam, sil_min=0.99, device=DEV)
    # (b)
    us = timed((("sparse", lambda: sparse.add(*view)), ("dense", lambda: dense.add(*view))), args.calls, args.untimed)
    cs, cd, k = sparse.counters.cpu().numpy(), dense.counters.cpu().numpy(), args.calls + args.untimed
    emit(dict(tag, part="b", calls=args.calls, untimed=args.untimed, blocks=n, sparse_samples=n * 512, dense_samples=SIDE ** 3, sparse_us_per_view=stat(us["sparse"]),
              dense_us_per_view=stat(us["dense"]), dense_over_sparse_median=round(statistics.median(us["dense"]) / statistics.median(us["sparse"]), 3),
              sparse_faster=bool(statistics.median(us["sparse"]) < statistics.median(us["dense"])), sparse_updates_per_view=[int(cs[1]) // k, int(cs[2]) // k],
              dense_updates_per_view=[int(cd[1]) // k, int(cd[2]) // k]))
    # (c): fresh volumes with every view once
    sparse.tsdf_w.zero_(); sparse.rgb_w.zero_(); sparse.counters.zero_()
    dense = ms.TsdfVolume(dims, origin, voxel, trunc, H, W, cam, sil_min=0.99, device=DEV)
    for v in views:
        sparse.add(*v)
        dense.add(*v)
    srows, stris, sc_ = sparse.extract()
    drows, dtris, dc_ = dense.extract()
    swork = torch.empty(int(lib.mm3dgs_tsdf_blocks_mesh_work_bytes(n)) // 8, dtype=torch.int64, device=DEV)
    dwork = torch.empty(int(lib.mm3dgs_tsdf_mesh_work_bytes(*dims)) // 8, dtype=torch.int64, device=DEV)
    mc = torch.empty(8, dtype=torch.int64, device=DEV)
    srows, stris = torch.empty(max(sc_["vertices"], 1), 4, dtype=torch.int32, device=DEV), torch.empty(max(sc_["triangles"], 1), 3, dtype=torch.int32, device=DEV)
    drows, dtris = torch.empty(max(dc_["vertices"], 1), 4, dtype=torch.int32, device=DEV), torch.empty(max(dc_["triangles"], 1), 3, dtype=torch.int32, device=DEV)

    def sparse_mesh():
        _lib.check(lib.mm3dgs_tsdf_blocks_mesh_plan(n, P(sparse.neighbours), P(sparse.tsdf_w), 1.0, P(swork), P(mc), _stream()))
        _lib.check(lib.mm3dgs_tsdf_blocks_mesh_emit(n, P(sparse.keys), P(sparse.neighbours), P(sparse.tsdf_w), P(sparse.rgb_w), ms.double3(sparse.anchor), voxel, P(swork), P(srows),
                                                    sc_["vertices"], P(stris), sc_["triangles"], P(mc), _stream()))

    def dense_mesh():
        _lib.check(lib.mm3dgs_tsdf_mesh_plan(SIDE, SIDE, SIDE, P(dense.tsdf_w), 1.0, P(dwork), P(mc), _stream()))
        _lib.check(lib.mm3dgs_tsdf_mesh_emit(SIDE, SIDE, SIDE, P(dense.tsdf_w), P(dense.rgb_w), ms.double3(dense.origin), voxel, P(dwork), P(drows), dc_["vertices"], P(dtris),
                                             dc_["triangles"], P(mc), _stream()))

    us = timed((("sparse", sparse_mesh), ("dense", dense_mesh)), args.calls, args.untimed)
    emit(dict(tag, part="c", calls=args.calls, untimed=args.untimed, blocks=n, sparse_plan_plus_emit_us=stat(us["sparse"]), dense_plan_plus_emit_us=stat(us["dense"]),
              dense_over_sparse_median=round(statistics.median(us["dense"]) / statistics.median(us["sparse"]), 3), sparse_mesh=[sc_["vertices"], sc_["triangles"]],
              dense_mesh=[dc_["vertices"], dc_["triangles"]], same_counts=bool(sc_["vertices"] == dc_["vertices"] and sc_["triangles"] == dc_["triangles"]),
              sparse_updates=[sc_["dist_updates"], sc_["colour_updates"]], dense_updates=[dc_["dist_updates"], dc_["colour_updates"]]))
    # (d)
    emit(dict(tag, part="d", blocks=n, pairs=int(rc[2]), valid_pixels=int(rc[1]), out_of_range=int(rc[5]), pool_bytes=n * ms.BLOCK_BYTES, table_bytes=sparse.table_bytes,
              max_blocks=sparse.max_blocks, keys_and_neighbours_bytes=n * (8 + 27 * 4), mesh_work_bytes=int(swork.numel()) * 8, dense_volume_bytes=24 * SIDE ** 3,
              dense_mesh_work_bytes=int(dwork.numel()) * 8, bounding_lattice=sparse.dims, pool_over_dense=round(n * ms.BLOCK_BYTES / (24 * SIDE ** 3), 4)))
    del sparse, dense, swork, dwork, srows, stris, drows, dtris
    torch.cuda.empty_cache()
    # (e)
    def run(volume):
        slam.cfg["mesh"] = dict(slam.cfg.get("mesh") or {}, bounds=None, voxel=voxel, every=1, source=source, volume=volume)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = slam.export_mesh()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    ms_, outs = {"sparse": [], "dense": []}, {}
    for k in range(args.repeats + 1):
        for volume in ("sparse", "dense"):
            t, outs[volume] = run(volume)
            if k:
                ms_[volume].append(t)
    med = {v: statistics.median(ms_[v]) for v in ms_}
    emit(dict(tag, part="e", repeats=args.repeats, gaussians=int(slam.gaussians.get_xyz.shape[0]),
              sparse_ms_export=dict(median=round(med["sparse"], 3), min=round(min(ms_["sparse"]), 3), max=round(max(ms_["sparse"]), 3)),
              dense_ms_export=dict(median=round(med["dense"], 3), min=round(min(ms_["dense"]), 3), max=round(max(ms_["dense"]), 3)),
              dense_over_sparse_median=round(med["dense"] / med["sparse"], 3), sparse_lattice=list(outs["sparse"]["lattice"]), dense_lattice=list(outs["dense"]["lattice"]),
              sparse_counters=outs["sparse"]["counters"], dense_counters=outs["dense"]["counters"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--untimed", type=int, default=20)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
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

    with tempfile.TemporaryDirectory() as tmp:
        for H, W in SHAPES:
            slam, seq = start(args, H, W, tmp)
            for source in ("render", "sensor"):
                one_config(slam, args, emit, H, W, source)
            del slam, seq
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
