#!/usr/bin/env python
"""sha256 of every output the kernels outside the tracking and mapping loops write (compact, align, eval, pointcloud, tsdf, geometry, cull, mesh depth),
over the case lists the GPU tests define, as one JSON file -- to compare two builds of the library bit for bit:

    MM3DGS_LIB=$PWD/mm3dgs_slam_amd/csrc/variants/libmm3dgs_hip_parent.so python tools/offloop_digest.py parent.json
    python tools/offloop_digest.py new.json          # each in a fresh process; then compare the two files

The drivers are the tests' own (tests/test_gpu_*.py: caller-owned buffers between guard words, the statement's checks included), so a
digest exists only for a call the tests accept.  The one output whose order the kernels leave to atomics, the within-cell order of
mm3dgs_nn_grid_build's records, is sorted by row index inside each cell before it is hashed, as test_gpu_geometry.py compares it."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

DEV = "cuda:0"
OUT = {}


def put(key, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a if isinstance(a, bytes) else np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a).tobytes())
    assert key not in OUT, key
    OUT[key] = h.hexdigest()


def surgery():
    import ctypes as C
    from tests import surgery_cases as cases, surgery_ref as ref, test_gpu_surgery as t
    lib, th = t._lib(), (cases.MIN_OPACITY, cases.MAX_SCALE, cases.MAX_SCREEN)
    for n in cases.SIZES:
        for use_radii in (True, False):
            opacity, scales, radii, placed = cases.prune_rows(n)
            r = radii if use_radii else None
            ref.move_prune_rows(opacity, scales, r, ref.prune_keep(opacity, scales, r, *th)[1], placed, *th)
            src = [t.Source(opacity), t.Source(scales), t.Source(radii)]
            k, counter = t.Guarded(n, 0xCD), t.Guarded(4, np.array([1000], np.uint32))
            assert t._prune_call(n, src[0], src[1], src[2] if use_radii else None, k, counter) == 0
            t._sync()
            put(f"prune {n} radii {use_radii}", k.read(np.uint8), counter.read(np.uint32))
        for pattern in cases.KEEP_PATTERNS:
            widths = (1, 3, 0, 4) if n >= cases.LARGE else (1, 3, 0, 4, 45)
            arrays = [a if a.shape[1] else None for a in cases.row_arrays(n, widths)]
            out, total = t._compact(n, cases.keep_bytes(n, pattern), arrays, 0xCD)      # (the plan's words are checked exactly in there)
            put(f"compact {n} {pattern}", np.uint32(total), *out)
    for H, W in cases.SEED_SHAPES:
        for row0, n_rest in ((0, 0), (5, 15)):
            c = cases.seed_case(H, W)
            src = {k: t.Source(c[k]) for k in ("color", "depth", "keep", "pose")}
            work, n = t._checked_plan(H * W, src["keep"], c["keep"])
            out, so = {}, t.lib_mod().Mm3dgsSeedOutputs()
            for name, w in dict(t.SEED_WIDTHS, f_rest=3 * n_rest).items():
                out[name] = t.Guarded((row0 + n) * w * 4, 0xCD)
                setattr(so, name, out[name].ptr)
            assert lib.mm3dgs_seed_gaussians(H, W, t._ptr(src["color"]), t._ptr(src["depth"]), t._ptr(src["keep"]), t._ptr(work), t._ptr(src["pose"]), c["fx"],
                                             c["fy"], c["cx"], c["cy"], row0, C.byref(so), n_rest, t._stream()) == 0
            t._sync()
            put(f"seed {H}x{W} row0 {row0} n_rest {n_rest}", *[g.read(np.uint8) for g in out.values()])
    for P, mix, N in cases.DENSIFY_RUNS:
        run = cases.densify_run(P, mix)
        arrays, grad_accum, denom, placed = cases.densify_rows(P, mix, n_rest=run["n_rest"])
        cls, _ = t._settled_classes(P, grad_accum, denom, arrays["scaling"], placed)
        moments = cases.densify_moments(arrays, [k for k in run["moment_groups"] if arrays[k].shape[1]])
        got = t._densify(P, arrays, moments, grad_accum, denom, cls, N, run["with_parent"], 0xCD)[0]      # (class bytes and plan words checked in there)
        put(f"densify {P} {mix} N {N}", *[got[k] for k in sorted(got)])
    for H, W in cases.COVIS_SHAPES:
        for view in cases.COVIS_VIEWS:
            for plain in (False, True):
                c = cases.covis_case(H, W, view, plain=plain)
                a = [c[k] for k in ("depth", "sil", "kf_pose", "cur_pose", "fx", "fy", "cx", "cy")]
                ref.move_covisibility_pixels(c["sil"], ref.covisibility(*a)[1], c["placed"])
                src, counts = [t.Source(c[k]) for k in ("depth", "sil", "kf_pose", "cur_pose")], t.Guarded(8, 0xCD)
                assert t._covis_call(H, W, *src, c, counts) == 0
                t._sync()
                put(f"covisibility {H}x{W} {view} plain {plain}", counts.read(np.uint32))


def pointcloud():
    from tests import pointcloud_cases as cases, test_gpu_pointcloud as t

    def run(key, H, W, views, voxel=0.0):
        cloud = t.Cloud(H, W, len(views) * H * W, voxel=voxel, work_fill=0xFF)
        for v in views:
            cloud.add(t.to_dev(v))
        put(key, *cloud.read())

    for H, W in cases.SHAPES:
        for pattern in cases.PATTERNS:
            run(f"cloud {H}x{W} {pattern}", H, W, [cases.view(H, W, pattern)])
    for H, W in ((17, 33), (520, 520)):
        v = cases.plane_view(H, W)
        for voxel in (1000.0, 2.0 ** -16, 3.3 * cases.footprint(v)):
            run(f"cloud thinned {H}x{W} voxel {voxel:.6g}", H, W, [v], voxel)
    for H, W in ((17, 33), (48, 64)):
        vs = t._stream_views(H, W)
        run(f"cloud stream {H}x{W}", H, W, vs, 3.3 * cases.footprint(vs[0]))


def mesh():
    from tests import mesh_cases as cases, test_gpu_mesh as t
    for dims, hw, pattern, n_views in t.INTEGRATE_CASES:
        case = cases.integrate_case(dims, hw[0], hw[1], pattern, n_views)
        vol = t.Volume(dims)
        for v in case["views"]:
            assert vol.integrate(t.to_dev(v), case) == 0
        put(f"integrate {dims} {hw} {pattern} x{n_views}", *vol.read())
    for dims in cases.MESH_SHAPES:
        for kind in cases.KINDS:
            vol = cases.analytic_volume(kind, dims)
            dv = t.Volume(dims, vol["tsdf_w"], vol["rgb_w"])
            m = t.Mesher(dv, vol["origin"], vol["voxel"], 0, 0)
            assert m.plan() == 0
            V, T = (int(x) for x in m.counters.cpu()[:2])
            m = t.Mesher(dv, vol["origin"], vol["voxel"], V, T, work_fill=0xFF)
            assert m.plan() == 0 and m.emit() == 0
            rows, tris, c = m.read()
            put(f"mesh {dims} {kind}", rows[:V], tris[:T], c)


def mesh_sparse():
    from tests import mesh_sparse_cases as sc, test_gpu_mesh_sparse as t
    from mm3dgs_slam_amd import mesh as ms

    def frozen(key, blk):
        put(f"blocks {key} keys", blk.keys.cpu()[:blk.n], blk.neighbours())

    def extract(key, blk, anchor, voxel):
        m = t.BlockMesher(blk, anchor, voxel, 0, 0)
        assert m.plan() == 0
        V, T = (int(x) for x in m.counters.cpu()[:2])
        m = t.BlockMesher(blk, anchor, voxel, V, T, work_fill=0xFF)
        assert m.plan() == 0 and m.emit() == 0
        rows, tris, c = m.read()
        put(f"blocks {key} mesh", rows[:V], tris[:T], c)

    wall = t._against_dense(sc.sphere_case(0.03, True))      # reserved, frozen and integrated, as the tests' `wall` fixture
    frozen("wall", wall["blk"])
    put("blocks wall pool", *wall["blk"].pool())
    extract("wall", wall["blk"], wall["case"]["anchor"], wall["case"]["voxel"])
    base = sc.scattered_case((17, 33), "all", 3)             # the anchor in the scene's middle, as the tests' `astride` fixture
    b0 = ms.key_blocks(sc.reserve_all(base)[0])
    case = dict(base, anchor=base["voxel"] * 8.0 * 0.5 * (b0.min(0) + b0.max(0) + 1) + np.array([0.0031, -0.0042, 0.0057]))
    blk, views = t.Blocks(case, 512), [t.to_dev(v) for v in case["views"]]
    for v in views:
        assert blk.reserve(v) == 0
    blk.freeze()
    for v in views:
        assert blk.integrate(v) == 0
    frozen("negative", blk)
    put("blocks negative pool", *blk.pool())
    extract("negative", blk, case["anchor"], case["voxel"])
    for name in ("one block", "2 x 2 x 2", "sphere", "torus", "sphere minus a third", "torus minus a third"):
        a = t._analytic(name)
        extract(name, t.GivenBlocks(a["keys"], *sc.to_pool(a["tsdf_w"], a["rgb_w"], a["blocks"], a["first"], a["dims"])), a["origin"], a["voxel"])


def cull():
    from tests import cull_cases as cases, test_gpu_cull as t
    scenes = [cases.random_scene(n, H=H, W=W, n_views=3, seed=n + 3) for n in cases.SIZES for H, W in ((12, 16), (48, 64))] + cases.analytic_scenes()
    scenes += [cases.frustum_only(s) for s in scenes] + cases.shape_scenes()      # (as the tests run them)
    for k, scene in enumerate(scenes):
        snap = t.Cull(scene, fill=0xFF).run().snapshot()
        put(f"cull {k} {scene['name']} {scene['H']}x{scene['W']}", *[snap[name] for name in sorted(snap)])


def mesh_depth():
    from tests import mesh_depth_cases as cases, test_gpu_mesh_depth as t
    for k, scene in enumerate(cases.host_scenes() + [cases.random_scene(48, seed=7, **cases.WIDE)]):
        r = t.Render(scene, fill=0xFF)
        assert r.call() == 0
        put(f"mesh depth {k} {scene['name']}", *r.read())      # (not the work buffer: the order inside a tile's list is the atomics')


def geometry():
    from mm3dgs_slam_amd import geometry as geo
    from tests import geometry_cases as cases, normals_cases as nc, test_gpu_geometry as t, test_gpu_normals as tn

    def nn(key, case):
        g = t.NN(case, 0xFF)
        assert g.build() == 0 and g.query() == 0
        dist, row, counters, cell_start, srt = g.read()
        cell = np.searchsorted(cell_start, np.arange(len(srt)), "right")      # the within-cell order is the atomics': by row index instead
        put(key, dist, row, counters, cell_start, srt[np.lexsort((srt[:, 3], cell))])
        rc, *out = tn._query_index(g)
        assert rc == 0
        put(key + " index", *out)

    for n_ref in cases.SIZES:
        for n_q in cases.SIZES:
            nn(f"nn sized {n_ref} x {n_q}", cases.sized_case(n_ref, n_q))
    for name, case in cases.nn_cases().items():
        nn(f"nn {name}", case)

    def sample(key, v, tris, density, seed):
        s = t.Sampler(v, tris, density, seed, 0)
        assert s.plan() == 0
        s = t.Sampler(v, tris, density, seed, int(s.counters.cpu()[0]), 0xFF)
        assert s.plan() == 0 and s.emit() == 0
        put(key, *s.read())
        rc, rows, tri = tn._emit_tri(s)
        assert rc == 0
        put(key + " tri", rows, tri, s.counters)

    def consistency(key, est, ref, density, max_dist=0.2):      # one direction on host-made inputs, as test_gpu_normals._direction
        fe, (rows_r, _, fr) = geo.sample_mesh_host(*est, density, 0, full=True), geo.sample_mesh_host(*ref, density, 0, full=True)
        index = geo.nn_index_host(fe[0], rows_r, 0.05, max_dist)[1]
        put(key, *tn._consistency(fe[2]["tri"], index, fr["tri"], est, ref))

    sphere, flat = nc.icosphere(2), cases.square_mesh()
    consistency("normals sphere on itself", sphere, sphere, 2000.0)
    consistency("normals flat, flipped winding", flat, nc.flipped(flat), 2000.0)
    consistency("normals floor / wall", *nc.floor_and_wall(), 500.0, max_dist=0.25)
    consistency("normals sphere shifted by 1 cm", sphere, nc.shifted(sphere, (0.01, 0, 0)), 2000.0)
    mesh, rng = nc.rejecting_mesh(), np.random.default_rng(5)      # ids out of range, as test_consistency_ids_out_of_range
    m = len(mesh[1])
    tri_q = rng.choice(np.array([0, 7, 1, 5, m, m + 1, 0x7fffffff, 0xfffffffe], dtype=np.uint32), 700)
    index = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 1 << 20, 0xfffffffe, 0xffffffff], dtype=np.uint32), 700)
    put("normals ids out of range", *tn._consistency(tri_q, index, np.array([0, 7, 6, m + 3, 0xffffffff, 7, 0], dtype=np.uint32), mesh, mesh))

    for m in (1, 255, 256, 257):
        sample(f"sampler random {m}", *cases.random_mesh(m, seed=m), 150.0, m)
    sample("sampler 262400 tiny triangles", *cases.tiny_mesh(), 1e4, 4)
    for where in ("first", "last"):
        sample(f"sampler wall {where}", *cases.wall_mesh(where), 100.0, 6)
    sample("sampler degenerate", *cases.degenerate_mesh()[:2], 100.0, 2)


def error_texts():
    """Return code and mm3dgs_last_error() text of single-fault calls of the six entry points that take a posed view and of the nn_query /
    mesh_sample_emit pairs.  Host checks only: every call is rejected before a pointer is looked at, so the pointers are made-up addresses."""
    import ctypes as C
    from mm3dgs_slam_amd import _lib
    lib, nan, inf, A = _lib.load(), float("nan"), float("inf"), 0x10000      # A: 16-byte aligned, never dereferenced
    vec3, org3 = (C.c_double * 3)(0.0, 0.0, 0.0), (C.c_int64 * 3)(0, 0, 0)

    def run(stem, call, good, faults):
        for what, over in faults.items():
            rc = call(dict(good, **over))
            put(f"error text {stem} {what}", str(rc).encode(), lib.mm3dgs_last_error())

    view = dict(H=12, W=16, fx=20.0, fy=21.0, cx=8.0, cy=6.0, pose=A)
    view_faults = {"H = 0": dict(H=0), "W < 0": dict(W=-3), "2^28": dict(H=1 << 14, W=(1 << 14) + 1), "fx NaN": dict(fx=nan), "fx = 0": dict(fx=0.0), "fy = 0": dict(fy=0.0),
                   "fy inf": dict(fy=inf), "cx NaN": dict(cx=nan), "cy inf": dict(cy=inf), "NULL pose": dict(pose=None), "misaligned pose": dict(pose=A + 2)}
    head = lambda a: (a["H"], a["W"], a["fx"], a["fy"], a["cx"], a["cy"], a["pose"])
    run("pointcloud_add_view", lambda a: lib.mm3dgs_pointcloud_add_view(*head(a), A, A, A, 0.5, 0.0, 0.0, 0, A, 100, None, 0, A, A, None), view, view_faults)
    run("tsdf_integrate", lambda a: lib.mm3dgs_tsdf_integrate(*head(a), A, A, A, 0.5, 0.0, vec3, 0.1, 0.3, 8, 8, 8, A, A, A, None), view, view_faults)
    run("tsdf_blocks_reserve", lambda a: lib.mm3dgs_tsdf_blocks_reserve(*head(a), A, A, 0.5, 0.0, vec3, 0.1, 0.3, None, A, 64, A, None), view, view_faults)
    run("tsdf_blocks_integrate", lambda a: lib.mm3dgs_tsdf_blocks_integrate(*head(a), A, A, A, 0.5, 0.0, vec3, 0.1, 0.3, A, 4, A, A, A, None), view, view_faults)
    run("cull_mark_view", lambda a: lib.mm3dgs_cull_mark_view(*head(a), A, 0.0, 0.1, 10.0, 0.01, 100, A, A, A, None), view, view_faults)
    run("mesh_depth_render", lambda a: lib.mm3dgs_mesh_depth_render(*head(a), 0.1, 10.0, 10, A, 10, A, 100, A, A, A, A, None), view, view_faults)

    nnq = dict(n_q=10, q=A, n_ref=10, cell=0.1, origin=org3, gx=4, gy=4, gz=4, cell_start=A, sorted=A, max_dist=0.5, threshold=0.1, dist=A, index=A, row=A, work=A)
    nnq_faults = {"n_q = 0": dict(n_q=0), "n_q > 2^30": dict(n_q=(1 << 30) + 1), "n_ref = 0": dict(n_ref=0), "gz = 0": dict(gz=0), "2^26 cells": dict(gx=512, gy=512, gz=257),
                  "cell NaN": dict(cell=nan), "max_dist = 0": dict(max_dist=0.0), "max_dist inf": dict(max_dist=inf), "2^20 rings": dict(cell=1e-9), "threshold < 0": dict(threshold=-0.5),
                  "NULL origin": dict(origin=None), "NULL q": dict(q=None), "NULL cell_start": dict(cell_start=None), "NULL sorted": dict(sorted=None), "NULL dist": dict(dist=None),
                  "NULL row": dict(row=None), "NULL work": dict(work=None), "misaligned q": dict(q=A + 8), "misaligned work": dict(work=A + 4), "misaligned dist": dict(dist=A + 2),
                  "misaligned cell_start": dict(cell_start=A + 1), "misaligned row": dict(row=A + 4)}
    pre = lambda a: (a["n_q"], a["q"], a["n_ref"], a["cell"], a["origin"], a["gx"], a["gy"], a["gz"], a["cell_start"], a["sorted"], a["max_dist"], a["threshold"], a["dist"])
    run("nn_query", lambda a: lib.mm3dgs_nn_query(*pre(a), a["row"], a["work"], None), nnq, nnq_faults)
    run("nn_query_index", lambda a: lib.mm3dgs_nn_query_index(*pre(a), a["index"], a["row"], a["work"], None), nnq,
        dict(nnq_faults, **{"NULL index": dict(index=None), "misaligned index": dict(index=A + 2)}))

    ms = dict(nv=10, v=A, m=10, tris=A, density=100.0, seed=1, work=A, rows=A, tri=A, cap=100, counters=A)
    ms_faults = {"m = 0": dict(m=0), "m > 2^30": dict(m=(1 << 30) + 1), "n_vertices = 0": dict(nv=0), "density = 0": dict(density=0.0), "density NaN": dict(density=nan),
                 "NULL vrows": dict(v=None), "NULL triangles": dict(tris=None), "NULL work": dict(work=None), "NULL counters": dict(counters=None), "NULL rows": dict(rows=None),
                 "cap > 2^31": dict(cap=(1 << 31) + 1), "misaligned rows": dict(rows=A + 8), "misaligned vrows": dict(v=A + 8), "misaligned work": dict(work=A + 4),
                 "misaligned triangles": dict(tris=A + 2)}
    pre_ms = lambda a: (a["nv"], a["v"], a["m"], a["tris"], a["density"], a["seed"], a["work"], a["rows"])
    run("mesh_sample_emit", lambda a: lib.mm3dgs_mesh_sample_emit(*pre_ms(a), a["cap"], a["counters"], None), ms, ms_faults)
    run("mesh_sample_emit_tri", lambda a: lib.mm3dgs_mesh_sample_emit_tri(*pre_ms(a), a["tri"], a["cap"], a["counters"], None), ms,
        dict(ms_faults, **{"NULL tri_out": dict(tri=None), "misaligned tri_out": dict(tri=A + 2)}))


def evaluation():
    from tests import eval_cases as ec, test_gpu_eval as t
    for case in ec.CASES:
        put("eval %s %dx%d" % case, t.score(*(x.to(DEV) for x in ec.inputs(*case)), fill=float("nan")))


def depth_align():
    from tests import depth_align_ref as R, test_gpu_depth_align as t
    for shape in R.SHAPES:
        est, depth, sil = R.make_inputs(*shape)
        put("align %dx%d" % shape, *t._run(est, depth, sil, planes=shape in R.ODD_SHAPES))
    est, depth, _ = R.make_inputs(17, 23)
    put("align 17x23 without a silhouette", *t._run(est, depth, None))


def pose_prediction():
    from mm3dgs_slam_amd.tracker import Tracker
    from tests import imu_cases, test_gpu_imu_predict as t
    cs = imu_cases.random_cases()
    for k, c in enumerate(cs):
        put(f"imu case {k}", t._kernel(c["p1"], c["p2"], c["imu6"], c["c2i"], c["dt_cam"], c["dt_imu"]))
        put(f"const vel case {k}", Tracker._predict_const_vel_device(t._dev(c["p1"]), t._dev(c["p2"])))
    for k, c in enumerate(cs[:8]):
        put(f"imu n = 0, case {k}", t._kernel(c["p1"], c["p2"], np.zeros((0, 6)), c["c2i"], c["dt_cam"], c["dt_imu"]))
        put(f"imu pose_m2 == pose_m1, case {k}", t._kernel(c["p1"], c["p1"], c["imu6"], c["c2i"], 1.0, c["dt_imu"]))
        put(f"imu identity c2i, case {k}", t._kernel(c["p1"], c["p2"], c["imu6"], np.eye(4), c["dt_cam"], c["dt_imu"]))


def main():
    from mm3dgs_slam_amd import _lib
    for stage in (surgery, pointcloud, mesh, mesh_sparse, geometry, cull, mesh_depth, error_texts, evaluation, depth_align, pose_prediction):
        t0 = time.time()
        before = len(OUT)
        stage()
        torch.cuda.synchronize()
        print(f"{stage.__name__}: {len(OUT) - before} digests, {time.time() - t0:.1f} s", flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(OUT, f, indent=0, sort_keys=True)
    print(f"{len(OUT)} digests of {_lib.LIB_PATH} -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
