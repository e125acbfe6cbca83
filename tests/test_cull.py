"""The host statement of the visibility culling (mm3dgs_slam_amd/cull.py) against an independent per-point loop and against scenes whose
answer is known by construction; the bindings of the three exports; the reader of foreign PLY files; and a `device: cpu` run whose reference
is a file that covers more than the cameras saw.  Every test prints its figures (`CULLERR ...`, pytest -s) before it asserts."""
import ctypes as C
import json
import os
import random
import re

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import cull as cl, export as ex, geometry as geo, mesh as ms, pointcloud as pc
from tests import cull_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(scene, min_views=1, cap=None):
    return cl.cull_host(scene["rows"], scene["views"], min_views=min_views, cap=cap, **cases.options(scene))


def test_cull_host_equals_the_brute_force_loop():
    scenes = []
    for s in cases.analytic_scenes():
        scenes += [s, cases.frustum_only(s)]
    r = cases.random_scene(300, n_views=3, seed=1)
    scenes += [r, cases.frustum_only(r), cases.random_scene(257, H=48, W=64, n_views=1, seed=2)] + cases.shape_scenes()
    for s in scenes:
        for min_views in (1, 2):
            kept, index, seen, counters = _host(s, min_views)
            bseen, bindex, bcounters = cases.brute_force(s, min_views)
            print(f"CULLERR host {s['name']} ({'occlusion' if s['views'][0][0] is not None else 'frustum'}, min_views {min_views}): counters {counters.tolist()}, "
                  f"brute force {bcounters.tolist()}, {int((seen != bseen).sum())} of {len(seen)} seen counts differ")
            assert seen.dtype == np.uint32 and index.dtype == np.uint32 and np.array_equal(seen, bseen) and np.array_equal(index, bindex)
            assert np.array_equal(counters, bcounters) and kept.tobytes() == s["rows"][bindex.astype(np.int64)].tobytes()
    # the random scene straddles the frustum: neither everything nor nothing is seen, and occlusion removes some more
    _, _, seen_o, c_o = _host(r)
    _, _, seen_f, c_f = _host(cases.frustum_only(r))
    assert 0 < c_o[2] < c_f[2] < len(r["rows"]) - c_f[5] and c_f[5] > 0 and bool((seen_o <= seen_f).all())


def test_analytic_scenes():
    for s in cases.analytic_scenes():
        for mode, scene in (("occlusion", s), ("frustum", cases.frustum_only(s))):
            kept, index, seen, counters = _host(scene)
            want = s["want_" + mode]
            wrong = [f"{s['why'][i]}: seen {int(seen[i])}, want {int(want[i])}" for i in np.flatnonzero(seen.astype(bool) != want)]
            print(f"CULLERR analytic {s['name']} ({mode}): seen {seen.tolist()}, want {want.astype(int).tolist()}, counters {counters.tolist()}")
            assert not wrong, wrong
            fin = np.isfinite(pc.rows_xyz(s["rows"])).all(1)
            assert counters.tolist() == [1, int(want.sum()), int(want.sum()), int(want.sum()), 0, int((~fin).sum()), 0, 0]
            assert np.array_equal(index, np.flatnonzero(want)) and kept.tobytes() == s["rows"][want].tobytes()
    assert int((~np.isfinite(pc.rows_xyz(cases.exact_scene()["rows"])).all(1)).sum()) == 3      # NaN, +Inf, -Inf: each counted once


def test_order_index_and_min_views_over_three_views():
    # three identity-rotation views side by side along x: a point at x sees ... the views whose window holds it
    poses = [np.array([1, 0, 0, 0, tx, 0, 0], dtype=np.float32) for tx in (0.0, 4.0, 8.0)]      # p_c = p_w + t
    s = dict(H=12, W=16, fx=1.0, fy=1.0, cx=0.0, cy=0.0, near=0.0, far=0.0, eps=0.0, depth_max=0.0, views=[(None, p) for p in poses])
    x = np.array([20.0, 6.0, -3.0, 9.0, 2.0, -8.5, 14.0, np.nan, -1.0], dtype=np.float32)      # u = x + tx must lie in [-0.5, 15.5)
    want_seen = np.array([0, 3, 2, 2, 3, 1, 1, 0, 2], dtype=np.uint32)
    s["rows"] = cases.rows_of(np.stack([x, np.zeros_like(x), np.ones_like(x)], 1))
    for min_views, want_index in ((1, [1, 2, 3, 4, 5, 6, 8]), (2, [1, 2, 3, 4, 8]), (3, [1, 4])):
        kept, index, seen, counters = _host(s, min_views)
        print(f"CULLERR min_views {min_views}: seen {seen.tolist()}, index {index.tolist()}, counters {counters.tolist()}")
        assert np.array_equal(seen, want_seen) and index.tolist() == want_index and kept.tobytes() == s["rows"][want_index].tobytes()
        assert counters.tolist() == [3, int(want_seen.sum()), len(want_index), len(want_index), 0, 1, 0, 0]
    kept, index, _, counters = _host(s, 1, cap=3)
    assert index.tolist() == [1, 2, 3] and len(kept) == 3 and counters.tolist()[2:5] == [7, 3, 4]
    for bad in (dict(near=-1.0), dict(eps=-0.5), dict(far=float("nan")), dict(min_views=0), dict(fx=float("nan")), dict(H=0)):
        with pytest.raises(ValueError):
            cl.cull_host(s["rows"], s["views"], **dict(cases.options(s), **bad))
    with pytest.raises(ValueError, match="every view"):
        cl.cull_host(s["rows"], [(None, poses[0]), (np.ones((12, 16), dtype=np.float32), poses[1])], **cases.options(s))


def test_cabi_declares_and_binds_the_three_symbols():
    from mm3dgs_slam_amd import _lib
    h = open(os.path.join(ROOT, "include", "mm3dgs.h")).read()
    lib = _lib.load()
    for name in ("mm3dgs_cull_mark_view", "mm3dgs_cull_work_bytes", "mm3dgs_cull_select"):
        assert re.search(r"\b" + name + r"\s*\(", h) and name in _lib.exported_symbols() and hasattr(lib, name), name
    P = C.c_void_p
    assert lib.mm3dgs_cull_mark_view.argtypes == [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, P, P, C.c_float, C.c_double, C.c_double,
                                                  C.c_double, C.c_uint64, P, P, P, P]
    assert lib.mm3dgs_cull_select.argtypes == [C.c_uint64, P, P, C.c_uint32, P, C.c_uint64, P, P, P, P]
    assert lib.mm3dgs_cull_work_bytes.argtypes == [C.c_uint64] and lib.mm3dgs_cull_work_bytes.restype is C.c_size_t
    assert lib.mm3dgs_cull_mark_view.restype is C.c_int and lib.mm3dgs_cull_select.restype is C.c_int
    for n in (0, 1, 257, cases.SECOND_ROUND, 1 << 30):
        b = int(lib.mm3dgs_cull_work_bytes(n))
        assert b > 0 and b % 8 == 0 and b >= 8 * ((n + 255) // 256), (n, b)
    assert int(lib.mm3dgs_cull_work_bytes((1 << 30) + 1)) == 0
    # the header states the rule and the counters, and the version has not moved
    for text in ("z_c > z_near", "floor(fx x_c / z_c + cx + 0.5)", "(double)d + eps", "[4] dropped for lack of room", "[5] skipped rows"):
        assert text in h, text
    assert lib.mm3dgs_version() == 213 and re.search(r"#define MM3DGS_ABI_VERSION 213\b", h)
    # calls the entry points refuse before anything is launched (no device is touched)
    FAKE = 0x1000
    ok = dict(H=12, W=16, fx=1.0, fy=1.0, cx=0.0, cy=0.0, pose=FAKE, depth=None, depth_max=0.0, near=0.0, far=0.0, eps=0.0, n=10, rows=FAKE, seen=FAKE, counters=FAKE)
    nan = float("nan")
    for what, over in {"NULL rows": dict(rows=None), "H = 0": dict(H=0), "W < 0": dict(W=-1), "near < 0": dict(near=-0.5), "eps < 0": dict(eps=-1.0), "fx NaN": dict(fx=nan),
                       "cy NaN": dict(cy=nan), "fy = 0": dict(fy=0.0), "far NaN": dict(far=nan), "NULL pose": dict(pose=None), "NULL counters": dict(counters=None),
                       "n > 2^30": dict(n=(1 << 30) + 1), "misaligned rows": dict(rows=FAKE + 8)}.items():
        a = dict(ok, **over)
        rc = lib.mm3dgs_cull_mark_view(a["H"], a["W"], a["fx"], a["fy"], a["cx"], a["cy"], a["pose"], a["depth"], a["depth_max"], a["near"], a["far"], a["eps"], a["n"],
                                       a["rows"], a["seen"], a["counters"], None)
        assert rc == -1 and lib.mm3dgs_last_error(), what
    for what, args in {"min_views = 0": (10, FAKE, FAKE, 0, FAKE, 10, None, FAKE, FAKE), "NULL work": (10, FAKE, FAKE, 1, FAKE, 10, None, None, FAKE),
                       "NULL seen": (10, FAKE, None, 1, FAKE, 10, None, FAKE, FAKE), "NULL out_rows": (10, FAKE, FAKE, 1, None, 10, None, FAKE, FAKE),
                       "cap > 2^31": (10, FAKE, FAKE, 1, FAKE, (1 << 31) + 1, None, FAKE, FAKE)}.items():
        assert lib.mm3dgs_cull_select(*args, None) == -1 and lib.mm3dgs_last_error(), what


def test_config_keys_and_their_validation():
    from mm3dgs_slam_amd.config import GEOMETRY_CULL, default_config
    assert GEOMETRY_CULL == {"cull": "none", "cull_eps": 0, "cull_near": 0, "cull_far": 0, "cull_min_views": 1}
    cfg = default_config(device="cpu")
    opt = ex.options(cfg, "geometry")
    assert opt["cull"] == "none" and opt["cull_eps"] == 0.05 and opt["cull_near"] == 0 and opt["cull_far"] == 0 and opt["cull_min_views"] == 1      # eps 0: the threshold
    cfg["geometry"].update(cull="Occlusion", cull_eps=0.02, threshold=0.1)
    assert ex.options(cfg, "geometry")["cull"] == "occlusion" and ex.options(cfg, "geometry")["cull_eps"] == 0.02
    for bad, match in ((dict(cull="visible"), "none / frustum / occlusion"), (dict(cull_eps=-1), "cull_eps"), (dict(cull_near=float("nan")), "cull_near"),
                       (dict(cull_min_views=0), "cull_min_views"), (dict(cull_far=-2), "cull_far")):
        with pytest.raises(ValueError, match=match):
            ex.options(dict(cfg, geometry=dict(cfg["geometry"], **bad)), "geometry")


def test_kernel_order_sum_is_the_stated_tree():
    """geometry.kernel_order_sum against a scalar walk of the stated order (a balanced tree per 256, lane t over the blocks t, t + 256, ...,
    then the lanes in order), and direction_row's default untouched by the option."""
    import math
    rng = np.random.default_rng(3)
    for n in (0, 1, 255, 256, 257, 1000, 256 * 257 + 3):
        v = rng.uniform(0, 1, n)

        def tree(a):
            return a[0] if len(a) == 1 else tree(a[:len(a) // 2]) + tree(a[len(a) // 2:])
        blocks = [tree(np.concatenate([v[b:b + 256], np.zeros(256 - len(v[b:b + 256]))])) for b in range(0, max(n, 1), 256)]
        lanes = [0.0] * 256
        for b, s in enumerate(blocks):
            lanes[b % 256] = lanes[b % 256] + s
        want = 0.0
        for s in lanes:
            want = want + s
        got = geo.kernel_order_sum(v)
        print(f"CULLERR kernel order sum, n = {n}: {got!r} (scalar walk {want!r}, exact {math.fsum(v)!r})")
        assert got == want and abs(got - math.fsum(v)) <= 1e-12 * max(n, 1)
    d = rng.uniform(0, 0.5, 700).astype(np.float32)
    d[::50] = np.nan
    a, b = geo.direction_row(d, np.zeros(700, dtype=bool), 0.05), geo.direction_row(d, np.zeros(700, dtype=bool), 0.05, "kernel")
    assert np.array_equal(a[[0, 3, 4, 5, 6, 7]], b[[0, 3, 4, 5, 6, 7]]) and np.allclose(a[1:3], b[1:3], rtol=1e-13, atol=0)
    dd = d[~np.isnan(d)].astype(np.float64)
    assert a[1] == dd.sum() / len(dd) and a[2] == np.sqrt((dd * dd).sum() / len(dd))


# ---- foreign PLY files ------------------------------------------------------------------------------------------------------------------
def _write_foreign(path, xyz, normals, rgb, faces, index_type="uint"):
    """A mesh as a dataset ships it: float x y z nx ny nz, uchar red green blue (no alpha), list uchar <index_type> vertex_indices."""
    vt = np.dtype([("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
    v = np.zeros(len(xyz), dtype=vt)
    v["xyz"], v["n"], v["rgb"] = xyz, normals, rgb
    header = ("ply\nformat binary_little_endian 1.0\ncomment written by a test\n" + f"element vertex {len(xyz)}\n"
              "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n" + f"element face {len(faces)}\nproperty list uchar {index_type} vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(v.tobytes())
        for f in faces:
            fh.write(bytes([len(f)]) + np.asarray(f, dtype="<u4").tobytes())
    return path


def test_read_foreign_ply(tmp_path):
    rng = np.random.default_rng(0)
    xyz = rng.uniform(-1, 1, (6, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (6, 3)).astype(np.uint8)
    faces = [[0, 1, 2], [2, 3, 4, 5], [5, 0, 1]]      # a triangle, a quad, a triangle
    path = _write_foreign(str(tmp_path / "gt.ply"), xyz, rng.normal(size=(6, 3)).astype(np.float32), rgb, faces)
    with pytest.raises(ValueError, match="not a mesh of write_mesh_ply"):
        ms.read_mesh_ply(path)
    for reader in (ms.read_foreign_ply, ms.read_surface_ply):
        rows, tris = reader(path)
        print(f"CULLERR foreign ply ({reader.__name__}): {len(rows)} vertices, triangles {tris.tolist()}")
        assert rows.dtype == np.int32 and tris.dtype == np.int32 and np.array_equal(pc.rows_xyz(rows), xyz)
        assert np.array_equal(pc.rows_rgba(rows)[:, :3], rgb) and bool((pc.rows_rgba(rows)[:, 3] == 255).all())
        assert tris.tolist() == [[0, 1, 2], [2, 3, 4], [2, 4, 5], [5, 0, 1]]      # the quad fanned from its corner 0, in file order
    rows, tris = ms.read_foreign_ply(_write_foreign(str(tmp_path / "int.ply"), xyz, xyz, rgb, [[0, 1, 2], [3, 4, 5]], index_type="int"))
    assert tris.tolist() == [[0, 1, 2], [3, 4, 5]]
    # a cloud without colour: 255 everywhere
    with open(tmp_path / "cloud.ply", "wb") as fh:
        fh.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 6\nproperty float x\nproperty float y\nproperty float z\nproperty double quality\nend_header\n")
        v = np.zeros(6, dtype=[("xyz", "<f4", 3), ("q", "<f8")])
        v["xyz"] = xyz
        fh.write(v.tobytes())
    cloud = ms.read_surface_ply(str(tmp_path / "cloud.ply"))
    assert cloud.shape == (6, 4) and np.array_equal(pc.rows_xyz(cloud), xyz) and bool((cloud[:, 3] == -1).all())
    # this package's own files still go through the strict readers, and read_mesh_ply still refuses a cloud
    own = pc.write_ply(str(tmp_path / "own.ply"), rows)
    assert ms.read_surface_ply(own).tobytes() == rows.tobytes()
    with pytest.raises(ValueError, match="not a mesh of write_mesh_ply"):
        ms.read_mesh_ply(own)
    # rejected: ASCII, big-endian, double coordinates, an index beyond the vertices, a short body, another element
    ascii_ = tmp_path / "ascii.ply"
    ascii_.write_text("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n0 0 0\n")
    big = tmp_path / "big.ply"
    big.write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    dbl = tmp_path / "double.ply"
    dbl.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty double x\nproperty double y\nproperty double z\nend_header\n")
    beyond = _write_foreign(str(tmp_path / "beyond.ply"), xyz, xyz, rgb, [[0, 1, 6]])
    short = tmp_path / "short.ply"
    short.write_bytes(open(path, "rb").read()[:-5])
    edges = tmp_path / "edges.ply"
    edges.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nelement edge 0\nproperty int a\nend_header\n")
    for bad in (ascii_, big, dbl, beyond, short, edges):
        for reader in (ms.read_foreign_ply, ms.read_surface_ply):
            with pytest.raises(ValueError):
                reader(str(bad))


# ---- a device: cpu run against a reference file that covers more than the cameras saw ------------------------------------------------------
MESH = {"voxel": 0.08, "every": 1, "export": False}
GEO = {"density": 400.0, "threshold": 0.05, "max_dist": 1.0}


def _cpu_slam(tmp, frames=4):
    """The stand-in run of `device: cpu` of tests/test_geometry.py (32 x 48, the oracle rasterizer injected), 4 frames, run to its end."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.renderer import Renderer
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from oracle.raster_ref import RefRasterizer
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device="cpu", height=32, width=48, tracking={"iters": 2}, mapping={"iters": 3, "kf_every": 2}, outputdir=str(tmp), mesh=dict(MESH),
                         geometry=dict(GEO, eval=False))
    seq = SyntheticSequence(cfg, frames, 600, seed=2, renderer=Renderer(cfg, rasterizer_cls=RefRasterizer))
    slam = SLAM(cfg, seq, rasterizer_cls=RefRasterizer)
    slam.run()
    return slam, seq, cfg


def _wall_behind(poses):
    """Four corners and two triangles of a 6 m x 6 m wall 3 m behind the cameras' centroid, across their mean viewing direction."""
    Rt = [pc.pose_rotation(p) for p in poses]
    centres = np.stack([-R.T @ t for R, t in Rt])
    fwd = np.mean([R[2] for R, _ in Rt], 0)
    fwd /= np.linalg.norm(fwd)
    a = np.cross(fwd, [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(fwd, a)
    o = centres.mean(0) - 3.0 * fwd
    corners = np.stack([o + 3.0 * (sa * a + sb * b) for sa, sb in ((-1, -1), (1, -1), (1, 1), (-1, 1))]).astype(np.float32)
    for R, t in Rt:      # behind every view: z_c < 0 at the corners, so on the whole (convex) wall
        assert bool(((corners.astype(np.float64) @ R[2] + t[2]) < -1.0).all())
    return corners, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


def test_cpu_run_against_a_reference_file_with_an_unseen_wall(tmp_path):
    slam, seq, cfg = _cpu_slam(tmp_path / "run")
    block = ex.options(cfg, "mesh")
    gt = ex.gt_poses(slam)
    rows, tris = ex.mesh_geometry(slam, dict(block, source="sensor"), gt)[:2]      # the run's own `reference: sensor` mesh
    corners, wall = _wall_behind(gt)
    nv = len(rows)
    ref_rows = np.concatenate([rows, cases.rows_of(corners, rgba=-1)])
    ref_tris = np.concatenate([tris, wall + nv]).astype(np.int32)
    ref_file = ms.write_mesh_ply(str(tmp_path / "reference.ply"), ref_rows, ref_tris)
    n_before_wall = geo.sample_mesh_host(rows, tris, GEO["density"], 0)[1]["samples"]
    ref_samples = geo.sample_mesh_host(ref_rows, ref_tris, GEO["density"], 0)[0]
    assert ref_samples[:n_before_wall].tobytes() == geo.sample_mesh_host(rows, tris, GEO["density"], 0)[0].tobytes()      # appending keeps the earlier samples

    def evaluate(name, **keys):
        slam.cfg["geometry"] = dict(GEO, eval=False, reference=ref_file, **keys)
        out = slam.evaluate_geometry(path=str(tmp_path / name))
        return out, json.load(open(tmp_path / name / "metrics.json"))

    parent, m_parent = evaluate("parent")                       # the call as it was before the keys existed
    none, m_none = evaluate("none", cull="none", cull_eps=0, cull_near=0, cull_far=0, cull_min_views=1)
    for f in ("metrics.json", "accuracy.ply", "completion.ply"):
        assert (tmp_path / "none" / f).read_bytes() == (tmp_path / "parent" / f).read_bytes(), f
    assert "cull" not in m_none and "cull" not in none
    fr, m_fr = evaluate("frustum", cull="frustum")
    oc, m_oc = evaluate("occlusion", cull="occlusion")
    print(f"CULLERR cpu run: none n_reference {m_none['n_reference']} completion ratio {m_none['completion_ratio']}; frustum {m_fr['n_reference']} / "
          f"{m_fr['completion_ratio']}; occlusion {m_oc['n_reference']} / {m_oc['completion_ratio']}; wall samples {len(ref_samples) - n_before_wall}; "
          f"cull blocks {json.dumps(m_fr['cull'])} {json.dumps(m_oc['cull'])}")
    assert len(ref_samples) - n_before_wall > 1000 and m_none["n_reference"] == len(ref_samples)
    assert m_none["n_reference"] > m_fr["n_reference"] and m_none["completion_ratio"] < m_fr["completion_ratio"]
    # no kept reference point lies on the wall: the samples are ordered by triangle, the wall's come last
    assert fr["reference_index"].max() < n_before_wall and oc["reference_index"].max() < n_before_wall
    # the kept sets are cull_host of the sampled rows, for the views the stage built
    spec = ex.cull_views(slam, ex.options(slam.cfg, "geometry", ), block)
    assert spec["mode"] == "occlusion" and len(spec["views"]) == 4 and spec["eps"] == GEO["threshold"]
    fspec = dict(spec, views=[(None, p) for _, p in spec["views"]], mode="frustum")
    est_samples = geo.sample_mesh_host(*ex.mesh_geometry(slam, block)[:2], GEO["density"], 0)[0]
    for result, s in ((fr, fspec), (oc, spec)):
        for side, samples in (("estimate", est_samples), ("reference", ref_samples)):
            kept, index, counts = cl.apply_host(samples, s)
            assert result[side + "_rows"].tobytes() == kept.tobytes() and np.array_equal(result[side + "_index"], index), (s["mode"], side)
            assert result["cull"][side] == counts
    for m, mode in ((m_fr, "frustum"), (m_oc, "occlusion")):
        c = m["cull"]
        assert c["mode"] == mode and c["eps"] == 0.05 and c["near"] == 0 and c["far"] == 0 and c["min_views"] == 1 and c["views"] == 4
        assert c["reference"]["rows"] == len(ref_samples) and c["reference"]["kept"] == m["n_reference"] and c["reference"]["skipped"] == 0
        assert c["estimate"]["rows"] == len(est_samples) and c["estimate"]["kept"] == m["n_estimate"]
        assert m["reference_to_estimate"]["n"] == m["n_reference"] and len(pc.read_ply(str(tmp_path / mode / "completion.ply"))) == m["n_reference"]
    assert m_oc["n_reference"] <= m_fr["n_reference"] and m_oc["n_estimate"] <= m_fr["n_estimate"]
    # occlusion needs the frames' sensor depth, frustum reads no frame

    class NoDepth:
        def __len__(self):
            return len(seq)

        def __getitem__(self, i):
            if slam.cfg["geometry"]["cull"] == "frustum":
                raise AssertionError("cull: frustum read a frame")
            c, _, p = seq[i]
            return c, None, p
    slam.seq = NoDepth()
    with pytest.raises(ValueError, match="frame 0 has no sensor depth"):
        evaluate("x", cull="occlusion")
    slam.cfg["geometry"]["cull"] = "frustum"
    assert len(ex.cull_views(slam, ex.options(slam.cfg, "geometry"), block)["views"]) == 4
