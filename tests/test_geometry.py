"""The host statement of the geometry scores (mm3dgs_slam_amd/geometry.py): the ring search against float64 brute force, analytic
comparisons, the surface sampler's statistics, the bindings of the seven exports, and a `device: cpu` run that scores its own export.
Every test prints its figures (`GEOERR ...`, pytest -s) before it asserts."""
import ctypes as C
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import geometry as geo, mesh as ms, pointcloud as pc
from tests import geometry_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nn_cases():
    out = cases.nn_cases()
    for n_ref, n_q in ((1, 1), (255, 257), (256, 256), (257, 1000), (1000, 255)):
        c = cases.sized_case(n_ref, n_q)
        out[c["name"]] = c
    return out


def test_ring_search_equals_float64_brute_force(nn_cases):
    for name, c in nn_cases.items():
        d, info = geo.nn_distances_host(c["query"], c["ref"], c["cell"], c["max_dist"])
        b, cl, d64 = geo.nn_brute_host(c["query"], c["ref"], c["max_dist"])
        same = np.array_equal(d.view(np.int32), b.view(np.int32))
        print(f"GEOERR host {name}: {len(d)} queries, {int(info['clamped'].sum())} clamped, {int(np.isnan(d).sum())} skipped, grid {info['dims']}; "
              f"max |ring - brute| = {float(np.nanmax(np.abs(d.astype(np.float64) - b))) if np.isfinite(b).any() else 0.0}")
        assert same and np.array_equal(info["clamped"], cl), name
    # three (cell, max_dist) pairs on random float32 points, as the rule was first checked
    rng = np.random.default_rng(0)
    R, Q = cases.rows_of(rng.uniform(-1, 1, (1500, 3))), cases.rows_of(rng.uniform(-1.5, 1.5, (700, 3)))
    for cell, md in ((0.05, 0.3), (0.2, 1.0), (0.5, 0.25)):
        d, info = geo.nn_distances_host(Q, R, cell, md)
        b, cl, _ = geo.nn_brute_host(Q, R, md)
        print(f"GEOERR host random cell {cell} max_dist {md}: max difference {float(np.abs(d - b).max())}")
        assert np.array_equal(d, b) and np.array_equal(info["clamped"], cl)


def test_edge_case_counts_are_what_the_blocks_say(nn_cases):
    c = nn_cases["edges"]
    d, info = geo.nn_distances_host(c["query"], c["ref"], c["cell"], c["max_dist"])
    row = geo.direction_row(d, info["clamped"], c["threshold"])
    print(f"GEOERR edges: row {row.tolist()}, reference rows skipped {info['ref_skipped']}")
    assert info["ref_skipped"] == 3 and row[6] == 3 and row[0] == len(d) - 3
    q = pc.rows_xyz(c["query"]).astype(np.float64)
    at = lambda y: int(np.flatnonzero((q[:, 1] == y) & (q[:, 0] == 0) & (q[:, 2] == 0))[0])
    assert d[at(12.0)] == np.float32(0.5) and not info["clamped"][at(12.0)]          # exactly max_dist
    assert d[at(16.0)] == np.float32(0.5) and info["clamped"][at(16.0)]              # 2^-20 beyond: clamped to the same stored value
    assert d[at(20.0)] <= np.float32(0.125) < d[at(24.0)]                            # the threshold tie and 2^-22 beyond it
    assert (d == 0).sum() == 2
    t = cases.termination_case()
    assert geo.nn_distances_host(t["query"], t["ref"], t["cell"], t["max_dist"])[0].tolist() == [1.1875]


def _sampled(v, tris, density=1e4, seed=0):
    return geo.sample_mesh_host(v, tris, density, seed)[0]


def test_analytic_comparisons():
    delta, density = float(np.float32(0.03)), 1e4      # the rows are float32: the squares are float32(0.03) apart
    s = density ** -0.5
    a, b = cases.square_mesh(0.0), cases.square_mesh(delta)
    r = geo.compare_host(_sampled(*a, density=density, seed=1), b, threshold=0.05, max_dist=1.0, density=density, seed=0)      # (two seeds: the samples differ)
    lo, hi = delta * (1 - 2.0 ** -24), np.sqrt(delta ** 2 + 2 * s * s)      # a stored distance is rounded to float32 once
    print(f"GEOERR squares {delta} apart: accuracy {r['accuracy']}, completion {r['completion']} in [{lo}, {hi}]; table {r['table'].tolist()}")
    assert lo <= r["accuracy"] <= hi and lo <= r["completion"] <= hi and r["table"][0, 3] > delta
    assert r["precision"] == 1.0 and r["recall"] == 1.0 and r["completion_ratio"] == 1.0 and r["fscore"] == 1.0
    assert r["table"][0, 5] == 0 and r["table"][1, 5] == 0 and abs(r["chamfer"] - 0.5 * (r["accuracy"] + r["completion"])) < 1e-15
    # half a square against the full one.  The half is sampled at 10^5 per m^2 (its largest hole is about sqrt(ln N / (pi density)) = 0.006 m,
    # so every reference sample over the half is within the threshold of 0.01 m), the full square at 4000: sigma = sqrt(1 / (4 n)) = 0.008,
    # and the threshold's margin beyond the half's edge moves the expectation by 0.01, well inside 5 sigma = 0.04
    half_rows = _sampled(*cases.square_mesh(0.0, x1=0.5), density=1e5, seed=3)
    half = geo.compare_host(half_rows, cases.square_mesh(0.0), threshold=0.01, max_dist=1.0, cell=0.05, density=4000.0, seed=3)
    n = half["table"][1, 0]
    sigma = np.sqrt(0.25 / n)
    print(f"GEOERR half square: completion ratio {half['completion_ratio']} against 0.5 +- 5 x {sigma} ({int(n)} samples); precision {half['precision']}")
    assert abs(half["completion_ratio"] - 0.5) <= 5 * sigma
    assert half["table"][0, 5] == 0 and half["table"][1, 5] == 0 and half["table"][0, 3] < 0.05      # (nothing clamped; the dense half lies on the sparse square)
    # a set against itself
    rows = _sampled(*cases.random_mesh(20, seed=4), density=500)
    self_ = geo.compare_host(rows, rows, threshold=0.05, max_dist=1.0)
    print(f"GEOERR self: {self_['table'].tolist()}")
    assert self_["accuracy"] == 0 and self_["completion"] == 0 and self_["chamfer"] == 0 and self_["fscore"] == 1.0 and self_["precision"] == 1.0
    assert self_["table"][:, 1:4].max() == 0 and (self_["table"][:, 4] == 1).all() and (self_["table"][:, 5:] == 0).all() and (self_["table"][:, 0] == len(rows)).all()
    empty = geo.derived_figures(np.zeros((2, 8)))
    assert empty["fscore"] == 0.0


def test_sampler_statement():
    v, tris = cases.random_mesh(257, seed=1)
    density = 300.0
    rows, c, f = geo.sample_mesh_host(v, tris, density, seed=11, full=True)
    xyz, tid = f["xyz"], f["tri"]
    P = pc.rows_xyz(v).astype(np.float64)[tris]      # [m,3,3]
    a, e1, e2 = P[tid, 0], P[tid, 1] - P[tid, 0], P[tid, 2] - P[tid, 0]
    # barycentric coordinates by least squares in the triangle's plane
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r = xyz - a
    b1, b2 = (r * e1).sum(1), (r * e2).sum(1)
    det = g11 * g22 - g12 * g12
    u, w = (g22 * b1 - g12 * b2) / det, (g11 * b2 - g12 * b1) / det
    total_area = f["area"].sum()
    sigma = np.sqrt(len(tris) / 12.0)      # the sum of m independent roundings, each uniform over a unit interval
    print(f"GEOERR sampler: {c}; min barycentric {min(u.min(), w.min(), (1 - u - w).min())}; total {c['samples']} against {total_area * density} +- 5 x {sigma}")
    assert min(u.min(), w.min(), (1 - u - w).min()) >= -1e-12
    assert abs(c["samples"] - total_area * density) <= 5 * sigma + 1
    assert bool((np.diff(tid) >= 0).all()) and np.array_equal(np.bincount(tid, minlength=len(tris)), f["counts"])
    # the four mid-point sub-triangles of one large triangle hold a quarter each
    sq = cases.rows_of([[0, 0, 0], [3, 0, 0], [0, 2, 0]]), np.array([[0, 1, 2]], dtype=np.int32)
    _, _, g = geo.sample_mesh_host(*sq, 4000.0, seed=5, full=True)
    uu, ww = g["xyz"][:, 0] / 3.0, g["xyz"][:, 1] / 2.0
    n = len(uu)
    parts = np.array([((uu < 0.5) & (ww < 0.5) & (uu + ww < 0.5)).sum(), (uu >= 0.5).sum(), (ww >= 0.5).sum(), ((uu < 0.5) & (ww < 0.5) & (uu + ww >= 0.5)).sum()])
    sig = np.sqrt(n * 0.25 * 0.75)
    print(f"GEOERR sampler quarters: {parts.tolist()} of {n}, 5 sigma = {5 * sig}")
    assert parts.sum() == n and bool((np.abs(parts - n / 4) <= 5 * sig).all())
    # rgba of the corner with the largest weight
    assert set(np.unique(g["xyz"][:, 2]).tolist()) == {0.0}
    # degenerate triangles
    dv, dt, kinds = cases.degenerate_mesh()
    _, dc, df = geo.sample_mesh_host(dv, dt, 100.0, seed=2, full=True)
    print(f"GEOERR sampler degenerate: {dc}, counts {df['counts'].tolist()}")
    assert dc["degenerate"] == 6 and [k for k, n_ in zip(kinds, df["counts"]) if n_ > 0] == ["sound", "sound"] and set(df["tri"].tolist()) == {0, 7}
    # seeds
    again = geo.sample_mesh_host(v, tris, density, seed=11)[0]
    other = geo.sample_mesh_host(v, tris, density, seed=12)[0]
    assert again.tobytes() == rows.tobytes() and other.tobytes() != rows.tobytes()
    capped, cc = geo.sample_mesh_host(v, tris, density, seed=11, cap=1000)
    assert capped.tobytes() == rows[:1000].tobytes() and cc["dropped"] == c["samples"] - 1000 and cc["written"] == 1000


def test_rgba_is_the_nearest_corners():
    v, tris = cases.square_mesh()
    rows, _, f = geo.sample_mesh_host(v, tris, 2000.0, seed=9, full=True)
    P = pc.rows_xyz(v).astype(np.float64)[tris][f["tri"]]      # [n,3,3]
    # barycentric weights of a planar triangle from the areas opposite each corner
    x = f["xyz"]
    area = lambda p, q, r: 0.5 * np.abs(np.cross(q - p, r - p)[:, 2])
    w = np.stack([area(x, P[:, 1], P[:, 2]), area(P[:, 0], x, P[:, 2]), area(P[:, 0], P[:, 1], x)], 1)
    clear = np.sort(w, 1)[:, 2] - np.sort(w, 1)[:, 1] > 1e-9
    want = v[tris[f["tri"], np.argmax(w, 1)], 3]
    assert clear.sum() > 0.99 * len(rows) and np.array_equal(rows[clear, 3], want[clear])


def test_mixer_is_the_stated_one():
    def mix(x):
        x ^= x >> 16; x = (x * 0x7feb352d) & 0xffffffff; x ^= x >> 15; x = (x * 0x846ca68b) & 0xffffffff; x ^= x >> 16
        return x
    for seed, t, k in ((0, 0, 0), (1, 2, 3), (0xffffffff, 262399, 0xffffffff), (12345, 7, 1 << 24)):
        want = mix((mix((mix((seed ^ 0x9e3779b9) & 0xffffffff) + t) & 0xffffffff) + k) & 0xffffffff)
        assert int(geo.sample_hash(seed, [t], [k])[0]) == want, (seed, t, k)


def test_cabi_declares_and_binds_the_seven_symbols():
    from mm3dgs_slam_amd import _lib
    h = open(os.path.join(ROOT, "include", "mm3dgs.h")).read()
    names = ("mm3dgs_nn_grid_work_bytes", "mm3dgs_nn_grid_build", "mm3dgs_nn_query_work_bytes", "mm3dgs_nn_query", "mm3dgs_mesh_sample_work_bytes",
             "mm3dgs_mesh_sample_plan", "mm3dgs_mesh_sample_emit")
    lib = _lib.load()
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", h) and name in _lib.exported_symbols() and hasattr(lib, name), name
    P = C.c_void_p
    assert lib.mm3dgs_nn_grid_build.argtypes == [C.c_uint64, P, C.c_double, C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, P, P, P, P, P]
    assert lib.mm3dgs_nn_query.argtypes == [C.c_uint64, P, C.c_uint64, C.c_double, C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, P, P, C.c_double, C.c_double,
                                            P, P, P, P]
    assert lib.mm3dgs_mesh_sample_plan.argtypes == [C.c_uint64, P, C.c_uint64, P, C.c_double, C.c_uint32, P, P, P]
    assert lib.mm3dgs_mesh_sample_emit.argtypes == [C.c_uint64, P, C.c_uint64, P, C.c_double, C.c_uint32, P, P, C.c_uint64, P, P]
    for fn in (lib.mm3dgs_nn_grid_work_bytes, lib.mm3dgs_nn_query_work_bytes, lib.mm3dgs_mesh_sample_work_bytes):
        assert fn.restype is C.c_size_t
    for fn in (lib.mm3dgs_nn_grid_build, lib.mm3dgs_nn_query, lib.mm3dgs_mesh_sample_plan, lib.mm3dgs_mesh_sample_emit):
        assert fn.restype is C.c_int
    for n_ref, g in ((1, (1, 1, 1)), (1000, (5, 4, 3)), (1 << 20, (64, 64, 65)), (1 << 30, (512, 512, 256))):
        n = int(lib.mm3dgs_nn_grid_work_bytes(n_ref, *g))
        assert n > 0 and n % 8 == 0 and n >= 4 * n_ref + 4 * g[0] * g[1] * g[2], (n_ref, g, n)
    for n_ref, g in ((0, (1, 1, 1)), ((1 << 30) + 1, (1, 1, 1)), (10, (0, 1, 1)), (10, (1, -1, 1)), (10, (512, 512, 257)), (10, (1 << 16, 1 << 16, 1 << 16))):
        assert int(lib.mm3dgs_nn_grid_work_bytes(n_ref, *g)) == 0, (n_ref, g)
    for fn in (lib.mm3dgs_nn_query_work_bytes, lib.mm3dgs_mesh_sample_work_bytes):
        for n in (1, 257, 262400, 1 << 30):
            assert int(fn(n)) > 0 and int(fn(n)) % 8 == 0, n
        for n in (0, (1 << 30) + 1):
            assert int(fn(n)) == 0, n
    assert lib.mm3dgs_version() == 213
    assert re.search(r"#define MM3DGS_ABI_VERSION 213\b", h)


def test_config_block_is_off_by_default():
    from mm3dgs_slam_amd.config import default_config, utmm_config
    for cfg in (default_config(), utmm_config()):
        assert cfg["geometry"] == {"eval": False, "estimate": "mesh", "reference": "sensor", "threshold": 0.05, "max_dist": 1.0, "density": 10000.0, "cell": 0,
                                   "seed": 0, "align": "none", "max_samples": 16777216}


def test_slam_top_accepts_the_geometry_switch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "slam_top.py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "--geometry" in out.stdout
    import slam_top
    assert callable(slam_top.evaluate_geometry_checkpoint)


def test_colour_by_distance_uses_the_viridis_table():
    from mm3dgs_slam_amd.debug_frames import viridis
    rows = cases.rows_of(np.zeros((4, 3)))
    out = geo.colour_by_distance(rows, np.array([0.0, 0.05, 0.2, np.nan], dtype=np.float32), 0.05)
    lut = np.floor(viridis().numpy() * 255.0 + 0.5).astype(np.uint8)
    got = pc.rows_rgba(out)
    assert got[0, :3].tolist() == lut[0].tolist() and got[1, :3].tolist() == lut[128].tolist() and got[2, :3].tolist() == lut[255].tolist()
    assert got[3].tolist() == [0, 0, 0, 255] and np.array_equal(out[:, :3], rows[:, :3])


def _cpu_slam(tmp, geometry, mesh, tracking=None):
    """The stand-in run of `device: cpu` of tests/test_mesh.py (32 x 48, 3 frames, the oracle rasterizer injected), run to its end."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.renderer import Renderer
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from oracle.raster_ref import RefRasterizer
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device="cpu", height=32, width=48, tracking=dict({"iters": 2}, **(tracking or {})), mapping={"iters": 3, "kf_every": 2},
                         outputdir=str(tmp), mesh=mesh, geometry=geometry)
    seq = SyntheticSequence(cfg, 3, 600, seed=2, renderer=Renderer(cfg, rasterizer_cls=RefRasterizer))
    slam = SLAM(cfg, seq, rasterizer_cls=RefRasterizer)
    slam.run()
    return slam, seq, cfg


def test_cpu_run_scores_its_export(tmp_path):
    MESH = {"voxel": 0.08, "every": 1, "export": False}
    GEO = {"density": 400.0, "threshold": 0.05, "max_dist": 1.0}
    on, seq, cfg = _cpu_slam(tmp_path / "on", dict(GEO, eval=True), MESH)
    out = on.geometry_eval
    assert out is not None
    m = json.load(open(tmp_path / "on" / "geometry" / "metrics.json"))
    print(f"GEOERR cpu run: {json.dumps({k: m[k] for k in ('accuracy', 'completion', 'completion_ratio', 'precision', 'fscore', 'chamfer', 'n_estimate', 'n_reference', 'cells')})}")
    for k in ("accuracy", "completion", "completion_ratio", "recall", "precision", "fscore", "chamfer"):
        assert np.isfinite(m[k]), k
    assert 0 <= m["accuracy"] < 1.0 and 0 <= m["completion"] < 1.0 and m["n_estimate"] > 0 and m["n_reference"] > 0 and m["cells"] == [0.05, 0.05]
    assert m["estimate_to_reference"]["n"] == m["n_estimate"] and m["reference_to_estimate"]["n"] == m["n_reference"]
    acc, comp = pc.read_ply(str(tmp_path / "on" / "geometry" / "accuracy.ply")), pc.read_ply(str(tmp_path / "on" / "geometry" / "completion.ply"))
    assert len(acc) == m["n_estimate"] and len(comp) == m["n_reference"]
    # the block off: the same poses and results.npz, no new directory
    off, _, _ = _cpu_slam(tmp_path / "off", dict(GEO, eval=False), MESH)
    a, b = np.load(tmp_path / "on" / "results.npz", allow_pickle=True), np.load(tmp_path / "off" / "results.npz", allow_pickle=True)
    assert list(a.keys()) == list(b.keys()) and a["pose_est"].tobytes() == b["pose_est"].tobytes() and a["pose_gt"].tobytes() == b["pose_gt"].tobytes()
    assert all(torch.equal(p, q) for p, q in zip(on.estimate_pose_list, off.estimate_pose_list))
    assert off.geometry_eval is None and not (tmp_path / "off" / "geometry").exists()
    # a file as the reference: the mesh the run exports, and the cloud; the point cloud as the estimate
    mesh_file = off.export_mesh(path=str(tmp_path / "ref"))["mesh"]
    by_file = off.evaluate_geometry(path=str(tmp_path / "by_file"), reference=mesh_file)
    print(f"GEOERR cpu run against its own mesh file: accuracy {by_file['accuracy']}, completion {by_file['completion']}")
    assert by_file["accuracy"] == 0 and by_file["completion"] == 0 and by_file["fscore"] == 1.0
    cfg_off = off.cfg
    cfg_off["pointcloud"].update(voxel=0.05, every=1)
    cloud_file = off.export_pointcloud(path=str(tmp_path / "refc"))["cloud"]
    by_cloud = off.evaluate_geometry(path=str(tmp_path / "by_cloud"), estimate="pointcloud", reference=cloud_file)
    assert by_cloud["accuracy"] == 0 and by_cloud["completion"] == 0 and by_cloud["n_estimate"] == len(pc.read_ply(cloud_file))
    with pytest.raises(ValueError, match="mesh / pointcloud"):
        off.evaluate_geometry(estimate="volume")
    cfg_off["geometry"]["align"] = "icp"
    with pytest.raises(ValueError, match="none / horn / umeyama"):
        off.evaluate_geometry()


def test_cpu_run_with_gt_poses_and_sensor_views_scores_zero(tmp_path):
    on, _, _ = _cpu_slam(tmp_path / "gt", {"eval": True, "density": 400.0}, {"voxel": 0.08, "every": 1, "source": "sensor"}, tracking={"use_gt_pose": True})
    m = json.load(open(tmp_path / "gt" / "geometry" / "metrics.json"))
    print(f"GEOERR cpu run, ground-truth poses and sensor views: accuracy {m['accuracy']}, completion {m['completion']}, {m['n_estimate']} points")
    assert m["accuracy"] == 0 and m["completion"] == 0 and m["fscore"] == 1.0 and m["n_estimate"] == m["n_reference"] > 0
    # the estimated trajectory is the true one: either alignment is the identity up to the rounding of its SVD and of the float32 rows
    for method in ("horn", "umeyama"):
        on.cfg["geometry"]["align"] = method
        aligned = on.evaluate_geometry(path=str(tmp_path / method))
        print(f"GEOERR cpu run, align {method}: accuracy {aligned['accuracy']}, completion {aligned['completion']}")
        assert aligned["accuracy"] < 1e-5 and aligned["completion"] < 1e-5 and aligned["n_estimate"] == m["n_estimate"]


def test_sensor_reference_needs_sensor_depth(tmp_path):
    on, seq, cfg = _cpu_slam(tmp_path / "d", {"eval": False, "density": 400.0}, {"voxel": 0.08, "every": 1})

    class NoDepth:
        def __len__(self):
            return len(seq)

        def __getitem__(self, i):
            c, _, p = seq[i]
            return c, None, p
    on.seq = NoDepth()
    with pytest.raises(ValueError, match="no sensor depth"):
        on.evaluate_geometry(path=str(tmp_path / "x"))
