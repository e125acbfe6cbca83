"""The host statement of the normals (mm3dgs_slam_amd/geometry.py: nn_index_host, normal_row, vertex_normals_host; mesh.py: the PLY layout
with normals; export.py: the two opt-in keys): the nearest row against brute force, the dots against an independent float64 computation,
exact cases, the fixed-point vertex normals against a plain float64 sum, and a `device: cpu` run with the keys on, off and absent.

Bars.  A dot and a normal component are one float32 rounding at magnitude <= 1 away from float64: 1.2e-7 (2^-23).  For the vertex normals
the fixed-point error adds at most 64 terms of 2^-41 relative to 2^E_v against |S_v| >= 2^(E_v - 4): 2^-31 (the test asserts both
conditions on its inputs).  Every test prints its figures (`NRMERR ...`, pytest -s) before it asserts."""
import json
import os
import random
import re

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import export as ex, geometry as geo, mesh as ms, pointcloud as pc
from tests import geometry_cases as gc, normals_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1.2e-7


# ---- nearest row ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ref", nc.N_REF)
def test_nearest_row_equals_brute_force(n_ref):
    for n_q in nc.N_Q:
        c = nc.index_case(n_ref, n_q)
        d, idx, info = geo.nn_index_host(c["query"], c["ref"], c["cell"], c["max_dist"])
        d0, info0 = geo.nn_distances_host(c["query"], c["ref"], c["cell"], c["max_dist"])
        bd, bidx = geo.nn_index_brute_host(c["query"], c["ref"], c["max_dist"])
        ties = nc.tie_counts(c)
        print(f"NRMERR index {c['name']}: {int((idx == geo.NO_INDEX).sum())} without a row, {int((ties > 1).sum())} ties (largest {int(ties.max())}), "
              f"{int(np.isnan(d).sum())} skipped, {int(info['clamped'].sum())} clamped")
        assert idx.dtype == np.uint32 and np.array_equal(idx, bidx)
        assert d.tobytes() == d0.tobytes() == bd.tobytes() and np.array_equal(info["clamped"], info0["clamped"])
        assert np.array_equal(idx == geo.NO_INDEX, np.isnan(d) | info["clamped"])
        if n_ref == 500:
            assert ties[0] == 8 and idx[0] == 10                       # the cube's centre: eight ties, the smallest row
        if n_ref == 3:
            assert ties[0] == 2 and idx[0] == 0 and d[0] == 0          # the doubled point
        if n_q >= 255:
            assert idx[1] == (30 if n_ref == 500 else 0) and (n_ref == 1 or ties[1] == 2)
            assert np.isnan(d[2]) and np.isnan(d[4]) and info["clamped"][3] and idx[3] == geo.NO_INDEX


# ---- one direction's row ----------------------------------------------------------------------------------------------------------------
def _independent_dots(est, ref, sets, tris, max_dist):
    """Brute-force neighbour and plain np.cross in float64: (dot float64 [n], counted)."""
    from mm3dgs_slam_amd.pointcloud import rows_xyz
    (qs, rs), (tq, tr) = sets, tris
    _, j = geo.nn_index_brute_host(qs, rs, max_dist)
    normal = lambda mesh: np.cross(*(lambda p, t: (p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]))(rows_xyz(mesh[0]).astype(np.float64), mesh[1]))
    nq, nr = normal(est), normal(ref)
    counted = j != geo.NO_INDEX
    a, b = nq[tq[counted]], nr[tr[j[counted]]]
    dot = np.full(len(qs), np.nan)
    dot[counted] = (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return dot, counted


def _host_normals(est, ref, density=2000.0, seed=0, **kw):
    return geo.compare_host(est, ref, threshold=0.05, max_dist=0.2, density=density, seed=seed, normals=True, **kw)


def test_normal_rows_against_an_independent_float64_computation():
    est, ref = nc.icosphere(2), nc.shifted(nc.icosphere(2), (0.01, 0.0, 0.0))
    r = _host_normals(est, ref)
    rows_e, _, fe = geo.sample_mesh_host(*est, 2000.0, 0, full=True)
    rows_r, _, fr = geo.sample_mesh_host(*ref, 2000.0, 0, full=True)
    for name, dots, (a, b), sets, tris, row in (("estimate -> reference", r["dot_estimate"], (est, ref), (rows_e, rows_r), (fe["tri"], fr["tri"]), r["normal_table"][0]),
                                              ("reference -> estimate", r["dot_reference"], (ref, est), (rows_r, rows_e), (fr["tri"], fe["tri"]), r["normal_table"][1])):
        want, counted = _independent_dots(a, b, sets, tris, 0.2)
        err = float(np.abs(dots[counted].astype(np.float64) - want[counted]).max())
        print(f"NRMERR sphere {name}: {int(counted.sum())} of {len(dots)} counted, max |dot - float64| = {err:.3e}, row {row.tolist()}")
        assert np.array_equal(~np.isnan(dots), counted) and err <= BAR
        assert row[0] == counted.sum() and row[5] == (~counted).sum() and row[6] == 0
        assert abs(row[1] - np.abs(want[counted]).mean()) <= BAR and abs(row[2] - want[counted].mean()) <= BAR and abs(row[3] - np.abs(want[counted]).min()) <= BAR
    assert 0.97 < r["normals"]["normal_consistency"] <= 1.0
    k = geo.normal_row(r["dot_estimate"], r["nearest_estimate"] == geo.NO_INDEX, sum_order="kernel")
    assert np.array_equal(k[[0, 3, 5, 6]], r["normal_table"][0][[0, 3, 5, 6]]) and np.abs(k - r["normal_table"][0]).max() <= 1e-12


def test_exact_cases():
    sphere = nc.icosphere(2)
    same = _host_normals(sphere, sphere)
    assert (same["dot_estimate"] == np.float32(1)).all() and (same["dot_reference"] == np.float32(1)).all()
    assert same["normals"] == {"normal_accuracy": 1.0, "normal_completion": 1.0, "normal_consistency": 1.0, "normal_accuracy_signed": 1.0,
                               "normal_completion_signed": 1.0, "normal_consistency_signed": 1.0}
    flat = gc.square_mesh()      # flat: a flipped winding moves the samples inside their triangle, and every face still has the one normal
    flip = _host_normals(flat, nc.flipped(flat))
    print(f"NRMERR exact: same {same['normal_table'].tolist()}, flipped {flip['normal_table'].tolist()}")
    assert flip["normals"]["normal_consistency"] == 1.0 and flip["normals"]["normal_consistency_signed"] == -1.0
    assert (flip["normal_table"][:, 1] == 1).all() and (flip["normal_table"][:, 2] == -1).all()
    floor, wall = nc.floor_and_wall()
    fw = geo.compare_host(floor, wall, threshold=0.05, max_dist=0.25, density=500.0, normals=True)
    counted = ~np.isnan(fw["dot_estimate"])
    print(f"NRMERR floor / wall: {int(counted.sum())} of {len(counted)} counted, table {fw['normal_table'].tolist()}")
    assert 0 < counted.sum() < len(counted) and (fw["dot_estimate"][counted] == 0).all() and (fw["dot_reference"][~np.isnan(fw["dot_reference"])] == 0).all()
    assert fw["normal_table"][0, 5] == (~counted).sum() and fw["normals"]["normal_consistency"] == 0.0
    cloud = geo.sample_mesh_host(*sphere, 500.0)[0]
    for a, b in ((cloud, sphere), (sphere, cloud)):
        with pytest.raises(ValueError, match="normals need a mesh"):
            geo.compare_host(a, b, normals=True)
    plain = geo.compare_host(flat, nc.flipped(flat), threshold=0.05, max_dist=0.2, density=2000.0)
    assert "normals" not in plain and plain["table"].tobytes() == flip["table"].tobytes() and plain["dist_estimate"].tobytes() == flip["dist_estimate"].tobytes()


def test_ids_out_of_range_are_counted_and_read_nothing():
    mesh = nc.rejecting_mesh()
    m = len(mesh[1])
    tri_q = np.array([0, 7, m, 0xfffffffe, 0, 0, 0, 1], dtype=np.uint32)
    index = np.array([0, 0, 0, 0, 3, 0xffffffff, 9, 2], dtype=np.uint32)      # 9: beyond tri_r; 3: a triangle id beyond the mesh
    tri_r = np.array([0, 7, 6, m + 3], dtype=np.uint32)
    dot, none = geo.normal_dots_host(tri_q, index, tri_r, mesh, mesh)
    row = geo.normal_row(dot, none)
    print(f"NRMERR ids: dot {dot.tolist()}, row {row.tolist()}")
    assert np.array_equal(np.isnan(dot), [False, False, True, True, True, True, True, True]) and none.tolist() == [False] * 5 + [True, False, False]
    assert dot[0] == 1 and dot[1] == 0 and row.tolist() == [2.0, 0.5, 0.5, 0.0, 0.0, 1.0, 5.0, 0.0]
    assert geo.normal_row(np.full(3, np.nan, np.float32), np.array([True, False, True])).tolist() == [0, 0, 0, 0, 0, 2, 1, 0]


# ---- vertex normals ---------------------------------------------------------------------------------------------------------------------
def _plain_normals(v, tris):
    p = pc.rows_xyz(v).astype(np.float64)
    c = np.cross(p[tris[:, 1]] - p[tris[:, 0]], p[tris[:, 2]] - p[tris[:, 0]])
    s = np.zeros((len(p), 3))
    for k in range(3):
        np.add.at(s, tris[:, k], c)
    return s / np.linalg.norm(s, axis=1)[:, None], c


def test_vertex_normals_exact_cases():
    v, tris = nc.octahedron()
    n, c = geo.vertex_normals_host(v, tris)
    assert n.dtype == np.float32 and np.array_equal(n, pc.rows_xyz(v)) and c == {"vertices": 6, "without_normal": 0, "rejected_triangles": 0}
    rng = np.random.default_rng(0)
    for mesh in (nc.octahedron(), nc.grid_mesh(), nc.fan_mesh(), nc.icosphere(2)):
        a = geo.vertex_normals_host(*mesh)[0]
        b = geo.vertex_normals_host(mesh[0], mesh[1][rng.permutation(len(mesh[1]))])[0]
        assert a.tobytes() == b.tobytes()
    v, tris = nc.rejecting_mesh()
    n, c = geo.vertex_normals_host(v, tris)
    print(f"NRMERR rejecting mesh: counters {c}, normals {n.tolist()}")
    assert c == {"vertices": 9, "without_normal": 5, "rejected_triangles": 7}
    assert not n[[3, 4, 5, 7, 8]].any() and (np.abs(np.linalg.norm(n[[0, 1, 2, 6]].astype(np.float64), axis=1) - 1) <= BAR).all()
    n0, c0 = geo.vertex_normals_host(v, np.zeros((0, 3), dtype=np.int32))
    assert not n0.any() and c0["without_normal"] == 9


@pytest.mark.parametrize("name", ["grid", "sphere", "single"])
def test_vertex_normals_against_a_plain_float64_sum(name):
    v, tris = {"grid": nc.grid_mesh, "sphere": lambda: nc.icosphere(2), "single": nc.single_triangle}[name]()
    want, c = _plain_normals(v, tris)
    # the conditions of the bound, asserted on the input: valence <= 64 and |S_v| >= 2^(E_v - 4)
    valence = np.bincount(tris.reshape(-1), minlength=len(v))
    _, Et = np.frexp(np.abs(c).max(1))
    Ev = np.full(len(v), -10000)
    for k in range(3):
        np.maximum.at(Ev, tris[:, k], Et)
    s = np.zeros((len(v), 3))
    for k in range(3):
        np.add.at(s, tris[:, k], c)
    assert valence.max() <= 64 and valence.min() >= 1 and (np.linalg.norm(s, axis=1) >= np.ldexp(1.0, Ev - 4)).all()
    got, counters = geo.vertex_normals_host(v, tris)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"NRMERR vertex normals {name}: {len(v)} vertices, valence <= {int(valence.max())}, max component error {err:.3e}")
    assert err <= BAR and counters["without_normal"] == 0


# ---- files ------------------------------------------------------------------------------------------------------------------------------
def test_ply_with_and_without_normals(tmp_path):
    v, tris = nc.icosphere(1)
    n = geo.vertex_normals_host(v, tris)[0]
    plain, with_n = str(tmp_path / "plain.ply"), str(tmp_path / "normals.ply")
    ms.write_mesh_ply(plain, v, tris)
    faces = np.empty(len(tris), dtype=ms._FACE)
    faces["n"], faces["v"] = 3, tris
    assert open(plain, "rb").read() == ms.mesh_header(len(v), len(tris)).encode("ascii") + v.astype("<i4").tobytes() + faces.tobytes()
    ms.write_mesh_ply(with_n, v, tris, n)
    data = open(with_n, "rb").read()
    head = data[:data.index(b"end_header\n") + 11].decode("ascii")
    assert "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar red\n" in head
    assert len(data) == len(head) + 28 * len(v) + 13 * len(tris)
    rv, rt, rn = ms.read_mesh_ply_normals(with_n)
    assert np.array_equal(rv, v) and np.array_equal(rt, tris) and rn.dtype == np.float32 and rn.tobytes() == n.tobytes()
    rv, rt = ms.read_mesh_ply(with_n)
    assert np.array_equal(rv, v) and np.array_equal(rt, tris)
    assert ms.read_mesh_ply_normals(plain)[2] is None and np.array_equal(ms.read_mesh_ply(plain)[0], v)
    sv, st = ms.read_surface_ply(with_n)
    fv, ft = ms.read_foreign_ply(with_n)
    assert np.array_equal(sv, v) and np.array_equal(st, tris) and np.array_equal(fv, v) and np.array_equal(ft, tris)
    with pytest.raises(ValueError, match="normals for"):
        ms.write_mesh_ply(with_n, v, tris, n[:-1])


# ---- options ----------------------------------------------------------------------------------------------------------------------------
def test_options_pin_and_validate_the_normal_keys():
    from mm3dgs_slam_amd.config import GEOMETRY_CULL, GEOMETRY_DEPTH, GEOMETRY_NORMALS, MESH_CLEAN, MESH_NORMALS, MESH_VOLUME, default_config
    assert GEOMETRY_NORMALS == {"normals": False} and MESH_NORMALS == {"normals": False}
    cfg = default_config(device="cpu")
    assert not set(GEOMETRY_NORMALS) & (set(cfg["geometry"]) | set(GEOMETRY_CULL) | set(GEOMETRY_DEPTH))
    assert not set(MESH_NORMALS) & (set(cfg["mesh"]) | set(MESH_CLEAN) | set(MESH_VOLUME))
    assert ex.options(cfg, "geometry")["normals"] is False and ex.options(cfg, "mesh")["normals"] is False
    for block in ("geometry", "mesh"):
        on = dict(cfg, **{block: dict(cfg[block], normals=True)})
        assert ex.options(on, block)["normals"] is True
        for bad in ("yes", 1, 2.0):
            with pytest.raises(ValueError, match=block + r"\.normals"):
                ex.options(dict(cfg, **{block: dict(cfg[block], normals=bad)}), block)


def test_cabi_declares_and_binds_the_new_symbols():
    from mm3dgs_slam_amd import _lib
    h = open(os.path.join(ROOT, "include", "mm3dgs.h")).read()
    for name in ("mm3dgs_nn_query_index", "mm3dgs_mesh_sample_emit_tri", "mm3dgs_normal_consistency_work_bytes", "mm3dgs_normal_consistency",
                 "mm3dgs_mesh_vertex_normals_work_bytes", "mm3dgs_mesh_vertex_normals"):
        assert re.search(r"\b" + name + r"\s*\(", h) and name in _lib.exported_symbols(), name
    lib = _lib.load()
    assert lib.mm3dgs_mesh_vertex_normals_work_bytes(0) == 0 and lib.mm3dgs_mesh_vertex_normals_work_bytes(1 << 31) == 0
    assert lib.mm3dgs_mesh_vertex_normals_work_bytes(1000) >= 1000 * 28
    assert lib.mm3dgs_normal_consistency_work_bytes(0) == 0 and lib.mm3dgs_normal_consistency_work_bytes((1 << 30) + 1) == 0
    assert lib.mm3dgs_normal_consistency_work_bytes(257) >= 2 * 64


# ---- a device: cpu run --------------------------------------------------------------------------------------------------------------------
MESH = {"voxel": 0.08, "every": 1, "export": False}
GEO = {"density": 400.0, "threshold": 0.05, "max_dist": 1.0}


@pytest.fixture(scope="module")
def cpu_run(tmp_path_factory):
    """The stand-in run of `device: cpu` of tests/test_mesh_depth.py (32 x 48, the oracle rasterizer injected), 4 frames, run to its end."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.renderer import Renderer
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from oracle.raster_ref import RefRasterizer
    tmp = tmp_path_factory.mktemp("normals_run")
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device="cpu", height=32, width=48, tracking={"iters": 2}, mapping={"iters": 3, "kf_every": 2}, outputdir=str(tmp), mesh=dict(MESH),
                         geometry=dict(GEO, eval=False))
    seq = SyntheticSequence(cfg, 4, 600, seed=2, renderer=Renderer(cfg, rasterizer_cls=RefRasterizer))
    slam = SLAM(cfg, seq, rasterizer_cls=RefRasterizer)
    slam.run()
    return slam, seq, cfg, tmp


def _stages(slam, tmp, name, geometry, mesh):
    slam.cfg["geometry"], slam.cfg["mesh"] = dict(GEO, eval=False, **geometry), dict(MESH, **mesh)
    g = slam.evaluate_geometry(path=str(tmp / name / "geometry"))
    m = slam.export_mesh(path=str(tmp / name / "mesh"))
    state = (np.stack([p.detach().numpy() for p in slam.estimate_pose_list]).tobytes(), open(tmp / "results.npz", "rb").read())
    return g, m, state


def test_cpu_run_with_the_keys_on_off_and_absent(cpu_run):
    slam, seq, cfg, tmp = cpu_run
    g_abs, m_abs, s_abs = _stages(slam, tmp, "absent", {}, {})
    g_off, m_off, s_off = _stages(slam, tmp, "off", {"normals": False}, {"normals": False})
    g_on, m_on, s_on = _stages(slam, tmp, "on", {"normals": True}, {"normals": True})
    assert s_abs == s_off == s_on
    files = lambda d: sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)
    assert files(tmp / "absent") == files(tmp / "off") == ["geometry/accuracy.ply", "geometry/completion.ply", "geometry/metrics.json", "mesh/mesh.ply"]
    for f in files(tmp / "absent"):
        assert (tmp / "absent" / f).read_bytes() == (tmp / "off" / f).read_bytes(), f
    assert files(tmp / "on") == ["geometry/accuracy.ply", "geometry/completion.ply", "geometry/metrics.json", "geometry/normals.npz", "mesh/mesh.ply"]
    for f in ("geometry/accuracy.ply", "geometry/completion.ply"):
        assert (tmp / "on" / f).read_bytes() == (tmp / "off" / f).read_bytes(), f
    met = json.load(open(tmp / "on" / "geometry" / "metrics.json"))
    block = met.pop("normals")
    assert met == json.load(open(tmp / "off" / "geometry" / "metrics.json")) and "normals" not in g_off
    z = np.load(tmp / "on" / "geometry" / "normals.npz")
    print(f"NRMERR cpu run: {json.dumps(block)}")
    assert block["normal_consistency"] == 0.5 * (block["normal_accuracy"] + block["normal_completion"]) == g_on["normals"]["normal_consistency"]
    assert 0.3 < block["normal_consistency"] <= 1.0 and block["estimate_to_reference"]["n"] > 0
    assert z["dot_estimate"].dtype == np.float32 and z["nearest_estimate"].dtype == np.uint32
    assert len(z["dot_estimate"]) == len(z["nearest_estimate"]) == met["n_estimate"] and len(z["dot_reference"]) == len(z["nearest_reference"]) == met["n_reference"]
    assert block["estimate_to_reference"]["n"] == int((~np.isnan(z["dot_estimate"])).sum())
    # mesh.ply: the same mesh, 28-byte vertices, the statement's normals
    v0, t0 = ms.read_mesh_ply(str(tmp / "off" / "mesh" / "mesh.ply"))
    v1, t1, n1 = ms.read_mesh_ply_normals(str(tmp / "on" / "mesh" / "mesh.ply"))
    assert np.array_equal(v0, v1) and np.array_equal(t0, t1) and len(v1) > 0
    assert os.path.getsize(tmp / "on" / "mesh" / "mesh.ply") - os.path.getsize(tmp / "off" / "mesh" / "mesh.ply") == 12 * len(v1) + len("property float nx\n") * 3
    want, counters = geo.vertex_normals_host(v1, t1)
    assert n1.tobytes() == want.tobytes() and m_on["normals"] == counters and "normals" not in m_off
    # the sparse volume and the cleaned mesh take the same road
    slam.cfg["mesh"] = dict(MESH, normals=True, volume="sparse", clean="largest")
    out = slam.export_mesh(path=str(tmp / "sparse"))
    v2, t2, n2 = ms.read_mesh_ply_normals(out["mesh"])
    assert len(v2) == out["clean"]["vertices"] and n2.tobytes() == geo.vertex_normals_host(v2, t2)[0].tobytes()
    # refused: a point cloud on either side
    slam.cfg["mesh"] = dict(MESH)
    for keys in ({"estimate": "pointcloud"}, {"reference": pc.write_ply(str(tmp / "cloud.ply"), geo.sample_mesh_host(v1, t1, 100.0)[0])}):
        slam.cfg["geometry"] = dict(GEO, eval=False, normals=True, **keys)
        with pytest.raises(ValueError, match=r"geometry\.normals"):
            slam.evaluate_geometry(path=str(tmp / "x"))
    slam.cfg["geometry"] = dict(GEO, eval=False)
