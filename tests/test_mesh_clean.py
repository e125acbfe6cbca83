"""Mesh cleaning on the host (mm3dgs_slam_amd/mesh_clean.py): components_host against scipy's connected_components, clean_host against a
boolean-mask statement written here, on every case of tests/mesh_clean_cases.py; the `mesh` block's two keys; the C ABI's declarations; and
a `device: cpu` run whose mesh gets a blob planted in a corner of the volume.  No GPU."""
import ctypes as C
import json
import os
import random
import re

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import export as ex, mesh as ms, mesh_clean as mc
from tests import mesh_clean_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cases.all_cases()
IDS = [c["name"] for c in CASES]


def scipy_labels(V, tri):
    """(number of components, component id per vertex) of the graph whose edges are the sides of the valid triangles."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    ok = ((tri >= 0) & (tri < V)).all(1)
    good = tri[ok].astype(np.int64)
    a = np.concatenate([good[:, 0], good[:, 1], good[:, 2]])
    b = np.concatenate([good[:, 1], good[:, 2], good[:, 0]])
    graph = coo_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(V, V))
    n, comp = connected_components(graph, directed=False)
    return n, comp, ok


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_components_host_against_scipy(case):
    tri, V = case["triangles"], len(case["rows"])
    label, tri_count, counters = mc.components_host(V, tri)
    assert label.dtype == np.uint32 and tri_count.dtype == np.uint32 and label.shape == tri_count.shape == (V,) and counters.dtype == np.int64
    if V == 0:
        assert counters.tolist() == [0, 0, len(tri), 0, 0, 0, 0, 0]
        return
    n, comp, ok = scipy_labels(V, tri)
    # the same partition: the pairs (scipy id, label) are a bijection between the two sets of names
    pairs = np.unique(np.stack([comp.astype(np.int64), label.astype(np.int64)], 1), axis=0)
    assert len(pairs) == n == len(np.unique(label)) == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1]))
    # labels are the per-component minima
    mins = np.full(n, V, dtype=np.int64)
    np.minimum.at(mins, comp, np.arange(V))
    assert np.array_equal(label, mins[comp])
    # tri_count is a direct count
    want = np.zeros(V, dtype=np.int64)
    for t in tri[ok]:
        want[mins[comp[t[0]]]] += 1
    assert np.array_equal(tri_count, want)
    used = np.zeros(V, dtype=bool)
    used[tri[ok].reshape(-1)] = True
    best = int(want.max())
    assert counters.tolist() == [int((want > 0).sum()), (best << 32 | (~int(np.argmax(want)) & 0xffffffff)) if best else 0, int((~ok).sum()), int((~used).sum()), 0, 0, 0, 0]
    assert mc.largest_of(counters) == ((best, int(np.argmax(want))) if best else (0, None))


def mask_statement(rows, tri, mode, min_triangles):
    """Cleaning from scipy's components with boolean masks: (rows', triangles', index, info)."""
    V, T = len(rows), len(tri)
    if V == 0:
        return rows[:0], tri[:0], np.zeros(0, dtype=np.uint32), {"components": 0, "components_kept": 0, "largest_triangles": 0, "vertices_removed": 0,
                                                                  "triangles_removed": T, "skipped": T}
    n, comp, ok = scipy_labels(V, tri)
    count = np.bincount(comp[tri[ok, 0]], minlength=n)
    first = np.full(n, V, dtype=np.int64)
    np.minimum.at(first, comp, np.arange(V))
    if mode == "small":
        keep = count >= min_triangles
    else:
        keep = np.zeros(n, dtype=bool)
        if count.max() > 0:
            tied = np.flatnonzero(count == count.max())
            keep[tied[np.argmin(first[tied])]] = True      # on a tie the component with the smallest vertex
    vmask = keep[comp] & (count[comp] > 0)
    tmask = ok.copy()
    tmask[ok] = vmask[tri[ok, 0]]
    new = np.cumsum(vmask) - 1
    info = {"components": int((count > 0).sum()), "components_kept": int((keep & (count > 0)).sum()), "largest_triangles": int(count.max()),
            "vertices_removed": int((~vmask).sum()), "triangles_removed": int((~tmask).sum()), "skipped": int((~ok).sum())}
    return rows[vmask], new[tri[tmask]].astype(np.int32), np.flatnonzero(vmask).astype(np.uint32), info


RUNS = [(c, m) for c in CASES for m in c["modes"]]


@pytest.mark.parametrize("case,mode", RUNS, ids=[f"{c['name']} {m[0]} {m[1]}" for c, m in RUNS])
def test_clean_host_against_the_mask_statement(case, mode):
    rows, tri = case["rows"], case["triangles"]
    got = mc.clean_host(rows, tri, *mode, full=True)
    want = mask_statement(rows, tri, *mode)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.uint32
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and np.array_equal(got[2], want[2]) and got[3] == want[3]
    assert list(got[3]) == list(mc.INFO_NAMES)
    # the original order survives: index ascends, and the kept triangles are a subsequence of the input through the remap
    assert bool((np.diff(got[2].astype(np.int64)) > 0).all()) and got[0].tobytes() == rows[got[2].astype(np.int64)].tobytes()
    c = got[4]
    assert (c[5], c[6], c[7]) == (len(got[0]), len(got[1]), 0) and c[4] == got[3]["components_kept"]
    # closed under re-cleaning, and nothing unreferenced is left
    again = mc.clean_host(got[0], got[1], *mode)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes() and np.array_equal(again[2], np.arange(len(got[0])))
    assert again[3]["vertices_removed"] == 0 and again[3]["triangles_removed"] == 0 and again[3]["skipped"] == 0
    assert ms.mesh_topology(len(got[0]), got[1])["unreferenced"] == 0
    if len(got[1]):
        assert 0 <= got[1].min() and got[1].max() < len(got[0])
    if case["name"] == "cleaning removes nothing":      # apart from the two unreferenced vertices 0 and 9
        assert got[2].tolist() == list(range(1, 9)) and np.array_equal(got[1], tri - 1) and got[3]["triangles_removed"] == 0
    if case["name"] == "a tie for the largest" and mode[0] == "largest":
        assert got[2].tolist() == list(range(6)) and np.array_equal(got[1], cases.strip(0, 4))
    if case["name"].startswith("marching") and mode in (("largest", 1), ("small", 49)):
        topo = ms.mesh_topology(len(got[0]), got[1])
        assert topo["closed"] and topo["euler"] == 2 and got[3]["components"] == 3 and got[3]["components_kept"] == 1


def test_caps_below_the_totals_return_the_prefix_and_count_the_rest():
    case = CASES[IDS.index("T = 257")]
    full = mc.clean_host(case["rows"], case["triangles"], "small", 4, full=True)
    nv, nt = len(full[0]), len(full[1])
    got = mc.clean_host(case["rows"], case["triangles"], "small", 4, vcap=nv - 5, tcap=nt // 2, full=True)
    assert got[0].tobytes() == full[0][:nv - 5].tobytes() and got[1].tobytes() == full[1][:nt // 2].tobytes() and np.array_equal(got[2], full[2][:nv - 5])
    assert got[4].tolist() == full[4].tolist()[:7] + [((nt - nt // 2) << 32) | 5]


def test_bad_arguments_raise():
    rows, tri = cases.rows_for(3), np.array([[0, 1, 2]], dtype=np.int32)
    for mode, n in (("none", 1), ("biggest", 1), ("small", 0), ("small", -3), ("small", 1.5), ("small", True), ("largest", 0)):
        with pytest.raises(ValueError, match="mesh clean"):
            mc.clean_host(rows, tri, mode, n)
    with pytest.raises(ValueError, match="CUDA device"):
        mc.clean_device(rows, tri, "small", 1, device="cpu")
    assert mc.clean(rows, tri, "largest", 1, device="cpu")[3]["components_kept"] == 1


def test_config_keys_and_their_validation():
    from mm3dgs_slam_amd.config import MESH_CLEAN, default_config
    assert MESH_CLEAN == {"clean": "none", "clean_min_triangles": 100}
    cfg = default_config(device="cpu")
    assert "clean" not in cfg["mesh"] and "clean_min_triangles" not in cfg["mesh"]
    opt = ex.options(cfg, "mesh")
    assert (opt["clean"], opt["clean_min_triangles"]) == ("none", 100)
    cfg["mesh"].update(clean="Largest", clean_min_triangles=7)
    opt = ex.options(cfg, "mesh")
    assert (opt["clean"], opt["clean_min_triangles"]) == ("largest", 7)
    cfg["mesh"]["clean"] = None
    assert ex.options(cfg, "mesh")["clean"] == "none"
    assert "clean" not in ex.options(cfg, "pointcloud")
    for key, bad in (("clean", "biggest"), ("clean", "frustum"), ("clean_min_triangles", 0), ("clean_min_triangles", -1), ("clean_min_triangles", 2.5),
                     ("clean_min_triangles", "many"), ("clean_min_triangles", None)):
        with pytest.raises(ValueError, match=r"mesh\." + key + " = "):
            ex.options(dict(cfg, mesh=dict(dict(cfg["mesh"], clean="small"), **{key: bad})), "mesh")


def test_cabi_declares_and_binds_the_four_symbols():
    from mm3dgs_slam_amd import _lib
    h = open(os.path.join(ROOT, "include", "mm3dgs.h")).read()
    lib = _lib.load()
    for name in ("mm3dgs_mesh_clean_work_bytes", "mm3dgs_mesh_components", "mm3dgs_mesh_clean_plan", "mm3dgs_mesh_clean_emit"):
        assert re.search(r"\b" + name + r"\s*\(", h) and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert re.search(r"#define MM3DGS_MESH_CLEAN_SMALL 1\b", h) and re.search(r"#define MM3DGS_MESH_CLEAN_LARGEST 2\b", h) and mc.MODE_IDS == {"small": 1, "largest": 2}
    assert lib.mm3dgs_mesh_clean_work_bytes.restype is C.c_size_t
    for V, T in ((0, 0), (1, 1), (257, 255), (1 << 20, 1 << 21), (1 << 30, 1 << 30)):
        n = int(lib.mm3dgs_mesh_clean_work_bytes(V, T))
        assert n > 0 and n % 8 == 0 and n >= 4 * V, (V, T, n)
    for V, T in (((1 << 30) + 1, 3), (3, (1 << 30) + 1), (1 << 63, 0)):
        assert int(lib.mm3dgs_mesh_clean_work_bytes(V, T)) == 0, (V, T)
    # the host-side checks of the three calls: each of these is rejected before a pointer is looked at (nothing is launched, no GPU is touched)
    assert lib.mm3dgs_mesh_components((1 << 30) + 1, 0, None, None, None, None, None) == -1 and b"2^30" in lib.mm3dgs_last_error()
    assert lib.mm3dgs_mesh_components(0, 0, None, None, None, None, None) == -1 and b"NULL" in lib.mm3dgs_last_error()
    assert lib.mm3dgs_mesh_clean_plan(0, 0, None, None, None, 0, 1, None, None, None) == -1 and b"mode" in lib.mm3dgs_last_error()
    assert lib.mm3dgs_mesh_clean_plan(0, 0, None, None, None, 3, 1, None, None, None) == -1 and b"mode" in lib.mm3dgs_last_error()
    assert lib.mm3dgs_mesh_clean_plan(0, 0, None, None, None, 1, 0, None, None, None) == -1 and b"min_triangles" in lib.mm3dgs_last_error()
    assert lib.mm3dgs_mesh_clean_emit(0, 0, None, None, None, None, (1 << 31) + 1, None, 0, None, None, None) == -1 and b"2^31" in lib.mm3dgs_last_error()
    assert lib.mm3dgs_mesh_clean_emit(0, 0, None, None, None, None, 0, None, 0, None, None, None) == -1 and b"NULL" in lib.mm3dgs_last_error()


# ---- a device: cpu run with a blob planted in a corner of the volume ---------------------------------------------------------------------
MESH = {"voxel": 0.08, "every": 1, "export": False}
GEO = {"density": 400.0, "threshold": 0.05, "max_dist": 1.0}


def _cpu_slam(tmp, frames=4):
    """The stand-in run of `device: cpu` of tests/test_cull.py (32 x 48, the oracle rasterizer injected, 4 frames), run to its end."""
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


def _plant_blob(volume):
    """One inside sample at (1, 1, 1) in a known, outside 3 x 3 x 3 corner of the lattice: the box is grown by trunc + voxel = 5 voxels, so
    no surface comes near."""
    t = volume.tsdf_w
    corner = t[:4, :4, :4]
    assert bool((corner[..., 0][corner[..., 1] >= 1] > 0).all()), "the corner of the lattice holds a surface"
    t[:3, :3, :3, 0] = 1.0
    t[:3, :3, :3, 1] = np.maximum(t[:3, :3, :3, 1], 1.0)
    t[1, 1, 1, 0] = -0.5


def test_cpu_run_with_a_planted_blob(tmp_path, monkeypatch, capsys):
    slam, seq, cfg = _cpu_slam(tmp_path / "run")

    def export(name, **keys):
        slam.cfg["mesh"] = dict(MESH, **keys)
        out = slam.export_mesh(path=str(tmp_path / name))
        return out, (tmp_path / name / "mesh.ply").read_bytes()

    parent, b_parent = export("parent")                     # the call as it was before the keys existed
    none, b_none = export("none", clean="none", clean_min_triangles=100)
    assert b_none == b_parent and none["counters"] == parent["counters"] and "clean" not in none and "clean" not in none["counters"]
    capsys.readouterr()
    largest, b_largest = export("largest", clean="largest")
    line = capsys.readouterr().out
    rows, tris = ms.read_mesh_ply(parent["mesh"])
    want = mc.clean_host(rows, tris, "largest", 1)
    assert b_largest == open(ms.write_mesh_ply(str(tmp_path / "want.ply"), want[0], want[1]), "rb").read()
    assert largest["clean"] == dict(want[3], mode="largest", min_triangles=100, vertices=len(want[0]), triangles=len(want[1])) == largest["counters"]["clean"]
    assert largest["counters"]["vertices"] == len(rows) and want[3]["components"] > 1 and want[3]["components_kept"] == 1
    assert f"kept 1 of {want[3]['components']} components" in line and f"removed {want[3]['vertices_removed']} vertices" in line
    # the blob
    extract = ms.HostTsdfVolume.extract
    monkeypatch.setattr(ms.HostTsdfVolume, "extract", lambda self: (_plant_blob(self), extract(self))[1])
    blob, b_blob = export("blob")
    brows, btris = ms.read_mesh_ply(blob["mesh"])
    lo = np.asarray(blob["origin"])
    xyz = brows[:, :3].copy().view(np.float32).astype(np.float64)
    in_corner = ((xyz >= lo - 1e-6) & (xyz <= lo + 2 * MESH["voxel"] + 1e-6)).all(1)
    blob_tris = in_corner[btris].all(1)
    assert in_corner.sum() == len(brows) - len(rows) > 0 and blob_tris.sum() == len(btris) - len(tris) > 0 and not in_corner[btris[~blob_tris]].any()
    # without cleaning the file holds the blob, and only the blob is new
    shift = np.cumsum(~in_corner) - 1
    assert brows[~in_corner].tobytes() == rows.tobytes() and np.array_equal(shift[btris[~blob_tris]], tris)
    # clean: largest loses exactly the blob's triangles more: the same file as without the blob
    cleaned, b_cleaned = export("blob_largest", clean="largest")
    assert b_cleaned == b_largest
    ci, li = cleaned["clean"], largest["clean"]
    assert ci["components"] == li["components"] + 1 and ci["triangles_removed"] == li["triangles_removed"] + int(blob_tris.sum())
    assert ci["vertices_removed"] == li["vertices_removed"] + int(in_corner.sum()) and ci["vertices"] == li["vertices"] and ci["triangles"] == li["triangles"]
    # clean: small at the blob's size keeps it, one more drops it
    nb = int(blob_tris.sum())
    kept, b_kept = export("blob_small_keep", clean="small", clean_min_triangles=nb)
    dropped, b_dropped = export("blob_small_drop", clean="small", clean_min_triangles=nb + 1)
    krows, ktris = ms.read_mesh_ply(kept["mesh"])
    drows, dtris = ms.read_mesh_ply(dropped["mesh"])
    in_k = ((krows[:, :3].copy().view(np.float32) >= lo - 1e-6) & (krows[:, :3].copy().view(np.float32) <= lo + 2 * MESH["voxel"] + 1e-6)).all(1)
    assert in_k.sum() == in_corner.sum() and len(ktris) - len(dtris) == nb and len(krows) - len(drows) == in_corner.sum()
    assert drows.tobytes() == mc.clean_host(rows, tris, "small", nb + 1)[0].tobytes()
    # the evaluation: both meshes come cleaned from the builder, metrics.json says so; without the keys nothing changes
    monkeypatch.setattr(ms.HostTsdfVolume, "extract", extract)

    def evaluate(name, **keys):
        slam.cfg["mesh"] = dict(MESH, **keys)
        slam.cfg["geometry"] = dict(GEO, eval=False)
        out = slam.evaluate_geometry(path=str(tmp_path / name))
        return out, json.load(open(tmp_path / name / "metrics.json"))

    g_parent, m_parent = evaluate("g_parent")
    g_none, m_none = evaluate("g_none", clean="none")
    for f in ("metrics.json", "accuracy.ply", "completion.ply"):
        assert (tmp_path / "g_none" / f).read_bytes() == (tmp_path / "g_parent" / f).read_bytes(), f
    assert "mesh_clean" not in m_none and "mesh_clean" not in g_none
    g_on, m_on = evaluate("g_on", clean="largest")
    block = m_on["mesh_clean"]
    assert block["mode"] == "largest" and block["min_triangles"] == 100 and block["estimate"] == largest["clean"]
    sensor = ex.mesh_geometry(slam, dict(ex.options(dict(cfg, mesh=dict(MESH)), "mesh"), source="sensor"), ex.gt_poses(slam))[:2]
    ref = mc.clean_host(sensor[0], sensor[1], "largest", 1)
    assert block["reference"] == dict(ref[3], mode="largest", min_triangles=100, vertices=len(ref[0]), triangles=len(ref[1]))
    from mm3dgs_slam_amd import geometry as geo      # the scored point sets are the samples of the cleaned meshes
    assert m_on["n_estimate"] == geo.sample_mesh_host(want[0], want[1], GEO["density"], 0)[1]["samples"] != m_none["n_estimate"]
    assert m_on["n_reference"] == geo.sample_mesh_host(ref[0], ref[1], GEO["density"], 0)[1]["samples"]
    # a reference file is left as it is
    ref_file = ms.write_mesh_ply(str(tmp_path / "reference.ply"), sensor[0], sensor[1])
    slam.cfg["geometry"] = dict(GEO, eval=False, reference=ref_file)
    slam.cfg["mesh"] = dict(MESH, clean="largest")
    out = slam.evaluate_geometry(path=str(tmp_path / "g_file"))
    assert out["n_reference"] == m_none["n_reference"] and "reference" not in out["mesh_clean"] and out["mesh_clean"]["estimate"] == largest["clean"]


def test_cli_round_trips_a_file(tmp_path, capsys):
    case = CASES[IDS.index("marching tetrahedra: sphere and two blobs")]
    src = ms.write_mesh_ply(str(tmp_path / "in.ply"), case["rows"], case["triangles"])
    info = mc.main([src, str(tmp_path / "out.ply"), "--mode", "small", "--min-triangles", "25"])
    want = mc.clean_host(case["rows"], case["triangles"], "small", 25)
    rows, tris = ms.read_mesh_ply(str(tmp_path / "out.ply"))
    assert rows.tobytes() == want[0].tobytes() and tris.tobytes() == want[1].tobytes() and info == want[3] and info["components_kept"] == 2
    assert "kept 2 of 3 components" in capsys.readouterr().out
    # the cleaned file cleans to itself; the default mode is small with the placeholder threshold; a cloud is refused
    mc.main([str(tmp_path / "out.ply"), str(tmp_path / "again.ply"), "--mode", "largest"])
    assert len(ms.read_mesh_ply(str(tmp_path / "again.ply"))[1]) == 2652
    assert mc.main([src, str(tmp_path / "default.ply")])["components_kept"] == 1
    from mm3dgs_slam_amd import pointcloud as pc
    with pytest.raises(SystemExit, match="point cloud"):
        mc.main([pc.write_ply(str(tmp_path / "cloud.ply"), case["rows"]), str(tmp_path / "x.ply")])
