"""The mesh export on the host (mm3dgs_slam_amd/mesh.py): marching tetrahedra on analytic distance fields (closed surfaces, Euler
characteristic, distance to the true surface, enclosed volume), the integration of posed views against its formula, the PLY file, the config
block and the export of a `device: cpu` run.  Every test prints its figures (`MESHERR ...`, pytest -s) before it asserts."""
import os
import random

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import mesh as ms
from mm3dgs_slam_amd import pointcloud as pc
from tests import mesh_cases as cases
from tests import pointcloud_cases as pcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 17
DIMS = (N, N, N)


@pytest.fixture(scope="module")
def meshes():
    out = {}
    for kind in cases.KINDS:
        vol = cases.analytic_volume(kind, DIMS)
        out[kind] = (vol,) + ms.mesh_host(vol["tsdf_w"], vol["rgb_w"], vol["origin"], vol["voxel"])
    return out


def test_case_table_is_the_sixteen_cases_with_outward_normals():
    assert [len(c) for c in ms.CASE_TRIANGLES] == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]], dtype=np.float64)
    rng = np.random.default_rng(0)
    for m in range(1, 15):
        ins = [i for i in range(4) if (m >> i) & 1]
        out = [i for i in range(4) if not (m >> i) & 1]
        for tri in ms.CASE_TRIANGLES[m]:
            for _ in range(20):      # wherever the crossings sit on their edges, the normal points from the inside to the outside vertices
                p = []
                for e in tri:
                    a, b = ms.TET_EDGES[e]
                    assert (a in ins) != (b in ins)
                    t = rng.uniform(0.05, 0.95)
                    p.append(v[a] + t * (v[b] - v[a]))
                nrm = np.cross(p[1] - p[0], p[2] - p[0])
                assert all(nrm @ (v[o] - v[i]) > 0 for i in ins for o in out), (m, tri)
    # the six tetrahedra tile the cube: every one has volume 1/6 and the odd permutations are the mirrored ones
    for k in range(6):
        c = np.array([[(q >> a) & 1 for a in range(3)] for q in ms.TET_CORNERS[k]], dtype=np.float64)
        det = np.linalg.det(c[1:] - c[0])
        assert abs(abs(det) - 1.0) < 1e-12 and (det < 0) == ms.TET_ODD[k]


@pytest.mark.parametrize("kind", cases.KINDS)
def test_mesh_host_on_analytic_distance_fields(meshes, kind):
    vol, rows, tris, counters = meshes[kind]
    xyz = pc.rows_xyz(rows).astype(np.float64)
    topo = ms.mesh_topology(len(rows), tris)
    dist = np.abs(cases.distance(kind, DIMS, xyz))
    bound = np.sqrt(3.0) * vol["voxel"]      # a vertex sits on a lattice edge of at most that length, which the true surface crosses too
    print(f"MESHERR host {kind} {N}^3: {len(rows)} vertices, {len(tris)} triangles, {topo}, largest distance to the surface {dist.max() / vol['voxel']:.3f} voxel")
    assert counters.tolist() == [len(rows), len(tris), len(rows), len(tris), 0, 0, 0, 0] and len(tris) > 0
    assert topo["unreferenced"] == 0 and topo["repeated"] == 0
    assert bool((dist <= bound).all())
    assert 0 <= tris.min() and tris.max() < len(rows)
    if kind == "plane":
        assert topo["boundary"] > 0      # open: it leaves the lattice
        return
    assert topo["closed"] and topo["euler"] == (2 if kind == "sphere" else 0)
    vol_mesh = ms.signed_volume(xyz, tris)
    if kind == "sphere":
        r = cases.radii(kind, DIMS)
        lo, hi = (4.0 / 3.0 * np.pi * (r + s * bound) ** 3 for s in (-1, 1))
    else:
        R, r = cases.radii(kind, DIMS)
        lo, hi = (2.0 * np.pi ** 2 * R * (r + s * bound) ** 2 if r + s * bound > 0 else 0.0 for s in (-1, 1))
    print(f"MESHERR host {kind} volume {vol_mesh:.6f} in [{lo:.6f}, {hi:.6f}]")
    assert vol_mesh > 0 and lo <= vol_mesh <= hi
    # the normals point towards free space: at every triangle the true distance grows along the normal
    p = xyz[tris]
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    area = np.linalg.norm(nrm, axis=1)
    big = area > 1e-3 * vol["voxel"] ** 2
    c = p.mean(1)[big]
    step = 0.25 * vol["voxel"] * nrm[big] / area[big, None]
    assert bool((cases.distance(kind, DIMS, c + step) > cases.distance(kind, DIMS, c - step)).all())


def test_vertex_order_positions_and_colours_of_the_host_statement():
    vol = cases.analytic_volume("sphere", (5, 4, 3))
    rows, tris, _ = ms.mesh_host(vol["tsdf_w"], vol["rgb_w"], vol["origin"], vol["voxel"])
    T, C = vol["tsdf_w"][..., 0].astype(np.float64), vol["rgb_w"][..., :3].astype(np.float64)
    nx, ny, nz = vol["dims"]
    want = []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                for d in range(1, 8):
                    a, b, c = i + (d & 1), j + ((d >> 1) & 1), k + ((d >> 2) & 1)
                    if a >= nx or b >= ny or c >= nz or (T[k, j, i] < 0) == (T[c, b, a] < 0):
                        continue      # (every cube of this volume is valid)
                    t = T[k, j, i] / (T[k, j, i] - T[c, b, a])
                    pos = vol["origin"] + vol["voxel"] * (np.array([i, j, k]) + t * np.array([d & 1, (d >> 1) & 1, (d >> 2) & 1]))
                    want.append((pos, C[k, j, i] + t * (C[c, b, a] - C[k, j, i])))
    assert len(want) == len(rows) > 0
    assert np.array_equal(pc.rows_xyz(rows), np.array([w[0] for w in want]).astype(np.float32))
    assert np.array_equal(pc.rows_rgba(rows)[:, :3], pc.quantise_colour(np.array([w[1] for w in want]).astype(np.float32)))
    assert bool((pc.rows_rgba(rows)[:, 3] == 255).all())


def test_half_known_volume_gives_an_open_surface_with_every_vertex_referenced():
    vol = cases.analytic_volume("sphere", DIMS, half_known=True)
    rows, tris, _ = ms.mesh_host(vol["tsdf_w"], vol["rgb_w"], vol["origin"], vol["voxel"])
    topo = ms.mesh_topology(len(rows), tris)
    print(f"MESHERR host half-known sphere: {len(rows)} vertices, {len(tris)} triangles, {topo}")
    assert len(tris) > 0 and topo["boundary"] > 0 and topo["unreferenced"] == 0 and topo["repeated"] == 0
    assert float(pc.rows_xyz(rows)[:, 0].max()) <= vol["origin"][0] + vol["voxel"] * (N // 2 - 1) + 1e-6      # nothing beyond the last valid cube
    # min_weight decides what is known
    none = ms.mesh_host(vol["tsdf_w"], vol["rgb_w"], vol["origin"], vol["voxel"], min_weight=2.0)
    assert len(none[0]) == 0 and len(none[1]) == 0


def _plane_view(H, W, depth_value):
    v = pcases.plane_view(H, W)
    v["depth"][:] = np.float32(depth_value)
    v["pose"] = np.array([1, 0, 0, 0, 0, 0, 0], dtype=np.float32)      # camera = world
    return v


def test_integrate_host_reproduces_the_truncated_distance_of_a_fronto_parallel_plane():
    H, W, D = 17, 33, 2.0
    v = _plane_view(H, W, D)
    cam = v["cam"]
    nx, ny, nz = 40, 20, 30
    voxel, trunc = 0.0413, 0.2
    origin = np.array([-0.8, -0.4, 1.4])
    tsdf_w, rgb_w = ms.empty_volume(nx, ny, nz)
    n, g = ms.integrate_host(tsdf_w, rgb_w, v["color"], v["depth"], None, v["pose"], **cam, origin=origin, voxel=voxel, trunc=trunc, full=True)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    x, y, z = (origin[a] + voxel * q for a, q in enumerate((i, j, k)))
    u, w = np.floor(cam["fx"] * x / z + cam["cx"] + 0.5), np.floor(cam["fy"] * y / z + cam["cy"] + 0.5)
    inside_image = (u >= 0) & (u < W) & (w >= 0) & (w < H)
    seen = inside_image & (D - z >= -trunc)
    print(f"MESHERR integrate plane: {int(seen.sum())} of {seen.size} samples seen, {n[1]} with colour, {int((~inside_image).sum())} outside the image")
    assert 0 < seen.sum() < seen.size and (~inside_image).any() and (D - z < -trunc).any() and (D - z > trunc).any()
    assert np.array_equal(g["upd"], seen) and n == (int(seen.sum()), int((seen & (D - z <= trunc)).sum()))
    assert np.array_equal(tsdf_w[..., 1], seen.astype(np.float32))
    assert np.array_equal(tsdf_w[..., 0], np.where(seen, np.minimum(1.0, (D - z) / trunc), 0.0).astype(np.float32))
    assert not tsdf_w[~seen].any() and not rgb_w[~seen].any()
    col = seen & (D - z <= trunc)
    assert np.array_equal(rgb_w[..., 3], col.astype(np.float32))
    ui, wi = np.where(col, u, 0).astype(int), np.where(col, w, 0).astype(int)
    for c in range(3):
        assert np.array_equal(rgb_w[..., c], np.where(col, v["color"][c][wi, ui], 0).astype(np.float32))
    # a second view at another depth: the two truncated distances average, the weights count
    v2 = _plane_view(H, W, D + 0.05)
    before = tsdf_w.copy()
    ms.integrate_host(tsdf_w, rgb_w, v2["color"], v2["depth"], None, v2["pose"], **cam, origin=origin, voxel=voxel, trunc=trunc)
    seen2 = inside_image & (np.float64(np.float32(D + 0.05)) - z >= -trunc)
    both = seen & seen2
    s2 = np.minimum(1.0, (np.float64(np.float32(D + 0.05)) - z) / trunc)
    assert both.any() and np.array_equal(tsdf_w[..., 1], seen.astype(np.float32) + seen2.astype(np.float32))
    assert np.array_equal(tsdf_w[..., 0][both], ((before[..., 0][both].astype(np.float64) + s2[both]) / 2.0).astype(np.float32))
    # the mesh of the two fused views is the plane between them
    rows, tris, _ = ms.mesh_host(tsdf_w, rgb_w, origin, voxel, min_weight=2.0)
    zs = pc.rows_xyz(rows)[:, 2]
    assert len(tris) > 0 and float(np.abs(zs - (D + 0.025)).max()) < 1e-3


@pytest.mark.parametrize("pattern", pcases.PATTERNS)
def test_integrate_host_follows_the_point_clouds_validity_patterns(pattern):
    H, W = 17, 33
    case = cases.integrate_case((17, 9, 6), H, W, pattern)
    v = case["views"][0]
    tsdf_w, rgb_w, counters, excluded = cases.integrate_all(case)
    ok = pc.valid_mask(v["depth"], v["sil"], v["sil_min"], v["depth_max"])
    nx, ny, nz = case["dims"]
    tw, rw = ms.empty_volume(nx, ny, nz)
    _, g = ms.integrate_host(tw, rw, v["color"], v["depth"], v["sil"], v["pose"], **v["cam"], origin=case["origin"], voxel=case["voxel"], trunc=case["trunc"],
                             sil_min=v["sil_min"], depth_max=v["depth_max"], full=True)
    front = g["z"] > 0
    u, w = np.floor(g["fu"]), np.floor(g["fv"])
    inside_image = front & (u >= 0) & (u < W) & (w >= 0) & (w < H)
    pix_ok = np.zeros_like(inside_image)
    pix_ok[inside_image] = ok[w[inside_image].astype(int), u[inside_image].astype(int)]
    print(f"MESHERR integrate {pattern}: {counters[1]} distance and {counters[2]} colour updates of {nx * ny * nz} samples, {int(inside_image.sum())} inside the image, "
          f"{int(pix_ok.sum())} on valid pixels, {int(excluded.sum())} excluded")
    assert not tsdf_w[~pix_ok].any() and not rgb_w[~pix_ok].any()      # outside the image or behind an invalid pixel: untouched
    assert np.array_equal(tsdf_w[..., 1] > 0, g["upd"]) and bool((g["upd"] <= pix_ok).all())
    assert counters == [1, int(g["upd"].sum()), int(g["col"].sum())]
    if pattern == "none":
        assert counters[1] == 0
    if pattern in ("all", "checker", "planted", "sil_edge", "depth_max_edge"):
        assert 0 < counters[2] < counters[1] < nx * ny * nz and inside_image.sum() < nx * ny * nz
        assert (pix_ok & ~g["upd"]).any()      # behind -trunc


def test_generic_poses_leave_no_sample_on_a_rounding_boundary():
    """The exclusion of tests/test_gpu_mesh.py (a pixel coordinate within 1e-9 of a rounding boundary, an sdf within 1e-9 trunc of +-trunc),
    counted on every integration case with the host statement alone: the cap is 0.1 % of the samples, generic poses leave out none."""
    worst = 0
    for dims in cases.INTEGRATE_SHAPES:
        for H, W in cases.VIEW_SHAPES:
            for pattern, n_views in (("all", 3), ("planted", 1), ("sil_edge", 1), ("depth_max_edge", 1)):
                excluded = cases.integrate_all(cases.integrate_case(dims, H, W, pattern, n_views))[3]
                assert excluded.sum() <= 1e-3 * excluded.size, (dims, H, W, pattern)
                worst = max(worst, int(excluded.sum()))
    print(f"MESHERR excluded samples over all integration cases: at most {worst}")
    assert worst == 0


def test_mesh_ply_round_trips_byte_for_byte(tmp_path, meshes):
    _, rows, tris, _ = meshes["sphere"]
    path = ms.write_mesh_ply(str(tmp_path / "mesh.ply"), rows, tris)
    raw = open(path, "rb").read()
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(rows)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face {len(tris)}\n"
              "property list uchar int vertex_indices\nend_header\n").encode("ascii")
    assert raw[:len(header)] == header and len(raw) == len(header) + 16 * len(rows) + 13 * len(tris)
    assert raw[len(header):len(header) + 16 * len(rows)] == rows.tobytes()
    first = raw[len(header) + 16 * len(rows):][:13]
    assert first[0] == 3 and np.frombuffer(first[1:], dtype="<i4").tolist() == tris[0].tolist()
    r2, t2 = ms.read_mesh_ply(path)
    assert r2.dtype == np.int32 and t2.dtype == np.int32 and r2.tobytes() == rows.tobytes() and t2.tobytes() == tris.tobytes()
    again = ms.write_mesh_ply(str(tmp_path / "again.ply"), torch.from_numpy(r2), torch.from_numpy(t2))      # tensors too
    assert open(again, "rb").read() == raw
    e = ms.read_mesh_ply(ms.write_mesh_ply(str(tmp_path / "empty.ply"), rows[:0], tris[:0]))
    assert e[0].shape == (0, 4) and e[1].shape == (0, 3)
    with pytest.raises(ValueError, match="not a mesh"):
        ms.read_mesh_ply(pc.write_ply(str(tmp_path / "cloud.ply"), rows))


def test_config_block_is_off_by_default():
    from mm3dgs_slam_amd.config import default_config, utmm_config
    for cfg in (default_config(), utmm_config()):
        assert cfg["mesh"] == {"export": False, "every": None, "voxel": 0.02, "trunc": 0, "source": "render", "sil_min": 0.99, "max_depth": 0,
                               "min_weight": 1, "bounds": None, "max_voxels": 1 << 28}


def test_cabi_declares_and_binds_the_five_symbols():
    import ctypes as C
    import re
    from mm3dgs_slam_amd import _lib
    h = open(os.path.join(ROOT, "include", "mm3dgs.h")).read()
    names = ("mm3dgs_tsdf_reset", "mm3dgs_tsdf_integrate", "mm3dgs_tsdf_mesh_work_bytes", "mm3dgs_tsdf_mesh_plan", "mm3dgs_tsdf_mesh_emit")
    lib = _lib.load()
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", h) and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert lib.mm3dgs_tsdf_mesh_work_bytes.restype is C.c_size_t
    for dims in ((2, 2, 2), (65, 65, 65), (1024, 1024, 1024)):
        n = int(lib.mm3dgs_tsdf_mesh_work_bytes(*dims))
        assert n > 0 and n % 8 == 0 and n >= 11 * dims[0] * dims[1] * dims[2], (dims, n)
    for dims in ((1, 5, 5), (5, 1, 5), (5, 5, 1), (0, 5, 5), (-2, 5, 5), (1025, 1024, 1024), (1 << 16, 1 << 16, 2)):
        assert int(lib.mm3dgs_tsdf_mesh_work_bytes(*dims)) == 0, dims


def _cpu_slam(tmp, mesh):
    """The stand-in run of `device: cpu` (32 x 48, 3 frames, the oracle rasterizer injected, as tests/test_pointcloud.py builds it), run to
    its end."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.renderer import Renderer
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from oracle.raster_ref import RefRasterizer
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device="cpu", height=32, width=48, tracking={"iters": 2}, mapping={"iters": 3, "kf_every": 2}, outputdir=str(tmp), mesh=mesh)
    seq = SyntheticSequence(cfg, 3, 600, seed=2, renderer=Renderer(cfg, rasterizer_cls=RefRasterizer))
    slam = SLAM(cfg, seq, rasterizer_cls=RefRasterizer)
    slam.run()      # with mesh.export the run writes mesh/mesh.ply behind results.npz
    return slam, seq, cfg


def test_export_of_a_cpu_run_goes_through_the_host_statement(tmp_path):
    MESH = {"voxel": 0.08, "every": 1}
    slam, seq, cfg = _cpu_slam(tmp_path / "on", dict(MESH, export=True))
    out = slam.mesh_export
    assert out is not None and (tmp_path / "on" / "mesh" / "mesh.ply").exists()
    c = out["counters"]
    on_poses = [p.detach().numpy().copy() for p in slam.estimate_pose_list]
    print(f"MESHERR cpu export: {c}, lattice {out['lattice']}")
    assert out["mesh"] == str(tmp_path / "on" / "mesh" / "mesh.ply")
    rows, tris = ms.read_mesh_ply(out["mesh"])
    assert len(rows) == c["vertices"] > 0 and len(tris) == c["triangles"] > 0 and c["views"] == 3 and c["dist_updates"] >= c["colour_updates"] > 0
    topo = ms.mesh_topology(len(rows), tris)
    assert topo["unreferenced"] == 0 and topo["repeated"] == 0
    # by hand: the same views through the host statement over the lattice the export reports
    nx, ny, nz = out["lattice"]
    assert abs(out["trunc"] - 4 * 0.08) < 1e-12 and np.allclose(np.asarray(out["origin"]) / 0.08, np.round(np.asarray(out["origin"]) / 0.08), atol=1e-9)
    tsdf_w, rgb_w = ms.empty_volume(nx, ny, nz)
    box_lo, box_hi = np.full(3, np.inf), np.full(3, -np.inf)
    with torch.no_grad():
        for i in range(3):
            r = slam.renderer.render(slam.gaussians, camera_pose=slam.estimate_pose_list[i])
            cam = {k: cfg["cam"][k] for k in ("fx", "fy", "cx", "cy")}
            ms.integrate_host(tsdf_w, rgb_w, r["render"], r["depth"][0], r["depth"][1], slam.estimate_pose_list[i], **cam, origin=out["origin"], voxel=0.08,
                              trunc=out["trunc"], sil_min=0.99)
            pts = pc.rows_xyz(pc.backproject_host(r["render"], r["depth"][0], r["depth"][1], slam.estimate_pose_list[i], **cam, sil_min=0.99))
            box_lo, box_hi = np.minimum(box_lo, pts.min(0)), np.maximum(box_hi, pts.max(0))
    want = ms.mesh_host(tsdf_w, rgb_w, out["origin"], 0.08, 1.0)
    assert want[0].tobytes() == rows.tobytes() and want[1].tobytes() == tris.tobytes()
    # the lattice holds the box of the lifted points, grown by trunc + voxel
    hi = np.asarray(out["origin"]) + 0.08 * (np.array(out["lattice"]) - 1)
    assert bool((np.asarray(out["origin"]) <= box_lo - 0.4 + 1e-5).all()) and bool((hi >= box_hi + 0.4 - 1e-5).all())
    assert bool((np.asarray(out["origin"]) > box_lo - 0.4 - 0.08 - 1e-5).all())
    # export: false runs no new code and leaves the same poses and results.npz
    off, _, _ = _cpu_slam(tmp_path / "off", dict(MESH, export=False))
    a, b = np.load(tmp_path / "on" / "results.npz", allow_pickle=True), np.load(tmp_path / "off" / "results.npz", allow_pickle=True)
    assert list(a.keys()) == list(b.keys()) and a["pose_est"].shape == (3, 7) and a["pose_est"].tobytes() == b["pose_est"].tobytes()
    assert all(np.array_equal(p, q) for p, q in zip(on_poses, [p.numpy() for p in off.estimate_pose_list]))
    assert off.mesh_export is None and not (tmp_path / "off" / "mesh").exists()
    # given bounds; a lattice above max_voxels is an error that names the box, the voxel size and the key
    cfg["mesh"]["bounds"] = [float(v) for v in np.concatenate([box_lo, box_hi])]
    small = slam.export_mesh(path=str(tmp_path / "bounds"))
    assert all(n >= 2 for n in small["lattice"]) and small["lattice"] != out["lattice"]
    cfg["mesh"]["bounds"] = None
    cfg["mesh"]["max_voxels"] = 1000
    with pytest.raises(ValueError, match=r"mesh\.max_voxels = 1000.*mesh\.voxel"):
        slam.export_mesh()
    with pytest.raises(ValueError, match=r"lattice of \d+ x \d+ x \d+ samples"):
        slam.export_mesh(voxel=0.05)
    with pytest.raises(ValueError, match="render / sensor"):
        slam.export_mesh(source="cloud")
    # the point cloud export shares the view loop and writes what it wrote
    cfg["pointcloud"].update(voxel=0.05, max_points=4096)
    cloud = slam.export_pointcloud(every=1)
    assert cloud["counters"]["views"] == 3 and cloud["counters"]["rows"] > 0
