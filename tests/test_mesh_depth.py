"""mesh_depth.render_host / compare_rows_host, the float64 statement the kernels of csrc/meshdepth.hip are held to, checked on its own: the
rectangle rule against the evaluation of every triangle on every pixel, analytic scenes (a tessellated plane without cracks, a floor that
crosses the camera plane, windings, permutations, every class of triangle, the bounds and a tie), the comparison row on every combination of
valid and invalid pixels, the options, and a `device: cpu` run that writes the depth L1 and culls against the rendered reference.

Bars.  A depth of the analytic scenes: |d - z| <= 2^-22 z -- the one rounding to float32 is at most 2^-24 relative, the double error is far
below that, which leaves a factor of 4.  The "kernel" sum order against numpy's: relative n 2^-52 -- the terms are non-negative, so no
reordering of n of them can cost more.  Everything else is exact.  Every test prints its figures (`MDERR ...`, pytest -s) before it asserts."""
import json
import random

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import cull as cl, export as ex, mesh as ms, mesh_depth as md, pointcloud as pc
from tests import mesh_depth_cases as cases

REL = 2.0 ** -22


def _render(s, **kw):
    return md.render_host(s["rows"], s["tris"], **dict(cases.args(s), **kw))


@pytest.mark.parametrize("s", cases.host_scenes(), ids=lambda s: s["name"])
def test_rectangles_change_nothing(s):
    d, t, c = _render(s)
    df, tf, cf = _render(s, full=True)
    print(f"MDERR rect {s['name']}: counters {c.tolist()}, full {cf.tolist()}; {int((t != tf).sum())} winners differ")
    assert d.tobytes() == df.tobytes() and np.array_equal(t, tf)
    assert c[[0, 1, 2, 3, 6]].tolist() == cf[[0, 1, 2, 3, 6]].tolist() and cf[4] == cf[5] == 0 and c[7] == 0
    assert c[1] + c[2] + c[3] == len(s["tris"]) and c[6] == int((t >= 0).sum()) and bool(((d == 0) == (t < 0)).all())
    st = md.setup_host(s["rows"], s["tris"], s["pose"], s["H"], s["W"], s["fx"], s["fy"], s["cx"], s["cy"], s["near"])
    assert c[4] == md.tile_pairs(st["rect"]) and c[5] == 0
    need = int(c[4])
    if need > 1:
        assert _render(s, max_pairs=need - 1)[2][4:6].tolist() == [need - 1, 1]


def test_tessellated_plane_has_no_cracks():
    s = cases.plane_grid()
    d, t, c = _render(s)
    u0, u1, v0, v1 = s["outline"]
    want = np.zeros((s["H"], s["W"]), dtype=bool)
    want[v0:v1 + 1, u0:u1 + 1] = True
    err = float(np.abs(d[want].astype(np.float64) - 2.0).max())
    print(f"MDERR plane: {int((t >= 0).sum())} hits of {int(want.sum())} wanted, {int(((t >= 0) != want).sum())} differ; max |d - 2| {err:.3e} (bar {REL * 2:.3e})")
    assert np.array_equal(t >= 0, want)      # the outline's own pixels, every shared edge and every vertex on a pixel centre included
    assert err <= REL * 2.0 and c.tolist()[:4] == [1, 128, 0, 0]
    assert len(np.unique(t[want])) > 100      # the quads' own triangles, not one that leaks over the rest


def test_floor_across_the_camera_plane():
    s = cases.floor()
    d, t, c = _render(s)
    v = np.arange(s["H"], dtype=np.float64)
    with np.errstate(divide="ignore"):
        z = s["fy"] / (v - s["cy"])
    rows = (v > s["cy"]) & (z <= 10.0)
    err = float((np.abs(d[rows].astype(np.float64) - z[rows, None]) / z[rows, None]).max())
    print(f"MDERR floor: {int((t >= 0).sum())} hits, rows {np.flatnonzero(rows)[[0, -1]].tolist()}; max relative error {err:.3e} (bar {REL:.3e}); counters {c.tolist()}")
    assert int(rows.sum()) * s["W"] == 1280 and c[6] == 1280
    assert np.array_equal(t >= 0, np.repeat(rows[:, None], s["W"], 1)) and err <= REL
    assert c.tolist()[:4] == [1, 2, 0, 0]


@pytest.mark.parametrize("s", [cases.plane_grid(), cases.floor(), cases.random_scene(60, seed=2), cases.stacked(7, n=30)], ids=lambda s: s["name"])
def test_winding_and_order_change_no_byte_of_the_depth(s):
    d, t, c = _render(s)
    dr, tr, cr = md.render_host(s["rows"], s["tris"][:, ::-1].copy(), **cases.args(s))
    assert dr.tobytes() == d.tobytes() and np.array_equal(tr, t) and np.array_equal(c, cr)
    perm = np.random.default_rng(5).permutation(len(s["tris"]))
    dp, tp, cp = md.render_host(s["rows"], s["tris"][perm], **cases.args(s))      # triangle k of the permuted mesh is triangle perm[k]
    assert dp.tobytes() == d.tobytes() and cp[[0, 1, 2, 3, 6]].tolist() == c[[0, 1, 2, 3, 6]].tolist()
    hit = t >= 0
    assert np.array_equal(tp >= 0, hit)
    # (two triangles at the very same depth on a pixel would make the lower index win in either order: the scenes here have none off an edge)
    same = perm[tp[hit]] == t[hit]
    print(f"MDERR permutation {s['name']}: {int(hit.sum())} hits, {int((~same).sum())} winners that differ (pixels on a shared edge)")
    z_tie = ~same
    if z_tie.any():      # a pixel exactly on a shared edge: both triangles give one depth, and each order takes its own lower index
        assert int(z_tie.sum()) <= int(hit.sum()) // 4
        assert bool((np.minimum(perm[tp[hit]][z_tie], t[hit][z_tie]) == t[hit][z_tie]).all())


def test_every_class_of_triangle():
    s, want, hitters = cases.classification()
    st = md.setup_host(s["rows"], s["tris"], s["pose"], s["H"], s["W"], s["fx"], s["fy"], s["cx"], s["cy"], s["near"])
    d, t, c = _render(s)
    print(f"MDERR classes: {st['cls'].tolist()} (want {want}); counters {c.tolist()}; winners {np.unique(t).tolist()}")
    assert st["cls"].tolist() == want and c.tolist()[:4] == [1, want.count(0), want.count(1), want.count(2)]
    assert np.unique(t[t >= 0]).tolist() == hitters and c[6] > 50
    assert bool((d[t >= 0] == np.float32(3.0)).all())


def test_near_and_far_on_and_one_ulp_beside_the_bound():
    for s, drawn, behind, hits in cases.bound_scenes():
        d, t, c = _render(s)
        print(f"MDERR bound {s['name']}: counters {c.tolist()}")
        assert c.tolist()[:4] == [1, drawn, 0, behind] and (c[6] > 50) == hits and (hits or c[6] == 0), s["name"]
        if hits:
            assert bool((d[t >= 0] == pc.rows_xyz(s["rows"])[0, 2]).all()), s["name"]      # exact arithmetic: the float32 depth is the plane's


def test_coplanar_triangles_the_lower_index_wins():
    for s in cases.tie_scenes():
        d, t, c = _render(s)
        alone = [md.render_host(s["rows"], s["tris"][k:k + 1], **cases.args(s))[1] >= 0 for k in (0, 1)]
        both = alone[0] & alone[1]
        print(f"MDERR {s['name']}: {int(both.sum())} shared pixels, winners there {np.unique(t[both]).tolist()}")
        assert int(both.sum()) > 20 and bool((t[both] == 0).all()) and bool((t[alone[1] & ~alone[0]] == 1).all())
        assert bool((d[alone[0] | alone[1]] == np.float32(3.0)).all())


def test_rejected_arguments():
    s = cases.floor()
    for bad in (dict(near=-1.0), dict(far=float("nan")), dict(far=float("inf")), dict(fx=0.0), dict(H=0), dict(cx=float("nan"))):
        with pytest.raises(ValueError):
            _render(s, **bad)
    with pytest.raises(ValueError, match="CUDA device"):
        md.MeshDepth(s["rows"], s["tris"], 48, 64, 32.0, 32.0, 32.0, 24.0, device="cpu")
    with pytest.raises(ValueError):
        md.compare_rows_host(np.zeros((2, 3), dtype=np.float32), np.zeros((3, 2), dtype=np.float32))


# ---- the comparison ------------------------------------------------------------------------------------------------------------------------
def test_compare_rows_every_combination():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    a = np.array([[1.0, 2.0, nan, inf, 0.0, -1.0, 3.0, 3.0, 3.0, 3.0, 3.0, nan, 4.5]], dtype=np.float32)
    b = np.array([[1.5, 2.0, 1.0, 1.0, 1.0, 1.0, nan, inf, 0.0, -2.0, -inf, -0.0, 2.5]], dtype=np.float32)
    row = md.compare_rows_host(a, b)[0]
    print(f"MDERR compare row {row.tolist()}")
    assert row[[0, 4, 5, 6, 7]].tolist() == [3, 4, 5, 1, 0]
    assert row[1] == (0.5 + 0.0 + 2.0) / 3 and row[2] == np.sqrt((0.25 + 4.0) / 3) and row[3] == 2.0
    assert md.compare_rows_host(a, b, "kernel")[0].tolist() == row.tolist()      # 13 small dyadic terms: every order is exact
    empty = md.compare_rows_host(np.array([[nan, 1.0, 0.0]], dtype=np.float32), np.array([[1.0, -1.0, inf]], dtype=np.float32))[0]
    assert empty.tolist() == [0, 0, 0, 0, 1, 1, 1, 0]
    stack = md.compare_rows_host(np.stack([a, a]), np.stack([b, a]))
    assert stack.shape == (2, 8) and stack[0].tolist() == row.tolist() and stack[1].tolist() == [8, 0, 0, 0, 0, 0, 5, 0]


@pytest.mark.parametrize("hw", ((1, 1), (17, 33), (48, 64), (120, 160)))
def test_compare_rows_kernel_order_against_numpy(hw):
    a, b = cases.depth_pair(*hw, seed=hw[0])
    k, n = md.compare_rows_host(a, b, "kernel")[0], md.compare_rows_host(a, b)[0]
    bar = max(n[0], 1) * 2.0 ** -52
    rel = [abs(k[i] - n[i]) / n[i] if n[i] else 0.0 for i in (1, 2)]
    print(f"MDERR compare {hw}: n {int(n[0])}, only {int(n[4])} / {int(n[5])}, neither {int(n[6])}; mean {k[1]!r} / {n[1]!r}, rms {k[2]!r} / {n[2]!r}; relative {rel} (bar {bar:.3e})")
    assert k[[0, 3, 4, 5, 6, 7]].tolist() == n[[0, 3, 4, 5, 6, 7]].tolist() and n[0] + n[4] + n[5] + n[6] == hw[0] * hw[1]
    assert max(rel) <= bar
    if hw[0] > 1:
        assert min(n[0], n[4], n[5], n[6]) > 0


def test_depth_l1_on_the_host():
    s = cases.plane_grid()
    moved = s["rows"].copy()
    moved[:, 2] = (pc.rows_xyz(s["rows"])[:, 2] + np.float32(0.25)).view(np.int32)      # the same surface 25 cm farther
    behind = np.array([1, 0, 0, 0, 0, 0, -50.0], dtype=np.float32)                       # a view that sees neither
    table, summary = md.depth_l1((moved, s["tris"]), (s["rows"], s["tris"]), [s["pose"], behind, s["pose"]], s["H"], s["W"], cases.CAM, device="cpu")
    print(f"MDERR depth_l1 host: {json.dumps(summary)}")
    assert table.shape == (3, 8) and summary["views"] == 3 and summary["empty_views"] == 1
    assert abs(summary["mean"] - 0.25) <= REL * 2.25 and abs(summary["pooled"] - 0.25) <= REL * 2.25 and abs(summary["rmse"] - 0.25) <= REL * 2.25
    assert 0 < summary["coverage"] < 1 and summary["counters"]["reference"]["views"] == 3 and summary["counters"]["reference"]["behind"] == 128
    assert table[1].tolist() == [0, 0, 0, 0, 0, 0, s["H"] * s["W"], 0]
    json.dumps(summary)


# ---- options and the stage -----------------------------------------------------------------------------------------------------------------
def test_options_pin_and_validate_the_depth_keys():
    from mm3dgs_slam_amd.config import GEOMETRY_DEPTH, default_config
    assert GEOMETRY_DEPTH == {"depth_l1": False, "cull_depth": "sensor", "depth_max_pairs": 1 << 25}
    cfg = default_config(device="cpu")
    assert not set(GEOMETRY_DEPTH) & set(cfg["geometry"])
    opt = ex.options(cfg, "geometry")
    assert all(opt[k] == v for k, v in GEOMETRY_DEPTH.items())
    cfg["geometry"] = dict(cfg["geometry"], depth_l1=True, cull_depth="Reference", depth_max_pairs=1000)
    opt = ex.options(cfg, "geometry")
    assert (opt["depth_l1"], opt["cull_depth"], opt["depth_max_pairs"]) == (True, "reference", 1000)
    for bad, text in ((dict(cull_depth="lidar"), r"geometry\.cull_depth = 'lidar' \(sensor / reference\)"), (dict(depth_max_pairs=0), r"geometry\.depth_max_pairs"),
                      (dict(depth_max_pairs=(1 << 31) + 1), r"geometry\.depth_max_pairs"), (dict(depth_max_pairs=2.5), r"geometry\.depth_max_pairs"),
                      (dict(depth_max_pairs=True), r"geometry\.depth_max_pairs")):
        with pytest.raises(ValueError, match=text):
            ex.options(dict(cfg, geometry=dict(cfg["geometry"], **bad)), "geometry")


MESH = {"voxel": 0.08, "every": 1, "export": False}
GEO = {"density": 400.0, "threshold": 0.05, "max_dist": 1.0}


@pytest.fixture(scope="module")
def cpu_run(tmp_path_factory):
    """The stand-in run of `device: cpu` of tests/test_cull.py (32 x 48, the oracle rasterizer injected), 4 frames, run to its end."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.renderer import Renderer
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from oracle.raster_ref import RefRasterizer
    tmp = tmp_path_factory.mktemp("mesh_depth_run")
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device="cpu", height=32, width=48, tracking={"iters": 2}, mapping={"iters": 3, "kf_every": 2}, outputdir=str(tmp), mesh=dict(MESH),
                         geometry=dict(GEO, eval=False))
    seq = SyntheticSequence(cfg, 4, 600, seed=2, renderer=Renderer(cfg, rasterizer_cls=RefRasterizer))
    slam = SLAM(cfg, seq, rasterizer_cls=RefRasterizer)
    slam.run()
    return slam, seq, cfg, tmp


def _evaluate(slam, tmp, name, **keys):
    slam.cfg["geometry"] = dict(GEO, eval=False, **keys)
    out = slam.evaluate_geometry(path=str(tmp / name))
    return out, json.load(open(tmp / name / "metrics.json"))


def test_cpu_run_writes_the_depth_l1_and_changes_nothing_else(cpu_run):
    slam, seq, cfg, tmp = cpu_run
    off, m_off = _evaluate(slam, tmp, "off")
    on, m_on = _evaluate(slam, tmp, "on", depth_l1=True)
    defaults, m_def = _evaluate(slam, tmp, "defaults", depth_l1=False, cull_depth="sensor", depth_max_pairs=1 << 25)
    for f in ("metrics.json", "accuracy.ply", "completion.ply"):
        assert (tmp / "defaults" / f).read_bytes() == (tmp / "off" / f).read_bytes(), f
    for f in ("accuracy.ply", "completion.ply"):
        assert (tmp / "on" / f).read_bytes() == (tmp / "off" / f).read_bytes(), f
    d = m_on.pop("depth_l1")
    assert "depth_l1" not in m_off and m_on == m_off and not (tmp / "off" / "depth_l1.npz").exists()
    rest = tmp / "on" / "rest.json"      # the file without the entry, written as the stage writes it
    with open(rest, "w") as fh:
        json.dump(m_on, fh, indent=1, sort_keys=True)
        fh.write("\n")
    assert rest.read_bytes() == (tmp / "off" / "metrics.json").read_bytes()
    z = np.load(tmp / "on" / "depth_l1.npz")
    print(f"MDERR cpu run: depth_l1 {json.dumps(d)}; table {z['table'].tolist()}")
    assert z["frames"].tolist() == [0, 1, 2, 3] and z["table"].shape == (4, 8) and d["views"] == 4 and d["empty_views"] == 0
    assert 0 < d["mean"] < 0.5 and d["mean"] <= d["rmse"] <= d["max"] and 0 < d["coverage"] <= 1
    assert d["counters"]["estimate"]["views"] == d["counters"]["reference"]["views"] == 4 and d["counters"]["estimate"]["dropped"] == 0
    # the table is the statement's, for the meshes and views the stage uses
    block = ex.options(slam.cfg, "mesh")
    gt = ex.gt_poses(slam)
    est, ref = ex.mesh_geometry(slam, block)[:2], ex.mesh_geometry(slam, dict(block, source="sensor"), gt)[:2]
    table, summary = md.depth_l1(est, ref, [gt[i] for i in range(4)], 32, 48, slam.cfg["cam"], device="cpu")
    assert table.tobytes() == z["table"].tobytes() and summary["mean"] == d["mean"]
    # refused: a point cloud on either side
    with pytest.raises(ValueError, match=r"geometry\.depth_l1"):
        _evaluate(slam, tmp, "x", depth_l1=True, estimate="pointcloud")
    cloud = pc.write_ply(str(tmp / "cloud.ply"), pc.as_np(ref[0], np.int32))
    with pytest.raises(ValueError, match=r"geometry\.depth_l1"):
        _evaluate(slam, tmp, "x", depth_l1=True, reference=cloud)


def test_cpu_run_culls_against_the_rendered_reference_without_sensor_depth(cpu_run):
    slam, seq, cfg, tmp = cpu_run
    block = ex.options(slam.cfg, "mesh")
    gt = ex.gt_poses(slam)
    rows, tris = ex.mesh_geometry(slam, dict(block, source="sensor"), gt)[:2]
    ref_file = ms.write_mesh_ply(str(tmp / "reference.ply"), rows, tris)
    sensor, m_sensor = _evaluate(slam, tmp, "sensor", cull="occlusion", reference=ref_file)

    class NoDepth:
        def __len__(self):
            return len(seq)

        def __getitem__(self, i):
            c, _, p = seq[i]
            return c, None, p
    slam.seq = NoDepth()
    try:
        with pytest.raises(ValueError, match="frame 0 has no sensor depth"):
            _evaluate(slam, tmp, "x", cull="occlusion", reference=ref_file)
        with pytest.raises(ValueError, match=r'geometry\.cull_depth "reference"'):
            _evaluate(slam, tmp, "x", cull="occlusion", cull_depth="reference", reference=str(tmp / "cloud.ply"))
        out, m = _evaluate(slam, tmp, "rendered", cull="occlusion", cull_depth="reference", reference=ref_file, depth_l1=True)
        spec = ex.cull_views(slam, ex.options(slam.cfg, "geometry"), block, (rows, tris))
    finally:
        slam.seq = seq
    c = m["cull"]
    print(f"MDERR cpu cull_depth reference: {json.dumps(c)}; with sensor depth {json.dumps(m_sensor['cull'])}")
    assert c["mode"] == "occlusion" and c["views"] == 4 and 0 < c["reference"]["kept"] <= c["reference"]["rows"] and 0 < c["estimate"]["kept"] < c["estimate"]["rows"]
    assert m["depth_l1"]["views"] == 4
    # each view's depth image is the reference mesh rendered at the frame's ground-truth pose, and the kept rows are cull_host's for them
    cam = slam.cfg["cam"]
    for (depth, pose), g in zip(spec["views"], gt):
        want = md.render_host(rows, tris, g, 32, 48, cam["fx"], cam["fy"], cam["cx"], cam["cy"])[0]
        assert np.asarray(depth).tobytes() == want.tobytes() and torch.equal(pose, g)
    for side in ("estimate", "reference"):
        assert out["cull"][side]["kept"] == len(out[side + "_rows"])
    samples = pc.as_np(out["reference_rows"], np.int32)
    again = cl.apply_host(samples, spec)
    assert again[0].tobytes() == samples.tobytes()      # culling the kept rows again keeps them all
