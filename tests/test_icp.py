"""The host statement of the registration step (mm3dgs_slam_amd/geometry.py: icp_host, _horn_solve, move_rows_host, register): the corner
scene's three motions recovered, the Jacobi solver against the SVD closed form, the stop rules, the `geometry.icp` keys, a `device: cpu` run
that registers its own export, and the bindings of the three exports.  Every test prints its figures (`ICPERR ...`, pytest -s) before it
asserts."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mm3dgs_slam_amd import export as ex, geometry as geo
from mm3dgs_slam_amd.eval_utils import align_horn
from tests import icp_cases as ic
from tests.geometry_cases import rows_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("motion,every", [(m, e) for m in range(3) for e in (1, 3)])
def test_corner_motion_is_recovered(motion, every):
    c = ic.corner_case(motion, every)
    r = ic.run_host(c)
    rot, tr = ic.motion_errors(r["T"], c["R"], c["t"])
    print(f"ICPERR host {c['name']}: {len(c['src'])} rows, status {r['status']} after {r['passes']} passes ({r['passes'] - 1} solves, Jacobi sweeps {r['sweeps']}), "
          f"fitness {r['fitness']}, rmse {r['rmse']}, rotation error {rot} rad, translation error {tr} m")
    assert r["status"] == 0 and r["passes"] <= ic.ITERS and r["fitness"] == 1.0
    assert rot < ic.BOUND and tr < ic.BOUND
    log = r["log"]
    assert (log[:r["passes"], 0] == 1).all() and (log[r["passes"]:] == 0).all() and (log[:r["passes"], 2] == len(c["src"])).all()
    assert np.array_equal(log[r["passes"] - 1, 9:12], r["T"][:, 3]) and log[r["passes"] - 1, 3] == r["fitness"] and log[r["passes"] - 1, 4] == r["rmse"]
    # the final index / dist are those of the source moved by the returned T
    d, i, _ = geo.nn_index_host(geo.move_rows_host(c["src"], r["T"]), c["ref"], ic.CELL, ic.MAX_DIST)
    assert np.array_equal(i, r["index"]) and d.tobytes() == r["dist"].tobytes()


def test_jacobi_solver_agrees_with_the_svd_closed_form():
    c = ic.corner_case(2)
    _, _, has, p, q, d2 = geo.icp_pairs_host(c["src"], c["ref"], ic.CELL, ic.MAX_DIST, np.eye(3, 4))
    T, quat, sweeps = geo._horn_solve(geo.icp_sums(has, p, q, d2))
    R, t, _ = align_horn(p[has].T, q[has].T)
    dR, dt = float(np.abs(T[:, :3] - R).max()), float(np.abs(T[:, 3] - t.reshape(3)).max())
    print(f"ICPERR solver on the first pass's {int(has.sum())} pairs of {c['name']}: |R - R_svd| {dR}, |t - t_svd| {dt}, {sweeps} sweeps, quaternion {quat}")
    assert has.sum() > 1000 and dR < 1e-10 and dt < 1e-10
    assert quat[0] >= 0 and abs(sum(v * v for v in quat) - 1.0) < 1e-15 and abs(np.linalg.det(T[:, :3]) - 1.0) < 1e-14
    # the two summation orders give a solver the same problem up to rounding
    Tk = geo._horn_solve(geo.icp_sums(has, p, q, d2, "kernel"))[0]
    assert float(np.abs(Tk - T).max()) < 1e-12


def test_jacobi_sweeps_end_by_an_exactly_zero_sum_well_below_the_cap():
    rng = np.random.default_rng(5)
    worst = 0
    for trial in range(600):
        n = int(rng.integers(3, 40))
        p = rng.normal(size=(n, 3)) * float(rng.choice([1e-6, 1e-3, 1.0, 1e3]))
        R = ic.rotation(float(rng.uniform(0, 180)), rng.normal(size=3))
        q = p @ R.T + rng.normal(size=3)
        if trial % 4 == 1:      # planar
            p[:, 2] = 0.0
            q = p @ R.T
        if trial % 4 == 2:      # collinear: the dominant eigenvalue is double
            p = np.outer(rng.normal(size=n), [1.0, 2.0, 3.0])
            q = p @ R.T
        if trial % 4 == 3:      # a half turn: w = 0
            q = p @ ic.rotation(180.0, rng.normal(size=3)).T
        T, quat, sweeps = geo._horn_solve(geo.icp_sums(np.ones(n, dtype=bool), p, q, np.zeros(n)))
        worst = max(worst, sweeps)
        assert np.isfinite(T).all() and abs(np.linalg.det(T[:, :3]) - 1.0) < 1e-12 and quat[0] >= 0, trial
        if trial % 4 in (0, 1):
            assert float(np.abs(T[:, :3] - R).max()) < 1e-6 * max(1.0, 1.0 / np.abs(p).max()), trial
    S = [3.0, 0, 0, 0, 0, 0, 0] + [0.0] * 10      # every sum zero: N(S) = 0, no sweep, the identity
    T0, q0, s0 = geo._horn_solve(S)
    print(f"ICPERR solver: at most {worst} sweeps over 600 random, planar, collinear and half-turn sets (cap {geo.ICP_SWEEPS}); zero matrix -> {q0} in {s0} sweeps")
    assert worst < 12 < geo.ICP_SWEEPS and s0 == 0 and q0 == [1.0, 0.0, 0.0, 0.0] and np.array_equal(T0, np.eye(3, 4))


def test_both_sum_orders_find_the_same_correspondences_on_every_pass():
    c = ic.corner_case(0)
    full = ic.run_host(c, "kernel")
    for iters in list(range(1, full["passes"])) + [ic.ITERS]:      # a run of `iters` solves ends on pass `iters`: its index is that pass's
        a, b = ic.run_host(c, "numpy", iters=iters), ic.run_host(c, "kernel", iters=iters)
        print(f"ICPERR sum orders, iters {iters}: passes {a['passes']} / {b['passes']}, max |T_numpy - T_kernel| {float(np.abs(a['T'] - b['T']).max())}")
        assert a["passes"] == b["passes"] and a["status"] == b["status"] and np.array_equal(a["index"], b["index"])
        assert (a["index"] != geo.NO_INDEX).all()


def test_move_rows_host():
    c = ic.rare_case()
    rows = c["src"].copy()
    rows[:, 3] = np.arange(len(rows), dtype=np.int32) * 7919
    assert geo.move_rows_host(rows, np.eye(3, 4)).tobytes() == rows.tobytes()      # (no coordinate of the set is -0.0, which 0 x y + would lose)
    T = np.concatenate([ic.rotation(30.0), [[0.5], [-0.25], [2.0]]], 1)
    out = geo.move_rows_host(rows, T)
    xyz, fin = geo.rows_xyz(rows).astype(np.float64), np.isfinite(geo.rows_xyz(rows)).all(1)
    want = (xyz[fin] @ T[:, :3].T + T[:, 3])
    err = float(np.abs(geo.rows_xyz(out)[fin].astype(np.float64) - want).max())
    print(f"ICPERR move_rows_host: {int((~fin).sum())} rows that are not finite of {len(rows)}, max |moved - R p - t| {err}")
    assert (~fin).sum() == 3 and out[~fin].tobytes() == rows[~fin].tobytes() and np.array_equal(out[:, 3], rows[:, 3])
    assert err <= 2.0 ** -24 * np.abs(want).max() * 1.01 + 1e-15      # one rounding to float32


def test_stop_rules():
    c = ic.corner_case(2)
    two = ic.run_host(dict(c, src=c["src"][:2]))
    assert two["status"] == 2 and two["passes"] == 1 and np.array_equal(two["T"], np.eye(3, 4)) and two["log"][0, 1] == 2 and two["log"][0, 12] == 2
    far = ic.run_host(dict(c, ref=rows_of(geo.rows_xyz(c["ref"]).astype(np.float64) + 10.0)))
    assert far["status"] == 2 and far["fitness"] == 0.0 and far["rmse"] == 0.0 and np.array_equal(far["T"], np.eye(3, 4)) and (far["index"] == geo.NO_INDEX).all()
    empty = ic.run_host(dict(c, ref=rows_of([[np.nan, 0, 0]])))
    assert empty["status"] == 2 and empty["fitness"] == 0.0
    one = ic.run_host(c, iters=1)
    print(f"ICPERR stop rules: two rows -> {two['status']}, far reference -> {far['status']} fitness {far['fitness']}, iters 1 -> {one['status']} after {one['passes']} passes")
    assert one["status"] == 1 and one["passes"] == 2 and one["log"][1, 12] == 1 and one["log"].shape == (2, 16)
    assert not np.array_equal(one["T"], np.eye(3, 4)) and np.array_equal(one["log"][0, 9:12], one["T"][:, 3])
    start = ic.run_host(c, iters=3)
    again = ic.run_host(c, start=start["T"])
    assert start["status"] == 1 and again["status"] == 0 and again["passes"] < ic.run_host(c)["passes"]
    for bad in (dict(iters=0), dict(iters=1001), dict(max_dist=0.0), dict(max_dist=float("nan")), dict(rel_fitness=-1.0), dict(rel_rmse=float("nan"))):
        with pytest.raises(ValueError, match="icp_"):
            ic.run_host(c, **bad)


def test_icp_options_and_their_validation():
    from mm3dgs_slam_amd.config import GEOMETRY_ICP, default_config, utmm_config
    assert GEOMETRY_ICP == {"icp": "none", "icp_max_dist": 0.1, "icp_iters": 30, "icp_rel_fitness": 1e-6, "icp_rel_rmse": 1e-6}
    for cfg in (default_config(), utmm_config()):      # the default block is still the pinned one
        assert cfg["geometry"] == {"eval": False, "estimate": "mesh", "reference": "sensor", "threshold": 0.05, "max_dist": 1.0, "density": 10000.0, "cell": 0,
                                   "seed": 0, "align": "none", "max_samples": 16777216}
    cfg = default_config(device="cpu")
    opt = ex.options(cfg, "geometry")
    assert {k: opt[k] for k in GEOMETRY_ICP} == GEOMETRY_ICP
    cfg["geometry"].update(icp="Point", icp_iters=5, icp_max_dist=0.2)
    opt = ex.options(cfg, "geometry")
    assert opt["icp"] == "point" and opt["icp_iters"] == 5 and opt["icp_max_dist"] == 0.2
    assert ex.options(dict(cfg, geometry=dict(cfg["geometry"], icp=None)), "geometry")["icp"] == "none"
    for bad, match in ((dict(icp="plane"), "none / point"), (dict(icp_max_dist=0), "icp_max_dist"), (dict(icp_max_dist=float("inf")), "icp_max_dist"),
                       (dict(icp_max_dist=1e6, cell=1e-3), "icp_max_dist"), (dict(icp_iters=0), "icp_iters"), (dict(icp_iters=1001), "icp_iters"),
                       (dict(icp_iters=2.5), "icp_iters"), (dict(icp_rel_fitness=-1e-9), "icp_rel_fitness"), (dict(icp_rel_rmse=float("nan")), "icp_rel_rmse"),
                       (dict(icp_rel_rmse="small"), "icp_rel_rmse")):
        with pytest.raises(ValueError, match=match):
            ex.options(dict(cfg, geometry=dict(cfg["geometry"], **bad)), "geometry")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "slam_top.py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "--geometry-icp" in out.stdout


def test_register_moves_a_mesh_by_its_vertices():
    v, tris = ic.box_mesh()
    R, t = ic.rotation(ic.MOTIONS[0][0]), np.asarray(ic.MOTIONS[0][1])
    moved = rows_of((geo.rows_xyz(v).astype(np.float64) - t) @ R, rgba=v[:, 3])
    (back, tris_out), rec = geo.register((moved, tris), (v, tris), device="cpu", density=2000.0, seed=3)
    rot, tr = ic.motion_errors(rec["T"], R, t)
    err = float(np.abs(geo.rows_xyz(back).astype(np.float64) - geo.rows_xyz(v)).max())
    print(f"ICPERR register, box mesh: status {rec['status']} after {rec['passes']} passes, fitness {rec['fitness_start']} -> {rec['fitness']}, rmse "
          f"{rec['rmse_start']} -> {rec['rmse']}, rotation error {rot}, translation error {tr}, max vertex error {err}, {rec['n_source']} / {rec['n_reference']} samples")
    assert tris_out is tris and np.array_equal(back[:, 3], v[:, 3]) and rec["n_source"] == len(geo.sample_mesh_host(moved, tris, 2000.0, 3)[0])
    # the sampler's counts and barycentric coordinates depend on the seed and the triangle alone, so the samples of the moved mesh are the
    # moved samples up to their float32 rounding: the true pairs exist, and the corner scene's bound holds
    assert rec["status"] == 0 and rec["fitness"] == 1.0 and rec["rmse"] < rec["rmse_start"] and rot < ic.BOUND and tr < ic.BOUND and err < ic.BOUND
    cloud, rec2 = geo.register(moved, v, device="cpu")      # clouds: taken as they are -- the eight corners against themselves
    assert rec2["n_source"] == 8 and rec2["status"] == 0 and float(np.abs(geo.rows_xyz(cloud).astype(np.float64) - geo.rows_xyz(v)).max()) < 1e-6


def test_cpu_run_registers_its_export(tmp_path):
    slam, _, _ = ic.cpu_slam(tmp_path / "run", {"eval": False, "density": 400.0}, {"voxel": 0.08, "every": 1, "source": "sensor"}, tracking={"use_gt_pose": True})

    def evaluate(name, **keys):
        slam.cfg["geometry"] = dict({"eval": False, "density": 400.0}, **keys)
        out = slam.evaluate_geometry(path=str(tmp_path / name))
        return out, json.load(open(tmp_path / name / "metrics.json"))

    parent, m_parent = evaluate("parent")      # the call as it was before the keys existed
    none, m_none = evaluate("none", icp="none", icp_max_dist=0.1, icp_iters=30, icp_rel_fitness=1e-6, icp_rel_rmse=1e-6)
    for f in ("metrics.json", "accuracy.ply", "completion.ply"):
        assert (tmp_path / "none" / f).read_bytes() == (tmp_path / "parent" / f).read_bytes(), f
    assert sorted(os.listdir(tmp_path / "none")) == sorted(os.listdir(tmp_path / "parent")) == ["accuracy.ply", "completion.ply", "metrics.json"]
    assert "icp" not in m_none and "icp" not in none
    on, m = evaluate("on", icp="point")
    b = m["icp"]
    print(f"ICPERR cpu run, ground-truth poses and sensor views, icp: point: accuracy {m['accuracy']}, completion {m['completion']}, icp block {json.dumps(b)}")
    assert m["accuracy"] < 1e-5 and m["completion"] < 1e-5 and m["n_estimate"] == m_parent["n_estimate"] > 0
    assert b["status"] == 0 and b["fitness"] == 1.0 and b["moved"] is True and b["status_name"] == "converged" and b["n_source"] == m["n_estimate"]
    assert (b["max_dist"], b["iters"], b["rel_fitness"], b["rel_rmse"]) == (0.1, 30, 1e-6, 1e-6) and np.asarray(b["T"]).shape == (3, 4)
    assert float(np.abs(np.asarray(b["T"]) - np.eye(3, 4)).max()) < 1e-6
    z = np.load(tmp_path / "on" / "icp.npz")
    assert z["T"].shape == (3, 4) and z["log"].shape == (31, 16) and int(z["status"]) == 0 and np.array_equal(z["T"], np.asarray(b["T"]))
    assert on["files"]["icp"] == str(tmp_path / "on" / "icp.npz")
    # too few correspondences is not an error: the estimate stays where it was, and the block says so
    from mm3dgs_slam_amd import pointcloud as pc
    away = pc.write_ply(str(tmp_path / "away.ply"), rows_of(geo.rows_xyz(ic.box_mesh()[0]).astype(np.float64) + 50.0))
    _, m_off = evaluate("away_off", reference=away)
    _, m_far = evaluate("away_on", reference=away, icp="point")
    print(f"ICPERR cpu run against a cloud 50 m away: icp block {json.dumps(m_far['icp'])}")
    assert m_far["icp"]["status"] == 2 and m_far["icp"]["moved"] is False and m_far["icp"]["fitness"] == 0.0 and m_far["icp"]["passes"] == 1
    assert np.array_equal(np.asarray(m_far["icp"]["T"]), np.eye(3, 4)) and m_far["accuracy"] == m_off["accuracy"]
    for f in ("accuracy.ply", "completion.ply"):
        assert (tmp_path / "away_on" / f).read_bytes() == (tmp_path / "away_off" / f).read_bytes(), f
    slam.cfg["geometry"]["icp"] = "plane"
    with pytest.raises(ValueError, match="none / point"):
        slam.evaluate_geometry(path=str(tmp_path / "x"))


def test_cabi_declares_and_binds_the_three_symbols():
    from mm3dgs_slam_amd import _lib
    h = open(os.path.join(ROOT, "include", "mm3dgs.h")).read()
    lib = _lib.load()
    for name in ("mm3dgs_icp_work_bytes", "mm3dgs_icp_point", "mm3dgs_rows_move"):
        assert re.search(r"\b" + name + r"\s*\(", h) and name in _lib.exported_symbols() and hasattr(lib, name) and re.fullmatch(r"mm3dgs_[a-z_]+", name), name
    P = C.c_void_p
    assert lib.mm3dgs_icp_point.argtypes == [C.c_uint64, P, C.c_uint64, C.c_double, C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, P, P, C.c_double, C.c_int,
                                             C.c_double, C.c_double, P, P, P, P, P, P]
    assert lib.mm3dgs_rows_move.argtypes == [C.c_uint64, P, P, P, P]
    assert lib.mm3dgs_icp_work_bytes.argtypes == [C.c_uint64] and lib.mm3dgs_icp_work_bytes.restype is C.c_size_t
    assert lib.mm3dgs_icp_point.restype is C.c_int and lib.mm3dgs_rows_move.restype is C.c_int
    for n in (1, 257, 65792, 1 << 30):
        b = int(lib.mm3dgs_icp_work_bytes(n))
        assert b > 0 and b % 8 == 0 and b >= 8 * 24 * ((n + 255) // 256), (n, b)
    for n in (0, (1 << 30) + 1):
        assert int(lib.mm3dgs_icp_work_bytes(n)) == 0, n
    assert lib.mm3dgs_version() == 213 and re.search(r"#define MM3DGS_ABI_VERSION 213\b", h)
    for text in ("((R0 p.x + R1 p.y) + R2 p.z) + t", "[12] passes run", "[13] status", "2 (iters + 1)", "rows_out may be rows_in"):
        assert text in h, text
    # calls the entry points refuse before anything is launched (no device is touched)
    FAKE, origin, nan = 0x1000, (C.c_int64 * 3)(0, 0, 0), float("nan")
    ok = dict(n_q=10, q_rows=FAKE, n_ref=10, cell=0.05, origin=origin, gx=4, gy=4, gz=4, cell_start=FAKE, sorted=FAKE, max_dist=0.1, iters=30, rel_fitness=1e-6,
              rel_rmse=1e-6, state=FAKE, log=FAKE, dist_out=None, index_out=None, work=FAKE)
    cases = {"n_q = 0": (dict(n_q=0), "n_q"), "n_q > 2^30": (dict(n_q=(1 << 30) + 1), "n_q"), "n_ref = 0": (dict(n_ref=0), "n_ref"),
             "n_ref > 2^30": (dict(n_ref=(1 << 30) + 1), "n_ref"), "grid": (dict(gx=0), "grid"), "cell": (dict(cell=0.0), "cell"), "max_dist NaN": (dict(max_dist=nan), "max_dist"),
             "rings": (dict(max_dist=1e6, cell=1e-3), "rings"), "iters = 0": (dict(iters=0), "iters"), "iters = 1001": (dict(iters=1001), "iters"),
             "rel_fitness < 0": (dict(rel_fitness=-1.0), "rel_fitness"), "rel_rmse NaN": (dict(rel_rmse=nan), "rel_rmse"), "NULL origin": (dict(origin=None), "origin_cell"),
             "NULL q_rows": (dict(q_rows=None), "NULL"), "NULL cell_start": (dict(cell_start=None), "NULL"), "NULL sorted": (dict(sorted=None), "NULL"),
             "NULL state": (dict(state=None), "NULL"), "NULL log": (dict(log=None), "NULL"), "NULL work": (dict(work=None), "NULL"),
             "misaligned q_rows": (dict(q_rows=FAKE + 8), "16-byte"), "misaligned sorted": (dict(sorted=FAKE + 4), "16-byte"), "misaligned state": (dict(state=FAKE + 4), "8-byte"),
             "misaligned log": (dict(log=FAKE + 4), "8-byte"), "misaligned work": (dict(work=FAKE + 2), "8-byte"), "misaligned dist_out": (dict(dist_out=FAKE + 2), "4-byte"),
             "misaligned index_out": (dict(index_out=FAKE + 1), "4-byte"), "misaligned cell_start": (dict(cell_start=FAKE + 2), "4-byte")}
    for what, (over, word) in cases.items():
        a = dict(ok, **over)
        rc = lib.mm3dgs_icp_point(a["n_q"], a["q_rows"], a["n_ref"], a["cell"], a["origin"], a["gx"], a["gy"], a["gz"], a["cell_start"], a["sorted"], a["max_dist"], a["iters"],
                                  a["rel_fitness"], a["rel_rmse"], a["state"], a["log"], a["dist_out"], a["index_out"], a["work"], None)
        msg = (lib.mm3dgs_last_error() or b"").decode()
        assert rc == -1 and msg.startswith("icp_point: ") and word in msg, (what, msg)
    for what, args, word in (("n = 0", (0, FAKE, FAKE, FAKE), "n ="), ("n > 2^30", ((1 << 30) + 1, FAKE, FAKE, FAKE), "n ="), ("NULL rows_in", (10, None, FAKE, FAKE), "NULL"),
                             ("NULL T", (10, FAKE, None, FAKE), "NULL"), ("NULL rows_out", (10, FAKE, FAKE, None), "NULL"), ("misaligned rows_in", (10, FAKE + 8, FAKE, FAKE), "16-byte"),
                             ("misaligned rows_out", (10, FAKE, FAKE, FAKE + 4), "16-byte"), ("misaligned T", (10, FAKE, FAKE + 4, FAKE), "8-byte")):
        rc = lib.mm3dgs_rows_move(*args, None)
        msg = (lib.mm3dgs_last_error() or b"").decode()
        assert rc == -1 and msg.startswith("rows_move: ") and word in msg, (what, msg)
