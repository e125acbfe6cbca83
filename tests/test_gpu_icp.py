"""mm3dgs_icp_point / mm3dgs_rows_move (csrc/geometry.hip) through the raw C ABI against the float64 host statement of
mm3dgs_slam_amd/geometry.py (icp_host with sum_order "kernel", move_rows_host), BYTE FOR BYTE: state[0:14], the whole log and the final
index / dist -- the device lane of the solver is the same sequence of + - x / sqrt as the host's, and the sums are added in one stated order.
Sizes at workgroup and wave boundaries, a second round of the finish over the partial rows, the rare branches, a start other than the
identity, determinism and the early return; then the Python surface (GeometryScorer.icp, register, evaluate_geometry).  Work buffers lie
between guard zones and every output has sentinel elements behind it.  Every test prints its figures (`ICPERR ...`, pytest -s) before it
asserts."""
import ctypes as C
import json
import random

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import geometry as geo, pointcloud as pc
from tests import icp_cases as ic
from tests.geometry_cases import rows_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096               # bytes of guard zone on each side of a work buffer
PAD = 8                    # elements behind every output that no call may touch
SENT = 0x7A7A7A7A          # every int32 of an untouched output element
WORK_SENT = 0xA5           # every byte of the guard zones


def _ptr(t):
    return None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _lib():
    from mm3dgs_slam_amd import _lib
    return _lib.load()


def _stream():
    from mm3dgs_slam_amd.rasterizer import _stream
    return _stream()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(nbytes, fill):
    buf = torch.full((2 * GUARD + nbytes,), WORK_SENT, dtype=torch.uint8, device=DEV)
    buf[GUARD:GUARD + nbytes] = fill
    return buf, buf.data_ptr() + GUARD


def _guards_ok(buf):
    b = buf.cpu().numpy()
    return bool((b[:GUARD] == WORK_SENT).all()) and bool((b[-GUARD:] == WORK_SENT).all())


class Icp:
    """Caller-owned buffers of one grid build and one mm3dgs_icp_point call: sentinel-filled outputs with PAD elements behind them, the work
    buffer between guards and filled with `fill`."""

    def __init__(self, case, iters=ic.ITERS, fill=0x00, start=None, want_index=True):
        lib = _lib()
        self.case, self.iters = case, iters
        self.ref, self.src = _dev(case["ref"]), _dev(case["src"])
        self.n_ref, self.n_q = len(case["ref"]), len(case["src"])
        xyz = pc.rows_xyz(case["ref"]).astype(np.float64)
        fin = xyz[np.isfinite(xyz).all(1)]
        self.cell, self.o, self.dims = geo.grid_for(fin.min(0), fin.max(0), ic.CELL)
        nc = self.dims[0] * self.dims[1] * self.dims[2]
        self.origin = (C.c_int64 * 3)(*[int(v) for v in self.o])
        self.cell_start = torch.empty(nc + 1, dtype=torch.int32, device=DEV)
        self.sorted = torch.empty(self.n_ref, 4, dtype=torch.int32, device=DEV)
        counters = torch.empty(8, dtype=torch.int64, device=DEV)
        gwork = torch.empty(int(lib.mm3dgs_nn_grid_work_bytes(self.n_ref, *self.dims)) // 8, dtype=torch.int64, device=DEV)
        assert lib.mm3dgs_nn_grid_build(self.n_ref, _ptr(self.ref), self.cell, self.origin, *self.dims, _ptr(self.cell_start), _ptr(self.sorted), _ptr(counters),
                                        _ptr(gwork), _stream()) == 0
        self.nlog = (iters + 1) * 16
        self.state = torch.full((2 * (16 + PAD),), SENT, dtype=torch.int32, device=DEV)      # [12:16] hold the sentinel: the call zeroes them
        self.state.view(torch.float64)[:12] = _dev(np.asarray(np.eye(3, 4) if start is None else start, dtype=np.float64).reshape(12))
        self.log = torch.full((2 * (self.nlog + PAD),), SENT, dtype=torch.int32, device=DEV)
        self.dist = torch.full((self.n_q + PAD,), SENT, dtype=torch.int32, device=DEV) if want_index else None
        self.index = torch.full((self.n_q + PAD,), SENT, dtype=torch.int32, device=DEV) if want_index else None
        self.nw = int(lib.mm3dgs_icp_work_bytes(self.n_q))
        assert self.nw > 0 and self.nw % 8 == 0
        self.wbuf, self.work = _guarded(self.nw, fill)

    def run(self, **over):
        a = dict(max_dist=ic.MAX_DIST, rel_fitness=ic.REL, rel_rmse=ic.REL)
        a.update(over)
        rc = _lib().mm3dgs_icp_point(self.n_q, _ptr(self.src), self.n_ref, self.cell, self.origin, *self.dims, _ptr(self.cell_start), _ptr(self.sorted), a["max_dist"],
                                     self.iters, a["rel_fitness"], a["rel_rmse"], _ptr(self.state), _ptr(self.log), _ptr(self.dist), _ptr(self.index), _ptr(self.work), _stream())
        torch.cuda.synchronize()
        return rc

    def read(self):
        """(state float64 [16], log float64 [iters + 1, 16], dist float32 [n_q], index uint32 [n_q]) after the guards and sentinels were checked."""
        state, log = self.state.cpu().numpy(), self.log.cpu().numpy()
        assert _guards_ok(self.wbuf), "a guard zone of the work buffer was written"
        assert bool((state[32:] == SENT).all()) and bool((log[2 * self.nlog:] == SENT).all()), "elements behind state / log were written"
        dist = index = None
        if self.dist is not None:
            dist, index = self.dist.cpu().numpy(), self.index.cpu().numpy()
            assert bool((dist[self.n_q:] == SENT).all()) and bool((index[self.n_q:] == SENT).all()), "elements behind dist_out / index_out were written"
            dist, index = dist[:self.n_q].view(np.float32).copy(), index[:self.n_q].view(np.uint32).copy()
        return state[:32].view(np.float64).copy(), log[:2 * self.nlog].view(np.float64).reshape(-1, 16).copy(), dist, index


def _check(case, iters=ic.ITERS, fill=0x00, start=None, host=None):
    """One device call held to the host statement byte for byte; returns (host result, device state, device log)."""
    host = ic.run_host(case, "kernel", iters=iters, start=start) if host is None else host
    dev = Icp(case, iters, fill, start)
    assert dev.run() == 0
    state, log, dist, index = dev.read()
    want = geo.icp_state(host)
    rot, tr = ic.motion_errors(state[:12], case["R"], case["t"])
    same = dict(state=state[:14].tobytes() == want[:14].tobytes(), log=log.tobytes() == host["log"].tobytes(), index=np.array_equal(index, host["index"]),
                dist=dist.tobytes() == host["dist"].tobytes())
    print(f"ICPERR device {case['name']} ({dev.n_q} x {dev.n_ref}, iters {iters}, fill {fill:#04x}): status {int(state[13])} after {int(state[12])} passes (host {host['status']} / "
          f"{host['passes']}), fitness {log[max(int(state[12]) - 1, 0), 3]}, rmse {log[max(int(state[12]) - 1, 0), 4]}, rotation error {rot} rad, translation error {tr} m; "
          f"max |T - T_host| {float(np.abs(state[:12] - want[:12]).max())}, max |log - log_host| {float(np.abs(log - host['log']).max())}, "
          f"{int((index != host['index']).sum())} index and {int((dist.view(np.int32) != host['dist'].view(np.int32)).sum())} dist values differ; equal bytes: {same}")
    assert (state[14:] == 0).all() and all(same.values()), same
    return host, state, log


@pytest.mark.parametrize("motion,every", [(m, e) for m in range(3) for e in (1, 3)])
def test_corner_cases_byte_for_byte(motion, every):
    case = ic.corner_case(motion, every)
    host, state, log = _check(case)
    rot, tr = ic.motion_errors(state[:12], case["R"], case["t"])
    assert int(state[13]) == 0 and log[int(state[12]) - 1, 3] == 1.0 and rot < ic.BOUND and tr < ic.BOUND


@pytest.mark.parametrize("n", (1, 255, 256, 257, 513))
def test_edge_sizes_byte_for_byte(n):
    c = ic.corner_case(2)
    host, state, _ = _check(dict(c, name=f"first {n} rows of {c['name']}", src=c["src"][:n]))
    assert (int(state[13]) == 2) == (n == 1)      # (a floor patch alone slides: 255 and 513 rows run into `iters`, status 1 -- all 31 passes)


def test_second_round_of_the_finish_byte_for_byte():
    case = ic.tiled_case()
    assert len(case["src"]) == 256 * 257      # 257 partial rows: lane 0 of the finish adds two
    _, state, _ = _check(case, fill=0xFF)
    assert int(state[13]) == 0


def test_rare_branches_byte_for_byte():
    case = ic.rare_case()
    host, state, log = _check(case, fill=0xFF)
    sxyz = pc.rows_xyz(case["src"])
    bad = ~np.isfinite(sxyz).all(1)
    none = host["index"] == geo.NO_INDEX
    grid_hi = np.nanmax(np.where(np.isfinite(pc.rows_xyz(case["ref"])), pc.rows_xyz(case["ref"]), np.nan), 0)
    outside = ~bad & ((sxyz > grid_hi + ic.MAX_DIST).any(1) | (sxyz < -ic.MAX_DIST - 0.02).any(1))
    print(f"ICPERR rare branches: {int(bad.sum())} rows not finite, {int((none & ~bad).sum())} finite rows without a correspondence ({int(outside.sum())} beyond the grid by more "
          f"than max_dist), finite rows {log[0, 2]}, n {log[:int(state[12]), 1].tolist()}")
    assert bad.sum() == 3 and np.isnan(host["dist"][bad]).all() and none[bad].all() and log[0, 2] == len(sxyz) - 3
    assert outside.sum() >= 3 and none[outside].all() and (host["dist"][outside] == np.float32(ic.MAX_DIST)).all()
    assert not bad[705:709].any() and not outside[705:709].any() and (~none[705:709]).sum() >= 2      # the four rows just outside the lattice: within reach
    # duplicates in the reference: rows 0 .. 39 are repeated at 42 .. 81, rows 142 .. 181 at the end -- the smaller row wins
    n_ref = len(case["ref"])
    assert ((host["index"] < 40).sum() > 0) and not ((host["index"] >= 42) & (host["index"] < 82)).any() and not ((host["index"] >= n_ref - 40) & ~none).any()
    assert ((host["index"] >= 142) & (host["index"] < 182)).sum() > 0 and not np.isin(host["index"], (40, 41)).any()


def test_start_other_than_the_identity():
    case = ic.corner_case(2)
    first, state, _ = _check(case, iters=3)
    assert first["status"] == 1 and first["passes"] == 4
    again, state2, _ = _check(dict(case, name=case["name"] + " from its own 3-iteration result"), start=state[:12].reshape(3, 4))
    assert int(state2[13]) == 0 and again["passes"] < ic.run_host(case)["passes"]


def test_two_calls_give_the_same_bytes_and_the_passes_behind_the_stop_return_at_entry():
    case = ic.corner_case(1)
    outs = []
    for fill in (0x00, 0xFF):
        dev = Icp(case, fill=fill)
        assert dev.run() == 0
        outs.append(dev.read())
    (s0, l0, d0, i0), (s1, l1, d1, i1) = outs
    passes = int(s0[12])
    print(f"ICPERR determinism: {passes} passes of {ic.ITERS + 1}; log rows behind the stop all zero: {bool((l0[passes:] == 0).all())}")
    assert s0.tobytes() == s1.tobytes() and l0.tobytes() == l1.tobytes() and d0.tobytes() == d1.tobytes() and i0.tobytes() == i1.tobytes()
    assert 1 < passes < ic.ITERS and (l0[:passes, 0] == 1).all() and (l0[passes:].view(np.int64) == 0).all()      # a pass that ran would have written its row
    # without the two optional arrays: the same state and log
    dev = Icp(case, want_index=False)
    assert dev.run() == 0
    s2, l2, _, _ = dev.read()
    assert s2.tobytes() == s0.tobytes() and l2.tobytes() == l0.tobytes()


@pytest.mark.parametrize("n", (1, 255, 256, 257))
def test_rows_move_byte_for_byte(n):
    lib = _lib()
    rows = ic.rare_case()["src"][:n].copy()
    rows[n // 2, 0] = np.float32(np.nan).view(np.int32)
    rows[:, 3] = np.arange(n, dtype=np.int32) * 7919 + 1
    T = np.concatenate([ic.rotation(30.0), [[0.5], [-0.25], [2.0]]], 1)
    want = geo.move_rows_host(rows, T)
    src, Td = _dev(rows), _dev(T.reshape(12))
    out = torch.full((n + PAD, 4), SENT, dtype=torch.int32, device=DEV)
    assert lib.mm3dgs_rows_move(n, _ptr(src), _ptr(Td), _ptr(out), _stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    print(f"ICPERR rows_move n = {n}: {int((got[:n] != want).sum())} of {4 * n} words differ from move_rows_host")
    assert got[:n].tobytes() == want.tobytes() and bool((got[n:] == SENT).all()) and src.cpu().numpy().tobytes() == rows.tobytes()
    assert lib.mm3dgs_rows_move(n, _ptr(src), _ptr(Td), _ptr(src), _stream()) == 0      # in place
    torch.cuda.synchronize()
    assert src.cpu().numpy().tobytes() == want.tobytes()
    assert geo.move_rows(rows, T, DEV).cpu().numpy().tobytes() == want.tobytes()


def test_register_and_compare_on_the_device():
    v, tris = ic.box_mesh()
    R, t = ic.rotation(ic.MOTIONS[0][0]), np.asarray(ic.MOTIONS[0][1])
    moved = rows_of((pc.rows_xyz(v).astype(np.float64) - t) @ R, rgba=v[:, 3])
    kw = dict(density=2000.0, seed=3)
    (back, tris_dev), rec = geo.register((_dev(moved), _dev(tris)), (_dev(v), _dev(tris)), device=DEV, **kw)
    (back_k, _), rec_k = geo.register((moved, tris), (v, tris), device="cpu", sum_order="kernel", **kw)
    (back_h, _), rec_h = geo.register((moved, tris), (v, tris), device="cpu", **kw)
    rot, tr = ic.motion_errors(rec["T"], R, t)
    print(f"ICPERR register on the device, box mesh: status {rec['status']} after {rec['passes']} passes, fitness {rec['fitness']}, rmse {rec['rmse']}, rotation error {rot}, "
          f"translation error {tr}; max |T - T_host| {float(np.abs(rec['T'] - rec_h['T']).max())} (numpy order), {float(np.abs(rec['T'] - rec_k['T']).max())} (kernel order)")
    assert back.is_cuda and back.cpu().numpy().tobytes() == back_k.tobytes() and tris_dev.cpu().numpy().tobytes() == tris.tobytes()
    # (against the numpy order the rows carry T's difference: R p + t with |p| + |t| < 2 m, T held to relative 2^-23 below -- a corner that
    #  comes back to 0 is a float32 of 1e-9, where the last bits of a double T show)
    assert np.array_equal(back_k[:, 3], back_h[:, 3]) and float(np.abs(pc.rows_xyz(back_k).astype(np.float64) - pc.rows_xyz(back_h)).max()) <= 2.0 ** -23 * 2.0
    for k in ("status", "passes", "n_source", "n_reference", "fitness", "fitness_start"):
        assert rec[k] == rec_k[k] == rec_h[k], k
    assert rec["T"].tobytes() == rec_k["T"].tobytes() and rec["log"].tobytes() == rec_k["log"].tobytes()
    # against the host path's own order: the bound of tests/test_gpu_geometry.py's host-against-device comparison
    for k in ("T", "rmse", "rmse_start"):
        assert np.allclose(rec[k], rec_h[k], rtol=2.0 ** -23, atol=0), k
    assert rec["status"] == 0 and rot < ic.BOUND and tr < ic.BOUND
    out = geo.compare((back, tris_dev), (_dev(v), _dev(tris)), device=DEV, threshold=0.05, max_dist=1.0, **kw)
    print(f"ICPERR compare behind register: accuracy {out['accuracy']}, completion {out['completion']}")
    assert out["accuracy"] < ic.BOUND and out["completion"] < ic.BOUND
    # a reference without a finite row: status 2 without a launch, nothing moves
    cloud, none = geo.register(_dev(moved), _dev(rows_of([[np.nan, 0, 0]])), device=DEV)
    assert none["status"] == 2 and none["passes"] == 1 and none["fitness"] == 0.0 and cloud.cpu().numpy().tobytes() == moved.tobytes() and none["log"][0, 2] == 8


def test_evaluate_geometry_with_icp_on_the_device(tmp_path):
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device=DEV, height=48, width=64, tracking={"iters": 5, "use_gt_pose": True}, mapping={"iters": 6, "kf_every": 2, "min_covisibility": 2.0},
                         outputdir=str(tmp_path), debug={"get_runtime_stats": False, "create_video": False, "save_keyframes": False}, eval_every=1, eval_on_device=False,
                         mesh={"voxel": 0.08, "export": False, "every": 1, "source": "sensor"}, geometry={"eval": False, "density": 2000.0, "icp": "point"})
    slam = SLAM(cfg, SyntheticSequence(cfg, 4, 2000, seed=5))
    slam.run()
    out = slam.evaluate_geometry(path=str(tmp_path / "geometry"))
    m = json.load(open(tmp_path / "geometry" / "metrics.json"))
    z = np.load(tmp_path / "geometry" / "icp.npz")
    print(f"ICPERR evaluate_geometry on the device: accuracy {m['accuracy']}, completion {m['completion']}, icp block {json.dumps(m['icp'])}")
    assert m["accuracy"] < 1e-5 and m["completion"] < 1e-5 and m["n_estimate"] > 0
    assert m["icp"]["status"] == 0 and m["icp"]["fitness"] == 1.0 and m["icp"]["moved"] is True and m["icp"]["n_source"] == m["n_estimate"]
    assert z["T"].shape == (3, 4) and z["log"].shape == (31, 16) and int(z["status"]) == 0 and out["files"]["icp"].endswith("icp.npz")
