"""mm3dgs_tsdf_integrate / mm3dgs_tsdf_mesh_plan / mm3dgs_tsdf_mesh_emit (csrc/tsdf.hip) through the raw C ABI against the host statement of
mm3dgs_slam_amd/mesh.py: the integration at lattices from one cube to several workgroups per row, one and three views, every validity
pattern of the pixel test; the mesh on analytic volumes at the shapes where count / scan / scatter can break (one cube, a partial last
workgroup, the second round of the 1024-wide scan); capacity, rejected calls, and the export of a native-loop run.

Bars.  Integration: weights and the three counters exact; |T_dev - T_host| <= k 2^-24 after k views (one float32 rounding per view that can
flip on double roundoff; the running mean damps it), the colour means likewise; a sample whose pixel coordinate is within 1e-9 of a rounding
boundary or whose sdf is within 1e-9 trunc of +-trunc in some view is left out and counted, at most 0.1 % of a case's samples
(tests/test_mesh.py: none with these poses).  Mesh: triangle indices and both totals exact; a position component within 2^-24 |p| + 2^-40
(|origin| + voxel n) of the float64 one; colour bytes within 1.  Every test prints its figures (`MESHERR ...`, pytest -s) before it asserts."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import mesh as ms
from mm3dgs_slam_amd import pointcloud as pc
from tests import mesh_cases as cases
from tests import pointcloud_cases as pcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096               # bytes of guard zone on each side of the work buffer
PAD = 8                    # rows and triangles behind the caps that no call may touch
SENT = 0x7A7A7A7A          # every int32 of an untouched row or triangle
WORK_SENT = 0xA5           # every byte of the guard zones


def _ptr(t):
    return None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _lib():
    from mm3dgs_slam_amd import _lib
    return _lib.load()


def _stream():
    from mm3dgs_slam_amd.rasterizer import _stream
    return _stream()


def _origin(o):
    return (C.c_double * 3)(*[float(v) for v in o])


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Volume:
    """Caller-owned buffers of one volume on the device, with sentinel words behind both arrays."""

    def __init__(self, dims, tsdf_w=None, rgb_w=None):
        self.nx, self.ny, self.nz = dims
        n = self.nx * self.ny * self.nz
        self.tw = torch.full((n + PAD, 2), float("nan"), dtype=torch.float32, device=DEV)
        self.rw = torch.full((n + PAD, 4), float("nan"), dtype=torch.float32, device=DEV)
        self.counters = torch.full((8,), -7, dtype=torch.int64, device=DEV)
        self.n = n
        assert _lib().mm3dgs_tsdf_reset(self.nx, self.ny, self.nz, _ptr(self.tw), _ptr(self.rw), _ptr(self.counters), _stream()) == 0
        torch.cuda.synchronize()
        assert not self.counters.cpu().any() and not self.tw[:n].cpu().numpy().any() and not self.rw[:n].cpu().numpy().any()
        if tsdf_w is not None:
            self.tw[:n] = _dev(tsdf_w.reshape(n, 2))
            self.rw[:n] = _dev(rgb_w.reshape(n, 4))

    def integrate(self, vd, case, **over):
        v = vd
        a = dict(H=v["depth"].shape[0], W=v["depth"].shape[1], fx=v["cam"]["fx"], fy=v["cam"]["fy"], cx=v["cam"]["cx"], cy=v["cam"]["cy"], pose=v["pose"],
                 color=v["color"], depth=v["depth"], sil=v["sil"], sil_min=v["sil_min"], depth_max=v["depth_max"], origin=_origin(case["origin"]),
                 voxel=case["voxel"], trunc=case["trunc"], nx=self.nx, ny=self.ny, nz=self.nz, tsdf_w=self.tw, rgb_w=self.rw, counters=self.counters)
        a.update(over)
        origin = a["origin"] if not isinstance(a["origin"], (list, tuple, np.ndarray)) else _origin(a["origin"])
        rc = _lib().mm3dgs_tsdf_integrate(a["H"], a["W"], a["fx"], a["fy"], a["cx"], a["cy"], _ptr(a["pose"]), _ptr(a["color"]), _ptr(a["depth"]), _ptr(a["sil"]),
                                          a["sil_min"], a["depth_max"], origin, a["voxel"], a["trunc"], a["nx"], a["ny"], a["nz"], _ptr(a["tsdf_w"]),
                                          _ptr(a["rgb_w"]), _ptr(a["counters"]), _stream())
        torch.cuda.synchronize()
        return rc

    def read(self):
        tw, rw = self.tw.cpu().numpy(), self.rw.cpu().numpy()
        assert np.isnan(tw[self.n:]).all() and np.isnan(rw[self.n:]).all(), "the words behind the volume were written"
        return tw[:self.n].reshape(self.nz, self.ny, self.nx, 2).copy(), rw[:self.n].reshape(self.nz, self.ny, self.nx, 4).copy(), self.counters.cpu().numpy().copy()


def to_dev(v):
    out = dict(v)
    for k in ("color", "depth", "sil", "pose"):
        out[k] = _dev(v[k])
    return out


INTEGRATE_CASES = [(dims, hw, "all", 1) for dims in cases.INTEGRATE_SHAPES for hw in cases.VIEW_SHAPES] \
    + [(dims, hw, "all", 3) for dims in cases.INTEGRATE_SHAPES for hw in cases.VIEW_SHAPES] \
    + [((17, 9, 6), (17, 33), p, 1) for p in pcases.PATTERNS if p != "all"] + [((65, 33, 5), (48, 64), p, 3) for p in ("checker", "planted", "sil_edge", "depth_max_edge")]


@pytest.mark.parametrize("dims,hw,pattern,n_views", INTEGRATE_CASES)
def test_integrate_against_the_float64_host_statement(dims, hw, pattern, n_views):
    case = cases.integrate_case(dims, hw[0], hw[1], pattern, n_views)
    tw_h, rw_h, c_h, excluded = cases.integrate_all(case)
    vol = Volume(dims)
    for v in case["views"]:
        assert vol.integrate(to_dev(v), case) == 0
    tw, rw, c = vol.read()
    keep = ~excluded
    bar = n_views * 2.0 ** -24
    with np.errstate(invalid="ignore"):
        dT = np.abs(tw[..., 0].astype(np.float64) - tw_h[..., 0].astype(np.float64))[keep]
        same_nan = np.isnan(rw[..., :3]) == np.isnan(rw_h[..., :3])
        dC = np.nan_to_num(np.abs(rw[..., :3].astype(np.float64) - rw_h[..., :3].astype(np.float64)), nan=0.0)[keep]
    print(f"MESHERR integrate {dims} view {hw} {pattern} x{n_views}: counters {c.tolist()} (host {c_h}), {int(excluded.sum())} of {excluded.size} samples excluded, "
          f"max |dT| = {dT.max() / 2.0 ** -24:.3f} x 2^-24, max |dC| = {dC.max() / 2.0 ** -24:.3f} x 2^-24 (bar {n_views})")
    assert excluded.sum() <= 1e-3 * excluded.size
    if not excluded.any():
        assert c.tolist() == c_h + [0] * 5
    assert c[0] == n_views and not c[3:].any()
    assert np.array_equal(tw[..., 1][keep], tw_h[..., 1][keep]) and np.array_equal(rw[..., 3][keep], rw_h[..., 3][keep])      # the weights, exact
    assert bool(same_nan[keep].all())
    assert dT.max() <= bar and dC.max() <= bar
    untouched = (tw_h[..., 1] == 0) & keep
    assert not tw[untouched].any() and not rw[untouched].any()


class Mesher:
    """work between guard zones, sentinel-filled rows and triangles with PAD entries behind the caps."""

    def __init__(self, vol, origin, voxel, vcap, tcap, work_fill=0x00, min_weight=1.0):
        self.vol, self.origin, self.voxel, self.vcap, self.tcap, self.min_weight = vol, origin, voxel, vcap, tcap, min_weight
        self.nwork = int(_lib().mm3dgs_tsdf_mesh_work_bytes(vol.nx, vol.ny, vol.nz))
        assert self.nwork > 0 and self.nwork % 8 == 0
        self.buf = torch.full((2 * GUARD + self.nwork,), WORK_SENT, dtype=torch.uint8, device=DEV)
        self.buf[GUARD:GUARD + self.nwork] = work_fill
        self.work = self.buf.data_ptr() + GUARD
        self.rows = torch.full((vcap + PAD, 4), SENT, dtype=torch.int32, device=DEV)
        self.tris = torch.full((tcap + PAD, 3), SENT, dtype=torch.int32, device=DEV)
        self.counters = torch.full((8,), -7, dtype=torch.int64, device=DEV)

    def plan(self, **over):
        v = self.vol
        a = dict(nx=v.nx, ny=v.ny, nz=v.nz, tsdf_w=v.tw, min_weight=self.min_weight, work=self.work, counters=self.counters)
        a.update(over)
        rc = _lib().mm3dgs_tsdf_mesh_plan(a["nx"], a["ny"], a["nz"], _ptr(a["tsdf_w"]), a["min_weight"], _ptr(a["work"]), _ptr(a["counters"]), _stream())
        torch.cuda.synchronize()
        return rc

    def emit(self, **over):
        v = self.vol
        a = dict(nx=v.nx, ny=v.ny, nz=v.nz, tsdf_w=v.tw, rgb_w=v.rw, origin=_origin(self.origin), voxel=self.voxel, work=self.work, rows=self.rows, vcap=self.vcap,
                 tris=self.tris, tcap=self.tcap, counters=self.counters)
        a.update(over)
        rc = _lib().mm3dgs_tsdf_mesh_emit(a["nx"], a["ny"], a["nz"], _ptr(a["tsdf_w"]), _ptr(a["rgb_w"]), a["origin"], a["voxel"], _ptr(a["work"]), _ptr(a["rows"]),
                                          a["vcap"], _ptr(a["tris"]), a["tcap"], _ptr(a["counters"]), _stream())
        torch.cuda.synchronize()
        return rc

    def read(self):
        """(rows [vcap + PAD, 4], triangles [tcap + PAD, 3], counters) on the host after checking the guards and the entries behind the caps."""
        rows, tris, buf = self.rows.cpu().numpy(), self.tris.cpu().numpy(), self.buf.cpu().numpy()
        assert bool((buf[:GUARD] == WORK_SENT).all()) and bool((buf[-GUARD:] == WORK_SENT).all()), "a guard zone of the work buffer was written"
        assert bool((rows[self.vcap:] == SENT).all()) and bool((tris[self.tcap:] == SENT).all()), "entries behind a cap were written"
        return rows, tris, self.counters.cpu().numpy().copy()


@pytest.fixture(scope="module")
def references():
    """The host mesh of every (shape, kind) once."""
    out = {}
    for dims in cases.MESH_SHAPES:
        for kind in cases.KINDS:
            vol = cases.analytic_volume(kind, dims)
            out[(dims, kind)] = (vol,) + ms.mesh_host(vol["tsdf_w"], vol["rgb_w"], vol["origin"], vol["voxel"], full=True)
    return out


def _check_mesh(tag, vol, rows, tris, want_rows, want_tris, xyz):
    """Triangles exact; positions against the float64 ones `xyz` of the host statement; colour bytes within 1."""
    assert np.array_equal(tris, want_tris), "triangle indices"
    assert len(rows) == len(want_rows) == len(xyz)
    if len(want_rows) == 0:
        return
    err = np.abs(pc.rows_xyz(rows).astype(np.float64) - xyz)
    bound = 2.0 ** -24 * np.abs(xyz) + 2.0 ** -40 * (np.abs(vol["origin"]) + vol["voxel"] * np.array(vol["dims"], dtype=np.float64))[None, :]
    dcol = np.abs(pc.rows_rgba(rows).astype(np.int64) - pc.rows_rgba(want_rows).astype(np.int64))
    differ = int((pc.rows_xyz(rows).view(np.int32) != pc.rows_xyz(want_rows).view(np.int32)).sum())
    print(f"MESHERR mesh {tag}: {len(rows)} vertices, {len(tris)} triangles; max position err / bound = {float((err / bound).max()):.3f}, {differ} of {3 * len(rows)} components "
          f"differ from the host's float32; max colour byte difference {int(dcol.max())}")
    assert bool((err <= bound).all())
    assert int(dcol.max()) <= 1 and bool((pc.rows_rgba(rows)[:, 3] == 255).all())


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("dims", cases.MESH_SHAPES)
def test_mesh_against_the_host_statement(references, dims, kind):
    vol, want_rows, want_tris, want_c, xyz64 = references[(dims, kind)]
    V, T = len(want_rows), len(want_tris)
    dv = Volume(dims, vol["tsdf_w"], vol["rgb_w"])
    outs = []
    for fill in (0x00, 0xFF):      # the work buffer's contents are irrelevant before plan
        m = Mesher(dv, vol["origin"], vol["voxel"], V, T, work_fill=fill)
        assert m.plan() == 0
        assert m.counters.cpu().tolist() == [V, T, 0, 0, 0, 0, 0, 0]
        assert m.emit() == 0
        rows, tris, c = m.read()
        assert c.tolist() == [V, T, V, T, 0, 0, 0, 0]
        outs.append((rows[:V].tobytes(), tris[:T].tobytes()))
    assert outs[0] == outs[1]
    _check_mesh(f"{dims} {kind}", vol, rows[:V], tris[:T], want_rows, want_tris, xyz64)
    # the topology of the device's own output
    topo = ms.mesh_topology(V, tris[:T])
    print(f"MESHERR mesh {dims} {kind}: {topo}")
    assert topo["unreferenced"] == 0 and topo["repeated"] == 0
    if dims[0] == dims[1] == dims[2] and dims[0] >= 17 and kind != "plane":
        assert topo["closed"] and topo["euler"] == (2 if kind == "sphere" else 0)
        xyz = pc.rows_xyz(rows[:V]).astype(np.float64)
        assert ms.signed_volume(xyz, tris[:T]) > 0 and bool((np.abs(cases.distance(kind, dims, xyz)) <= np.sqrt(3.0) * vol["voxel"]).all())
    if dims == (2, 2, 2) and kind == "plane":
        assert T > 0      # the one cube is cut
    # the volume itself is read only
    tw, rw, _ = dv.read()
    assert tw.tobytes() == vol["tsdf_w"].tobytes() and rw.tobytes() == vol["rgb_w"].tobytes()


def test_half_known_volume_gives_an_open_surface_with_every_vertex_referenced():
    dims = (17, 17, 17)
    vol = cases.analytic_volume("sphere", dims, half_known=True)
    want_rows, want_tris, _, xyz64 = ms.mesh_host(vol["tsdf_w"], vol["rgb_w"], vol["origin"], vol["voxel"], full=True)
    V, T = len(want_rows), len(want_tris)
    m = Mesher(Volume(dims, vol["tsdf_w"], vol["rgb_w"]), vol["origin"], vol["voxel"], V, T, work_fill=0xFF)
    assert m.plan() == 0 and m.emit() == 0
    rows, tris, c = m.read()
    topo = ms.mesh_topology(V, tris[:T])
    print(f"MESHERR mesh half-known sphere: counters {c.tolist()}, {topo}")
    assert c.tolist() == [V, T, V, T, 0, 0, 0, 0] and T > 0
    _check_mesh("half-known sphere", vol, rows[:V], tris[:T], want_rows, want_tris, xyz64)
    assert topo["boundary"] > 0 and topo["unreferenced"] == 0 and topo["repeated"] == 0
    # min_weight above every weight: nothing is known, an empty mesh
    m2 = Mesher(m.vol, vol["origin"], vol["voxel"], V, T, min_weight=2.0)
    assert m2.plan() == 0 and m2.emit() == 0
    assert m2.read()[2].tolist() == [0] * 8 and bool((m2.rows.cpu().numpy() == SENT).all()) and bool((m2.tris.cpu().numpy() == SENT).all())


def test_caps_below_the_totals_end_as_counts(references):
    dims, kind = (17, 9, 6), "sphere"
    vol, want_rows, want_tris = references[(dims, kind)][:3]
    V, T = len(want_rows), len(want_tris)
    assert V > 20 and T > 20
    dv = Volume(dims, vol["tsdf_w"], vol["rgb_w"])
    for vcap, tcap in ((V // 2, T), (V, T // 3), (V // 2, T // 3), (0, 0)):
        m = Mesher(dv, vol["origin"], vol["voxel"], vcap, tcap)
        assert m.plan() == 0 and m.emit() == 0
        rows, tris, c = m.read()      # (checks that nothing behind the caps was written)
        ok = (np.arange(T) < tcap) & (want_tris < vcap).all(1)
        print(f"MESHERR caps vcap {vcap} of {V}, tcap {tcap} of {T}: counters {c.tolist()}, {int(ok.sum())} triangles expected")
        assert c.tolist() == [V, T, min(V, vcap), int(ok.sum()), V - min(V, vcap), T - int(ok.sum()), 0, 0]
        assert np.array_equal(rows[:vcap, 3], want_rows[:vcap, 3])
        assert np.array_equal(tris[:tcap][ok[:tcap]], want_tris[:tcap][ok[:tcap]])
        assert bool((tris[:tcap][~ok[:tcap]] == SENT).all())      # a dropped triangle's place keeps what it held
    # NULL rows and triangles are fine with caps of 0
    m = Mesher(dv, vol["origin"], vol["voxel"], 0, 0)
    assert m.plan() == 0 and m.emit(rows=None, tris=None) == 0
    assert m.counters.cpu().tolist() == [V, T, 0, 0, V, T, 0, 0]


def test_rejected_calls_return_minus_one_and_write_nothing():
    dims = (17, 9, 6)
    H, W = 17, 33
    case = cases.integrate_case(dims, H, W, "sil_edge")
    vd = to_dev(case["views"][0])
    vol = cases.analytic_volume("sphere", dims)
    dv = Volume(dims, vol["tsdf_w"], vol["rgb_w"])
    m = Mesher(dv, vol["origin"], vol["voxel"], 64, 64)
    before = {"tw": dv.tw.cpu(), "rw": dv.rw.cpu(), "counters": dv.counters.cpu(), "buf": m.buf.cpu(), "rows": m.rows.cpu(), "tris": m.tris.cpu(), "mc": m.counters.cpu()}
    nan, inf = float("nan"), float("inf")
    lib = _lib()
    bad = {
        **pcases.view_faults(vd["pose"].data_ptr()),
        "nx = 1": dict(nx=1), "ny = 0": dict(ny=0), "nz < 0": dict(nz=-4), "more than 2^30 samples": dict(nx=1025, ny=1024, nz=1024), "a product that wraps": dict(nx=1 << 16, ny=1 << 16, nz=1 << 16),
        "NULL color": dict(color=None), "NULL depth": dict(depth=None), "NULL origin": dict(origin=None), "NULL tsdf_w": dict(tsdf_w=None),
        "NULL rgb_w": dict(rgb_w=None), "NULL counters": dict(counters=None),
        "voxel = 0": dict(voxel=0.0), "voxel < 0": dict(voxel=-0.01), "voxel NaN": dict(voxel=nan), "voxel inf": dict(voxel=inf),
        "trunc = 0": dict(trunc=0.0), "trunc < 0": dict(trunc=-0.1), "trunc NaN": dict(trunc=nan), "trunc inf": dict(trunc=inf),
        "origin NaN": dict(origin=[0.0, nan, 0.0]), "origin inf": dict(origin=[inf, 0.0, 0.0]),
        "misaligned tsdf_w": dict(tsdf_w=dv.tw.data_ptr() + 4), "misaligned rgb_w": dict(rgb_w=dv.rw.data_ptr() + 8), "misaligned counters": dict(counters=dv.counters.data_ptr() + 4),
        "misaligned color": dict(color=vd["color"].data_ptr() + 2), "misaligned depth": dict(depth=vd["depth"].data_ptr() + 1), "misaligned sil": dict(sil=vd["sil"].data_ptr() + 3),
    }
    for what, over in bad.items():
        assert dv.integrate(vd, case, **over) == -1, what
        assert lib.mm3dgs_last_error(), what
    bad_plan = {"nx = 1": dict(nx=1), "more than 2^30 samples": dict(nx=1025, ny=1024, nz=1024), "NULL tsdf_w": dict(tsdf_w=None), "NULL work": dict(work=None),
                "NULL counters": dict(counters=None), "min_weight NaN": dict(min_weight=nan), "misaligned tsdf_w": dict(tsdf_w=dv.tw.data_ptr() + 4),
                "misaligned work": dict(work=m.work + 4), "misaligned counters": dict(counters=m.counters.data_ptr() + 4)}
    for what, over in bad_plan.items():
        assert m.plan(**over) == -1, what
        assert lib.mm3dgs_last_error(), what
    bad_emit = {"nz = 1": dict(nz=1), "more than 2^30 samples": dict(nx=1025, ny=1024, nz=1024), "NULL tsdf_w": dict(tsdf_w=None), "NULL rgb_w": dict(rgb_w=None),
                "NULL origin": dict(origin=None), "NULL work": dict(work=None), "NULL rows": dict(rows=None), "NULL triangles": dict(tris=None), "NULL counters": dict(counters=None),
                "voxel = 0": dict(voxel=0.0), "voxel NaN": dict(voxel=nan), "voxel inf": dict(voxel=inf), "origin NaN": dict(origin=_origin([nan, 0, 0])),
                "misaligned rows": dict(rows=m.rows.data_ptr() + 8), "misaligned rgb_w": dict(rgb_w=dv.rw.data_ptr() + 8), "misaligned tsdf_w": dict(tsdf_w=dv.tw.data_ptr() + 4),
                "misaligned work": dict(work=m.work + 4), "misaligned triangles": dict(tris=m.tris.data_ptr() + 2), "misaligned counters": dict(counters=m.counters.data_ptr() + 4)}
    for what, over in bad_emit.items():
        assert m.emit(**over) == -1, what
        assert lib.mm3dgs_last_error(), what
    assert lib.mm3dgs_tsdf_reset(1, 9, 6, _ptr(dv.tw), _ptr(dv.rw), _ptr(dv.counters), _stream()) == -1
    assert lib.mm3dgs_tsdf_reset(17, 9, 6, None, _ptr(dv.rw), _ptr(dv.counters), _stream()) == -1
    assert lib.mm3dgs_tsdf_reset(17, 9, 6, _ptr(dv.tw), _ptr(dv.rw.data_ptr() + 8), _ptr(dv.counters), _stream()) == -1
    assert lib.mm3dgs_tsdf_reset(17, 9, 6, _ptr(dv.tw), _ptr(dv.rw), None, _stream()) == -1
    torch.cuda.synchronize()
    now = {"tw": dv.tw, "rw": dv.rw, "counters": dv.counters, "buf": m.buf, "rows": m.rows, "tris": m.tris, "mc": m.counters}
    for name, t in before.items():
        a, b = now[name].cpu(), t
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), name
    for shape in ((1, 9, 6), (17, 0, 6), (17, 9, -1), (1025, 1024, 1024), (1 << 16, 1 << 16, 1 << 16)):
        assert int(lib.mm3dgs_tsdf_mesh_work_bytes(*shape)) == 0, shape
    assert dv.integrate(vd, case) == 0 and dv.integrate(vd, case, sil=None) == 0      # the silhouette is optional
    assert m.plan() == 0 and m.emit() == 0


def test_view_fault_texts():
    dims, (H, W) = (17, 9, 6), (17, 33)
    case = cases.integrate_case(dims, H, W, "all")
    vd, vol = to_dev(case["views"][0]), Volume(dims)
    for over, text in pcases.view_fault_texts("tsdf_integrate", H, W, vd["pose"].data_ptr(), "the images and the pose must be 4-byte aligned"):
        assert vol.integrate(vd, case, **over) == -1 and _lib().mm3dgs_last_error().decode() == text, over


PARENT_KEYS = ["pose_est", "pose_gt", "keyframes", "ate_rmse", "psnr_list", "ssim_list", "lpips_list"]
MESH = {"voxel": 0.08}


def _run(tmp, export, frames=4):
    """The small native run of tests/test_gpu_pointcloud.py::_run (48 x 64, 4 frames), with the mesh block."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device=DEV, height=48, width=64, tracking={"iters": 5}, mapping={"iters": 6, "kf_every": 2, "min_covisibility": 2.0},
                         outputdir=str(tmp), debug={"get_runtime_stats": False, "create_video": False, "save_keyframes": False},
                         eval_every=1, eval_on_device=False, mesh=dict(MESH, export=export))
    seq = SyntheticSequence(cfg, frames, 2000, seed=5)
    slam = SLAM(cfg, seq)
    from mm3dgs_slam_amd.fused import FusedMapper, FusedTracker
    assert isinstance(slam.tracker, FusedTracker) and isinstance(slam.mapper, FusedMapper)
    slam.run()
    return slam, seq, cfg


def _same(a, b):
    """Byte-for-byte equality of two results.npz entries (object arrays: of their lists and dicts, leaf by leaf)."""
    if isinstance(a, np.ndarray) and a.dtype == object:
        return isinstance(b, np.ndarray) and a.shape == b.shape and all(_same(p, q) for p, q in zip(a.reshape(-1), b.reshape(-1)))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(p, q) for p, q in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    return np.asarray(a).dtype == np.asarray(b).dtype and np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_native_run_exports_its_mesh_and_the_checkpoint_reproduces_it(tmp_path):
    import slam_top
    n = 4
    on_dir, off_dir = tmp_path / "on", tmp_path / "off"
    on, seq, cfg_on = _run(on_dir, True, n)
    off, _, cfg_off = _run(off_dir, False, n)
    a = np.load(on_dir / "results.npz", allow_pickle=True)
    b = np.load(off_dir / "results.npz", allow_pickle=True)
    assert a["pose_est"].shape == (n, 7) and list(a.keys()) == list(b.keys()) == PARENT_KEYS
    for key in PARENT_KEYS:      # (the two archives differ in their members' time stamps only: every array byte for byte)
        assert _same(a[key], b[key]), key
    assert all(torch.equal(p, q) for p, q in zip(on.estimate_pose_list, off.estimate_pose_list))
    assert off.mesh_export is None and not (off_dir / "mesh").exists()
    out = on.mesh_export
    c = out["counters"]
    print(f"MESHERR run: {c}, lattice {out['lattice']}")
    mesh_bytes = (on_dir / "mesh" / "mesh.ply").read_bytes()
    rows, tris = ms.read_mesh_ply(out["mesh"])
    assert out["mesh"] == str(on_dir / "mesh" / "mesh.ply") and len(rows) == c["vertices"] > 0 and len(tris) == c["triangles"] > 0 and c["views"] == 2
    assert mesh_bytes[:len(ms.mesh_header(len(rows), len(tris)))] == ms.mesh_header(len(rows), len(tris)).encode("ascii")
    topo = ms.mesh_topology(len(rows), tris)
    assert topo["unreferenced"] == 0 and topo["repeated"] == 0 and 0 <= tris.min() and tris.max() < len(rows)
    # a volume driven by hand over renderer.render at the stored poses (every = mapping.kf_every = 2: frames 0 and 2), on the host
    nx, ny, nz = out["lattice"]
    tsdf_w, rgb_w = ms.empty_volume(nx, ny, nz)
    cam = {k: cfg_on["cam"][k] for k in ("fx", "fy", "cx", "cy")}
    with torch.no_grad():
        for idx in (0, 2):
            pose = torch.tensor(a["pose_est"][idx], device=DEV)
            r = on.renderer.render(on.gaussians, camera_pose=pose)
            ms.integrate_host(tsdf_w, rgb_w, r["render"], r["depth"][0], r["depth"][1], pose, **cam, origin=out["origin"], voxel=out["voxel"], trunc=out["trunc"], sil_min=0.99)
    want = ms.mesh_host(tsdf_w, rgb_w, out["origin"], out["voxel"], 1.0)
    print(f"MESHERR run: host statement over the same views {len(want[0])} vertices, {len(want[1])} triangles")
    assert len(want[0]) == len(rows) and np.array_equal(want[1], tris)
    # the checkpoint route, from the files of the run without the export: only mesh/ is added, the same file
    before = (off_dir / "results.npz").read_bytes()
    listing = sorted(os.listdir(off_dir))
    ck = slam_top.export_mesh_checkpoint(dict(cfg_off, mesh=dict(MESH, export=False)), seq)
    assert ck["iteration"] == n and ck["counters"] == c and ck["lattice"] == out["lattice"]
    assert (off_dir / "mesh" / "mesh.ply").read_bytes() == mesh_bytes
    assert (off_dir / "results.npz").read_bytes() == before and sorted(os.listdir(off_dir)) == sorted(listing + ["mesh"])
    # a lattice above max_voxels is an error that names the key
    cfg_on["mesh"]["max_voxels"] = 1000
    with pytest.raises(ValueError, match=r"mesh\.max_voxels = 1000"):
        on.export_mesh()


def test_both_device_builders_reject_a_wrong_shaped_view_before_any_launch():
    """`pointcloud.device_view`, the view contract of PointCloudBuilder.add and TsdfVolume.add: a colour or silhouette tensor of the wrong
    shape is a ValueError that names the caller's class, raised before a launch -- both builders' counters read the same afterwards."""
    H, W = 2, 3
    cam = {"fx": 4.0, "fy": 4.0, "cx": 1.0, "cy": 0.5}
    color, depth, sil = torch.rand(3, H, W, device=DEV), torch.full((H, W), 1.5, device=DEV), torch.ones(H, W, device=DEV)
    pose = torch.tensor([1.0, 0, 0, 0, 0, 0, 0], device=DEV)
    cloud = pc.PointCloudBuilder(H, W, cam, voxel=0.01, max_points=64, device=DEV)
    volume = ms.TsdfVolume((4, 4, 4), [-1.0, -1.0, 0.5], 0.5, 2.0, H, W, cam, device=DEV)
    for builder, name in ((cloud, "PointCloudBuilder"), (volume, "TsdfVolume")):
        builder.add(color, depth, sil, pose)      # a good view first: the counters are not all zero
        before = builder.counters.cpu().clone()
        assert int(before[6 if builder is cloud else 0]) == 1, before
        for bad in ((torch.rand(3, W, H, device=DEV), depth, sil, pose), (color, depth, torch.ones(H, W + 1, device=DEV), pose),
                    (torch.rand(4, H, W, device=DEV), depth, None, pose)):
            with pytest.raises(ValueError, match=name + r"\.add: color \[3,2,3\]"):
                builder.add(*bad)
        torch.cuda.synchronize()
        assert torch.equal(builder.counters.cpu(), before), (name, before, builder.counters.cpu())
    assert cloud.view == 1
