"""mm3dgs_pointcloud_add_view (csrc/pointcloud.hip) through the raw C ABI against the host statement of mm3dgs_slam_amd/pointcloud.py, at
the shapes where a count / scan / scatter compaction can break (one pixel, exactly one workgroup, a partial last one, a second round of the
1024-wide scan) and with every validity pattern of the pixel test; the voxel selection against the host's first-occurrence selection, bit for
bit; handled overflow; rejected calls; and the export of a native-loop run.

Bars: rgba, counts and row order exact.  A position component: |device - float64| <= 2^-24 |float64| + 2^-40 scale, scale = |R|^T (|p_c| +
|t|) -- the one rounding to float32 at the store, plus 10^4 times the double roundoff (1.1e-16) of the roughly ten double operations before
it.  With a voxel size the expected rows are the host selection applied to the device's own unthinned rows, so that stage is exact.
Every test prints its figures (`PCDERR ...`, pytest -s) before it asserts."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import pointcloud as pc
from tests import pointcloud_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096               # bytes of guard zone on each side of the work buffer
PAD = 8                    # rows behind `cap` that no call may touch
SENT = 0x7A7A7A7A          # every int32 of an untouched row
WORK_SENT = 0xA5           # every byte of the guard zones


def _ptr(t):
    return None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _lib():
    from mm3dgs_slam_amd import _lib
    return _lib.load()


def _stream():
    from mm3dgs_slam_amd.rasterizer import _stream
    return _stream()


def to_dev(v):
    out = dict(v)
    for k in ("color", "depth", "sil", "pose"):
        out[k] = None if v[k] is None else torch.from_numpy(np.ascontiguousarray(v[k])).to(DEV)
    return out


def host_rows(v, full=False):
    return pc.backproject_host(v["color"], v["depth"], v["sil"], v["pose"], **v["cam"], sil_min=v["sil_min"], depth_max=v["depth_max"], full=full)


class Cloud:
    """Caller-owned buffers of one cloud: sentinel-filled rows (cap + PAD), the table, the counters, the work buffer between guard zones."""

    def __init__(self, H, W, cap, voxel=0.0, slots=None, work_fill=0x00):
        self.H, self.W, self.cap, self.voxel = H, W, cap, float(voxel)
        self.rows = torch.full((cap + PAD, 4), SENT, dtype=torch.int32, device=DEV)
        self.slots = 0
        self.table = None
        if voxel > 0:
            self.slots = slots or max(64, 1 << int(2 * cap - 1).bit_length())
            self.table = torch.empty(self.slots, 2, dtype=torch.int64, device=DEV)
        self.counters = torch.full((8,), -7, dtype=torch.int64, device=DEV)
        self.nwork = int(_lib().mm3dgs_pointcloud_work_bytes(H, W))
        assert self.nwork > 0 and self.nwork % 8 == 0
        self.buf = torch.full((2 * GUARD + self.nwork,), WORK_SENT, dtype=torch.uint8, device=DEV)
        self.buf[GUARD:GUARD + self.nwork] = work_fill
        self.work = self.buf.data_ptr() + GUARD
        self.view = 0
        assert _lib().mm3dgs_pointcloud_reset(_ptr(self.table), self.slots, _ptr(self.counters), _stream()) == 0
        torch.cuda.synchronize()
        assert not self.counters.cpu().any()
        if self.table is not None:
            assert bool((self.table.cpu() == -1).all())

    def call(self, v, view=None, **over):
        a = dict(H=self.H, W=self.W, fx=v["cam"]["fx"], fy=v["cam"]["fy"], cx=v["cam"]["cx"], cy=v["cam"]["cy"], pose=v["pose"], color=v["color"],
                 depth=v["depth"], sil=v["sil"], sil_min=v["sil_min"], depth_max=v["depth_max"], voxel=self.voxel, view=self.view if view is None else view,
                 rows=self.rows, cap=self.cap, table=self.table, slots=self.slots, counters=self.counters, work=self.work)
        a.update(over)
        rc = _lib().mm3dgs_pointcloud_add_view(a["H"], a["W"], a["fx"], a["fy"], a["cx"], a["cy"], _ptr(a["pose"]), _ptr(a["color"]), _ptr(a["depth"]),
                                               _ptr(a["sil"]), a["sil_min"], a["depth_max"], a["voxel"], a["view"], _ptr(a["rows"]), a["cap"], _ptr(a["table"]),
                                               a["slots"], _ptr(a["counters"]), _ptr(a["work"]), _stream())
        torch.cuda.synchronize()
        return rc

    def add(self, v, view=None):
        assert self.call(v, view) == 0
        self.view = (self.view if view is None else view) + 1

    def read(self):
        """(rows [n,4] int32, counters [8] int64) on the host, after checking the guards, the rows behind the count and the invariant."""
        c = self.counters.cpu().numpy()
        rows, buf = self.rows.cpu().numpy(), self.buf.cpu().numpy()
        n = int(c[0])
        assert 0 <= n <= self.cap and c[7] == 0 and bool((c >= 0).all()), c
        assert c[1] == c[0] + c[2] + c[3] + c[4] + c[5], c
        assert bool((rows[n:] == SENT).all()), "rows behind the count were written"
        assert bool((buf[:GUARD] == WORK_SENT).all()) and bool((buf[-GUARD:] == WORK_SENT).all()), "a guard zone of the work buffer was written"
        return rows[:n].copy(), c.copy()


@pytest.fixture(scope="module")
def views():
    """Every (shape, pattern) view once: the host arrays, the device tensors and the float64 host statement."""
    out = {}
    for H, W in cases.SHAPES:
        for pattern in cases.PATTERNS:
            v = cases.view(H, W, pattern)
            out[(H, W, pattern)] = (v, to_dev(v), host_rows(v, full=True))
    return out


@pytest.mark.parametrize("pattern", cases.PATTERNS)
@pytest.mark.parametrize("H,W", cases.SHAPES)
def test_unthinned_rows_against_the_float64_host_statement(views, H, W, pattern):
    v, vd, (ref, xyz, scale, idx) = views[(H, W, pattern)]
    fills = (0x00, 0xFF) if (H, W) != (520, 520) else (0xFF,)      # the work buffer's contents are irrelevant: zeros, and NaN bytes
    for fill in fills:
        cloud = Cloud(H, W, H * W, work_fill=fill)
        cloud.add(vd)
        rows, c = cloud.read()
        assert c.tolist() == [len(ref), len(ref), 0, 0, 0, 0, 1, 0], (c, len(ref))
        assert np.array_equal(rows[:, 3], ref[:, 3])                                   # rgba exact; with the count: the host mask, in raster order
        got = pc.rows_xyz(rows).astype(np.float64)
        err, bound = np.abs(got - xyz), 2.0 ** -24 * np.abs(xyz) + 2.0 ** -40 * scale
        differ = int((pc.rows_xyz(rows).view(np.int32) != pc.rows_xyz(ref).view(np.int32)).sum())
        print(f"PCDERR unthinned {H}x{W} {pattern} fill {fill:#04x}: {len(rows)} rows of {H * W} pixels; max err / bound = "
              f"{float((err / bound).max()) if len(rows) else 0.0:.3f}; {differ} of {3 * len(rows)} components differ from the host's float32")
        assert bool((err <= bound).all())
    if pattern in ("checker", "planted", "sil_edge", "depth_max_edge"):
        assert 0 < len(ref) < H * W or H * W == 1
    if pattern == "last":
        assert idx.tolist() == [H * W - 1]


def test_unthinned_views_append_behind_the_rows_already_there(views):
    H, W = 17, 33
    a, b = views[(H, W, "checker")], views[(H, W, "planted")]
    cloud = Cloud(H, W, 2 * H * W)
    cloud.add(a[1])
    first, _ = cloud.read()
    cloud.add(b[1])
    rows, c = cloud.read()
    assert c[0] == len(a[2][0]) + len(b[2][0]) and c[6] == 2
    assert rows[:len(first)].tobytes() == first.tobytes() and np.array_equal(rows[len(first):, 3], b[2][0][:, 3])


def _unthinned(vd, H, W):
    cloud = Cloud(H, W, H * W)
    cloud.add(vd)
    return cloud.read()[0]


@pytest.mark.parametrize("H,W", [(17, 33), (520, 520)])
def test_one_thinned_view_equals_the_host_selection_of_the_devices_rows(H, W):
    v = cases.plane_view(H, W)
    vd = to_dev(v)
    base = _unthinned(vd, H, W)
    xyz = pc.rows_xyz(base)
    assert float(xyz.min()) > 0.0 and float(xyz.max()) < 16.0      # every point in the positive octant: one huge voxel holds them all
    for name, voxel in (("huge", 1000.0), ("tiny", 2.0 ** -16), ("between", 3.3 * cases.footprint(v))):
        want = base[pc.voxel_select_host(xyz, voxel)]
        cloud = Cloud(H, W, H * W, voxel=voxel)
        cloud.add(vd)
        rows, c = cloud.read()
        print(f"PCDERR thinned {H}x{W} {name} voxel {voxel:.3g}: {len(rows)} rows (host {len(want)}) of {len(base)} valid, counters {c.tolist()}")
        assert rows.tobytes() == want.tobytes()
        assert c.tolist() == [len(want), len(base), len(base) - len(want), 0, 0, 0, 1, 0]
        if name == "huge":
            assert len(rows) == 1 and rows.tobytes() == base[:1].tobytes()      # maximal contention on one slot: the first pixel wins
        elif name == "tiny":
            assert rows.tobytes() == base.tobytes()                             # nothing merges
        else:
            assert 1 < len(rows) < len(base)


def _stream_views(H, W):
    return [cases.plane_view(H, W, k, shift=(0.06 * k, -0.03 * k, 0.02 * k)) for k in range(3)]


def _run_stream(H, W, vds, voxel, work_fill=0x00, cap=None):
    cloud = Cloud(H, W, cap or 3 * H * W, voxel=voxel, work_fill=work_fill)
    for vd in vds:
        cloud.add(vd)
    return cloud


@pytest.mark.parametrize("H,W", [(17, 33), (48, 64)])
def test_streamed_views_keep_the_first_point_that_reached_a_voxel(H, W):
    vs = _stream_views(H, W)
    vds = [to_dev(v) for v in vs]
    voxel = 3.3 * cases.footprint(vs[0])
    bases = [_unthinned(vd, H, W) for vd in vds]
    seen, want = set(), []
    for b in bases:
        want.append(b[pc.voxel_select_host(pc.rows_xyz(b), voxel, seen)])
    # the same as one selection over the concatenated stream
    cat = np.concatenate(bases)
    assert np.concatenate(want).tobytes() == cat[pc.voxel_select_host(pc.rows_xyz(cat), voxel)].tobytes()
    cloud = _run_stream(H, W, vds, voxel)
    rows, c = cloud.read()
    print(f"PCDERR stream {H}x{W}: rows per view {[len(w) for w in want]} of {[len(b) for b in bases]} valid, counters {c.tolist()}")
    assert rows.tobytes() == np.concatenate(want).tobytes()
    assert len(want[1]) > 0 and len(want[1]) < len(bases[1])      # the second view adds some voxels and merges into others
    assert c.tolist() == [len(rows), len(cat), len(cat) - len(rows), 0, 0, 0, 3, 0]
    # the first view again, under a larger view number: no new row, every valid pixel merges
    cloud.add(vds[0])
    rows2, c2 = cloud.read()
    assert rows2.tobytes() == rows.tobytes()
    assert c2.tolist() == [c[0], c[1] + len(bases[0]), c[2] + len(bases[0]), 0, 0, 0, 4, 0]


def test_fresh_builders_repeat_their_bytes_whatever_the_work_buffer_held():
    H, W = 48, 64
    vs = _stream_views(H, W)
    vds = [to_dev(v) for v in vs]
    voxel = 3.3 * cases.footprint(vs[0])
    a, b, c = (_run_stream(H, W, vds, voxel, fill).read() for fill in (0x00, 0x00, 0xFF))
    assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and len(a[0]) > 0
    assert a[1].tolist() == b[1].tolist() == c[1].tolist()


def test_a_full_row_buffer_and_a_full_table_end_as_counts():
    H, W = 17, 33
    v = cases.plane_view(H, W)
    vd = to_dev(v)
    base = _unthinned(vd, H, W)
    # cap smaller than the points, without and with a voxel size
    cap = 100
    cloud = Cloud(H, W, cap)
    cloud.add(vd)
    rows, c = cloud.read()      # (checks that the rows behind cap keep the sentinel)
    assert c.tolist() == [cap, len(base), 0, 0, 0, len(base) - cap, 1, 0] and rows.tobytes() == base[:cap].tobytes()
    voxel = 2.0 ** -16
    cloud = Cloud(H, W, cap, voxel=voxel, slots=2048)
    cloud.add(vd)
    rows, c = cloud.read()
    assert c.tolist() == [cap, len(base), 0, 0, 0, len(base) - cap, 1, 0] and rows.tobytes() == base[:cap].tobytes()
    cloud.add(vd)               # the buffer stays full: the voxels are known, every pixel merges
    rows, c2 = cloud.read()
    assert c2.tolist() == [cap, 2 * len(base), len(base), 0, 0, len(base) - cap, 2, 0]
    # a 64-slot table and more than 64 distinct voxels
    first = base[pc.voxel_select_host(pc.rows_xyz(base), voxel)]
    assert len(first) > 64
    cloud = Cloud(H, W, H * W, voxel=voxel, slots=64)
    cloud.add(vd)
    rows, c = cloud.read()
    print(f"PCDERR 64-slot table: {len(rows)} rows of {len(first)} voxels, counters {c.tolist()}")
    assert 0 < c[0] <= 64 and c[4] > 0 and c[4] == len(base) - c[0] - c[2]
    keys = {r.tobytes(): k for k, r in enumerate(first)}
    order = [keys[r.tobytes()] for r in rows]                 # every row is one of the host's first-occurrence rows ...
    assert order == sorted(order) and len(set(order)) == len(order)      # ... once, in raster order
    # the Python builder reports it
    b = pc.PointCloudBuilder(H, W, v["cam"], voxel=0.0, max_points=cap, sil_min=v["sil_min"], depth_max=0.0, device=DEV)
    b.add(vd["color"], vd["depth"], None, vd["pose"])
    with pytest.raises(RuntimeError, match=r"pointcloud\.max_points"):
        b.finish()
    assert b.read_counters()["capacity_dropped"] == len(base) - cap and b.rows().cpu().numpy().tobytes() == base[:cap].tobytes()


def test_points_beyond_the_cell_range_are_counted_and_absent():
    H, W = 17, 33
    v = cases.plane_view(H, W)
    voxel = 2.0 ** -16                                   # 2^20 cells end at 16 m
    v["depth"].reshape(-1)[10::50] = 40.0                # far beyond it
    vd = to_dev(v)
    base = _unthinned(vd, H, W)
    keys, ok = pc.voxel_keys(pc.rows_xyz(base), voxel)
    assert 0 < int((~ok).sum()) == int((v["depth"] == 40.0).sum())
    cloud = Cloud(H, W, H * W, voxel=voxel)
    cloud.add(vd)
    rows, c = cloud.read()
    want = base[pc.voxel_select_host(pc.rows_xyz(base), voxel)]
    print(f"PCDERR out of range: {int((~ok).sum())} points beyond 2^20 cells, counters {c.tolist()}")
    assert rows.tobytes() == want.tobytes() and c[3] == int((~ok).sum()) and c[0] == len(base) - c[3] and float(pc.rows_xyz(rows).max()) < 16.0


def test_rejected_calls_return_minus_one_and_write_nothing():
    H, W = 17, 33
    v = cases.view(H, W, "sil_edge")
    vd = to_dev(v)
    cloud = Cloud(H, W, H * W, voxel=0.05)
    before = {"rows": cloud.rows.cpu(), "table": cloud.table.cpu(), "counters": cloud.counters.cpu(), "buf": cloud.buf.cpu()}
    nan, inf = float("nan"), float("inf")
    bad = {
        **cases.view_faults(vd["pose"].data_ptr()),
        "NULL color": dict(color=None), "NULL depth": dict(depth=None), "NULL rows": dict(rows=None),
        "NULL counters": dict(counters=None), "NULL work": dict(work=None),
        "voxel < 0": dict(voxel=-0.01), "voxel NaN": dict(voxel=nan), "voxel inf": dict(voxel=inf),
        "voxel > 0 without a table": dict(table=None), "slots not a power of two": dict(slots=96), "slots below 64": dict(slots=32), "slots 0": dict(slots=0),
        "misaligned rows": dict(rows=cloud.rows.data_ptr() + 8), "misaligned table": dict(table=cloud.table.data_ptr() + 8),
        "misaligned counters": dict(counters=cloud.counters.data_ptr() + 4), "misaligned work": dict(work=cloud.work + 4),
        "misaligned color": dict(color=vd["color"].data_ptr() + 2), "misaligned depth": dict(depth=vd["depth"].data_ptr() + 1),
        "misaligned sil": dict(sil=vd["sil"].data_ptr() + 3),
    }
    for what, over in bad.items():
        assert cloud.call(vd, **over) == -1, what
        assert _lib().mm3dgs_last_error(), what
    lib = _lib()
    assert lib.mm3dgs_pointcloud_reset(_ptr(cloud.table), cloud.slots, None, _stream()) == -1
    assert lib.mm3dgs_pointcloud_reset(_ptr(cloud.table), 96, _ptr(cloud.counters), _stream()) == -1
    assert lib.mm3dgs_pointcloud_reset(_ptr(cloud.table.data_ptr() + 8), cloud.slots, _ptr(cloud.counters), _stream()) == -1
    assert lib.mm3dgs_pointcloud_reset(_ptr(cloud.table), cloud.slots, _ptr(cloud.counters.data_ptr() + 4), _stream()) == -1
    torch.cuda.synchronize()
    for name, t in before.items():
        assert torch.equal(getattr(cloud, name).cpu(), t), name
    for shape in ((0, W), (H, 0), (-1, W), (H, -1), (1 << 14, (1 << 14) + 1)):
        assert int(lib.mm3dgs_pointcloud_work_bytes(*shape)) == 0, shape
    assert cloud.call(vd) == 0 and cloud.call(vd, sil=None, view=1) == 0      # the silhouette is optional


def test_view_fault_texts():
    H, W = 17, 33
    vd = to_dev(cases.view(H, W, "all"))
    cloud = Cloud(H, W, H * W)
    for over, text in cases.view_fault_texts("pointcloud_add_view", H, W, vd["pose"].data_ptr(), "the images and the pose must be 4-byte aligned"):
        assert cloud.call(vd, **over) == -1 and _lib().mm3dgs_last_error().decode() == text, over


PARENT_KEYS = ["pose_est", "pose_gt", "keyframes", "ate_rmse", "psnr_list", "ssim_list", "lpips_list"]
POINTCLOUD = {"voxel": 0.02, "max_points": 1 << 16}


def _run(tmp, export, frames=4):
    """The small native run of tests/test_gpu_eval.py::_run (48 x 64, 4 frames), with the point cloud block."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device=DEV, height=48, width=64, tracking={"iters": 5}, mapping={"iters": 6, "kf_every": 2, "min_covisibility": 2.0},
                         outputdir=str(tmp), debug={"get_runtime_stats": False, "create_video": False, "save_keyframes": False},
                         eval_every=1, eval_on_device=False, pointcloud=dict(POINTCLOUD, export=export))
    seq = SyntheticSequence(cfg, frames, 2000, seed=5)
    slam = SLAM(cfg, seq)
    from mm3dgs_slam_amd.fused import FusedMapper, FusedTracker
    assert isinstance(slam.tracker, FusedTracker) and isinstance(slam.mapper, FusedMapper)
    slam.run()
    return slam, seq, cfg


def test_native_run_exports_its_cloud_and_the_checkpoint_reproduces_it(tmp_path):
    import slam_top
    n = 4
    on_dir, off_dir = tmp_path / "on", tmp_path / "off"
    on, seq, cfg_on = _run(on_dir, True, n)
    off, _, cfg_off = _run(off_dir, False, n)
    a = np.load(on_dir / "results.npz", allow_pickle=True)
    b = np.load(off_dir / "results.npz", allow_pickle=True)
    assert a["pose_est"].shape == (n, 7) and a["pose_est"].tobytes() == b["pose_est"].tobytes()
    assert list(a.keys()) == list(b.keys()) == PARENT_KEYS
    assert off.pointcloud_export is None and not (off_dir / "pointcloud").exists()
    out = on.pointcloud_export
    c = out["counters"]
    cloud_bytes = (on_dir / "pointcloud" / "cloud.ply").read_bytes()
    rows = pc.read_ply(out["cloud"])
    print(f"PCDERR run: {c}")
    assert out["cloud"] == str(on_dir / "pointcloud" / "cloud.ply") and len(rows) == c["rows"] > 0 and c["views"] == 2 and c["merged"] > 0
    assert cloud_bytes == pc.cloud_header(c["rows"]).encode("ascii") + rows.tobytes()
    assert len(np.unique(pc.voxel_keys(pc.rows_xyz(rows), POINTCLOUD["voxel"])[0])) == len(rows)
    # a builder driven by hand over renderer.render at the stored poses (every = mapping.kf_every = 2: frames 0 and 2)
    builder = pc.PointCloudBuilder(48, 64, cfg_on["cam"], voxel=POINTCLOUD["voxel"], max_points=POINTCLOUD["max_points"], sil_min=0.99, depth_max=0.0, device=DEV)
    with torch.no_grad():
        for idx in (0, 2):
            pose = torch.tensor(a["pose_est"][idx], device=DEV)
            r = on.renderer.render(on.gaussians, camera_pose=pose)
            builder.add(r["render"], r["depth"][0], r["depth"][1], pose)
    assert builder.finish() == c and builder.rows().cpu().numpy().tobytes() == rows.tobytes()
    xyz, rgb, edges = pc.read_trajectory_ply(out["trajectory"])
    assert len(xyz) == n and len(edges) == n - 1
    # the checkpoint route, from the files of the run without the export: only pointcloud/ is added, the same cloud
    before = (off_dir / "results.npz").read_bytes()
    listing = sorted(os.listdir(off_dir))
    cfg_ck = dict(cfg_off, pointcloud=dict(POINTCLOUD, export=False))
    ck = slam_top.export_pointcloud_checkpoint(cfg_ck, seq)
    assert ck["iteration"] == n and ck["counters"] == c
    assert (off_dir / "pointcloud" / "cloud.ply").read_bytes() == cloud_bytes
    assert (off_dir / "pointcloud" / "trajectory.ply").read_bytes() == (on_dir / "pointcloud" / "trajectory.ply").read_bytes()
    assert (off_dir / "results.npz").read_bytes() == before and sorted(os.listdir(off_dir)) == sorted(listing + ["pointcloud"])
    # the sensor source: one view, no thinning, one row per pixel with valid sensor depth
    s = on.export_pointcloud(path=str(tmp_path / "sensor"), every=100, voxel=0.0, source="sensor")
    d = seq[0][1]
    assert s["counters"]["views"] == 1 and s["counters"]["rows"] == int(((d > 0) & torch.isfinite(d)).sum()) == len(pc.read_ply(s["cloud"]))
    want = pc.backproject_host(seq[0][0], d, None, on.estimate_pose_list[0], **{k: cfg_on["cam"][k] for k in ("fx", "fy", "cx", "cy")})
    assert np.array_equal(pc.read_ply(s["cloud"])[:, 3], want[:, 3])
