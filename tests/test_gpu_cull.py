"""mm3dgs_cull_mark_view / mm3dgs_cull_select (csrc/cull.hip) through the raw C ABI against the float64 host statement cull.cull_host, bit
for bit -- seen, the kept rows, index and the counters are integers and copied bytes, and tests/cull_cases.py says why no comparison can
fall on the other side on the device --, at the sizes where a count / scan / scatter can break (one row, one workgroup and its neighbours,
the second round of the 1024-wide scan), on points exactly on and one ulp beside every bound, with all, no and only skipped rows; a cap
below the kept count; rejected calls; the Python surface; and a native run that culls its evaluation.  Every test prints its figures
(`CULLERR ...`, pytest -s) before it asserts."""
import json
import os
import random

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import cull as cl, geometry as geo, pointcloud as pc
from tests import cull_cases as cases, pointcloud_cases as pcases
from tests.test_gpu_geometry import _dev, _guarded, _guards_ok, _lib, _ptr, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 8                    # elements behind seen and the counters that no call may touch
SENT = 0x7A7A7A7A          # every int32 of an untouched output element (the bytes 0x7A)


class Cull:
    """Caller-owned buffers of the views and one select: out_rows, index and work between guard zones, sentinels behind seen and counters."""

    def __init__(self, scene, min_views=1, cap=None, fill=0x00):
        self.s, self.min_views = scene, min_views
        self.n = len(scene["rows"])
        self.cap = self.n if cap is None else cap
        self.rows = _dev(scene["rows"]) if self.n else torch.zeros(1, 4, dtype=torch.int32, device=DEV)
        self.views = [(None if d is None else _dev(d), _dev(p)) for d, p in scene["views"]]
        self.nwork = int(_lib().mm3dgs_cull_work_bytes(self.n))
        assert self.nwork > 0 and self.nwork % 8 == 0
        self.obuf, self.out = _guarded(16 * max(self.cap, 1), 0x7A)
        self.ibuf, self.index = _guarded(4 * max(self.cap, 1), 0x7A)
        self.wbuf, self.work = _guarded(self.nwork, fill)
        self.reset()

    def reset(self):
        self.seen = torch.full((self.n + PAD,), SENT, dtype=torch.int32, device=DEV)
        self.seen[:self.n] = 0
        self.counters = torch.full((8 + PAD,), -7, dtype=torch.int64, device=DEV)
        self.counters[:8] = 0

    def mark(self, view=0, **over):
        s = self.s
        depth, pose = self.views[view]
        a = dict(H=s["H"], W=s["W"], fx=s["fx"], fy=s["fy"], cx=s["cx"], cy=s["cy"], pose=pose, depth=depth, depth_max=s["depth_max"], near=s["near"], far=s["far"],
                 eps=s["eps"], n=self.n, rows=self.rows, seen=self.seen, counters=self.counters)
        a.update(over)
        rc = _lib().mm3dgs_cull_mark_view(a["H"], a["W"], a["fx"], a["fy"], a["cx"], a["cy"], _ptr(a["pose"]), _ptr(a["depth"]), a["depth_max"], a["near"], a["far"],
                                          a["eps"], a["n"], _ptr(a["rows"]), _ptr(a["seen"]), _ptr(a["counters"]), _stream())
        torch.cuda.synchronize()
        return rc

    def select(self, **over):
        a = dict(n=self.n, rows=self.rows, seen=self.seen, min_views=self.min_views, out=self.out, cap=self.cap, index=self.index, work=self.work,
                 counters=self.counters)
        a.update(over)
        rc = _lib().mm3dgs_cull_select(a["n"], _ptr(a["rows"]), _ptr(a["seen"]), a["min_views"], _ptr(a["out"]), a["cap"], _ptr(a["index"]), _ptr(a["work"]),
                                       _ptr(a["counters"]), _stream())
        torch.cuda.synchronize()
        return rc

    def run(self):
        for v in range(len(self.views)):
            assert self.mark(v) == 0
        assert self.select() == 0
        return self

    def snapshot(self):
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("seen", "counters", "obuf", "ibuf", "wbuf")}

    def read(self):
        """(seen uint32 [n], kept rows [written,4] int32, index uint32 [written], counters int64 [8]) after the guards and sentinels were checked."""
        s = self.snapshot()
        G = 4096
        assert _guards_ok(self.obuf) and _guards_ok(self.ibuf) and _guards_ok(self.wbuf), "a guard zone was written"
        assert bool((s["seen"][self.n:] == SENT).all()) and bool((s["counters"][8:] == -7).all()), "elements behind seen / counters were written"
        c = s["counters"][:8].copy()
        w = int(c[3])
        out, idx = s["obuf"][G:len(s["obuf"]) - G], s["ibuf"][G:len(s["ibuf"]) - G]
        assert bool((out[16 * w:] == 0x7A).all()) and bool((idx[4 * w:] == 0x7A).all()), "rows or indices behind the written count were written"
        return s["seen"][:self.n].view(np.uint32).copy(), out[:16 * w].view(np.int32).reshape(w, 4).copy(), idx[:4 * w].view(np.uint32).copy(), c


def _check(scene, min_views=1, cap=None, fill=0x00):
    kept, index, seen, counters = cl.cull_host(scene["rows"], scene["views"], min_views=min_views, cap=cap, **cases.options(scene))
    c = Cull(scene, min_views, cap, fill).run()
    dseen, dkept, dindex, dcounters = c.read()
    mode = "occlusion" if scene["views"][0][0] is not None else "frustum"
    print(f"CULLERR device {scene['name']} ({mode}, min_views {min_views}, cap {cap}, fill {fill:#04x}): counters {dcounters.tolist()}, host {counters.tolist()}; "
          f"{int((dseen != seen).sum())} of {len(seen)} seen counts differ, {int((dindex != index).sum()) if len(dindex) == len(index) else 'all'} indices differ")
    assert np.array_equal(dcounters, counters)
    assert np.array_equal(dseen, seen) and np.array_equal(dindex, index) and dkept.tobytes() == kept.tobytes()
    return c, (dseen, dkept, dindex, dcounters)


@pytest.mark.parametrize("hw", ((12, 16), (48, 64)))
@pytest.mark.parametrize("n", cases.SIZES)
def test_sizes_views_and_modes_against_the_host_statement(n, hw):
    for n_views in (1, 3):
        scene = cases.random_scene(n, H=hw[0], W=hw[1], n_views=n_views, seed=n + n_views)
        _check(scene, min_views=1, fill=0xFF if n % 2 else 0x00)
        _check(cases.frustum_only(scene), min_views=min(2, n_views))


def test_second_round_of_the_scan():
    scene = cases.random_scene(cases.SECOND_ROUND, H=48, W=64, n_views=3, seed=9)
    _, (seen, kept, index, counters) = _check(scene, fill=0xFF)
    assert 0 < counters[2] < cases.SECOND_ROUND and int(index[-1]) > 262144 - 4096      # kept rows beyond the first 1024 blocks of 256
    _check(cases.frustum_only(scene), min_views=2)


def test_analytic_scenes_on_and_beside_the_bounds():
    for s in cases.analytic_scenes():
        for mode, scene in (("occlusion", s), ("frustum", cases.frustum_only(s))):
            _, (seen, kept, index, counters) = _check(scene)
            want = s["want_" + mode]
            wrong = [f"{s['why'][i]}: seen {int(seen[i])}, want {int(want[i])}" for i in np.flatnonzero(seen.astype(bool) != want)]
            assert not wrong, wrong
            assert np.array_equal(index, np.flatnonzero(want))


def test_set_shapes():
    for s in cases.shape_scenes():
        _, (seen, kept, index, counters) = _check(s)
        assert counters.tolist() == [1, s["kept"], s["kept"], s["kept"], 0, s["skipped"], 0, 0], s["name"]
    # n = 0 with NULL rows, seen and out_rows: a valid call that updates the counters only
    c = Cull(cases.shape_scenes()[3])
    c.counters[2:8] = 99
    assert c.mark(rows=None, seen=None) == 0 and c.select(rows=None, seen=None, out=None, index=None, cap=0) == 0
    assert c.read()[3].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]


def test_cap_below_the_kept_count():
    scene = cases.frustum_only(cases.random_scene(1000, n_views=3, seed=4))
    total = int(cl.cull_host(scene["rows"], scene["views"], **cases.options(scene))[3][2])
    assert total > 300
    for cap in (0, 1, 255, 256, total - 1, total, total + 5):
        c, (seen, kept, index, counters) = _check(scene, cap=cap)
        written = min(cap, total)
        assert counters.tolist()[2:5] == [total, written, total - written] and len(kept) == written


def test_two_identical_calls_give_identical_bytes():
    scene = cases.random_scene(1000, H=48, W=64, n_views=3, seed=6)
    c = Cull(scene).run()
    first = c.snapshot()
    c.reset()
    c.run()
    second = c.snapshot()
    for k in ("seen", "counters", "obuf", "ibuf"):
        assert first[k].tobytes() == second[k].tobytes(), k


def test_rejected_calls_return_minus_one_and_write_nothing():
    lib = _lib()
    scene = cases.random_scene(257, n_views=1, seed=8)
    c = Cull(scene).run()
    before = c.snapshot()
    nan, inf = float("nan"), float("inf")
    bad_mark = {**pcases.view_faults(c.views[0][1].data_ptr()), "NULL rows": dict(rows=None), "NULL seen": dict(seen=None), "NULL counters": dict(counters=None),
                "H < 0": dict(H=-12), "W = 0": dict(W=0), "2^29 pixels": dict(H=1 << 15, W=1 << 14), "near < 0": dict(near=-0.25), "near NaN": dict(near=nan),
                "far < 0": dict(far=-1.0), "far inf": dict(far=inf), "eps < 0": dict(eps=-0.01), "eps NaN": dict(eps=nan),
                "depth_max NaN": dict(depth_max=nan), "n > 2^30": dict(n=(1 << 30) + 1),
                "misaligned rows": dict(rows=c.rows.data_ptr() + 8), "misaligned seen": dict(seen=c.seen.data_ptr() + 2),
                "misaligned counters": dict(counters=c.counters.data_ptr() + 4), "misaligned depth": dict(depth=c.views[0][0].data_ptr() + 2)}
    for what, over in bad_mark.items():
        assert c.mark(**over) == -1, what
        assert lib.mm3dgs_last_error(), what
    bad_select = {"NULL rows": dict(rows=None), "NULL seen": dict(seen=None), "NULL out_rows": dict(out=None), "NULL work": dict(work=None),
                  "NULL counters": dict(counters=None), "min_views = 0": dict(min_views=0), "n > 2^30": dict(n=(1 << 30) + 1), "cap > 2^31": dict(cap=(1 << 31) + 1),
                  "misaligned rows": dict(rows=c.rows.data_ptr() + 8), "misaligned out_rows": dict(out=c.out + 8), "misaligned work": dict(work=c.work + 4),
                  "misaligned counters": dict(counters=c.counters.data_ptr() + 4), "misaligned seen": dict(seen=c.seen.data_ptr() + 2),
                  "misaligned index": dict(index=c.index + 2)}
    for what, over in bad_select.items():
        assert c.select(**over) == -1, what
        assert lib.mm3dgs_last_error(), what
    torch.cuda.synchronize()
    now = c.snapshot()
    for k, a in before.items():
        assert now[k].tobytes() == a.tobytes(), k
    assert int(lib.mm3dgs_cull_work_bytes((1 << 30) + 1)) == 0


def test_view_fault_texts():
    scene = cases.random_scene(257, n_views=1, seed=8)
    c = Cull(scene)
    for over, text in pcases.view_fault_texts("cull_mark_view", scene["H"], scene["W"], c.views[0][1].data_ptr(), "seen, the depth image and the pose must be 4-byte aligned"):
        assert c.mark(**over) == -1 and _lib().mm3dgs_last_error().decode() == text, over


def test_compare_device_equals_compare_host_with_culling():
    """One small mesh-against-cloud pair, half of each outside the two views: the kept rows byte for byte, the table bit for bit.  The
    host adds the distances in the kernels' order (compare_host's sum_order "kernel"): with numpy's own order the same stored distances gave
    an rms one ulp apart on the MI355X (0.30221648342253143 against the device's 0.3022164834225314, occlusion pair) -- the order of the
    sum, not a distance, a kept row or a count, was what differed."""
    from tests import geometry_cases as gc
    rng = np.random.default_rng(12)
    mesh = gc.random_mesh(40, seed=21)
    v = mesh[0].copy()
    v[:, :3] = (pc.rows_xyz(v) * np.float32(1.5) + np.array([0, 0, 2.5], dtype=np.float32)).view(np.int32)      # in front of the cameras, wider than they see
    cloud = cases.rows_of(np.stack([rng.uniform(-2, 2, 600), rng.uniform(-2, 2, 600), rng.uniform(1.0, 4.0, 600)], 1))
    H, W = 48, 64
    cam = {"fx": 64.0, "fy": 64.0, "cx": 31.5, "cy": 23.5}
    poses = [np.array([1, 0, 0, 0, 0, 0, 0], dtype=np.float32), np.array([0.99, 0.0, 0.12, 0.0, 0.3, 0.0, 0.1], dtype=np.float32)]
    depth = [np.full((H, W), 3.0, dtype=np.float32), cases._depth(H, W, rng)]
    for views in ([(None, p) for p in poses], list(zip(depth, poses))):
        spec = cl.spec(views, H, W, cam, near=0.1, far=5.0, eps=0.05, min_views=1, depth_max=8.0)
        kw = dict(threshold=0.05, max_dist=1.0, density=60.0, seed=3, cull=spec)
        host = geo.compare((v, mesh[1]), cloud, device="cpu", sum_order="kernel", **kw)
        dev = geo.compare((v, mesh[1]), cloud, device=DEV, **kw)
        print(f"CULLERR compare ({spec['mode']}): cull {json.dumps(dev['cull'])}; device table {dev['table'].tolist()}; host table {host['table'].tolist()}")
        assert dev["cull"] == host["cull"] and 0 < dev["cull"]["estimate"]["kept"] < dev["cull"]["estimate"]["rows"]
        assert 0 < dev["cull"]["reference"]["kept"] < 600
        for k in ("estimate_rows", "reference_rows", "estimate_index", "reference_index"):
            assert dev[k].is_cuda and dev[k].cpu().numpy().tobytes() == np.ascontiguousarray(host[k]).view(np.int32).tobytes(), k
        assert dev["n_estimate"] == host["n_estimate"] and dev["n_reference"] == host["n_reference"]
        assert dev["dist_estimate"].cpu().numpy().tobytes() == host["dist_estimate"].tobytes() and dev["dist_reference"].cpu().numpy().tobytes() == host["dist_reference"].tobytes()
        assert dev["table"].tobytes() == host["table"].tobytes()


PARENT_KEYS = ["pose_est", "pose_gt", "keyframes", "ate_rmse", "psnr_list", "ssim_list", "lpips_list"]
MESH = {"voxel": 0.08, "export": False}
GEO = {"density": 2000.0, "threshold": 0.05, "max_dist": 1.0, "eval": True}


def _run(tmp, geometry, frames=4):
    """The small native run of tests/test_gpu_geometry.py::_run (48 x 64, 4 frames, 5 / 6 iterations, kf_every 2)."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device=DEV, height=48, width=64, tracking={"iters": 5}, mapping={"iters": 6, "kf_every": 2, "min_covisibility": 2.0},
                         outputdir=str(tmp), debug={"get_runtime_stats": False, "create_video": False, "save_keyframes": False},
                         eval_every=1, eval_on_device=False, mesh=dict(MESH), geometry=dict(geometry))
    seq = SyntheticSequence(cfg, frames, 2000, seed=5)
    slam = SLAM(cfg, seq)
    from mm3dgs_slam_amd.fused import FusedMapper, FusedTracker
    assert isinstance(slam.tracker, FusedTracker) and isinstance(slam.mapper, FusedMapper)
    slam.run()
    return slam, seq, cfg


def test_native_run_culls_its_evaluation_and_the_checkpoint_reproduces_it(tmp_path):
    import slam_top
    from tests.test_gpu_mesh import _same
    n = 4
    on_dir, off_dir = tmp_path / "on", tmp_path / "off"
    on, seq, cfg_on = _run(on_dir, dict(GEO, cull="occlusion"), n)
    off, _, cfg_off = _run(off_dir, dict(GEO), n)
    a, b = np.load(on_dir / "results.npz", allow_pickle=True), np.load(off_dir / "results.npz", allow_pickle=True)
    assert a["pose_est"].shape == (n, 7) and list(a.keys()) == list(b.keys()) == PARENT_KEYS
    for key in PARENT_KEYS:
        assert _same(a[key], b[key]), key
    assert all(torch.equal(p, q) for p, q in zip(on.estimate_pose_list, off.estimate_pose_list))
    m_on, m_off = json.load(open(on_dir / "geometry" / "metrics.json")), json.load(open(off_dir / "geometry" / "metrics.json"))
    c = m_on["cull"]
    print(f"CULLERR run: cull {json.dumps(c)}; n_estimate {m_on['n_estimate']} (off {m_off['n_estimate']}), n_reference {m_on['n_reference']} (off {m_off['n_reference']}), "
          f"accuracy {m_on['accuracy']} completion {m_on['completion']}")
    assert "cull" not in m_off and c["mode"] == "occlusion" and c["views"] == 2 and c["eps"] == 0.05 and c["min_views"] == 1      # frames 0 and 2 (kf_every 2)
    assert c["estimate"]["rows"] == m_off["n_estimate"] and c["reference"]["rows"] == m_off["n_reference"]
    assert 0 < c["estimate"]["kept"] == m_on["n_estimate"] <= m_off["n_estimate"] and 0 < c["reference"]["kept"] == m_on["n_reference"] <= m_off["n_reference"]
    # every row the device kept is one the host statement keeps, for the views the stage built, and the kept rows are in their original order
    from mm3dgs_slam_amd import export as ex
    r = on.geometry_eval
    spec = ex.cull_views(on, ex.options(on.cfg, "geometry"), ex.options(on.cfg, "mesh"))
    host_spec = dict(spec, views=[(d.cpu().numpy(), p.cpu().numpy()) for d, p in spec["views"]])
    for side in ("estimate", "reference"):
        rows = r[side + "_rows"].cpu().numpy()
        again = cl.apply_host(rows, host_spec)
        assert again[0].tobytes() == rows.tobytes() and again[2]["kept"] == len(rows) == c[side]["kept"], side
        index = r[side + "_index"].cpu().numpy().astype(np.int64)
        assert bool((np.diff(index) > 0).all()) and (len(index) == 0 or index[-1] < c[side]["rows"]), side
    # the checkpoint route, from the files of the run without the key: the same figures
    raw = (on_dir / "geometry" / "metrics.json").read_bytes()
    ck = slam_top.evaluate_geometry_checkpoint(dict(cfg_off, outputdir=str(off_dir), geometry=dict(GEO, eval=False, cull="occlusion")), seq)
    assert ck["iteration"] == n
    assert (off_dir / "geometry" / "metrics.json").read_bytes() == raw
    assert (off_dir / "geometry" / "completion.ply").read_bytes() == (on_dir / "geometry" / "completion.ply").read_bytes()
