"""mm3dgs_mesh_depth_render / mm3dgs_depth_compare (csrc/meshdepth.hip) through the raw C ABI against the float64 host statement
mesh_depth.render_host / compare_rows_host, bit for bit: the depth image's bytes, the winning triangles and the counters [0..4], [6] (the
host statement fills [4] from the same rectangle rule) -- every operation of the rule is a double product, sum, quotient or comparison in
one stated order, without contraction on either side, so no value can differ --, at the sizes where a count / scan / scatter and a tile's
batched list can break, with guard zones around both images and the work buffer and sentinels behind the counters; a capacity below the
need; rejected calls; the Python surface; and a native run that scores its depth L1 and culls against the rendered reference.  Every test
prints its figures (`MDERR ...`, pytest -s) before it asserts."""
import json

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import cull as cl, export as ex, mesh_depth as md
from tests import mesh_depth_cases as cases, pointcloud_cases as pcases
from tests.test_gpu_geometry import _dev, _guarded, _guards_ok, _lib, _ptr, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 8                    # elements behind the counters that no call may touch
G = 4096                   # the guard zones of tests/test_gpu_geometry.py, in bytes
HELD = [0, 1, 2, 3, 4, 6]


class Render:
    """Caller-owned buffers of one view: both images and the work buffer between guard zones, sentinels behind the counters."""

    def __init__(self, scene, max_pairs=None, fill=0x00):
        self.s = scene
        self.V, self.T, self.H, self.W = len(scene["rows"]), len(scene["tris"]), scene["H"], scene["W"]
        self.rows = _dev(scene["rows"]) if self.V else None
        self.tris = _dev(scene["tris"]) if self.T else None
        self.pose = _dev(scene["pose"])
        self.max_pairs = 1 << 16 if max_pairs is None else max_pairs
        self.nwork = int(_lib().mm3dgs_mesh_depth_work_bytes(self.V, self.T, self.H, self.W, self.max_pairs))
        assert self.nwork > 0 and self.nwork % 8 == 0
        self.dbuf, self.depth = _guarded(4 * self.H * self.W, 0x7A)
        self.tbuf, self.tri = _guarded(4 * self.H * self.W, 0x7A)
        self.wbuf, self.work = _guarded(self.nwork, fill)
        self.counters = torch.full((8 + PAD,), -7, dtype=torch.int64, device=DEV)
        self.counters[:8] = 0

    def call(self, **over):
        s = self.s
        a = dict(H=self.H, W=self.W, fx=s["fx"], fy=s["fy"], cx=s["cx"], cy=s["cy"], pose=self.pose, near=s["near"], far=s["far"], V=self.V, rows=self.rows, T=self.T,
                 tris=self.tris, max_pairs=self.max_pairs, depth=self.depth, tri=self.tri, work=self.work, counters=self.counters)
        a.update(over)
        rc = _lib().mm3dgs_mesh_depth_render(a["H"], a["W"], a["fx"], a["fy"], a["cx"], a["cy"], _ptr(a["pose"]), a["near"], a["far"], a["V"], _ptr(a["rows"]), a["T"],
                                             _ptr(a["tris"]), a["max_pairs"], _ptr(a["depth"]), _ptr(a["tri"]), _ptr(a["work"]), _ptr(a["counters"]), _stream())
        torch.cuda.synchronize()
        return rc

    def snapshot(self):
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("counters", "dbuf", "tbuf", "wbuf")}

    def read(self):
        """(depth float32 [H,W], tri int32 [H,W], counters int64 [8]) after the guards and sentinels were checked."""
        s = self.snapshot()
        assert _guards_ok(self.dbuf) and _guards_ok(self.tbuf) and _guards_ok(self.wbuf), "a guard zone was written"
        assert bool((s["counters"][8:] == -7).all()) and s["counters"][7] == 0, "elements behind the counters, or counters[7], were written"
        img = lambda b, t: b[G:len(b) - G].view(t).reshape(self.H, self.W).copy()
        return img(s["dbuf"], np.float32), img(s["tbuf"], np.int32), s["counters"][:8].copy()


def _host(scene, **kw):
    return md.render_host(scene["rows"], scene["tris"], **dict(cases.args(scene), **kw))


def _check(scene, fill=0x00, max_pairs=None):
    hd, ht, hc = _host(scene)
    r = Render(scene, max_pairs, fill)
    assert r.call() == 0, _lib().mm3dgs_last_error()
    d, t, c = r.read()
    print(f"MDERR device {scene['name']} (fill {fill:#04x}): counters {c.tolist()}, host {hc.tolist()}; {int((d.view(np.int32) != hd.view(np.int32)).sum())} depths and "
          f"{int((t != ht).sum())} winners of {d.size} differ")
    assert c[HELD].tolist() == hc[HELD].tolist() and c[5] == 0
    assert d.tobytes() == hd.tobytes() and np.array_equal(t, ht)
    return r, (d, t, c)


SIZES = [cases.random_scene(3, seed=4, H=1, W=1, cx=0.0, cy=0.0, fx=2.0, fy=2.0), cases.random_scene(257, seed=3, H=17, W=33, cx=16.0, cy=8.0),
         cases.random_scene(1, seed=1), cases.random_scene(60, seed=2), cases.random_scene(513, seed=5), cases.random_scene(256, seed=6, crossing=False)]


@pytest.mark.parametrize("scene", SIZES, ids=lambda s: s["name"])
def test_sizes_against_the_host_statement(scene):
    _, (d, t, c) = _check(scene, fill=0xFF if len(scene["tris"]) % 2 else 0x00)
    if len(scene["tris"]) >= 60:
        assert c[6] > 100 and c[1] > 10


def test_second_round_of_the_scan():
    """16 x 17600 is 1100 tiles: the tiles from 1024 on are offset by the scan's carry."""
    scene = cases.random_scene(48, seed=7, **cases.WIDE)
    _, (d, t, c) = _check(scene, fill=0xFF)
    assert int((t[:, 16384:] >= 0).sum()) > 50 and int((t[:, :16384] >= 0).sum()) > 50
    _, (d, t, c) = _check(cases.whole_image(**cases.WIDE))
    assert c[4] == 1100 and c[6] == 16 * 17600


def test_empty_meshes_still_write_the_image_and_count_the_view():
    for scene in (cases.random_scene(0, 0), cases.random_scene(5, 0), cases.random_scene(0, 7)):
        _, (d, t, c) = _check(scene, fill=0xFF)
        assert bool((d.view(np.int32) == 0).all()) and bool((t == -1).all())
        assert c.tolist() == [1, 0, len(scene["tris"]), 0, 0, 0, 0, 0]


@pytest.mark.parametrize("at", (299, 0, 150))
def test_a_list_longer_than_one_batch(at):
    _, (d, t, c) = _check(cases.stacked(at))
    assert bool((t[17:31, 17:31] == at).all()) and bool((d[17:31, 17:31] == np.float32(1.5)).all())


def test_analytic_scenes():
    _, (d, t, c) = _check(cases.whole_image())
    assert c[4] == 12 and c[6] == 48 * 64 and bool((d == np.float32(2.0)).all())
    _, (d, t, c) = _check(cases.floor(), fill=0xFF)
    assert c[6] == 1280 and bool((t[28:] >= 0).all()) and bool((t[:28] == -1).all())
    s = cases.plane_grid()
    _, (d, t, c) = _check(s)
    u0, u1, v0, v1 = s["outline"]
    assert bool((t[v0:v1 + 1, u0:u1 + 1] >= 0).all()) and c[6] == (u1 - u0 + 1) * (v1 - v0 + 1)
    s, want, hitters = cases.classification()
    _, (d, t, c) = _check(s)
    assert c.tolist()[:4] == [1, want.count(0), want.count(1), want.count(2)] and np.unique(t[t >= 0]).tolist() == hitters
    for s, drawn, behind, hits in cases.bound_scenes():
        _, (d, t, c) = _check(s)
        assert c.tolist()[:4] == [1, drawn, 0, behind] and (c[6] > 50) == hits, s["name"]
    for s in cases.tie_scenes():
        _, (d, t, c) = _check(s)
        assert set(np.unique(t).tolist()) == {-1, 0, 1}


def test_tri_out_null_and_accumulating_counters():
    scene = cases.random_scene(60, seed=2)
    hd, ht, hc = _host(scene)
    r = Render(scene)
    assert r.call(tri=None) == 0 and r.call(tri=None) == 0
    s = r.snapshot()
    d, _, c = r.read()
    assert d.tobytes() == hd.tobytes() and bool((s["tbuf"][G:-G] == 0x7A).all())
    assert c[HELD].tolist() == (2 * hc[HELD]).tolist()


def test_two_identical_calls_give_identical_bytes():
    scene = cases.random_scene(513, seed=5)
    runs = []
    for _ in range(2):
        r = Render(scene, fill=0xFF)
        assert r.call() == 0
        runs.append(r.snapshot())
    for k in ("counters", "dbuf", "tbuf"):
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k


def test_capacity_below_and_at_the_need():
    scene = cases.stacked(150)
    need = int(_host(scene)[2][4])
    assert need > 600
    for max_pairs in (need - 5, 300, 1, 0):
        r = Render(scene, max_pairs, fill=0xFF)
        assert r.call() == 0
        d, t, c = r.read()      # (the guards are checked; the image of a call that dropped pairs is void)
        print(f"MDERR capacity {max_pairs} of {need}: counters {c.tolist()}")
        assert c[5] == need - max_pairs and c[4] == max_pairs
    _check(scene, max_pairs=need)


def test_rejected_calls_return_non_zero_and_write_nothing():
    lib = _lib()
    scene = cases.random_scene(60, seed=2)
    r = Render(scene)
    assert r.call() == 0
    before = r.snapshot()
    nan, inf = float("nan"), float("inf")
    bad = {**pcases.view_faults(r.pose.data_ptr()), "NULL rows": dict(rows=None), "NULL triangles": dict(tris=None), "NULL depth": dict(depth=None), "NULL work": dict(work=None),
           "NULL counters": dict(counters=None), "2^29 pixels": dict(H=1 << 15, W=1 << 14),
           "fy NaN": dict(fy=nan), "cx inf": dict(cx=inf), "cy NaN": dict(cy=nan), "near < 0": dict(near=-0.5), "near NaN": dict(near=nan), "far < 0": dict(far=-1.0),
           "far inf": dict(far=inf), "V > 2^30": dict(V=(1 << 30) + 1), "T > 2^30": dict(T=(1 << 30) + 1), "max_pairs > 2^31": dict(max_pairs=(1 << 31) + 1),
           "misaligned rows": dict(rows=r.rows.data_ptr() + 8), "misaligned triangles": dict(tris=r.tris.data_ptr() + 2),
           "misaligned depth": dict(depth=r.depth + 2), "misaligned tri": dict(tri=r.tri + 1), "misaligned work": dict(work=r.work + 4),
           "misaligned counters": dict(counters=r.counters.data_ptr() + 4)}
    for what, over in bad.items():
        assert r.call(**over) != 0, what
        assert lib.mm3dgs_last_error(), what
    a = torch.ones(4, 4, device=DEV)
    row = torch.zeros(8, dtype=torch.float64, device=DEV)
    work = torch.zeros(64, dtype=torch.float64, device=DEV)
    for what, args in {"NULL a": (4, 4, None, a, work, row), "NULL b": (4, 4, a, None, work, row), "NULL work": (4, 4, a, a, None, row), "NULL row": (4, 4, a, a, work, None),
                       "H = 0": (0, 4, a, a, work, row), "too many pixels": (1 << 15, 1 << 14, a, a, work, row), "misaligned a": (4, 3, a.data_ptr() + 2, a, work, row),
                       "misaligned row": (4, 4, a, a, work, row.data_ptr() + 4)}.items():
        assert lib.mm3dgs_depth_compare(args[0], args[1], _ptr(args[2]), _ptr(args[3]), _ptr(args[4]), _ptr(args[5]), _stream()) != 0, what
        assert lib.mm3dgs_last_error(), what
    torch.cuda.synchronize()
    now = r.snapshot()
    for k, v in before.items():
        assert now[k].tobytes() == v.tobytes(), k
    assert bool((row == 0).all())
    assert int(lib.mm3dgs_mesh_depth_work_bytes((1 << 30) + 1, 1, 4, 4, 1)) == 0 and int(lib.mm3dgs_mesh_depth_work_bytes(1, (1 << 30) + 1, 4, 4, 1)) == 0
    assert int(lib.mm3dgs_mesh_depth_work_bytes(1, 1, 0, 4, 1)) == 0 and int(lib.mm3dgs_mesh_depth_work_bytes(1, 1, 1 << 15, 1 << 14, 1)) == 0
    assert int(lib.mm3dgs_mesh_depth_work_bytes(1, 1, 4, 4, (1 << 31) + 1)) == 0 and int(lib.mm3dgs_depth_compare_work_bytes(0, 4)) == 0


def test_view_fault_texts():
    r = Render(cases.random_scene(60, seed=2))
    for over, text in pcases.view_fault_texts("mesh_depth_render", r.H, r.W, r.pose.data_ptr(), "triangles, depth_out, tri_out and the pose must be 4-byte aligned"):
        assert r.call(**over) == -1 and _lib().mm3dgs_last_error().decode() == text, over


@pytest.mark.parametrize("hw", ((1, 1), (17, 33), (48, 64), (480, 640)))
def test_depth_compare_equals_the_host_row_in_kernel_order(hw):
    lib = _lib()
    H, W = hw
    pairs = [cases.depth_pair(H, W, seed=H + k) for k in range(3)]
    if H == 1:      # one pixel: one combination per pair
        pairs = [(np.float32([[x]]), np.float32([[y]])) for x, y in ((1.5, 2.0), (np.nan, 2.0), (1.5, 0.0), (-1.0, np.inf))]
    n = len(pairs)
    table = torch.full((n + 2, 8), -3.0, dtype=torch.float64, device=DEV)      # a row before and a row behind that stay untouched
    nwork = int(lib.mm3dgs_depth_compare_work_bytes(H, W))
    assert nwork == 64 * ((H * W + 255) // 256)
    wbuf, work = _guarded(nwork, 0xFF)
    for k, (a, b) in enumerate(pairs):
        assert lib.mm3dgs_depth_compare(H, W, _ptr(_dev(a)), _ptr(_dev(b)), _ptr(work), _ptr(table[k + 1]), _stream()) == 0
        torch.cuda.synchronize()
    got = table.cpu().numpy()
    want = np.stack([md.compare_rows_host(a, b, "kernel")[0] for a, b in pairs])
    print(f"MDERR compare {hw}: device {got[1:-1].tolist()}; host {want.tolist()}")
    assert _guards_ok(wbuf) and bool((got[0] == -3.0).all()) and bool((got[-1] == -3.0).all())
    assert got[1:-1].tobytes() == want.tobytes()
    if H > 1:
        assert bool((want[:, [0, 4, 5, 6]] > 0).all())


def test_python_surface_against_the_host_path():
    s = cases.random_scene(200, seed=9)
    moved = s["rows"].copy()
    moved[:, :3] = (moved[:, :3].view(np.float32) + np.float32(0.03)).view(np.int32)
    poses = [s["pose"], np.array([0.99, 0.0, 0.1, 0.05, -0.2, 0.1, 0.3], dtype=np.float32), np.array([1, 0, 0, 0, 0, 0, -60.0], dtype=np.float32)]
    cam = {k: s[k] for k in ("fx", "fy", "cx", "cy")}
    kw = dict(H=s["H"], W=s["W"], cam=cam, near=s["near"], far=s["far"])
    ht, hs = md.depth_l1((moved, s["tris"]), (s["rows"], s["tris"]), poses, device="cpu", sum_order="kernel", **kw)
    dt, ds = md.depth_l1((moved, s["tris"]), (s["rows"], s["tris"]), poses, device=DEV, **kw)
    print(f"MDERR depth_l1: device {json.dumps(ds)}; host {json.dumps(hs)}")
    assert dt.tobytes() == ht.tobytes() and ds == hs and ds["views"] == 3 and ds["empty_views"] == 1 and ht[0, 0] > 100
    m = md.MeshDepth(s["rows"], s["tris"], s["H"], s["W"], near=s["near"], far=s["far"], device=DEV, **cam)
    for pose in poses:
        d, t = m.render(pose)
        hd, htri, _ = _host(dict(s, pose=pose))
        assert d.is_cuda and d.cpu().numpy().tobytes() == hd.tobytes() and np.array_equal(t.cpu().numpy(), htri)
    assert m.finish()[0] == 3
    small = md.MeshDepth(s["rows"], s["tris"], s["H"], s["W"], near=s["near"], far=s["far"], max_pairs=10, device=DEV, **cam)
    small.render(poses[0])
    with pytest.raises(RuntimeError, match=r"geometry\.depth_max_pairs"):
        small.finish()
    with pytest.raises(ValueError):
        md.MeshDepth(s["rows"], s["tris"], s["H"], s["W"], max_pairs=(1 << 31) + 1, device=DEV, **cam)


def test_native_run_scores_its_depth_l1_and_culls_against_the_rendered_reference(tmp_path):
    from tests.test_gpu_cull import GEO, PARENT_KEYS, _run
    from tests.test_gpu_mesh import _same
    n = 4
    on, seq, _ = _run(tmp_path / "on", dict(GEO, depth_l1=True), n)
    off, _, _ = _run(tmp_path / "off", dict(GEO), n)
    a, b = np.load(tmp_path / "on" / "results.npz", allow_pickle=True), np.load(tmp_path / "off" / "results.npz", allow_pickle=True)
    assert list(a.keys()) == list(b.keys()) == PARENT_KEYS
    for key in PARENT_KEYS:
        assert _same(a[key], b[key]), key
    assert all(torch.equal(p, q) for p, q in zip(on.estimate_pose_list, off.estimate_pose_list))
    m_on, m_off = json.load(open(tmp_path / "on" / "geometry" / "metrics.json")), json.load(open(tmp_path / "off" / "geometry" / "metrics.json"))
    d = m_on.pop("depth_l1")
    z = np.load(tmp_path / "on" / "geometry" / "depth_l1.npz")
    print(f"MDERR run: depth_l1 {json.dumps(d)}; table {z['table'].tolist()}")
    assert "depth_l1" not in m_off and m_on == m_off
    assert d["views"] == 2 and z["frames"].tolist() == [0, 2] and z["table"].shape == (2, 8)      # frames 0 and 2 (kf_every 2)
    assert d["counters"]["estimate"]["dropped"] == 0 and d["counters"]["reference"]["views"] == 2 and d["empty_views"] == 0 and 0 < d["mean"] < 1
    # the table is the host statement's for the meshes and views the stage uses, sums in kernel order
    block, gt = ex.options(on.cfg, "mesh"), ex.gt_poses(on)
    est, ref = ex.mesh_geometry(on, block)[:2], ex.mesh_geometry(on, dict(block, source="sensor"), gt)[:2]
    cam, H, W = on.cfg["cam"], 48, 64
    host = md.depth_l1(est, ref, [gt[0], gt[2]], H, W, cam, device="cpu", sum_order="kernel")[0]
    assert host.tobytes() == z["table"].tobytes()
    # cull: occlusion against the rendered reference keeps what cull_host keeps when fed the host-rendered depths
    sampled = on.geometry_eval      # (no culling: the sampled rows of both sides)
    on.cfg["geometry"] = dict(GEO, eval=False, cull="occlusion", cull_depth="reference")
    culled = on.evaluate_geometry(path=str(tmp_path / "culled"))
    views = [(md.render_host(ref[0], ref[1], gt[i], H, W, cam["fx"], cam["fy"], cam["cx"], cam["cy"])[0], gt[i].cpu().numpy()) for i in (0, 2)]
    spec = cl.spec(views, H, W, cam, eps=GEO["threshold"], depth_max=float(block["max_depth"]))
    for side in ("estimate", "reference"):
        kept, _, counts = cl.apply_host(sampled[side + "_rows"].cpu().numpy(), spec)
        print(f"MDERR run cull {side}: device {json.dumps(culled['cull'][side])}; host {json.dumps(counts)}")
        assert culled["cull"][side] == counts and 0 < counts["kept"] and culled[side + "_rows"].cpu().numpy().tobytes() == kept.tobytes()
