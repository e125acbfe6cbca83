"""mm3dgs_mesh_components / mm3dgs_mesh_clean_plan / mm3dgs_mesh_clean_emit (csrc/meshclean.hip) through the raw C ABI against the host
statement of mm3dgs_slam_amd/mesh_clean.py on every case of tests/mesh_clean_cases.py.  The rule is in integers and row bytes are only
moved, so every comparison is exact: label, tri_count, the eight counters, the kept rows, the re-indexed triangles and the index.  Also:
nothing outside the outputs is written (sentinels behind every array, guard zones around the work buffer, inputs unchanged), rejected
calls, caps below the totals, two calls giving the same bytes, clean_device, and the export of a native-loop run with cleaning on and off."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import mesh as ms, mesh_clean as mc
from tests import mesh_clean_cases as cases
from tests.test_gpu_geometry import _dev, _guarded, _guards_ok, _lib, _ptr, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 8                    # elements behind every array that no call may touch
SENT = 0x7A7A7A7A          # every int32 of an untouched output element
CASES = cases.all_cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def references():
    """The host statement of every case once: name -> (label, tri_count, counters, {mode: clean_host(..., full=True)})."""
    out = {}
    for c in CASES:
        out[c["name"]] = mc.components_host(len(c["rows"]), c["triangles"]) + ({m: mc.clean_host(c["rows"], c["triangles"], *m, full=True) for m in c["modes"]},)
    return out


class Cleaner:
    """Caller-owned buffers of one mesh on the device: sentinel-filled outputs with PAD elements behind them, the work buffer between
    guard zones, the inputs with PAD sentinel elements behind them too."""

    def __init__(self, case, vcap=0, tcap=0, fill=0x00):
        self.V, self.T, self.vcap, self.tcap = len(case["rows"]), len(case["triangles"]), vcap, tcap
        full = lambda n, w=None: torch.full((n + PAD,) if w is None else (n + PAD, w), SENT, dtype=torch.int32, device=DEV)
        self.rows, self.tris = full(self.V, 4), full(self.T, 3)
        if self.V:
            self.rows[:self.V] = _dev(case["rows"])
        if self.T:
            self.tris[:self.T] = _dev(case["triangles"])
        self.inputs = (self.rows.cpu(), self.tris.cpu())
        self.label, self.tri_count = full(self.V), full(self.V)
        self.counters = torch.full((8 + PAD,), -7, dtype=torch.int64, device=DEV)
        self.out_rows, self.out_tris, self.index = full(vcap, 4), full(tcap, 3), full(vcap)
        self.nwork = int(_lib().mm3dgs_mesh_clean_work_bytes(self.V, self.T))
        assert self.nwork > 0 and self.nwork % 8 == 0
        self.buf, self.work = _guarded(self.nwork, fill)

    def components(self, **over):
        a = dict(V=self.V, T=self.T, tris=self.tris, label=self.label, tri_count=self.tri_count, counters=self.counters)
        a.update(over)
        rc = _lib().mm3dgs_mesh_components(a["V"], a["T"], _ptr(a["tris"]), _ptr(a["label"]), _ptr(a["tri_count"]), _ptr(a["counters"]), _stream())
        torch.cuda.synchronize()
        return rc

    def plan(self, mode, min_triangles, **over):
        a = dict(V=self.V, T=self.T, tris=self.tris, label=self.label, tri_count=self.tri_count, mode=mc.MODE_IDS.get(mode, mode), min_triangles=min_triangles,
                 work=self.work, counters=self.counters)
        a.update(over)
        rc = _lib().mm3dgs_mesh_clean_plan(a["V"], a["T"], _ptr(a["tris"]), _ptr(a["label"]), _ptr(a["tri_count"]), a["mode"], a["min_triangles"], _ptr(a["work"]),
                                           _ptr(a["counters"]), _stream())
        torch.cuda.synchronize()
        return rc

    def emit(self, **over):
        a = dict(V=self.V, T=self.T, rows=self.rows, tris=self.tris, work=self.work, out_rows=self.out_rows, vcap=self.vcap, out_tris=self.out_tris, tcap=self.tcap,
                 index=self.index, counters=self.counters)
        a.update(over)
        rc = _lib().mm3dgs_mesh_clean_emit(a["V"], a["T"], _ptr(a["rows"]), _ptr(a["tris"]), _ptr(a["work"]), _ptr(a["out_rows"]), a["vcap"], _ptr(a["out_tris"]),
                                           a["tcap"], _ptr(a["index"]), _ptr(a["counters"]), _stream())
        torch.cuda.synchronize()
        return rc

    def state(self):
        return {k: getattr(self, k).cpu() for k in ("rows", "tris", "label", "tri_count", "counters", "out_rows", "out_tris", "index", "buf")}

    def read(self):
        """dict of the host copies after checking the guards, the elements behind every array and the inputs."""
        s = {k: v.numpy() for k, v in self.state().items()}
        assert _guards_ok(self.buf), "a guard zone of the work buffer was written"
        assert torch.equal(self.rows.cpu(), self.inputs[0]) and torch.equal(self.tris.cpu(), self.inputs[1]), "an input was written"
        assert bool((s["label"][self.V:] == SENT).all()) and bool((s["tri_count"][self.V:] == SENT).all()), "elements behind label / tri_count were written"
        assert bool((s["counters"][8:] == -7).all()), "elements behind the counters were written"
        assert bool((s["out_rows"][self.vcap:] == SENT).all()) and bool((s["out_tris"][self.tcap:] == SENT).all()) and bool((s["index"][self.vcap:] == SENT).all()), \
            "elements behind a cap were written"
        return s


def _check_components(cl, want, words=8):
    """label, tri_count and the first `words` counters against the host statement (4: after a plan, which owns the other four)."""
    label, tri_count, counters = want
    s = cl.read()
    assert s["label"][:cl.V].view(np.uint32).tobytes() == label.tobytes(), "label"
    assert s["tri_count"][:cl.V].view(np.uint32).tobytes() == tri_count.tobytes(), "tri_count"
    assert s["counters"][:words].tolist() == counters.tolist()[:words], "counters"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_case_against_the_host_statement(references, case):
    want = references[case["name"]]
    probe = Cleaner(case)
    assert probe.components() == 0
    _check_components(probe, want[:3])
    for k, mode in enumerate(case["modes"]):
        rows, tris, index, info, counters = want[3][mode][:5]
        cl = Cleaner(case, len(rows), len(tris), fill=0xFF if k % 2 else 0x00)      # the work buffer's contents are irrelevant before the plan
        assert cl.components() == 0 and cl.plan(*mode) == 0
        assert cl.counters[:8].cpu().tolist() == counters.tolist()[:7] + [0], mode
        assert cl.emit() == 0
        s = cl.read()
        print(f"CLEANERR {case['name']} {mode}: V {cl.V}, T {cl.T}, counters {s['counters'][:8].tolist()}, info {info}")
        assert s["counters"][:8].tolist() == counters.tolist(), mode
        assert s["out_rows"][:cl.vcap].tobytes() == rows.tobytes(), mode
        assert s["out_tris"][:cl.tcap].tobytes() == tris.tobytes(), mode
        assert s["index"][:cl.vcap].view(np.uint32).tobytes() == index.tobytes(), mode
        assert mc.info_of(cl.V, cl.T, s["counters"][:8]) == info
        _check_components(cl, want[:3], words=4)      # the plan and emit read label, tri_count and counters [0..3], they do not write them
    # index is optional
    mode = case["modes"][0]
    rows, tris = want[3][mode][:2]
    cl = Cleaner(case, len(rows), len(tris))
    assert cl.components() == 0 and cl.plan(*mode) == 0 and cl.emit(index=None) == 0
    s = cl.read()
    assert s["out_rows"][:cl.vcap].tobytes() == rows.tobytes() and s["out_tris"][:cl.tcap].tobytes() == tris.tobytes() and bool((s["index"] == SENT).all())


def test_two_calls_give_the_same_bytes(references):
    case = CASES[IDS.index("ribbon shuffled shuffled triangles")]
    mode = ("largest", 1)
    rows, tris = references[case["name"]][3][mode][:2]
    outs = []
    for _ in range(2):
        cl = Cleaner(case, len(rows), len(tris))
        assert cl.components() == 0 and cl.plan(*mode) == 0 and cl.emit() == 0
        s = cl.read()
        outs.append(tuple(s[k].tobytes() for k in ("label", "tri_count", "counters", "out_rows", "out_tris", "index")))
    assert outs[0] == outs[1]
    assert outs[0][3] == np.concatenate([rows, np.full((PAD, 4), SENT, dtype=np.int32)]).tobytes()      # and they are the host statement's


def test_caps_below_the_kept_counts(references):
    case = CASES[IDS.index("T = 257")]
    mode = ("small", 4)
    rows, tris, index, _, counters = references[case["name"]][3][mode][:5]
    nv, nt = len(rows), len(tris)
    assert nv > 20 and nt > 20
    for vcap, tcap in ((nv - 5, nt), (nv, nt // 2), (nv // 3, nt // 2), (0, 0), (nv + 3, nt + 3)):
        cl = Cleaner(case, vcap, tcap)
        assert cl.components() == 0 and cl.plan(*mode) == 0 and cl.emit() == 0
        s = cl.read()      # (checks that nothing behind the caps was written)
        wv, wt = min(nv, vcap), min(nt, tcap)
        print(f"CLEANERR caps vcap {vcap} of {nv}, tcap {tcap} of {nt}: counters {s['counters'][:8].tolist()}")
        assert s["counters"][:8].tolist() == counters.tolist()[:7] + [((nt - wt) << 32) | (nv - wv)]
        assert s["out_rows"][:wv].tobytes() == rows[:wv].tobytes() and s["out_tris"][:wt].tobytes() == tris[:wt].tobytes()
        assert s["index"][:wv].view(np.uint32).tobytes() == index[:wv].tobytes()
        assert bool((s["out_rows"][wv:] == SENT).all()) and bool((s["out_tris"][wt:] == SENT).all()) and bool((s["index"][wv:] == SENT).all())
        want = mc.clean_host(case["rows"], case["triangles"], *mode, vcap=vcap, tcap=tcap, full=True)
        assert want[4].tolist() == s["counters"][:8].tolist() and want[0].tobytes() == s["out_rows"][:wv].tobytes()
    # NULL outputs are fine with caps of 0
    cl = Cleaner(case, 0, 0)
    assert cl.components() == 0 and cl.plan(*mode) == 0 and cl.emit(out_rows=None, out_tris=None, index=None) == 0
    assert cl.counters[:8].cpu().tolist() == counters.tolist()[:7] + [(nt << 32) | nv]


def test_rejected_calls_return_minus_one_and_write_nothing():
    case = CASES[IDS.index("T = 257")]
    cl = Cleaner(case, 64, 64)
    before = cl.state()
    lib = _lib()
    big = (1 << 30) + 1
    bad_components = {"V above 2^30": dict(V=big), "T above 2^30": dict(T=big), "NULL triangles": dict(tris=None), "NULL label": dict(label=None),
                      "NULL tri_count": dict(tri_count=None), "NULL counters": dict(counters=None), "misaligned triangles": dict(tris=cl.tris.data_ptr() + 2),
                      "misaligned label": dict(label=cl.label.data_ptr() + 1), "misaligned tri_count": dict(tri_count=cl.tri_count.data_ptr() + 2),
                      "misaligned counters": dict(counters=cl.counters.data_ptr() + 4)}
    for what, over in bad_components.items():
        assert cl.components(**over) == -1, what
        assert lib.mm3dgs_last_error(), what
    bad_plan = {"V above 2^30": dict(V=big), "T above 2^30": dict(T=big), "NULL triangles": dict(tris=None), "NULL label": dict(label=None), "NULL tri_count": dict(tri_count=None), "NULL work": dict(work=None),
                "NULL counters": dict(counters=None), "misaligned triangles": dict(tris=cl.tris.data_ptr() + 2), "misaligned label": dict(label=cl.label.data_ptr() + 2),
                "misaligned tri_count": dict(tri_count=cl.tri_count.data_ptr() + 1), "misaligned work": dict(work=cl.work + 4),
                "misaligned counters": dict(counters=cl.counters.data_ptr() + 4)}
    for what, over in bad_plan.items():
        assert cl.plan("small", 4, **over) == -1, what
        assert lib.mm3dgs_last_error(), what
    assert cl.plan("small", 0) == -1 and b"min_triangles" in lib.mm3dgs_last_error()
    for mode in (0, 3, -1):
        assert cl.plan(mode, 4) == -1 and b"mode" in lib.mm3dgs_last_error(), mode
    bad_emit = {"V above 2^30": dict(V=big), "T above 2^30": dict(T=big), "vcap above 2^31": dict(vcap=(1 << 31) + 1), "tcap above 2^31": dict(tcap=(1 << 31) + 1),
                "NULL rows": dict(rows=None), "NULL triangles": dict(tris=None), "NULL work": dict(work=None), "NULL out_rows": dict(out_rows=None),
                "NULL out_triangles": dict(out_tris=None), "NULL counters": dict(counters=None), "misaligned rows": dict(rows=cl.rows.data_ptr() + 8),
                "misaligned out_rows": dict(out_rows=cl.out_rows.data_ptr() + 4), "misaligned triangles": dict(tris=cl.tris.data_ptr() + 2),
                "misaligned out_triangles": dict(out_tris=cl.out_tris.data_ptr() + 2), "misaligned index": dict(index=cl.index.data_ptr() + 2),
                "misaligned work": dict(work=cl.work + 4), "misaligned counters": dict(counters=cl.counters.data_ptr() + 4)}
    for what, over in bad_emit.items():
        assert cl.emit(**over) == -1, what
        assert lib.mm3dgs_last_error(), what
    now = cl.state()
    for name, t in before.items():
        assert torch.equal(now[name], t), name
    for V, T in ((big, 3), (3, big)):
        assert int(lib.mm3dgs_mesh_clean_work_bytes(V, T)) == 0
    # min_triangles is not looked at in mode largest, and the same buffers serve a good call
    assert cl.components() == 0 and cl.plan("largest", 0) == 0 and cl.emit() == 0
    cl.read()


def test_clean_device_against_clean_host(references):
    case = CASES[IDS.index("marching tetrahedra: sphere and two blobs")]
    for mode in case["modes"]:
        rows, tris, index, info = references[case["name"]][3][mode][:4]
        got = mc.clean(_dev(case["rows"]), _dev(case["triangles"]), *mode, device=DEV)
        assert got[0].device.type == "cuda" and got[0].dtype == got[1].dtype == got[2].dtype == torch.int32
        assert got[0].cpu().numpy().tobytes() == rows.tobytes() and got[1].cpu().numpy().tobytes() == tris.tobytes()
        assert got[2].cpu().numpy().view(np.uint32).tobytes() == index.tobytes() and got[3] == info, mode
    # numpy in, and the empty mesh
    got = mc.clean_device(case["rows"], case["triangles"], "largest", 1, device=DEV)
    assert ms.mesh_topology(len(got[0]), got[1].cpu().numpy())["closed"]
    got = mc.clean_device(np.zeros((0, 4), dtype=np.int32), np.zeros((0, 3), dtype=np.int32), "small", 1, device=DEV)
    assert got[0].shape == (0, 4) and got[1].shape == (0, 3) and got[2].shape == (0,) and got[3] == dict.fromkeys(mc.INFO_NAMES, 0)


PARENT_KEYS = ["pose_est", "pose_gt", "keyframes", "ate_rmse", "psnr_list", "ssim_list", "lpips_list"]
MESH = {"voxel": 0.08}


def _run(tmp, mesh, frames=4):
    """The small native run of tests/test_gpu_mesh.py::_run (48 x 64, 4 frames), with the mesh block."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device=DEV, height=48, width=64, tracking={"iters": 5}, mapping={"iters": 6, "kf_every": 2, "min_covisibility": 2.0},
                         outputdir=str(tmp), debug={"get_runtime_stats": False, "create_video": False, "save_keyframes": False},
                         eval_every=1, eval_on_device=False, mesh=dict(MESH, **mesh))
    seq = SyntheticSequence(cfg, frames, 2000, seed=5)
    slam = SLAM(cfg, seq)
    from mm3dgs_slam_amd.fused import FusedMapper, FusedTracker
    assert isinstance(slam.tracker, FusedTracker) and isinstance(slam.mapper, FusedMapper)
    slam.run()
    return slam, seq, cfg


def test_native_run_exports_its_mesh_cleaned_and_changes_nothing_else(tmp_path):
    from tests.test_gpu_mesh import _same
    n = 4
    on_dir, off_dir = tmp_path / "on", tmp_path / "off"
    on, _, _ = _run(on_dir, dict(export=True, clean="small", clean_min_triangles=30), n)
    off, _, _ = _run(off_dir, dict(export=True), n)
    a = np.load(on_dir / "results.npz", allow_pickle=True)
    b = np.load(off_dir / "results.npz", allow_pickle=True)
    assert a["pose_est"].shape == (n, 7) and list(a.keys()) == list(b.keys()) == PARENT_KEYS
    for key in PARENT_KEYS:
        assert _same(a[key], b[key]), key
    assert all(torch.equal(p, q) for p, q in zip(on.estimate_pose_list, off.estimate_pose_list))
    rows, tris = ms.read_mesh_ply(off.mesh_export["mesh"])
    crows, ctris = ms.read_mesh_ply(on.mesh_export["mesh"])
    want = mc.clean_host(rows, tris, "small", 30)
    info = on.mesh_export["clean"]
    print(f"CLEANERR run: {len(rows)} vertices, {len(tris)} triangles; cleaned {info}")
    assert "clean" not in off.mesh_export and "clean" not in off.mesh_export["counters"]
    assert crows.tobytes() == want[0].tobytes() and ctris.tobytes() == want[1].tobytes()
    assert info == dict(want[3], mode="small", min_triangles=30, vertices=len(crows), triangles=len(ctris))
    assert {k: v for k, v in on.mesh_export["counters"].items() if k != "clean"} == off.mesh_export["counters"]
    assert ms.mesh_topology(len(crows), ctris)["unreferenced"] == 0
