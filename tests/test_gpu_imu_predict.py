"""mm3dgs_propagate_imu (ABI 213) and tracking.imu_on_device on the GPU: the one-lane double-precision kernel against the reference's own
output and against its float64 host restatement (pose_utils.propagate_imu_np), its argument checks, the tracker's device path (no pose
read-back) and a UTMM-shaped SLAM run that starts every frame from it."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import _lib, pose_utils
from tests import imu_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(__file__), "golden")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _kernel(p1, p2, imu6, c2i, dt_cam, dt_imu):
    from mm3dgs_slam_amd.tracker import propagate_imu_device
    return propagate_imu_device(_dev(p1), _dev(p2), _dev(imu6).reshape(-1, 6), _dev(c2i), dt_cam, dt_imu).cpu().numpy()


def _held_to_host(p1, p2, imu6, c2i, dt_cam, dt_imu, what):
    """The kernel against propagate_imu_np on the float32 values the kernel is handed, at the bar of the constant-velocity kernel's test
    (test_gpu_fused.py::test_pose_prediction_kernel_matches_the_golden_pose_algebra): 2.4e-7 * max(1, |host|), ~2 float32 ulp -- both
    sides evaluate one algebra in double and round once."""
    p1, p2, imu6, c2i = (imu_cases.f32(a) for a in (p1, p2, imu6, c2i))
    host = pose_utils.propagate_imu_np(p1, p2, imu6.reshape(-1, 6), c2i, dt_cam, dt_imu).astype(np.float32)
    dev = _kernel(p1, p2, imu6, c2i, dt_cam, dt_imu)
    err, bar = float(np.abs(host - dev).max()), 2.4e-7 * max(1.0, float(np.abs(host).max()))
    print(f"{what}: |kernel - host| = {err:.3e} (bar {bar:.3e})")
    assert err <= bar, (what, err, bar, host, dev)
    return dev


def test_imu_prediction_kernel_reproduces_the_reference_output():
    """tests/golden/g2_imu.npz["out"]: the reference's propagate_imu on 8 samples with the shipped tf.txt extrinsic, at the bar of
    test_golden_host.py::test_g2_imu_propagation_and_euler.  Fails on the parent commit: no such symbol."""
    d = np.load(os.path.join(G, "g2_imu.npz"))
    imu6 = np.concatenate([d["imu"][:, 13:16], d["imu"][:, 25:28]], 1)
    got = _kernel(d["camm1"], d["camm2"], imu6, d["c2i"], 1.0 / 30.0, 1.0 / 100.0)
    want = d["out"]
    err = float(np.abs(got - want).max())
    print("kernel vs g2_imu out:", err)
    assert err <= 2e-5 * max(1.0, float(np.abs(want).max())), (err, got, want)


def test_imu_prediction_kernel_matches_the_float64_host_restatement():
    """The 64 seeded cases of tests/imu_cases.py (general extrinsic, 1-12 samples), then the edges: no sample, pose_m2 == pose_m1 with
    dt_cam = 1 (the tracker's idx < 2 case) and the identity extrinsic (the synthetic rig)."""
    cases = imu_cases.random_cases()
    for k, c in enumerate(cases):
        _held_to_host(c["p1"], c["p2"], c["imu6"], c["c2i"], c["dt_cam"], c["dt_imu"], f"case {k}")
    for k, c in enumerate(cases[:8]):
        got = _held_to_host(c["p1"], c["p2"], np.zeros((0, 6)), c["c2i"], c["dt_cam"], c["dt_imu"], f"n = 0, case {k}")
        q = c["p1"][:4] / np.linalg.norm(c["p1"][:4])
        assert abs(float(np.linalg.norm(got[:4].astype(np.float64))) - 1.0) <= 2.4e-7           # renormalised ...
        assert np.abs(np.abs(got[:4]) - np.abs(q)).max() <= 2.4e-7 and np.abs(got[4:] - c["p1"][4:]).max() <= 2.4e-7 * max(1.0, np.abs(c["p1"]).max())   # ... pose of pose_m1
        _held_to_host(c["p1"], c["p1"], c["imu6"], c["c2i"], 1.0, c["dt_imu"], f"pose_m2 == pose_m1, case {k}")
        g_imu = imu_cases.quat_to_R(c["p1"][:4]) @ np.asarray(pose_utils.GRAVITY)       # the accelerometer rows for the identity extrinsic
        imu6 = np.concatenate([c["imu6"][:, :3], c["imu6"][:, 3:] - c["imu6"][:, 3:].mean(0) + g_imu], 1)
        _held_to_host(c["p1"], c["p2"], imu6, np.eye(4), c["dt_cam"], c["dt_imu"], f"identity c2i, case {k}")


def test_imu_prediction_kernel_leaves_the_samples_alone():
    """The reference subtracts gravity from the caller's rows in place; the kernel reads them only: bit-identical before and after."""
    from mm3dgs_slam_amd.tracker import propagate_imu_device
    c = imu_cases.random_cases(8, seed=21)[3]
    imu6 = _dev(c["imu6"])
    before = imu6.clone()
    propagate_imu_device(_dev(c["p1"]), _dev(c["p2"]), imu6, _dev(c["c2i"]), c["dt_cam"], c["dt_imu"])
    torch.cuda.synchronize()
    assert torch.equal(imu6.view(torch.int32), before.view(torch.int32))


def test_imu_prediction_entry_point_refuses_bad_arguments_before_any_launch():
    """n = -1 and dt_cam = 0 (or a non-finite dt) give -2 with a text, a NULL out_pose (or imu6 with n > 0) gives -1; nothing is launched, so
    the output keeps its sentinel."""
    lib = _lib.load()
    c = imu_cases.random_cases(2, seed=4)[0]
    p1, p2, imu6, c2i = _dev(c["p1"]), _dev(c["p2"]), _dev(c["imu6"]), _dev(c["c2i"])
    out = torch.full((7,), -77.0, device=DEV)
    n = int(imu6.shape[0])
    P = lambda t: C.c_void_p(t.data_ptr())
    g = pose_utils.GRAVITY
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(imu=P(imu6), n=n, dt_cam=0.04, dt_imu=0.01, out_p=P(out)):
        return lib.mm3dgs_propagate_imu(P(p1), P(p2), imu, n, P(c2i), dt_cam, dt_imu, g[0], g[1], g[2], out_p, stream)

    assert call(n=-1) == -2 and b"n = -1" in lib.mm3dgs_last_error()
    assert call(dt_cam=0.0) == -2 and b"dt_cam" in lib.mm3dgs_last_error()
    assert call(dt_cam=float("nan")) == -2 and call(dt_imu=float("inf")) == -2
    assert call(out_p=C.c_void_p(None)) == -1
    assert call(imu=C.c_void_p(None)) == -1
    torch.cuda.synchronize()
    assert bool((out == -77.0).all())
    assert call(imu=C.c_void_p(None), n=0) == 0          # imu6 may be NULL when there is no sample
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == -77.0).any())


def _tracker(key, cls=None):
    from mm3dgs_slam_amd.config import utmm_config
    from mm3dgs_slam_amd.fused import FusedTracker
    c = imu_cases.random_cases(4, seed=13)[2]
    poses = [_dev(c["p2"]), _dev(c["p2"]), _dev(c["p1"]), None]
    rows = torch.from_numpy(imu_cases.rows30(c["imu6"])).float()
    cfg = utmm_config(device=DEV, tracking={"imu_on_device": key})
    trk = (cls or FusedTracker)(cfg, None, None, poses, tf={"c2i": torch.from_numpy(c["c2i"]).float()}, tstamps=[0.0, 0.04, 0.08, 0.12])
    return trk, rows, c


def test_device_imu_prediction_reads_nothing_back(monkeypatch):
    """predict_pose(idx >= 2) on device poses with Tensor.cpu / .item / .tolist / .numpy raising on a device tensor: with
    tracking.imu_on_device the call goes through (and returns the kernel's pose); with the key false the same patch makes it raise --
    the host path's pose read-back, i.e. the patch does see the drain."""
    on, rows, c = _tracker(True)
    off, _, _ = _tracker(False)
    on.predict_pose(3, rows.clone()); torch.cuda.synchronize()        # (first use: library load, pinned allocator, extrinsic upload)

    def guard(name):
        orig = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            if self.is_cuda:
                raise AssertionError(f"Tensor.{name} on a device tensor: a read-back")
            return orig(self, *a, **k)
        return f
    with monkeypatch.context() as m:
        for name in ("cpu", "item", "tolist", "numpy"):
            m.setattr(torch.Tensor, name, guard(name))
        pred = on.predict_pose(3, rows.clone())
        assert pred.is_cuda and pred.shape == (7,)
        with pytest.raises(AssertionError, match="read-back"):
            off.predict_pose(3, rows.clone())
    want = pose_utils.propagate_imu_np(imu_cases.f32(c["p1"]), imu_cases.f32(c["p2"]), c["imu6"], imu_cases.f32(c["c2i"]), 0.08 - 0.04, 0.01).astype(np.float32)
    err = float(np.abs(pred.cpu().numpy() - want).max())
    assert err <= 2.4e-7 * max(1.0, float(np.abs(want).max())), (err, pred, want)
    # idx - 2 < 0: p2 = p1, dt_cam = 1 (zero velocity at the start), as on the host path
    first = on.predict_pose(1, rows.clone()).cpu().numpy()
    p = imu_cases.f32(c["p2"])
    want = pose_utils.propagate_imu_np(p, p, c["imu6"], imu_cases.f32(c["c2i"]), 1.0, 0.01).astype(np.float32)
    assert float(np.abs(first - want).max()) <= 2.4e-7 * max(1.0, float(np.abs(want).max()))


def test_utmm_shaped_config_tracks_from_the_device_imu_prediction():
    """test_gpu_fused.py::test_utmm_shaped_config_with_imu_runs_natively_and_tracks with tracking.imu_on_device: the same 5 frames, 166x320,
    30 k Gaussians, the same seeds and the same bars -- pose errors of frames 1-4 under 1 cm, the frame-4 prediction within 2e-2 of the
    ground truth -- and that prediction equal to propagate_imu_np of the tracker's own estimates to the 2-ulp bar."""
    from mm3dgs_slam_amd.config import utmm_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = utmm_config(device=DEV, tracking={"iters": 30, "use_imu_loss": True, "imu_T_weight": 1.0, "imu_q_weight": 0.1, "imu_on_device": True},
                      mapping={"iters": 20})
    cfg["desired_height"], cfg["desired_width"] = 166, 320
    for k in ("fx", "fy", "cx", "cy"):
        cfg["cam"][k] *= 0.5
    seq = SyntheticSequence(cfg, 5, 30000, seed=3)
    slam = SLAM(cfg, seq)
    assert type(slam.tracker).__name__ == "FusedTracker" and type(slam.mapper).__name__ == "FusedMapper"
    for i in range(5):
        slam.step(i)
    errs = slam.pose_errors()
    print("pose errors:", errs)
    assert max(errs[1:]) < 0.01, errs
    rows = seq.imu(4)
    pred = slam.tracker.predict_pose(4, rows)
    assert pred.is_cuda
    imu6 = torch.cat([rows[:, 13:16], rows[:, 25:28]], 1).double().numpy()
    want = pose_utils.propagate_imu_np(slam.estimate_pose_list[3].cpu().double().numpy(), slam.estimate_pose_list[2].cpu().double().numpy(), imu6,
                                       seq.tf["c2i"].double().numpy(), seq.tstamps[3] - seq.tstamps[2], 0.01).astype(np.float32)
    err = float(np.abs(pred.cpu().numpy() - want).max())
    print("frame-4 prediction: |device - propagate_imu_np| =", err)
    assert err <= 2.4e-7 * max(1.0, float(np.abs(want).max())), (err, pred, want)
    assert (pred - seq.poses[4]).abs().max() < 2e-2
