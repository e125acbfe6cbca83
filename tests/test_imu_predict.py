"""The tracker's IMU pose prediction on the device (tracking.imu_on_device, ABI 213), host side: the float64 numpy restatement
pose_utils.propagate_imu_np -- the yardstick mm3dgs_propagate_imu is held to on the GPU (tests/test_gpu_imu_predict.py) -- against the
reference's own output and against pose_utils.propagate_imu; the C ABI; the config key and the tracker's choice of path on CPU poses."""
import os

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import _lib, pose_utils
from tests import imu_cases

G = os.path.join(os.path.dirname(__file__), "golden")


def test_numpy_imu_propagation_reproduces_the_reference_output():
    """tests/golden/g2_imu.npz: the reference's propagate_imu on 8 samples with the shipped tf.txt extrinsic (not the identity), at the bar
    of test_golden_host.py::test_g2_imu_propagation_and_euler."""
    d = np.load(os.path.join(G, "g2_imu.npz"))
    imu6 = np.concatenate([d["imu"][:, 13:16], d["imu"][:, 25:28]], 1)
    before = imu6.copy()
    got = pose_utils.propagate_imu_np(d["camm1"], d["camm2"], imu6, d["c2i"], 1.0 / 30.0, 1.0 / 100.0)
    want = d["out"].astype(np.float64)
    err = np.abs(got - want).max()
    print("propagate_imu_np vs g2_imu out:", err)
    assert got.dtype == np.float64 and got.shape == (7,)
    assert err <= 2e-5 * max(1.0, np.abs(want).max()), err
    assert np.array_equal(imu6, before)            # the samples are read only (the reference subtracts gravity in place)


def test_numpy_imu_propagation_matches_the_torch_one_in_float64(monkeypatch):
    """64 seeded cases (tests/imu_cases.py), propagate_imu_np against pose_utils.propagate_imu evaluated in float64 torch, to 1e-12: both
    double, only the operation order (closed-form rigid inverses against torch.linalg.inv, numpy against torch products) differs.

    pose_utils.propagate_imu mirrors the reference's float32 habits -- get_camera_from_tensor ends in .float(), euler_matrix starts from
    torch.eye(4) of the default dtype -- so it is run here with float64 as torch's default dtype and Tensor.float keeping doubles:
    the same function, every intermediate in double."""
    monkeypatch.setattr(torch.Tensor, "float", lambda self, *a, **k: self.double())
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        worst = 0.0
        for c in imu_cases.random_cases():
            rows = torch.from_numpy(imu_cases.rows30(c["imu6"]))
            want = pose_utils.propagate_imu(torch.from_numpy(c["p1"]), torch.from_numpy(c["p2"]), rows, torch.from_numpy(c["c2i"]), c["dt_cam"], c["dt_imu"])
            assert want.dtype == torch.float64
            got = pose_utils.propagate_imu_np(c["p1"], c["p2"], c["imu6"], c["c2i"], c["dt_cam"], c["dt_imu"])
            err = np.abs(got - want.numpy()).max()
            worst = max(worst, err)
            assert err <= 1e-12, (err, got, want)
    finally:
        torch.set_default_dtype(old)
    print("propagate_imu_np vs float64 torch, worst of 64:", worst)


def test_numpy_imu_propagation_edge_cases():
    """No sample: the pose of frame idx-1 with a unit quaternion.  Identity extrinsic, equal poses (the tracker's idx < 2 case: zero velocity)
    and samples that only carry gravity: the pose stays where it is."""
    c = imu_cases.random_cases(4, seed=9)[0]
    got = pose_utils.propagate_imu_np(c["p1"], c["p2"], np.zeros((0, 6)), c["c2i"], c["dt_cam"], c["dt_imu"])
    want = np.concatenate([c["p1"][:4] / np.linalg.norm(c["p1"][:4]), c["p1"][4:]])
    if want[np.argmax(np.abs(want[:4]))] < 0:      # (the branch makes the largest component positive)
        want[:4] = -want[:4]
    assert np.abs(got - want).max() <= 1e-14
    g_imu = imu_cases.quat_to_R(c["p1"][:4]) @ np.asarray(pose_utils.GRAVITY)
    still = np.concatenate([np.zeros((5, 3)), np.tile(g_imu, (5, 1))], 1)
    got = pose_utils.propagate_imu_np(c["p1"], c["p1"], still, np.eye(4), 1.0, 0.01)
    assert np.abs(got - want).max() <= 1e-14


def test_library_exports_the_imu_prediction_at_abi_213():
    """Fails on the parent commit (ABI 212, no such symbol)."""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _lib.load()
    assert "mm3dgs_propagate_imu" in _lib.exported_symbols()
    assert hasattr(lib, "mm3dgs_propagate_imu")
    assert lib.mm3dgs_version() == 213


def test_imu_on_device_is_opt_in_and_cpu_poses_take_the_host_path():
    """tracking.imu_on_device defaults to false; with the key true and poses on the CPU (the torch-graph loops on the CPU) predict_pose
    is the host chain, bit for bit."""
    from mm3dgs_slam_amd.config import default_config, utmm_config
    from mm3dgs_slam_amd.tracker import Tracker
    assert default_config(device="cpu")["tracking"]["imu_on_device"] is False
    assert utmm_config(device="cpu")["tracking"]["imu_on_device"] is False
    c = imu_cases.random_cases(4, seed=2)[1]
    poses = [torch.from_numpy(c["p2"]).float(), torch.from_numpy(c["p1"]).float(), None]
    rows = torch.from_numpy(imu_cases.rows30(c["imu6"])).float()
    tf, ts = {"c2i": torch.from_numpy(c["c2i"]).float()}, [0.0, 0.04, 0.08]
    got = {}
    for key in (False, True):
        cfg = utmm_config(device="cpu", tracking={"imu_on_device": key})
        got[key] = Tracker(cfg, None, None, poses, tf=tf, tstamps=ts).predict_pose(2, rows.clone())
    want = pose_utils.propagate_imu(poses[1], poses[0], rows.clone(), tf["c2i"], 0.04, 0.01)
    assert torch.equal(got[False], want) and torch.equal(got[True], want)
