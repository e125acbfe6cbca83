"""The depth alignment's float64 restatement (tests/depth_align_ref.py) held to the reference's own fixture, to the host path
(depth_utils.get_scale_shift_LS) and to the singular cases, and the CPU side of the opt-in key depth_align_on_device: the C ABI names,
the default, and that CPU tensors keep taking the host path.  The kernels themselves are held in tests/test_gpu_depth_align.py."""
import os

import numpy as np
import pytest
import torch

from tests import depth_align_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def test_restatement_reproduces_the_reference_least_squares_fixture():
    """tests/golden/g11_depth_align.npz (the reference's get_scale_shift, utils/depth_utils.py:44-99) at the bars of
    test_golden_host.py::test_g11_depth_alignment_matches_the_reference_least_squares; the stored mask goes in as a 0 / 1 silhouette with
    est_min = -inf, as the GPU test passes it to the kernel."""
    F = np.load(os.path.join(HERE, "golden", "g11_depth_align.npz"))
    for k in range(3):
        est, depth, mask = (F[f"c{k}_{n}"] for n in ("est", "depth", "mask"))
        fit = R.align_ref(est, depth, mask.astype(np.float32), est_min=-np.inf)
        rs, rt = float(F[f"c{k}_scale"].reshape(-1)[0]), float(F[f"c{k}_shift"].reshape(-1)[0])
        print(f"g11 case {k}: scale {float(fit['scale'])!r} (reference {rs!r}), shift {float(fit['shift'])!r} ({rt!r})")
        assert fit["ok"]
        assert abs(float(fit["scale"]) - rs) <= 2e-4 * abs(rs), (k, fit["scale"], rs)
        assert abs(float(fit["shift"]) - rt) <= 2e-4 * abs(rt) + 1e-6, (k, fit["shift"], rt)
        scaled, ref = R.apply_ref(est, fit["scale"], fit["shift"]), F[f"c{k}_scaled"]
        ok = mask.astype(bool) & np.isfinite(ref) & (np.abs(ref) < 50)
        assert (np.abs(scaled - ref)[ok] <= 1e-3 * np.abs(ref)[ok] + 1e-4).all(), k


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_agrees_with_the_host_path(shape):
    """Float32 scale and shift of the restatement against get_scale_shift_LS on the seeded inputs of every shape of the GPU test, at
    bar B (depth_align_ref.bar_scale / bar_shift); ok and the identity fit at 1x1."""
    from mm3dgs_slam_amd.depth_utils import get_scale_shift_LS
    est, depth, sil = R.make_inputs(*shape)
    fit = R.align_ref(est, depth, sil)
    te, td, ts = (torch.from_numpy(a) for a in (est, depth, sil))
    s, t, ok = get_scale_shift_LS(te, td, (ts > 0.99) & (te > 1e-6), return_ok=True)
    ds, dt = abs(float(s) - float(fit["scale"])), abs(float(t) - float(fit["shift"]))
    bs, bt = R.bar_scale(fit["scale"]), R.bar_shift(fit["scale"], fit["shift"], np.abs(est).mean())
    print(f"{shape}: n = {fit['n']:.0f}, ok = {fit['ok']}, |d scale| = {ds:.3e} (bar {bs:.3e}), |d shift| = {dt:.3e} (bar {bt:.3e})")
    assert bool(ok) == fit["ok"] == (shape != (1, 1))
    assert ds <= bs and dt <= bt
    if shape == (1, 1):
        assert float(fit["scale"]) == 1.0 and float(fit["shift"]) == 0.0 and fit["n"] == 1.0
    if shape == (1, 2):
        assert fit["n"] == 2.0          # exactly determined: the line through the two pixels
        assert np.allclose(float(fit["scale"]) * est.astype(np.float64) + float(fit["shift"]), 1.0 / depth.astype(np.float64), rtol=1e-4)


def test_restatement_gives_the_identity_on_the_singular_cases():
    """The cases of test_golden_host.py::test_depth_alignment_ignores_masked_out_garbage_and_survives_a_singular_fit: no valid pixel, a
    constant estimate (0.25: exact sums; 0.3: sums that do not cancel exactly), a nearly constant one -- scale 1, shift 0, ok 0 -- and
    garbage of the estimate outside the mask does not move the fit by a bit."""
    g = torch.Generator().manual_seed(3)
    depth = 1.0 + 3.0 * torch.rand(24, 32, generator=g)
    est = 0.7 / depth + 0.05
    mask = torch.rand(24, 32, generator=g) > 0.3
    nearly = torch.full_like(est, 0.3) * (1.0 + 2e-7 * torch.randn(24, 32, generator=g))
    sil = mask.float().numpy()
    for e, m in ((est, np.zeros_like(sil)), (torch.full_like(est, 0.25), sil), (torch.full_like(est, 0.3), sil), (nearly, sil)):
        fit = R.align_ref(e.numpy(), depth.numpy(), m)
        assert float(fit["scale"]) == 1.0 and float(fit["shift"]) == 0.0 and not fit["ok"]
        assert list(fit["fit"][:3]) == [1.0, 0.0, 0.0] and not fit["fit"][8:].any()
    clean = R.align_ref(est.numpy(), depth.numpy(), sil)
    assert clean["ok"]
    dirty = est.clone()
    dirty[~mask] = float("nan")
    dirty.view(-1)[int((~mask).view(-1).nonzero()[0])] = float("inf")
    assert np.array_equal(R.align_ref(dirty.numpy(), depth.numpy(), sil)["fit"], clean["fit"])
    # the deliberate difference from the host path: a depth whose inverse overflows is left out (the host path returns NaN there)
    tiny = depth.numpy().copy()
    idx = np.argwhere(mask.numpy())[0]
    tiny[idx[0], idx[1]] = np.float32(1e-45)
    left_out = R.align_ref(est.numpy(), tiny, sil)
    assert left_out["ok"] and left_out["n"] == clean["n"] - 1 and np.isfinite(left_out["fit"]).all()


def test_the_c_abi_declares_the_alignment_entry_points():
    """Fails on the parent commit: its library has no such symbols."""
    from mm3dgs_slam_amd import _lib
    assert {"mm3dgs_align_depth", "mm3dgs_align_depth_work_bytes"} <= set(_lib.exported_symbols())


def test_the_key_is_off_by_default():
    from mm3dgs_slam_amd.config import default_config, utmm_config
    assert default_config()["depth_align_on_device"] is False and utmm_config()["depth_align_on_device"] is False


@pytest.mark.parametrize("dataset, idx", [("synthetic", 0), ("synthetic", 2), ("utmm", 0), ("utmm", 2)])
def test_cpu_tensors_take_the_host_path_with_the_key_on(dataset, idx):
    """scale_depth_estimate(on_device=True) on CPU tensors: the host code, bit for bit what on_device=False returns, on the first frame
    (the arbitrary scale; UT-MM: the fit to the sensor depth) and on a later one."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.depth_utils import scale_depth_estimate
    cfg = default_config(device="cpu", height=17, width=23, use_gt_depth=False)
    cfg["dataset"] = dataset
    est, depth, sil = (torch.from_numpy(a) for a in R.make_inputs(17, 23))
    render = lambda: (depth * 1.25, sil)
    off = scale_depth_estimate(cfg, idx, est, depth, render)
    on = scale_depth_estimate(cfg, idx, est, depth, render, on_device=True)
    on2, fit = scale_depth_estimate(cfg, idx, est, depth, render, on_device=True, return_fit=True)
    assert fit is None
    assert torch.equal(off.view(torch.int32), on.view(torch.int32)) and torch.equal(off.view(torch.int32), on2.view(torch.int32))
