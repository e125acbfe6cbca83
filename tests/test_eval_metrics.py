"""The image evaluation on the host (mm3dgs_slam_amd/eval_utils.py: image_metrics_host, camera_centers) and the pieces that need no GPU:
the C ABI of mm3dgs_eval_image, the config key, the refusals.  tests/test_gpu_eval.py holds the kernels to image_metrics_host."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import eval_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mm3dgs_eval_image", "mm3dgs_eval_image_work_bytes")


def test_header_binding_and_library_carry_the_two_symbols():
    from mm3dgs_slam_amd import _lib
    header = open(os.path.join(ROOT, "include", "mm3dgs.h")).read()
    declared = set(re.findall(r"\b(mm3dgs_[a-z_]+)\s*\(", header))
    for name in SYMBOLS:
        assert name in declared and name in _lib.exported_symbols(), name
    assert int(re.search(r"#define\s+MM3DGS_ABI_VERSION\s+(\d+)", header).group(1)) == 213      # purely additive
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    # the size function needs no device: one row of 12 doubles per 16x16 tile, 0 for a rejected shape
    assert lib.mm3dgs_eval_image_work_bytes(480, 640) >= 30 * 40 * 12 * 8
    assert lib.mm3dgs_eval_image_work_bytes(1, 1) >= 12 * 8 and lib.mm3dgs_eval_image_work_bytes(1, 1) % 8 == 0
    for H, W in ((0, 5), (5, 0), (-1, 5), (5, -1), (1 << 14, (1 << 14) + 1)):
        assert lib.mm3dgs_eval_image_work_bytes(H, W) == 0, (H, W)
    assert lib.mm3dgs_eval_image_work_bytes(1 << 14, 1 << 14) > 0


@pytest.mark.parametrize("family,H,W", ec.CASES)
def test_host_metrics_equal_the_independent_statement(family, H, W):
    """image_metrics_host (conv2d, torch float64) against the numpy restatement (shifted slices): two float64 evaluations, 1e-12 relative
    (unit roundoff 1.1e-16 over 121-term windows and <= 99 072-term sums); its psnr and ssim against today's float32 chain within 1e-5 dB
    and 1e-6 (measured on these inputs: <= 2.2e-6 dB, <= 2.5e-7)."""
    from mm3dgs_slam_amd.eval_utils import image_metrics_host, psnr
    from mm3dgs_slam_amd.loss_utils import ssim
    image, gt, depth, gt_depth = ec.inputs(family, H, W)
    row = ec.reference(family, H, W)
    assert row.dtype == torch.float64 and tuple(row.shape) == (16,)
    want = ec.statement(image, gt, depth, gt_depth)
    got = row.numpy()
    assert float(got[4:7].min()) >= 1.6e-4 and math.isfinite(got[0])      # what the GPU test's relative bounds rely on
    assert got[3] == want[3] and not got[11:].any()
    for c in range(11):
        if c != 3:
            assert abs(got[c] - want[c]) <= 1e-12 * abs(want[c]), (c, got[c], want[c])
    d_psnr = abs(float(psnr(image, gt).mean()) - got[0])
    d_ssim = abs(float(ssim(image, gt)) - got[1])
    print(f"EVALHOST {family} {H}x{W}: |psnr32 - psnr64| = {d_psnr:.2e} dB, |ssim32 - ssim64| = {d_ssim:.2e}")
    assert d_psnr <= 1e-5 and d_ssim <= 1e-6
    assert torch.equal(image_metrics_host(image, gt)[[0, 1, 4, 5, 6, 7, 8, 9]], row[[0, 1, 4, 5, 6, 7, 8, 9]])      # the colour part does not depend on depth


def test_degenerate_rows_on_the_host():
    from mm3dgs_slam_amd.eval_utils import image_metrics_host
    cases = ec.degenerate_cases()
    same = image_metrics_host(*cases["same"]).numpy()
    assert same[0] == math.inf and not same[4:7].any() and abs(same[1] - 1.0) <= 1e-12 and np.allclose(same[7:10], 1.0, atol=1e-12)
    for name in ("no_valid", "no_depth"):
        row = image_metrics_host(*cases[name]).numpy()
        assert math.isnan(row[2]) and math.isnan(row[10]) and row[3] == 0.0, name
        assert math.isfinite(row[0]) and math.isfinite(row[1])
    image, gt, depth, gd = cases["planted"]
    H, W = gd.shape
    row = image_metrics_host(image, gt, depth, gd).numpy()
    assert row[3] == H * W - 5                                    # of the six planted values only 1e-30 counts
    tiny = image_metrics_host(*cases["only_tiny"]).numpy()
    assert tiny[3] == 1.0 and tiny[2] == abs(float(depth[0, 2]) - float(np.float32(1e-30))) and tiny[10] == tiny[2]
    want = ec.statement(image, gt, depth, gd)
    assert abs(row[2] - want[2]) <= 1e-12 * want[2] and abs(row[10] - want[10]) <= 1e-12 * want[10]
    nan_depth = depth.clone()
    nan_depth[5, 5] = float("nan")                                # a NaN of the rendered depth at a valid pixel propagates ...
    assert math.isnan(float(image_metrics_host(image, gt, nan_depth, gd)[2]))
    nan_depth = depth.clone()
    nan_depth[0, 0] = float("nan")                                # ... and at an invalid one never reaches the sums
    assert float(image_metrics_host(image, gt, nan_depth, gd)[2]) == row[2]
    with pytest.raises(ValueError):
        image_metrics_host(image, gt, depth, None)


def test_camera_centers_inverts_a_pose_and_twice_returns_it():
    from mm3dgs_slam_amd.eval_utils import camera_centers
    # one pose by hand: a quarter turn about z (x -> y) and t = (1, 2, 3): R^T = a quarter turn back, -R^T t = (-2, 1, -3)
    h = math.sqrt(0.5)
    inv = camera_centers(np.array([[h, 0.0, 0.0, h, 1.0, 2.0, 3.0]]))
    assert inv.dtype == torch.float64 and tuple(inv.shape) == (1, 7)
    assert np.allclose(inv.numpy(), [[h, 0.0, 0.0, -h, -2.0, 1.0, -3.0]], atol=1e-15)
    g = torch.Generator().manual_seed(3)
    q = torch.randn(20, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True) * torch.sign(q[:, :1])     # unit, w > 0
    poses = torch.cat([q, torch.randn(20, 3, generator=g, dtype=torch.float64)], 1)
    back = camera_centers(camera_centers(poses))
    assert float((back - poses).abs().max()) <= 1e-12
    # against the matrix route of the reference's script, in float64
    from mm3dgs_slam_amd.pose_utils import quad2rotation
    M = torch.eye(4, dtype=torch.float64).repeat(20, 1, 1)
    M[:, :3, :3], M[:, :3, 3] = quad2rotation(poses[:, :4]), poses[:, 4:]
    assert float((torch.linalg.inv(M)[:, :3, 3] - camera_centers(poses)[:, 4:]).abs().max()) <= 1e-12


def test_c2w_ate_of_a_similarity_transformed_copy_is_zero():
    """Umeyama aligns scale, rotation and translation: a trajectory against a similarity-transformed copy of its camera centres."""
    from mm3dgs_slam_amd.eval_utils import camera_centers, evaluate_ate_rmse
    from mm3dgs_slam_amd.pose_utils import quad2rotation, rotation2quad
    g = torch.Generator().manual_seed(4)
    n = 30
    q = torch.randn(n, 4, generator=g, dtype=torch.float64)
    c2w = torch.cat([q / q.norm(dim=1, keepdim=True), torch.randn(n, 3, generator=g, dtype=torch.float64)], 1)
    S = quad2rotation(torch.tensor([[0.8, 0.1, -0.5, 0.3]], dtype=torch.float64))[0]
    moved = torch.cat([rotation2quad(S @ quad2rotation(c2w[:, :4])), 1.7 * (c2w[:, 4:] @ S.T) + torch.tensor([0.3, -2.0, 5.0], dtype=torch.float64)], 1)
    est, gt = camera_centers(c2w), camera_centers(moved)          # two world->camera trajectories whose centres differ by the similarity
    assert float((camera_centers(est)[:, 4:] - c2w[:, 4:]).abs().max()) <= 1e-12
    _, rmse = evaluate_ate_rmse(camera_centers(est).numpy(), camera_centers(gt).numpy())
    print(f"EVALHOST c2w ATE of a similarity-transformed copy: {rmse:.2e} m")
    assert rmse <= 1e-6


def test_key_defaults_to_off_and_the_device_paths_refuse_the_host():
    from mm3dgs_slam_amd.config import default_config, utmm_config
    from mm3dgs_slam_amd.eval_utils import image_metrics_device
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from mm3dgs_slam_amd.renderer import Renderer
    from oracle.raster_ref import RefRasterizer
    assert default_config(device="cpu")["eval_on_device"] is False and utmm_config(device="cpu")["eval_on_device"] is False
    image, gt, depth, gt_depth = ec.inputs("random", 5, 7)
    with pytest.raises(RuntimeError, match="device tensors"):
        image_metrics_device(image, gt, depth, gt_depth, torch.zeros(16, dtype=torch.float64))
    cfg = default_config(device="cpu", height=32, width=48, eval_on_device=True)
    seq = SyntheticSequence(default_config(device="cpu", height=32, width=48), 1, 300, seed=1, renderer=Renderer(cfg, rasterizer_cls=RefRasterizer))
    with pytest.raises(ValueError, match="eval_on_device"):
        SLAM(cfg, seq, rasterizer_cls=RefRasterizer)
    slam = SLAM(default_config(device="cpu", height=32, width=48), seq, rasterizer_cls=RefRasterizer)
    slam.cfg["eval_on_device"] = True
    with pytest.raises(ValueError, match="eval_on_device"):
        slam.evaluate_images(1)
