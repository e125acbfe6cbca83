"""Trajectory / image metrics the harness writes into ``results.npz`` (reference ``utils/eval_utils.py:139-189,231-294``,
``utils/image_utils.py:17-19``).  Pose part only: LPIPS needs a downloaded VGG network (out of scope).

``evaluate_ate_rmse(est, gt, "umeyama")`` aligns the translation columns ``[:, 4:]`` of the ESTIMATE to the ground truth with the
similarity transform of Umeyama (IEEE PAMI 13(4), 1991; scale + rotation + translation, reflection guarded by the sign of
det(U) det(V)), rotates the estimated quaternions by the same rotation, and returns (aligned poses [n,7], RMSE of the residual
translation).  The reference calls it on the raw 7-vectors (world->camera), ``slam/SLAM.py:339-343``; ``camera_centers`` gives the
inverse-pose vectors its ``scripts/eval_traj.py:68-77`` aligns instead ("ATE RMSE c2w").

Image part: one frame's scores are a row of sixteen float64 values (include/mm3dgs.h, mm3dgs_eval_image) -- psnr, ssim, depth_l1, n,
mse[3], ssim[3], depth_rmse, five zeros.  ``image_metrics_host`` states them in plain torch float64 on any device (the reference and the
CPU path); ``image_metrics_device`` is the same row from two HIP launches (csrc/eval.hip), written into a row of a device table so that a
whole evaluation is read back once (the opt-in key ``eval_on_device``, ``SLAM.evaluate_images``)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from .loss_utils import window_1d
from .pose_utils import quad2rotation, rotation2quad


def align_umeyama(model: np.ndarray, data: np.ndarray, known_scale: bool = False):
    """s, R, t with model ~ s R data + t (least squares over the n x 3 point sets)."""
    mu_m, mu_d = model.mean(0), data.mean(0)
    m0, d0 = model - mu_m, data - mu_d
    n = model.shape[0]
    C = m0.T @ d0 / n
    sigma2 = (d0 * d0).sum() / n
    U, D, Vt = np.linalg.svd(C)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt.T) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    s = 1.0 if known_scale else float(np.trace(np.diag(D) @ S) / sigma2)
    t = (mu_m - s * R @ mu_d)[:, None]
    return s, R, t


def align_horn(model: np.ndarray, data: np.ndarray):
    """Closed-form rigid alignment of Horn (reference ``utils/eval_utils.py:193-228``): R, t with data ~ R model + t for 3 x n point
    sets, and the per-point residual norms."""
    mu_m, mu_d = model.mean(1, keepdims=True), data.mean(1, keepdims=True)
    Wm = (model - mu_m) @ (data - mu_d).T                   # sum of outer(model_i, data_i)
    U, _, Vh = np.linalg.svd(Wm.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1
    R = U @ S @ Vh
    t = mu_d - R @ mu_m
    err = R @ model + t - data
    return R, t, np.sqrt((err * err).sum(0))


def evaluate_ate_rmse(est_poses, gt_poses, method: str = "umeyama"):
    assert len(est_poses) == len(gt_poses), "Estimated trajectory and GT trajectory must have equal length"
    est = est_poses.detach().cpu().numpy() if isinstance(est_poses, torch.Tensor) else np.asarray(est_poses)
    gt = gt_poses.detach().cpu().numpy() if isinstance(gt_poses, torch.Tensor) else np.asarray(gt_poses)
    est_traj, gt_traj = est[:, 4:], gt[:, 4:]
    aligned = est.copy()
    if method.lower() == "umeyama":
        s, R, t = align_umeyama(gt_traj, est_traj)
        q = rotation2quad(torch.matmul(torch.tensor(R).float(), quad2rotation(torch.as_tensor(est[:, :4]).float()).float()))
        aligned[:, :4] = q.numpy()
        aligned[:, 4:] = (s * (R @ est_traj.T) + t).T
        ate = np.linalg.norm(aligned[:, 4:] - gt_traj, axis=1)
    elif method.lower() == "horn":       # rigid (no scale), utils/eval_utils.py:249-266
        R, t, ate = align_horn(est_traj.T, gt_traj.T)
        q = rotation2quad(torch.matmul(torch.tensor(R).float(), quad2rotation(torch.as_tensor(est[:, :4]).float()).float()))
        aligned[:, :4] = q.numpy()
        aligned[:, 4:] = (R @ est_traj.T + t).T
    else:                                # (the reference's fall-through, utils/eval_utils.py:231-294: no alignment -- said aloud here)
        import warnings
        warnings.warn(f"evaluate_ate_rmse: unknown alignment method {method!r} (umeyama / horn): the trajectories are compared without alignment")
        ate = np.linalg.norm(est_traj - gt_traj, axis=1)
    rmse = float(np.sqrt(np.dot(ate, ate) / len(ate)))
    if isinstance(est_poses, torch.Tensor):
        aligned = torch.tensor(aligned)
    return aligned, rmse


def psnr(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    mse = ((img1 - img2) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def camera_centers(poses7):
    """The inverse of every pose 7-vector (qw,qx,qy,qz,tx,ty,tz): world->camera in, camera->world out -- what scripts/eval_traj.py:68-77
    builds with get_tensor_from_camera(inv(get_camera_from_tensor(p))), here in closed form (R^T, -R^T t) and float64.  The translation
    columns are the camera centres: ``evaluate_ate_rmse(camera_centers(est), camera_centers(gt))`` is the reference's "ATE RMSE c2w".
    Of the two quaternions of a rotation the one with w >= 0 is returned, so that inverting twice returns a pose given that way.
    Returns a float64 tensor [n,7] on the CPU."""
    p = torch.as_tensor(np.asarray(poses7.detach().cpu()) if isinstance(poses7, torch.Tensor) else np.asarray(poses7), dtype=torch.float64)
    p = p.reshape(-1, 7)
    Rt = quad2rotation(p[:, :4]).transpose(1, 2)
    t = -(Rt @ p[:, 4:, None])[:, :, 0]
    q = rotation2quad(Rt)
    q = torch.where(q[:, :1] < 0, -q, q)
    return torch.cat([q, t], 1)


def image_metrics_host(image, gt, depth=None, gt_depth=None):
    """The sixteen scores of one frame (include/mm3dgs.h, mm3dgs_eval_image) in plain torch float64, on the inputs' device: image, gt
    [3,H,W]; depth, gt_depth [H,W], both or neither.  [0] psnr = mean over the channels of 20 log10(1 / sqrt(mse_c)) (+inf for mse_c == 0),
    [1] ssim (utils/loss_utils.py:95-154: window = outer product of the float32 taps, zero padding 5, C1 = 0.01^2, C2 = 0.03^2),
    [2] depth_l1 = mean |depth - gt_depth| over { 0 < gt_depth < +inf, a float32 test } (NaN without such a pixel or without depth images),
    [3] the number of those pixels, [4..6] mse_c, [7..9] the channels' SSIM means, [10] depth_rmse over the same pixels, [11..15] zeros."""
    if (depth is None) != (gt_depth is None):
        raise ValueError("image_metrics_host: depth and gt_depth are given together or not at all")
    x, g = image.detach().double(), gt.detach().double()
    if x.dim() != 3 or x.shape[0] != 3 or x.shape != g.shape:
        raise ValueError(f"image_metrics_host: image and gt are [3,H,W] images of one size; got {tuple(image.shape)}, {tuple(gt.shape)}")
    hw = float(x.shape[1] * x.shape[2])
    row = torch.zeros(16, dtype=torch.float64, device=x.device)
    mse = ((x - g) ** 2).reshape(3, -1).sum(1) / hw
    row[0] = (20.0 * torch.log10(1.0 / torch.sqrt(mse))).mean()
    row[4:7] = mse
    w1 = window_1d().to(x.device).double()
    w2 = (w1[:, None] * w1[None, :]).expand(3, 1, 11, 11).contiguous()
    blur = lambda t: F.conv2d(t[None], w2, padding=5, groups=3)[0]
    mu1, mu2 = blur(x), blur(g)
    s11, s22, s12 = blur(x * x) - mu1 * mu1, blur(g * g) - mu2 * mu2, blur(x * g) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    smap = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))
    per_channel = smap.reshape(3, -1).sum(1)
    row[1] = per_channel.sum() / (3.0 * hw)
    row[7:10] = per_channel / hw
    row[2] = row[10] = float("nan")
    if depth is not None:
        gd = gt_depth.detach().float()
        if depth.shape != gd.shape or tuple(gd.shape) != tuple(x.shape[1:]):
            raise ValueError(f"image_metrics_host: depth and gt_depth are [H,W] images of the colour images' size; got {tuple(depth.shape)}, {tuple(gd.shape)}")
        valid = (gd > 0) & (gd < float("inf"))
        d = (depth.detach().double() - gd.double()).abs()[valid]
        n = int(valid.sum())
        row[3] = n
        if n > 0:
            row[2] = d.sum() / n
            row[10] = torch.sqrt((d * d).sum() / n)
    return row


_EVAL_WORK = {}      # (H, W, device) -> the kernels' tile-row buffer (contents irrelevant between calls; calls on one stream are ordered)
_EVAL_WINDOW = None


def image_metrics_device(image, gt, depth, gt_depth, row_out):
    """The row of ``image_metrics_host`` by mm3dgs_eval_image (csrc/eval.hip): two launches on the current stream, written to ``row_out``
    -- 16 float64 on the device, typically ``table[k]`` of an ``[n,16]`` table --, nothing read back.  depth and gt_depth: both or both
    None.  Views are taken as they are when their elements are contiguous (planes of a [6,H,W] render); there is no host path behind this
    function: host tensors raise."""
    import ctypes as C
    from . import _lib
    from .rasterizer import _stream
    global _EVAL_WINDOW
    tensors = [image, gt, row_out] + ([] if depth is None else [depth]) + ([] if gt_depth is None else [gt_depth])
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError("image_metrics_device needs device tensors (the host path is image_metrics_host)")
    if (depth is None) != (gt_depth is None):
        raise ValueError("image_metrics_device: depth and gt_depth are given together or not at all")
    if image.dim() != 3 or image.shape[0] != 3 or image.shape != gt.shape:
        raise ValueError(f"image_metrics_device: image and gt are [3,H,W] images of one size; got {tuple(image.shape)}, {tuple(gt.shape)}")
    H, W = int(image.shape[1]), int(image.shape[2])
    if depth is not None and (tuple(depth.shape) != (H, W) or tuple(gt_depth.shape) != (H, W)):
        raise ValueError(f"image_metrics_device: depth and gt_depth are [{H},{W}] images; got {tuple(depth.shape)}, {tuple(gt_depth.shape)}")
    if row_out.dtype != torch.float64 or row_out.numel() != 16 or not row_out.is_contiguous():
        raise ValueError("image_metrics_device: row_out is 16 contiguous float64 values")
    prep = lambda t: None if t is None else t.detach().float().contiguous()      # (no copy for a float32 tensor with contiguous elements)
    image_c, gt_c, depth_c, gt_depth_c = prep(image), prep(gt), prep(depth), prep(gt_depth)
    lib = _lib.load()
    key = (H, W, image_c.device)
    work = _EVAL_WORK.get(key)
    if work is None:
        work = _EVAL_WORK[key] = torch.empty(int(lib.mm3dgs_eval_image_work_bytes(H, W)) // 8, dtype=torch.float64, device=image_c.device)
    if _EVAL_WINDOW is None:
        _EVAL_WINDOW = (C.c_float * 11)(*window_1d().tolist())
    ptr = _lib.ptr
    _lib.check(lib.mm3dgs_eval_image(H, W, ptr(image_c), ptr(gt_c), ptr(depth_c), ptr(gt_depth_c), _EVAL_WINDOW, ptr(work), ptr(row_out),
                                     _stream()))
    return row_out
