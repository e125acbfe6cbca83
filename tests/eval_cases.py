"""Cases and host statements that tests/test_eval_metrics.py (CPU) and tests/test_gpu_eval.py (GPU) share for the image evaluation
(include/mm3dgs.h: mm3dgs_eval_image; mm3dgs_slam_amd/eval_utils.py: image_metrics_host / image_metrics_device).

The inputs are those of the loss tests (tests/loss_ref.py make_inputs: `out6[:3]`, `gt`, `out6[3]`, `ref` as image, gt, depth, gt_depth).
`statement` restates the sixteen values from the header's formulas in numpy float64 without a convolution operator (two passes of shifted
slices); `ssim_maps` is torch's own evaluation of the SSIM map in a chosen dtype, for the measured float32 distance E32."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import loss_ref as lr

SHAPES = [(1, 1), (5, 7), (16, 16), (17, 33), (37, 21), (48, 64), (80, 208), (16, 2064)]
FAMILIES = lr.FAMILIES
CASES = [(f, H, W) for f in FAMILIES for H, W in SHAPES]
DOUBLE_COLS = (0, 2, 4, 5, 6, 10)      # summed in double on both sides; column 3 (n) is exact
REL_DOUBLE = 1e-9                      # <= 33 024 summands per sum at unit roundoff 1.1e-16: <= 4e-12 relative; the rest is margin
PSNR_ABS = 1e-9                        # dB


@functools.lru_cache(maxsize=None)
def inputs(family, H, W):
    """(image[3,H,W], gt[3,H,W], depth[H,W], gt_depth[H,W]) float32 on the CPU; computed once, never written to."""
    out6, gt, ref = lr.make_inputs(family, H, W)
    return out6[:3].contiguous(), gt, out6[3].contiguous(), ref


@functools.lru_cache(maxsize=None)
def reference(family, H, W):
    """image_metrics_host on the CPU copy: the reference of the GPU test."""
    from mm3dgs_slam_amd.eval_utils import image_metrics_host
    return image_metrics_host(*inputs(family, H, W))


def statement(image, gt, depth=None, gt_depth=None):
    """The sixteen values in numpy float64, from the formulas of include/mm3dgs.h."""
    x, g = image.numpy().astype(np.float64), gt.numpy().astype(np.float64)
    _, H, W = x.shape
    w = np.array(lr.gauss_window(), dtype=np.float64)

    def blur(a):
        p = np.pad(a, ((0, 0), (5, 5), (5, 5)))
        h = sum(w[k] * p[:, :, k:k + W] for k in range(11))
        return sum(w[k] * h[:, k:k + H, :] for k in range(11))

    row = np.zeros(16)
    mse = ((x - g) ** 2).reshape(3, -1).sum(1) / (H * W)
    with np.errstate(divide="ignore"):
        row[0] = np.mean(20.0 * np.log10(1.0 / np.sqrt(mse)))
    row[4:7] = mse
    m1, m2 = blur(x), blur(g)
    s1, s2, s12 = blur(x * x) - m1 * m1, blur(g * g) - m2 * m2, blur(x * g) - m1 * m2
    smap = (2 * m1 * m2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2) / ((m1 * m1 + m2 * m2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    row[1] = smap.sum() / (3 * H * W)
    row[7:10] = smap.reshape(3, -1).sum(1) / (H * W)
    row[2] = row[10] = math.nan
    if depth is not None:
        gd = gt_depth.numpy()
        assert gd.dtype == np.float32
        valid = (gd > np.float32(0)) & (gd < np.float32(np.inf))
        n = int(valid.sum())
        row[3] = n
        if n:
            d = np.abs(depth.numpy().astype(np.float64) - gd.astype(np.float64))[valid]
            row[2], row[10] = d.sum() / n, math.sqrt((d * d).sum() / n)
    return row


def ssim_maps(image, gt, dtype):
    """[3,H,W]: the SSIM map as mm3dgs_slam_amd.loss_utils.ssim evaluates it (grouped 11x11 convolutions), in `dtype`."""
    w1 = torch.tensor(lr.gauss_window(), dtype=torch.float32)
    w2 = (w1[:, None] @ w1[None, :]).to(dtype).expand(3, 1, 11, 11).contiguous()
    x, g = image.to(dtype), gt.to(dtype)
    blur = lambda t: F.conv2d(t[None], w2, padding=5, groups=3)[0]
    m1, m2 = blur(x), blur(g)
    s1, s2, s12 = blur(x * x) - m1 * m1, blur(g * g) - m2 * m2, blur(x * g) - m1 * m2
    return ((2 * m1 * m2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((m1 * m1 + m2 * m2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))


@functools.lru_cache(maxsize=None)
def e32(family, H, W):
    """(E32 of column 1, [E32 of columns 7, 8, 9]): the mean over the pixels of |smap_float32 - smap_float64|."""
    image, gt, _, _ = inputs(family, H, W)
    d = (ssim_maps(image, gt, torch.float32).double() - ssim_maps(image, gt, torch.float64)).abs()
    return float(d.mean()), [float(d[c].mean()) for c in range(3)]


def ssim_bound(e):
    return lr.FACTOR * e + lr.ulp32(1.0)


def planted_gt_depth(H=17, W=33):
    """The gt_depth of inputs("random", H, W) with 0.0, -0.0, 1e-30, NaN, +inf and -1 as its ONLY entries that differ from 2.5 outside
    the first row, which holds them: of the six only 1e-30 counts."""
    gd = torch.full((H, W), 2.5)
    gd[0, :6] = torch.tensor([0.0, -0.0, 1e-30, float("nan"), float("inf"), -1.0])
    return gd


def degenerate_cases(H=17, W=33):
    """name -> (image, gt, depth or None, gt_depth or None) on the CPU."""
    image, gt, depth, gt_depth = inputs("random", H, W)
    only = torch.zeros(H, W)
    only[0, :6] = torch.tensor([0.0, -0.0, 1e-30, float("nan"), float("inf"), -1.0])
    return {
        "same": (image, image.clone(), depth, gt_depth),
        "no_valid": (image, gt, depth, torch.tensor([0.0, -0.0, float("nan"), float("inf"), -1.0, -float("inf")]).repeat(H * W)[:H * W].reshape(H, W).contiguous()),
        "no_depth": (image, gt, None, None),
        "planted": (image, gt, depth, planted_gt_depth(H, W)),
        "only_tiny": (image, gt, depth, only),
    }
