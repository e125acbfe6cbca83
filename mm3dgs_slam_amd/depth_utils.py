"""Per-frame alignment of a monocular depth estimate to the map (reference ``slam/SLAM.py:411-448`` with
``utils/depth_utils.py:44-99``): when the configuration has no sensor depth (``use_gt_depth: false`` -- what ``configs/TUM.yml:8``
ships), every frame renders the map once at the tracked pose (no gradients) and fits ``scale * est + shift`` to the INVERSE rendered
depth by least squares over { silhouette > 0.99, est > 1e-6 }; ``1 / (scale * est + shift)`` is the depth the mapper seeds from and the
target of its Pearson term.  The monocular network itself (MiDaS, a download) is out of scope: ``est`` is an input.

The reference gathers the valid pixels (``torch.where`` -> a host synchronisation) and solves the 2 x 2 normal equations with
``torch.inverse``; here the masked-out pixels stay in place as zero rows of ``H`` (the normal equations are the same sums), the 2 x 2
inverse is written out, and nothing leaves the device.

``align_depth_device`` is the same fit and its application as two HIP launches (``mm3dgs_align_depth``, csrc/align.hip) with the fit
record -- scale, shift, whether the system had a fit, the pixel count and the four sums -- as a device tensor; the opt-in key
``depth_align_on_device`` routes ``scale_depth_estimate`` through it."""
from __future__ import annotations

import torch


def get_scale_shift_LS(est_depth, render_depth, mask=None, return_ok=False):
    """(scale, shift) with ``scale * est + shift ~ 1 / render_depth`` over the pixels where ``mask`` holds and the inverse rendered
    depth is positive (utils/depth_utils.py:44-96, ``num_samples == -1``).  Returns two 1-element tensors on the inputs' device; with
    ``return_ok`` also a 0-dim bool tensor: whether the system had a fit (see below)."""
    inv = 1.0 / render_depth                      # (the estimate is an inverse depth)
    if mask is not None:
        inv = torch.where(mask, inv, torch.zeros_like(inv))
    valid = inv > 0
    # normal equations H^T H x = H^T z with H = [est, 1] over the valid pixels, as five masked sums (a [2, HW] x [HW, 2] product is a
    # skinny GEMM: 0.56 ms per call at 640x480 through hipBLASLt -- measured in the first round-4 trace -- against ~10 us per reduction)
    # (torch.where, not a product with the 0/1 mask: a NaN / inf of the network at a masked-out pixel must not reach the sums -- the
    #  reference gathers the valid pixels only)
    # The five sums and the 2 x 2 solve run in float64: det = a00 a11 - a01^2 cancels to ~1e-7 of its terms for a nearly
    # constant estimate, which is float32's own rounding -- a float32 det there is noise that passes any relative threshold.
    h = torch.where(valid, est_depth, torch.zeros_like(est_depth)).double()
    z = torch.where(valid, inv, torch.zeros_like(inv)).double()
    a00, a01, a11 = (h * h).sum(), h.sum(), valid.sum().double()
    b0, b1 = (h * z).sum(), z.sum()
    det = a00 * a11 - a01 * a01
    # a singular system (fewer than two valid pixels, or a constant estimate over them: the reference's torch.inverse raises there) has
    # no fit: the identity (scale 1, shift 0) is returned instead of NaN / inf that would silently flow into seeding and the Pearson
    # target -- decided on the device (no host read-back).  det / (a00 a11) = the estimate's variance over its mean square: below 1e-9
    # (a spread of 3e-5 of the mean) the inputs' own float32 rounding decides the fit.
    ok = (a11 >= 2) & (det.abs() > 1e-9 * (a00 * a11).abs().clamp_min(1e-300)) & torch.isfinite(det)
    safe = torch.where(ok, det, torch.ones_like(det))
    scale = torch.where(ok, (a11 * b0 - a01 * b1) / safe, torch.ones_like(det)).to(est_depth.dtype).reshape(1)
    shift = torch.where(ok, (a00 * b1 - a01 * b0) / safe, torch.zeros_like(det)).to(est_depth.dtype).reshape(1)
    return (scale, shift, ok) if return_ok else (scale, shift)


_WORK = {}      # (H, W, device) -> the kernels' row buffer (contents irrelevant between calls; calls on one stream are ordered)


def align_depth_device(est, depth, sil=None, sil_min=0.99, est_min=1e-6):
    """``(1 / (scale * est + shift), fit)`` with the least-squares fit of ``scale * est + shift`` to ``1 / depth`` over
    { sil > sil_min, est > est_min, 0 < 1 / depth < inf } -- without ``sil`` over { depth > 0, 1 / depth < inf } -- by mm3dgs_align_depth:
    two launches on the current stream, nothing read back.  ``fit``: 16 float64 on the device = scale, shift (the float32 values), ok
    (0 / 1), the number of valid pixels, a00, a01, b0, b1, zeros; not ok (fewer than two valid pixels, an estimate constant over them) is
    the identity fit.  One difference from ``get_scale_shift_LS``: a pixel whose depth is so small that ``1 / depth`` overflows is left
    out here and makes the host path return NaN.  The scaled estimate is a fresh tensor on every call (keyframes keep it)."""
    from . import _lib
    from .rasterizer import _stream
    if not (est.is_cuda and depth.is_cuda and (sil is None or sil.is_cuda)):
        raise RuntimeError("align_depth_device needs device tensors (the host path is get_scale_shift_LS)")
    H, W = int(est.shape[-2]), int(est.shape[-1])
    if est.numel() != H * W or depth.numel() != H * W or (sil is not None and sil.numel() != H * W):
        raise ValueError(f"align_depth_device: est, depth and sil are [H,W] images of one size; got {tuple(est.shape)}, {tuple(depth.shape)}"
                         + (f", {tuple(sil.shape)}" if sil is not None else ""))
    est_c, depth_c = est.detach().float().contiguous(), depth.detach().float().contiguous()
    sil_c = None if sil is None else sil.detach().float().contiguous()
    lib = _lib.load()
    key = (H, W, est_c.device)
    work = _WORK.get(key)
    if work is None:
        work = _WORK[key] = torch.empty(int(lib.mm3dgs_align_depth_work_bytes(H, W)) // 8, dtype=torch.float64, device=est_c.device)
    fit = torch.empty(16, dtype=torch.float64, device=est_c.device)
    out = torch.empty_like(est_c)
    P = _lib.ptr
    _lib.check(lib.mm3dgs_align_depth(H, W, P(est_c), P(depth_c), P(sil_c), float(sil_min), float(est_min), P(work), P(fit), P(out), _stream()))
    return out, fit


def scale_depth_estimate(cfg, idx, est_depth, gt_depth, render_depth_sil, resumed=False, on_device=False, return_fit=False):
    """``est_depth_scaled`` of slam/SLAM.py:411-448.  render_depth_sil: a callable returning (depth, silhouette) of the map at the
    frame's estimated pose (only called for idx > 0, or on a resumed run).  ``on_device`` (the key ``depth_align_on_device``): the two
    fits run through ``align_depth_device`` when the tensors are on the GPU.  ``return_fit``: also the fit record of that path (None
    where no fit ran on the device)."""
    if on_device and est_depth.is_cuda:
        fit = None
        with torch.no_grad():
            if idx == 0 and not resumed:
                if str(cfg.get("dataset", "")).lower() == "utmm":
                    out, fit = align_depth_device(est_depth, gt_depth)
                else:
                    out = 1.0 / (est_depth + 0.001) * float(cfg["cam"]["png_depth_scale"]) / 10.0
            else:
                depth, sil = render_depth_sil()
                out, fit = align_depth_device(est_depth, depth, sil)
        return (out, fit) if return_fit else out
    if return_fit:
        return scale_depth_estimate(cfg, idx, est_depth, gt_depth, render_depth_sil, resumed), None
    with torch.no_grad():
        if idx == 0 and not resumed:
            if str(cfg.get("dataset", "")).lower() == "utmm":
                # "until visual-inertial initialization is implemented": the first estimate is fitted to the sensor depth
                scale, shift = get_scale_shift_LS(est_depth, gt_depth, gt_depth > 0)
                return 1.0 / (scale * est_depth + shift)
            return 1.0 / (est_depth + 0.001) * float(cfg["cam"]["png_depth_scale"]) / 10.0      # "arbitrarily scale the first frame"
        depth, sil = render_depth_sil()
        mask = (sil > 0.99) & (est_depth > 1e-6)
        scale, shift = get_scale_shift_LS(est_depth, depth, mask)
        return 1.0 / (scale * est_depth + shift)
