"""Host reference of the image losses behind `Mm3dgsLossConfig` (include/mm3dgs.h), written from that header and from the reference's
formulas (utils/loss_utils.py:43-68,95-154, slam/tracker.py:104-155, slam/mapper.py:836-873) -- not from the kernels: plain torch on
the CPU, float64 by default, the gradient image from autograd of the scalar.  `dtype=torch.float32` evaluates the very same
statements in float32: the yardstick that says how far two equally valid float32 evaluations of these losses lie apart.

Also the input generators and the error measures that tests/test_loss_ref.py (CPU) and tests/test_gpu_loss.py (GPU) share.

Channel layout of `out6`: 0..2 RGB, 3 depth (alpha-weighted z), 4 silhouette, 5 depth^2.  No loss term reaches planes 4 and 5."""
import math

import numpy as np
import torch
import torch.nn.functional as F

FIELDS = ("w_l1", "w_ssim", "w_pearson", "l1_mask", "pearson_mask", "pearson_invert", "sil_thr", "window", "w_depth_l1", "depth_l1_mask",
          "l1_sum")
TILE = 16         # the kernels' tile edge (only the error REGIONS below know about it; the reference itself has no tiles)
BAND = 5          # half width of the 11-tap window: the band of pixels whose window reaches the zero padding


def gauss_window():
    """utils/loss_utils.py:95-98: the normalised 11-tap Gaussian, sigma 1.5, as float32 values."""
    g = torch.tensor([math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)])
    return [float(v) for v in (g / g.sum()).float()]


def cfg_fields(w_l1=0.0, w_ssim=0.0, w_pearson=0.0, l1_mask=0, pearson_mask=0, pearson_invert=0, sil_thr=0.5, window=None, w_depth_l1=0.0,
               depth_l1_mask=0, l1_sum=0):
    return dict(w_l1=w_l1, w_ssim=w_ssim, w_pearson=w_pearson, l1_mask=l1_mask, pearson_mask=pearson_mask, pearson_invert=pearson_invert,
                sil_thr=sil_thr, window=gauss_window() if window is None else list(window), w_depth_l1=w_depth_l1,
                depth_l1_mask=depth_l1_mask, l1_sum=l1_sum)


def _get(cfg, name):
    """A field of a dict of FIELDS or of a struct with those attributes (the ctypes Mm3dgsLossConfig)."""
    v = cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)
    if name == "window":
        return [float(np.float32(w)) for w in v]
    if name in ("w_l1", "w_ssim", "w_pearson", "sil_thr", "w_depth_l1"):
        return float(np.float32(v))       # the struct holds float32: the float32 value widened, so no mask differs by rounding
    return int(v)


def _corr(a, b):
    """Pearson correlation, the textbook definition torchmetrics' pearson_corrcoef computes (utils/loss_utils.py:11)."""
    a = a - a.mean()
    b = b - b.mean()
    return (a * b).sum() / torch.sqrt((a * a).sum() * (b * b).sum())


def _ssim(x, y, window, dtype):
    """utils/loss_utils.py:95-154: 11x11 window = outer product of the 1-D window held in float32 (:101-103), zero padding 5,
    C1 = 0.01^2, C2 = 0.03^2, mean over 3 H W."""
    w1 = torch.tensor(window, dtype=torch.float32)
    w2 = (w1[:, None] @ w1[None, :]).to(dtype).expand(3, 1, 11, 11).contiguous()

    def blur(t):
        return F.conv2d(t[None], w2, padding=5, groups=3)[0]

    mu1, mu2 = blur(x), blur(y)
    s11 = blur(x * x) - mu1 * mu1
    s22 = blur(y * y) - mu2 * mu2
    s12 = blur(x * y) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))).mean()


def loss_ref(cfg, out6, gt, ref=None, dtype=torch.float64):
    """(loss4, dL[6, H, W]) of `cfg` (a dict of FIELDS or an Mm3dgsLossConfig) on float32 tensors out6[6, H, W], gt[3, H, W] and
    ref[H, W] or None, evaluated in `dtype` on the CPU.  loss4 = {total, colour l1, 1 - ssim, 1 - rho or the depth-L1 term}."""
    c = {k: _get(cfg, k) for k in FIELDS}
    if (c["w_pearson"] != 0.0 or c["w_depth_l1"] != 0.0 or (c["l1_mask"] & 2)) and ref is None:
        raise ValueError("this configuration needs a reference depth")
    if c["w_pearson"] != 0.0 and c["w_depth_l1"] != 0.0:
        raise ValueError("the depth-L1 and Pearson terms are exclusive")
    x = out6.detach().cpu().to(dtype).clone().requires_grad_(True)
    g = gt.detach().cpu().to(dtype)
    r = ref.detach().cpu().to(dtype) if ref is not None else None
    image, depth, sil = x[:3], x[3], x[4]
    zero = torch.zeros((), dtype=dtype)
    smask = sil.detach() > c["sil_thr"]

    def mask(bits):      # bit0 silhouette > sil_thr, bit1 ref > 0, 0: all pixels
        m = torch.ones_like(smask)
        if bits & 1:
            m = m & smask
        if bits & 2:
            m = m & (r > 0)
        return m

    # colour L1 over l1_mask: mean over the 3 n masked elements, or their sum (l1_sum)
    m = mask(c["l1_mask"])
    d = (image - g).abs()[:, m]
    if c["l1_sum"]:
        l1 = d.sum()
    elif int(m.sum()) == 0:
        l1 = zero            # empty L1 mask: term 0, gradient 0  (loss_pixel.h loss_scalars / loss_l1_scale: `n_l1 > 0.0 ? ... : 0`)
    else:
        l1 = d.mean()
    ss = 1.0 - _ssim(image, g, c["window"], dtype) if c["w_ssim"] != 0.0 else zero
    lp = zero
    if c["w_pearson"] != 0.0:
        m = mask(c["pearson_mask"])
        if int(m.sum()) > 1:
            rd, e = depth[m], r[m]
            if c["pearson_invert"]:      # utils/loss_utils.py:53-57
                lp = torch.minimum(1 - _corr(-e, rd), 1 - _corr(1 / (e + 200.0), rd))
            else:
                lp = 1 - _corr(e, rd)
        # else: at most one masked pixel, the term is off  (loss.hip pearson_scalars: `pearson_on && n > 1.0`)
    dl = zero
    if c["w_depth_l1"] != 0.0:
        m = mask(c["depth_l1_mask"])
        dd = (r - depth).abs()[m]
        if c["l1_sum"]:
            dl = dd.sum()
        elif int(m.sum()) > 0:
            dl = dd.mean()
        # else: empty depth mask, term 0  (loss.hip variant_scalars: `n_d > 0.0 ? ... : 0.0`)
    total = c["w_l1"] * l1 + c["w_ssim"] * ss + c["w_pearson"] * lp + c["w_depth_l1"] * dl
    # loss4[3] is the depth-L1 term when w_depth_l1 != 0, else 1 - rho  (loss.hip variant_scalars: `cfg.w_depth != 0.f ? dl : loss_p`)
    loss4 = torch.stack([t.detach() * 1.0 for t in (total, l1, ss, dl if c["w_depth_l1"] != 0.0 else lp)])
    dL = torch.autograd.grad(total, x)[0] if total.requires_grad else torch.zeros_like(x)
    return loss4, dL.detach()


# ---- input generators -------------------------------------------------------------------------------------------------------------
SIL_THRS = (0.99, 0.5)      # the two thresholds the configurations of the tests use
MIN_DIFF = 1e-3             # no colour element has 0 < |out - gt| < MIN_DIFF: the sign of out - gt is never a matter of rounding


def hole_rect(H, W):
    """The rectangular hole of zeros in the reference depth: rows H/4 .. H/2, columns W/4 .. 3W/4."""
    return H // 4, H // 2, W // 4, (3 * W) // 4


def _common_planes(H, W, gen):
    depth = 1.0 + 2.0 * torch.rand(H, W, generator=gen)
    sil = (0.85 + 0.2 * torch.rand(H, W, generator=gen)).clamp(max=1.0)      # 30 % above 0.99 (25 % exactly 1), all above 0.5
    ref = 1.1 * depth + (0.1 * torch.randn(H, W, generator=gen)).abs()
    y0, y1, x0, x1 = hole_rect(H, W)
    ref[y0:y1, x0:x1] = 0.0
    return depth, sil, ref


def planted_pixels(H, W, seed):
    """Flat indices of the 12 planted pixels (distinct, anywhere in the image); none when the image has fewer than 24 pixels."""
    if H * W < 24:
        return []
    return torch.randperm(H * W, generator=torch.Generator().manual_seed(1000 + seed))[:12].tolist()


def make_inputs(family, H, W, seed=0, plant=True):
    """(out6[6, H, W], gt[3, H, W], ref[H, W]) float32.
    random: rgb uniform, gt = clamp(rgb + 0.2 randn), depth in [1, 3], ref = 1.1 depth + |noise| with a rectangular hole of zeros.
    flat:   colours piecewise constant on 8x8 blocks (dark blocks included) with noise of 1e-3, gt offset per block by 0.01 .. 0.05:
            E[x^2] - mu^2 is then ~1e-6 against C2 = 9e-4, where an approximate SSIM shows.
    plant:  on top, 12 pixels with  sil == float32(thr) and its two float32 neighbours, for both thresholds of SIL_THRS;
            ref == 0.0, -0.0 and 1e-30;  out == gt exactly in one channel (three pixels, one per channel)."""
    gen = torch.Generator().manual_seed(seed * 7919 + H * 131 + W)
    if family == "random":
        rgb = 0.05 + 0.9 * torch.rand(3, H, W, generator=gen)
        n = 0.2 * torch.randn(3, H, W, generator=gen)
        n = torch.where(n < 0, -1.0, 1.0) * n.abs().clamp(min=2 * MIN_DIFF)
        gt = (rgb + n).clamp(0.0, 1.0)
    elif family == "flat":
        bh, bw = (H + 7) // 8, (W + 7) // 8
        levels = torch.tensor([0.004, 0.02, 0.3, 0.7, 0.95])
        base = levels[torch.randint(0, 5, (3, bh, bw), generator=gen)]
        delta = torch.where(base < 0.5, 1.0, -1.0) * (0.01 + 0.04 * torch.rand(3, bh, bw, generator=gen))

        def up(t):
            return t.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W]

        rgb = up(base) + 1e-3 * (2 * torch.rand(3, H, W, generator=gen) - 1)
        gt = up(base + delta) + 1e-3 * (2 * torch.rand(3, H, W, generator=gen) - 1)
    else:
        raise ValueError(family)
    depth, sil, ref = _common_planes(H, W, gen)
    if plant:
        px = planted_pixels(H, W, seed)
        if px:
            sil_f, ref_f, rgb_f, gt_f = sil.view(-1), ref.view(-1), rgb.view(3, -1), gt.view(3, -1)
            k = 0
            for thr in SIL_THRS:
                t = np.float32(thr)
                for v in (t, np.nextafter(t, np.float32(2)), np.nextafter(t, np.float32(-2))):
                    sil_f[px[k]] = float(v)
                    k += 1
            for v in (0.0, -0.0, 1e-30):
                ref_f[px[k]] = v
                k += 1
            for ch in range(3):
                gt_f[ch, px[k]] = rgb_f[ch, px[k]]
                k += 1
    out6 = torch.cat([rgb, depth[None], sil[None], (depth * depth)[None]], 0).float().contiguous()
    return out6, gt.float().contiguous(), ref.float().contiguous()


# ---- error measures ---------------------------------------------------------------------------------------------------------------
def regions(H, W):
    """Three disjoint pixel sets: the 5-pixel image border band (window in the zero padding), the other pixels of partial 16x16
    tiles, the interior.  Empty ones are left out."""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    border = (yy < BAND) | (yy >= H - BAND) | (xx < BAND) | (xx >= W - BAND)
    partial = ((xx // TILE + 1) * TILE > W) | ((yy // TILE + 1) * TILE > H)
    reg = {"border": border, "partial": partial & ~border, "interior": ~partial & ~border}
    return {k: v for k, v in reg.items() if bool(v.any())}


def ulp32(v):
    """One float32 ulp at magnitude v."""
    return float(np.spacing(np.float32(abs(v))))


def plane_errors(a, ref, H, W):
    """Error measures of a gradient plane (or a stack of planes [..., H, W]) `a` against the float64 `ref`: rel_l2 and max|delta| / max|ref| over each region.
    A non-finite difference gives inf."""
    a, ref = a.detach().cpu().double(), ref.double()
    delta = a - ref
    if not bool(torch.isfinite(delta).all()):
        return {k: float("inf") for k in ["rel_l2"] + ["max_" + r for r in regions(H, W)]}
    scale, norm = float(ref.abs().max()), float(ref.norm())
    e = {"rel_l2": float(delta.norm()) / norm}
    for name, m in regions(H, W).items():
        e["max_" + name] = float(delta[..., m].abs().max()) / scale
    return e


def plane_floors(ref, H, W):
    """The absolute floor of the bound, one float32 ulp of the plane's largest magnitude per pixel, in the units of plane_errors."""
    scale, norm = float(ref.abs().max()), float(ref.double().norm())
    u = ulp32(scale)
    f = {"rel_l2": u * math.sqrt(ref.numel()) / norm}
    for name in regions(H, W):
        f["max_" + name] = u / scale
    return f


FACTOR = 8.0     # kernel error <= FACTOR * (float32 restatement's error) + floor: other, equally valid float32 summation orders + v_rcp_f32


def bound(e32, floor, factor=FACTOR):
    return factor * e32 + floor


# ---- the cases of tests/test_gpu_loss.py (their inputs are checked on the CPU by tests/test_loss_ref.py) ---------------------------
SHAPES = [(1, 1), (5, 7), (11, 48), (16, 16), (17, 33), (37, 21), (48, 64), (80, 208), (16, 2064), (112, 112)]
FAMILIES = ("random", "flat")
# name -> (fields, takes a reference depth).  The first six are the kinds of test_fused_loss_matches_torch_losses.
CONFIGS = {
    "track": (cfg_fields(w_l1=1.0, l1_mask=1, pearson_invert=1, sil_thr=0.99), False),
    "track_pearson": (cfg_fields(w_l1=1.0, w_pearson=0.05, l1_mask=1, pearson_mask=3, pearson_invert=1, sil_thr=0.99), True),
    "map": (cfg_fields(w_l1=0.8, w_ssim=0.2, w_pearson=0.05, pearson_mask=2), True),
    "map_estdepth": (cfg_fields(w_l1=0.8, w_ssim=0.2, w_pearson=0.05), True),
    "splatam_track": (cfg_fields(w_l1=0.5, l1_mask=3, sil_thr=0.99, w_depth_l1=1.0, depth_l1_mask=3, l1_sum=1), True),
    "splatam_map": (cfg_fields(w_l1=0.4, w_ssim=0.1, w_depth_l1=1.0, depth_l1_mask=2), True),
    "l1_mask2": (cfg_fields(w_l1=1.0, l1_mask=2), True),
    "ssim_only": (cfg_fields(w_ssim=1.0), False),
    "pearson": (cfg_fields(w_pearson=1.0, pearson_mask=2), True),
    "pearson_invert": (cfg_fields(w_pearson=1.0, pearson_mask=3, pearson_invert=1, sil_thr=0.99), True),
    "no_loss4": (cfg_fields(w_l1=0.8, w_ssim=0.2, w_pearson=0.05, pearson_mask=2), True),      # called with loss4 = NULL
}


def pearson_moments(cfg, out6, ref):
    """n and, for the rendered depth and each target the configuration correlates it with, (centred sum of squares, raw sum of
    squares) in float64: how much of the raw moment the covariance form `sxx - sx^2 / n` has to cancel."""
    c = {k: _get(cfg, k) for k in FIELDS}
    m = torch.ones(out6.shape[1:], dtype=torch.bool)
    if c["pearson_mask"] & 1:
        m = m & (out6[4] > c["sil_thr"])
    if c["pearson_mask"] & 2:
        m = m & (ref > 0)
    x, e = out6[3][m].double(), ref[m].double()
    targets = {"depth": x}
    if c["pearson_invert"]:
        targets["-ref"], targets["1/(ref+200)"] = -e, 1 / (e + 200.0)
    else:
        targets["ref"] = e
    n = int(m.sum())
    return n, {k: (float(((v - v.mean()) ** 2).sum()), float((v * v).sum())) for k, v in targets.items()} if n > 1 else {}
