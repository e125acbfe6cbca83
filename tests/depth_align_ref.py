"""Float64 numpy restatement of the depth alignment (mm3dgs_align_depth, csrc/align.hip): pixel rule, sums, solve and apply.  It is the
yardstick of tests/test_depth_align.py (CPU) and tests/test_gpu_depth_align.py, together with the seeded inputs, the shape list and the
derived bars both files use.

Pixel rule: with a silhouette a pixel is considered iff sil > sil_min and est > est_min (strict, float32); without one iff depth > 0.
A considered pixel is valid iff 0 < z < +inf, z = the correctly rounded float32 quotient 1 / depth widened to double (numpy's float32
division is correctly rounded).  A depth so small that 1 / depth overflows is therefore excluded -- the one deliberate difference from
depth_utils.get_scale_shift_LS, which sums that pixel and returns NaN.  Sums over the valid pixels in double, h = est:
a00 = sum h^2, a01 = sum h, n = sum 1, b0 = sum h z, b1 = sum z; det = a00 n - a01^2;
ok = n >= 2 and |det| > 1e-9 max(|a00 n|, 1e-300) and isfinite(det); scale = (n b0 - a01 b1) / det, shift = (a00 b1 - a01 b0) / det, each
rounded once to float32; not ok: scale 1, shift 0.  Apply: 1 / (scale * est + shift) in float32 with the float32 scale and shift, an
unfused multiply and add and a correctly rounded division (numpy's float32 operators are exactly that)."""
import numpy as np

SIL_MIN, EST_MIN = np.float32(0.99), np.float32(1e-6)

# the launch constants of csrc/align.hip: 256 lanes per workgroup, at most 256 workgroups -- one grid sweep covers 65536 pixels
WG, MAX_ROWS = 256, 256
BEYOND_ONE_SWEEP = (1, WG * MAX_ROWS + 1)          # 65537 pixels (a prime): every lane one pixel, lane 0 of workgroup 0 a second one

# the smallest shapes at which the kernels can go wrong: n = 1 (identity, ok 0) | n = 2 (the boundary of n >= 2) | a short wave | one wave
# | a wave plus one lane | one workgroup | ragged tail, odd H W | one pixel beyond a full grid sweep | the SLAM frame, once
SHAPES = [(1, 1), (1, 2), (7, 9), (8, 8), (5, 13), (16, 16), (17, 23), BEYOND_ONE_SWEEP, (480, 640)]
ODD_SHAPES = [(7, 9), (5, 13), (17, 23)]           # depth and silhouette travel as planes 3 and 4 of one [6,H,W] image there


def make_inputs(H, W, seed=0):
    """depth = 1 + 3 u, est = 700 / (depth (1 + 0.02 g) + 0.4) + 40, silhouette mostly above 0.99 (the first two pixels always): well
    conditioned (the coefficient of variation of est is above 0.1) and every summed term is positive.  float32 [H,W] each."""
    rng = np.random.default_rng(1000 * seed + 31 * H + W)
    depth = (1.0 + 3.0 * rng.random((H, W))).astype(np.float32)
    est = (700.0 / (depth.astype(np.float64) * (1.0 + 0.02 * rng.standard_normal((H, W))) + 0.4) + 40.0).astype(np.float32)
    u = rng.random((H, W))
    sil = np.where(u < 0.8, 1.0, u).astype(np.float32)
    sil.reshape(-1)[:2] = 1.0
    return est, depth, sil


def valid_mask(est, depth, sil=None, sil_min=SIL_MIN, est_min=EST_MIN):
    est, depth = np.asarray(est, np.float32), np.asarray(depth, np.float32)
    with np.errstate(all="ignore"):
        zf = (np.float32(1.0) / depth).astype(np.float32)
        if sil is not None:
            considered = (np.asarray(sil, np.float32) > np.float32(sil_min)) & (est > np.float32(est_min))
        else:
            considered = depth > 0
        return considered & (zf > 0) & np.isfinite(zf), zf


def align_ref(est, depth, sil=None, sil_min=SIL_MIN, est_min=EST_MIN):
    """dict: scale, shift (np.float32), ok (bool), n, a00, a01, b0, b1 (float), fit (the 16-double record of the C entry point)."""
    valid, zf = valid_mask(est, depth, sil, sil_min, est_min)
    h = np.asarray(est, np.float32)[valid].astype(np.float64)
    z = zf[valid].astype(np.float64)
    with np.errstate(all="ignore"):
        a00, a01, n, b0, b1 = float((h * h).sum()), float(h.sum()), float(valid.sum()), float((h * z).sum()), float(z.sum())
        a00, a01, n, b0, b1 = (np.float64(v) for v in (a00, a01, n, b0, b1))
        det = a00 * n - a01 * a01
        ok = bool(n >= 2 and abs(det) > 1e-9 * max(abs(a00 * n), 1e-300) and np.isfinite(det))
        scale = np.float32((n * b0 - a01 * b1) / det) if ok else np.float32(1.0)
        shift = np.float32((a00 * b1 - a01 * b0) / det) if ok else np.float32(0.0)
    fit = np.zeros(16)
    fit[:8] = [float(scale), float(shift), float(ok), n, a00, a01, b0, b1]
    return {"scale": scale, "shift": shift, "ok": ok, "n": float(n), "a00": float(a00), "a01": float(a01), "b0": float(b0), "b1": float(b1),
            "fit": fit}


def apply_ref(est, scale, shift):
    est = np.asarray(est, np.float32)
    with np.errstate(all="ignore"):
        return (np.float32(1.0) / (np.float32(scale) * est + np.float32(shift))).astype(np.float32)


# ---- bars (derived, not tuned) ----------------------------------------------------------------------------------------------------
def bar_sums(n, ref):
    """A: every term of a00, a01, b0, b1 is positive on the seeded inputs and a product of two float32 values is exact in double, so ANY
    summation order of n terms is within (n - 1) 2^-53 of the exact sum, relatively; two orders (device, restatement) within 2 n 2^-53."""
    return 2.0 * n * 2.0 ** -53 * abs(ref)


def bar_scale(scale):
    """B: one float32 rounding (2^-24 relative) of a double quotient whose own error is bar A times the system's conditioning (<= ~100 on
    these inputs, ~1e-11 in all) on each side: at most a float32 ulp apart (2^-23), doubled."""
    return 4.0 * 2.0 ** -24 * abs(float(scale))


def bar_shift(scale, shift, mean_abs_est):
    """B for the shift = mean z - scale mean est: its rounding is relative to the larger of the two terms it cancels."""
    return 4.0 * 2.0 ** -24 * (abs(float(shift)) + abs(float(scale)) * float(mean_abs_est))


def ulp_diff(a, ref):
    """|a - ref| in units of ref's float32 spacing (NaN where either is not finite)."""
    a, ref = np.asarray(a, np.float32), np.asarray(ref, np.float32)
    with np.errstate(all="ignore"):
        return np.abs(a.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
