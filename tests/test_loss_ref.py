"""The float64 host reference of the image losses (tests/loss_ref.py) checked on its own, without a GPU: it reproduces the upstream
project's numbers (fixture G8), equals `mm3dgs_slam_amd.loss_utils` evaluated in float64, returns exact zeros in the degenerate
cases the kernels promise zeros for, and the inputs it generates for tests/test_gpu_loss.py are well conditioned."""
import os

import numpy as np
import pytest
import torch

from tests import loss_ref as lr


@pytest.fixture(scope="module")
def g8():
    d = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(os.path.dirname(__file__), "golden", "g8_loss.npz")).items()}
    d["out6"] = torch.cat([d["img"], d["depth"][None], d["sil"][None], (d["depth"] ** 2)[None]], 0).contiguous()
    return d


G8_CASES = {      # fixture value key, fixture gradient key, configuration, the fixture's value as a function of loss4
    "l1": ("d_l1", lr.cfg_fields(w_l1=1.0), lambda l: l[0]),
    "l1_masked": ("d_l1_masked", lr.cfg_fields(w_l1=1.0, l1_mask=1, sil_thr=0.99), lambda l: l[0]),
    "ssim": ("d_ssim", lr.cfg_fields(w_ssim=-1.0), lambda l: 1.0 - l[2]),      # total = -(1 - ssim): its gradient is d ssim
    "map_photo": ("d_map_photo", lr.cfg_fields(w_l1=0.8, w_ssim=0.2), lambda l: l[0]),
}


@pytest.mark.parametrize("key", list(G8_CASES))
def test_reference_reproduces_fixture_g8_values_and_gradients(g8, key):
    """The fixture holds a float32 evaluation (the upstream functions on float32 tensors, stored as float32).  Its distance from the
    exact value is that of a float32 evaluation, and this module has one to measure with: the float32 restatement.  Bound, per
    measure:  8 x |float32 restatement - float64 reference| + one float32 ulp of the largest magnitude (the fixture's storage).
    Measured (value |delta|; gradient rel_l2 / largest max-measure), bound in brackets:
      l1         2.8e-09 [3.0e-08]   7.5e-09 / 7.5e-09 [1.3e-07 / 1.3e-07]
      l1_masked  3.1e-09 [3.2e-08]   2.8e-08 / 2.8e-08 [3.7e-07 / 3.0e-07]
      ssim       5.2e-08 [4.7e-07]   4.6e-06 / 1.2e-05 [3.7e-05 / 9.5e-05]
      map_photo  4.3e-09 [4.9e-08]   3.0e-06 / 9.6e-06 [2.5e-05 / 7.5e-05]
    (the smooth fixture images have local variances near C2, so a float32 SSIM gradient carries ~5e-6, not the ~3e-7 of random images)"""
    gkey, cfg, value = G8_CASES[key]
    H, W = g8["sil"].shape
    l64, d64 = lr.loss_ref(cfg, g8["out6"], g8["gt"])
    l32, d32 = lr.loss_ref(cfg, g8["out6"], g8["gt"], dtype=torch.float32)
    v64, v32 = float(value(l64)), float(value(l32.double()))
    err, b = abs(float(g8[key]) - v64), lr.bound(abs(v32 - v64), lr.ulp32(v64))
    print(f"G8 {key}: value {err:.2e} bound {b:.2e}")
    assert err <= b
    e32, floor, e = lr.plane_errors(d32[:3], d64[:3], H, W), lr.plane_floors(d64[:3], H, W), lr.plane_errors(g8[gkey], d64[:3], H, W)
    for m in e:
        print(f"G8 {key}: {gkey} {m} {e[m]:.2e} bound {lr.bound(e32[m], floor[m]):.2e}")
        assert e[m] <= lr.bound(e32[m], floor[m]), (m, e[m], e32[m])
    assert float(d64[3:].abs().max()) == 0.0


@pytest.mark.parametrize("key,cfg", [
    ("pearson_track_gt", lr.cfg_fields(w_pearson=1.0, pearson_mask=3, pearson_invert=1, sil_thr=0.99)),
    ("pearson_map_gt", lr.cfg_fields(w_pearson=1.0, pearson_mask=2)),
    ("pearson_track_est", lr.cfg_fields(w_pearson=1.0, pearson_mask=1, pearson_invert=1, sil_thr=0.99)),
    ("pearson_map_est", lr.cfg_fields(w_pearson=1.0)),
])
def test_reference_reproduces_fixture_g8_pearson_values(g8, key, cfg):
    """These four are float64 in the fixture: scipy.stats.pearsonr on the widened arguments of the upstream pearson_loss.
    `map` (one target, ref itself): both sides float64 on the same numbers, 1e-12 relative.  `track` (min over -ref and
    1 / (ref + 200)): upstream forms 1 / (ref + 200) on float32 tensors BEFORE the widening, so the fixture carries that target's
    float32 rounding (6e-8 of a quantity that varies by ~1e-3 of its mean) -- the float32 yardstick again, 8 x |float32 restatement
    - float64 reference|.  The `est` pair correlates with ref.clamp_min(0.5).
    Measured: track_gt 0 [6.3e-07], map_gt 2.2e-16 [2.9e-14], track_est 2.2e-06 [1.8e-05], map_est 0 [3.7e-13]."""
    ref = g8["ref_depth"].clamp_min(0.5) if key.endswith("est") else g8["ref_depth"]
    l64, _ = lr.loss_ref(cfg, g8["out6"], g8["gt"], ref)
    err = abs(float(l64[3]) - float(g8[key]))
    if "track" in key:
        l32, _ = lr.loss_ref(cfg, g8["out6"], g8["gt"], ref, dtype=torch.float32)
        b = lr.bound(abs(float(l32[3]) - float(l64[3])), 0.0)
    else:
        b = 1e-12 * abs(float(g8[key]))
    print(f"G8 {key}: {err:.2e} bound {b:.2e}")
    assert err <= b
    assert float(l64[0]) == float(l64[3])


def _loss_utils_f64(kind, out6, gt, ref):
    """The six kinds of tests/test_gpu_fused.py::test_fused_loss_matches_torch_losses, written with loss_utils as that test writes them."""
    from mm3dgs_slam_amd.loss_utils import l1_loss, pearson_loss, ssim
    out = out6.double().requires_grad_(True)
    color, depth = gt.double(), ref.double()
    image, d, sil = out[:3], out[3], out[4]
    if kind == "splatam_track":
        mask = (depth > 0) & (sil > float(np.float32(0.99)))
        loss = (depth - d).abs()[mask].sum() + float(np.float32(0.5)) * (color - image).abs()[:, mask].sum()
        terms = ((color - image).abs()[:, mask].sum(), 0.0, (depth - d).abs()[mask].sum())
    elif kind == "splatam_map":
        w1, w2 = float(np.float32(0.4)), float(np.float32(0.1))
        terms = (l1_loss(image, color), 1.0 - ssim(image, color), (depth - d).abs()[depth > 0].mean())
        loss = terms[2] + w1 * terms[0] + w2 * terms[1]
    elif kind.startswith("track"):
        presence = sil > float(np.float32(0.99))
        terms = [l1_loss(image, color, presence), 0.0, 0.0]
        loss = terms[0]
        if kind == "track_pearson":
            terms[2] = pearson_loss(d, depth, mask=presence & (depth > 0), invert_estimate=True)
            loss = loss + float(np.float32(0.05)) * terms[2]
    else:
        terms = [l1_loss(image, color), 1.0 - ssim(image, color), None]
        terms[2] = pearson_loss(d, depth, mask=depth > 0 if kind == "map" else None, invert_estimate=False)
        loss = float(np.float32(0.8)) * terms[0] + float(np.float32(0.2)) * terms[1] + float(np.float32(0.05)) * terms[2]
    loss.backward()
    return torch.stack([torch.as_tensor(float(t.detach() if torch.is_tensor(t) else t), dtype=torch.float64) for t in (loss,) + tuple(terms)]), out.grad


@pytest.mark.parametrize("kind", ["track", "track_pearson", "map", "map_estdepth", "splatam_track", "splatam_map"])
@pytest.mark.parametrize("shape", [(5, 7), (37, 21), (48, 64)])
def test_reference_equals_loss_utils_in_float64(kind, shape):
    """Both sides float64, only the summation order differs: 1e-12 relative, on the four values and on every gradient plane."""
    H, W = shape
    out6, gt, ref = lr.make_inputs("random", H, W)
    cfg, _ = lr.CONFIGS[kind]
    l_u, d_u = _loss_utils_f64(kind, out6, gt, ref)
    l_r, d_r = lr.loss_ref(cfg, out6, gt, ref)
    assert float((l_r - l_u).abs().max()) <= 1e-12 * float(l_u.abs().max()), (l_r, l_u)
    for p in range(6):
        assert float((d_r[p] - d_u[p]).abs().max()) <= 1e-12 * float(d_u[p].abs().max()), p
    assert float(d_r[4:].abs().max()) == 0.0


def test_degenerate_conventions_give_exact_zeros():
    H, W = 17, 33
    out6, gt, ref = lr.make_inputs("random", H, W)
    for dtype in (torch.float64, torch.float32):
        # empty L1 mask: the silhouette is below the threshold everywhere
        low = out6.clone()
        low[4] = 0.5
        l, d = lr.loss_ref(lr.cfg_fields(w_l1=1.0, l1_mask=1, sil_thr=0.99), low, gt, dtype=dtype)
        assert float(l.abs().max()) == 0.0 and float(d.abs().max()) == 0.0
        # empty { ref > 0 } masks: colour L1 over l1_mask = 3, depth-L1 mean over depth_l1_mask = 2
        zref = torch.zeros_like(ref)
        l, d = lr.loss_ref(lr.cfg_fields(w_l1=1.0, l1_mask=3, sil_thr=0.99, w_depth_l1=1.0, depth_l1_mask=2), out6, gt, zref, dtype=dtype)
        assert float(l.abs().max()) == 0.0 and float(d.abs().max()) == 0.0
        # Pearson with no masked pixel, and with exactly one: the term is off
        one = zref.clone()
        one[7, 11] = 2.0
        for r in (zref, one):
            l, d = lr.loss_ref(lr.cfg_fields(w_pearson=1.0, pearson_mask=2), out6, gt, r, dtype=dtype)
            assert float(l[0]) == 0.0 and float(l[3]) == 0.0 and float(d.abs().max()) == 0.0
    # loss4[3]: the depth-L1 term when w_depth_l1 != 0, else 1 - rho
    l, _ = lr.loss_ref(lr.CONFIGS["splatam_map"][0], out6, gt, ref)
    m = ref > 0
    assert abs(float(l[3]) - float((ref.double() - out6[3].double()).abs()[m].mean())) <= 1e-15
    l, _ = lr.loss_ref(lr.CONFIGS["pearson"][0], out6, gt, ref)
    rho = np.corrcoef(out6[3][m].double().numpy(), ref[m].double().numpy())[0, 1]
    assert abs(float(l[3]) - (1.0 - rho)) <= 1e-12


def test_all_zero_rendered_depth_under_a_pearson_mask_is_nan_in_both_precisions():
    """cxx == 0 exactly: 0 / 0.  The reference does not paper over it (nor does loss_utils): the case is the caller's to avoid."""
    out6, gt, ref = lr.make_inputs("random", 17, 33)
    out6[3] = 0.0
    for dtype in (torch.float64, torch.float32):
        l, d = lr.loss_ref(lr.CONFIGS["pearson"][0], out6, gt, ref, dtype=dtype)
        assert torch.isnan(l[0]) and torch.isnan(l[3]) and torch.isfinite(l[1:3]).all()
        assert torch.equal(torch.isnan(d[3]), ref > 0) and float(d[3][~(ref > 0)].abs().max()) == 0.0


@pytest.mark.parametrize("family", lr.FAMILIES)
@pytest.mark.parametrize("shape", lr.SHAPES)
def test_generated_inputs_are_well_conditioned(shape, family):
    H, W = shape
    out6, gt, ref = lr.make_inputs(family, H, W)
    px = lr.planted_pixels(H, W, 0)
    assert len(px) == (12 if H * W >= 24 else 0) and len(set(px)) == len(px)
    # colours: exact ties only where planted, otherwise |out - gt| >= 1e-3 -- the sign of the L1 gradient is not a rounding matter
    diff = (out6[:3].double() - gt.double()).abs().view(3, -1)
    ties = diff == 0
    assert int(ties.sum()) == (3 if px else 0)
    for ch in range(3 if px else 0):
        assert bool(ties[ch, px[9 + ch]])
    assert float(diff[~ties].min()) >= lr.MIN_DIFF
    assert float(out6[:3].min()) > 0.0 and float(out6[:3].max()) < 1.0 and float(gt.min()) >= 0.0 and float(gt.max()) <= 1.0
    sil, refv = out6[4].view(-1), ref.view(-1)
    if px:
        # the planted silhouettes: on each threshold, one float32 above and one below it; the planted references 0.0, -0.0, 1e-30
        for i, thr in enumerate(lr.SIL_THRS):
            t = np.float32(thr)
            got = [np.float32(float(sil[px[3 * i + k]])) for k in range(3)]
            assert got[0] == t and got[1] > t and got[2] < t and np.nextafter(got[2], np.float32(2)) == t == np.nextafter(got[1], np.float32(-2))
        z = [float(refv[px[6 + k]]) for k in range(3)]
        assert z[0] == 0.0 and z[1] == 0.0 and np.signbit(np.float32(z[1])) and not np.signbit(np.float32(z[0])) and 0.0 < z[2] < 1e-29
    # masks hold the share of pixels they claim: { sil > 0.99 } 30 %, { sil > 0.5 } all, { ref > 0 } everything but the hole and two plants
    y0, y1, x0, x1 = lr.hole_rect(H, W)
    hole = torch.zeros(H, W, dtype=torch.bool)
    hole[y0:y1, x0:x1] = True
    expect = ~hole.view(-1)
    if px:
        expect[px[6]], expect[px[7]], expect[px[8]] = False, False, True
    assert torch.equal(refv > 0, expect)
    assert bool((out6[4] > 0.5).sum() >= H * W - 2) and float(out6[4].max()) <= 1.0
    if H * W >= 256:
        share = float((out6[4] > float(np.float32(0.99))).float().mean())
        assert 0.2 <= share <= 0.4, share
        assert 0.05 <= float(hole.float().mean()) <= 0.15
    assert float(out6[3].min()) >= 1.0 and float(out6[3].max()) <= 3.0 and torch.equal(out6[5], out6[3] * out6[3])
    # Pearson: enough pixels, and the centred sums of squares are a fair share of the raw ones, so cxx ctt is far from 0 and the
    # covariance form keeps its digits in double.  (1 / (ref + 200) varies by ~1e-3 of its mean: its share is ~1e-6 by construction,
    # the reason the kernels hold these moments in double -- loss_pixel.h.)
    for name in ("track_pearson", "map", "map_estdepth", "pearson", "pearson_invert"):
        n, mom = lr.pearson_moments(lr.CONFIGS[name][0], out6, ref)
        if H * W == 1:
            assert n <= 1
            continue
        assert n >= (0.1 * H * W if H * W >= 256 else 4), (name, n)
        for target, (centred, raw) in mom.items():
            assert centred / raw >= (1e-8 if target.startswith("1/") else 1e-3), (name, target, centred / raw)
