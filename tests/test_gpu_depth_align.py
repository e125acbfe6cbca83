"""mm3dgs_align_depth (csrc/align.hip) and the key depth_align_on_device on the GPU: the sums, the solve and the apply against
the float64 restatement (tests/depth_align_ref.py) at derived bars on the shapes where the kernels can go wrong, the edge cases of the
pixel rule, the reference's own fixture, the argument checks, and the route through SLAM.step with its per-frame fit record.  Every test
here fails on the parent commit: the symbol does not exist there."""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import _lib
from tests import depth_align_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(__file__), "golden")
EDGE = (17, 23)


def _run(est, depth, sil=None, planes=False, **kw):
    """align_depth_device on numpy images -> (fit [16] float64, out [H,W] float32).  planes: depth and silhouette as planes 3 and 4 of
    one [6,H,W] device image, the way the SLAM frame path hands them over (at odd H W they start on a 4-byte boundary only)."""
    from mm3dgs_slam_amd.depth_utils import align_depth_device
    e = torch.from_numpy(np.ascontiguousarray(est, dtype=np.float32)).to(DEV)
    if planes:
        H, W = est.shape
        img = torch.zeros(6, H, W, device=DEV)
        img[3], img[4] = torch.from_numpy(depth).to(DEV), torch.from_numpy(sil).to(DEV)
        d, s = img[3], img[4]
        assert d.is_contiguous() and s.is_contiguous() and (d.data_ptr() % 16 != 0 or s.data_ptr() % 16 != 0)
    else:
        d = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).to(DEV)
        s = None if sil is None else torch.from_numpy(np.ascontiguousarray(sil, dtype=np.float32)).to(DEV)
    out, fit = align_depth_device(e, d, s, **kw)
    assert out.dtype == torch.float32 and out.shape == e.shape and fit.dtype == torch.float64 and fit.shape == (16,) and fit.is_cuda
    return fit.cpu().numpy(), out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """seeded inputs and the restatement's fit of one shape, computed once and left unchanged"""
    est, depth, sil = R.make_inputs(*shape)
    return est, depth, sil, R.align_ref(est, depth, sil)


def _hold_sums(fit, ref, what):
    """bar A on a00, a01, b0, b1; n and ok exactly; the zero tail"""
    assert fit[3] == ref["n"] and fit[2] == float(ref["ok"]), (what, fit[:4], ref["n"], ref["ok"])
    for k, name in ((4, "a00"), (5, "a01"), (6, "b0"), (7, "b1")):
        err, bar = abs(fit[k] - ref[name]), R.bar_sums(ref["n"], ref[name])
        print(f"{what}: {name} |dev - ref| = {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (what, name, fit[k], ref[name], err, bar)
    assert not fit[8:].any()


def _hold_apply(out, est, fit, what):
    """bar C: torch on the CPU with the device's own float32 (scale, shift); <= 4 float32 ulp at every finite pixel, expected 0"""
    s, t = torch.tensor(np.float32(fit[0])), torch.tensor(np.float32(fit[1]))
    assert float(s) == fit[0] and float(t) == fit[1]          # the record holds float32 values
    ref = (1.0 / (s * torch.from_numpy(np.ascontiguousarray(est)) + t)).numpy()
    fin = np.isfinite(ref)
    ulp = R.ulp_diff(out[fin], ref[fin])
    print(f"{what}: apply, {int((out.view(np.int32) != ref.view(np.int32)).sum())} of {out.size} pixels not bit-identical, "
          f"max {float(ulp.max()) if ulp.size else 0.0:.2f} ulp")
    assert (ulp <= 4).all(), (what, float(ulp.max()))
    assert np.array_equal(out[~fin], ref[~fin], equal_nan=True), what


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_alignment_kernels_match_the_float64_restatement(shape):
    """Sums at bar A, n and ok exactly, float32 scale and shift at bar B, the scaled image at bar C -- on 1x1 (n = 1: identity), 1x2 (the
    boundary of n >= 2), a short wave, one wave, a wave plus a lane, one workgroup, a ragged odd-sized image, one pixel beyond a full
    sweep of the 256 x 256-lane grid (depth_align_ref.BEYOND_ONE_SWEEP = 1 x 65537) and the 480x640 SLAM frame."""
    est, depth, sil, ref = _case(shape)
    fit, out = _run(est, depth, sil, planes=shape in R.ODD_SHAPES)
    what = f"{shape[0]}x{shape[1]}"
    _hold_sums(fit, ref, what)
    ds, dt = abs(fit[0] - float(ref["scale"])), abs(fit[1] - float(ref["shift"]))
    bs, bt = R.bar_scale(ref["scale"]), R.bar_shift(ref["scale"], ref["shift"], np.abs(est).mean())
    print(f"{what}: |d scale| = {ds:.3e} (bar {bs:.3e}), |d shift| = {dt:.3e} (bar {bt:.3e})")
    assert ds <= bs and dt <= bt
    if shape == (1, 1):
        assert list(fit[:4]) == [1.0, 0.0, 0.0, 1.0]
    else:
        assert fit[2] == 1.0
    _hold_apply(out, est, fit, what)


def test_systems_without_a_fit_return_the_identity_and_say_so():
    """17x23: every pixel masked out, exactly one valid pixel, two valid pixels with equal est, a constant est (0.25: exact sums; 0.3:
    sums that do not cancel exactly) and a nearly constant one (0.3 (1 + 2e-7 g)) -- scale 1, shift 0, ok 0, the pixel count exact, and
    the scaled image is 1 / est."""
    est, depth, sil, _ = _case(EDGE)
    rng = np.random.default_rng(7)
    one, two = np.zeros_like(sil), np.zeros_like(sil)
    one[5, 7] = 1.0
    two[5, 7] = two[11, 2] = 1.0
    same = est.copy()
    same[11, 2] = same[5, 7]
    nearly = (0.3 * (1.0 + 2e-7 * rng.standard_normal(EDGE))).astype(np.float32)
    cases = {"all masked": (est, np.zeros_like(sil)), "one pixel": (est, one), "two equal": (same, two),
             "constant 0.25": (np.full(EDGE, 0.25, np.float32), sil), "constant 0.3": (np.full(EDGE, 0.3, np.float32), sil), "nearly constant": (nearly, sil)}
    for what, (e, s) in cases.items():
        fit, out = _run(e, depth, s, planes=True)
        ref = R.align_ref(e, depth, s)
        assert not ref["ok"]
        print(what, fit[:8])
        assert list(fit[:3]) == [1.0, 0.0, 0.0] and fit[3] == ref["n"], (what, fit)
        _hold_apply(out, e, fit, what)
    fit, _ = _run(est, depth, two, planes=True)          # (and two DIFFERENT values are a fit)
    assert fit[2] == 1.0 and fit[3] == 2.0


def test_garbage_outside_the_considered_pixels_does_not_reach_the_sums():
    """NaN and inf of est where the silhouette fails: the fit record is bit-identical to the clean one and the scaled image equals
    torch's under equal_nan.  Depth 0, negative, +inf, NaN and a subnormal depth (whose inverse overflows: the documented difference from
    the host path) at silhouette-passing pixels: excluded, sums as the restatement's.  sil == float32(0.99) and est == float32(1e-6)
    exactly: excluded (strict comparisons)."""
    est, depth, sil, ref = _case(EDGE)
    clean, _ = _run(est, depth, sil, planes=True)
    outside = np.argwhere(~(sil > R.SIL_MIN))
    assert len(outside) > 8
    dirty = est.copy()
    dirty[~(sil > R.SIL_MIN)] = np.nan
    dirty[outside[0][0], outside[0][1]] = np.inf
    dirty[outside[1][0], outside[1][1]] = -np.inf
    fit, out = _run(dirty, depth, sil, planes=True)
    assert np.array_equal(fit.view(np.int64), clean.view(np.int64))
    _hold_apply(out, dirty, fit, "dirty est")

    inside = np.argwhere(sil > R.SIL_MIN)
    bad = depth.copy()
    for (y, x), v in zip(inside[:5], (0.0, -2.0, np.inf, np.nan, 1e-45)):
        bad[y, x] = v
    fit, _ = _run(est, bad, sil, planes=True)
    want = R.align_ref(est, bad, sil)
    assert want["n"] == ref["n"] - 5 and np.isfinite(fit).all()
    _hold_sums(fit, want, "bad depth")
    assert fit[0] == float(want["scale"]) or abs(fit[0] - float(want["scale"])) <= R.bar_scale(want["scale"])

    edge_sil, edge_est = sil.copy(), est.copy()
    (y0, x0), (y1, x1) = inside[6], inside[9]
    edge_sil[y0, x0], edge_est[y1, x1] = np.float32(0.99), np.float32(1e-6)
    fit, _ = _run(edge_est, depth, edge_sil, planes=True)
    want = R.align_ref(edge_est, depth, edge_sil)
    assert want["n"] == ref["n"] - 2
    _hold_sums(fit, want, "thresholds")


def test_without_a_silhouette_the_mask_is_positive_depth():
    """silhouette NULL (the UT-MM first frame, fitted to the sensor depth over gt_depth > 0): holes of the sensor (0) stay out, est is not
    thresholded."""
    est, depth, _, _ = _case(EDGE)
    holes = depth.copy()
    holes[::3, ::4] = 0.0
    holes[2, 3] = -1.0
    low = est.copy()
    low[1, 1] = np.float32(1e-7)          # below est_min: still summed, the rule has no est threshold here
    fit, out = _run(low, holes, None)
    want = R.align_ref(low, holes, None)
    assert want["n"] == float((holes > 0).sum())
    _hold_sums(fit, want, "no silhouette")
    assert abs(fit[0] - float(want["scale"])) <= R.bar_scale(want["scale"])
    assert abs(fit[1] - float(want["shift"])) <= R.bar_shift(want["scale"], want["shift"], np.abs(low).mean())
    _hold_apply(out, low, fit, "no silhouette")


@pytest.mark.parametrize("shape", [EDGE, (480, 640)], ids=["17x23", "480x640"])
def test_two_calls_give_the_same_bits_and_fresh_outputs(shape):
    from mm3dgs_slam_amd.depth_utils import align_depth_device
    est, depth, sil = (torch.from_numpy(a).to(DEV) for a in _case(shape)[:3])
    o1, f1 = align_depth_device(est, depth, sil)
    keep = o1.clone()
    o2, f2 = align_depth_device(est * 2.0, depth, sil)          # another fit in between, through the same cached work buffer
    o3, f3 = align_depth_device(est, depth, sil)
    torch.cuda.synchronize()
    assert o1.data_ptr() != o2.data_ptr() != o3.data_ptr() and f1.data_ptr() != f3.data_ptr()
    assert torch.equal(o1.view(torch.int32), keep.view(torch.int32))          # a later call did not write into an earlier result
    assert torch.equal(f1.view(torch.int64), f3.view(torch.int64)) and torch.equal(o1.view(torch.int32), o3.view(torch.int32))
    assert not torch.equal(f1, f2)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """H <= 0, W <= 0 and a NULL est, depth, work or fit (or a misaligned work / fit): -1 with a text in mm3dgs_last_error; nothing is
    launched, the outputs keep their sentinel.  The work size is a positive multiple of 8 that covers one 64-byte row per workgroup."""
    lib = _lib.load()
    H, W = EDGE
    est, depth, sil = (torch.from_numpy(a).to(DEV) for a in _case(EDGE)[:3])
    nbytes = int(lib.mm3dgs_align_depth_work_bytes(H, W))
    assert nbytes >= 64 * ((H * W + R.WG - 1) // R.WG) and nbytes % 8 == 0
    assert int(lib.mm3dgs_align_depth_work_bytes(480, 640)) >= 64 * R.MAX_ROWS and int(lib.mm3dgs_align_depth_work_bytes(0, 5)) == 0
    work = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device=DEV)
    fit = torch.full((17,), -77.0, dtype=torch.float64, device=DEV)
    out = torch.full((H, W), -77.0, device=DEV)
    P = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(None)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(H=H, W=W, e=P(est), d=P(depth), s=P(sil), w=P(work), f=P(fit), o=P(out)):
        return lib.mm3dgs_align_depth(H, W, e, d, s, 0.99, 1e-6, w, f, o, stream)

    for kw in ({"H": 0}, {"W": -1}, {"e": null}, {"d": null}, {"w": null}, {"f": null},
               {"w": C.c_void_p(work.data_ptr() + 4)}, {"f": C.c_void_p(fit.data_ptr() + 4)}):
        assert call(**kw) == -1, kw
        assert b"align_depth" in lib.mm3dgs_last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == -77.0).all()) and bool((fit == -77.0).all())
    assert call(s=null) == 0 and call(o=null) == 0          # the silhouette and the scaled image are optional
    torch.cuda.synchronize()
    assert bool((out != -77.0).all()) and float(fit[2]) == 1.0 and float(fit[16]) == -77.0


def test_g11_fixture_through_the_kernels():
    """tests/golden/g11_depth_align.npz, the reference's own get_scale_shift: the stored mask as a 0 / 1 silhouette, est_min = -inf; the
    bars of test_golden_host.py::test_g11_depth_alignment_matches_the_reference_least_squares."""
    F = np.load(os.path.join(G, "g11_depth_align.npz"))
    for k in range(3):
        est, depth, mask = (F[f"c{k}_{n}"] for n in ("est", "depth", "mask"))
        fit, scaled = _run(est, depth, mask.astype(np.float32), est_min=float("-inf"))
        rs, rt = float(F[f"c{k}_scale"].reshape(-1)[0]), float(F[f"c{k}_shift"].reshape(-1)[0])
        print(f"g11 case {k}: scale {fit[0]!r} (reference {rs!r}), shift {fit[1]!r} ({rt!r})")
        assert fit[2] == 1.0
        assert abs(fit[0] - rs) <= 2e-4 * abs(rs) and abs(fit[1] - rt) <= 2e-4 * abs(rt) + 1e-6, (k, fit[:2], rs, rt)
        ref = F[f"c{k}_scaled"]
        ok = mask.astype(bool) & np.isfinite(ref) & (np.abs(ref) < 50)
        assert (np.abs(scaled - ref)[ok] <= 1e-3 * np.abs(ref)[ok] + 1e-4).all(), k
        want = R.align_ref(est, depth, mask.astype(np.float32), est_min=-np.inf)          # and the restatement, on real-looking data
        assert fit[3] == want["n"] and abs(fit[0] - float(want["scale"])) <= R.bar_scale(want["scale"])


# ---- through SLAM.step ----------------------------------------------------------------------------------------------------------------
def _slam(key, outputdir=None):
    """the configuration of test_slam_cpu.py::test_frames_without_sensor_depth_align_the_monocular_estimate_to_the_map_every_frame on the
    GPU with the native loops"""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device=DEV, height=32, width=48, use_gt_depth=False, depth_align_on_device=key, tracking={"iters": 3},
                         mapping={"iters": 4, "kf_every": 1, "min_covisibility": 2.0})
    if outputdir is not None:
        cfg["outputdir"] = str(outputdir)
    seq = SyntheticSequence(cfg, 3, 600, seed=5)
    slam = SLAM(cfg, seq)
    assert type(slam.tracker).__name__ == "FusedTracker" and type(slam.mapper).__name__ == "FusedMapper"
    return cfg, seq, slam


def _forbid_host_fit(monkeypatch):
    from mm3dgs_slam_amd import depth_utils

    def raising(*a, **k):
        raise AssertionError("get_scale_shift_LS: the host fit ran")
    monkeypatch.setattr(depth_utils, "get_scale_shift_LS", raising)


PARENT_RESULT_KEYS = {"pose_est", "pose_gt", "keyframes", "ate_rmse", "psnr_list", "ssim_list", "lpips_list"}


def test_slam_frames_take_the_device_fit_and_record_it(monkeypatch, tmp_path, capsys):
    """depth_align_on_device through SLAM.step with the host fit patched to raise (the routing), the CPU test's own assertions on the
    frames after the first, every frame's scaled estimate against the unpatched host path on the same render (bar C over the finite
    pixels), no aliasing between the frames' outputs, one ok fit record per aligned frame, and results.npz: depth_align."""
    from mm3dgs_slam_amd.depth_utils import scale_depth_estimate
    cfg, seq, slam = _slam(True, tmp_path)
    seen, renders, kept = [], {}, []
    real_run, real_render = slam.mapper.run_frame, slam.mapper._render_depth_sil
    slam.mapper.run_frame = lambda idx, color, depth, est_scaled, *a, **k: (seen.append(est_scaled), kept.append(est_scaled.clone()),
                                                                            real_run(idx, color, depth, est_scaled, *a, **k))[2]

    def render(pose):
        d, s = real_render(pose)
        renders[len(seen)] = (d.clone(), s.clone())
        return d, s
    slam.mapper._render_depth_sil = render
    with monkeypatch.context() as m:
        _forbid_host_fit(m)
        for i in range(3):
            slam.step(i)
    slam.mapper.run_frame, slam.mapper._render_depth_sil = real_run, real_render
    torch.cuda.synchronize()
    assert torch.allclose(seen[0], 1.0 / (seq.est(0) + 0.001) * 500.0)          # the arbitrary first-frame scale stays as it is
    for i in (1, 2):
        d, sil = slam.mapper._render_depth_sil(slam.estimate_pose_list[i])
        mask = (sil > 0.99) & (seq[i][1] > 0)
        assert int(mask.sum()) > 100
        rel = ((seen[i] - d).abs() / d)[mask]
        print(f"frame {i}: {int(mask.sum())} masked pixels, median relative difference to the rendered depth {float(rel.median()):.4f}")
        assert float(rel.median()) < 0.05, float(rel.median())
        d, sil = renders[i]          # what the frame's fit saw
        # the unpatched host path on the same render, evaluated by torch on the CPU
        host = scale_depth_estimate(dict(cfg, device="cpu"), i, seq.est(i).cpu(), seq[i][1].cpu(), lambda: (d.cpu(), sil.cpu())).numpy()
        dev = seen[i].cpu().numpy()
        fin = np.isfinite(host)
        ulp = R.ulp_diff(dev[fin], host[fin])
        print(f"frame {i}: device vs host scaled estimate, {int((dev.view(np.int32) != host.view(np.int32)).sum())} of {dev.size} pixels not "
              f"bit-identical, max {float(ulp.max()):.2f} ulp; fit {slam.depth_fits[i - 1][:4].tolist()}")
        assert (ulp <= 4).all(), (i, float(ulp.max()))
    # the keyframe aliasing trap: frame 1's scaled estimate (kept by its keyframe) was not overwritten by frame 2's
    assert seen[1].data_ptr() != seen[2].data_ptr()
    for i in range(3):
        assert torch.equal(seen[i].view(torch.int32), kept[i].view(torch.int32)), i
    assert slam.depth_fit_frames == [1, 2] and len(slam.depth_fits) == 2
    for f in slam.depth_fits:
        assert f.is_cuda and f.shape == (16,) and float(f[2]) == 1.0 and float(f[3]) > 100
    figures = capsys.readouterr().out
    res = slam.save_results(3)
    assert "Warning" not in capsys.readouterr().out
    saved = np.load(os.path.join(str(tmp_path), "results.npz"), allow_pickle=True)
    assert set(saved.files) == PARENT_RESULT_KEYS | {"depth_align"}
    table = saved["depth_align"]
    assert table.shape == (3, 4) and np.isnan(table[0]).all()
    assert np.array_equal(table[1:], torch.stack(slam.depth_fits)[:, :4].cpu().numpy()) and np.array_equal(res["depth_align"], table, equal_nan=True)
    # a frame whose system had no fit is named once
    slam.depth_fits[1] = torch.tensor([1.0, 0.0, 0.0, 1.0] + [0.0] * 12, dtype=torch.float64, device=DEV)
    bad = slam.depth_align_table(3)
    text = capsys.readouterr().out
    assert text.count("Warning") == 1 and "[2]" in text and list(bad[2]) == [1.0, 0.0, 0.0, 1.0]
    with capsys.disabled():
        print(figures, end="")


def test_with_the_key_off_the_frame_runs_the_host_fit_and_results_keep_their_keys(monkeypatch, tmp_path):
    """The same patch with the key false makes frame 1 raise -- it does see the host fit -- and an unpatched run writes exactly the
    parent's results.npz keys and records nothing."""
    _, _, slam = _slam(False, tmp_path)
    slam.step(0)
    with monkeypatch.context() as m:
        _forbid_host_fit(m)
        with pytest.raises(AssertionError, match="the host fit ran"):
            slam.step(1)
    _, _, slam = _slam(False, tmp_path)
    for i in range(2):
        slam.step(i)
    slam.save_results(2)
    saved = np.load(os.path.join(str(tmp_path), "results.npz"), allow_pickle=True)
    assert set(saved.files) == PARENT_RESULT_KEYS and slam.depth_fits == []


def test_utmm_first_frame_is_fitted_to_the_sensor_depth_on_the_device(monkeypatch):
    """The UT-MM first-frame branch of scale_depth_estimate with on_device: mm3dgs_align_depth without a silhouette over gt_depth > 0, the
    host fit never runs, and the result meets the host path's at bar C."""
    from mm3dgs_slam_amd import depth_utils
    from mm3dgs_slam_amd.config import utmm_config
    cfg = utmm_config(device=DEV, use_gt_depth=False)
    cfg["dataset"] = "utmm"
    est, depth, _, _ = _case(EDGE)
    gt = depth.copy()
    gt[::4, ::3] = 0.0
    e, g = torch.from_numpy(est).to(DEV), torch.from_numpy(gt).to(DEV)
    host = depth_utils.scale_depth_estimate(dict(cfg, device="cpu"), 0, e.cpu(), g.cpu(), None).numpy()
    with monkeypatch.context() as m:
        _forbid_host_fit(m)
        out, fit = depth_utils.scale_depth_estimate(cfg, 0, e, g, None, on_device=True, return_fit=True)
    assert float(fit[2]) == 1.0 and float(fit[3]) == float((gt > 0).sum())
    ulp = R.ulp_diff(out.cpu().numpy(), host)
    print("UT-MM first frame: max", float(ulp.max()), "ulp against the host path")
    assert (ulp <= 4).all()
