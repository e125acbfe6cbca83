"""mm3dgs_eval_image (csrc/eval.hip) against the float64 host statement eval_utils.image_metrics_host, at the shapes where a tiled 11-tap
kernel can go wrong (a tile edge, the 5-pixel padding band, a partial tile, a multi-row reduction, a wide grid), and the evaluation of a
native-loop run with `eval_on_device` off and on.

Bars (include/mm3dgs.h): the columns summed in double (psnr, depth_l1, mse, depth_rmse) to 1e-9 relative (psnr: 1e-9 dB absolute) -- at most
33 024 summands per sum at unit roundoff 1.1e-16 is <= 4e-12, the rest is margin --, n exactly; the SSIM columns to

    |device - float64|  <=  8 x E32  +  one float32 ulp of 1,    E32 = mean over the pixels of |smap_float32 - smap_float64|,

the distance of torch's own float32 evaluation of the map from the float64 one, computed at run time (tests/eval_cases.py); 8 is
tests/loss_ref.py's FACTOR.  Every test prints its figures (`EVALERR ...`, pytest -s) before it asserts; DESIGN.md holds the largest."""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest
import torch

from tests import eval_cases as ec
from tests import loss_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096          # bytes of guard zone on each side of the work buffer
SENTINEL = -12345.5   # the rows of the table a call must not touch


def _ptr(t):
    return None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _window():
    return (C.c_float * 11)(*lr.gauss_window())


def _work_bytes(H, W):
    from mm3dgs_slam_amd import _lib
    return int(_lib.load().mm3dgs_eval_image_work_bytes(H, W))


def raw_call(H, W, image, gt, depth, gt_depth, work, row, window="own"):
    """mm3dgs_eval_image through the C ABI (tensors or raw addresses); returns the return code."""
    from mm3dgs_slam_amd import _lib
    from mm3dgs_slam_amd.rasterizer import _stream
    rc = _lib.load().mm3dgs_eval_image(H, W, _ptr(image), _ptr(gt), _ptr(depth), _ptr(gt_depth), _window() if window == "own" else window,
                                       _ptr(work), _ptr(row), _stream())
    torch.cuda.synchronize()
    return rc


def score(image, gt, depth, gt_depth, fill=0.0):
    """One call with the row in the middle of a 48-double table of sentinels and the work buffer between guard zones filled with `fill`;
    checks that nothing else was written and returns the row (CPU, float64)."""
    H, W = image.shape[1:]
    n = _work_bytes(H, W)
    assert n > 0 and n % 8 == 0
    buf = torch.full(((2 * GUARD + n) // 8,), fill, dtype=torch.float64, device=DEV)
    table = torch.full((3, 16), SENTINEL, dtype=torch.float64, device=DEV)
    assert raw_call(H, W, image, gt, depth, gt_depth, buf.data_ptr() + GUARD, table[1]) == 0
    t, b = table.cpu(), buf.cpu()
    assert bool((t[0] == SENTINEL).all()) and bool((t[2] == SENTINEL).all())
    g = GUARD // 8
    guard = torch.cat([b[:g], b[-g:]])
    assert bool(torch.isnan(guard).all()) if math.isnan(fill) else bool((guard == fill).all())
    return t[1].clone()


@pytest.fixture(scope="module")
def device_inputs():
    return {case: tuple(t.to(DEV) for t in ec.inputs(*case)) for case in ec.CASES}


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("family,H,W", ec.CASES)
def test_kernel_rows_against_the_float64_host_statement(device_inputs, family, H, W):
    ref = ec.reference(family, H, W).numpy()
    got = score(*device_inputs[(family, H, W)]).numpy()
    e_all, e_ch = ec.e32(family, H, W)
    errs = {c: (abs(got[c] - ref[c]) if c == 0 else _rel(got[c], ref[c])) for c in ec.DOUBLE_COLS}
    ssim_err = [abs(got[1] - ref[1])] + [abs(got[7 + c] - ref[7 + c]) for c in range(3)]
    ssim_bnd = [ec.ssim_bound(e_all)] + [ec.ssim_bound(e) for e in e_ch]
    print(f"EVALERR {family} {H}x{W}: psnr {errs[0]:.1e} dB, depth_l1 {errs[2]:.1e}, mse {max(errs[4], errs[5], errs[6]):.1e}, rmse {errs[10]:.1e} (rel); "
          f"ssim {ssim_err[0]:.2e} of {ssim_bnd[0]:.2e} (E32 {e_all:.2e}), per channel " + ", ".join(f"{e:.2e} of {b:.2e}" for e, b in zip(ssim_err[1:], ssim_bnd[1:])))
    assert math.isfinite(ref[0])
    assert got[3] == ref[3]
    assert errs[0] <= ec.PSNR_ABS
    for c in ec.DOUBLE_COLS[1:]:
        assert errs[c] <= ec.REL_DOUBLE, (c, got[c], ref[c])
    for e, b in zip(ssim_err, ssim_bnd):
        assert e <= b, (ssim_err, ssim_bnd)
    assert not got[11:].any()


def test_degenerate_rows_on_the_device():
    from mm3dgs_slam_amd.eval_utils import image_metrics_host
    cases = ec.degenerate_cases()
    dev = lambda name: tuple(None if t is None else t.to(DEV) for t in cases[name])
    same = score(*dev("same")).numpy()
    print(f"EVALERR image == gt: psnr {same[0]}, |ssim - 1| = {abs(same[1] - 1.0):.2e}, mse {same[4:7]}")
    assert same[0] == math.inf and not same[4:7].any() and abs(same[1] - 1.0) <= 1e-6
    for name in ("no_valid", "no_depth"):
        row = score(*dev(name)).numpy()
        ref = image_metrics_host(*cases[name]).numpy()
        assert math.isnan(row[2]) and math.isnan(row[10]) and row[3] == 0.0, (name, row)
        assert abs(row[0] - ref[0]) <= ec.PSNR_ABS
    for name in ("planted", "only_tiny"):
        row = score(*dev(name)).numpy()
        ref = image_metrics_host(*cases[name]).numpy()
        print(f"EVALERR {name} gt_depth: n {row[3]} (reference {ref[3]}), depth_l1 rel {_rel(row[2], ref[2]):.1e}, rmse rel {_rel(row[10], ref[10]):.1e}")
        assert row[3] == ref[3] and _rel(row[2], ref[2]) <= ec.REL_DOUBLE and _rel(row[10], ref[10]) <= ec.REL_DOUBLE
    image, gt, depth, gd = dev("planted")
    nan_depth = depth.clone()
    nan_depth[5, 5] = float("nan")      # a valid pixel: the NaN propagates
    assert math.isnan(float(score(image, gt, nan_depth, gd)[2]))
    nan_depth = depth.clone()
    nan_depth[0, 0] = float("nan")      # gt_depth == 0 there: never read into the sums
    assert torch.equal(score(image, gt, nan_depth, gd), score(image, gt, depth, gd))


@pytest.mark.parametrize("H,W", [(17, 33), (48, 64)])
def test_views_give_the_bits_of_contiguous_copies(H, W):
    """Planes of a [6,H,W] render (H W odd at 17x33: the depth plane starts on a 4-byte boundary only) and a buffer entered one float in."""
    from mm3dgs_slam_amd.eval_utils import image_metrics_device
    out6, gt, ref = (t.to(DEV) for t in lr.make_inputs("random", H, W))
    want = score(out6[:3].contiguous(), gt, out6[3].contiguous(), ref)
    assert out6[3].data_ptr() == out6.data_ptr() + 12 * H * W
    assert torch.equal(score(out6[:3], gt, out6[3], ref), want)
    off = torch.zeros(4 * H * W + 1, device=DEV)
    off[1:3 * H * W + 1] = gt.reshape(-1)
    off[3 * H * W + 1:] = ref.reshape(-1)
    gt_off, ref_off = off[1:3 * H * W + 1].view(3, H, W), off[3 * H * W + 1:].view(H, W)
    assert gt_off.data_ptr() == off.data_ptr() + 4
    assert torch.equal(score(out6[:3], gt_off, out6[3], ref_off), want)
    table = torch.full((3, 16), SENTINEL, dtype=torch.float64, device=DEV)      # the Python entry: views as they are, a row of a table
    image_metrics_device(out6[:3], gt_off, out6[3], ref_off, table[2])
    t = table.cpu()
    assert torch.equal(t[2], want) and bool((t[:2] == SENTINEL).all())
    with pytest.raises(RuntimeError, match="device tensors"):
        image_metrics_device(out6[:3].cpu(), gt, out6[3], ref, table[0])


def test_calls_repeat_their_bits_and_ignore_the_work_buffers_contents(device_inputs):
    for case in (("random", 37, 21), ("flat", 80, 208)):
        args = device_inputs[case]
        zeroed = score(*args, fill=0.0)
        assert torch.equal(score(*args, fill=0.0), zeroed)
        assert torch.equal(score(*args, fill=float("nan")), zeroed)
    # two calls on one work buffer, the second on what the first left there
    H, W = 37, 21
    args = device_inputs[("random", H, W)]
    work = torch.empty(_work_bytes(H, W) // 8, dtype=torch.float64, device=DEV)
    table = torch.zeros(2, 16, dtype=torch.float64, device=DEV)
    assert raw_call(H, W, *args, work, table[0]) == 0 and raw_call(H, W, *args, work, table[1]) == 0
    assert torch.equal(table[0].cpu(), table[1].cpu()) and torch.equal(table[0].cpu(), score(*args))


def test_rejected_calls_return_minus_one_and_write_nothing(device_inputs):
    from mm3dgs_slam_amd import _lib
    H, W = 17, 33
    image, gt, depth, gd = device_inputs[("random", H, W)]
    n = _work_bytes(H, W)
    work = torch.full((n // 8,), SENTINEL, dtype=torch.float64, device=DEV)
    table = torch.full((3, 16), SENTINEL, dtype=torch.float64, device=DEV)
    row, wp = table[1], work.data_ptr()
    NULL_WINDOW = C.POINTER(C.c_float)()
    bad = {
        "H = 0": lambda: raw_call(0, W, image, gt, depth, gd, work, row),
        "W < 0": lambda: raw_call(H, -3, image, gt, depth, gd, work, row),
        "more than 2^28 pixels": lambda: raw_call(1 << 14, (1 << 14) + 1, image, gt, depth, gd, work, row),
        "NULL image": lambda: raw_call(H, W, None, gt, depth, gd, work, row),
        "NULL gt": lambda: raw_call(H, W, image, None, depth, gd, work, row),
        "NULL window": lambda: raw_call(H, W, image, gt, depth, gd, work, row, window=NULL_WINDOW),
        "NULL work": lambda: raw_call(H, W, image, gt, depth, gd, None, row),
        "NULL row": lambda: raw_call(H, W, image, gt, depth, gd, work, None),
        "depth without gt_depth": lambda: raw_call(H, W, image, gt, depth, None, work, row),
        "gt_depth without depth": lambda: raw_call(H, W, image, gt, None, gd, work, row),
        "misaligned work": lambda: raw_call(H, W, image, gt, depth, gd, wp + 4, row),
        "misaligned row": lambda: raw_call(H, W, image, gt, depth, gd, work, row.data_ptr() + 4),
        "misaligned image": lambda: raw_call(H, W, image.data_ptr() + 2, gt, depth, gd, work, row),
        "misaligned gt": lambda: raw_call(H, W, image, gt.data_ptr() + 1, depth, gd, work, row),
        "misaligned depth": lambda: raw_call(H, W, image, gt, depth.data_ptr() + 2, gd, work, row),
        "misaligned gt_depth": lambda: raw_call(H, W, image, gt, depth, gd.data_ptr() + 3, work, row),
    }
    for what, call in bad.items():
        assert call() == -1, what
        assert _lib.load().mm3dgs_last_error(), what
    torch.cuda.synchronize()
    assert bool((table.cpu() == SENTINEL).all()) and bool((work.cpu() == SENTINEL).all())
    for shape in ((0, W), (H, 0), (-1, W), (H, -1), (1 << 14, (1 << 14) + 1)):
        assert _work_bytes(*shape) == 0, shape
    assert raw_call(H, W, image, gt, None, None, work, row) == 0      # no depth images at all is a valid call


PARENT_KEYS = ["pose_est", "pose_gt", "keyframes", "ate_rmse", "psnr_list", "ssim_list", "lpips_list"]


def _run(tmp, eval_on_device, frames=4):
    """The small native run of tests/test_gpu_debug_frames.py::_run, with `eval_every: 1` and the evaluation key."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device=DEV, height=48, width=64, tracking={"iters": 5}, mapping={"iters": 6, "kf_every": 2, "min_covisibility": 2.0},
                         outputdir=str(tmp), debug={"get_runtime_stats": False, "create_video": False, "save_keyframes": False},
                         eval_every=1, eval_on_device=eval_on_device)
    seq = SyntheticSequence(cfg, frames, 2000, seed=5)
    slam = SLAM(cfg, seq)
    from mm3dgs_slam_amd.fused import FusedMapper, FusedTracker
    assert isinstance(slam.tracker, FusedTracker) and isinstance(slam.mapper, FusedMapper)
    slam.run()
    return slam, seq, cfg


def test_native_run_scores_its_frames_on_the_device_and_eval_reproduces_them(tmp_path):
    import slam_top
    from mm3dgs_slam_amd.eval_utils import image_metrics_host
    n = 4
    on_dir, off_dir = tmp_path / "on", tmp_path / "off"
    on, seq, cfg_on = _run(on_dir, True, n)
    off, _, _ = _run(off_dir, False, n)
    a = np.load(on_dir / "results.npz", allow_pickle=True)
    b = np.load(off_dir / "results.npz", allow_pickle=True)
    assert a["pose_est"].shape == (n, 7) and a["pose_est"].tobytes() == b["pose_est"].tobytes()
    assert list(b.keys()) == PARENT_KEYS
    assert list(a.keys()) == PARENT_KEYS + ["eval_table", "eval_frames", "depth_l1_list"]
    assert a["eval_table"].shape == (n, 16) and a["eval_table"].dtype == np.float64
    assert a["eval_frames"].dtype == np.int64 and a["eval_frames"].tolist() == [0, 1, 2, 3]
    for key in ("psnr_list", "ssim_list"):
        assert a[key].shape == b[key].shape == (n,) and a[key].dtype == b[key].dtype == np.float32
    d_psnr, d_ssim = np.abs(a["psnr_list"].astype(np.float64) - b["psnr_list"]), np.abs(a["ssim_list"].astype(np.float64) - b["ssim_list"])
    print(f"EVALERR run: psnr {a['psnr_list']} on / {b['psnr_list']} off, max |delta| {d_psnr.max():.2e} dB; ssim max |delta| {d_ssim.max():.2e}")
    assert d_psnr.max() <= 1e-4 and d_ssim.max() <= 1e-5
    assert np.array_equal(a["psnr_list"], a["eval_table"][:, 0].astype(np.float32)) and np.array_equal(a["depth_l1_list"], a["eval_table"][:, 2])
    with torch.no_grad():
        for k in range(n):
            result = on.renderer.render(on.gaussians, camera_pose=on.estimate_pose_list[k])
            ref = image_metrics_host(result["render"].cpu(), seq[k][0].cpu(), result["depth"][0].cpu(), seq[k][1].cpu()).numpy()
            assert ref[3] > 0 and a["eval_table"][k, 3] == ref[3]
            assert _rel(a["depth_l1_list"][k], ref[2]) <= ec.REL_DOUBLE, (k, a["depth_l1_list"][k], ref[2])
    # --eval: the checkpoint scored again, from the files alone; nothing written
    before = (on_dir / "results.npz").read_bytes()
    listing = sorted(os.listdir(on_dir))
    out = slam_top.evaluate_checkpoint(cfg_on, seq)
    assert out["iteration"] == n and len(out["psnr_list"]) == n
    d = np.abs(np.asarray(out["psnr_list"], dtype=np.float64) - a["psnr_list"])
    print(f"EVALERR --eval: psnr {np.asarray(out['psnr_list'])}, max |delta| to the stored list {d.max():.2e} dB; ATE {out['ate_rmse']:.3e} m, c2w {out['ate_rmse_c2w']:.3e} m")
    assert d.max() <= 1e-4                     # the map read back from its PLY file, rendered and scored by the same kernels
    assert out["ate_rmse"] == float(a["ate_rmse"]) and math.isfinite(out["ate_rmse_c2w"])
    assert (on_dir / "results.npz").read_bytes() == before and sorted(os.listdir(on_dir)) == listing
