"""mm3dgs_mosaic (csrc/mosaic.hip) against the host composer (debug_frames.compose_host), and the debug outputs of a native-loop run.

Bar (include/mm3dgs.h): the same bytes, every one -- zero differing bytes, no tolerance, nothing left out.  Both sides state the same
operators: one float32 subtraction, an exact product with 255 in double, float32 (a - lo) / (hi - lo) with the correctly rounded division,
a table lookup."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(1, 1), (2, 3), (16, 37), (33, 130), (48, 64)]
# per grid: the layouts (names of the panel pool, row-major) it is exercised with
LAYOUTS = {
    (2, 3): [["c_edge", "c_view", "diff", "d_bins", "d_view", "d_nan"], ["c_view", "c_edge", "diff_edge", "d_const", "d_off", "d_rand"]],
    (1, 3): [["d_nan", "c_edge", "d_bins"], ["diff", "d_const", "c_view"]],
    (2, 1): [["c_view", "d_view"], ["d_nan", "diff_edge"]],
    (1, 1): [["c_edge"], ["d_bins"], ["diff"], ["d_nan"], ["d_off"]],
}
SENTINEL, PAD = 0xA5, 64


def pool(H, W):
    """The panels of one shape, on the host.  A "view" panel is a plane (or the first three) of a [6,H,W] render, "off" starts one float
    into its buffer: only a float's alignment."""
    from mm3dgs_slam_amd import debug_frames as df
    g = torch.Generator().manual_seed(100 * H + W)
    HW = H * W
    render6 = torch.rand(6, H, W, generator=g)
    render6[3] = 0.5 + 3.0 * render6[3]
    c_edge = torch.rand(3, H, W, generator=g) * 1.6 - 0.3                       # below 0 and above 1
    special = torch.tensor([float("nan"), -0.0, 1.0, 0.0, 2.0, -1.0, 1.0 / 255, 0.5, 254.5 / 255, float("inf"), -float("inf"), 1e-30])
    k = min(len(special), c_edge.numel())
    c_edge.view(-1)[:k] = special[:k]
    c_other = torch.rand(3, H, W, generator=g)
    d_bins = ((torch.arange(HW) % 257).float() / 256).reshape(H, W)             # exactly k / 256, k = 0 .. 256: lo = 0, hi = 1 once H W >= 257
    d_const = torch.full((H, W), 1.75)
    d_rand = torch.randn(H, W, generator=g) * 40.0
    d_nan = d_rand.abs() + 0.1
    d_nan.view(-1)[HW // 2] = float("nan")
    off_buf = torch.rand(HW + 1, generator=g)
    return {"render6": render6, "off_buf": off_buf,
            "c_edge": (df.COLOR, c_edge, None), "c_view": (df.COLOR, render6[:3], None), "diff": (df.ABSDIFF, render6[:3], c_other),
            "diff_edge": (df.ABSDIFF, c_other, c_edge), "d_bins": (df.DEPTH, d_bins, None), "d_view": (df.DEPTH, render6[3], None),
            "d_const": (df.DEPTH, d_const, None), "d_nan": (df.DEPTH, d_nan, None), "d_rand": (df.DEPTH, d_rand, None),
            "d_off": (df.DEPTH, off_buf[1:].view(H, W), None)}


def on_device(p):
    """The pool on the GPU with the views kept views: a plane of the uploaded [6,H,W] tensor, a buffer entered one float in."""
    render6, off_buf = p["render6"].to(DEV), p["off_buf"].to(DEV)
    H, W = render6.shape[1:]
    out = {}
    for name, v in p.items():
        if name in ("render6", "off_buf"):
            continue
        kind, a, b = v
        if name in ("c_view", "diff"):
            a = render6[:3]
        elif name == "d_view":
            a = render6[3]
        elif name == "d_off":
            a = off_buf[1:].view(H, W)
        else:
            a = a.to(DEV)
        out[name] = (kind, a, None if b is None else b.to(DEV))
    assert out["d_view"][1].data_ptr() == render6.data_ptr() + 12 * H * W and out["d_off"][1].data_ptr() == off_buf.data_ptr() + 4
    return out


@pytest.fixture(scope="module")
def cases():
    """Per shape: the panel pool on both sides and the host composer's bytes for every (grid, layout, quant, bgr); computed once, left unchanged."""
    from mm3dgs_slam_amd import debug_frames as df
    out = {}
    for H, W in SHAPES:
        host = pool(H, W)
        want = {}
        for (rows, cols), layouts in LAYOUTS.items():
            for li, names in enumerate(layouts):
                for quant in (0, 1):
                    for bgr in (0, 1):
                        want[(rows, cols, li, quant, bgr)] = df.compose_host([host[n] for n in names], rows, cols, quant, bool(bgr))
        out[(H, W)] = (host, on_device(host), want)
    return out


def raw_call(H, W, rows, cols, panels, quant, bgr, out_ptr, work_ptr, lut_ptr="own", kinds=None, a_ptrs=None, b_ptrs=None):
    from mm3dgs_slam_amd import debug_frames as df
    if lut_ptr == "own":
        lut_ptr = _lut(quant).data_ptr()
    kinds = [k for k, _, _ in panels] if kinds is None else kinds
    a_ptrs = [a.data_ptr() for _, a, _ in panels] if a_ptrs is None else a_ptrs
    b_ptrs = [0 if b is None else b.data_ptr() for _, _, b in panels] if b_ptrs is None else b_ptrs
    return df.mosaic_call(H, W, rows, cols, kinds, a_ptrs, b_ptrs, lut_ptr, quant, bgr, work_ptr, out_ptr)


_luts = {}


def _lut(quant):
    from mm3dgs_slam_amd import debug_frames as df
    if quant not in _luts:
        _luts[quant] = df.lut_u8(quant).to(DEV)
    return _luts[quant]


def _work(H, W, rows, cols):
    from mm3dgs_slam_amd import _lib
    n = int(_lib.load().mm3dgs_mosaic_work_bytes(H, W, rows, cols))
    assert n > 0 and n % 8 == 0
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_gives_the_host_composers_bytes(cases, H, W):
    host, dev, want = cases[(H, W)]
    checked = 0
    for (rows, cols), layouts in LAYOUTS.items():
        n = rows * H * cols * W * 3
        work = _work(H, W, rows, cols)
        for li, names in enumerate(layouts):
            panels = [dev[k] for k in names]
            for quant in (0, 1):
                for bgr in (0, 1):
                    shift = (checked + li) % 4                     # out starts at every byte alignment in turn
                    buf = torch.full((PAD + shift + n + PAD,), SENTINEL, dtype=torch.uint8, device=DEV)
                    work.fill_(0xFF)
                    out_ptr = buf.data_ptr() + PAD + shift
                    assert raw_call(H, W, rows, cols, panels, quant, bgr, out_ptr, work.data_ptr()) == 0
                    first = buf.cpu()
                    assert raw_call(H, W, rows, cols, panels, quant, bgr, out_ptr, work.data_ptr()) == 0      # work now holds the first call's records
                    second = buf.cpu()
                    got = first[PAD + shift: PAD + shift + n].reshape(rows * H, cols * W, 3)
                    ref = want[(rows, cols, li, quant, bgr)]
                    diff = int((got != ref).sum())
                    print(f"{H}x{W} grid {rows}x{cols} layout {li} quant {quant} bgr {bgr} shift {shift}: {diff} of {n} bytes differ")
                    assert diff == 0, (H, W, rows, cols, names, quant, bgr)
                    assert bool((first[: PAD + shift] == SENTINEL).all()) and bool((first[PAD + shift + n:] == SENTINEL).all())
                    assert torch.equal(first, second)
                    checked += 1
    assert checked == 4 * sum(len(v) for v in LAYOUTS.values())


def test_the_planted_inputs_reach_the_places_they_are_meant_for(cases):
    """The pool does hold what the comparison above relies on (at the largest shape): every bin edge with lo = 0 and hi = 1, a constant
    panel, exactly one NaN, colours below 0, above 1 and NaN -- and the host bytes show them: black panels next to untouched ones."""
    from mm3dgs_slam_amd import debug_frames as df
    H, W = 48, 64
    host, dev, want = cases[(H, W)]
    bins = host["d_bins"][1]
    assert float(bins.min()) == 0.0 and float(bins.max()) == 1.0 and len(torch.unique(bins)) == 257
    assert int(torch.isnan(host["d_nan"][1]).sum()) == 1 and len(torch.unique(host["d_const"][1])) == 1
    c = host["c_edge"][1]
    assert bool((c < 0).any()) and bool((c > 1).any()) and bool(torch.isnan(c).any()) and bool(torch.isinf(c).any())
    ref = want[(2, 3, 0, 0, 0)].numpy()                                    # c_edge c_view diff / d_bins d_view d_nan
    assert not ref[H:, 2 * W:].any() and ref[H:, :W].any() and ref[H:, W:2 * W].any()
    lut = df.lut_u8(0).numpy()
    assert np.array_equal(ref[H, 0], lut[0]) and np.array_equal(ref[H + 4, 0], lut[255])      # value 256 / 256 sits at pixel 256 = (4, 0)
    assert not want[(2, 3, 1, 0, 0)].numpy()[H:, :W].any()                 # d_const


def test_rejected_calls_return_minus_one_and_write_nothing(cases):
    from mm3dgs_slam_amd import _lib
    H, W = 16, 37
    host, dev, _ = cases[(H, W)]
    panels = [dev[k] for k in LAYOUTS[(2, 3)][0]]
    n = 2 * H * 3 * W * 3
    buf = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.uint8, device=DEV)
    out_ptr = buf.data_ptr() + PAD
    work = _work(H, W, 2, 3)
    wp = work.data_ptr()
    a_ptrs = [a.data_ptr() for _, a, _ in panels]
    b_ptrs = [0 if b is None else b.data_ptr() for _, _, b in panels]
    nine = [dev["c_view"]] * 9
    bad = {
        "H = 0": lambda: raw_call(0, W, 2, 3, panels, 0, 0, out_ptr, wp),
        "W < 0": lambda: raw_call(H, -1, 2, 3, panels, 0, 0, out_ptr, wp),
        "rows = 0": lambda: raw_call(H, W, 0, 3, panels, 0, 0, out_ptr, wp),
        "cols < 0": lambda: raw_call(H, W, 2, -3, panels, 0, 0, out_ptr, wp),
        "nine panels": lambda: raw_call(H, W, 3, 3, nine, 0, 0, out_ptr, wp),
        "unknown kind": lambda: raw_call(H, W, 2, 3, panels, 0, 0, out_ptr, wp, kinds=[0, 0, 1, 2, 3, 2]),
        "negative kind": lambda: raw_call(H, W, 2, 3, panels, 0, 0, out_ptr, wp, kinds=[-1, 0, 1, 2, 2, 2]),
        "NULL a entry": lambda: raw_call(H, W, 2, 3, panels, 0, 0, out_ptr, wp, a_ptrs=a_ptrs[:4] + [0] + a_ptrs[5:]),
        "NULL b entry of kind 1": lambda: raw_call(H, W, 2, 3, panels, 0, 0, out_ptr, wp, b_ptrs=[0] * 6),
        "NULL lut with a depth panel": lambda: raw_call(H, W, 2, 3, panels, 0, 0, out_ptr, wp, lut_ptr=0),
        "NULL work": lambda: raw_call(H, W, 2, 3, panels, 0, 0, out_ptr, 0),
        "NULL out": lambda: raw_call(H, W, 2, 3, panels, 0, 0, 0, wp),
        "misaligned work": lambda: raw_call(H, W, 2, 3, panels, 0, 0, out_ptr, wp + 4),
        "quant = 2": lambda: raw_call(H, W, 2, 3, panels, 2, 0, out_ptr, wp, lut_ptr=_lut(0).data_ptr()),
    }
    for what, call in bad.items():
        assert call() == -1, what
        assert _lib.load().mm3dgs_last_error(), what
    torch.cuda.synchronize()
    assert bool((buf.cpu() == SENTINEL).all())
    assert bool((work.cpu() == 0xFF).all())
    # a NULL lut is fine without a depth panel
    colour = [dev["c_edge"], dev["c_view"], dev["diff"]]
    assert raw_call(H, W, 1, 3, colour, 0, 0, out_ptr, wp, lut_ptr=0) == 0
    torch.cuda.synchronize()


def test_compose_device_reuses_its_buffers_and_compose_dispatches(cases):
    from mm3dgs_slam_amd import debug_frames as df
    H, W = 33, 130
    host, dev, want = cases[(H, W)]
    names = LAYOUTS[(2, 3)][0]
    a = df.compose_device([dev[k] for k in names], 2, 3, quant=0, bgr=False)
    assert a.dtype == torch.uint8 and tuple(a.shape) == (2 * H, 3 * W, 3) and a.is_cuda
    assert torch.equal(a.cpu(), want[(2, 3, 0, 0, 0)])
    b = df.compose([dev[k] for k in LAYOUTS[(2, 3)][1]], 2, 3, quant=0, bgr=True)
    assert b.data_ptr() == a.data_ptr()                                     # once per shape
    assert torch.equal(b.cpu(), want[(2, 3, 1, 0, 1)])
    c = df.compose([host[k] for k in names], 2, 3, quant=1)                 # host tensors: the host path
    assert not c.is_cuda and torch.equal(c, want[(2, 3, 0, 1, 0)])
    r = df.compose_device([dev["c_view"], dev["d_view"]], 2, 1, quant=1)
    assert torch.equal(r.cpu(), want[(2, 1, 0, 1, 0)])


def _run(tmp, debug_on, frames=4):
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device=DEV, height=48, width=64, tracking={"iters": 5}, mapping={"iters": 6, "kf_every": 2, "min_covisibility": 2.0},
                         outputdir=str(tmp), debug={"get_runtime_stats": False, "create_video": debug_on, "save_keyframes": debug_on})
    seq = SyntheticSequence(cfg, frames, 2000, seed=5)
    slam = SLAM(cfg, seq)
    from mm3dgs_slam_amd.fused import FusedMapper, FusedTracker
    assert isinstance(slam.tracker, FusedTracker) and isinstance(slam.mapper, FusedMapper)
    slam.run()
    return slam, seq


def test_native_run_writes_the_debug_outputs_and_keeps_its_poses(tmp_path):
    from PIL import Image
    from mm3dgs_slam_amd import debug_frames as df
    n, H, W = 4, 48, 64
    on_dir, off_dir = tmp_path / "on", tmp_path / "off"
    on, seq = _run(on_dir, True, n)
    off, _ = _run(off_dir, False, n)
    video = sorted(os.listdir(on_dir / "debug_video"))
    want = ["000000_00000_map.png"] + [f"{2 * i - 1 + k:06d}_{i:05d}_{name}.png" for i in range(1, n) for k, name in enumerate(("track", "map"))]
    assert video == want and len(video) == 2 * n - 1
    for f in video:
        assert np.asarray(Image.open(on_dir / "debug_video" / f)).shape == (2 * H, 3 * W, 3)
    kf_idx = [kf.idx for kf in on.mapper.keyframes]
    assert len(kf_idx) >= 2 and sorted(os.listdir(on_dir / "keyframes")) == [f"{i:05d}.png" for i in kf_idx]
    for i in kf_idx:
        assert np.asarray(Image.open(on_dir / "keyframes" / f"{i:05d}.png")).shape == (H, W, 3)
    color = seq[0][0].cpu()
    first = np.asarray(Image.open(on_dir / "debug_video" / video[0]))
    assert np.array_equal(first[:H, :W], np.trunc(color.double().numpy() * 255).astype(np.uint8).transpose(1, 2, 0))
    # the frame on disk is the host composer's frame of the same panels: the last "map" frame, recomposed from the finished run
    last = n - 1
    with torch.no_grad():
        result = on.renderer.render(on.gaussians, camera_pose=on.estimate_pose_list[last])
    gt_color, gt_depth, _ = seq[last]
    panels = [(df.COLOR, gt_color, None), (df.COLOR, result["render"], None), (df.ABSDIFF, result["render"], gt_color),
              (df.DEPTH, gt_depth, None), (df.DEPTH, result["depth"][0], None), (df.DEPTH, gt_depth, None)]
    assert torch.equal(df.compose_device(panels, 2, 3).cpu(), df.compose_host(panels, 2, 3))
    if last not in kf_idx:      # (a keyframe's third panel is the seeding mask instead)
        assert np.array_equal(np.asarray(Image.open(on_dir / "debug_video" / video[-1])), df.compose_host(panels, 2, 3).numpy())
    assert not os.path.exists(off_dir / "debug_video") and not os.path.exists(off_dir / "keyframes")
    a = np.load(on_dir / "results.npz", allow_pickle=True)["pose_est"]
    b = np.load(off_dir / "results.npz", allow_pickle=True)["pose_est"]
    assert a.shape == (n, 7) and a.tobytes() == b.tobytes()
    written = on.render(every=1)
    assert len(written) == 2 * n and sorted(os.listdir(on_dir / "render")) == sorted(os.path.basename(p) for p in written)
    want_gt = df.compose_host([(df.COLOR, seq[1][0], None), (df.DEPTH, seq[1][1], None)], 2, 1, quant=1).numpy()
    assert np.array_equal(np.asarray(Image.open(on_dir / "render" / "gt00001.png")), want_gt)
