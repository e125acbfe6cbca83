"""Debug outputs on the CPU (mm3dgs_slam_amd/debug_frames.py): the host composer against the reference's own frames (tests/golden/
g14_video.npz, written by make_golden_video.py), the committed colour table against matplotlib, and debug.create_video /
debug.save_keyframes / SLAM.render() on a small CPU run with the oracle rasterizer injected, as tests/test_slam_cpu.py builds its runs."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import debug_frames as df

HERE = os.path.dirname(os.path.abspath(__file__))
H, W, N_FRAMES = 48, 64, 3


@pytest.fixture(scope="module")
def g14():
    g = np.load(os.path.join(HERE, "golden", "g14_video.npz"))
    return {k: g[k] for k in g.files}


def _t(g14, k):
    return torch.from_numpy(g14[k])


def _video_panels(g14, third):
    gt_color, image = _t(g14, "gt_color"), _t(g14, "image")
    return [(df.COLOR, gt_color, None), (df.COLOR, image, None), (df.ABSDIFF, image, gt_color),
            (df.DEPTH, _t(g14, "gt_depth"), None), (df.DEPTH, _t(g14, "depth"), None), (df.DEPTH, third, None)]


@pytest.mark.parametrize("name,third", [("video_est", "est_scaled"), ("video_gt", "gt_depth"), ("video_mask", "mask")])
def test_host_composer_gives_the_reference_video_frame_byte_for_byte(g14, name, third):
    got = df.compose_host(_video_panels(g14, _t(g14, third).float()), 2, 3, quant=0, bgr=False)
    assert got.dtype == torch.uint8 and tuple(got.shape) == g14[name].shape == (24, 60, 3)
    assert int((got.numpy() != g14[name]).sum()) == 0
    # what the reference hands its video writer (cv2.cvtColor RGB2BGR): the same bytes with the channel axis reversed
    bgr = df.compose_host(_video_panels(g14, _t(g14, third).float()), 2, 3, quant=0, bgr=True)
    assert np.array_equal(bgr.numpy(), g14[name][:, :, ::-1])


def test_host_composer_gives_the_reference_render_pair_byte_for_byte(g14):
    for name, color, depth in (("render", "image", "depth"), ("render_gt", "gt_color", "gt_depth")):
        got = df.compose_host([(df.COLOR, _t(g14, color), None), (df.DEPTH, _t(g14, depth), None)], 2, 1, quant=1)
        assert tuple(got.shape) == g14[name].shape == (24, 20, 3)
        assert int((got.numpy() != g14[name]).sum()) == 0, name


def test_committed_table_is_matplotlibs_viridis():
    table = df.viridis()
    assert table.dtype == torch.float64 and tuple(table.shape) == (256, 3)
    assert float(table.min()) >= 0.0 and float(table.max()) <= 1.0
    for quant in (0, 1):
        lut = df.lut_u8(quant)
        assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3)
        want = np.trunc(np.clip(table.numpy() * 255 + (0.5 if quant else 0.0), 0, 255)).astype(np.uint8)
        assert np.array_equal(lut.numpy(), want)
    matplotlib = pytest.importorskip("matplotlib")
    want = np.asarray(matplotlib.colormaps["viridis"](np.arange(256))[:, :3], dtype=np.float64)
    assert np.array_equal(table.numpy(), want)


def test_host_composer_edge_rules():
    """The rules the header states beyond the reference's defined range: saturation, NaN -> 0, a depth panel with a NaN or without a range
    is black and leaves its neighbours alone, t = 1 takes the last table entry."""
    color = torch.tensor([-0.5, -0.0, 0.0, 0.999 / 255, 1.2 / 255, 254.7 / 255, 1.0, 1.5, float("nan"), float("inf"), -float("inf"), 0.5])
    color = color.reshape(1, 3, 4).repeat(3, 1, 1)
    want0 = np.array([0, 0, 0, 0, 1, 254, 255, 255, 0, 255, 0, 127], dtype=np.uint8)
    want1 = np.array([0, 0, 0, 1, 1, 255, 255, 255, 0, 255, 0, 128], dtype=np.uint8)
    for quant, want in ((0, want0), (1, want1)):
        got = df.compose_host([(df.COLOR, color, None)], 1, 1, quant=quant)
        assert np.array_equal(got.numpy()[:, :, 0].reshape(-1), want), (quant, got.numpy()[:, :, 0].reshape(-1))
    ramp = (torch.arange(12).float() / 11).reshape(3, 4)
    nan_depth = ramp.clone(); nan_depth[1, 2] = float("nan")
    flat = torch.full((3, 4), 2.5)
    got = df.compose_host([(df.DEPTH, ramp, None), (df.DEPTH, nan_depth, None), (df.DEPTH, flat, None), (df.DEPTH, ramp, None)], 1, 4, quant=0).numpy()
    assert got.shape == (3, 16, 3)
    assert not got[:, 4:12].any()                                              # the NaN panel and the constant panel: black
    assert np.array_equal(got[:, 0:4], got[:, 12:16]) and got[:, 0:4].any()    # the others untouched
    lut = df.lut_u8(0).numpy()
    assert np.array_equal(got[0, 0], lut[0]) and np.array_equal(got[2, 3], lut[255])


def _run(tmp, debug_on, frames=N_FRAMES):
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.renderer import Renderer
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from oracle.raster_ref import RefRasterizer
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device="cpu", height=H, width=W, tracking={"iters": 2}, mapping={"iters": 3, "kf_every": 2, "min_covisibility": 2.0},
                         outputdir=str(tmp), debug={"get_runtime_stats": False, "create_video": debug_on, "save_keyframes": debug_on})
    seq = SyntheticSequence(cfg, frames, 500, seed=5, renderer=Renderer(cfg, rasterizer_cls=RefRasterizer))
    slam = SLAM(cfg, seq, rasterizer_cls=RefRasterizer)
    slam.run()
    return slam, seq


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The same 3-frame 64 x 48 CPU run with both debug keys on and with both off; run once, read by the tests below."""
    on_dir, off_dir = tmp_path_factory.mktemp("debug_on"), tmp_path_factory.mktemp("debug_off")
    on, seq = _run(on_dir, True)
    off, _ = _run(off_dir, False)
    return {"on": on, "off": off, "seq": seq, "on_dir": str(on_dir), "off_dir": str(off_dir)}


def _decode(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_cpu_run_writes_the_video_frames_and_keyframes(runs):
    n = N_FRAMES
    video = sorted(os.listdir(os.path.join(runs["on_dir"], "debug_video")))
    want = ["000000_00000_map.png"] + [f"{2 * i - 1 + k:06d}_{i:05d}_{name}.png" for i in range(1, n) for k, name in enumerate(("track", "map"))]
    assert video == want and len(video) == 2 * n - 1
    for f in video:
        img = _decode(os.path.join(runs["on_dir"], "debug_video", f))
        assert img.shape == (2 * H, 3 * W, 3) and img.dtype == np.uint8
    kf_idx = [kf.idx for kf in runs["on"].mapper.keyframes]
    assert len(kf_idx) >= 2
    assert sorted(os.listdir(os.path.join(runs["on_dir"], "keyframes"))) == [f"{i:05d}.png" for i in kf_idx]
    for i in kf_idx:
        img = _decode(os.path.join(runs["on_dir"], "keyframes", f"{i:05d}.png"))
        color = runs["seq"][i][0]
        assert np.array_equal(img, color.mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy())      # save_image's float32 rule
    # frame 0, "map": the top-left panel is the frame itself, truncated
    img = _decode(os.path.join(runs["on_dir"], "debug_video", video[0]))
    color = runs["seq"][0][0]
    assert np.array_equal(img[:H, :W], np.trunc(color.double().numpy() * 255).astype(np.uint8).transpose(1, 2, 0))
    # frame 0 seeded Gaussians: its third depth panel shows the mask (two values only: the two ends of the table)
    lut = df.lut_u8(0).numpy()
    panel = img[H:, 2 * W:].reshape(-1, 3)
    assert set(map(tuple, np.unique(panel, axis=0))) <= {tuple(lut[0]), tuple(lut[255])}
    # nothing of this without the keys
    assert not os.path.exists(os.path.join(runs["off_dir"], "debug_video")) and not os.path.exists(os.path.join(runs["off_dir"], "keyframes"))


def test_debug_outputs_do_not_change_a_pose(runs):
    a = np.load(os.path.join(runs["on_dir"], "results.npz"), allow_pickle=True)["pose_est"]
    b = np.load(os.path.join(runs["off_dir"], "results.npz"), allow_pickle=True)["pose_est"]
    assert a.shape == (N_FRAMES, 7) and a.tobytes() == b.tobytes()


def test_render_writes_an_image_pair_per_selected_frame(runs):
    slam = runs["off"]
    written = slam.render(every=1)
    folder = os.path.join(runs["off_dir"], "render")
    assert len(written) == 2 * N_FRAMES and sorted(os.listdir(folder)) == sorted(os.path.basename(p) for p in written)
    assert sorted(os.listdir(folder)) == sorted([f"gt{i:05d}.png" for i in range(N_FRAMES)] + [f"render{i:05d}.png" for i in range(N_FRAMES)])
    for p in written:
        assert _decode(p).shape == (2 * H, W, 3)
    color, depth, _ = runs["seq"][1]
    want = df.compose_host([(df.COLOR, color, None), (df.DEPTH, depth, None)], 2, 1, quant=1).numpy()
    assert np.array_equal(_decode(os.path.join(folder, "gt00001.png")), want)
    assert np.array_equal(want[:H], color.mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).numpy())
    assert len(slam.render(every=2)) == 2 * len(range(0, N_FRAMES, 2))


def test_frame_sink_numbers_files_and_never_reuses_a_slot_early(tmp_path):
    sink = df.FrameSink(str(tmp_path / "frames"))
    frames = [torch.full((5, 7, 3), 10 * k, dtype=torch.uint8) for k in range(6)]
    for k, f in enumerate(frames):
        f[0, 0, 0] = k
        sink.put(f, 3 * k, "map")
    sink.close()
    sink.close()                                             # idempotent
    files = sorted(os.listdir(tmp_path / "frames"))
    assert files == [f"{k:06d}_{3 * k:05d}_map.png" for k in range(6)]
    for k, name in enumerate(files):
        assert np.array_equal(_decode(tmp_path / "frames" / name), frames[k].numpy())
    with pytest.raises(RuntimeError):
        sink.put(frames[0], 0, "map")


def test_library_exports_the_mosaic_entry_points():
    from mm3dgs_slam_amd import _lib
    assert {"mm3dgs_mosaic", "mm3dgs_mosaic_work_bytes"} <= set(_lib.exported_symbols())
    lib = C.CDLL(_lib.LIB_PATH)                              # (no device is touched: the size query is host arithmetic)
    fn = lib.mm3dgs_mosaic_work_bytes
    fn.restype, fn.argtypes = C.c_size_t, [C.c_int] * 4
    assert hasattr(lib, "mm3dgs_mosaic")
    for shape in ((480, 640, 2, 3), (1, 1, 1, 1), (33, 130, 2, 1), (7, 5, 1, 8)):
        n = fn(*shape)
        assert n > 0 and n % 8 == 0, shape
    for shape in ((0, 640, 2, 3), (480, -1, 2, 3), (480, 640, 3, 3), (480, 640, 0, 1), (1 << 14, 1 << 14, 1, 2)):
        assert fn(*shape) == 0, shape
