"""mm3dgs_ingest_frame (csrc/ingest.hip) against the host path (dataset.ingest_host), and RecordedSequence on the GPU.

Bars (include/mm3dgs.h): depth bit-exact at every shape; colour bit-exact wherever Ws / W and Hs / H are integers (the bilinear weights
are 0 or 0.5, the blend is exact, only the correctly rounded division by 255 rounds), 1e-6 elsewhere (fewer than eight float32
roundings of at most 6e-8 each on values of at most 1)."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (source, output, colour is bit-exact)
SHAPES = [((5, 7), (5, 7), True),           # odd width, unaligned rows: scalar path
          ((8, 12), (8, 12), True),         # packed path
          ((37, 67), (37, 67), True),       # more than one workgroup, with a tail
          ((6, 8), (3, 4), True),
          ((66, 128), (33, 64), True),      # UT-MM's exact 2x
          ((12, 12), (4, 4), True),         # odd integer ratio
          ((7, 9), (5, 4), False),
          ((4, 5), (6, 10), False)]         # upscale, both borders clamp
SCALES = (5000.0, 1000.0)


def raw_frame(Hs, Ws, seed=0):
    g = torch.Generator().manual_seed(1000 * Hs + Ws + seed)
    rgb = torch.randint(0, 256, (Hs, Ws, 3), generator=g, dtype=torch.uint8).numpy()
    depth = torch.randint(0, 65536, (Hs, Ws), generator=g).numpy().astype(np.uint16)
    rgb[0, 0], rgb[0, 1], rgb[-1, -1], rgb[-1, 0] = 0, 255, 255, 0
    depth[0, 0], depth[0, 1], depth[0, 2], depth[-1, -1], depth[-1, 0] = 0, 1, 65535, 65535, 0
    return rgb, depth


@pytest.fixture(scope="module")
def cases():
    """Inputs and the host path's outputs, computed once and left unchanged."""
    from mm3dgs_slam_amd import dataset as ds
    out = {}
    for src, dst, _ in SHAPES:
        rgb, depth = raw_frame(*src)
        host = {s: ds.ingest_host(rgb, depth, s, dst[0], dst[1], DEV) for s in SCALES}
        out[(src, dst)] = (rgb, depth, host)
    return out


def dev_i16(depth):
    return torch.from_numpy(depth.view(np.int16).copy()).to(DEV)


def call(Hs, Ws, rgb_ptr, depth_ptr, scale, H, W, color_ptr, out_depth_ptr):
    from mm3dgs_slam_amd import _lib
    from mm3dgs_slam_amd.rasterizer import _stream
    p = lambda v: None if v is None else C.c_void_p(v)
    return _lib.load().mm3dgs_ingest_frame(Hs, Ws, p(rgb_ptr), p(depth_ptr), float(scale), H, W, p(color_ptr), p(out_depth_ptr), _stream())


def compare(color, depth, host_color, host_depth, exact, what):
    err = float((color.double() - host_color.double()).abs().max())
    print(f"{what}: colour max |kernel - host| = {err:.3e}, equal bits {torch.equal(color, host_color)}; depth equal bits "
          f"{None if depth is None else torch.equal(depth, host_depth)}")
    if depth is not None:
        assert torch.equal(depth, host_depth), what
    if exact:
        assert torch.equal(color, host_color), what
    else:
        assert err <= 1e-6, what
    assert float(color.min()) >= 0.0 and float(color.max()) <= 1.0


@pytest.mark.parametrize("src,dst,exact", SHAPES)
def test_kernel_matches_the_host_path(cases, src, dst, exact):
    from mm3dgs_slam_amd import dataset as ds
    rgb, depth, host = cases[(src, dst)]
    rgb_d, depth_d = torch.from_numpy(rgb).to(DEV), dev_i16(depth)
    for s in SCALES:
        color, d = ds.ingest_device(rgb_d, depth_d, s, dst[0], dst[1])
        assert color.shape == (3, *dst) and d.shape == dst and color.dtype == d.dtype == torch.float32
        compare(color, d, host[s][0], host[s][1], exact, f"{src}->{dst} scale {s}")
        zero = torch.from_numpy(depth.astype(np.int64) == 0)
        if src == dst:
            assert bool((d.cpu()[zero] == 0).all()) and int(zero.sum()) >= 2      # zero stays zero
            planted = color[:, 0, :2].cpu()
            assert bool((planted[:, 0] == 0).all()) and bool((planted[:, 1] == 1).all())      # 0 -> 0.0, 255 -> exactly 1.0


@pytest.mark.parametrize("src,dst,exact", [SHAPES[1], SHAPES[3], SHAPES[6]])
def test_source_pointer_offset_by_one_byte(cases, src, dst, exact):
    """rgb one byte into a larger buffer: the kernel assumes no alignment of the source (the packed path must not be taken)."""
    rgb, depth, host = cases[(src, dst)]
    n = rgb.size
    buf = torch.full((n + 16,), 0xAB, dtype=torch.uint8, device=DEV)
    buf[1:1 + n] = torch.from_numpy(rgb.reshape(-1)).to(DEV)
    depth_d = dev_i16(depth)
    color = torch.empty(3, *dst, device=DEV)
    d = torch.empty(*dst, device=DEV)
    assert buf.data_ptr() % 4 == 0
    assert call(src[0], src[1], buf.data_ptr() + 1, depth_d.data_ptr(), 5000.0, dst[0], dst[1], color.data_ptr(), d.data_ptr()) == 0
    compare(color, d, host[5000.0][0], host[5000.0][1], exact, f"offset {src}->{dst}")


@pytest.mark.parametrize("src,dst,exact", [SHAPES[0], SHAPES[1], SHAPES[6]])
def test_colour_only_call(cases, src, dst, exact):
    from mm3dgs_slam_amd import dataset as ds
    rgb, _, host = cases[(src, dst)]
    color, d = ds.ingest_device(torch.from_numpy(rgb).to(DEV), None, 5000.0, dst[0], dst[1])
    assert d is None
    compare(color, None, host[5000.0][0], None, exact, f"colour only {src}->{dst}")


def test_rejected_calls_return_minus_one_and_write_nothing(cases):
    """Argument checks, not faults: every pointer handed over is valid or NULL."""
    from mm3dgs_slam_amd import _lib
    src, dst = (8, 12), (8, 12)
    rgb, depth, _ = cases[(src, dst)]
    rgb_d, depth_d = torch.from_numpy(rgb).to(DEV), dev_i16(depth)
    color = torch.full((3, *dst), -7.0, device=DEV)
    d = torch.full(dst, -7.0, device=DEV)
    a = dict(Hs=8, Ws=12, rgb_ptr=rgb_d.data_ptr(), depth_ptr=depth_d.data_ptr(), scale=5000.0, H=8, W=12, color_ptr=color.data_ptr(),
             out_depth_ptr=d.data_ptr())
    bad = [dict(a, Hs=0), dict(a, Ws=0), dict(a, H=0), dict(a, W=0), dict(a, H=-3),      # zero / negative sizes
           dict(a, out_depth_ptr=None),                                               # a depth pointer without its output
           dict(a, depth_ptr=None),                                                   # an output without its pointer
           dict(a, scale=0.0), dict(a, scale=-1.0), dict(a, scale=float("nan")), dict(a, scale=float("inf")),
           dict(a, rgb_ptr=None), dict(a, color_ptr=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"ingest_frame" in _lib.load().mm3dgs_last_error()
    torch.cuda.synchronize()
    assert bool((color == -7.0).all()) and bool((d == -7.0).all())
    assert call(**a) == 0      # and the same arguments, untouched, are accepted
    torch.cuda.synchronize()
    assert bool((color != -7.0).all()) and bool((d != -7.0).all())


def _write_golden_scene(tmp_path, kind="tum"):
    from tests.test_dataset import make_cfg, write_scene
    write_scene(tmp_path, kind)
    return make_cfg


def test_staging_slots_are_not_overwritten_while_a_frame_is_in_flight(tmp_path):
    """Five frames fetched back to back without synchronising (two staging slots, prefetch on), then compared with the host path."""
    from mm3dgs_slam_amd import dataset as ds
    make_cfg = _write_golden_scene(tmp_path)
    dev_seq = ds.RecordedSequence(make_cfg(tmp_path, "tum", device=DEV, ingest_on_device=True, prefetch=True))
    host_seq = ds.RecordedSequence(make_cfg(tmp_path, "tum", device=DEV, ingest_on_device=False, prefetch=False))
    assert dev_seq.on_device and not host_seq.on_device and dev_seq.H == 12 and dev_seq.W == 16
    got = [dev_seq[i] for i in range(5)]
    torch.cuda.synchronize()
    for i, (color, depth, pose) in enumerate(got):
        hc, hd, hp = host_seq[i]
        assert torch.equal(color, hc) and torch.equal(depth, hd) and torch.equal(pose, hp), i
    assert not torch.equal(got[0][0], got[1][0])
    dev_seq.close(); host_seq.close()


def test_slam_over_a_recorded_sequence_host_and_device_ingest_agree(tmp_path):
    """Three 64x48 frames of a synthetic scene, quantised and written as a TUM directory.  At native size the two ingest paths give the
    same bits, so the runs must too: bit-identical poses, the same number of Gaussians; results.npz has the reference's keys."""
    from mm3dgs_slam_amd import dataset as ds
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    H, W = 48, 64
    base = lambda **kw: default_config(device=DEV, height=H, width=W, tracking={"iters": 4}, mapping={"iters": 5, "kf_every": 1}, **kw)
    src = SyntheticSequence(base(), 3, 2000, seed=3)
    frames = [ds.quantise_frame(c, d, 5000.0) for c, d in src.frames]
    folder = tmp_path / "rec" / "scene"
    ds.write_tum_sequence(str(folder), frames, src.poses, [100.0 + 0.1 * i for i in range(3)])
    runs = {}
    for on_device in (False, True):
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        cfg = base(dataset="tum", inputdir=str(tmp_path / "rec"), scene="scene", ingest_on_device=on_device,
                   outputdir=str(tmp_path / f"out{int(on_device)}"))
        cfg["cam"].update(image_height=H, image_width=W)
        seq = ds.RecordedSequence(cfg)
        assert len(seq) == 3 and seq.on_device is on_device
        slam = SLAM(cfg, seq)
        assert type(slam.tracker).__name__ == "FusedTracker" and type(slam.mapper).__name__ == "FusedMapper"
        slam.run()
        runs[on_device] = (torch.stack([p.detach() for p in slam.estimate_pose_list]).cpu(), int(slam.gaussians.get_xyz.shape[0]),
                           [t.clone() for t in seq[1][:2]], cfg["outputdir"])
        seq.close()
    (pose_h, n_h, img_h, _), (pose_d, n_d, img_d, out_d) = runs[False], runs[True]
    assert torch.equal(img_h[0], img_d[0]) and torch.equal(img_h[1], img_d[1])
    rgb1, d1 = frames[1]
    assert torch.equal(img_d[0].cpu(), torch.from_numpy(rgb1).permute(2, 0, 1).float() / torch.tensor(255.0))
    print("pose difference host / device ingest:", float((pose_h - pose_d).abs().max()), "Gaussians", n_h, n_d)
    assert torch.equal(pose_h, pose_d) and n_h == n_d and n_h > 0
    res = np.load(os.path.join(out_d, "results.npz"), allow_pickle=True)
    assert {"pose_est", "pose_gt", "keyframes", "ate_rmse", "psnr_list", "ssim_list", "lpips_list"} <= set(res.files)
    assert res["pose_est"].shape == (3, 7) and res["pose_gt"].shape == (3, 7) and np.isfinite(float(res["ate_rmse"]))
    assert os.path.isfile(os.path.join(out_d, "point_cloud", "iteration_3", "point_cloud.ply"))
