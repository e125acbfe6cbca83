"""Monocular depth estimates of a recorded sequence read from disk (config key est_depth_dir), host side: dataset.ingest_est_host against
torch's own F.interpolate (the step of the reference's MiDaS.estimate_depth that is reproduced), the loader, and a monocular SLAM run on
the CPU over a recorded directory.  Every test here fails without the feature (no ingest_est_host, no est on a RecordedSequence)."""
import os
import random

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import dataset as ds
from tests.est_depth_cases import CASES, DTYPES, SHAPES, source
from tests.test_dataset import G, H, W, make_cfg, write_scene

EPS32 = float(torch.finfo(torch.float32).eps)


@pytest.mark.parametrize("src,dst,same", SHAPES)
def test_host_path_is_torchs_bilinear_interpolation(src, dst, same):
    """Before the single rounding: 1e-12 x max|source| (about eight float64 roundings of 1.1e-16 each, with wide margin).  After it:
    one float32 ulp of the largest value, finfo(float32).eps x max|source| x scale."""
    for dtype, scale in CASES:
        raw = source(*src, dtype)
        as_double = torch.from_numpy(raw.astype(np.float64))
        peak = float(as_double.abs().max())
        ref = torch.nn.functional.interpolate(as_double[None, None], size=dst, mode="bilinear", align_corners=False)[0, 0]
        wide = ds.resize_est_host(raw, *dst)
        got = ds.ingest_est_host(raw, scale, *dst)
        e64 = float((wide - ref).abs().max())
        e32 = float((got.double() - (ref * scale).float().double()).abs().max())
        print(f"{src}->{dst} {np.dtype(dtype).name} scale {scale}: float64 error {e64:.3e} (bar {1e-12 * peak:.3e}), float32 error {e32:.3e} "
              f"(bar {EPS32 * peak * scale:.3e})")
        assert wide.dtype == torch.float64 and got.dtype == torch.float32 and tuple(got.shape) == dst and got.device.type == "cpu"
        assert e64 <= 1e-12 * peak
        assert e32 <= EPS32 * peak * scale


@pytest.mark.parametrize("src,dst,same", [s for s in SHAPES if s[2]])
def test_equal_sizes_return_the_source_values_bit_for_bit(src, dst, same):
    for dtype, scale in CASES:
        raw = source(*src, dtype)
        got = ds.ingest_est_host(raw, scale, *dst).numpy()
        want = (raw.astype(np.float64) * scale).astype(np.float32)      # (float)((double)v * s)
        assert np.array_equal(got, want), (dtype, scale)
        if scale == 1.0 and dtype != np.uint16:
            assert np.array_equal(got.astype(dtype), raw)
    raw = source(*src, np.float32)
    out = ds.ingest_est_host(raw, 1.0, *dst)
    out += 1.0                                                           # a fresh tensor: the source is not aliased
    assert np.array_equal(raw, source(*src, np.float32))


def test_host_path_refuses_other_arrays():
    for bad in (np.zeros((4, 5), np.float64), np.zeros((2, 4, 5), np.float32), np.zeros((4, 5), np.uint8)):
        with pytest.raises(ValueError, match="depth estimate"):
            ds.ingest_est_host(bad, 1.0, 4, 5)


# ---- loader ------------------------------------------------------------------------------------------------------------------------------
EST_SHAPE = (9, 14)      # another resolution than the 12 x 16 frames


def est_array(n, dtype=np.float32, shape=EST_SHAPE):
    return source(*shape, dtype, seed=50 + n)


def write_estimates(scene, kind, dtype=np.float32, ext=".npy", folder="est_depth", shape=EST_SHAPE):
    """One estimate per colour image of the fixture scene, named by the colour image's stem.  Returns {stem: array}."""
    from PIL import Image
    os.makedirs(os.path.join(scene, folder), exist_ok=True)
    out = {}
    for n, name in enumerate(G[f"{kind}/names_c"]):
        stem = os.path.splitext(os.path.basename(str(name)))[0]
        out[stem] = est_array(n, dtype, shape)
        path = os.path.join(scene, folder, stem + ext)
        if ext == ".npy":
            np.save(path, out[stem])
        else:
            Image.fromarray(out[stem]).save(path)
    return out


def stem_of(path):
    return os.path.splitext(os.path.basename(path))[0]


@pytest.fixture(scope="module")
def est_scenes(tmp_path_factory):
    out = {}
    for kind in ("tum", "utmm"):
        root = tmp_path_factory.mktemp("est_" + kind)
        scene = write_scene(root, kind)
        out[kind] = (root, write_estimates(scene, kind))
    return out


@pytest.mark.parametrize("kind", ["tum", "utmm"])
@pytest.mark.parametrize("sl", [(0, 1, -1), (1, 2, -1), (2, 1, 5), (0, 3, -1)])
def test_estimates_stay_in_step_with_the_kept_frames(est_scenes, kind, sl):
    root, ests = est_scenes[kind]
    seq = ds.RecordedSequence(make_cfg(root, kind, *sl, est_depth_dir="est_depth", prefetch=False))
    assert len(seq.est_paths) == len(seq) == len(seq.color_paths) and len(seq) >= 2
    for i in range(len(seq)):
        assert stem_of(seq.est_paths[i]) == stem_of(seq.color_paths[i])
        got = seq.est(i)
        assert got.dtype == torch.float32 and tuple(got.shape) == (H, W)
        assert torch.equal(got, ds.ingest_est_host(ests[stem_of(seq.color_paths[i])], 1.0, H, W)), i
    capped = ds.RecordedSequence(make_cfg(root, kind, *sl, est_depth_dir="est_depth", prefetch=False), frames=2)
    assert len(capped.est_paths) == 2 and capped.est_paths == seq.est_paths[:2]
    seq.close(); capped.close()


def test_without_the_key_a_recorded_sequence_has_no_est(est_scenes):
    root, _ = est_scenes["tum"]
    for extra in ({}, {"est_depth_dir": ""}, {"est_depth_dir": None}):
        seq = ds.RecordedSequence(make_cfg(root, "tum", **extra))
        assert not hasattr(seq, "est")
        seq.close()
    assert not hasattr(ds.RecordedSequence, "est")
    seq = ds.RecordedSequence(make_cfg(root, "tum", est_depth_dir="est_depth"))
    assert hasattr(seq, "est")
    seq.close()


@pytest.mark.parametrize("kind", ["tum", "utmm"])
def test_any_access_order_with_and_without_prefetch_gives_the_same_tensors(est_scenes, kind):
    root, ests = est_scenes[kind]
    want = lambda seq, i: ds.ingest_est_host(ests[stem_of(seq.color_paths[i])], 1.0, H, W)
    got = {}
    for prefetch in (False, True):
        seq = ds.RecordedSequence(make_cfg(root, kind, est_depth_dir="est_depth", prefetch=prefetch))
        out = []
        for i in (0, 1, 2):                         # the order of SLAM.step: the frame, then its estimate
            frame = seq[i]
            out.append((i, frame[0].clone(), seq.est(i)))
        for i in (4, 0, 3):                         # the estimate alone
            out.append((i, None, seq.est(i)))
        for i in (3, 2, 1, 0):                      # backwards, as evaluate_images goes; estimate first, twice, then the frame
            a, b = seq.est(i), seq.est(i)
            assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()
            out.append((i, seq[i][0].clone(), a))
        i = 2
        frame = seq[i]; seq.est(4)                   # an estimate of another frame in between does not disturb the next frame
        out.append((3, seq[3][0].clone(), seq.est(3)))
        for i, _, e in out:
            assert torch.equal(e, want(seq, i)), (prefetch, i)
        got[prefetch] = out
        seq.close()
    plain = ds.RecordedSequence(make_cfg(root, kind, prefetch=False))
    for (i, ca, ea), (j, cb, eb) in zip(got[False], got[True]):
        assert i == j and torch.equal(ea, eb) and (ca is None or (torch.equal(ca, cb) and torch.equal(ca, plain[i][0])))
    plain.close()


def test_seq_then_est_costs_no_second_decode(est_scenes):
    root, _ = est_scenes["tum"]
    calls = []

    def counting(path):
        calls.append(path)
        return ds.decode_est(path)

    seq = ds.RecordedSequence(make_cfg(root, "tum", est_depth_dir="est_depth", prefetch=False), est_decoder=counting)
    calls.clear()                                    # (the constructor reads the first file to size the staging buffers)
    for i in range(3):
        seq[i]
        seq.est(i)
    assert calls == seq.est_paths[:3]
    seq.close()


def test_png_estimates_are_scaled_integers_and_npy_wins_over_png(tmp_path):
    scene = write_scene(tmp_path, "tum")
    ests = write_estimates(scene, "tum", np.uint16, ".png")
    cfg = make_cfg(tmp_path, "tum", est_depth_dir="est_depth", prefetch=False)
    cfg["cam"]["est_depth_scale"] = 0.25
    seq = ds.RecordedSequence(cfg)
    assert all(p.endswith(".png") for p in seq.est_paths)
    for i in (0, 2):
        assert torch.equal(seq.est(i), ds.ingest_est_host(ests[stem_of(seq.color_paths[i])], 0.25, H, W))
    seq.close()
    half = write_estimates(scene, "tum", np.float16, ".npy")      # now both exist: .npy first, used as it is (no scale)
    seq = ds.RecordedSequence(cfg)
    assert all(p.endswith(".npy") for p in seq.est_paths)
    assert torch.equal(seq.est(1), ds.ingest_est_host(half[stem_of(seq.color_paths[1])], 1.0, H, W))
    seq.close()


def test_bad_estimate_files_raise_with_the_file_named(tmp_path):
    from PIL import Image
    names = [os.path.splitext(os.path.basename(str(n)))[0] for n in G["tum/0/color_names"]]
    esc = lambda s: s.replace(".", r"\.")

    def scene_with(sub):
        scene = write_scene(tmp_path / sub, "tum")
        write_estimates(scene, "tum")
        return scene, make_cfg(tmp_path / sub, "tum", est_depth_dir="est_depth", prefetch=False)

    # a missing file of a LATER kept frame: in the constructor
    scene, cfg = scene_with("missing")
    os.remove(os.path.join(scene, "est_depth", names[3] + ".npy"))
    with pytest.raises(ValueError, match=esc(names[3])):
        ds.RecordedSequence(cfg)
    ds.RecordedSequence(dict(cfg, early_stop_idx=3)).close()      # ... of a frame that is not kept: no error
    # float64, 3-D, another shape, another dtype: when that frame is decoded (frame 1), or in the constructor (frame 0)
    bad = {"float64": np.zeros(EST_SHAPE, np.float64), "three_d": np.zeros((1, *EST_SHAPE), np.float32),
           "shape": np.zeros((EST_SHAPE[0] + 1, EST_SHAPE[1]), np.float32), "dtype": np.zeros(EST_SHAPE, np.float16),
           "fortran": np.asfortranarray(est_array(0))}
    for sub, arr in bad.items():
        scene, cfg = scene_with(sub)
        np.save(os.path.join(scene, "est_depth", names[1] + ".npy"), arr)
        seq = ds.RecordedSequence(cfg)
        seq[0], seq.est(0)
        with pytest.raises(ValueError, match=esc(names[1])):
            seq.est(1)
        with pytest.raises(ValueError, match=esc(names[1])):
            seq[1]
        seq.close()
        if sub in ("float64", "three_d", "fortran"):
            np.save(os.path.join(scene, "est_depth", names[0] + ".npy"), arr)
            with pytest.raises(ValueError, match=esc(names[0])):
                ds.RecordedSequence(cfg)
    # an 8-bit PNG
    scene = write_scene(tmp_path / "png8", "tum")
    write_estimates(scene, "tum", np.uint16, ".png")
    Image.fromarray(np.zeros(EST_SHAPE, np.uint8)).save(os.path.join(scene, "est_depth", names[1] + ".png"))
    seq = ds.RecordedSequence(make_cfg(tmp_path / "png8", "tum", est_depth_dir="est_depth", prefetch=False))
    with pytest.raises(ValueError, match=esc(names[1])):
        seq.est(1)
    seq.close()


def test_write_tum_sequence_round_trips_estimates(tmp_path):
    g = torch.Generator().manual_seed(3)
    frames = [(torch.randint(0, 256, (6, 8, 3), generator=g, dtype=torch.uint8).numpy(),
               torch.randint(1, 65536, (6, 8), generator=g).numpy().astype(np.uint16)) for _ in range(3)]
    poses = [torch.tensor([1.0, 0, 0, 0, 0.01 * i, 0, 0]) for i in range(3)]
    stamps = [10.0 + 0.1 * i for i in range(3)]
    ests = [source(5, 7, np.float16, seed=i) for i in range(2)] + [torch.from_numpy(source(5, 7, np.float16, seed=2))]
    ds.write_tum_sequence(str(tmp_path / "with" / "scene"), frames, poses, stamps, est=ests)
    ds.write_tum_sequence(str(tmp_path / "without" / "scene"), frames, poses, stamps)
    assert not os.path.exists(tmp_path / "without" / "scene" / "est_depth")      # the default leaves the output as it was
    assert sorted(os.listdir(tmp_path / "with" / "scene" / "est_depth")) == ["0000.npy", "0001.npy", "0002.npy"]
    cam = {"image_height": 6, "image_width": 8, "fx": 10.0, "fy": 10.0, "cx": 4.0, "cy": 3.0, "png_depth_scale": 5000.0}
    cfg = {"dataset": "tum", "device": "cpu", "inputdir": str(tmp_path / "with"), "scene": "scene", "desired_height": 6, "desired_width": 8,
           "cam": cam, "ingest_on_device": False, "est_depth_dir": "est_depth"}
    seq = ds.RecordedSequence(cfg)
    assert len(seq) == 3
    for i in range(3):
        assert torch.equal(seq.est(i), ds.ingest_est_host(np.asarray(ests[i]), 1.0, 6, 8))
    seq.close()
    with pytest.raises(ValueError, match="estimates"):
        ds.write_tum_sequence(str(tmp_path / "short" / "scene"), frames, poses, stamps, est=ests[:2])


def test_library_binding_declares_the_estimate_entry_point():
    from mm3dgs_slam_amd import _lib
    assert "mm3dgs_ingest_est" in _lib.exported_symbols()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    assert hasattr(_lib.load(), "mm3dgs_ingest_est")
    with pytest.raises(ValueError, match="GPU"):
        ds.ingest_est_device(torch.zeros(4, 5), 1.0, 4, 5)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_monocular_slam_over_a_recorded_directory_on_the_cpu(tmp_path):
    """The setup of test_slam_cpu.py's monocular test: a SyntheticSequence's frames (quantised) and its est(i) arrays (float32 .npy at
    native size: they come back bit for bit) recorded as a TUM directory.  A RecordedSequence with est_depth_dir runs the monocular path
    exactly like one that is handed the same arrays from memory."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.renderer import Renderer
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from oracle.raster_ref import RefRasterizer
    Hh, Ww = 32, 48
    base = lambda **kw: default_config(device="cpu", height=Hh, width=Ww, use_gt_depth=False, tracking={"iters": 3},
                                       mapping={"iters": 4, "kf_every": 1, "min_covisibility": 2.0}, **kw)
    cfg0 = base()
    src = SyntheticSequence(cfg0, 3, 600, seed=5, renderer=Renderer(cfg0, rasterizer_cls=RefRasterizer))
    ests = [src.est(i).clone() for i in range(3)]
    scale = float(cfg0["cam"]["png_depth_scale"])
    ds.write_tum_sequence(str(tmp_path / "rec" / "scene"), [ds.quantise_frame(c, d, scale) for c, d in src.frames], src.poses,
                          [100.0 + 0.1 * i for i in range(3)], est=ests)
    runs = {}
    for from_disk in (True, False):
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        cfg = base(dataset="tum", inputdir=str(tmp_path / "rec"), scene="scene", ingest_on_device=False)
        cfg["cam"].update(image_height=Hh, image_width=Ww)
        if from_disk:
            cfg["est_depth_dir"] = "est_depth"
        seq = ds.RecordedSequence(cfg)
        if from_disk:
            assert all(torch.equal(seq.est(i), ests[i]) for i in range(3))
        else:
            assert not hasattr(seq, "est")
            seq.est = lambda i: ests[i].clone()
        slam = SLAM(cfg, seq, rasterizer_cls=RefRasterizer)
        seen, real = [], slam.mapper.run_frame
        slam.mapper.run_frame = lambda idx, color, depth, est_scaled, *a, **k: (seen.append(est_scaled.clone()), real(idx, color, depth, est_scaled, *a, **k))[1]
        for i in range(3):
            slam.step(i)
        runs[from_disk] = (torch.stack([p.detach() for p in slam.estimate_pose_list]), int(slam.gaussians.get_xyz.shape[0]), seen)
        seq.close()
    (pose_a, n_a, seen_a), (pose_b, n_b, seen_b) = runs[True], runs[False]
    assert torch.equal(pose_a, pose_b) and n_a == n_b and n_a > 0
    # the monocular path really ran: frame 0 takes the reference's first-frame scale of the raw estimate, 1 / (est + 0.001) * png_depth_scale / 10
    assert torch.equal(seen_a[0], 1.0 / (ests[0] + 0.001) * scale / 10)
    assert all(torch.equal(a, b) for a, b in zip(seen_a, seen_b)) and len(seen_a) == 3
