"""RecordedSequence on the CPU against tests/golden/g13_dataset.npz (the reference's TUMDataset / UTMMDataset run on two tiny generated
directories, tests/golden/make_golden_dataset.py): the directories are rebuilt in tmp_path from the stored list-file texts and image
arrays, and every product of the loader is compared with what the reference returned."""
import os

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import dataset as ds

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "g13_dataset.npz"))
SLICES = [tuple(int(v) for v in row) for row in G["slices"]]
CAM = {str(k): float(v) for k, v in zip(G["cam_keys"], G["cam_values"])}
H, W = int(CAM["image_height"]), int(CAM["image_width"])


def write_scene(root, kind, texts=None, skip=()):
    from PIL import Image
    scene = os.path.join(str(root), "scene")
    os.makedirs(os.path.join(scene, "rgb"), exist_ok=True)
    os.makedirs(os.path.join(scene, "depth"), exist_ok=True)
    for key in G.files:
        if key.startswith(f"{kind}/file/"):
            name = key.split("/")[-1]
            with open(os.path.join(scene, name), "w") as f:
                f.write((texts or {}).get(name, str(G[key])))
    for n, (c, d) in enumerate(zip(G[f"{kind}/colors"], G[f"{kind}/depths"])):
        Image.fromarray(c, "RGB").save(os.path.join(scene, str(G[f"{kind}/names_c"][n])))
        Image.fromarray(d).save(os.path.join(scene, str(G[f"{kind}/names_d"][n])))
    return scene


def make_cfg(root, kind, start=0, stride=1, end=-1, **extra):
    cam = dict(CAM, image_height=H, image_width=W, png_depth_scale=5000.0 if kind == "tum" else 1000.0)
    cfg = {"dataset": kind, "device": "cpu", "inputdir": str(root), "scene": "scene", "start_idx": start, "stride": stride,
           "desired_height": H, "desired_width": W, "cam": cam, "ingest_on_device": False}
    if end != -1:
        cfg["early_stop_idx"] = end
    cfg.update(extra)
    return cfg


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    root = {kind: tmp_path_factory.mktemp(kind) for kind in ("tum", "utmm")}
    for kind in root:
        write_scene(root[kind], kind)
    return root


@pytest.mark.parametrize("kind", ["tum", "utmm"])
@pytest.mark.parametrize("s", range(len(SLICES)))
def test_loader_matches_the_reference(scenes, kind, s):
    start, stride, end = SLICES[s]
    cfg = make_cfg(scenes[kind], kind, start, stride, end)
    seq = ds.RecordedSequence(cfg)
    pre = f"{kind}/{s}/"
    rel = lambda paths: [os.path.relpath(p, seq.folder) for p in paths]
    assert rel(seq.color_paths) == [str(v) for v in G[pre + "color_names"]]      # names and order: exact
    assert rel(seq.depth_paths) == [str(v) for v in G[pre + "depth_names"]]
    assert len(seq) == len(G[pre + "color_names"]) == len(seq.poses)
    assert np.array_equal(seq.rel_c2w.numpy(), G[pre + "rel_poses"]) and seq.rel_c2w.dtype == torch.float32
    pose7 = torch.stack(seq.poses).numpy()
    assert np.abs(pose7 - G[pre + "pose7"]).max() <= 1e-6
    K = G[pre + "intrinsics"]
    assert np.array_equal(seq.intrinsics.numpy(), np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], dtype=np.float32))
    for i in range(len(seq)):
        color, depth, pose = seq[i]
        assert color.dtype == depth.dtype == torch.float32 and color.shape == (3, H, W) and depth.shape == (H, W)
        want_c = np.transpose(G[pre + "color"][i], (2, 0, 1)) / np.float32(255.0)      # slam/SLAM.py:388-390, the correctly rounded division
        assert want_c.dtype == np.float32 and np.array_equal(color.numpy(), want_c)
        assert np.array_equal(depth.numpy(), G[pre + "depth"][i][..., 0])
        assert torch.equal(pose, seq.poses[i])
    if kind == "utmm":
        assert np.array_equal(np.array(seq.tstamps, dtype=np.float64), G[pre + "tstamps"])
        assert [int(m.shape[0]) for m in seq.imus] == [int(v) for v in G[pre + "imu_counts"]]
        assert np.array_equal(torch.cat(seq.imus, 0).numpy(), G[pre + "imu_rows"])
        assert np.array_equal(torch.cat([seq.imu(i) for i in range(len(seq))], 0).numpy(), G[pre + "imu_item"])
        assert len(set(int(v) for v in G[pre + "imu_counts"])) > 1                   # the fixture's intervals are uneven
        assert np.array_equal(seq.tf["c2i"].numpy(), G[pre + "c2i"]) and seq.tf["c2i"].dtype == torch.float32
    else:
        assert len(seq.tstamps) == len(seq)
        with pytest.raises(ValueError, match="no IMU"):
            seq.imu(1)
    seq.close()


@pytest.mark.parametrize("kind", ["tum", "utmm"])
def test_scaled_intrinsics_are_written_back_as_python_floats(scenes, kind, monkeypatch):
    """datautils.scale_intrinsics at a 5x7 target; no frame is fetched (the reference's cv2 stub cannot resize)."""
    cfg = make_cfg(scenes[kind], kind, desired_height=5, desired_width=7)
    seq = ds.RecordedSequence(cfg)
    K = G[f"{kind}/intrinsics_5x7"]
    want = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
    got = [cfg["cam"][k] for k in ("fx", "fy", "cx", "cy")]
    assert all(type(v) is float for v in got)
    assert np.array_equal(np.array(got, dtype=np.float32), np.array(want, dtype=np.float32)) and got == [float(v) for v in want]
    seq.close()


@pytest.fixture(scope="module")
def resize_inputs():
    g = torch.Generator().manual_seed(7)
    out = {}
    for (Hs, Ws) in ((6, 8), (7, 9), (4, 5)):
        rgb = torch.randint(0, 256, (Hs, Ws, 3), generator=g, dtype=torch.uint8).numpy()
        depth = torch.randint(0, 65536, (Hs, Ws), generator=g).numpy().astype(np.uint16)
        rgb[0, 0], rgb[-1, -1] = 0, 255
        depth[0, 0], depth[0, 1], depth[-1, -1] = 0, 1, 65535
        out[(Hs, Ws)] = (rgb, depth)
    return out


@pytest.mark.parametrize("src,dst", [((6, 8), (3, 4)), ((7, 9), (5, 4)), ((4, 5), (6, 10))])
def test_host_resize_against_an_independent_float64_reference(resize_inputs, src, dst):
    """Colour against torch's own bilinear interpolation (align_corners=False: the same half-pixel rule, written independently) in
    float64, at 1e-6 on [0,1]; depth against nearest indices written out in plain Python."""
    rgb, depth = resize_inputs[src]
    (Hs, Ws), (Ho, Wo) = src, dst
    color, d = ds.ingest_host(rgb, depth, 5000.0, Ho, Wo)
    ref = torch.nn.functional.interpolate(torch.from_numpy(rgb).double().permute(2, 0, 1)[None], size=(Ho, Wo), mode="bilinear",
                                          align_corners=False)[0] / 255.0
    err = float((color.double() - ref).abs().max())
    print(f"{src}->{dst}: colour max error {err:.3e}")
    assert color.dtype == torch.float32 and color.shape == (3, Ho, Wo) and err <= 1e-6
    want = np.empty((Ho, Wo), dtype=np.float32)
    for y in range(Ho):
        for x in range(Wo):
            ys, xs = min(int(np.floor(y * (Hs / Ho))), Hs - 1), min(int(np.floor(x * (Ws / Wo))), Ws - 1)
            want[y, x] = np.float32(np.float64(depth[ys, xs]) / 5000.0)
    assert d.dtype == torch.float32 and np.array_equal(d.numpy(), want)


def test_prefetch_on_and_off_give_identical_frames(scenes):
    order = (0, 1, 2, 5, 0, 3)
    got = {}
    for prefetch in (False, True):
        seq = ds.RecordedSequence(make_cfg(scenes["utmm"], "utmm", prefetch=prefetch))
        assert (seq._pool is not None) == prefetch
        got[prefetch] = [tuple(t.clone() for t in seq[i]) for i in order]
        seq.close()
    for a, b, i in zip(got[False], got[True], order):
        assert all(torch.equal(u, v) for u, v in zip(a, b)), i
    # and the frames are the requested ones, not the hinted ones
    for (color, _, _), i in zip(got[True], order):
        n = list(G["utmm/names_c"]).index(str(G["utmm/0/color_names"][i]))
        assert np.array_equal(color.numpy(), np.transpose(G["utmm/colors"][n], (2, 0, 1)).astype(np.float32) / np.float32(255.0))


def test_malformed_directories_raise_with_the_file_named(tmp_path):
    # a list file whose lines have unequal lengths
    text = str(G["tum/file/depth.txt"]).splitlines()
    text[2] = text[2].split(" ")[0]
    root = tmp_path / "lists"
    write_scene(root, "tum", texts={"depth.txt": "\n".join(text) + "\n"})
    with pytest.raises(ValueError, match=r"depth\.txt"):
        ds.RecordedSequence(make_cfg(root, "tum"))
    # an RGBA colour image, an 8-bit depth image
    from PIL import Image
    for sub, name, image in (("rgba", str(G["tum/names_c"][1]), Image.fromarray(np.zeros((H, W, 4), np.uint8), "RGBA")),
                             ("depth8", str(G["tum/names_d"][1]), Image.fromarray(np.zeros((H, W), np.uint8)))):
        root = tmp_path / sub
        scene = write_scene(root, "tum")
        image.save(os.path.join(scene, name))
        seq = ds.RecordedSequence(make_cfg(root, "tum", prefetch=False))
        seq[0]
        with pytest.raises(ValueError, match=name.replace(".", r"\.")):
            seq[1]
    # a missing pose list, an image of another size than cam says
    root = tmp_path / "nopose"
    scene = write_scene(root, "tum")
    os.remove(os.path.join(scene, "groundtruth.txt"))
    with pytest.raises(ValueError, match="groundtruth.txt"):
        ds.RecordedSequence(make_cfg(root, "tum"))
    root = tmp_path / "size"
    scene = write_scene(root, "tum")
    Image.fromarray(np.zeros((H + 1, W, 3), np.uint8), "RGB").save(os.path.join(scene, str(G["tum/names_c"][0])))
    with pytest.raises(ValueError, match=str(G["tum/names_c"][0]).replace(".", r"\.")):
        ds.RecordedSequence(make_cfg(root, "tum", prefetch=False))[0]


def test_a_failed_prefetch_of_a_frame_nobody_asks_for_is_not_an_error(tmp_path):
    from PIL import Image
    scene = write_scene(tmp_path, "tum")
    Image.fromarray(np.zeros((H, W, 4), np.uint8), "RGBA").save(os.path.join(scene, str(G["tum/names_c"][1])))
    seq = ds.RecordedSequence(make_cfg(tmp_path, "tum", prefetch=True))
    a = seq[0][0].clone()      # queues the decode of the broken frame 1
    b = seq[2][0]              # ... which is only a hint
    assert not torch.equal(a, b)
    with pytest.raises(ValueError, match="RGB"):
        seq[0], seq[1]
    seq.close()


def test_slam_top_picks_the_frame_source_from_the_config(scenes):
    import slam_top
    from mm3dgs_slam_amd.config import default_config, utmm_config
    assert slam_top.sequence_source(default_config(device="cpu")) == "synthetic"
    for inputdir in ("", None):      # what the reference's configs ship: `inputdir:` is empty
        assert slam_top.sequence_source(dict(default_config(device="cpu"), dataset="tum", inputdir=inputdir)) == "synthetic"
        assert slam_top.sequence_source(dict(utmm_config(device="cpu"), dataset="utmm", inputdir=inputdir)) == "synthetic"
    assert slam_top.sequence_source(dict(default_config(device="cpu"), dataset="synthetic", inputdir=str(scenes["tum"]))) == "synthetic"
    assert slam_top.sequence_source(dict(default_config(device="cpu"), dataset="replica", inputdir=str(scenes["tum"]))) == "synthetic"
    cfg = make_cfg(scenes["tum"], "TUM")
    assert slam_top.sequence_source(cfg) == "recorded"
    seq = slam_top.build_sequence(cfg, frames=3)
    assert isinstance(seq, ds.RecordedSequence) and len(seq) == 3 and len(seq.poses) == 3
    seq.close()
    assert len(slam_top.build_sequence(make_cfg(scenes["utmm"], "utmm"))) == len(G["utmm/0/color_names"])


def test_device_ingest_is_refused_on_the_cpu(scenes):
    with pytest.raises(ValueError, match="ingest_on_device"):
        ds.RecordedSequence(make_cfg(scenes["tum"], "tum", ingest_on_device=True))
    assert ds.RecordedSequence(dict(make_cfg(scenes["tum"], "tum"), ingest_on_device=None)).on_device is False      # default on the CPU: host
