"""G13: the reference's TUM / UT-MM dataset classes on two tiny generated directories (build container only).

    python tests/golden/make_golden_dataset.py      ->  tests/golden/g13_dataset.npz

`gradslam_datasets.TUMDataset` and `UTMMDataset` are executed as they are.  Modules they import at the top and that are absent here are
stubbed: `natsort`; `imageio` (`imread` is provided by PIL); `cv2` (`resize` asserts that the size is unchanged and returns a copy: the
fixture records frames at native size only); `kornia.geometry.linalg`, of which `relative_transformation` uses
`compose_transformations` on 4x4 matrices -- provided as the 4x4 matrix product, `inv(pose[0]) @ pose[i]` in float32; `np.unicode_` is
aliased to `str` where numpy dropped it.

Two directories of 12x16 images.  The stamps are chosen so that every association rule bites: a depth stamp beyond `max_dt`, two colour
stamps closer than 1/32 s (TUM thins the second), a colour frame without a pose within `max_dt`; the UT-MM directory has `imu.txt`
with uneven row counts per interval and `tf.txt`.  Stored: the list-file texts and the image arrays (the test rebuilds the directories
from them), and for (start, stride, early_stop) in {(0,1,none), (0,2,none), (2,1,9)} what the reference returns: the chosen colour and
depth file names, relative poses, the 7-vector poses of the reference's `get_tensor_from_camera(inverse(c2w))`, `tstamps`, the IMU
tensors (concatenated, with their row counts), `c2i`, the intrinsics of `dataset[0]`, and `dataset[i]` colour and depth.  Also
`datautils.scale_intrinsics` at a 5x7 target.  Data only: nothing of the reference's code goes into the npz."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402

H, W = 12, 16
CAM = {"image_height": H, "image_width": W, "fx": 14.25, "fy": 13.5, "cx": 7.6, "cy": 5.8, "png_depth_scale": 5000.0}
SLICES = ((0, 1, -1), (0, 2, -1), (2, 1, 9))


def stub():
    mg.stub_modules()
    from PIL import Image
    if not hasattr(np, "unicode_"):
        np.unicode_ = str
    sys.modules["imageio"].imread = lambda p: np.asarray(Image.open(p))
    sys.modules["natsort"].natsorted = sorted

    def resize(img, size, interpolation=None):
        assert (img.shape[1], img.shape[0]) == tuple(size), (img.shape, size)
        return img.copy()
    sys.modules["cv2"].resize = resize
    sys.modules["cv2"].INTER_LINEAR, sys.modules["cv2"].INTER_NEAREST = 1, 0
    for name in ("kornia", "kornia.geometry", "kornia.geometry.linalg"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["kornia.geometry.linalg"].compose_transformations = torch.matmul
    sys.modules["kornia.geometry.linalg"].inverse_transformation = torch.inverse


def quat(rng, k):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = 0.05 * k + 0.3
    return np.concatenate([ax * np.sin(ang / 2), [np.cos(ang / 2)]])      # x y z w


def make_lists(kind, rng):
    """(texts, colour names, depth names): 16 colour stamps 0.1 s apart from t0, plus one 0.02 s after frame 5."""
    t0 = 1305031100.0 if kind == "tum" else 1700000000.0
    base = [t0 + 0.1 * k for k in range(16)]
    extra = base[5] + 0.02
    rgb_t = sorted(base + [extra])
    rgb, depth, pose, names_c, names_d = [], [], ["# timestamp tx ty tz qx qy qz qw"], [], []
    far = 0.085 if kind == "tum" else 0.02      # beyond max_dt (0.08 / 0.015), still the nearest depth stamp
    for n, t in enumerate(rgb_t):
        names_c.append(f"rgb/{n:04d}.png")
        names_d.append(f"depth/{n:04d}.png")
        rgb.append(f"{t:.6f} {names_c[-1]}")
        dt = far if n == 3 else (0.004 if kind == "tum" else 0.002)
        depth.append(f"{t + dt:.6f} {names_d[-1]}")
    for k, t in enumerate(base):
        if k == 9:
            continue                              # colour frame 9 has no pose within max_dt (its neighbours' are 0.1 s away)
        p = np.concatenate([0.05 * k + 0.01 * rng.normal(size=3), quat(rng, k)])
        pose.append(f"{t + 0.001:.6f} " + " ".join(f"{v:.7f}" for v in p))
    texts = {"rgb.txt": "\n".join(rgb) + "\n", "depth.txt": "\n".join(depth) + "\n", "groundtruth.txt": "\n".join(pose) + "\n"}
    if kind == "utmm":
        rows, t = [], t0 - 0.03
        while t < base[-1] + 0.02:
            on_frame = min(abs(t - b) for b in base) < 0.005
            if on_frame or rng.random() < 0.7:      # rows are dropped between the frames: uneven counts per interval
                rows.append(f"{t:.6f} " + " ".join(f"{v:.6f}" for v in rng.normal(size=30)))
            t += 0.01
        texts["imu.txt"] = "\n".join(rows) + "\n"
        texts["tf.txt"] = " ".join(f"{v:.7f}" for v in np.concatenate([[0.03, -0.01, 0.02], quat(rng, 3)])) + "\n"
    return texts, names_c, names_d


def write_dir(root, texts, names_c, names_d, colors, depths):
    from PIL import Image
    os.makedirs(os.path.join(root, "rgb")), os.makedirs(os.path.join(root, "depth"))
    for name, text in texts.items():
        with open(os.path.join(root, name), "w") as f:
            f.write(text)
    for n, (c, d) in enumerate(zip(colors, depths)):
        Image.fromarray(c, "RGB").save(os.path.join(root, names_c[n]))
        Image.fromarray(d).save(os.path.join(root, names_d[n]))


def main():
    stub()
    from gradslam_datasets import TUMDataset, UTMMDataset
    from gradslam_datasets import datautils
    from utils.pose_utils import get_tensor_from_camera
    out = {"slices": np.array(SLICES), "cam_keys": np.array(sorted(CAM)), "cam_values": np.array([CAM[k] for k in sorted(CAM)])}
    for kind, cls in (("tum", TUMDataset), ("utmm", UTMMDataset)):
        rng = np.random.default_rng(13 if kind == "tum" else 14)
        texts, names_c, names_d = make_lists(kind, rng)
        n = len(names_c)
        colors = rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
        depths = rng.integers(0, 65536, size=(n, H, W)).astype(np.uint16)
        depths[:, 0, :3] = (0, 1, 65535)
        colors[:, 0, 0], colors[:, 0, 1] = 0, 255
        for name, text in texts.items():
            out[f"{kind}/file/{name}"] = np.array(text)
        out[f"{kind}/names_c"], out[f"{kind}/names_d"] = np.array(names_c), np.array(names_d)
        out[f"{kind}/colors"], out[f"{kind}/depths"] = colors, depths
        cfg = {"dataset": kind, "cam": dict(CAM, png_depth_scale=5000.0 if kind == "tum" else 1000.0)}
        with tempfile.TemporaryDirectory() as tmp:
            write_dir(os.path.join(tmp, "scene"), texts, names_c, names_d, colors, depths)
            for s, (start, stride, end) in enumerate(SLICES):
                with mg._CpuMode():
                    ds = cls(config_dict=cfg, basedir=tmp, sequence="scene", start=start, end=end, stride=stride, desired_height=H,
                             desired_width=W, device="cpu", relative_pose=True, ignore_bad=False, use_train_split=True)
                    items = [ds[i] for i in range(len(ds))]
                    pre = f"{kind}/{s}/"
                    out[pre + "color_names"] = np.array([os.path.relpath(p, ds.input_folder) for p in ds.color_paths])
                    out[pre + "depth_names"] = np.array([os.path.relpath(p, ds.input_folder) for p in ds.depth_paths])
                    out[pre + "rel_poses"] = mg.t2n(ds.transformed_poses)
                    out[pre + "pose7"] = np.stack([mg.t2n(get_tensor_from_camera(torch.inverse(it[3]))) for it in items])
                    out[pre + "color"] = np.stack([mg.t2n(it[0]) for it in items])      # [n,H,W,3] float32 in [0,255]
                    out[pre + "depth"] = np.stack([mg.t2n(it[1]) for it in items])      # [n,H,W,1] float32 metres
                    out[pre + "intrinsics"] = mg.t2n(items[0][2])
                    assert all(it[0].dtype == torch.float32 and it[1].dtype == torch.float32 for it in items)
                    if kind == "utmm":
                        out[pre + "tstamps"] = np.array(ds.tstamps, dtype=np.float64)
                        out[pre + "imu_counts"] = np.array([int(m.shape[0]) for m in ds.imus])
                        out[pre + "imu_rows"] = mg.t2n(torch.cat(ds.imus, 0))
                        out[pre + "imu_item"] = np.concatenate([mg.t2n(it[4]) for it in items], 0)      # what dataset[i] hands out, frame by frame
                        out[pre + "c2i"] = mg.t2n(ds.get_c2i_tf())
                    if s == 0:
                        out[f"{kind}/intrinsics_5x7"] = mg.t2n(datautils.scale_intrinsics(ds.get_cam_K(), 5.0 / H, 7.0 / W))
                    print(kind, (start, stride, end), "frames", len(ds), list(out[pre + "color_names"]))
    path = os.path.join(HERE, "g13_dataset.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
