"""G15: the reference's pixel-to-world lift of an RGB-D render (build container only; needs matplotlib for the module's imports).

    python tests/golden/make_golden_pointcloud.py

`scripts/visualizer.py::rgbd2pcd` (:69-112) is imported and executed as is: `.cuda()` is a no-op (make_golden._CpuMode), the modules the
reference's package imports and this container lacks are stubbed (make_golden.stub_modules), and `open3d` -- imported at the module top for
the interactive window, which is out of scope -- is a stand-in whose `utility.Vector3dVector` returns the array it is given, so that the
function's two return values are the float64 copies of its float32 points and colours.

Inputs: seeded colour / depth images at 17 x 33 and 48 x 64, a pose with a rotation of about 40 degrees about a skew axis and a translation
of the order of the depths, non-integer intrinsics.  Stored: the inputs and the returned points [H W, 3] and colours [H W, 3] (float64)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402

mg.stub_modules()
o3d = types.ModuleType("open3d")
o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: a, Vector2iVector=lambda a: a)
sys.modules["open3d"] = o3d

SHAPES = ((17, 33), (48, 64))


def main():
    sys.path.insert(0, os.path.join(mg.REF, "scripts"))
    import visualizer
    g = torch.Generator().manual_seed(15)
    pose = torch.tensor([0.93, 0.21, -0.27, 0.12, 0.35, -0.2, 0.6])
    pose[:4] /= pose[:4].norm()
    out = {"pose": mg.t2n(pose)}
    for H, W in SHAPES:
        cam = {"fx": 41.37 * W / 33.0, "fy": 40.91 * W / 33.0, "cx": 0.5 * W - 0.85, "cy": 0.5 * H + 0.4}
        yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
        color = torch.rand(3, H, W, generator=g)
        depth = 1.2 + 0.04 * xx + 0.025 * yy + 0.3 * torch.rand(H, W, generator=g)
        with mg._CpuMode():
            pts, cols = visualizer.rgbd2pcd(color, depth, pose, {"cam": cam})
        tag = f"{H}x{W}"
        out[f"cam_{tag}"] = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], dtype=np.float64)
        out[f"color_{tag}"], out[f"depth_{tag}"] = mg.t2n(color), mg.t2n(depth)
        out[f"pts_{tag}"], out[f"cols_{tag}"] = np.asarray(pts), np.asarray(cols)
        print(tag, out[f"pts_{tag}"].shape, out[f"pts_{tag}"].dtype, out[f"cols_{tag}"].shape, float(np.abs(out[f"pts_{tag}"]).max()))
    path = os.path.join(HERE, "g15_pointcloud.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
