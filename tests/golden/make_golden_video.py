"""G14: the reference's debug-video frame and SLAM.render() image pair (build container only; needs matplotlib).

    python tests/golden/make_golden_video.py

`utils/depth_utils.py::depth_to_rgb` (:14-34) is imported and executed as is -- `cv2`, imported at its module top and absent here, is
stubbed, and `.cuda()` is a no-op (make_golden._CpuMode) -- with the installed matplotlib doing the colour-map lookup.  Around it the
operator chains of `slam/SLAM.py` are restated line by line, since `save_video_frame` and `render` themselves need a SLAM object, a
`cv2.VideoWriter` and `torchvision`:

* video (`slam/SLAM.py:243-275`): cat([gt_color, image, |image - gt_color|], 2) over cat of three depth_to_rgb images, cat(dim=1),
  `(vid_image * 255).to(torch.uint8).permute(1, 2, 0)`; the last depth image is the rescaled estimate (`use_gt_depth: false`, :251-259), the
  sensor depth again (`use_gt_depth: true`, :260-268) or the float of the mask of newly seeded pixels (:474-481).  Stored in RGB order;
  `cv2.cvtColor(..., COLOR_RGB2BGR)` (:275) is the reversal of the last axis.
* render (`slam/SLAM.py:180-193`): `torchvision.utils.save_image(torch.cat([image, depth_to_rgb(depth)], dim=1))` and the same for the frame
  and its sensor depth.  torchvision is absent here; for one image `save_image` is `make_grid` (the identity on a single [3,H,W] tensor) and
  `grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8)` (torchvision/utils.py, save_image), restated below.

Inputs: 12 x 20, seeded, colours in [0, 1] so that the reference's cast stays defined.  Stored: the inputs and the expected uint8 arrays."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg          # noqa: E402

mg.stub_modules()


def video_frame(depth_to_rgb, gt_color, image, gt_depth, depth, third):
    vid_image = torch.cat([gt_color, image, torch.abs(image - gt_color)], dim=2)
    depth_image = torch.cat([depth_to_rgb(gt_depth), depth_to_rgb(depth), depth_to_rgb(third)], dim=2)
    vid_image = torch.cat([vid_image, depth_image], dim=1)
    return (vid_image * 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()


def save_image_bytes(tensor):
    return tensor.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()


def main():
    from utils.depth_utils import depth_to_rgb
    g = torch.Generator().manual_seed(14)
    H, W = 12, 20
    yy, xx = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
    gt_color = torch.rand(3, H, W, generator=g)
    image = (gt_color + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    gt_color[:, 0, 0], gt_color[:, 0, 1], image[:, 0, 0], image[:, 0, 1] = 0.0, 1.0, 1.0, 0.0      # the ends of the range, and |diff| = 1
    gt_depth = 1.5 + 0.1 * xx + 0.05 * yy + 0.02 * torch.randn(H, W, generator=g)
    gt_depth[3:5, 4:9] = 0.0                                                                  # holes of the sensor
    depth = gt_depth + 0.05 * torch.randn(H, W, generator=g)
    est_scaled = 1.0 / (0.3 + 0.02 * xx + 0.01 * torch.rand(H, W, generator=g))
    mask = torch.rand(H, W, generator=g) < 0.3
    out = {"gt_color": mg.t2n(gt_color), "image": mg.t2n(image), "gt_depth": mg.t2n(gt_depth), "depth": mg.t2n(depth),
           "est_scaled": mg.t2n(est_scaled), "mask": mask.numpy()}
    with mg._CpuMode():
        out["video_est"] = video_frame(depth_to_rgb, gt_color, image, gt_depth, depth, est_scaled)          # use_gt_depth: false
        out["video_gt"] = video_frame(depth_to_rgb, gt_color, image, gt_depth, depth, gt_depth)             # use_gt_depth: true
        out["video_mask"] = video_frame(depth_to_rgb, gt_color, image, gt_depth, depth, mask.float())       # a frame that seeded Gaussians
        out["render"] = save_image_bytes(torch.cat([image, depth_to_rgb(depth)], dim=1))
        out["render_gt"] = save_image_bytes(torch.cat([gt_color, depth_to_rgb(gt_depth)], dim=1))
    for k in ("video_est", "video_gt", "video_mask", "render", "render_gt"):
        print(k, out[k].shape, out[k].dtype, int(out[k].astype(np.int64).sum()))
    path = os.path.join(HERE, "g14_video.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
