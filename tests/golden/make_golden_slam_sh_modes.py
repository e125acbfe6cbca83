"""G9 variants at an ACTIVE SH degree in the two direction sources besides the shipped one (build container only).

    python tests/golden/make_golden_slam_sh_modes.py            # g9_sh2_python_active.npz, g9_no_transform_sh_active.npz
    python tests/golden/make_golden_slam_sh_modes.py --large    # the g9L_* forms (160x120)

Runs the reference's own classes through `make_golden_slam.run_reference` exactly like the other G9 variants, with the map resumed at its
maximal SH degree (slam/gaussian_model.py:363) as in `sh2_active`, but with the viewing direction taken
  * `sh2_python_active` (pipeline.convert_SHs_python: true): from the WORLD mean about the origin -- slam/renderer.py:179-193 evaluates SH in
    Python on pc.get_xyz - camera_pos, and camera_pos is 0 because the shipped mode's view matrix is the identity;
  * `no_transform_sh_active` (pipeline.transform_means_python: false): from the world mean minus the camera centre w2c^-1[3, :3], in the
    rasterizer (the CPU oracle stands in for the CUDA extension).
The inputs are the stored frames of the existing set (tests/g9_util.load_frames), so the frame files are not rewritten."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(1, ROOT)

import torch  # noqa: E402

import make_golden_slam as mgs  # noqa: E402  (reads --large from sys.argv)

NEW = {
    "sh2_python_active": dict(pipeline={"convert_SHs_python": True}, tracking={"iters": 8}, mapping=dict(mgs._MAP, iters=12, sh_degree=2),
                              _resumed_sh=True),
    "no_transform_sh_active": dict(pipeline={"transform_means_python": False}, tracking={"iters": 8}, mapping=dict(mgs._MAP, iters=12, sh_degree=2),
                                   _resumed_sh=True),
}


def main():
    from tests import g9_util
    mgs.VARIANTS.update(NEW)
    for name in NEW:
        mgs.SHORT[name] = 4 if mgs.LARGE else 3
    mgs.mg.stub_modules()
    sys.modules["pyiqa"].create_metric = lambda *a, **k: None

    def pearson_corrcoef(preds, target):
        x, y = preds - preds.mean(), target - target.mean()
        return (x * y).sum() / torch.sqrt((x * x).sum() * (y * y).sum())
    sys.modules["torchmetrics.functional.regression"].pearson_corrcoef = pearson_corrcoef
    F = g9_util.load_frames(mgs.PREFIX)
    frames = [(torch.from_numpy(c.copy()), torch.from_numpy(d.copy())) for c, d in zip(F["color"], F["depth"])]
    gt_poses = torch.from_numpy(F["gt_poses"].copy())
    imu = torch.from_numpy(F["imu"].copy())
    est = [torch.from_numpy(e.copy()) for e in F["est"]]
    est_scaled = [torch.from_numpy(e.copy()) for e in F["est_scaled"]]
    for name in (sys.argv[1:] or list(NEW)):
        mgs.run_reference(name, mgs.VARIANTS[name], frames, gt_poses, imu, [float(t) for t in F["tstamps"]], est, est_scaled)


if __name__ == "__main__":
    main()
