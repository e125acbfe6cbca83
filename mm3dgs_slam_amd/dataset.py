"""Recorded RGB-D sequences from disk: TUM-format and UT-MM-format directories (reference ``gradslam_datasets/tum.py``, ``utmm.py``,
``basedataset.py``), as a frame source with the protocol of ``slam.SyntheticSequence`` (``len``, ``seq[i] -> (color [3,H,W], depth
[H,W], gt_pose [7] world->camera)`` on ``cfg["device"]``, ``poses``, ``tstamps``, ``tf``, ``imu(i)``, and -- only with the config key
``est_depth_dir`` -- ``est(i) -> [H,W]``, the monocular depth estimate; without the key there is no attribute ``est`` and with
``use_gt_depth: false`` the loop uses the sensor depth).

Directory (``inputdir/scene``): ``rgb.txt``, ``depth.txt``, ``groundtruth.txt`` or ``pose.txt`` (first line skipped), for UT-MM also
``imu.txt`` and ``tf.txt``; lines are ``stamp name`` / ``stamp tx ty tz qx qy qz qw`` / ``stamp <imu columns>``, separated by single
blanks.  Association is the reference's, literally: per colour stamp the nearest depth and pose stamp (and IMU row), kept when all are
closer than ``max_dt`` (TUM 0.08 s, UT-MM 0.015 s); TUM then thins to frames more than 1/32 s apart (``tum.py:100-105``); UT-MM gives
frame k the IMU rows ``lstart..lend`` since the previous kept frame, and turns the robot-frame pose into the optical frame
(``pose_matrix_from_quaternion_tf``).  Then ``[start_idx : early_stop_idx : stride]``, poses relative to the first kept frame
(``inv(pose[0]) @ pose[i]`` in float32) and ``gt_pose = get_tensor_from_camera(inverse(c2w))``.

IMU rows under a stride: ``basedataset.py:196-213`` concatenates ``stride`` consecutive per-frame blocks counting from block 0 up to
``end`` -- it ignores ``start_idx``, and frame k (original frame ``start + k stride``) gets blocks ``k stride .. k stride + stride - 1``,
i.e. with a stride of 2 frame 1 gets the rows of the intervals ending at original frames 2 and 3, not 1 and 2; with ``early_stop_idx``
the list has more entries than frames.  Kept exactly as written there (the golden fixture pins it); it is right for stride 1, start 0.

Frame ingest, chosen by ``cfg["ingest_on_device"]``:
  false  ``ingest_host``: the reference's host chain in torch on the CPU -- float64 bilinear (colour) / nearest (depth) resize by the
         formulas of ``mm3dgs_ingest_frame`` (include/mm3dgs.h), depth / png_depth_scale, ``.float()``, upload of 16 bytes per pixel,
         permute, / 255.  The fallback for ``device: cpu`` and the yardstick of the kernel.  The division by 255 is the correctly rounded
         float32 one (a tensor divisor: torch's device kernel turns a Python-scalar divisor into a multiplication by 1/255).
  true   the decoded bytes go to pinned staging buffers, up as raw uint8 / uint16 (5 bytes per source pixel, non-blocking), and
         ``mm3dgs_ingest_frame`` writes both images in one launch on the current stream.  Two staging slots, an event after each upload
         that is waited on before the slot is rewritten: a frame in flight is never overwritten.
The formulas are meant to be ``cv2.resize``'s (INTER_LINEAR / INTER_NEAREST on float64 input); cv2 was not available, so that match is
unchecked.  ``prefetch`` (default on): ONE worker thread decodes frame i + 1 into the free slot while frame i is tracked and mapped; it
touches host memory only, and a prefetched frame is only a hint -- any access order gives the same frames.

Monocular depth estimates (``est_depth_dir``, a folder inside ``inputdir/scene``).  The depth network (MiDaS through torch.hub in the
reference) stays out of scope; its raw per-frame output is read from disk and the reference's last step -- ``F.interpolate(prediction,
size=(H, W), mode="bilinear", align_corners=False)`` of ``utils/depth_utils.py`` -- is done here.  The estimate of a kept colour frame is
the file whose stem is the stem of the colour image's basename (``rgb/1305031452.791720.png`` -> ``est_depth/1305031452.791720.npy``, else
``.png``): a ``.npy`` holds a 2-D C-contiguous float32 or float16 array at any resolution, used as it is; a ``.png`` is 16-bit greyscale
(what MiDaS' run.py writes), its integers times ``cam.est_depth_scale`` (default 1).  Every kept frame needs its file (checked in the
constructor) and all files have the first one's shape and dtype (the staging buffers are sized once).  ``est(i)`` is
``ingest_est_host`` (float64 bilinear by ``_axis``, rounded once) on the host path and ``mm3dgs_ingest_est`` on the device path, where the
raw array travels in the frame's staging slot: decoded by the same prefetch job, uploaded with the frame under the same event.  It
returns a fresh tensor on every call (keyframes keep the estimate), the same in any access order.  Neither path has been timed."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .pose_utils import get_tensor_from_camera

RECORDED_DATASETS = ("tum", "utmm")
# The device path becomes the default on a CUDA device only once tools/ingest_ab.py has shown its median per-frame time below the host
# path's at both measured shapes (profiles/r11_ingest.jsonl).  NOT MEASURED yet: the device path ships opt-in.
INGEST_ON_DEVICE_DEFAULT = False


def is_recorded(cfg):
    """True when the config names a recorded sequence: a non-empty ``inputdir`` and ``dataset`` tum / utmm."""
    return bool(cfg.get("inputdir")) and str(cfg.get("dataset", "")).lower() in RECORDED_DATASETS


def _parse_list(path, skiprows=0, min_cols=2):
    """np.loadtxt as the reference calls it (single-blank separated strings, '#' comments); a malformed file is named in the error."""
    if not os.path.isfile(path):
        raise ValueError(f"{path}: missing list file")
    try:
        data = np.loadtxt(path, delimiter=" ", dtype=str, skiprows=skiprows)
    except ValueError as e:
        raise ValueError(f"{path}: malformed list file (lines of unequal length?): {e}") from e
    data = data.reshape(1, -1) if data.ndim == 1 else data
    if data.ndim != 2 or data.shape[0] == 0 or data.shape[1] < min_cols:
        raise ValueError(f"{path}: expected lines of at least {min_cols} blank-separated fields, got an array of shape {data.shape}")
    return data


def _rotation(q):
    from scipy.spatial.transform import Rotation      # (the reference's own quaternion convention and arithmetic: x y z w)
    return Rotation.from_quat(q).as_matrix()


def _pose_tum(pvec):
    pose = np.eye(4)
    pose[:3, :3] = _rotation(pvec[3:])
    pose[:3, 3] = pvec[:3]
    return pose


def _pose_utmm(pvec):
    """Robot frame -> camera optical frame (z forward, x right, y down), utmm.py:104-120."""
    r2w = np.eye(4)
    r2w[:3, :3] = _rotation(pvec[3:])
    c2r = np.eye(4)
    c2r[:3, :3] = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], dtype=np.float64)
    r2w = r2w @ c2r
    r2w[:3, 3] = pvec[:3]
    return r2w


def _associate(t_image, t_depth, t_pose, t_imu, max_dt):
    """(i, j, k, l) per kept colour frame; l = IMU row indices since the previous kept frame (None without IMU)."""
    out, lstart = [], 0
    for i, t in enumerate(t_image):
        j = np.argmin(np.abs(t_depth - t))
        k = np.argmin(np.abs(t_pose - t))
        ok = (np.abs(t_depth[j] - t) < max_dt) and (np.abs(t_pose[k] - t) < max_dt)
        if t_imu is None:
            if ok:
                out.append((i, j, k, None))
            continue
        lend = np.argmin(np.abs(t_imu - t))
        if ok and (np.abs(t_imu[lend] - t) < max_dt):
            out.append((i, j, k, np.arange(lstart, lend + 1, step=1)))
            lstart = lend + 1
    return out


def _axis(n_out, n_src):
    """Bilinear source coordinates along one axis: (i0, i1, weight of i1), float64."""
    f = (torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_src / n_out) - 0.5
    fl = torch.floor(f)
    w = f - fl
    edge = (fl < 0) | (fl >= n_src - 1)
    w = torch.where(edge, torch.zeros_like(w), w)
    i0 = fl.clamp(0, n_src - 1).long()
    return i0, (i0 + 1).clamp(max=n_src - 1), w


def _nearest(n_out, n_src):
    return torch.floor(torch.arange(n_out, dtype=torch.float64) * (n_src / n_out)).long().clamp(max=n_src - 1)


def resize_host(rgb, depth, H, W):
    """float64 resize of raw arrays: rgb [Hs,Ws,3] -> [H,W,3] bilinear, depth [Hs,Ws] -> [H,W] nearest (depth may be None)."""
    color = torch.as_tensor(np.ascontiguousarray(rgb)).double()
    Hs, Ws = color.shape[:2]
    d = None if depth is None else torch.as_tensor(np.ascontiguousarray(depth).astype(np.int64)).double()
    if (Hs, Ws) != (H, W):
        x0, x1, a = _axis(W, Ws)
        y0, y1, b = _axis(H, Hs)
        a, b = a[None, :, None], b[:, None, None]
        top = (1.0 - a) * color[y0][:, x0] + a * color[y0][:, x1]
        bot = (1.0 - a) * color[y1][:, x0] + a * color[y1][:, x1]
        color = (1.0 - b) * top + b * bot
        if d is not None:
            d = d[_nearest(H, Hs)][:, _nearest(W, Ws)]
    return color, d


def ingest_host(rgb, depth, png_depth_scale, H, W, device="cpu"):
    """The host path: raw uint8 [Hs,Ws,3] and uint16 [Hs,Ws] arrays -> (color [3,H,W] in [0,1], depth [H,W] metres), float32 on `device`."""
    color, d = resize_host(rgb, depth, H, W)
    color = color.float().to(device)
    color = (color.permute(2, 0, 1) / torch.tensor(255.0, device=device)).contiguous()
    if d is not None:
        d = (d / float(png_depth_scale)).float().to(device)
    return color, d


def ingest_device(rgb_dev, depth_dev, png_depth_scale, H, W):
    """``mm3dgs_ingest_frame`` on the current stream: rgb_dev uint8 [Hs,Ws,3] (any view with contiguous bytes), depth_dev a 2-byte integer
    tensor [Hs,Ws] or None, both on the GPU.  Returns fresh (color [3,H,W], depth [H,W] or None)."""
    from . import _lib
    from .rasterizer import _stream
    if not rgb_dev.is_cuda or rgb_dev.dtype != torch.uint8 or rgb_dev.dim() != 3 or rgb_dev.shape[2] != 3 or not rgb_dev.is_contiguous():
        raise ValueError(f"ingest_device: rgb must be a contiguous uint8 [Hs,Ws,3] tensor on the GPU, got {rgb_dev.dtype} {tuple(rgb_dev.shape)}")
    Hs, Ws = int(rgb_dev.shape[0]), int(rgb_dev.shape[1])
    if depth_dev is not None and (not depth_dev.is_cuda or depth_dev.element_size() != 2 or tuple(depth_dev.shape) != (Hs, Ws)
                                  or not depth_dev.is_contiguous()):
        raise ValueError(f"ingest_device: depth must be a contiguous 16-bit [{Hs},{Ws}] tensor on the GPU, got {depth_dev.dtype} {tuple(depth_dev.shape)}")
    color = torch.empty(3, H, W, dtype=torch.float32, device=rgb_dev.device)
    d = None if depth_dev is None else torch.empty(H, W, dtype=torch.float32, device=rgb_dev.device)
    P = _lib.ptr
    _lib.check(_lib.load().mm3dgs_ingest_frame(Hs, Ws, P(rgb_dev), P(depth_dev), float(png_depth_scale), int(H), int(W), P(color), P(d), _stream()))
    return color, d


EST_DTYPES = {np.dtype(np.float32): 0, np.dtype(np.float16): 1, np.dtype(np.uint16): 2}      # the dtype codes of mm3dgs_ingest_est


def resize_est_host(raw, H, W):
    """float64 bilinear resize of a raw 2-D float32 / float16 / uint16 array [Hs,Ws] -> [H,W] by `_axis` (= F.interpolate with
    align_corners=False); nothing is rounded to float32 yet.  Equal sizes: the values themselves, no blend."""
    raw = np.asarray(raw)
    if raw.ndim != 2 or raw.dtype not in EST_DTYPES:
        raise ValueError(f"a depth estimate must be a 2-D float32, float16 or uint16 array, got {raw.dtype} {raw.shape}")
    p = torch.as_tensor(raw.astype(np.int64) if raw.dtype == np.uint16 else np.ascontiguousarray(raw)).double()
    Hs, Ws = p.shape
    if (Hs, Ws) != (H, W):
        x0, x1, a = _axis(W, Ws)
        y0, y1, b = _axis(H, Hs)
        a, b = a[None, :], b[:, None]
        top = (1.0 - a) * p[y0][:, x0] + a * p[y0][:, x1]
        bot = (1.0 - a) * p[y1][:, x0] + a * p[y1][:, x1]
        p = (1.0 - b) * top + b * bot
    return p


def ingest_est_host(raw, scale, H, W, device="cpu"):
    """The host path of the monocular estimate: raw [Hs,Ws] -> float32 [H,W] on `device`: `resize_est_host`, times `scale` in float64,
    rounded once.  The fallback for ``device: cpu`` and the yardstick of ``mm3dgs_ingest_est``; always a fresh tensor."""
    return (resize_est_host(raw, H, W) * float(scale)).float().to(device)


def ingest_est_device(raw_dev, scale, H, W):
    """``mm3dgs_ingest_est`` on the current stream: raw_dev a contiguous [Hs,Ws] float32 / float16 / 2-byte integer (the bits of uint16)
    tensor on the GPU.  Returns a fresh float32 [H,W] tensor."""
    from . import _lib
    from .rasterizer import _stream
    code = 0 if raw_dev.dtype == torch.float32 else 1 if raw_dev.dtype == torch.float16 else 2
    if not raw_dev.is_cuda or raw_dev.dim() != 2 or not raw_dev.is_contiguous() or (code == 2 and (raw_dev.is_floating_point() or raw_dev.element_size() != 2)):
        raise ValueError(f"ingest_est_device: a contiguous float32 / float16 / 16-bit integer [Hs,Ws] tensor on the GPU is needed, got "
                         f"{raw_dev.dtype} {tuple(raw_dev.shape)} on {raw_dev.device}")
    out = torch.empty(H, W, dtype=torch.float32, device=raw_dev.device)
    _lib.check(_lib.load().mm3dgs_ingest_est(int(raw_dev.shape[0]), int(raw_dev.shape[1]), _lib.ptr(raw_dev), code, float(scale), int(H), int(W),
                                             _lib.ptr(out), _stream()))
    return out


def decode_est(path):
    """The raw monocular estimate of one frame: a 2-D C-contiguous float32 / float16 array from a .npy, uint16 from a 16-bit greyscale
    .png.  Anything else is an error that names the file."""
    if path.lower().endswith(".npy"):
        try:
            arr = np.load(path, allow_pickle=False)
        except Exception as e:
            raise ValueError(f"{path}: not a readable .npy array: {e}") from e
        if arr.ndim != 2 or arr.dtype not in (np.float32, np.float16) or not arr.flags["C_CONTIGUOUS"] or arr.size == 0:
            raise ValueError(f"{path}: a depth estimate must be a non-empty 2-D C-contiguous float32 or float16 array, got {arr.dtype} {arr.shape}"
                             f"{'' if arr.flags['C_CONTIGUOUS'] else ' (not C-contiguous)'}")
        return arr
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("I;16", "I;16L", "I;16B", "I;16N"):
            raise ValueError(f"{path}: a depth estimate image must be 16-bit greyscale, got PIL mode {im.mode!r}")
        return np.ascontiguousarray(np.asarray(im).astype(np.uint16, copy=False))


def decode_png(color_path, depth_path):
    """(uint8 [Hs,Ws,3], uint16 [Hs,Ws]) with PIL.  Anything but 8-bit RGB / 16-bit greyscale is an error that names the file."""
    from PIL import Image
    with Image.open(color_path) as im:
        if im.mode != "RGB":
            raise ValueError(f"{color_path}: colour image must be 8-bit RGB, got PIL mode {im.mode!r}")
        rgb = np.asarray(im, dtype=np.uint8)
    with Image.open(depth_path) as im:
        if im.mode not in ("I;16", "I;16L", "I;16B", "I;16N"):
            raise ValueError(f"{depth_path}: depth image must be 16-bit greyscale, got PIL mode {im.mode!r}")
        depth = np.asarray(im).astype(np.uint16, copy=False)
    return rgb, depth


def quantise_frame(color, depth, png_depth_scale):
    """float [3,H,W] in [0,1] and [H,W] metres -> what a sensor file holds: uint8 [H,W,3] and uint16 [H,W] numpy arrays."""
    rgb = (color.detach().float().clamp(0, 1) * 255.0).round().permute(1, 2, 0).to(torch.uint8).cpu().numpy()
    d = (depth.detach().double() * float(png_depth_scale)).round().clamp(0, 65535).cpu().numpy().astype(np.uint16)
    return np.ascontiguousarray(rgb), np.ascontiguousarray(d)


def write_tum_sequence(folder, frames, poses, tstamps, est=None):
    """Record frames as a TUM-format directory: `frames` = [(uint8 [H,W,3], uint16 [H,W])], `poses` = world->camera 7-vectors (the
    package's layout), `tstamps` in seconds.  rgb/NNNN.png, depth/NNNN.png, rgb.txt, depth.txt, groundtruth.txt.  `est`: one 2-D float32 /
    float16 array (or tensor) per frame, the monocular estimate at any resolution, written as est_depth/NNNN.npy (`est_depth_dir: est_depth`)."""
    from PIL import Image
    from scipy.spatial.transform import Rotation
    from .pose_utils import get_camera_from_tensor
    os.makedirs(os.path.join(folder, "rgb"), exist_ok=True)
    os.makedirs(os.path.join(folder, "depth"), exist_ok=True)
    if est is not None:
        if len(est) != len(frames):
            raise ValueError(f"write_tum_sequence: {len(est)} estimates for {len(frames)} frames")
        os.makedirs(os.path.join(folder, "est_depth"), exist_ok=True)
        for n, e in enumerate(est):
            e = np.ascontiguousarray(e.detach().cpu().numpy() if torch.is_tensor(e) else e)
            if e.ndim != 2 or e.dtype not in (np.float32, np.float16):
                raise ValueError(f"write_tum_sequence: estimate {n} must be a 2-D float32 or float16 array, got {e.dtype} {e.shape}")
            np.save(os.path.join(folder, "est_depth", f"{n:04d}.npy"), e)
    rgb_txt, depth_txt, gt_txt = [], [], ["# timestamp tx ty tz qx qy qz qw"]
    for n, ((rgb, d), pose, t) in enumerate(zip(frames, poses, tstamps)):
        Image.fromarray(rgb, "RGB").save(os.path.join(folder, "rgb", f"{n:04d}.png"))
        Image.fromarray(d).save(os.path.join(folder, "depth", f"{n:04d}.png"))
        c2w = np.linalg.inv(get_camera_from_tensor(pose.detach().cpu()).double().numpy())
        q = Rotation.from_matrix(c2w[:3, :3]).as_quat()
        rgb_txt.append(f"{t:.6f} rgb/{n:04d}.png")
        depth_txt.append(f"{t:.6f} depth/{n:04d}.png")
        gt_txt.append(f"{t:.6f} " + " ".join(f"{v:.9f}" for v in (*c2w[:3, 3], *q)))
    for name, lines in (("rgb.txt", rgb_txt), ("depth.txt", depth_txt), ("groundtruth.txt", gt_txt)):
        with open(os.path.join(folder, name), "w") as f:
            f.write("\n".join(lines) + "\n")


class _Slot:
    """One staging slot: host arrays the decoder writes (pinned on the device path), their raw device copies, the event of the last upload.
    `est_like` (the first frame's raw estimate, or None) adds a buffer of its shape and dtype; est_idx / est_dev_idx say which frame's
    estimate the host buffer and its device copy hold."""

    def __init__(self, Hs, Ws, device, on_device, est_like=None):
        self.event = None
        self.est, self.est_idx, self.est_dev_idx = None, None, None
        if est_like is not None:
            t = {0: torch.float32, 1: torch.float16, 2: torch.int16}[EST_DTYPES[est_like.dtype]]      # (int16: the bits of uint16)
            self._est_t = torch.empty(est_like.shape, dtype=t)
            if on_device:
                self._est_t = self._est_t.pin_memory()
                self.est_dev = torch.empty(est_like.shape, dtype=t, device=device)
            self.est = self._est_t.numpy().view(est_like.dtype)
        if on_device:
            self._rgb_t = torch.empty(Hs, Ws, 3, dtype=torch.uint8).pin_memory()
            self._depth_t = torch.empty(Hs, Ws, dtype=torch.int16).pin_memory()      # (the bits of the uint16 image)
            self.rgb, self.depth = self._rgb_t.numpy(), self._depth_t.numpy().view(np.uint16)
            self.rgb_dev = torch.empty(Hs, Ws, 3, dtype=torch.uint8, device=device)
            self.depth_dev = torch.empty(Hs, Ws, dtype=torch.int16, device=device)
        else:
            self.rgb, self.depth = np.empty((Hs, Ws, 3), np.uint8), np.empty((Hs, Ws), np.uint16)

    def wait(self):
        if self.event is not None:
            self.event.synchronize()

    def upload(self):
        self.rgb_dev.copy_(self._rgb_t, non_blocking=True)
        self.depth_dev.copy_(self._depth_t, non_blocking=True)
        if self.est is not None and self.est_idx is not None:
            self.est_dev.copy_(self._est_t, non_blocking=True)
            self.est_dev_idx = self.est_idx
        self._record()

    def upload_est(self):
        self.est_dev.copy_(self._est_t, non_blocking=True)
        self.est_dev_idx = self.est_idx
        self._record()

    def _record(self):
        if self.event is None:
            self.event = torch.cuda.Event()
        self.event.record()


class RecordedSequence:
    """See the module docstring.  Config keys (the reference's): dataset (tum | utmm), inputdir, scene, start_idx, stride,
    early_stop_idx, desired_height, desired_width, cam.{image_height, image_width, fx, fy, cx, cy, png_depth_scale}; plus
    ingest_on_device, prefetch, est_depth_dir and cam.est_depth_scale.  The constructor writes the intrinsics scaled to the desired size
    back into ``cfg["cam"]`` (Python floats; float32 arithmetic of datautils.scale_intrinsics) -- build it BEFORE a Renderer is built from
    that cfg.  `frames` caps the length (slam_top's --frames).  `est_decoder` reads one estimate file (`decode_est`)."""

    def __init__(self, cfg, frames=None, decoder=decode_png, est_decoder=decode_est):
        self.cfg = cfg
        self.name = str(cfg["dataset"]).lower()
        if self.name not in RECORDED_DATASETS:
            raise ValueError(f"RecordedSequence reads dataset tum or utmm, not {cfg['dataset']!r}")
        self.device = torch.device(cfg["device"])
        self.folder = os.path.join(cfg["inputdir"], cfg.get("scene") or "")
        cam = cfg["cam"]
        self.png_depth_scale = float(cam["png_depth_scale"])
        self.Hs, self.Ws = int(cam["image_height"]), int(cam["image_width"])
        self.H, self.W = int(cfg["desired_height"]), int(cfg["desired_width"])
        self._decoder = decoder
        self._load_lists(int(cfg.get("start_idx", 0) or 0), int(cfg.get("stride", 1) or 1), int(cfg.get("early_stop_idx", -1)))
        if frames is not None:
            self.color_paths, self.depth_paths = self.color_paths[:frames], self.depth_paths[:frames]
            self.c2w, self.tstamps = self.c2w[:frames], self.tstamps[:frames]
        # relative poses (basedataset.py:287-305: inverse of the repeated first pose, composed with every pose, float32), then the 7-vectors
        P = torch.stack(self.c2w)
        self.rel_c2w = torch.matmul(torch.inverse(P[0].unsqueeze(0).repeat(P.shape[0], 1, 1)), P)
        self.poses = [get_tensor_from_camera(torch.inverse(M)).to(self.device) for M in self.rel_c2w]
        # datautils.scale_intrinsics: float32 entries times the Python-float ratios
        K = torch.tensor([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], dtype=torch.float64).to(torch.float)
        h_ratio, w_ratio = float(self.H) / self.Hs, float(self.W) / self.Ws
        K[0] *= w_ratio; K[1] *= h_ratio; K[2] *= w_ratio; K[3] *= h_ratio
        self.intrinsics = K
        cam["fx"], cam["fy"], cam["cx"], cam["cy"] = (float(v) for v in K)
        on_dev = cfg.get("ingest_on_device")
        self.on_device = (INGEST_ON_DEVICE_DEFAULT and self.device.type == "cuda") if on_dev is None else bool(on_dev)
        if self.on_device and self.device.type != "cuda":
            raise ValueError("ingest_on_device needs a CUDA device (there is no CPU kernel); use ingest_on_device: false")
        self.prefetch = bool(cfg.get("prefetch", True))
        self.est_paths, est_like = None, None
        if cfg.get("est_depth_dir"):
            self._est_decoder = est_decoder
            self.est_depth_scale = float(cam.get("est_depth_scale", 1.0) or 1.0)
            if not (self.est_depth_scale > 0.0 and np.isfinite(self.est_depth_scale)):
                raise ValueError(f"cam.est_depth_scale must be finite and positive, got {self.est_depth_scale}")
            self.est_paths = self._est_files(os.path.join(self.folder, str(cfg["est_depth_dir"])))
            est_like = est_decoder(self.est_paths[0])
            self.est = self._est      # bound on the instance: SLAM.step asks hasattr(seq, "est")
        self._slots = [_Slot(self.Hs, self.Ws, self.device, self.on_device, est_like) for _ in range(2)]
        self._next, self._pending = 0, None
        self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="mm3dgs-decode") if self.prefetch else None

    # ---- lists, association, poses -------------------------------------------------------------------------------------------------
    def _load_lists(self, start, stride, end):
        f = self.folder
        pose_list = next((p for p in (os.path.join(f, "groundtruth.txt"), os.path.join(f, "pose.txt")) if os.path.isfile(p)), None)
        if pose_list is None:
            raise ValueError(f"{f}: neither groundtruth.txt nor pose.txt")
        image_data, depth_data = _parse_list(os.path.join(f, "rgb.txt")), _parse_list(os.path.join(f, "depth.txt"))
        pose_data = _parse_list(pose_list, skiprows=1, min_cols=8)
        pose_vecs = pose_data[:, 1:].astype(np.float64)
        t_image, t_depth, t_pose = (d[:, 0].astype(np.float64) for d in (image_data, depth_data, pose_data))
        utmm = self.name == "utmm"
        if utmm:
            imu_data = _parse_list(os.path.join(f, "imu.txt"), min_cols=29)
            imu_vecs, t_imu = imu_data[:, 1:].astype(np.float64), imu_data[:, 0].astype(np.float64)
            assoc = _associate(t_image, t_depth, t_pose, t_imu, max_dt=0.015)
        else:
            assoc = _associate(t_image, t_depth, t_pose, None, max_dt=0.08)
            keep = [0]                                  # tum.py:100-105: frames more than 1/32 s after the last kept one
            for n in range(1, len(assoc)):
                if t_image[assoc[n][0]] - t_image[assoc[keep[-1]][0]] > 1.0 / 32:
                    keep.append(n)
            assoc = [assoc[n] for n in keep] if assoc else []
        if not assoc:
            raise ValueError(f"{f}: no colour frame has a depth image and a pose within max_dt")
        color_paths = [os.path.join(f, image_data[i, 1]) for i, _, _, _ in assoc]
        depth_paths = [os.path.join(f, depth_data[j, 1]) for _, j, _, _ in assoc]
        if len(color_paths) != len(depth_paths):
            raise ValueError(f"{f}: number of color and depth images must be the same")
        to_pose = _pose_utmm if utmm else _pose_tum
        c2w = [torch.from_numpy(to_pose(pose_vecs[k])).float() for _, _, k, _ in assoc]
        tstamps = [t_image[i] for i, _, _, _ in assoc]
        num = len(color_paths)
        if start < 0:
            raise ValueError(f"start_idx must not be negative, got {start}")
        if not (end == -1 or end > start):
            raise ValueError(f"early_stop_idx ({end}) must be -1 (all frames) or greater than start_idx ({start})")
        if end == -1:
            end = num
        sl = slice(start, end, stride)
        self.color_paths, self.depth_paths, self.c2w, self.tstamps = color_paths[sl], depth_paths[sl], c2w[sl], tstamps[sl]
        if not self.color_paths:
            raise ValueError(f"{f}: no frame left in [{start}:{end}:{stride}] of {num}")
        self.tf, self.imus = {}, None
        if utmm:
            imus = [torch.from_numpy(imu_vecs[l, :]).float() for _, _, _, l in assoc]
            self.imus, idx = [], 0                      # basedataset.py:196-213, as written (see the module docstring)
            while idx < end:
                cat = torch.empty(0)
                for _ in range(stride):
                    if idx >= end:
                        break
                    cat = torch.cat([cat, imus[idx]], dim=0)
                    idx += 1
                self.imus.append(cat)
            tf_data = _parse_list(os.path.join(f, "tf.txt"), min_cols=7).astype(np.float64).reshape(-1)
            self.tf = {"c2i": torch.from_numpy(np.linalg.inv(_pose_tum(tf_data))).float()}      # tf.txt is IMU -> camera (utmm.py:299-309)

    def __len__(self):
        return len(self.color_paths)

    def imu(self, i):
        """IMU rows of frame i (a fresh float32 tensor on the device: the host predictor subtracts gravity in place)."""
        if self.imus is None:
            raise ValueError(f"{self.folder}: a {self.name} sequence has no IMU rows (tracking.dynamics_model: imu needs dataset utmm)")
        return self.imus[i].to(self.device).type(torch.float32).clone()

    # ---- frames --------------------------------------------------------------------------------------------------------------------
    def _est_files(self, folder):
        """The estimate file of every kept colour frame (after slicing and the `frames` cap): same stem, .npy before .png."""
        paths = []
        for c in self.color_paths:
            stem = os.path.splitext(os.path.basename(c))[0]
            found = next((p for p in (os.path.join(folder, stem + ext) for ext in (".npy", ".png")) if os.path.isfile(p)), None)
            if found is None:
                raise ValueError(f"{os.path.join(folder, stem + '.npy')}: missing depth estimate of {c} (neither .npy nor .png)")
            paths.append(found)
        return paths

    def _decode_est_into(self, i, slot):
        slot.est_idx = None
        raw = self._est_decoder(self.est_paths[i])
        if raw.shape != slot.est.shape or raw.dtype != slot.est.dtype:
            raise ValueError(f"{self.est_paths[i]}: depth estimate is {raw.dtype} {tuple(raw.shape)}, the first frame's "
                             f"({self.est_paths[0]}) is {slot.est.dtype} {tuple(slot.est.shape)}")
        np.copyto(slot.est, raw)
        slot.est_idx = i

    def _est(self, i):
        """The monocular estimate of frame i, float32 [H,W] on the device: a fresh tensor on every call.  After ``seq[i]`` the slot still
        holds the decoded (and, on the device path, uploaded) array; otherwise the file is decoded into the slot no prefetch writes to."""
        if not 0 <= i < len(self):
            raise IndexError(i)
        slot = self._slots[1 - self._next]      # (a pending prefetch always targets _slots[_next])
        if slot.est_idx != i:
            slot.wait()
            self._decode_est_into(i, slot)
        scale = self.est_depth_scale if slot.est.dtype == np.uint16 else 1.0
        if not self.on_device:
            return ingest_est_host(slot.est, scale, self.H, self.W, self.device)
        if slot.est_dev_idx != i:
            slot.upload_est()
        return ingest_est_device(slot.est_dev, scale, self.H, self.W)

    def _decode_into(self, i, slot):
        if self.est_paths is not None:
            slot.est_idx = None
        rgb, depth = self._decoder(self.color_paths[i], self.depth_paths[i])
        for arr, path, want in ((rgb, self.color_paths[i], (self.Hs, self.Ws, 3)), (depth, self.depth_paths[i], (self.Hs, self.Ws))):
            if tuple(arr.shape) != want:
                raise ValueError(f"{path}: image is {tuple(arr.shape)}, cam.image_height / image_width say {want}")
        np.copyto(slot.rgb, rgb)
        np.copyto(slot.depth, depth)
        if self.est_paths is not None:
            self._decode_est_into(i, slot)

    def _staged(self, i):
        """The slot that holds the decoded frame i: the prefetched one if the hint was right, a synchronous decode otherwise."""
        pending, self._pending = self._pending, None
        if pending is not None:
            p_idx, slot, fut = pending
            try:
                fut.result()
            except Exception:
                if p_idx == i:
                    raise
            if p_idx != i:      # a wrong hint: the slot is free (its upload was waited for before the decode was queued)
                self._decode_into(i, slot)
            return slot
        slot = self._slots[self._next]
        slot.wait()
        self._decode_into(i, slot)
        return slot

    def __getitem__(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        slot = self._staged(i)
        if self.on_device:
            slot.upload()
            color, depth = ingest_device(slot.rgb_dev, slot.depth_dev, self.png_depth_scale, self.H, self.W)
        else:
            color, depth = ingest_host(slot.rgb, slot.depth, self.png_depth_scale, self.H, self.W, self.device)
        other = self._slots[1 - self._slots.index(slot)]
        self._next = self._slots.index(other)
        if self._pool is not None and i + 1 < len(self):
            other.wait()        # on this thread: the worker touches host memory only
            self._pending = (i + 1, other, self._pool.submit(self._decode_into, i + 1, other))
        return color, depth, self.poses[i]

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool, self._pending = None, None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
