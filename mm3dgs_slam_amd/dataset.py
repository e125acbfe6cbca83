"""Recorded RGB-D sequences from disk: TUM-format and UT-MM-format directories (reference ``gradslam_datasets/tum.py``, ``utmm.py``,
``basedataset.py``), as a frame source with the protocol of ``slam.SyntheticSequence`` (``len``, ``seq[i] -> (color [3,H,W], depth
[H,W], gt_pose [7] world->camera)`` on ``cfg["device"]``, ``poses``, ``tstamps``, ``tf``, ``imu(i)``; no ``est``: the monocular
network is out of scope, so with ``use_gt_depth: false`` the loop uses the sensor depth).

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
touches host memory only, and a prefetched frame is only a hint -- any access order gives the same frames."""
from __future__ import annotations

import ctypes as C
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
    _lib.check(_lib.load().mm3dgs_ingest_frame(Hs, Ws, C.c_void_p(rgb_dev.data_ptr()), None if depth_dev is None else C.c_void_p(depth_dev.data_ptr()),
                                               float(png_depth_scale), int(H), int(W), C.c_void_p(color.data_ptr()),
                                               None if d is None else C.c_void_p(d.data_ptr()), _stream()))
    return color, d


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


def write_tum_sequence(folder, frames, poses, tstamps):
    """Record frames as a TUM-format directory: `frames` = [(uint8 [H,W,3], uint16 [H,W])], `poses` = world->camera 7-vectors (the
    package's layout), `tstamps` in seconds.  rgb/NNNN.png, depth/NNNN.png, rgb.txt, depth.txt, groundtruth.txt."""
    from PIL import Image
    from scipy.spatial.transform import Rotation
    from .pose_utils import get_camera_from_tensor
    os.makedirs(os.path.join(folder, "rgb"), exist_ok=True)
    os.makedirs(os.path.join(folder, "depth"), exist_ok=True)
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
    """One staging slot: host arrays the decoder writes (pinned on the device path), their raw device copies, the event of the last upload."""

    def __init__(self, Hs, Ws, device, on_device):
        self.event = None
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
        if self.event is None:
            self.event = torch.cuda.Event()
        self.event.record()


class RecordedSequence:
    """See the module docstring.  Config keys (the reference's): dataset (tum | utmm), inputdir, scene, start_idx, stride,
    early_stop_idx, desired_height, desired_width, cam.{image_height, image_width, fx, fy, cx, cy, png_depth_scale}; plus
    ingest_on_device and prefetch.  The constructor writes the intrinsics scaled to the desired size back into ``cfg["cam"]`` (Python
    floats; float32 arithmetic of datautils.scale_intrinsics) -- build it BEFORE a Renderer is built from that cfg.  `frames` caps the
    length (slam_top's --frames)."""

    def __init__(self, cfg, frames=None, decoder=decode_png):
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
        self._slots = [_Slot(self.Hs, self.Ws, self.device, self.on_device) for _ in range(2)]
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
    def _decode_into(self, i, slot):
        rgb, depth = self._decoder(self.color_paths[i], self.depth_paths[i])
        for arr, path, want in ((rgb, self.color_paths[i], (self.Hs, self.Ws, 3)), (depth, self.depth_paths[i], (self.Hs, self.Ws))):
            if tuple(arr.shape) != want:
                raise ValueError(f"{path}: image is {tuple(arr.shape)}, cam.image_height / image_width say {want}")
        np.copyto(slot.rgb, rgb)
        np.copyto(slot.depth, depth)

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
