"""Debug outputs of a run (reference ``slam/SLAM.py:116-139,148-195,233-276,450-485``, ``slam/mapper.py:991-1000``): the per-frame 2 x 3
mosaic of ``debug.create_video``, the image-over-depth pairs of ``SLAM.render()`` and the keyframe images of ``debug.save_keyframes``.

A mosaic is ``rows x cols`` panels of H x W pixels, each a ``(kind, a, b)`` triple, row-major:

* ``(COLOR, a, None)``: a float32 ``[3,H,W]`` image;
* ``(ABSDIFF, a, b)``: ``torch.abs(a - b)`` of two of them;
* ``(DEPTH, a, None)``: a float32 ``[H,W]`` depth image through the reference's ``depth_to_rgb`` (``utils/depth_utils.py:14-34``: normalise by
  the image's own minimum and maximum, matplotlib's ``viridis``).

The result is one uint8 ``[rows H, cols W, 3]`` image.  Two paths give the same bytes, every one (tests/test_gpu_debug_frames.py):

* ``compose_host``: the reference's operator chain, literally, in torch on the CPU -- the path of ``device: cpu`` and the yardstick;
* ``compose_device``: one call of ``mm3dgs_mosaic`` (csrc/mosaic.hip, semantics in include/mm3dgs.h) on the current stream; only the
  finished bytes leave the device.  The reference's chain costs three device -> host -> device round trips per frame.

The colour table is matplotlib's ``viridis`` (released under CC0), committed as data (``viridis.txt``: 256 rows of R G B, float64, written
with 17 significant digits) so that nothing here imports matplotlib at run time; matplotlib's lookup of a float x in [0, 1] is
``table[min(int(x * 256), 255)]``, and a NaN takes its "bad" colour (0, 0, 0, 0).

Quantisers (``quant``): 0 is the debug video's ``(vid_image * 255).to(torch.uint8)`` on the float64 tensor that ``torch.cat`` of a float32
image and a float64 colour map produces, saturating outside [0, 1] (where the reference is undefined); 1 is ``torchvision.utils.save_image``'s
``mul(255).add_(0.5).clamp_(0, 255).to(uint8)`` on the same float64 tensor, as ``SLAM.render()`` uses.  A NaN gives 0 in both.

``FrameSink`` writes frames as numbered PNG files from one writer thread; an mp4 container is out of scope (INTEGRATION.md has the ffmpeg
line that turns the folder into a video).
"""
from __future__ import annotations

import ctypes as C
import os
import queue
import threading

import numpy as np
import torch

COLOR, ABSDIFF, DEPTH = 0, 1, 2

_HERE = os.path.dirname(os.path.abspath(__file__))
_table = None
_lut_host = {}
_lut_dev = {}
_buffers = {}


def viridis():
    """matplotlib's viridis as a float64 [256,3] tensor (RGB in [0,1])."""
    global _table
    if _table is None:
        t = np.loadtxt(os.path.join(_HERE, "viridis.txt"), dtype=np.float64)
        if t.shape != (256, 3):
            raise RuntimeError(f"viridis.txt holds {t.shape}, not 256 rows of R G B")
        _table = torch.from_numpy(t)
    return _table


def quantise(img, quant):
    """float64 tensor -> uint8 with the rule of `quant` (module docstring)."""
    p = img.double() * 255
    if quant:
        p = p + 0.5
    return torch.nan_to_num(p, nan=0.0).clamp(0, 255).to(torch.uint8)


def lut_u8(quant):
    """The colour table quantised with the rule of `quant`: uint8 [256,3] on the CPU."""
    q = 1 if quant else 0
    if q not in _lut_host:
        _lut_host[q] = quantise(viridis(), q).contiguous()
    return _lut_host[q]


def depth_to_rgb_host(depth):
    """utils/depth_utils.py:14-34 on the CPU with the committed table in place of the matplotlib call: float32 arithmetic, float64 [3,H,W]
    result; a NaN of the normalised image is (0, 0, 0)."""
    depth = depth.detach().float().cpu()
    lo, hi = torch.min(depth), torch.max(depth)
    t = torch.clamp((depth - lo) / (hi - lo), min=0, max=1)
    bad = torch.isnan(t)
    idx = torch.where(bad, torch.zeros_like(t), t * 256).to(torch.int64).clamp(max=255)
    rgb = viridis()[idx]                                    # [H,W,3] float64
    rgb = torch.where(bad[..., None], torch.zeros_like(rgb), rgb)
    return rgb.permute(2, 0, 1)


def _check_panels(panels, rows, cols):
    if rows <= 0 or cols <= 0 or rows * cols > 8 or len(panels) != rows * cols:
        raise ValueError(f"a mosaic has rows x cols <= 8 panels, got {rows} x {cols} with {len(panels)} panels")
    H, W = int(panels[0][1].shape[-2]), int(panels[0][1].shape[-1])
    for kind, a, b in panels:
        want = (H, W) if kind == DEPTH else (3, H, W)
        if kind not in (COLOR, ABSDIFF, DEPTH) or tuple(a.shape) != want or (kind == ABSDIFF and (b is None or tuple(b.shape) != want)):
            raise ValueError(f"panel of kind {kind}: expected {want}, got {tuple(a.shape)}" + ("" if b is None else f" and {tuple(b.shape)}"))
    return H, W


def compose_host(panels, rows, cols, quant=0, bgr=False):
    """The mosaic by the reference's operator chain on the CPU: uint8 [rows H, cols W, 3]."""
    _check_panels(panels, rows, cols)
    images = []
    for kind, a, b in panels:
        if kind == DEPTH:
            images.append(depth_to_rgb_host(a))
        elif kind == ABSDIFF:
            images.append(torch.abs(a.detach().float().cpu() - b.detach().float().cpu()))
        else:
            images.append(a.detach().float().cpu())
    strips = [torch.cat(images[r * cols:(r + 1) * cols], dim=2) for r in range(rows)]
    # (a strip of colour panels only is float32; torch.cat with a float64 strip widens it exactly, and so does quantise)
    out = quantise(torch.cat([s.double() for s in strips], dim=1), quant).permute(1, 2, 0)
    if bgr:
        out = out.flip(2)
    return out.contiguous()


def mosaic_call(H, W, rows, cols, kinds, a_ptrs, b_ptrs, lut_ptr, quant, bgr, work_ptr, out_ptr):
    """``mm3dgs_mosaic`` on the current stream with raw device addresses (0 / None: NULL); returns the library's return code."""
    from . import _lib
    from .rasterizer import _stream
    n = len(kinds)
    kind_arr = (C.c_int32 * n)(*[int(k) for k in kinds])
    a_arr = (C.c_void_p * n)(*[p or None for p in a_ptrs])
    b_arr = (C.c_void_p * n)(*[p or None for p in b_ptrs])
    return _lib.load().mm3dgs_mosaic(int(H), int(W), int(rows), int(cols), kind_arr, a_arr, b_arr, lut_ptr or None, int(quant), int(bool(bgr)),
                                     work_ptr or None, out_ptr or None, _stream())      # (a c_void_p parameter takes the address as it is)


def compose_device(panels, rows, cols, quant=0, bgr=False):
    """The mosaic by ``mm3dgs_mosaic`` on the current stream: uint8 [rows H, cols W, 3] on the panels' device.  The result and the work
    buffer are allocated once per shape and device: the returned tensor is overwritten by the next call with the same shape (stream-ordered:
    copy it, or enqueue its use, before that)."""
    from . import _lib
    H, W = _check_panels(panels, rows, cols)
    dev = panels[0][1].device
    keep = []

    def plane(t):
        if t.device != dev:
            raise ValueError("compose_device: the panels live on different devices")
        t = t.detach()
        if t.dtype != torch.float32 or not t.is_contiguous():
            t = t.float().contiguous()
        keep.append(t)
        return t.data_ptr()

    a_ptrs = [plane(a) for _, a, _ in panels]
    b_ptrs = [plane(b) if kind == ABSDIFF else 0 for kind, _, b in panels]
    q = 1 if quant else 0
    if (q, dev) not in _lut_dev:
        _lut_dev[(q, dev)] = lut_u8(q).to(dev)
    key = (H, W, rows, cols, dev)
    if key not in _buffers:
        nbytes = int(_lib.load().mm3dgs_mosaic_work_bytes(H, W, rows, cols))
        if nbytes <= 0:
            raise ValueError(f"compose_device: {rows} x {cols} panels of {H} x {W} is not a shape mm3dgs_mosaic takes")
        _buffers[key] = (torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(rows * H, cols * W, 3, dtype=torch.uint8, device=dev))
    work, out = _buffers[key]
    _lib.check(mosaic_call(H, W, rows, cols, [k for k, _, _ in panels], a_ptrs, b_ptrs, _lut_dev[(q, dev)].data_ptr(), q, bgr, work.data_ptr(),
                           out.data_ptr()))
    return out


def compose(panels, rows, cols, quant=0, bgr=False):
    """``compose_device`` for panels on a GPU, ``compose_host`` otherwise -- the same bytes either way.  On a GPU the library is required:
    a missing library is an error, not a reason to compose on the host."""
    if panels[0][1].is_cuda:
        return compose_device(panels, rows, cols, quant, bgr)
    return compose_host(panels, rows, cols, quant, bgr)


def save_png(frame, path):
    """uint8 [H,W,3] tensor (any device) -> PNG, synchronously."""
    from PIL import Image
    Image.fromarray(frame.detach().cpu().contiguous().numpy()).save(path, compress_level=1)


def keyframe_u8(color):
    """A float32 [3,H,W] image as ``torchvision.utils.save_image`` stores it: mul(255).add(0.5).clamp(0, 255).to(uint8) on the tensor's
    device, as [H,W,3]."""
    return color.detach().mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


class FrameSink:
    """Numbered PNG frames ``dir/{n:06d}_{idx:05d}_{name}.png`` (n counts the frames handed in) written by ONE thread.

    ``put`` copies the finished frame into one of two host buffers -- pinned, non-blocking and followed by an event for a frame on a GPU --
    and returns; the writer thread waits for the event, encodes the PNG (PIL, ``compress_level=1``) and only then gives the buffer back, so
    a slot is never reused before its file is written: a third ``put`` waits for the writer.  The thread touches host memory only.
    ``close`` drains the queue, joins the thread and raises what the writer failed with, if anything."""

    SLOTS = 2

    def __init__(self, directory):
        self.dir = directory
        os.makedirs(directory, exist_ok=True)
        self.n = 0
        self._bufs = None
        self._free = queue.Queue()
        self._todo = queue.Queue()
        self._error = None
        self._thread = threading.Thread(target=self._write_loop, name="mm3dgs-frame-sink", daemon=True)
        self._thread.start()

    def put(self, frame, idx, name):
        if self._thread is None:
            raise RuntimeError("FrameSink.put after close")
        if self._bufs is None:
            self._bufs = [torch.empty(frame.shape, dtype=torch.uint8, pin_memory=frame.is_cuda) for _ in range(self.SLOTS)]
            for s in range(self.SLOTS):
                self._free.put(s)
        if frame.dtype != torch.uint8 or frame.shape != self._bufs[0].shape:
            raise ValueError(f"FrameSink: frame {frame.dtype} {tuple(frame.shape)}, expected uint8 {tuple(self._bufs[0].shape)}")
        slot = self._free.get()
        self._bufs[slot].copy_(frame, non_blocking=True)
        event = None
        if frame.is_cuda:
            event = torch.cuda.Event()
            event.record()
        path = os.path.join(self.dir, f"{self.n:06d}_{int(idx):05d}_{name}.png")
        self.n += 1
        self._todo.put((slot, event, path))
        return path

    def _write_loop(self):
        from PIL import Image
        while True:
            item = self._todo.get()
            if item is None:
                return
            slot, event, path = item
            try:
                if event is not None:
                    event.synchronize()
                Image.fromarray(self._bufs[slot].numpy()).save(path, compress_level=1)
            except Exception as e:      # noqa: BLE001 -- kept for close(): the run goes on without this frame
                if self._error is None:
                    self._error = e
            finally:
                self._free.put(slot)

    def close(self):
        if self._thread is None:
            return
        self._todo.put(None)
        self._thread.join()
        self._thread = None
        if self._error is not None:
            raise self._error
