"""Small tensor helpers with the reference's conventions (``utils/general_utils.py``): ``inverse_sigmoid`` (:21-22),
``build_rotation`` (:78-99, quaternion (w,x,y,z) normalised), ``build_scaling_rotation`` (:101-110),
``strip_symmetric``/``strip_lowerdiag`` (:64-76: [xx,xy,xz,yy,yz,zz]), ``get_expon_lr_func`` (:32-62).  Device follows
the inputs (the reference hard-codes "cuda")."""
import numpy as np
import torch

from .pose_utils import quad2rotation


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def build_rotation(r):
    return quad2rotation(r)


def build_scaling_rotation(s, r):
    return build_rotation(r) * s[:, None, :]          # R @ diag(s)


def strip_lowerdiag(L):
    return torch.stack([L[:, 0, 0], L[:, 0, 1], L[:, 0, 2], L[:, 1, 1], L[:, 1, 2], L[:, 2, 2]], 1)


strip_symmetric = strip_lowerdiag


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """Log-linear interpolation lr_init -> lr_final over max_steps with an optional sine warm-up."""
    def lr_at(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        warm = 1.0
        if lr_delay_steps > 0:
            warm = lr_delay_mult + (1 - lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
        t = np.clip(step / max_steps, 0, 1)
        return warm * np.exp((1 - t) * np.log(lr_init) + t * np.log(lr_final))
    return lr_at


# ---- the split samples of densification (GaussianModel.densify_and_split; csrc/compact.hip mirrors this bit for bit) ----------
# The reference draws them with torch.normal (slam/gaussian_model.py:496-498), which no two devices reproduce.  Here they come from a
# stateless counter-based generator instead: murmur3's fmix32 finaliser over (seed, parent row, child k, draw j), 24-bit uniforms,
# Box-Muller.  The integer part is exact int64 tensor arithmetic (no product exceeds 2^49); the float part is float32 in the order the
# kernel evaluates it.
_M32 = 0xFFFFFFFF
TWO_PI_F32 = float(np.float32(2.0 * np.pi))


def _mul32(h, c):
    """(h * c) mod 2^32 for h < 2^32 held in int64, without a product that overflows 63 bits."""
    return (h * (c & 0xFFFF) + (((h * (c >> 16)) & 0xFFFF) << 16)) & _M32


def fmix32(h):
    """murmur3's 32-bit finaliser on an int64 tensor (or a Python int) of values < 2^32."""
    h = h ^ (h >> 16)
    h = _mul32(h, 0x85EBCA6B)
    h = h ^ (h >> 13)
    h = _mul32(h, 0xC2B2AE35)
    return h ^ (h >> 16)


def densify_keys(seed, rows, N):
    """uint32 keys (as int64) [N, len(rows), 6]: key_j = fmix32(fmix32(fmix32(seed) ^ row) ^ (8 k + j))."""
    r = torch.as_tensor(rows).to(torch.int64).reshape(-1)
    base = fmix32(fmix32(int(seed) & _M32) ^ r)
    kj = 8 * torch.arange(N, dtype=torch.int64, device=r.device)[:, None] + torch.arange(6, dtype=torch.int64, device=r.device)[None, :]
    return fmix32(base[None, :, None] ^ kj[:, None, :])


def densify_normals(seed, rows, N):
    """Standard normal samples [N * len(rows), 3] for the children of the split rows `rows` (indices before densification), in the
    reference's draw order (`.repeat(N, 1)`: child k of parent s is row k * len(rows) + s).  u_j = ((key_j >> 8) + 0.5) 2^-24,
    z_a = sqrt(-2 ln u_2a) cos(2 pi u_2a+1)."""
    key = densify_keys(seed, rows, N)
    u = ((key >> 8).to(torch.float32) + 0.5) * (2.0 ** -24)
    z = torch.sqrt(-2.0 * torch.log(u[..., 0::2])) * torch.cos(u[..., 1::2] * TWO_PI_F32)
    return z.reshape(-1, 3)


def densify_seed(base, frame, iteration):
    """The 31-bit seed of a densification step of the mapping loops: a hash of (mapping.densify_seed, frame index, iteration), so that
    a re-run of the same step (the native loop's overflow recovery) draws the same samples."""
    return fmix32(fmix32(fmix32(int(base) & _M32) ^ (int(frame) & _M32)) ^ (int(iteration) & _M32)) & 0x7FFFFFFF


def densify_frame(mapping_cfg, frame):
    """Whether the pruning steps of this frame's mapping loop densify: `mapping.densify` (default false) and every
    densification_interval-th frame (the reference's commented-out call site, slam/mapper.py:913-927)."""
    return bool(mapping_cfg.get("densify", False)) and frame % int(mapping_cfg["densification_interval"]) == 0
