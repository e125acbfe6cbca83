"""Shapes and sources shared by tests/test_est_depth.py and tests/test_gpu_est_depth.py (the monocular depth estimate read from disk)."""
import numpy as np
import torch

# (source, output, the sizes are equal)
SHAPES = [((5, 7), (5, 7), True),           # general path at identity
          ((8, 12), (8, 12), True),         # packed path
          ((36, 68), (36, 68), True),       # packed path, several workgroups and a tail
          ((6, 8), (3, 4), False),          # integer downscale
          ((7, 9), (5, 4), False),          # non-integer downscale
          ((4, 5), (6, 10), False),         # upscale, both borders clamp
          ((24, 32), (30, 40), False),      # the network's 0.8 ratio
          ((3, 130), (2, 300), False),      # more than one workgroup per row
          ((1, 1), (3, 5), False), ((3, 4), (1, 1), False)]      # degenerate sizes
DTYPES = (np.float32, np.float16, np.uint16)      # dtype codes 0, 1, 2 of mm3dgs_ingest_est
# (dtype, scale): every dtype at 1.0, uint16 also at 0.25
CASES = [(np.float32, 1.0), (np.float16, 1.0), (np.uint16, 1.0), (np.uint16, 0.25)]


def source(Hs, Ws, dtype, seed=0):
    """A raw estimate [Hs,Ws]: MiDaS-like magnitudes (float: up to ~3000; uint16: the full range), extremes planted where there is room."""
    g = torch.Generator().manual_seed(1000 * Hs + Ws + seed)
    if dtype == np.uint16:
        a = torch.randint(0, 65536, (Hs, Ws), generator=g).numpy().astype(np.uint16)
        planted = (0, 1, 65535)
    else:
        a = (torch.rand(Hs, Ws, generator=g, dtype=torch.float64) * 3000.0).numpy().astype(dtype)
        planted = (0.0, 1e-3, 3000.0)
    flat = a.reshape(-1)
    for k, v in enumerate(planted[:max(0, flat.size - 1)]):
        flat[-1 - k] = v
    return np.ascontiguousarray(a)
