"""The host reference of the per-tile lists (tests/list_ref.py) checked on its own, without a GPU: on random splat records from the
float32 projection of synthetic clouds, the float32 mirror of the block masks must keep the float64 property it is meant to keep
(no left-out block reaches alpha 1/255), stay inside the block rectangle, and leave only a handful of bits to the error band of
the hardware log; the depth order must be the float64 oracle's (tile, depth, id) order."""
import numpy as np
import pytest
import torch

from oracle.raster_ref import RefSettings, bin_ref, preprocess_ref
from tests import list_ref as lr
from tests import parity_util as pu


def _pre(P, H, W, seed, log_scale=-3.0, low_opacity=0.0):
    case = pu.make_case(P=P, H=H, W=W, seed=seed, log_scale=log_scale)
    dt = torch.float32
    op = case["opacities"].to(dt).clone()
    if low_opacity:      # opacities below 1/255 (mask mode 0: nothing listed) and just above it (tau near 0)
        g = torch.Generator().manual_seed(seed + 11)
        sel = torch.rand(P, generator=g) < low_opacity
        op[sel] = (torch.rand(int(sel.sum()), 1, generator=g) * 2.0 / 255.0).to(dt)
    s = RefSettings(H, W, case["tanx"], case["tany"], case["bg"].to(dt), 1.0, case["view"].to(dt), case["proj"].to(dt), 0,
                    case["campos"].to(dt))
    with torch.no_grad():
        pre = preprocess_ref(case["means3D"].to(dt), None, op, None, case["colors"].to(dt), case["scales"].to(dt),
                             case["rotations"].to(dt), None, s)
    return pre


def _pairs(pre):
    """Every (Gaussian, tile) pair of the projection: the float32 splat words A, B, the rectangle, the tile."""
    gx, gy = pre["grid"]
    ids, ranges = bin_ref(pre)
    tile = np.repeat(np.arange(gx * gy), np.diff(ranges.numpy()))
    ids = ids.numpy()
    xy, con, op = pre["xy"].numpy(), pre["conic"].numpy(), pre["opacity"].numpy()
    A = np.stack([xy[ids, 0], xy[ids, 1], con[ids, 0], con[ids, 1]], 1).astype(np.float32)
    B = np.stack([con[ids, 2], op[ids], np.zeros_like(op[ids]), np.zeros_like(op[ids])], 1).astype(np.float32)
    rect = np.stack([r.numpy() for r in pre["rect"]], 1)[ids]
    return ids, tile % gx, tile // gx, A, B, rect


@pytest.mark.parametrize("seed,log_scale,low", [(0, -3.0, 0.0), (1, -2.2, 0.2), (2, -3.6, 0.1)])
def test_mirror_masks_keep_the_float64_alpha_bound(seed, log_scale, low):
    pre = _pre(6000, 96, 136, seed, log_scale, low)
    ids, ttx, tty, A, B, rect = _pairs(pre)
    assert ids.size > 5000
    lower, upper = lr.mask_band(A, B, rect, ttx, tty)
    assert np.all((lower & ~upper) == 0), "the mask must grow with tau"
    # the property holds for the SMALLER mask (more blocks left out): then it holds for anything the kernel may choose in the band
    amax = lr.max_alpha_outside(A, B, ttx, tty, lower)
    assert amax.max() < lr.ALPHA_MIN * (1.0 - lr.PROPERTY_MARGIN), amax.max() * 255
    # and the mask is not trivially conservative: most pairs leave some block out, and the listed blocks do reach 1/255 somewhere
    full = lr.max_alpha_outside(A, B, ttx, tty, np.zeros_like(lower))
    listed = lower != 0
    assert (lower != 0xffff).mean() > 0.3
    assert (full[listed] >= lr.ALPHA_MIN * 0.5).mean() > 0.9
    amb = int(lr.popcount(upper & ~lower).sum())
    assert amb <= 1e-4 * 16 * ids.size, (amb, ids.size)
    if low:
        assert ((B[:, 1] * np.float32(255.0)) <= 1.0).sum() > 50 and not lower[(B[:, 1] * np.float32(255.0)) < 1.0].any()


def test_mirror_masks_lie_inside_the_block_rectangle():
    pre = _pre(6000, 96, 136, 3, -2.5, 0.05)
    ids, ttx, tty, A, B, rect = _pairs(pre)
    for tau in lr.tau_band(B[:, 1]):
        mc = lr.mask_consts(A, B, tau)
        bx0, by0, bw, bh = lr.block_rect(A, B, rect, tau)
        m = lr.tile_block_mask_in_rect(mc, ttx, tty, (bx0, by0, bw, bh))
        # the bits of the block rectangle alone (mode 2 = every block of the rectangle)
        full = lr.tile_block_mask_in_rect((mc[0], mc[1], mc[2], mc[3], mc[4], np.full_like(mc[5], 2)), ttx, tty, (bx0, by0, bw, bh))
        assert np.all((m & ~full) == 0)
        # the rectangle lies inside the tile rectangle, in blocks
        nz = (bw > 0) & (bh > 0)
        assert np.all(bx0[nz] >= 4 * rect[nz, 0]) and np.all(bx0[nz] + bw[nz] <= 4 * rect[nz, 2])
        assert np.all(by0[nz] >= 4 * rect[nz, 1]) and np.all(by0[nz] + bh[nz] <= 4 * rect[nz, 3])
        # and every listed block is inside the image's tile grid of this pair
        assert np.all(m <= 0xffff)


def test_order_function_agrees_with_the_oracle_binning():
    pre = _pre(3000, 80, 112, 4, -2.6)
    gx, gy = pre["grid"]
    ids, ranges = bin_ref(pre)
    depth = pre["depth"].numpy().astype(np.float32)
    rect = np.stack([r.numpy() for r in pre["rect"]], 1)
    radii = pre["radii"].numpy()
    lens = []
    for t in range(gx * gy):
        exp = ids[ranges[t]:ranges[t + 1]].numpy()
        got = lr.expected_order(depth, rect, radii, t, gx)
        assert np.array_equal(got, exp), t
        lens.append(got.size)
    assert max(lens) > 100


def test_buffer_offsets_follow_the_library_sizes():
    """The readers' layouts end where the library's own size functions say the buffers end (csrc/mm3dgs_common.h)."""
    from mm3dgs_slam_amd import _lib
    lib = _lib.load()      # (built by __graft_entry__.build(); its size functions are pure host arithmetic)
    al = lambda v: (v + 255) // 256 * 256
    for P in (1, 255, 256, 257, 1000, 300001):
        o = lr.geom_offsets(P)
        assert o["poserec"] + lr._al(P * 20 * 4) == lib.mm3dgs_geom_bytes(P)
        # splat | depth | rect | clamped | tileoff | block_tiles | poserec, written out
        assert al(48 * P) + al(4 * P) + al(8 * P) + al(P) + al(4 * P) + al(4 * ((P + 255) // 256 + 1)) + al(80 * P) == lib.mm3dgs_geom_bytes(P)
    for H, W in ((48, 64), (120, 168), (1080, 1920)):
        o = lr.image_offsets(H, W)
        T = ((W + 15) // 16) * ((H + 15) // 16)
        assert o["tile_order"] + lr._al(4 * max((T + 7) // 8 * 8, 8 * 256)) == lib.mm3dgs_image_bytes(H, W)
    for N in (1, 65536, 1000003):
        o = lr.bin_offsets(N)
        assert o["trec"] + lr._al(4 * N) == lib.mm3dgs_binning_bytes(N)
