"""The per-tile sort and the sixteen 4x4-block lists of every entry point, read back from the state buffers and compared EXACTLY with
the host reference of tests/list_ref.py on every tile: depth order (through the unique per-tile records of the sorted bin words),
block masks (float32 mirror of tile_mask.h, the hardware log's band excluded and counted), block lists and subcount, the float64
alpha bound of every left-out block, and the header words.  Each test asserts that its scenes reach the sort tiers it is there for
(list lengths <= 1024: rank sort + run merge; (1024, 2048]: bitonic_lds_regs in 2048 keys; (2048, 16384]: in 16384 keys or, inside the
fused kernels, the global-memory network; > 16384: the global-memory network), and the SLAM rows compare their block lists with each
other: packed bins, direct bins, separate and fused sort launches, forward and tracking launches list the same splats."""

import numpy as np
import pytest
import torch

from tests import list_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (P, H, W, seed, scale offset, every n-th splat enlarged by 3.5 in log scale (0: none)).  Tile lengths per tier (<= 1024, (1024, 2048],
# (2048, 16384], > 16384) as the float64 oracle's projection predicts them, packed bins: MIXED [15, 33, 40, 0], CROWDED [0, 0, 7, 5];
# direct bins (empty pairs dropped): MIXED [19, 69, 0, 0], DENSE [13, 38, 37, 0] (longest 2377: inside the 1.5 * 2048 + 128 span)
MIXED = (20000, 120, 168, 3, 0.0, 97)
DENSE = (20000, 120, 168, 3, 0.15, 97)
CROWDED = (20000, 48, 64, 3, 1.0, 0)
FAINT = 0.05     # fraction of the splats with an opacity below 2 / 255 (half of them under 1/255: mask mode 0, the direct bins' empty-pair drop)


def _scene(P, H, W, seed, add, huge_every):
    from mm3dgs_slam_amd import synthetic as syn
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.gaussian_model import GaussianModel
    from mm3dgs_slam_amd.renderer import Renderer
    cfg = default_config(device=DEV, height=H, width=W)
    c = cfg["cam"]
    color, depth = syn.rgbd_frame(H, W, seed=seed)
    G = syn.seed_gaussians(color, depth, c["fx"], c["fy"], c["cx"], c["cy"], P, seed=seed, isotropic=False)
    g = GaussianModel(cfg)
    g.training_setup()
    gen = torch.Generator().manual_seed(seed)
    sc = G["scaling"] + torch.tensor([1.2, -0.8, 0.0]) + add        # anisotropic, several tiles per splat
    if huge_every:
        sc[::huge_every] += 3.5                                    # splats of more than 32 tiles (the wave-cooperative binning path)
    logit = torch.randn(P, 1, generator=gen) * 1.5
    faint = torch.rand(P, generator=gen) < FAINT
    o = torch.rand(int(faint.sum()), 1, generator=gen) * (2.0 / 255.0) + 1e-5
    logit[faint] = torch.log(o / (1.0 - o))
    g.densification_postfix(G["xyz"].to(DEV), G["f_dc"].to(DEV), torch.zeros(P, 0, 3, device=DEV), logit.to(DEV), sc.to(DEV),
                            (G["rotation"] * (0.5 + torch.rand(P, 1, generator=gen))).to(DEV), G["rgb"].to(DEV))
    pose = torch.tensor([0.995, 0.03, -0.02, 0.04, 0.03, -0.02, 0.05], device=DEV) * 1.3
    pose[4:] /= 1.3
    return cfg, g, Renderer(cfg), pose, color.to(DEV)


def _report(name, stats, extra=""):
    print(f"\n[lists] {name}: tiers {lr.tier_counts(stats.lens)} {stats} {extra}")


def _slam_state(eng):
    return lr.ListState(eng.geom, eng.img_state, eng.binning, eng.P, eng.H, eng.W, eng.n_cap, eng.radii)


def _trec_cap(eng):
    """api.hip slam_direct_bins: per-tile records per projection workgroup."""
    nb = max((eng.P + 255) // 256, 1)
    return min(eng.n_cap // nb, 0xffffffff // nb)


def _check_all(st, direct, trec_cap=0, clean=True):
    """Every tile of the image, plus the header words: N, the longest list, no overflow; persistent state leaves its counters zero."""
    stats = lr.check_tiles(st, range(st.T), direct, trec_cap)
    area = st.area()
    assert st.hdr["overflow"] == 0
    assert st.hdr["num_rendered"] == int(area.sum()), (st.hdr, int(area.sum()))
    assert st.hdr["max_tile_len"] == max(stats.lens), (st.hdr["max_tile_len"], max(stats.lens))
    assert (st.hdr["bin_cap"] != 0) == direct
    if not direct:
        assert int(st.ranges[st.T]) == st.hdr["num_rendered"]
    assert not st.tile_count.any(), "tile_count must be left zero"
    if clean:
        assert not st.cursor.any(), "cursor must be left zero on persistent state"
    return stats


def _lists(st):
    """The block lists of every tile (ids and counts) as one comparable tuple per tile."""
    got = st.read_tiles(range(st.T))
    return {t: tuple(tuple(x.tolist()) for x in v["lists"]) for t, v in got.items()}


def _reached(stats, tiers):
    counts = lr.tier_counts(stats.lens)
    for i in tiers:
        assert counts[i] > 0, f"tier {i} not reached: tiles per tier {counts}"
    return counts


def _engine(R, direct, hint):
    from mm3dgs_slam_amd.fused import FusedEngine
    eng = FusedEngine(R)
    eng.DIRECT_BINS = direct
    eng.max_tile_len = hint
    return eng


def test_generic_path_lists_match_the_host_reference():
    """mm3dgs_forward (GaussianRasterizer): two sort launches, the 2048-key LDS tier and the 16384-key tier with the global-memory tail."""
    from mm3dgs_slam_amd import rasterizer as rz
    total = lr.Stats()
    for spec in (MIXED, CROWDED):
        cfg, g, R, pose, _ = _scene(*spec)
        r = R.render(g, pose)          # (keeps the autograd graph, which holds the binning state, alive while the lists are read)
        torch.cuda.synchronize()
        s = rz.last_state()
        st = lr.ListState(s["geom"], s["img"], s["binning"], s["P"], s["H"], s["W"], s["N"], s["radii"])
        stats = _check_all(st, direct=False, clean=False)
        _report(f"generic {spec}", stats)
        total.lens += stats.lens
        total.ambiguous_bits += stats.ambiguous_bits
        total.pairs += stats.pairs
        del r
    _reached(total, (0, 1, 2, 3))
    assert total.ambiguous_bits <= 1e-4 * 16 * total.pairs


@pytest.mark.parametrize("row", ["packed_fused", "packed_separate", "direct"])
def test_slam_forward_lists_match_the_host_reference(row):
    """mm3dgs_slam_forward: packed bins with the sort inside the forward launch (hint <= 2048; longer lists through the global-memory
    network inside it), packed bins with separate sort launches (no hint), direct bins (register emitter up to 1024, the barrier
    emitter reading `payload` beyond, the global-memory network with direct keys past 2048: the hint sizes the span 1.5 * 2048 + 128)."""
    specs = {"packed_fused": (MIXED,), "packed_separate": (MIXED, CROWDED), "direct": (MIXED, DENSE)}[row]
    total = lr.Stats()
    for spec in specs:
        cfg, g, R, pose, _ = _scene(*spec)
        eng = _engine(R, row == "direct", 1 << 30 if row == "packed_separate" else 2048)
        eng.forward(pose, g, need_grads=False)
        torch.cuda.synchronize()
        assert eng.direct == (row == "direct")
        st = _slam_state(eng)
        stats = _check_all(st, direct=row == "direct", trec_cap=_trec_cap(eng) if row == "direct" else 0)
        _report(f"slam {row} {spec}", stats, f"n_cap={eng.n_cap}")
        total.lens += stats.lens
        total.ambiguous_bits += stats.ambiguous_bits
        total.pairs += stats.pairs
    _reached(total, {"packed_fused": (0, 1, 2), "packed_separate": (0, 1, 2, 3), "direct": (0, 1, 2)}[row])
    assert total.ambiguous_bits <= 1e-4 * 16 * total.pairs


# 129 x 97 = 12 513 tiles: above MAX_LDS_TILES (12 288, mm3dgs_common.h), where the projection kernels' per-workgroup LDS histogram is off and
# every lane counts its tiles in global memory
WIDE = (700, 1552, 2064, 3, 0.0, 97)


def _covering_rects(st):
    """Per tile: how many of the tile rectangles read back from the state hold it."""
    cnt = np.zeros((st.gy, st.gx), np.int64)
    for x0, y0, x1, y1 in st.rect.cpu().numpy():
        cnt[y0:y1, x0:x1] += 1
    return cnt.reshape(-1)


@pytest.mark.parametrize("path", ["generic", "slam_packed"])
def test_tile_counts_on_a_grid_too_big_for_the_lds_histogram(path):
    """The tile counting of preprocess_fwd_kernel (generic) and slam_preprocess_fwd_kernel (mm3dgs_slam_forward, packed bins; direct bins
    do not exist at this size) with global atomics instead of the LDS histogram: the tile ranges are the per-tile counts of the covering
    rectangles, own-lane (<= 32 tiles) and wave-cooperative (> 32 tiles) footprints both present, the header agrees, the counters are
    left zero, and the lists of 32 tiles -- the longest among them -- match the host reference."""
    cfg, g, R, pose, _ = _scene(*WIDE)
    if path == "generic":
        from mm3dgs_slam_amd import rasterizer as rz
        r = R.render(g, pose)          # (keeps the autograd graph, which holds the binning state, alive while the lists are read)
        torch.cuda.synchronize()
        s = rz.last_state()
        st = lr.ListState(s["geom"], s["img"], s["binning"], s["P"], s["H"], s["W"], s["N"], s["radii"])
    else:
        eng = _engine(R, False, 1 << 30)
        eng.forward(pose, g, need_grads=False)
        torch.cuda.synchronize()
        assert not eng.direct
        st = _slam_state(eng)
    assert st.T == 129 * 97 and st.T > 12288
    area = st.area().cpu().numpy()
    assert ((area > 0) & (area <= 32)).any() and (area > 32).any(), np.bincount(np.minimum(area, 33))
    lens = np.diff(st.ranges)
    assert np.array_equal(lens, _covering_rects(st))
    assert st.hdr["num_rendered"] == int(area.sum()) and st.hdr["overflow"] == 0, st.hdr
    assert not st.tile_count.any(), "tile_count must be left zero"
    tiles = sorted(set(np.linspace(0, st.T - 1, 31).astype(int).tolist()) | {int(lens.argmax())})
    stats = lr.check_tiles(st, tiles, False)
    _report(f"wide grid {path}", stats, f"footprints <= 32: {int(((area > 0) & (area <= 32)).sum())}, > 32: {int((area > 32).sum())}")


def test_block_lists_agree_across_the_slam_entry_points():
    """Same map, same pose: the block lists (ids and counts) of packed bins with fused or separate sort launches, direct bins, and the
    tracking launch (mm3dgs_slam_track, pose chain on, one iteration at learning rate 0) with packed and with direct bins are identical
    -- and the tracking launches' lists match the host reference themselves (tiers <= 1024 and (1024, 2048])."""
    from mm3dgs_slam_amd import _lib
    from mm3dgs_slam_amd.fused import _loss_cfg
    cfg, g, R, pose, color = _scene(*MIXED)
    lists = {}
    for name, direct, hint in (("packed_fused", False, 2048), ("packed_separate", False, 1 << 30), ("direct", True, 2048)):
        eng = _engine(R, direct, hint)
        eng.forward(pose, g)
        torch.cuda.synchronize()
        lists[name] = _lists(_slam_state(eng))
    with torch.no_grad():
        gt = R.render(g, pose)["render"].contiguous()
    for direct in (False, True):
        eng = _engine(R, direct, 2048)
        p = pose.clone().contiguous()
        m, v = torch.zeros(7, device=DEV), torch.zeros(7, device=DEV)
        step = torch.zeros(1, dtype=torch.int32, device=DEV)
        lcfg = _loss_cfg(eng.H, eng.W, 1.0, 0.0, 0.0, 1, 0, 1, 0.99)
        ad = _lib.Mm3dgsPoseAdam()
        ad.pose, ad.m, ad.v, ad.step = p.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr()
        ad.lr_q, ad.lr_t, ad.beta1, ad.beta2, ad.eps = 0.0, 0.0, 0.9, 0.999, 1e-8
        eng.track_loop(1, p, g, lcfg, gt, None, ad)
        torch.cuda.synchronize()
        assert int(step) == 1 and torch.equal(p, pose) and eng.direct == direct
        st = _slam_state(eng)
        stats = _check_all(st, direct, _trec_cap(eng) if direct else 0)
        _report(f"track {'direct' if direct else 'packed'}", stats)
        _reached(stats, (0, 1))
        lists["track_direct" if direct else "track_packed"] = _lists(st)
    ref = lists["packed_fused"]
    for name, got in lists.items():
        diff = [t for t in ref if ref[t] != got[t]]
        assert not diff, f"{name}: block lists differ from packed_fused on tiles {diff[:8]}"
