"""Native fused SLAM iteration (mm3dgs_slam_forward / mm3dgs_loss / mm3dgs_slam_backward / mm3dgs_adam) vs the
torch-graph path built from the same (oracle-checked) generic rasterizer and the reference-mirroring torch losses."""
import random

import os
import numpy as np
import pytest
import torch

from tests import parity_util as pu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _setup(P=20000, H=240, W=320, iso=False, seed=0, white=False):
    from mm3dgs_slam_amd import synthetic as syn
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.gaussian_model import GaussianModel
    from mm3dgs_slam_amd.renderer import Renderer
    cfg = default_config(device=DEV, height=H, width=W, pipeline={"force_isotropic": iso}, white_background=white)
    c = cfg["cam"]
    color, depth = syn.rgbd_frame(H, W, seed=seed)
    G = syn.seed_gaussians(color, depth, c["fx"], c["fy"], c["cx"], c["cy"], P, seed=seed, isotropic=False)
    g = GaussianModel(cfg)
    g.training_setup()
    gen = torch.Generator().manual_seed(seed)
    # strongly anisotropic splats: otherwise the rotation gradient (the tangential part of d/dq, a small difference of
    # large radial terms) sits at the float32 noise floor of BOTH implementations and cannot be compared
    G["scaling"] = G["scaling"] + torch.tensor([1.2, -0.8, 0.0])
    g.densification_postfix(G["xyz"].to(DEV), G["f_dc"].to(DEV), torch.zeros(P, 0, 3, device=DEV),
                            (torch.randn(P, 1, generator=gen) * 1.5).to(DEV), G["scaling"].to(DEV),
                            (G["rotation"] * (0.5 + torch.rand(P, 1, generator=gen))).to(DEV), G["rgb"].to(DEV))
    pose = torch.tensor([0.995, 0.03, -0.02, 0.04, 0.03, -0.02, 0.05], device=DEV) * 1.3
    pose[4:] /= 1.3
    return cfg, g, Renderer(cfg), pose, color.to(DEV), depth.to(DEV)


@pytest.mark.parametrize("white", [False, True])
def test_fused_forward_and_backward_match_torch_graph(white):
    """white=True: `white_background` (slam/renderer.py:80-83) -- the reference composites BOTH passes over bg (:196-214), so the
    native bundle adds T_final * bg to the depth / silhouette / depth^2 channels too (silhouette == 1 everywhere) and the
    backward carries the -T_final bg . dL term of those channels."""
    from mm3dgs_slam_amd.fused import FusedEngine
    for iso in (False, True):
        cfg, g, R, pose, color, depth = _setup(iso=iso, white=white)
        eng = FusedEngine(R)
        si = eng.forward(pose, g, need_grads=True)
        assert eng.check_capacity()
        p = pose.clone().requires_grad_(True)
        res = R.render(g, p)
        ref = torch.cat([res["render"], res["depth"]], 0)
        assert pu.rel_l2(eng.out, ref) < 1e-5
        if white:
            assert float((eng.out[4] - 1.0).abs().max()) < 1e-5
        assert torch.equal(eng.radii, res["radii"])
        w = torch.randn(6, eng.H, eng.W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        (ref * w).sum().backward()
        eng.dL.copy_(w)
        stats = (torch.zeros_like(g.max_radii2D), torch.zeros_like(g.xyz_gradient_accum), torch.zeros_like(g.denom))
        eng.backward(si, grads=eng.grads, stats=stats, dpose=eng.dpose)
        tol = 5e-4
        assert pu.rel_l2(eng.dpose, p.grad) < tol, (eng.dpose, p.grad)
        for name, param in (("xyz", g._xyz), ("f_dc", g._features_dc), ("opacity", g._opacity), ("scaling", g._scaling),
                            ("rotation", g._rotation)):
            if name == "rotation" and iso:
                # an isotropic covariance does not depend on the rotation: both gradients are pure rounding noise
                assert eng.grads[name].abs().max() < 1e-3 * (eng.grads["scaling"].abs().max() + 1e-6)
                continue
            assert pu.rel_l2(eng.grads[name], param.grad) < (5e-3 if name == "rotation" else tol), (name, iso)
        vis = res["visibility_filter"]
        assert torch.allclose(stats[2][:, 0], vis.float())
        assert torch.allclose(stats[0], torch.where(vis, res["radii"].float(), torch.zeros_like(stats[0])))
        gn = torch.norm(res["viewspace_points"].grad[:, :2], dim=-1) * vis
        assert pu.rel_l2(stats[1][:, 0], gn) < tol
        for prm in (g._xyz, g._features_dc, g._opacity, g._scaling, g._rotation):
            prm.grad = None


@pytest.mark.parametrize("kind", ["track", "track_pearson", "map", "map_estdepth", "splatam_track", "splatam_map"])
def test_fused_loss_matches_torch_losses(kind):
    # (the precision check of these kernels, against float64 at edge shapes, is tests/test_gpu_loss.py; this one ties them to the torch-graph losses)
    from mm3dgs_slam_amd.fused import FusedEngine, _loss_cfg
    from mm3dgs_slam_amd.loss_utils import l1_loss, pearson_loss, ssim
    cfg, g, R, pose, color, depth = _setup(P=15000, H=200, W=272)
    eng = FusedEngine(R)
    eng.forward(pose, g)
    out = eng.out.clone().requires_grad_(True)
    image, d, sil = out[:3], out[3], out[4]
    est = depth * 0.8 + 0.3
    if kind.startswith("splatam"):
        # `method: splatam` (slam/tracker.py:110-126, slam/mapper.py:836-855), written like the torch-graph loops do; a hole in the
        # sensor depth exercises the { gt_depth > 0 } masks
        depth = depth.clone()
        depth[20:70, 40:150] = 0.0
        if kind == "splatam_track":
            mask = (depth > 0) & (sil > 0.99)
            loss = (depth - d).abs()[mask].sum() + 0.5 * (color - image).abs()[:, mask].sum()
            lc = _loss_cfg(eng.H, eng.W, 0.5, 0.0, 0.0, 3, 0, 0, 0.99, w_depth_l1=1.0, depth_l1_mask=3, l1_sum=1)
        else:
            loss = (depth - d).abs()[depth > 0].mean() + 0.5 * (0.8 * l1_loss(image, color) + 0.2 * (1.0 - ssim(image, color)))
            lc = _loss_cfg(eng.H, eng.W, 0.5 * 0.8, 0.5 * 0.2, 0.0, 0, 0, 0, 0.5, w_depth_l1=1.0, depth_l1_mask=2)
        ref = depth
    elif kind.startswith("track"):
        presence = sil > 0.99
        loss = (image - color).abs()[:, presence].mean()
        lc = _loss_cfg(eng.H, eng.W, 1.0, 0.0, 0.0, 1, 0, 1, 0.99)
        ref = None
        if kind == "track_pearson":
            loss = loss + 0.05 * pearson_loss(d, depth, mask=presence & (depth > 0), invert_estimate=True)
            lc = _loss_cfg(eng.H, eng.W, 1.0, 0.0, 0.05, 1, 3, 1, 0.99)
            ref = depth
    else:
        loss = 0.8 * l1_loss(image, color) + 0.2 * (1.0 - ssim(image, color))
        if kind == "map":
            loss = loss + 0.05 * pearson_loss(d, depth, mask=depth > 0, invert_estimate=False)
            lc, ref = _loss_cfg(eng.H, eng.W, 0.8, 0.2, 0.05, 0, 2, 0, 0.5), depth
        else:
            loss = loss + 0.05 * pearson_loss(d, est, invert_estimate=False)
            lc, ref = _loss_cfg(eng.H, eng.W, 0.8, 0.2, 0.05, 0, 0, 0, 0.5), est
    loss.backward()
    eng.loss_call(lc, color, ref)
    torch.cuda.synchronize()
    assert abs(float(eng.loss[0]) - float(loss)) < 2e-5 * max(1.0, abs(float(loss))), (eng.loss, loss)
    assert pu.rel_l2(eng.dL, out.grad) < 2e-4


def test_fused_adam_matches_torch_adam():
    from mm3dgs_slam_amd import _lib
    from mm3dgs_slam_amd.rasterizer import _stream
    torch.manual_seed(0)
    p1 = torch.randn(1000, 3, device=DEV); p2 = torch.randn(1000, 1, device=DEV)
    q1, q2 = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [q1], "lr": 1e-3}, {"params": [q2], "lr": 5e-2}], lr=0.0, eps=1e-15)
    m1, v1, m2, v2 = (torch.zeros_like(t) for t in (p1, p1, p2, p2))
    lib = _lib.load()
    for step in range(1, 6):
        g1, g2 = torch.randn_like(p1), torch.randn_like(p2) * 10
        q1.grad, q2.grad = g1.clone(), g2.clone()
        opt.step()
        tab = (_lib.Mm3dgsAdamGroup * 8)()
        for e, (p, gr, m, v, lr) in zip(tab, ((p1, g1, m1, v1, 1e-3), (p2, g2, m2, v2, 5e-2))):
            e.param, e.grad, e.exp_avg, e.exp_avg_sq, e.n, e.lr = p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr
        _lib.check(lib.mm3dgs_adam(tab, 2, step, 0.9, 0.999, 1e-15, _stream()))
    torch.cuda.synchronize()
    assert torch.allclose(p1, q1.detach(), atol=1e-6, rtol=1e-5) and torch.allclose(p2, q2.detach(), atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("method", ["vigs", "splatam"])
def test_fused_tracker_and_mapper_follow_the_torch_graph_loops(method):
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.fused import FusedEngine
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    results = {}
    for native in (False, True):
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        # (splatam prunes at mapping iterations 0 and 20: 24 iterations cover both)
        cfg = default_config(device=DEV, height=240, width=320, method=method, tracking={"iters": 40},
                             mapping={"iters": 24 if method == "splatam" else 12})
        seq = SyntheticSequence(cfg, 3, 30000, seed=4)
        slam = SLAM(cfg, seq, native_loops=native)
        random.seed(1)
        for i in range(3):
            slam.step(i)
        if native:
            assert FusedEngine.eligible(cfg, slam.gaussians) and slam.tracker.tracking_iter_count > 0   # (only the native loop counts without get_runtime_stats)
        results[native] = (torch.stack(slam.estimate_pose_list[:3]).cpu(), slam.gaussians._xyz.detach().cpu(),
                           slam.gaussians._opacity.detach().cpu(), slam.pose_errors())
    a, b = results[False], results[True]
    # two float32 pipelines + Adam: same trajectory, not the same bits (the torch graph's MIOpen convolutions are not even
    # run-to-run deterministic)
    assert (a[0] - b[0]).abs().max() < 4e-3, (a[0], b[0])
    if method == "splatam":
        # splatam prunes by opacity inside the loop (iterations 0 and 20): a Gaussian within rounding of the 0.005 threshold may
        # go either way (measured: 77169 against 77171 rows), after which the two maps are no longer row-aligned -- compare the
        # populations
        na, nb = a[1].shape[0], b[1].shape[0]
        assert abs(na - nb) <= 1e-3 * na, (na, nb)
        qs = torch.tensor([0.05, 0.25, 0.5, 0.75, 0.95])
        assert (torch.quantile(a[2].flatten()[:100000], qs) - torch.quantile(b[2].flatten()[:100000], qs)).abs().max() < 0.05
        assert (a[1].mean(0) - b[1].mean(0)).abs().max() < 1e-3 and b[3][1] < 0.01 and b[3][2] < 0.01, b[3]
        return
    assert a[1].shape == b[1].shape
    # Adam(eps=1e-15) turns the sign of a ~0 gradient into a full-size step, so individual Gaussians may diverge between
    # two float32 implementations; the population must not
    assert pu.rel_l2(b[1], a[1]) < 1e-3 and (a[2] - b[2]).abs().median() < 5e-3 and torch.quantile((a[2] - b[2]).abs().flatten()[:100000], 0.99) < 0.1, ((a[2] - b[2]).abs().median(), torch.quantile((a[2] - b[2]).abs().flatten()[:100000], 0.99))
    assert b[3][1] < 0.01 and b[3][2] < 0.01, b[3]


def _setup_slam_like(P, H, W, iso, seed):
    """A map as the SLAM loop sees it (slam/mapper.py:437-474,644-668 seeding after a little optimisation): one Gaussian per sampled
    pixel of an RGB-D frame in raster order, scale ~ the pixel footprint (isotropic, or x U[0.5, 2] per axis with random rotations),
    opacity logits around 0, viewed from a pose a tracking step away from the seeding pose."""
    from mm3dgs_slam_amd import synthetic as syn
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.gaussian_model import GaussianModel
    from mm3dgs_slam_amd.renderer import Renderer
    cfg = default_config(device=DEV, height=H, width=W, pipeline={"force_isotropic": iso})
    c = cfg["cam"]
    color, depth = syn.rgbd_frame(H, W, seed=seed)
    G = syn.seed_gaussians(color, depth, c["fx"], c["fy"], c["cx"], c["cy"], P, seed=seed, isotropic=iso)
    g = GaussianModel(cfg)
    g.training_setup()
    gen = torch.Generator().manual_seed(seed)
    g.densification_postfix(G["xyz"].to(DEV), (G["f_dc"] + 0.3 * torch.randn(P, 1, 3, generator=gen)).to(DEV), torch.zeros(P, 0, 3, device=DEV),
                            (0.5 * torch.randn(P, 1, generator=gen)).to(DEV), (G["scaling"] + 0.15 * torch.randn(P, 3 if not iso else 1, generator=gen)).to(DEV),
                            G["rotation"].to(DEV), G["rgb"].to(DEV))
    pose = torch.tensor([1.0, 0.004, -0.003, 0.002, 0.01, -0.008, 0.012], device=DEV)
    return cfg, g, Renderer(cfg), pose, color.to(DEV), depth.to(DEV)


def native_vs_oracle(seed=0, direct=False, P=3000, H=120, W=160, floor=False, slam_like=False, iso=False, world=False, setup=None, n_tiles=0, raw=False):
    """rel-L2 errors of the native SLAM path (pose transform, activations, depth bundle, compositors, chain rules: one fused forward +
    backward) against the float64 CPU oracle driven through the torch-graph Renderer.  direct: second render of the engine (direct bins)
    instead of its first (packed bins).  floor: also the errors of the ORACLE evaluated in float32 against itself in float64 on the same
    scene (what float32 arithmetic costs there, whatever the implementation), as "f32:" keys.  Gradient image: white noise on a stress
    scene (strongly anisotropic splats, random opacities), or -- slam_like -- the gradient of the mapping loss (0.8 L1 + 0.2 (1 - SSIM) on the
    colours + 0.05 (1 - Pearson) on the depth channel, slam/mapper.py:856-873) against the frame the map was seeded from, evaluated at the
    float64 oracle's image and handed to both sides.
    setup: a prepared (cfg, model, Renderer, pose, colour target, depth target) instead of the seeded scenes.  n_tiles > 0: the
    TILE-SAMPLED oracle (oracle.raster_ref.rasterize_tiles_ref: the projection's integer decisions for every Gaussian, the
    differentiable projection / depth order / compositing for n_tiles tiles -- the heaviest, the lightest, the image corners, seeded
    random ones) for maps of BASELINE.json's sizes; the gradient image is then zero outside those tiles on both sides, derived
    (slam_like) from the HIP image, and "img" compares the sampled tiles' pixels."""
    import copy
    import functools
    import mm3dgs_slam_amd.pose_utils as P_
    import mm3dgs_slam_amd.renderer as rmod
    from mm3dgs_slam_amd.fused import FusedEngine
    from mm3dgs_slam_amd.renderer import Renderer
    from oracle.raster_ref import RefRasterizer
    cfg, g, R, pose, color, depth = setup if setup is not None else (_setup_slam_like(P, H, W, iso, seed) if slam_like else _setup(P=P, H=H, W=W, seed=seed))
    if world:      # pipeline.transform_means_python: false (slam/renderer.py:117-124): world-frame means under the full view matrix
        cfg["pipeline"]["transform_means_python"] = False
        assert R.cfg["pipeline"]["transform_means_python"] is False
    eng = FusedEngine(R)
    si = eng.forward(pose, g, need_grads=True)
    assert si.world_means == (1 if world else 0)
    assert eng.check_capacity()
    if direct:
        si = eng.forward(pose, g, need_grads=True)
        assert eng.direct
    keys = ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation")
    depth_key = None
    if n_tiles:      # the float32 view depths the kernels sorted by (geom_state: csrc/mm3dgs_common.h geom_view) -> the oracle's depth ORDER
        off = (eng.P * 48 + 255) // 256 * 256
        depth_key = eng.geom[off:off + 4 * eng.P].view(torch.float32).clone().cpu()
    ccfg = copy.deepcopy(cfg)
    ccfg["device"] = "cpu"
    W6 = {}      # the gradient image: drawn (stress scenes) or derived from the float64 oracle's image (SLAM-like scenes), then shared
    sample = {}  # tile-sampled oracle: the tiles, chosen at the oracle's first pass from its own pair counts

    def choose_tiles(counts):      # (called with the pair counts at every oracle pass; the choice is made once)
        if "tiles" not in sample:
            sample["tiles"] = pu.pick_tiles(counts, n_tiles, seed)
            sample["mask"] = pu.tile_mask(eng.H, eng.W, sample["tiles"])
            sample["max_list"] = int(counts.max())
        return sample["tiles"]

    def gradient_image(ref64):
        if n_tiles:      # (the oracle's image is zero outside its tiles: the loss is evaluated at the HIP image -- a weight image both sides share)
            # gradients only on the tiles whose float32 decisions (depth order of surface splats a float32 ulp apart, 1/255, T < 1e-4) agree with
            # float64: tests/test_gpu_fullsize.py says why
            sample["errs"] = pu.tile_errors(eng.out.detach().cpu(), ref64.detach(), sample["tiles"])
            sample["clean"] = pu.clean_tiles(sample["errs"])
            sample["mask"] = pu.tile_mask(eng.H, eng.W, sample["clean"])
            ref64 = eng.out.detach().double().cpu()
        if not slam_like:
            w = torch.randn(6, eng.H, eng.W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).double().cpu()
            return w * sample["mask"] if n_tiles else w
        from mm3dgs_slam_amd.loss_utils import l1_loss, pearson_loss, ssim
        x = ref64.detach().clone().requires_grad_(True)
        gt, gd = color.double().cpu(), depth.double().cpu()
        loss = 0.8 * l1_loss(x[:3], gt) + 0.2 * (1.0 - ssim(x[:3], gt)) + 0.05 * pearson_loss(x[3], gd, mask=gd > 0, invert_estimate=False)
        loss.backward()
        w = x.grad.float().double()          # float32-representable: both sides see the same numbers
        return w * sample["mask"] if n_tiles else w

    def oracle(dt):
        class PC:
            active_sh_degree = 0
            max_sh_degree = 0
        pc = PC()
        leaf = {k: getattr(g, k).detach().to(dt).cpu().requires_grad_(True) for k in keys}
        pc._xyz, pc._scaling, pc._rotation = leaf["_xyz"], leaf["_scaling"], leaf["_rotation"]
        pc.get_xyz, pc.get_opacity, pc.get_scaling = leaf["_xyz"], torch.sigmoid(leaf["_opacity"]), torch.exp(leaf["_scaling"])
        pc.get_rotation, pc.get_features = torch.nn.functional.normalize(leaf["_rotation"]), leaf["_features_dc"]
        Rc = Renderer(ccfg, rasterizer_cls=functools.partial(RefRasterizer, tiles=choose_tiles, depth_key=depth_key) if n_tiles else RefRasterizer)
        Rc.projection_matrix, Rc.background, Rc._eye = Rc.projection_matrix.to(dt), Rc.background.to(dt), Rc._eye.to(dt)
        orig = rmod.get_camera_from_tensor

        def cam(t):     # the dtype-preserving twin of get_camera_from_tensor (which casts to float32 like the reference does)
            return torch.cat([torch.cat([P_.quad2rotation(t[None, :4])[0], t[4:7, None]], 1),
                              torch.tensor([[0.0, 0, 0, 1]], dtype=t.dtype)], 0)
        rmod.get_camera_from_tensor = cam
        try:
            p_ = pose.detach().to(dt).cpu().requires_grad_(True)
            r_ = Rc.render(pc, p_)
            ref_ = torch.cat([r_["render"], r_["depth"]], 0)
            if "w" not in W6:
                W6["w"] = gradient_image(ref_)
            (ref_ * W6["w"].to(dt)).sum().backward()
        finally:
            rmod.get_camera_from_tensor = orig
        return ref_.detach(), p_.grad, {k: leaf[k].grad for k in keys}

    ref, dp, lg = oracle(torch.float64)
    if n_tiles:      # the exact list check (tests/list_ref.py) on every sampled tile and the kernels' heaviest one, before the backward
        from tests import list_ref as lr
        st = lr.ListState(eng.geom, eng.img_state, eng.binning, eng.P, eng.H, eng.W, eng.n_cap, eng.radii)
        direct_bins = st.hdr["bin_cap"] != 0
        lens = [st.span(t)[1] for t in range(st.T)]
        heaviest = int(np.argmax(lens))
        nb = max((eng.P + 255) // 256, 1)
        stats = lr.check_tiles(st, list(dict.fromkeys(list(sample["tiles"]) + [heaviest])), direct_bins,
                               min(eng.n_cap // nb, 0xffffffff // nb) if direct_bins else 0)
        list_stats = (stats.tiles, str(stats), lr.tier_counts(stats.lens))
    eng.dL.copy_(W6["w"].float().to(DEV))
    eng.backward(si, grads=eng.grads, dpose=eng.dpose)
    assert eng.check_capacity()
    names = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("opacity", "_opacity"), ("scaling", "_scaling"), ("rotation", "_rotation"))
    sel = pu.tile_mask(eng.H, eng.W, sample["tiles"]) if n_tiles else slice(None)
    m = {"img": pu.rel_l2(eng.out.cpu()[:, sel], ref[:, sel]), "d_pose": pu.rel_l2(eng.dpose, dp)}
    if n_tiles:
        m["tiles"], m["max_list"], m["tile_errors"] = list(sample["tiles"]), sample["max_list"], sample["errs"]
        m["clean_tiles"], m["img_worst_tile"] = len(sample["clean"]), max(e for e, _ in sample["errs"].values())
        m["img_clean_tiles_max"] = max([sample["errs"][t][0] for t in sample["clean"]], default=0.0)
        # the sort depths against the float64 view depth z = (R(q / |q|) x + t)_z (float32 rounding of a three-term sum)
        q64 = pose.detach().double().cpu()
        z64 = g._xyz.detach().double().cpu() @ P_.quad2rotation(q64[None, :4])[0][2] + q64[6]
        vis = (eng.radii > 0).cpu()
        m["depth_key_rel_err"] = float(((depth_key[vis].double() - z64[vis]).abs() / z64[vis].abs()).max())
        m["lists_checked"], m["lists"], m["list_tiers"] = list_stats
    for name, key in names:
        m["d_" + name] = pu.rel_l2(eng.grads[name], lg[key])
    if raw:      # (diagnostics: the gradient arrays themselves)
        m["raw"] = {"hip": {name: eng.grads[name].detach().cpu().clone() for name, _ in names}, "oracle": {name: lg[key] for name, key in names},
                    "lists": None, "radii": eng.radii.cpu().clone()}
    if floor:
        ref32, dp32, lg32 = oracle(torch.float32)
        if raw:
            m["raw"]["f32"] = {name: lg32[key] for name, key in names}
        m["f32:img"], m["f32:d_pose"] = pu.rel_l2(ref32[:, sel], ref[:, sel]), pu.rel_l2(dp32, dp)
        if n_tiles:      # tiles on which float32 arithmetic itself flips a decision (same order, same CLEAN_PIXEL_TOL as the kernels' count)
            m["f32:clean_tiles"] = len(pu.clean_tiles(pu.tile_errors(ref32, ref, sample["tiles"])))
        for name, key in names:
            m["f32:d_" + name] = pu.rel_l2(lg32[key], lg[key])
    return m


def test_pose_gradient_on_slam_like_scenes_matches_float64_oracle():
    """north_star's pose-gradient bar (<= 1e-5) on the population the SLAM loop produces, not on curated cases: 16 seeded maps
    (8 isotropic as configs/UTMM.yml forces them, 8 anisotropic), a tracking-sized pose offset, the gradient image of the mapping
    loss; direct bins (the path the loops run).  Beside every HIP number stands the float32 evaluation of the ORACLE on the same
    scene.  Measured on MI355X: 12 of the 16 scenes sit at 5e-7 .. 1e-6 (HIP and float32 oracle alike); on the other four a float32
    decision differs from float64 (a surface seeded from a fronto-parallel box has groups of almost equal depths: two splats swap
    their compositing order, or a 1/255 / T < 1e-4 test flips) and BOTH evaluations leave the bar together (seed 33: 2.1e-4 / 2.1e-4;
    seed 34: HIP 2.8e-5, float32 oracle 1.2e-4; seed 31 isotropic: HIP 8.6e-7, float32 oracle 2.8e-5).  Asserted: wherever float32
    arithmetic can meet the bar the kernels meet it; nowhere are they worse than 1.5 x the float32 oracle; at least 10 of 16 scenes are
    under 1e-5 outright; Gaussian-side gradients likewise against GRAD_TOL."""
    rows = []
    for seed in range(30, 38):
        for iso in (False, True):
            m = native_vs_oracle(seed, direct=True, slam_like=True, iso=iso, floor=True)
            rows.append((seed, iso, m))
            print(f"seed {seed} iso {iso}: " + "  ".join(f"{k} {m[k]:.1e}/{m['f32:' + k]:.1e}" for k in m if not k.startswith("f32:")), flush=True)
    for seed, iso, m in rows:
        assert m["img"] <= pu.IMG_TOL, (seed, iso, m)
        assert m["d_pose"] <= max(1e-5, 1.5 * m["f32:d_pose"]), (seed, iso, m)
        if m["f32:d_pose"] <= 1e-5:
            assert m["d_pose"] <= 1e-5, (seed, iso, m)
        for k, v in m.items():
            if k.startswith("d_") and k != "d_pose" and not (iso and k == "d_rotation"):      # (isotropic: the rotation gradient is rounding noise on both sides)
                assert v <= max(pu.GRAD_TOL, 1.5 * m["f32:" + k]), (seed, iso, k, m)
    assert sum(1 for _, _, m in rows if m["d_pose"] <= 1e-5) >= 10, [m["d_pose"] for _, _, m in rows]


@pytest.mark.parametrize("seed,direct", [(0, False), (0, True), (3, True)])
def test_fused_path_matches_float64_oracle(seed, direct):
    """The fused kernels against the float64 CPU oracle: the strongest statement of parity for the SLAM path (packed and direct bins)."""
    m = native_vs_oracle(seed, direct)
    assert m["img"] <= pu.IMG_TOL, m
    assert m["d_pose"] <= 1e-5, m          # north_star: pose gradients <= 1e-5
    for k, v in m.items():
        if k.startswith("d_") and k != "d_pose":
            assert v <= pu.GRAD_TOL, (k, m)


def test_world_frame_means_path_matches_float64_oracle_on_a_population():
    """`transform_means_python: false` natively (round 4): world-frame means, the covariance rotated into the view, the pose gradient
    through the view matrix as well (the oracle side differentiates viewmatrix / projmatrix / campos through the torch graph of
    slam/renderer.py:117-124), the depth bundle with the reference's transposed matrix (:207-214).  Six stress scenes and four SLAM-like
    ones, none chosen, every number beside the float32 evaluation of the ORACLE on the same scene.  Measured (tools/world_sweep.py): the
    projection is as precise as in the camera-frame mode (conic 1.2e-7 median, pixel centre 3.5e-6 px: tools/world_conic_diag.py); image
    4e-7 .. 5e-6; pose gradient 3.4e-6 .. 9.7e-6 on three stress scenes and 8e-7 .. 5e-6 on the SLAM-like ones, where float32 itself
    holds (floor 4e-7 .. 9.6e-6: in this mode the pose gradient also carries the covariance-rotation terms, which largely cancel over the
    map, so its float32 floor is higher than the camera-frame mode's), 2e-5 .. 9e-5 on three stress scenes where a compositing decision
    flips in the kernels only (seed 3: the opacity and colour gradients, which no pose chain touches, move by 1.8e-4 with it).  Asserted:
    image under IMG_TOL everywhere; pose gradient under 1e-5 or 1.5 x the float32 oracle on at least half the scenes and under
    FLIP_TOL = 1e-4 on all but SLAM-like scenes whose float32 oracle is off by as much; Gaussian-side gradients likewise against GRAD_TOL."""
    FLIP_TOL = 1e-4
    ok_pose, rows = 0, []
    for slam_like, seeds in ((False, range(6)), (True, range(30, 34))):
        for seed in seeds:
            m = native_vs_oracle(seed, direct=True, world=True, floor=True, slam_like=slam_like, P=4000 if slam_like else 3000)
            rows.append((slam_like, seed, m))
            assert m["img"] <= max(pu.IMG_TOL, 1.5 * m["f32:img"]), (seed, m)
            floor = m["f32:d_pose"]
            ok_pose += m["d_pose"] <= max(1e-5, 1.5 * floor)
            assert m["d_pose"] <= max(FLIP_TOL, 1.5 * floor), (slam_like, seed, m)
            for k in ("d_xyz", "d_f_dc", "d_opacity", "d_scaling", "d_rotation"):
                assert m[k] <= max(3 * pu.GRAD_TOL, 1.5 * m["f32:" + k]), (slam_like, seed, k, m)      # (3 x: a flip scene -- seed 3: 3.0e-4)
    assert ok_pose >= len(rows) // 2, [(s, sd, m["d_pose"], m["f32:d_pose"]) for s, sd, m in rows]


def _window_worker(rank, world, port, out):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)     # both ranks share the one GPU of the test box
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from mm3dgs_slam_amd.window_parallel import WindowParallel
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device=DEV, height=120, width=160, tracking={"iters": 5}, mapping={"iters": 6, "kf_every": 1})
    seq = SyntheticSequence(cfg, 3, 6000, seed=6)
    slam = SLAM(cfg, seq, window=WindowParallel(rank, world))
    assert type(slam.mapper).__name__ == "FusedMapper"
    for i in range(3):
        slam.step(i)
    torch.save({"xyz": slam.gaussians._xyz.detach().cpu(), "op": slam.gaussians._opacity.detach().cpu(),
                "acc": slam.gaussians.xyz_gradient_accum.cpu()}, os.path.join(out, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_fused_mapper_window_parallel_two_ranks(tmp_path):
    """Native mapping loop with the keyframe window sharded over 2 ranks (gloo, both on this GPU): ranks stay identical."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_window_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    assert a["xyz"].shape == b["xyz"].shape and a["xyz"].shape[0] > 0
    assert torch.equal(a["xyz"], b["xyz"]) and torch.equal(a["op"], b["op"]) and torch.equal(a["acc"], b["acc"])
    # and both equal the single-process window-batch = 2 run of the native loop (same two views per optimiser step, gradients
    # summed locally instead of by the all-reduce): SURVEY.md 8e's parity baseline of a 2-rank run
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from mm3dgs_slam_amd.window_parallel import WindowParallel
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device=DEV, height=120, width=160, tracking={"iters": 5}, mapping={"iters": 6, "kf_every": 1})
    seq = SyntheticSequence(cfg, 3, 6000, seed=6)
    slam = SLAM(cfg, seq, window=WindowParallel(0, 1, batch=2))
    for i in range(3):
        slam.step(i)
    g = slam.gaussians
    assert g._xyz.shape == a["xyz"].shape
    assert torch.allclose(g._xyz.detach().cpu(), a["xyz"], rtol=1e-5, atol=1e-7), (g._xyz.detach().cpu() - a["xyz"]).abs().max()
    assert torch.allclose(g._opacity.detach().cpu(), a["op"], rtol=1e-5, atol=1e-6)
    assert torch.allclose(g.xyz_gradient_accum.cpu(), a["acc"], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("ba", [False, True])
def test_window_step_fused_with_the_next_projection_is_bit_identical(ba, monkeypatch):
    """The multi-GPU window's optimiser step: mm3dgs_slam_adam_project (Adam from the reduced gradient arrays + projection and binning of
    the next view in one launch, that view's mm3dgs_slam_map call carrying MM3DGS_FWD_PROJECTED) against mm3dgs_adam followed by the
    view's own projection launch -- same map, same poses, same statistics, bit for bit, with bundle adjustment's opt_mask riding in the
    Adam struct on one side and multiplied into the gradients on the other."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.fused import FusedMapper
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from mm3dgs_slam_amd.window_parallel import WindowParallel
    from mm3dgs_slam_amd.fused import FusedEngine, _engine
    outs, n_fused = [], []
    real = FusedEngine.adam_project
    def counting(self, *a, **k):
        n_fused[-1] += 1
        return real(self, *a, **k)
    monkeypatch.setattr(FusedEngine, "adam_project", counting)
    for fuse in (True, False):
        monkeypatch.setattr(FusedMapper, "fuse_adam_project", fuse)
        n_fused.append(0)
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        cfg = default_config(device=DEV, height=120, width=160, tracking={"iters": 5}, mapping={"iters": 8, "kf_every": 1, "do_BA": ba})
        seq = SyntheticSequence(cfg, 3, 6000, seed=6)
        slam = SLAM(cfg, seq, window=WindowParallel(0, 1, batch=2))
        for i in range(3):
            slam.step(i)
        eng = _engine(slam.renderer)
        g = slam.gaussians
        outs.append((g._xyz.detach().clone(), g._opacity.detach().clone(), g._scaling.detach().clone(), g._rotation.detach().clone(), g._features_dc.detach().clone(),
                     g.xyz_gradient_accum.clone(), g.max_radii2D.clone(), torch.stack([p.detach().clone() for p in slam.estimate_pose_list[:3]]),
                     [kf.pose.detach().clone() for kf in slam.mapper.keyframes], eng.out.clone()))
    a, b = outs
    assert n_fused[0] >= 10 and n_fused[1] == 0, n_fused          # the fused launch really served the steps of the first run
    assert a[0].shape == b[0].shape and a[0].shape[0] > 0
    for x, y in zip(a[:8], b[:8]):
        assert torch.equal(x, y), (x - y).abs().max()
    for x, y in zip(a[8], b[8]):
        assert torch.equal(x, y)
    assert torch.equal(a[9], b[9])


@pytest.mark.parametrize("long_lists", [False, True])
def test_sort_fused_into_the_forward_launch_is_bit_identical(long_lists, monkeypatch):
    """MM3DGS_FWD_SHORT_LISTS selects the sort + forward-composite kernel; it must reproduce the separate launches bit for
    bit (same sort order, same lists, same records) -- also when a tile list exceeds its 2048-key LDS tier and takes the
    global-memory path inside the fused kernel.  (Packed bins on both sides; the direct bins have their own test below.)"""
    from mm3dgs_slam_amd.fused import FusedEngine
    monkeypatch.setattr(FusedEngine, "DIRECT_BINS", False)
    if long_lists:
        cfg, g, R, pose, color, depth = _setup(P=12000, H=48, W=64, seed=3)
        with torch.no_grad():
            g._scaling += 2.0          # every splat covers most of the small image: thousands of splats per tile
    else:
        cfg, g, R, pose, color, depth = _setup(P=20000, H=120, W=168, seed=3)
    eng = FusedEngine(R)
    outs = []
    for hint in (1 << 30, 100):        # no hint -> separate sort launches; "short lists" -> fused kernel
        eng.max_tile_len = hint
        si = eng.forward(pose, g, need_grads=True)
        torch.cuda.synchronize()
        hdr = eng.img_state[:16].view(torch.int32).cpu()
        eng.dL.copy_(torch.randn(6, eng.H, eng.W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)))
        eng.backward(si, grads=eng.grads, dpose=eng.dpose)
        outs.append((eng.out.clone(), eng.radii.clone(), eng.dpose.clone(), {k: v.clone() for k, v in eng.grads.items()}, int(hdr[2])))
    a, b = outs
    if long_lists:
        assert a[4] > 2048, a[4]       # the case really exercises the long-list path
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[2], b[2])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


@pytest.mark.parametrize("huge", [False, True])
def test_direct_bins_reproduce_the_packed_bins_bit_for_bit(huge, monkeypatch):
    """MM3DGS_FWD_DIRECT_BINS (projection + binning in one launch, one fixed span of pairs per tile, block masks and record
    indices produced per pair by the binning kernel) against the packed bins (projection, scatter with its own scan, masks
    computed by the sort): same lists, same records, hence the same image, radii, pose gradient and Gaussian gradients bit for
    bit -- also with splats that cover more than 32 tiles (the wave-cooperative path of the binning kernel)."""
    from mm3dgs_slam_amd.fused import FusedEngine
    cfg, g, R, pose, color, depth = _setup(P=8000, H=120, W=168, seed=3)
    if huge:
        with torch.no_grad():
            g._scaling[::97] += 3.5          # ~80 splats of 100+ pixels
    outs = []
    for direct in (False, True):
        monkeypatch.setattr(FusedEngine, "DIRECT_BINS", direct)
        eng = FusedEngine(R)
        eng.forward(pose, g, need_grads=True)
        assert eng.check_capacity()
        for rep in range(2):                  # twice: the persistent counters must be left clean
            si = eng.forward(pose, g, need_grads=True)
            assert eng.direct == direct, (eng.max_tile_len, eng.P, eng.n_cap)
            eng.dL.copy_(torch.randn(6, eng.H, eng.W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)))
            eng.backward(si, grads=eng.grads, dpose=eng.dpose)
        torch.cuda.synchronize()
        hdr = eng.img_state[:32].view(torch.int32).cpu()
        assert int(hdr[1]) == 0
        assert (int(hdr[7]) != 0) == direct
        outs.append((eng.out.clone(), eng.radii.clone(), eng.dpose.clone(), {k: v.clone() for k, v in eng.grads.items()}, int(hdr[0]), int(hdr[2])))
    a, b = outs
    # same N (pairs touched, the reference's num_rendered); the direct bins' lists are SHORTER since round 4: a pair whose 3-sigma tile
    # rectangle reaches a tile that its { alpha >= 1/255 } region cannot touch takes no slot there (15 - 20 % of the pairs)
    assert a[4] == b[4] and b[5] <= a[5] and b[5] >= 0.6 * a[5], (a[4:], b[4:])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[2], b[2])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


@pytest.mark.parametrize("pearson", [False, True])
def test_tracking_loss_folded_into_the_compositors_matches_the_loss_kernels(pearson, monkeypatch):
    """mm3dgs_slam_track folds an SSIM-free loss into the forward epilogue / backward prologue; the pose trajectory must
    match the three-kernel loss path (same arithmetic per pixel, only the summation order of the tile sums differs)."""
    from mm3dgs_slam_amd import _lib
    from mm3dgs_slam_amd.fused import FusedEngine, _loss_cfg
    monkeypatch.setattr(FusedEngine, "DIRECT_BINS", False)      # (the "short lists" hint below is not a real list length: packed bins)
    cfg, g, R, pose0, color, depth = _setup(P=20000, H=120, W=168, seed=4)
    with torch.no_grad():
        gt = torch.cat([R.render(g, pose0)["render"]], 0).contiguous()
        ref = R.render(g, pose0)["depth"][0].contiguous()
    results = []
    for no_fold in ("1", "0"):
        monkeypatch.setenv("MM3DGS_NO_FOLDED_LOSS", no_fold)
        eng = FusedEngine(R)
        eng.max_tile_len = 100                       # "short lists" hint: the fused sort kernel (required for folding)
        pose = (pose0 + torch.tensor([0.0, 0.004, -0.003, 0.002, 0.01, -0.008, 0.012], device=DEV)).contiguous()
        m, v = torch.zeros(7, device=DEV), torch.zeros(7, device=DEV)
        step = torch.zeros(1, dtype=torch.int32, device=DEV)
        lcfg = _loss_cfg(eng.H, eng.W, 1.0, 0.0, 0.05 if pearson else 0.0, 1, 1 if pearson else 0, 1, 0.99)
        ad = _lib.Mm3dgsPoseAdam()
        ad.pose, ad.m, ad.v, ad.step = pose.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr()
        ad.lr_q, ad.lr_t, ad.beta1, ad.beta2, ad.eps = 0.002, 0.002, 0.9, 0.999, 1e-8
        eng.track_loop(12, pose, g, lcfg, gt, ref if pearson else None, ad)
        torch.cuda.synchronize()
        results.append((pose.clone(), eng.loss.clone(), int(step)))
    (pa, la, sa), (pb, lb, sb) = results
    assert sa == sb == 12
    assert (pa - pb).abs().max() < 2e-5, (pa, pb)
    assert (la - lb).abs().max() < 1e-5 * max(1.0, float(la.abs().max())), (la, lb)


@pytest.mark.parametrize("direct", [False, True])
def test_tracking_iteration_in_one_compositor_launch_matches_the_separate_launches(direct, monkeypatch):
    """mm3dgs_slam_track with the masked-L1 loss runs sort + forward + backward compositing as ONE launch (the backward pass picks
    its pixel's transmittance, contributor count and colours up from memory the same lane just wrote); MM3DGS_NO_FUSED_TRACK=1
    keeps the two compositor launches.  Same arithmetic, same order: the pose trajectories must be identical."""
    from mm3dgs_slam_amd import _lib
    from mm3dgs_slam_amd.fused import FusedEngine, _loss_cfg
    monkeypatch.setattr(FusedEngine, "DIRECT_BINS", direct)
    cfg, g, R, pose0, color, depth = _setup(P=8000, H=120, W=168, seed=4)
    with torch.no_grad():
        gt = torch.cat([R.render(g, pose0)["render"]], 0).contiguous()
    results = []
    for no_fuse in ("1", "0"):
        monkeypatch.setenv("MM3DGS_NO_FUSED_TRACK", no_fuse)
        eng = FusedEngine(R)
        eng.forward(pose0, g)
        assert eng.check_capacity() and eng.max_tile_len <= eng.FAST_PATH_MAX_LIST
        pose = (pose0 + torch.tensor([0.0, 0.004, -0.003, 0.002, 0.01, -0.008, 0.012], device=DEV)).contiguous()
        m, v = torch.zeros(7, device=DEV), torch.zeros(7, device=DEV)
        step = torch.zeros(1, dtype=torch.int32, device=DEV)
        lcfg = _loss_cfg(eng.H, eng.W, 1.0, 0.0, 0.0, 1, 0, 1, 0.99)
        ad = _lib.Mm3dgsPoseAdam()
        ad.pose, ad.m, ad.v, ad.step = pose.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr()
        ad.lr_q, ad.lr_t, ad.beta1, ad.beta2, ad.eps = 0.002, 0.002, 0.9, 0.999, 1e-8
        eng.track_loop(12, pose, g, lcfg, gt, None, ad)
        torch.cuda.synchronize()
        assert eng.check_capacity() and eng.direct == direct
        results.append((pose.clone(), eng.loss.clone(), eng.out.clone(), int(step)))
    (pa, la, oa, sa), (pb, lb, ob, sb) = results
    assert sa == sb == 12
    assert torch.equal(pa, pb), (pa, pb)
    assert torch.equal(la, lb) and torch.equal(oa, ob)


@pytest.mark.parametrize("pearson,white,P,H,W", [(False, False, 20000, 120, 168), (True, False, 20000, 120, 168), (False, True, 20000, 120, 168)]
                         + [(pearson, white, P, 48, 64) for P in (255, 257) for pearson, white in ((False, False), (True, False), (False, True))],
                         ids=["False-False", "True-False", "False-True"]
                         + [f"{pearson}-{white}-P{P}-48x64" for P in (255, 257) for pearson, white in ((False, False), (True, False), (False, True))])
def test_tracking_pose_chain_matches_the_record_path(pearson, white, P, H, W, monkeypatch):
    """Round 6: mm3dgs_slam_track applies the pose chain per (block, splat) inside the tracking compositor (GeomView.poserec: the projection writes
    every splat's linear map from its gradient moments to dL/d(camera-space mean); the compositor leaves one pose row per tile) -- no gradient
    records, no per-tile combine, no backward-projection launch.  MM3DGS_NO_POSE_CHAIN=1 keeps the record path, the one the float64 oracle
    comparisons run on (mm3dgs_slam_backward): the pose GRADIENT of an iteration (read back as Adam's first moment after one step with the
    learning rates at 0: m = 0.1 g) must agree to float32 rounding of two summation orders, and so must a 12-step trajectory.  Masked L1 (the
    fused sort + forward + backward launch), + Pearson (separate compositor launches, dL3 != 0), white background (the general loop instance:
    four lanes per entry).  The 48x64 cases put P on either side of the 256-Gaussian projection workgroup that geom_state's block_tiles and,
    behind it, poserec are laid out on (one workgroup with a dead lane, two workgroups with one live lane in the second)."""
    from mm3dgs_slam_amd import _lib
    from mm3dgs_slam_amd.fused import FusedEngine, _loss_cfg
    cfg, g, R, pose0, color, depth = _setup(P=P, H=H, W=W, seed=4, white=white)
    with torch.no_grad():
        r0 = R.render(g, pose0)
        gt, ref = r0["render"].contiguous(), r0["depth"][0].contiguous()
    out = {}
    for no_chain in ("1", "0"):
        monkeypatch.setenv("MM3DGS_NO_POSE_CHAIN", no_chain)
        eng = FusedEngine(R)
        eng.forward(pose0, g)
        assert eng.check_capacity()
        res = []
        for lr, n in ((0.0, 1), (0.002, 12)):
            pose = (pose0 + torch.tensor([0.0, 0.004, -0.003, 0.002, 0.01, -0.008, 0.012], device=DEV)).contiguous()
            m, v = torch.zeros(7, device=DEV), torch.zeros(7, device=DEV)
            step = torch.zeros(1, dtype=torch.int32, device=DEV)
            lcfg = _loss_cfg(eng.H, eng.W, 1.0, 0.0, 0.05 if pearson else 0.0, 1, 1 if pearson else 0, 1, 0.99)
            ad = _lib.Mm3dgsPoseAdam()
            ad.pose, ad.m, ad.v, ad.step = pose.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr()
            ad.lr_q, ad.lr_t, ad.beta1, ad.beta2, ad.eps = lr, lr, 0.9, 0.999, 1e-8
            eng.track_loop(n, pose, g, lcfg, gt, ref if pearson else None, ad)
            torch.cuda.synchronize()
            assert eng.check_capacity() and int(step) == n
            res.append((pose.clone(), (m / 0.1).clone(), eng.loss.clone()))
        out[no_chain] = res
    (p1a, ga, la), (p12a, _, _) = out["1"]
    (p1b, gb, lb), (p12b, _, _) = out["0"]
    print(f"pose chain P={P} {H}x{W}: rel_l2 {pu.rel_l2(gb, ga):.3e}  loss equal {torch.equal(la, lb)}  12-step pose diff {float((p12a - p12b).abs().max()):.3e}")
    assert torch.equal(p1a, p1b) and float(ga.abs().max()) > 0
    assert pu.rel_l2(gb, ga) < 2e-6, (ga, gb)
    assert torch.equal(la, lb)
    # (48x64: the white-background case at P = 255 measured 3.42e-6 on the 12-step poses before the layout change, every other small case
    #  under 1e-7 -- twice that figure, for the summation order of lists this short)
    assert (p12a - p12b).abs().max() < (2e-6 if (H, W) != (48, 64) else 2 * 3.4235e-6), (p12a, p12b)


def test_fused_path_with_huge_splats_matches_torch_graph():
    """Same for the native SLAM path: a map whose Gaussians each cover dozens of tiles (wave-cooperative gather of the
    dense gradient records, block rectangles far larger than a tile)."""
    from mm3dgs_slam_amd.fused import FusedEngine
    cfg, g, R, pose, color, depth = _setup(P=300, H=128, W=160, seed=6)
    with torch.no_grad():
        g._scaling += 3.0
    eng = FusedEngine(R)
    si = eng.forward(pose, g, need_grads=True)
    assert eng.check_capacity()
    p = pose.clone().requires_grad_(True)
    res = R.render(g, p)
    ref = torch.cat([res["render"], res["depth"]], 0)
    assert int((res["radii"] > 40).sum()) > 100       # the case really has huge splats
    assert pu.rel_l2(eng.out, ref) < 1e-5
    w = torch.randn(6, eng.H, eng.W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    (ref * w).sum().backward()
    eng.dL.copy_(w)
    eng.backward(si, grads=eng.grads, dpose=eng.dpose)
    assert pu.rel_l2(eng.dpose, p.grad) < 5e-4, (eng.dpose, p.grad)
    for name, param in (("xyz", g._xyz), ("f_dc", g._features_dc), ("opacity", g._opacity), ("scaling", g._scaling)):
        assert pu.rel_l2(eng.grads[name], param.grad) < 5e-4, name


# ---- round 2: the optimiser code the benchmark actually runs, one step at a time --------------------------------------
def _mk_adam_state(g):
    """(Mm3dgsMapAdam over fresh moments, dict of the moment tensors) for the five native parameter groups."""
    from mm3dgs_slam_amd import _lib
    ma = _lib.Mm3dgsMapAdam()
    lrs = dict(xyz=1.6e-4, f_dc=2.5e-3, opacity=5e-2, scaling=1e-3, rotation=1e-3)
    st = {}
    for i, (name, prm) in enumerate((("xyz", g._xyz), ("f_dc", g._features_dc), ("opacity", g._opacity), ("scaling", g._scaling),
                                     ("rotation", g._rotation))):
        st[name] = (prm, torch.zeros_like(prm), torch.zeros_like(prm), lrs[name])
        ma.param[i], ma.exp_avg[i], ma.exp_avg_sq[i], ma.lr[i] = prm.data_ptr(), st[name][1].data_ptr(), st[name][2].data_ptr(), lrs[name]
    ma.beta1, ma.beta2, ma.eps, ma.step = 0.9, 0.999, 1e-15, 1
    return ma, st


@pytest.mark.parametrize("iso", [False, True])
def test_in_kernel_map_adam_equals_gradient_output_plus_torch_adam(iso):
    """mm3dgs_slam_backward with `map_adam` (the step the benchmark's mapping loop takes inside slam_preprocess_bwd) against
    the SAME kernel's gradient outputs fed to torch.optim.Adam(eps=1e-15), three consecutive steps (bias corrections,
    moment carry-over).  <= 1e-6 relative on parameters and moments."""
    from mm3dgs_slam_amd.fused import FusedEngine
    cfg, g, R, pose, color, depth = _setup(P=12000, H=120, W=160, iso=iso, seed=5)
    eng = FusedEngine(R)
    names = ("xyz", "f_dc", "opacity", "scaling", "rotation")
    with torch.no_grad():
        ref_params = {n: p.detach().clone().requires_grad_(True) for n, p in zip(names, (g._xyz, g._features_dc, g._opacity, g._scaling, g._rotation))}
    ma, st = _mk_adam_state(g)
    opt = torch.optim.Adam([{"params": [ref_params[n]], "lr": st[n][3]} for n in names], lr=0.0, eps=1e-15)
    gen = torch.Generator(device=DEV).manual_seed(9)
    with torch.no_grad():
        for step in range(1, 4):
            si = eng.forward(pose, g, need_grads=True)
            eng.dL.copy_(torch.randn(6, eng.H, eng.W, device=DEV, generator=gen))
            # (1) gradients only, from the current parameters
            eng.backward(si, grads=eng.grads)
            for n in names:
                ref_params[n].grad = eng.grads[n].reshape(ref_params[n].shape).clone()
            # (2) the same backward with the Adam step inside the kernel
            ma.step = step
            eng.backward(si, map_adam=ma)
            opt.step()
            torch.cuda.synchronize()
            for n in names:
                prm, m_, v_, _ = st[n]
                s_ref = opt.state[ref_params[n]]
                assert pu.rel_l2(prm, ref_params[n]) <= 1e-6, (n, step, "param")
                assert pu.rel_l2(m_, s_ref["exp_avg"]) <= 1e-6, (n, step, "exp_avg")
                assert pu.rel_l2(v_, s_ref["exp_avg_sq"]) <= 1e-6, (n, step, "exp_avg_sq")
                # and element-wise: Adam(eps=1e-15) normalises every gradient to ~lr, so a relative bound per element is meaningful
                assert (prm - ref_params[n]).abs().max() <= 2e-6 * max(1.0, float(ref_params[n].abs().max())) + 1e-3 * st[n][3], (n, step)
    assert eng.check_capacity()


def test_on_device_pose_adam_follows_torch_adam_step_for_step():
    """mm3dgs_slam_backward with `pose_adam` (slam_pose_finish_kernel) against its own dL/dpose output fed to
    torch.optim.Adam (two groups: translation lr, rotation lr; default eps 1e-8 -- slam/tracker.py:233-246), five steps."""
    from mm3dgs_slam_amd import _lib
    from mm3dgs_slam_amd.fused import FusedEngine
    cfg, g, R, pose0, color, depth = _setup(P=12000, H=120, W=160, seed=6)
    eng = FusedEngine(R)
    pose = pose0.clone().contiguous()
    m, v = torch.zeros(7, device=DEV), torch.zeros(7, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    ad = _lib.Mm3dgsPoseAdam()
    ad.pose, ad.m, ad.v, ad.step = pose.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr()
    ad.lr_q, ad.lr_t, ad.beta1, ad.beta2, ad.eps = 0.003, 0.001, 0.9, 0.999, 1e-8
    q_ref, t_ref = pose0[:4].clone().requires_grad_(True), pose0[4:].clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [t_ref], "lr": 0.001}, {"params": [q_ref], "lr": 0.003}])
    gen = torch.Generator(device=DEV).manual_seed(3)
    with torch.no_grad():
        for it in range(5):
            si = eng.forward(pose, g)
            eng.dL.copy_(torch.randn(6, eng.H, eng.W, device=DEV, generator=gen) * 1e-3)
            eng.backward(si, dpose=eng.dpose)                       # gradient at the current pose
            q_ref.grad, t_ref.grad = eng.dpose[:4].clone(), eng.dpose[4:].clone()
            eng.backward(si, pose_adam=ad)                          # same gradient, stepped on the device
            opt.step()
            torch.cuda.synchronize()
            ref = torch.cat([q_ref.detach(), t_ref.detach()])
            assert int(step) == it + 1
            assert (pose - ref).abs().max() <= 1e-6, (it, pose, ref)
            assert pu.rel_l2(m, torch.cat([opt.state[q_ref]["exp_avg"], opt.state[t_ref]["exp_avg"]])) <= 1e-6
            assert pu.rel_l2(v, torch.cat([opt.state[q_ref]["exp_avg_sq"], opt.state[t_ref]["exp_avg_sq"]])) <= 1e-6


def test_loss_kernels_match_the_reference_fixture_g8():
    """mm3dgs_loss against G8 (tests/golden/make_golden.py: the reference's own l1_loss / ssim and autograd):
    0.8 L1 + 0.2 (1 - SSIM) value and gradient image, masked-L1 (tracking) value and gradient."""
    import os
    from mm3dgs_slam_amd import _lib
    from mm3dgs_slam_amd.fused import _loss_cfg, _p
    from mm3dgs_slam_amd.rasterizer import _stream
    d = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(os.path.dirname(__file__), "golden", "g8_loss.npz")).items()}
    H, W = d["img"].shape[1:]
    lib = _lib.load()
    out6 = torch.cat([d["img"], d["depth"][None], d["sil"][None], (d["depth"] ** 2)[None]], 0).to(DEV).contiguous()
    gt = d["gt"].to(DEV).contiguous()
    work = torch.empty(lib.mm3dgs_loss_work_bytes(H, W), dtype=torch.uint8, device=DEV)
    dL, loss4 = torch.empty(6, H, W, device=DEV), torch.zeros(4, device=DEV)
    lc = _loss_cfg(H, W, 0.8, 0.2, 0.0, 0, 0, 0, 0.5)
    _lib.check(lib.mm3dgs_loss(lc, _p(out6), _p(gt), None, _p(work), _p(dL), _p(loss4), _stream()))
    torch.cuda.synchronize()
    assert abs(float(loss4[0]) - float(d["map_photo"])) <= 2e-6
    assert abs(float(loss4[1]) - float(d["l1"])) <= 2e-6 and abs((1.0 - float(loss4[2])) - float(d["ssim"])) <= 2e-6
    assert pu.rel_l2(dL[:3], d["d_map_photo"]) <= 2e-5
    assert float(dL[3:].abs().max()) == 0.0
    lc = _loss_cfg(H, W, 1.0, 0.0, 0.0, 1, 0, 1, 0.99)           # tracking: masked mean L1 over silhouette > 0.99
    _lib.check(lib.mm3dgs_loss(lc, _p(out6), _p(gt), None, _p(work), _p(dL), _p(loss4), _stream()))
    torch.cuda.synchronize()
    assert abs(float(loss4[0]) - float(d["l1_masked"])) <= 2e-6
    assert pu.rel_l2(dL[:3], d["d_l1_masked"]) <= 1e-6
    # Pearson call patterns (values): mapping with gt depth (mask ref > 0), tracking with gt depth (silhouette & ref > 0, min of two targets)
    ref = d["ref_depth"].to(DEV).contiguous()
    for lc, key in ((_loss_cfg(H, W, 0.0, 0.0, 1.0, 0, 2, 0, 0.5), "pearson_map_gt"), (_loss_cfg(H, W, 0.0, 0.0, 1.0, 1, 3, 1, 0.99), "pearson_track_gt")):
        _lib.check(lib.mm3dgs_loss(lc, _p(out6), _p(gt), _p(ref), _p(work), _p(dL), _p(loss4), _stream()))
        torch.cuda.synchronize()
        assert abs(float(loss4[3]) - float(d[key])) <= 2e-5, (key, float(loss4[3]), float(d[key]))


def test_native_tracker_with_imu_prior_follows_the_torch_graph_tracker():
    """tracking.use_imu_loss: rel_pose_loss (utils/loss_utils.py:20-40, slam/tracker.py:146-155) added on the device in
    slam_pose_finish_kernel; trajectory vs the torch-graph Tracker with the same (guarded) residual."""
    from mm3dgs_slam_amd.fused import FusedTracker
    from mm3dgs_slam_amd.tracker import Tracker
    cfg, g, R, pose0, color, depth = _setup(P=15000, H=120, W=160, seed=8)
    cfg["tracking"].update(use_imu_loss=True, imu_T_weight=5.0, imu_q_weight=0.5, iters=25)
    with torch.no_grad():
        res = R.render(g, pose0)
        gt_color, gt_depth = res["render"].contiguous(), res["depth"][0].contiguous()
    start = (pose0 + torch.tensor([0.0, 0.003, -0.002, 0.002, 0.008, -0.006, 0.01], device=DEV)).contiguous()
    outs = []
    for cls in (Tracker, FusedTracker):
        trk = cls(cfg, g, R, [None, None])
        q = start[:4].clone().requires_grad_(True); T = start[4:].clone().requires_grad_(True)
        opt = torch.optim.Adam([{"params": [T], "lr": cfg["tracking"]["position_lr"]}, {"params": [q], "lr": cfg["tracking"]["rotation_lr"]}])
        loss, _ = trk.optimize_cam(1, 25, opt, q, T, gt_color, gt_depth, gt_depth)
        outs.append((torch.cat([q.detach(), T.detach()]), float(loss)))
    (pa, la), (pb, lb) = outs
    assert torch.isfinite(pa).all() and torch.isfinite(pb).all()
    assert (pa - pb).abs().max() < 3e-4, (pa, pb)
    assert abs(la - lb) < 1e-3 * max(1.0, abs(la)), (la, lb)
    # the prior really acts: without it the same start ends somewhere else
    cfg["tracking"].update(use_imu_loss=False)
    trk = FusedTracker(cfg, g, R, [None, None])
    q = start[:4].clone().requires_grad_(True); T = start[4:].clone().requires_grad_(True)
    trk.optimize_cam(1, 25, None, q, T, gt_color, gt_depth, gt_depth)
    assert (torch.cat([q.detach(), T.detach()]) - pb).abs().max() > 1e-4


@pytest.mark.parametrize("variant", ["l1", "pearson", "imu"])
def test_native_tracker_keeps_the_best_candidate_like_the_torch_graph_tracker(variant):
    """keep_best_candidate (this repository's option for what slam/tracker.py:88-91,161-181 computes and, by a rebinding bug, discards): the
    pose-finish kernel keeps { loss at the rendered pose, pose after the step } of the best iteration (Mm3dgsPoseAdam.best) in all three forms
    of the tracking loop -- masked L1 alone (the loss is formed inside the finish kernel), with the Pearson term (formed by the compositor /
    loss launches before it), with the IMU prior (added by the finish kernel).  A start far from the optimum and large learning rates make
    the loss non-monotonic, so the best candidate is NOT the last iterate; it must be the torch-graph Tracker's."""
    from mm3dgs_slam_amd.fused import FusedTracker
    from mm3dgs_slam_amd.tracker import Tracker
    cfg, g, R, pose0, color, depth = _setup(P=15000, H=120, W=160, seed=8)
    cfg["tracking"].update(iters=30, position_lr=0.004, rotation_lr=0.006)      # overshoots: the loss goes up and down
    if variant == "pearson":
        cfg["tracking"].update(use_depth_estimate_loss=True, pearson_weight=0.05)
    if variant == "imu":
        cfg["tracking"].update(use_imu_loss=True, imu_T_weight=5.0, imu_q_weight=0.5)
    with torch.no_grad():
        res = R.render(g, pose0)
        gt_color, gt_depth = res["render"].contiguous(), res["depth"][0].contiguous()
    start = (pose0 + torch.tensor([0.0, 0.004, -0.003, 0.003, 0.012, -0.009, 0.015], device=DEV)).contiguous()
    outs = {}
    for name, cls, keep in (("graph", Tracker, True), ("native", FusedTracker, True), ("native_last", FusedTracker, False)):
        trk = cls(cfg, g, R, [None, None], keep_best_candidate=keep)
        q = start[:4].clone().requires_grad_(True); T = start[4:].clone().requires_grad_(True)
        opt = torch.optim.Adam([{"params": [T], "lr": cfg["tracking"]["position_lr"]}, {"params": [q], "lr": cfg["tracking"]["rotation_lr"]}])
        trk.optimize_cam(1, 30, opt, q, T, gt_color, gt_depth, gt_depth)
        outs[name] = torch.cat([q.detach(), T.detach()])
    assert all(torch.isfinite(v).all() for v in outs.values())
    # the candidate is a pose of the SAME trajectory in both programs (the trajectories agree to ~1e-4 per test_native_tracker_with_imu_prior...);
    # picking another iteration would be off by a whole optimiser step (4e-3 here)
    assert (outs["graph"] - outs["native"]).abs().max() < 5e-4, (outs["graph"], outs["native"])
    if variant != "imu":      # (the prior pulls the pose back: with it the loss decreases monotonically here and the last iterate IS the best)
        assert (outs["native"] - outs["native_last"]).abs().max() > 1e-3, "the best candidate should not be the last iterate in this set-up"


@pytest.mark.parametrize("direct", [False, True])
def test_binning_overflow_is_sticky_and_the_loops_recover(direct, monkeypatch):
    """A capacity far too small for the scene: the header's overflow flag must survive later (non-overflowing) forwards until
    the host reads it, and FusedTracker / FusedMapper must end where a run with ample capacity ends (restore + re-run).
    Packed bins run out of total capacity, direct bins (one fixed span per tile) out of per-tile capacity."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.fused import FusedEngine, _engine
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    monkeypatch.setattr(FusedEngine, "DIRECT_BINS", direct)
    cfg, g, R, pose, color, depth = _setup(P=12000, H=120, W=160, seed=9)
    eng = FusedEngine(R)
    eng.forward(pose, g, need_grads=True)
    assert eng.check_capacity()
    n_true = int(eng.ratio * eng.P + 0.5)
    true_ratio = eng.ratio
    # a capacity model that claims ~0 pairs per Gaussian (and one-entry tile lists) -> tiny binning buffer -> overflow (flagged);
    # then a view that fits: the flag, the maximum N and the maximum list length must still be there
    eng.MIN_PAIRS = 64
    eng.ratio, eng.n_cap, eng.max_tile_len = 0.01, 0, 1
    eng.forward(pose, g, need_grads=True)
    assert eng.direct == direct
    assert eng.n_cap < n_true
    far = pose.clone(); far[6] -= 1000.0                    # the whole map behind the camera: nothing rendered, no overflow
    eng.forward(far, g, need_grads=True)
    torch.cuda.synchronize()
    hdr = eng.img_state[:16].view(torch.int32).cpu()
    assert int(hdr[1]) == 1 and int(hdr[3]) >= n_true - 1 and int(hdr[0]) < n_true       # sticky overflow / max N; last N small
    assert not eng.check_capacity()
    assert eng.ratio >= true_ratio * 0.999                   # capacity model learned the true need from the overflowing call
    assert eng.check_capacity()                              # cleared by the read
    # whole loops: same result with a deliberately starved engine as with a healthy one
    results = []
    for starve in (False, True):
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        cfg2 = default_config(device=DEV, height=120, width=160, tracking={"iters": 6}, mapping={"iters": 8})
        seq = SyntheticSequence(cfg2, 3, 8000, seed=2)
        slam = SLAM(cfg2, seq)
        slam.step(0)
        e = _engine(slam.renderer)
        if starve:
            e.MIN_PAIRS = 64
            e.ratio = 0.02                                   # capacity model claims ~0 pairs per Gaussian -> tiny buffers
            e.n_cap = 0
            e.max_tile_len = 1
        random.seed(5)
        slam.step(1); slam.step(2)
        results.append((torch.stack(slam.estimate_pose_list[:3]).cpu(), slam.gaussians._xyz.detach().cpu(), getattr(e, "overflows", 0)))
    (pa, xa, oa), (pb, xb, ob) = results
    assert oa == 0 and ob >= 1
    assert torch.equal(pa, pb) and torch.equal(xa, xb)


@pytest.mark.parametrize("direct", [False, True])
def test_an_overflowing_iteration_is_void_not_garbage(direct, monkeypatch):
    """a forward that overflows drops pairs WITHOUT writing their per-tile gradient records; with the lazy capacity
    checks nothing restores the map afterwards.  The backward entry points therefore read the sticky overflow word and take no
    optimiser step at all while it is set (csrc/fused.hip slam_bwd_body, slam_pose_finish_kernel): parameters, Adam moments,
    statistics and the tracked pose must come out of a starved loop bit-identical to what went in -- and move again once the word is
    cleared and the capacity raised."""
    from mm3dgs_slam_amd.fused import FusedEngine, _loss_cfg
    from mm3dgs_slam_amd import _lib
    monkeypatch.setattr(FusedEngine, "DIRECT_BINS", direct)
    cfg, g, R, pose, color, depth = _setup(P=12000, H=120, W=160, seed=9)
    eng = FusedEngine(R)
    eng.forward(pose, g, need_grads=True)
    assert eng.check_capacity()
    with torch.no_grad():
        gt = eng.out[:3].clone().contiguous(); ref = eng.out[3].clone().contiguous()
    opt = g.optimizer
    names = ("xyz", "f_dc", "opacity", "scaling", "rotation")

    def adam(n):
        ma = _lib.Mm3dgsMapAdam()
        for i, name in enumerate(names):
            group = next(gr for gr in opt.param_groups if gr["name"] == name)
            p_ = group["params"][0]
            st = opt.state[p_]
            if "exp_avg" not in st:
                st["step"] = torch.tensor(0.0); st["exp_avg"] = torch.zeros_like(p_); st["exp_avg_sq"] = torch.zeros_like(p_)
            ma.param[i], ma.exp_avg[i], ma.exp_avg_sq[i] = p_.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            ma.lr[i] = float(group["lr"]) if float(group["lr"]) > 0 else 1e-3
        ma.beta1, ma.beta2, ma.eps, ma.step = 0.9, 0.999, 1e-15, 1
        return ma

    def state():
        out = [t.detach().clone() for t in (g._xyz, g._features_dc, g._opacity, g._scaling, g._rotation, g.max_radii2D, g.xyz_gradient_accum, g.denom)]
        for name in names:
            st = opt.state[next(gr for gr in opt.param_groups if gr["name"] == name)["params"][0]]
            out += [st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
        return out

    lcfg = _loss_cfg(eng.H, eng.W, 0.8, 0.2, 0.05, 0, 2, 0, 0.5)
    view = (pose + torch.tensor([0.0, 0.002, -0.001, 0.001, 0.01, -0.005, 0.004], device=DEV)).contiguous()
    views = [(view, gt, ref)] * 4
    stats = (g.max_radii2D, g.xyz_gradient_accum, g.denom)
    ma = adam(4)
    before = state()
    # starve the engine: tiny buffers -> every forward of the run overflows (flagged sticky), no host check in between
    eng.MIN_PAIRS = 64
    eng.ratio, eng.n_cap, eng.max_tile_len = 0.01, 0, 1
    eng.map_loop(views, g, lcfg, stats, ma)
    torch.cuda.synchronize()
    assert int(eng.img_state[:8].view(torch.int32).cpu()[1]) == 1
    for a, b in zip(before, state()):
        assert torch.equal(a, b)
    # tracking: the pose and its Adam state stay put as well
    p0 = view.clone(); m_, v_ = torch.zeros(7, device=DEV), torch.zeros(7, device=DEV); step = torch.zeros(1, dtype=torch.int32, device=DEV)
    ad = _lib.Mm3dgsPoseAdam()
    ad.pose, ad.m, ad.v, ad.step = p0.data_ptr(), m_.data_ptr(), v_.data_ptr(), step.data_ptr()
    ad.lr_q, ad.lr_t, ad.beta1, ad.beta2, ad.eps = 0.003, 0.001, 0.9, 0.999, 1e-8
    eng.track_loop(3, p0, g, _loss_cfg(eng.H, eng.W, 1.0, 0.0, 0.0, 1, 0, 1, 0.99), gt, None, ad)
    torch.cuda.synchronize()
    assert torch.equal(p0, view) and int(step.cpu()[0]) == 0 and float(m_.abs().max()) == 0.0
    # the host reads the header (clears the word, raises the capacity): the same calls now do their work
    assert not eng.check_capacity()
    for _ in range(4):      # (the capacity model may need more than one overflowing call to learn every one of its three limits)
        eng.map_loop(views, g, lcfg, stats, ma)
        torch.cuda.synchronize()
        if eng.check_capacity():
            break
    else:
        raise AssertionError("capacity never sufficed")
    eng.track_loop(3, p0, g, _loss_cfg(eng.H, eng.W, 1.0, 0.0, 0.0, 1, 0, 1, 0.99), gt, None, ad)
    torch.cuda.synchronize()
    assert eng.check_capacity()
    after = state()
    assert not torch.equal(before[0], after[0]) and all(torch.isfinite(t).all() for t in after)
    assert not torch.equal(p0, view) and int(step.cpu()[0]) == 3


def test_load_balanced_tile_table_is_a_permutation_and_changes_nothing_but_speed(monkeypatch):
    """The SLAM loops deal the tiles of every XCD's span to its workgroup slots by the list lengths of the last render (binning.hip
    tile_order_kernel; MM3DGS_NO_TILE_ORDER=1 keeps the arithmetic workgroup -> tile map).  The table must be a permutation of the grid's
    tiles (+ zeros for the workgroups beyond it), and three SLAM frames must end bit-identical with and without it -- every per-tile
    result lands at an address that depends on the tile alone."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.fused import _engine
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence

    def run(flag, H, W):
        monkeypatch.setenv("MM3DGS_NO_TILE_ORDER", flag)
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        cfg = default_config(device=DEV, height=H, width=W, tracking={"iters": 5}, mapping={"iters": 12, "kf_every": 1, "pruning_interval": 5})
        seq = SyntheticSequence(cfg, 3, 6000, seed=6)
        slam = SLAM(cfg, seq)
        for i in range(3):
            slam.step(i)
        g, e = slam.gaussians, _engine(slam.renderer)
        torch.cuda.synchronize()
        T = ((W + 15) // 16) * ((H + 15) // 16)
        up = lambda v: (v + 255) // 256 * 256
        off = 256 + up(T * 4) + up((T + 1) * 4) + up(T * 4) + up(T * 16 * 4) + 2 * up(H * W * 4)
        n = (T + 7) // 8 * 8
        table = e.img_state[off:off + 4 * n].view(torch.int32).cpu().numpy()
        valid = int(e.img_state[36:40].view(torch.int32).cpu()[0])
        state = dict(xyz=g._xyz.detach().clone(), op=g._opacity.detach().clone(), sc=g._scaling.detach().clone(), fdc=g._features_dc.detach().clone(),
                     acc=g.xyz_gradient_accum.clone(), poses=torch.stack([p.detach().clone() for p in slam.estimate_pose_list[:3]]))
        return state, table, valid, T
    # 260 tiles (33 per XCD: two rounds of CU slots), 88 (11 per XCD: one round), the TUM grid (1200: 150 per XCD, five rounds) and the UTMM grid
    # (840: 105 per XCD, four rounds)
    for H, W in ((208, 320), (120, 170), (480, 640), (330, 640)):
        a, table, valid, T = run("0", H, W)
        assert valid == (H << 16 | W)
        assert sorted(int(v) for v in table if v) == list(range(1, T + 1)), "not a permutation of the tiles"
        assert int((table == 0).sum()) == len(table) - T
        # every XCD's span is contiguous in tile order, the spans follow each other, and each fills its XCD's first slots
        per_xcd = [sorted(int(v) - 1 for v in table[x::8] if v) for x in range(8)]
        for x, tl in enumerate(per_xcd):
            assert tl == list(range(tl[0], tl[0] + len(tl))), x
            assert all(int(v) != 0 for v in table[x::8][:len(tl)]) and all(int(v) == 0 for v in table[x::8][len(tl):]), x
        assert [tl[0] for tl in per_xcd] == [0] + [per_xcd[x - 1][-1] + 1 for x in range(1, 8)]
        b, _, valid_off, _ = run("1", H, W)
        assert valid_off == 0                        # (fresh engine, never written)
        for k in a:
            assert torch.equal(a[k], b[k]), (H, W, k)


def test_keyframe_test_with_deferred_capacity_check_recovers_from_an_overflowing_render():
    """The keyframe test's render does not read its capacity header back on its own: the copy rides on the read-back of the covisibility
    counters (FusedEngine.check_capacity_begin / _end).  If that render overflowed, covisibility_ratio_dense must notice, render again
    with the raised capacity and return the ratio of the complete render -- the same number a healthy engine gives."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.fused import _engine
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg2 = default_config(device=DEV, height=120, width=160, tracking={"iters": 4}, mapping={"iters": 4})
    seq = SyntheticSequence(cfg2, 3, 8000, seed=2)
    slam = SLAM(cfg2, seq)
    slam.step(0); slam.step(1)
    m, e = slam.mapper, _engine(slam.renderer)
    kf_pose, cur_pose = m.keyframes[-1].pose, slam.estimate_pose_list[1]

    def ratio():
        m._defer_render_check = True
        try:
            with torch.no_grad():
                depth, sil = m._render_depth_sil(kf_pose)
                assert m._pending_render_check is not None          # (the check really was deferred)
                return float(m.covisibility_ratio_dense(depth, sil, kf_pose, cur_pose))
        finally:
            m._defer_render_check, m._pending_render_check = False, None
    healthy, before = ratio(), getattr(e, "overflows", 0)
    assert 0.5 < healthy <= 1.0
    e.MIN_PAIRS, e.ratio, e.n_cap, e.max_tile_len = 64, 0.02, 0, 1       # capacity model claims ~0 pairs per Gaussian -> tiny buffers
    starved = ratio()
    assert getattr(e, "overflows", 0) == before + 1
    assert starved == healthy, (starved, healthy)
    assert e.check_capacity()                                            # nothing left pending in the header


@pytest.mark.parametrize("pearson", [False, True])
def test_mapping_loss_via_forward_rows_matches_the_standalone_loss_kernels(pearson, monkeypatch):
    """Three forms of the mapping loss inside mm3dgs_slam_map, same per-pixel arithmetic, different launch structure:
    A  MM3DGS_NO_FORWARD_ROWS=1: the standalone mm3dgs_loss (tile sums + SSIM maps, finish, gradient image with 6 planes);
    B  tile sums from the forward compositor's epilogue, reduced by the SSIM kernel's extra workgroup, gradient image with 4 planes
       (MM3DGS_NO_FOLDED_LOSS=1 keeps the gradient pass a launch of its own);
    C  (default) as B with the gradient pass inside the backward compositor's prologue -- no gradient image at all."""
    from mm3dgs_slam_amd.fused import FusedEngine, _loss_cfg
    cfg, g, R, pose, color, depth = _setup(P=15000, H=200, W=272, seed=11)
    lc = _loss_cfg(200, 272, 0.8, 0.2, 0.05 if pearson else 0.0, 0, 2 if pearson else 0, 0, 0.5)
    ref = depth.contiguous() if pearson else None
    res = {}
    for name, no_rows, no_fold in (("A", "1", "0"), ("B", "0", "1"), ("C", "0", "0")):
        monkeypatch.setenv("MM3DGS_NO_FORWARD_ROWS", no_rows)
        monkeypatch.setenv("MM3DGS_NO_FOLDED_LOSS", no_fold)
        eng = FusedEngine(R)
        eng.max_tile_len = 100          # "short lists": the fused sort + composite kernel (carries the epilogue)
        eng.dL.fill_(float("nan"))      # planes the form does not write must not be read
        eng.map_loop([(pose.contiguous(), color.contiguous(), ref)], g, lc, None, None, grads=eng_grads(eng, g))
        torch.cuda.synchronize()
        assert eng.check_capacity()
        res[name] = ({k: v.clone() for k, v in eng.grads.items()}, eng.loss.clone(), eng.dL.clone())
    ga, la, da = res["A"]
    assert torch.isfinite(da).all() and torch.isfinite(res["B"][2][:4]).all() and torch.isnan(res["B"][2][4:]).all()
    assert torch.isnan(res["C"][2]).all()                    # form C never touches the gradient image
    assert pu.rel_l2(res["B"][2][:4], da[:4]) < 1e-6
    for name in ("B", "C"):
        gb, lb, _ = res[name]
        assert (la - lb).abs().max() < 1e-6 * max(1.0, float(la.abs().max())), (name, la, lb)
        for k in ga:
            assert torch.isfinite(gb[k]).all(), (name, k)
            assert pu.rel_l2(gb[k], ga[k]) < 1e-5, (name, k)


def eng_grads(eng, g):
    eng._ensure(int(g._xyz.shape[0]), True)
    return eng.grads


def test_device_prune_compaction_matches_the_torch_surgery():
    """GaussianModel.prune on the device (predicate kernel + order-preserving compaction of parameters, Adam moments and statistics,
    csrc/compact.hip) against the torch path (slam/gaussian_model.py:380-451,574-588 mirrored in prune_points): same rows, same order.
    The edge sizes (one row .. 1025 workgroups), the NaN rows and the guard words are in tests/test_gpu_surgery.py."""
    import copy
    from mm3dgs_slam_amd.gaussian_model import GaussianModel
    from tests import densify_util as du
    cfg, g, R, pose, color, depth = _setup(P=5000, H=120, W=160, seed=15)
    gen = torch.Generator().manual_seed(4)
    with torch.no_grad():
        g._opacity += (torch.randn(5000, 1, generator=gen) * 4).to(DEV)          # some below sigmoid^-1(0.005)
        g._scaling[::7] += 3.0                                                     # some larger than 0.1 * extent
        g.max_radii2D = (torch.rand(5000, generator=gen) * 150).to(DEV)           # some above the screen-size threshold
    # give the optimiser real moments
    for grp in g.optimizer.param_groups:
        p = grp["params"][0]
        p.grad = torch.randn_like(p)
    g.optimizer.step()
    g.xyz_gradient_accum = torch.rand(5000, 1, device=DEV); g.denom = torch.rand(5000, 1, device=DEV)
    # second input: fixture G12 (SH degree 3: f_rest has 15 rows of its own to move; the reference's moments), its own thresholds
    f = du.load()
    for g, min_opacity, extent in ((g, 0.005, 1.3), (du.model_from_fixture(f, DEV), float(f["min_opacity"]), float(f["extent"]))):
        P = int(g._xyz.shape[0])
        ref = copy.deepcopy(g)
        ref._native = lambda: False                     # force the torch mirror on the copy
        mask_ref = ref.prune(min_opacity, extent, 100.0)
        mask_dev = g.prune(min_opacity, extent, 100.0)
        torch.cuda.synchronize()
        assert 100 < int(mask_ref.sum()) < P - 100
        assert torch.equal(mask_ref, mask_dev)
        for name in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_rgb", "xyz_gradient_accum", "denom", "max_radii2D"):
            assert torch.equal(getattr(g, name).detach(), getattr(ref, name).detach()), name
        for ga, gb in zip(g.optimizer.param_groups, ref.optimizer.param_groups):
            sa, sb = g.optimizer.state[ga["params"][0]], ref.optimizer.state[gb["params"][0]]
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), ga["name"]
        # nothing to prune: every tensor object stays, gradients are dropped (the reference's no-op optimiser step)
        before = g._xyz
        g._xyz.grad = torch.zeros_like(g._xyz)
        g.prune(0.0, 1e9, None)
        assert g._xyz is before and g._xyz.grad is None


def test_device_seeding_matches_the_reference_fixture_g7_and_the_torch_mirror():
    """mm3dgs_seed_gaussians against G7 (the reference's get_pointcloud + initialisation on a 32x24 RGB-D, tests/golden) and, at
    640x480 with a sparse mask, against the torch mirror Mapper.initialize_new_gaussians (same rows in the same raster order).
    The edge shapes (1x1 .. 513x512, 1026 workgroups), row0 and n_rest against the float64 statement are in tests/test_gpu_surgery.py."""
    import os
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.gaussian_model import GaussianModel
    from mm3dgs_slam_amd.sh_utils import RGB2SH
    d = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(os.path.dirname(__file__), "golden", "g7_seed.npz")).items()}
    H, W = d["depth"].shape
    fx, fy, cx, cy = (float(v) for v in d["intr"])
    cfg = default_config(device=DEV, height=H, width=W)
    g = GaussianModel(cfg); g.training_setup()
    mask = (d["depth"] > 0).to(DEV)
    n = g.seed_device(d["color"].to(DEV), d["depth"].to(DEV), mask, d["pose"].to(DEV), fx, fy, cx, cy)
    torch.cuda.synchronize()
    assert n == d["cld"].shape[0] == g._xyz.shape[0]
    assert (g._xyz.detach().cpu() - d["cld"][:, :3]).abs().max() < 2e-5
    assert (g._rgb.detach().cpu() - d["cld"][:, 3:6]).abs().max() == 0
    assert (g._scaling.detach().cpu() - d["log_scale"][:, None]).abs().max() < 2e-6
    assert (g._features_dc.detach().cpu()[:, 0] - RGB2SH(d["cld"][:, 3:6])).abs().max() < 1e-6
    assert float(g._opacity.abs().max()) == 0 and torch.equal(g._rotation.detach().cpu(), torch.tensor([[1.0, 0, 0, 0]]).repeat(n, 1))
    # appended behind an existing map, moments extended with zeros, statistics reset
    for grp in g.optimizer.param_groups:
        grp["params"][0].grad = torch.ones_like(grp["params"][0])
    g.optimizer.step()
    old_xyz = g._xyz.detach().clone()
    n2 = g.seed_device(d["color"].to(DEV), d["depth"].to(DEV), mask & (torch.rand(H, W, device=DEV) < 0.3), d["pose"].to(DEV), fx, fy, cx, cy)
    assert g._xyz.shape[0] == n + n2 and torch.equal(g._xyz.detach()[:n], old_xyz)
    st = g.optimizer.state[g._xyz]
    assert float(st["exp_avg"][n:].abs().max()) == 0 and float(st["exp_avg"][:n].abs().min()) > 0
    assert g.denom.shape == (n + n2, 1) and float(g.denom.abs().max()) == 0


def test_covisible_gaussians_from_the_projection_stage_alone():
    """FusedMapper.get_covisible_gaussians (mm3dgs_slam_visibility: projection only) == the reference's way (a full render per view,
    visibility_filter summed, >= 2; slam/mapper.py:690-716)."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.fused import FusedMapper
    from mm3dgs_slam_amd.mapper import KeyFrame, Mapper
    cfg, g, R, pose, color, depth = _setup(P=20000, H=120, W=160, seed=17)
    poses = [pose, pose + torch.tensor([0, 0.02, -0.01, 0.0, 0.4, 0.0, 0.1], device=DEV), pose + torch.tensor([0, -0.03, 0.02, 0.01, -0.5, 0.1, -0.2], device=DEV)]
    fm, tm = FusedMapper(cfg, g, R, [None] * 4), Mapper(cfg, g, R, [None] * 4)
    for mp in (fm, tm):
        mp.keyframes = [KeyFrame(i, color, p, depth) for i, p in enumerate(poses)]
    cur = pose + torch.tensor([0, 0.01, 0.01, -0.02, 0.2, -0.3, 0.05], device=DEV)
    a = fm.get_covisible_gaussians([0, 1, 2, -1], cur)
    b = tm.get_covisible_gaussians([0, 1, 2, -1], cur)
    assert a.dtype == torch.bool and a.shape == b.shape
    assert 1000 < int(b.sum()) < 20000
    assert int((a != b).sum()) <= 2          # (two float32 projection pipelines: a borderline radius may differ)


def test_pose_prediction_kernel_matches_the_golden_pose_algebra():
    """mm3dgs_propagate_const_vel (utils/pose_utils.py:203-216 on the device, one double-precision lane) against the reference's own
    outputs (tests/golden/g1_pose.npz: propagate_const_vel on 32 pose pairs, generated by importing the reference) and against the float64 host
    restatement the tracker used before (propagate_const_vel_np) on poses one tracking step apart, where it must agree to the last bit
    of float32 almost everywhere (<= 1 ulp: both evaluate the same algebra in double)."""
    from mm3dgs_slam_amd.pose_utils import propagate_const_vel_np
    from mm3dgs_slam_amd.tracker import Tracker
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "g1_pose.npz"))
    poses = torch.from_numpy(d["poses"]).float()
    got = torch.stack([Tracker._predict_const_vel_device(poses[i].to(DEV), poses[i + 1].to(DEV)) for i in range(32)]).cpu()
    want = torch.from_numpy(d["const_vel"]).float()
    # (q and -q are the same rotation: the golden vectors come from the reference's branch choice, the same one)
    assert float((got - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max())), float((got - want).abs().max())      # (the bar of tests/test_golden_host.py)
    gen = torch.Generator().manual_seed(3)
    for _ in range(64):
        a = torch.cat([torch.nn.functional.normalize(torch.randn(4, generator=gen), dim=0) * (1.0 + 0.01 * torch.randn(1, generator=gen)),
                       torch.randn(3, generator=gen)])
        b = a + torch.cat([0.004 * torch.randn(4, generator=gen), 0.01 * torch.randn(3, generator=gen)])
        host = torch.from_numpy(propagate_const_vel_np(a.numpy(), b.numpy())).float()
        dev = Tracker._predict_const_vel_device(a.to(DEV), b.to(DEV)).cpu()
        assert float((host - dev).abs().max()) <= 2.4e-7 * max(1.0, float(host.abs().max())), (host, dev)


def test_keyframe_covisibility_ratio_kernel_matches_the_torch_formulation():
    """mm3dgs_covisibility_ratio (one kernel over the rendered depth / silhouette planes) against Mapper.covisibility_ratio_dense
    (the reference's get_depth_pointcloud + is_covisible, slam/mapper.py:141-216, as element-wise torch operators): the same
    points pass the same tests -- also with a view that loses part of the surface and with invalid (zero-silhouette) pixels."""
    from mm3dgs_slam_amd.fused import FusedMapper
    from mm3dgs_slam_amd.mapper import Mapper
    cfg, g, R, pose, color, depth = _setup(P=12000, H=120, W=160, seed=13)
    fm = FusedMapper.__new__(FusedMapper)
    fm.cfg, fm.gaussians, fm.renderer = cfg, g, R
    with torch.no_grad():
        d, sil = fm._render_depth_sil(pose)
        d, sil = d.clone(), sil.clone()
        sil[:10, :] = 0.5                                      # not surface
        for shift in (0.0, 0.4, 1.5):
            cur = pose.clone(); cur[4] += shift; cur[1] += 0.05 * shift
            a = float(FusedMapper.covisibility_ratio_dense(fm, d, sil, pose, cur))
            b = float(Mapper.covisibility_ratio_dense(fm, d, sil, pose, cur))
            # (same pose: every pixel of image column 0 / row 0 re-projects onto the boundary uu = 0 / vv = 0 itself, and lands on
            #  either side of it in float32 -- in both implementations; elsewhere only a stray boundary pixel can differ)
            assert abs(a - b) <= (2e-3 if shift == 0.0 else 2e-4), (shift, a, b)
            assert 0.0 <= a <= 1.0
    assert b < 0.9                                             # the last view really lost part of the surface


def test_native_bundle_adjustment_follows_the_torch_graph_loop():
    """mapping.do_BA natively (pose Adam on the device inside mm3dgs_slam_map, gradient masking by covisibility inside the in-kernel map
    Adam) against the torch-graph Mapper.optimize_map with do_BA (slam/mapper.py:718-795,931-942): the same window (three keyframes +
    the current frame, poses slightly off), the same keyframe picks, one optimize_map call each.  Reference quirk: the keyframe poses
    never receive a gradient there (fresh views, see fused.py), only the current pose is refined -- both loops must agree on that;
    mapping.ba_optimize_keyframes turns the intended behaviour on in the native loop."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    results = {}
    for name, native, kf_opt in (("torch", False, False), ("native", True, False), ("native_kf", True, True)):
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        cfg = default_config(device=DEV, height=120, width=160, tracking={"iters": 10},
                             mapping={"iters": 12, "do_BA": True, "ba_optimize_keyframes": kf_opt})
        seq = SyntheticSequence(cfg, 5, 8000, seed=4)
        slam = SLAM(cfg, seq, native_loops=native)
        slam.step(0)                                           # seeds the map, first keyframe (BA is off at idx 0)
        mp = slam.mapper
        off = torch.tensor([0.0, 0.002, -0.001, 0.001, 0.004, -0.003, 0.005], device=DEV)
        for i in (1, 2):                                       # two more keyframes at slightly wrong poses, no seeding
            color, depth, gt_pose = seq[i]
            mp.add_keyframe(i, (gt_pose + off * i).clone(), color, depth, depth)
        start_kf = torch.stack([kf.pose for kf in mp.keyframes]).detach().cpu().clone()
        color, depth, gt_pose = seq[3]
        cur = (gt_pose - off).clone()
        start_cur = cur.detach().cpu().clone()
        slam.estimate_pose_list[3] = cur
        random.seed(7)
        mp.optimize_map(3, 12, [0, 1, 2, -1], None, cur, color, depth, depth)
        torch.cuda.synchronize()
        results[name] = (cur.detach().cpu(), torch.stack([kf.pose for kf in mp.keyframes]).detach().cpu(), slam.gaussians._xyz.detach().cpu(),
                         start_kf, start_cur)
    a, b, c = results["torch"], results["native"], results["native_kf"]
    assert a[2].shape == b[2].shape
    assert torch.equal(a[1], a[3]) and torch.equal(b[1], b[3])            # keyframe poses untouched (the reference's quirk), both loops
    assert (a[0] - a[4]).abs().max() > 1e-4                                # ... while the current pose IS refined
    assert (a[0] - b[0]).abs().max() < 5e-4, (a[0], b[0])
    assert pu.rel_l2(b[2], a[2]) < 2e-3
    assert (c[1][1:] - c[3][1:]).abs().max() > 1e-4                        # the flag: window keyframe poses move too


def test_native_bundle_adjustment_with_a_window_batch_follows_the_torch_graph_window():
    """Round 4: do_BA with a sharded mapping window on the HIP loops (two views per optimiser step: Mm3dgsMapView.dpose_out_or_null hands
    each view's pose gradient out, fused.py sums them per pose and steps the poses that were rendered with mm3dgs_adam) against the
    torch-graph window loop (slam/mapper.py:742-760,803-825,944-948 with WindowParallel batch 2): the refined current pose, the untouched
    keyframe poses (the reference's quirk), the map."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from mm3dgs_slam_amd.window_parallel import WindowParallel
    results = {}
    for name, native, kf_opt in (("torch", False, False), ("native", True, False), ("native_kf", True, True)):
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        cfg = default_config(device=DEV, height=120, width=160, tracking={"iters": 10},
                             mapping={"iters": 12, "do_BA": True, "ba_optimize_keyframes": kf_opt})
        seq = SyntheticSequence(cfg, 5, 8000, seed=4)
        slam = SLAM(cfg, seq, native_loops=native, window=WindowParallel(0, 1, batch=2))
        slam.step(0)
        mp = slam.mapper
        off = torch.tensor([0.0, 0.002, -0.001, 0.001, 0.004, -0.003, 0.005], device=DEV)
        for i in (1, 2):
            color, depth, gt_pose = seq[i]
            mp.add_keyframe(i, (gt_pose + off * i).clone(), color, depth, depth)
        start_kf = torch.stack([kf.pose for kf in mp.keyframes]).detach().cpu().clone()
        color, depth, gt_pose = seq[3]
        cur = (gt_pose - off).clone()
        start_cur = cur.detach().cpu().clone()
        slam.estimate_pose_list[3] = cur
        random.seed(7)
        mp.optimize_map(3, 12, [0, 1, 2, -1], None, cur, color, depth, depth)
        torch.cuda.synchronize()
        if native:
            assert type(mp).__name__ == "FusedMapper" and mp._ba_ids, "the native window loop must have handled the bundle adjustment"
        results[name] = (cur.detach().cpu(), torch.stack([kf.pose for kf in mp.keyframes]).detach().cpu(), slam.gaussians._xyz.detach().cpu(),
                         start_kf, start_cur)
    a, b, c = results["torch"], results["native"], results["native_kf"]
    assert a[2].shape == b[2].shape
    assert torch.equal(a[1], a[3]) and torch.equal(b[1], b[3])
    assert (a[0] - a[4]).abs().max() > 1e-4
    assert (a[0] - b[0]).abs().max() < 5e-4, (a[0], b[0])
    assert pu.rel_l2(b[2], a[2]) < 2e-3
    assert (c[1][1:] - c[3][1:]).abs().max() > 1e-4


def test_utmm_shaped_config_with_imu_runs_natively_and_tracks():
    """BASELINE.json configs[2] in miniature: configs/UTMM.yml settings (isotropic Gaussians, IMU dead-reckoning for the pose prediction
    over the synthetic IMU rows, Pearson term, IMU relative-pose residual) through the native loops; the trajectory stays on the ground
    truth and the IMU prediction is what the tracker starts from."""
    from mm3dgs_slam_amd.config import utmm_config
    from mm3dgs_slam_amd.pose_utils import propagate_imu
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = utmm_config(device=DEV, tracking={"iters": 30, "use_imu_loss": True, "imu_T_weight": 1.0, "imu_q_weight": 0.1}, mapping={"iters": 20})
    cfg["desired_height"], cfg["desired_width"] = 166, 320          # quarter-size image for the test, same intrinsics scaling
    for k in ("fx", "fy", "cx", "cy"):
        cfg["cam"][k] *= 0.5
    seq = SyntheticSequence(cfg, 5, 30000, seed=3)
    slam = SLAM(cfg, seq)
    assert type(slam.tracker).__name__ == "FusedTracker" and type(slam.mapper).__name__ == "FusedMapper"
    for i in range(5):
        slam.step(i)
    errs = slam.pose_errors()
    assert max(errs[1:]) < 0.01, errs                       # < 1 cm on a trajectory that moves ~1-2 cm per frame
    # the prediction the tracker started frame 4 from is the IMU propagation of its own estimates
    pred = slam.tracker.predict_pose(4, seq.imu(4)).to(DEV)
    want = propagate_imu(slam.estimate_pose_list[3].cpu(), slam.estimate_pose_list[2].cpu(), seq.imu(4), seq.tf["c2i"], seq.dt_cam, 0.01).to(DEV)
    assert torch.allclose(pred, want, atol=1e-6)
    assert (pred - seq.poses[4]).abs().max() < 2e-2          # (dead-reckoned from ESTIMATED poses: their mm-level errors enter the velocity)


def test_backward_launch_that_projects_the_next_view_is_bit_identical(monkeypatch):
    """slam_bwd_project_kernel (the backward projection + Adam step of mapping iteration k and the projection + binning of iteration k + 1
    in one launch, the stepped parameters handed over in registers) against the two separate launches (MM3DGS_NO_FUSED_PROJECT): three SLAM
    frames (tracking, keyframes, pruning, a window of several views), every parameter, statistic and pose bit for bit.  This only holds
    because fused.hip pins floating-point contraction to the source (`#pragma clang fp contract(on)`): with hipcc's default the optimiser
    fused differently around the inlined projection and ~9 % of the conics came out one bit away -- after three frames 3 % of the opacity
    logits differed by more than 1e-5 (Adam with eps = 1e-15 turns last-bit noise of near-zero gradients into +-lr steps)."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence

    def run(flag):
        monkeypatch.setenv("MM3DGS_NO_FUSED_PROJECT", flag)
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        cfg = default_config(device=DEV, height=120, width=160, tracking={"iters": 5}, mapping={"iters": 12, "kf_every": 1, "pruning_interval": 5})
        seq = SyntheticSequence(cfg, 3, 6000, seed=6)
        slam = SLAM(cfg, seq)
        for i in range(3):
            slam.step(i)
        g = slam.gaussians
        return dict(xyz=g._xyz.detach().clone(), op=g._opacity.detach().clone(), sc=g._scaling.detach().clone(), rot=g._rotation.detach().clone(),
                    fdc=g._features_dc.detach().clone(), acc=g.xyz_gradient_accum.clone(), rad=g.max_radii2D.clone(),
                    poses=torch.stack([p.detach().clone() for p in slam.estimate_pose_list[:3]]))
    a, b = run("1"), run("0")
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))
