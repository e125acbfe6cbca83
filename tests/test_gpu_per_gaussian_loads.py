"""The per-Gaussian kernels' loads and stores (csrc/fused.hip: slam_bwd_body, slam_project_vals) at edge sizes.

slam_bwd_body requests everything a lane reads but the gradient records in ONE first round -- the Adam state, the densification statistics and
the opt_mask byte included -- holds it across the record gather and writes the Adam results as one store per array and Gaussian (12 bytes
on the [P, 3] arrays).  The tests here run it on maps of P in {1, 63, 256, 257, 700} Gaussians on a 96x128 image (6x8 tiles) whose arrays
sit 4 bytes past a 16-byte boundary between guard words; every map with P >= 63 holds a Gaussian behind the 0.2 near plane, one off
screen (radii == 0), one covering 17 .. 32 tiles (the record gather's wave path) and, in the LAST row of every array, one covering more than
32 tiles (the binning's wave path)."""
import types

import pytest
import torch

from tests import parity_util as pu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 96, 128
SIZES = [1, 63, 256, 257, 700]
NAMES = ("xyz", "f_dc", "opacity", "scaling", "rotation")
LRS = dict(xyz=1.6e-4, f_dc=2.5e-3, opacity=5e-2, scaling=1e-3, rotation=1e-3)
GUARD_WORDS = 64                 # on each side; a multiple of 4, so that word GUARD_WORDS + 1 of a (256-byte aligned) allocation is 4 bytes past a 16-byte boundary
GUARD_BITS = 0x7FC0DEAD          # (a NaN pattern: compared as integers)


def _quat_R(q):
    w, x, y, z = (q / q.norm()).tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


_SCENES = {}


def _scene(P):
    """(cfg, GaussianModel, Renderer, pose, gt colour, gt depth, ids of the special Gaussians) -- built once per size, never modified (the
    tests run the kernels on guarded COPIES of the model's arrays)."""
    if P in _SCENES:
        return _SCENES[P]
    from mm3dgs_slam_amd import synthetic as syn
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.gaussian_model import GaussianModel
    from mm3dgs_slam_amd.renderer import Renderer
    cfg = default_config(device=DEV, height=H, width=W)
    c = cfg["cam"]
    color, depth = syn.rgbd_frame(H, W, seed=P)
    G = syn.seed_gaussians(color, depth, c["fx"], c["fy"], c["cx"], c["cy"], P, seed=P, isotropic=False)
    gen = torch.Generator().manual_seed(P)
    G["scaling"] = G["scaling"] + torch.tensor([1.2, -0.8, 0.0])
    opacity = torch.randn(P, 1, generator=gen) * 1.5
    rotation = G["rotation"] * (0.5 + torch.rand(P, 1, generator=gen))
    pose = torch.tensor([0.995, 0.03, -0.02, 0.04, 0.03, -0.02, 0.05]) * 1.3       # (an unnormalised quaternion)
    pose[4:] /= 1.3
    ids = {}
    if P < 63:
        # (a lone Gaussian: large and opaque enough to be seen by the tracking loss' presence mask)
        G["scaling"] = G["scaling"] + 1.0
        opacity[:] = 2.0
    if P >= 63:
        Rm, t = _quat_R(pose[:4]), pose[4:]
        fx, fy, cx, cy = c["fx"], c["fy"], c["cx"], c["cy"]

        def place(i, px, py, z, sigma_px):
            # camera-space mean that projects to pixel (px, py) at depth z, as a world mean (p = R x + t); a sphere of sigma_px pixels
            p = torch.tensor([(px - cx) / fx * z, (py - cy) / fy * z, z])
            G["xyz"][i] = Rm.T @ (p - t)
            G["scaling"][i] = torch.log(torch.tensor(sigma_px * z / fx)).expand(3)
            rotation[i] = torch.tensor([1.0, 0.0, 0.0, 0.0])
            opacity[i] = -1.0
        ids = dict(behind=0, off=1, wave=P // 2, huge=P - 1)
        place(0, 64.0, 48.0, 0.1, 0.5)             # behind the near plane (camera z 0.1 < 0.2)
        place(1, 128.0 + 60 * fx / 2.0, 48.0, 2.0, 1.0)      # 60 m to the right at 2 m: its tile rectangle is empty, radii == 0
        # radius ceil(3 sqrt(sigma^2 + 0.3)) = 31 about (70, 50): tiles x 2 .. 6, y 1 .. 4 or 5 -> 20 or 25 tiles (29 <= radius <= 34 keeps it within 17 .. 32)
        place(P // 2, 70.0, 50.0, 2.0, 10.2)
        place(P - 1, 64.0, 48.0, 2.0, 20.0)        # radius 61 about the centre: all 48 tiles
    g = GaussianModel(cfg)
    g.training_setup()
    g.densification_postfix(G["xyz"].to(DEV), G["f_dc"].to(DEV), torch.zeros(P, 0, 3, device=DEV), opacity.to(DEV), G["scaling"].to(DEV),
                            rotation.to(DEV), G["rgb"].to(DEV))
    _SCENES[P] = (cfg, g, Renderer(cfg), pose.to(DEV).contiguous(), color.to(DEV), depth.to(DEV), ids)
    return _SCENES[P]


class _Guarded:
    """A float array as a slice of a larger buffer that starts 4 bytes past a 16-byte boundary, guard words on both sides."""

    def __init__(self, src):
        n = src.numel()
        self.buf = torch.empty(GUARD_WORDS + 1 + n + GUARD_WORDS + 3, dtype=torch.int32, device=DEV).fill_(GUARD_BITS)
        self.t = self.buf.view(torch.float32)[GUARD_WORDS + 1:GUARD_WORDS + 1 + n].view(src.shape)
        self.t.copy_(src)
        assert self.t.data_ptr() % 16 == 4 and self.t.is_contiguous()
        self.n = n

    def intact(self):
        lo, hi = self.buf[:GUARD_WORDS + 1], self.buf[GUARD_WORDS + 1 + self.n:]
        return bool((lo == GUARD_BITS).all()) and bool((hi == GUARD_BITS).all())


def _guarded_map(g, gen, zero_moments):
    """Guarded copies of the model's five parameter arrays and their Adam moments; (model stand-in for FusedEngine, Mm3dgsMapAdam, the arrays)."""
    from mm3dgs_slam_amd import _lib
    prm = dict(zip(NAMES, (g._xyz, g._features_dc, g._opacity, g._scaling, g._rotation)))
    arr = {}
    ma = _lib.Mm3dgsMapAdam()
    for i, n in enumerate(NAMES):
        p = prm[n].detach()
        m0 = torch.zeros_like(p) if zero_moments else torch.randn(p.shape, device=DEV, generator=gen) * 1e-3
        v0 = torch.zeros_like(p) if zero_moments else torch.rand(p.shape, device=DEV, generator=gen) * 1e-6
        arr[n] = (_Guarded(p), _Guarded(m0), _Guarded(v0))
        ma.param[i], ma.exp_avg[i], ma.exp_avg_sq[i], ma.lr[i] = arr[n][0].t.data_ptr(), arr[n][1].t.data_ptr(), arr[n][2].t.data_ptr(), LRS[n]
    ma.beta1, ma.beta2, ma.eps, ma.step = 0.9, 0.999, 1e-15, 1
    P = int(g._xyz.shape[0])
    gs = types.SimpleNamespace(_xyz=arr["xyz"][0].t, _features_dc=arr["f_dc"][0].t, _opacity=arr["opacity"][0].t, _scaling=arr["scaling"][0].t,
                               _rotation=arr["rotation"][0].t, _features_rest=torch.zeros(P, 0, 3, device=DEV), active_sh_degree=0)
    return gs, ma, arr


def _guarded_stats(P, gen):
    # (small against the gradient norms they accumulate: the increment read back as new - old is then exact to ~1e-9)
    return tuple(_Guarded(0.01 + 0.01 * torch.rand(shape, device=DEV, generator=gen)) for shape in ((P,), (P, 1), (P, 1)))


def _check_specials(radii, ids):
    if not ids:
        return
    r = radii.cpu()
    assert int(r[ids["behind"]]) == 0 and int(r[ids["off"]]) == 0
    assert 29 <= int(r[ids["wave"]]) <= 34, int(r[ids["wave"]])
    assert int(r[ids["huge"]]) >= 50, int(r[ids["huge"]])


# twice the deviation measured on the parent commit's kernels at these scenes (the largest of the five sizes; see the docstring below)
GRAD_ACCUM_TOL = 2 * 3.23e-6


@pytest.mark.parametrize("P", SIZES)
def test_state_and_statistics_between_guard_words(P):
    """One mm3dgs_slam_backward with the in-kernel Adam and the densification statistics, every parameter, moment and statistic array a
    guarded slice 4 bytes past a 16-byte boundary: the guard words stay intact (a 16-byte store on the last row of a [P, 3] array would
    reach into them), a Gaussian with radii == 0 keeps its three statistics bit for bit, a visible one has denom + 1 and
    max(old, radii) exactly, and its grad_accum grows by the screen-space gradient norm of the torch-graph Renderer path on the same scene
    and dL.  That last bound is twice the deviation of the parent commit's kernels at these scenes, measured once on MI355X as
    rel_l2(increment, reference) per size: P = 1: 1.85e-7, 63: 2.35e-6, 256: 2.47e-6, 257: 3.23e-6, 700: 2.25e-6 (this commit's kernels give
    the same five figures: the arithmetic is unchanged)."""
    from mm3dgs_slam_amd.fused import FusedEngine
    cfg, g, R, pose, color, depth, ids = _scene(P)
    gen = torch.Generator(device=DEV).manual_seed(100 + P)
    gs, ma, arr = _guarded_map(g, gen, zero_moments=False)
    stats = _guarded_stats(P, gen)
    old = [s.t.clone() for s in stats]
    w = torch.randn(6, H, W, device=DEV, generator=gen)
    # reference: the torch graph over the generic rasterizer
    p = pose.clone().requires_grad_(True)
    res = R.render(g, p)
    (torch.cat([res["render"], res["depth"]], 0) * w).sum().backward()
    vis = res["visibility_filter"]
    gn = torch.norm(res["viewspace_points"].grad[:, :2], dim=-1) * vis
    for prm in (g._xyz, g._features_dc, g._opacity, g._scaling, g._rotation):
        prm.grad = None
    eng = FusedEngine(R)
    with torch.no_grad():
        si = eng.forward(pose, gs, need_grads=True)
        eng.dL.copy_(w)
        eng.backward(si, map_adam=ma, stats=tuple(s.t for s in stats))
        torch.cuda.synchronize()
    radii = eng.radii.clone()
    assert torch.equal(radii, res["radii"])
    _check_specials(radii, ids)
    for n in NAMES:
        for a in arr[n]:
            assert a.intact(), n
    for s in stats:
        assert s.intact()
    seen = radii > 0
    assert bool(seen.any())
    new = [s.t for s in stats]
    for o, s in zip(old, new):
        assert torch.equal(o.reshape(-1)[~seen], s.reshape(-1)[~seen])
    assert torch.equal(new[2][:, 0][seen], old[2][:, 0][seen] + 1.0)
    assert torch.equal(new[0][seen], torch.maximum(old[0], radii.float())[seen])
    inc = (new[1][:, 0] - old[1][:, 0])[seen]
    dev = pu.rel_l2(inc, gn[seen])
    print(f"grad_accum increment vs torch graph, P = {P}: rel_l2 {dev:.3e} (bound {GRAD_ACCUM_TOL:.1e})")
    assert dev <= GRAD_ACCUM_TOL, dev
    # the step moved something, and nothing it wrote is broken
    assert not torch.equal(arr["xyz"][0].t, g._xyz.detach())
    assert all(bool(torch.isfinite(a.t).all()) for n in NAMES for a in arr[n])
    assert eng.check_capacity()


@pytest.mark.parametrize("P", SIZES)
def test_in_kernel_adam_with_opt_mask_equals_gradient_output_plus_torch_adam(P):
    """mm3dgs_slam_backward with `map_adam` against the same kernel's gradient outputs fed to torch.optim.Adam(eps=1e-15), three consecutive
    steps on guarded arrays, opt_mask zero on a third of the Gaussians (their gradient is zero): parameters and both moments to 1e-6
    relative (the bounds of test_in_kernel_map_adam_equals_gradient_output_plus_torch_adam); the masked Gaussians, which start from zero
    moments, keep parameters and moments bit for bit."""
    from mm3dgs_slam_amd.fused import FusedEngine
    cfg, g, R, pose, color, depth, ids = _scene(P)
    gen = torch.Generator(device=DEV).manual_seed(200 + P)
    gs, ma, arr = _guarded_map(g, gen, zero_moments=True)
    mask = (torch.arange(P, device=DEV) % 3 != 1).to(torch.uint8).contiguous()       # (P = 1: its one Gaussian may move)
    ma.opt_mask = mask.data_ptr()
    keep = mask.bool()
    start = {n: arr[n][0].t.clone() for n in NAMES}
    ref_params = {n: arr[n][0].t.clone().requires_grad_(True) for n in NAMES}
    opt = torch.optim.Adam([{"params": [ref_params[n]], "lr": LRS[n]} for n in NAMES], lr=0.0, eps=1e-15)
    eng = FusedEngine(R)
    with torch.no_grad():
        for step in range(1, 4):
            si = eng.forward(pose, gs, need_grads=True)
            if step == 1:
                _check_specials(eng.radii, ids)
            eng.dL.copy_(torch.randn(6, H, W, device=DEV, generator=gen))
            eng.backward(si, grads=eng.grads)
            for n in NAMES:
                gr = eng.grads[n].reshape(ref_params[n].shape).clone()
                gr[~keep] = 0.0
                ref_params[n].grad = gr
            ma.step = step
            eng.backward(si, map_adam=ma)
            opt.step()
            torch.cuda.synchronize()
            for n in NAMES:
                prm, m_, v_ = (a.t for a in arr[n])
                s_ref = opt.state[ref_params[n]]
                assert pu.rel_l2(prm, ref_params[n]) <= 1e-6, (n, step, "param")
                assert pu.rel_l2(m_, s_ref["exp_avg"]) <= 1e-6, (n, step, "exp_avg")
                assert pu.rel_l2(v_, s_ref["exp_avg_sq"]) <= 1e-6, (n, step, "exp_avg_sq")
                assert (prm - ref_params[n]).abs().max() <= 2e-6 * max(1.0, float(ref_params[n].abs().max())) + 1e-3 * LRS[n], (n, step)
    for n in NAMES:
        prm, m_, v_ = arr[n]
        assert prm.intact() and m_.intact() and v_.intact(), n
        assert torch.equal(prm.t[~keep], start[n][~keep]), n
        assert not bool(m_.t[~keep].any()) and not bool(v_.t[~keep].any()), n
    assert not torch.equal(arr["xyz"][0].t[keep], start["xyz"][keep])
    assert eng.check_capacity()


@pytest.mark.parametrize("P", SIZES)
def test_mapping_and_tracking_loops_are_bit_identical_across_the_fused_launch(P, monkeypatch):
    """Six mapping iterations with statistics through mm3dgs_slam_map -- slam_bwd_project_kernel: the backward body and the next view's
    projection in one launch -- then five tracking iterations on the map they leave (slam_project_bin_kernel), against the same loops with
    MM3DGS_NO_FUSED_PROJECT=1 (slam_preprocess_bwd_kernel and slam_project_bin_kernel as separate launches): parameters, moments,
    statistics and the tracked pose bit for bit.  The two instances are held to each other here, the shared body to independent
    references above."""
    from mm3dgs_slam_amd import _lib
    from mm3dgs_slam_amd.fused import FusedEngine, _loss_cfg
    cfg, g, R, pose, color, depth, ids = _scene(P)
    with torch.no_grad():
        r0 = R.render(g, pose)
        gt, ref = r0["render"].contiguous(), r0["depth"][0].contiguous()
    d1 = torch.tensor([0.0, 0.002, -0.001, 0.001, 0.01, -0.005, 0.004], device=DEV)
    views_poses = [(pose + d1).contiguous(), (pose - 0.5 * d1).contiguous()]

    def run(flag):
        monkeypatch.setenv("MM3DGS_NO_FUSED_PROJECT", flag)
        gen = torch.Generator(device=DEV).manual_seed(300 + P)
        gs, ma, arr = _guarded_map(g, gen, zero_moments=False)
        stats = _guarded_stats(P, gen)
        eng = FusedEngine(R)
        with torch.no_grad():
            eng.forward(pose, gs)
            assert eng.check_capacity()      # (the list lengths are known from here on: direct bins, the fused launch's condition)
            _check_specials(eng.radii, ids)
            views = [(views_poses[k % 2], gt, ref) for k in range(6)]
            eng.map_loop(views, gs, _loss_cfg(H, W, 0.8, 0.2, 0.05, 0, 2, 0, 0.5), tuple(s.t for s in stats), ma)
            assert eng.direct
            tp = (pose + 2.0 * d1).contiguous()
            m, v = torch.zeros(7, device=DEV), torch.zeros(7, device=DEV)
            step = torch.zeros(1, dtype=torch.int32, device=DEV)
            ad = _lib.Mm3dgsPoseAdam()
            ad.pose, ad.m, ad.v, ad.step = tp.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr()
            ad.lr_q, ad.lr_t, ad.beta1, ad.beta2, ad.eps = 0.002, 0.002, 0.9, 0.999, 1e-8
            # (presence mask at silhouette > 0.05: these sparse maps have no pixel above the shipped 0.99, and a loss over no pixel moves no pose)
            eng.track_loop(5, tp, gs, _loss_cfg(H, W, 1.0, 0.0, 0.0, 1, 0, 1, 0.05), gt, None, ad)
            torch.cuda.synchronize()
        assert int(step) == 5
        assert eng.check_capacity()
        guards = [a for n in NAMES for a in arr[n]] + list(stats)
        assert all(a.intact() for a in guards)
        return [a.t.clone() for a in guards] + [tp.clone(), m.clone(), v.clone()]

    a, b = run("1"), run("0")
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (i, float((x - y).abs().max()))
    # (and the loops did move the map, the statistics and the pose)
    assert not torch.equal(a[0], g._xyz.detach()) and bool((a[-4] > 1.0).any()) and not torch.equal(a[-3], (pose + 2.0 * d1))
