"""Native loops at an ACTIVE SH degree with the two viewing-direction sources besides the shipped one (ABI 211, Mm3dgsSlamInputs.sh_dir;
slam/renderer.py:117-124,179-193):

  mode A  transform_means_python: true, convert_SHs_python: true   d = x / |x|              (world mean about the origin: camera_pos = 0)
  mode B  transform_means_python: false, either SH flag            d = (x - c) / |x - c|    (c = w2c^-1[3, :3], the camera centre)

Held to the torch-graph renderer over the generic HIP rasterizer, to the float64 oracle, to the torch-graph loops and to the reference's own
classes (fixtures g9_ / g9L_sh2_python_active, no_transform_sh_active), like tests/test_gpu_sh_native.py holds mode 0."""
import random

import numpy as np
import pytest
import torch

from tests import parity_util as pu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = {"A": dict(transform_means_python=True, convert_SHs_python=True),
         "B": dict(transform_means_python=False, convert_SHs_python=False),
         "B_python_sh": dict(transform_means_python=False, convert_SHs_python=True)}


def _setup(mode, deg, P=20000, H=240, W=320, seed=0, max_deg=3):
    """tests/test_gpu_sh_native.py's map (f_rest rows, active degree raised like load_ply leaves it) under the mode's pipeline flags."""
    from mm3dgs_slam_amd import synthetic as syn
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.gaussian_model import GaussianModel
    from mm3dgs_slam_amd.renderer import Renderer
    pipe = dict(MODES[mode]) if isinstance(mode, str) else dict(mode)
    cfg = default_config(device=DEV, height=H, width=W, pipeline=pipe, mapping={"sh_degree": max_deg})
    c = cfg["cam"]
    color, depth = syn.rgbd_frame(H, W, seed=seed)
    G = syn.seed_gaussians(color, depth, c["fx"], c["fy"], c["cx"], c["cy"], P, seed=seed, isotropic=False)
    g = GaussianModel(cfg)
    g.training_setup()
    gen = torch.Generator().manual_seed(seed + 11)
    n_rest = (max_deg + 1) ** 2 - 1
    G["scaling"] = G["scaling"] + torch.tensor([0.6, -0.4, 0.0])
    g.densification_postfix(G["xyz"].to(DEV), G["f_dc"].to(DEV), (0.25 * torch.randn(P, n_rest, 3, generator=gen)).to(DEV),
                            (torch.randn(P, 1, generator=gen) * 1.2).to(DEV), G["scaling"].to(DEV),
                            (G["rotation"] * (0.5 + torch.rand(P, 1, generator=gen))).to(DEV), G["rgb"].to(DEV))
    g.active_sh_degree = deg
    pose = torch.tensor([0.995, 0.03, -0.02, 0.04, 0.03, -0.02, 0.05], device=DEV) * 1.3
    pose[4:] /= 1.3
    return cfg, g, Renderer(cfg), pose


def _torch_render(R, g, pose, w, detach_centre=False):
    """The torch-graph render's 6 channels and dL/dpose for the weight image w (optionally with the camera centre detached)."""
    p = pose.clone().requires_grad_(True)
    inv = torch.linalg.inv
    if detach_centre:
        torch.linalg.inv = lambda m: inv(m).detach()
    try:
        res = R.render(g, p)
    finally:
        torch.linalg.inv = inv
    out = torch.cat([res["render"], res["depth"]], 0)
    (out * w).sum().backward()
    return out.detach(), p.grad.detach().clone(), res["radii"]


PARAMS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"), ("scaling", "_scaling"), ("rotation", "_rotation"))


@pytest.mark.parametrize("deg", [1, 2, 3])
@pytest.mark.parametrize("mode", list(MODES))
def test_native_forward_and_backward_match_the_torch_graph(mode, deg):
    from mm3dgs_slam_amd.fused import FusedEngine
    from mm3dgs_slam_amd.renderer import Renderer
    cfg, g, R, pose = _setup(mode, deg)
    assert FusedEngine.eligible(cfg, g)
    eng = FusedEngine(R)
    w = torch.randn(6, eng.H, eng.W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    for direct in (False, True):      # first render: packed bins; second: direct bins
        si = eng.forward(pose, g, need_grads=True)
        assert eng.check_capacity() and eng.direct == direct
        assert si.sh_dir == (1 if mode == "A" else 2)
        for prm in (getattr(g, k) for _, k in PARAMS):
            prm.grad = None
        ref, dpose_ref, radii = _torch_render(R, g, pose, w)
        assert pu.rel_l2(eng.out, ref) < 1e-5
        assert torch.equal(eng.radii, radii)
        eng.dL.copy_(w)
        eng.backward(si, grads=eng.grads, dpose=eng.dpose)
        torch.cuda.synchronize()
        tol = 2e-3
        m = {"d_pose": pu.rel_l2(eng.dpose, dpose_ref), **{n: pu.rel_l2(eng.grads[n], getattr(g, k).grad) for n, k in PARAMS}}
        print(mode, deg, direct, {k: f"{v:.1e}" for k, v in m.items()}, flush=True)
        assert m["d_pose"] < tol, (eng.dpose, dpose_ref)
        for name, _ in PARAMS:
            assert m[name] < (5e-3 if name == "rotation" else tol), (name, m)
        nb = (deg + 1) ** 2 - 1
        assert float(eng.grads["f_rest"][:, :nb].abs().max()) > 0
        if nb < eng.grads["f_rest"].shape[1]:
            assert float(eng.grads["f_rest"][:, nb:].abs().max()) == 0.0
    for prm in (getattr(g, k) for _, k in PARAMS):
        prm.grad = None
    if mode != "A":
        # the camera centre's pose terms matter: autograd's pose gradient without them moves by more than twice the native path's distance from
        # the full one.  (In this scene the centre term is a small share of dL/dpose -- the means' screen positions dominate it: measured 1.7e-4 /
        # 1.1e-4 / 7.3e-4 relative at degrees 1 / 2 / 3, against 3.6e-5 / 4.1e-5 / 4.3e-5 native-to-autograd -- so it cannot clear 10x the 2e-3 bar.)
        _, dpose_detached, _ = _torch_render(R, g, pose, w, detach_centre=True)
        gap, err = pu.rel_l2(dpose_detached, dpose_ref), pu.rel_l2(eng.dpose, dpose_ref)
        print(mode, deg, "centre term", f"{gap:.1e}", "native error", f"{err:.1e}", flush=True)
        assert gap > 2 * err, (gap, err)
    else:
        # the test tells the direction sources apart: mode 0's camera-space direction renders a different image
        R0 = Renderer(dict(cfg, pipeline=dict(cfg["pipeline"], convert_SHs_python=False)))
        with torch.no_grad():
            r0 = R0.render(g, pose)
        gap = pu.rel_l2(torch.cat([r0["render"], r0["depth"]], 0), ref)
        print(mode, deg, "mode-0 image gap", f"{gap:.1e}", flush=True)
        assert gap > 10 * 1e-5, gap
    for prm in (getattr(g, k) for _, k in PARAMS):
        prm.grad = None


@pytest.mark.parametrize("mode", ["A", "B"])
def test_native_path_at_sh_degree_two_matches_the_float64_oracle(mode):
    import copy
    import mm3dgs_slam_amd.pose_utils as P_
    import mm3dgs_slam_amd.renderer as rmod
    from mm3dgs_slam_amd.fused import FusedEngine
    from mm3dgs_slam_amd.renderer import Renderer
    from oracle.raster_ref import RefRasterizer
    deg = 2
    cfg, g, R, pose = _setup(mode, deg, P=3000, H=120, W=160, seed=3, max_deg=2)
    eng = FusedEngine(R)
    eng.forward(pose, g, need_grads=True)
    assert eng.check_capacity()
    si = eng.forward(pose, g, need_grads=True)
    assert eng.direct
    keys = [k for _, k in PARAMS]
    ccfg = copy.deepcopy(cfg)
    ccfg["device"] = "cpu"
    w6 = torch.randn(6, eng.H, eng.W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).double().cpu()

    class PC:
        active_sh_degree = deg
        max_sh_degree = 2
    pc = PC()
    leaf = {k: getattr(g, k).detach().double().cpu().requires_grad_(True) for k in keys}
    pc._xyz, pc._scaling, pc._rotation = leaf["_xyz"], leaf["_scaling"], leaf["_rotation"]
    pc.get_xyz, pc.get_opacity, pc.get_scaling = leaf["_xyz"], torch.sigmoid(leaf["_opacity"]), torch.exp(leaf["_scaling"])
    pc.get_rotation, pc.get_features = torch.nn.functional.normalize(leaf["_rotation"]), torch.cat([leaf["_features_dc"], leaf["_features_rest"]], 1)
    Rc = Renderer(ccfg, rasterizer_cls=RefRasterizer)
    Rc.projection_matrix, Rc.background, Rc._eye = Rc.projection_matrix.double(), Rc.background.double(), Rc._eye.double()
    orig = rmod.get_camera_from_tensor

    def cam(t):
        return torch.cat([torch.cat([P_.quad2rotation(t[None, :4])[0], t[4:7, None]], 1), torch.tensor([[0.0, 0, 0, 1]], dtype=t.dtype)], 0)
    rmod.get_camera_from_tensor = cam
    try:
        p_ = pose.detach().double().cpu().requires_grad_(True)
        r_ = Rc.render(pc, p_)
        ref = torch.cat([r_["render"], r_["depth"]], 0)
        (ref * w6).sum().backward()
    finally:
        rmod.get_camera_from_tensor = orig
    eng.dL.copy_(w6.float().to(DEV))
    eng.backward(si, grads=eng.grads, dpose=eng.dpose)
    torch.cuda.synchronize()
    m = {"img": pu.rel_l2(eng.out, ref.detach()), "d_pose": pu.rel_l2(eng.dpose, p_.grad)}
    for name, key in PARAMS:
        m["d_" + name] = pu.rel_l2(eng.grads[name], leaf[key].grad)
    print(mode, {k: f"{v:.2e}" for k, v in m.items()}, flush=True)
    assert m["img"] <= pu.IMG_TOL, m
    assert m["d_pose"] <= 1e-5, m
    for k, v in m.items():
        if k.startswith("d_") and k != "d_pose":
            assert v <= pu.GRAD_TOL, (k, m)


@pytest.mark.parametrize("mode,ba", [("A", False), ("B", False), ("B_python_sh", False), ("B", True)])
def test_native_loops_follow_the_torch_graph_loops(mode, ba):
    """Three SLAM frames at active degree 2, native against torch-graph loops, at the bars of tests/test_gpu_sh_native.py (mode B with bundle
    adjustment too: the per-view camera-centre pose gradient through the in-kernel BA step)."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.fused import FusedEngine
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    results = {}
    for native in (False, True):
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        cfg = default_config(device=DEV, height=240, width=320, pipeline=dict(MODES[mode]), tracking={"iters": 40},
                             mapping={"iters": 12, "sh_degree": 2, **({"do_BA": True} if ba else {})})
        seq = SyntheticSequence(cfg, 3, 30000, seed=4)
        slam = SLAM(cfg, seq, native_loops=native)
        slam.gaussians.active_sh_degree = 2
        random.seed(1)
        for i in range(3):
            slam.step(i)
        if native:
            assert FusedEngine.eligible(cfg, slam.gaussians) and slam.tracker.tracking_iter_count > 0
        results[native] = (torch.stack(slam.estimate_pose_list[:3]).cpu(), slam.gaussians._xyz.detach().cpu(), slam.gaussians._opacity.detach().cpu(),
                           slam.gaussians._features_rest.detach().cpu(), slam.pose_errors())
    a, b = results[False], results[True]
    print(mode, ba, float((a[0] - b[0]).abs().max()), pu.rel_l2(b[1], a[1]) if a[1].shape == b[1].shape else None, b[4], flush=True)
    if ba:
        # (bundle adjustment: the raw quaternions' norm has no gradient and drifts under both optimisers -- 9e-3 in w at frame 2, 1e-3 in the
        #  direction -- so compare the camera matrices, as tests/test_golden_slam.py does)
        from mm3dgs_slam_amd.pose_utils import get_camera_from_tensor as M
        dM = max(float((M(a[0][i]) - M(b[0][i])).abs().max()) for i in range(3))
        print(mode, ba, "camera matrices", f"{dM:.1e}", flush=True)
        assert dM < 4e-3, dM
    else:
        assert (a[0] - b[0]).abs().max() < 4e-3, (a[0], b[0])
    assert a[1].shape == b[1].shape
    assert pu.rel_l2(b[1], a[1]) < 1e-3 and (a[2] - b[2]).abs().median() < 5e-2
    assert float(b[3].abs().max()) > 0 and abs(float(a[3].abs().mean()) - float(b[3].abs().mean())) < 0.1 * float(a[3].abs().mean()) + 1e-6
    assert b[4][1] < 0.01 and b[4][2] < 0.01, b[4]


# Per-frame bars of the new G9 variants (camera-matrix difference, largest moment difference), 3x what the native loops measured against the
# reference's own classes, capped at tests/test_gpu_golden_slam.py's global bars (camera 5e-3 at 160x120 / 1e-3 at 64x48 once the rows
# differ, moments 1e-2 / 5e-3).  A table of its own: the existing tables are not touched.
SH_MODES_MEASURED = {      # one measurement on an MI355X (floors 1e-6 / 1e-5, as tests/test_gpu_golden_slam.py's g9L bars)
    ("g9", "sh2_python_active"): [(9.31e-10, 1.55e-06), (8.85e-09, 6.11e-07), (5.26e-08, 2.38e-07)],
    ("g9", "no_transform_sh_active"): [(9.31e-10, 1.25e-06), (1.43e-08, 5.96e-07), (4.25e-08, 2.21e-06)],
    ("g9L", "sh2_python_active"): [(9.31e-10, 1.53e-06), (2.77e-06, 7.15e-07), (2.72e-05, 2.09e-04), (2.15e-05, 3.29e-04)],
    ("g9L", "no_transform_sh_active"): [(9.31e-10, 1.07e-04), (3.07e-05, 1.10e-04), (1.24e-04, 5.02e-04), (1.06e-04, 3.48e-04)],
}


def _bars(prefix, variant, idx):
    cap = (5e-3, 1e-2) if prefix == "g9L" else (1e-3, 5e-3)
    pose, mom = SH_MODES_MEASURED[(prefix, variant)][idx]
    return min(max(3.0 * pose, 1e-6), cap[0]), min(max(3.0 * mom, 1e-5), cap[1])


@pytest.mark.parametrize("prefix", ["g9", "g9L"])
@pytest.mark.parametrize("variant", ["sh2_python_active", "no_transform_sh_active"])
def test_native_hip_loops_reproduce_the_new_fixtures(variant, prefix):
    from mm3dgs_slam_amd.pose_utils import get_camera_from_tensor
    from tests import g9_util
    from tests.test_gpu_golden_slam import run_variant
    slam, G, rows = run_variant(variant, prefix=prefix)
    want_kf = [[int(v) for v in s.split(",")] for s in G["keyframes"]]
    print(variant, prefix, [(f"{r['pose_diff']:.2e}", f"{float(np.abs(r['moments'] - r['moments_ref']).max()):.2e}", r["P"] - r["P_ref"]) for r in rows], flush=True)
    for r in rows:
        idx = r["idx"]
        assert r["keyframes"] == want_kf[idx], (idx, r["keyframes"], want_kf[idx])
        assert abs(r["P"] - r["P_ref"]) <= max(2, 0.005 * r["P_ref"]), (idx, r["P"], r["P_ref"])
        pose_bar, mom_bar = _bars(prefix, variant, idx)
        assert r["pose_diff"] < pose_bar, (idx, r["pose_diff"], pose_bar)
        assert float(np.abs(r["moments"] - r["moments_ref"]).max()) <= mom_bar, (idx, r["moments"], r["moments_ref"])
    graph = [",".join(map(str, sorted(slam.mapper.covisibility_graph[k]))) for k in range(len(slam.mapper.keyframes))]
    assert graph == [str(s) for s in G["graph"]]
    for kf, ref in zip(slam.mapper.keyframes, G["keyframe_poses"]):
        d = (get_camera_from_tensor(kf.pose.detach().cpu().float()) - get_camera_from_tensor(torch.from_numpy(ref))).abs().max()
        assert d < (5e-3 if prefix == "g9L" else 5e-4), (kf.idx, float(d))
    g = slam.gaussians
    for name, t in (("xyz", g._xyz), ("opacity", g._opacity), ("scaling", g._scaling), ("rotation", g._rotation), ("f_dc", g._features_dc)):
        got, ref = g9_util.final_quantiles(G, name, t)
        for col in range(got.shape[1]):
            a, b = got[:, col], ref[:, col]
            assert (a - b).abs().max() < 0.02 * max(1.0, float(b.abs().max())), (name, col, a, b)
    after = np.array([random.random(), float(np.random.rand()), float(torch.rand(1))])
    assert np.allclose(after, G["rng_after"]), (after, G["rng_after"])


def test_degree_zero_ignores_the_direction_source_and_bad_combinations_are_refused():
    from mm3dgs_slam_amd.fused import FusedEngine
    outs = []
    for world in (False, True):
        cfg, g, R, pose = _setup({"transform_means_python": not world}, 0, P=6000, H=120, W=160, seed=2, max_deg=2)
        eng = FusedEngine(R)
        base = eng.inputs
        w = torch.randn(6, eng.H, eng.W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
        ref = None
        for d in (0, 1, 2):
            def inputs(pose_, g_, d=d):
                si = base(pose_, g_)
                si.sh_dir = d
                return si
            eng.inputs = inputs
            si = eng.forward(pose, g, need_grads=True)
            assert eng.check_capacity()
            si = eng.forward(pose, g, need_grads=True)
            eng.dL.copy_(w)
            eng.backward(si, grads=eng.grads, dpose=eng.dpose)
            torch.cuda.synchronize()
            got = [eng.out.clone(), eng.radii.clone(), eng.dpose.clone()] + [eng.grads[n].clone() for n in ("xyz", "f_dc", "opacity", "scaling", "rotation")]
            if ref is None:
                ref = got
            else:
                assert all(torch.equal(a, b) for a, b in zip(got, ref)), (world, d)
        outs.append(ref[0])
        # at an active degree the direction source must match the means' frame
        g.active_sh_degree = 2
        for d in ((0, 1) if world else (2,)):
            def inputs(pose_, g_, d=d):
                si = base(pose_, g_)
                si.sh_dir = d
                return si
            eng.inputs = inputs
            with pytest.raises(RuntimeError, match="mm3dgs error -2: " + ("world_means = 1 needs sh_dir = 2" if world else r"sh_dir = 2 \(direction from the camera centre\) needs world_means = 1")):
                eng.forward(pose, g, need_grads=True)
        eng.inputs = base
        eng.forward(pose, g, need_grads=True)        # the matching source is accepted
        torch.cuda.synchronize()
    assert not torch.equal(outs[0], outs[1])
