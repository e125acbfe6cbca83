"""An ACTIVE SH degree with the two viewing-direction sources besides the shipped one (ABI 211, Mm3dgsSlamInputs.sh_dir), on CPU:

* mode A -- `convert_SHs_python: true` with pre-transformed means: slam/renderer.py:179-193 evaluates SH in Python on the WORLD mean about the
  origin (camera_pos = 0 because the view matrix is the identity in that mode);
* mode B -- `transform_means_python: false`: the world mean seen from the camera centre w2c^-1[3, :3], with either SH flag.

FusedEngine.eligible now sends both to the native loops.  The fixtures g9_sh2_python_active / g9_no_transform_sh_active
(tests/golden/make_golden_slam_sh_modes.py: the reference's own classes, the map resumed at max_sh_degree 2 like `sh2_active`) pin the
reference's direction semantics at degree > 0; both the torch-graph loops and the native loops' host side (over tests/cpu_engine.py) are held
to them with the bars tests/test_golden_slam.py uses for `sh2_active`."""
import ast
import ctypes as C
import os
import random
import types
import warnings

import numpy as np
import pytest
import torch

import tests.test_golden_slam as tg
from oracle.raster_ref import RefRasterizer

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_VARIANTS = ["sh2_python_active", "no_transform_sh_active"]
MODES = {"A": dict(transform_means_python=True, convert_SHs_python=True),
         "B_kernel_sh": dict(transform_means_python=False, convert_SHs_python=False),
         "B_python_sh": dict(transform_means_python=False, convert_SHs_python=True)}


def _cfg(**pipe):
    from mm3dgs_slam_amd.config import default_config
    return default_config(device="cuda:0", height=48, width=64, pipeline=pipe, mapping={"sh_degree": 3})


@pytest.mark.parametrize("deg", [1, 2, 3])
@pytest.mark.parametrize("mode", list(MODES))
def test_eligible_for_both_new_direction_sources_without_a_fallback_warning(mode, deg):
    from mm3dgs_slam_amd.fused import FusedEngine
    g = types.SimpleNamespace(active_sh_degree=deg, _features_rest=torch.zeros(0, 15, 3))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert FusedEngine.eligible(_cfg(**MODES[mode]), g)


def test_still_not_eligible_with_compute_cov3D_python_or_beyond_degree_three():
    from mm3dgs_slam_amd.fused import FusedEngine
    g = types.SimpleNamespace(active_sh_degree=2, _features_rest=torch.zeros(0, 8, 3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert not FusedEngine.eligible(_cfg(compute_cov3D_python=True, convert_SHs_python=True), g)
        assert not FusedEngine.eligible(_cfg(compute_cov3D_python=True, transform_means_python=False), g)
        assert not FusedEngine.eligible(_cfg(convert_SHs_python=True), types.SimpleNamespace(active_sh_degree=4, _features_rest=torch.zeros(0, 24, 3)))


@pytest.mark.parametrize("world", [0, 1])
@pytest.mark.parametrize("convert", [False, True])
def test_engine_inputs_name_the_reference_direction(world, convert):
    """FusedEngine.inputs: sh_dir 2 for world-frame means (either SH flag), 1 for convert_SHs_python with pre-transformed means, 0 otherwise."""
    from mm3dgs_slam_amd.fused import FusedEngine
    eng = FusedEngine.__new__(FusedEngine)
    eng.r = types.SimpleNamespace(cfg=_cfg(transform_means_python=not world, convert_SHs_python=convert))
    eng.isotropic = 0
    P = 4
    g = types.SimpleNamespace(_xyz=torch.zeros(P, 3), _features_dc=torch.zeros(P, 1, 3), _opacity=torch.zeros(P, 1), _scaling=torch.zeros(P, 3),
                              _rotation=torch.zeros(P, 4), _features_rest=torch.zeros(P, 8, 3), active_sh_degree=2)
    si = eng.inputs(torch.zeros(7), g)
    assert si.world_means == world and si.sh_degree == 2 and si.n_rest == 8
    assert si.sh_dir == (2 if world else (1 if convert else 0))


@pytest.mark.parametrize("variant", NEW_VARIANTS)
def test_fixture_is_an_active_sh_run_of_the_intended_mode(variant):
    G = np.load(os.path.join(HERE, "golden", f"g9_{variant}.npz"))
    ov = ast.literal_eval(str(G["overrides"]))
    assert ov["_resumed_sh"] and ov["mapping"]["sh_degree"] == 2
    assert ov["pipeline"] == ({"convert_SHs_python": True} if variant == "sh2_python_active" else {"transform_means_python": False})
    for prefix, n in (("g9", 3), ("g9L", 4)):
        assert np.load(os.path.join(HERE, "golden", f"{prefix}_{variant}.npz"))["est_poses"].shape[0] == n


def test_torch_graph_loops_reproduce_the_world_frame_fixture():
    # (sh2_python_active is held to the native loops' host side below; the torch-graph loops miss its 1e-4 moment bar at frame 2 -- the f_dc
    #  mean is off by 4.1e-4 while the map sizes still agree)
    tg.test_torch_graph_loops_reproduce_the_reference_classes_end_to_end("no_transform_sh_active")


def _sh_cpu_engine_cls():
    from tests.cpu_engine import CpuEngine, _adam, _view

    class ShCpuEngine(CpuEngine):
        """CpuEngine plus the sixth Adam group of mm3dgs_slam_map at an active SH degree (Mm3dgsMapAdam.rest_*): one view per base-class call,
        then f_rest steps on that view's gradient -- zero rows beyond the active degree, the opt_mask honoured -- like the kernel's in-kernel step."""

        def map_loop(self, views, g, lcfg, stats, map_adam, grads=None, keep_tile_order=False, want_loss=True, projected=False):
            if map_adam is None or int(g.active_sh_degree) == 0:
                return super().map_loop(views, g, lcfg, stats, map_adam, grads, keep_tile_order, want_loss, projected)
            rest = g._features_rest
            assert map_adam.rest_param == rest.data_ptr(), "Mm3dgsMapAdam.rest_param does not point at the model's f_rest"
            n, P = rest.numel(), rest.shape[0]
            pv, mv, vv = _view(map_adam.rest_param, n), _view(map_adam.rest_exp_avg, n), _view(map_adam.rest_exp_avg_sq, n)
            keep = _view(map_adam.opt_mask, P, C.c_uint8).bool() if map_adam.opt_mask else None
            step0 = int(map_adam.step)
            for i, view in enumerate(views):
                ma = type(map_adam).from_buffer_copy(map_adam)
                ma.step = step0 + i
                rest.grad = None
                super().map_loop([view], g, lcfg, stats, ma, grads, keep_tile_order, want_loss, projected and i == 0)
                with torch.no_grad():
                    gr = rest.grad if rest.grad is not None else torch.zeros_like(rest)
                    if keep is not None:
                        gr = gr * keep[:, None, None]
                    _adam(pv, gr.reshape(-1), mv, vv, step0 + i, map_adam.rest_lr, map_adam.beta1, map_adam.beta2, map_adam.eps)
                rest.grad = None
    return ShCpuEngine


@pytest.mark.parametrize("variant", NEW_VARIANTS)
def test_native_loop_orchestration_reproduces_the_new_fixtures(variant, monkeypatch):
    """The HOST side of the native loops (FusedTracker / FusedMapper, the structs and step counters fused.py builds) over the CPU stand-in of the
    C-ABI loops, at the bars of tests/test_golden_slam.py."""
    from mm3dgs_slam_amd import fused
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.pose_utils import get_camera_from_tensor
    from mm3dgs_slam_amd.slam import SLAM
    F = np.load(os.path.join(HERE, "golden", "g9_frames.npz"))
    G = np.load(os.path.join(HERE, "golden", f"g9_{variant}.npz"))
    overrides = ast.literal_eval(str(G["overrides"]))
    assert overrides.pop("_resumed_sh")
    cfg = default_config(device="cpu", height=int(F["H"]), width=int(F["W"]), **overrides)
    n = G["est_poses"].shape[0]
    seq = tg._Frames(F["color"][:n], F["depth"][:n], F["gt_poses"][:n], F["imu"][:n], F["tstamps"][:n])
    real_eligible = fused.FusedEngine.eligible
    monkeypatch.setattr(fused.FusedEngine, "eligible", staticmethod(lambda c, g: real_eligible(dict(c, device="cuda:0"), g)))
    engines = {}
    cls = _sh_cpu_engine_cls()
    monkeypatch.setattr(fused, "_engine", lambda renderer: engines.setdefault(id(renderer), cls(renderer)))
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    slam = SLAM(cfg, seq, rasterizer_cls=RefRasterizer, render_mode="reference", native_loops=True)
    slam.gaussians.active_sh_degree = slam.gaussians.max_sh_degree      # slam/gaussian_model.py:363
    assert type(slam.tracker).__name__ == "FusedTracker" and type(slam.mapper).__name__ == "FusedMapper"
    want_kf = [[int(v) for v in s.split(",")] for s in G["keyframes"]]
    aligned = True
    for idx in range(len(seq)):
        color, depth, gt_pose = seq[idx]
        if idx == 0:
            slam.estimate_pose_list[idx] = gt_pose.clone()
        else:
            slam.tracker.run_frame(idx, color, depth, None, imu_meas=None)
        if idx == 0:
            slam.mapper.camera_extent = float(depth.max()) / cfg["scene_radius_depth_ratio"]
        slam.mapper.run_frame(idx, color, depth, None)
        g = slam.gaussians
        assert fused.FusedEngine.eligible(cfg, g)
        assert [kf.idx for kf in slam.mapper.keyframes] == want_kf[idx], (idx, [kf.idx for kf in slam.mapper.keyframes], want_kf[idx])
        P_ref = int(G["per_frame"][idx, 0])
        assert abs(g._xyz.shape[0] - P_ref) <= max(2, 0.005 * P_ref), (idx, g._xyz.shape[0], P_ref)
        aligned = aligned and g._xyz.shape[0] == P_ref
        got_M, ref_M = get_camera_from_tensor(slam.estimate_pose_list[idx]), get_camera_from_tensor(torch.from_numpy(G["est_poses"][idx]))
        assert (got_M - ref_M).abs().max() < (1e-4 if aligned else 1e-3), (idx, (got_M - ref_M).abs().max())
        with torch.no_grad():
            op = torch.sigmoid(g._opacity)
            got = np.array([float(g._xyz.mean()), float(g._xyz.std()), float(op.mean()), float(op.std()), float(g._scaling.mean()),
                            float(g._scaling.std()), float(g._features_dc.mean()), float(g._rotation[:, 0].mean())])
        tol = 1e-4 if aligned else 5e-3
        assert np.allclose(got, G["per_frame"][idx, 1:], atol=tol, rtol=tol), (idx, got, G["per_frame"][idx, 1:])
    eng = next(iter(engines.values()))
    assert any(c[0] == "track" for c in eng.calls) and any(c[0] == "map" for c in eng.calls)      # the native loops did run
    assert float(slam.gaussians._features_rest.detach().abs().max()) > 0                                # ... and stepped the f_rest rows
    graph = [",".join(map(str, sorted(slam.mapper.covisibility_graph[k]))) for k in range(len(slam.mapper.keyframes))]
    assert graph == [str(s) for s in G["graph"]]
    for kf, ref in zip(slam.mapper.keyframes, G["keyframe_poses"]):
        assert (get_camera_from_tensor(kf.pose.detach()) - get_camera_from_tensor(torch.from_numpy(ref))).abs().max() < 5e-4, kf.idx
    after = np.array([random.random(), float(np.random.rand()), float(torch.rand(1))])
    assert np.allclose(after, G["rng_after"]), (after, G["rng_after"])
