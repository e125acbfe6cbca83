"""The multi-GPU mapping window on the NATIVE loops at an ACTIVE SH degree (ABI 212), on CPU: fused.py's window orchestration over the SH
stand-in engine (tests/cpu_engine_sh.py: the W-wide flat gradient buffer with its f_rest block, d_f_rest outputs, the sixth Adam group), two
gloo ranks, at the sizes of tests/test_window_parallel.py with mapping.sh_degree 2 and the map at active degree 2 (a resumed map).

Before ABI 212 fused.py handed every such window to the torch-graph Mapper.optimize_map; every SLAM-level run here asserts that the native
loop served it (map calls with an f_rest gradient output, Mapper.optimize_map never entered)."""
import os
import random
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

MODES = {"default": {}, "python_sh": {"convert_SHs_python": True}, "world_means": {"transform_means_python": False}}
DENSIFY = {"densify": True, "densification_interval": 1, "pruning_interval": 2, "densify_grad_threshold": 5e-5}


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _build(window, native=False, ba=False, mode="default", densify=False):
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.renderer import Renderer
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from oracle.raster_ref import RefRasterizer
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    mapping = {"iters": 5 if ba else 3, "kf_every": 1, "do_BA": ba, "sh_degree": 2, **(DENSIFY if densify else {})}
    cfg = default_config(device="cpu", height=32, width=48, tracking={"iters": 2}, mapping=mapping, pipeline=dict(MODES[mode]))
    seq = SyntheticSequence(cfg, 3, 500, seed=5, renderer=Renderer(cfg, rasterizer_cls=RefRasterizer))
    slam = SLAM(cfg, seq, rasterizer_cls=RefRasterizer, render_mode="reference" if native else "fused", window=window, native_loops=native)
    slam.gaussians.active_sh_degree = 2      # a map resumed from a checkpoint (slam/gaussian_model.py:363)
    return slam


def _install(setattr_fn=None):
    """The native loops' host side over tests/cpu_engine_sh.py; Mapper.optimize_map (the torch-graph loop) counted."""
    from mm3dgs_slam_amd import fused, mapper
    from tests import cpu_engine_sh
    patches, registry = cpu_engine_sh.install(fused)
    for name, value in patches.items():
        (setattr_fn or setattr)(fused.FusedEngine if name == "eligible" else fused, name, value)
    entered = []
    real = mapper.Mapper.optimize_map

    def counted(self, *a, **k):
        entered.append(1)
        return real(self, *a, **k)
    (setattr_fn or setattr)(mapper.Mapper, "optimize_map", counted)
    return registry, entered


def _assert_native(registry, entered):
    engines = list(registry.values())
    assert engines and sum(len(e.rest_outputs) for e in engines) > 0, "no mm3dgs_slam_map call wrote an f_rest gradient"
    assert not entered, f"the torch-graph Mapper.optimize_map ran {len(entered)} times"


def _run(slam, ba=False):
    for i in range(3):
        slam.step(i)
    if ba:      # (tests/test_window_parallel.py's three-view bundle-adjustment window)
        color, depth, _ = slam.seq[2]
        slam.mapper.optimize_map(2, 6, [0] * (len(slam.mapper.keyframes) + 1) + [-1] if len(slam.mapper.keyframes) < 2 else [0, 1, -1], None,
                                 slam.estimate_pose_list[2], color, depth, None)


def _state(slam):
    g = slam.gaussians
    return {"xyz": g._xyz.detach(), "op": g._opacity.detach(), "scaling": g._scaling.detach(), "rotation": g._rotation.detach(),
            "f_dc": g._features_dc.detach(), "f_rest": g._features_rest.detach(), "acc": g.xyz_gradient_accum.clone(), "denom": g.denom.clone(),
            "radii": g.max_radii2D.clone(), "poses": torch.stack(slam.estimate_pose_list[:3])}


def _moments(slam):
    opt = slam.gaussians.optimizer
    out = {}
    for gr in opt.param_groups:
        st = opt.state.get(gr["params"][0], {})
        if "exp_avg" in st:
            out["m_" + gr["name"]], out["v_" + gr["name"]] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    return out


def _worker(rank, world, port, out, mode, ba, optimizer, tag, densify):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    from mm3dgs_slam_amd.gaussian_model import GaussianModel
    from mm3dgs_slam_amd.window_parallel import WindowParallel
    registry, entered = _install()
    dens_log = []
    real_dp = GaussianModel.densify_and_prune

    def densify_and_prune(self, *a, **k):
        P0 = int(self._xyz.shape[0])
        mask, parent = real_dp(self, *a, **k)
        dens_log.append((P0, None if parent is None else int(parent.shape[0])))
        return mask, parent
    GaussianModel.densify_and_prune = densify_and_prune
    slam = _build(WindowParallel(rank, world, optimizer=optimizer), native=True, ba=ba, mode=mode, densify=densify)
    _run(slam, ba)
    _assert_native(registry, entered)
    st = _state(slam)
    st.update(_moments(slam))
    st["view_log"] = list(next(iter(registry.values())).view_log)
    st["sharded_steps"] = torch.tensor(slam.mapper.window.sharded_steps)
    st["dens_log"] = dens_log
    torch.save(st, os.path.join(out, f"{tag}{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _spawn(tmp_path, mode="default", ba=False, optimizer="allreduce", tag="r", densify=False):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), mode, ba, optimizer, tag, densify), nprocs=2, join=True)
    return [torch.load(tmp_path / f"{tag}{r}.pt") for r in range(2)]


@pytest.mark.parametrize("mode", list(MODES))
def test_two_native_ranks_equal_window_batch_two_and_the_torch_graph_window(mode, tmp_path, monkeypatch):
    """Two native gloo ranks (per-view mm3dgs_slam_map with f_rest gradient outputs, one flat all-reduce over W P, mm3dgs_adam with f_rest
    among its groups -- the default step at SH > 0) == one native rank with window-batch 2 (rtol 1e-5 / atol 1e-7) == the torch-graph window-batch-2 loop (rtol
    2e-4 / atol 2e-6): the bars of tests/test_window_parallel.py:147,155, in each of the three SH direction modes."""
    a, b = _spawn(tmp_path, mode)
    for k in ("view_log", "dens_log", "sharded_steps"):
        a.pop(k); b.pop(k)
    assert a["xyz"].shape[0] > 0 and float(a["f_rest"].abs().max()) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k
    from mm3dgs_slam_amd.window_parallel import WindowParallel
    torch.set_num_threads(2)
    registry, entered = _install(monkeypatch.setattr)
    one = _build(WindowParallel(0, 1, batch=2), native=True, mode=mode)
    _run(one)
    _assert_native(registry, entered)
    ref = _state(one)
    for k in ref:
        assert ref[k].shape == a[k].shape, k
        assert torch.allclose(ref[k], a[k], rtol=1e-5, atol=1e-7), (mode, k, float((ref[k] - a[k]).abs().max()))
    monkeypatch.undo()
    graph = _build(WindowParallel(0, 1, batch=2), mode=mode)
    _run(graph)
    tg = _state(graph)
    # (the arrays tests/test_window_parallel.py:152-155 compares, + f_rest.  Not the raw quaternions: their norm has no gradient, and the two
    #  loops' rotation logits already differ by up to 1.7e-3 at SH degree 0 -- 1382 of 6120 elements outside this bar, measured on this very
    #  configuration with active_sh_degree 0 -- against 2.6e-3 / 1415 at degree 2)
    tg.pop("rotation")
    for k in tg:
        assert tg[k].shape == ref[k].shape, k
        assert torch.allclose(tg[k], ref[k], rtol=2e-4, atol=2e-6), (mode, k, float((tg[k] - ref[k]).abs().max()))


@pytest.mark.parametrize("ba,densify", [(False, False), (True, False), (False, True)])
def test_sharded_step_two_ranks_is_bit_identical_to_the_all_reduce_step(ba, densify, tmp_path):
    """optimizer="reduce_scatter" (the sharded step over W P elements: slices that cut through the f_rest block too, f_rest moments gathered
    before the pruning / densification surgery and at the end of the loop) against "allreduce" over two gloo ranks: parameters, statistics,
    poses and every Adam moment, f_rest's included, bit for bit."""
    A = _spawn(tmp_path, ba=ba, optimizer="allreduce", tag="a", densify=densify)
    S = _spawn(tmp_path, ba=ba, optimizer="reduce_scatter", tag="s", densify=densify)
    for r in range(2):
        a, s = A[r], S[r]
        assert a.pop("view_log") == s.pop("view_log")
        assert int(a.pop("sharded_steps")) == 0 and int(s.pop("sharded_steps")) > 0
        da, ds = a.pop("dens_log"), s.pop("dens_log")
        assert da == ds
        if densify:      # a densification step really fired and grew the map (parent rows beyond the map it started from)
            assert any(p is not None and p > P0 for P0, p in da), da
        assert "m_f_rest" in a and "v_f_rest" in a and float(a["v_f_rest"].abs().max()) > 0
        for k in a:
            assert torch.equal(a[k], s[k]), (r, k, float((a[k] - s[k]).abs().max()))


@pytest.mark.parametrize("ba", [False, True])
def test_fused_adam_and_projection_step_equals_the_two_call_step(ba, monkeypatch):
    """mm3dgs_slam_adam_project with the sixth group against mm3dgs_adam over the flat buffer (f_rest one of its groups) + a self-projecting
    next call, window-batch 2 at SH 2: the same views in the same order, and the map, the statistics, the poses and the moments bit for bit."""
    from mm3dgs_slam_amd import fused
    from mm3dgs_slam_amd.window_parallel import WindowParallel
    torch.set_num_threads(2)
    registry, entered = _install(monkeypatch.setattr)
    states, logs, n_fused = [], [], []
    for fuse in (True, False):
        monkeypatch.setattr(fused.FusedMapper, "fuse_adam_project", fuse)
        monkeypatch.setattr(fused.FusedMapper, "fuse_adam_project_sh", fuse)      # (the fused SH step is opt-in)
        registry.clear()
        slam = _build(WindowParallel(0, 1, batch=2), native=True, ba=ba)
        _run(slam, ba=ba)
        _assert_native(registry, entered)
        states.append({**_state(slam), **_moments(slam)})
        eng = next(iter(registry.values()))
        logs.append(list(eng.view_log))
        n_fused.append(sum(1 for c in eng.calls if c[0] == "adam_project"))
    assert n_fused[0] > 0 and n_fused[1] == 0, n_fused
    assert logs[0] == logs[1]
    assert "m_f_rest" in states[0] and states[0].keys() == states[1].keys()
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), (k, float((states[0][k] - states[1][k]).abs().max()))


def test_shard_bounds_and_the_engine_flat_buffer_cover_the_f_rest_columns():
    """shard_bounds partitions n = W P for W = 14 + 3 n_rest (n_rest 0, 3, 8, 15), and FusedEngine's flat buffer holds world x S elements of
    it (what a reduce-scatter / all-gather over `world` ranks touches) for world 1, 2, 3, 8; at degree 0 the layout is the 14-column one."""
    from mm3dgs_slam_amd.fused import FusedEngine
    from mm3dgs_slam_amd.window_parallel import WindowParallel
    lib = types.SimpleNamespace(mm3dgs_geom_bytes=lambda P: 16, mm3dgs_binning_bytes=lambda n: 16, mm3dgs_backward_scratch_bytes=lambda P, n: 16)
    for n_rest in (0, 3, 8, 15):
        W = 14 + 3 * n_rest
        for P in (1, 37, 1530, 6001):
            eng = FusedEngine.__new__(FusedEngine)
            eng.dev, eng.lib, eng.H, eng.W, eng.P, eng.n_cap, eng.ratio, eng.max_tile_len = torch.device("cpu"), lib, 48, 64, -1, 0, None, 1 << 30
            eng.grads = None
            eng.bind_rest_rows(types.SimpleNamespace(active_sh_degree=2 if n_rest else 0, _features_rest=torch.zeros(P, n_rest, 3)))
            eng._ensure(P, True)
            assert eng.flat_width == W and eng.acc.numel() == W * P
            assert eng.flat.numel() == (W + 2) * P + 64
            if n_rest == 0:
                assert "f_rest" not in eng.grads
            else:
                fr = eng.grads["f_rest"]
                assert fr.shape == (P, n_rest, 3) and fr.data_ptr() == eng.flat[14 * P:].data_ptr()
            assert eng.stat_delta[1].data_ptr() == eng.flat[W * P:].data_ptr() and eng.stat_delta[2].data_ptr() == eng.flat[(W + 1) * P:].data_ptr()
            for world in (1, 2, 3, 8):
                spans = [WindowParallel(r, world).shard_bounds(W * P) for r in range(world)]
                S = spans[0][0]
                assert all(s[0] == S for s in spans) and S % 4 == 0 and W * P <= world * S <= W * P + 4 * world + 3
                assert eng.flat.numel() >= world * S
                covered = 0
                for r, (_, lo, hi) in enumerate(spans):
                    assert lo == min(r * S, W * P) and lo <= hi <= W * P
                    covered += hi - lo
                assert covered == W * P
