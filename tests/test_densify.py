"""Densification (clone + split, slam/gaussian_model.py:490-592) on CPU: the torch path of GaussianModel against the reference's own
code (fixture G12), the stateless split-sample generator, reset_opacity, and `mapping.densify` in both mapping loops' host side and in
a two-rank window.  The device path is held to the same fixture and to the torch path in tests/test_gpu_densify.py."""
import os
import random
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from mm3dgs_slam_amd.general_utils import densify_keys, densify_normals, densify_seed
from mm3dgs_slam_amd.gaussian_model import GaussianModel
from tests import densify_util as du


@pytest.fixture(scope="module")
def fx():
    return du.load()


def test_torch_path_reproduces_the_reference_densify_and_prune(fx):
    g = du.model_from_fixture(fx, "cpu")
    mask, parent = du.densify_fixture(g, fx)
    worst = du.compare_to_reference(du.state(g), fx, mask)
    assert worst <= du.COMPUTED_TOL
    # the fixture exercises every class: clones, splits, unselected rows, never-seen rows, and the prune after the densification
    P, n_split = fx["in_xyz"].shape[0], fx["split_rows"].shape[0]
    n_clone = mask.shape[0] - (P - n_split) - 2 * n_split
    assert n_clone > 20 and n_split > 20 and mask.sum() > 0 and (fx["in_denom"] == 0).sum() > 100
    assert fx["in_f_rest"].shape[1] == 15
    # parent: every row after the densification came from the row it names (children: same rotation / colour, different position)
    assert parent.shape == mask.shape
    for name in ("rotation", "f_rest", "opacity", "rgb"):
        assert np.array_equal(fx["in_" + name][parent][~mask], fx["out_" + name])


def test_nothing_selected_keeps_the_rows_and_still_zeroes_the_statistics(fx):
    g = du.model_from_fixture(fx, "cpu")
    mask, parent = du.densify_fixture(g, fx, grad_threshold=1.0)
    assert parent is None and np.array_equal(mask, fx["none_prune_mask"])
    s = du.state(g)
    for name in du.GROUPS:
        assert np.array_equal(s[name], fx["in_" + name][~mask])
        assert np.array_equal(s["m_" + name], fx["in_m_" + name][~mask])
        assert s["step_" + name] == float(fx["none_step_" + name])
    for k in ("grad_accum", "denom", "max_radii2D"):
        assert np.array_equal(s[k], fx["none_" + k]) and not s[k].any()
    # with nothing pruned either, the parameter objects stay in place and lose their gradients (the convention of prune_points)
    g = du.model_from_fixture(fx, "cpu")
    g._xyz.grad = torch.ones_like(g._xyz)
    before = g._xyz
    _, parent = g.densify_and_prune(1.0, 0.0, 1e9, None, seed=1)
    assert parent is None and g._xyz is before and g._xyz.grad is None and not g.denom.any()


def test_generator_keys_are_pinned_and_the_normals_are_standard(fx):
    for seed, row, k, j, key in fx["keys"]:
        assert int(densify_keys(int(seed), torch.tensor([int(row)]), int(k) + 1)[int(k), 0, int(j)]) == int(key)
    rows = torch.arange(500_000)
    z = densify_normals(99, rows, 2).double()
    assert z.shape == (1_000_000, 3)
    assert abs(float(z.mean())) < 3e-3 and abs(float(z.var()) - 1.0) < 5e-3
    assert torch.isfinite(z).all()
    assert torch.equal(densify_normals(99, rows[:1000], 2), densify_normals(99, rows[:1000], 2))
    assert not torch.equal(densify_normals(99, rows[:1000], 2), densify_normals(100, rows[:1000], 2))
    # child k of parent s is row k * S + s; a row's samples do not depend on which other rows are split
    a, b = densify_normals(5, torch.tensor([3, 7, 11]), 2), densify_normals(5, torch.tensor([7]), 2)
    assert torch.equal(a[1], b[0]) and torch.equal(a[4], b[1])
    assert densify_seed(0, 3, 50) == densify_seed(0, 3, 50) != densify_seed(0, 3, 51) and 0 <= densify_seed(7, 1, 0) < 2 ** 31


def test_reset_opacity_matches_the_reference(fx):
    g = du.model_from_fixture(fx, "cpu")
    g.reset_opacity()
    s = du.state(g)
    assert np.array_equal(s["opacity"], fx["ro_opacity"])
    assert np.array_equal(s["m_opacity"], fx["ro_m_opacity"]) and np.array_equal(s["v_opacity"], fx["ro_v_opacity"])
    assert not s["m_opacity"].any() and s["step_opacity"] == float(fx["ro_step_opacity"])
    assert np.array_equal(s["xyz"], fx["in_xyz"]) and np.array_equal(s["m_xyz"], fx["in_m_xyz"])


def test_densify_and_clone_and_split_have_the_reference_signatures(fx):
    g = du.model_from_fixture(fx, "cpu")
    grads = (g.xyz_gradient_accum / g.denom).nan_to_num(0.0)
    P = g._xyz.shape[0]
    clone = g.densify_and_clone(grads, float(fx["grad_threshold"]), float(fx["extent"]))
    assert g._xyz.shape[0] == P + int(clone.sum())
    split = g.densify_and_split(grads, float(fx["grad_threshold"]), float(fx["extent"]), N=2, seed=int(fx["seed"]))
    assert g._xyz.shape[0] == P + int(clone.sum()) + int(split.sum())
    g2 = du.model_from_fixture(fx, "cpu")
    g2.densify(float(fx["grad_threshold"]), float(fx["extent"]), seed=int(fx["seed"]))
    assert torch.equal(g._xyz, g2._xyz)


# ---- the mapping loops ------------------------------------------------------------------------------------------------------------
def _slam(native, densify, ba=False, frames=3, window=None):
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.renderer import Renderer
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from oracle.raster_ref import RefRasterizer
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    mapping = {"iters": 7, "kf_every": 1, "pruning_interval": 3, "densify_until_iter": 6, "do_BA": ba, "seed_fraction": 0.15,
               "densification_interval": 1, "densify_grad_threshold": 5e-5}
    if densify is not None:
        mapping["densify"] = densify
    cfg = default_config(device="cpu", height=48, width=64, tracking={"iters": 3}, mapping=mapping)
    seq = SyntheticSequence(cfg, frames, 800, seed=5, renderer=Renderer(cfg, rasterizer_cls=RefRasterizer))
    return SLAM(cfg, seq, rasterizer_cls=RefRasterizer, render_mode="reference" if native else "fused", window=window, native_loops=native)


def _install_cpu_engine(monkeypatch):
    from mm3dgs_slam_amd import fused
    from tests import cpu_engine
    patches, _ = cpu_engine.install(fused)
    for name, value in patches.items():
        monkeypatch.setattr(fused.FusedEngine if name == "eligible" else fused, name, value)


@pytest.mark.parametrize("native", [False, True])
def test_mapping_loops_densify_at_pruning_steps_and_carry_the_ba_mask(native, monkeypatch):
    if native:
        _install_cpu_engine(monkeypatch)
    log = []
    real_densify, real_prune = GaussianModel.densify_and_prune, GaussianModel.prune

    def densify_and_prune(self, *a, **k):
        P0 = int(self._xyz.shape[0])
        mask, parent = real_densify(self, *a, **k)
        log.append(("densify", P0, None if parent is None else int(parent.shape[0]), int(self._xyz.shape[0]), k.get("seed")))
        return mask, parent

    def prune(self, *a, **k):
        P0 = int(self._xyz.shape[0])
        out = real_prune(self, *a, **k)
        log.append(("prune", P0, int(self._xyz.shape[0])))
        return out
    monkeypatch.setattr(GaussianModel, "densify_and_prune", densify_and_prune)
    monkeypatch.setattr(GaussianModel, "prune", prune)
    slam = _slam(native, True, ba=True)
    masks = []
    for i in range(3):
        slam.step(i)
        om = getattr(slam.mapper, "_opt_mask", None) if native else None
        masks.append(om)
    dens = [e for e in log if e[0] == "densify"]
    # frames 0..2 x pruning iterations 0, 3, 6: nine densify steps, each followed by its prune (and no prune on its own)
    assert len(dens) == 9 and sum(e[0] == "prune" for e in log) == 9
    assert any(e[2] is not None and e[2] > e[1] for e in dens), dens          # the map grew at some densify step
    assert len(set(e[4] for e in dens)) == 9                                   # one seed per (frame, iteration)
    if native:
        assert masks[-1] is not None and masks[-1].shape[0] == slam.gaussians._xyz.shape[0]
    for p in slam.gaussians._params().values():
        assert torch.isfinite(p).all()


def test_ba_mask_children_take_their_parents_flag(fx):
    g = du.model_from_fixture(fx, "cpu")
    flags = torch.from_numpy(np.arange(fx["in_xyz"].shape[0]) % 3 == 0)
    mask, parent = g.densify_and_prune(float(fx["grad_threshold"]), float(fx["min_opacity"]), float(fx["extent"]), float(fx["max_screen_size"]),
                                       seed=int(fx["seed"]))
    carried = GaussianModel.carry_rows(flags, parent, mask)
    assert carried.shape[0] == g._xyz.shape[0]
    assert torch.equal(carried, torch.from_numpy(np.asarray(flags)[parent][~mask.numpy()]))


@pytest.mark.parametrize("native", [False, True])
def test_densify_absent_equals_densify_false(native, monkeypatch):
    if native:
        _install_cpu_engine(monkeypatch)
    out = []
    for flag in (None, False):
        slam = _slam(native, flag, frames=2)
        for i in range(2):
            slam.step(i)
        out.append((slam.gaussians._xyz.detach().clone(), slam.gaussians._opacity.detach().clone(), torch.stack(slam.estimate_pose_list[:2])))
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ---- two-rank window (gloo) -------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, out, native):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    from mm3dgs_slam_amd.window_parallel import WindowParallel
    if native:
        from mm3dgs_slam_amd import fused
        from tests import cpu_engine
        patches, _ = cpu_engine.install(fused)
        for name, value in patches.items():
            setattr(fused.FusedEngine if name == "eligible" else fused, name, value)
    slam = _slam(native, True, frames=2, window=WindowParallel(rank, world))
    P = []
    for i in range(2):
        slam.step(i)
        P.append(int(slam.gaussians._xyz.shape[0]))
    g = slam.gaussians
    st = {"P": torch.tensor(P), "xyz": g._xyz.detach(), "scaling": g._scaling.detach(), "op": g._opacity.detach(), "acc": g.xyz_gradient_accum.clone()}
    for gr in g.optimizer.param_groups:
        s = g.optimizer.state.get(gr["params"][0], {})
        if "exp_avg" in s:
            st["m_" + gr["name"]], st["v_" + gr["name"]] = s["exp_avg"].clone(), s["exp_avg_sq"].clone()
    torch.save(st, os.path.join(out, f"d{int(native)}_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("native", [False, True])
def test_two_rank_window_densifies_identically_on_both_ranks(native, tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), native), nprocs=2, join=True)
    a, b = torch.load(tmp_path / f"d{int(native)}_0.pt"), torch.load(tmp_path / f"d{int(native)}_1.pt")
    assert a.keys() == b.keys() and any(k.startswith("m_") for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert a["xyz"].shape[0] > 0
