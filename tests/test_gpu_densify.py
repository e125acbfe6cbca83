"""Densification on the device (csrc/compact.hip: densify_classify / densify_scan / densify_rows through mm3dgs_densify_plan /
mm3dgs_densify_rows, GaussianModel.densify_device) against the torch path on the same state, against the reference's own output
(fixture G12), and inside the native mapping loop with `mapping.densify: true`."""
import random

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd.gaussian_model import GaussianModel
from tests import densify_util as du

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _random_arrays(P, sh_degree, seed):
    g = torch.Generator().manual_seed(seed)
    n_rest = (sh_degree + 1) ** 2 - 1
    a = {"xyz": torch.randn(P, 3, generator=g) * 1.5 + torch.tensor([0.0, 0.0, 3.0]), "f_dc": torch.randn(P, 1, 3, generator=g),
         "f_rest": torch.randn(P, n_rest, 3, generator=g) * 0.1, "opacity": torch.randn(P, 1, generator=g) * 3.0,
         "scaling": torch.rand(P, 3, generator=g) * 3.4 - 5.0, "rotation": torch.randn(P, 4, generator=g), "rgb": torch.rand(P, 3, generator=g)}
    denom = torch.randint(0, 6, (P, 1), generator=g).float()
    a["grad_accum"], a["denom"] = torch.rand(P, 1, generator=g) * 6e-4 * denom, denom
    a["max_radii2D"] = torch.rand(P, generator=g) * 200.0
    for name in du.GROUPS:
        a["m_" + name] = torch.randn(a[name].shape, generator=g) * 1e-3
        a["v_" + name] = torch.rand(a[name].shape, generator=g) * 1e-6
    return {k: v.numpy() for k, v in a.items()}


def _arrays_of(g):
    s = du.state(g)
    out = {k: s[k] for k in s if not k.startswith("step_")}
    out["max_radii2D"] = s["max_radii2D"]
    return out


def _device_vs_torch(a, sh_degree, percent_dense, grad_t, extent, seed):
    dev = du.model_from_arrays(a, "", DEV, sh_degree, percent_dense)
    ref = du.model_from_arrays(a, "", DEV, sh_degree, percent_dense)
    P = dev._xyz.shape[0]
    parent_d = dev.densify_device(grad_t, extent, seed)
    parent_t = ref._densify_torch(grad_t, extent, seed)
    torch.cuda.synchronize()
    assert parent_d is not None and parent_t is not None
    parent_d, parent_t = parent_d.long().cpu().numpy(), parent_t.cpu().numpy()
    assert np.array_equal(parent_d, parent_t)                          # counts, classes and row order
    sd, st = du.state(dev), du.state(ref)
    # the classes, from the predicate (the rows are [kept][clones][child 0 of each split row][child 1 ...])
    grads = np.nan_to_num(a["grad_accum"][:, 0] / a["denom"][:, 0], nan=0.0)
    split_parents = (grads >= np.float32(grad_t)) & (np.exp(a["scaling"]).max(1) > np.float32(percent_dense * extent))
    n_split = int(split_parents.sum())
    n_keep = P - n_split
    n_clone = parent_d.shape[0] - n_keep - 2 * n_split
    is_new = np.arange(parent_d.shape[0]) >= n_keep
    child = np.arange(parent_d.shape[0]) >= n_keep + n_clone
    assert np.array_equal(np.sort(parent_d[child][:n_split]), np.nonzero(split_parents)[0])
    worst = 0.0
    for name in du.GROUPS:
        if name in ("xyz", "scaling"):
            assert np.array_equal(sd[name][~child], st[name][~child]), name
            if child.any():
                d = np.abs(sd[name][child] - st[name][child])
                assert np.all(d <= du.COMPUTED_TOL + 2.4e-7 * np.abs(st[name][child])), (name, float(d.max()))
                worst = max(worst, float(d.max()))
        else:
            assert np.array_equal(sd[name], st[name]), name
        assert ("m_" + name in sd) == ("m_" + name in st) == ("m_" + name in a), name      # (groups without Adam state stay without)
        if "m_" + name not in a:
            continue
        for mv in ("m_", "v_"):
            assert np.array_equal(sd[mv + name], st[mv + name]), mv + name
            assert not sd[mv + name][is_new].any(), mv + name
        assert sd["step_" + name] == st["step_" + name]
    for k in ("grad_accum", "denom", "max_radii2D"):
        assert sd[k].shape[0] == parent_d.shape[0] and not sd[k].any(), k
    assert n_split > 0 and n_clone > 0          # both clones and splits happened
    return worst, n_split, n_clone


@pytest.mark.parametrize("sh_degree", [0, 3])
def test_device_path_equals_torch_path_at_20k(sh_degree):
    a = _random_arrays(20000, sh_degree, seed=20 + sh_degree)
    worst, n_split, n_clone = _device_vs_torch(a, sh_degree, 0.01, 2e-4, 2.5, seed=777)
    print(f"20k sh{sh_degree}: split {n_split} clone {n_clone}, max |split xyz / scaling difference| {worst:.3e}")


@pytest.mark.parametrize("sh_degree", [0, 3])
def test_device_path_equals_torch_path_on_a_natively_mapped_configs1_map(sh_degree):
    """The configs[1] workload's map (640x480, ~150 k Gaussians from frame 0's thinned seeding) with statistics accumulated by real
    native mapping iterations."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device=DEV, height=480, width=640, tracking={"iters": 5},
                         mapping={"iters": 20, "pruning_interval": 50, "sh_degree": sh_degree, "seed_fraction": 150000 / (0.95 * 480 * 640)})
    seq = SyntheticSequence(cfg, 2, 150000, seed=1)
    slam = SLAM(cfg, seq)
    slam.step(0)
    g = slam.gaussians
    torch.cuda.synchronize()
    assert g._xyz.shape[0] > 100000 and int((g.denom > 0).sum()) > 10000
    a = _arrays_of(g)
    seen = (a["denom"] > 0)
    thr = float(np.quantile((a["grad_accum"][seen] / a["denom"][seen]), 0.8))      # the top fifth of the seen rows densify
    extent = float(slam.mapper.camera_extent)
    # (frame 0's seeded Gaussians are all far below the shipped percent_dense * extent: a percent_dense at their median max scale
    #  gives this state both clones and splits)
    pd = float(np.median(np.exp(a["scaling"]).max(1))) / extent
    assert "m_xyz" in a and "m_rgb" not in a          # (the native loop steps five groups: rgb and, at SH degree 0 active, f_rest have no state)
    worst, n_split, n_clone = _device_vs_torch(a, sh_degree, pd, thr, extent, seed=4242)
    print(f"configs[1] map P {a['xyz'].shape[0]} sh{sh_degree}: split {n_split} clone {n_clone}, max difference {worst:.3e}")


def test_fixture_on_the_device_matches_the_reference():
    fx = du.load()
    g = du.model_from_fixture(fx, DEV)
    mask, parent = du.densify_fixture(g, fx)
    worst = du.compare_to_reference(du.state(g), fx, mask)
    print(f"G12 on the device: max |computed - reference| {worst:.3e}")
    g = du.model_from_fixture(fx, DEV)
    mask, parent = du.densify_fixture(g, fx, grad_threshold=1.0)
    assert parent is None and np.array_equal(mask, fx["none_prune_mask"])
    s = du.state(g)
    for k in ("grad_accum", "denom", "max_radii2D"):
        assert not s[k].any()


def test_native_mapping_loop_with_densify_grows_the_map_and_is_deterministic(monkeypatch):
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    grew = []
    real = GaussianModel.densify_and_prune

    def densify_and_prune(self, *a, **k):
        P0 = int(self._xyz.shape[0])
        out = real(self, *a, **k)
        grew.append((P0, None if out[1] is None else int(out[1].shape[0])))
        return out
    monkeypatch.setattr(GaussianModel, "densify_and_prune", densify_and_prune)
    runs = []
    for _ in range(2):
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        cfg = default_config(device=DEV, height=120, width=160, tracking={"iters": 10},
                             mapping={"iters": 12, "kf_every": 1, "pruning_interval": 4, "densify_until_iter": 10, "seed_fraction": 0.2,
                                      "densify": True, "densification_interval": 1})
        seq = SyntheticSequence(cfg, 3, 6000, seed=6)
        slam = SLAM(cfg, seq)
        assert type(slam.mapper).__name__ == "FusedMapper"
        for i in range(3):
            slam.step(i)
        torch.cuda.synchronize()
        g = slam.gaussians
        for p in g._params().values():
            assert torch.isfinite(p).all()
        runs.append({k: v.detach().clone() for k, v in g._params().items()} | {"poses": torch.stack(slam.estimate_pose_list[:3])})
    assert len(grew) == 2 * 3 * 3 and any(n is not None and n > p for p, n in grew), grew
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
