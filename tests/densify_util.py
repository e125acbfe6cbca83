"""TEST INFRASTRUCTURE for the densification tests (tests/test_densify.py on CPU, tests/test_gpu_densify.py on the GPU): the G12 fixture
(tests/golden/g12_densify.npz, written by tests/golden/make_golden_densify.py from the reference's own GaussianModel) loaded into this
repository's GaussianModel, and the comparison of a densified model with the reference's output.  Never imported by the product."""
import os

import numpy as np
import torch

from mm3dgs_slam_amd.config import default_config
from mm3dgs_slam_amd.gaussian_model import GaussianModel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_densify.npz")
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "rgb")
COMPUTED_TOL = 1e-6


def load():
    """The fixture with its full arrays: inputs `in_<name>` from their int16 codes, the reference's outputs `out_<name>` rebuilt from
    the stored parent rows and computed child values (the generator asserts the rebuild bit-identical to the reference's arrays)."""
    f = dict(np.load(GOLDEN))
    for k in [k for k in f if k.startswith("q_")]:
        f["in_" + k[2:]] = (f[k].astype(np.float64) * float(f["step_" + k[2:]])).astype(np.float32)
    f.update(rebuild_outputs(f))
    return f


def rebuild_outputs(f):
    """out_* of the reference's densify_and_prune from f's inputs, `out_parent` (input row of every surviving output row),
    `out_prune_mask`, `split_rows` and the children's computed `out_child_xyz` / `out_child_scaling`: every other value is a copy of
    the parent row, the rows the densification added have zero moments, the statistics are zero."""
    parent, child = f["out_parent"].astype(np.int64), child_rows(f)
    P, n_split = f["in_xyz"].shape[0], f["split_rows"].shape[0]
    new = np.nonzero(~f["out_prune_mask"])[0] >= P - n_split          # (pre-prune position past the unsplit input rows)
    out = {}
    for name in GROUPS:
        v = f["in_" + name][parent]
        if name in ("xyz", "scaling"):
            v[child] = f["out_child_" + name]
        out["out_" + name] = v
        for mv in ("m_", "v_"):
            m = f["in_" + mv + name][parent]
            m[new] = 0.0
            out["out_" + mv + name] = m
    n = parent.shape[0]
    out["out_grad_accum"], out["out_denom"], out["out_max_radii2D"] = np.zeros((n, 1), np.float32), np.zeros((n, 1), np.float32), np.zeros(n, np.float32)
    return out


def model_from_arrays(a, prefix, device, sh_degree, percent_dense, step=7.0):
    """A GaussianModel on `device` holding the arrays a[prefix + name] (parameters, m_/v_ moments, statistics)."""
    cfg = default_config(device=device, mapping={"sh_degree": sh_degree, "percent_dense": float(percent_dense)})
    g = GaussianModel(cfg)
    t = lambda k: torch.as_tensor(np.ascontiguousarray(a[prefix + k])).to(device)
    g._xyz, g._features_dc, g._features_rest, g._opacity = t("xyz"), t("f_dc"), t("f_rest"), t("opacity")
    g._scaling, g._rotation, g._rgb = t("scaling"), t("rotation"), t("rgb")
    g.training_setup()
    for group in g.optimizer.param_groups:
        name = group["name"]
        if prefix + "m_" + name in a:          # (absent: a group without Adam state, like f_rest / rgb after native mapping at SH degree 0)
            g.optimizer.state[group["params"][0]] = {"step": torch.tensor(float(step)), "exp_avg": t("m_" + name).clone(),
                                                     "exp_avg_sq": t("v_" + name).clone()}
    g.xyz_gradient_accum, g.denom, g.max_radii2D = t("grad_accum").clone(), t("denom").clone(), t("max_radii2D").clone()
    return g


def model_from_fixture(f, device):
    return model_from_arrays(f, "in_", device, 3, f["percent_dense"], float(f["in_step"]))


def densify_fixture(g, f, grad_threshold=None):
    """densify_and_prune with the fixture's arguments -> (prune mask, parent) on the host."""
    gt = float(f["grad_threshold"]) if grad_threshold is None else grad_threshold
    mask, parent = g.densify_and_prune(gt, float(f["min_opacity"]), float(f["extent"]), float(f["max_screen_size"]), seed=int(f["seed"]))
    return mask.cpu().numpy(), (None if parent is None else parent.cpu().numpy())


def state(g):
    out = {}
    for group in g.optimizer.param_groups:
        p = group["params"][0]
        st = g.optimizer.state.get(p, {})
        out[group["name"]] = p.detach().cpu().numpy()
        if "exp_avg" in st:
            out["m_" + group["name"]] = st["exp_avg"].cpu().numpy()
            out["v_" + group["name"]] = st["exp_avg_sq"].cpu().numpy()
            out["step_" + group["name"]] = float(st["step"])
    out["grad_accum"], out["denom"] = g.xyz_gradient_accum.cpu().numpy(), g.denom.cpu().numpy()
    out["max_radii2D"] = g.max_radii2D.cpu().numpy()
    return out


def child_rows(f):
    """bool over the reference's output rows: the split children (their xyz / scaling are computed, everything else is copied)."""
    P, n_split, N = f["in_xyz"].shape[0], f["split_rows"].shape[0], int(f["N"])
    mask = f["out_prune_mask"]
    n_keep = P - n_split
    n_clone = mask.shape[0] - n_keep - N * n_split
    return (np.arange(mask.shape[0]) >= n_keep + n_clone)[~mask]


def compare_to_reference(s, f, mask):
    """Every array of the densified state `s` (state()) against the reference's `out_*`: copied values bit-identical, the children's
    xyz and scaling within COMPUTED_TOL.  Returns the largest difference of the computed values."""
    assert np.array_equal(mask, f["out_prune_mask"])
    child = child_rows(f)
    worst = 0.0
    for name in GROUPS:
        ref, got = f["out_" + name], s[name]
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        if name in ("xyz", "scaling"):
            assert np.array_equal(got[~child], ref[~child]), name
            d = float(np.abs(got[child] - ref[child]).max()) if child.any() else 0.0
            assert d <= COMPUTED_TOL, (name, d)
            worst = max(worst, d)
        else:
            assert np.array_equal(got, ref), name
        for mv in ("m_", "v_"):
            assert np.array_equal(s[mv + name], f["out_" + mv + name]), mv + name
        assert s["step_" + name] == float(f["out_step_" + name]), name
    for k in ("grad_accum", "denom", "max_radii2D"):
        assert s[k].shape == f["out_" + k].shape and not s[k].any(), k
    return worst
