"""The host bookkeeping of GaussianModel's device row surgery (prune -> prune_mask_device + compact_device, seed_device), run on the CPU
against the torch surgery (prune_points, densification_postfix) of a deep copy of the same model: parameters, Adam moments and step
counters, the set of groups that has Adam state, the densification statistics, fresh leaves and the keys of ``optimizer.state``.

The library is a stand-in (`_RowLib`) for the entry points whose semantics are pure row movement.  It dereferences the very pointers
and tables gaussian_model.py hands over (host tensors: `from_address` views are what the kernels' global-memory accesses are on the
GPU) and records every call.  The seeding stand-in writes, into the rows it is told to write, the raster index of the pixel each row
comes from -- order and extent, not the kernel's arithmetic, which tests/test_gpu_fused.py holds to fixture G7.  Densification has no
stand-in (its row placement is the kernel's own): tests/test_densify.py and tests/test_gpu_densify.py cover it."""
import copy
import ctypes as C

import pytest
import torch

from mm3dgs_slam_amd import gaussian_model as gm
from mm3dgs_slam_amd.config import default_config
from tests.cpu_engine import _view

PARAMS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_rgb")
STATS = ("xyz_gradient_accum", "denom", "max_radii2D")


def _addr(p):
    return int(getattr(p, "value", p) or 0)


class _RowLib:
    def __init__(self):
        self.calls = []

    def mm3dgs_compact_work_bytes(self, n):
        self.calls.append("work_bytes")
        return 64

    def mm3dgs_compact_plan(self, n, keep, work, n_keep, stream):
        self.calls.append("plan")
        _view(_addr(n_keep), 1, C.c_int32)[0] = int(_view(_addr(keep), n, C.c_uint8).sum()) if n else 0
        return 0

    def mm3dgs_compact_rows(self, P, keep, work, table, n_arrays, stream):
        self.calls.append("rows")
        kept = _view(_addr(keep), P, C.c_uint8) != 0
        n_keep = int(kept.sum())
        for e in table[:n_arrays]:
            assert e.width > 0 and e.src and e.dst
            src = _view(e.src, P * e.width, C.c_int32).view(P, e.width)
            _view(e.dst, n_keep * e.width, C.c_int32).view(n_keep, e.width).copy_(src[kept])
        return 0

    def mm3dgs_seed_gaussians(self, H, W, color, depth, keep, work, pose, fx, fy, cx, cy, row0, outputs, n_rest, stream):
        self.calls.append("seed")
        pixels = torch.nonzero(_view(_addr(keep), H * W, C.c_uint8)).squeeze(1).float()
        n, so = pixels.numel(), outputs._obj
        for name, width in dict(xyz=3, f_dc=3, f_rest=3 * n_rest, opacity=1, scaling=3, rotation=4, rgb=3).items():
            if width:
                _view(getattr(so, name), (row0 + n) * width).view(row0 + n, width)[row0:] = pixels[:, None]
        return 0

    def mm3dgs_prune_mask(self, P, opacity, scaling, radii, min_opacity, max_scale, max_screen, keep, counter, stream):
        self.calls.append("prune_mask")
        prune = torch.sigmoid(_view(_addr(opacity), P)) < min_opacity
        prune |= torch.exp(_view(_addr(scaling), 3 * P).view(P, 3)).max(dim=1).values > max_scale
        if radii is not None:
            prune |= _view(_addr(radii), P) > max_screen
        _view(_addr(keep), P, C.c_uint8).copy_(~prune)
        _view(_addr(counter), 1, C.c_int32)[0] += int(prune.sum())
        return 0


@pytest.fixture
def lib(monkeypatch):
    lib = _RowLib()
    monkeypatch.setattr(gm, "_library", lambda: lib)
    monkeypatch.setattr(gm, "_stream", lambda: None)
    return lib


def _model(P, sh_degree, stateless=(), seed=0):
    """A host model with real Adam moments on every group not in `stateless`, a pending gradient on every parameter (which no
    surgery may keep), non-zero statistics, and rows for each clause of the pruning predicate to fire on."""
    g = gm.GaussianModel(default_config(device="cpu", mapping={"sh_degree": sh_degree}))
    gen = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=gen)
    g._xyz, g._features_dc, g._features_rest = r(P, 3), r(P, 1, 3), r(P, (sh_degree + 1) ** 2 - 1, 3)
    g._opacity, g._scaling, g._rotation, g._rgb = r(P, 1) * 4, r(P, 3) * 0.5 - 4.0, r(P, 4), r(P, 3)
    g._scaling[::7] += 3.0
    g.training_setup()
    if P:
        for group in g.optimizer.param_groups:
            if group["name"] not in stateless:
                group["params"][0].grad = r(*group["params"][0].shape)
        g.optimizer.step()
    for group in g.optimizer.param_groups:
        group["params"][0].grad = r(*group["params"][0].shape)
    g.xyz_gradient_accum, g.denom = torch.rand(P, 1, generator=gen) + 0.5, torch.rand(P, 1, generator=gen) + 0.5
    g.max_radii2D = torch.rand(P, generator=gen) * 150 + 1
    return g


def _pair(g):
    """(g forced onto the device path, a deep copy forced onto the torch path)."""
    ref = copy.deepcopy(g)
    g._native, ref._native = (lambda: True), (lambda: False)
    return g, ref


def _check_consistent(g):
    """Fresh leaves without gradients, and an optimiser state keyed by them alone."""
    params = [group["params"][0] for group in g.optimizer.param_groups]
    for attr, group, p in zip(PARAMS, g.optimizer.param_groups, params):
        assert getattr(g, attr) is p, attr
        assert p.is_leaf and p.requires_grad and p.grad is None, attr
        st = g.optimizer.state.get(p)
        assert st is None or (st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape), attr
    assert all(any(k is p for p in params) for k in g.optimizer.state), "stale key in optimizer.state"
    for attr in STATS:
        assert getattr(g, attr).shape[0] == g._xyz.shape[0], attr


def _check_same(g, ref):
    for attr in PARAMS + STATS:
        a, b = getattr(g, attr).detach(), getattr(ref, attr).detach()
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), attr
    for ga, gb in zip(g.optimizer.param_groups, ref.optimizer.param_groups):
        sa, sb = g.optimizer.state.get(ga["params"][0]), ref.optimizer.state.get(gb["params"][0])
        assert ga["name"] == gb["name"] and ga["lr"] == gb["lr"]
        assert (sa is None) == (sb is None), ga["name"]
        if sa is not None:
            assert sorted(sa) == sorted(sb) and float(sa["step"]) == float(sb["step"]), ga["name"]
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), ga["name"]
    assert g.generation == ref.generation
    _check_consistent(g)
    _check_consistent(ref)


def _stateful(g):
    return {group["name"] for group in g.optimizer.param_groups if group["params"][0] in g.optimizer.state}


@pytest.mark.parametrize("sh_degree,stateless", [(0, ()), (3, ()), (3, ("f_rest", "rgb"))])
def test_prune_some_rows(lib, sh_degree, stateless):
    g, ref = _pair(_model(257, sh_degree, stateless))
    assert _stateful(g) == set(gm._GROUPS) - set(stateless)
    mask_ref, mask = ref.prune(0.005, 1.3, 100.0), g.prune(0.005, 1.3, 100.0)
    assert lib.calls == ["prune_mask", "work_bytes", "plan", "rows"]
    assert torch.equal(mask, mask_ref) and 20 < int(mask.sum()) < 237
    assert g._features_rest.shape == (257 - int(mask.sum()), (sh_degree + 1) ** 2 - 1, 3)
    assert _stateful(g) == set(gm._GROUPS) - set(stateless)
    _check_same(g, ref)
    assert g.generation == 1 and len(g._surgery_keepalive) == 3


def test_prune_none_leaves_every_tensor_in_place(lib):
    g, ref = _pair(_model(257, 3))
    before = [getattr(g, a) for a in PARAMS + STATS] + [g.optimizer.state[g._xyz]["exp_avg"]]
    mask_ref, mask = ref.prune(0.0, 1e9, None), g.prune(0.0, 1e9, None)
    assert lib.calls == ["prune_mask", "work_bytes", "plan"]
    assert not mask.any() and not mask_ref.any()
    assert all(a is b for a, b in zip(before, [getattr(g, a) for a in PARAMS + STATS] + [g.optimizer.state[g._xyz]["exp_avg"]]))
    assert g.generation == 0
    _check_same(g, ref)


@pytest.mark.parametrize("P", [257, 1])
def test_prune_all_installs_empty_tensors_without_a_row_launch(lib, P):
    g, ref = _pair(_model(P, 3))
    mask_ref, mask = ref.prune(2.0, 1.3, None), g.prune(2.0, 1.3, None)
    assert lib.calls == ["prune_mask", "work_bytes", "plan"]
    assert mask.all() and mask_ref.all()
    assert g._xyz.shape == (0, 3) and g._features_rest.shape == (0, 15, 3) and g.max_radii2D.shape == (0,) and g.denom.shape == (0, 1)
    assert g.optimizer.state[g._rotation]["exp_avg_sq"].shape == (0, 4)
    _check_same(g, ref)
    assert g.generation == 1


def test_a_single_row_that_is_kept(lib):
    g, ref = _pair(_model(1, 0))
    xyz = g._xyz
    ref.prune(0.0, 1e9, None)
    g.prune(0.0, 1e9, None)
    assert g._xyz is xyz and g._xyz.shape == (1, 3) and g.generation == 0
    _check_same(g, ref)


def _frame(H, W, pixels):
    mask = torch.zeros(H * W, dtype=torch.bool)
    mask[pixels] = True
    return torch.rand(3, H, W), torch.rand(H, W) + 1.0, mask.reshape(H, W), torch.tensor([1.0, 0, 0, 0, 0, 0, 0])


def _seed_both(g, ref, frame, pixels):
    """seed_device on g; on ref, densification_postfix fed the rows the stand-in writes: the raster index of every masked pixel."""
    n = g.seed_device(*frame, 10.0, 10.0, 2.0, 2.5)
    assert n == len(pixels)
    row = torch.tensor(sorted(pixels), dtype=torch.float32)
    ref.densification_postfix(*(row.reshape((n,) + (1,) * (getattr(ref, a).dim() - 1)).expand((n,) + tuple(getattr(ref, a).shape[1:]))
                                for a in PARAMS))
    return n


@pytest.mark.parametrize("sh_degree", [0, 3])
def test_seed_an_empty_map_then_behind_its_rows_then_nothing(lib, sh_degree):
    g, ref = _pair(_model(0, sh_degree))
    first = [1, 2, 5, 9, 12, 18, 19]
    assert _seed_both(g, ref, _frame(4, 5, first), first) == 7
    assert lib.calls == ["work_bytes", "plan", "seed"]
    assert g._xyz.detach()[:, 0].tolist() == [float(i) for i in first] and g._features_rest.shape == (7, (sh_degree + 1) ** 2 - 1, 3)
    assert not _stateful(g)
    _check_same(g, ref)
    # moments, a pending gradient and non-zero statistics on both, then seven rows become eleven
    for m in (g, ref):
        for i, group in enumerate(m.optimizer.param_groups):
            group["params"][0].grad = torch.full_like(group["params"][0], 1.0 + i)
        m.optimizer.step()
        for attr in STATS:
            getattr(m, attr).add_(1.0)
    old = {a: getattr(g, a).detach().clone() for a in PARAMS}
    old_m = g.optimizer.state[g._xyz]["exp_avg"].clone()
    second = [0, 7, 8, 19]
    del lib.calls[:]
    assert _seed_both(g, ref, _frame(4, 5, second), second) == 4
    assert lib.calls == ["work_bytes", "plan", "seed"]
    for a in PARAMS:
        assert torch.equal(getattr(g, a).detach()[:7], old[a]), a
    m = g.optimizer.state[g._xyz]["exp_avg"]
    assert torch.equal(m[:7], old_m) and float(m[:7].abs().min()) > 0 and not m[7:].any()
    for attr in STATS:
        assert getattr(g, attr).shape[0] == 11 and not getattr(g, attr).any(), attr
    assert _stateful(g) == set(gm._GROUPS)
    _check_same(g, ref)
    # an all-false mask: no seeding launch, the rebuild still happens
    xyz, generation = g._xyz, g.generation
    del lib.calls[:]
    assert _seed_both(g, ref, _frame(4, 5, []), []) == 0
    assert lib.calls == ["work_bytes", "plan"]
    assert g._xyz is not xyz and g.generation == generation + 1 and g._xyz.shape == (11, 3)
    _check_same(g, ref)


def test_restore_of_a_snapshot_after_a_prune(lib):
    g, _ = _pair(_model(257, 3, ("f_rest", "rgb")))
    want = copy.deepcopy(g)
    snap = g.snapshot()
    g.prune(0.005, 1.3, 100.0)
    for i, group in enumerate(g.optimizer.param_groups):
        group["lr"] = 0.5 + i
        group["params"][0].grad = torch.ones_like(group["params"][0])
    g.optimizer.step()                      # every group has state now, and another step count
    assert g._xyz.shape[0] < 257 and _stateful(g) == set(gm._GROUPS)
    generation = g.generation
    g.restore(snap)
    assert g.generation == generation + 1
    want.generation = g.generation
    _check_same(g, want)
    assert _stateful(g) == set(gm._GROUPS) - {"f_rest", "rgb"}
    g._xyz.data.add_(1.0)                   # the snapshot stays valid: it shares no memory with the restored model
    assert torch.equal(snap["groups"][0][1], want._xyz.detach())


def test_replace_tensor_to_optimizer_is_the_walk_of_one_group():
    g = _model(33, 3, ("rgb",))
    before = {a: getattr(g, a) for a in PARAMS + STATS}
    step = float(g.optimizer.state[g._opacity]["step"])
    new = torch.full((33, 1), -2.0)
    out = g.replace_tensor_to_optimizer(new, "opacity")
    assert list(out) == ["opacity"] and out["opacity"] is g.optimizer.param_groups[3]["params"][0] is g._opacity
    assert torch.equal(g._opacity.detach(), new) and g.generation == 1
    st = g.optimizer.state[g._opacity]
    assert float(st["step"]) == step and not st["exp_avg"].any() and not st["exp_avg_sq"].any() and st["exp_avg"].shape == (33, 1)
    for a in PARAMS + STATS:
        if a != "_opacity":
            assert getattr(g, a) is before[a], a
    assert _stateful(g) == set(gm._GROUPS) - {"rgb"} and before["_opacity"] not in g.optimizer.state
    assert g._opacity.is_leaf and g._opacity.requires_grad and g._opacity.grad is None
    g.replace_tensor_to_optimizer(torch.zeros(33, 3), "rgb")          # a group without Adam state gets none
    assert "rgb" not in _stateful(g)
