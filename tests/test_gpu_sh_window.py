"""The multi-GPU mapping window natively at an ACTIVE SH degree (ABI 212) on the HIP kernels: mm3dgs_slam_adam_project with the sixth Adam
group and the SH projection from the stepped f_rest rows, and the native window loops at SH 2 (fused against two-call steps, two gloo ranks,
RCCL with one rank).  Sizes of the existing window tests: 120x160, 6000 Gaussians, seed 6."""
import ctypes as C
import os
import random
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"default": {}, "python_sh": {"convert_SHs_python": True}, "world_means": {"transform_means_python": False}}
LRS = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=2.5e-3 / 20, opacity=5e-2, scaling=1e-3, rotation=1e-3)
NAMES = ("xyz", "f_dc", "opacity", "scaling", "rotation")


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


# ---- 5. the C ABI ----------------------------------------------------------------------------------------------------------------------
def _model(mode, n_rest, P=6000, H=120, W=160, seed=6):
    from mm3dgs_slam_amd import synthetic as syn
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.gaussian_model import GaussianModel
    from mm3dgs_slam_amd.renderer import Renderer
    max_deg = {8: 2, 15: 3}[n_rest]
    cfg = default_config(device=DEV, height=H, width=W, pipeline=dict(MODES[mode]), mapping={"sh_degree": max_deg})
    c = cfg["cam"]
    color, depth = syn.rgbd_frame(H, W, seed=seed)
    G = syn.seed_gaussians(color, depth, c["fx"], c["fy"], c["cx"], c["cy"], P, seed=seed, isotropic=False)
    g = GaussianModel(cfg)
    g.training_setup()
    gen = torch.Generator().manual_seed(seed + 11)
    G["scaling"] = G["scaling"] + torch.tensor([0.6, -0.4, 0.0])
    g.densification_postfix(G["xyz"].to(DEV), G["f_dc"].to(DEV), (0.25 * torch.randn(P, n_rest, 3, generator=gen)).to(DEV),
                            (torch.randn(P, 1, generator=gen) * 1.2).to(DEV), G["scaling"].to(DEV),
                            (G["rotation"] * (0.5 + torch.rand(P, 1, generator=gen))).to(DEV), G["rgb"].to(DEV))
    g.active_sh_degree = 2
    pose = torch.tensor([0.995, 0.03, -0.02, 0.04, 0.03, -0.02, 0.05], device=DEV) * 1.3
    pose[4:] /= 1.3
    return cfg, g, Renderer(cfg), pose, color.to(DEV)


def _params(g):
    return dict(xyz=g._xyz, f_dc=g._features_dc, f_rest=g._features_rest, opacity=g._opacity, scaling=g._scaling, rotation=g._rotation)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n_rest", [8, 15])
def test_adam_project_at_sh_two_equals_adam_then_the_projecting_map_call(n_rest, mode, masked):
    """One mm3dgs_slam_adam_project call at sh_degree 2 (P = 6000, not a multiple of 256) against mm3dgs_adam over the same arrays (the six
    groups) followed by a self-projecting mm3dgs_slam_map call: it returns 0, parameters and moments of all six groups bit for bit (n_rest 15:
    the inactive rows' nonzero moments decay), the radii and the next mm3dgs_slam_map call's output (MM3DGS_FWD_PROJECTED) bit for bit.  A call
    without d_f_rest or without the rest Adam group returns -2 and leaves the parameters untouched."""
    from mm3dgs_slam_amd import _lib
    from mm3dgs_slam_amd.fused import FusedEngine, _loss_cfg, _p, _stream
    cfg, g, R, pose, color = _model(mode, n_rest)
    P = int(g._xyz.shape[0])
    assert P % 256 != 0
    eng = FusedEngine(R)
    eng.forward(pose, g, need_grads=True)
    assert eng.check_capacity()
    eng.forward(pose, g, need_grads=True)
    assert eng.can_adam_project(g) and eng.flat_width == 14 + 3 * n_rest and eng.grads["f_rest"].shape == (P, n_rest, 3)
    gen = torch.Generator(device=DEV).manual_seed(7)
    prm = _params(g)
    with torch.no_grad():
        eng.flat.normal_(generator=gen).mul_(1e-3)
        eng.grads["f_rest"][:, 8:] = 0.0          # (mm3dgs_slam_map writes zero rows beyond the active degree)
        moments = {k: (torch.randn(p.shape, device=DEV, generator=gen) * 1e-3, torch.rand(p.shape, device=DEV, generator=gen) * 1e-6) for k, p in prm.items()}
    mask = (torch.rand(P, device=DEV, generator=gen) < 0.7).to(torch.uint8) if masked else None
    grads0, params0 = eng.flat.clone(), {k: p.detach().clone() for k, p in prm.items()}
    next_pose = (pose + torch.tensor([0.0, 0.004, -0.003, 0.002, 0.01, -0.006, 0.004], device=DEV)).contiguous()
    lcfg = _loss_cfg(eng.H, eng.W, 0.8, 0.2, 0.0, 0, 0, 0, 0.5)
    step = 3

    def map_adam(rest=True):
        ma = _lib.Mm3dgsMapAdam()
        for i, n in enumerate(NAMES):
            ma.param[i], ma.exp_avg[i], ma.exp_avg_sq[i], ma.lr[i] = prm[n].data_ptr(), moments[n][0].data_ptr(), moments[n][1].data_ptr(), LRS[n]
        if rest:
            ma.rest_param, ma.rest_exp_avg, ma.rest_exp_avg_sq, ma.rest_lr = prm["f_rest"].data_ptr(), moments["f_rest"][0].data_ptr(), moments["f_rest"][1].data_ptr(), LRS["f_rest"]
        ma.beta1, ma.beta2, ma.eps, ma.step = 0.9, 0.999, 1e-15, step
        if mask is not None:
            ma.opt_mask = mask.data_ptr()
        return ma

    def restore():
        with torch.no_grad():
            eng.flat.copy_(grads0)
            for k, p in prm.items():
                p.copy_(params0[k])
                moments[k][0].copy_(mom0[k][0]); moments[k][1].copy_(mom0[k][1])

    mom0 = {k: (m.clone(), v.clone()) for k, (m, v) in moments.items()}

    def raw_call(sg, ma):
        si = eng.inputs(next_pose, g)
        return eng.lib.mm3dgs_slam_adam_project(C.byref(eng.cam), P, C.byref(si), C.byref(sg), C.byref(ma), _p(eng.radii), _p(eng.geom), _p(eng.img_state),
                                                _p(eng.binning), eng.n_cap, eng._flags(), _stream())

    # missing pieces of the sixth group: -2, nothing launched
    sg = _lib.Mm3dgsSlamGrads()
    for i, n in enumerate(("d_xyz", "d_f_dc", "d_opacity", "d_scaling", "d_rotation")):
        setattr(sg, n, eng.grads[NAMES[i]].data_ptr())
    assert raw_call(sg, map_adam()) == -2                     # no d_f_rest
    sg.d_f_rest = eng.grads["f_rest"].data_ptr()
    assert raw_call(sg, map_adam(rest=False)) == -2           # no rest Adam group
    torch.cuda.synchronize()
    for k, p in prm.items():
        assert torch.equal(p, params0[k]), k
        assert torch.equal(moments[k][0], mom0[k][0]) and torch.equal(moments[k][1], mom0[k][1]), k

    # (1) the fused call, then the next view's map call marked projected
    assert raw_call(sg, map_adam()) == 0
    fused = ({k: p.detach().clone() for k, p in prm.items()}, {k: (m.clone(), v.clone()) for k, (m, v) in moments.items()}, eng.radii.clone())
    view = [(next_pose, color.contiguous(), None)]
    eng.map_loop(view, g, lcfg, None, None, grads=eng.grads, projected=True)
    assert eng.check_capacity()
    fused_next = (eng.out.clone(), eng.radii.clone(), eng.flat.clone())

    # (2) mm3dgs_adam over the same arrays (opt_mask multiplied into the gradients, as fused.py's two-call step does), then the map call
    restore()
    with torch.no_grad():
        if mask is not None:
            for t in eng.grads.values():
                t.mul_(mask.to(t.dtype).view(-1, *([1] * (t.dim() - 1))))
    table = (_lib.Mm3dgsAdamGroup * 8)()
    for j, n in enumerate(("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")):
        e = table[j]
        e.param, e.grad, e.exp_avg, e.exp_avg_sq = prm[n].data_ptr(), eng.grads[n].data_ptr(), moments[n][0].data_ptr(), moments[n][1].data_ptr()
        e.n, e.lr = prm[n].numel(), LRS[n]
    _lib.check(eng.lib.mm3dgs_adam(table, 6, step, 0.9, 0.999, 1e-15, _stream()))
    torch.cuda.synchronize()
    for k, p in prm.items():
        assert torch.equal(p, fused[0][k]), (k, float((p - fused[0][k]).abs().max()))
        assert torch.equal(moments[k][0], fused[1][k][0]) and torch.equal(moments[k][1], fused[1][k][1]), k
    if n_rest == 15:      # the inactive rows started from nonzero moments, and the step decayed them
        assert float(mom0["f_rest"][1][:, 8:].abs().min()) > 0
        assert bool((moments["f_rest"][1][:, 8:] < mom0["f_rest"][1][:, 8:]).all())
        assert bool(((moments["f_rest"][0][:, 8:].abs() < mom0["f_rest"][0][:, 8:].abs()) | (mom0["f_rest"][0][:, 8:] == 0)).all())
    eng.map_loop(view, g, lcfg, None, None, grads=eng.grads)
    assert eng.check_capacity()
    assert torch.equal(eng.radii, fused[2]) and torch.equal(eng.radii, fused_next[1])
    assert torch.equal(eng.out, fused_next[0])
    assert torch.equal(eng.flat, fused_next[2])


# ---- 6. / 7. the native window loops ---------------------------------------------------------------------------------------------------
def _slam(window, mode="default", ba=False, iters=8):
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device=DEV, height=120, width=160, pipeline=dict(MODES[mode]), tracking={"iters": 5},
                         mapping={"iters": iters, "kf_every": 1, "do_BA": ba, "sh_degree": 2})
    seq = SyntheticSequence(cfg, 3, 6000, seed=6)
    slam = SLAM(cfg, seq, window=window)
    slam.gaussians.active_sh_degree = 2
    assert type(slam.mapper).__name__ == "FusedMapper"
    return slam


def _watch(patch):
    """Record the engine's map calls with an f_rest gradient output and every entry into the torch-graph Mapper.optimize_map."""
    from mm3dgs_slam_amd import mapper
    from mm3dgs_slam_amd.fused import FusedEngine
    rec = {"rest_out": 0, "graph": 0}
    real_map, real_opt = FusedEngine.map_loop, mapper.Mapper.optimize_map

    def map_loop(self, views, g, *a, **k):
        grads = k.get("grads", a[3] if len(a) > 3 else None)
        if grads is not None and self.rest_grad(g) is not None:
            rec["rest_out"] += 1
        return real_map(self, views, g, *a, **k)

    def optimize_map(self, *a, **k):
        rec["graph"] += 1
        return real_opt(self, *a, **k)
    patch(FusedEngine, "map_loop", map_loop)
    patch(mapper.Mapper, "optimize_map", optimize_map)
    return rec


def _full_state(slam):
    g = slam.gaussians
    st = {"xyz": g._xyz, "op": g._opacity, "sc": g._scaling, "rot": g._rotation, "f_dc": g._features_dc, "f_rest": g._features_rest,
          "acc": g.xyz_gradient_accum, "radii": g.max_radii2D, "poses": torch.stack([p.detach() for p in slam.estimate_pose_list[:3]])}
    st = {k: v.detach().cpu().clone() for k, v in st.items()}
    for gr in g.optimizer.param_groups:
        s = g.optimizer.state.get(gr["params"][0], {})
        if "exp_avg" in s:
            st["m_" + gr["name"]], st["v_" + gr["name"]] = s["exp_avg"].cpu().clone(), s["exp_avg_sq"].cpu().clone()
    return st


@pytest.mark.parametrize("ba", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
def test_window_step_fused_with_the_next_projection_is_bit_identical_at_sh_two(mode, ba, monkeypatch):
    """tests/test_gpu_fused.py:464 at SH 2: WindowParallel(0, 1, batch=2), mm3dgs_slam_adam_project with the sixth group against mm3dgs_adam over
    the flat buffer + a self-projecting next call -- parameters (f_rest included), moments, statistics, poses bit for bit, >= 10 fused steps."""
    from mm3dgs_slam_amd.fused import FusedEngine, FusedMapper, _engine
    from mm3dgs_slam_amd.window_parallel import WindowParallel
    rec = _watch(monkeypatch.setattr)
    real = FusedEngine.adam_project
    n_fused, outs = [], []

    def counting(self, *a, **k):
        n_fused[-1] += 1
        return real(self, *a, **k)
    monkeypatch.setattr(FusedEngine, "adam_project", counting)
    for fuse in (True, False):
        monkeypatch.setattr(FusedMapper, "fuse_adam_project", fuse)
        monkeypatch.setattr(FusedMapper, "fuse_adam_project_sh", fuse)      # (the fused SH step is opt-in)
        n_fused.append(0)
        slam = _slam(WindowParallel(0, 1, batch=2), mode, ba)
        for i in range(3):
            slam.step(i)
        st = _full_state(slam)
        st["out"] = _engine(slam.renderer).out.cpu().clone()
        st["kf"] = torch.stack([kf.pose.detach().cpu() for kf in slam.mapper.keyframes])
        outs.append(st)
    assert rec["rest_out"] > 0 and rec["graph"] == 0, rec
    assert n_fused[0] >= 10 and n_fused[1] == 0, n_fused
    a, b = outs
    assert "m_f_rest" in a and float(a["f_rest"].abs().max()) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))


def _gloo_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)     # both ranks share the one GPU of the test box
    from mm3dgs_slam_amd.window_parallel import WindowParallel
    rec = _watch(setattr)
    slam = _slam(WindowParallel(rank, world), iters=6)
    for i in range(3):
        slam.step(i)
    st = _full_state(slam)
    st["rec"] = rec
    torch.save(st, os.path.join(out, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_at_sh_two_equal_native_window_batch_two(tmp_path, monkeypatch):
    """Two gloo ranks on this GPU at SH 2 (the native window: f_rest in the flat all-reduce and in the fused step): the ranks identical, and both
    equal to the single-process native window-batch-2 run at the bars of tests/test_gpu_fused.py:458-460 (f_rest at the means' bar)."""
    import torch.multiprocessing as mp
    from mm3dgs_slam_amd.window_parallel import WindowParallel
    mp.spawn(_gloo_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    for r in (a, b):
        rec = r.pop("rec")
        assert rec["rest_out"] > 0 and rec["graph"] == 0, rec
    for k in a:
        assert torch.equal(a[k], b[k]), k
    rec = _watch(monkeypatch.setattr)
    slam = _slam(WindowParallel(0, 1, batch=2), iters=6)
    for i in range(3):
        slam.step(i)
    assert rec["rest_out"] > 0 and rec["graph"] == 0, rec
    ref = _full_state(slam)
    assert ref["xyz"].shape == a["xyz"].shape and float(a["f_rest"].abs().max()) > 0
    assert torch.allclose(ref["xyz"], a["xyz"], rtol=1e-5, atol=1e-7), float((ref["xyz"] - a["xyz"]).abs().max())
    assert torch.allclose(ref["op"], a["op"], rtol=1e-5, atol=1e-6)
    assert torch.allclose(ref["acc"], a["acc"], rtol=1e-5, atol=1e-7)
    assert torch.allclose(ref["f_rest"], a["f_rest"], rtol=1e-5, atol=1e-7), float((ref["f_rest"] - a["f_rest"]).abs().max())


# ---- 8. RCCL with one rank ---------------------------------------------------------------------------------------------------------------
WORKER = r'''
import os, random, sys
import numpy as np
import torch
import torch.distributed as dist
sys.path.insert(0, sys.argv[1])
out = sys.argv[2]
os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = sys.argv[3]
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
from mm3dgs_slam_amd.config import default_config
from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
from mm3dgs_slam_amd.window_parallel import WindowParallel
from mm3dgs_slam_amd import fused, mapper
rec = {"rest_out": 0, "graph": 0}
real_map, real_opt = fused.FusedEngine.map_loop, mapper.Mapper.optimize_map
def map_loop(self, views, g, *a, **k):
    grads = k.get("grads", a[3] if len(a) > 3 else None)
    if grads is not None and self.rest_grad(g) is not None:
        rec["rest_out"] += 1
    return real_map(self, views, g, *a, **k)
def optimize_map(self, *a, **k):
    rec["graph"] += 1
    return real_opt(self, *a, **k)
fused.FusedEngine.map_loop, mapper.Mapper.optimize_map = map_loop, optimize_map
res = {}
runs = (("rccl", "allreduce", True, True), ("plain", None, True, True), ("unfused", "allreduce", False, True), ("sharded", "reduce_scatter", True, True),
        ("graph", "allreduce", True, False))
for name, opt, fuse, native in runs:
    window = None if opt is None else WindowParallel(0, 1, always_reduce=True, optimizer=opt)
    fused.FusedMapper.fuse_adam_project = fuse
    rec["rest_out"], rec["graph"] = 0, 0
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device="cuda:0", height=120, width=160, tracking={"iters": 5}, mapping={"iters": 8, "kf_every": 1, "sh_degree": 2})
    seq = SyntheticSequence(cfg, 3, 6000, seed=6)
    slam = SLAM(cfg, seq, window=window, native_loops=native)
    slam.gaussians.active_sh_degree = 2
    for i in range(3):
        slam.step(i)
    g = slam.gaussians
    r = {"xyz": g._xyz.detach().cpu(), "op": g._opacity.detach().cpu(), "sc": g._scaling.detach().cpu(), "f_rest": g._features_rest.detach().cpu(),
         "acc": g.xyz_gradient_accum.cpu(), "radii": g.max_radii2D.cpu(), "poses": torch.stack([p.detach().cpu() for p in slam.estimate_pose_list[:3]]),
         "sharded_steps": 0 if window is None else window.sharded_steps, "pose_errors": slam.pose_errors(), "rec": dict(rec)}
    for pname, p in (("xyz", g._xyz), ("f_rest", g._features_rest)):
        st_ = g.optimizer.state[p]
        r["m_" + pname], r["v_" + pname] = st_["exp_avg"].detach().cpu(), st_["exp_avg_sq"].detach().cpu()
    res[name] = r
res["backend"] = dist.get_backend()
torch.save(res, out)
dist.destroy_process_group()
'''


def test_native_sh_window_over_rccl_world_one(tmp_path):
    """The RCCL path (backend "nccl", world 1, collectives forced) at SH 2, as tests/test_gpu_rccl.py at degree 0: against the plain single-view
    native loop at that test's bars (f_rest among the arrays); the unfused all-reduce step against the sharded one bit for bit, f_rest moments
    included; the native window against the torch-graph window at the bars of tests/test_gpu_sh_modes.py:206-212."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    out = tmp_path / "res.pt"
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, str(script), ROOT, str(out), str(_free_port())], env=env, timeout=900, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    res = torch.load(out)
    assert res["backend"] == "nccl"
    for name in ("rccl", "plain", "unfused", "sharded"):
        assert res[name]["rec"]["graph"] == 0, (name, res[name]["rec"])
        assert name == "plain" or res[name]["rec"]["rest_out"] > 0, (name, res[name]["rec"])
    a, b = res["rccl"], res["plain"]
    assert a["xyz"].shape == b["xyz"].shape and a["xyz"].shape[0] > 0
    assert torch.allclose(a["poses"], b["poses"], rtol=1e-5, atol=1e-6), float((a["poses"] - b["poses"]).abs().max())
    for k in ("xyz", "op", "sc", "f_rest", "acc", "radii"):
        d = (a[k] - b[k]).abs()
        off = d > 1e-6 + 1e-5 * b[k].abs()
        print(k, float(off.float().mean()), float(d.max()), flush=True)
        assert float(off.float().mean()) <= 1e-3, (k, float(off.float().mean()), float(d.max()))
        assert float(d.max()) <= 0.2, (k, float(d.max()))
    u, sh = res["unfused"], res["sharded"]
    assert sh["sharded_steps"] > 0 and u["sharded_steps"] == 0
    for k in ("xyz", "op", "sc", "f_rest", "acc", "radii", "poses", "m_xyz", "v_xyz", "m_f_rest", "v_f_rest"):
        assert torch.equal(u[k], sh[k]), (k, float((u[k] - sh[k]).abs().max()))
    tg, nat = res["graph"], res["rccl"]
    assert tg["rec"]["graph"] > 0
    print("graph vs native", float((tg["poses"] - nat["poses"]).abs().max()), nat["pose_errors"], flush=True)
    assert (tg["poses"] - nat["poses"]).abs().max() < 4e-3
    assert tg["xyz"].shape == nat["xyz"].shape
    assert float(torch.linalg.norm(nat["xyz"] - tg["xyz"]) / torch.linalg.norm(tg["xyz"])) < 1e-3 and (tg["op"] - nat["op"]).abs().median() < 5e-2
    assert float(nat["f_rest"].abs().max()) > 0 and abs(float(tg["f_rest"].abs().mean()) - float(nat["f_rest"].abs().mean())) < 0.1 * float(tg["f_rest"].abs().mean()) + 1e-6
    assert nat["pose_errors"][1] < 0.01 and nat["pose_errors"][2] < 0.01, nat["pose_errors"]
