"""Scene state: the Gaussian map and its Adam optimiser (reference ``slam/gaussian_model.py``).

Same parameter set, activations, optimiser groups and group surgery as the reference so that the mapper loop reads the
same (file:line are into ``slam/gaussian_model.py``):
  parameters  _xyz[P,3] _features_dc[P,1,3] _features_rest[P,M-1,3] _opacity[P,1] _scaling[P,3] _rotation[P,4] _rgb[P,3]
  getters     exp / normalize / sigmoid / cat                                  (:108-137)
  optimiser   Adam(lr=0, eps=1e-15), one group per parameter, names xyz f_dc f_rest opacity scaling rotation rgb (:143-195)
  surgery     densification_postfix -> cat_tensors_to_optimizer (:418-487), prune -> prune_points -> _prune_optimizer
              (:380-417, :574-588): parameters are REPLACED by fresh ``nn.Parameter`` objects, so a gradient computed
              before the prune never reaches ``optimizer.step()`` (SURVEY.md section 3.3 -- reproduced on purpose)
  densify     densify_and_clone / densify_and_split / densify / densify_and_prune (:490-592), reset_opacity and
              replace_tensor_to_optimizer (:259-264, :360-378); the split samples come from general_utils.densify_normals
              (a stateless generator the device path reproduces) instead of torch.normal
  stats       max_radii2D, xyz_gradient_accum, denom; add_densification_stats (:594-598)
PLY import/export keeps the reference's attribute order (:205-257) with a dependency-free binary writer.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from .general_utils import (build_rotation, build_scaling_rotation, densify_normals, get_expon_lr_func, inverse_sigmoid,
                            strip_symmetric)

_GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "rgb")


def draw_densify_seed():
    """The seed of a densification without one: 31 bits from torch's global CPU generator (the reference's dependence on the global
    RNG, for direct callers; the mapping loops pass general_utils.densify_seed)."""
    return int(torch.randint(0, 2 ** 31, (1,)).item())


class GaussianModel:
    def __init__(self, cfg):
        self.cfg = cfg
        dev = cfg["device"]
        self.active_sh_degree = 0
        self.max_sh_degree = cfg["mapping"]["sh_degree"]
        n_rest = (self.max_sh_degree + 1) ** 2 - 1
        self._xyz = torch.empty(0, 3, device=dev)
        self._features_dc = torch.empty(0, 1, 3, device=dev)
        self._features_rest = torch.empty(0, n_rest, 3, device=dev)
        self._scaling = torch.empty(0, 3, device=dev)
        self._rotation = torch.empty(0, 4, device=dev)
        self._opacity = torch.empty(0, 1, device=dev)
        self._rgb = torch.empty(0, 3, device=dev)
        self.max_radii2D = torch.empty(0, device=dev)
        self.xyz_gradient_accum = torch.empty(0, 1, device=dev)
        self.denom = torch.empty(0, 1, device=dev)
        self.optimizer = None
        self.percent_dense = 0
        self.spatial_lr_scale = 0
        self.generation = 0        # bumped whenever the parameter tensors are replaced (prune / densify / restore)

    # ---- activations --------------------------------------------------------------------------------------------
    scaling_activation = staticmethod(torch.exp)
    scaling_inverse_activation = staticmethod(torch.log)
    opacity_activation = staticmethod(torch.sigmoid)
    inverse_opacity_activation = staticmethod(inverse_sigmoid)
    rotation_activation = staticmethod(torch.nn.functional.normalize)

    @property
    def get_scaling(self):
        return torch.exp(self._scaling)

    @property
    def get_rotation(self):
        return torch.nn.functional.normalize(self._rotation)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_rgb(self):
        return self._rgb

    @property
    def get_opacity(self):
        return torch.sigmoid(self._opacity)

    def get_covariance(self, scaling_modifier=1):
        L = build_scaling_rotation(scaling_modifier * self.get_scaling, self._rotation)
        return strip_symmetric(L @ L.transpose(1, 2))

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    # ---- optimiser ----------------------------------------------------------------------------------------------
    def _params(self):
        return dict(xyz=self._xyz, f_dc=self._features_dc, f_rest=self._features_rest, opacity=self._opacity,
                    scaling=self._scaling, rotation=self._rotation, rgb=self._rgb)

    def _assign(self, t):
        self._xyz, self._features_dc, self._features_rest = t["xyz"], t["f_dc"], t["f_rest"]
        self._opacity, self._scaling, self._rotation, self._rgb = t["opacity"], t["scaling"], t["rotation"], t["rgb"]

    def training_setup(self):
        m = self.cfg["mapping"]
        self.percent_dense = m["percent_dense"]
        self.spatial_lr_scale = m["spatial_lr_scale"]
        n, dev = self._xyz.shape[0], self.cfg["device"]
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        lrs = dict(xyz=m["position_lr_init"] * self.spatial_lr_scale, f_dc=m["feature_lr"], f_rest=m["feature_lr"] / 20.0,
                   opacity=m["opacity_lr"], scaling=m["scaling_lr"], rotation=m["rotation_lr"], rgb=m["rgb_lr"])
        params = {k: nn.Parameter(v.detach().clone().requires_grad_(True)) for k, v in self._params().items()}
        self._assign(params)
        self.optimizer = torch.optim.Adam([{"params": [params[k]], "lr": lrs[k], "name": k} for k in _GROUPS],
                                          lr=0.0, eps=1e-15)
        self.xyz_scheduler_args = get_expon_lr_func(lr_init=m["position_lr_init"] * self.spatial_lr_scale,
                                                    lr_final=m["position_lr_final"] * self.spatial_lr_scale,
                                                    lr_delay_mult=m["position_lr_delay_mult"],
                                                    max_steps=m["position_lr_max_steps"])

    def update_learning_rate(self, iteration):
        for group in self.optimizer.param_groups:
            if group["name"] == "xyz":
                group["lr"] = self.xyz_scheduler_args(iteration)
                return group["lr"]

    def _rebuild_groups(self, transform_param, transform_state):
        """Replace every group's parameter by ``transform_param(old)`` (a new leaf) and carry the Adam moments
        through ``transform_state`` -- the reference's cat/prune surgery."""
        out = {}
        self.generation += 1
        for group in self.optimizer.param_groups:
            old = group["params"][0]
            state = self.optimizer.state.pop(old, None)
            new = nn.Parameter(transform_param(group["name"], old.detach()).requires_grad_(True))
            if state is not None and "exp_avg" in state:
                state["exp_avg"] = transform_state(group["name"], state["exp_avg"])
                state["exp_avg_sq"] = transform_state(group["name"], state["exp_avg_sq"])
                self.optimizer.state[new] = state
            group["params"][0] = new
            out[group["name"]] = new
        return out

    # ---- snapshot / restore (overflow recovery of the native mapping loop, fused.py) -----------------------------------
    def snapshot(self):
        """Copies of everything a mapping loop mutates: parameters, Adam moments and step counters, learning rates, the
        densification statistics.  ~24 device copies (26 MB at 150 k Gaussians)."""
        groups = []
        for group in self.optimizer.param_groups:
            p = group["params"][0]
            st = self.optimizer.state.get(p, {})
            groups.append((group["name"], p.detach().clone(), {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}, group["lr"]))
        return dict(groups=groups, stats=(self.xyz_gradient_accum.clone(), self.denom.clone(), self.max_radii2D.clone()))

    def restore(self, snap):
        """Back to a ``snapshot()`` (which stays valid: tensors are copied again)."""
        by_name = {name: (p, st, lr) for name, p, st, lr in snap["groups"]}
        out = {}
        self.generation += 1
        for group in self.optimizer.param_groups:
            self.optimizer.state.pop(group["params"][0], None)
            p, st, lr = by_name[group["name"]]
            new = nn.Parameter(p.clone().requires_grad_(True))
            if st:
                self.optimizer.state[new] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
            group["params"][0] = new
            group["lr"] = lr
            out[group["name"]] = new
        self._assign(out)
        self.xyz_gradient_accum, self.denom, self.max_radii2D = (t.clone() for t in snap["stats"])

    # ---- device-side surgery (csrc/compact.hip through the C ABI; CUDA tensors only) ---------------------------------------
    def _native(self):
        return str(self.cfg["device"]).startswith("cuda")

    def prune_mask_device(self, min_opacity, extent, max_screen_size=None, counter_ptr=None):
        """The pruning predicate of ``prune`` evaluated by one kernel: returns the uint8 keep mask; the number of pruned
        Gaussians is ADDED to the device word at ``counter_ptr`` (no host synchronisation)."""
        import ctypes as C
        from . import _lib
        from .rasterizer import _stream
        lib = _lib.load()
        P = int(self._xyz.shape[0])
        keep = torch.empty(P, dtype=torch.uint8, device=self._xyz.device)
        if counter_ptr is None:
            self._prune_counter = torch.zeros(1, dtype=torch.int32, device=self._xyz.device)
            counter_ptr = self._prune_counter.data_ptr()
        radii = self.max_radii2D if max_screen_size is not None else None
        _lib.check(lib.mm3dgs_prune_mask(P, C.c_void_p(self._opacity.data_ptr()), C.c_void_p(self._scaling.data_ptr()),
                                         C.c_void_p(radii.data_ptr()) if radii is not None else None, float(min_opacity), float(0.1 * extent),
                                         float(max_screen_size if max_screen_size is not None else 0.0), C.c_void_p(keep.data_ptr()),
                                         C.c_void_p(counter_ptr), _stream()))
        return keep

    def compact_device(self, keep):
        """``prune_points(~keep)`` with the order-preserving compaction kernels: one plan (counts + scan), ONE 4-byte read-back
        for the new size, one scatter launch over every parameter, Adam moment and statistic (instead of a nonzero and ~24
        index_select launches).  Nothing to prune leaves every tensor in place, like ``prune_points``."""
        import ctypes as C
        from . import _lib
        from .rasterizer import _stream
        lib = _lib.load()
        P = int(keep.shape[0])
        dev = keep.device
        work = torch.empty(lib.mm3dgs_compact_work_bytes(P), dtype=torch.uint8, device=dev)
        n_keep = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.mm3dgs_compact_plan(P, C.c_void_p(keep.data_ptr()), C.c_void_p(work.data_ptr()), C.c_void_p(n_keep.data_ptr()), _stream()))
        n = int(n_keep.item())
        if n == P:
            for group in self.optimizer.param_groups:
                group["params"][0].grad = None
            return
        pairs = []                      # (old tensor, new tensor)

        def moved(t):
            new = torch.empty((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
            pairs.append((t.detach(), new))
            return new
        out = {}
        self.generation += 1
        for group in self.optimizer.param_groups:
            old = group["params"][0]
            state = self.optimizer.state.pop(old, None)
            new = nn.Parameter(moved(old).requires_grad_(True))
            if state is not None and "exp_avg" in state:
                state["exp_avg"], state["exp_avg_sq"] = moved(state["exp_avg"]), moved(state["exp_avg_sq"])
                self.optimizer.state[new] = state
            group["params"][0] = new
            out[group["name"]] = new
        self._assign(out)
        self.xyz_gradient_accum, self.denom, self.max_radii2D = moved(self.xyz_gradient_accum), moved(self.denom), moved(self.max_radii2D)
        table = (_lib.Mm3dgsCompactArray * 32)()
        k = 0
        for old, new in pairs:
            w = int(old[0].numel()) if old.shape[0] > 0 else 0
            if w == 0:
                continue
            table[k].src, table[k].dst, table[k].width = old.data_ptr(), new.data_ptr(), w
            k += 1
        if n == 0:
            return      # every Gaussian pruned: the empty tensors are in place (their data_ptr() is NULL, nothing to move)
        _lib.check(lib.mm3dgs_compact_rows(P, C.c_void_p(keep.data_ptr()), C.c_void_p(work.data_ptr()), table, k, _stream()))
        self._surgery_keepalive = (pairs, keep, work)      # the launch is asynchronous

    def seed_device(self, color, depth, mask, pose, fx, fy, cx, cy):
        """``densification_postfix`` with the rows of the new Gaussians written by the seeding kernel: one Gaussian per pixel of
        ``mask`` (bool [H,W], raster order), initialised as slam/mapper.py:437-474,644-668 do.  Returns the number added."""
        import ctypes as C
        from . import _lib
        from .rasterizer import _stream
        lib = _lib.load()
        dev = depth.device
        H, W = depth.shape
        keep = mask.reshape(-1).to(torch.uint8).contiguous()
        work = torch.empty(lib.mm3dgs_compact_work_bytes(H * W), dtype=torch.uint8, device=dev)
        n_new = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.mm3dgs_compact_plan(H * W, C.c_void_p(keep.data_ptr()), C.c_void_p(work.data_ptr()), C.c_void_p(n_new.data_ptr()), _stream()))
        n = int(n_new.item())           # (a keyframe event: the new size must be known to allocate)
        P = int(self._xyz.shape[0])

        def grown(t, zero_tail):
            new = (torch.zeros if zero_tail else torch.empty)((P + n,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
            if P:
                new[:P].copy_(t.detach())
            return new
        out = {}
        self.generation += 1
        for group in self.optimizer.param_groups:
            old = group["params"][0]
            state = self.optimizer.state.pop(old, None)
            new = nn.Parameter(grown(old, False).requires_grad_(True))
            if state is not None and "exp_avg" in state:
                state["exp_avg"], state["exp_avg_sq"] = grown(state["exp_avg"], True), grown(state["exp_avg_sq"], True)
                self.optimizer.state[new] = state
            group["params"][0] = new
            out[group["name"]] = new
        self._assign(out)
        so = _lib.Mm3dgsSeedOutputs()
        so.xyz, so.f_dc, so.f_rest = self._xyz.data_ptr(), self._features_dc.data_ptr(), self._features_rest.data_ptr()
        so.opacity, so.scaling, so.rotation, so.rgb = self._opacity.data_ptr(), self._scaling.data_ptr(), self._rotation.data_ptr(), self._rgb.data_ptr()
        color, depth, pose = color.contiguous().float(), depth.contiguous().float(), pose.detach().contiguous().float()
        if n:
            _lib.check(lib.mm3dgs_seed_gaussians(H, W, C.c_void_p(color.data_ptr()), C.c_void_p(depth.data_ptr()), C.c_void_p(keep.data_ptr()),
                                                 C.c_void_p(work.data_ptr()), C.c_void_p(pose.data_ptr()), float(fx), float(fy), float(cx), float(cy),
                                                 P, C.byref(so), int(self._features_rest.shape[1]), _stream()))
        self.xyz_gradient_accum = torch.zeros((P + n, 1), device=dev)
        self.denom = torch.zeros((P + n, 1), device=dev)
        self.max_radii2D = torch.zeros((P + n,), device=dev)
        self._surgery_keepalive = (keep, work, color, depth, pose)
        return n

    def densify_device(self, max_grad, extent, seed, N=2):
        """``densify`` (clone + split) with the kernels of csrc/compact.hip: one classify-and-plan pass (class byte per row and three
        order-preserving ranks), ONE 12-byte read-back of {n_keep, n_clone, n_split} to size the new tensors, one scatter launch
        that writes every destination row of every parameter, Adam moment and statistic.  Returns the parent row of every new row
        (int32), or None when nothing was selected (tensors left in place, gradients dropped, statistics zeroed)."""
        import ctypes as C
        from . import _lib
        from .rasterizer import _stream
        lib = _lib.load()
        P = int(self._xyz.shape[0])
        dev = self._xyz.device
        work = torch.empty(lib.mm3dgs_densify_work_bytes(P), dtype=torch.uint8, device=dev)
        counts = torch.empty(3, dtype=torch.int32, device=dev)
        _lib.check(lib.mm3dgs_densify_plan(P, C.c_void_p(self.xyz_gradient_accum.data_ptr()), C.c_void_p(self.denom.data_ptr()),
                                           C.c_void_p(self._scaling.data_ptr()), float(max_grad), float(self.percent_dense * extent),
                                           C.c_void_p(work.data_ptr()), C.c_void_p(counts.data_ptr()), _stream()))
        n_keep, n_clone, n_split = (int(v) for v in counts.tolist())
        if n_clone == 0 and n_split == 0:
            self._drop_grads_and_stats()
            return None
        n = n_keep + n_clone + N * n_split
        st = _lib.Mm3dgsDensifyState()
        keep = []

        def fresh(t):
            new = torch.empty((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
            keep.append(t)
            return new
        out = {}
        self.generation += 1
        for gi, group in enumerate(self.optimizer.param_groups):
            assert group["name"] == _GROUPS[gi]       # (the kernel finds xyz / scaling / rotation by position)
            old = group["params"][0].detach()
            state = self.optimizer.state.pop(group["params"][0], None)
            new = nn.Parameter(fresh(old).requires_grad_(True))
            e = st.group[gi]
            e.src, e.dst, e.width = old.data_ptr(), new.data_ptr(), int(old[0].numel()) if P else 0
            if state is not None and "exp_avg" in state:
                m, v = state["exp_avg"], state["exp_avg_sq"]
                state["exp_avg"], state["exp_avg_sq"] = fresh(m), fresh(v)
                e.m_src, e.m_dst, e.v_src, e.v_dst = m.data_ptr(), state["exp_avg"].data_ptr(), v.data_ptr(), state["exp_avg_sq"].data_ptr()
                self.optimizer.state[new] = state
            group["params"][0] = new
            out[group["name"]] = new
        self._assign(out)
        self.xyz_gradient_accum, self.denom, self.max_radii2D = fresh(self.xyz_gradient_accum), fresh(self.denom), fresh(self.max_radii2D)
        st.grad_accum, st.denom, st.max_radii2D = self.xyz_gradient_accum.data_ptr(), self.denom.data_ptr(), self.max_radii2D.data_ptr()
        parent = torch.empty(n, dtype=torch.int32, device=dev)
        st.parent = parent.data_ptr()
        _lib.check(lib.mm3dgs_densify_rows(P, C.c_void_p(work.data_ptr()), n_keep, n_clone, n_split, N, int(seed) & 0xFFFFFFFF, C.byref(st),
                                           _stream()))
        self._surgery_keepalive = (keep, work)      # the launch is asynchronous
        return parent

    def prune_points(self, mask):
        # ONE nonzero (one host sync) shared by the ~24 tensors instead of a boolean-mask gather (= nonzero + sync) per
        # tensor; nothing to prune (the common case in SLAM: two pruning steps per frame) leaves every tensor, parameter
        # object and Adam moment in place -- the same values the rebuild would produce
        idx = torch.nonzero(~mask, as_tuple=False).squeeze(1)
        if idx.numel() == mask.numel():
            # the rebuild would hand the optimiser fresh parameters WITHOUT gradients, which is what makes the reference's
            # optimizer.step() of a pruning iteration a no-op: keep that
            for group in self.optimizer.param_groups:
                group["params"][0].grad = None
            return
        self._assign(self._rebuild_groups(lambda n, p: p.index_select(0, idx), lambda n, s: s.index_select(0, idx)))
        self.xyz_gradient_accum = self.xyz_gradient_accum.index_select(0, idx)
        self.denom = self.denom.index_select(0, idx)
        self.max_radii2D = self.max_radii2D.index_select(0, idx)

    def densification_postfix(self, new_xyz, new_features_dc, new_features_rest, new_opacities, new_scaling,
                              new_rotation, new_rgb):
        ext = dict(xyz=new_xyz, f_dc=new_features_dc, f_rest=new_features_rest, opacity=new_opacities,
                   scaling=new_scaling, rotation=new_rotation, rgb=new_rgb)
        self._assign(self._rebuild_groups(lambda n, p: torch.cat((p, ext[n].to(p)), 0),
                                          lambda n, s: torch.cat((s, torch.zeros_like(ext[n]).to(s)), 0)))
        n, dev = self._xyz.shape[0], self.cfg["device"]
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        self.max_radii2D = torch.zeros((n,), device=dev)

    def prune(self, min_opacity, extent, max_screen_size=None, lazy_mask=False):
        """Returns the mask of the pruned Gaussians; lazy_mask: a zero-argument callable that produces it (the native loop only needs it
        under bundle adjustment, and an operator launched after the read-back delays the next run by its dispatch time)."""
        if self._native():
            # predicate, plan and compaction on the device (three small launches + a 4-byte read-back of the new size)
            keep = self.prune_mask_device(min_opacity, extent, max_screen_size)
            self.compact_device(keep)
            return (lambda: keep == 0) if lazy_mask else keep == 0
        mask = (self.get_opacity < min_opacity).squeeze(-1)
        big = self.get_scaling.max(dim=1).values > 0.1 * extent
        if max_screen_size is not None:
            big = torch.logical_or(big, self.max_radii2D > max_screen_size)
        mask = torch.logical_or(mask, big)
        self.prune_points(mask)
        return (lambda: mask) if lazy_mask else mask

    # ---- densification (slam/gaussian_model.py:490-592) ---------------------------------------------------------------------------
    def _drop_grads_and_stats(self):
        """densification_postfix with nothing to add: the tensors stay in place (same values as the rebuild), the gradients go (the
        rebuild would hand the optimiser fresh parameters without them) and the statistics are zeroed, as the postfix always does."""
        for group in self.optimizer.param_groups:
            group["params"][0].grad = None
        torch._foreach_zero_([self.xyz_gradient_accum, self.denom, self.max_radii2D])

    @torch.no_grad()
    def densify_and_clone(self, grads, grad_threshold, scene_extent):
        """Appends a copy of every row with |grad| >= grad_threshold and max scale <= percent_dense * scene_extent (:560-583).
        Returns the selection mask over the rows before the call."""
        sel = torch.norm(grads, dim=-1) >= grad_threshold
        sel = torch.logical_and(sel, self.get_scaling.max(dim=1).values <= self.percent_dense * scene_extent)
        if not bool(sel.any()):
            self._drop_grads_and_stats()
            return sel
        self.densification_postfix(self._xyz[sel], self._features_dc[sel], self._features_rest[sel], self._opacity[sel],
                                   self._scaling[sel], self._rotation[sel], self._rgb[sel])
        return sel

    @torch.no_grad()
    def densify_and_split(self, grads, grad_threshold, scene_extent, N=2, seed=None):
        """Replaces every row with grad >= grad_threshold and max scale > percent_dense * scene_extent (rows appended since `grads`
        was taken count as grad 0) by N children (:490-538): xyz = R(q) (exp(s) z) + xyz, scaling = log(exp(s) / (0.8 N)), the rest
        copied; children appended k-major after the existing rows, parents removed.  z = densify_normals(seed, parent rows, N) where
        the reference draws torch.normal; seed None takes one from torch's global generator.  Returns the selection mask."""
        n_init = self._xyz.shape[0]
        padded = torch.zeros((n_init,), device=self._xyz.device)
        padded[: grads.shape[0]] = grads.reshape(-1)
        sel = torch.logical_and(padded >= grad_threshold, self.get_scaling.max(dim=1).values > self.percent_dense * scene_extent)
        rows = torch.nonzero(sel, as_tuple=False).squeeze(1)
        if rows.numel() == 0:
            self._drop_grads_and_stats()
            return sel
        if seed is None:
            seed = draw_densify_seed()
        stds = self.get_scaling[sel].repeat(N, 1)
        samples = stds * densify_normals(seed, rows, N).to(stds.device)
        rots = build_rotation(self._rotation[sel]).repeat(N, 1, 1)
        new_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + self._xyz[sel].repeat(N, 1)
        new_scaling = torch.log(self.get_scaling[sel].repeat(N, 1) / (0.8 * N))
        self.densification_postfix(new_xyz.detach(), self._features_dc[sel].repeat(N, 1, 1), self._features_rest[sel].repeat(N, 1, 1),
                                   self._opacity[sel].repeat(N, 1), new_scaling.detach(), self._rotation[sel].repeat(N, 1),
                                   self._rgb[sel].repeat(N, 1))
        self.prune_points(torch.cat((sel, torch.zeros(N * rows.numel(), device=sel.device, dtype=torch.bool))))
        return sel

    def _densify_torch(self, max_grad, extent, seed, N=2):
        P0 = int(self._xyz.shape[0])
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        clone = self.densify_and_clone(grads, max_grad, extent)
        split = self.densify_and_split(grads, max_grad, extent, N=N, seed=seed)[:P0]
        if not bool(clone.any()) and not bool(split.any()):
            return None
        ar = torch.arange(P0, device=clone.device)
        return torch.cat((ar[~split], ar[clone], ar[split].repeat(N)))

    def densify(self, max_grad, extent, seed=None):
        """Clone, then split (:585-590), on the device for CUDA tensors.  Returns the parent row (index before the call) of every
        row after it, or None when nothing was added (the rows are then unchanged)."""
        if seed is None:
            seed = draw_densify_seed()
        if self._native():
            return self.densify_device(max_grad, extent, seed)
        return self._densify_torch(max_grad, extent, seed)

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, seed=None, lazy_mask=False):
        """densify, then prune (:590-592).  Returns (prune mask over the densified rows, parent rows or None -- see densify): a per-row
        mask m of the map before the call becomes ``carry_rows(m, parent, prune_mask)`` after it.  lazy_mask as in prune."""
        parent = self.densify(max_grad, extent, seed)
        # densification zeroed max_radii2D, so the screen-size clause of this prune cannot fire: the reference's behaviour, kept
        return self.prune(min_opacity, extent, max_screen_size, lazy_mask=lazy_mask), parent

    @staticmethod
    def carry_rows(mask, parent, prune_mask):
        """A per-row tensor of the map before densify_and_prune, on the rows after it: children inherit their parent's row."""
        if parent is not None:
            mask = mask.index_select(0, parent.to(torch.int64))
        return mask[~prune_mask]

    def replace_tensor_to_optimizer(self, tensor, name):
        """The group `name` gets `tensor` as a fresh parameter with zeroed Adam moments (:360-378)."""
        out = {}
        self.generation += 1
        for group in self.optimizer.param_groups:
            if group["name"] != name:
                continue
            state = self.optimizer.state.pop(group["params"][0], None)
            new = nn.Parameter(tensor.requires_grad_(True))
            if state is not None:
                state["exp_avg"] = torch.zeros_like(tensor)
                state["exp_avg_sq"] = torch.zeros_like(tensor)
                self.optimizer.state[new] = state
            group["params"][0] = new
            out[name] = new
        return out

    @torch.no_grad()
    def reset_opacity(self):
        """opacity = inverse_sigmoid(min(sigmoid(opacity), 0.01)), moments of the opacity group zeroed (:259-264).  No loop calls it
        (the reference has no call site)."""
        op = self.get_opacity.detach()
        self._opacity = self.replace_tensor_to_optimizer(inverse_sigmoid(torch.min(op, torch.ones_like(op) * 0.01)), "opacity")["opacity"]

    def add_densification_stats(self, viewspace_point_tensor, update_filter):
        self.xyz_gradient_accum[update_filter] += torch.norm(viewspace_point_tensor.grad[update_filter, :2], dim=-1,
                                                             keepdim=True)
        self.denom[update_filter] += 1

    # ---- PLY (reference attribute order, slam/gaussian_model.py:205-257) ------------------------------------------
    def construct_list_of_attributes(self):
        names = ["x", "y", "z", "nx", "ny", "nz"]
        names += [f"f_dc_{i}" for i in range(self._features_dc.shape[1] * self._features_dc.shape[2])]
        names += [f"f_rest_{i}" for i in range(self._features_rest.shape[1] * self._features_rest.shape[2])]
        names += ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]
        names += [f"rgb_{i}" for i in range(3)]
        return names

    def save_ply(self, path):
        f = lambda t: t.detach().float().cpu().numpy()
        xyz = f(self._xyz)
        cols = [xyz, np.zeros_like(xyz), f(self._features_dc.transpose(1, 2).flatten(1)),
                f(self._features_rest.transpose(1, 2).flatten(1)), f(self._opacity), f(self._scaling), f(self._rotation),
                f(self._rgb)]
        data = np.concatenate(cols, axis=1).astype("<f4")
        names = self.construct_list_of_attributes()
        assert data.shape[1] == len(names)
        header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {data.shape[0]}\n"
        header += "".join(f"property float {n}\n" for n in names) + "end_header\n"
        with open(path, "wb") as fh:
            fh.write(header.encode("ascii"))
            fh.write(data.tobytes())

    def load_ply(self, path):
        with open(path, "rb") as fh:
            names, count = [], 0
            while True:
                line = fh.readline().decode("ascii").strip()
                if line.startswith("element vertex"):
                    count = int(line.split()[-1])
                elif line.startswith("property float"):
                    names.append(line.split()[-1])
                elif line == "end_header":
                    break
            data = np.frombuffer(fh.read(count * len(names) * 4), dtype="<f4").reshape(count, len(names))
        col = {n: i for i, n in enumerate(names)}
        dev = self.cfg["device"]
        grab = lambda prefix: torch.tensor(data[:, [col[n] for n in names if n.startswith(prefix)]].copy(), device=dev)
        n_rest = (self.max_sh_degree + 1) ** 2 - 1
        self._xyz = torch.tensor(data[:, [col["x"], col["y"], col["z"]]].copy(), device=dev)
        self._features_dc = grab("f_dc_").reshape(count, 3, 1).transpose(1, 2).contiguous()
        self._features_rest = grab("f_rest_").reshape(count, 3, n_rest).transpose(1, 2).contiguous()
        self._opacity = torch.tensor(data[:, [col["opacity"]]].copy(), device=dev)
        self._scaling = grab("scale_")
        self._rotation = grab("rot_")
        self._rgb = grab("rgb_") if any(n.startswith("rgb_") for n in names) else torch.zeros(count, 3, device=dev)
        self.max_radii2D = torch.zeros((count,), device=dev)
        self.active_sh_degree = self.max_sh_degree
