"""Scene state: the Gaussian map and its Adam optimiser (reference ``slam/gaussian_model.py``).

Same parameter set, activations, optimiser groups and group surgery as the reference so that the mapper loop reads the
same (file:line are into ``slam/gaussian_model.py``):
  parameters  _xyz[P,3] _features_dc[P,1,3] _features_rest[P,M-1,3] _opacity[P,1] _scaling[P,3] _rotation[P,4] _rgb[P,3]
  getters     exp / normalize / sigmoid / cat                                  (:108-137)
  optimiser   Adam(lr=0, eps=1e-15), one group per parameter, names xyz f_dc f_rest opacity scaling rotation rgb (:143-195)
  surgery     densification_postfix -> cat_tensors_to_optimizer (:418-487), prune -> prune_points -> _prune_optimizer
              (:380-417, :574-588): parameters are REPLACED by fresh ``nn.Parameter`` objects, so a gradient computed
              before the prune never reaches ``optimizer.step()`` (SURVEY.md section 3.3 -- reproduced on purpose); every
              form of it, torch or device, is one walk: ``_rebuild_groups``
  densify     densify_and_clone / densify_and_split / densify / densify_and_prune (:490-592), reset_opacity and
              replace_tensor_to_optimizer (:259-264, :360-378); the split samples come from general_utils.densify_normals
              (a stateless generator the device path reproduces) instead of torch.normal
  stats       max_radii2D, xyz_gradient_accum, denom; add_densification_stats (:594-598)
PLY import/export keeps the reference's attribute order (:205-257) with a dependency-free binary writer.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
from torch import nn

from . import _lib
from .general_utils import (build_rotation, build_scaling_rotation, densify_normals, get_expon_lr_func, inverse_sigmoid,
                            strip_symmetric)
from .rasterizer import _ptr, _stream

_GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "rgb")
_ATTRS = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling",
              rotation="_rotation", rgb="_rgb")                     # optimiser group -> the model's attribute
_STATS = ("xyz_gradient_accum", "denom", "max_radii2D")          # the densification statistics: one row per Gaussian, like the groups


def _library():
    """The C ABI the device surgery calls.  With ``_stream`` the seam of this module: a CPU test replaces the two module attributes
    and runs the same host bookkeeping on host tensors."""
    return _lib.load()


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
        return {name: getattr(self, attr) for name, attr in _ATTRS.items()}

    def _assign(self, t):
        for name, tensor in t.items():
            setattr(self, _ATTRS[name], tensor)

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

    def _install(self, group, tensor, state):
        """`tensor` becomes the parameter of `group` and of the model: a fresh leaf that requires a gradient and has none (a gradient
        computed before the surgery never reaches ``optimizer.step()``), with `state` (None or empty: no
        Adam state) keyed by it and the old parameter's key gone."""
        self.optimizer.state.pop(group["params"][0], None)
        new = nn.Parameter(tensor.requires_grad_(True))
        if state:
            self.optimizer.state[new] = state
        group["params"][0] = new
        self._assign({group["name"]: new})
        return new

    def _rebuild_groups(self, remake, only=None):
        """Row surgery -- the reference's cat/prune surgery and every device form of it walk the optimiser's groups here and nowhere
        else.  ``remake(name, role, tensor)`` says what becomes of each tensor: role "param" for a group's parameter, "exp_avg" /
        "exp_avg_sq" for its Adam moments (a group without moments is not asked, and loses whatever state it had; the step counter
        stays with the moments), "stat" for the three statistics, `name` then being the attribute.  `only` restricts the walk to one
        group.  Bumps `generation`; returns the new parameters by group name."""
        out = {}
        self.generation += 1
        for group in self.optimizer.param_groups:
            name = group["name"]
            if only not in (None, name):
                continue
            old = group["params"][0]
            state = self.optimizer.state.get(old)
            tensor = remake(name, "param", old.detach())
            if state is not None and "exp_avg" in state:
                for role in ("exp_avg", "exp_avg_sq"):
                    state[role] = remake(name, role, state[role])
            else:
                state = None
            out[name] = self._install(group, tensor, state)
        for attr in _STATS:
            setattr(self, attr, remake(attr, "stat", getattr(self, attr)))
        return out

    def _drop_grads(self):
        """What a surgery that moves no row leaves of itself: the tensors stay in place (the values the rebuild would produce), the
        gradients go, because the rebuild would hand the optimiser fresh parameters without them."""
        for group in self.optimizer.param_groups:
            group["params"][0].grad = None

    # ---- snapshot / restore (overflow recovery of the native mapping loop, fused.py) -----------------------------------
    def snapshot(self):
        """Copies of everything a mapping loop mutates: parameters, Adam moments and step counters, learning rates, the
        densification statistics.  ~24 device copies (26 MB at 150 k Gaussians)."""
        groups = []
        for group in self.optimizer.param_groups:
            p = group["params"][0]
            st = self.optimizer.state.get(p, {})
            groups.append((group["name"], p.detach().clone(), {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}, group["lr"]))
        return dict(groups=groups, stats=tuple(getattr(self, attr).clone() for attr in _STATS))

    def restore(self, snap):
        """Back to a ``snapshot()`` (which stays valid: tensors are copied again).  Not a row surgery: whole state dicts (step counter
        included) and the learning rates come from the snapshot whatever the groups hold now, so it walks on its own and shares
        `_install` with `_rebuild_groups`."""
        by_name = {name: (p, st, lr) for name, p, st, lr in snap["groups"]}
        self.generation += 1
        for group in self.optimizer.param_groups:
            p, st, lr = by_name[group["name"]]
            self._install(group, p.clone(), {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()})
            group["lr"] = lr
        for attr, t in zip(_STATS, snap["stats"]):
            setattr(self, attr, t.clone())

    # ---- device-side surgery (csrc/compact.hip through the C ABI; CUDA tensors only) ---------------------------------------
    def _native(self):
        return str(self.cfg["device"]).startswith("cuda")

    def prune_mask_device(self, min_opacity, extent, max_screen_size=None, counter_ptr=None):
        """The pruning predicate of ``prune`` evaluated by one kernel: returns the uint8 keep mask; the number of pruned
        Gaussians is ADDED to the device word at ``counter_ptr`` (no host synchronisation)."""
        P = int(self._xyz.shape[0])
        keep = torch.empty(P, dtype=torch.uint8, device=self._xyz.device)
        if counter_ptr is None:
            self._prune_counter = torch.zeros(1, dtype=torch.int32, device=self._xyz.device)
            counter_ptr = self._prune_counter.data_ptr()
        radii = self.max_radii2D if max_screen_size is not None else None
        _lib.check(_library().mm3dgs_prune_mask(P, _ptr(self._opacity), _ptr(self._scaling), _ptr(radii), float(min_opacity),
                                                float(0.1 * extent), float(max_screen_size if max_screen_size is not None else 0.0),
                                                _ptr(keep), counter_ptr, _stream()))      # (a c_void_p parameter takes the address as it is)
        return keep

    def compact_device(self, keep):
        """``prune_points(~keep)`` with the order-preserving compaction kernels: one plan (counts + scan), ONE 4-byte read-back
        for the new size, one scatter launch over every parameter, Adam moment and statistic (instead of a nonzero and ~24
        index_select launches).  Nothing to prune leaves every tensor in place, like ``prune_points``."""
        P = int(keep.shape[0])
        lib, dev = _library(), keep.device
        work, n = self._plan_rows(lib, keep)
        if n == P:
            return self._drop_grads()      # nothing pruned: every tensor object stays, `generation` too, no table is built
        table, pairs = (_lib.Mm3dgsCompactArray * 32)(), []      # (24 arrays at most: 7 parameters, 14 moments, 3 statistics)

        def moved(name, role, t):
            new = torch.empty((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
            width = int(t[0].numel())          # (P > n >= 0: there is a row 0)
            if width:                          # a zero-width array (f_rest at SH degree 0) has no bytes to move and stays out
                e = table[len(pairs)]
                e.src, e.dst, e.width = t.data_ptr(), new.data_ptr(), width
                pairs.append((t, new))
            return new
        self._rebuild_groups(moved)
        if n == 0:
            return      # every Gaussian pruned: the empty tensors are in place (their data_ptr() is NULL, nothing to move)
        _lib.check(lib.mm3dgs_compact_rows(P, _ptr(keep), _ptr(work), table, len(pairs), _stream()))
        self._surgery_keepalive = (pairs, keep, work)      # the launch is asynchronous

    @staticmethod
    def _plan_rows(lib, keep):
        """The plan of an order-preserving compaction by the uint8 mask `keep` (counts + scan into the work buffer the row kernels
        read) and its ONE 4-byte read-back.  Returns (work buffer, number of rows kept)."""
        work = torch.empty(lib.mm3dgs_compact_work_bytes(keep.shape[0]), dtype=torch.uint8, device=keep.device)
        n_keep = torch.zeros(1, dtype=torch.int32, device=keep.device)
        _lib.check(lib.mm3dgs_compact_plan(keep.shape[0], _ptr(keep), _ptr(work), _ptr(n_keep), _stream()))
        return work, int(n_keep.item())

    def seed_device(self, color, depth, mask, pose, fx, fy, cx, cy):
        """``densification_postfix`` with the rows of the new Gaussians written by the seeding kernel: one Gaussian per pixel of
        ``mask`` (bool [H,W], raster order), initialised as slam/mapper.py:437-474,644-668 do.  Returns the number added."""
        lib, dev = _library(), depth.device
        H, W = depth.shape
        keep = mask.reshape(-1).to(torch.uint8).contiguous()
        work, n = self._plan_rows(lib, keep)           # (a keyframe event: the new size must be known to allocate)
        P = int(self._xyz.shape[0])

        def grown(name, role, t):
            # parameters: the kernel writes the tail; moments: zero tail; statistics: zeros, not carried (as densification_postfix)
            new = (torch.empty if role == "param" else torch.zeros)((P + n,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
            if P and role != "stat":       # (an empty map: nothing is copied from the old tensors)
                new[:P].copy_(t)
            return new
        # n == 0 still rebuilds (fresh parameter objects, generation bumped), as densification_postfix with empty extensions does
        self._rebuild_groups(grown)
        so = _lib.Mm3dgsSeedOutputs()
        for name, attr in _ATTRS.items():
            setattr(so, name, getattr(self, attr).data_ptr())
        color, depth, pose = color.contiguous().float(), depth.contiguous().float(), pose.detach().contiguous().float()
        if n:
            _lib.check(lib.mm3dgs_seed_gaussians(H, W, _ptr(color), _ptr(depth), _ptr(keep), _ptr(work), _ptr(pose), float(fx), float(fy),
                                                 float(cx), float(cy), P, C.byref(so), int(self._features_rest.shape[1]), _stream()))
        self._surgery_keepalive = (keep, work, color, depth, pose)      # the launch is asynchronous
        return n

    def densify_device(self, max_grad, extent, seed, N=2):
        """``densify`` (clone + split) with the kernels of csrc/compact.hip: one classify-and-plan pass (class byte per row and three
        order-preserving ranks), ONE 12-byte read-back of {n_keep, n_clone, n_split} to size the new tensors, one scatter launch
        that writes every destination row of every parameter, Adam moment and statistic.  Returns the parent row of every new row
        (int32), or None when nothing was selected (tensors left in place, gradients dropped, statistics zeroed)."""
        lib, dev = _library(), self._xyz.device
        P = int(self._xyz.shape[0])
        work = torch.empty(lib.mm3dgs_densify_work_bytes(P), dtype=torch.uint8, device=dev)
        counts = torch.empty(3, dtype=torch.int32, device=dev)
        _lib.check(lib.mm3dgs_densify_plan(P, _ptr(self.xyz_gradient_accum), _ptr(self.denom), _ptr(self._scaling), float(max_grad),
                                           float(self.percent_dense * extent), _ptr(work), _ptr(counts), _stream()))
        n_keep, n_clone, n_split = (int(v) for v in counts.tolist())
        if n_clone == 0 and n_split == 0:
            self._drop_grads_and_stats()
            return None
        n = n_keep + n_clone + N * n_split
        # the kernel finds xyz / scaling / rotation by their position in Mm3dgsDensifyState.group
        assert tuple(group["name"] for group in self.optimizer.param_groups) == _GROUPS
        st = _lib.Mm3dgsDensifyState()
        fields = dict(param=("src", "dst"), exp_avg=("m_src", "m_dst"), exp_avg_sq=("v_src", "v_dst"))
        old = []

        def fresh(name, role, t):
            new = torch.empty((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
            old.append(t)
            if role != "stat":
                e = st.group[_GROUPS.index(name)]           # (the moment pointers of a group without moments stay NULL)
                setattr(e, fields[role][0], t.data_ptr())
                setattr(e, fields[role][1], new.data_ptr())
                if role == "param":
                    e.width = int(t[0].numel()) if P else 0
            return new
        self._rebuild_groups(fresh)
        st.grad_accum, st.denom, st.max_radii2D = (getattr(self, attr).data_ptr() for attr in _STATS)      # (destinations only)
        parent = torch.empty(n, dtype=torch.int32, device=dev)
        st.parent = parent.data_ptr()
        _lib.check(lib.mm3dgs_densify_rows(P, _ptr(work), n_keep, n_clone, n_split, N, int(seed) & 0xFFFFFFFF, C.byref(st), _stream()))
        self._surgery_keepalive = (old, work)      # the launch is asynchronous
        return parent

    def prune_points(self, mask):
        # ONE nonzero (one host sync) shared by the ~24 tensors instead of a boolean-mask gather (= nonzero + sync) per
        # tensor; nothing to prune (the common case in SLAM: two pruning steps per frame) leaves every tensor, parameter
        # object and Adam moment in place -- the same values the rebuild would produce
        idx = torch.nonzero(~mask, as_tuple=False).squeeze(1)
        if idx.numel() == mask.numel():
            return self._drop_grads()
        self._rebuild_groups(lambda name, role, t: t.index_select(0, idx))

    def densification_postfix(self, new_xyz, new_features_dc, new_features_rest, new_opacities, new_scaling,
                              new_rotation, new_rgb):
        ext = dict(xyz=new_xyz, f_dc=new_features_dc, f_rest=new_features_rest, opacity=new_opacities,
                   scaling=new_scaling, rotation=new_rotation, rgb=new_rgb)
        n, dev = self._xyz.shape[0] + new_xyz.shape[0], self.cfg["device"]

        def extended(name, role, t):
            if role == "stat":          # zeros at the new length, not carried
                return torch.zeros((n,) + tuple(t.shape[1:]), device=dev)
            return torch.cat((t, (ext[name] if role == "param" else torch.zeros_like(ext[name])).to(t)), 0)
        self._rebuild_groups(extended)

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
        self._drop_grads()
        torch._foreach_zero_([getattr(self, attr) for attr in _STATS])

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
        """The group `name` gets `tensor` as a fresh parameter with zeroed Adam moments (:360-378): the walk restricted to one group,
        the rows and with them the statistics staying as they are.  Returns {name: the new parameter}."""
        def replaced(_, role, t):
            if role == "stat":
                return t
            return tensor if role == "param" else torch.zeros_like(tensor)
        return self._rebuild_groups(replaced, only=name)

    @torch.no_grad()
    def reset_opacity(self):
        """opacity = inverse_sigmoid(min(sigmoid(opacity), 0.01)), moments of the opacity group zeroed (:259-264).  No loop calls it
        (the reference has no call site)."""
        op = self.get_opacity.detach()
        self.replace_tensor_to_optimizer(inverse_sigmoid(torch.min(op, torch.ones_like(op) * 0.01)), "opacity")

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
