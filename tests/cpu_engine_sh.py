"""TEST INFRASTRUCTURE: tests/cpu_engine.CpuEngine at an ACTIVE SH degree for the multi-GPU mapping window (ABI 212).  What it adds:

* FusedEngine's W-wide flat gradient layout [xyz 3P | f_dc 3P | opacity P | scaling 3P | rotation 4P | f_rest 3 n P | accum P | denom P]
  (W = 14 + 3 n, n = rest_rows: the model's n_rest at an active degree, 0 otherwise -- then byte for byte the base class's layout);
* d_f_rest outputs in map_loop (Mm3dgsSlamGrads.d_f_rest = the flat's f_rest block), rows beyond the active degree zero as the kernels
  write them;
* the sixth Adam group (Mm3dgsMapAdam.rest_*) in map_loop and adam_project, opt_mask honoured, every row stepped.

Every map_loop call that wrote an f_rest gradient is recorded in `rest_outputs` (the tests' evidence that the native loop served the
window).  Never imported by the product."""
import ctypes as C

import torch

from tests.cpu_engine import CpuEngine, _adam, _view


def _rest_grad(rest, deg):
    """The f_rest gradient the kernels write: autograd's, zero where the graph left none and beyond the active degree."""
    gr = rest.grad.clone() if rest.grad is not None else torch.zeros_like(rest)
    gr[:, (deg + 1) ** 2 - 1:] = 0.0
    return gr


class ShCpuEngine(CpuEngine):
    rest_rows = 0

    def __init__(self, renderer):
        super().__init__(renderer)
        self.rest_outputs = []
        self._flat_rest = 0

    @property
    def flat_width(self):
        return 14 + 3 * self.rest_rows

    def bind_rest_rows(self, g):
        self.rest_rows = int(g._features_rest.shape[1]) if int(getattr(g, "active_sh_degree", 0)) > 0 else 0

    def _ensure(self, P, need_grads):
        if P != self.P:
            self.P, self.grads = P, None
        if need_grads and (self.grads is None or self._flat_rest != self.rest_rows):
            n, W = self.rest_rows, self.flat_width
            self.flat = torch.zeros((W + 2) * P + 64)
            o = [0, 3 * P, 6 * P, 7 * P, 10 * P, 14 * P, W * P, (W + 1) * P, (W + 2) * P]
            v = lambda i, shape: self.flat[o[i]:o[i + 1]].view(shape)
            self.grads = dict(xyz=v(0, (P, 3)), f_dc=v(1, (P, 1, 3)), opacity=v(2, (P, 1)), scaling=v(3, (P, 3)), rotation=v(4, (P, 4)))
            if n:
                self.grads["f_rest"] = v(5, (P, n, 3))
            self.acc = torch.zeros(W * P)
            self.stat_delta = (torch.zeros(P), v(6, (P, 1)), v(7, (P, 1)))
            self._flat_rest = n

    def _rest_adam(self, map_adam, g, gr, step):
        rest = g._features_rest
        assert map_adam.rest_param == rest.data_ptr(), "Mm3dgsMapAdam.rest_param does not point at the model's f_rest"
        n, P = rest.numel(), rest.shape[0]
        pv, mv, vv = _view(map_adam.rest_param, n), _view(map_adam.rest_exp_avg, n), _view(map_adam.rest_exp_avg_sq, n)
        if map_adam.opt_mask:
            gr = gr * _view(map_adam.opt_mask, P, C.c_uint8).bool()[:, None, None]
        _adam(pv, gr.reshape(-1), mv, vv, step, map_adam.rest_lr, map_adam.beta1, map_adam.beta2, map_adam.eps)

    def map_loop(self, views, g, lcfg, stats, map_adam, grads=None, keep_tile_order=False, want_loss=True, projected=False):
        deg = int(getattr(g, "active_sh_degree", 0))
        if deg == 0:
            return super().map_loop(views, g, lcfg, stats, map_adam, grads, keep_tile_order, want_loss, projected)
        self.bind_rest_rows(g)
        self._ensure(int(g._xyz.shape[0]), True)
        rest = g._features_rest
        for i, view in enumerate(views):      # one view per base-class call, then the sixth group / the f_rest output of that view
            ma = None
            if map_adam is not None:
                ma = type(map_adam).from_buffer_copy(map_adam)
                ma.step = int(map_adam.step) + i
            rest.grad = None
            super().map_loop([view], g, lcfg, stats, ma, grads, keep_tile_order, want_loss, projected and i == 0)
            with torch.no_grad():
                gr = _rest_grad(rest, deg)
                if ma is not None:
                    self._rest_adam(ma, g, gr, int(ma.step))
                elif grads is not None:
                    assert "f_rest" in grads and grads["f_rest"].data_ptr() == self.flat[14 * self.P:].data_ptr(), "d_f_rest is not the flat's f_rest block"
                    grads["f_rest"].copy_(gr)
                    self.rest_outputs.append(len(self.calls) - 1)
            rest.grad = None
        if len(views) > 1:      # (the base class logged one call per view: fold them into the one C call this was)
            del self.calls[-len(views):]
            del self.view_log[-len(views):]
            self.calls.append(("map", len(views), stats is not None, map_adam is not None))
            self.view_log.append(tuple(round(float(v[1].double().sum()), 4) for v in views))

    def adam_project(self, next_pose, g, grads, map_adam):
        super().adam_project(next_pose, g, grads, map_adam)
        deg = int(getattr(g, "active_sh_degree", 0))
        if deg > 0:
            assert map_adam.rest_param, "mm3dgs_slam_adam_project at an active SH degree needs the f_rest Adam group"
            with torch.no_grad():
                self._rest_adam(map_adam, g, grads["f_rest"].clone(), int(map_adam.step))


def install(fused_module, registry=None):
    """tests/cpu_engine.install with ShCpuEngine as the engine."""
    registry = {} if registry is None else registry
    real = fused_module.FusedEngine.__dict__["eligible"].__func__
    return dict(eligible=staticmethod(lambda c, g: real(dict(c, device="cuda:0"), g)),
                _engine=lambda renderer: registry.setdefault(id(renderer), ShCpuEngine(renderer)), _stream=lambda: None), registry
