"""Debug probe: at the first diverging mapping run of a SLAM sequence, execute it twice from the same state (fused backward+projection
launch on / off) and compare every buffer."""
import os, sys, random
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from mm3dgs_slam_amd import fused
from mm3dgs_slam_amd.config import default_config
from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence

ncall = [0]
_ml = fused.FusedEngine.map_loop
TARGET = int(sys.argv[1]) if len(sys.argv) > 1 else 3
def map_loop(self, views, g, lcfg, stats, map_adam, grads=None):
    ncall[0] += 1
    if ncall[0] != TARGET or map_adam is None:
        return _ml(self, views, g, lcfg, stats, map_adam, grads)
    opt = g.optimizer
    tens = []
    for gr in opt.param_groups:
        p = gr["params"][0]; st = opt.state.get(p, {})
        tens += [p.data] + [st[k] for k in ("exp_avg", "exp_avg_sq") if k in st]
    tens += list(stats) if stats is not None else []
    saved = [t.clone() for t in tens]
    print("views:", [v[0].tolist() for v in views], "same tensor:", views[0][0].data_ptr() == views[-1][0].data_ptr())
    res = {}
    for flag in ("1", "0", "1"):
        os.environ["MM3DGS_NO_FUSED_PROJECT"] = flag
        for t, s in zip(tens, saved):
            t.copy_(s)
        self.geom.zero_(); self.binning.zero_(); self.scratch.zero_(); self.radii.zero_()
        torch.cuda.synchronize()
        _ml(self, views, g, lcfg, stats, map_adam, grads)
        torch.cuda.synchronize()
        r = dict(out=self.out.clone(), radii=self.radii.clone(), geom=self.geom.clone(), xyz=g._xyz.data.clone(), op=g._opacity.data.clone(),
                 sc=g._scaling.data.clone(), fdc=g._features_dc.data.clone(), rot=g._rotation.data.clone())
        if stats is not None:
            r["accum"] = stats[1].clone(); r["maxr"] = stats[0].clone()
        if flag in res:
            print("repeat of", flag, {k: int((res[flag][k] != r[k]).sum()) for k in r})
        res[flag] = r
    a, b = res["1"], res["0"]
    P = int(g._xyz.shape[0])
    print("P", P, "n", len(views))
    for k in a:
        ne = (a[k] != b[k])
        print(" ", k, "differs in", int(ne.sum()), "of", ne.numel())
    # geometry sub-arrays
    def up(x, a=256): return (x + a - 1) // a * a
    offs, c = {}, 0
    for name, n in (("splat", P * 48), ("depth", P * 4), ("rect", P * 8), ("clamped", P), ("tileoff", P * 4), ("block_tiles", ((P + 255) // 256 + 1) * 4)):
        offs[name] = (c, c + n); c += up(n)
    ga, gb = a["geom"], b["geom"]
    for name, (s, e) in offs.items():
        ne = (ga[s:e] != gb[s:e])
        print("  geom.%s differs in %d bytes of %d" % (name, int(ne.sum()), e - s))
        if name == "splat" and int(ne.sum()):
            fa, fb = ga[s:e].view(torch.float32).view(P, 12), gb[s:e].view(torch.float32).view(P, 12)
            rows = (fa != fb).any(1).nonzero().flatten()
            print("   rows:", rows[:8].tolist(), "n", rows.numel())
            for rr in rows[:3].tolist():
                print("   ", rr, fa[rr].tolist(), fb[rr].tolist(), "xyz", a["xyz"][rr].tolist(), b["xyz"][rr].tolist())
    sys.exit(0)
fused.FusedEngine.map_loop = map_loop

torch.manual_seed(0); random.seed(0); np.random.seed(0)
cfg = default_config(device="cuda", height=120, width=160, tracking={"iters": 5}, mapping={"iters": 3, "kf_every": 1, "pruning_interval": 5})
seq = SyntheticSequence(cfg, 3, 6000, seed=6)
slam = SLAM(cfg, seq)
for i in range(2):
    slam.step(i)
