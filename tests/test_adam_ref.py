"""tests/adam_ref.py checked on the CPU: the float64 statement against torch.optim.Adam on float64 tensors, honest float32 inside the 2 x
bars on every input tests/test_gpu_adam.py uses, four subtly wrong float32 steps outside them, and the sharded step's group tables.

Printed by `pytest -s` (CPU, 2026-10-20): largest error / (2 x bar) of the float32 evaluations over all inputs: step32 p 0.499, m 0.124,
v 0.296; step32_fma p 0.499, m 0.124, v 0.294 (p: a half-ulp rounding just above a power of two is 0.5 by itself).  Elements with a
gradient at which a mutant breaks a bar: o2 formed in float32 99.9 %, eps under the root 35.2 %, bias corrections of step + 1 99.9 % /
step - 1 99.9 %, beta1 for 1 - beta1 100 %."""
import numpy as np
import pytest
import torch

from tests import adam_ref as ar


def test_statement_equals_torch_adam_in_float64():
    """Three steps, six groups with their own learning rates: step64 fed float64 scalars equals torch.optim.Adam(eps=1e-15) on float64
    tensors to 1e-14 relative (parameters and both moments); the float32 scalars lie within u relative of the double ones."""
    rng = np.random.default_rng(5)
    n = 500
    p0 = [rng.normal(size=n) for _ in ar.LRS]
    params = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in p0]
    opt = torch.optim.Adam([{"params": [q], "lr": lr} for q, lr in zip(params, ar.LRS)], lr=0.0, betas=(ar.BETA1, ar.BETA2), eps=ar.EPS)
    state = [(x.copy(), np.zeros(n), np.zeros(n)) for x in p0]
    for step in (1, 2, 3):
        grads = [rng.normal(size=n) * 10.0 ** rng.uniform(-6, 2, n) for _ in ar.LRS]
        for q, g in zip(params, grads):
            q.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        for i, lr in enumerate(ar.LRS):
            state[i] = ar.step64(*state[i], grads[i], ar.scalars64(step, lr=lr))
            st = opt.state[params[i]]
            for got, want in zip(state[i], (params[i].detach(), st["exp_avg"], st["exp_avg_sq"])):
                want = want.numpy()
                assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max(), (step, i)
    for step in (1, 2, 3, 7, 1000, 20000):
        for lr in ar.LRS:
            for a, b in zip(ar.scalars(step, lr=lr), ar.scalars64(step, lr=lr)):
                assert a.dtype == np.float32 and abs(float(a) - b) <= ar.U * abs(b), (step, lr)


def test_honest_float32_stays_inside_the_bars():
    """step32 and step32_fma on every input of the device tests: inside the 2 x bars whichever products are contracted."""
    top = {}
    for name, p, m, v, g, sc in ar.cpu_cases():
        for fn in (ar.step32, ar.step32_fma):
            r = ar.ratios(*fn(p, m, v, g, sc), p, m, v, g, sc)
            top[fn.__name__] = tuple(max(a, b) for a, b in zip(top.get(fn.__name__, (0.0, 0.0, 0.0)), r))
            assert max(r) <= 1.0, (name, fn.__name__, r)
    for k, r in top.items():
        print(f"ADAMREF {k}: largest error / (2 x bar): p {r[0]:.3f} m {r[1]:.3f} v {r[2]:.3f}")


def _eps_under_the_root(p, m, v, g, sc):
    p, m, v, g = (np.asarray(x, np.float32) for x in (p, m, v, g))
    with np.errstate(invalid="ignore"):
        m1 = m + (g - m) * sc.o1
        v1 = v * sc.b2 + g * g * sc.o2
        return p - sc.s * (m1 / (np.sqrt(v1 + sc.e) / sc.c)), m1, v1


def _mutants(step, lr):
    sc = ar.scalars(step, lr=lr)
    yield "o2 in float32", ar.step32, sc._replace(o2=np.float32(1.0) - np.float32(0.999))
    yield "eps under the root", _eps_under_the_root, sc
    yield "bias corrections of step + 1", ar.step32, sc._replace(c=ar.scalars(step + 1, lr=lr).c, s=ar.scalars(step + 1, lr=lr).s)
    if step > 1:
        yield "bias corrections of step - 1", ar.step32, sc._replace(c=ar.scalars(step - 1, lr=lr).c, s=ar.scalars(step - 1, lr=lr).s)
    yield "beta1 for 1 - beta1", ar.step32, sc._replace(o1=np.float32(ar.BETA1))


# The fraction of (finite) elements at which each mutant must break a bar.  o2 off by 1.3e-5 relative moves v* by 1.3e-5 g g o2, and g g o2
# is at least a sixth of v* after at most five steps of history: 2e-6 v* against a bar of 8 u v* = 4.8e-7 v*: every element with a
# gradient.  A bias correction of the neighbouring step moves s r by >= 2.5e-5 relative even at step 20000 (and by tens of per cent at
# steps 1 .. 4) against ~10 u: nearly every element.  beta1 for 1 - beta1 moves m* by 0.8 |g - m|: every element.  eps under the root
# changes q by e / (2 v*) relative, visible where that exceeds ~1e-4, v* < 5e-12, |g| below ~1e-4: a third of a log-uniform 1e-8 .. 1e3.
MUTANT_FRACTION = {"o2 in float32": 0.9, "eps under the root": 0.2, "bias corrections of step + 1": 0.9, "bias corrections of step - 1": 0.9,
                   "beta1 for 1 - beta1": 0.9}


def test_mutants_break_a_bar():
    """Four subtly wrong float32 steps on the inputs of the sizes test (63 <= n <= 1029): each misses a 2 x bar on the fraction of elements
    MUTANT_FRACTION derives, so a kernel with one of these mistakes cannot pass tests/test_gpu_adam.py."""
    hit, tot = {}, {}
    for n in ar.SIZES:
        if n < 63 or n > 70000:
            continue
        c, step, lr = ar.size_case(n)
        live = np.isfinite(c.g) & (c.g != 0)
        sc = ar.scalars(step, lr=lr)
        want, bar = ar.step64(c.p, c.m, c.v, c.g, sc), ar.bars(c.p, c.m, c.v, c.g, sc)
        for name, fn, msc in _mutants(step, lr):
            got = fn(c.p, c.m, c.v, c.g, msc)
            bad = np.zeros(n, bool)
            for a, w, b in zip(got, want, bar):
                bad |= ar.broken(a, w, b)
            hit[name] = hit.get(name, 0) + int((bad & live).sum())
            tot[name] = tot.get(name, 0) + int(live.sum())
    assert set(hit) == set(MUTANT_FRACTION)
    for name in hit:
        print(f"ADAMREF mutant '{name}': breaks a bar at {hit[name]} of {tot[name]} elements ({100.0 * hit[name] / tot[name]:.1f} %)")
    for name in hit:
        assert hit[name] >= MUTANT_FRACTION[name] * tot[name], name


def test_worst_reports_nan_and_exactness():
    one = np.ones(3)
    assert ar.worst([1.0, np.nan, 1.0], [1.0, np.nan, 1.0], one) == 0.0
    assert ar.worst([1.0, 2.0, 1.0], [1.0, np.nan, 1.0], one) == np.inf
    assert ar.worst([1.0, np.nan, 1.0], [1.0, 1.0, 1.0], one) == np.inf
    assert ar.worst([1.0, 1.0, 1.5], [1.0, 1.0, 1.0], [1.0, 1.0, 0.0]) == np.inf
    assert ar.worst([1.0, 1.0, 3.0], [1.0, 1.0, 1.0], one) == 1.0


@pytest.mark.parametrize("world", [1, 2, 3, 5, 8])
def test_shard_tables_cover_every_element_once(world):
    """The product's table builder over every rank's WindowParallel.shard_bounds: the entries of all ranks cover [0, W P) exactly once, each
    with its group's learning rate and with consistent offsets into the four arrays; at most 8 entries per rank."""
    from mm3dgs_slam_amd.fused import shard_table
    from mm3dgs_slam_amd.window_parallel import WindowParallel
    BASE = {"p": 1 << 40, "m": 2 << 40, "v": 3 << 40}       # (addresses are only computed with: one fictitious allocation per array kind)
    GRAD = 4 << 40
    for P in (1, 3, 63, 257, 1000):
        for W in (14, 38, 59):
            n = W * P
            ranges = ar.flat_ranges(P, W)
            seen = np.zeros(n, np.int32)
            for rank in range(world):
                S, lo, hi = WindowParallel(rank, world).shard_bounds(n)
                assert (S, lo, hi) == ar.shard_bounds(rank, world, n) and S % 4 == 0 and S * world >= n
                table, k = shard_table([(a, b, BASE["p"] + 4 * a, BASE["m"] + 4 * a, BASE["v"] + 4 * a, lr) for a, b, lr in ranges], lo, hi, GRAD)
                assert 0 <= k <= 8
                for e in (table[j] for j in range(k)):
                    i0 = (e.param - BASE["p"]) // 4
                    assert e.n > 0 and (e.param - BASE["p"]) % 4 == 0
                    assert e.exp_avg - BASE["m"] == 4 * i0 and e.exp_avg_sq - BASE["v"] == 4 * i0 and e.grad - GRAD == 4 * (i0 - lo)
                    assert lo <= i0 and i0 + e.n <= hi
                    own = [lr for a, b, lr in ranges if a <= i0 and i0 + e.n <= b]
                    assert own == [e.lr]
                    seen[i0:i0 + e.n] += 1
            assert (seen == 1).all(), (P, W, world)
