"""mm3dgs_adam (csrc/fused.hip: fused_adam_kernel) through the raw C ABI against the float64 statement tests/adam_ref.py, on every path the
product takes it: both bodies (float4: n % 4 == 0 and four 16-byte aligned pointers; scalar: everything else), the capped grid's second
trip, the eight-entry group table, every rank's call of the element-sharded step made on one device, the pose table of the sharded bundle
adjustment, and the in-kernel step of mm3dgs_slam_backward against the entry point.

Every array is a buffer the test owns between guard words, 16-byte aligned or 4 bytes past alignment; after each call the guards are
intact and `grad` equals its copy.  Parameters and both moments are held to TWICE the derived bounds of tests/adam_ref.py (its docstring
has the derivation; nothing here is a measured tolerance): a printed ratio is max |kernel - float64| / (2 x bound), so <= 1 passes.
Everything that compares two device results compares bits.  Each test prints `ADAMERR ...` (pytest -s) before it asserts.

Measured on MI355X, 2026-10-20, largest ratio over the cases of each test, p / m / v (a half-ulp rounding of p just above a power of two
is 0.5 by itself; honest float32 on the CPU gives 0.499 / 0.124 / 0.296 on the same inputs, tests/test_adam_ref.py):
    sizes and bodies 0.499 / 0.124 / 0.294 (each n: the same figures from both bodies)    sixteen patterns 0.440 / 0.073 / 0.198
    table of eight   0.486 / 0.096 / 0.250      sharded (whole-group call) 0.497 / 0.114 / 0.287      pose table 0.416 / 0.105 / 0.163
    special elements 0.161 / 0.023 / 0.095      in-kernel and entry point  0.482 / 0.146 / 0.302
and every bit-for-bit comparison held: float4 == scalar body, eight groups == eight calls, all ranks' sharded calls == the whole-group
call, in-kernel step == gradient output + mm3dgs_adam (the gradients repeated bit for bit)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import adam_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD_WORDS = 64                 # on each side; a multiple of 4: word GUARD_WORDS of a (256-byte aligned) allocation is 16-byte aligned
GUARD_BITS = 0x7FC0DEAD          # (a NaN pattern: compared as integers)


def _lib():
    from mm3dgs_slam_amd import _lib
    return _lib.load()


def _stream():
    from mm3dgs_slam_amd.rasterizer import _stream
    return _stream()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


class Guarded:
    """A float32 array on the device between guard words, `off` words (0 or 1) past a 16-byte boundary, and its first content."""

    def __init__(self, a, off=0):
        a = np.ascontiguousarray(a, np.float32).reshape(-1)
        self.n, self.lo = a.size, GUARD_WORDS + off
        self.buf = torch.full((GUARD_WORDS + off + self.n + GUARD_WORDS + 3,), GUARD_BITS, dtype=torch.int32, device=DEV)
        if self.n:
            self.buf[self.lo:self.lo + self.n] = torch.from_numpy(a.view(np.int32)).to(DEV)
        self.ptr = self.buf.data_ptr() + 4 * self.lo
        assert self.ptr % 16 == 4 * off
        self.first = a.view(np.int32).copy()

    def bits(self):
        """The data as int32 on the host, after checking both guard zones."""
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == GUARD_BITS).all(), "the guard words in front of the array were written"
        assert (b[self.lo + self.n:] == GUARD_BITS).all(), "the guard words behind the array were written"
        return b[self.lo:self.lo + self.n].copy()

    def read(self):
        return self.bits().view(np.float32)

    def untouched(self):
        return np.array_equal(self.bits(), self.first)


class State:
    """Guarded p, g, m, v of one group; offs = words past alignment of (param, grad, exp_avg, exp_avg_sq)."""

    def __init__(self, p, m, v, g, offs=(0, 0, 0, 0)):
        self.p, self.g, self.m, self.v = (Guarded(a, o) for a, o in zip((p, g, m, v), offs))
        self.n = self.p.n

    def entry(self, lr, lo=0, hi=None):
        """(param, grad, exp_avg, exp_avg_sq, n, lr) over the elements [lo, hi)."""
        hi = self.n if hi is None else hi
        return tuple(b.ptr + 4 * lo for b in (self.p, self.g, self.m, self.v)) + (hi - lo, lr)

    def vec(self):
        return self.n % 4 == 0 and all(b.ptr % 16 == 0 for b in (self.p, self.g, self.m, self.v))

    def result(self):
        """(p, m, v) as float32 after a call: guards intact, the gradient untouched."""
        assert self.g.untouched(), "the gradient was written"
        return self.p.read(), self.m.read(), self.v.read()


def _fill(table, entries):
    for e, (p, g, m, v, n, lr) in zip(table, entries):
        e.param, e.grad, e.exp_avg, e.exp_avg_sq, e.n, e.lr = p, g, m, v, n, lr


def _adam(entries, step):
    """One mm3dgs_adam call over (param, grad, exp_avg, exp_avg_sq, n, lr) entries (addresses; None is NULL); waits for it."""
    from mm3dgs_slam_amd import _lib as mod
    table = (mod.Mm3dgsAdamGroup * 8)()
    _fill(table, entries)
    rc = _lib().mm3dgs_adam(table, len(entries), step, ar.BETA1, ar.BETA2, ar.EPS, _stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib().mm3dgs_last_error()


def _same_bits(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---- sizes and bodies ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _size_ref(n):
    c, step, lr = ar.size_case(n)
    sc = ar.scalars(step, lr=lr)
    return c, step, lr, ar.step64(c.p, c.m, c.v, c.g, sc), ar.bars(c.p, c.m, c.v, c.g, sc)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", ar.SIZES)
def test_sizes_and_bodies(n, off):
    """One group of n floats, all four pointers aligned (the float4 body where n % 4 == 0) or all 4 bytes past alignment (the scalar
    body): 1 .. 1029 around the float4 and workgroup edges; 2097152 = exactly one trip of the 2048-workgroup grid in the float4 body,
    2097156 the first float4 of a second trip, 2098181 the scalar body at the cap: five trips, the last one 1029 elements."""
    c, step, lr, want, bar = _size_ref(n)
    s = State(c.p, c.m, c.v, c.g, (off,) * 4)
    assert s.vec() == (off == 0 and n % 4 == 0)
    _adam([s.entry(lr)], step)
    r = tuple(ar.worst(a, w, b) for a, w, b in zip(s.result(), want, bar))
    print(f"ADAMERR sizes n {n} {'float4' if s.vec() else 'scalar'} body step {step}: p {r[0]:.3f} m {r[1]:.3f} v {r[2]:.3f}")
    assert max(r) <= 1.0, r


def test_sixteen_alignment_patterns_give_the_same_bits():
    """n = 1028 with each of param, grad, exp_avg, exp_avg_sq aligned or 4 bytes off: only the all-aligned pattern may take the float4
    body; all sixteen results have the same bits, and they meet the bars."""
    c = ar.make_case(ar.PATTERN_N, 2)
    sc = ar.scalars(ar.PATTERN_STEP, lr=ar.PATTERN_LR)
    first = None
    for k in range(16):
        offs = tuple((k >> j) & 1 for j in range(4))
        s = State(c.p, c.m, c.v, c.g, offs)
        assert s.vec() == (k == 0)
        _adam([s.entry(ar.PATTERN_LR)], ar.PATTERN_STEP)
        got = s.result()
        if first is None:
            first = got
            r = ar.ratios(*got, c.p, c.m, c.v, c.g, sc)
            print(f"ADAMERR patterns n {ar.PATTERN_N}: p {r[0]:.3f} m {r[1]:.3f} v {r[2]:.3f}")
            assert max(r) <= 1.0, r
        assert _same_bits(got, first), offs


# ---- the group table ----------------------------------------------------------------------------------------------------------------
def test_group_table_of_eight_equals_eight_single_calls():
    """One call with eight groups -- float4 and scalar bodies mixed, the largest (which sizes the grid) fourth, two NULL groups of n = 0,
    one with lr = 0 -- meets the bars and equals, bit for bit, eight single-group calls from the same start.  The lr = 0 group keeps its
    parameters bit for bit (all but the two elements with a NaN gradient) while its moments step."""
    cases = [ar.make_case(n, 30 + i) for i, (n, _, _) in enumerate(ar.TABLE_GROUPS)]

    def start():
        return [State(c.p, c.m, c.v, c.g, (off,) * 4) if n else None for c, (n, off, _) in zip(cases, ar.TABLE_GROUPS)]

    def entries(states):
        return [s.entry(lr) if s else (None, None, None, None, 0, lr) for s, (_, _, lr) in zip(states, ar.TABLE_GROUPS)]
    one, each = start(), start()
    assert [s.vec() for s in one if s] == [True, False, False, True, False, True]
    _adam(entries(one), ar.TABLE_STEP)
    for e in entries(each):
        _adam([e], ar.TABLE_STEP)
    top = (0.0, 0.0, 0.0)
    for i, (c, (n, _, lr)) in enumerate(zip(cases, ar.TABLE_GROUPS)):
        if not n:
            continue
        got = one[i].result()
        top = tuple(max(a, b) for a, b in zip(top, ar.ratios(*got, c.p, c.m, c.v, c.g, ar.scalars(ar.TABLE_STEP, lr=lr))))
        assert _same_bits(got, each[i].result()), i
        if lr == 0.0:
            ok = np.setdiff1d(np.arange(n), c.nan)      # (0 x NaN is NaN: the element with the NaN gradient is lost at any lr, as in torch)
            assert np.array_equal(_bits(got[0])[ok], _bits(c.p)[ok]) and len(c.nan) == 2
            assert not one[i].m.untouched() and not one[i].v.untouched()
    print(f"ADAMERR table of eight: p {top[0]:.3f} m {top[1]:.3f} v {top[2]:.3f}")
    assert max(top) <= 1.0, top


# ---- the element-sharded step, every rank's call on one device --------------------------------------------------------------------------
@pytest.mark.parametrize("W", ar.SHARD_W)
@pytest.mark.parametrize("P", ar.SHARD_P)
def test_sharded_step_of_every_rank_equals_the_whole_group_step(P, W):
    """_MapLoop._sharded_adam's call for every rank of world 2, 3 and 8: the rank's WindowParallel.shard_bounds of the flat [W P], the
    product's shard_table over the groups' own arrays, the gradient in a separate shard_g buffer as the reduce-scatter leaves it.  After
    all ranks have stepped, parameters and both moments equal one whole-group call from the same start bit for bit (which meets the bars).
    At P = 257 and 6001 (P % 4 == 1: every group but the first starts off a 16-byte boundary of the flat layout) no entry qualifies for the
    float4 body -- but one: rank 0 of world 8 at W = 14 owns S = 452 / 10504 elements, all inside xyz, the group at flat offset 0, so its one
    entry is aligned and a multiple of 4 long, and the comparison then also holds the two bodies to each other."""
    from mm3dgs_slam_amd.fused import shard_table
    from mm3dgs_slam_amd.window_parallel import WindowParallel
    n = W * P
    c = ar.make_case(n, 40)
    ranges = ar.flat_ranges(P, W)

    def start():
        return [State(c.p[a:b], c.m[a:b], c.v[a:b], c.g[a:b]) for a, b, _ in ranges]
    whole = start()
    _adam([s.entry(lr) for s, (_, _, lr) in zip(whole, ranges)], ar.SHARD_STEP)
    want = [s.result() for s in whole]
    top = (0.0, 0.0, 0.0)
    for got, (a, b, lr) in zip(want, ranges):
        r = ar.ratios(*got, c.p[a:b], c.m[a:b], c.v[a:b], c.g[a:b], ar.scalars(ar.SHARD_STEP, lr=lr))
        top = tuple(max(x, y) for x, y in zip(top, r))
    print(f"ADAMERR sharded P {P} W {W} (whole-group call): p {top[0]:.3f} m {top[1]:.3f} v {top[2]:.3f}")
    assert max(top) <= 1.0, top
    lib = _lib()
    for world in ar.SHARD_WORLD:
        states, vec_entries = start(), []
        for rank in range(world):
            S, lo, hi = WindowParallel(rank, world).shard_bounds(n)
            sg = np.zeros(S, np.float32)
            sg[:hi - lo] = c.g[lo:hi]
            shard_g = Guarded(sg)
            table, k = shard_table([(a, b, s.p.ptr, s.m.ptr, s.v.ptr, lr) for s, (a, b, lr) in zip(states, ranges)], lo, hi, shard_g.ptr)
            assert (k > 0) == (hi > lo)
            for j in range(k):
                e = table[j]
                if e.n % 4 == 0 and (e.param | e.grad | e.exp_avg | e.exp_avg_sq) % 16 == 0:
                    vec_entries.append((rank, j))
            if k:       # (as the product: a rank whose slice is empty makes no call)
                assert lib.mm3dgs_adam(table, k, ar.SHARD_STEP, ar.BETA1, ar.BETA2, ar.EPS, _stream()) == 0, lib.mm3dgs_last_error()
                torch.cuda.synchronize()
            assert shard_g.untouched()
        if P % 4:
            assert vec_entries == ([(0, 0)] if (W, world) == (14, 8) else []), (world, vec_entries)
        for s, w_, (a, b, _) in zip(states, want, ranges):
            assert s.g.untouched()      # (the groups' own gradient arrays are not part of a sharded call)
            assert _same_bits((s.p.read(), s.m.read(), s.v.read()), w_), (world, a, b)
        print(f"ADAMERR sharded P {P} W {W} world {world}: bit-identical to the whole-group call; float4 entries {vec_entries}")


# ---- the pose table of the sharded bundle adjustment ------------------------------------------------------------------------------------
def test_pose_table_of_the_sharded_bundle_adjustment():
    """Exactly _MapLoop._ba_step's table: 7-float buffers, group [0:4] with cam_q_lr (float4 body) and [4:7] with cam_t_lr (scalar body,
    its pointers 16 bytes into the buffers).  Steps 1, 2, 3 in a row and a step 20000 (bias corrections ~ 1), each against the statement
    fed the device's own previous state, so the bars do not compound."""
    top = (0.0, 0.0, 0.0)
    c = ar.pose_case(1)
    p, m, v = c.p, np.zeros(7, np.float32), np.zeros(7, np.float32)
    for step in ar.POSE_STEPS:
        cs = ar.pose_case(step)
        if step == 20000:
            p, m, v = cs.p, cs.m, cs.v
        s = State(p, m, v, cs.g)
        _adam([s.entry(ar.POSE_LRS[0], 0, 4), s.entry(ar.POSE_LRS[1], 4, 7)], step)
        got = s.result()
        for (a, b), lr in zip(((0, 4), (4, 7)), ar.POSE_LRS):
            r = ar.ratios(*(x[a:b] for x in got), p[a:b], m[a:b], v[a:b], cs.g[a:b], ar.scalars(step, lr=lr))
            print(f"ADAMERR pose step {step} [{a}:{b}]: p {r[0]:.3f} m {r[1]:.3f} v {r[2]:.3f}")
            top = tuple(max(x, y) for x, y in zip(top, r))
        assert not np.array_equal(_bits(got[0]), _bits(p))
        p, m, v = got
    assert max(top) <= 1.0, top


# ---- special elements -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
def test_special_elements(off):
    """n = 1028 in both bodies: an unseen element (g = m = v = 0) keeps all three words bit for bit; a decay-only element (g = 0) meets the
    bars and its moments shrink; the NaN gradient makes exactly its own p, m and v NaN -- its three float4 neighbours meet the bars."""
    c = ar.make_case(1028, 3)
    step, lr = 2, 5e-2
    sc = ar.scalars(step, lr=lr)
    s = State(c.p, c.m, c.v, c.g, (off,) * 4)
    assert s.vec() == (off == 0)
    _adam([s.entry(lr)], step)
    got = s.result()
    assert len(c.unseen) == 2 and len(c.decay) == 2 and len(c.nan) == 2
    for a, a0 in zip(got, (c.p, c.m, c.v)):
        assert np.array_equal(_bits(a)[c.unseen], _bits(a0)[c.unseen])
    assert np.isnan(got[0][c.nan]).all() and np.isnan(got[1][c.nan]).all() and np.isnan(got[2][c.nan]).all()
    assert all(int(np.isnan(a).sum()) == 2 for a in got)
    assert (np.abs(got[1][c.decay]) < np.abs(c.m[c.decay])).all() and (got[2][c.decay] < c.v[c.decay]).all()
    near = np.unique(np.concatenate([c.decay] + [np.arange(i // 4 * 4, i // 4 * 4 + 4) for i in c.nan]))
    r = ar.ratios(*(a[near] for a in got), c.p[near], c.m[near], c.v[near], c.g[near], sc)
    print(f"ADAMERR special elements ({'float4' if off == 0 else 'scalar'} body; decay-only and the NaN's float4 neighbours): p {r[0]:.3f} m {r[1]:.3f} v {r[2]:.3f}")
    assert max(r) <= 1.0, r
    assert max(ar.ratios(*got, c.p, c.m, c.v, c.g, sc)) <= 1.0


# ---- rejected calls ---------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing():
    """A NULL table, n_groups -1 and 9, step 0, each of the four pointers NULL with n > 0: -1, a message, nothing written.  n_groups = 0: 0
    and nothing written."""
    from mm3dgs_slam_amd import _lib as mod
    lib = _lib()
    c = ar.make_case(64, 4)
    s = State(c.p, c.m, c.v, c.g)
    good = s.entry(1e-3)

    def call(entries, n_groups, step, null_table=False):
        table = (mod.Mm3dgsAdamGroup * 9)()
        _fill(table, entries)
        rc = lib.mm3dgs_adam(None if null_table else C.cast(table, C.POINTER(mod.Mm3dgsAdamGroup)), n_groups, step, ar.BETA1, ar.BETA2, ar.EPS,
                             _stream())
        torch.cuda.synchronize()
        assert all(b.untouched() for b in (s.p, s.g, s.m, s.v))
        assert rc == 0 or lib.mm3dgs_last_error()
        return rc
    bad = [("NULL table", call([good], 1, 1, null_table=True)), ("n_groups -1", call([good], -1, 1)), ("n_groups 9", call([good] * 9, 9, 1)),
           ("step 0", call([good], 1, 0))]
    for k, name in enumerate(("param", "grad", "exp_avg", "exp_avg_sq")):
        e = list(good)
        e[k] = None
        # (behind a good group: the whole call is refused, not only the bad entry)
        bad.append((f"NULL {name}", call([good, tuple(e)], 2, 1)))
    for what, rc in bad:
        assert rc == -1, what
    assert call([good], 1, -3) == -1 and lib.mm3dgs_last_error()
    assert call([good], 0, 1) == 0


def test_rejected_call_leaves_a_message():
    lib = _lib()
    assert lib.mm3dgs_adam(None, 1, 1, ar.BETA1, ar.BETA2, ar.EPS, _stream()) == -1
    msg = lib.mm3dgs_last_error()
    assert msg and b"group table" in msg
    c = ar.make_case(4, 5)
    s = State(c.p, c.m, c.v, c.g)
    from mm3dgs_slam_amd import _lib as mod
    table = (mod.Mm3dgsAdamGroup * 8)()
    _fill(table, [s.entry(1e-3)])
    assert lib.mm3dgs_adam(table, 1, 0, ar.BETA1, ar.BETA2, ar.EPS, _stream()) == -1
    assert b"step" in lib.mm3dgs_last_error()
    table[0].grad = None
    assert lib.mm3dgs_adam(table, 1, 1, ar.BETA1, ar.BETA2, ar.EPS, _stream()) == -1
    assert b"NULL in group 0" in lib.mm3dgs_last_error()
    torch.cuda.synchronize()
    assert all(b.untouched() for b in (s.p, s.g, s.m, s.v))


# ---- the in-kernel step against the entry point -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [63, 257])
def test_in_kernel_step_equals_the_entry_point(P):
    """mm3dgs_slam_backward with `map_adam` (slam_bwd_body's in-kernel adam_elem) against the same entry point's gradient outputs fed to
    mm3dgs_adam, on the scenes and guarded maps of tests/test_gpu_per_gaussian_loads.py.  Both sets of arrays sit 4 bytes past alignment,
    so mm3dgs_adam takes its scalar body.  The gradient-output call is made twice first: its gradients repeat bit for bit (reported), which
    is what lets the comparison be exact -- parameters and both moments of all five groups bit for bit.  (Were the gradients not to
    repeat, the in-kernel result would be held to the 2 x bars of the statement over the first call's gradients instead.)"""
    from tests.test_gpu_per_gaussian_loads import H, LRS, NAMES, W, _Guarded, _guarded_map, _scene
    from mm3dgs_slam_amd.fused import FusedEngine
    cfg, g, R, pose, color, depth, ids = _scene(P)
    gen = torch.Generator(device=DEV).manual_seed(400 + P)
    gs, ma, arr = _guarded_map(g, gen, zero_moments=False)
    copies = {n: tuple(_Guarded(a.t) for a in arr[n]) for n in NAMES}
    step = 3
    ma.step = step
    eng = FusedEngine(R)
    with torch.no_grad():
        si = eng.forward(pose, gs, need_grads=True)
        eng.dL.copy_(torch.randn(6, H, W, device=DEV, generator=gen))
        eng.backward(si, grads=eng.grads)
        torch.cuda.synchronize()
        grads = {n: Guarded(eng.grads[n].detach().cpu().numpy(), 1) for n in NAMES}
        eng.backward(si, grads=eng.grads)
        torch.cuda.synchronize()
        repeat = all(np.array_equal(_bits(eng.grads[n].cpu().numpy()).reshape(-1), grads[n].first) for n in NAMES)
        eng.backward(si, map_adam=ma)
        torch.cuda.synchronize()
    assert eng.check_capacity()
    start = {n: tuple(a.t.cpu().numpy().reshape(-1).copy() for a in copies[n]) for n in NAMES}
    _adam([(copies[n][0].t.data_ptr(), grads[n].ptr, copies[n][1].t.data_ptr(), copies[n][2].t.data_ptr(), copies[n][0].n, LRS[n]) for n in NAMES],
          step)
    assert all(a.intact() for n in NAMES for a in arr[n] + copies[n]) and all(grads[n].untouched() for n in NAMES)
    top, same = (0.0, 0.0, 0.0), True
    for n in NAMES:
        inner = tuple(a.t.cpu().numpy().reshape(-1) for a in arr[n])
        entry = tuple(a.t.cpu().numpy().reshape(-1) for a in copies[n])
        gr = grads[n].first.view(np.float32)
        assert np.abs(gr).max() > 0 and not np.array_equal(_bits(inner[0]), _bits(start[n][0]))
        sc = ar.scalars(step, lr=LRS[n])
        top = tuple(max(x) for x in zip(top, ar.ratios(*entry, *start[n], gr, sc), ar.ratios(*inner, *start[n], gr, sc)))
        same = same and _same_bits(inner, entry)
    print(f"ADAMERR in-kernel P {P}: gradients repeat bit for bit: {repeat}; in-kernel == entry point bit for bit: {same}; "
          f"either against float64: p {top[0]:.3f} m {top[1]:.3f} v {top[2]:.3f}")
    assert max(top) <= 1.0, top
    if repeat:
        assert same
