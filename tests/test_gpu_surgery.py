"""The map-surgery kernels of csrc/compact.hip through the raw C ABI -- prune predicate, compaction plan and rows, seeding, densification
plan and rows, covisibility counters -- against the float64 host statement tests/surgery_ref.py, on buffers the test owns, at the row counts
where a count / scan / scatter can break: 1, 63 .. 65, 255 .. 257, 262144 (exactly 1024 workgroups) and 262145 (the second round of the
1024-wide scan of the per-workgroup counts, which nothing else in the suite reaches through compact.hip).

Every destination is sized exactly to what the statement says it holds and sits between guard words, 4 bytes past a 16-byte boundary;
every source is compared with its copy after the call; work buffers are 0xFF before the plan, and each plan is compared word for word
with the statement's BEFORE the scatter that places rows by it runs (a scatter never sees a plan the test has not checked, and is only
ever called with the counts its own plan returned).  Every plan + scatter runs twice over different garbage: identical bytes.

Exact: every decision (keep byte, class, counter), every count, row order, parent, every copied word, zero moments / statistics, f_dc
(the float32 evaluation: the division is correctly rounded).  Decisions are exact because tests/surgery_cases.py keeps drawn inputs
1e-4 (relative) away from every threshold (checked on the CPU by tests/test_surgery_ref.py; the rare closer one is moved, < 1 %), NaN
and on-the-threshold inputs being placed by hand.  Computed values -- seeded xyz and log-scale, split children's xyz and scaling -- are
held to four times the float32 noise of the statement itself, in the form |kernel - float64| <= 4 D (1 + |float64|); see DEV_*.
Each test prints its figures (`SURGERR ...`, pytest -s) before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import surgery_cases as cases
from tests import surgery_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# D = max |float32 statement - float64 statement| / (1 + |float64 statement|) over every input of this file, CPU, 2026-10-20
# (tests/test_surgery_ref.py recomputes each and holds it below these); the kernels are allowed BAR = 4 D: another operation order and
# the device's logf / cosf / expf, a few ulp and not numpy's.
DEV_SEED_XYZ = 2.36e-7            # seeded xyz (513x512)              -> bar 9.4e-7 (1 + |x|)
DEV_SEED_SCALING = 5.37e-8        # seeded log-scale (513x512)        -> bar 2.1e-7 (1 + |s|)
DEV_CHILD_XYZ = 6.79e-7           # children's xyz (P 262145, mix)    -> bar 2.7e-6 (1 + |x|)
DEV_CHILD_SCALING = 1.20e-7       # children's scaling (P 262144)     -> bar 4.8e-7 (1 + |s|)
BAR = 4.0
# largest kernel deviation seen, same form, MI355X, 2026-10-20: seeded xyz 1.91e-7 (0.8 D), seeded log-scale 1.58e-7 (2.9 D: logf near
# |log| = 5 is a few ulp off numpy's), children's xyz 6.79e-7 (1.0 D), children's scaling 1.57e-7 (1.3 D)

GUARD_WORDS = 64                 # on each side; with one more word in front the data starts 4 bytes past a 16-byte boundary
GUARD_BITS = 0x7FC0DEAD          # (a NaN pattern: compared as integers)
FILLS = (0xCD, 0x5A)             # the garbage a destination holds before the call, first and second run
MOVED_CAP = 0.01


def _lib():
    from mm3dgs_slam_amd import _lib
    return _lib.load()


def lib_mod():
    """The binding module (its ctypes structures)."""
    from mm3dgs_slam_amd import _lib
    return _lib


def _stream():
    from mm3dgs_slam_amd.rasterizer import _stream
    return _stream()


def _ptr(x):
    if x is None:
        return None
    return C.c_void_p(x if isinstance(x, int) else x.ptr)


def _sync():
    torch.cuda.synchronize()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


class Guarded:
    """`nbytes` of device memory between guard words.  `fill`: the byte every data byte holds before the call, or a numpy array."""

    def __init__(self, nbytes, fill):
        words = (nbytes + 3) // 4
        self.buf = torch.full((GUARD_WORDS + 1 + words + GUARD_WORDS + 3,), GUARD_BITS, dtype=torch.int32, device=DEV)
        self.bytes = self.buf.view(torch.uint8)
        self.lo, self.hi = 4 * (GUARD_WORDS + 1), 4 * (GUARD_WORDS + 1) + nbytes
        self.ptr = self.buf.data_ptr() + self.lo
        assert self.ptr % 16 == 4
        self.pristine = np.tile(np.frombuffer(np.int32(GUARD_BITS).tobytes(), np.uint8), self.buf.shape[0])
        if nbytes:
            if isinstance(fill, np.ndarray):
                self.bytes[self.lo:self.hi] = torch.from_numpy(np.ascontiguousarray(fill).view(np.uint8).reshape(-1)).to(DEV)
            else:
                self.bytes[self.lo:self.hi] = fill
        self.first = self.read(np.uint8)

    def write_head(self, a):
        """The first bytes of the data (rows a call must leave alone)."""
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        if b.shape[0]:
            self.bytes[self.lo:self.lo + b.shape[0]] = torch.from_numpy(b).to(DEV)
        self.first = self.read(np.uint8)

    def read(self, dtype=np.float32):
        """The data on the host, after checking both guard zones."""
        b = self.bytes.cpu().numpy()
        assert np.array_equal(b[:self.lo], self.pristine[:self.lo]), "the guard words in front of the array were written"
        assert np.array_equal(b[self.hi:], self.pristine[self.hi:]), "the guard words behind the array were written"
        return b[self.lo:self.hi].copy().view(dtype)

    def untouched(self):
        return np.array_equal(self.read(np.uint8), self.first)


class Source:
    """A read-only input on the device and its copy."""

    def __init__(self, a):
        self.t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)
        self.copy = self.t.clone()
        self.ptr = self.t.data_ptr()
        assert self.ptr != 0

    def unchanged(self):
        return torch.equal(self.t, self.copy)


def _within(got, want, dev):
    """(all within BAR dev (1 + |want|), the largest deviation seen in the form of dev)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not want.size:
        return True, 0.0
    err = np.abs(got - want)
    return bool((err <= BAR * dev * (1.0 + np.abs(want))).all()), float((err / (1.0 + np.abs(want))).max())


# ---- prune ------------------------------------------------------------------------------------------------------------------------
def _prune_call(n, opacity, scales, radii, keep, counter, thresholds=(cases.MIN_OPACITY, cases.MAX_SCALE, cases.MAX_SCREEN)):
    return _lib().mm3dgs_prune_mask(n, _ptr(opacity), _ptr(scales), _ptr(radii), *thresholds, _ptr(keep), _ptr(counter), _stream())


@pytest.mark.parametrize("use_radii", [True, False])
@pytest.mark.parametrize("n", cases.SIZES)
def test_prune_mask_and_counter(n, use_radii):
    opacity, scales, radii, placed = cases.prune_rows(n)
    r = radii if use_radii else None
    th = (cases.MIN_OPACITY, cases.MAX_SCALE, cases.MAX_SCREEN)
    _, margin = ref.prune_keep(opacity, scales, r, *th)
    moved = ref.move_prune_rows(opacity, scales, r, margin, placed, *th)
    assert moved <= MOVED_CAP * n
    keep, margin = ref.prune_keep(opacity, scales, r, *th)
    assert not ((margin < ref.MARGIN) & ~placed).any()
    n_pruned = int((keep == 0).sum())
    if n >= 63:
        o_fires = ref.prune_keep(opacity, scales - 20, None, *th)[0] == 0
        s_fires = ref.prune_keep(opacity * 0 + 5, scales, None, *th)[0] == 0
        assert o_fires.any() and s_fires.any() and (not use_radii or (radii > cases.MAX_SCREEN).any())      # all three clauses fire
    runs = []
    for fill in FILLS:
        src = [Source(opacity), Source(scales), Source(radii)]
        k, counter = Guarded(n, fill), Guarded(4, np.array([1000], np.uint32))
        assert _prune_call(n, src[0], src[1], src[2] if use_radii else None, k, counter) == 0
        _sync()
        got, cnt = k.read(np.uint8), int(counter.read(np.uint32)[0])
        print(f"SURGERR prune n {n} radii {use_radii}: {n_pruned} pruned (kernel {int((got == 0).sum())}), counter {cnt - 1000}, {moved} moved")
        assert np.array_equal(got, keep), np.nonzero(got != keep)[0][:8]
        assert cnt == 1000 + n_pruned
        assert _prune_call(n, src[0], src[1], src[2] if use_radii else None, k, counter) == 0      # the count is added, not stored
        _sync()
        assert np.array_equal(k.read(np.uint8), keep) and int(counter.read(np.uint32)[0]) == 1000 + 2 * n_pruned
        assert all(s.unchanged() for s in src)
        runs.append(got.tobytes())
    assert runs[0] == runs[1]


def test_prune_mask_exactly_on_the_scale_threshold_and_with_no_rows():
    # exp(0) = 1 in every precision: with max_scale = 1 the first row is on the threshold and stays (>), the second is above it
    opacity, scales = np.float32([[1.0], [1.0], [1.0]]), np.float32([[0, -1, -1], [-1, 0.5, -1], [-1, -1, -0.5]])
    src = [Source(opacity), Source(scales)]
    k, counter = Guarded(3, 0xCD), Guarded(4, np.array([0], np.uint32))
    assert _prune_call(3, src[0], src[1], None, k, counter, (cases.MIN_OPACITY, 1.0, 0.0)) == 0
    _sync()
    assert k.read(np.uint8).tolist() == [1, 0, 1] == ref.prune_keep(opacity, scales, None, cases.MIN_OPACITY, 1.0, 0.0)[0].tolist()
    assert int(counter.read(np.uint32)[0]) == 1
    # P = 0: returns 0 and writes nothing
    k, counter = Guarded(8, 0xCD), Guarded(4, 0xCD)
    assert _prune_call(0, src[0], src[1], None, k, counter) == 0
    _sync()
    assert k.untouched() and counter.untouched()


# ---- compaction -------------------------------------------------------------------------------------------------------------------
def _checked_plan(n, keep_src, keep):
    """mm3dgs_compact_plan into a 0xFF work buffer, compared with the statement: (work, count)."""
    lib = _lib()
    nbytes = int(lib.mm3dgs_compact_work_bytes(n))
    nb = (n + 255) // 256
    assert nbytes >= 4 * (nb + 1) and nbytes % 4 == 0
    work, n_keep = Guarded(nbytes, 0xFF), Guarded(4, 0xFF)
    assert lib.mm3dgs_compact_plan(n, _ptr(keep_src), _ptr(work), _ptr(n_keep), _stream()) == 0
    _sync()
    pre, total = ref.block_prefix(keep)
    w = work.read(np.uint32)
    assert np.array_equal(w[:nb], pre), "the plan's per-workgroup prefix"
    assert bool((w[nb:] == 0xFFFFFFFF).all()), "the plan wrote behind its nb words"
    assert int(n_keep.read(np.uint32)[0]) == total
    work.first = work.read(np.uint8)
    return work, total


def _compact(n, keep, arrays, fill):
    """Plan + rows of one compaction over `arrays` (a None entry: a zero-width entry of the table).  Returns the destination bytes."""
    lib = _lib()
    ks = Source(keep)
    work, total = _checked_plan(n, ks, keep)
    table = (lib_mod().Mm3dgsCompactArray * max(len(arrays), 1))()
    src, dst = [], []
    for e, a in zip(table, arrays):
        if a is None:
            e.src, e.dst, e.width = None, None, 0
            continue
        s, d = Source(a), Guarded(total * a.shape[1] * 4, fill)
        e.src, e.dst, e.width = s.ptr, d.ptr, a.shape[1]
        src.append(s)
        dst.append(d)
    assert lib.mm3dgs_compact_rows(n, _ptr(ks), _ptr(work), table, len(arrays), _stream()) == 0
    _sync()
    want, count = ref.compact(keep, [a for a in arrays if a is not None])
    assert count == total
    out = []
    for k, (d, w) in enumerate(zip(dst, want)):
        got = d.read(np.int32)
        assert np.array_equal(got, _bits(w).reshape(-1)), f"array {k} (width {w.shape[1]})"
        out.append(got.tobytes())
    assert ks.unchanged() and all(s.unchanged() for s in src) and work.untouched()
    return out, total


@pytest.mark.parametrize("pattern", cases.KEEP_PATTERNS)
@pytest.mark.parametrize("n", cases.SIZES)
def test_compaction_plan_and_rows(n, pattern):
    keep = cases.keep_bytes(n, pattern)
    widths = (1, 3, 0, 4) if n >= cases.LARGE else (1, 3, 0, 4, 45)      # (a zero-width entry in the table: skipped)
    arrays = [a if a.shape[1] else None for a in cases.row_arrays(n, widths)]
    runs = [_compact(n, keep, arrays, fill) for fill in FILLS]
    print(f"SURGERR compact n {n} {pattern}: {runs[0][1]} kept, widths {widths}")
    assert runs[0] == runs[1]
    if pattern == "bytes" and n >= 63:
        assert len(set(keep.tolist())) == 5
    if pattern == "hole" and n >= 768:
        assert not keep[256:512].any() and keep[:256].all() and keep[512:768].all()


@pytest.mark.parametrize("n_arrays", [24, 32])
def test_compaction_of_24_and_32_arrays_in_one_call(n_arrays):
    n = 257
    keep = cases.keep_bytes(n, "random")
    widths = [(1, 3, 4, 45, 2, 0, 5, 16)[k % 8] for k in range(n_arrays)]
    arrays = [a if a.shape[1] else None for a in cases.row_arrays(n, widths, seed=n_arrays)]
    runs = [_compact(n, keep, arrays, fill) for fill in FILLS]
    assert runs[0] == runs[1] and len(runs[0][0]) == sum(1 for w in widths if w)


def test_compaction_plan_of_no_elements():
    lib = _lib()
    work, n_keep = Guarded(int(lib.mm3dgs_compact_work_bytes(0)), 0xFF), Guarded(4, 0xFF)
    assert lib.mm3dgs_compact_plan(0, None, _ptr(work), _ptr(n_keep), _stream()) == 0
    _sync()
    assert int(n_keep.read(np.uint32)[0]) == 0 and work.untouched()


# ---- seeding ----------------------------------------------------------------------------------------------------------------------
SEED_WIDTHS = dict(xyz=3, f_dc=3, f_rest=None, opacity=1, scaling=3, rotation=4, rgb=3)


@pytest.mark.parametrize("n_rest", [0, 15])
@pytest.mark.parametrize("row0", [0, 5])
@pytest.mark.parametrize("H,W", cases.SEED_SHAPES)
def test_seeding_rows(H, W, row0, n_rest):
    lib = _lib()
    c = cases.seed_case(H, W)
    a = [c[k] for k in ("color", "depth", "keep", "pose", "fx", "fy", "cx", "cy")]
    s64, s32 = ref.seed(*a, n_rest), ref.seed(*a, n_rest, dtype=np.float32)
    n = s64["xyz"].shape[0]
    widths = dict(SEED_WIDTHS, f_rest=3 * n_rest)
    runs, worst = [], {}
    for fill in FILLS:
        src = {k: Source(c[k]) for k in ("color", "depth", "keep", "pose")}
        work, total = _checked_plan(H * W, src["keep"], c["keep"])
        assert total == n
        out, so, heads = {}, lib_mod().Mm3dgsSeedOutputs(), {}
        for k, (name, w) in enumerate(widths.items()):
            out[name] = Guarded((row0 + n) * w * 4, fill)
            heads[name] = (np.arange(row0 * w, dtype=np.float32) + np.float32(100 * k + 0.25))
            out[name].write_head(heads[name])
            setattr(so, name, out[name].ptr)
        assert lib.mm3dgs_seed_gaussians(H, W, _ptr(src["color"]), _ptr(src["depth"]), _ptr(src["keep"]), _ptr(work), _ptr(src["pose"]), c["fx"], c["fy"],
                                         c["cx"], c["cy"], row0, C.byref(so), n_rest, _stream()) == 0
        _sync()
        got = {}
        for name, w in widths.items():
            g = out[name].read(np.float32).reshape(row0 + n, w)
            assert np.array_equal(_bits(g[:row0]).reshape(-1), _bits(heads[name])), f"{name}: rows below row0 were written"
            got[name] = g[row0:]
        ok_x, worst["xyz"] = _within(got["xyz"], s64["xyz"], DEV_SEED_XYZ)
        ok_s, worst["scaling"] = _within(got["scaling"], s64["scaling"], DEV_SEED_SCALING)
        print(f"SURGERR seed {H}x{W} row0 {row0} n_rest {n_rest}: {n} rows; kernel deviation xyz {worst['xyz']:.3e} (D {DEV_SEED_XYZ:.3e}), "
              f"log-scale {worst['scaling']:.3e} (D {DEV_SEED_SCALING:.3e})")
        for name in ("rgb", "opacity", "rotation", "f_rest"):          # bit for bit; with rgb in raster order: the row order
            assert np.array_equal(_bits(got[name]), _bits(s64[name])), name
        assert np.array_equal(_bits(got["f_dc"]), _bits(s32["f_dc"])), "f_dc against (rgb - 0.5f) / C0f"
        assert ok_x and ok_s
        assert all(s.unchanged() for s in src.values()) and work.untouched()
        runs.append([out[name].read(np.uint8).tobytes() for name in widths])
    assert runs[0] == runs[1]


# ---- densification ----------------------------------------------------------------------------------------------------------------
def _checked_densify_plan(P, src, cls, max_clone_scale=cases.MAX_CLONE_SCALE):
    """mm3dgs_densify_plan into a 0xFF work buffer, compared with the statement: (work, the plan's own counts)."""
    lib = _lib()
    nbytes, nb, cb = int(lib.mm3dgs_densify_work_bytes(P)), (P + 255) // 256, (P + 255) // 256 * 256
    assert nbytes >= cb + 4 * (3 * nb + 1)
    work, counts = Guarded(nbytes, 0xFF), Guarded(12, 0xFF)
    assert lib.mm3dgs_densify_plan(P, _ptr(src["grad_accum"]), _ptr(src["denom"]), _ptr(src["scaling"]), cases.MAX_GRAD, max_clone_scale, _ptr(work),
                                   _ptr(counts), _stream()) == 0
    _sync()
    w = work.read(np.uint8)
    assert np.array_equal(w[:P], cls), ("class bytes", np.nonzero(w[:P] != cls)[0][:8])
    assert bool((w[P:cb] == 0xFF).all())
    words = w[cb:].view(np.uint32)
    flags = (cls < 2, cls == ref.CLONE, cls == ref.SPLIT)
    for k, f in enumerate(flags):
        assert np.array_equal(words[k * nb:(k + 1) * nb], ref.block_prefix(f)[0]), f"the plan's per-workgroup prefix of class set {k}"
    assert bool((words[3 * nb:] == 0xFFFFFFFF).all()), "the plan wrote behind its 3 nb words"
    got = [int(v) for v in counts.read(np.uint32)]
    assert got == [int(f.sum()) for f in flags], got
    work.first = work.read(np.uint8)
    return work, got


def _densify(P, arrays, moments, grad_accum, denom, cls, N, with_parent, fill, max_clone_scale=cases.MAX_CLONE_SCALE):
    lib = _lib()
    out = ref.densify(arrays, moments, cls, N, cases.DENSIFY_SEED)
    n = out["n"]
    src = {k: Source(v) for k, v in arrays.items() if v.shape[1]}
    src.update(grad_accum=Source(grad_accum), denom=Source(denom))
    work, (n_keep, n_clone, n_split) = _checked_densify_plan(P, src, cls, max_clone_scale)
    assert (n_keep, n_clone, n_split) == (out["n_keep"], out["n_clone"], out["n_split"])
    st, dst, msrc = lib_mod().Mm3dgsDensifyState(), {}, {}
    for k, name in enumerate(ref.GROUPS):
        w = arrays[name].shape[1]
        e = st.group[k]
        e.width = w
        if not w:
            continue                                  # a zero-width group: NULL pointers, skipped
        dst[name] = Guarded(n * w * 4, fill)
        e.src, e.dst = src[name].ptr, dst[name].ptr
        if name in moments:                           # (else: a group without Adam state, NULL m_dst / v_dst)
            for tag, m in zip(("m_", "v_"), moments[name]):
                msrc[tag + name], dst[tag + name] = Source(m), Guarded(n * w * 4, fill)
            e.m_src, e.m_dst, e.v_src, e.v_dst = msrc["m_" + name].ptr, dst["m_" + name].ptr, msrc["v_" + name].ptr, dst["v_" + name].ptr
    for name in ("grad_accum", "denom", "max_radii2D"):
        dst["stat_" + name] = Guarded(n * 4, fill)
        setattr(st, name, dst["stat_" + name].ptr)
    if with_parent:
        dst["parent"] = Guarded(n * 4, fill)
        st.parent = dst["parent"].ptr
    # (the counts are the plan's own, read back from the device, and equal to the statement's)
    assert lib.mm3dgs_densify_rows(P, _ptr(work), n_keep, n_clone, n_split, N, cases.DENSIFY_SEED, C.byref(st), _stream()) == 0
    _sync()
    child, worst = out["child"], {}
    for name in ref.GROUPS:
        if name not in dst:
            continue
        got = dst[name].read(np.float32).reshape(n, -1)
        if name in ("xyz", "scaling"):
            assert np.array_equal(_bits(got[~child]), _bits(out[name][~child])), name
            ok, worst[name] = _within(got[child], out["child_" + name], DEV_CHILD_XYZ if name == "xyz" else DEV_CHILD_SCALING)
            assert ok, (name, worst[name])
        else:
            assert np.array_equal(_bits(got), _bits(out[name])), name
        for tag in ("m_", "v_"):
            if tag + name in dst:
                assert np.array_equal(_bits(dst[tag + name].read(np.float32).reshape(n, -1)), _bits(out[tag + name])), tag + name
    for name in ("grad_accum", "denom", "max_radii2D"):
        assert not dst["stat_" + name].read(np.int32).any(), name
    if with_parent:
        assert np.array_equal(dst["parent"].read(np.int32), out["parent"])
    assert all(s.unchanged() for s in src.values()) and all(s.unchanged() for s in msrc.values()) and work.untouched()
    return {k: d.read(np.uint8).tobytes() for k, d in dst.items()}, out, worst


def _settled_classes(P, grad_accum, denom, scaling, placed):
    cls, margin = ref.densify_classes(grad_accum, denom, scaling, cases.MAX_GRAD, cases.MAX_CLONE_SCALE)
    moved = ref.move_densify_rows(grad_accum, denom, scaling, margin, placed, cases.MAX_GRAD, cases.MAX_CLONE_SCALE)
    assert moved <= MOVED_CAP * P
    cls, margin = ref.densify_classes(grad_accum, denom, scaling, cases.MAX_GRAD, cases.MAX_CLONE_SCALE)
    assert not ((margin < ref.MARGIN) & ~placed).any()
    return cls, moved


@pytest.mark.parametrize("P,mix,N", cases.DENSIFY_RUNS)
def test_densification_plan_and_rows(P, mix, N):
    run = cases.densify_run(P, mix)
    arrays, grad_accum, denom, placed = cases.densify_rows(P, mix, n_rest=run["n_rest"])
    cls, moved = _settled_classes(P, grad_accum, denom, arrays["scaling"], placed)
    moments = cases.densify_moments(arrays, [k for k in run["moment_groups"] if arrays[k].shape[1]])
    runs = [_densify(P, arrays, moments, grad_accum, denom, cls, N, run["with_parent"], fill) for fill in FILLS]
    out, worst = runs[0][1], runs[0][2]
    print(f"SURGERR densify P {P} {mix} N {N} n_rest {run['n_rest']} moments {len(moments)} parent {run['with_parent']}: keep {out['n_keep']} clone "
          f"{out['n_clone']} split {out['n_split']} -> {out['n']} rows, {moved} moved; kernel deviation child xyz {worst['xyz']:.3e} (D {DEV_CHILD_XYZ:.3e}), "
          f"child scaling {worst['scaling']:.3e} (D {DEV_CHILD_SCALING:.3e})")
    assert runs[0][0] == runs[1][0]
    if mix == "none":
        assert (out["n_keep"], out["n_clone"], out["n_split"], out["n"]) == (P, 0, 0, P)      # rows called with (P, 0, 0): every row copied
    if mix == "all_split":
        assert out["n"] == N * P


def test_densification_classes_exactly_on_the_thresholds():
    """exp(0) = 1 in every precision: with max_clone_scale = 1 a row whose largest log-scale is 0 is ON the clone threshold (<=: clone),
    and 2 / 4 is MAX_GRAD exactly (>=: selected)."""
    P = 6
    arrays, grad_accum, denom, _ = cases.densify_rows(P, "none", n_rest=0)
    arrays["scaling"][:] = np.float32([[0, -1, -1], [-1, 0, -2], [-3, -1, 0], [-1, 0.5, -1], [0, 0, 0], [-1, -1, -1]])
    grad_accum[:], denom[:] = np.float32([2, 2, 2, 2, 1.9999999, 3]), 4.0
    cls, _ = ref.densify_classes(grad_accum, denom, arrays["scaling"], cases.MAX_GRAD, 1.0)
    assert cls.tolist() == [1, 1, 1, 2, 0, 1]
    moments = cases.densify_moments(arrays, ("xyz", "scaling"))
    runs = [_densify(P, arrays, moments, grad_accum, denom, cls, 2, True, fill, max_clone_scale=1.0) for fill in FILLS]
    assert runs[0][0] == runs[1][0] and runs[0][1]["n"] == 5 + 4 + 2


# ---- covisibility -----------------------------------------------------------------------------------------------------------------
def _covis_call(H, W, depth, sil, kp, cp, c, counts):
    return _lib().mm3dgs_covisibility_ratio(H, W, _ptr(depth), _ptr(sil), _ptr(kp), _ptr(cp), c["fx"], c["fy"], c["cx"], c["cy"], _ptr(counts), _stream())


@pytest.mark.parametrize("plain", [False, True])
@pytest.mark.parametrize("view", cases.COVIS_VIEWS)
@pytest.mark.parametrize("H,W", cases.COVIS_SHAPES)
def test_covisibility_counters(H, W, view, plain):
    c = cases.covis_case(H, W, view, plain=plain)
    a = lambda: [c[k] for k in ("depth", "sil", "kf_pose", "cur_pose", "fx", "fy", "cx", "cy")]
    _, margin = ref.covisibility(*a())
    moved = ref.move_covisibility_pixels(c["sil"], margin, c["placed"])
    assert moved <= MOVED_CAP * H * W
    want, margin = ref.covisibility(*a())
    assert not ((margin < ref.MARGIN) & ~c["placed"].reshape(-1)).any()
    runs = []
    for fill in FILLS:
        src = [Source(c[k]) for k in ("depth", "sil", "kf_pose", "cur_pose")]
        counts = Guarded(8, fill)
        assert _covis_call(H, W, *src, c, counts) == 0
        _sync()
        got = tuple(int(v) for v in counts.read(np.uint32))
        print(f"SURGERR covisibility {H}x{W} {view} plain {plain}: inside / tested {got} (statement {want}), {moved} moved")
        assert got == want
        assert _covis_call(H, W, *src, c, counts) == 0          # the call zeroes the counters itself
        _sync()
        assert tuple(int(v) for v in counts.read(np.uint32)) == want
        assert all(s.unchanged() for s in src)
        runs.append(got)
    assert runs[0] == runs[1]


def test_covisibility_of_an_empty_image():
    c = cases.covis_case(4, 4, "keeps_all")
    src = [Source(c[k]) for k in ("depth", "sil", "kf_pose", "cur_pose")]
    for H, W in ((0, 5), (5, 0), (0, 0)):
        counts = Guarded(8, 0xCD)
        assert _covis_call(H, W, *src, c, counts) == 0
        _sync()
        assert counts.read(np.uint32).tolist() == [0, 0]


# ---- rejected calls ---------------------------------------------------------------------------------------------------------------
def test_rejected_calls_return_minus_one_and_write_nothing():
    """Every refusal api.hip makes before a launch, for each entry point of the family (no call here reaches a kernel)."""
    lib, lm = _lib(), lib_mod()
    P, N = 8, 2
    arrays, grad_accum, denom, _ = cases.densify_rows(P, "mix", n_rest=0)
    src = {k: Source(v) for k, v in arrays.items() if v.shape[1]}
    f = Source(np.ones(64, np.float32))          # any readable float array
    keep = Source(np.ones(P, np.uint8))
    out = {k: Guarded(256, 0xCD) for k in ("a", "b", "c", "d", "e", "f", "g", "work", "count", "keep")}
    o, work, count, s = out["a"], out["work"], out["count"], _stream()
    BIG = 1 << 31

    def table(n, width=3, src_ptr=f.ptr, dst_ptr=o.ptr):
        t = (lm.Mm3dgsCompactArray * max(n, 1))()
        for e in t:
            e.src, e.dst, e.width = src_ptr, dst_ptr, width
        return t

    def seed_out(**null):
        so = lm.Mm3dgsSeedOutputs()
        for name, g in zip(SEED_WIDTHS, "abcdefg"):
            setattr(so, name, None if name in null else out[g].ptr)
        return so

    def seed_call(H=2, W=2, color=f, depth=f, k=keep, w=work, pose=f, so="default", n_rest=0):
        so = seed_out() if so == "default" else so
        return lib.mm3dgs_seed_gaussians(H, W, _ptr(color), _ptr(depth), _ptr(k), _ptr(w), _ptr(pose), 50.0, 51.0, 1.0, 1.0, 0,
                                         None if so is None else C.byref(so), n_rest, s)

    def state(width0=3, neg=False, null_src=False, orphan_moment=False, **null):
        st = lm.Mm3dgsDensifyState()
        for k, name in enumerate(ref.GROUPS):
            e = st.group[k]
            e.width = arrays[name].shape[1]
            if e.width:
                e.src, e.dst = src[name].ptr, out["abcdefg"[k]].ptr
        st.group[0].width = width0
        if neg:
            st.group[1].width = -1
        if null_src:
            st.group[3].src = None
        if orphan_moment:
            st.group[3].m_dst = out["g"].ptr
        for name, g in zip(("grad_accum", "denom", "max_radii2D"), "efg"):
            setattr(st, name, None if name in null else out[g].ptr)
        return st

    def rows_call(P_=P, w=work, counts=(P, 0, 0), N_=N, st="default"):
        st = state() if st == "default" else st
        return lib.mm3dgs_densify_rows(P_, _ptr(w), *counts, N_, 1, None if st is None else C.byref(st), s)

    def covis(H=2, W=2, depth=f, sil=f, kp=f, cp=f, counts=count):
        return lib.mm3dgs_covisibility_ratio(H, W, _ptr(depth), _ptr(sil), _ptr(kp), _ptr(cp), 50.0, 51.0, 1.0, 1.0, _ptr(counts), s)

    def plan(n=P, k=keep, w=work, c=count):
        return lib.mm3dgs_compact_plan(n, _ptr(k), _ptr(w), _ptr(c), s)

    def dplan(P_=P, ga=f, de=f, sc=f, w=work, c=count):
        return lib.mm3dgs_densify_plan(P_, _ptr(ga), _ptr(de), _ptr(sc), 0.5, 0.05, _ptr(w), _ptr(c), s)

    bad = {
        "prune: P < 0": lambda: _prune_call(-1, f, f, f, out["keep"], count),
        "prune: NULL opacity": lambda: _prune_call(P, None, f, f, out["keep"], count),
        "prune: NULL scales": lambda: _prune_call(P, f, None, f, out["keep"], count),
        "prune: NULL keep": lambda: _prune_call(P, f, f, f, None, count),
        "prune: NULL counter": lambda: _prune_call(P, f, f, f, out["keep"], None),
        "plan: n = 2^31": lambda: plan(n=BIG),
        "plan: n = (size_t)-1": lambda: plan(n=C.c_size_t(-1).value),
        "plan: NULL keep": lambda: plan(k=None),
        "plan: NULL work": lambda: plan(w=None),
        "plan: NULL count": lambda: plan(c=None),
        "rows: n = 2^31": lambda: lib.mm3dgs_compact_rows(BIG, _ptr(keep), _ptr(work), table(1), 1, s),
        "rows: n_arrays < 0": lambda: lib.mm3dgs_compact_rows(P, _ptr(keep), _ptr(work), table(1), -1, s),
        "rows: 33 arrays": lambda: lib.mm3dgs_compact_rows(P, _ptr(keep), _ptr(work), table(33), 33, s),
        "rows: NULL keep": lambda: lib.mm3dgs_compact_rows(P, None, _ptr(work), table(1), 1, s),
        "rows: NULL work": lambda: lib.mm3dgs_compact_rows(P, _ptr(keep), None, table(1), 1, s),
        "rows: NULL table": lambda: lib.mm3dgs_compact_rows(P, _ptr(keep), _ptr(work), None, 1, s),
        "rows: negative width": lambda: lib.mm3dgs_compact_rows(P, _ptr(keep), _ptr(work), table(2, width=-3), 2, s),
        "rows: NULL src": lambda: lib.mm3dgs_compact_rows(P, _ptr(keep), _ptr(work), table(2, src_ptr=None), 2, s),
        "rows: NULL dst": lambda: lib.mm3dgs_compact_rows(P, _ptr(keep), _ptr(work), table(2, dst_ptr=None), 2, s),
        "seed: H = 0": lambda: seed_call(H=0),
        "seed: W < 0": lambda: seed_call(W=-2),
        "seed: 2^32 pixels": lambda: seed_call(H=1 << 16, W=1 << 16),
        "seed: NULL color": lambda: seed_call(color=None),
        "seed: NULL depth": lambda: seed_call(depth=None),
        "seed: NULL keep": lambda: seed_call(k=None),
        "seed: NULL work": lambda: seed_call(w=None),
        "seed: NULL pose": lambda: seed_call(pose=None),
        "seed: NULL outputs": lambda: seed_call(so=None),
        "seed: NULL xyz": lambda: seed_call(so=seed_out(xyz=1)),
        "seed: NULL rgb": lambda: seed_call(so=seed_out(rgb=1)),
        "seed: NULL f_rest with n_rest": lambda: seed_call(so=seed_out(f_rest=1), n_rest=3),
        "densify plan: P = 2^31": lambda: dplan(P_=BIG),
        "densify plan: NULL grad_accum": lambda: dplan(ga=None),
        "densify plan: NULL denom": lambda: dplan(de=None),
        "densify plan: NULL scales": lambda: dplan(sc=None),
        "densify plan: NULL work": lambda: dplan(w=None),
        "densify plan: NULL counts": lambda: dplan(c=None),
        "densify rows: P = 2^31": lambda: rows_call(P_=BIG, counts=(BIG, 0, 0)),
        "densify rows: N = 0": lambda: rows_call(N_=0),
        "densify rows: N = 65": lambda: rows_call(N_=65),
        "densify rows: N < 0": lambda: rows_call(N_=-1),
        "densify rows: n_keep + n_split != P": lambda: rows_call(counts=(P - 1, 0, 0)),
        "densify rows: n_keep + n_split != P (more)": lambda: rows_call(counts=(P, 0, 1)),
        "densify rows: n_clone > n_keep": lambda: rows_call(counts=(P - 2, P - 1, 2)),
        "densify rows: NULL work": lambda: rows_call(w=None),
        "densify rows: NULL state": lambda: rows_call(st=None),
        "densify rows: NULL grad_accum": lambda: rows_call(st=state(grad_accum=1)),
        "densify rows: NULL max_radii2D": lambda: rows_call(st=state(max_radii2D=1)),
        "densify rows: negative width": lambda: rows_call(st=state(neg=True)),
        "densify rows: NULL src": lambda: rows_call(st=state(null_src=True)),
        "densify rows: moment destination without source": lambda: rows_call(st=state(orphan_moment=True)),
        "densify rows: split with xyz of width 2": lambda: rows_call(counts=(P - 1, 0, 1), st=state(width0=2)),
        "covisibility: H < 0": lambda: covis(H=-1),
        "covisibility: W < 0": lambda: covis(W=-1),
        "covisibility: NULL depth": lambda: covis(depth=None),
        "covisibility: NULL silhouette": lambda: covis(sil=None),
        "covisibility: NULL keyframe pose": lambda: covis(kp=None),
        "covisibility: NULL current pose": lambda: covis(cp=None),
        "covisibility: NULL counts": lambda: covis(counts=None),
    }
    for what, call in bad.items():
        assert call() == -1, what
        assert lib.mm3dgs_last_error(), what
    _sync()
    for name, g in out.items():
        assert g.untouched(), name
    assert all(v.unchanged() for v in src.values()) and f.unchanged() and keep.unchanged()
