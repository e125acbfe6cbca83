"""mm3dgs_nn_grid_build / mm3dgs_nn_query / mm3dgs_mesh_sample_plan / mm3dgs_mesh_sample_emit (csrc/geometry.hip) through the raw C ABI
against the float64 host statement of mm3dgs_slam_amd/geometry.py, at the sizes where a count / scan / scatter build and a ring search can
break (one row, exactly one workgroup and its neighbours, a second round of the 1024-wide scan, queries outside the grid, the termination
bound, ties at max_dist and at the threshold, rows that are not finite); rejected calls; and the evaluation of a native-loop run.

Bars.  dist_out: |device - float64| <= 2^-24 d (1 + 2^-20) -- the one rounding to float32 at the store plus about 10^9 double roundoffs
over the five double operations before it; NaN exactly where the statement has it; the n, within, clamped and skipped counts exact (the
case builders assert that no float64 distance lies within relative 1e-6 of a bar unless it equals it); the row's max = max(dist_out)
exactly; mean and rms within relative 1e-12 (n 2^-53 at n <= 1000, with margin) of float64 numpy over the device's own dist_out.  Sampler:
counts, order and rgba exact against sample_mesh_host; a position component |device - float64| <= 2^-24 |float64| + 2^-45 (|a| + |b| + |c|).
Every test prints its figures (`GEOERR ...`, pytest -s) before it asserts."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import geometry as geo, pointcloud as pc
from tests import geometry_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096               # bytes of guard zone on each side of a work buffer
PAD = 8                    # elements behind every output that no call may touch
SENT = 0x7A7A7A7A          # every int32 of an untouched output element
WORK_SENT = 0xA5           # every byte of the guard zones


def _ptr(t):
    return None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _lib():
    from mm3dgs_slam_amd import _lib
    return _lib.load()


def _stream():
    from mm3dgs_slam_amd.rasterizer import _stream
    return _stream()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(nbytes, fill):
    buf = torch.full((2 * GUARD + nbytes,), WORK_SENT, dtype=torch.uint8, device=DEV)
    buf[GUARD:GUARD + nbytes] = fill
    return buf, buf.data_ptr() + GUARD


def _guards_ok(buf):
    b = buf.cpu().numpy()
    return bool((b[:GUARD] == WORK_SENT).all()) and bool((b[-GUARD:] == WORK_SENT).all())


def _origin(o):
    return (C.c_int64 * 3)(*[int(v) for v in o])


class NN:
    """Caller-owned buffers of one build and one query: sentinel-filled outputs with PAD elements behind them, work buffers between guards."""

    def __init__(self, case, fill=0x00):
        self.case = case
        self.ref, self.q = _dev(case["ref"]), _dev(case["query"])
        self.n_ref, self.n_q = len(case["ref"]), len(case["query"])
        xyz = pc.rows_xyz(case["ref"]).astype(np.float64)
        fin = xyz[np.isfinite(xyz).all(1)]
        self.cell, self.o, self.dims = geo.grid_for(fin.min(0), fin.max(0), case["cell"])
        self.nc = self.dims[0] * self.dims[1] * self.dims[2]
        self.cell_start = torch.full((self.nc + 1 + PAD,), SENT, dtype=torch.int32, device=DEV)
        self.sorted = torch.full((self.n_ref + PAD, 4), SENT, dtype=torch.int32, device=DEV)
        self.counters = torch.full((8 + PAD,), -7, dtype=torch.int64, device=DEV)
        self.dist = torch.full((self.n_q + PAD,), SENT, dtype=torch.int32, device=DEV)
        self.row = torch.full((2 * (8 + PAD),), SENT, dtype=torch.int32, device=DEV)
        lib = _lib()
        self.ngw, self.nqw = int(lib.mm3dgs_nn_grid_work_bytes(self.n_ref, *self.dims)), int(lib.mm3dgs_nn_query_work_bytes(self.n_q))
        assert self.ngw > 0 and self.ngw % 8 == 0 and self.nqw > 0 and self.nqw % 8 == 0
        self.gbuf, self.gwork = _guarded(self.ngw, fill)
        self.qbuf, self.qwork = _guarded(self.nqw, fill)

    def build(self, **over):
        a = dict(n_ref=self.n_ref, rows=self.ref, cell=self.cell, origin=_origin(self.o), gx=self.dims[0], gy=self.dims[1], gz=self.dims[2],
                 cell_start=self.cell_start, sorted=self.sorted, counters=self.counters, work=self.gwork)
        a.update(over)
        rc = _lib().mm3dgs_nn_grid_build(a["n_ref"], _ptr(a["rows"]), a["cell"], a["origin"], a["gx"], a["gy"], a["gz"], _ptr(a["cell_start"]), _ptr(a["sorted"]),
                                         _ptr(a["counters"]), _ptr(a["work"]), _stream())
        torch.cuda.synchronize()
        return rc

    def query(self, **over):
        c = self.case
        a = dict(n_q=self.n_q, q=self.q, n_ref=self.n_ref, cell=self.cell, origin=_origin(self.o), gx=self.dims[0], gy=self.dims[1], gz=self.dims[2],
                 cell_start=self.cell_start, sorted=self.sorted, max_dist=c["max_dist"], threshold=c["threshold"], dist=self.dist, row=self.row, work=self.qwork)
        a.update(over)
        rc = _lib().mm3dgs_nn_query(a["n_q"], _ptr(a["q"]), a["n_ref"], a["cell"], a["origin"], a["gx"], a["gy"], a["gz"], _ptr(a["cell_start"]), _ptr(a["sorted"]),
                                    a["max_dist"], a["threshold"], _ptr(a["dist"]), _ptr(a["row"]), _ptr(a["work"]), _stream())
        torch.cuda.synchronize()
        return rc

    def snapshot(self):
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("cell_start", "sorted", "counters", "dist", "row", "gbuf", "qbuf")}

    def read(self):
        """(dist float32 [n_q], row float64 [8], counters int64 [8], cell_start, sorted) after the guards and the sentinels were checked."""
        s = self.snapshot()
        assert _guards_ok(self.gbuf) and _guards_ok(self.qbuf), "a guard zone of a work buffer was written"
        assert bool((s["cell_start"][self.nc + 1:] == SENT).all()) and bool((s["counters"][8:] == -7).all()), "elements behind cell_start / counters were written"
        assert bool((s["dist"][self.n_q:] == SENT).all()) and bool((s["row"][16:] == SENT).all()), "elements behind dist_out / row were written"
        n_in = int(s["counters"][0])
        assert bool((s["sorted"][n_in:] == SENT).all()), "records behind the count were written"
        return s["dist"][:self.n_q].view(np.float32).copy(), s["row"][:16].view(np.float64).copy(), s["counters"][:8].copy(), s["cell_start"][:self.nc + 1].copy(), s["sorted"][:n_in].copy()


def _check_nn(name, case, fill=0x00):
    nn = NN(case, fill)
    assert nn.build() == 0 and nn.query() == 0
    dist, row, counters, cell_start, srt = nn.read()
    want, clamped, d64 = geo.nn_brute_host(case["query"], case["ref"], case["max_dist"])
    rxyz = pc.rows_xyz(case["ref"])
    rfin = np.isfinite(rxyz).all(1)
    # the grid: every finite reference row once, in its cell
    assert counters.tolist() == [int(rfin.sum()), int((~rfin).sum()), 0, nn.nc, 0, 0, 0, 0], counters
    assert cell_start[0] == 0 and cell_start[-1] == counters[0] and bool((np.diff(cell_start) >= 0).all())
    assert sorted(srt[:, 3].tolist()) == np.flatnonzero(rfin).tolist() and np.array_equal(srt[:, :3], case["ref"][srt[:, 3], :3])
    cells = np.floor(pc.rows_xyz(srt).astype(np.float64) / nn.cell).astype(np.int64) - nn.o
    lin = (cells[:, 2] * nn.dims[1] + cells[:, 1]) * nn.dims[0] + cells[:, 0]
    assert bool((np.diff(lin) >= 0).all()) and np.array_equal(np.searchsorted(lin, np.arange(nn.nc + 1), "left"), cell_start)
    # the distances
    nan_same = np.array_equal(np.isnan(dist), np.isnan(want))
    scored = ~np.isnan(want)
    f64 = np.minimum(d64[scored], case["max_dist"])
    err, bound = np.abs(dist[scored].astype(np.float64) - f64), 2.0 ** -24 * f64 * (1 + 2.0 ** -20)
    n = int(scored.sum())
    within = int((dist[scored] <= np.float32(case["threshold"])).sum())
    d = dist[scored].astype(np.float64)
    mean, rms = (d.sum() / n, np.sqrt((d * d).sum() / n)) if n else (0.0, 0.0)
    rel = lambda a, b: abs(a - b) / b if b else abs(a - b)
    print(f"GEOERR nn {name} fill {fill:#04x}: {nn.n_ref} x {nn.n_q}, grid {nn.dims}; max err / bound = {float((err / np.maximum(bound, 1e-300)).max()) if n else 0.0:.3f}; "
          f"{int((dist.view(np.int32) != want.view(np.int32)).sum())} stored values differ from the host's float32; row {row.tolist()}; want n {n} within {within} "
          f"clamped {int(clamped.sum())} skipped {int((~scored).sum())}; mean rel {rel(row[1], mean):.2e} rms rel {rel(row[2], rms):.2e}")
    assert nan_same and bool((err <= bound).all())
    assert row[0] == n and row[5] == int(clamped.sum()) and row[6] == int((~scored).sum()) and row[7] == 0
    assert row[4] == (within / n if n else 0.0) and within == int((want[scored] <= np.float32(case["threshold"])).sum())
    assert row[3] == (float(dist[scored].max()) if n else 0.0)
    assert rel(row[1], mean) <= 1e-12 and rel(row[2], rms) <= 1e-12
    assert np.array_equal(dist[clamped], np.full(int(clamped.sum()), np.float32(case["max_dist"])))
    return nn, dist, row


@pytest.fixture(scope="module")
def nn_cases():
    return cases.nn_cases()


@pytest.mark.parametrize("n_q", cases.SIZES)
@pytest.mark.parametrize("n_ref", cases.SIZES)
def test_nn_sizes_against_float64_brute_force(n_ref, n_q):
    _check_nn(f"sized {n_ref} x {n_q}", cases.sized_case(n_ref, n_q), fill=0xFF if (n_ref + n_q) % 2 else 0x00)


@pytest.mark.parametrize("name", ("300 references in one cell", "one reference per cell of 5 x 4 x 3", "64 x 64 x 65 cells", "termination bound", "edges"))
def test_nn_edge_cases_against_float64_brute_force(nn_cases, name):
    case = nn_cases[name]
    nn, dist, row = _check_nn(name, case)
    _check_nn(name, case, fill=0xFF)      # the work buffers' contents are irrelevant: zeros, and NaN bytes
    if name == "termination bound":
        assert dist.tolist() == [1.1875]
    if name == "edges":
        q = pc.rows_xyz(case["query"]).astype(np.float64)
        at = lambda y: int(np.flatnonzero((q[:, 1] == y) & (q[:, 0] == 0) & (q[:, 2] == 0))[0])
        assert dist[at(12.0)] == np.float32(0.5) and dist[at(16.0)] == np.float32(0.5) and row[5] == 13 and row[6] == 3
        assert dist[at(20.0)] == np.float32(0.125) and dist[at(24.0)] == np.float32(0.125 + 2.0 ** -22) and int((dist == 0).sum()) == 2
    # the same bytes on a second call, and with the reference rows permuted
    before = nn.snapshot()
    assert nn.build() == 0 and nn.query() == 0
    after = nn.snapshot()
    assert before["dist"].tobytes() == after["dist"].tobytes() and before["row"].tobytes() == after["row"].tobytes()
    perm = np.random.default_rng(3).permutation(len(case["ref"]))
    other = NN(dict(case, ref=case["ref"][perm]))
    assert other.build() == 0 and other.query() == 0
    d2, r2 = other.read()[:2]
    assert d2.tobytes() == dist.tobytes() and r2.tobytes() == row.tobytes()


class Sampler:
    def __init__(self, v, tris, density, seed, cap, fill=0x00):
        self.v, self.tris, self.density, self.seed, self.cap = _dev(v), _dev(tris), float(density), int(seed), int(cap)
        self.nv, self.m = len(v), len(tris)
        self.rows = torch.full((self.cap + PAD, 4), SENT, dtype=torch.int32, device=DEV)
        self.counters = torch.full((8 + PAD,), -7, dtype=torch.int64, device=DEV)
        self.nwork = int(_lib().mm3dgs_mesh_sample_work_bytes(self.m))
        assert self.nwork > 0 and self.nwork % 8 == 0
        self.buf, self.work = _guarded(self.nwork, fill)

    def _args(self, over):
        a = dict(nv=self.nv, v=self.v, m=self.m, tris=self.tris, density=self.density, seed=self.seed, work=self.work, rows=self.rows, cap=self.cap,
                 counters=self.counters)
        a.update(over)
        return a

    def plan(self, **over):
        a = self._args(over)
        rc = _lib().mm3dgs_mesh_sample_plan(a["nv"], _ptr(a["v"]), a["m"], _ptr(a["tris"]), a["density"], a["seed"], _ptr(a["work"]), _ptr(a["counters"]), _stream())
        torch.cuda.synchronize()
        return rc

    def emit(self, **over):
        a = self._args(over)
        rc = _lib().mm3dgs_mesh_sample_emit(a["nv"], _ptr(a["v"]), a["m"], _ptr(a["tris"]), a["density"], a["seed"], _ptr(a["work"]), _ptr(a["rows"]), a["cap"],
                                            _ptr(a["counters"]), _stream())
        torch.cuda.synchronize()
        return rc

    def snapshot(self):
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("rows", "counters", "buf")}

    def read(self):
        s = self.snapshot()
        c = s["counters"][:8]
        assert _guards_ok(self.buf), "a guard zone of the work buffer was written"
        assert bool((s["counters"][8:] == -7).all()) and bool((s["rows"][int(c[2]):] == SENT).all()), "elements behind the outputs were written"
        return s["rows"][:int(c[2])].copy(), c.copy()


def _check_sampler(name, v, tris, density, seed, cap=None, fill=0x00):
    want, wc, f = geo.sample_mesh_host(v, tris, density, seed, full=True)
    total = wc["samples"]
    cap = total if cap is None else cap
    s = Sampler(v, tris, density, seed, cap, fill)
    assert s.plan() == 0
    planned = s.counters.cpu().numpy()[:8].tolist()
    assert s.emit() == 0
    rows, c = s.read()
    written = min(total, cap)
    got, ref = pc.rows_xyz(rows).astype(np.float64), f["xyz"][:written]
    err, bound = np.abs(got - ref), 2.0 ** -24 * np.abs(ref) + 2.0 ** -45 * f["scale"][:written]
    print(f"GEOERR sampler {name} fill {fill:#04x}: {len(tris)} triangles, counters {c.tolist()} (host {wc}); max err / bound = "
          f"{float((err / np.maximum(bound, 1e-300)).max()) if written else 0.0:.3f}; {int((rows[:, :3] != want[:written, :3]).sum())} of {3 * written} components "
          f"differ from the host's float32")
    assert planned == [total, wc["degenerate"], 0, 0, len(tris), 0, 0, 0]
    assert c.tolist() == [total, wc["degenerate"], written, total - written, len(tris), 0, 0, 0]
    assert np.array_equal(rows[:, 3], want[:written, 3])      # rgba exact; with the counts: the host's triangles in the host's order
    assert bool((err <= bound).all())
    return s, rows


@pytest.mark.parametrize("m", (1, 255, 256, 257))
def test_sampler_sizes_against_the_host_statement(m):
    v, tris = cases.random_mesh(m, seed=m)
    _check_sampler(f"random {m}", v, tris, 150.0, seed=m)
    _check_sampler(f"random {m}", v, tris, 150.0, seed=m + 1, fill=0xFF)


def test_sampler_second_scan_round():
    v, tris = cases.tiny_mesh()
    s, rows = _check_sampler("262400 tiny triangles", v, tris, 1e4, seed=4, fill=0xFF)
    counts = geo.sample_mesh_host(v, tris, 1e4, 4, full=True)[2]["counts"]
    assert set(np.unique(counts).tolist()) == {0, 1} and 0.4 < counts.mean() < 0.6
    before = s.snapshot()
    assert s.plan() == 0 and s.emit() == 0
    after = s.snapshot()
    assert before["rows"].tobytes() == after["rows"].tobytes() and before["counters"].tobytes() == after["counters"].tobytes()


@pytest.mark.parametrize("where", ("first", "last"))
def test_sampler_wall_between_empty_triangles(where):
    v, tris = cases.wall_mesh(where)
    _, rows = _check_sampler(f"wall {where}", v, tris, 100.0, seed=6)
    f = geo.sample_mesh_host(v, tris, 100.0, 6, full=True)[2]
    t = 0 if where == "first" else len(tris) - 1
    assert f["counts"][t] in (400, 401) and f["counts"].sum() - f["counts"][t] <= 2 and len(rows) == f["counts"].sum()


def test_sampler_degenerate_triangles_and_cap():
    v, tris, kinds = cases.degenerate_mesh()
    _, rows = _check_sampler("degenerate", v, tris, 100.0, seed=2)
    assert len(rows) > 0
    v, tris = cases.random_mesh(257, seed=1)
    total = geo.sample_mesh_host(v, tris, 150.0, 11)[1]["samples"]
    for cap in (0, 1, 255, 256, total - 1):
        _check_sampler(f"cap {cap} of {total}", v, tris, 150.0, seed=11, cap=cap)


def test_rejected_calls_return_minus_one_and_write_nothing(nn_cases):
    lib = _lib()
    nn = NN(nn_cases["one reference per cell of 5 x 4 x 3"])
    assert nn.build() == 0 and nn.query() == 0
    v, tris = cases.random_mesh(257, seed=1)
    s = Sampler(v, tris, 150.0, 11, 4096)
    assert s.plan() == 0 and s.emit() == 0
    before = dict(nn.snapshot(), **{"s_" + k: a for k, a in s.snapshot().items()})
    nan, inf = float("nan"), float("inf")
    bad_build = {"n_ref = 0": dict(n_ref=0), "n_ref > 2^30": dict(n_ref=(1 << 30) + 1), "gx = 0": dict(gx=0), "more than 2^26 cells": dict(gx=512, gy=512, gz=257),
                 "cell = 0": dict(cell=0.0), "cell < 0": dict(cell=-0.25), "cell NaN": dict(cell=nan), "cell inf": dict(cell=inf), "NULL origin": dict(origin=None),
                 "origin beyond 2^40": dict(origin=_origin([1 << 41, 0, 0])), "NULL rows": dict(rows=None), "NULL cell_start": dict(cell_start=None),
                 "NULL sorted": dict(sorted=None), "NULL counters": dict(counters=None), "NULL work": dict(work=None),
                 "misaligned rows": dict(rows=nn.ref.data_ptr() + 8), "misaligned sorted": dict(sorted=nn.sorted.data_ptr() + 8),
                 "misaligned counters": dict(counters=nn.counters.data_ptr() + 4), "misaligned work": dict(work=nn.gwork + 4),
                 "misaligned cell_start": dict(cell_start=nn.cell_start.data_ptr() + 2)}
    for what, over in bad_build.items():
        assert nn.build(**over) == -1, what
        assert lib.mm3dgs_last_error(), what
    bad_query = {"n_q = 0": dict(n_q=0), "n_ref = 0": dict(n_ref=0), "gz = 0": dict(gz=0), "more than 2^26 cells": dict(gx=512, gy=512, gz=257),
                 "cell = 0": dict(cell=0.0), "cell NaN": dict(cell=nan), "max_dist = 0": dict(max_dist=0.0), "max_dist < 0": dict(max_dist=-1.0),
                 "max_dist NaN": dict(max_dist=nan), "max_dist inf": dict(max_dist=inf), "more than 2^20 rings": dict(cell=1e-9), "threshold NaN": dict(threshold=nan),
                 "threshold < 0": dict(threshold=-0.5), "NULL origin": dict(origin=None), "NULL q": dict(q=None), "NULL cell_start": dict(cell_start=None),
                 "NULL sorted": dict(sorted=None), "NULL dist": dict(dist=None), "NULL row": dict(row=None), "NULL work": dict(work=None),
                 "misaligned q": dict(q=nn.q.data_ptr() + 8), "misaligned sorted": dict(sorted=nn.sorted.data_ptr() + 4), "misaligned row": dict(row=nn.row.data_ptr() + 4),
                 "misaligned work": dict(work=nn.qwork + 4), "misaligned dist": dict(dist=nn.dist.data_ptr() + 2), "misaligned cell_start": dict(cell_start=nn.cell_start.data_ptr() + 1)}
    for what, over in bad_query.items():
        assert nn.query(**over) == -1, what
        assert lib.mm3dgs_last_error(), what
    bad_sample = {"m = 0": dict(m=0), "m > 2^30": dict(m=(1 << 30) + 1), "n_vertices = 0": dict(nv=0), "density = 0": dict(density=0.0), "density < 0": dict(density=-1.0),
                  "density NaN": dict(density=nan), "density inf": dict(density=inf), "NULL vrows": dict(v=None), "NULL triangles": dict(tris=None), "NULL work": dict(work=None),
                  "NULL counters": dict(counters=None), "misaligned vrows": dict(v=s.v.data_ptr() + 8), "misaligned triangles": dict(tris=s.tris.data_ptr() + 2),
                  "misaligned work": dict(work=s.work + 4), "misaligned counters": dict(counters=s.counters.data_ptr() + 4)}
    for what, over in bad_sample.items():
        assert s.plan(**over) == -1, what
        assert s.emit(**over) == -1, what
        assert lib.mm3dgs_last_error(), what
    for what, over in {"NULL rows": dict(rows=None), "misaligned rows": dict(rows=s.rows.data_ptr() + 8), "cap > 2^31": dict(cap=(1 << 31) + 1)}.items():
        assert s.emit(**over) == -1, what
    torch.cuda.synchronize()
    now = dict(nn.snapshot(), **{"s_" + k: a for k, a in s.snapshot().items()})
    for k, a in before.items():
        assert now[k].tobytes() == a.tobytes(), k
    assert int(lib.mm3dgs_nn_grid_work_bytes(0, 5, 4, 3)) == 0 and int(lib.mm3dgs_nn_grid_work_bytes(10, 512, 512, 257)) == 0
    assert int(lib.mm3dgs_nn_query_work_bytes(0)) == 0 and int(lib.mm3dgs_mesh_sample_work_bytes(0)) == 0
    assert nn.build() == 0 and nn.query() == 0 and s.plan() == 0 and s.emit() == 0


def pair_fault_texts(who, index=False, tri=False):
    """(overrides, mm3dgs_last_error() text) of single faults of mm3dgs_nn_query / _index (`who` names the call, index: the longer pointer
    lists) or of mm3dgs_mesh_sample_emit / _tri, for the drivers here and in tests/test_gpu_normals.py.  The texts are the ones api.hip had
    while each member of a pair had a body of its own: they are part of the C ABI's behaviour."""
    if who.startswith("nn_query"):
        return [(dict(n_q=0), f"{who}: n_q = 0 (1 .. 2^30)"), (dict(max_dist=0.0), f"{who}: max_dist = 0 (must be finite and positive)"),
                (dict(gx=512, gy=512, gz=257), f"{who}: grid 512 x 512 x 257 (every size at least 1, at most 2^26 cells)"),
                (dict(dist=None), f"{who}: NULL argument (q_rows, cell_start, sorted, dist_out, {'index_out, ' if index else ''}row and work are required)"),
                ("misaligned dist", f"{who}: cell_start{', dist_out and index_out' if index else ' and dist_out'} must be 4-byte aligned")]
    return [(dict(cap=(1 << 31) + 1), f"{who}: cap = 2147483649 (at most 2^31)"), (dict(density=0.0), f"{who}: density = 0 (must be finite and positive)"),
            (dict(m=0), f"{who}: m = 0 triangles (1 .. 2^30)"), (dict(rows=None), f"{who}: rows {'or tri_out ' if tri else ''}is NULL with a cap above 0"),
            ("misaligned rows", f"{who}: rows must be 16-byte aligned")]


def test_pair_fault_texts(nn_cases):
    nn = NN(nn_cases["one reference per cell of 5 x 4 x 3"])
    assert nn.build() == 0
    for over, text in pair_fault_texts("nn_query"):
        over = dict(dist=nn.dist.data_ptr() + 2) if over == "misaligned dist" else over
        assert nn.query(**over) == -1 and _lib().mm3dgs_last_error().decode() == text, over
    s = Sampler(*cases.random_mesh(257, seed=1), 150.0, 11, 4096)
    assert s.plan() == 0
    for over, text in pair_fault_texts("mesh_sample_emit"):
        over = dict(rows=s.rows.data_ptr() + 8) if over == "misaligned rows" else over
        assert s.emit(**over) == -1 and _lib().mm3dgs_last_error().decode() == text, over


def test_python_surface_matches_the_host_path():
    """GeometryScorer / sample_mesh_device / compare_device against compare_host: the same counts, and figures that differ by the float32
    roundings of individual stored distances only (the sets are the same bytes: the device's samples are compared against the host's)."""
    a, b = cases.square_mesh(0.0), cases.square_mesh(float(np.float32(0.03)))
    rows_dev, c = geo.sample_mesh_device(a[0], a[1], 2000.0, seed=1, device=DEV)
    rows_host = geo.sample_mesh_host(a[0], a[1], 2000.0, seed=1)[0]
    assert c["samples"] == len(rows_host) and np.array_equal(rows_dev.cpu().numpy()[:, 3], rows_host[:, 3])
    dev = geo.compare(rows_host, b, device=DEV, threshold=0.05, max_dist=1.0, density=2000.0, seed=0)
    host = geo.compare(dev["estimate_rows"].cpu().numpy(), dev["reference_rows"].cpu().numpy(), device="cpu", threshold=0.05, max_dist=1.0)
    print(f"GEOERR python surface: device table {dev['table'].tolist()}, host table {host['table'].tolist()}")
    assert np.array_equal(dev["table"][:, [0, 4, 5, 6, 7]], host["table"][:, [0, 4, 5, 6, 7]])
    assert np.allclose(dev["table"][:, 1:4], host["table"][:, 1:4], rtol=2.0 ** -23, atol=0)
    assert dev["dist_estimate"].is_cuda and dev["dist_estimate"].shape[0] == len(rows_host) and dev["cells"] == [0.05, 0.05]
    # a reference without a finite point: every finite query is clamped
    none = geo.compare(rows_host, cases.rows_of([[np.nan, 0, 0]]), device=DEV, threshold=0.05, max_dist=1.0)
    assert none["table"][0, 5] == len(rows_host) and none["accuracy"] == 1.0 and none["counters"]["reference_skipped"] == 1


PARENT_KEYS = ["pose_est", "pose_gt", "keyframes", "ate_rmse", "psnr_list", "ssim_list", "lpips_list"]
MESH = {"voxel": 0.08, "export": False}
GEO = {"density": 2000.0, "threshold": 0.05, "max_dist": 1.0}


def _run(tmp, evaluate, frames=4):
    """The small native run of tests/test_gpu_mesh.py::_run (48 x 64, 4 frames, 5 / 6 iterations, kf_every 2), with the geometry block."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device=DEV, height=48, width=64, tracking={"iters": 5}, mapping={"iters": 6, "kf_every": 2, "min_covisibility": 2.0},
                         outputdir=str(tmp), debug={"get_runtime_stats": False, "create_video": False, "save_keyframes": False},
                         eval_every=1, eval_on_device=False, mesh=dict(MESH), geometry=dict(GEO, eval=evaluate))
    seq = SyntheticSequence(cfg, frames, 2000, seed=5)
    slam = SLAM(cfg, seq)
    from mm3dgs_slam_amd.fused import FusedMapper, FusedTracker
    assert isinstance(slam.tracker, FusedTracker) and isinstance(slam.mapper, FusedMapper)
    slam.run()
    return slam, seq, cfg


def test_native_run_scores_its_mesh_and_the_checkpoint_reproduces_it(tmp_path):
    import slam_top
    from tests.test_gpu_mesh import _same
    n = 4
    on_dir, off_dir = tmp_path / "on", tmp_path / "off"
    on, seq, cfg_on = _run(on_dir, True, n)
    off, _, cfg_off = _run(off_dir, False, n)
    a = np.load(on_dir / "results.npz", allow_pickle=True)
    b = np.load(off_dir / "results.npz", allow_pickle=True)
    assert a["pose_est"].shape == (n, 7) and list(a.keys()) == list(b.keys()) == PARENT_KEYS
    for key in PARENT_KEYS:
        assert _same(a[key], b[key]), key
    assert all(torch.equal(p, q) for p, q in zip(on.estimate_pose_list, off.estimate_pose_list))
    assert off.geometry_eval is None and not (off_dir / "geometry").exists() and on.geometry_eval is not None
    raw = (on_dir / "geometry" / "metrics.json").read_bytes()
    m = json.loads(raw)
    print(f"GEOERR run: {json.dumps({k: m[k] for k in ('accuracy', 'completion', 'completion_ratio', 'precision', 'fscore', 'chamfer', 'n_estimate', 'n_reference', 'cells')})}")
    for k in ("accuracy", "completion", "completion_ratio", "recall", "precision", "fscore", "chamfer"):
        assert np.isfinite(m[k]), k
    assert 0 <= m["accuracy"] < 1.0 and 0 <= m["completion"] < 1.0 and m["n_estimate"] > 0 and m["n_reference"] > 0
    assert len(pc.read_ply(str(on_dir / "geometry" / "accuracy.ply"))) == m["n_estimate"]
    assert len(pc.read_ply(str(on_dir / "geometry" / "completion.ply"))) == m["n_reference"]
    # the device's sets through the host statement: the same counts, figures within the float32 rounding of single distances
    r = on.geometry_eval
    host = geo.compare_host(r["estimate_rows"].cpu().numpy(), r["reference_rows"].cpu().numpy(), threshold=0.05, max_dist=1.0)
    print(f"GEOERR run: device table {r['table'].tolist()}, host statement over the same sets {host['table'].tolist()}")
    assert np.array_equal(r["table"][:, [0, 5, 6]], host["table"][:, [0, 5, 6]]) and np.allclose(r["table"][:, 1:4], host["table"][:, 1:4], rtol=2.0 ** -22, atol=0)
    # the checkpoint route, from the files of the run without the block: only geometry/ is added, the same bytes
    before = (off_dir / "results.npz").read_bytes()
    listing = sorted(os.listdir(off_dir))
    ck = slam_top.evaluate_geometry_checkpoint(dict(cfg_off, geometry=dict(GEO, eval=False)), seq)
    assert ck["iteration"] == n
    assert (off_dir / "geometry" / "metrics.json").read_bytes() == raw
    assert (off_dir / "geometry" / "accuracy.ply").read_bytes() == (on_dir / "geometry" / "accuracy.ply").read_bytes()
    assert (off_dir / "results.npz").read_bytes() == before and sorted(os.listdir(off_dir)) == sorted(listing + ["geometry"])
