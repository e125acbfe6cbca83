"""Geometry scores of an exported reconstruction against a reference surface: accuracy, completion, completion ratio, precision, recall,
F-score and Chamfer distance, as every RGB-D SLAM paper that ships a mesh reports them.  Both sides are point sets in the cloud's 16-byte
rows (``[n,4] int32 = {float32 x, y, z; rgba}``, ``pointcloud.rows_xyz`` / ``rows_rgba``); a mesh (vertex rows + ``int32 [m,3]`` triangles,
as ``mesh.read_mesh_ply`` returns them) is first sampled area-uniformly.  On a GPU the nearest-neighbour search and the sampler are HIP
kernels (``csrc/geometry.hip``, ``GeometryScorer`` / ``sample_mesh_device``) and only a small table is read back; ``nn_distances_host`` /
``sample_mesh_host`` / ``compare_host`` are the float64 numpy statement of the same rules: the yardstick of the kernels and the path of
``device: cpu``.

**Point sets.**  A row with a coordinate that is not finite is skipped: on the reference side it is left out of the grid and counted, on
the query side it gets the distance NaN, is left out of every figure and is counted.

**Truncated nearest-neighbour distance.**  ``d(q) = min(max_dist, min_p |q - p|)``, the distance in double from the float32 coordinates
(each coordinate widened, then subtracted; three squares, a sum, a square root), rounded to float32 once, at the store.  q is *clamped* when
the double distance is ``> max_dist`` (an empty neighbourhood included) and *within* when its stored float32 distance is ``<=
float32(threshold)``.

**The search** is a uniform grid over the reference set: ``cell index = floor((double)x / cell) - origin_cell`` per axis, origin and sizes
from the reference's bounding box.  The cells at Chebyshev ring 0, 1, 2, ... around the query's own cell (unclamped: it may lie outside the
grid) are searched, clipped to the grid; the search stops after ring r when ``best <= r cell`` -- every unsearched point is farther, so the
result is exact -- and after ring ``ceil(max_dist / cell)``.  (The kernel searches rings 0 and 1 in one step, starts at the first ring that
touches the grid and also stops when no further ring does: a superset and an empty remainder, the same minimum.)

**One direction's row** is eight float64 values: n scored queries, mean d, rms d, max d, within / n, clamped count, skipped queries, 0 --
over the stored float32 distances widened to double; the four figures are 0 when n is 0.  **A comparison** is the two rows
(estimate -> reference, reference -> estimate) and ``accuracy = row_er[1]``, ``completion = row_re[1]``, ``completion_ratio = recall =
row_re[4]``, ``precision = row_er[4]``, ``fscore = 2 P R / (P + R)`` (0 when P + R = 0), ``chamfer = (accuracy + completion) / 2``.  When
both clamped counts are zero these are the untruncated figures of the literature.

**Surface sampling.**  Per triangle t with corners a, b, c widened to double: ``A = 0.5 |(b - a) x (c - a)|`` and ``n_t = min(floor(A
density + u_t), 2^23)`` with ``u_t = h(seed, t, 0xffffffff) 2^-32`` -- stochastic rounding: the expected count is proportional to the area
and no area prefix sum is needed.  ``n_t = 0``, and the triangle is counted as degenerate, when an index is outside ``[0, n_vertices)``, a
corner is not finite, or A is 0 or not finite.  Sample j of triangle t: ``r1 = h(seed, t, 2j) 2^-32``, ``r2 = h(seed, t, 2j + 1) 2^-32``; if
``r1 + r2 > 1`` both are replaced by ``1 - r``; ``p = a + r1 (b - a) + r2 (c - a)`` in double, rounded once to float32; rgba is that of the
corner with the largest weight among ``(1 - r1 - r2, r1, r2)``, lowest index on a tie (exact comparisons: the weights are multiples of
2^-32).  Samples are ordered by triangle, then j.  ``h(seed, t, k) = mix32(mix32(mix32(seed ^ 0x9e3779b9) + t) + k)`` in uint32
arithmetic, ``mix32(x)``: ``x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16`` (``ms_mix`` / ``ms_hash`` in the
kernel file state the same one).

**Culling** (``cull=``, off by default; ``cull.py`` states the rule).  A reference file covers the whole scene, a run sees part of it: with
the run's views given, both point sets are reduced -- after sampling, before the search -- to the rows at least ``min_views`` views could
have seen (inside a view's frustum; with depth images also not behind the surface the view measured), and every figure, array and file is
about the kept rows."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from .pointcloud import as_np, rows_xyz

ROW_NAMES = ("n", "mean", "rms", "max", "within_ratio", "clamped", "skipped", "reserved")
SAMPLE_COUNTERS = ("samples", "degenerate", "written", "dropped", "triangles", "reserved5", "overflow", "reserved7")
MAX_CELLS = 1 << 26
MAX_RINGS = 1 << 20
TRI_MAX = 1 << 23      # samples of one triangle


# ---- the mixer ------------------------------------------------------------------------------------------------------------------
def mix32(x):
    x = np.asarray(x, dtype=np.uint32).copy().reshape(-1)
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d); x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b); x ^= x >> np.uint32(16)
    return x


def sample_hash(seed, t, k):
    """h(seed, t, k) as uint32 arrays (t, k broadcast)."""
    t, k = np.broadcast_arrays(np.asarray(t, dtype=np.uint32).reshape(-1), np.asarray(k, dtype=np.uint32).reshape(-1))
    s = mix32(np.array([(int(seed) ^ 0x9e3779b9) & 0xffffffff], dtype=np.uint32))
    return mix32(mix32(s + t) + k)


# ---- the grid -------------------------------------------------------------------------------------------------------------------
def grid_for(lo, hi, cell):
    """(cell, origin_cell int64 [3], dims [3]) of the grid over the box lo .. hi (the finite reference positions' minimum and maximum):
    origin = floor(lo / cell), dims = floor(hi / cell) - origin + 1; `cell` is doubled until the grid has at most 2^26 cells."""
    lo, hi, cell = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64), float(cell)
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError(f"cell = {cell} (must be finite and positive)")
    while True:
        o = np.floor(lo / cell)
        dims = np.floor(hi / cell) - o + 1.0
        if np.abs(o).max() < float(1 << 40) and dims[0] * dims[1] * dims[2] <= MAX_CELLS:
            return cell, o.astype(np.int64), [int(v) for v in dims]
        cell *= 2.0


def _finite_rows(rows):
    xyz = rows_xyz(rows)
    return xyz, np.isfinite(xyz).all(1)


def nn_distances_host(query, reference, cell, max_dist, grid=None):
    """(dist float32 [n_q], info): the truncated nearest-neighbour distance of every query row to the reference rows by the ring search of
    the module docstring, in float64; NaN for a skipped query.  info: clamped (bool [n_q]), ref_skipped, cell (the one used), origin_cell,
    dims.  `grid` (cell, origin_cell, dims) overrides the grid taken from the reference's box."""
    qxyz, qfin = _finite_rows(query)
    rxyz, rfin = _finite_rows(reference)
    max_dist = float(max_dist)
    if not (np.isfinite(max_dist) and max_dist > 0):
        raise ValueError(f"max_dist = {max_dist} (must be finite and positive)")
    nq = len(qxyz)
    dist = np.full(nq, np.nan, dtype=np.float32)
    clamped = np.zeros(nq, dtype=bool)
    R = rxyz[rfin].astype(np.float64)
    info = {"clamped": clamped, "ref_skipped": int((~rfin).sum()), "cell": float(cell), "origin_cell": np.zeros(3, dtype=np.int64), "dims": [1, 1, 1]}
    if len(R) == 0:
        dist[qfin] = np.float32(max_dist)
        clamped[qfin] = True
        return dist, info
    cell, o, dims = grid if grid is not None else grid_for(R.min(0), R.max(0), cell)
    info.update(cell=float(cell), origin_cell=np.asarray(o, dtype=np.int64), dims=list(dims))
    g = np.asarray(dims, dtype=np.int64)
    if float(np.ceil(max_dist / cell)) > MAX_RINGS:
        raise ValueError(f"max_dist / cell = {max_dist / cell} (at most 2^20 rings)")
    rmax = max(int(np.ceil(max_dist / cell)), 1)
    rc = np.floor(R / cell).astype(np.int64) - np.asarray(o, dtype=np.int64)
    inside = ((rc >= 0) & (rc < g)).all(1)      # (with an explicit grid a reference point may lie outside it: left out)
    R, rc = R[inside], rc[inside]
    lin = (rc[:, 2] * g[1] + rc[:, 1]) * g[0] + rc[:, 0]
    order = np.argsort(lin, kind="stable")
    R, lin = R[order], lin[order]
    qi = np.flatnonzero(qfin)
    Q = qxyz[qi].astype(np.float64)
    with np.errstate(over="ignore"):
        c = np.floor(Q / cell) - np.asarray(o, dtype=np.float64)
    r0 = np.maximum(np.maximum(-c, c - (g - 1.0)).max(1), 0.0)      # the first ring that touches the grid
    rfar = np.maximum(c, (g - 1.0) - c).max(1)                       # the last one that does
    ci = np.clip(c, -float(1 << 41), float(1 << 41)).astype(np.int64)
    best2 = np.full(len(Q), np.inf)
    active = np.flatnonzero(r0 <= rmax)
    for r in range(0, rmax + 1):
        if not len(active):
            break
        act = active[r0[active] <= r]
        if len(act):
            rng = np.arange(-r, r + 1)
            touches = lambda a, d: bool(((ci[act, a] + d >= 0) & (ci[act, a] + d < g[a])).any())      # (skips offsets that leave the grid for every query)
            for dz in rng:
                if not touches(2, dz):
                    continue
                for dy in rng:
                    if not touches(1, dy):
                        continue
                    for dx in (rng if max(abs(dz), abs(dy)) == r else ((-r, r) if r else (0,))):
                        cc = ci[act] + np.array([dx, dy, dz], dtype=np.int64)
                        ok = ((cc >= 0) & (cc < g)).all(1)
                        if not ok.any():
                            continue
                        ids, cc = act[ok], cc[ok]
                        key = (cc[:, 2] * g[1] + cc[:, 1]) * g[0] + cc[:, 0]
                        b, e = np.searchsorted(lin, key, "left"), np.searchsorted(lin, key, "right")
                        n = e - b
                        if not n.sum():
                            continue
                        owner = np.repeat(np.arange(len(ids)), n)
                        cand = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n) + np.repeat(b, n)
                        d = Q[ids[owner]] - R[cand]
                        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
                        np.minimum.at(best2, ids[owner], d2)
        stop = (np.sqrt(best2[active]) <= r * cell) | (rfar[active] <= r)
        active = active[~stop]
    d = np.sqrt(best2)
    cl = ~(d <= max_dist)
    dist[qi] = np.where(cl, np.float32(max_dist), d.astype(np.float32))
    clamped[qi] = cl
    return dist, info


def nn_brute_host(query, reference, max_dist):
    """The same distances by float64 brute force (tests): (dist float32 [n_q], clamped, the float64 distances before the clamp)."""
    qxyz, qfin = _finite_rows(query)
    rxyz, rfin = _finite_rows(reference)
    R = rxyz[rfin].astype(np.float64)
    d = np.full(len(qxyz), np.inf)
    for k in np.flatnonzero(qfin):
        if len(R):
            e = qxyz[k].astype(np.float64) - R
            d[k] = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]).min())
    cl = qfin & ~(d <= float(max_dist))
    out = np.where(cl, np.float32(max_dist), d.astype(np.float32)).astype(np.float32)
    out[~qfin] = np.nan
    d[~qfin] = np.nan
    return out, cl, d


def kernel_order_sum(values):
    """The float64 sum of one value per query (0 for a skipped one) in mm3dgs_nn_query's fixed order: a balanced binary tree over the 256
    lanes of a workgroup (the wave's DPP sum, then (w0 + w1) + (w2 + w3)); then ng_finish_kernel: lane t adds the workgroups t, t + 256,
    ... in order, and the 256 lanes are added in order.  Padding lanes add 0.0, which changes no sum."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    nb = max((len(v) + 255) // 256, 1)
    a = np.zeros(nb * 256, dtype=np.float64)
    a[:len(v)] = v
    a = a.reshape(nb, 256)
    while a.shape[1] > 1:
        a = a[:, 0::2] + a[:, 1::2]
    rounds = np.zeros(((nb + 255) // 256) * 256, dtype=np.float64)
    rounds[:nb] = a[:, 0]
    lanes = np.zeros(256, dtype=np.float64)
    for chunk in rounds.reshape(-1, 256):
        lanes = lanes + chunk
    return float(np.add.accumulate(lanes)[-1])


def direction_row(dist, clamped, threshold, sum_order="numpy"):
    """The eight figures of one direction from the stored float32 distances (NaN = skipped) and the clamped mask.  `sum_order` "kernel"
    adds the distances and their squares in the kernels' order (``kernel_order_sum``): the mean and the rms then carry the device's
    roundings, and a device table can be held to this one bit for bit; "numpy" (the default, what every output of the host path uses)
    differs from it in the last bits."""
    dist = np.asarray(dist, dtype=np.float32)
    scored = ~np.isnan(dist)
    d = dist[scored].astype(np.float64)
    n = len(d)
    row = np.zeros(8, dtype=np.float64)
    row[0] = n
    if n:
        row[1], row[2], row[3] = d.sum() / n, np.sqrt((d * d).sum() / n), d.max()
        if sum_order == "kernel":
            z = np.where(scored, dist, np.float32(0)).astype(np.float64)
            row[1], row[2] = kernel_order_sum(z) / n, np.sqrt(kernel_order_sum(z * z) / n)
        row[4] = float((dist[scored] <= np.float32(threshold)).sum()) / n
    row[5] = float(np.asarray(clamped, dtype=bool)[scored].sum())
    row[6] = float((~scored).sum())
    return row


def derived_figures(table):
    """The derived values of a [2,8] table (row 0: estimate -> reference, row 1: reference -> estimate)."""
    t = np.asarray(table, dtype=np.float64).reshape(2, 8)
    P, R = float(t[0, 4]), float(t[1, 4])
    return {"accuracy": float(t[0, 1]), "completion": float(t[1, 1]), "completion_ratio": R, "recall": R, "precision": P,
            "fscore": 2.0 * P * R / (P + R) if P + R > 0 else 0.0, "chamfer": 0.5 * (float(t[0, 1]) + float(t[1, 1]))}


# ---- surface sampling ---------------------------------------------------------------------------------------------------------------
def _triangle_counts(vrows, triangles, density, seed):
    xyz = rows_xyz(vrows).astype(np.float64)
    tri = as_np(triangles, np.int32).reshape(-1, 3).astype(np.int64)
    m, nv = len(tri), len(xyz)
    ok = ((tri >= 0) & (tri < nv)).all(1)
    ti = np.where(ok[:, None], tri, 0)
    a, b, c = (xyz[ti[:, k]] if nv else np.zeros((m, 3)) for k in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        ok &= np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1)
        e1, e2 = b - a, c - a
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        A = 0.5 * np.sqrt(cx * cx + cy * cy + cz * cz)
        ok &= (A > 0) & (A < np.inf)
        u = sample_hash(seed, np.arange(m, dtype=np.uint32), np.uint32(0xffffffff)).astype(np.float64) * 2.0 ** -32
        nt = np.where(ok, np.minimum(np.floor(np.where(ok, A, 0.0) * float(density) + u), float(TRI_MAX)), 0.0).astype(np.int64)
    return nt, ok, (a, e1, e2, ti), np.where(ok, A, 0.0)


def sample_mesh_host(vrows, triangles, density, seed=0, cap=None, full=False):
    """(rows [n,4] int32, counters dict): the samples of a mesh by the rules of the module docstring; at most `cap` rows are returned (the
    rest is counted as dropped).  With ``full`` also dict(xyz: the float64 positions, tri: the triangle of every sample, scale: |a| + |b| +
    |c| per sample and component, counts: n_t, area: A per triangle)."""
    density = float(density)
    if not (np.isfinite(density) and density > 0):
        raise ValueError(f"density = {density} (must be finite and positive)")
    vr = as_np(vrows, np.int32).reshape(-1, 4)
    nt, ok, (a, e1, e2, ti), area = _triangle_counts(vr, triangles, density, seed)
    m = len(nt)
    total = int(nt.sum())
    if total > 0xffffffff:
        raise ValueError(f"{total} samples: more than 2^32 - 1; lower the density")
    written = total if cap is None else min(total, int(cap))
    pre = np.cumsum(nt) - nt
    tid = np.repeat(np.arange(m), nt)[:written]
    j = (np.arange(written) - pre[tid]).astype(np.uint32)
    r1 = sample_hash(seed, tid.astype(np.uint32), np.uint32(2) * j).astype(np.float64) * 2.0 ** -32
    r2 = sample_hash(seed, tid.astype(np.uint32), np.uint32(2) * j + np.uint32(1)).astype(np.float64) * 2.0 ** -32
    flip = r1 + r2 > 1.0
    r1, r2 = np.where(flip, 1.0 - r1, r1), np.where(flip, 1.0 - r2, r2)
    w0 = 1.0 - r1 - r2
    xyz = a[tid] + r1[:, None] * e1[tid] + r2[:, None] * e2[tid]
    corner = np.where((w0 >= r1) & (w0 >= r2), 0, np.where(r1 >= r2, 1, 2))
    rows = np.empty((written, 4), dtype=np.int32)
    rows[:, :3] = xyz.astype(np.float32).view(np.int32)
    rows[:, 3] = vr[ti[tid, corner], 3] if written else 0
    counters = {"samples": total, "degenerate": int((~ok).sum()), "written": written, "dropped": total - written, "triangles": m}
    if not full:
        return rows, counters
    av = np.abs(a[tid])
    scale = av + np.abs(a[tid] + e1[tid]) + np.abs(a[tid] + e2[tid])
    return rows, counters, {"xyz": xyz, "tri": tid, "scale": scale, "counts": nt, "area": area}


def sample_mesh_device(vrows, triangles, density, seed=0, max_samples=1 << 24, device="cuda:0"):
    """The device sampler: (rows tensor [n,4] int32 on the device, counters dict) -- one mm3dgs_mesh_sample_plan, one read-back of the
    counter block, the exact allocation, one mm3dgs_mesh_sample_emit.  Raises when the samples exceed `max_samples`."""
    from . import _lib
    from .rasterizer import _stream
    lib, P = _lib.load(), _lib.ptr
    vr = torch.as_tensor(vrows, device=device).to(torch.int32).reshape(-1, 4).contiguous()
    tr = torch.as_tensor(triangles, device=device).to(torch.int32).reshape(-1, 3).contiguous()
    m, nv = int(tr.shape[0]), int(vr.shape[0])
    if m == 0 or nv == 0:
        return torch.empty(0, 4, dtype=torch.int32, device=device), dict(zip(SAMPLE_COUNTERS[:5], (0, m, 0, 0, m)))
    nbytes = int(lib.mm3dgs_mesh_sample_work_bytes(m))
    if nbytes == 0:
        raise ValueError(f"mesh of {m} triangles: at most 2^30")
    work = torch.empty(nbytes // 8, dtype=torch.int64, device=device)
    counters = torch.empty(8, dtype=torch.int64, device=device)
    _lib.check(lib.mm3dgs_mesh_sample_plan(nv, P(vr), m, P(tr), float(density), int(seed) & 0xffffffff, P(work), P(counters), _stream()))
    c = counters.cpu().numpy()      # the one read-back before the allocation
    total = int(c[0])
    if c[6] or total > int(max_samples):
        raise ValueError(f"{total} surface samples at density {density} per m^2: more than max_samples = {int(max_samples)}; lower geometry.density "
                         f"or raise geometry.max_samples")
    rows = torch.empty(max(total, 1), 4, dtype=torch.int32, device=device)
    _lib.check(lib.mm3dgs_mesh_sample_emit(nv, P(vr), m, P(tr), float(density), int(seed) & 0xffffffff, P(work), P(rows), total, P(counters), _stream()))
    return rows[:total], {"samples": total, "degenerate": int(c[1]), "written": total, "dropped": 0, "triangles": m}


# ---- the device path ------------------------------------------------------------------------------------------------------------------
class GeometryScorer:
    """The device search structure of one reference point set: the grid is built once (one read-back of the box and the finite count, then
    one mm3dgs_nn_grid_build); ``query`` is one mm3dgs_nn_query call on the current stream and returns device tensors (dist float32 [n_q],
    row float64 [8]) without a read-back.  For the other direction build a second scorer over the other set."""

    def __init__(self, reference, cell, max_dist, threshold, device="cuda:0"):
        from . import _lib
        from .rasterizer import _stream
        import ctypes as C
        if not str(device).startswith("cuda"):
            raise ValueError("GeometryScorer needs a CUDA device (the host path is nn_distances_host)")
        self.lib, self.device = _lib.load(), device
        self.max_dist, self.threshold = float(max_dist), float(threshold)
        if not (np.isfinite(self.max_dist) and self.max_dist > 0):
            raise ValueError(f"max_dist = {max_dist} (must be finite and positive)")
        self.rows = torch.as_tensor(reference, device=device).to(torch.int32).reshape(-1, 4).contiguous()
        self.n_ref = int(self.rows.shape[0])
        self.ref_skipped, self.grid = 0, None
        self.cell, self.origin_cell, self.dims = float(cell), np.zeros(3, dtype=np.int64), [1, 1, 1]
        if self.n_ref == 0:
            return
        xyz = self.rows[:, :3].view(torch.float32).double()
        fin = torch.isfinite(xyz).all(1, keepdim=True)
        inf = torch.tensor(float("inf"), device=device, dtype=torch.float64)
        box = torch.cat([torch.where(fin, xyz, inf).amin(0), torch.where(fin, xyz, -inf).amax(0), fin.sum().double().reshape(1)]).cpu().numpy()
        self.ref_skipped = self.n_ref - int(box[6])
        if int(box[6]) == 0:
            return
        self.cell, self.origin_cell, self.dims = grid_for(box[:3], box[3:6], cell)
        if float(np.ceil(self.max_dist / self.cell)) > MAX_RINGS:
            raise ValueError(f"max_dist / cell = {self.max_dist / self.cell} (at most 2^20 rings)")
        gx, gy, gz = self.dims
        nbytes = int(self.lib.mm3dgs_nn_grid_work_bytes(self.n_ref, gx, gy, gz))
        if nbytes == 0:
            raise ValueError(f"reference of {self.n_ref} rows over {gx} x {gy} x {gz} cells: at most 2^30 rows and 2^26 cells")
        P = _lib.ptr
        self._origin = (C.c_int64 * 3)(*[int(v) for v in self.origin_cell])
        self.cell_start = torch.empty(gx * gy * gz + 1, dtype=torch.int32, device=device)
        self.sorted = torch.empty(self.n_ref, 4, dtype=torch.int32, device=device)
        self.counters = torch.empty(8, dtype=torch.int64, device=device)
        work = torch.empty(nbytes // 8, dtype=torch.int64, device=device)
        _lib.check(self.lib.mm3dgs_nn_grid_build(self.n_ref, P(self.rows), self.cell, self._origin, gx, gy, gz, P(self.cell_start), P(self.sorted),
                                                 P(self.counters), P(work), _stream()))
        self.grid = True

    def query(self, rows, dist=None, row=None):
        """(dist [n_q] float32, row [8] float64) on the device for the query rows [n_q,4] int32."""
        from . import _lib
        from .rasterizer import _stream
        q = torch.as_tensor(rows, device=self.device).to(torch.int32).reshape(-1, 4).contiguous()
        nq = int(q.shape[0])
        dist = torch.empty(nq, dtype=torch.float32, device=self.device) if dist is None else dist
        row = torch.zeros(8, dtype=torch.float64, device=self.device) if row is None else row
        if nq == 0:
            row.zero_()
            return dist, row
        if self.grid is None:      # no finite reference point: every finite query is clamped (no kernel has anything to search)
            fin = torch.isfinite(q[:, :3].view(torch.float32)).all(1)
            dist.copy_(torch.where(fin, torch.full_like(dist, self.max_dist), torch.full_like(dist, float("nan"))))
            n = fin.sum().double()
            md = float(np.float32(self.max_dist))
            has = (n > 0).double()
            row.copy_(torch.stack([n, has * md, has * md, has * md, has * float(np.float32(md) <= np.float32(self.threshold)), n, nq - n, n * 0]))
            return dist, row
        P = _lib.ptr
        gx, gy, gz = self.dims
        work = torch.empty(int(self.lib.mm3dgs_nn_query_work_bytes(nq)) // 8, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.mm3dgs_nn_query(nq, P(q), self.n_ref, self.cell, self._origin, gx, gy, gz, P(self.cell_start), P(self.sorted), self.max_dist,
                                            self.threshold, P(dist), P(row), P(work), _stream()))
        return dist, row


# ---- comparisons ----------------------------------------------------------------------------------------------------------------------
def _is_mesh(side):
    return isinstance(side, (tuple, list)) and len(side) == 2


def compare_host(estimate, reference, threshold=0.05, max_dist=1.0, cell=0, density=10000.0, seed=0, max_samples=1 << 24, cull=None, sum_order="numpy"):
    """The comparison of the module docstring on the host (`sum_order`: ``direction_row``).  Each side is rows [n,4] int32 or (vertex rows, triangles).  Returns a dict:
    the derived figures, table [2,8], cells (the cell each grid used), counters, n_estimate, n_reference, and the arrays estimate_rows,
    reference_rows, dist_estimate, dist_reference.  `cull` (``cull.spec``: the run's views plus the options; None: off) removes from both
    point sets, after sampling and before the search, what no view could have seen: everything returned is then about the kept points,
    and the result gains `cull` (``cull.summary``) and estimate_index / reference_index (the original row of every kept row)."""
    cell = float(cell) if cell and float(cell) > 0 else float(threshold)
    sets, counters = [], {}
    for name, side in (("estimate", estimate), ("reference", reference)):
        if _is_mesh(side):
            rows, c = sample_mesh_host(side[0], side[1], density, seed)
            if c["samples"] > int(max_samples):
                raise ValueError(f"{c['samples']} surface samples at density {density} per m^2: more than max_samples = {int(max_samples)}")
            counters[name + "_sampler"] = c
        else:
            rows = as_np(side, np.int32).reshape(-1, 4)
        sets.append(rows)
    culled = None
    if cull is not None:
        from . import cull as cl
        (sets[0], ie, ce), (sets[1], ir, cr) = cl.apply_host(sets[0], cull), cl.apply_host(sets[1], cull)
        culled = (cl.summary(cull, ce, cr), ie, ir)
    d_er, i_er = nn_distances_host(sets[0], sets[1], cell, max_dist)
    d_re, i_re = nn_distances_host(sets[1], sets[0], cell, max_dist)
    table = np.stack([direction_row(d_er, i_er["clamped"], threshold, sum_order), direction_row(d_re, i_re["clamped"], threshold, sum_order)])
    counters.update(reference_skipped=i_er["ref_skipped"], estimate_skipped=i_re["ref_skipped"])
    return _result(table, (i_er["cell"], i_re["cell"]), counters, sets, (d_er, d_re), threshold, max_dist, culled)


def compare_device(estimate, reference, threshold=0.05, max_dist=1.0, cell=0, density=10000.0, seed=0, max_samples=1 << 24, device="cuda:0", cull=None):
    """The same comparison on the device: meshes sampled by the kernels, one GeometryScorer per direction, the [2,8] table read back once;
    the rows and distances stay device tensors.  `cull` as in ``compare_host``: one ``cull.Culler`` per side (one mm3dgs_cull_mark_view
    per view, one mm3dgs_cull_select and one read-back of its counters)."""
    cell = float(cell) if cell and float(cell) > 0 else float(threshold)
    sets, counters = [], {}
    for name, side in (("estimate", estimate), ("reference", reference)):
        if _is_mesh(side):
            rows, counters[name + "_sampler"] = sample_mesh_device(side[0], side[1], density, seed, max_samples, device)
        else:
            rows = torch.as_tensor(side, device=device).to(torch.int32).reshape(-1, 4).contiguous()
        sets.append(rows)
    culled = None
    if cull is not None:
        from . import cull as cl
        views = cl.device_views(cull, device)
        (sets[0], ie, ce), (sets[1], ir, cr) = cl.apply_device(sets[0], cull, views, device), cl.apply_device(sets[1], cull, views, device)
        culled = (cl.summary(cull, ce, cr), ie, ir)
    on_ref = GeometryScorer(sets[1], cell, max_dist, threshold, device)
    on_est = GeometryScorer(sets[0], cell, max_dist, threshold, device)
    table = torch.zeros(2, 8, dtype=torch.float64, device=device)
    d_er, _ = on_ref.query(sets[0], row=table[0])
    d_re, _ = on_est.query(sets[1], row=table[1])
    counters.update(reference_skipped=on_ref.ref_skipped, estimate_skipped=on_est.ref_skipped)
    return _result(table.cpu().numpy(), (on_ref.cell, on_est.cell), counters, sets, (d_er, d_re), threshold, max_dist, culled)      # the one read-back


def _result(table, cells, counters, sets, dists, threshold, max_dist, culled=None):
    out = derived_figures(table)
    if culled is not None:
        out.update(cull=culled[0], estimate_index=culled[1], reference_index=culled[2])
    out.update(table=np.asarray(table, dtype=np.float64), cells=[float(c) for c in cells], counters=counters, threshold=float(threshold),
               max_dist=float(max_dist), n_estimate=int(sets[0].shape[0]), n_reference=int(sets[1].shape[0]),
               estimate_rows=sets[0], reference_rows=sets[1], dist_estimate=dists[0], dist_reference=dists[1])
    return out


def compare(estimate, reference, device="cpu", **kw):
    """``compare_device`` on a CUDA device, ``compare_host`` otherwise."""
    if str(device).startswith("cuda"):
        return compare_device(estimate, reference, device=device, **kw)
    return compare_host(estimate, reference, **kw)


def align_rows(rows, est_poses, gt_poses, method):
    """The rows with their positions moved by the trajectory alignment estimate -> ground truth (eval_utils.align_horn / align_umeyama
    of the camera centres of every frame that has an estimated pose; the two lists run frame by frame), applied in torch float64 and
    rounded once to float32."""
    from .eval_utils import align_horn, align_umeyama, camera_centers
    pairs = [(e.detach(), g.detach()) for e, g in zip(est_poses, gt_poses) if e is not None]
    est_c = camera_centers(torch.stack([e for e, _ in pairs]))[:, 4:].numpy()
    gt_c = camera_centers(torch.stack([g for _, g in pairs]))[:, 4:].numpy()
    if method == "horn":
        R, t, _ = align_horn(est_c.T, gt_c.T)
        s = 1.0
    else:
        s, R, t = align_umeyama(gt_c, est_c)
    rows = torch.as_tensor(rows).to(torch.int32).reshape(-1, 4)
    A = torch.tensor(s * np.asarray(R), dtype=torch.float64, device=rows.device)
    b = torch.tensor(np.asarray(t).reshape(3), dtype=torch.float64, device=rows.device)
    xyz = rows[:, :3].contiguous().view(torch.float32).double() @ A.T + b
    return torch.cat([xyz.float().view(torch.int32), rows[:, 3:]], 1).contiguous()


# ---- outputs --------------------------------------------------------------------------------------------------------------------------
def colour_by_distance(rows, dist, threshold):
    """The rows with their colour replaced by viridis(d / (2 threshold)) (debug_frames' table and lookup, bytes rounded; a NaN is black),
    encoded on the host."""
    from .debug_frames import viridis
    rows = as_np(rows, np.int32).reshape(-1, 4).copy()
    d = as_np(dist, np.float32).reshape(-1).astype(np.float64)
    lut = np.floor(viridis().numpy() * 255.0 + 0.5).astype(np.uint32)
    with np.errstate(invalid="ignore"):
        t = np.clip(d / (2.0 * float(threshold)), 0.0, 1.0)
    bad = np.isnan(t)
    idx = np.minimum((np.where(bad, 0.0, t) * 256.0).astype(np.int64), 255)
    rgb = np.where(bad[:, None], 0, lut[idx])
    rows[:, 3] = (rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16) | np.uint32(0xff000000)).astype(np.uint32).view(np.int32)
    return rows


def metrics_dict(result, extra=None):
    """The JSON-ready part of a comparison."""
    out = {k: result[k] for k in ("accuracy", "completion", "completion_ratio", "recall", "precision", "fscore", "chamfer", "threshold", "max_dist",
                                  "cells", "n_estimate", "n_reference", "counters")}
    t = result["table"]
    out["estimate_to_reference"] = {name: float(t[0, k]) for k, name in enumerate(ROW_NAMES[:7])}
    out["reference_to_estimate"] = {name: float(t[1, k]) for k, name in enumerate(ROW_NAMES[:7])}
    if result.get("cull") is not None:
        out["cull"] = result["cull"]
    out.update(extra or {})
    return out


def write_outputs(path, result, extra=None):
    """path/metrics.json, path/accuracy.ply (the estimate's points coloured by distance over [0, 2 threshold]) and path/completion.ply (the
    reference's points likewise).  Returns the three paths."""
    from .pointcloud import write_ply
    os.makedirs(path, exist_ok=True)
    files = {"metrics": os.path.join(path, "metrics.json")}
    with open(files["metrics"], "w") as fh:
        json.dump(metrics_dict(result, extra), fh, indent=1, sort_keys=True)
        fh.write("\n")
    files["accuracy"] = write_ply(os.path.join(path, "accuracy.ply"), colour_by_distance(result["estimate_rows"], result["dist_estimate"], result["threshold"]))
    files["completion"] = write_ply(os.path.join(path, "completion.ply"), colour_by_distance(result["reference_rows"], result["dist_reference"], result["threshold"]))
    return files
