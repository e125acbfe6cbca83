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
about the kept rows.

**Normals** (``normals=`` / ``vertex_normals``, both opt-in; the kernels and the numpy statement follow the rules below).

*Face cross product.*  ``c_t = (b - a) x (c - a)`` from the float32 corners widened to double, no contraction, exactly as the sampler's
area forms it (``ms_cross`` on the device, ``_face_cross`` here: one statement for the area, the consistency and the vertex normals).  A
triangle is *rejected* when the sampler's load rejects it (an index outside ``[0, n_vertices)``, a corner that is not finite) or when
``c . c`` is 0 or not finite.

*Nearest row.*  ``nn_index_host`` / mm3dgs_nn_query_index do the search above and also give ``index[i]`` (uint32): the original
reference row of the record with the smallest double squared distance, the smallest row on an exact tie (so duplicates in the reference
are decided), ``0xffffffff`` when the query is skipped or clamped.  The ring stop rule leaves only strictly farther records unsearched, so
the lexicographic minimum over ``(d2, row)`` of the searched records is the global one.  The distances and the row are those of the
search without the index.  *Sample -> triangle*: the sampler also gives the triangle of every sample (``sample_mesh_host(full=True)``:
``tri``; mm3dgs_mesh_sample_emit_tri: ``tri_out``).

*One direction's normal row.*  For query i with its triangle ``tq``, its nearest row ``j = index[i]`` and that row's triangle ``tr``:
``dot = (c_tq . c_tr) / (sqrt(c_tq . c_tq) sqrt(c_tr . c_tr))`` in double, clamped to [-1, 1], rounded once to float32 at the store.  The
dot is NaN and the query is not counted when j is none (this test comes first), or when j or a triangle id is out of range or a triangle
is rejected (nothing is read for such ids).  The row is eight float64 values over the stored float32 dots widened to double, summed in
``kernel_order_sum``'s order on the device: n counted, mean |dot|, mean dot, min |dot|, 0, not counted: no neighbour, not counted:
bad triangle, 0; the means and the min are 0 when n is 0 (``normal_row``, the twin of ``direction_row``).  ``normal_accuracy =
row_er[1]``, ``normal_completion = row_re[1]``, ``normal_consistency = (normal_accuracy + normal_completion) / 2``, and the same three
from field 2 as ``*_signed``.  |dot| is the headline because a dataset's mesh and a TSDF mesh need not share an orientation (what
Occupancy Networks' evaluator does for meshes that are not watertight).  The normal under a sample is its face's, recomputed from the
faces: a file's stored normals are never used.

*Vertex normals* are area-weighted, and no order of arrival changes a bit: every triangle t that is not rejected has ``E_t``, the binary
exponent of ``max(|c_x|, |c_y|, |c_z|)`` as ``frexp`` returns it; ``E_v = max E_t`` over the triangles with corner v; every such triangle
adds ``llrint(ldexp(c_k, 40 - E_v))``, k = x, y, z, to three int64 sums ``S_v`` (a term is below 2^40, so the sums are exact up to a valence
of 2^22 and wrap in two's complement beyond); ``n_v = S_v / sqrt(S_v . S_v)`` in double from the sums converted to double, rounded once
to float32; ``(0, 0, 0)``, and counted, when v has no such triangle or ``S_v = 0``.

**Registration** (``icp_host`` / mm3dgs_icp_point, ``register``; opt-in, `geometry.icp: point`).  NICE-SLAM's ``eval_recon`` registers the
reconstruction to the ground truth by point-to-point ICP (Open3D ``registration_icp``: correspondence distance 0.1 m, identity start, 30
iterations, 1e-6 / 1e-6) before it measures a distance.  The rule here: source rows are the estimate, the target set is the reference,
the state is ``T = (R, t)`` (twelve doubles, row-major [3,4]) and pass k = 0, 1, ... is

1. *move and search*: every finite source row p (widened) gives ``p' = ((R0 p.x + R1 p.y) + R2 p.z) + t`` per component, no contraction,
   rounded once to float32 (``move_rows_host``); the correspondence of p is what ``nn_index_host`` returns for the row p' with
   ``max_dist = icp_max_dist`` -- the same grid, rings, stop rule and lexicographic minimum over ``(d2, original row)``; none for a
   clamped row or one that is not finite;
2. *sum*, over the rows with a correspondence q and with p the ORIGINAL coordinates (so a solve gives the absolute transform and nothing
   is composed): n, sum p, sum q, the nine sums ``p_a q_b`` (each product rounded, then added) and sum d2 (the double squared distance of
   the search), 17 in all, in ``kernel_order_sum``'s order on the device; with them the finite source rows;
3. *figures*: ``fitness = n / finite rows``, ``rmse = sqrt(sum d2 / n)``, 0 with n = 0 -- those of the T the pass started with;
4. *stop*: status 0 when k > 0 and ``|fitness_k - fitness_{k-1}| < rel_fitness`` and ``|rmse_k - rmse_{k-1}| < rel_rmse`` (Open3D's
   absolute differences); else status 2 when n < 3; else status 1 when k == iters.  T stays: the last pass only evaluates, and the
   reported figures belong to the returned T;
5. *solve* otherwise (``_horn_solve``, ``icp_horn`` on the device: one sequence of ``+ - x / sqrt``, so the two agree bit for bit):
   ``S = sum p q^T - sum p sum q^T / n``, Horn's symmetric 4 x 4 matrix N(S), its dominant eigenvector by cyclic Jacobi rotations,
   ``w >= 0``, normalised; R from the quaternion, ``t = sum q / n - R sum p / n``."""
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
NO_INDEX = np.uint32(0xffffffff)      # no nearest row: the query is skipped or clamped
NORMAL_ROW_NAMES = ("n", "mean_abs_dot", "mean_dot", "min_abs_dot", "reserved4", "no_neighbour", "bad_triangle", "reserved7")
NORMAL_COUNTERS = ("vertices", "without_normal", "rejected_triangles")
FRAC_BITS = 40         # fixed-point bits of the vertex-normal sums below a vertex's largest face exponent


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
    return _nn_search(query, reference, cell, max_dist, grid, False)[::2]


def nn_index_host(query, reference, cell, max_dist, grid=None):
    """(dist, index uint32 [n_q], info): ``nn_distances_host`` (the same distances and info) with the nearest row of the module docstring:
    the original reference row of the smallest float64 squared distance, the smallest row on a tie, NO_INDEX for a skipped or clamped
    query."""
    return _nn_search(query, reference, cell, max_dist, grid, True)


def _nn_search(query, reference, cell, max_dist, grid, want_index):
    qxyz, qfin = _finite_rows(query)
    rxyz, rfin = _finite_rows(reference)
    max_dist = float(max_dist)
    if not (np.isfinite(max_dist) and max_dist > 0):
        raise ValueError(f"max_dist = {max_dist} (must be finite and positive)")
    nq = len(qxyz)
    dist = np.full(nq, np.nan, dtype=np.float32)
    index = np.full(nq, NO_INDEX, dtype=np.uint32)
    clamped = np.zeros(nq, dtype=bool)
    R = rxyz[rfin].astype(np.float64)
    orig = np.flatnonzero(rfin)
    info = {"clamped": clamped, "ref_skipped": int((~rfin).sum()), "cell": float(cell), "origin_cell": np.zeros(3, dtype=np.int64), "dims": [1, 1, 1]}
    if len(R) == 0:
        dist[qfin] = np.float32(max_dist)
        clamped[qfin] = True
        return dist, index, info
    cell, o, dims = grid if grid is not None else grid_for(R.min(0), R.max(0), cell)
    info.update(cell=float(cell), origin_cell=np.asarray(o, dtype=np.int64), dims=list(dims))
    g = np.asarray(dims, dtype=np.int64)
    if float(np.ceil(max_dist / cell)) > MAX_RINGS:
        raise ValueError(f"max_dist / cell = {max_dist / cell} (at most 2^20 rings)")
    rmax = max(int(np.ceil(max_dist / cell)), 1)
    rc = np.floor(R / cell).astype(np.int64) - np.asarray(o, dtype=np.int64)
    inside = ((rc >= 0) & (rc < g)).all(1)      # (with an explicit grid a reference point may lie outside it: left out)
    R, rc, orig = R[inside], rc[inside], orig[inside]
    lin = (rc[:, 2] * g[1] + rc[:, 1]) * g[0] + rc[:, 0]
    order = np.argsort(lin, kind="stable")
    R, lin, orig = R[order], lin[order], orig[order]
    qi = np.flatnonzero(qfin)
    Q = qxyz[qi].astype(np.float64)
    with np.errstate(over="ignore"):
        c = np.floor(Q / cell) - np.asarray(o, dtype=np.float64)
    r0 = np.maximum(np.maximum(-c, c - (g - 1.0)).max(1), 0.0)      # the first ring that touches the grid
    rfar = np.maximum(c, (g - 1.0) - c).max(1)                       # the last one that does
    ci = np.clip(c, -float(1 << 41), float(1 << 41)).astype(np.int64)
    best2 = np.full(len(Q), np.inf)
    besti = np.full(len(Q), int(NO_INDEX), dtype=np.int64)
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
                        before = best2[ids]
                        np.minimum.at(best2, ids[owner], d2)
                        if want_index:      # the lexicographic minimum over (d2, original row)
                            besti[ids[best2[ids] < before]] = int(NO_INDEX)
                            hit = d2 == best2[ids[owner]]
                            np.minimum.at(besti, ids[owner][hit], orig[cand[hit]])
        stop = (np.sqrt(best2[active]) <= r * cell) | (rfar[active] <= r)
        active = active[~stop]
    d = np.sqrt(best2)
    cl = ~(d <= max_dist)
    dist[qi] = np.where(cl, np.float32(max_dist), d.astype(np.float32))
    clamped[qi] = cl
    index[qi] = np.where(cl, int(NO_INDEX), besti).astype(np.uint32)
    return dist, index, info


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


def nn_index_brute_host(query, reference, max_dist):
    """``nn_index_host`` by float64 brute force (tests): (dist float32 [n_q], index uint32 [n_q])."""
    qxyz, qfin = _finite_rows(query)
    rxyz, rfin = _finite_rows(reference)
    orig = np.flatnonzero(rfin)
    R = rxyz[rfin].astype(np.float64)
    dist = np.full(len(qxyz), np.nan, dtype=np.float32)
    index = np.full(len(qxyz), NO_INDEX, dtype=np.uint32)
    for k in np.flatnonzero(qfin):
        d, j = np.inf, int(NO_INDEX)
        if len(R):
            e = qxyz[k].astype(np.float64) - R
            d2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]
            d, j = np.sqrt(d2.min()), int(orig[d2 == d2.min()].min())
        cl = not d <= float(max_dist)
        dist[k], index[k] = (np.float32(max_dist), NO_INDEX) if cl else (np.float32(d), j)
    return dist, index


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
def _face_cross(vrows, triangles):
    """The face cross product of the module docstring: (c float64 [m,3], c . c, loaded: the triangles ms_load accepts, (a, e1, e2, ti))."""
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
        cc = cx * cx + cy * cy + cz * cz
    return np.stack([cx, cy, cz], 1), cc, ok, (a, e1, e2, ti)


def face_cross_host(vrows, triangles):
    """(c float64 [m,3], c . c [m], ok bool [m]) per triangle; ok False: rejected (the values of such a row mean nothing)."""
    c, cc, ok, _ = _face_cross(vrows, triangles)
    with np.errstate(invalid="ignore"):
        ok = ok & (cc > 0) & (cc < np.inf)
    return c, cc, ok


def _triangle_counts(vrows, triangles, density, seed):
    _, cc, ok, (a, e1, e2, ti) = _face_cross(vrows, triangles)
    m = len(ti)
    with np.errstate(invalid="ignore", over="ignore"):
        A = 0.5 * np.sqrt(cc)
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


def sample_mesh_device(vrows, triangles, density, seed=0, max_samples=1 << 24, device="cuda:0", want_tri=False):
    """The device sampler: (rows tensor [n,4] int32 on the device, counters dict) -- one mm3dgs_mesh_sample_plan, one read-back of the
    counter block, the exact allocation, one mm3dgs_mesh_sample_emit.  Raises when the samples exceed `max_samples`.  With `want_tri`
    (rows, counters, tri int32 [n]: the triangle of every sample) through mm3dgs_mesh_sample_emit_tri."""
    from . import _lib
    from .rasterizer import _stream
    lib, P = _lib.load(), _lib.ptr
    vr = torch.as_tensor(vrows, device=device).to(torch.int32).reshape(-1, 4).contiguous()
    tr = torch.as_tensor(triangles, device=device).to(torch.int32).reshape(-1, 3).contiguous()
    m, nv = int(tr.shape[0]), int(vr.shape[0])
    if m == 0 or nv == 0:
        out = torch.empty(0, 4, dtype=torch.int32, device=device), dict(zip(SAMPLE_COUNTERS[:5], (0, m, 0, 0, m)))
        return out + (torch.empty(0, dtype=torch.int32, device=device),) if want_tri else out
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
    out = {"samples": total, "degenerate": int(c[1]), "written": total, "dropped": 0, "triangles": m}
    if want_tri:
        tri = torch.empty(max(total, 1), dtype=torch.int32, device=device)
        _lib.check(lib.mm3dgs_mesh_sample_emit_tri(nv, P(vr), m, P(tr), float(density), int(seed) & 0xffffffff, P(work), P(rows), P(tri), total, P(counters), _stream()))
        return rows[:total], out, tri[:total]
    _lib.check(lib.mm3dgs_mesh_sample_emit(nv, P(vr), m, P(tr), float(density), int(seed) & 0xffffffff, P(work), P(rows), total, P(counters), _stream()))
    return rows[:total], out


# ---- normals ------------------------------------------------------------------------------------------------------------------------
def normal_dots_host(tri_q, index, tri_r, mesh_q, mesh_r):
    """(dot float32 [n_q], no_neighbour bool [n_q]) of one direction by the rules of the module docstring: tri_q [n_q] the triangle of every
    query sample (of mesh_q = (vertex rows, triangles)), index [n_q] its nearest reference row (NO_INDEX: none), tri_r [n_r] the triangle
    of every reference row (of mesh_r).  NaN: not counted."""
    tq, j = as_np(tri_q, np.int64).reshape(-1) & 0xffffffff, as_np(index, np.int64).reshape(-1) & 0xffffffff
    tr_all = as_np(tri_r, np.int64).reshape(-1) & 0xffffffff
    cq, qq, okq = face_cross_host(*mesh_q)
    cr, rr, okr = face_cross_host(*mesh_r)
    none = j == int(NO_INDEX)
    good = ~none & (j < len(tr_all))
    tr = np.where(good, tr_all[np.where(good, j, 0)] if len(tr_all) else 0, 0)
    good &= (tq < len(okq)) & (tr < len(okr))
    tq, tr = np.where(good, tq, 0), np.where(good, tr, 0)
    if len(okq) and len(okr):
        good &= okq[tq] & okr[tr]
    else:
        good &= False
    dot = np.full(len(tq), np.nan, dtype=np.float32)
    if good.any():
        a, b = cq[tq[good]], cr[tr[good]]
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            d = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]) / (np.sqrt(qq[tq[good]]) * np.sqrt(rr[tr[good]]))
            d = np.where(d < -1.0, -1.0, np.where(d > 1.0, 1.0, d))
        dot[good] = d.astype(np.float32)
    return dot, none


def normal_row(dot, no_neighbour, sum_order="numpy"):
    """The eight figures of one direction's normals (NORMAL_ROW_NAMES) from the stored float32 dots (NaN = not counted) and the mask of the
    queries without a neighbour; the host twin of ``direction_row`` (`sum_order` as there)."""
    dot = np.asarray(dot, dtype=np.float32)
    counted = ~np.isnan(dot)
    d = dot[counted].astype(np.float64)
    n = len(d)
    row = np.zeros(8, dtype=np.float64)
    row[0] = n
    if n:
        row[1], row[2], row[3] = np.abs(d).sum() / n, d.sum() / n, np.abs(d).min()
        if sum_order == "kernel":
            z = np.where(counted, dot, np.float32(0)).astype(np.float64)
            row[1], row[2] = kernel_order_sum(np.abs(z)) / n, kernel_order_sum(z) / n
    none = np.asarray(no_neighbour, dtype=bool) & ~counted
    row[5] = float(none.sum())
    row[6] = float((~counted & ~none).sum())
    return row


def normal_figures(table):
    """The derived values of a [2,8] normal table (row 0: estimate -> reference, row 1: reference -> estimate)."""
    t = np.asarray(table, dtype=np.float64).reshape(2, 8)
    return {"normal_accuracy": float(t[0, 1]), "normal_completion": float(t[1, 1]), "normal_consistency": 0.5 * (float(t[0, 1]) + float(t[1, 1])),
            "normal_accuracy_signed": float(t[0, 2]), "normal_completion_signed": float(t[1, 2]),
            "normal_consistency_signed": 0.5 * (float(t[0, 2]) + float(t[1, 2]))}


def vertex_normals_host(vrows, triangles):
    """(normals float32 [n_vertices,3], counters dict) by the fixed-point rule of the module docstring."""
    nv = len(as_np(vrows, np.int32).reshape(-1, 4))
    c, _, ok = face_cross_host(vrows, triangles)
    tri = as_np(triangles, np.int32).reshape(-1, 3).astype(np.int64)[ok]
    c = c[ok]
    none = np.iinfo(np.int64).min
    E = np.full(nv, none, dtype=np.int64)
    S = np.zeros((nv, 3), dtype=np.int64)
    if len(tri):
        _, Et = np.frexp(np.abs(c).max(1))
        for k in range(3):
            np.maximum.at(E, tri[:, k], Et.astype(np.int64))
        for k in range(3):
            term = np.rint(np.ldexp(c, (FRAC_BITS - E[tri[:, k]])[:, None].astype(np.int64))).astype(np.int64)
            for a in range(3):
                np.add.at(S[:, a], tri[:, k], term[:, a])      # (int64 adds wrap as the device's do)
    s = S.astype(np.float64)
    ss = s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2]
    has = (E != none) & (ss > 0)
    normals = np.zeros((nv, 3), dtype=np.float32)
    normals[has] = (s[has] / np.sqrt(ss[has])[:, None]).astype(np.float32)
    return normals, {"vertices": nv, "without_normal": int((~has).sum()), "rejected_triangles": int((~ok).sum())}


def vertex_normals_device(vrows, triangles, device="cuda:0"):
    """The same on the device: (normals tensor float32 [n_vertices,3], counters tensor int64 [8]) from one mm3dgs_mesh_vertex_normals call,
    no read-back."""
    from . import _lib
    from .rasterizer import _stream
    lib, P = _lib.load(), _lib.ptr
    vr = torch.as_tensor(vrows, device=device).to(torch.int32).reshape(-1, 4).contiguous()
    tr = torch.as_tensor(triangles, device=device).to(torch.int32).reshape(-1, 3).contiguous()
    m, nv = int(tr.shape[0]), int(vr.shape[0])
    normals = torch.zeros(nv, 3, dtype=torch.float32, device=device)
    counters = torch.zeros(8, dtype=torch.int64, device=device)
    if m == 0 or nv == 0:
        counters[0], counters[1] = nv, nv
        return normals, counters
    nbytes = int(lib.mm3dgs_mesh_vertex_normals_work_bytes(nv))
    if nbytes == 0 or m > 1 << 30:
        raise ValueError(f"mesh of {nv} vertices and {m} triangles: at most 2^31 - 1 and 2^30")
    work = torch.empty(nbytes // 8, dtype=torch.int64, device=device)
    _lib.check(lib.mm3dgs_mesh_vertex_normals(nv, P(vr), m, P(tr), P(normals), P(work), P(counters), _stream()))
    return normals, counters


def vertex_normals(vrows, triangles, device="cpu"):
    """(normals float32 [n_vertices,3], counters dict): ``vertex_normals_device`` on a CUDA device (numpy after one read-back),
    ``vertex_normals_host`` otherwise."""
    if not str(device).startswith("cuda"):
        return vertex_normals_host(as_np(vrows, np.int32), as_np(triangles, np.int32))
    normals, counters = vertex_normals_device(vrows, triangles, device)
    c = counters.cpu().numpy()
    return normals.cpu().numpy(), dict(zip(NORMAL_COUNTERS, (int(v) for v in c[:3])))


def normal_consistency_device(tri_q, index, tri_r, mesh_q, mesh_r, dot=None, row=None, device="cuda:0"):
    """(dot [n_q] float32, row [8] float64) on the device: one mm3dgs_normal_consistency call, no read-back; the arguments of
    ``normal_dots_host`` as int32 / uint32-valued tensors and (vertex rows, triangles) tensors."""
    from . import _lib
    from .rasterizer import _stream
    lib, P = _lib.load(), _lib.ptr
    as32 = lambda t, w: torch.as_tensor(t, device=device).to(torch.int32).reshape(-1, w).contiguous()
    tq, ix, tr = as32(tri_q, 1), as32(index, 1), as32(tri_r, 1)
    vq, fq, vr, fr = as32(mesh_q[0], 4), as32(mesh_q[1], 3), as32(mesh_r[0], 4), as32(mesh_r[1], 3)
    nq = int(tq.shape[0])
    dot = torch.empty(nq, dtype=torch.float32, device=device) if dot is None else dot
    row = torch.zeros(8, dtype=torch.float64, device=device) if row is None else row
    if nq == 0:
        row.zero_()
        return dot, row
    if min(int(tr.shape[0]), int(vq.shape[0]), int(fq.shape[0]), int(vr.shape[0]), int(fr.shape[0])) == 0:      # nothing to look up: no kernel has anything to read
        dot.fill_(float("nan"))
        none = (ix.reshape(-1) == -1).sum().double()
        row.copy_(torch.stack([none * 0, none * 0, none * 0, none * 0, none * 0, none, nq - none, none * 0]))
        return dot, row
    work = torch.empty(int(lib.mm3dgs_normal_consistency_work_bytes(nq)) // 8, dtype=torch.int64, device=device)
    _lib.check(lib.mm3dgs_normal_consistency(nq, P(tq), P(ix), int(tr.shape[0]), P(tr), int(vq.shape[0]), P(vq), int(fq.shape[0]), P(fq), int(vr.shape[0]), P(vr),
                                             int(fr.shape[0]), P(fr), P(dot), P(row), P(work), _stream()))
    return dot, row


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

    def query(self, rows, dist=None, row=None, index=None):
        """(dist [n_q] float32, row [8] float64) on the device for the query rows [n_q,4] int32.  With `index` (int32 [n_q], holding the
        uint32 values) mm3dgs_nn_query_index also writes the nearest reference row of every query into it (-1 = 0xffffffff: none)."""
        from . import _lib
        from .rasterizer import _stream
        q = torch.as_tensor(rows, device=self.device).to(torch.int32).reshape(-1, 4).contiguous()
        nq = int(q.shape[0])
        dist = torch.empty(nq, dtype=torch.float32, device=self.device) if dist is None else dist
        row = torch.zeros(8, dtype=torch.float64, device=self.device) if row is None else row
        if nq == 0:
            row.zero_()
            return dist, row
        if index is not None and self.grid is None:
            index.fill_(-1)
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
        if index is not None:
            _lib.check(self.lib.mm3dgs_nn_query_index(nq, P(q), self.n_ref, self.cell, self._origin, gx, gy, gz, P(self.cell_start), P(self.sorted), self.max_dist,
                                                      self.threshold, P(dist), P(index), P(row), P(work), _stream()))
            return dist, row
        _lib.check(self.lib.mm3dgs_nn_query(nq, P(q), self.n_ref, self.cell, self._origin, gx, gy, gz, P(self.cell_start), P(self.sorted), self.max_dist,
                                            self.threshold, P(dist), P(row), P(work), _stream()))
        return dist, row

    def icp(self, rows, max_dist=0.1, iters=30, rel_fitness=1e-6, rel_rmse=1e-6, start=None, want_index=False):
        """Point-to-point ICP of the source rows [n,4] int32 onto this reference (``icp_host`` states the rule): one mm3dgs_icp_point call on
        the current stream -- a zeroing launch and 2 (iters + 1) launches, the stop decided on the device -- and no read-back.  Returns
        device tensors: state float64 [16] ([0:12] T, [12] passes run, [13] status), log float64 [iters + 1, 16], and with `want_index`
        dist float32 [n] / index int32 [n] (holding the uint32 values) of the last pass that ran.  `start`: a [3,4] T other than the
        identity.  A reference without finite rows, or no source row, gives status 2 without a launch."""
        from . import _lib
        from .rasterizer import _stream
        max_dist, iters, rel_fitness, rel_rmse = _check_icp(max_dist, iters, rel_fitness, rel_rmse)
        if float(np.ceil(max_dist / self.cell)) > MAX_RINGS:
            raise ValueError(f"icp_max_dist / cell = {max_dist / self.cell} (at most 2^20 rings)")
        q = torch.as_tensor(rows, device=self.device).to(torch.int32).reshape(-1, 4).contiguous()
        nq = int(q.shape[0])
        state = torch.zeros(16, dtype=torch.float64, device=self.device)
        state[:12] = torch.as_tensor(_IDENTITY if start is None else np.asarray(as_np(start, np.float64)).reshape(12), dtype=torch.float64, device=self.device)
        log = torch.zeros(iters + 1, 16, dtype=torch.float64, device=self.device)
        out = {"state": state, "log": log}
        if want_index:
            out.update(dist=torch.empty(nq, dtype=torch.float32, device=self.device), index=torch.empty(nq, dtype=torch.int32, device=self.device))
        if nq == 0 or self.grid is None:      # nothing to search: pass 0 finds no correspondence and stops (no kernel has anything to read)
            fin = torch.isfinite(q[:, :3].view(torch.float32)).all(1)
            state[12], state[13] = 1.0, 2.0
            log[0, 0], log[0, 2], log[0, 12] = 1.0, fin.sum().double(), 2.0
            log[0, 9:12] = state[3:12:4]
            if want_index:
                out["dist"].copy_(torch.where(fin, torch.full_like(out["dist"], max_dist), torch.full_like(out["dist"], float("nan"))))
                out["index"].fill_(-1)
            return out
        P = _lib.ptr
        gx, gy, gz = self.dims
        work = torch.empty(int(self.lib.mm3dgs_icp_work_bytes(nq)) // 8, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.mm3dgs_icp_point(nq, P(q), self.n_ref, self.cell, self._origin, gx, gy, gz, P(self.cell_start), P(self.sorted), max_dist, iters,
                                             rel_fitness, rel_rmse, P(state), P(log), P(out.get("dist")), P(out.get("index")), P(work), _stream()))
        return out


# ---- comparisons ----------------------------------------------------------------------------------------------------------------------
def _is_mesh(side):
    return isinstance(side, (tuple, list)) and len(side) == 2


def _need_meshes(estimate, reference):
    if not (_is_mesh(estimate) and _is_mesh(reference)):
        raise ValueError("normals need a mesh on both sides (a point cloud has no faces)")


def compare_host(estimate, reference, threshold=0.05, max_dist=1.0, cell=0, density=10000.0, seed=0, max_samples=1 << 24, cull=None, sum_order="numpy",
                 normals=False):
    """The comparison of the module docstring on the host (`sum_order`: ``direction_row``).  Each side is rows [n,4] int32 or (vertex rows, triangles).  Returns a dict:
    the derived figures, table [2,8], cells (the cell each grid used), counters, n_estimate, n_reference, and the arrays estimate_rows,
    reference_rows, dist_estimate, dist_reference.  `cull` (``cull.spec``: the run's views plus the options; None: off) removes from both
    point sets, after sampling and before the search, what no view could have seen: everything returned is then about the kept points,
    and the result gains `cull` (``cull.summary``) and estimate_index / reference_index (the original row of every kept row).  `normals`
    (both sides must be meshes, ValueError otherwise) adds the normal scores of the module docstring: `normals` (``normal_figures``),
    normal_table [2,8], dot_estimate, dot_reference and nearest_estimate / nearest_reference (the nearest row of the other set, uint32)."""
    cell = float(cell) if cell and float(cell) > 0 else float(threshold)
    if normals:
        _need_meshes(estimate, reference)
    sets, counters, tris = [], {}, []
    for name, side in (("estimate", estimate), ("reference", reference)):
        if _is_mesh(side):
            rows, c, *full = sample_mesh_host(side[0], side[1], density, seed, full=bool(normals))
            tris += [f["tri"] for f in full]
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
    d_er, n_er, i_er = _nn_search(sets[0], sets[1], cell, max_dist, None, bool(normals))
    d_re, n_re, i_re = _nn_search(sets[1], sets[0], cell, max_dist, None, bool(normals))
    table = np.stack([direction_row(d_er, i_er["clamped"], threshold, sum_order), direction_row(d_re, i_re["clamped"], threshold, sum_order)])
    counters.update(reference_skipped=i_er["ref_skipped"], estimate_skipped=i_re["ref_skipped"])
    out = _result(table, (i_er["cell"], i_re["cell"]), counters, sets, (d_er, d_re), threshold, max_dist, culled)
    if normals:
        te, tr = (t if culled is None else t[as_np(i, np.int64)] for t, i in zip(tris, (culled or (None, None, None))[1:]))
        dot_e, none_e = normal_dots_host(te, n_er, tr, estimate, reference)
        dot_r, none_r = normal_dots_host(tr, n_re, te, reference, estimate)
        _normal_result(out, np.stack([normal_row(dot_e, none_e, sum_order), normal_row(dot_r, none_r, sum_order)]), (dot_e, dot_r), (n_er, n_re))
    return out


def compare_device(estimate, reference, threshold=0.05, max_dist=1.0, cell=0, density=10000.0, seed=0, max_samples=1 << 24, device="cuda:0", cull=None,
                   normals=False):
    """The same comparison on the device: meshes sampled by the kernels, one GeometryScorer per direction, the [2,8] table read back once;
    the rows and distances stay device tensors.  `cull` as in ``compare_host``: one ``cull.Culler`` per side (one mm3dgs_cull_mark_view
    per view, one mm3dgs_cull_select and one read-back of its counters).  `normals` as in ``compare_host``: the samplers also give the
    triangle of every sample, the two queries the nearest row, one mm3dgs_normal_consistency per direction fills a second [2,8] table, and
    both tables are read back together; the dots and nearest rows stay device tensors (the rows as int32 holding the uint32 values)."""
    cell = float(cell) if cell and float(cell) > 0 else float(threshold)
    if normals:
        _need_meshes(estimate, reference)
    sets, counters, tris = [], {}, []
    for name, side in (("estimate", estimate), ("reference", reference)):
        if _is_mesh(side) and normals:
            rows, counters[name + "_sampler"], tri = sample_mesh_device(side[0], side[1], density, seed, max_samples, device, want_tri=True)
            tris.append(tri)
        elif _is_mesh(side):
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
    table = torch.zeros(4 if normals else 2, 8, dtype=torch.float64, device=device)
    n_er = torch.empty(sets[0].shape[0], dtype=torch.int32, device=device) if normals else None
    n_re = torch.empty(sets[1].shape[0], dtype=torch.int32, device=device) if normals else None
    d_er, _ = on_ref.query(sets[0], row=table[0], index=n_er)
    d_re, _ = on_est.query(sets[1], row=table[1], index=n_re)
    counters.update(reference_skipped=on_ref.ref_skipped, estimate_skipped=on_est.ref_skipped)
    if normals:
        te, tr = (t if culled is None else t[torch.as_tensor(i, device=device).long()] for t, i in zip(tris, (culled or (None, None, None))[1:]))
        dot_e, _ = normal_consistency_device(te, n_er, tr, estimate, reference, row=table[2], device=device)
        dot_r, _ = normal_consistency_device(tr, n_re, te, reference, estimate, row=table[3], device=device)
    both = table.cpu().numpy()      # the one read-back
    out = _result(both[:2], (on_ref.cell, on_est.cell), counters, sets, (d_er, d_re), threshold, max_dist, culled)
    if normals:
        _normal_result(out, both[2:], (dot_e, dot_r), (n_er, n_re))
    return out


def _result(table, cells, counters, sets, dists, threshold, max_dist, culled=None):
    out = derived_figures(table)
    if culled is not None:
        out.update(cull=culled[0], estimate_index=culled[1], reference_index=culled[2])
    out.update(table=np.asarray(table, dtype=np.float64), cells=[float(c) for c in cells], counters=counters, threshold=float(threshold),
               max_dist=float(max_dist), n_estimate=int(sets[0].shape[0]), n_reference=int(sets[1].shape[0]),
               estimate_rows=sets[0], reference_rows=sets[1], dist_estimate=dists[0], dist_reference=dists[1])
    return out


def _normal_result(out, table, dots, nearest):
    out.update(normals=normal_figures(table), normal_table=np.asarray(table, dtype=np.float64), dot_estimate=dots[0], dot_reference=dots[1],
               nearest_estimate=nearest[0], nearest_reference=nearest[1])


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


# ---- registration ---------------------------------------------------------------------------------------------------------------------
ICP_STATUS = ("converged", "iterations", "too_few_correspondences")
ICP_SWEEPS = 50        # the Jacobi solver's cap (see ``_horn_solve``)
ICP_MAX_ITERS = 1000
_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def move_rows_host(rows, T):
    """The rows with every finite position moved by T ([3,4] float64, (R | t)) by the component rule of the module docstring, rounded once
    to float32; the rgba, and a row that is not finite, as they are.  (The identity returns the input bytes except for a coordinate of -0.0,
    which the sum with 0 x y turns into 0.0.)"""
    rows = as_np(rows, np.int32).reshape(-1, 4)
    T = np.asarray(T, dtype=np.float64).reshape(3, 4)
    xyz, fin = _finite_rows(rows)
    p = xyz.astype(np.float64)
    out = rows.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        moved = np.stack([((T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2]) + T[a, 3] for a in range(3)], 1).astype(np.float32)
    out[fin, :3] = moved[fin].view(np.int32)
    return out


def _horn_solve(s):
    """(T [3,4] float64, quaternion [w, x, y, z], sweeps) from the 17 sums ``n, sum p [3], sum q [3], sum p_a q_b [9], -``: Horn's closed
    form with ``q ~ R p + t``.  Python floats (IEEE doubles) and ``+ - x / sqrt`` only, written operation by operation as ``icp_horn`` in
    csrc/geometry.hip is, so the device agrees bit for bit.  Cyclic Jacobi rotations in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a
    sweep starts only while an off-diagonal element is not exactly zero, and from the fifth sweep on an element below the rounding of
    both its diagonal neighbours is set to zero, so the sum reaches zero: a 4 x 4 matrix gets there in well under ten sweeps
    (tests/test_icp.py counts them), and ICP_SWEEPS = 50 is the classical cap that only bounds the loop."""
    from math import sqrt
    s = [float(v) for v in s]
    n = s[0]
    S = [[s[7 + 3 * a + b] - (s[1 + a] * s[4 + b]) / n for b in range(3)] for a in range(3)]
    A = [[0.0] * 4 for _ in range(4)]
    A[0][0] = (S[0][0] + S[1][1]) + S[2][2]
    A[0][1] = S[1][2] - S[2][1]
    A[0][2] = S[2][0] - S[0][2]
    A[0][3] = S[0][1] - S[1][0]
    A[1][1] = (S[0][0] - S[1][1]) - S[2][2]
    A[1][2] = S[0][1] + S[1][0]
    A[1][3] = S[2][0] + S[0][2]
    A[2][2] = (S[1][1] - S[0][0]) - S[2][2]
    A[2][3] = S[1][2] + S[2][1]
    A[3][3] = (S[2][2] - S[0][0]) - S[1][1]
    for a in range(4):
        for b in range(a):
            A[a][b] = A[b][a]
    V = [[1.0 if a == b else 0.0 for b in range(4)] for a in range(4)]
    sweeps = 0
    for sweep in range(ICP_SWEEPS):
        off = ((((abs(A[0][1]) + abs(A[0][2])) + abs(A[0][3])) + abs(A[1][2])) + abs(A[1][3])) + abs(A[2][3])
        if off == 0.0:
            break
        sweeps += 1
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                g = 100.0 * abs(apq)
                if sweep > 3 and abs(A[p][p]) + g == abs(A[p][p]) and abs(A[q][q]) + g == abs(A[q][q]):
                    A[p][q] = A[q][p] = 0.0
                    continue
                h = A[q][q] - A[p][p]
                if abs(h) + g == abs(h):
                    t = apq / h
                else:
                    theta = (0.5 * h) / apq
                    t = 1.0 / (abs(theta) + sqrt(1.0 + theta * theta))
                    if theta < 0.0:
                        t = -t
                c = 1.0 / sqrt(t * t + 1.0)
                sn = t * c
                A[p][p] = A[p][p] - t * apq
                A[q][q] = A[q][q] + t * apq
                A[p][q] = A[q][p] = 0.0
                for r in range(4):
                    if r != p and r != q:
                        arp, arq = A[r][p], A[r][q]
                        A[r][p] = A[p][r] = c * arp - sn * arq
                        A[r][q] = A[q][r] = sn * arp + c * arq
                    vrp, vrq = V[r][p], V[r][q]
                    V[r][p] = c * vrp - sn * vrq
                    V[r][q] = sn * vrp + c * vrq
    top, w, x, y, z = A[0][0], V[0][0], V[1][0], V[2][0], V[3][0]      # the largest eigenvalue, the first one on a tie
    for k in range(1, 4):
        if A[k][k] > top:
            top, w, x, y, z = A[k][k], V[0][k], V[1][k], V[2][k], V[3][k]
    if w < 0.0:
        w, x, y, z = -w, -x, -y, -z
    ln = sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / ln, x / ln, y / ln, z / ln
    ww, xx, yy, zz, xy, xz, yz, wx, wy, wz = w * w, x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    R = [[((ww + xx) - yy) - zz, 2.0 * (xy - wz), 2.0 * (xz + wy)],
         [2.0 * (xy + wz), ((ww - xx) + yy) - zz, 2.0 * (yz - wx)],
         [2.0 * (xz - wy), 2.0 * (yz + wx), ((ww - xx) - yy) + zz]]
    mp = [s[1] / n, s[2] / n, s[3] / n]
    T = np.zeros((3, 4), dtype=np.float64)
    for a in range(3):
        T[a, :3] = R[a]
        T[a, 3] = s[4 + a] / n - ((R[a][0] * mp[0] + R[a][1] * mp[1]) + R[a][2] * mp[2])
    return T, [w, x, y, z], sweeps


def _check_icp(max_dist, iters, rel_fitness, rel_rmse):
    max_dist, rel_fitness, rel_rmse = float(max_dist), float(rel_fitness), float(rel_rmse)
    if not (np.isfinite(max_dist) and max_dist > 0):
        raise ValueError(f"icp_max_dist = {max_dist} (must be finite and positive)")
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 1 <= int(iters) <= ICP_MAX_ITERS:
        raise ValueError(f"icp_iters = {iters!r} (an integer, 1 .. {ICP_MAX_ITERS})")
    if not rel_fitness >= 0:
        raise ValueError(f"icp_rel_fitness = {rel_fitness} (must not be negative)")
    if not rel_rmse >= 0:
        raise ValueError(f"icp_rel_rmse = {rel_rmse} (must not be negative)")
    return max_dist, int(iters), rel_fitness, rel_rmse


def icp_pairs_host(source_rows, reference_rows, cell, max_dist, T, grid=None):
    """One pass's move and search: (dist, index, has bool [n], p float64 [n,3]: the original coordinates, q [n,3]: the correspondence, d2
    [n]: the double squared distance; p, q, d2 are 0 where `has` is False)."""
    src = as_np(source_rows, np.int32).reshape(-1, 4)
    ref = as_np(reference_rows, np.int32).reshape(-1, 4)
    moved = move_rows_host(src, T)
    dist, index, _ = _nn_search(moved, ref, cell, max_dist, grid, True)
    has = index != NO_INDEX
    j = np.where(has, index, 0).astype(np.int64)
    Rf = rows_xyz(ref).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.where(has[:, None], Rf[j] if len(Rf) else 0.0, 0.0)
        p = np.where(has[:, None], rows_xyz(src).astype(np.float64), 0.0)
        d = rows_xyz(moved).astype(np.float64) - (Rf[j] if len(Rf) else 0.0)
        d2 = np.where(has, d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2], 0.0)
    return dist, index, has, p, q, d2


def icp_sums(has, p, q, d2, sum_order="numpy"):
    """The 17 sums of a pass as Python floats, each column added by numpy or in ``kernel_order_sum``'s order."""
    add = kernel_order_sum if sum_order == "kernel" else (lambda v: float(np.sum(v)))
    cols = [has.astype(np.float64)] + [p[:, a] for a in range(3)] + [q[:, a] for a in range(3)] + [p[:, a] * q[:, b] for a in range(3) for b in range(3)] + [d2]
    return [add(c) for c in cols]


def icp_host(source_rows, reference_rows, cell, max_dist=0.1, iters=30, rel_fitness=1e-6, rel_rmse=1e-6, sum_order="numpy", start=None):
    """Point-to-point ICP of the source rows onto the reference rows by the rule of the module docstring, in float64 numpy: the statement
    mm3dgs_icp_point is held to (bit for bit with `sum_order` "kernel") and the path of ``device: cpu``.  Returns a dict: T [3,4] float64,
    status (0 converged, 1 `iters` reached, 2 fewer than 3 correspondences), passes, log [iters + 1, 16] float64 -- per pass [0] 1 when it
    ran, [1] n, [2] finite source rows, [3] fitness, [4] rmse, [5:9] the quaternion of the latest solve (0 before the first), [9:12] t behind
    the pass, [12] the status on the row of the pass that stopped, the rest 0 --, the index / dist of the last pass (what ``nn_index_host``
    gives for the source moved by the returned T), fitness, rmse and sweeps (the Jacobi sweeps of every solve).  `start`: a [3,4] T other
    than the identity."""
    max_dist, iters, rel_fitness, rel_rmse = _check_icp(max_dist, iters, rel_fitness, rel_rmse)
    src = as_np(source_rows, np.int32).reshape(-1, 4)
    ref = as_np(reference_rows, np.int32).reshape(-1, 4)
    rxyz, rfin = _finite_rows(ref)
    grid = grid_for(rxyz[rfin].astype(np.float64).min(0), rxyz[rfin].astype(np.float64).max(0), cell) if rfin.any() else None
    finite = float(_finite_rows(src)[1].sum())
    T = np.asarray(_IDENTITY if start is None else start, dtype=np.float64).reshape(3, 4).copy()
    quat, log, sweeps = [0.0] * 4, np.zeros((iters + 1, 16), dtype=np.float64), []
    before = None
    for k in range(iters + 1):
        dist, index, has, p, q, d2 = icp_pairs_host(src, ref, cell, max_dist, T, grid)
        s = icp_sums(has, p, q, d2, sum_order)
        n = s[0]
        fitness = n / finite if n > 0 else 0.0
        rmse = float(np.sqrt(s[16] / n)) if n > 0 else 0.0
        status = -1
        if before is not None and abs(fitness - before[0]) < rel_fitness and abs(rmse - before[1]) < rel_rmse:
            status = 0
        elif n < 3:
            status = 2
        elif k == iters:
            status = 1
        if status < 0:
            T, quat, sw = _horn_solve(s)
            sweeps.append(sw)
        before = (fitness, rmse)
        log[k, :5] = (1.0, n, finite, fitness, rmse)
        log[k, 5:9], log[k, 9:12], log[k, 12] = quat, T[:, 3], max(status, 0)
        if status >= 0:
            break
    return {"T": T, "status": status, "passes": k + 1, "log": log, "index": index, "dist": dist, "fitness": fitness, "rmse": rmse, "sweeps": sweeps}


def icp_state(result):
    """The 16 doubles mm3dgs_icp_point leaves in `state` for a result of ``icp_host``."""
    return np.concatenate([np.asarray(result["T"], dtype=np.float64).reshape(12), [float(result["passes"]), float(result["status"]), 0.0, 0.0]])


def icp_record(state, log, n_source, n_reference):
    """The record of a registration from `state` [16] and `log`: T, status, passes, fitness and rmse of the returned T, those of the start,
    and the sizes of the two point sets."""
    state, log = np.asarray(state, dtype=np.float64).reshape(16), np.asarray(log, dtype=np.float64).reshape(-1, 16)
    passes = int(state[12])
    last = log[max(passes - 1, 0)]
    return {"T": state[:12].reshape(3, 4).copy(), "status": int(state[13]), "passes": passes, "fitness": float(last[3]), "rmse": float(last[4]),
            "fitness_start": float(log[0, 3]), "rmse_start": float(log[0, 4]), "n_source": int(n_source), "n_reference": int(n_reference)}


def move_rows(rows, T, device="cpu"):
    """The rows moved by T: one mm3dgs_rows_move call on a CUDA device (rows and T -- 12 doubles -- may be device tensors; a device tensor
    comes back, nothing is read back), ``move_rows_host`` otherwise."""
    if not str(device).startswith("cuda"):
        return move_rows_host(as_np(rows, np.int32), as_np(T, np.float64))
    from . import _lib
    from .rasterizer import _stream
    r = torch.as_tensor(rows, device=device).to(torch.int32).reshape(-1, 4).contiguous()
    t = torch.as_tensor(T, device=device).to(torch.float64).reshape(-1)[:12].contiguous()
    out = torch.empty_like(r)
    if int(r.shape[0]):
        _lib.check(_lib.load().mm3dgs_rows_move(int(r.shape[0]), _lib.ptr(r), _lib.ptr(t), _lib.ptr(out), _stream()))
    return out


def _point_set(side, device, density, seed, max_samples):
    """The point set of one side as ``compare_host`` / ``compare_device`` take it: a mesh sampled, a cloud as it is."""
    on_device = str(device).startswith("cuda")
    if _is_mesh(side):
        if on_device:
            return sample_mesh_device(side[0], side[1], density, seed, max_samples, device)[0]
        rows, c = sample_mesh_host(side[0], side[1], density, seed)
        if c["samples"] > int(max_samples):
            raise ValueError(f"{c['samples']} surface samples at density {density} per m^2: more than max_samples = {int(max_samples)}")
        return rows
    return torch.as_tensor(side, device=device).to(torch.int32).reshape(-1, 4).contiguous() if on_device else as_np(side, np.int32).reshape(-1, 4)


def register(estimate, reference, device="cpu", threshold=0.05, cell=0, density=10000.0, seed=0, max_samples=1 << 24, max_dist=0.1, iters=30,
             rel_fitness=1e-6, rel_rmse=1e-6, sum_order="numpy"):
    """The estimate registered to the reference by point-to-point ICP (the rule of the module docstring): (the moved estimate, the
    record).  Each side is rows [n,4] int32 or (vertex rows, triangles); a mesh side is sampled exactly as ``compare`` samples it (the
    same `density`, `seed`, `max_samples`), a cloud side is taken as it is, and the reference grid has the scoring cell (`cell`, 0:
    `threshold`).  Of a mesh estimate the vertex rows are moved and the triangles are left; a later ``compare`` samples the moved mesh
    again -- the second sampling is accepted: the samples of a moved mesh are not the moved samples in the last bit, and the scores are
    about the mesh that is written.  On a CUDA device: one grid build, one mm3dgs_icp_point, one mm3dgs_rows_move and one read-back of
    state + log; the moved rows stay on the device.  The record: T [3,4] (reference ~ R estimate + t), status (``ICP_STATUS``), passes,
    fitness / rmse of the returned T and fitness_start / rmse_start of the start, n_source, n_reference, log.  With status 2 (fewer than 3
    correspondences) the estimate is returned as it was."""
    cell = float(cell) if cell and float(cell) > 0 else float(threshold)
    src, ref = _point_set(estimate, device, density, seed, max_samples), _point_set(reference, device, density, seed, max_samples)
    rows = estimate[0] if _is_mesh(estimate) else estimate
    if str(device).startswith("cuda"):
        out = GeometryScorer(ref, cell, max_dist, threshold, device).icp(src, max_dist, iters, rel_fitness, rel_rmse)
        both = torch.cat([out["state"], out["log"].reshape(-1)]).cpu().numpy()      # the one read-back
        state, log = both[:16], both[16:].reshape(-1, 16)
        moved = move_rows(rows, out["state"], device) if int(state[13]) != 2 else rows
    else:
        result = icp_host(src, ref, cell, max_dist, iters, rel_fitness, rel_rmse, sum_order)
        state, log = icp_state(result), result["log"]
        moved = move_rows_host(rows, result["T"]) if result["status"] != 2 else rows
    record = dict(icp_record(state, log, src.shape[0], ref.shape[0]), log=log)
    return ((moved, estimate[1]) if _is_mesh(estimate) else moved), record


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
    if result.get("normals") is not None:
        nt = result["normal_table"]
        out["normals"] = dict(result["normals"], estimate_to_reference={name: float(nt[0, k]) for k, name in enumerate(NORMAL_ROW_NAMES[:7]) if k != 4},
                              reference_to_estimate={name: float(nt[1, k]) for k, name in enumerate(NORMAL_ROW_NAMES[:7]) if k != 4})
    out.update(extra or {})
    return out


def write_outputs(path, result, extra=None):
    """path/metrics.json, path/accuracy.ply (the estimate's points coloured by distance over [0, 2 threshold]) and path/completion.ply (the
    reference's points likewise); with normal scores also path/normals.npz (dot_estimate, dot_reference float32 and nearest_estimate,
    nearest_reference uint32: per point of either set the dot product and the nearest row of the other set, 0xffffffff: none).  Returns the
    paths."""
    from .pointcloud import write_ply
    os.makedirs(path, exist_ok=True)
    files = {"metrics": os.path.join(path, "metrics.json")}
    with open(files["metrics"], "w") as fh:
        json.dump(metrics_dict(result, extra), fh, indent=1, sort_keys=True)
        fh.write("\n")
    files["accuracy"] = write_ply(os.path.join(path, "accuracy.ply"), colour_by_distance(result["estimate_rows"], result["dist_estimate"], result["threshold"]))
    files["completion"] = write_ply(os.path.join(path, "completion.ply"), colour_by_distance(result["reference_rows"], result["dist_reference"], result["threshold"]))
    if result.get("normals") is not None:
        files["normals"] = os.path.join(path, "normals.npz")
        np.savez(files["normals"], dot_estimate=as_np(result["dot_estimate"], np.float32), dot_reference=as_np(result["dot_reference"], np.float32),
                 nearest_estimate=as_np(result["nearest_estimate"], np.int64).astype(np.uint32), nearest_reference=as_np(result["nearest_reference"], np.int64).astype(np.uint32))
    return files
