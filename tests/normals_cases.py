"""Inputs shared by tests/test_normals.py (CPU) and tests/test_gpu_normals.py: point sets for the nearest-row search (duplicates, an
eight-fold tie, queries outside the grid and beyond max_dist, rows that are not finite on both sides) and small meshes for the sampler's
triangle ids, the normal consistency and the vertex normals.  Everything is numpy on the host; the GPU tests move it over once."""
import numpy as np

from tests import geometry_cases as gc

N_Q = (1, 255, 256, 257, 1000)      # one row; exactly one workgroup and its neighbours; four workgroups, the last partial
N_REF = (1, 3, 500)
CELL, MAX_DIST, THRESHOLD = gc.CELL, gc.MAX_DIST, gc.THRESHOLD
CUBE = 3.0 + 0.5 * np.array([[i, j, k] for k in (0, 1) for j in (0, 1) for i in (0, 1)], dtype=np.float64)      # the 2 x 2 x 2 lattice cube
CENTRE = np.array([3.25, 3.25, 3.25])       # 0.1875 = 3 / 16 from each corner in squared distance, exactly


def index_case(n_ref, n_q):
    """dict(ref, query, cell, max_dist, threshold).  500 references: rows 10..17 the cube, rows 40..43 copies of rows 30..33, rows 100 / 101
    not finite; 3 references: rows 0 and 2 equal; query 0 is the cube's centre (500) or the doubled point (3); with 255 queries or more,
    query 1 sits on a doubled reference, 2 and 4 are not finite, 3 is far outside the grid."""
    rng = np.random.default_rng(77 * n_ref + n_q)
    ref = gc.dyadic(rng, n_ref, -1, 1)
    q = gc.dyadic(rng, n_q, -1.75, 1.75)
    if n_ref == 500:
        ref[10:18] = CUBE
        ref[40:44] = ref[30:34]
        ref[100], ref[101] = [gc.NAN, 0, 0], [0, gc.INF, 0]
        q[0] = CENTRE
    elif n_ref == 3:
        ref[2] = ref[0]
        q[0] = ref[0]
    if n_q >= 255:
        q[1] = ref[30] if n_ref == 500 else ref[0]
        q[2], q[3], q[4] = [gc.NAN, gc.NAN, gc.NAN], [40.0, 40.0, 40.0], [0, -gc.INF, 0.5]
    return dict(name=f"index {n_ref} x {n_q}", ref=gc.rows_of(ref), query=gc.rows_of(q), cell=CELL, max_dist=MAX_DIST, threshold=THRESHOLD)


def tie_counts(case):
    """Per query the number of finite reference rows at the smallest float64 squared distance (0 for a query that is not finite)."""
    from mm3dgs_slam_amd import pointcloud as pc
    R, Q = pc.rows_xyz(case["ref"]).astype(np.float64), pc.rows_xyz(case["query"]).astype(np.float64)
    R = R[np.isfinite(R).all(1)]
    out = np.zeros(len(Q), dtype=np.int64)
    for k in np.flatnonzero(np.isfinite(Q).all(1)):
        e = Q[k] - R
        d2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]
        out[k] = int((d2 == d2.min()).sum())
    return out


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
def octahedron():
    v = gc.rows_of([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], rgba=np.arange(6) + 1)
    tris = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int32)      # outward
    return v, tris


def icosphere(levels=2, radius=0.5, centre=(0.0, 0.0, 0.0)):
    """20 x 4^levels outward triangles on a sphere (levels 2: 320 triangles, 162 vertices)."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [np.array(p, dtype=np.float64) for p in ((-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
                                                 (-g, 0, -1), (-g, 0, 1))]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8),
         (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                mid[key] = len(v)
                v.append(0.5 * (v[a] + v[b]))
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    p = np.stack(v)
    p = radius * p / np.sqrt((p * p).sum(1))[:, None] + np.asarray(centre, dtype=np.float64)
    return gc.rows_of(p, rgba=np.arange(len(p)) + 7), np.asarray(f, dtype=np.int32)


def shifted(mesh, by):
    v, tris = mesh
    from mm3dgs_slam_amd import pointcloud as pc
    return gc.rows_of(pc.rows_xyz(v).astype(np.float64) + np.asarray(by, dtype=np.float64), rgba=v[:, 3].view(np.uint32)), tris


def flipped(mesh):
    return mesh[0], np.ascontiguousarray(mesh[1][:, [0, 2, 1]])


def floor_and_wall():
    """The unit floor z = 0 and the unit wall x = 0 that share the edge x = z = 0, two triangles each (normals +z and +x)."""
    floor = gc.rows_of([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    wall = gc.rows_of([[0, 0, 0], [0, 1, 0], [0, 1, 1], [0, 0, 1]]), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    return floor, wall


def grid_mesh(n=17, seed=3):
    """An n x n height field (289 vertices, 512 triangles at n = 17; interior valence 6)."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    p = np.stack([i * 0.0625, j * 0.0625, 0.03 * rng.standard_normal((n, n))], -1).reshape(-1, 3)
    idx = (i * n + j)[:-1, :-1].reshape(-1)
    tris = np.concatenate([np.stack([idx, idx + n, idx + n + 1], 1), np.stack([idx, idx + n + 1, idx + 1], 1)]).astype(np.int32)
    return gc.rows_of(p, rgba=np.arange(n * n) + 1), tris


def fan_mesh(m=1000, seed=4):
    """m triangles around vertex 0 (a cone's apex): every triangle adds to the same three sums."""
    rng = np.random.default_rng(seed)
    a = 2.0 * np.pi * np.arange(m) / m
    rim = np.stack([np.cos(a), np.sin(a), 0.05 * rng.standard_normal(m)], 1)
    p = np.concatenate([[[0.0, 0.0, 0.7]], rim])
    k = np.arange(m)
    return gc.rows_of(p), np.stack([np.zeros(m, dtype=np.int64), 1 + k, 1 + (k + 1) % m], 1).astype(np.int32)


def rejecting_mesh():
    """``geometry_cases.degenerate_mesh`` (triangles 0 and 7 are sound, every other kind is rejected) with two more vertices -- 7, which
    makes triangle 1 collinear, and 8, which no triangle names -- and triangle 8 with an index beyond the vertices.  Vertices 3, 4, 5 and 7
    are named by rejected triangles only."""
    v, tris, _ = gc.degenerate_mesh()
    v = np.concatenate([v, gc.rows_of([[3, 0, 0], [5, 5, 5]])])
    return v, np.concatenate([tris, np.array([[0, 1, 9]], dtype=np.int32)])


def sparse_sample_mesh(m=300):
    """m triangles: every seventh is rejected (an index of -1), and runs of 1e-4 m slivers that get no sample lie between the others."""
    v, tris = gc.tiny_mesh(m, s=0.02)
    v, tris = v.copy(), tris.copy()
    t = np.arange(m)
    small = (t // 10) % 3 == 1
    for k in np.flatnonzero(small):
        v[3 * k + 1, 0] = np.float32(np.float64(v[3 * k:3 * k + 1, 0].view(np.float32)[0]) + 1e-4).view(np.int32)
        v[3 * k + 2, 1] = np.float32(np.float64(v[3 * k:3 * k + 1, 1].view(np.float32)[0]) + 1e-4).view(np.int32)
    tris[::7, 0] = -1
    return v, tris


def single_triangle():
    return gc.rows_of([[0, 0, 0], [0.3, 0, 0], [0, 0.4, 0.1]], rgba=[1, 2, 3]), np.array([[0, 1, 2]], dtype=np.int32)
