"""Inputs shared by tests/test_geometry.py (CPU) and tests/test_gpu_geometry.py: point sets for the nearest-neighbour search (dyadic
coordinates wherever an equality decides a count) and small meshes for the sampler.  Everything is numpy on the host; the GPU tests move it
over once.  A nearest-neighbour case is a dict(ref, query: rows [n,4] int32; cell, max_dist, threshold); `checked` asserts on the CPU that
no float64 distance lies within relative 1e-6 of `threshold` or `max_dist` unless it equals it exactly (a deliberate dyadic tie, computed
without rounding), so that no rounding can flip a count and nothing has to be excluded from a comparison."""
import numpy as np

from mm3dgs_slam_amd import geometry as geo

SIZES = (1, 255, 256, 257, 1000)      # one row; exactly one workgroup and its neighbours; four workgroups, the last partial
CELL, MAX_DIST, THRESHOLD = 0.25, 0.5, 0.125
NAN, INF = float("nan"), float("inf")


def rows_of(xyz, rgba=None):
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    rows = np.empty((len(xyz), 4), dtype=np.int32)
    with np.errstate(over="ignore"):
        rows[:, :3] = xyz.astype(np.float32).view(np.int32)
    rows[:, 3] = np.int32(-1) if rgba is None else np.asarray(rgba, dtype=np.uint32).view(np.int32)
    return rows


def dyadic(rng, n, lo, hi, bits=10):
    """n points with coordinates that are multiples of 2^-bits in [lo, hi)."""
    s = float(1 << bits)
    return rng.integers(int(lo * s), int(hi * s), size=(n, 3)).astype(np.float64) / s


def checked(case):
    d = geo.nn_brute_host(case["query"], case["ref"], case["max_dist"])[2]
    d = d[np.isfinite(d)]
    for bar in (case["threshold"], case["max_dist"]):
        near = (d != bar) & (np.abs(d - bar) <= 1e-6 * bar)
        assert not near.any(), (case.get("name"), bar, d[near])
    return case


def sized_case(n_ref, n_q):
    rng = np.random.default_rng(1000 * n_ref + n_q)
    return checked(dict(name=f"sized {n_ref} x {n_q}", ref=rows_of(dyadic(rng, n_ref, -1, 1)), query=rows_of(dyadic(rng, n_q, -1.25, 1.25)), cell=CELL,
                        max_dist=MAX_DIST, threshold=THRESHOLD))


def single_cell_case():
    rng = np.random.default_rng(7)
    return checked(dict(name="300 references in one cell", ref=rows_of(dyadic(rng, 300, 0, 0.25)), query=rows_of(dyadic(rng, 257, -0.5, 0.75)), cell=CELL,
                        max_dist=MAX_DIST, threshold=THRESHOLD))


def lattice_case():
    rng = np.random.default_rng(8)
    i, j, k = np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij")
    ref = (np.stack([i, j, k], -1).reshape(-1, 3) + 0.5) * CELL
    return checked(dict(name="one reference per cell of 5 x 4 x 3", ref=rows_of(ref), query=rows_of(dyadic(rng, 300, -0.5, 1.75)), cell=CELL, max_dist=MAX_DIST,
                        threshold=THRESHOLD))


def big_grid_case():
    """64 x 64 x 65 cells = 266 240 > 1024 x 256: the cell scan's second 1024-wide round; 500 points, the two box corners among them."""
    rng = np.random.default_rng(9)
    ref = np.concatenate([[[0.0, 0.0, 0.0], [15.875, 15.875, 16.125]], dyadic(rng, 498, 0, 15.875)])
    q = np.concatenate([ref[::5] + np.array([0.0625, 0.0, -0.03125]), dyadic(rng, 200, -1, 17)])
    case = checked(dict(name="64 x 64 x 65 cells", ref=rows_of(ref), query=rows_of(q), cell=CELL, max_dist=MAX_DIST, threshold=THRESHOLD))
    xyz = ref
    assert geo.grid_for(xyz.min(0), xyz.max(0), CELL)[2] == [64, 64, 65]
    return case


def termination_case():
    """cell 1: the query's ring-1 corner cell (1,1,1) holds a point at 1.705 cells, the ring-2 axis cell (2,0,0) one at 1.1875: a search that
    stopped after ring 1 (best <= 2 cell, say) would return the farther one."""
    q = np.array([[0.875, 0.5, 0.5]])
    ref = np.array([[0.875 + 0.984375, 0.5 + 0.984375, 0.5 + 0.984375], [2.0625, 0.5, 0.5], [0.0, 0.0, -3.0]])
    case = checked(dict(name="termination bound", ref=rows_of(ref), query=rows_of(q), cell=1.0, max_dist=4.0, threshold=1.25))
    cells = np.floor(ref[:2]).astype(int) - np.floor(q).astype(int)
    assert cells.tolist() == [[1, 1, 1], [2, 0, 0]]
    assert geo.nn_brute_host(case["query"], case["ref"], 4.0)[2].tolist() == [1.1875]
    return case


def edge_case():
    """Isolated clusters 4 m apart along y (cell 0.25, max_dist 0.5, threshold 0.125): each block is (reference points, query points)."""
    e20, e22 = 2.0 ** -20, 2.0 ** -22
    blocks = [
        ([[-0.0625, 0, 0]], [[0.0625, 0, 0], [-0.1875, 0, 0]]),                                   # negative coordinates: floor, not truncation (cells -1 | 0)
        ([[-0.3125, -0.3125, -0.3125], [-0.75, -0.5, -0.25]], [[-0.25, -0.25, -0.25], [-0.5, -0.5, -0.5]]),   # queries on cell faces, corners and a reference's cell border
        ([[0.375, 0.125, 0.625]], [[0.375, 0.125, 0.625], [0.375, 0.125, 0.625]]),                # queries exactly on a reference point: d = 0
        ([[0.5, 0, 0]], [[0, 0, 0]]),                                                             # exactly max_dist: not clamped
        ([[0.5 + e20, 0, 0]], [[0, 0, 0]]),                                                       # max_dist + 2^-20: clamped
        ([[0.125, 0, 0]], [[0, 0, 0]]),                                                           # exactly the threshold: within
        ([[0.125 + e22, 0, 0]], [[0, 0, 0]]),                                                     # threshold + 2^-22: not within
        ([[0, 0, 0], [NAN, 0, 0], [0, INF, 0], [0, 0, -INF]], [[0.0625, 0, 0], [NAN, NAN, NAN], [INF, 0, 0], [0, -INF, 0.5]]),   # rows that are not finite, both sides
    ]
    ref, q = [], []
    for b, (r, qq) in enumerate(blocks):
        off = np.array([0.0, 4.0 * b, 0.0])
        ref.append(np.asarray(r, dtype=np.float64) + off)
        q.append(np.asarray(qq, dtype=np.float64) + off)
    ref, q = np.concatenate(ref), np.concatenate(q)
    # past each of the six faces of the reference's box, within and beyond max_dist of the nearest reference
    fin = ref[np.isfinite(ref).all(1)]
    lo, hi = fin.min(0), fin.max(0)
    out = []
    for a in range(3):
        for side, base in ((-1.0, lo), (1.0, hi)):
            anchor = fin[np.argmin(fin[:, a]) if side < 0 else np.argmax(fin[:, a])]
            for step in (0.375, 0.75, 40.0):
                p = anchor.copy()
                p[a] = base[a] + side * step
                out.append(p)
    q = np.concatenate([q, np.asarray(out)])
    return checked(dict(name="edges", ref=rows_of(ref), query=rows_of(q), cell=CELL, max_dist=MAX_DIST, threshold=THRESHOLD))


def nn_cases():
    return {c["name"]: c for c in (single_cell_case(), lattice_case(), big_grid_case(), termination_case(), edge_case())}


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
def random_mesh(m, seed=0):
    rng = np.random.default_rng(seed)
    nv = max(3, m + 2)
    v = rows_of(rng.uniform(-1, 1, (nv, 3)), rgba=rng.integers(0, 1 << 32, nv, dtype=np.uint64).astype(np.uint32))
    tris = np.stack([rng.permutation(nv)[:3] for _ in range(m)]).astype(np.int32)
    return v, tris


def tiny_mesh(m=262400, s=0.01):
    """m right triangles of legs s (area s^2 / 2) on a grid, three vertices each: m / 256 = 1025 workgroups, the scan's second round."""
    t = np.arange(m)
    base = np.stack([(t % 512) * 0.03125, (t // 512) * 0.03125, np.zeros(m)], 1)
    v = np.stack([base, base + [s, 0, 0], base + [0, s, 0]], 1).reshape(-1, 3)
    rgba = (np.arange(3 * m, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    return rows_of(v, rgba), np.arange(3 * m, dtype=np.int32).reshape(m, 3)


def wall_mesh(where, m=600):
    """One 4 m^2 triangle as the first / last of m triangles; the others are 1e-4 m slivers (area 5e-9)."""
    v, tris = tiny_mesh(m, s=1e-4)
    v = v.copy()
    t = 0 if where == "first" else m - 1
    v[3 * t:3 * t + 3, :3] = rows_of([[1.0, 2.0, 3.0], [5.0, 2.0, 3.0], [1.0, 4.0, 3.0]])[:, :3]
    return v, tris


def degenerate_mesh():
    """Triangles 0 and 7 are sound; the others are degenerate, one of each kind (an area that is not finite cannot arise from finite float32
    corners in double: the largest cross product is about 1e78)."""
    v = rows_of([[0, 0, 0], [1, 0, 0], [0, 1, 0], [NAN, 0, 0], [0, INF, 0], [2, 0, 0], [0, 0, 1]], rgba=np.arange(7) + 100)
    tris = np.array([[0, 1, 2], [0, 1, 7], [-1, 1, 2], [0, 3, 2], [4, 1, 2], [0, 0, 2], [0, 1, 5], [0, 2, 6]], dtype=np.int32)
    kinds = ("sound", "index >= n_vertices", "index < 0", "NaN corner", "inf corner", "repeated vertex", "collinear", "sound")
    return v, tris, kinds


def square_mesh(z=0.0, x1=1.0):
    """The rectangle [0, x1] x [0, 1] at height z as two triangles."""
    v = rows_of([[0, 0, z], [x1, 0, z], [x1, 1, z], [0, 1, z]], rgba=[0xff0000ff, 0xff00ff00, 0xffff0000, 0xffffffff])
    return v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
