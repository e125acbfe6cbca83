"""Inputs shared by tests/test_mesh_clean.py (CPU) and tests/test_gpu_mesh_clean.py: tiny indexed meshes built in numpy -- the empty sizes,
the smallest meshes, odd triangles (degenerate, duplicated, invalid indices, unreferenced vertices), the edges of the two modes, sizes
around one workgroup, one mesh beyond 262 144 triangles (the second round of the 1024-wide scan), a long ribbon in three index orders and
two triangle orders, and the marching-tetrahedra output of a sphere with two small blobs.  A case is dict(name, rows [V,4] int32,
triangles [T,3] int32, modes: [(mode, min_triangles) ...]); row bytes are arbitrary (NaN patterns included: they are moved, never read)."""
import numpy as np

from mm3dgs_slam_amd import mesh as ms
from tests import mesh_cases

DEFAULT_MODES = (("small", 1), ("small", 2), ("largest", 1))
RIBBON = 1 << 14
BIG_T = 262144 + 257


def rows_for(V, seed=0):
    r = np.random.RandomState(1000 + seed).randint(-2 ** 31, 2 ** 31, size=(V, 4), dtype=np.int64).astype(np.int32)
    if V:
        r[::7, 1] = np.int32(0x7fc00000)      # a NaN
        r[::5, 0] = np.array([0xff800000], dtype=np.uint32).view(np.int32)[0]      # -inf
    return r


def case(name, V, triangles, modes=DEFAULT_MODES, seed=0):
    return {"name": name, "rows": rows_for(V, seed), "triangles": np.asarray(triangles, dtype=np.int64).reshape(-1, 3).astype(np.int32), "modes": tuple(modes)}


def strip(first, n_triangles):
    """n triangles over the vertices first .. first + n + 1: one component."""
    i = first + np.arange(n_triangles)
    return np.stack([i, i + 1, i + 2], 1)


def strips(sizes, gaps=None):
    """Disjoint strips of the given triangle counts, one behind the other, `gaps[k]` unreferenced vertices in front of strip k: (V, triangles)."""
    at, out = 0, []
    for k, n in enumerate(sizes):
        at += 0 if gaps is None else gaps[k]
        out.append(strip(at, n))
        at += n + 2
    return at, np.concatenate(out) if out else np.zeros((0, 3), dtype=np.int64)


def strips_to(total_vertices=None, total_triangles=None):
    """Strips of 1, 2, ..., 7, 1, 2, ... triangles until exactly the given number of vertices (the rest, below 3, unreferenced) or triangles."""
    sizes, k, v, t = [], 0, 0, 0
    while True:
        n = k % 7 + 1
        if total_triangles is not None:
            n = min(n, total_triangles - t)
            if n == 0:
                break
        elif v + n + 2 > total_vertices:
            break
        sizes.append(n); v += n + 2; t += n; k += 1
    V, tris = strips(sizes)
    return (total_vertices if total_vertices is not None else V), tris


def ribbon(order, shuffle_triangles):
    """A strip over 2^14 vertices -- one component, a chain as long as the mesh -- with the vertices renamed in ascending, descending or
    shuffled order and the triangles in file order or shuffled (fixed seeds)."""
    name = {"ascending": np.arange(RIBBON), "descending": np.arange(RIBBON)[::-1], "shuffled": np.random.RandomState(7).permutation(RIBBON)}[order]
    tris = name[strip(0, RIBBON - 2)]
    if shuffle_triangles:
        tris = tris[np.random.RandomState(11).permutation(len(tris))]
    return case(f"ribbon {order}{' shuffled triangles' if shuffle_triangles else ''}", RIBBON, tris, (("small", RIBBON - 2), ("small", RIBBON - 1), ("largest", 1)))


def blob_volume():
    """mesh_cases' sphere in a 17^3 lattice with two small blobs planted beyond the truncation band: one inside sample and two adjacent ones."""
    vol = mesh_cases.analytic_volume("sphere", (17, 17, 17))
    t = vol["tsdf_w"]
    assert t[1, 1, 1, 0] == 1.0 and t[2, 14, 14, 0] == 1.0 and t[2, 14, 13, 0] == 1.0
    t[1, 1, 1, 0] = -0.5
    t[2, 14, 14, 0] = -0.25
    t[2, 14, 13, 0] = -0.75
    return vol


def marching_tetrahedra():
    vol = blob_volume()
    rows, tris, _ = ms.mesh_host(vol["tsdf_w"], vol["rgb_w"], vol["origin"], vol["voxel"])
    return {"name": "marching tetrahedra: sphere and two blobs", "rows": rows, "triangles": tris, "modes": (("small", 1), ("small", 25), ("small", 49), ("largest", 1))}      # the blobs have 24 and 48 triangles


def small_cases():
    """Every case but the big one and the ribbons."""
    M = 3
    unref_v, unref_t = strips([2, 1, 3], gaps=[2, 3, 0])      # two in front, three in the middle; the case adds two at the end
    out = [
        case("V = 0", 0, []),
        case("V = 0 with triangles", 0, [[0, 1, 2], [-1, 0, 0]]),
        case("T = 0, V = 5", 5, []),
        case("one triangle", 3, [[0, 1, 2]]),
        case("two triangles sharing an edge", 4, [[0, 1, 2], [2, 1, 3]]),
        case("two triangles sharing one vertex", 5, [[0, 1, 2], [2, 3, 4]]),
        case("two disjoint triangles", 6, [[3, 4, 5], [0, 1, 2]]),
        case("degenerate triangles", 6, [[0, 0, 1], [2, 2, 2], [1, 3, 3], [4, 5, 4]]),
        case("a duplicated triangle", 7, [[0, 1, 2], [0, 1, 2], [3, 4, 5], [2, 1, 0]], (("small", 1), ("small", 2), ("small", 3), ("small", 4), ("largest", 1))),
        case("invalid triangles mixed in", 7, [[0, 1, 2], [-1, 1, 2], [2, 3, 7], [4, 5, 6], [0, 2 ** 31 - 1, 4], [6, 5, 4], [7, 7, 7], [3, -2 ** 31, 3]]),
        case("unreferenced vertices at the front, middle and end", unref_v + 2, unref_t, (("small", 1), ("small", 2), ("small", 3), ("largest", 1))),
        case("components of min - 1, min and min + 1 triangles", *strips([M + 1, M - 1, M, M - 1, M + 1, M]), modes=(("small", M), ("small", M + 1), ("small", M + 2), ("largest", 1))),
        # the tie for the largest: the component with the lower label comes later in the triangle list
        case("a tie for the largest", 12, np.concatenate([strip(6, 4), strip(0, 4)]), (("largest", 1), ("small", 4), ("small", 5))),
        case("a tie of three, the lowest label in the middle of the list", 15, np.concatenate([strip(10, 3), strip(0, 3), strip(5, 3)]), (("largest", 1),)),
        case("cleaning removes nothing", 10, np.concatenate([strip(1, 6), [[8, 1, 3]]]), (("small", 1), ("small", 7), ("largest", 1))),
    ]
    for n in (255, 256, 257):
        out.append(case(f"V = {n}", *strips_to(total_vertices=n), modes=(("small", 4), ("largest", 1)), seed=n))
        out.append(case(f"T = {n}", *strips_to(total_triangles=n), modes=(("small", 4), ("largest", 1)), seed=n))
    out.append(marching_tetrahedra())
    return out


def ribbon_cases():
    return [ribbon(order, shuffled) for order in ("ascending", "descending", "shuffled") for shuffled in (False, True)]


def big_case():
    """More than 262 144 triangles, every triangle its own component (V = 3 T), the vertices of a triangle far apart."""
    T = BIG_T
    t = np.arange(T)
    return case("every triangle its own component", 3 * T, np.stack([t, t + T, t + 2 * T], 1), (("small", 1), ("small", 2), ("largest", 1)))


def all_cases():
    return small_cases() + ribbon_cases() + [big_case()]
