"""The connected components of an indexed triangle mesh, and the mesh without its small disconnected pieces -- the "floaters" that a fused
volume leaves beside the surface (a few stray Gaussians in a rendered view, depth speckle in a sensor frame) and that the published
protocols drop before a mesh is shown or scored (NICE-SLAM's ``clean_mesh``, Co-SLAM's ``cull_mesh.py``, Open3D's
``cluster_connected_triangles`` + ``remove_triangles_by_mask``).  On a GPU the labelling is one ``mm3dgs_mesh_components`` call and the
removal one ``mm3dgs_mesh_clean_plan`` / ``mm3dgs_mesh_clean_emit`` pair (``csrc/meshclean.hip``, ``clean_device``); ``components_host`` /
``clean_host`` are the numpy statement of the same rule: the yardstick of the kernels, byte for byte, and the path of ``device: cpu``.

The rule is in integers only.  The input is ``rows [V,4] int32`` (16 bytes per vertex, moved and never read as numbers) and ``triangles
[T,3] int32``, as ``TsdfVolume.extract`` / ``mesh.mesh_host`` return them.

* A triangle is **valid** when its three indices lie in ``[0, V)``.  An invalid triangle joins nothing and is counted nowhere but in
  ``skipped``; cleaning drops it.  A degenerate triangle (a repeated index) is valid and counts as one triangle.
* Two vertices are **connected** when a valid triangle uses both; components are the transitive closure.  This is connectivity through
  shared *vertices*.  Open3D and trimesh connect triangles through shared *edges*; the two differ only where pieces of the surface touch
  in a single vertex (the pinch points of the marching-tetrahedra surface), which this rule counts as one piece.
* ``label[v]`` is the smallest vertex index of v's component; a vertex that no valid triangle uses has ``label[v] = v``.
* ``tri_count[r]`` is the number of valid triangles whose vertices carry label r, 0 at every index that is not a label.
* Mode ``small`` keeps the components with ``tri_count >= min_triangles`` (at least 1); mode ``largest`` the one component with the
  greatest ``tri_count``, on a tie the one with the smallest label.  Without a valid triangle nothing is kept.
* Kept vertices are the vertices of kept components -- which all have a triangle, so a vertex that nothing references is dropped too --
  in their original order, row bytes untouched; kept triangles follow in their original order, re-indexed; ``index[k]`` is the original
  vertex of kept vertex k.

**Counters** (int64 [8]): [0] components with a triangle, [1] the largest as ``(tri_count << 32) | (~label & 0xffffffff)`` (0: none), [2]
skipped triangles, [3] vertices no valid triangle uses, [4] components kept, [5] vertices kept, [6] triangles kept, [7] ``(kept triangles
not written << 32) | kept vertices not written`` when a cap is below a total.

``python -m mm3dgs_slam_amd.mesh_clean in.ply out.ply [--mode small|largest] [--min-triangles N] [--device cpu|cuda:0]`` cleans any mesh
file that ``mesh.read_surface_ply`` loads."""
from __future__ import annotations

import numpy as np
import torch

from .pointcloud import as_np

MODES = ("none", "small", "largest")
MODE_IDS = {"small": 1, "largest": 2}      # MM3DGS_MESH_CLEAN_SMALL / _LARGEST
INFO_NAMES = ("components", "components_kept", "largest_triangles", "vertices_removed", "triangles_removed", "skipped")
MAX_ROWS = 1 << 30


def check_options(mode, min_triangles):
    """(mode, min_triangles) validated as the entry points validate them; ``none`` is not a mode of a cleaning call."""
    mode = str(mode).lower()
    if mode not in MODE_IDS:
        raise ValueError(f"mesh clean mode = {mode!r} (small / largest)")
    if isinstance(min_triangles, bool) or int(min_triangles) != min_triangles or int(min_triangles) < 1 or int(min_triangles) >= 1 << 32:
        raise ValueError(f"mesh clean min_triangles = {min_triangles!r} (an integer, at least 1)")
    return mode, int(min_triangles)


def _sizes(V, T):
    if not (0 <= V <= MAX_ROWS and 0 <= T <= MAX_ROWS):
        raise ValueError(f"mesh of {V} vertices and {T} triangles (each at most 2^30)")


def valid_triangles(V, triangles):
    """bool [T]: the triangles whose three indices lie in [0, V)."""
    tri = as_np(triangles, np.int32).reshape(-1, 3)
    return ((tri >= 0) & (tri < int(V))).all(1)


def components_host(V, triangles):
    """(label uint32 [V], tri_count uint32 [V], counters int64 [8], of which [4:] are 0) by the rule of the module docstring.  Labels go
    down until nothing changes: every edge hands the smaller of its two labels to both ends and to both ends' labels, then every label
    is replaced by its label's label until that is stable.  A label is always a vertex of the same component at or below its vertex, so
    the fixed point -- equal along every edge, each its own label -- is the component's minimum."""
    V = int(V)
    tri = as_np(triangles, np.int32).reshape(-1, 3)
    _sizes(V, len(tri))
    ok = valid_triangles(V, tri)
    good = tri[ok].astype(np.int64)
    a = np.concatenate([good[:, 0], good[:, 1]])
    b = np.concatenate([good[:, 1], good[:, 2]])
    label = np.arange(V, dtype=np.int64)
    while len(a):
        before = label
        label = label.copy()
        la, lb = before[a], before[b]
        m = np.minimum(la, lb)
        for at in (a, b, la, lb):
            np.minimum.at(label, at, m)
        while True:
            up = label[label]
            if np.array_equal(up, label):
                break
            label = up
        if np.array_equal(label, before):
            break
    tri_count = np.bincount(label[good[:, 0]], minlength=V).astype(np.int64) if V else np.zeros(0, dtype=np.int64)
    counters = np.zeros(8, dtype=np.int64)
    counters[0] = int((tri_count > 0).sum())
    if len(good):
        r = int(np.argmax(tri_count))      # the first of the greatest counts: the smallest label
        counters[1] = (int(tri_count[r]) << 32) | (~r & 0xffffffff)
    counters[2] = len(tri) - len(good)
    counters[3] = int(((tri_count == 0) & (label == np.arange(V))).sum())
    return label.astype(np.uint32), tri_count.astype(np.uint32), counters


def largest_of(counters):
    """(tri_count, label) of the largest component from counters[1]; (0, None) without a valid triangle."""
    k = int(counters[1])
    return (k >> 32, ~k & 0xffffffff) if k else (0, None)


def kept_components(label, tri_count, counters, mode, min_triangles):
    """bool [V]: is the component whose label is r kept (False at every index that is not the label of a component with a triangle)."""
    mode, min_triangles = check_options(mode, min_triangles)
    tri_count = np.asarray(tri_count).astype(np.int64)
    if mode == "small":
        return tri_count >= min_triangles
    keep = np.zeros(len(tri_count), dtype=bool)
    n, r = largest_of(counters)
    if n:
        keep[r] = True
    return keep


def info_of(V, T, counters):
    """The ``info`` dict of a cleaning from its sizes and counters."""
    c = [int(v) for v in counters]
    return {"components": c[0], "components_kept": c[4], "largest_triangles": c[1] >> 32, "vertices_removed": int(V) - c[5],
            "triangles_removed": int(T) - c[6], "skipped": c[2]}


def clean_host(rows, triangles, mode="small", min_triangles=100, vcap=None, tcap=None, full=False):
    """(rows' [V',4] int32, triangles' [T',3] int32, index uint32 [V'], info) by the rule of the module docstring; `vcap` / `tcap`: at most
    so many kept rows / triangles are returned, the rest counted in counters[7].  With ``full`` also (counters int64 [8], label, tri_count)."""
    mode, min_triangles = check_options(mode, min_triangles)
    rows = as_np(rows, np.int32).reshape(-1, 4)
    tri = as_np(triangles, np.int32).reshape(-1, 3)
    V, T = len(rows), len(tri)
    label, tri_count, counters = components_host(V, tri)
    keep = kept_components(label, tri_count, counters, mode, min_triangles)
    vkeep = keep[label.astype(np.int64)] if V else np.zeros(0, dtype=bool)
    ok = valid_triangles(V, tri)
    tkeep = ok.copy()
    tkeep[ok] = vkeep[tri[ok, 0].astype(np.int64)]
    index = np.flatnonzero(vkeep)
    remap = np.full(V, -1, dtype=np.int64)
    remap[index] = np.arange(len(index))
    out_tri = remap[tri[tkeep].astype(np.int64)].astype(np.int32).reshape(-1, 3)
    counters[4] = int((keep & (label == np.arange(V))).sum())
    counters[5], counters[6] = len(index), len(out_tri)
    nv = len(index) if vcap is None else min(len(index), int(vcap))
    nt = len(out_tri) if tcap is None else min(len(out_tri), int(tcap))
    counters[7] = ((len(out_tri) - nt) << 32) | (len(index) - nv)
    out = (rows[index[:nv]].copy(), out_tri[:nt].copy(), index[:nv].astype(np.uint32), info_of(V, T, counters))
    return out + (counters, label, tri_count) if full else out


def clean_device(rows, triangles, mode="small", min_triangles=100, device="cuda:0"):
    """``clean_host`` on the device: mm3dgs_mesh_components, mm3dgs_mesh_clean_plan, one read-back of the counters, exact allocations and
    mm3dgs_mesh_clean_emit.  Returns device tensors (index: int32 storage of uint32) and the info dict."""
    from . import _lib
    from .rasterizer import _stream
    if not str(device).startswith("cuda"):
        raise ValueError("clean_device needs a CUDA device (the host path is clean_host)")
    mode, min_triangles = check_options(mode, min_triangles)
    rows = torch.as_tensor(rows, device=device).to(torch.int32).reshape(-1, 4).contiguous()
    tri = torch.as_tensor(triangles, device=device).to(torch.int32).reshape(-1, 3).contiguous()
    V, T = int(rows.shape[0]), int(tri.shape[0])
    _sizes(V, T)
    lib, P = _lib.load(), _lib.ptr
    label = torch.empty(max(V, 1), dtype=torch.int32, device=device)
    tri_count = torch.empty(max(V, 1), dtype=torch.int32, device=device)
    counters = torch.empty(8, dtype=torch.int64, device=device)
    work = torch.empty(int(lib.mm3dgs_mesh_clean_work_bytes(V, T)) // 8, dtype=torch.int64, device=device)
    _lib.check(lib.mm3dgs_mesh_components(V, T, P(tri), P(label), P(tri_count), P(counters), _stream()))
    _lib.check(lib.mm3dgs_mesh_clean_plan(V, T, P(tri), P(label), P(tri_count), MODE_IDS[mode], min_triangles, P(work), P(counters), _stream()))
    c = counters.cpu().numpy().copy()      # the one read-back before the allocations
    nv, nt = int(c[5]), int(c[6])
    out_rows = torch.empty(max(nv, 1), 4, dtype=torch.int32, device=device)
    out_tri = torch.empty(max(nt, 1), 3, dtype=torch.int32, device=device)
    index = torch.empty(max(nv, 1), dtype=torch.int32, device=device)
    _lib.check(lib.mm3dgs_mesh_clean_emit(V, T, P(rows), P(tri), P(work), P(out_rows), nv, P(out_tri), nt, P(index), P(counters), _stream()))
    return out_rows[:nv], out_tri[:nt], index[:nv], info_of(V, T, c)      # the allocations are exact: nothing is dropped


def clean(rows, triangles, mode="small", min_triangles=100, device="cpu"):
    """``clean_device`` on a CUDA device, ``clean_host`` otherwise."""
    if str(device).startswith("cuda"):
        return clean_device(rows, triangles, mode, min_triangles, device=device)
    return clean_host(rows, triangles, mode, min_triangles)


def summary(mode, min_triangles, info):
    """One line for the print-outs."""
    return (f"cleaned ({mode}" + (f", at least {min_triangles} triangles" if mode == "small" else "") + f"): kept {info['components_kept']} of "
            f"{info['components']} components, removed {info['vertices_removed']} vertices and {info['triangles_removed']} triangles")


def main(argv=None):
    import argparse
    from .config import MESH_CLEAN
    from .mesh import read_surface_ply, write_mesh_ply
    ap = argparse.ArgumentParser(prog="python -m mm3dgs_slam_amd.mesh_clean", description="Remove the small disconnected pieces of a triangle mesh (binary PLY).")
    ap.add_argument("input", help="a mesh PLY file: one written by this package, or a dataset's (mesh.read_surface_ply)")
    ap.add_argument("output", help="the cleaned mesh (mesh.write_mesh_ply)")
    ap.add_argument("--mode", choices=("small", "largest"), default="small", help="small: drop the components below --min-triangles; largest: keep one component")
    ap.add_argument("--min-triangles", type=int, default=MESH_CLEAN["clean_min_triangles"], help="mode small: the fewest triangles of a kept component")
    ap.add_argument("--device", default="cpu", help="cpu (the host statement) or a CUDA device such as cuda:0 (the HIP kernels)")
    args = ap.parse_args(argv)
    surface = read_surface_ply(args.input)
    if not isinstance(surface, tuple):
        raise SystemExit(f"{args.input}: a point cloud (no face element); nothing to clean")
    rows, tris, _, info = clean(surface[0], surface[1], args.mode, args.min_triangles, device=args.device)
    write_mesh_ply(args.output, rows, tris)
    print(f"Mesh {summary(args.mode, args.min_triangles, info)}; {len(rows)} vertices, {len(tris)} triangles in {args.output}")
    return info


if __name__ == "__main__":
    main()
