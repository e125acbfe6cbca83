"""The reconstruction as a coloured triangle mesh: the RGB-D image of every exported view -- the map rendered at the estimated pose, or the
frame itself -- is fused into a dense truncated signed distance volume (running means of the truncated distance and of the colour, one
weight each), and the zero level of the volume is extracted by marching tetrahedra into an indexed mesh, written as a binary PLY file that
MeshLab or any PLY reader opens.  The reference stops at the point cloud (``scripts/visualizer.py``; Open3D did the rest for its authors).

The volume is two arrays over an ``nx x ny x nz`` lattice of sample points, x fastest: ``tsdf_w [nz,ny,nx,2]`` float32 (truncated distance
in [-1, 1], observation weight) and ``rgb_w [nz,ny,nx,4]`` float32 (mean colour, colour weight); sample (i, j, k) sits at ``origin + voxel
(i, j, k)``; all zeros is the empty volume.  On a GPU one view is one ``mm3dgs_tsdf_integrate`` call and the mesh one ``mm3dgs_tsdf_mesh_plan``
+ ``mm3dgs_tsdf_mesh_emit`` pair (``csrc/tsdf.hip``, ``TsdfVolume``); ``integrate_host`` / ``mesh_host`` are the float64 statement of the same
rules, rounded to float32 exactly where the device stores do: the yardstick of the kernels and the path of ``device: cpu``
(``HostTsdfVolume``).

Marching tetrahedra: every lattice cube is cut into the six Kuhn tetrahedra -- the monotone paths from corner (0,0,0) to (1,1,1), one per
axis permutation, the same cut in every cube, so face diagonals agree between neighbours and the surface closes.  A sample is *known* if
its weight is at least ``min_weight`` and *inside* if its distance is negative; a cube is *valid* if its 8 corners are known.  A surface
vertex lies on a lattice edge that leaves a sample q in one of the 7 directions d in {0,1}^3 \\ {0} (d as a 3-bit number, x the low bit);
the edge carries a vertex iff its endpoints differ in *inside* and at least one valid cube contains it.  Vertices are ordered by q in raster
order, then by d; triangles by cube in raster order, then by tetrahedron, then by case order; the normal points from inside to outside.

With ``mesh.volume: sparse`` the volume is held in blocks of 8 x 8 x 8 samples, only where a view's truncation band reaches (``reserve_host``,
``HostSparseTsdfVolume``, ``SparseTsdfVolume`` over ``csrc/tsdf_sparse.hip``): the statement stands above those classes."""
from __future__ import annotations

import numpy as np
import torch

from .pointcloud import CLOUD_PROPERTIES, as_np, cam_args, device_view, pose_rotation, quantise_colour, read_header, read_ply, valid_mask

INTEGRATE_COUNTERS = ("views", "dist_updates", "colour_updates")
MESH_COUNTERS = ("vertices", "triangles", "vertices_written", "triangles_written", "vertices_dropped", "triangles_dropped")
MAX_SAMPLES = 1 << 30

# ---- the decomposition --------------------------------------------------------------------------------------------------------
TET_PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))      # tetrahedron order: the axis permutations, lexicographic
TET_CORNERS = tuple((0, 1 << a, (1 << a) | (1 << b), 7) for a, b, _ in TET_PERMS)    # cube corners (bit 0 x, bit 1 y, bit 2 z) along the path
TET_ODD = tuple(p in ((0, 2, 1), (1, 0, 2), (2, 1, 0)) for p in TET_PERMS)            # an odd permutation mirrors the tetrahedron
TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))                         # local vertex pairs, lower path position first
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def _case_table():
    """[16] lists of triangles (three tetrahedron-edge ids each) of a positively oriented tetrahedron, by its 4-bit inside mask (bit v:
    local vertex v is inside).  One inside (or one outside) vertex: the triangle of its three edges, the other ends ascending; two: the
    quadrilateral (a,c) (a,d) (b,d) (b,c) of the inside pair a < b and the outside pair c < d as the triangles (0,1,2) and (0,2,3) of that
    cycle.  The winding is then fixed so that the normal points from the inside vertices to the outside ones (checked on the unit Kuhn
    tetrahedron with every crossing at its edge's midpoint: the case decides the winding, the crossing positions do not)."""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]], dtype=np.float64)
    eid = {e: k for k, e in enumerate(TET_EDGES)}
    e = lambda a, b: eid[(min(a, b), max(a, b))]
    mid = lambda k: 0.5 * (v[TET_EDGES[k][0]] + v[TET_EDGES[k][1]])
    table = []
    for m in range(16):
        ins = [i for i in range(4) if (m >> i) & 1]
        out = [i for i in range(4) if not (m >> i) & 1]
        if len(ins) in (0, 4):
            tris = []
        elif len(ins) == 1:
            tris = [[e(ins[0], o) for o in out]]
        elif len(ins) == 3:
            tris = [[e(out[0], i) for i in ins]]
        else:
            (a, b), (c, d) = ins, out
            tris = [[e(a, c), e(a, d), e(b, d)], [e(a, c), e(b, d), e(b, c)]]
        fixed = []
        for t in tris:
            p = [mid(k) for k in t]
            if np.cross(p[1] - p[0], p[2] - p[0]) @ (v[out].mean(0) - v[ins].mean(0)) < 0:
                t = [t[0], t[2], t[1]]
            fixed.append(tuple(t))
        table.append(tuple(fixed))
    return tuple(table)


CASE_TRIANGLES = _case_table()
CASE_COUNT = np.array([len(c) for c in CASE_TRIANGLES], dtype=np.int64)
_CASE_ARRAY = np.zeros((16, 2, 3), dtype=np.int64)
for _m, _c in enumerate(CASE_TRIANGLES):
    for _s, _t in enumerate(_c):
        _CASE_ARRAY[_m, _s] = _t


def empty_volume(nx, ny, nz):
    """(tsdf_w [nz,ny,nx,2], rgb_w [nz,ny,nx,4]) float32 zeros: the empty volume."""
    return np.zeros((nz, ny, nx, 2), dtype=np.float32), np.zeros((nz, ny, nx, 4), dtype=np.float32)


def check_lattice(nx, ny, nz):
    if min(nx, ny, nz) < 2 or int(nx) * int(ny) * int(nz) > MAX_SAMPLES:
        raise ValueError(f"lattice {nx} x {ny} x {nz}: every size must be at least 2 and the product at most 2^30")


def view_bounds(depth, sil, pose, cam, sil_min, depth_max):
    """(lo [3], hi [3]) float64 on the input's device: the box of one view's lifted valid pixels -- the rules of ``pointcloud.valid_mask``,
    ``pose_rotation`` and ``backproject_host`` with torch operators, nothing read back.  No valid pixel: (+inf, -inf)."""
    d = depth.detach().float()
    ok = (d > 0) & torch.isfinite(d)
    if depth_max > 0:
        ok &= d <= depth_max
    if sil is not None:
        ok &= sil.detach().float() > sil_min
    H, W = d.shape
    v, u = torch.meshgrid(torch.arange(H, device=d.device, dtype=torch.float64), torch.arange(W, device=d.device, dtype=torch.float64), indexing="ij")
    z = d.double()
    p = pose.detach().double().reshape(7)
    q = p[:4] / p[:4].norm()
    w, x, y, zz = q[0], q[1], q[2], q[3]
    R = torch.stack([torch.stack([1 - 2 * (y * y + zz * zz), 2 * (x * y - w * zz), 2 * (x * zz + w * y)]),
                     torch.stack([2 * (x * y + w * zz), 1 - 2 * (x * x + zz * zz), 2 * (y * zz - w * x)]),
                     torch.stack([2 * (x * zz - w * y), 2 * (y * zz + w * x), 1 - 2 * (x * x + y * y)])])
    pc = torch.stack([(u - float(cam["cx"])) / float(cam["fx"]) * z, (v - float(cam["cy"])) / float(cam["fy"]) * z, z], -1).reshape(-1, 3)
    pw = (pc - p[4:]) @ R                      # rows: R^T (p_c - t)
    m = ok.reshape(-1, 1)
    inf = torch.tensor(float("inf"), device=d.device, dtype=torch.float64)
    return torch.where(m, pw, inf).amin(0), torch.where(m, pw, -inf).amax(0)


def lattice_for(box, voxel, max_voxels):
    """(origin float64 [3], dims [3]) of the lattice over the box [xmin, ymin, zmin, xmax, ymax, zmax]: the origin snapped down to a
    multiple of voxel, per axis ceil(extent / voxel) + 1 samples and at least 2; more than `max_voxels` (at most 2^30) is an error."""
    origin = np.floor(box[:3] / voxel) * voxel
    dims = [max(int(np.ceil((box[3 + a] - origin[a]) / voxel)) + 1, 2) for a in range(3)]
    if dims[0] * dims[1] * dims[2] > min(int(max_voxels), MAX_SAMPLES):
        raise ValueError(f"mesh export: the box {box[:3].tolist()} .. {box[3:].tolist()} at mesh.voxel = {voxel} m is a lattice of "
                         f"{dims[0]} x {dims[1]} x {dims[2]} samples, more than mesh.max_voxels = {int(max_voxels)} (at most 2^30); raise "
                         f"mesh.voxel or mesh.max_voxels, or set mesh.bounds")
    return origin, dims


# ---- integration ----------------------------------------------------------------------------------------------------------------
def integrate_host(tsdf_w, rgb_w, color, depth, sil, pose, fx, fy, cx, cy, origin, voxel, trunc, sil_min=0.0, depth_max=0.0, full=False, first=(0, 0, 0)):
    """One view into the volume, in place, in float64 from the float32 inputs.  Per sample: p_c = R p_w + t, skipped if z <= 0; pixel u =
    floor(fx x / z + cx + 0.5), v likewise (pixel centres at integer coordinates), skipped outside the image or where the pixel fails the
    point cloud's validity test; sdf = depth - z, skipped if sdf < -trunc; s = min(1, sdf / trunc); T <- (T W + s) / (W + 1), W <- W + 1,
    rounded to float32 once; the colour mean and its weight likewise, only if sdf <= trunc.  Returns (distance updates, colour updates);
    with ``full`` also dict(upd, col: the masks [nz,ny,nx]; fu, fv: the pixel coordinates before the floor; sdf; z).  ``first``: the
    (signed) lattice index of the array's sample [0,0,0]: sample [k,j,i] sits at origin + voxel (first + (i, j, k))."""
    col = as_np(color, np.float32)
    d = as_np(depth, np.float32)
    H, W = d.shape
    nz, ny, nx = tsdf_w.shape[:3]
    ok = valid_mask(d, sil, sil_min, depth_max)
    R, t = pose_rotation(pose)
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    voxel, trunc = float(voxel), float(trunc)
    f = [int(a) for a in first]
    pw = [o[0] + voxel * (f[0] + np.arange(nx, dtype=np.int64)).astype(np.float64)[None, None, :],
          o[1] + voxel * (f[1] + np.arange(ny, dtype=np.int64)).astype(np.float64)[None, :, None],
          o[2] + voxel * (f[2] + np.arange(nz, dtype=np.int64)).astype(np.float64)[:, None, None]]
    x, y, z = (R[a, 0] * pw[0] + R[a, 1] * pw[1] + R[a, 2] * pw[2] + t[a] for a in range(3))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        fu = float(fx) * x / z + float(cx) + 0.5
        fv = float(fy) * y / z + float(cy) + 0.5
        u, v = np.floor(fu), np.floor(fv)
        seen = (z > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    ui, vi = np.where(seen, u, 0).astype(np.int64), np.where(seen, v, 0).astype(np.int64)
    seen &= ok[vi, ui]
    dz = d[vi, ui].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        sdf = np.where(seen, dz, 0.0) - z
        upd = seen & ~(sdf < -trunc)
        cupd = upd & (sdf <= trunc)
        s = np.minimum(1.0, sdf / trunc)
    T, Wt = tsdf_w[..., 0].astype(np.float64), tsdf_w[..., 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        tsdf_w[..., 0] = np.where(upd, (T * Wt + s) / (Wt + 1.0), T).astype(np.float32)
        tsdf_w[..., 1] = np.where(upd, Wt + 1.0, Wt).astype(np.float32)
        Cw = rgb_w[..., 3].astype(np.float64)
        for c in range(3):
            C = rgb_w[..., c].astype(np.float64)
            rgb_w[..., c] = np.where(cupd, (C * Cw + col[c][vi, ui].astype(np.float64)) / (Cw + 1.0), C).astype(np.float32)
        rgb_w[..., 3] = np.where(cupd, Cw + 1.0, Cw).astype(np.float32)
    n = (int(upd.sum()), int(cupd.sum()))
    if not full:
        return n
    return n, {"upd": upd, "col": cupd, "fu": fu, "fv": fv, "sdf": sdf, "z": z, "seen": seen}


# ---- extraction -----------------------------------------------------------------------------------------------------------------
def _shift(a, dz, dy, dx, fill):
    """b[k,j,i] = a[k+dz, j+dy, i+dx], `fill` beyond the lattice."""
    b = np.full_like(a, fill)
    nz, ny, nx = a.shape
    b[:nz - dz, :ny - dy, :nx - dx] = a[dz:, dy:, dx:]
    return b


def mesh_host(tsdf_w, rgb_w, origin, voxel, min_weight=1.0, full=False, first=(0, 0, 0), where=False):
    """The mesh of a volume: (rows [V,4] int32 = {float32 x, y, z bits; rgba}, triangles [T,3] int32, counters int64 [8] = V, T, V, T, 0,
    0, 0, 0).  Vertex (q, d): t = T0 / (T0 - T1) of the distances at q and q + d, p = origin + voxel (q + t d), colour c0 + t (c1 - c0)
    of the endpoints' mean colours, all in float64, rounded once to float32; the colour bytes by ``quantise_colour``, alpha 255.  With
    ``full`` also the float64 positions [V,3].  ``first``: the (signed) lattice index of the array's sample [0,0,0], so q = first + the
    array index.  ``where``: also the flat array index of every vertex's sample q [V] and of every triangle's cube [T] (what a
    reordering needs)."""
    tsdf_w, rgb_w = np.asarray(tsdf_w, dtype=np.float32), np.asarray(rgb_w, dtype=np.float32)
    nz, ny, nx = tsdf_w.shape[:3]
    check_lattice(nx, ny, nz)
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    voxel = float(voxel)
    T = tsdf_w[..., 0]
    with np.errstate(invalid="ignore"):
        known = tsdf_w[..., 1] >= np.float32(min_weight)
        inside = T < 0
    off = lambda c: ((c >> 2) & 1, (c >> 1) & 1, c & 1)      # (dz, dy, dx) of a corner / direction
    stride = lambda c: off(c)[0] * ny * nx + off(c)[1] * nx + off(c)[2]
    valid = np.ones((nz, ny, nx), dtype=bool)                # cube with origin q: its 8 corners known (False on the upper faces)
    corners = np.zeros((nz, ny, nx), dtype=np.int64)         # its corners' inside bits
    for c in range(8):
        valid &= _shift(known, *off(c), False)
        corners |= _shift(inside, *off(c), False).astype(np.int64) << c
    vp = np.zeros((nz + 1, ny + 1, nx + 1), dtype=bool)      # vp[q + 1] = valid[q]; index 0: the cube at -1
    vp[1:, 1:, 1:] = valid
    vmask = np.zeros((nz, ny, nx), dtype=np.int64)
    for d in range(1, 8):
        dz, dy, dx = off(d)
        near = np.zeros((nz, ny, nx), dtype=bool)            # some valid cube contains the edge (q, d): origins q - e, e within the zero bits of d
        for e in range(8):
            if e & d:
                continue
            ez, ey, ex = off(e)
            near |= vp[1 - ez:1 - ez + nz, 1 - ey:1 - ey + ny, 1 - ex:1 - ex + nx]
        vmask |= (near & (inside != _shift(inside, dz, dy, dx, False))).astype(np.int64) << d
    vm = vmask.reshape(-1)
    vcount = POPCOUNT[vm]
    vbase = np.cumsum(vcount) - vcount
    V = int(vcount.sum())
    xyz = np.zeros((V, 3), dtype=np.float64)
    rgb = np.zeros((V, 3), dtype=np.float64)
    Tf, Cf = T.reshape(-1).astype(np.float64), rgb_w.reshape(-1, 4)[:, :3].astype(np.float64)
    for d in range(1, 8):
        q = np.flatnonzero((vm >> d) & 1)
        idx = vbase[q] + POPCOUNT[vm[q] & ((1 << d) - 1)]
        t = Tf[q] / (Tf[q] - Tf[q + stride(d)])
        qi = (np.stack([q % nx, (q // nx) % ny, q // (nx * ny)], 1) + np.array([int(a) for a in first], dtype=np.int64)[None, :]).astype(np.float64)
        dv = np.array([d & 1, (d >> 1) & 1, (d >> 2) & 1], dtype=np.float64)
        xyz[idx] = o[None, :] + voxel * (qi + t[:, None] * dv[None, :])
        with np.errstate(invalid="ignore"):
            rgb[idx] = Cf[q] + t[:, None] * (Cf[q + stride(d)] - Cf[q])
    vq = np.repeat(np.arange(len(vm), dtype=np.int64), vcount)      # (a sample's vertices are consecutive, by d)
    rows = np.empty((V, 4), dtype=np.int32)
    rows[:, :3] = xyz.astype(np.float32).view(np.int32)
    with np.errstate(invalid="ignore"):
        b = quantise_colour(rgb.astype(np.float32)).astype(np.uint32)
    rows[:, 3] = (b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | np.uint32(0xff000000)).view(np.int32)
    # triangles
    cm, ok = corners.reshape(-1), valid.reshape(-1)
    tmask = [sum(((cm >> TET_CORNERS[k][v]) & 1) << v for v in range(4)) for k in range(6)]
    per_tet = [np.where(ok, CASE_COUNT[m], 0) for m in tmask]
    tcount = sum(per_tet)
    tbase = np.cumsum(tcount) - tcount
    Tn = int(tcount.sum())
    tris = np.zeros((Tn, 3), dtype=np.int64)
    before = np.zeros_like(tcount)
    for k in range(6):
        for s in range(2):
            q = np.flatnonzero(per_tet[k] > s)
            case = _CASE_ARRAY[tmask[k][q], s]               # [m, 3] tetrahedron-edge ids
            if TET_ODD[k]:
                case = case[:, [0, 2, 1]]
            out = np.empty((len(q), 3), dtype=np.int64)
            for j in range(3):
                lo = np.array([TET_CORNERS[k][a] for a, _ in TET_EDGES], dtype=np.int64)[case[:, j]]
                hi = np.array([TET_CORNERS[k][b] for _, b in TET_EDGES], dtype=np.int64)[case[:, j]]
                cs = np.array([stride(c) for c in range(8)], dtype=np.int64)
                smp = q + cs[lo]
                out[:, j] = vbase[smp] + POPCOUNT[vm[smp] & ((1 << (hi ^ lo)) - 1)]
            tris[tbase[q] + before[q] + s] = out
        before = before + per_tet[k]
    out = (rows, tris.astype(np.int32), np.array([V, Tn, V, Tn, 0, 0, 0, 0], dtype=np.int64))
    if full:
        out += (xyz,)
    if where:
        out += (vq, np.repeat(np.arange(len(tcount), dtype=np.int64), tcount))
    return out


# ---- checks on a mesh (tests, tools) ----------------------------------------------------------------------------------------------
def mesh_topology(n_vertices, triangles):
    """dict(closed: every directed edge occurs once and its reverse once; boundary: directed edges without their reverse; repeated:
    directed edges that occur more than once; euler: V - E + F; unreferenced: vertices no triangle uses)."""
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    a = np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2]])
    b = np.concatenate([tri[:, 1], tri[:, 2], tri[:, 0]])
    n = max(int(n_vertices), 1)
    fwd, counts = np.unique(a * n + b, return_counts=True)
    boundary = int((~np.isin(b * n + a, fwd)).sum())
    undirected = len(np.unique(np.minimum(a, b) * n + np.maximum(a, b)))
    used = np.zeros(int(n_vertices), dtype=bool)
    used[tri.reshape(-1)] = True
    repeated = int((counts > 1).sum())
    return {"closed": boundary == 0 and repeated == 0 and len(tri) > 0, "boundary": boundary, "repeated": repeated,
            "euler": int(n_vertices) - undirected + len(tri), "unreferenced": int((~used).sum())}


def signed_volume(xyz, triangles):
    """The volume enclosed by a closed mesh, positive when the normals point outwards."""
    p = np.asarray(xyz, dtype=np.float64)[np.asarray(triangles, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


# ---- volumes --------------------------------------------------------------------------------------------------------------------
def _mesh_counters(integrate, mesh):
    out = {name: int(integrate[k]) for k, name in enumerate(INTEGRATE_COUNTERS)}
    out.update({name: int(mesh[k]) for k, name in enumerate(MESH_COUNTERS)})
    return out


def _check_voxel_trunc(voxel, trunc, max_trunc_voxels=None):
    voxel, trunc = float(voxel), float(trunc)
    if not (np.isfinite(voxel) and voxel > 0 and np.isfinite(trunc) and trunc > 0):
        raise ValueError(f"voxel = {voxel}, trunc = {trunc} (both must be finite and positive)")
    if max_trunc_voxels is not None and not trunc <= max_trunc_voxels * voxel:
        raise ValueError(f"trunc = {trunc} is more than {max_trunc_voxels} voxel = {max_trunc_voxels * voxel}")
    return voxel, trunc


def double3(v):
    """A numpy origin or anchor as the C ABI's ``const double*`` of three values."""
    import ctypes as C
    return (C.c_double * 3)(*v.tolist())


def _emit_exact(device, totals, emit):
    """What both device extractions do behind the read-back of the plan's totals [V, T, ...]: rows and triangles allocated at exactly V and
    T, `emit(rows, V, triangles, T)`, and the emit's counter row -- the allocations are exact: nothing is dropped."""
    V, T = int(totals[0]), int(totals[1])
    if V >= 1 << 31:
        raise ValueError(f"mesh of {V} vertices: more than int32 triangle indices reach; raise mesh.voxel")
    rows = torch.empty(max(V, 1), 4, dtype=torch.int32, device=device)
    tris = torch.empty(max(T, 1), 3, dtype=torch.int32, device=device)
    emit(rows, V, tris, T)
    return rows[:V], tris[:T], np.array([V, T, V, T, 0, 0, 0, 0], dtype=np.int64)


class HostTsdfVolume:
    """The volume of ``device: cpu``: the host statement, view by view."""

    def __init__(self, dims, origin, voxel, trunc, H, W, cam, sil_min=0.99, depth_max=0.0, min_weight=1.0, device=None):
        self.nx, self.ny, self.nz = (int(v) for v in dims)
        check_lattice(self.nx, self.ny, self.nz)
        self.origin, (self.voxel, self.trunc) = np.asarray(origin, dtype=np.float64).reshape(3).copy(), _check_voxel_trunc(voxel, trunc)
        self.H, self.W, self.cam = int(H), int(W), cam
        self.sil_min, self.depth_max, self.min_weight = float(sil_min), float(depth_max), float(min_weight)
        self.tsdf_w, self.rgb_w = empty_volume(self.nx, self.ny, self.nz)
        self.c = [0, 0, 0]

    def add(self, color, depth, sil, pose):
        c = self.cam
        n = integrate_host(self.tsdf_w, self.rgb_w, color, depth, sil, pose, c["fx"], c["fy"], c["cx"], c["cy"], self.origin, self.voxel, self.trunc,
                           self.sil_min, self.depth_max)
        self.c[0] += 1; self.c[1] += n[0]; self.c[2] += n[1]

    def extract(self):
        rows, tris, m = mesh_host(self.tsdf_w, self.rgb_w, self.origin, self.voxel, self.min_weight)
        return rows, tris, _mesh_counters(self.c, m)


class TsdfVolume:
    """The device volume: owns the two arrays and the integration counters; ``add`` is one mm3dgs_tsdf_integrate call on the current stream,
    ``extract`` one mm3dgs_tsdf_mesh_plan, one read-back of the two totals, exact allocations and one mm3dgs_tsdf_mesh_emit."""

    def __init__(self, dims, origin, voxel, trunc, H, W, cam, sil_min=0.99, depth_max=0.0, min_weight=1.0, device="cuda:0"):
        from . import _lib
        self.nx, self.ny, self.nz = (int(v) for v in dims)
        check_lattice(self.nx, self.ny, self.nz)
        if not str(device).startswith("cuda"):
            raise ValueError("TsdfVolume needs a CUDA device (the host path is HostTsdfVolume)")
        self.origin, self.voxel, self.trunc = np.asarray(origin, dtype=np.float64).reshape(3).copy(), float(voxel), float(trunc)
        self.H, self.W, self.cam, self.device = int(H), int(W), cam, device
        self.sil_min, self.depth_max, self.min_weight = float(sil_min), float(depth_max), float(min_weight)
        self.lib = _lib.load()
        self.tsdf_w = torch.zeros(self.nz, self.ny, self.nx, 2, dtype=torch.float32, device=device)
        self.rgb_w = torch.zeros(self.nz, self.ny, self.nx, 4, dtype=torch.float32, device=device)
        self.counters = torch.zeros(8, dtype=torch.int64, device=device)

    def add(self, color, depth, sil, pose):
        from . import _lib
        from .rasterizer import _stream
        color_c, depth_c, sil_c, pose_c = device_view("TsdfVolume", self.H, self.W, color, depth, sil, pose)
        P = _lib.ptr
        _lib.check(self.lib.mm3dgs_tsdf_integrate(self.H, self.W, *cam_args(self.cam), P(pose_c), P(color_c), P(depth_c), P(sil_c), self.sil_min, self.depth_max,
                                                  double3(self.origin), self.voxel, self.trunc, self.nx, self.ny, self.nz, P(self.tsdf_w), P(self.rgb_w), P(self.counters), _stream()))

    def extract(self):
        """(rows [V,4] int32, triangles [T,3] int32, counters): tensors on the device."""
        from . import _lib
        from .rasterizer import _stream
        P = _lib.ptr
        nbytes = int(self.lib.mm3dgs_tsdf_mesh_work_bytes(self.nx, self.ny, self.nz))
        work = torch.empty(nbytes // 8, dtype=torch.int64, device=self.device)
        mc = torch.empty(8, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.mm3dgs_tsdf_mesh_plan(self.nx, self.ny, self.nz, P(self.tsdf_w), self.min_weight, P(work), P(mc), _stream()))
        totals = torch.cat([mc, self.counters]).cpu().numpy()      # the one read-back before the allocation
        rows, tris, m = _emit_exact(self.device, totals, lambda rows, V, tris, T: _lib.check(self.lib.mm3dgs_tsdf_mesh_emit(
            self.nx, self.ny, self.nz, P(self.tsdf_w), P(self.rgb_w), double3(self.origin), self.voxel, P(work), P(rows), V, P(tris), T, P(mc), _stream())))
        return rows, tris, _mesh_counters(totals[8:], m)


# ---- the volume as voxel blocks (mesh.volume: sparse) ------------------------------------------------------------------------------------
# One statement; the host path below and csrc/tsdf_sparse.hip both follow it.
#   Lattice      sample (i, j, k) in Z^3 (signed) sits at anchor + voxel (i, j, k), in float64 exactly in that form; block b = floor(index /
#                8) per axis, |b| < 2^20; key = (bz + 2^20) << 42 | (by + 2^20) << 21 | (bx + 2^20): ascending keys are blocks in z-major
#                raster order.
#   Reservation  per view, the only thing that decides which blocks exist.  A pixel (u, v) that passes ``valid_mask`` with depth d is lifted
#                to its world point P (``backproject_host``'s rule, not rounded); ax = (|u - cx| trunc + (d + trunc) / 2) / |fx|, ay
#                likewise, R = sqrt(ax^2 + ay^2 + trunc^2); per axis every block from floor(floor((P - R - anchor) / voxel) / 8) to
#                floor(ceil((P + R - anchor) / voxel) / 8) is reserved (with ``mesh.bounds``: only the blocks that intersect the box).
#                Why this R: a sample that the integration updates through (u, v) with |sdf| <= trunc has |z - d| <= trunc; its projection
#                is at most half a pixel from (u, v), so |x - (u - cx) z / fx| <= z / (2 |fx|); with p_d the pixel's point at depth d,
#                |x - x_d| <= |u - cx| |z - d| / |fx| + z / (2 |fx|) <= (|u - cx| trunc + (d + trunc) / 2) / |fx| = ax, likewise ay, and
#                |z - d| <= trunc: the sample lies within R of P.  floor and ceil leave a whole sample of slack for roundoff.  A pixel
#                whose box leaves |b| < 2^20 or spans more than 8 blocks on an axis is skipped and counted (trunc <= 16 voxel keeps a
#                box of an ordinary view within 6).
#   Two passes   all views are reserved, the set is frozen (keys sorted ascending; block r of the pool is the r-th key; the pool is tsdf_w
#                [n,512,2] and rgb_w [n,512,4], x fastest inside a block), then all views are integrated: every sample of a reserved block
#                carries exactly what the dense volume would hold there, every other sample is unknown (weight 0) and never touched.
#   Mesh         the dense rule applied to that masked lattice; vertices by block in ascending key, then by sample in raster order inside
#                the block, then by d; triangles by block, then cube, then tetrahedron, then case.
# Consequence: the sparse mesh is the dense mesh minus the triangles of cubes that have a corner in an unreserved block -- a cube that
# needs a negative sample next to a block no pixel's band reached.
BLOCK = 8
BLOCK_BIAS = 1 << 20
MAX_BLOCKS = 1 << 21
MAX_TRUNC_VOXELS = 16
MAX_BOX = 8                      # blocks a pixel's box may span per axis
BLOCK_BYTES = 512 * 24
RESERVE_COUNTERS = ("views", "valid", "pairs", "blocks", "dropped", "out_of_range", "index_errors")


def block_keys(blocks):
    """int64 keys of block coordinates [n,3] = (bx, by, bz), each |b| < 2^20."""
    b = np.asarray(blocks, dtype=np.int64).reshape(-1, 3) + BLOCK_BIAS
    return (b[:, 2] << 42) | (b[:, 1] << 21) | b[:, 0]


def key_blocks(keys):
    """Block coordinates [n,3] = (bx, by, bz) of int64 keys."""
    k = np.asarray(keys).astype(np.int64).reshape(-1)
    return np.stack([k & 0x1fffff, (k >> 21) & 0x1fffff, (k >> 42) & 0x1fffff], 1) - BLOCK_BIAS


def block_clip(bounds, anchor, voxel):
    """None, or int [6] = the lowest and the highest block coordinate per axis that holds a sample inside the box `bounds` = [xmin, ymin,
    zmin, xmax, ymax, zmax]."""
    if bounds is None:
        return None
    box, o = np.asarray(bounds, dtype=np.float64).reshape(6), np.asarray(anchor, dtype=np.float64).reshape(3)
    lo = np.floor(np.ceil((box[:3] - o) / float(voxel)) / BLOCK)
    hi = np.floor(np.floor((box[3:] - o) / float(voxel)) / BLOCK)
    return np.clip(np.concatenate([lo, hi]), -(BLOCK_BIAS - 1), BLOCK_BIAS - 1).astype(np.int64)


def reserve_host(depth, sil, pose, fx, fy, cx, cy, voxel, trunc, anchor=(0.0, 0.0, 0.0), sil_min=0.0, depth_max=0.0, clip=None, full=False):
    """The block set of one view in float64: (keys int64 [m] ascending, dict(valid, pairs, out_of_range)).  With ``full`` the dict also
    holds `near`: the valid pixels whose box edge lies within 1e-9 sample of a sample boundary on some axis (there another evaluation
    order may decide differently), and `keys_without_near`: the keys of all other pixels."""
    d = as_np(depth, np.float32)
    H, W = d.shape
    voxel, trunc = float(voxel), float(trunc)
    if not trunc <= MAX_TRUNC_VOXELS * voxel:
        raise ValueError(f"trunc = {trunc} is more than {MAX_TRUNC_VOXELS} voxel = {MAX_TRUNC_VOXELS * voxel}")
    idx = np.flatnonzero(valid_mask(d, sil, sil_min, depth_max).reshape(-1))
    z = d.reshape(-1)[idx].astype(np.float64)
    u, v = (idx % W).astype(np.float64), (idx // W).astype(np.float64)
    R, t = pose_rotation(pose)
    o = np.asarray(anchor, dtype=np.float64).reshape(3)
    fx, fy, cx, cy = float(fx), float(fy), float(cx), float(cy)
    c = [(u - cx) / fx * z - t[0], (v - cy) / fy * z - t[1], z - t[2]]
    ax = (np.abs(u - cx) * trunc + 0.5 * (z + trunc)) / abs(fx)
    ay = (np.abs(v - cy) * trunc + 0.5 * (z + trunc)) / abs(fy)
    rad = np.sqrt(ax * ax + ay * ay + trunc * trunc)
    ok = np.ones(len(idx), dtype=bool)
    near = np.zeros(len(idx), dtype=bool)
    lo, hi = np.zeros((len(idx), 3), dtype=np.int64), np.zeros((len(idx), 3), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            P = R[0, a] * c[0] + R[1, a] * c[1] + R[2, a] * c[2]
            ql, qh = (P - rad - o[a]) / voxel, (P + rad - o[a]) / voxel
            for q in (ql, qh):
                frac = q - np.floor(q)
                near |= (frac < 1e-9) | (frac > 1 - 1e-9)
            bl, bh = np.floor(np.floor(ql) / BLOCK), np.floor(np.ceil(qh) / BLOCK)
            fine = (np.abs(bl) < BLOCK_BIAS) & (np.abs(bh) < BLOCK_BIAS) & (bh - bl < MAX_BOX)      # (a NaN fails)
            ok &= fine
            lo[:, a], hi[:, a] = np.where(fine, bl, 0).astype(np.int64), np.where(fine, bh, 0).astype(np.int64)
    if clip is not None:
        cl = np.asarray(clip, dtype=np.int64).reshape(6)
        lo, hi = np.maximum(lo, cl[None, :3]), np.minimum(hi, cl[None, 3:])
    keys, clean, pairs = [], [], 0
    span = (hi - lo)[ok].max(0) + 1 if ok.any() else np.zeros(3, dtype=np.int64)
    for dz in range(int(max(span[2], 0))):
        for dy in range(int(max(span[1], 0))):
            for dx in range(int(max(span[0], 0))):
                b = lo + np.array([dx, dy, dz], dtype=np.int64)[None, :]
                m = ok & (b <= hi).all(1)
                pairs += int(m.sum())
                keys.append(block_keys(b[m]))
                if full:
                    clean.append(block_keys(b[m & ~near]))
    cat = lambda parts: np.unique(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.int64)
    info = {"valid": len(idx), "pairs": pairs, "out_of_range": int((~ok).sum())}
    if full:
        info.update(near=int(near.sum()), keys_without_near=cat(clean))
    return cat(keys), info


def _frozen_lattice(keys, anchor, voxel):
    """(blocks [n,3], first [3] = the lattice index of the bounding lattice's first sample, dims [3], origin float64 [3]) of sorted keys."""
    blocks = key_blocks(keys)
    bmin, bmax = blocks.min(0), blocks.max(0)
    first = BLOCK * bmin
    return blocks, first, [int(v) for v in BLOCK * (bmax - bmin + 1)], np.asarray(anchor, dtype=np.float64).reshape(3) + float(voxel) * first.astype(np.float64)


def pool_index(blocks, first, dims, flat):
    """The pool index rank 512 + local raster index of the bounding lattice's samples `flat` (flat array indices, x fastest) -- -1 where the
    sample's block is not one of `blocks` [n,3] (ascending keys)."""
    nx, ny, nz = dims
    rank = np.full((nz // BLOCK, ny // BLOCK, nx // BLOCK), -1, dtype=np.int64)
    rel = blocks - first[None, :] // BLOCK
    rank[rel[:, 2], rel[:, 1], rel[:, 0]] = np.arange(len(blocks))
    flat = np.asarray(flat, dtype=np.int64)
    i, j, k = flat % nx, (flat // nx) % ny, flat // (nx * ny)
    r = rank[k // BLOCK, j // BLOCK, i // BLOCK]
    return np.where(r >= 0, r * 512 + (k % BLOCK) * 64 + (j % BLOCK) * BLOCK + i % BLOCK, -1)


def reorder_to_blocks(rows, tris, vq, tq, blocks, first, dims):
    """A mesh of ``mesh_host(..., where=True)`` over the bounding lattice in the voxel-block order: vertices by block in ascending key, then
    by sample in raster order inside the block, then by d; triangles by block, then cube, then tetrahedron, then case."""
    perm = np.argsort(pool_index(blocks, first, dims, vq), kind="stable")
    inv = np.empty(len(perm), dtype=np.int64)
    inv[perm] = np.arange(len(perm))
    order = np.argsort(pool_index(blocks, first, dims, tq), kind="stable")
    return rows[perm], inv[tris.astype(np.int64)][order].astype(np.int32).reshape(-1, 3), perm


def mesh_blocks_host(keys, tsdf_w, rgb_w, anchor, voxel, min_weight=1.0, full=False):
    """The mesh of a pool (tsdf_w [n,512,2], rgb_w [n,512,4], block r = the r-th of the ascending `keys`): ``mesh_host`` over the block
    set's bounding lattice, unknown outside the blocks, in the voxel-block order.  Returns what ``mesh_host`` returns."""
    keys = np.asarray(keys).astype(np.int64).reshape(-1)
    if len(keys) == 0 or not bool((np.diff(keys) > 0).all()):
        raise ValueError("mesh_blocks_host: the keys must be strictly ascending and at least one")
    blocks, first, dims, _ = _frozen_lattice(keys, anchor, voxel)
    nx, ny, nz = dims
    check_lattice(nx, ny, nz)
    s = pool_index(blocks, first, dims, np.arange(nx * ny * nz))
    tw, rw = np.zeros((nx * ny * nz, 2), dtype=np.float32), np.zeros((nx * ny * nz, 4), dtype=np.float32)
    tw[s >= 0], rw[s >= 0] = np.asarray(tsdf_w, dtype=np.float32).reshape(-1, 2)[s[s >= 0]], np.asarray(rgb_w, dtype=np.float32).reshape(-1, 4)[s[s >= 0]]
    rows, tris, m, xyz, vq, tq = mesh_host(tw.reshape(nz, ny, nx, 2), rw.reshape(nz, ny, nx, 4), anchor, voxel, min_weight, full=True, first=first, where=True)
    rows, tris, perm = reorder_to_blocks(rows, tris, vq, tq, blocks, first, dims)
    return (rows, tris, m, xyz[perm]) if full else (rows, tris, m)


def _sparse_counters(integrate, mesh, reserve, n):
    out = _mesh_counters(integrate, mesh)
    out.update(blocks=int(n), pairs=int(reserve[2]), volume_bytes=int(n) * BLOCK_BYTES, reserved_pixels=int(reserve[1]), out_of_range=int(reserve[5]))
    return out


def _check_frozen(c, max_blocks, voxel):
    """The counters of a reservation [views, valid, pairs, blocks, dropped, out of range, ...] before the pool is made."""
    if int(c[1]) == 0:
        raise ValueError("mesh export: no view has a valid pixel (mesh.sil_min, mesh.max_depth)")
    if int(c[4]) > 0 or int(c[3]) > int(max_blocks):
        raise ValueError(f"mesh export: the views need {int(c[3])} voxel blocks ({int(c[4])} dropped), more than mesh.max_blocks = {int(max_blocks)} "
                         f"(at most 2^21) hold at mesh.voxel = {voxel} m; raise mesh.max_blocks or mesh.voxel, or set mesh.bounds")
    if int(c[3]) == 0:
        raise ValueError(f"mesh export: no voxel block was reserved ({int(c[5])} of {int(c[1])} valid pixels out of range; mesh.bounds, mesh.voxel)")


def _sparse_options(voxel, trunc, max_blocks):
    voxel, trunc = _check_voxel_trunc(voxel, trunc, MAX_TRUNC_VOXELS)
    if not 1 <= int(max_blocks) <= MAX_BLOCKS:
        raise ValueError(f"max_blocks = {max_blocks} (1 .. 2^21)")
    return voxel, trunc, int(max_blocks)


class HostSparseTsdfVolume:
    """The voxel-block volume of ``device: cpu``: ``reserve`` every view, ``freeze``, ``add`` every view, ``extract``.  The host statement
    run over the block set's bounding lattice -- ``integrate_host`` / ``mesh_host`` with the unreserved samples zeroed after every view --
    and reordered to the block order; it holds that whole lattice (at most 2^30 samples), so it is the yardstick, not the memory saving."""

    def __init__(self, voxel, trunc, H, W, cam, sil_min=0.99, depth_max=0.0, min_weight=1.0, max_blocks=1 << 18, bounds=None, anchor=(0.0, 0.0, 0.0), device=None):
        self.voxel, self.trunc, self.max_blocks = _sparse_options(voxel, trunc, max_blocks)
        self.anchor = np.asarray(anchor, dtype=np.float64).reshape(3).copy()
        self.H, self.W, self.cam = int(H), int(W), cam
        self.sil_min, self.depth_max, self.min_weight = float(sil_min), float(depth_max), float(min_weight)
        self.clip = block_clip(bounds, self.anchor, self.voxel)
        self.keys, self.rc, self.c = np.zeros(0, dtype=np.int64), [0] * 8, [0, 0, 0]
        self.blocks = None

    def reserve(self, depth, sil, pose):
        if self.blocks is not None:
            raise RuntimeError("HostSparseTsdfVolume.reserve after freeze")
        c = self.cam
        keys, info = reserve_host(depth, sil, pose, c["fx"], c["fy"], c["cx"], c["cy"], self.voxel, self.trunc, self.anchor, self.sil_min, self.depth_max, self.clip)
        self.keys = np.union1d(self.keys, keys)
        self.rc[0] += 1; self.rc[1] += info["valid"]; self.rc[2] += info["pairs"]; self.rc[5] += info["out_of_range"]
        self.rc[3] = len(self.keys)

    def freeze(self):
        _check_frozen(self.rc, self.max_blocks, self.voxel)
        self.blocks, self.first, self.dims, self.origin = _frozen_lattice(self.keys, self.anchor, self.voxel)
        nx, ny, nz = self.dims
        if nx * ny * nz > MAX_SAMPLES:
            raise ValueError(f"mesh export: the host path holds the block set's bounding lattice, {nx} x {ny} x {nz} samples (at most 2^30); raise mesh.voxel or set mesh.bounds")
        self.tsdf_w, self.rgb_w = empty_volume(nx, ny, nz)
        self.reserved = (pool_index(self.blocks, self.first, self.dims, np.arange(nx * ny * nz)) >= 0).reshape(nz, ny, nx)
        return len(self.keys)

    def add(self, color, depth, sil, pose):
        if self.blocks is None:
            raise RuntimeError("HostSparseTsdfVolume.add before freeze")
        c = self.cam
        _, g = integrate_host(self.tsdf_w, self.rgb_w, color, depth, sil, pose, c["fx"], c["fy"], c["cx"], c["cy"], self.anchor, self.voxel, self.trunc,
                              self.sil_min, self.depth_max, full=True, first=self.first)
        self.tsdf_w[~self.reserved] = 0      # a sample outside the frozen set is never touched
        self.rgb_w[~self.reserved] = 0
        self.c[0] += 1; self.c[1] += int((g["upd"] & self.reserved).sum()); self.c[2] += int((g["col"] & self.reserved).sum())

    def pool(self):
        """(tsdf_w [n,512,2], rgb_w [n,512,4]): the reserved blocks' samples in the pool's order."""
        nx, ny, nz = self.dims
        s = pool_index(self.blocks, self.first, self.dims, np.arange(nx * ny * nz))
        at = np.argsort(s, kind="stable")[int((s < 0).sum()):]
        return self.tsdf_w.reshape(-1, 2)[at].reshape(-1, 512, 2), self.rgb_w.reshape(-1, 4)[at].reshape(-1, 512, 4)

    def extract(self):
        rows, tris, m, vq, tq = mesh_host(self.tsdf_w, self.rgb_w, self.anchor, self.voxel, self.min_weight, first=self.first, where=True)
        rows, tris, _ = reorder_to_blocks(rows, tris, vq, tq, self.blocks, self.first, self.dims)
        return rows, tris, _sparse_counters(self.c, m, self.rc, len(self.keys))


class SparseTsdfVolume:
    """The device voxel-block volume: owns the table, the counters and -- from ``freeze`` on -- the sorted keys, the neighbour table and the
    pool.  ``reserve`` is one mm3dgs_tsdf_blocks_reserve call on the current stream; ``freeze`` one read-back of the counters, one
    mm3dgs_tsdf_blocks_list, one torch.sort (once per export: plumbing) and one mm3dgs_tsdf_blocks_index; ``add`` one
    mm3dgs_tsdf_blocks_integrate; ``extract`` one mm3dgs_tsdf_blocks_mesh_plan, one read-back (the totals, the counters and the block
    set's bounding box), exact allocations and one mm3dgs_tsdf_blocks_mesh_emit."""

    def __init__(self, voxel, trunc, H, W, cam, sil_min=0.99, depth_max=0.0, min_weight=1.0, max_blocks=1 << 18, bounds=None, anchor=(0.0, 0.0, 0.0), device="cuda:0"):
        import ctypes as C
        from . import _lib
        from .rasterizer import _stream
        if not str(device).startswith("cuda"):
            raise ValueError("SparseTsdfVolume needs a CUDA device (the host path is HostSparseTsdfVolume)")
        self.voxel, self.trunc, self.max_blocks = _sparse_options(voxel, trunc, max_blocks)
        self.anchor = np.asarray(anchor, dtype=np.float64).reshape(3).copy()
        self.H, self.W, self.cam, self.device = int(H), int(W), cam, device
        self.sil_min, self.depth_max, self.min_weight = float(sil_min), float(depth_max), float(min_weight)
        clip = block_clip(bounds, self.anchor, self.voxel)
        self.clip = None if clip is None else (C.c_int * 6)(*[int(v) for v in clip])
        self.lib = _lib.load()
        self.table_bytes = int(self.lib.mm3dgs_tsdf_blocks_table_bytes(self.max_blocks))
        self.table = torch.empty(self.table_bytes // 8, dtype=torch.int64, device=device)
        self.rc = torch.zeros(8, dtype=torch.int64, device=device)          # the reservation's counters
        self.counters = torch.zeros(8, dtype=torch.int64, device=device)    # the integration's
        self.n = None
        _lib.check(self.lib.mm3dgs_tsdf_blocks_reset(_lib.ptr(self.table), self.max_blocks, _lib.ptr(self.rc), _stream()))

    def reserve(self, depth, sil, pose):
        from . import _lib
        from .rasterizer import _stream
        if self.n is not None:
            raise RuntimeError("SparseTsdfVolume.reserve after freeze")
        _, depth_c, sil_c, pose_c = device_view("SparseTsdfVolume", self.H, self.W, None, depth, sil, pose, "reserve")
        P = _lib.ptr
        _lib.check(self.lib.mm3dgs_tsdf_blocks_reserve(self.H, self.W, *cam_args(self.cam), P(pose_c), P(depth_c), P(sil_c), self.sil_min, self.depth_max,
                                                       double3(self.anchor), self.voxel, self.trunc, self.clip, P(self.table), self.max_blocks, P(self.rc), _stream()))

    def freeze(self):
        """Lists, sorts and indexes the block set and allocates the pool at exactly n blocks; returns n.  ValueError when blocks were
        dropped (``mesh.max_blocks``) or no view had a valid pixel."""
        from . import _lib
        from .rasterizer import _stream
        P = _lib.ptr
        c = self.rc.cpu().numpy()      # the one read-back
        _check_frozen(c, self.max_blocks, self.voxel)
        n = int(c[3])
        keys = torch.empty(n, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.mm3dgs_tsdf_blocks_list(P(self.table), self.max_blocks, P(keys), n, _stream()))
        self.keys = torch.sort(keys).values.contiguous()
        self.neighbours = torch.empty(n, 27, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.mm3dgs_tsdf_blocks_index(P(self.table), self.max_blocks, P(self.keys), n, P(self.neighbours), P(self.rc), _stream()))
        self.tsdf_w = torch.zeros(n, 512, 2, dtype=torch.float32, device=self.device)
        self.rgb_w = torch.zeros(n, 512, 4, dtype=torch.float32, device=self.device)
        self.n = n
        return n

    def add(self, color, depth, sil, pose):
        from . import _lib
        from .rasterizer import _stream
        if self.n is None:
            raise RuntimeError("SparseTsdfVolume.add before freeze")
        color_c, depth_c, sil_c, pose_c = device_view("SparseTsdfVolume", self.H, self.W, color, depth, sil, pose)
        P = _lib.ptr
        _lib.check(self.lib.mm3dgs_tsdf_blocks_integrate(self.H, self.W, *cam_args(self.cam), P(pose_c), P(color_c), P(depth_c), P(sil_c), self.sil_min, self.depth_max,
                                                         double3(self.anchor), self.voxel, self.trunc, P(self.keys), self.n, P(self.tsdf_w), P(self.rgb_w), P(self.counters), _stream()))

    def extract(self):
        """(rows [V,4] int32, triangles [T,3] int32, counters): tensors on the device; sets ``dims`` and ``origin`` of the bounding lattice."""
        from . import _lib
        from .rasterizer import _stream
        P, n = _lib.ptr, self.n
        nbytes = int(self.lib.mm3dgs_tsdf_blocks_mesh_work_bytes(n))
        work = torch.empty(nbytes // 8, dtype=torch.int64, device=self.device)
        mc = torch.empty(8, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.mm3dgs_tsdf_blocks_mesh_plan(n, P(self.neighbours), P(self.tsdf_w), self.min_weight, P(work), P(mc), _stream()))
        digits = torch.stack([self.keys & 0x1fffff, (self.keys >> 21) & 0x1fffff, self.keys >> 42], 1)      # bx, by, bz + 2^20
        totals = torch.cat([mc, self.counters, self.rc, digits.amin(0), digits.amax(0)]).cpu().numpy()      # the one read-back before the allocation
        rc = totals[16:24]
        if int(rc[6]):
            raise RuntimeError(f"SparseTsdfVolume: mm3dgs_tsdf_blocks_index rejected {int(rc[6])} of the {n} sorted keys")
        bmin, bmax = totals[24:27].astype(np.int64) - BLOCK_BIAS, totals[27:30].astype(np.int64) - BLOCK_BIAS
        self.dims = [int(v) for v in BLOCK * (bmax - bmin + 1)]
        self.origin = self.anchor + self.voxel * (BLOCK * bmin).astype(np.float64)
        rows, tris, m = _emit_exact(self.device, totals, lambda rows, V, tris, T: _lib.check(self.lib.mm3dgs_tsdf_blocks_mesh_emit(
            n, P(self.keys), P(self.neighbours), P(self.tsdf_w), P(self.rgb_w), double3(self.anchor), self.voxel, P(work), P(rows), V, P(tris), T, P(mc), _stream())))
        return rows, tris, _sparse_counters(totals[8:16], m, rc, n)


# ---- files ----------------------------------------------------------------------------------------------------------------------
_FACE =np.dtype([("n", "u1"), ("v", "<i4", 3)])
NORMAL_PROPERTIES = "property float nx\nproperty float ny\nproperty float nz\n"


def mesh_header(n_vertices, n_faces, normals=False):
    props = CLOUD_PROPERTIES.replace("property uchar red\n", NORMAL_PROPERTIES + "property uchar red\n") if normals else CLOUD_PROPERTIES
    return ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {int(n_vertices)}\n" + props
            + f"element face {int(n_faces)}\nproperty list uchar int vertex_indices\nend_header\n")


def write_mesh_ply(path, rows, triangles, normals=None):
    """Binary little-endian PLY: ``float x y z; uchar red green blue alpha`` per vertex (the row bytes as they are), ``list uchar int
    vertex_indices`` per face (the byte 3, then three int32).  With `normals` (float32 [V,3], ``geometry.vertex_normals``) a vertex is
    ``float x y z; float nx ny nz; uchar red green blue alpha`` (28 bytes); without them the file is what it has always been."""
    rows = as_np(rows, np.int32).reshape(-1, 4)
    tri = as_np(triangles, np.int32).reshape(-1, 3)
    faces = np.empty(len(tri), dtype=_FACE)
    faces["n"] = 3
    faces["v"] = tri
    body = rows.astype("<i4", copy=False)
    if normals is not None:
        nrm = as_np(normals, np.float32).reshape(-1, 3)
        if len(nrm) != len(rows):
            raise ValueError(f"{len(nrm)} normals for {len(rows)} vertices")
        body = np.concatenate([body[:, :3], nrm.astype("<f4", copy=False).view("<i4"), body[:, 3:]], 1)
    with open(path, "wb") as fh:
        fh.write(mesh_header(len(rows), len(tri), normals is not None).encode("ascii"))
        fh.write(np.ascontiguousarray(body).tobytes())
        fh.write(faces.tobytes())
    return path


def read_mesh_ply_normals(path):
    """(rows [V,4] int32, triangles [T,3] int32, normals float32 [V,3] or None) of a file written by ``write_mesh_ply``."""
    plain = ["x", "y", "z", "red", "green", "blue", "alpha"]
    with open(path, "rb") as fh:
        elements = read_header(fh)
        names = [p for _, p in elements[0][2]] if elements else []
        if ([e[0] for e in elements] != ["vertex", "face"] or names not in (plain, plain[:3] + ["nx", "ny", "nz"] + plain[3:])
                or elements[1][2] != [("list", "uchar")]):
            raise ValueError(f"{path}: not a mesh of write_mesh_ply")
        nv, nf, words = elements[0][1], elements[1][1], 4 if names == plain else 7
        body, faces = fh.read(4 * words * nv), fh.read(_FACE.itemsize * nf)
    if len(body) != 4 * words * nv or len(faces) != _FACE.itemsize * nf:
        raise ValueError(f"{path}: {len(body)} + {len(faces)} body bytes for {nv} vertices and {nf} faces")
    f = np.frombuffer(faces, dtype=_FACE)
    if not bool((f["n"] == 3).all()):
        raise ValueError(f"{path}: a face that is not a triangle")
    body = np.frombuffer(body, dtype="<i4").reshape(nv, words)
    if words == 4:
        return body.copy(), f["v"].astype(np.int32).copy(), None
    return np.ascontiguousarray(body[:, [0, 1, 2, 6]]), f["v"].astype(np.int32).copy(), np.ascontiguousarray(body[:, 3:6]).view(np.float32)


def read_mesh_ply(path):
    """(rows [V,4] int32, triangles [T,3] int32) of a file written by ``write_mesh_ply`` (with or without normals, which are dropped)."""
    return read_mesh_ply_normals(path)[:2]


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2", "int": "<i4",
              "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8"}


def _foreign_header(fh, path):
    """[(element name, count, [(property name, scalar type) or (property name, count type, item type)])] of a binary little-endian header."""
    if fh.readline().strip() != b"ply":
        raise ValueError(f"{path}: not a PLY file")
    elements, fmt = [], None
    while True:
        line = fh.readline()
        if not line:
            raise ValueError(f"{path}: PLY header without end_header")
        try:
            words = line.decode("ascii").split()
        except UnicodeDecodeError:
            raise ValueError(f"{path}: PLY header is not ASCII") from None
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "format":
            fmt = words[1] if len(words) > 1 else None
        elif words[0] == "element" and len(words) == 3 and words[2].isdigit():
            elements.append((words[1], int(words[2]), []))
        elif words[0] == "property" and elements and len(words) == 3 and words[1] in _PLY_TYPES:
            elements[-1][2].append((words[2], words[1]))
        elif words[0] == "property" and elements and len(words) == 5 and words[1] == "list" and words[2] in _PLY_TYPES and words[3] in _PLY_TYPES:
            elements[-1][2].append((words[4], words[2], words[3]))
        elif words[0] == "end_header":
            break
        else:
            raise ValueError(f"{path}: PLY header line {line!r}")
    if fmt != "binary_little_endian":
        raise ValueError(f"{path}: PLY format {fmt} (binary_little_endian only)")
    return elements


def read_foreign_ply(path):
    """A binary little-endian PLY file of another writer (a dataset's ground-truth mesh): rows [V,4] int32, or (rows, triangles [T,3] int32)
    when the file has a `face` element.  The `vertex` element: fixed-size scalar properties that include float x, y, z; the colour from
    uchar red, green, blue where present, else 255; alpha from uchar alpha where present, else 255; every other property (normals, ...) is
    skipped.  The optional `face` element, right behind it: one list property, a uchar count with int or uint indices; a polygon of more
    than three corners is fanned from corner 0, one of fewer is dropped.  Anything else -- ASCII or big-endian files, other elements, an
    index beyond the vertices, a short body -- raises ValueError."""
    with open(path, "rb") as fh:
        elements = _foreign_header(fh, path)
        names = [e[0] for e in elements]
        if names not in (["vertex"], ["vertex", "face"]):
            raise ValueError(f"{path}: elements {names} (vertex, then optionally face)")
        _, nv, props = elements[0]
        if any(len(p) != 2 for p in props) or len({p[0] for p in props}) != len(props):
            raise ValueError(f"{path}: the vertex element must have distinct scalar properties")
        vtype = np.dtype([(name, _PLY_TYPES[t]) for name, t in props])
        if any(k not in vtype.names or vtype[k] != np.dtype("<f4") for k in "xyz"):
            raise ValueError(f"{path}: the vertex element needs float x, y, z")
        body = fh.read(vtype.itemsize * nv)
        if len(body) != vtype.itemsize * nv:
            raise ValueError(f"{path}: {len(body)} body bytes for {nv} vertices of {vtype.itemsize} bytes")
        vert = np.frombuffer(body, dtype=vtype)
        faces = None
        if len(elements) == 2:
            _, nf, fprops = elements[1]
            if len(fprops) != 1 or len(fprops[0]) != 3 or _PLY_TYPES[fprops[0][1]] != "u1" or _PLY_TYPES[fprops[0][2]] not in ("<i4", "<u4"):
                raise ValueError(f"{path}: the face element must be one list property of uchar counts and int / uint indices")
            faces = (nf, fh.read())
    rows = np.empty((nv, 4), dtype=np.int32)
    for k, name in enumerate("xyz"):
        rows[:, k] = vert[name].view(np.int32)
    rgba = np.full((nv, 4), 255, dtype=np.uint32)
    for k, name in enumerate(("red", "green", "blue", "alpha")):
        if name in vtype.names and vtype[name] == np.dtype("u1"):
            rgba[:, k] = vert[name]
    rows[:, 3] = (rgba[:, 0] | (rgba[:, 1] << 8) | (rgba[:, 2] << 16) | (rgba[:, 3] << 24)).astype(np.uint32).view(np.int32)
    if faces is None:
        return rows
    nf, data = faces
    raw = np.frombuffer(data, dtype=np.uint8)
    # the start of every face record: a uniform corner count is one strided view, anything else is walked
    k0 = int(raw[0]) if nf and len(raw) else 0
    if nf and len(raw) >= nf * (1 + 4 * k0) and bool((raw[:nf * (1 + 4 * k0):1 + 4 * k0] == k0).all()):
        starts, counts = np.arange(nf, dtype=np.int64) * (1 + 4 * k0), np.full(nf, k0, dtype=np.int64)
    else:
        starts, counts, at = np.empty(nf, dtype=np.int64), np.empty(nf, dtype=np.int64), 0
        for f in range(nf):
            if at >= len(raw):
                raise ValueError(f"{path}: the body ends inside face {f}")
            starts[f], counts[f] = at, int(raw[at])
            at += 1 + 4 * int(raw[at])
    if nf and int(starts[-1] + 1 + 4 * counts[-1]) > len(raw):
        raise ValueError(f"{path}: the body ends inside the faces")
    tris = []
    for k in np.unique(counts):
        if k < 3:
            continue
        s = starts[counts == k]
        idx = raw[(s[:, None] + 1 + np.arange(4 * k)[None, :])].reshape(-1, 4 * int(k)).copy().view("<u4").astype(np.int64)      # [faces, k]
        if idx.size and (idx.max() >= nv):
            raise ValueError(f"{path}: a face index beyond the {nv} vertices")
        fan = np.stack([np.stack([idx[:, 0], idx[:, j], idx[:, j + 1]], 1) for j in range(1, int(k) - 1)], 1)      # [faces, k - 2, 3]
        tris.append((np.repeat(s, int(k) - 2), fan.reshape(-1, 3)))
    if not tris:
        return rows, np.zeros((0, 3), dtype=np.int32)
    order = np.argsort(np.concatenate([t[0] for t in tris]), kind="stable")      # file order, a polygon's fan in corner order
    return rows, np.concatenate([t[1] for t in tris])[order].astype(np.int32)


def read_surface_ply(path):
    """A surface file: one of this package's two writers -- ``read_mesh_ply`` (rows, triangles) when the header has a face element, else
    ``read_ply`` rows --, and when those strict readers reject it, ``read_foreign_ply`` (a dataset's mesh: normals, no alpha, uint indices)."""
    try:
        with open(path, "rb") as fh:
            has_faces = any(e[0] == "face" for e in read_header(fh))
        return read_mesh_ply(path) if has_faces else read_ply(path)
    except (ValueError, IndexError):
        return read_foreign_ply(path)
