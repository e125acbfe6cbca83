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
order, then by d; triangles by cube in raster order, then by tetrahedron, then by case order; the normal points from inside to outside."""
from __future__ import annotations

import numpy as np
import torch

from .pointcloud import CLOUD_PROPERTIES, as_np, device_view, pose_rotation, quantise_colour, read_header, read_ply, valid_mask

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
def integrate_host(tsdf_w, rgb_w, color, depth, sil, pose, fx, fy, cx, cy, origin, voxel, trunc, sil_min=0.0, depth_max=0.0, full=False):
    """One view into the volume, in place, in float64 from the float32 inputs.  Per sample: p_c = R p_w + t, skipped if z <= 0; pixel u =
    floor(fx x / z + cx + 0.5), v likewise (pixel centres at integer coordinates), skipped outside the image or where the pixel fails the
    point cloud's validity test; sdf = depth - z, skipped if sdf < -trunc; s = min(1, sdf / trunc); T <- (T W + s) / (W + 1), W <- W + 1,
    rounded to float32 once; the colour mean and its weight likewise, only if sdf <= trunc.  Returns (distance updates, colour updates);
    with ``full`` also dict(upd, col: the masks [nz,ny,nx]; fu, fv: the pixel coordinates before the floor; sdf; z)."""
    col = as_np(color, np.float32)
    d = as_np(depth, np.float32)
    H, W = d.shape
    nz, ny, nx = tsdf_w.shape[:3]
    ok = valid_mask(d, sil, sil_min, depth_max)
    R, t = pose_rotation(pose)
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    voxel, trunc = float(voxel), float(trunc)
    pw = [o[0] + voxel * np.arange(nx, dtype=np.float64)[None, None, :], o[1] + voxel * np.arange(ny, dtype=np.float64)[None, :, None],
          o[2] + voxel * np.arange(nz, dtype=np.float64)[:, None, None]]
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


def mesh_host(tsdf_w, rgb_w, origin, voxel, min_weight=1.0, full=False):
    """The mesh of a volume: (rows [V,4] int32 = {float32 x, y, z bits; rgba}, triangles [T,3] int32, counters int64 [8] = V, T, V, T, 0,
    0, 0, 0).  Vertex (q, d): t = T0 / (T0 - T1) of the distances at q and q + d, p = origin + voxel (q + t d), colour c0 + t (c1 - c0)
    of the endpoints' mean colours, all in float64, rounded once to float32; the colour bytes by ``quantise_colour``, alpha 255.  With
    ``full`` also the float64 positions [V,3]."""
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
        qi = np.stack([q % nx, (q // nx) % ny, q // (nx * ny)], 1).astype(np.float64)
        dv = np.array([d & 1, (d >> 1) & 1, (d >> 2) & 1], dtype=np.float64)
        xyz[idx] = o[None, :] + voxel * (qi + t[:, None] * dv[None, :])
        with np.errstate(invalid="ignore"):
            rgb[idx] = Cf[q] + t[:, None] * (Cf[q + stride(d)] - Cf[q])
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
    return out + (xyz,) if full else out


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


class HostTsdfVolume:
    """The volume of ``device: cpu``: the host statement, view by view."""

    def __init__(self, dims, origin, voxel, trunc, H, W, cam, sil_min=0.99, depth_max=0.0, min_weight=1.0, device=None):
        self.nx, self.ny, self.nz = (int(v) for v in dims)
        check_lattice(self.nx, self.ny, self.nz)
        self.origin, self.voxel, self.trunc = np.asarray(origin, dtype=np.float64).reshape(3).copy(), float(voxel), float(trunc)
        if not (np.isfinite(self.voxel) and self.voxel > 0 and np.isfinite(self.trunc) and self.trunc > 0):
            raise ValueError(f"voxel = {voxel}, trunc = {trunc} (both must be finite and positive)")
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

    def _origin(self):
        import ctypes as C
        return (C.c_double * 3)(*self.origin.tolist())

    def add(self, color, depth, sil, pose):
        from . import _lib
        from .rasterizer import _stream
        color_c, depth_c, sil_c, pose_c = device_view("TsdfVolume", self.H, self.W, color, depth, sil, pose)
        c, P = self.cam, _lib.ptr
        _lib.check(self.lib.mm3dgs_tsdf_integrate(self.H, self.W, float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"]), P(pose_c), P(color_c),
                                                  P(depth_c), P(sil_c), self.sil_min, self.depth_max, self._origin(), self.voxel, self.trunc,
                                                  self.nx, self.ny, self.nz, P(self.tsdf_w), P(self.rgb_w), P(self.counters), _stream()))

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
        V, T = int(totals[0]), int(totals[1])
        if V >= 1 << 31:
            raise ValueError(f"mesh of {V} vertices: more than int32 triangle indices reach; raise mesh.voxel")
        rows = torch.empty(max(V, 1), 4, dtype=torch.int32, device=self.device)
        tris = torch.empty(max(T, 1), 3, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.mm3dgs_tsdf_mesh_emit(self.nx, self.ny, self.nz, P(self.tsdf_w), P(self.rgb_w), self._origin(), self.voxel, P(work), P(rows), V,
                                                  P(tris), T, P(mc), _stream()))
        m = np.array([V, T, V, T, 0, 0, 0, 0], dtype=np.int64)     # the allocations are exact: nothing is dropped
        return rows[:V], tris[:T], _mesh_counters(totals[8:], m)


# ---- files ----------------------------------------------------------------------------------------------------------------------
_FACE = np.dtype([("n", "u1"), ("v", "<i4", 3)])


def mesh_header(n_vertices, n_faces):
    return ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {int(n_vertices)}\n" + CLOUD_PROPERTIES
            + f"element face {int(n_faces)}\nproperty list uchar int vertex_indices\nend_header\n")


def write_mesh_ply(path, rows, triangles):
    """Binary little-endian PLY: ``float x y z; uchar red green blue alpha`` per vertex (the row bytes as they are), ``list uchar int
    vertex_indices`` per face (the byte 3, then three int32)."""
    rows = as_np(rows, np.int32).reshape(-1, 4)
    tri = as_np(triangles, np.int32).reshape(-1, 3)
    faces = np.empty(len(tri), dtype=_FACE)
    faces["n"] = 3
    faces["v"] = tri
    with open(path, "wb") as fh:
        fh.write(mesh_header(len(rows), len(tri)).encode("ascii"))
        fh.write(rows.astype("<i4", copy=False).tobytes())
        fh.write(faces.tobytes())
    return path


def read_mesh_ply(path):
    """(rows [V,4] int32, triangles [T,3] int32) of a file written by ``write_mesh_ply``."""
    with open(path, "rb") as fh:
        elements = read_header(fh)
        if ([e[0] for e in elements] != ["vertex", "face"] or [p for _, p in elements[0][2]] != ["x", "y", "z", "red", "green", "blue", "alpha"]
                or elements[1][2] != [("list", "uchar")]):
            raise ValueError(f"{path}: not a mesh of write_mesh_ply")
        nv, nf = elements[0][1], elements[1][1]
        body, faces = fh.read(16 * nv), fh.read(_FACE.itemsize * nf)
    if len(body) != 16 * nv or len(faces) != _FACE.itemsize * nf:
        raise ValueError(f"{path}: {len(body)} + {len(faces)} body bytes for {nv} vertices and {nf} faces")
    f = np.frombuffer(faces, dtype=_FACE)
    if not bool((f["n"] == 3).all()):
        raise ValueError(f"{path}: a face that is not a triangle")
    return np.frombuffer(body, dtype="<i4").reshape(nv, 4).copy(), f["v"].astype(np.int32).copy()


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
