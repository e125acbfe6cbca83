"""mm3dgs_nn_query_index / mm3dgs_mesh_sample_emit_tri / mm3dgs_normal_consistency / mm3dgs_mesh_vertex_normals (csrc/geometry.hip)
through the raw C ABI against the host statement of mm3dgs_slam_amd/geometry.py, byte for byte: the nearest row with ties and duplicates,
the sampler's triangle ids, the dots and the row of eight figures in the kernels' summation order, the fixed-point vertex normals whatever
the order of the triangles; rejected calls; `compare_device(normals=True)` and `mesh.normals` end to end.  Outputs carry PAD sentinel
elements behind them and work buffers lie between guard zones (tests/test_gpu_geometry.py's helpers).  Every test prints its figures
(`NRMERR ...`, pytest -s) before it asserts."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import cull as cl, geometry as geo, mesh as ms, pointcloud as pc
from tests import geometry_cases as gc, mesh_cases, normals_cases as nc
from tests import test_gpu_geometry as g

pytestmark = pytest.mark.gpu
DEV, PAD, SENT = g.DEV, g.PAD, g.SENT
_ptr, _lib, _stream, _dev = g._ptr, g._lib, g._stream, g._dev


def _sentinel(n, width=None):
    return torch.full((n + PAD,) if width is None else (n + PAD, width), SENT, dtype=torch.int32, device=DEV)


# ---- the nearest row ----------------------------------------------------------------------------------------------------------------------
def _query_index(nn, **over):
    """One mm3dgs_nn_query_index on the grid `nn` (tests/test_gpu_geometry.py: NN) has built: (rc, dist int32 bits, row, index uint32)."""
    c = nn.case
    dist, index, row = _sentinel(nn.n_q), _sentinel(nn.n_q), _sentinel(16)
    a = dict(n_q=nn.n_q, q=nn.q, n_ref=nn.n_ref, cell=nn.cell, origin=g._origin(nn.o), gx=nn.dims[0], gy=nn.dims[1], gz=nn.dims[2], cell_start=nn.cell_start,
             sorted=nn.sorted, max_dist=c["max_dist"], threshold=c["threshold"], dist=dist, index=index, row=row, work=nn.qwork)
    a.update(over)
    rc = _lib().mm3dgs_nn_query_index(a["n_q"], _ptr(a["q"]), a["n_ref"], a["cell"], a["origin"], a["gx"], a["gy"], a["gz"], _ptr(a["cell_start"]), _ptr(a["sorted"]),
                                      a["max_dist"], a["threshold"], _ptr(a["dist"]), _ptr(a["index"]), _ptr(a["row"]), _ptr(a["work"]), _stream())
    torch.cuda.synchronize()
    d, i, r = dist.cpu().numpy(), index.cpu().numpy(), row.cpu().numpy()
    if rc == 0:
        assert (d[nn.n_q:] == SENT).all() and (i[nn.n_q:] == SENT).all() and (r[16:] == SENT).all() and g._guards_ok(nn.qbuf), "written behind an output"
    return rc, d[:nn.n_q].copy(), r[:16].view(np.float64).copy(), i[:nn.n_q].view(np.uint32).copy()


@pytest.mark.parametrize("n_ref", nc.N_REF)
@pytest.mark.parametrize("n_q", nc.N_Q)
def test_nn_query_index_against_the_host_statement(n_q, n_ref):
    c = nc.index_case(n_ref, n_q)
    nn = g.NN(c, fill=0xFF)
    assert nn.build() == 0 and nn.query() == 0
    old_dist, old_row = nn.read()[:2]
    rc, dist, row, index = _query_index(nn)
    want_d, want_i, info = geo.nn_index_host(c["query"], c["ref"], c["cell"], c["max_dist"])
    ties = nc.tie_counts(c)
    print(f"NRMERR gpu index {c['name']}: {int((index != want_i).sum())} rows differ from the host's, {int((index == geo.NO_INDEX).sum())} without a row, "
          f"{int((ties > 1).sum())} ties; row {row.tolist()}")
    assert rc == 0 and dist.tobytes() == old_dist.tobytes() and row.tobytes() == old_row.tobytes()
    assert dist.tobytes() == want_d.tobytes() and np.array_equal(index, want_i)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(_query_index(nn)[1:], (dist, row, index)))      # a second call: the same bytes
    # a permuted reference: the permuted rows without a tie, the smallest row with one
    perm = np.random.default_rng(n_q + n_ref).permutation(n_ref)
    pn = g.NN(dict(c, ref=np.ascontiguousarray(c["ref"][perm])), fill=0x00)
    assert pn.build() == 0
    _, pd, prow, pi = _query_index(pn)
    want_p = geo.nn_index_brute_host(c["query"], c["ref"][perm], c["max_dist"])[1]
    found = index != geo.NO_INDEX
    assert pd.tobytes() == dist.tobytes() and prow.tobytes() == row.tobytes() and np.array_equal(pi, want_p) and np.array_equal(pi != geo.NO_INDEX, found)
    single = found & (ties == 1)
    assert np.array_equal(perm[pi[single]], index[single])
    if n_ref == 500:
        assert ties[0] == 8 and index[0] == 10 and pi[0] == np.argsort(perm)[10:18].min()


# ---- the sampler's triangle ids -------------------------------------------------------------------------------------------------------------
def _emit_tri(s, **over):
    rows, tri = _sentinel(s.cap, 4), _sentinel(s.cap)
    a = dict(s._args({}), rows=rows, tri=tri)
    a.update(over)
    rc = _lib().mm3dgs_mesh_sample_emit_tri(a["nv"], _ptr(a["v"]), a["m"], _ptr(a["tris"]), a["density"], a["seed"], _ptr(a["work"]), _ptr(a["rows"]), _ptr(a["tri"]),
                                            a["cap"], _ptr(a["counters"]), _stream())
    torch.cuda.synchronize()
    return rc, rows.cpu().numpy(), tri.cpu().numpy()


@pytest.mark.parametrize("name,density", [("single", 900.0), ("sparse", 9000.0), ("grid", 150.0), ("grid", 300.0), ("grid", 450.0)])
def test_emit_tri_against_the_host_statement(name, density):
    v, tris = {"single": nc.single_triangle, "sparse": nc.sparse_sample_mesh, "grid": nc.grid_mesh}[name]()
    want, wc, f = geo.sample_mesh_host(v, tris, density, 5, full=True)
    total = wc["samples"]
    if name == "grid":      # the totals on both sides of 256 and of 512
        assert {150.0: total < 256, 300.0: 256 < total < 512, 450.0: total > 512}[density], total
    if name == "sparse":
        assert wc["degenerate"] >= 40 and (f["counts"] == 0).sum() > 100 and total > 256
    s = g.Sampler(v, tris, density, 5, total, 0xFF)
    assert s.plan() == 0 and s.emit() == 0
    rows, c = s.read()
    rc, rows2, tri = _emit_tri(s)
    c2 = s.counters.cpu().numpy()[:8]
    print(f"NRMERR gpu emit_tri {name} at {density}: {total} samples of {len(tris)} triangles ({wc['degenerate']} rejected), counters {c2.tolist()}")
    assert rc == 0 and rows2[:total].tobytes() == rows.tobytes() == want.tobytes() and c2.tobytes() == c.tobytes()
    assert np.array_equal(tri[:total], f["tri"]) and (tri[total:] == SENT).all() and (rows2[total:] == SENT).all() and g._guards_ok(s.buf)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(_emit_tri(s)[1:], (rows2, tri)))
    # the python surface
    drows, dc, dtri = geo.sample_mesh_device(v, tris, density, 5, device=DEV, want_tri=True)
    assert drows.cpu().numpy().tobytes() == want.tobytes() and np.array_equal(dtri.cpu().numpy(), f["tri"]) and dc["samples"] == total


# ---- the consistency call -------------------------------------------------------------------------------------------------------------------
def _consistency(tri_q, index, tri_r, mesh_q, mesh_r):
    n = len(tri_q)
    dot, row = _sentinel(n), _sentinel(16)
    as_i32 = lambda a: _dev(np.asarray(a, dtype=np.uint32).view(np.int32))
    geo.normal_consistency_device(as_i32(tri_q), as_i32(index), as_i32(tri_r), tuple(_dev(a) for a in mesh_q), tuple(_dev(a) for a in mesh_r),
                                  dot=dot[:n].view(torch.float32), row=row[:16].view(torch.float64), device=DEV)
    torch.cuda.synchronize()
    d, r = dot.cpu().numpy(), row.cpu().numpy()
    assert (d[n:] == SENT).all() and (r[16:] == SENT).all(), "written behind an output"
    return d[:n].view(np.float32).copy(), r[:16].view(np.float64).copy()


def _direction(name, est, ref, density, max_dist=0.2):
    """One direction on host-made inputs: the kernel's dots and row against normal_dots_host / normal_row in the kernels' order."""
    rows_e, _, fe = geo.sample_mesh_host(*est, density, 0, full=True)
    rows_r, _, fr = geo.sample_mesh_host(*ref, density, 0, full=True)
    index = geo.nn_index_host(rows_e, rows_r, 0.05, max_dist)[1]
    want, none = geo.normal_dots_host(fe["tri"], index, fr["tri"], est, ref)
    wrow = geo.normal_row(want, none, sum_order="kernel")
    dot, row = _consistency(fe["tri"], index, fr["tri"], est, ref)
    again = _consistency(fe["tri"], index, fr["tri"], est, ref)
    print(f"NRMERR gpu consistency {name}: {len(dot)} queries, {int((dot.view(np.int32) != want.view(np.int32)).sum())} dots differ from the host's; row {row.tolist()}; "
          f"host {wrow.tolist()}")
    assert dot.tobytes() == want.tobytes() and row.tobytes() == wrow.tobytes() and again[0].tobytes() == dot.tobytes() and again[1].tobytes() == row.tobytes()
    return dot, row


def test_consistency_against_the_host_statement():
    sphere, flat = nc.icosphere(2), gc.square_mesh()
    dot, row = _direction("sphere on itself", sphere, sphere, 2000.0)
    assert (dot == 1).all() and row[:4].tolist() == [len(dot), 1.0, 1.0, 1.0] and len(dot) > 1024
    dot, row = _direction("flat, flipped winding", flat, nc.flipped(flat), 2000.0)
    assert (dot == -1).all() and row[1:4].tolist() == [1.0, -1.0, 1.0]
    floor, wall = nc.floor_and_wall()
    dot, row = _direction("floor / wall", floor, wall, 500.0, max_dist=0.25)
    assert 0 < row[0] < len(dot) and (dot[~np.isnan(dot)] == 0).all() and row[5] == np.isnan(dot).sum() and row[1:4].tolist() == [0, 0, 0]
    dot, row = _direction("sphere shifted by 1 cm", sphere, nc.shifted(sphere, (0.01, 0, 0)), 2000.0)
    assert row[0] == len(dot) and 0.97 < row[1] < 1.0 and row[3] > 0.8
    dot, row = _direction("shifted sphere back", nc.shifted(sphere, (0.01, 0, 0)), sphere, 2000.0)
    assert row[0] == len(dot) and 0.97 < row[1] < 1.0


def test_consistency_ids_out_of_range():
    mesh = nc.rejecting_mesh()
    m = len(mesh[1])
    rng = np.random.default_rng(5)
    n = 700
    tri_q = rng.choice(np.array([0, 7, 1, 5, m, m + 1, 0x7fffffff, 0xfffffffe], dtype=np.uint32), n)
    tri_r = np.array([0, 7, 6, m + 3, 0xffffffff, 7, 0], dtype=np.uint32)
    index = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7, 1 << 20, 0xfffffffe, 0xffffffff], dtype=np.uint32), n)
    want, none = geo.normal_dots_host(tri_q, index, tri_r, mesh, mesh)
    wrow = geo.normal_row(want, none, sum_order="kernel")
    dot, row = _consistency(tri_q, index, tri_r, mesh, mesh)
    print(f"NRMERR gpu consistency ids: row {row.tolist()}; host {wrow.tolist()}")
    assert dot.tobytes() == want.tobytes() and row.tobytes() == wrow.tobytes()
    assert row[0] > 0 and row[5] > 0 and row[6] > 0 and row[0] + row[5] + row[6] == n and set(np.unique(dot[~np.isnan(dot)]).tolist()) == {0.0, 1.0}


# ---- vertex normals ---------------------------------------------------------------------------------------------------------------------------
def _vertex_normals(v, tris, fill=0xFF, over=None):
    nv, m = len(v), len(tris)
    normals = _sentinel(3 * nv)
    counters = torch.full((8 + PAD,), -7, dtype=torch.int64, device=DEV)
    nbytes = int(_lib().mm3dgs_mesh_vertex_normals_work_bytes(nv))
    assert nbytes >= 28 * nv and nbytes % 8 == 0
    buf, work = g._guarded(nbytes, fill)
    a = dict(nv=nv, v=_dev(v), m=m, tris=_dev(tris), normals=normals, work=work, counters=counters)
    a.update(over or {})
    rc = _lib().mm3dgs_mesh_vertex_normals(a["nv"], _ptr(a["v"]), a["m"], _ptr(a["tris"]), _ptr(a["normals"]), _ptr(a["work"]), _ptr(a["counters"]), _stream())
    torch.cuda.synchronize()
    n, c = normals.cpu().numpy(), counters.cpu().numpy()
    if rc == 0:
        assert (n[3 * nv:] == SENT).all() and (c[8:] == -7).all() and g._guards_ok(buf), "written behind an output"
    return rc, n[:3 * nv].view(np.float32).reshape(nv, 3).copy(), c[:8].copy(), (n, c)


@pytest.mark.parametrize("name", ["one vertex", "octahedron", "grid 17 x 17", "fan of 1000", "rejecting"])
def test_vertex_normals_against_the_host_statement(name):
    v, tris = {"one vertex": lambda: (gc.rows_of([[1, 2, 3]]), np.zeros((1, 3), dtype=np.int32)), "octahedron": nc.octahedron, "grid 17 x 17": nc.grid_mesh,
               "fan of 1000": nc.fan_mesh, "rejecting": nc.rejecting_mesh}[name]()
    want, wc = geo.vertex_normals_host(v, tris)
    rc, n, c, _ = _vertex_normals(v, tris)
    print(f"NRMERR gpu vertex normals {name}: {len(v)} vertices, {len(tris)} triangles, counters {c.tolist()} (host {wc}); "
          f"{int((n.view(np.int32) != want.view(np.int32)).sum())} components differ from the host's")
    assert rc == 0 and n.tobytes() == want.tobytes() and c.tolist() == [wc["vertices"], wc["without_normal"], wc["rejected_triangles"], 0, 0, 0, 0, 0]
    shuffled = tris[np.random.default_rng(1).permutation(len(tris))]
    assert _vertex_normals(v, shuffled, fill=0x00)[1].tobytes() == n.tobytes() and _vertex_normals(v, tris)[1].tobytes() == n.tobytes()
    if name == "octahedron":
        assert np.array_equal(n, pc.rows_xyz(v))
    dn, dc = geo.vertex_normals(_dev(v), _dev(tris), DEV)
    assert dn.tobytes() == want.tobytes() and dc == wc


# ---- rejected calls -----------------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_return_minus_one_and_write_nothing():
    lib = _lib()
    nan, inf = float("nan"), float("inf")
    nn = g.NN(nc.index_case(500, 257))
    assert nn.build() == 0
    before = nn.snapshot()
    bad = {"n_q = 0": dict(n_q=0), "n_q > 2^30": dict(n_q=(1 << 30) + 1), "n_ref = 0": dict(n_ref=0), "gz = 0": dict(gz=0), "more than 2^26 cells": dict(gx=512, gy=512, gz=257),
           "cell NaN": dict(cell=nan), "max_dist = 0": dict(max_dist=0.0), "max_dist < 0": dict(max_dist=-1.0), "max_dist NaN": dict(max_dist=nan), "max_dist inf": dict(max_dist=inf),
           "more than 2^20 rings": dict(cell=1e-9), "threshold < 0": dict(threshold=-0.5), "NULL origin": dict(origin=None), "NULL q": dict(q=None),
           "NULL cell_start": dict(cell_start=None), "NULL sorted": dict(sorted=None), "NULL dist": dict(dist=None), "NULL index": dict(index=None), "NULL row": dict(row=None),
           "NULL work": dict(work=None), "misaligned q": dict(q=nn.q.data_ptr() + 8), "misaligned work": dict(work=nn.qwork + 4),
           "misaligned index": dict(index=nn.dist.data_ptr() + 2)}
    for what, over in bad.items():
        rc, d, r, i = _query_index(nn, **over)
        assert rc == -1 and lib.mm3dgs_last_error(), what
        if "dist" not in over:
            assert (d.view(np.int32) == SENT).all(), what
        if "index" not in over:
            assert (i.view(np.int32) == SENT).all(), what
    assert all(nn.snapshot()[k].tobytes() == a.tobytes() for k, a in before.items())
    v, tris = gc.random_mesh(257, seed=1)
    s = g.Sampler(v, tris, 150.0, 11, 4096)
    assert s.plan() == 0
    bad = {"m = 0": dict(m=0), "m > 2^30": dict(m=(1 << 30) + 1), "n_vertices = 0": dict(nv=0), "density NaN": dict(density=nan), "NULL vrows": dict(v=None),
           "NULL triangles": dict(tris=None), "NULL work": dict(work=None), "NULL counters": dict(counters=None), "NULL rows": dict(rows=None), "NULL tri_out": dict(tri=None),
           "cap > 2^31": dict(cap=(1 << 31) + 1), "misaligned tri_out": dict(tri=s.rows.data_ptr() + 2), "misaligned rows": dict(rows=s.rows.data_ptr() + 8)}
    for what, over in bad.items():
        rc, rows, tri = _emit_tri(s, **over)
        assert rc == -1 and lib.mm3dgs_last_error() and (rows == SENT).all() and (tri == SENT).all(), what
    # the consistency call
    mesh = tuple(_dev(a) for a in nc.octahedron())
    ids = _dev(np.zeros(16, dtype=np.int32))
    out, row = _sentinel(16), _sentinel(16)
    work = torch.zeros(int(lib.mm3dgs_normal_consistency_work_bytes(16)) // 8, dtype=torch.int64, device=DEV)
    good = dict(n_q=16, tri_q=ids, index=ids, n_r=16, tri_r=ids, nvq=6, vq=mesh[0], mq=8, fq=mesh[1], nvr=6, vr=mesh[0], mr=8, fr=mesh[1], dot=out, row=row, work=work)
    call = lambda a: lib.mm3dgs_normal_consistency(a["n_q"], _ptr(a["tri_q"]), _ptr(a["index"]), a["n_r"], _ptr(a["tri_r"]), a["nvq"], _ptr(a["vq"]), a["mq"], _ptr(a["fq"]), a["nvr"],
                                                   _ptr(a["vr"]), a["mr"], _ptr(a["fr"]), _ptr(a["dot"]), _ptr(a["row"]), _ptr(a["work"]), _stream())
    bad = [dict(n_q=0), dict(n_q=(1 << 30) + 1), dict(n_r=0), dict(n_r=(1 << 30) + 1), dict(mq=0), dict(mr=(1 << 30) + 1), dict(nvq=0), dict(nvr=1 << 31)]
    bad += [{k: None} for k in ("tri_q", "index", "tri_r", "vq", "fq", "vr", "fr", "dot", "row", "work")]
    bad += [dict(vq=mesh[0].data_ptr() + 8), dict(row=row.data_ptr() + 4), dict(work=work.data_ptr() + 4), dict(dot=out.data_ptr() + 2), dict(tri_r=ids.data_ptr() + 1)]
    for over in bad:
        assert call(dict(good, **over)) == -1 and lib.mm3dgs_last_error(), over
    torch.cuda.synchronize()
    assert (out == SENT).all() and (row == SENT).all() and not work.any()
    assert call(good) == 0
    torch.cuda.synchronize()
    assert (out[:16].view(torch.float32) == 1).all()
    # vertex normals
    v, tris = nc.octahedron()
    dv = _dev(v)
    for over in (dict(nv=0), dict(nv=1 << 31), dict(m=0), dict(m=(1 << 30) + 1), dict(v=None), dict(tris=None), dict(normals=None), dict(work=None), dict(counters=None),
                 dict(v=dv.data_ptr() + 8), dict(work=dv.data_ptr() + 4), dict(counters=dv.data_ptr() + 4), dict(normals=dv.data_ptr() + 2)):
        rc, _, _, (n, c) = _vertex_normals(v, tris, over=over)
        assert rc == -1 and lib.mm3dgs_last_error(), over
        assert ("normals" in over or (n == SENT).all()) and ("counters" in over or (c == -7).all()), over
    assert int(lib.mm3dgs_mesh_vertex_normals_work_bytes(0)) == 0 and int(lib.mm3dgs_normal_consistency_work_bytes(0)) == 0


def test_pair_fault_texts():
    nn = g.NN(nc.index_case(500, 257))
    assert nn.build() == 0
    faults = g.pair_fault_texts("nn_query_index", index=True) + [(dict(index=None), "nn_query_index: NULL argument (q_rows, cell_start, sorted, dist_out, index_out, row and work are required)"),
                                                                  (dict(index=nn.dist.data_ptr() + 2), "nn_query_index: cell_start, dist_out and index_out must be 4-byte aligned")]
    for over, text in faults:
        over = dict(dist=nn.dist.data_ptr() + 2) if over == "misaligned dist" else over
        assert _query_index(nn, **over)[0] == -1 and _lib().mm3dgs_last_error().decode() == text, over
    s = g.Sampler(*gc.random_mesh(257, seed=1), 150.0, 11, 4096)
    assert s.plan() == 0
    faults = g.pair_fault_texts("mesh_sample_emit_tri", tri=True) + [(dict(tri=None), "mesh_sample_emit_tri: rows or tri_out is NULL with a cap above 0"),
                                                                     (dict(tri=s.rows.data_ptr() + 2), "mesh_sample_emit_tri: tri_out must be 4-byte aligned")]
    for over, text in faults:
        over = dict(rows=s.rows.data_ptr() + 8) if over == "misaligned rows" else over
        assert _emit_tri(s, **over)[0] == -1 and _lib().mm3dgs_last_error().decode() == text, over


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_scene():
    """The sphere of tests/mesh_cases.py in a 17^3 lattice, meshed on the host, as the estimate; the same mesh 1 cm along x as the reference;
    a view whose frustum cuts through both."""
    vol = mesh_cases.analytic_volume("sphere", (17, 17, 17))
    rows, tris = ms.mesh_host(vol["tsdf_w"], vol["rgb_w"], vol["origin"], vol["voxel"])[:2]
    centre = mesh_cases.ORIGIN + mesh_cases.VOXEL * (8 + mesh_cases.OFF)
    pose = np.array([1, 0, 0, 0, -centre[0], 1.0 - centre[1], 2.5 - centre[2]], dtype=np.float32)      # the centre at (0, 1, 2.5): on the image's lower edge
    spec = cl.spec([(None, pose)], 48, 64, {"fx": 60.0, "fy": 60.0, "cx": 32.0, "cy": 24.0}, near=0.1, far=5.0, eps=0.05, min_views=1, depth_max=8.0)
    return (rows, tris), nc.shifted((rows, tris), (0.01, 0.0, 0.0)), spec


@pytest.mark.parametrize("culled", [False, True])
def test_compare_device_with_normals_equals_the_host_path(sphere_scene, culled):
    est, ref, spec = sphere_scene
    kw = dict(threshold=0.05, max_dist=0.5, density=3000.0, seed=2, **({"cull": spec} if culled else {}))
    host = geo.compare(est, ref, device="cpu", sum_order="kernel", normals=True, **kw)
    dev = geo.compare(est, ref, device=DEV, normals=True, **kw)
    plain = geo.compare(est, ref, device=DEV, **kw)
    print(f"NRMERR gpu compare (culled {culled}): {dev['n_estimate']} / {dev['n_reference']} points; normals {json.dumps(dev['normals'])}; device table "
          f"{dev['normal_table'].tolist()}; host table {host['normal_table'].tolist()}")
    if culled:
        assert dev["cull"] == host["cull"] and 0 < dev["cull"]["estimate"]["kept"] < dev["cull"]["estimate"]["rows"]
    assert dev["normal_table"].tobytes() == host["normal_table"].tobytes() and dev["normals"] == host["normals"] and dev["normal_table"][0, 0] > 256
    assert dev["table"].tobytes() == plain["table"].tobytes() == host["table"].tobytes() and "normals" not in plain
    for k in ("dot_estimate", "dot_reference", "dist_estimate", "dist_reference"):
        assert dev[k].is_cuda and dev[k].cpu().numpy().tobytes() == host[k].tobytes(), k
    for k in ("nearest_estimate", "nearest_reference"):
        assert dev[k].cpu().numpy().view(np.uint32).tobytes() == host[k].tobytes(), k
    assert plain["dist_estimate"].cpu().numpy().tobytes() == host["dist_estimate"].tobytes()
    assert 0.9 < dev["normals"]["normal_consistency"] <= 1.0


@pytest.fixture(scope="module")
def native_run(tmp_path_factory):
    return g._run(tmp_path_factory.mktemp("normals_native"), False)[0]


@pytest.mark.parametrize("volume", ["dense", "sparse"])
def test_native_run_writes_the_host_paths_normals(native_run, tmp_path, volume):
    slam = native_run
    slam.cfg["mesh"] = dict(g.MESH, volume=volume)
    off = slam.export_mesh(path=str(tmp_path / "off"))
    slam.cfg["mesh"] = dict(g.MESH, volume=volume, normals=True)
    on = slam.export_mesh(path=str(tmp_path / "on"))
    v0, t0 = ms.read_mesh_ply(off["mesh"])
    v1, t1, n1 = ms.read_mesh_ply_normals(on["mesh"])
    want, wc = geo.vertex_normals_host(v1, t1)
    print(f"NRMERR gpu run ({volume}): {len(v1)} vertices, {len(t1)} triangles, counters {on['normals']}")
    assert len(v1) > 100 and np.array_equal(v0, v1) and np.array_equal(t0, t1) and "normals" not in off
    assert on["normals"] == wc and wc["without_normal"] < len(v1)
    host_file = ms.write_mesh_ply(str(tmp_path / "host.ply"), v1, t1, want)      # the host path's file for the same mesh
    assert open(on["mesh"], "rb").read() == open(host_file, "rb").read()
    plain_file = ms.write_mesh_ply(str(tmp_path / "plain.ply"), v1, t1)
    assert open(off["mesh"], "rb").read() == open(plain_file, "rb").read()
