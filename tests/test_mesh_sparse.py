"""The mesh export's voxel-block volume on the host (mesh.volume: sparse; mm3dgs_slam_amd/mesh.py: reserve_host, HostSparseTsdfVolume,
mesh_blocks_host, the `first` offset of integrate_host / mesh_host): the reservation covers the truncation band, the sparse mesh is the
dense mesh of the masked lattice in the documented order, negative block coordinates, the config keys and the export of a `device: cpu`
run.  Every test prints its figures (`MESHERR ...`, pytest -s) before it asserts."""
import os
import random

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import mesh as ms
from tests import mesh_cases as cases
from tests import mesh_sparse_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _block_order(idx, first, dims):
    """Sort key of bounding-lattice samples in the documented order, without mesh.pool_index: (block key, raster index inside the block)."""
    nx, ny, nz = dims
    q = np.stack([idx % nx, (idx // nx) % ny, idx // (nx * ny)], 1) + np.asarray(first, dtype=np.int64)[None, :]
    key = ms.block_keys(q // 8)
    local = (q[:, 2] % 8) * 64 + (q[:, 1] % 8) * 8 + q[:, 0] % 8
    return key, local


def _reordered(tsdf_w, rgb_w, anchor, voxel, first, dims):
    """mesh_host of a bounding lattice, brought into the documented order by a lexsort on (block key, local index, d) -- the test's own route."""
    rows, tris, m, vq, tq = ms.mesh_host(tsdf_w, rgb_w, anchor, voxel, first=first, where=True)
    kv, lv = _block_order(vq, first, dims)
    perm = np.lexsort((np.arange(len(vq)), lv, kv))
    inv = np.empty(len(perm), dtype=np.int64)
    inv[perm] = np.arange(len(perm))
    kt, lt = _block_order(tq, first, dims)
    order = np.lexsort((np.arange(len(tq)), lt, kt))
    return rows[perm], inv[tris.astype(np.int64)][order].astype(np.int32).reshape(-1, 3)


# ---- 1. coverage ---------------------------------------------------------------------------------------------------------------------
COVER = [((33, 33, 19), (48, 64), p, n) for p, n in (("all", 2), ("checker", 3), ("planted", 2), ("sil_edge", 2), ("depth_max_edge", 3))] + [((17, 9, 6), (17, 33), "all", 3)]


@pytest.mark.parametrize("dims,hw,pattern,n_views", COVER)
def test_reservation_covers_the_band_of_scattered_depth_views(dims, hw, pattern, n_views):
    case = cases.integrate_case(dims, hw[0], hw[1], pattern, n_views)
    nx, ny, nz = dims
    band = pairs = valid = 0
    for v in case["views"]:
        keys, info = ms.reserve_host(v["depth"], v["sil"], v["pose"], **v["cam"], voxel=case["voxel"], trunc=case["trunc"], anchor=case["origin"], sil_min=v["sil_min"],
                                     depth_max=v["depth_max"])
        tw, rw = ms.empty_volume(nx, ny, nz)
        _, g = ms.integrate_host(tw, rw, v["color"], v["depth"], v["sil"], v["pose"], **v["cam"], origin=case["origin"], voxel=case["voxel"], trunc=case["trunc"],
                                 sil_min=v["sil_min"], depth_max=v["depth_max"], full=True)
        k, j, i = np.nonzero(g["col"])
        got = ms.block_keys(np.stack([i // 8, j // 8, k // 8], 1))      # anchor = the lattice's origin: sample (i, j, k) has the lattice index (i, j, k)
        missing = int((~np.isin(got, keys)).sum())
        band += len(got); pairs += info["pairs"]; valid += info["valid"]
        assert missing == 0, f"{missing} of {len(got)} band samples outside the reserved blocks"
        assert info["out_of_range"] == 0
    print(f"MESHERR sparse coverage {dims} {hw} {pattern} x{n_views}: 0 of {band} band samples outside the reserved blocks; {pairs / max(valid, 1):.2f} pairs per valid pixel")
    assert band > 0


# ---- 2. sphere scenes ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spheres():
    """The two sphere scenes once: (case, frozen and integrated HostSparseTsdfVolume)."""
    out = {}
    for name, voxel, wall in (("sphere", 0.02, False), ("sphere+wall", 0.03, True)):
        case = sc.sphere_case(voxel, wall)
        out[name] = (case, sc.host_volume(case))
    return out


@pytest.mark.parametrize("name", ["sphere", "sphere+wall"])
def test_sphere_scene_gives_the_dense_mesh_and_its_band_is_covered(spheres, name):
    case, vol = spheres[name]
    rows, tris, c = vol.extract()
    tw, rw, cd = sc.dense_over(case, vol.first, vol.dims)
    want_rows, want_tris, _ = ms.mesh_host(tw, rw, case["anchor"], case["voxel"], first=vol.first)
    box = int(np.prod(np.asarray(vol.dims) // 8))
    a, b = sc.mesh_sets(rows, tris), sc.mesh_sets(want_rows, want_tris)
    print(f"MESHERR sparse {name}: {c['blocks']} blocks of a {box}-block box ({c['pairs'] / c['reserved_pixels']:.2f} pairs per pixel); sparse {len(rows)} / {len(tris)}, "
          f"dense {len(want_rows)} / {len(want_tris)} vertices / triangles; updates {c['dist_updates']} / {c['colour_updates']} (dense {cd[1]} / {cd[2]})")
    assert c["blocks"] < box and len(rows) > 1000
    assert a[2] and b[2]      # no vertex twice
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert c["colour_updates"] == cd[2] and c["dist_updates"] <= cd[1]      # the band is covered: every colour update falls in a reserved block
    # coverage, sample by sample
    tw, rw = ms.empty_volume(*vol.dims)
    for v in case["views"]:
        _, g = ms.integrate_host(tw, rw, v["color"], v["depth"], v["sil"], v["pose"], **v["cam"], origin=case["anchor"], voxel=case["voxel"], trunc=case["trunc"], full=True,
                                 first=vol.first)
        assert not (g["col"] & ~vol.reserved).any()
    if name == "sphere":
        assert (c["blocks"], box, len(rows), len(tris)) == (193, 280, 9550, 18224)
    else:
        assert 2 * c["blocks"] > 1024      # more than 1024 per-256 counts: the second round of the scan


# ---- 3. scattered depth: the masked dense mesh, in the documented order ---------------------------------------------------------------
@pytest.mark.parametrize("hw,pattern,n_views", [((17, 33), "all", 1), ((48, 64), "checker", 3), ((48, 64), "planted", 2)])
def test_scattered_depth_views_give_the_masked_dense_mesh_in_block_order(hw, pattern, n_views):
    case = sc.scattered_case(hw, pattern, n_views)
    vol = sc.host_volume(case)
    rows, tris, c = vol.extract()
    tw, rw, cd = sc.dense_over(case, vol.first, vol.dims, mask=vol.reserved)
    want_rows, want_tris = _reordered(tw, rw, case["anchor"], case["voxel"], vol.first, vol.dims)
    full = sc.dense_over(case, vol.first, vol.dims)
    dense = ms.mesh_host(full[0], full[1], case["anchor"], case["voxel"], first=vol.first)
    print(f"MESHERR sparse scattered {hw} {pattern} x{n_views}: {c['blocks']} blocks, {len(rows)} vertices, {len(tris)} triangles (unmasked dense: {len(dense[0])} / {len(dense[1])})")
    assert len(tris) > 0
    assert rows.tobytes() == want_rows.tobytes() and tris.tobytes() == want_tris.tobytes()
    assert [c["views"], c["dist_updates"], c["colour_updates"]] == cd
    assert len(dense[1]) >= len(tris)      # the sparse mesh is the dense one minus the cubes that touch an unreserved block
    ptw, prw = vol.pool()
    again = ms.mesh_blocks_host(vol.keys, ptw, prw, case["anchor"], case["voxel"])
    assert again[0].tobytes() == rows.tobytes() and again[1].tobytes() == tris.tobytes()


# ---- 4. analytic volumes as blocks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sphere", "torus"])
def test_analytic_volume_as_blocks(kind):
    a = sc.analytic_blocks(kind)
    ptw, prw = sc.to_pool(a["tsdf_w"], a["rgb_w"], a["blocks"], a["first"], a["dims"])
    rows, tris, m = ms.mesh_blocks_host(a["keys"], ptw, prw, a["origin"], a["voxel"])
    vol = cases.analytic_volume(kind, (65, 65, 65))
    want = ms.mesh_host(vol["tsdf_w"], vol["rgb_w"], vol["origin"], vol["voxel"])
    topo = ms.mesh_topology(len(rows), tris)
    print(f"MESHERR sparse analytic {kind}: {len(a['keys'])} blocks, {len(rows)} vertices, {len(tris)} triangles, {topo}")
    sa, sb = sc.mesh_sets(rows, tris), sc.mesh_sets(want[0], want[1])
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]) and m.tolist() == want[2].tolist()
    assert topo["closed"] and topo["euler"] == (2 if kind == "sphere" else 0)
    # a third of the blocks removed: the mesh of the masked volume, in the documented order
    b = sc.analytic_blocks(kind, drop_third=True)
    ptw, prw = sc.to_pool(b["tsdf_w"], b["rgb_w"], b["blocks"], b["first"], b["dims"])
    rows, tris, _ = ms.mesh_blocks_host(b["keys"], ptw, prw, b["origin"], b["voxel"])
    want_rows, want_tris = _reordered(b["tsdf_w"], b["rgb_w"], b["origin"], b["voxel"], b["first"], b["dims"])
    print(f"MESHERR sparse analytic {kind} minus a third of the blocks: {len(b['keys'])} blocks, {len(rows)} vertices, {len(tris)} triangles")
    assert 0 < len(tris) < len(want[1])
    assert rows.tobytes() == want_rows.tobytes() and tris.tobytes() == want_tris.tobytes()
    assert not ms.mesh_topology(len(rows), tris)["closed"]


# ---- 5. the `first` offset -----------------------------------------------------------------------------------------------------------
def test_first_offset_of_the_host_statement():
    dims = (17, 9, 6)
    case = cases.integrate_case(dims, 17, 33, "all", 2)
    outs = []
    for kw in ({}, {"first": (0, 0, 0)}):
        tw, rw = ms.empty_volume(*dims)
        n = [ms.integrate_host(tw, rw, v["color"], v["depth"], v["sil"], v["pose"], **v["cam"], origin=case["origin"], voxel=case["voxel"], trunc=case["trunc"], **kw)
             for v in case["views"]]
        mesh = ms.mesh_host(tw, rw, case["origin"], case["voxel"], **kw)
        outs.append((tw.tobytes(), rw.tobytes(), n, mesh[0].tobytes(), mesh[1].tobytes(), mesh[2].tobytes()))
    assert outs[0] == outs[1]
    # the lattice shifted by `first` with the origin moved the other way: the same sample positions up to roundoff, the same index sets
    first = np.array([-8, 8, -16])
    moved = case["origin"] - case["voxel"] * first
    tw2, rw2 = ms.empty_volume(*dims)
    masks, masks2 = [], []
    tw, rw = ms.empty_volume(*dims)
    for v in case["views"]:
        a = dict(sil_min=v["sil_min"], depth_max=v["depth_max"], voxel=case["voxel"], trunc=case["trunc"], full=True)
        masks.append(ms.integrate_host(tw, rw, v["color"], v["depth"], v["sil"], v["pose"], **v["cam"], origin=case["origin"], **a)[1])
        masks2.append(ms.integrate_host(tw2, rw2, v["color"], v["depth"], v["sil"], v["pose"], **v["cam"], origin=moved, first=first, **a)[1])
    m1 = ms.mesh_host(tw, rw, case["origin"], case["voxel"], full=True)
    m2 = ms.mesh_host(tw2, rw2, moved, case["voxel"], full=True, first=first)
    dp = float(np.abs(m1[3] - m2[3]).max()) if len(m1[3]) else 0.0
    print(f"MESHERR first offset: {len(m1[0])} vertices, {len(m1[1])} triangles; max position difference {dp:.3e}")
    for g, h in zip(masks, masks2):
        assert np.array_equal(g["upd"], h["upd"]) and np.array_equal(g["col"], h["col"])
    assert np.array_equal(m1[1], m2[1]) and len(m1[0]) == len(m2[0]) and dp <= 1e-12 and len(m1[1]) > 0


# ---- 6. negative block coordinates ---------------------------------------------------------------------------------------------------
def test_an_anchor_astride_zero_gives_negative_block_coordinates(spheres):
    ref_case, ref_vol = spheres["sphere"]
    middle = ref_vol.origin + 0.5 * ref_case["voxel"] * np.asarray(ref_vol.dims)
    anchor = middle + np.array([0.0031, -0.0042, 0.0057])      # the scene's middle: blocks on both sides of zero on every axis
    case = sc.sphere_case(0.02, False, anchor=anchor)
    vol = sc.host_volume(case)
    rows, tris, c = vol.extract()
    b = ms.key_blocks(vol.keys)
    print(f"MESHERR sparse negative blocks: {c['blocks']} blocks, coordinates {b.min(0).tolist()} .. {b.max(0).tolist()}, {len(rows)} vertices, {len(tris)} triangles")
    assert bool((b.min(0) < 0).all()) and bool((b.max(0) >= 0).all())
    assert np.array_equal(ms.key_blocks(ms.block_keys(b)), b) and bool((np.diff(vol.keys) > 0).all())
    order = np.lexsort((b[:, 0], b[:, 1], b[:, 2]))      # ascending keys = z-major raster order of the signed coordinates
    assert np.array_equal(order, np.arange(len(b)))
    tw, rw, _ = sc.dense_over(case, vol.first, vol.dims)
    want = ms.mesh_host(tw, rw, anchor, case["voxel"], first=vol.first)
    sa, sb = sc.mesh_sets(rows, tris), sc.mesh_sets(want[0], want[1])
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]) and len(tris) > 1000
    tw, rw, _ = sc.dense_over(case, vol.first, vol.dims, mask=vol.reserved)
    want_rows, want_tris = _reordered(tw, rw, anchor, case["voxel"], vol.first, vol.dims)
    assert rows.tobytes() == want_rows.tobytes() and tris.tobytes() == want_tris.tobytes()
    assert vol.first.min() < 0 and np.allclose(vol.origin, anchor + case["voxel"] * vol.first)


def test_reservation_limits():
    case = sc.sphere_case(0.02, False, n_views=1)
    v = case["views"][0]
    a = dict(voxel=0.02, sil_min=v["sil_min"], depth_max=v["depth_max"])
    with pytest.raises(ValueError, match="16 voxel"):
        ms.reserve_host(v["depth"], v["sil"], v["pose"], **v["cam"], trunc=0.33, **a)
    keys, info = ms.reserve_host(v["depth"], v["sil"], v["pose"], **v["cam"], trunc=0.32, **a)      # exactly 16 voxel
    assert len(keys) > 0 and info["out_of_range"] == 0
    # an anchor 2^21 blocks away: every pixel is out of range and counted, none reserved
    far, info = ms.reserve_host(v["depth"], v["sil"], v["pose"], **v["cam"], trunc=0.08, anchor=(0.02 * 8 * (1 << 21), 0, 0), **a)
    assert len(far) == 0 and info["out_of_range"] == info["valid"] > 0 and info["pairs"] == 0
    # mesh.bounds: only the blocks that intersect the box
    b = ms.key_blocks(keys)
    lo = 0.02 * 8 * (b.min(0) + 1) + 0.001
    clip = ms.block_clip(np.concatenate([lo, lo + 0.02 * 8 * 2]), (0, 0, 0), 0.02)
    inside, _ = ms.reserve_host(v["depth"], v["sil"], v["pose"], **v["cam"], trunc=0.32, clip=clip, **a)
    bi = ms.key_blocks(inside)
    assert 0 < len(inside) < len(keys) and bool(np.isin(inside, keys).all()) and bool((bi >= clip[:3]).all()) and bool((bi <= clip[3:]).all())
    want = keys[((b >= clip[:3]) & (b <= clip[3:])).all(1)]
    assert np.array_equal(inside, want)
    vol = ms.HostSparseTsdfVolume(0.02, 0.08, *v["depth"].shape, v["cam"], max_blocks=8)
    vol.reserve(v["depth"], v["sil"], v["pose"])
    with pytest.raises(ValueError, match=r"mesh\.max_blocks = 8.*mesh\.voxel"):
        vol.freeze()
    empty = ms.HostSparseTsdfVolume(0.02, 0.08, *v["depth"].shape, v["cam"])
    empty.reserve(np.zeros_like(v["depth"]), None, v["pose"])
    with pytest.raises(ValueError, match="no view has a valid pixel"):
        empty.freeze()


# ---- 7. options and the export of a `device: cpu` run -----------------------------------------------------------------------------------
def test_options_validate_the_two_keys():
    from mm3dgs_slam_amd.config import MESH_VOLUME, default_config
    from mm3dgs_slam_amd.export import options
    assert MESH_VOLUME == {"volume": "dense", "max_blocks": 1 << 18}
    cfg = default_config()
    opt = options(cfg, "mesh")
    assert opt["volume"] == "dense" and opt["max_blocks"] == 1 << 18
    cfg["mesh"] = dict(cfg["mesh"], volume="Sparse", max_blocks=1 << 21)
    assert options(cfg, "mesh")["volume"] == "sparse" and options(cfg, "mesh")["max_blocks"] == 1 << 21
    for bad, match in ((dict(volume="octree"), r"mesh\.volume"), (dict(max_blocks=0), r"mesh\.max_blocks"), (dict(max_blocks=(1 << 21) + 1), r"mesh\.max_blocks"),
                       (dict(max_blocks=2.5), r"mesh\.max_blocks"), (dict(max_blocks=True), r"mesh\.max_blocks"), (dict(volume="sparse", trunc=0.33), r"mesh\.trunc")):
        cfg["mesh"] = dict(default_config()["mesh"], **bad)
        with pytest.raises(ValueError, match=match):
            options(cfg, "mesh")
    cfg["mesh"] = dict(default_config()["mesh"], volume="dense", trunc=0.33)      # the dense volume has no such bound
    assert options(cfg, "mesh")["trunc"] == 0.33
    cfg["mesh"] = dict(default_config()["mesh"], volume="sparse", trunc=0.32)
    assert options(cfg, "mesh")["trunc"] == 0.32


def test_cabi_declares_and_binds_the_block_symbols():
    import ctypes as C
    import re
    from mm3dgs_slam_amd import _lib
    h = open(os.path.join(ROOT, "include", "mm3dgs.h")).read()
    names = ("mm3dgs_tsdf_blocks_table_bytes", "mm3dgs_tsdf_blocks_reset", "mm3dgs_tsdf_blocks_reserve", "mm3dgs_tsdf_blocks_list", "mm3dgs_tsdf_blocks_index",
             "mm3dgs_tsdf_blocks_integrate", "mm3dgs_tsdf_blocks_mesh_work_bytes", "mm3dgs_tsdf_blocks_mesh_plan", "mm3dgs_tsdf_blocks_mesh_emit")
    lib = _lib.load()
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", h) and name in _lib.exported_symbols() and hasattr(lib, name), name
    assert lib.mm3dgs_tsdf_blocks_table_bytes.restype is C.c_size_t and lib.mm3dgs_tsdf_blocks_mesh_work_bytes.restype is C.c_size_t
    for mb in (1, 3, 64, 1 << 18, 1 << 21):
        slots = 2
        while slots < 2 * mb:
            slots *= 2
        n = int(lib.mm3dgs_tsdf_blocks_table_bytes(mb))
        assert n % 8 == 0 and n >= 12 * slots, (mb, n)
        w = int(lib.mm3dgs_tsdf_blocks_mesh_work_bytes(mb))
        assert w % 8 == 0 and w >= 11 * 512 * mb, (mb, w)
    for mb in (0, (1 << 21) + 1, 1 << 40):
        assert int(lib.mm3dgs_tsdf_blocks_table_bytes(mb)) == 0 and int(lib.mm3dgs_tsdf_blocks_mesh_work_bytes(mb)) == 0, mb


def _cpu_slam(tmp, mesh):
    """The stand-in run of `device: cpu` of tests/test_mesh.py (32 x 48, 3 frames, the oracle rasterizer injected), run to its end."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.renderer import Renderer
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    from oracle.raster_ref import RefRasterizer
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    cfg = default_config(device="cpu", height=32, width=48, tracking={"iters": 2}, mapping={"iters": 3, "kf_every": 2}, outputdir=str(tmp), mesh=mesh)
    seq = SyntheticSequence(cfg, 3, 600, seed=2, renderer=Renderer(cfg, rasterizer_cls=RefRasterizer))
    slam = SLAM(cfg, seq, rasterizer_cls=RefRasterizer)
    slam.run()
    return slam, seq, cfg


def test_export_of_a_cpu_run_with_the_sparse_volume(tmp_path):
    MESH = {"voxel": 0.04, "every": 1, "max_voxels": 65536}
    slam, seq, cfg = _cpu_slam(tmp_path / "run", dict(MESH, export=False))
    with pytest.raises(ValueError, match=r"mesh\.max_voxels = 65536"):      # the dense lattice over the box of the views does not fit
        slam.export_mesh()
    cfg["mesh"]["volume"] = "sparse"
    out = slam.export_mesh()
    rows, tris = ms.read_mesh_ply(out["mesh"])
    c = out["counters"]
    print(f"MESHERR sparse cpu export: {c}, lattice {out['lattice']}, origin {out['origin']}")
    assert out["volume"] == "sparse" and out["blocks"] == c["blocks"] > 0 and out["pairs"] == c["pairs"] > 0 and out["volume_bytes"] == c["blocks"] * 512 * 24
    assert len(rows) == c["vertices"] > 0 and len(tris) == c["triangles"] > 0 and c["views"] == 3
    nx, ny, nz = out["lattice"]
    assert nx % 8 == ny % 8 == nz % 8 == 0 and nx * ny * nz > 65536 and c["blocks"] * 512 < nx * ny * nz
    topo = ms.mesh_topology(len(rows), tris)
    assert topo["unreferenced"] == 0 and topo["repeated"] == 0
    # by hand: the same views through the host classes, and against the dense mesh over the bounding lattice
    cam = {k: cfg["cam"][k] for k in ("fx", "fy", "cx", "cy")}
    first = np.round(np.asarray(out["origin"]) / 0.04).astype(np.int64)
    tsdf_w, rgb_w = ms.empty_volume(nx, ny, nz)
    with torch.no_grad():
        for i in range(3):
            r = slam.renderer.render(slam.gaussians, camera_pose=slam.estimate_pose_list[i])
            ms.integrate_host(tsdf_w, rgb_w, r["render"], r["depth"][0], r["depth"][1], slam.estimate_pose_list[i], **cam, origin=(0, 0, 0), voxel=0.04, trunc=out["trunc"],
                              sil_min=0.99, first=first)
    dense = ms.mesh_host(tsdf_w, rgb_w, (0, 0, 0), 0.04, 1.0, first=first)
    ta, tb = {t.tobytes() for t in rows[tris]}, {t.tobytes() for t in dense[0][dense[1]]}      # a triangle as its three vertex rows
    print(f"MESHERR sparse cpu export: dense over the bounding lattice {len(dense[0])} / {len(dense[1])}; {len(tb - ta)} triangles of cubes that touch an unreserved block")
    assert ta <= tb and len(ta) == len(tris)
    # the geometry evaluation and the cleaning take rows and triangles: they run unchanged
    cfg["mesh"]["clean"] = "largest"
    cleaned = slam.export_mesh(path=str(tmp_path / "clean"))
    assert cleaned["clean"]["triangles"] <= c["triangles"] and cleaned["volume"] == "sparse"
    cfg["mesh"]["clean"] = "none"
    # max_blocks below the need names the key; trunc above 16 voxel is an error of the options
    cfg["mesh"]["max_blocks"] = 4
    with pytest.raises(ValueError, match=r"mesh\.max_blocks = 4"):
        slam.export_mesh()
    cfg["mesh"].update(max_blocks=1 << 18, trunc=0.7)
    with pytest.raises(ValueError, match=r"mesh\.trunc"):
        slam.export_mesh()


def test_volume_dense_is_byte_identical_to_the_key_absent(tmp_path):
    MESH = {"voxel": 0.08, "every": 1}
    slam, seq, cfg = _cpu_slam(tmp_path / "run", dict(MESH, export=False))
    a = slam.export_mesh(path=str(tmp_path / "absent"))
    cfg["mesh"]["volume"] = "dense"
    b = slam.export_mesh(path=str(tmp_path / "dense"))
    assert (tmp_path / "absent" / "mesh.ply").read_bytes() == (tmp_path / "dense" / "mesh.ply").read_bytes()
    assert {k: v for k, v in a.items() if k != "mesh"} == {k: v for k, v in b.items() if k != "mesh"} and "volume" not in a
