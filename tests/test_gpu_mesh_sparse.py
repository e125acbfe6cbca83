"""mm3dgs_tsdf_blocks_* (csrc/tsdf_sparse.hip) through the raw C ABI: the reservation against mesh.reserve_host, list and index against a numpy
lookup, the integration against the dense kernel mm3dgs_tsdf_integrate byte for byte, the mesh against the dense kernels mm3dgs_tsdf_mesh_plan
/ _emit over the masked lattice and against mesh.mesh_blocks_host, determinism, rejected calls, and the export of a native-loop run.  Every
caller-owned array carries sentinel words behind it, the table and the work buffer lie between guard zones.

Bars.  Reservation: the key set and the counters exact; a pixel whose box edge lies within 1e-9 sample of a sample boundary is left out and
counted, at most 0.1 % of a case's pixels (the host statement reports none for these poses, and the test checks that).  Integration against
the dense kernel: every byte of every reserved block equal (both call one device function).  Against the host statement: the bars of
tests/test_gpu_mesh.py (weights and counters exact, |dT|, |dC| <= k 2^-24 after k views, exclusions <= 0.1 %).  Mesh against the dense
kernels: rows and triangles equal byte for byte after the documented reordering; against the host statement: triangle indices and totals
exact, a position component within 2^-24 |p| + 2^-40 (|anchor| + voxel max |index|), colour bytes within 1.  Every test prints its figures
(`MESHERR ...`, pytest -s) before it asserts."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from mm3dgs_slam_amd import mesh as ms
from mm3dgs_slam_amd import pointcloud as pc
from tests import mesh_cases as cases
from tests import mesh_sparse_cases as sc
from tests import pointcloud_cases as pcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096               # bytes of guard zone on each side of the table and of the work buffer
PAD = 8                    # entries behind every caller-owned array that no call may touch
SENT = 0x7A7A7A7A          # every int32 of an untouched row, triangle or neighbour entry
KEY_SENT = 0x5B5B5B5B5B5B5B5B
WORK_SENT = 0xA5           # every byte of the guard zones


def _ptr(t):
    return None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _lib():
    from mm3dgs_slam_amd import _lib
    return _lib.load()


def _stream():
    from mm3dgs_slam_amd.rasterizer import _stream
    return _stream()


def _vec(o):
    return None if o is None else (C.c_double * 3)(*[float(v) for v in o])


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def to_dev(v):
    out = dict(v)
    for k in ("color", "depth", "sil", "pose"):
        out[k] = _dev(v[k])
    return out


class Blocks:
    """Caller-owned buffers of one voxel-block volume on the device: the table between guard zones, the two counter arrays, and -- from
    `freeze` on -- keys, neighbours and the pool, each with sentinel entries behind it."""

    def __init__(self, case, max_blocks, table_fill=0x00):
        self.case, self.max_blocks = case, max_blocks
        self.nbytes = int(_lib().mm3dgs_tsdf_blocks_table_bytes(max_blocks))
        assert self.nbytes > 0 and self.nbytes % 8 == 0
        self.buf = torch.full((2 * GUARD + self.nbytes,), WORK_SENT, dtype=torch.uint8, device=DEV)
        self.buf[GUARD:GUARD + self.nbytes] = table_fill      # the table's contents are irrelevant before the reset
        self.table = self.buf.data_ptr() + GUARD
        self.rc = torch.full((8,), -7, dtype=torch.int64, device=DEV)
        self.ic = torch.zeros(8, dtype=torch.int64, device=DEV)
        assert _lib().mm3dgs_tsdf_blocks_reset(_ptr(self.table), max_blocks, _ptr(self.rc), _stream()) == 0
        torch.cuda.synchronize()
        assert not self.rc.cpu().any()
        self.n = 0

    def view_args(self, v, **over):
        a = dict(H=v["depth"].shape[0], W=v["depth"].shape[1], fx=v["cam"]["fx"], fy=v["cam"]["fy"], cx=v["cam"]["cx"], cy=v["cam"]["cy"], pose=v["pose"],
                 color=v["color"], depth=v["depth"], sil=v["sil"], sil_min=v["sil_min"], depth_max=v["depth_max"], anchor=self.case["anchor"], voxel=self.case["voxel"],
                 trunc=self.case["trunc"], clip=None, table=self.table, max_blocks=self.max_blocks, rc=self.rc, ic=self.ic)
        a.update(over)
        return a

    def reserve(self, v, **over):
        a = self.view_args(v, **over)
        clip = None if a["clip"] is None else (C.c_int * 6)(*[int(x) for x in a["clip"]])
        rc = _lib().mm3dgs_tsdf_blocks_reserve(a["H"], a["W"], a["fx"], a["fy"], a["cx"], a["cy"], _ptr(a["pose"]), _ptr(a["depth"]), _ptr(a["sil"]), a["sil_min"],
                                               a["depth_max"], _vec(a["anchor"]), a["voxel"], a["trunc"], clip, _ptr(a["table"]), a["max_blocks"], _ptr(a["rc"]), _stream())
        torch.cuda.synchronize()
        return rc

    def counters(self):
        return self.rc.cpu().numpy().copy()

    def check_guards(self):
        buf = self.buf.cpu().numpy()
        assert bool((buf[:GUARD] == WORK_SENT).all()) and bool((buf[-GUARD:] == WORK_SENT).all()), "a guard zone of the table was written"

    def list(self, cap=None):
        """The table's keys, sorted (numpy int64), after checking the entries behind the cap."""
        n = int(self.counters()[3]) if cap is None else cap
        keys = torch.full((n + PAD,), KEY_SENT, dtype=torch.int64, device=DEV)
        assert _lib().mm3dgs_tsdf_blocks_list(_ptr(self.table), self.max_blocks, _ptr(keys), n, _stream()) == 0
        torch.cuda.synchronize()
        k = keys.cpu().numpy()
        assert bool((k[n:] == KEY_SENT).all()), "keys behind the cap were written"
        self.check_guards()
        return np.sort(k[:n])

    def index(self, keys, **over):
        n = len(keys)
        self.keys = torch.full((n + PAD,), KEY_SENT, dtype=torch.int64, device=DEV)
        self.keys[:n] = _dev(np.asarray(keys, dtype=np.int64))
        self.nbr = torch.full((n + PAD, 27), SENT, dtype=torch.int32, device=DEV)
        a = dict(table=self.table, max_blocks=self.max_blocks, keys=self.keys, n=n, nbr=self.nbr, rc=self.rc)
        a.update(over)
        rc = _lib().mm3dgs_tsdf_blocks_index(_ptr(a["table"]), a["max_blocks"], _ptr(a["keys"]), a["n"], _ptr(a["nbr"]), _ptr(a["rc"]), _stream())
        torch.cuda.synchronize()
        self.n = n
        return rc

    def neighbours(self):
        nb = self.nbr.cpu().numpy()
        assert bool((nb[self.n:] == SENT).all()), "neighbour entries behind the table were written"
        self.check_guards()
        return nb[:self.n]

    def freeze(self):
        keys = self.list()
        assert self.index(keys) == 0 and int(self.counters()[6]) == 0
        self.alloc_pool()
        return keys

    def alloc_pool(self, tsdf_w=None, rgb_w=None):
        n = self.n
        self.tw = torch.full((n * 512 + PAD, 2), float("nan"), dtype=torch.float32, device=DEV)
        self.rw = torch.full((n * 512 + PAD, 4), float("nan"), dtype=torch.float32, device=DEV)
        self.tw[:n * 512] = 0 if tsdf_w is None else _dev(tsdf_w.reshape(-1, 2))
        self.rw[:n * 512] = 0 if rgb_w is None else _dev(rgb_w.reshape(-1, 4))

    def integrate(self, v, **over):
        a = self.view_args(v, keys=self.keys, n=self.n, tsdf_w=self.tw, rgb_w=self.rw)
        a.update(over)
        rc = _lib().mm3dgs_tsdf_blocks_integrate(a["H"], a["W"], a["fx"], a["fy"], a["cx"], a["cy"], _ptr(a["pose"]), _ptr(a["color"]), _ptr(a["depth"]), _ptr(a["sil"]),
                                                 a["sil_min"], a["depth_max"], _vec(a["anchor"]), a["voxel"], a["trunc"], _ptr(a["keys"]), a["n"], _ptr(a["tsdf_w"]),
                                                 _ptr(a["rgb_w"]), _ptr(a["ic"]), _stream())
        torch.cuda.synchronize()
        return rc

    def pool(self):
        tw, rw = self.tw.cpu().numpy(), self.rw.cpu().numpy()
        n = self.n * 512
        assert np.isnan(tw[n:]).all() and np.isnan(rw[n:]).all(), "the words behind the pool were written"
        assert bool((self.keys.cpu().numpy()[self.n:] == KEY_SENT).all())
        return tw[:n].reshape(-1, 512, 2).copy(), rw[:n].reshape(-1, 512, 4).copy(), self.ic.cpu().numpy().copy()


class BlockMesher:
    """work between guard zones, sentinel-filled rows and triangles with PAD entries behind the caps."""

    def __init__(self, blk, anchor, voxel, vcap, tcap, work_fill=0x00, min_weight=1.0):
        self.blk, self.anchor, self.voxel, self.vcap, self.tcap, self.min_weight = blk, anchor, voxel, vcap, tcap, min_weight
        self.nwork = int(_lib().mm3dgs_tsdf_blocks_mesh_work_bytes(blk.n))
        assert self.nwork > 0 and self.nwork % 8 == 0
        self.buf = torch.full((2 * GUARD + self.nwork,), WORK_SENT, dtype=torch.uint8, device=DEV)
        self.buf[GUARD:GUARD + self.nwork] = work_fill
        self.work = self.buf.data_ptr() + GUARD
        self.rows = torch.full((vcap + PAD, 4), SENT, dtype=torch.int32, device=DEV)
        self.tris = torch.full((tcap + PAD, 3), SENT, dtype=torch.int32, device=DEV)
        self.counters = torch.full((8,), -7, dtype=torch.int64, device=DEV)

    def plan(self, **over):
        b = self.blk
        a = dict(n=b.n, nbr=b.nbr, tsdf_w=b.tw, min_weight=self.min_weight, work=self.work, counters=self.counters)
        a.update(over)
        rc = _lib().mm3dgs_tsdf_blocks_mesh_plan(a["n"], _ptr(a["nbr"]), _ptr(a["tsdf_w"]), a["min_weight"], _ptr(a["work"]), _ptr(a["counters"]), _stream())
        torch.cuda.synchronize()
        return rc

    def emit(self, **over):
        b = self.blk
        a = dict(n=b.n, keys=b.keys, nbr=b.nbr, tsdf_w=b.tw, rgb_w=b.rw, anchor=_vec(self.anchor), voxel=self.voxel, work=self.work, rows=self.rows, vcap=self.vcap,
                 tris=self.tris, tcap=self.tcap, counters=self.counters)
        a.update(over)
        rc = _lib().mm3dgs_tsdf_blocks_mesh_emit(a["n"], _ptr(a["keys"]), _ptr(a["nbr"]), _ptr(a["tsdf_w"]), _ptr(a["rgb_w"]), a["anchor"], a["voxel"], _ptr(a["work"]),
                                                 _ptr(a["rows"]), a["vcap"], _ptr(a["tris"]), a["tcap"], _ptr(a["counters"]), _stream())
        torch.cuda.synchronize()
        return rc

    def read(self):
        rows, tris, buf = self.rows.cpu().numpy(), self.tris.cpu().numpy(), self.buf.cpu().numpy()
        assert bool((buf[:GUARD] == WORK_SENT).all()) and bool((buf[-GUARD:] == WORK_SENT).all()), "a guard zone of the work buffer was written"
        assert bool((rows[self.vcap:] == SENT).all()) and bool((tris[self.tcap:] == SENT).all()), "entries behind a cap were written"
        return rows, tris, self.counters.cpu().numpy().copy()


def _mesh_blocks(blk, anchor, voxel, work_fill=0x00):
    """The device mesh of a frozen, filled Blocks: (rows [V,4], triangles [T,3]) with exact caps from the plan's totals."""
    probe = BlockMesher(blk, anchor, voxel, 0, 0, work_fill)
    assert probe.plan() == 0
    V, T = (int(x) for x in probe.counters.cpu()[:2])
    assert probe.counters.cpu().tolist() == [V, T, 0, 0, 0, 0, 0, 0]
    m = BlockMesher(blk, anchor, voxel, V, T, work_fill)
    assert m.plan() == 0 and m.emit() == 0
    rows, tris, c = m.read()
    assert c.tolist() == [V, T, V, T, 0, 0, 0, 0]
    return rows[:V], tris[:T]


# ---- 1. reservation ------------------------------------------------------------------------------------------------------------------
RESERVE_CASES = [((17, 33), p, 1) for p in pcases.PATTERNS] + [((48, 64), p, 3) for p in pcases.PATTERNS] + [((17, 33), "all", 3), ((48, 64), "all", 1)]


@pytest.mark.parametrize("hw,pattern,n_views", RESERVE_CASES)
def test_reserve_against_the_host_statement(hw, pattern, n_views):
    case = sc.scattered_case(hw, pattern, n_views)
    want, c_h, near, clean = sc.reserve_all(case, full=True)
    blk = Blocks(case, 1024, table_fill=0xFF)
    for v in case["views"]:
        assert blk.reserve(to_dev(v)) == 0
    c = blk.counters()
    keys = blk.list()
    print(f"MESHERR sparse reserve {hw} {pattern} x{n_views}: counters {c.tolist()} (host {c_h}), {len(keys)} blocks, {near} of {c_h[1]} pixels near a sample boundary")
    assert near <= 1e-3 * max(c_h[1], 1)
    assert bool(np.isin(clean, keys).all()) and bool(np.isin(keys, want).all())
    if near == 0:
        assert np.array_equal(keys, want) and c.tolist() == c_h + [0, 0]
    assert c[0] == n_views and c[1] == c_h[1] and c[4] == 0 and c[6] == 0 and c[7] == 0
    blk.check_guards()


def test_reserve_with_a_clip_box_and_out_of_range_pixels():
    case = sc.sphere_case(0.03, True, n_views=2)
    all_keys, _, _ = sc.reserve_all(case)
    b = ms.key_blocks(all_keys)
    clip = np.concatenate([b.min(0) + 2, b.max(0) - 3])
    want, c_h, near = sc.reserve_all(case, clip=clip)
    blk = Blocks(case, 2048)
    for v in case["views"]:
        assert blk.reserve(to_dev(v), clip=clip) == 0
    keys, c = blk.list(), blk.counters()
    print(f"MESHERR sparse reserve clip {clip.tolist()}: counters {c.tolist()} (host {c_h}), {len(all_keys)} blocks without the clip")
    assert near == 0 and 0 < len(want) < len(all_keys) and np.array_equal(keys, want) and c.tolist() == c_h + [0, 0]
    far = dict(case, anchor=np.array([case["voxel"] * 8 * (1 << 21), 0.0, 0.0]))
    blk = Blocks(far, 64)
    assert blk.reserve(to_dev(case["views"][0])) == 0
    c = blk.counters()
    assert c[1] == c[5] > 0 and c[2] == c[3] == c[4] == 0


def test_reserve_into_a_table_of_64_blocks_and_one_that_is_too_small():
    case = sc.sphere_case(0.04, False, n_views=1)
    want, c_h, near = sc.reserve_all(case)
    assert near == 0 and 56 <= len(want) <= 64      # a load of about 1/2 in 128 slots: long probe chains
    blk = Blocks(case, 64, table_fill=0xFF)
    assert blk.reserve(to_dev(case["views"][0])) == 0
    keys, c = blk.list(), blk.counters()
    print(f"MESHERR sparse reserve max_blocks 64: counters {c.tolist()} (host {c_h})")
    assert np.array_equal(keys, want) and c.tolist() == c_h + [0, 0]
    # max_blocks below the need: counted, nothing outside the table is written, and the device class refuses to freeze
    small = Blocks(case, 16, table_fill=0xFF)
    assert small.reserve(to_dev(case["views"][0])) == 0
    c = small.counters()
    got = small.list(64)
    print(f"MESHERR sparse reserve max_blocks 16: counters {c.tolist()}")
    small.check_guards()
    assert c[4] >= len(want) - 16 > 0 and c[1] == c_h[1] and c[3] > 16 and bool(np.isin(got[got != KEY_SENT], want).all())
    v = case["views"][0]
    vol = ms.SparseTsdfVolume(case["voxel"], case["trunc"], *v["depth"].shape, v["cam"], sil_min=v["sil_min"], max_blocks=16, device=DEV)
    vol.reserve(_dev(v["depth"]), None, _dev(v["pose"]))
    with pytest.raises(ValueError, match=r"mesh\.max_blocks = 16.*mesh\.voxel"):
        vol.freeze()
    empty = ms.SparseTsdfVolume(case["voxel"], case["trunc"], *v["depth"].shape, v["cam"], device=DEV)
    empty.reserve(_dev(np.zeros_like(v["depth"])), None, _dev(v["pose"]))
    with pytest.raises(ValueError, match="no view has a valid pixel"):
        empty.freeze()


# ---- 2. list and index -----------------------------------------------------------------------------------------------------------------
def _one_pixel_case():
    """One valid pixel at trunc = 16 voxel: its box spans 5 blocks per axis, and a clip picks the blocks of an arrangement out of it."""
    v = pcases.view(17, 33, "last")
    case = {"views": [v], "voxel": 0.05, "trunc": 0.8, "anchor": np.zeros(3)}
    keys, _, near = sc.reserve_all(case)
    b = ms.key_blocks(keys)
    assert near == 0 and bool((b.max(0) - b.min(0) >= 3).all())
    return case, to_dev(v), b.min(0)


def test_index_of_small_arrangements():
    case, vd, b0 = _one_pixel_case()
    arrangements = {"one block": [b0], "2 x 2 x 2": [b0 + np.array([i, j, k]) for k in (0, 1) for j in (0, 1) for i in (0, 1)],
                    "three blocks that do not touch": [b0, b0 + np.array([2, 0, 0]), b0 + np.array([0, 2, 2])]}
    for name, blocks in arrangements.items():
        blk = Blocks(case, 8)
        if name == "2 x 2 x 2":
            assert blk.reserve(vd, clip=np.concatenate([b0, b0 + 1])) == 0
        else:
            for b in blocks:
                assert blk.reserve(vd, clip=np.concatenate([b, b])) == 0
        keys = blk.list()
        want = np.sort(ms.block_keys(np.array(blocks)))
        assert np.array_equal(keys, want), name
        assert blk.index(keys) == 0
        nb, c = blk.neighbours(), blk.counters()
        print(f"MESHERR sparse index {name}: {len(keys)} blocks, {int((nb >= 0).sum())} neighbour entries, counters {c.tolist()}")
        assert c[6] == 0 and np.array_equal(nb, sc.neighbours_host(keys)) and np.array_equal(nb[:, 13], np.arange(len(keys)))
        if len(keys) == 1:
            assert bool((np.delete(nb[0], 13) == -1).all())
        if name == "2 x 2 x 2":
            assert bool(((nb >= 0).sum(1) == 8).all())
        if name.startswith("three"):
            assert int((nb >= 0).sum()) == 3
        # unsorted keys, a repeated key and a foreign key set the error counter and index nothing
        if len(keys) > 1:
            for bad in (keys[::-1].copy(), np.concatenate([keys[:1], keys[:1], keys[2:]]), np.concatenate([keys[:-1], keys[-1:] + 5])):
                assert blk.index(bad) == 0
                assert int(blk.counters()[6]) > 0, bad
                assert bool((blk.nbr.cpu().numpy() == SENT).all())
            assert blk.index(keys) == 0 and int(blk.counters()[6]) == 0 and np.array_equal(blk.neighbours(), sc.neighbours_host(keys))      # the counter is the last call's


@pytest.fixture(scope="module")
def wall():
    """The sphere-and-wall scene once: the case at an anchor that makes every block coordinate positive, its host keys, and the frozen
    device blocks with the three views integrated -- after the first view and after the third --, next to the dense kernel's volume over
    [0, 8 (bmax + 1)) with origin = anchor."""
    return _against_dense(sc.sphere_case(0.03, True))


def _against_dense(case):
    first_keys, _, _ = sc.reserve_all(case)
    down = ms.key_blocks(first_keys).min(0) - 1
    case = dict(case, anchor=case["anchor"] + case["voxel"] * 8.0 * down)      # the anchor moved down by whole blocks: reserve again
    want, c_h, near = sc.reserve_all(case)
    b = ms.key_blocks(want)
    assert near == 0 and b.min() >= 0
    dims = [int(x) for x in 8 * (b.max(0) + 1)]
    blk = Blocks(case, 1024)
    views = [to_dev(v) for v in case["views"]]
    for v in views:
        assert blk.reserve(v) == 0
    keys = blk.freeze()
    assert np.array_equal(keys, want)
    n = dims[0] * dims[1] * dims[2]
    dtw = torch.full((n + PAD, 2), float("nan"), dtype=torch.float32, device=DEV)
    drw = torch.full((n + PAD, 4), float("nan"), dtype=torch.float32, device=DEV)
    dc = torch.zeros(8, dtype=torch.int64, device=DEV)
    lib = _lib()
    assert lib.mm3dgs_tsdf_reset(dims[0], dims[1], dims[2], _ptr(dtw), _ptr(drw), _ptr(dc), _stream()) == 0
    s = ms.pool_index(b, np.zeros(3, dtype=np.int64), dims, np.arange(n))
    at = np.argsort(s, kind="stable")[int((s < 0).sum()):]      # dense flat index of every pool sample
    snaps = []
    for k, v in enumerate(views):
        assert blk.integrate(v) == 0
        assert lib.mm3dgs_tsdf_integrate(v["depth"].shape[0], v["depth"].shape[1], v["cam"]["fx"], v["cam"]["fy"], v["cam"]["cx"], v["cam"]["cy"], _ptr(v["pose"]),
                                         _ptr(v["color"]), _ptr(v["depth"]), _ptr(v["sil"]), v["sil_min"], v["depth_max"], _vec(case["anchor"]), case["voxel"], case["trunc"],
                                         dims[0], dims[1], dims[2], _ptr(dtw), _ptr(drw), _ptr(dc), _stream()) == 0
        torch.cuda.synchronize()
        if k in (0, len(views) - 1):
            snaps.append((k + 1,) + blk.pool() + (dtw.cpu().numpy()[:n].copy(), drw.cpu().numpy()[:n].copy(), dc.cpu().numpy().copy()))
    return {"case": case, "keys": keys, "blocks": b, "dims": dims, "blk": blk, "snaps": snaps, "at": at, "reserved": (s >= 0).reshape(dims[2], dims[1], dims[0]), "dtw": dtw, "drw": drw}


def test_index_of_the_wall_scene_equals_a_numpy_lookup(wall):
    nb = wall["blk"].neighbours()
    print(f"MESHERR sparse index wall scene: {len(wall['keys'])} blocks, {int((nb >= 0).sum())} neighbour entries")
    assert 2 * len(wall["keys"]) > 1024      # more than 1024 per-256 counts: the second round of the scan in the extraction
    assert np.array_equal(nb, sc.neighbours_host(wall["keys"]))


# ---- 3. integration against the dense kernel --------------------------------------------------------------------------------------------
def _same_as_dense(tag, d):
    for k, ptw, prw, ic, dtw, drw, dc in d["snaps"]:
        at = d["at"]
        same_t, same_c = ptw.reshape(-1, 2).view(np.int32) == dtw[at].view(np.int32), prw.reshape(-1, 4).view(np.int32) == drw[at].view(np.int32)
        dist, col = int(dtw[at][:, 1].astype(np.float64).sum()), int(drw[at][:, 3].astype(np.float64).sum())      # a weight counts its sample's updates
        print(f"MESHERR sparse integrate {tag} after {k} view(s): {len(at)} samples in {len(d['keys'])} blocks, {int((~same_t).sum())} distance and {int((~same_c).sum())} colour "
              f"words differ from the dense kernel's; counters {ic.tolist()}, dense {dc.tolist()} of which {dist} / {col} in the blocks")
        assert bool(same_t.all()) and bool(same_c.all())
        assert ic.tolist() == [k, dist, col, 0, 0, 0, 0, 0] and dc[0] == k
        assert col == dc[2] and dist <= dc[1] and col > 0      # the band lies inside the blocks: every colour update of the dense volume is there


def test_integrate_equals_the_dense_kernel_byte_for_byte(wall):
    _same_as_dense("sphere + wall", wall)


@pytest.mark.parametrize("hw,pattern,n_views", [((17, 33), "all", 3), ((48, 64), "sil_edge", 3), ((48, 64), "depth_max_edge", 3), ((48, 64), "planted", 1)])
def test_integrate_scattered_views_equals_the_dense_kernel(hw, pattern, n_views):
    _same_as_dense(f"{hw} {pattern}", _against_dense(sc.scattered_case(hw, pattern, n_views)))


@pytest.fixture(scope="module")
def astride():
    """A scattered-depth case whose anchor lies in the scene's middle (negative block coordinates), frozen and integrated on the device,
    next to the host statement over the bounding lattice."""
    base = sc.scattered_case((17, 33), "all", 3)
    k0, _, _ = sc.reserve_all(base)
    b0 = ms.key_blocks(k0)
    case = dict(base, anchor=base["voxel"] * 8.0 * 0.5 * (b0.min(0) + b0.max(0) + 1) + np.array([0.0031, -0.0042, 0.0057]))
    want, c_h, near = sc.reserve_all(case)
    blk = Blocks(case, 512)
    views = [to_dev(v) for v in case["views"]]
    for v in views:
        assert blk.reserve(v) == 0
    keys = blk.freeze()
    for v in views:
        assert blk.integrate(v) == 0
    blocks, first, dims, origin = ms._frozen_lattice(want, case["anchor"], case["voxel"])
    n = dims[0] * dims[1] * dims[2]
    s = ms.pool_index(blocks, first, dims, np.arange(n))
    reserved = (s >= 0).reshape(dims[2], dims[1], dims[0])
    tw, rw, c, excluded = sc.dense_over(case, first, dims, mask=reserved, excluded=True)
    return {"case": case, "want": want, "near": near, "keys": keys, "blk": blk, "blocks": blocks, "first": first, "dims": dims, "host": (tw, rw, c, excluded), "s": s}


def test_integrate_with_negative_block_coordinates_against_the_host_statement(astride):
    d = astride
    assert d["near"] == 0 and np.array_equal(d["keys"], d["want"])
    b = d["blocks"]
    assert bool((b.min(0) < 0).all()) and bool((b.max(0) >= 0).all())
    tw_h, rw_h, c_h, excluded = d["host"]
    at = np.argsort(d["s"], kind="stable")[int((d["s"] < 0).sum()):]
    ptw, prw, ic = d["blk"].pool()
    tw, rw = ptw.reshape(-1, 2), prw.reshape(-1, 4)
    hw_, hr_, ex = tw_h.reshape(-1, 2)[at], rw_h.reshape(-1, 4)[at], excluded.reshape(-1)[at]
    keep, k = ~ex, 3
    with np.errstate(invalid="ignore"):
        dT = np.abs(tw[:, 0].astype(np.float64) - hw_[:, 0].astype(np.float64))[keep]
        same_nan = np.isnan(rw[:, :3]) == np.isnan(hr_[:, :3])
        dC = np.nan_to_num(np.abs(rw[:, :3].astype(np.float64) - hr_[:, :3].astype(np.float64)), nan=0.0)[keep]
    print(f"MESHERR sparse integrate negative blocks {b.min(0).tolist()} .. {b.max(0).tolist()}: counters {ic.tolist()} (host {c_h}), {int(ex.sum())} of {ex.size} samples excluded, "
          f"max |dT| = {dT.max() / 2.0 ** -24:.3f} x 2^-24, max |dC| = {dC.max() / 2.0 ** -24:.3f} x 2^-24 (bar {k})")
    assert ex.sum() <= 1e-3 * ex.size
    if not ex.any():
        assert ic.tolist() == c_h + [0] * 5
    assert np.array_equal(tw[:, 1][keep], hw_[:, 1][keep]) and np.array_equal(rw[:, 3][keep], hr_[:, 3][keep])      # the weights, exact
    assert bool(same_nan[keep].all()) and dT.max() <= k * 2.0 ** -24 and dC.max() <= k * 2.0 ** -24


# ---- 4. the mesh ---------------------------------------------------------------------------------------------------------------------------
def _check_mesh(tag, anchor, voxel, reach, rows, tris, want_rows, want_tris, xyz):
    """Triangles exact; positions against the float64 ones `xyz` of the host statement; colour bytes within 1 (tests/test_gpu_mesh.py's bars)."""
    assert np.array_equal(tris, want_tris), "triangle indices"
    assert len(rows) == len(want_rows) == len(xyz) > 0
    err = np.abs(pc.rows_xyz(rows).astype(np.float64) - xyz)
    bound = 2.0 ** -24 * np.abs(xyz) + 2.0 ** -40 * (np.abs(np.asarray(anchor, dtype=np.float64)) + voxel * np.asarray(reach, dtype=np.float64))[None, :]
    dcol = np.abs(pc.rows_rgba(rows).astype(np.int64) - pc.rows_rgba(want_rows).astype(np.int64))
    differ = int((pc.rows_xyz(rows).view(np.int32) != pc.rows_xyz(want_rows).view(np.int32)).sum())
    print(f"MESHERR sparse mesh {tag}: {len(rows)} vertices, {len(tris)} triangles; max position err / bound = {float((err / bound).max()):.3f}, {differ} of {3 * len(rows)} components "
          f"differ from the host's float32; max colour byte difference {int(dcol.max())}")
    assert bool((err <= bound).all())
    assert int(dcol.max()) <= 1 and bool((pc.rows_rgba(rows)[:, 3] == 255).all())


def test_mesh_of_the_wall_scene_equals_the_dense_kernels_on_the_masked_lattice(wall):
    d, case, dims = wall, wall["case"], wall["dims"]
    rows, tris = _mesh_blocks(d["blk"], case["anchor"], case["voxel"], work_fill=0xFF)
    # the dense volume of the dense kernel with its unreserved samples zeroed on the device, through the dense mesh kernels
    n = dims[0] * dims[1] * dims[2]
    mask = _dev(d["reserved"].reshape(-1))
    dtw, drw = d["dtw"].clone(), d["drw"].clone()
    dtw[:n][~mask] = 0
    drw[:n][~mask] = 0
    lib = _lib()
    nwork = int(lib.mm3dgs_tsdf_mesh_work_bytes(*dims))
    work = torch.empty(nwork // 8, dtype=torch.int64, device=DEV)
    mc = torch.zeros(8, dtype=torch.int64, device=DEV)
    assert lib.mm3dgs_tsdf_mesh_plan(dims[0], dims[1], dims[2], _ptr(dtw), 1.0, _ptr(work), _ptr(mc), _stream()) == 0
    V, T = (int(x) for x in mc.cpu()[:2])
    drows, dtris = torch.empty(max(V, 1), 4, dtype=torch.int32, device=DEV), torch.empty(max(T, 1), 3, dtype=torch.int32, device=DEV)
    assert lib.mm3dgs_tsdf_mesh_emit(dims[0], dims[1], dims[2], _ptr(dtw), _ptr(drw), _vec(case["anchor"]), case["voxel"], _ptr(work), _ptr(drows), V, _ptr(dtris), T, _ptr(mc),
                                     _stream()) == 0
    torch.cuda.synchronize()
    drows, dtris = drows.cpu().numpy()[:V], dtris.cpu().numpy()[:T]
    # the documented reordering, in numpy: the sample of every vertex and the cube of every triangle from the host statement on the same bytes
    htw, hrw = dtw.cpu().numpy()[:n].reshape(dims[2], dims[1], dims[0], 2), drw.cpu().numpy()[:n].reshape(dims[2], dims[1], dims[0], 4)
    hrows, htris, _, vq, tq = ms.mesh_host(htw, hrw, case["anchor"], case["voxel"], where=True)
    assert len(hrows) == V and np.array_equal(htris, dtris)
    want_rows, want_tris, _ = ms.reorder_to_blocks(drows, dtris, vq, tq, d["blocks"], np.zeros(3, dtype=np.int64), dims)
    full = d["snaps"][-1]
    un = ms.mesh_host(full[4].reshape(dims[2], dims[1], dims[0], 2), full[5].reshape(dims[2], dims[1], dims[0], 4), case["anchor"], case["voxel"])
    print(f"MESHERR sparse mesh wall scene: {len(rows)} vertices, {len(tris)} triangles in {len(d['keys'])} blocks; the dense kernels on the masked lattice {V} / {T}, "
          f"on the unmasked one {len(un[0])} / {len(un[1])}")
    assert len(tris) > 10000 and rows.tobytes() == want_rows.tobytes() and tris.tobytes() == want_tris.tobytes()
    topo = ms.mesh_topology(len(rows), tris)
    assert topo["unreferenced"] == 0 and topo["repeated"] == 0


def _analytic(name):
    if name == "one block":
        vol = cases.analytic_volume("sphere", (8, 8, 8))
        return {"tsdf_w": vol["tsdf_w"], "rgb_w": vol["rgb_w"], "blocks": np.zeros((1, 3), dtype=np.int64), "keys": ms.block_keys(np.zeros((1, 3))), "first": np.zeros(3, dtype=np.int64),
                "dims": [8, 8, 8], "origin": vol["origin"], "voxel": vol["voxel"]}
    if name == "2 x 2 x 2":      # the sphere's centre on the corner the eight blocks share: cubes that span 2, 4 and 8 blocks, vertices on seam edges
        vol = cases.analytic_volume("sphere", (16, 16, 16))
        blocks = np.array([[i, j, k] for k in (0, 1) for j in (0, 1) for i in (0, 1)])
        return {"tsdf_w": vol["tsdf_w"], "rgb_w": vol["rgb_w"], "blocks": blocks, "keys": ms.block_keys(blocks), "first": np.zeros(3, dtype=np.int64), "dims": [16, 16, 16],
                "origin": vol["origin"], "voxel": vol["voxel"]}
    kind, drop = name.split()[0], name.endswith("minus a third")
    return sc.analytic_blocks(kind, drop_third=drop)


class GivenBlocks(Blocks):
    """Keys, neighbours and a pool written directly (the mesh calls take arrays: no table is needed), with the sentinel entries behind them."""

    def __init__(self, keys, tsdf_w, rgb_w):
        self.n = len(keys)
        self.keys = torch.full((self.n + PAD,), KEY_SENT, dtype=torch.int64, device=DEV)
        self.keys[:self.n] = _dev(np.asarray(keys, dtype=np.int64))
        self.nbr = torch.full((self.n + PAD, 27), SENT, dtype=torch.int32, device=DEV)
        self.nbr[:self.n] = _dev(sc.neighbours_host(keys))
        self.alloc_pool(tsdf_w, rgb_w)


@pytest.mark.parametrize("name", ["one block", "2 x 2 x 2", "sphere", "torus", "sphere minus a third", "torus minus a third"])
def test_mesh_of_analytic_volumes_against_the_host_statement(name):
    a = _analytic(name)
    ptw, prw = sc.to_pool(a["tsdf_w"], a["rgb_w"], a["blocks"], a["first"], a["dims"])
    want_rows, want_tris, m, xyz = ms.mesh_blocks_host(a["keys"], ptw, prw, a["origin"], a["voxel"], full=True)
    blk = GivenBlocks(a["keys"], ptw, prw)
    outs = []
    for fill in (0x00, 0xFF):      # the work buffer's contents are irrelevant before plan
        rows, tris = _mesh_blocks(blk, a["origin"], a["voxel"], work_fill=fill)
        outs.append((rows.tobytes(), tris.tobytes()))
    assert outs[0] == outs[1] and m[:2].tolist() == [len(rows), len(tris)]
    _check_mesh(name, a["origin"], a["voxel"], a["dims"], rows, tris, want_rows, want_tris, xyz)
    topo = ms.mesh_topology(len(rows), tris)
    print(f"MESHERR sparse mesh {name}: {blk.n} blocks, {topo}")
    assert topo["unreferenced"] == 0 and topo["repeated"] == 0
    if name in ("2 x 2 x 2", "sphere", "torus"):
        assert topo["closed"] and topo["euler"] == (0 if name == "torus" else 2)
    if name == "2 x 2 x 2":
        # vertices on the seams: some edge (q, d) has q in one block and q + d in another
        q = np.floor((xyz - a["origin"][None, :]) / a["voxel"] + 1e-9).astype(np.int64)
        assert int(((q % 8 == 7).any(1)).sum()) > 0
    assert blk.tw.cpu().numpy()[:blk.n * 512].tobytes() == ptw.tobytes() and blk.rw.cpu().numpy()[:blk.n * 512].tobytes() == prw.tobytes()      # the pool is read only


def test_mesh_with_negative_block_coordinates_against_the_host_statement(astride):
    d, case = astride, astride["case"]
    ptw, prw, _ = d["blk"].pool()
    want_rows, want_tris, m, xyz = ms.mesh_blocks_host(d["keys"], ptw, prw, case["anchor"], case["voxel"], full=True)
    rows, tris = _mesh_blocks(d["blk"], case["anchor"], case["voxel"])
    reach = np.abs(np.concatenate([d["first"], d["first"] + np.asarray(d["dims"])])).reshape(2, 3).max(0)
    _check_mesh("negative blocks", case["anchor"], case["voxel"], reach, rows, tris, want_rows, want_tris, xyz)


def test_caps_below_the_totals_end_as_counts():
    a = _analytic("2 x 2 x 2")
    ptw, prw = sc.to_pool(a["tsdf_w"], a["rgb_w"], a["blocks"], a["first"], a["dims"])
    want_rows, want_tris, _ = ms.mesh_blocks_host(a["keys"], ptw, prw, a["origin"], a["voxel"])
    V, T = len(want_rows), len(want_tris)
    blk = GivenBlocks(a["keys"], ptw, prw)
    for vcap, tcap in ((V // 2, T), (V, T // 3), (0, 0)):
        m = BlockMesher(blk, a["origin"], a["voxel"], vcap, tcap)
        assert m.plan() == 0 and m.emit() == 0
        rows, tris, c = m.read()
        ok = (np.arange(T) < tcap) & (want_tris < vcap).all(1)
        print(f"MESHERR sparse caps vcap {vcap} of {V}, tcap {tcap} of {T}: counters {c.tolist()}, {int(ok.sum())} triangles expected")
        assert c.tolist() == [V, T, min(V, vcap), int(ok.sum()), V - min(V, vcap), T - int(ok.sum()), 0, 0]
        assert np.array_equal(rows[:vcap, 3], want_rows[:vcap, 3]) and np.array_equal(tris[:tcap][ok[:tcap]], want_tris[:tcap][ok[:tcap]])
        assert bool((tris[:tcap][~ok[:tcap]] == SENT).all())


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------------------
def _full_run(case, reserve_order):
    v0 = case["views"][0]
    vol = ms.SparseTsdfVolume(case["voxel"], case["trunc"], *v0["depth"].shape, v0["cam"], sil_min=v0["sil_min"], depth_max=v0["depth_max"], max_blocks=1024, device=DEV)
    views = [to_dev(v) for v in case["views"]]
    for k in reserve_order:
        vol.reserve(views[k]["depth"], views[k]["sil"], views[k]["pose"])
    n = vol.freeze()
    for v in views:      # the integration order is the same in every run
        vol.add(v["color"], v["depth"], v["sil"], v["pose"])
    rows, tris, c = vol.extract()
    torch.cuda.synchronize()
    return {"keys": vol.keys.cpu().numpy().tobytes(), "nbr": vol.neighbours.cpu().numpy().tobytes(), "tw": vol.tsdf_w.cpu().numpy().tobytes(), "rw": vol.rgb_w.cpu().numpy().tobytes(),
            "rows": rows.cpu().numpy().tobytes(), "tris": tris.cpu().numpy().tobytes()}, c, (vol.dims, vol.origin.tolist()), (rows.cpu().numpy(), tris.cpu().numpy())


def test_two_runs_and_a_reversed_reservation_give_the_same_bytes():
    case = sc.sphere_case(0.02, False)
    a, ca, la, mesh = _full_run(case, (0, 1, 2))
    b, cb, lb, _ = _full_run(case, (0, 1, 2))
    r, cr, lr, _ = _full_run(case, (2, 1, 0))
    print(f"MESHERR sparse determinism: {ca}, lattice {la}")
    for name in a:
        assert a[name] == b[name], name
        assert a[name] == r[name], name + " (views reserved in reverse order)"
    assert ca == cb == cr and la == lb == lr
    # and the device class against the host class: the documented order, the counters
    host = sc.host_volume(case)
    hrows, htris, hc = host.extract()
    assert ca["blocks"] == hc["blocks"] == 193 and ca["pairs"] == hc["pairs"] and la[0] == host.dims and np.allclose(la[1], host.origin, atol=0, rtol=0)
    assert np.array_equal(mesh[1], htris) and len(mesh[0]) == len(hrows)
    excluded = sc.dense_over(case, host.first, host.dims, mask=host.reserved, excluded=True)[3] & host.reserved
    print(f"MESHERR sparse determinism: host {hc}, {int(excluded.sum())} samples near a rounding boundary")
    if not excluded.any():
        assert (ca["views"], ca["dist_updates"], ca["colour_updates"]) == (hc["views"], hc["dist_updates"], hc["colour_updates"])


# ---- 6. rejected calls -----------------------------------------------------------------------------------------------------------------
def test_rejected_calls_return_minus_one_and_write_nothing():
    case = sc.sphere_case(0.04, False, n_views=1)
    vd = to_dev(case["views"][0])
    blk = Blocks(case, 64)
    assert blk.reserve(vd) == 0
    blk.freeze()
    assert blk.integrate(vd) == 0
    m = BlockMesher(blk, case["anchor"], case["voxel"], 64, 64)
    assert m.plan() == 0 and m.emit() == 0
    torch.cuda.synchronize()
    state = lambda: {"table": blk.buf.cpu(), "rc": blk.rc.cpu(), "ic": blk.ic.cpu(), "keys": blk.keys.cpu(), "nbr": blk.nbr.cpu(), "tw": blk.tw.cpu().view(torch.int32),
                     "rw": blk.rw.cpu().view(torch.int32), "work": m.buf.cpu(), "rows": m.rows.cpu(), "tris": m.tris.cpu(), "mc": m.counters.cpu()}
    before = state()
    nan, inf = float("nan"), float("inf")
    lib = _lib()
    big = (1 << 21) + 1
    common = {**pcases.view_faults(vd["pose"].data_ptr()), "NULL depth": dict(depth=None),
              "NULL anchor": dict(anchor=None), "voxel = 0": dict(voxel=0.0), "voxel NaN": dict(voxel=nan), "voxel inf": dict(voxel=inf), "trunc = 0": dict(trunc=0.0),
              "trunc NaN": dict(trunc=nan), "trunc inf": dict(trunc=inf), "trunc > 16 voxel": dict(trunc=16.5 * case["voxel"]), "anchor NaN": dict(anchor=[0.0, nan, 0.0]),
              "anchor inf": dict(anchor=[inf, 0.0, 0.0]), "fy NaN": dict(fy=nan),
              "misaligned depth": dict(depth=vd["depth"].data_ptr() + 1), "misaligned sil": dict(sil=vd["depth"].data_ptr() + 2)}
    bad_reserve = dict(common, **{"max_blocks = 0": dict(max_blocks=0), "max_blocks above 2^21": dict(max_blocks=big), "NULL table": dict(table=None), "NULL counters": dict(rc=None),
                                  "misaligned table": dict(table=blk.table + 4), "misaligned counters": dict(rc=blk.rc.data_ptr() + 4)})
    for what, over in bad_reserve.items():
        assert blk.reserve(vd, **over) == -1, what
        assert lib.mm3dgs_last_error(), what
    bad_integrate = dict(common, **{"n = 0": dict(n=0), "n above 2^21": dict(n=big), "NULL color": dict(color=None), "NULL keys": dict(keys=None), "NULL tsdf_w": dict(tsdf_w=None),
                                    "NULL rgb_w": dict(rgb_w=None), "NULL counters": dict(ic=None), "misaligned color": dict(color=vd["color"].data_ptr() + 2),
                                    "misaligned keys": dict(keys=blk.keys.data_ptr() + 4), "misaligned tsdf_w": dict(tsdf_w=blk.tw.data_ptr() + 4),
                                    "misaligned rgb_w": dict(rgb_w=blk.rw.data_ptr() + 8), "misaligned counters": dict(ic=blk.ic.data_ptr() + 4)})
    for what, over in bad_integrate.items():
        assert blk.integrate(vd, **over) == -1, what
        assert lib.mm3dgs_last_error(), what
    S, T, K = _stream(), blk.table, blk.keys
    for what, rc in {
        "reset max_blocks = 0": lib.mm3dgs_tsdf_blocks_reset(_ptr(T), 0, _ptr(blk.rc), S), "reset max_blocks above 2^21": lib.mm3dgs_tsdf_blocks_reset(_ptr(T), big, _ptr(blk.rc), S),
        "reset NULL table": lib.mm3dgs_tsdf_blocks_reset(None, 64, _ptr(blk.rc), S), "reset NULL counters": lib.mm3dgs_tsdf_blocks_reset(_ptr(T), 64, None, S),
        "reset misaligned table": lib.mm3dgs_tsdf_blocks_reset(_ptr(T + 4), 64, _ptr(blk.rc), S),
        "list max_blocks = 0": lib.mm3dgs_tsdf_blocks_list(_ptr(T), 0, _ptr(K), 8, S), "list NULL table": lib.mm3dgs_tsdf_blocks_list(None, 64, _ptr(K), 8, S),
        "list NULL keys": lib.mm3dgs_tsdf_blocks_list(_ptr(T), 64, None, 8, S), "list misaligned keys": lib.mm3dgs_tsdf_blocks_list(_ptr(T), 64, _ptr(K.data_ptr() + 4), 8, S),
        "index n = 0": lib.mm3dgs_tsdf_blocks_index(_ptr(T), 64, _ptr(K), 0, _ptr(blk.nbr), _ptr(blk.rc), S),
        "index n above 2^21": lib.mm3dgs_tsdf_blocks_index(_ptr(T), 64, _ptr(K), big, _ptr(blk.nbr), _ptr(blk.rc), S),
        "index max_blocks = 0": lib.mm3dgs_tsdf_blocks_index(_ptr(T), 0, _ptr(K), blk.n, _ptr(blk.nbr), _ptr(blk.rc), S),
        "index NULL keys": lib.mm3dgs_tsdf_blocks_index(_ptr(T), 64, None, blk.n, _ptr(blk.nbr), _ptr(blk.rc), S),
        "index NULL neighbours": lib.mm3dgs_tsdf_blocks_index(_ptr(T), 64, _ptr(K), blk.n, None, _ptr(blk.rc), S),
        "index NULL counters": lib.mm3dgs_tsdf_blocks_index(_ptr(T), 64, _ptr(K), blk.n, _ptr(blk.nbr), None, S),
        "index misaligned neighbours": lib.mm3dgs_tsdf_blocks_index(_ptr(T), 64, _ptr(K), blk.n, _ptr(blk.nbr.data_ptr() + 2), _ptr(blk.rc), S),
        "index misaligned keys": lib.mm3dgs_tsdf_blocks_index(_ptr(T), 64, _ptr(K.data_ptr() + 4), blk.n, _ptr(blk.nbr), _ptr(blk.rc), S),
    }.items():
        assert rc == -1, what
    bad_plan = {"n = 0": dict(n=0), "n above 2^21": dict(n=big), "NULL neighbours": dict(nbr=None), "NULL tsdf_w": dict(tsdf_w=None), "NULL work": dict(work=None),
                "NULL counters": dict(counters=None), "min_weight NaN": dict(min_weight=nan), "misaligned tsdf_w": dict(tsdf_w=blk.tw.data_ptr() + 4),
                "misaligned work": dict(work=m.work + 4), "misaligned neighbours": dict(nbr=blk.nbr.data_ptr() + 2), "misaligned counters": dict(counters=m.counters.data_ptr() + 4)}
    for what, over in bad_plan.items():
        assert m.plan(**over) == -1, what
        assert lib.mm3dgs_last_error(), what
    bad_emit = {"n = 0": dict(n=0), "n above 2^21": dict(n=big), "NULL keys": dict(keys=None), "NULL neighbours": dict(nbr=None), "NULL tsdf_w": dict(tsdf_w=None),
                "NULL rgb_w": dict(rgb_w=None), "NULL anchor": dict(anchor=None), "NULL work": dict(work=None), "NULL rows": dict(rows=None), "NULL triangles": dict(tris=None),
                "NULL counters": dict(counters=None), "voxel = 0": dict(voxel=0.0), "voxel NaN": dict(voxel=nan), "anchor NaN": dict(anchor=_vec([nan, 0, 0])),
                "misaligned rows": dict(rows=m.rows.data_ptr() + 8), "misaligned rgb_w": dict(rgb_w=blk.rw.data_ptr() + 8), "misaligned keys": dict(keys=blk.keys.data_ptr() + 4),
                "misaligned work": dict(work=m.work + 4), "misaligned triangles": dict(tris=m.tris.data_ptr() + 2), "misaligned counters": dict(counters=m.counters.data_ptr() + 4)}
    for what, over in bad_emit.items():
        assert m.emit(**over) == -1, what
        assert lib.mm3dgs_last_error(), what
    torch.cuda.synchronize()
    now = state()
    for name, t in before.items():
        assert torch.equal(now[name], t), name
    assert int(lib.mm3dgs_tsdf_blocks_table_bytes(0)) == 0 and int(lib.mm3dgs_tsdf_blocks_table_bytes(big)) == 0 and int(lib.mm3dgs_tsdf_blocks_mesh_work_bytes(0)) == 0
    assert blk.reserve(vd) == 0 and blk.reserve(vd, sil=None) == 0 and blk.integrate(vd) == 0 and m.plan() == 0 and m.emit() == 0      # the same calls, unharmed


@pytest.mark.parametrize("who", ("tsdf_blocks_reserve", "tsdf_blocks_integrate"))
def test_view_fault_texts(who):
    case = sc.sphere_case(0.04, False, n_views=1)
    vd = to_dev(case["views"][0])
    blk = Blocks(case, 64)
    assert blk.reserve(vd) == 0
    blk.freeze()
    call = blk.reserve if who == "tsdf_blocks_reserve" else blk.integrate
    H, W = vd["depth"].shape
    for over, text in pcases.view_fault_texts(who, H, W, vd["pose"].data_ptr(), "the images and the pose must be 4-byte aligned"):
        assert call(vd, **over) == -1 and _lib().mm3dgs_last_error().decode() == text, over


# ---- 7. the export of a native-loop run ------------------------------------------------------------------------------------------------------
PARENT_KEYS = ["pose_est", "pose_gt", "keyframes", "ate_rmse", "psnr_list", "ssim_list", "lpips_list"]
MESH = {"voxel": 0.08}


def _run(tmp, volume, frames=4):
    """The small native run of tests/test_gpu_mesh.py::_run (48 x 64, 4 frames) with the mesh export on and `mesh.volume` as given."""
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    torch.manual_seed(0); random.seed(0); np.random.seed(0)
    mesh = dict(MESH, export=True) if volume is None else dict(MESH, export=True, volume=volume)
    cfg = default_config(device=DEV, height=48, width=64, tracking={"iters": 5}, mapping={"iters": 6, "kf_every": 2, "min_covisibility": 2.0},
                         outputdir=str(tmp), debug={"get_runtime_stats": False, "create_video": False, "save_keyframes": False},
                         eval_every=1, eval_on_device=False, mesh=mesh)
    seq = SyntheticSequence(cfg, frames, 2000, seed=5)
    slam = SLAM(cfg, seq)
    from mm3dgs_slam_amd.fused import FusedMapper, FusedTracker
    assert isinstance(slam.tracker, FusedTracker) and isinstance(slam.mapper, FusedMapper)
    slam.run()
    return slam, seq, cfg


def test_native_run_exports_its_mesh_through_the_sparse_volume(tmp_path):
    from tests.test_gpu_mesh import _same
    n = 4
    on_dir, off_dir = tmp_path / "sparse", tmp_path / "dense"
    on, _, cfg_on = _run(on_dir, "sparse", n)
    off, _, _ = _run(off_dir, None, n)
    a = np.load(on_dir / "results.npz", allow_pickle=True)
    b = np.load(off_dir / "results.npz", allow_pickle=True)
    assert list(a.keys()) == list(b.keys()) == PARENT_KEYS
    for key in PARENT_KEYS:
        assert _same(a[key], b[key]), key
    assert all(torch.equal(p, q) for p, q in zip(on.estimate_pose_list, off.estimate_pose_list))
    out, dense = on.mesh_export, off.mesh_export
    c, cd = out["counters"], dense["counters"]
    rows, tris = ms.read_mesh_ply(out["mesh"])
    print(f"MESHERR sparse run: {c}, lattice {out['lattice']} at {out['origin']}; dense {cd['vertices']} / {cd['triangles']} over {dense['lattice']}")
    assert out["volume"] == "sparse" and "volume" not in dense and c["views"] == 2 and len(rows) == c["vertices"] > 0 and len(tris) == c["triangles"] > 0
    assert out["volume_bytes"] == c["blocks"] * 512 * 24 < 24 * int(np.prod(dense["lattice"]))
    topo = ms.mesh_topology(len(rows), tris)
    assert topo["unreferenced"] == 0 and topo["repeated"] == 0
    # by hand on the host over the lattice the export reports: the same views, reserved and integrated by the host statement
    cam = {k: cfg_on["cam"][k] for k in ("fx", "fy", "cx", "cy")}
    first = np.round(np.asarray(out["origin"]) / out["voxel"]).astype(np.int64)
    nx, ny, nz = out["lattice"]
    tsdf_w, rgb_w = ms.empty_volume(nx, ny, nz)
    keys = np.zeros(0, dtype=np.int64)
    with torch.no_grad():
        for idx in (0, 2):
            pose = torch.tensor(a["pose_est"][idx], device=DEV)
            r = on.renderer.render(on.gaussians, camera_pose=pose)
            keys = np.union1d(keys, ms.reserve_host(r["depth"][0], r["depth"][1], pose, **cam, voxel=out["voxel"], trunc=out["trunc"], sil_min=0.99)[0])
            ms.integrate_host(tsdf_w, rgb_w, r["render"], r["depth"][0], r["depth"][1], pose, **cam, origin=(0, 0, 0), voxel=out["voxel"], trunc=out["trunc"], sil_min=0.99, first=first)
    assert len(keys) == c["blocks"]
    blocks = ms.key_blocks(keys)
    assert np.array_equal(8 * blocks.min(0), first) and [int(v) for v in 8 * (blocks.max(0) - blocks.min(0) + 1)] == list(out["lattice"])
    un = ms.mesh_host(tsdf_w, rgb_w, (0, 0, 0), out["voxel"], 1.0, first=first)
    reserved = (ms.pool_index(blocks, first, [nx, ny, nz], np.arange(nx * ny * nz)) >= 0).reshape(nz, ny, nx)
    tsdf_w[~reserved] = 0
    rgb_w[~reserved] = 0
    mrows, mtris, _, vq, tq = ms.mesh_host(tsdf_w, rgb_w, (0, 0, 0), out["voxel"], 1.0, first=first, where=True)
    want_rows, want_tris, _ = ms.reorder_to_blocks(mrows, mtris, vq, tq, blocks, first, [nx, ny, nz])
    print(f"MESHERR sparse run: host statement over the same views, masked {len(want_rows)} / {len(want_tris)}, unmasked {len(un[0])} / {len(un[1])}: "
          f"{len(un[1]) - len(want_tris)} triangles of cubes that touch an unreserved block; the dense export {cd['vertices']} / {cd['triangles']}")
    assert len(want_rows) == len(rows) and np.array_equal(want_tris, tris)
    assert len(un[1]) >= len(tris)
    # the same export again: the same file
    again = on.export_mesh(path=str(tmp_path / "again"))
    assert (tmp_path / "again" / "mesh.ply").read_bytes() == (on_dir / "mesh" / "mesh.ply").read_bytes() and again["counters"] == c
    cfg_on["mesh"]["max_blocks"] = 8
    with pytest.raises(ValueError, match=r"mesh\.max_blocks = 8"):
        on.export_mesh()
