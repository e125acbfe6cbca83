"""tests/surgery_ref.py (the float64 host statement of csrc/compact.hip's kernels) against the torch path -- GaussianModel on the CPU through
prune and _densify_torch, Mapper.covisibility_ratio_dense -- and the fixtures G7 and G12; and the generators of tests/surgery_cases.py
against the margin rule.  CPU only.  What tests/test_gpu_surgery.py then holds the kernels to is this statement."""
import os

import numpy as np
import pytest
import torch

from tests import densify_util as du
from tests import surgery_cases as cases
from tests import surgery_ref as ref
from tests import test_gpu_surgery as tg

MOVED_CAP = 0.01


def _model(arrays, moments, grad_accum, denom, radii, n_rest, percent_dense=0.01):
    a = {"in_" + k: v for k, v in arrays.items()}
    a["in_f_dc"], a["in_f_rest"] = arrays["f_dc"].reshape(-1, 1, 3), arrays["f_rest"].reshape(-1, n_rest, 3)
    for k, (m, v) in moments.items():
        a["in_m_" + k], a["in_v_" + k] = m.reshape(a["in_" + k].shape), v.reshape(a["in_" + k].shape)
    a["in_grad_accum"], a["in_denom"], a["in_max_radii2D"] = grad_accum.reshape(-1, 1), denom.reshape(-1, 1), radii
    sh = {0: 0, 3: 1, 15: 3}[n_rest]
    return du.model_from_arrays(a, "in_", "cpu", sh, percent_dense)


def _flat(s):
    return {k: (v.reshape(v.shape[0], -1) if isinstance(v, np.ndarray) and v.ndim > 1 else v) for k, v in s.items()}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- prune + compaction -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_radii", [True, False])
def test_prune_and_compaction_equal_the_torch_path_on_random_rows_and_every_nan_row(use_radii):
    P, n_rest = 300, 3
    opacity, scales, radii, placed = cases.prune_rows(P)
    arrays, grad_accum, denom, _ = cases.densify_rows(P, "mix", n_rest=n_rest)
    arrays["opacity"], arrays["scaling"] = opacity, scales
    moments = cases.densify_moments(arrays, ("xyz", "f_dc", "opacity", "scaling", "rotation"))
    keep, margin = ref.prune_keep(opacity, scales, radii if use_radii else None, cases.MIN_OPACITY, cases.MAX_SCALE, cases.MAX_SCREEN)
    assert int(((margin < ref.MARGIN) & ~placed).sum()) == 0
    g = _model(arrays, moments, grad_accum, denom, radii, n_rest)
    mask = g.prune(cases.MIN_OPACITY, cases.MAX_SCALE / 0.1, cases.MAX_SCREEN if use_radii else None).numpy()
    assert np.array_equal(mask, keep == 0)
    # the NaN rows one by one, as the torch path decides them (rows 5 ..: cases.PRUNE_PLACED)
    want = [1, 1, 1, 1, 1, 0, 1, 0, 1, 0] if use_radii else [1, 1, 1, 1, 1, 0, 1, 0, 1, 1]
    assert keep[5:5 + len(want)].tolist() == want and keep[-1] == 1
    assert 30 < int(mask.sum()) < P - 30
    s = _flat(du.state(g))
    names = list(ref.GROUPS) + ["m_" + k for k in moments] + ["v_" + k for k in moments]
    src = [arrays[k] for k in ref.GROUPS] + [moments[k][0] for k in moments] + [moments[k][1] for k in moments]
    out, n = ref.compact(keep, src + [grad_accum, denom, radii])
    assert n == P - int(mask.sum())
    for name, o in zip(names + ["grad_accum", "denom", "max_radii2D"], out):
        assert np.array_equal(_bits(s[name].reshape(o.shape)), _bits(o)), name
    # the float32 evaluation takes the same decisions away from the thresholds
    assert np.array_equal(ref.prune_keep(opacity, scales, radii if use_radii else None, cases.MIN_OPACITY, cases.MAX_SCALE, cases.MAX_SCREEN,
                                         dtype=np.float32)[0], keep)


def test_nan_scale_rows_are_kept_by_torch_in_every_position():
    """What the prune kernel has to follow: torch.max propagates a NaN and the comparison with it is false."""
    for s in ((np.nan, 5.0, 0.0), (5.0, np.nan, 0.0), (0.0, 1.0, np.nan)):
        t = torch.tensor([s])
        assert not bool((torch.exp(t).max(dim=1).values > 0.13).any())
        keep, margin = ref.prune_keep(np.float32([[1.0]]), np.float32([s]), None, 0.005, 0.13, 100.0)
        assert keep.tolist() == [1] and margin[0] > 0.9
        # a maximum that drops the NaN (fmaxf) prunes the row: the divergence the kernel had
        assert float(np.exp(np.nanmax(np.float32(s)))) > 0.13


@pytest.mark.parametrize("n", cases.SIZES)
def test_prune_generator_meets_the_margin_cap(n):
    opacity, scales, radii, placed = cases.prune_rows(n)
    for r in (radii, None):
        keep, margin = ref.prune_keep(opacity, scales, r, cases.MIN_OPACITY, cases.MAX_SCALE, cases.MAX_SCREEN)
        assert int(((margin < ref.MARGIN) & ~placed).sum()) <= MOVED_CAP * n
        if n >= 63:
            assert 0 < int(keep.sum()) < n


def test_block_prefix_and_compact():
    keep = cases.keep_bytes(700, "bytes")
    pre, total = ref.block_prefix(keep)
    k = keep != 0
    assert pre.tolist() == [0, int(k[:256].sum()), int(k[:512].sum())] and total == int(k.sum())
    (a,), n = ref.compact(keep, [np.arange(700)])
    assert n == total and a.tolist() == np.nonzero(k)[0].tolist()
    pre, total = ref.block_prefix(np.zeros(0, np.uint8))
    assert pre.shape == (0,) and total == 0


# ---- densification ----------------------------------------------------------------------------------------------------------------
def _child_bars(out64, out32):
    d_xyz, d_s = ref.deviation(out32["child_xyz"], out64["child_xyz"]), ref.deviation(out32["child_scaling"], out64["child_scaling"])
    return d_xyz, d_s


@pytest.mark.parametrize("N", [1, 2, 3])
def test_densification_equals_the_torch_path_on_random_rows(N):
    P, n_rest, seed = 300, 3, 4242 + N
    arrays, grad_accum, denom, placed = cases.densify_rows(P, "mix", n_rest=n_rest)
    moments = cases.densify_moments(arrays, ("xyz", "f_dc", "opacity", "scaling", "rotation"))      # f_rest and rgb: groups without Adam state
    cls, margin = ref.densify_classes(grad_accum, denom, arrays["scaling"], cases.MAX_GRAD, cases.MAX_CLONE_SCALE)
    assert int(((margin < ref.MARGIN) & ~placed).sum()) == 0
    assert cls[7:13].tolist() == [0, 0, 1, 0, 2, 1]              # the rows placed by hand (cases.densify_rows)
    assert np.array_equal(ref.densify_classes(grad_accum, denom, arrays["scaling"], cases.MAX_GRAD, cases.MAX_CLONE_SCALE, dtype=np.float32)[0], cls)
    out = ref.densify(arrays, moments, cls, N, seed)
    out32 = ref.densify(arrays, moments, cls, N, seed, dtype=np.float32)
    g = _model(arrays, moments, grad_accum, denom, np.ones(P, np.float32), n_rest, percent_dense=0.01)
    parent = g._densify_torch(cases.MAX_GRAD, cases.MAX_CLONE_SCALE / 0.01, seed, N=N).numpy()
    assert min(out["n_clone"], out["n_split"], out["n_keep"] - out["n_clone"]) > 30
    assert np.array_equal(parent, out["parent"])
    s = _flat(du.state(g))
    child = out["child"]
    d_xyz, d_s = _child_bars(out, out32)
    for name in ref.GROUPS:
        got = s[name].reshape(out[name].shape)
        if name in ("xyz", "scaling"):
            assert np.array_equal(_bits(got[~child]), _bits(out[name][~child])), name
            want, d = out["child_" + name], d_xyz if name == "xyz" else d_s
            err = np.abs(got[child].astype(np.float64) - want)
            assert bool((err <= 4 * d * (1 + np.abs(want))).all()), (name, float(err.max()), d)
        else:
            assert np.array_equal(_bits(got), _bits(out[name])), name
        if name in moments:
            for tag in ("m_", "v_"):
                assert np.array_equal(_bits(s[tag + name].reshape(out[tag + name].shape)), _bits(out[tag + name])), tag + name
            assert not out["m_" + name][out["n_keep"]:].any() and out["m_" + name][:out["n_keep"]].any()
        else:
            assert "m_" + name not in s
    for k in ("grad_accum", "denom", "max_radii2D"):
        assert s[k].shape[0] == out["n"] and not s[k].any() and not out[k].any()


@pytest.mark.parametrize("P,mix", [(P, mix) for P in cases.SIZES for mix in cases.DENSIFY_MIXES])
def test_densify_generator_meets_the_margin_cap_and_gives_its_mix(P, mix):
    arrays, grad_accum, denom, placed = cases.densify_rows(P, mix, n_rest=cases.densify_run(P, mix)["n_rest"])
    cls, margin = ref.densify_classes(grad_accum, denom, arrays["scaling"], cases.MAX_GRAD, cases.MAX_CLONE_SCALE)
    assert int(((margin < ref.MARGIN) & ~placed).sum()) <= MOVED_CAP * P
    n = [int((cls == c).sum()) for c in range(3)]
    if mix == "none":
        assert n == [P, 0, 0]
    elif mix == "all_clone":
        assert n == [0, P, 0]
    elif mix == "all_split":
        assert n == [0, 0, P]
    elif mix == "split_last":
        assert cls[-1] == ref.SPLIT and not (cls[:256 * ((P - 1) // 256)] == ref.SPLIT).any()
    elif P >= 63:
        assert min(n) > 0


def test_fixture_g12_prune_and_densify():
    """The statement on the reference's own densify_and_prune output (G12), and against the torch path on the same inputs."""
    f = du.load()
    N, seed = int(f["N"]), int(f["seed"])
    arrays = {k: f["in_" + k].reshape(f["in_" + k].shape[0], -1) for k in ref.GROUPS}
    moments = {k: (f["in_m_" + k], f["in_v_" + k]) for k in ref.GROUPS}
    th = float(np.float32(f["percent_dense"]) * np.float32(f["extent"]))
    cls, _ = ref.densify_classes(f["in_grad_accum"], f["in_denom"], f["in_scaling"], float(f["grad_threshold"]), th)
    assert np.array_equal(np.nonzero(cls == ref.SPLIT)[0], f["split_rows"])
    out = ref.densify(arrays, moments, cls, N, seed)
    out32 = ref.densify(arrays, moments, cls, N, seed, dtype=np.float32)
    # prune of the densified map: the statistics are zero, so the screen clause cannot fire
    xyz, scaling = out["xyz"].astype(np.float64), out["scaling"].astype(np.float64)
    xyz[out["child"]], scaling[out["child"]] = out["child_xyz"], out["child_scaling"]
    keep, _ = ref.prune_keep(out["opacity"], scaling.astype(np.float32), out["max_radii2D"], float(f["min_opacity"]), 0.1 * float(f["extent"]),
                             float(f["max_screen_size"]))
    assert np.array_equal(keep == 0, f["out_prune_mask"])
    k = keep != 0
    assert np.array_equal(out["parent"][k], f["out_parent"])
    child = out["child"][k]
    assert np.array_equal(child, du.child_rows(f))
    d_xyz, d_s = _child_bars(out, out32)
    for name in ref.GROUPS:
        want, got = f["out_" + name].reshape(int(k.sum()), -1), out[name][k]
        if name in ("xyz", "scaling"):
            assert np.array_equal(_bits(got[~child]), _bits(want[~child])), name
            mine, d = (xyz if name == "xyz" else scaling)[k][child], d_xyz if name == "xyz" else d_s
            assert bool((np.abs(mine - want[child]) <= 4 * d * (1 + np.abs(mine))).all()), name
        else:
            assert np.array_equal(_bits(got), _bits(want)), name
        for tag in ("m_", "v_"):
            assert np.array_equal(_bits(out[tag + name][k]), _bits(f["out_" + tag + name].reshape(int(k.sum()), -1))), tag + name
    # the torch path on the same inputs
    g = du.model_from_fixture(f, "cpu")
    mask, parent = du.densify_fixture(g, f)
    assert np.array_equal(mask, keep == 0) and np.array_equal(parent, out["parent"])
    # the prune alone, on the fixture's inputs (radii clause on)
    g = du.model_from_fixture(f, "cpu")
    keep_in, _ = ref.prune_keep(f["in_opacity"], f["in_scaling"], f["in_max_radii2D"], float(f["min_opacity"]), 0.1 * float(f["extent"]),
                                float(f["max_screen_size"]))
    mask = g.prune(float(f["min_opacity"]), float(f["extent"]), float(f["max_screen_size"])).numpy()
    assert np.array_equal(mask, keep_in == 0) and 0 < int(mask.sum()) < mask.shape[0]
    (xyz_kept,), _ = ref.compact(keep_in, [f["in_xyz"]])
    assert np.array_equal(_bits(g._xyz.detach().numpy()), _bits(xyz_kept))


# ---- seeding ----------------------------------------------------------------------------------------------------------------------
def test_fixture_g7_seeding():
    from mm3dgs_slam_amd.sh_utils import RGB2SH
    d = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "g7_seed.npz")))
    fx, fy, cx, cy = (float(v) for v in d["intr"])
    for dtype in (np.float64, np.float32):
        s = ref.seed(d["color"], d["depth"], d["depth"] > 0, d["pose"], fx, fy, cx, cy, 0, dtype=dtype)
        n = d["cld"].shape[0]
        assert s["xyz"].shape == (n, 3)
        assert float(np.abs(s["xyz"] - d["cld"][:, :3]).max()) < 2e-5
        assert float(np.abs(s["scaling"] - d["log_scale"][:, None]).max()) < 2e-6
        assert float(np.abs(s["f_dc"] - RGB2SH(torch.from_numpy(d["cld"][:, 3:6])).numpy()).max()) < 1e-6
        assert np.array_equal(_bits(s["rgb"]), _bits(d["cld"][:, 3:6]))
        assert not s["opacity"].any() and s["rotation"].tolist() == [[1.0, 0.0, 0.0, 0.0]] * n and s["f_rest"].shape == (n, 0)


@pytest.mark.parametrize("H,W", cases.SEED_SHAPES)
def test_seed_inputs_deviate_by_no_more_than_the_stated_float32_noise(H, W):
    c = cases.seed_case(H, W)
    a = [c[k] for k in ("color", "depth", "keep", "pose", "fx", "fy", "cx", "cy")]
    s64, s32 = ref.seed(*a, 0), ref.seed(*a, 0, dtype=np.float32)
    assert s64["xyz"].shape[0] == int(c["keep"].sum()) and c["keep"][0] and c["keep"][-1]
    assert ref.deviation(s32["xyz"], s64["xyz"]) <= tg.DEV_SEED_XYZ
    assert ref.deviation(s32["scaling"], s64["scaling"]) <= tg.DEV_SEED_SCALING


@pytest.mark.parametrize("P,mix,N", cases.DENSIFY_RUNS)
def test_densify_inputs_deviate_by_no_more_than_the_stated_float32_noise(P, mix, N):
    arrays, grad_accum, denom, placed = cases.densify_rows(P, mix, n_rest=cases.densify_run(P, mix)["n_rest"])
    cls, margin = ref.densify_classes(grad_accum, denom, arrays["scaling"], cases.MAX_GRAD, cases.MAX_CLONE_SCALE)
    assert not ((margin < ref.MARGIN) & ~placed).any()          # (nothing moves: these are the arrays the GPU test runs)
    d_xyz, d_s = _child_bars(ref.densify(arrays, {}, cls, N, cases.DENSIFY_SEED), ref.densify(arrays, {}, cls, N, cases.DENSIFY_SEED, dtype=np.float32))
    assert d_xyz <= tg.DEV_CHILD_XYZ and d_s <= tg.DEV_CHILD_SCALING, (d_xyz, d_s)


# ---- covisibility -----------------------------------------------------------------------------------------------------------------
def _torch_counts(c):
    """(ratio of Mapper.covisibility_ratio_dense, number of points it tests -- its own selection, restated with its own operators)."""
    from mm3dgs_slam_amd.mapper import Mapper
    from mm3dgs_slam_amd.pose_utils import apply_rigid, get_camera_from_tensor, rigid_inverse
    m = Mapper.__new__(Mapper)
    m.cfg = {"cam": {k: c[k] for k in ("fx", "fy", "cx", "cy")}}
    depth, sil, kp, cp = (torch.from_numpy(c[k]) for k in ("depth", "sil", "kf_pose", "cur_pose"))
    ratio = float(m.covisibility_ratio_dense(depth, sil, kp, cp))
    u, v = m._pix_grid
    z = torch.where(sil > 0.99, depth, torch.zeros_like(depth)).reshape(-1)
    cam = torch.stack(((u - c["cx"]) / c["fx"] * z, (v - c["cy"]) / c["fy"] * z, z), -1)
    pts = apply_rigid(cam, rigid_inverse(get_camera_from_tensor(kp)))
    return ratio, int(((z > 0) & (torch.round(pts, decimals=4).abs().sum(1) > 0)).sum())


@pytest.mark.parametrize("view", cases.COVIS_VIEWS)
@pytest.mark.parametrize("H,W", cases.COVIS_SHAPES)
def test_covisibility_counts_equal_the_torch_formulation_and_the_generator_meets_the_cap(H, W, view):
    for plain in (False, True):
        c = cases.covis_case(H, W, view, plain=plain)
        a = lambda: [c[k] for k in ("depth", "sil", "kf_pose", "cur_pose", "fx", "fy", "cx", "cy")]
        _, margin = ref.covisibility(*a())
        moved = ref.move_covisibility_pixels(c["sil"], margin, c["placed"])
        assert moved <= MOVED_CAP * H * W, moved
        (n_in, n_sel), margin = ref.covisibility(*a())
        assert int(((margin < ref.MARGIN) & ~c["placed"].reshape(-1)).sum()) == 0
        assert ref.covisibility(*a(), dtype=np.float32)[0] == (n_in, n_sel)
        ratio, n_sel_torch = _torch_counts(c)
        assert n_sel == n_sel_torch
        assert ratio == float(torch.tensor(n_in) / torch.tensor(n_sel).clamp_min(1)), (ratio, n_in, n_sel)
        surface = int(((c["sil"] > 0.99) & (c["depth"] > 0)).sum())
        if plain:
            assert n_sel == surface == H * W - moved
        elif H * W > 1:
            assert n_sel == surface - 1 and surface < H * W          # the point at the world origin is a surface point that is not tested
        else:
            assert (n_in, n_sel) == (0, 0)                          # the lone pixel is the point at the origin
        if view == "keeps_all":
            assert n_in == n_sel
        elif view == "behind":
            assert n_in == 0
        elif H * W >= 255:
            assert 0.3 * n_sel < n_in < 0.7 * n_sel
