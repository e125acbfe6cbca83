"""TEST INFRASTRUCTURE: the host statement of the map-surgery kernels (csrc/compact.hip) -- the prune predicate, order-preserving
compaction, seeding from an RGB-D frame, densification (classes, row placement, split children) and the keyframe test's covisibility
counters -- in numpy, float64 by default, from the float32 inputs the kernels read.  No torch autograd, no GPU; never imported by the
product.  tests/test_surgery_ref.py holds it to the torch path (GaussianModel on the CPU, Mapper.covisibility_ratio_dense) and to the
fixtures G7 and G12; tests/test_gpu_surgery.py holds the kernels to it.

Every function takes ``dtype`` (np.float64, or np.float32: the same statement evaluated in the kernels' precision).  The difference
of the two evaluations is what the tolerances of the computed values are measured against (``deviation``).

Decisions (prune, class, inside / selected) are compared exactly by the tests, so each deciding function also returns a margin per
element: the smallest relative distance of a compared quantity from its threshold.  A test moves the elements whose margin is below
MARGIN out of the way (``move_*``) before it runs a kernel, and the generators are chosen so that fewer than 1 % have to move."""
import numpy as np
import torch

from mm3dgs_slam_amd.general_utils import densify_keys

C0 = 0.28209479177387814                  # sh_utils.C0
TWO_PI_F32 = float(np.float32(6.28318548))
MARGIN = 1e-4
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "rgb")
KEEP, CLONE, SPLIT = 0, 1, 2


def _quiet():
    return np.errstate(all="ignore")


def _rel(value, threshold):
    """|value - threshold| relative to the threshold (absolute at a zero threshold); a NaN never sits on a threshold: inf."""
    d = np.abs(np.asarray(value, np.float64) - float(threshold)) / (abs(float(threshold)) if threshold != 0 else 1.0)
    return np.where(np.isnan(d), np.inf, d)


def _max_nan(x):
    """Row maximum with torch.max's rule: a NaN wins (np.max propagates it too)."""
    return np.max(x, axis=1)


def deviation(f32, f64):
    """The largest difference of the float32 from the float64 evaluation in the form abs + rel |value| with abs = rel = D:
    D = max |f32 - f64| / (1 + |f64|).  A bar of k D allows k D (1 + |value|)."""
    f32, f64 = np.asarray(f32, np.float64), np.asarray(f64, np.float64)
    return float((np.abs(f32 - f64) / (1.0 + np.abs(f64))).max()) if f64.size else 0.0


def _rotation(q, dtype):
    """R(q / |q|) for quaternions (w, x, y, z) [..., 4] -> [..., 3, 3]."""
    q = np.asarray(q).astype(dtype)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    one, two = dtype(1), dtype(2)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                  two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                  two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


# ---- prune ------------------------------------------------------------------------------------------------------------------------
def prune_keep(opacity, log_scales, radii_or_none, min_opacity, max_scale, max_screen, dtype=np.float64):
    """(keep uint8 [P], margin float64 [P]).  Pruned: sigmoid(o) < min_opacity || max_k exp(s_k) > max_scale || radius > max_screen
    (the last only with radii).  The thresholds are the float32 values the C ABI carries.  A NaN makes its clause false, as in torch:
    in any scale component (torch.max propagates it), in the opacity, in the radius."""
    min_opacity, max_scale, max_screen = (dtype(np.float32(v)) for v in (min_opacity, max_scale, max_screen))
    with _quiet():
        o = np.asarray(opacity).reshape(-1).astype(dtype)
        sig = dtype(1) / (dtype(1) + np.exp(-o))
        smax = _max_nan(np.exp(np.asarray(log_scales).reshape(-1, 3).astype(dtype)))
        pruned = (sig < min_opacity) | (smax > max_scale)
        margin = np.minimum(_rel(sig, min_opacity), _rel(smax, max_scale))
        if radii_or_none is not None:
            r = np.asarray(radii_or_none).reshape(-1).astype(dtype)
            pruned |= r > max_screen
            margin = np.minimum(margin, _rel(r, max_screen))
    return (~pruned).astype(np.uint8), margin


def move_prune_rows(opacity, log_scales, radii_or_none, margin, placed, min_opacity, max_scale, max_screen):
    """Rows closer than MARGIN to a threshold (and not placed by hand) go to twice every threshold, in place.  Returns their number."""
    move = (margin < MARGIN) & ~placed
    opacity.reshape(-1)[move] = np.float32(np.log(2.0 * min_opacity / (1.0 - 2.0 * min_opacity)))
    log_scales.reshape(-1, 3)[move] = np.float32(np.log(2.0 * max_scale))
    if radii_or_none is not None:
        radii_or_none.reshape(-1)[move] = np.float32(2.0 * max_screen)
    return int(move.sum())


# ---- compaction -------------------------------------------------------------------------------------------------------------------
def compact(keep, arrays):
    """([a[keep != 0] for a in arrays], count): the rows whose keep byte is not zero, in order."""
    k = np.asarray(keep).reshape(-1) != 0
    return [np.asarray(a)[k] for a in arrays], int(k.sum())


def block_prefix(flags, block=256):
    """(exclusive prefix of the per-`block` counts of flags, total): what a plan leaves in its work buffer."""
    f = np.asarray(flags).reshape(-1) != 0
    nb = (f.shape[0] + block - 1) // block
    counts = np.add.reduceat(f.astype(np.int64), np.arange(0, nb * block, block)[:nb]) if f.shape[0] else np.zeros(0, np.int64)
    pre = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return pre[:-1].astype(np.uint32), int(pre[-1])


# ---- seeding ----------------------------------------------------------------------------------------------------------------------
def seed(color, depth, keep, pose7, fx, fy, cx, cy, n_rest, dtype=np.float64):
    """The rows of one new Gaussian per kept pixel, raster order: dict of xyz [n,3], f_dc [n,3], f_rest [n,3 n_rest], opacity [n,1],
    scaling [n,3], rotation [n,4], rgb [n,3].  x_w = R^T (x_c - t) with R of the normalised quaternion, x_c the back-projected pixel;
    log-scale log(z / ((fx + fy) / 2)); f_dc = (rgb - 0.5) / C0; opacity logit 0; identity rotation; zero f_rest."""
    H, W = np.asarray(depth).shape
    idx = np.nonzero(np.asarray(keep).reshape(-1))[0]
    n = idx.shape[0]
    fx, fy, cx, cy = (dtype(np.float32(v)) for v in (fx, fy, cx, cy))
    pose = np.asarray(pose7).astype(dtype)
    R, t = _rotation(pose[:4], dtype), pose[4:]
    u, v = (idx % W).astype(dtype), (idx // W).astype(dtype)
    z = np.asarray(depth).reshape(-1)[idx].astype(dtype)
    with _quiet():
        c = np.stack([(u - cx) / fx * z - t[0], (v - cy) / fy * z - t[1], z - t[2]], -1)
        xyz = c @ R                                          # (R^T c per row)
        ls = np.log(z / ((fx + fy) * dtype(0.5)))
    rgb = np.asarray(color).reshape(3, -1)[:, idx].T.astype(np.float32)
    rot = np.zeros((n, 4), np.float32)
    rot[:, 0] = 1.0
    return dict(xyz=xyz.astype(dtype), f_dc=(rgb.astype(dtype) - dtype(0.5)) / dtype(C0), f_rest=np.zeros((n, 3 * n_rest), np.float32),
                opacity=np.zeros((n, 1), np.float32), scaling=np.repeat(ls[:, None], 3, 1).astype(dtype), rotation=rot, rgb=rgb)


# ---- densification ----------------------------------------------------------------------------------------------------------------
def densify_classes(grad_accum, denom, log_scales, max_grad, max_clone_scale, dtype=np.float64):
    """(class uint8 [P], margin [P]).  g = grad_accum / denom with 0 / 0 -> 0 (any NaN -> 0); s = max_k exp(s_k), NaN wins; split if
    g >= max_grad and s > max_clone_scale, clone if g >= max_grad and s <= max_clone_scale, kept otherwise (a NaN s: kept)."""
    max_grad, max_clone_scale = dtype(np.float32(max_grad)), dtype(np.float32(max_clone_scale))
    with _quiet():
        g = np.asarray(grad_accum).reshape(-1).astype(dtype) / np.asarray(denom).reshape(-1).astype(dtype)
        g = np.where(np.isnan(g), dtype(0), g)
        s = _max_nan(np.exp(np.asarray(log_scales).reshape(-1, 3).astype(dtype)))
        sel = g >= max_grad
        cls = np.where(sel & (s > max_clone_scale), SPLIT, np.where(sel & (s <= max_clone_scale), CLONE, KEEP)).astype(np.uint8)
        margin = np.minimum(_rel(g, max_grad), _rel(s, max_clone_scale))
    return cls, margin


def move_densify_rows(grad_accum, denom, log_scales, margin, placed, max_grad, max_clone_scale):
    """Rows closer than MARGIN to a threshold (and not placed by hand) go to twice both thresholds, in place.  Returns their number."""
    move = (margin < MARGIN) & ~placed
    grad_accum.reshape(-1)[move] = np.float32(2.0 * max_grad)
    denom.reshape(-1)[move] = 1.0
    log_scales.reshape(-1, 3)[move] = np.float32(np.log(2.0 * max_clone_scale))
    return int(move.sum())


def densify(arrays, moments, classes, N, seed, dtype=np.float64):
    """The densified map in the order [kept rows (class < 2)][clones][child 0 of each split row] ... [child N-1].
    arrays: {group: [P, width]} (float32); moments: {group: (exp_avg, exp_avg_sq)} for the groups that have Adam state.
    Returns a dict with
      parent        int32 [n]: the source row of every output row
      n_keep, n_clone, n_split, n
      <group>       float32 [n, width]: the parent's row (exact copies; for xyz / scaling the children's rows are placeholders)
      m_<group>, v_<group>   float32: the parent's moments on the kept rows, zeros on every new row
      child         bool [n]: the split children
      child_xyz, child_scaling   dtype [N n_split, 3]: xyz = R(q / |q|) (exp(s) z) + xyz, scaling = log(exp(s) / (0.8 N)), with
                    z_a = sqrt(-2 ln u_2a) cos(u_2a+1 6.28318548f), u_j = ((key_j >> 8) + 0.5) 2^-24, key = general_utils.densify_keys
      grad_accum, denom, max_radii2D   zeros at the new length."""
    cls = np.asarray(classes).reshape(-1)
    P = cls.shape[0]
    ar = np.arange(P, dtype=np.int64)
    kept, clones, split = ar[cls < 2], ar[cls == CLONE], ar[cls == SPLIT]
    parent = np.concatenate([kept, clones, np.tile(split, N)])
    n = parent.shape[0]
    out = dict(parent=parent.astype(np.int32), n_keep=len(kept), n_clone=len(clones), n_split=len(split), n=n)
    new = np.arange(n) >= len(kept)
    out["child"] = np.arange(n) >= len(kept) + len(clones)
    for name in GROUPS:
        a = np.asarray(arrays[name])
        out[name] = a.reshape(P, -1)[parent]
        if name in moments:
            for tag, m in zip(("m_", "v_"), moments[name]):
                mm = np.asarray(m).reshape(P, -1)[parent]
                mm[new] = 0.0
                out[tag + name] = mm
    keys = densify_keys(int(seed), torch.from_numpy(split), N).numpy()              # [N, n_split, 6], exact integers
    with _quiet():
        u = ((keys >> 8).astype(dtype) + dtype(0.5)) * dtype(2.0 ** -24)
        zn = np.sqrt(dtype(-2) * np.log(u[..., 0::2])) * np.cos(u[..., 1::2] * dtype(TWO_PI_F32))      # [N, n_split, 3]
        sc = np.exp(np.asarray(arrays["scaling"]).reshape(P, 3)[split].astype(dtype))
        R = _rotation(np.asarray(arrays["rotation"]).reshape(P, 4)[split], dtype)
        xyz = np.asarray(arrays["xyz"]).reshape(P, 3)[split].astype(dtype)
        v = sc[None] * zn
        out["child_xyz"] = (np.einsum("sab,ksb->ksa", R, v) + xyz[None]).reshape(-1, 3).astype(dtype)
        out["child_scaling"] = np.tile(np.log(sc / dtype(0.8 * N)), (N, 1)).astype(dtype)
    out["grad_accum"], out["denom"], out["max_radii2D"] = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    return out


# ---- covisibility -----------------------------------------------------------------------------------------------------------------
def covisibility(depth, sil, kf_pose, cur_pose, fx, fy, cx, cy, dtype=np.float64):
    """((n_inside, n_selected), margin [H W]).  Surface points of the keyframe: z = depth where sil > 0.99 and z > 0, back-projected to
    the world (p_w = Rk^T (x_c - tk)), dropped where every |p_w| 1e4 <= 0.5 (they round to the origin at four decimals); selected points
    are projected into the current view (p = Rc p_w + tc, zc = p_z + 1e-5, uu = (fx p_x + cx p_z) / zc, vv alike) and counted inside
    where 0 < uu < W, 0 < vv < H and zc > 0.
    Margin: sil from 0.99 and z from 0 (a z of exactly 0 is decided without arithmetic: no margin); on a surface pixel also the largest
    |p_w| 1e4 from 0.5; on a selected one also uu from 0 and W (relative to W), vv from 0 and H (relative to H), zc from 0 (relative to
    the magnitudes it is summed from)."""
    H, W = np.asarray(depth).shape
    fx, fy, cx, cy = (dtype(np.float32(v)) for v in (fx, fy, cx, cy))
    thr = dtype(np.float32(0.99))
    kp, cp = np.asarray(kf_pose).astype(dtype), np.asarray(cur_pose).astype(dtype)
    Rk, tk, Rc, tc = _rotation(kp[:4], dtype), kp[4:], _rotation(cp[:4], dtype), cp[4:]
    s = np.asarray(sil).reshape(-1).astype(dtype)
    d = np.asarray(depth).reshape(-1).astype(dtype)
    i = np.arange(H * W)
    u, v = (i % W).astype(dtype), (i // W).astype(dtype)
    with _quiet():
        z = np.where(s > thr, d, dtype(0))
        surface = z > 0
        c = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1)
        pw = (c - tk) @ Rk
        far = np.abs(pw * dtype(10000)).max(1)
        sel = surface & (far > dtype(0.5))
        p = pw @ Rc.T + tc
        zc = p[:, 2] + dtype(np.float32(1e-5))
        uu, vv = (fx * p[:, 0] + cx * p[:, 2]) / zc, (fy * p[:, 1] + cy * p[:, 2]) / zc
        inside = sel & (uu < W) & (uu > 0) & (vv < H) & (vv > 0) & (zc > 0)
        margin = np.minimum(_rel(s, thr), np.where(d == 0, np.inf, np.abs(d.astype(np.float64))))
        on_surface = np.where(surface, _rel(far, 0.5), np.inf)
        zscale = np.abs(pw) @ np.abs(Rc[2]) + abs(tc[2]) + 1e-5
        on_sel = np.minimum.reduce([np.abs(uu) / W, np.abs(uu - W) / W, np.abs(vv) / H, np.abs(vv - H) / H, np.abs(zc) / zscale])
        on_sel = np.where(sel & ~np.isnan(on_sel), on_sel, np.inf)
        margin = np.minimum(margin, np.minimum(on_surface, on_sel.astype(np.float64)))
    return (int(inside.sum()), int(sel.sum())), margin.astype(np.float64)


def move_covisibility_pixels(sil, margin, placed):
    """Pixels closer than MARGIN to a threshold (and not placed by hand) get silhouette 0.5, in place.  Returns their number."""
    move = (margin < MARGIN) & ~placed.reshape(-1)
    sil.reshape(-1)[move] = 0.5
    return int(move.sum())
