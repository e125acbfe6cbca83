"""mm3dgs_ingest_est (csrc/ingest.hip) against the host path (dataset.ingest_est_host), and a RecordedSequence with est_depth_dir on the GPU.

Bars (include/mm3dgs.h): bit-identical at equal sizes (the value itself times the scale, rounded once on both sides); elsewhere
|kernel - host| <= finfo(float32).eps x max|source| x scale -- both sides are float64 evaluations of one expression rounded once, so they
can differ by one float32 ulp of a value no larger than the largest tap; tests/test_est_depth.py holds the host path to torch's own
F.interpolate at that same bar."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from tests.est_depth_cases import CASES, SHAPES, source

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = float(torch.finfo(torch.float32).eps)
CODE = {np.dtype(np.float32): 0, np.dtype(np.float16): 1, np.dtype(np.uint16): 2}


@pytest.fixture(scope="module")
def cases():
    """Sources and the host path's outputs (on the CPU), computed once and left unchanged."""
    from mm3dgs_slam_amd import dataset as ds
    out = {}
    for src, dst, _ in SHAPES:
        for dtype, scale in CASES:
            raw = source(*src, dtype)
            out[(src, dst, np.dtype(dtype), scale)] = (raw, ds.ingest_est_host(raw, scale, *dst))
    return out


def to_dev(raw):
    return torch.from_numpy(raw.view(np.int16).copy() if raw.dtype == np.uint16 else raw.copy()).to(DEV)


def call(Hs, Ws, est_ptr, dtype, scale, H, W, out_ptr):
    from mm3dgs_slam_amd import _lib
    from mm3dgs_slam_amd.rasterizer import _stream
    p = lambda v: None if v is None else C.c_void_p(v)
    return _lib.load().mm3dgs_ingest_est(Hs, Ws, p(est_ptr), int(dtype), float(scale), H, W, p(out_ptr), _stream())


def compare(got, host, raw, scale, same, what):
    got = got.cpu()
    err = float((got.double() - host.double()).abs().max())
    bar = EPS32 * float(np.abs(raw.astype(np.float64)).max()) * scale
    print(f"{what}: max |kernel - host| = {err:.3e} (bar {bar:.3e}), equal bits {torch.equal(got, host)}")
    assert got.dtype == torch.float32 and got.shape == host.shape
    if same:
        assert torch.equal(got, host), what
    else:
        assert err <= bar, what


@pytest.mark.parametrize("src,dst,same", SHAPES)
def test_kernel_matches_the_host_path(cases, src, dst, same):
    from mm3dgs_slam_amd import dataset as ds
    for dtype, scale in CASES:
        raw, host = cases[(src, dst, np.dtype(dtype), scale)]
        got = ds.ingest_est_device(to_dev(raw), scale, *dst)
        compare(got, host, raw, scale, same, f"{src}->{dst} {np.dtype(dtype).name} scale {scale}")


@pytest.mark.parametrize("src,dst,same", [SHAPES[0], SHAPES[1], SHAPES[4], SHAPES[5], SHAPES[6]])
def test_non_finite_sources_give_the_host_paths_pattern(src, dst, same):
    """One NaN and one inf in a float32 source: neither side special-cases them, both restate the same operators (0 * inf is NaN), so the
    same output pixels are NaN, the same are infinite, and the rest meet the bar."""
    from mm3dgs_slam_amd import dataset as ds
    raw = source(*src, np.float32, seed=9)
    (x0, x1, _), (y0, _, _) = ds._axis(dst[1], src[1]), ds._axis(dst[0], src[0])      # taps that some output pixel does read
    raw[int(y0[dst[0] // 2]), int(x0[dst[1] // 2])] = np.nan
    raw[int(y0[0]), int(x1[dst[1] - 1])] = np.inf
    host = ds.ingest_est_host(raw, 1.0, *dst)
    got = ds.ingest_est_device(to_dev(raw), 1.0, *dst).cpu()
    assert int(torch.isnan(host).sum()) >= 1 and int((~torch.isfinite(host)).sum()) >= 2
    assert torch.equal(torch.isnan(got), torch.isnan(host)) and torch.equal(torch.isposinf(got), torch.isposinf(host))
    assert not bool(torch.isneginf(got).any()) and not bool(torch.isneginf(host).any())
    fin = torch.isfinite(host)
    print(f"{src}->{dst}: {int((~fin).sum())} non-finite output pixels of {fin.numel()}")
    if same:
        assert int((~fin).sum()) == 2 and torch.equal(got[fin], host[fin])      # equal sizes: no blend, nothing spreads
    else:
        assert float((got[fin].double() - host[fin].double()).abs().max()) <= EPS32 * 3000.0


@pytest.mark.parametrize("src,dst,same", [SHAPES[1], SHAPES[2]])
def test_packed_and_general_path_give_the_same_bits(cases, src, dst, same):
    """The same data one element into a larger buffer: the source misses the packed path's alignment, so the general kernel runs."""
    for dtype, scale in CASES:
        raw, host = cases[(src, dst, np.dtype(dtype), scale)]
        aligned_src = to_dev(raw)
        n, size = raw.size, raw.dtype.itemsize
        buf = torch.zeros(n + 8, dtype=aligned_src.dtype, device=DEV)
        buf[1:1 + n] = aligned_src.reshape(-1)
        a = torch.full(dst, -7.0, device=DEV)
        b = torch.full(dst, -7.0, device=DEV)
        assert aligned_src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0 and a.data_ptr() % 16 == 0
        assert call(*src, aligned_src.data_ptr(), CODE[raw.dtype], scale, *dst, a.data_ptr()) == 0
        assert call(*src, buf.data_ptr() + size, CODE[raw.dtype], scale, *dst, b.data_ptr()) == 0
        assert torch.equal(a, b) and torch.equal(a.cpu(), host), (dtype, scale)
        # an output that misses the float4 alignment takes the general path too
        c = torch.full((dst[0] * dst[1] + 4,), -7.0, device=DEV)
        assert call(*src, aligned_src.data_ptr(), CODE[raw.dtype], scale, *dst, c.data_ptr() + 4) == 0
        assert torch.equal(c[1:1 + n].reshape(dst), a) and float(c[0]) == -7.0 and bool((c[1 + n:] == -7.0).all())


def test_rejected_calls_return_minus_one_and_write_nothing(cases):
    """Argument checks, not faults: every pointer handed over is valid (inside an allocation) or NULL."""
    from mm3dgs_slam_amd import _lib
    src = dst = (8, 12)
    raw, _ = cases[(src, dst, np.dtype(np.float32), 1.0)]
    est = torch.zeros(raw.size + 4, device=DEV)
    est[:raw.size] = to_dev(raw).reshape(-1)
    out = torch.full((dst[0] * dst[1] + 4,), -7.0, device=DEV)
    a = dict(Hs=8, Ws=12, est_ptr=est.data_ptr(), dtype=0, scale=1.0, H=8, W=12, out_ptr=out.data_ptr())
    bad = [dict(a, Hs=0), dict(a, Ws=0), dict(a, H=0), dict(a, W=0), dict(a, H=-3), dict(a, Ws=-1),      # non-positive sizes
           dict(a, Hs=1 << 16, Ws=1 << 15), dict(a, H=1 << 15, W=(1 << 15) + 1),                       # more than 2^30 pixels
           dict(a, est_ptr=None), dict(a, out_ptr=None),
           dict(a, dtype=-1), dict(a, dtype=3),
           dict(a, est_ptr=est.data_ptr() + 2), dict(a, dtype=1, est_ptr=est.data_ptr() + 1), dict(a, dtype=2, est_ptr=est.data_ptr() + 1),
           dict(a, out_ptr=out.data_ptr() + 2),
           dict(a, scale=0.0), dict(a, scale=-1.0), dict(a, scale=float("nan")), dict(a, scale=float("inf"))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"ingest_est" in _lib.load().mm3dgs_last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call(**a) == 0      # and the same arguments, untouched, are accepted
    torch.cuda.synchronize()
    assert bool((out[:96] != -7.0).all()) and bool((out[96:] == -7.0).all())
    for dtype in (1, 2):       # 2-byte alignment is enough for the 16-bit types
        assert call(**dict(a, dtype=dtype, Hs=4, Ws=6, H=2, W=3, est_ptr=est.data_ptr() + 2)) == 0
    torch.cuda.synchronize()


def test_staging_slots_carry_the_estimate_and_are_not_overwritten_in_flight(tmp_path):
    """Five frames fetched back to back as seq[i], seq.est(i) without synchronising (two staging slots, prefetch on), then compared with a
    host-ingest sequence.  The estimates are float16 at the frame size, so both paths deliver the same bits."""
    from mm3dgs_slam_amd import dataset as ds
    from tests.test_dataset import make_cfg, write_scene
    from tests.test_est_depth import stem_of, write_estimates
    scene = write_scene(tmp_path, "tum")
    ests = write_estimates(scene, "tum", np.float16, shape=(12, 16))
    small = write_estimates(scene, "tum", np.float32, folder="est_small")      # 9 x 14 -> 12 x 16: held to the bar, not to equal bits
    dev_seq = ds.RecordedSequence(make_cfg(tmp_path, "tum", device=DEV, ingest_on_device=True, prefetch=True, est_depth_dir="est_depth"))
    host_seq = ds.RecordedSequence(make_cfg(tmp_path, "tum", device=DEV, ingest_on_device=False, prefetch=False, est_depth_dir="est_depth"))
    assert dev_seq.on_device and not host_seq.on_device and (dev_seq.H, dev_seq.W) == (12, 16)
    got = []
    for i in range(5):
        frame = dev_seq[i]
        got.append((frame, dev_seq.est(i)))
    torch.cuda.synchronize()
    for i, ((color, depth, pose), est) in enumerate(got):
        hc, hd, hp = host_seq[i]
        he = host_seq.est(i)
        assert est.is_cuda and est.dtype == torch.float32 and tuple(est.shape) == (12, 16)
        assert torch.equal(color, hc) and torch.equal(depth, hd) and torch.equal(pose, hp) and torch.equal(est, he), i
        assert torch.equal(est.cpu(), torch.from_numpy(ests[stem_of(dev_seq.color_paths[i])].astype(np.float32))), i
    assert got[1][1].data_ptr() != got[2][1].data_ptr() and not torch.equal(got[1][1], got[2][1])
    # any other order gives the same tensors: the estimate alone, repeated, backwards
    for i in (4, 0, 3, 3, 2, 1):
        assert torch.equal(dev_seq.est(i), got[i][1]), i
    assert torch.equal(dev_seq[2][0], got[2][0][0]) and torch.equal(dev_seq.est(2), got[2][1])
    dev_seq.close(); host_seq.close()
    dev_seq = ds.RecordedSequence(make_cfg(tmp_path, "tum", device=DEV, ingest_on_device=True, prefetch=True, est_depth_dir="est_small"))
    for i in range(3):
        dev_seq[i]
        raw = small[stem_of(dev_seq.color_paths[i])]
        host = ds.ingest_est_host(raw, 1.0, 12, 16)
        assert float((dev_seq.est(i).cpu().double() - host.double()).abs().max()) <= EPS32 * float(raw.max())
    dev_seq.close()


def test_monocular_slam_over_a_recorded_sequence_on_the_native_loops(tmp_path):
    """tests/test_est_depth.py's end-to-end test at 64x48 on FusedTracker / FusedMapper with depth_align_on_device: three frames of a
    synthetic scene and their estimates (float32 at native size: both ingest paths deliver the same bits) recorded as a TUM directory.
    Host ingest, device ingest and a run that is handed the estimates from memory give bit-identical poses and the same map size."""
    from mm3dgs_slam_amd import dataset as ds
    from mm3dgs_slam_amd.config import default_config
    from mm3dgs_slam_amd.slam import SLAM, SyntheticSequence
    H, W = 48, 64
    base = lambda **kw: default_config(device=DEV, height=H, width=W, use_gt_depth=False, depth_align_on_device=True, tracking={"iters": 4},
                                       mapping={"iters": 5, "kf_every": 1}, **kw)
    src = SyntheticSequence(base(), 3, 2000, seed=3)
    ests = [src.est(i).clone() for i in range(3)]
    scale = float(base()["cam"]["png_depth_scale"])
    ds.write_tum_sequence(str(tmp_path / "rec" / "scene"), [ds.quantise_frame(c, d, scale) for c, d in src.frames], src.poses,
                          [100.0 + 0.1 * i for i in range(3)], est=ests)
    runs = {}
    for name, on_device, from_disk in (("host", False, True), ("device", True, True), ("memory", False, False)):
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        cfg = base(dataset="tum", inputdir=str(tmp_path / "rec"), scene="scene", ingest_on_device=on_device, outputdir=str(tmp_path / name))
        cfg["cam"].update(image_height=H, image_width=W)
        if from_disk:
            cfg["est_depth_dir"] = "est_depth"
        seq = ds.RecordedSequence(cfg)
        if from_disk:
            assert seq.on_device is on_device and all(torch.equal(seq.est(i), ests[i]) for i in range(3))
        else:
            assert not hasattr(seq, "est")
            seq.est = lambda i: ests[i].clone()
        slam = SLAM(cfg, seq)
        assert type(slam.tracker).__name__ == "FusedTracker" and type(slam.mapper).__name__ == "FusedMapper"
        seen, real = [], slam.mapper.run_frame
        slam.mapper.run_frame = lambda idx, color, depth, est_scaled, *a, **k: (seen.append(est_scaled.clone()), real(idx, color, depth, est_scaled, *a, **k))[1]
        slam.run()
        runs[name] = (torch.stack([p.detach() for p in slam.estimate_pose_list]).cpu(), int(slam.gaussians.get_xyz.shape[0]), seen)
        seq.close()
    pose, n, seen = runs["host"]
    assert n > 0 and torch.equal(seen[0], 1.0 / (ests[0] + 0.001) * scale / 10)      # the monocular path ran
    for name in ("device", "memory"):
        print(f"host vs {name}: pose difference {float((pose - runs[name][0]).abs().max())}, Gaussians {n} / {runs[name][1]}")
        assert torch.equal(pose, runs[name][0]) and runs[name][1] == n, name
    for name in ("host", "device"):
        table = np.load(os.path.join(str(tmp_path / name), "results.npz"), allow_pickle=True)["depth_align"]
        assert table.shape == (3, 4) and np.isnan(table[0]).all() and table[1, 2] == 1.0 and table[2, 2] == 1.0, (name, table)
