"""The image-loss kernels (csrc/loss.hip, loss_tile.h, loss_pixel.h) against the float64 host reference tests/loss_ref.py, at the shapes
where a tiled 11-tap kernel can go wrong, with a tolerance measured per case instead of fixed in advance:

    kernel error  <=  8 x (error of the float32 CPU restatement of the same loss)  +  one float32 ulp of the plane's largest magnitude

in every measure (rel_l2 of a plane; max|delta| / max|ref| over the image border band, the partial tiles, the interior; each of the
four loss values).  The factor 8 covers the other, equally valid float32 summation orders (separable fma strips against a 121-tap
convolution, a DPP tree against a serial sum) and v_rcp_f32's 1 ulp; a genuine defect (a wrong tap, a missing halo zero, a dropped
term) is 1e-3 or more.  DESIGN.md, "Loss kernels: measured error", holds the measured figures.  Every test prints its figures
(`LOSSERR ...`, pytest -s) before it asserts."""
import ctypes as C
import functools

import pytest
import torch

from tests import loss_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 4096       # bytes of guard zone on each side of a buffer the kernels own


@functools.lru_cache(maxsize=None)
def _inputs(family, H, W):
    return lr.make_inputs(family, H, W)


@functools.lru_cache(maxsize=None)
def _reference(name, family, H, W):
    """(loss4, dL) of the float64 reference and of the float32 restatement: computed once per case, shared, never written to."""
    fields, use_ref = lr.CONFIGS[name]
    out6, gt, ref = _inputs(family, H, W)
    r = ref if use_ref else None
    return lr.loss_ref(fields, out6, gt, r) + lr.loss_ref(fields, out6, gt, r, dtype=torch.float32)


def _struct(fields, H, W):
    from mm3dgs_slam_amd.fused import _loss_cfg
    f = fields
    c = _loss_cfg(H, W, f["w_l1"], f["w_ssim"], f["w_pearson"], f["l1_mask"], f["pearson_mask"], f["pearson_invert"], f["sil_thr"],
                  w_depth_l1=f["w_depth_l1"], depth_l1_mask=f["depth_l1_mask"], l1_sum=f["l1_sum"])
    for i, w in enumerate(f["window"]):
        c.window[i] = w
    return c


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _call(fields, H, W, out6, gt, ref, work, dL, loss4):
    """mm3dgs_loss through the C ABI on device tensors; returns the return code (no exception: the refusal tests read it)."""
    from mm3dgs_slam_amd import _lib
    from mm3dgs_slam_amd.rasterizer import _stream
    rc = _lib.load().mm3dgs_loss(C.byref(_struct(fields, H, W)), _ptr(out6), _ptr(gt), _ptr(ref), _ptr(work), _ptr(dL), _ptr(loss4), _stream())
    torch.cuda.synchronize()
    return rc


def _work(H, W, fill=None):
    from mm3dgs_slam_amd import _lib
    n = _lib.load().mm3dgs_loss_work_bytes(H, W)
    return torch.empty(n, dtype=torch.uint8, device=DEV) if fill is None else torch.full((n,), fill, dtype=torch.uint8, device=DEV)


def _run(fields, H, W, out6, gt, ref, want_loss4=True, work=None, fill=None):
    """A standalone loss call on CPU inputs in fresh buffers; (loss4 or None, dL) on the CPU."""
    dev = [t.to(DEV).contiguous() if t is not None else None for t in (out6, gt, ref)]
    dL = torch.empty(6, H, W, device=DEV) if fill is None else torch.full((6 * H * W * 4,), fill, dtype=torch.uint8, device=DEV).view(torch.float32).view(6, H, W)
    loss4 = torch.zeros(4, device=DEV) if want_loss4 else None
    assert _call(fields, H, W, dev[0], dev[1], dev[2], _work(H, W, fill) if work is None else work, dL, loss4) == 0
    return (loss4.cpu() if want_loss4 else None), dL.cpu()


def check_against_reference(tag, H, W, fields, loss4, dL, l64, d64, l32, d32, planes=4, factor=lr.FACTOR):
    """The assertions of one case: loss values (loss4 None: not asked for), each live gradient plane in every measure, planes 4 and 5
    exactly 0 (planes == 6), mask membership."""
    fails = []
    if loss4 is not None:
        assert bool(torch.isfinite(loss4).all()), loss4
        floor = lr.ulp32(float(l64.abs().max()))
        for i, nm in enumerate(("total", "l1", "1-ssim", "term3")):
            e32, err = abs(float(l32[i]) - float(l64[i])), abs(float(loss4[i]) - float(l64[i]))
            b = lr.bound(e32, floor, factor)
            print(f"LOSSERR {tag} loss4.{nm} e32={e32:.2e} err={err:.2e} bound={b:.2e}")
            if err > b:
                fails.append((nm, err, b))
    if dL is None:        # a form without a gradient image
        assert not fails, fails
        return
    assert bool(torch.isfinite(dL[:planes]).all())
    for p in range(4):
        if float(d64[p].abs().max()) == 0.0:       # no term reaches this plane: exact zeros
            assert float(dL[p].abs().max()) == 0.0, p
            continue
        e32, floor, err = lr.plane_errors(d32[p], d64[p], H, W), lr.plane_floors(d64[p], H, W), lr.plane_errors(dL[p], d64[p], H, W)
        for m in err:
            b = lr.bound(e32[m], floor[m], factor)
            print(f"LOSSERR {tag} dL{p}.{m} e32={e32[m]:.2e} err={err[m]:.2e} bound={b:.2e}")
            if not err[m] <= b:
                fails.append((p, m, err[m], b))
    if planes == 6:
        assert float(dL[4:].abs().max()) == 0.0
    # mask membership, exact: the pixels with an L1 gradient (readable where no SSIM term covers the colour planes) and the
    # pixels with a Pearson / depth-L1 gradient are the reference's
    if fields["w_ssim"] == 0.0:
        assert torch.equal((dL[:3] != 0).any(0), (d64[:3] != 0).any(0)), "L1 mask membership"
    assert torch.equal(dL[3] != 0, d64[3] != 0), "depth-plane mask membership"
    assert not fails, fails


@pytest.mark.parametrize("family", lr.FAMILIES)
@pytest.mark.parametrize("name", list(lr.CONFIGS))
@pytest.mark.parametrize("shape", lr.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_kernels_match_the_float64_reference(shape, name, family):
    H, W = shape
    fields, use_ref = lr.CONFIGS[name]
    out6, gt, ref = _inputs(family, H, W)
    l64, d64, l32, d32 = _reference(name, family, H, W)
    loss4, dL = _run(fields, H, W, out6, gt, ref if use_ref else None, want_loss4=name != "no_loss4")
    check_against_reference(f"{H}x{W} {name} {family}", H, W, fields, loss4, dL, l64, d64, l32, d32, planes=6)


# ---- ownership, staleness, determinism --------------------------------------------------------------------------------------------
SSIM_PEARSON = lr.CONFIGS["map"][0]
OWN_SHAPES = [(17, 33), (80, 208)]


def _guarded(nbytes):
    """A buffer of `nbytes` inside a larger allocation with GUARD bytes of 0xA5 on both sides: (whole, inner view)."""
    whole = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return whole, whole[GUARD:GUARD + nbytes]


@pytest.mark.parametrize("shape", OWN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_writes_only_the_buffers_it_owns(shape):
    H, W = shape
    cpu = _inputs("random", H, W)
    out6, gt, ref = (t.to(DEV).contiguous() for t in cpu)
    from mm3dgs_slam_amd import _lib
    wn = _lib.load().mm3dgs_loss_work_bytes(H, W)
    gw, work = _guarded(wn)
    gd, dLb = _guarded(6 * H * W * 4)
    gl, l4b = _guarded(16)
    dL, loss4 = dLb.view(torch.float32).view(6, H, W), l4b.view(torch.float32)
    assert _call(SSIM_PEARSON, H, W, out6, gt, ref, work, dL, loss4) == 0
    for whole, n in ((gw, wn), (gd, 6 * H * W * 4), (gl, 16)):
        assert bool((whole[:GUARD] == 0xA5).all()) and bool((whole[GUARD + n:] == 0xA5).all())
    for dev, host in zip((out6, gt, ref), cpu):
        assert torch.equal(dev.cpu().view(torch.int32), host.view(torch.int32))
    assert bool(torch.isfinite(dL).all()) and bool(torch.isfinite(loss4).all())      # ... and it did write what it owns


@pytest.mark.parametrize("shape", OWN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_reads_no_stale_slot_and_is_deterministic(shape):
    H, W = shape
    out6, gt, ref = _inputs("random", H, W)
    l0, d0 = _run(SSIM_PEARSON, H, W, out6, gt, ref, fill=0x00)
    l1, d1 = _run(SSIM_PEARSON, H, W, out6, gt, ref, fill=0xFF)      # work and dL all NaN before the call
    l2, d2 = _run(SSIM_PEARSON, H, W, out6, gt, ref, fill=0x00)
    assert bool(torch.isfinite(l1).all()) and bool(torch.isfinite(d1).all())
    for l, d in ((l1, d1), (l2, d2)):
        assert torch.equal(l.view(torch.int32), l0.view(torch.int32)) and torch.equal(d.view(torch.int32), d0.view(torch.int32))


def test_loss_in_a_reused_work_buffer_equals_a_fresh_one():
    (Hb, Wb), (Hs, Ws) = (80, 208), (17, 33)
    work = _work(Hb, Wb, fill=0x00)
    big = _inputs("random", Hb, Wb)
    _run(SSIM_PEARSON, Hb, Wb, *big, work=work)
    small = _inputs("flat", Hs, Ws)
    other = lr.CONFIGS["track_pearson"][0]
    for fields in (other, lr.CONFIGS["splatam_map"][0], SSIM_PEARSON):
        l_re, d_re = _run(fields, Hs, Ws, *small, work=work)
        l_fr, d_fr = _run(fields, Hs, Ws, *small, fill=0x00)
        assert torch.equal(l_re.view(torch.int32), l_fr.view(torch.int32)) and torch.equal(d_re.view(torch.int32), d_fr.view(torch.int32))


# ---- degenerate inputs ------------------------------------------------------------------------------------------------------------
def _degenerate_cases():
    H, W = 17, 33
    out6, gt, ref = _inputs("random", H, W)
    low = out6.clone()
    low[4] = 0.5
    zref = torch.zeros_like(ref)
    one = zref.clone()
    one[7, 11] = 2.0
    return {
        "sil_below_thr": (lr.cfg_fields(w_l1=1.0, l1_mask=1, sil_thr=0.99), low, None),
        "ref_zero_l1_depth": (lr.cfg_fields(w_l1=1.0, l1_mask=3, sil_thr=0.5, w_depth_l1=1.0, depth_l1_mask=2), out6, zref),
        "ref_zero_l1_depth_sums": (lr.cfg_fields(w_l1=1.0, l1_mask=3, sil_thr=0.5, w_depth_l1=1.0, depth_l1_mask=2, l1_sum=1), out6, zref),
        "ref_zero_pearson": (lr.cfg_fields(w_l1=1.0, w_pearson=1.0, l1_mask=3, pearson_mask=2), out6, zref),
        "ref_zero_pearson_invert": (lr.cfg_fields(w_l1=1.0, w_pearson=1.0, l1_mask=3, pearson_mask=2, pearson_invert=1), out6, zref),
        "one_pearson_pixel": (lr.cfg_fields(w_pearson=1.0, pearson_mask=2), out6, one),
        "one_pearson_pixel_invert": (lr.cfg_fields(w_pearson=1.0, pearson_mask=2, pearson_invert=1), out6, one),
    }, gt


@pytest.mark.parametrize("case", ["sil_below_thr", "ref_zero_l1_depth", "ref_zero_l1_depth_sums", "ref_zero_pearson", "ref_zero_pearson_invert",
                                  "one_pearson_pixel", "one_pearson_pixel_invert"])
def test_empty_masks_give_exact_zeros_not_nan(case):
    H, W = 17, 33
    cases, gt = _degenerate_cases()
    fields, out6, ref = cases[case]
    l64, d64 = lr.loss_ref(fields, out6, gt, ref)
    assert float(d64.abs().max()) == 0.0 and float(l64[0]) == 0.0 and float(l64[3]) == 0.0       # the reference's conventions
    loss4, dL = _run(fields, H, W, out6, gt, ref, fill=0xFF)
    assert bool(torch.isfinite(loss4).all()) and bool(torch.isfinite(dL).all())
    assert float(dL.abs().max()) == 0.0
    assert float(loss4[0]) == 0.0 and float(loss4[3]) == 0.0
    if case.startswith("one_pearson"):       # w_l1 = 0, l1_mask = 0: the colour L1 value is still reported
        l32, _ = lr.loss_ref(fields, out6, gt, ref, dtype=torch.float32)
        assert abs(float(loss4[1]) - float(l64[1])) <= lr.bound(abs(float(l32[1]) - float(l64[1])), lr.ulp32(float(l64[1])))
    else:
        assert float(loss4[1]) == 0.0
    assert float(loss4[2]) == 0.0


@pytest.mark.parametrize("invert", [0, 1])
def test_all_zero_rendered_depth_under_a_pearson_mask_is_non_finite_where_the_reference_is(invert):
    """cxx == 0 exactly: 0 / 0 in the float64 reference and in loss_utils.  The kernels must not turn it into finite garbage: the
    Pearson value, the total and the masked pixels of the depth plane are non-finite, everything else is as usual."""
    H, W = 17, 33
    out6, gt, ref = (t.clone() for t in _inputs("random", H, W))
    out6[3] = 0.0
    fields = lr.cfg_fields(w_l1=1.0, w_pearson=1.0, pearson_mask=2, pearson_invert=invert)
    l64, d64 = lr.loss_ref(fields, out6, gt, ref)
    assert bool(torch.isnan(l64[0])) and bool(torch.isnan(l64[3])) and torch.equal(torch.isnan(d64[3]), ref > 0)
    loss4, dL = _run(fields, H, W, out6, gt, ref)
    assert torch.equal(~torch.isfinite(loss4), ~torch.isfinite(l64)), loss4
    assert torch.equal(~torch.isfinite(dL), ~torch.isfinite(d64))
    assert float(dL[3][~(ref > 0)].abs().max()) == 0.0 and float(dL[4:].abs().max()) == 0.0
    _, d32 = lr.loss_ref(fields, out6, gt, ref, dtype=torch.float32)
    e32, floor, e = lr.plane_errors(d32[:3], d64[:3], H, W), lr.plane_floors(d64[:3], H, W), lr.plane_errors(dL[:3], d64[:3], H, W)
    for m in e:        # the colour planes are untouched by the NaN
        assert e[m] <= lr.bound(e32[m], floor[m]), (m, e[m], e32[m])


# ---- argument refusal -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pearson_without_ref", "l1_mask2_without_ref", "depth_l1_without_ref", "depth_l1_with_pearson", "H_zero", "H_negative"])
def test_loss_refuses_bad_arguments_before_any_launch(case):
    from mm3dgs_slam_amd import _lib
    H, W = 17, 33
    out6, gt, ref = (t.to(DEV).contiguous() for t in _inputs("random", H, W))
    fields, r, h = {
        "pearson_without_ref": (lr.cfg_fields(w_l1=1.0, w_pearson=0.05), None, H),
        "l1_mask2_without_ref": (lr.cfg_fields(w_l1=1.0, l1_mask=2), None, H),
        "depth_l1_without_ref": (lr.cfg_fields(w_l1=1.0, w_depth_l1=1.0), None, H),
        "depth_l1_with_pearson": (lr.cfg_fields(w_l1=1.0, w_depth_l1=1.0, w_pearson=0.05), ref, H),
        "H_zero": (lr.cfg_fields(w_l1=1.0), ref, 0),
        "H_negative": (lr.cfg_fields(w_l1=1.0), ref, -H),
    }[case]
    work = _work(H, W, fill=0xA5)
    dL = torch.full((6, H, W), 7.0, device=DEV)
    loss4 = torch.full((4,), 7.0, device=DEV)
    rc = _call(fields, h, W, out6, gt, r, work, dL, loss4)
    assert rc != 0 and _lib.load().mm3dgs_last_error()
    # nothing ran: every output still holds its fill
    assert bool((dL == 7.0).all()) and bool((loss4 == 7.0).all()) and bool((work == 0xA5).all())


# ---- the three forms of the mapping loop's loss against the reference -----------------------------------------------------------------
@pytest.mark.parametrize("pearson", [False, True])
@pytest.mark.parametrize("shape", [(72, 104), (112, 112), (80, 208)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_mapping_loop_loss_forms_match_the_float64_reference(shape, pearson, monkeypatch):
    """One mm3dgs_slam_map iteration without Adam, in its three forms (test_mapping_loss_via_forward_rows_matches_the_standalone_loss_kernels
    compares them with each other): A the standalone kernels, B tile rows from the forward epilogue reduced by the SSIM kernel's extra
    workgroup (35 / 49 / 65 rows: both sides of reduce_rows_256's 48- and 64-row steps) and a 4-plane gradient image, C the gradient
    pass inside the backward compositor.  Each form's loss values against the reference evaluated on that form's own rendered image;
    the gradient image of A and B against the reference's."""
    from mm3dgs_slam_amd.fused import FusedEngine
    from tests.test_gpu_fused import _setup, eng_grads
    H, W = shape
    cfg, g, R, pose, color, depth = _setup(P=3000, H=H, W=W, seed=11)
    fields = lr.cfg_fields(w_l1=0.8, w_ssim=0.2, w_pearson=0.05 if pearson else 0.0, pearson_mask=2 if pearson else 0)
    lc = _struct(fields, H, W)
    ref = depth.contiguous() if pearson else None
    gt_cpu, ref_cpu = color.cpu(), (ref.cpu() if pearson else None)
    cache = None
    for form, no_rows, no_fold in (("A", "1", "0"), ("B", "0", "1"), ("C", "0", "0")):
        monkeypatch.setenv("MM3DGS_NO_FORWARD_ROWS", no_rows)
        monkeypatch.setenv("MM3DGS_NO_FOLDED_LOSS", no_fold)
        eng = FusedEngine(R)
        eng.max_tile_len = 100          # "short lists": the fused sort + composite kernel (carries the epilogue)
        eng.dL.fill_(float("nan"))
        eng.loss_work.fill_(0xFF)       # a row or a slot read before it is written is a NaN
        eng.map_loop([(pose.contiguous(), color.contiguous(), ref)], g, lc, None, None, grads=eng_grads(eng, g))
        torch.cuda.synchronize()
        assert eng.check_capacity()
        out, loss4, dL = eng.out.cpu(), eng.loss.cpu(), eng.dL.cpu()
        if cache is None or not torch.equal(cache[0], out):
            cache = (out, lr.loss_ref(fields, out, gt_cpu, ref_cpu) + lr.loss_ref(fields, out, gt_cpu, ref_cpu, dtype=torch.float32))
        l64, d64, l32, d32 = cache[1]
        tag = f"{H}x{W} form{form} {'pearson' if pearson else 'photo'}"
        if form == "C":        # no gradient image at all in this form
            assert bool(torch.isnan(dL).all())
            dL = None
        else:
            assert bool(torch.isnan(dL[4:]).all()) == (form == "B")
        check_against_reference(tag, H, W, fields, loss4, dL, l64, d64, l32, d32, planes=6 if form == "A" else 4)
