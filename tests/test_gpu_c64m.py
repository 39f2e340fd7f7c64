"""-m gpu: conv64m_kernel (csrc/esr_c64m.hip, round 6) -- the 64 -> 64 3x3 family on v_mfma_f32_32x32x16: RFDB's c{j}_r = lrelu(conv3x3(x) + x)
(rfdn_baseline/block.py:150-158) plain and with the next distillation 1x1 + LeakyReLU in its epilogue.  Checked against an fp64 reference on the
same 16-bit inputs and the blob's EFFECTIVE weights (tolerance: the one rounding of the stored value + fp32 accumulation noise), at shapes with
more 16 x 16 tiles than persistent blocks, ragged edges, several images, logical channel counts below the physical 64."""
import ctypes

import pytest
import torch

import _persist_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def _tf(compute):
    return "true" if compute == "bf16" else "false"


def _tol(ref, dt, extra=0.0):
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    return ref.abs() * eps * 1.01 + 3e-5 * max(1.0, float(ref.abs().max())) + extra


@pytest.mark.parametrize("compute", ["bf16", "f16"])
@pytest.mark.parametrize("n,c,hw,res_in", [(1, 64, (270, 480), True), (1, 50, (339, 510), True), (3, 64, (160, 144), False), (2, 50, (250, 203), True),
                                           (32, 50, (64, 64), True),
                                           # other widths of 49 .. 64 at the kernel's threshold: 256 tiles of 16 x 16, a ragged right edge
                                           (4, 49, (128, 120), True), (4, 57, (128, 120), False), (4, 63, (128, 120), True)])
def test_conv64m_plain_matches_fp64_reference(compute, n, c, hw, res_in):
    dt = DT[compute]
    case = P.conv64m(compute, n, c, hw, res_in, n + c + hw[0])
    ref = case.refs[0]
    for it in range(3):                  # a race would not show every time
        (y,), names = (case.outs, case.names) if it == 0 else case.extra["launch"]()
        assert len(names) == 1 and names[0].startswith(f"conv64m_kernel<{_tf(compute)}, false, false, 4, false>"), names
        got = y.permute(0, 3, 1, 2)[:, :c].double()
        bad = int(((got - ref).abs() > _tol(ref, dt)).sum())
        assert bad == 0, (bad, float((got - ref).abs().max()))
    print(f"conv64m {compute} c={c} {n}x{hw}: max|got - ref| = {float((got - ref).abs().max()):.3e} ({float(((got - ref).abs() / _tol(ref, dt)).max()):.3f} of the bound)")
    assert torch.all(y[..., c:(c + 7) // 8 * 8] == 0)        # pad channels of the last 16-byte granule are zeros


@pytest.mark.parametrize("compute", ["bf16", "f16"])
@pytest.mark.parametrize("n,c,pc,hw,res_in", [(1, 50, 25, (339, 510), True), (8, 50, 25, (128, 128), True), (9, 64, 32, (100, 77), True), (5, 50, 25, (64, 250), False),
                                              (4, 49, 17, (128, 120), True), (4, 57, 24, (128, 120), True), (4, 63, 32, (128, 120), False)])      # other widths
def test_conv64m_post_matches_fp64_reference(compute, n, c, pc, hw, res_in):
    dt = DT[compute]
    case = P.conv64m(compute, n, c, hw, res_in, n * 10 + hw[0] + c, pc=pc)
    ref = case.refs[0]
    for it in range(2):
        (y, yp), names = (case.outs, case.names) if it == 0 else case.extra["launch"]()
        assert len(names) == 1 and names[0].startswith(f"conv64m_kernel<{_tf(compute)}, true, false, 4, false>"), names
        got = y.permute(0, 3, 1, 2)[:, :c].double()
        bad = int(((got - ref).abs() > _tol(ref, dt)).sum())
        assert bad == 0, (bad, float((got - ref).abs().max()))
        # the post 1x1 + LeakyReLU.  bf16: it sees the fp32 activations as hi + lo (16 mantissa bits) and hi + lo weights; fp16: the rounded
        # activations (the stored y) and the weights' high parts
        extra = 2e-4
        pref = case.extra["post_ref"](got)
        gp = yp.permute(0, 3, 1, 2)[:, :pc].double()
        badp = int(((gp - pref).abs() > _tol(pref, dt, extra)).sum())
        assert badp == 0, (badp, float((gp - pref).abs().max()))
    print(f"conv64m + post {compute} c={c} pc={pc} {n}x{hw}: max|y - ref| = {float((got - ref).abs().max()):.3e} "
          f"({float(((got - ref).abs() / _tol(ref, dt)).max()):.3f} of the bound), max|post - ref| = {float((gp - pref).abs().max()):.3e} "
          f"({float(((gp - pref).abs() / _tol(pref, dt, extra)).max()):.3f})")
    assert torch.all(yp[..., pc:] == 0) and torch.all(y[..., c:(c + 7) // 8 * 8] == 0)


def test_conv64m_is_the_kernel_that_runs():
    """the 64 -> 64 3x3s of an RFDN forward at >= 256 tiles take conv64m_kernel (named by the device symbol the library launched)"""
    from ntire2022_esr_amd.registry import select_model
    m = select_model(0, torch.device(DEV))[0]
    m.set_compute("bf16")
    x = (torch.rand(1, 3, 339, 510) * 255.0).to(DEV)
    m(x)
    m.enable_profiling(1)
    m(x)
    torch.cuda.synchronize()
    m.collect_profile()
    m(x)
    torch.cuda.synchronize()
    names = {o["kernel"] for o in m.collect_profile()}
    m.disable_profiling()
    assert any(k.startswith("conv64m_kernel<true, true, false, 4, false>") for k in names), names          # c1_r / c2_r with the next distillation 1x1
    assert any(k.startswith("conv64m_kernel<true, false, false, 4, false>") for k in names), names         # c3_r
    assert any(k.startswith("conv64m_kernel<true, false, true, 4, false>") for k in names), names          # LR_conv on hi + lo pairs


@pytest.mark.parametrize("compute", ["bf16", "f16"])
@pytest.mark.parametrize("n,hw,nf,dc,f", [(1, (339, 510), 50, 25, 16), (4, (128, 144), 50, 25, 16), (2, (250, 203), 64, 32, 16), (32, (64, 64), 50, 25, 12),
                                          # other widths at the kernel's threshold (256 tiles of 16 x 16, a ragged right edge): both ends of nf in 49 .. 64,
                                          # of dc in 17 .. 32 and of f in 1 .. 16, and widths at / one past a 16-byte granule
                                          (4, (128, 120), 49, 17, 1), (4, (128, 120), 57, 24, 8), (4, (128, 120), 56, 31, 9), (4, (128, 120), 63, 32, 16),
                                          # one output tile: esr_pack_conv_s16 emits no 32x32x16 image for it -- refused, nothing is launched
                                          (4, (128, 120), 50, 16, 16)])
def test_rfdb_tail_matches_fp64_reference(compute, n, hw, nf, dc, f):
    """rfdb_tail_kernel (ABI v12, esr_conv_desc.tail_* in 16-bit storage): r4 = round(lrelu(c4(r3))), v = c5 . [d1 d2 d3 r4], c1 = conv1 . v in one
    launch (rfdn_baseline/block.py:161-164, :117), against fp64 on the same 16-bit inputs and the blobs' effective weights."""
    from ntire2022_esr_amd import _lib as L
    dt = DT[compute]
    case = P.block_tail(compute, n, hw, nf, dc, f, False)
    (v, c1), d, st = case.outs, case.extra["d"], case.extra["st"]
    if dc <= 16:
        assert case.names is None and L.lib().esr_conv_tail_supported(ctypes.byref(d)) == 0
        assert L.STATUS[L.lib().esr_conv2d_f32(ctypes.byref(d), st)] == "ESR_ERR_UNSUPPORTED"
        torch.cuda.synchronize()
        assert torch.all(v == 7.0) and torch.all(c1 == 7.0)
        return
    assert L.lib().esr_conv_tail_supported(ctypes.byref(d)) == 1
    vref, (extra, extra_c) = case.refs[0], case.extra["slack"]
    for it in range(3):
        names = case.names if it == 0 else case.extra["launch"]()
        assert len(names) == 1 and names[0].startswith(f"rfdb_tail_kernel<{_tf(compute)}, 4, false>"), names
        got = v.permute(0, 3, 1, 2)[:, :nf].double()
        bad = int(((got - vref).abs() > _tol(vref, dt, extra)).sum())
        assert bad == 0, (bad, float((got - vref).abs().max()))
        cref = case.extra["c1_ref"](got)
        gc = c1.permute(0, 3, 1, 2)[:, :f].double()
        badc = int(((gc - cref).abs() > _tol(cref, dt, extra_c)).sum())
        assert badc == 0, (badc, float((gc - cref).abs().max()))
    print(f"rfdb tail {compute} ({nf}, {dc}, {f}) {n}x{hw}: max|v - ref| = {float((got - vref).abs().max()):.3e} "
          f"({float(((got - vref).abs() / _tol(vref, dt, extra)).max()):.3f} of the bound), max|c1 - ref| = {float((gc - cref).abs().max()):.3e} "
          f"({float(((gc - cref).abs() / _tol(cref, dt, extra_c)).max()):.3f})")
    assert torch.all(v[..., (nf + 7) // 8 * 8:] == 7.0) and torch.all(v[..., nf:(nf + 7) // 8 * 8] == 0)
    assert torch.all(c1[..., f:(f + 7) // 8 * 8] == 0)


@pytest.mark.parametrize("compute", ["bf16", "f16"])
def test_rfdn_with_and_without_the_fused_block_tail(compute):
    """model.fuse_tail: the same network with RFDB's c4 / c5 + esa.conv1 as two launches or as rfdb_tail_kernel.  The fused form keeps c5's
    weights as hi + lo and v's low part for conv1 (the launches: one 16-bit value each), so the two differ by storage noise; measured against the
    fp32 engine the fused network must not be the worse one"""
    from ntire2022_esr_amd.registry import select_model
    m = select_model(0, torch.device(DEV))[0]
    x = (torch.rand(1, 3, 339, 510, generator=torch.Generator().manual_seed(3)) * 255.0).to(DEV)
    m.set_compute("f32")
    y32 = m(x).clone()
    m.set_compute(compute)
    y1 = m(x).clone()
    m.enable_profiling(1); m(x); torch.cuda.synchronize(); m.collect_profile(); m(x); torch.cuda.synchronize()
    names = {o["kernel"] for o in m.collect_profile()}
    m.disable_profiling()
    assert any(k.startswith("rfdb_tail_kernel") for k in names), names
    m.fuse_tail = False
    y0 = m(x).clone()
    m.fuse_tail = True

    def psnr(a, b):
        return float(10.0 * torch.log10(255.0 ** 2 / ((a - b) ** 2).mean().clamp_min(1e-12)))
    fused, separate, between = psnr(y1, y32), psnr(y0, y32), psnr(y1, y0)
    assert fused > separate - 0.5, (fused, separate, between)
    assert between > (50.0 if compute == "bf16" else 64.0), (fused, separate, between)
    assert torch.equal(m(x), y1)


@pytest.mark.parametrize("n,c,hw,act", [(1, 50, (339, 510), 0), (2, 64, (250, 203), 1), (32, 50, (64, 64), 0), (5, 50, (100, 177), 0),
                                        (4, 49, (128, 120), 0), (4, 57, (128, 120), 1), (4, 63, (128, 120), 0)])      # other widths, 256 tiles
def test_conv64m_hilo_lr_conv_matches_fp64_reference(n, c, hw, act):
    """conv64m_kernel<bf16, plain, HL>: the LR conv behind the long skip on hi + lo pairs (RFDN: LR_conv(out_B) + out_fea, rfdn_baseline/RFDN.py:50-52)
    -- the residual pair of ANOTHER tensor as eight selection MFMAs in front of the next row pair's stream, the fp32 result stored as a hi + lo
    pair.  hi + lo is the fp64 result to two bf16 numbers; every image alone (fewer than 256 tiles: conv_s16_kernel's HILO instantiation) agrees
    to the same bound; rows / columns beyond the image and pad channels stay untouched / zero."""
    from ntire2022_esr_amd import _lib as L
    cp = 64
    case = P.lr_hilo(n, c, hw, act, cp)
    rin, ref = case.extra["rin"], case.refs[0]
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ksize = n, hw[0], hw[1], c, c, 3
    d.in_layout = d.out_layout = L.NHWC
    d.storage, d.act, d.res_mode, d.hilo, d.hilo_stride = L.STORE["bf16"], act, L.RES_PRE_ACT, L.HILO_RES | L.HILO_OUT, 4096
    d.res = L.View(ctypes.c_void_p(rin.data_ptr()), cp, 0)
    assert L.lib().esr_conv_block_waves(ctypes.byref(d)) == 1
    tol = ref.abs() * 2.0 ** -15 + 3e-5 * max(1.0, float(ref.abs().max()))
    for it in range(2):
        (y,), names = (case.outs, case.names) if it == 0 else case.chunk(0, n)
        assert len(names) == 1 and names[0].startswith("conv64m_kernel<true, false, true, 4, false>"), names
        torch.cuda.synchronize()
        assert tuple(y.shape) == (2, n, *hw, cp)
        got = (y[0].double() + y[1].double()).permute(0, 3, 1, 2)[:, :c]
        assert int(((got - ref).abs() > tol).sum()) == 0, float(((got - ref).abs() - tol).max())
        assert bool((y[1].float().abs() <= y[0].float().abs() * 2.0 ** -7 + 1e-30).all())          # the low parts are remainders of the high ones
        assert torch.all(y[..., (c + 7) // 8 * 8:] == 0) or c == 64
    if n > 1 and n <= 5:
        y1 = case.chunk(0, 1)[0][0]                                                                # the general kernel
        g1 = (y1[0].double() + y1[1].double()).permute(0, 3, 1, 2)[:, :c]
        assert int(((g1 - ref[:1]).abs() > tol[:1]).sum()) == 0
        assert float((g1 - got[:1]).abs().max()) <= 2.0 * float(tol[:1].max())


@pytest.mark.parametrize("compute", ["f16", "bf16"])
@pytest.mark.parametrize("n,hw,C,dc,f", [(1, (339, 510), 48, 24, 12), (4, (128, 160), 48, 24, 16), (2, (250, 203), 40, 20, 10),
                                         (4, (128, 120), 33, 17, 1), (4, (128, 120), 41, 31, 8), (4, (128, 120), 47, 32, 9)])      # other widths, 256 tiles
def test_esdb_tail_matches_fp64_reference(compute, n, hw, C, dc, f):
    """rfdb_tail_kernel<.., 3, true>: ESDB's tail (team18_bsrn.py:165-171, :109) -- c4 = BSConvU as a dense 3x3 over 48 physical channels with
    the merged pointwise bias's border table and GELU, r4 never stored, v = c5 . [d1 d2 d3 r4], c1_ = esa.conv1 . v -- against fp64 on the
    same 16-bit inputs, the blobs' effective weights and the exact GELU (the kernel's polynomial: |error| <= 1.3e-4 on [-4, 4], 2.13e-4 below -4, esr_s16_dev.h)."""
    from ntire2022_esr_amd import _lib as L
    dt = DT[compute]
    case = P.block_tail(compute, n, hw, C, dc, f, True)
    (v, c1), d = case.outs, case.extra["d"]
    assert L.lib().esr_conv_tail_supported(ctypes.byref(d)) == 1
    vref, (extra, extra_c) = case.refs[0], case.extra["slack"]
    for it in range(2):
        names = case.names if it == 0 else case.extra["launch"]()
        assert len(names) == 1 and names[0].startswith(f"rfdb_tail_kernel<{_tf(compute)}, 3, true>"), names
        got = v.permute(0, 3, 1, 2)[:, :C].double()
        bad = int(((got - vref).abs() > _tol(vref, dt, extra)).sum())
        assert bad == 0, (bad, float((got - vref).abs().max()))
        cref = case.extra["c1_ref"](got)
        gc = c1.permute(0, 3, 1, 2)[:, :f].double()
        badc = int(((gc - cref).abs() > _tol(cref, dt, extra_c)).sum())
        assert badc == 0, (badc, float((gc - cref).abs().max()))
    print(f"esdb tail {compute} ({C}, {dc}, {f}) {n}x{hw}: max|v - ref| = {float((got - vref).abs().max()):.3e} "
          f"({float(((got - vref).abs() / _tol(vref, dt, extra)).max()):.3f} of the bound), max|c1 - ref| = {float((gc - cref).abs().max()):.3e} "
          f"({float(((gc - cref).abs() / _tol(cref, dt, extra_c)).max()):.3f})")
    assert torch.all(v[..., (C + 7) // 8 * 8:] == 7.0) and torch.all(v[..., C:(C + 7) // 8 * 8] == 0)
    assert torch.all(c1[..., f:(f + 7) // 8 * 8] == 0)


def test_bsrn_with_and_without_the_fused_block_tail():
    """model.fuse_tail on BSRN fp16 (BASELINE config [4]): ESDB's c4 / c5 + esa.conv1 as two launches or as rfdb_tail_kernel<false, 3, true>;
    against the fp32 engine the fused network must not be the worse one."""
    from ntire2022_esr_amd.registry import select_model
    m = select_model(18, torch.device(DEV))[0]
    x = (torch.rand(1, 3, 270, 480, generator=torch.Generator().manual_seed(3)) * 255.0).to(DEV)
    m.set_compute("f32")
    y32 = m(x).clone()
    m.set_compute("f16")
    y1 = m(x).clone()
    m.enable_profiling(1); m(x); torch.cuda.synchronize(); m.collect_profile(); m(x); torch.cuda.synchronize()
    names = {o["kernel"] for o in m.collect_profile()}
    m.disable_profiling()
    assert any(k.startswith("rfdb_tail_kernel<false, 3, true>") for k in names), names
    assert any(k.startswith("conv64m_kernel<false, true, false, 3, true>") for k in names), names         # c1_r / c2_r + the next distillation Linear
    assert any(k.startswith("conv64m_kernel<false, false, false, 3, true>") for k in names), names        # c3_r
    m.fuse_tail = False
    y0 = m(x).clone()
    m.fuse_tail = True

    def psnr(a, b):
        return float(10.0 * torch.log10(255.0 ** 2 / ((a - b) ** 2).mean().clamp_min(1e-12)))
    fused, separate, between = psnr(y1, y32), psnr(y0, y32), psnr(y1, y0)
    assert fused > separate - 0.5, (fused, separate, between)
    assert between > 60.0, (fused, separate, between)
    assert torch.equal(m(x), y1)


@pytest.mark.parametrize("compute,post", [("f16", True), ("f16", False), ("bf16", False)])
@pytest.mark.parametrize("n,c,hw,pc", [pytest.param(1, 48, (270, 480), 24, id="1-48-hw0"), pytest.param(6, 40, (144, 160), 20, id="6-40-hw1"),
                                       pytest.param(3, 48, (250, 203), 24, id="3-48-hw2"),
                                       # other widths: c over 33 .. 48, the post 1x1's two output tiles over 17 .. 32
                                       (8, 33, (128, 128), 17), (8, 41, (128, 128), 24), (8, 47, (128, 128), 32)])
def test_esdb_r_on_conv64m_matches_fp64_reference(compute, post, n, c, hw, pc):
    """conv64m_kernel<.., 3, true>: ESDB's c{j}_r (team18_bsrn.py:150-163) -- gelu(dense BSConvU(x) + table row + x) over 48 physical channels,
    plain or (fp16) with the next distillation Linear + GELU behind it -- against fp64 on the same 16-bit inputs, the blob's effective weights and
    the exact GELU (the kernel's polynomial: |error| <= 1.3e-4 on [-4, 4], 2.13e-4 below -4)."""
    from ntire2022_esr_amd import _lib as L
    dt = DT[compute]
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ksize = n, hw[0], hw[1], c, c, 3
    d.in_layout = d.out_layout = L.NHWC
    d.storage = L.STORE[compute]
    assert L.lib().esr_conv_block_waves(ctypes.byref(d)) == 1
    case = P.esdb_r(compute, post, n, c, hw, pc)
    ref = case.refs[0]
    for it in range(2):
        out, names = (case.outs, case.names) if it == 0 else case.extra["launch"]()
        assert len(names) == 1 and names[0].startswith(f"conv64m_kernel<{_tf(compute)}, {'true' if post else 'false'}, false, 3, true>"), names
        torch.cuda.synchronize()
        y, yp = out if post else (out[0], None)
        got = y.permute(0, 3, 1, 2)[:, :c].double()
        bad = int(((got - ref).abs() > _tol(ref, dt, 2.6e-4)).sum())
        assert bad == 0, (bad, float((got - ref).abs().max()))
        assert torch.all(y[..., c:] == 0)
        if post:
            pref = case.extra["post_ref"](got)
            gp = yp.permute(0, 3, 1, 2)[:, :pc].double()
            badp = int(((gp - pref).abs() > _tol(pref, dt, 4e-4)).sum())
            assert badp == 0, (badp, float((gp - pref).abs().max()))
            assert torch.all(yp[..., pc:] == 0)
