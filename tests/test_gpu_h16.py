"""-m gpu: the 16-bit-STORAGE path (bf16 / fp16 activations in HBM = MFMA operands, fp32 accumulate, one rounding at
the store).  Kernel logic is checked against an fp64 reference on the same 16-bit inputs and the blob's effective
weights (tolerance: that one rounding); the rounding itself is then bounded at network level as a PSNR shift."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _persist_cases as P
from conftest import GOLD, load_sd_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _ulp_ok(got, ref, dt):
    """got (16-bit, as float) vs the fp64 reference: one rounding (half an ulp) + the fp32 accumulation noise"""
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    tol = ref.abs() * eps * 1.01 + 3e-5 * max(1.0, float(ref.abs().max()))
    return bool(((got.double() - ref).abs() <= tol).all()), float(((got.double() - ref).abs() - tol).max())


def _same_or_one_step(a, b, dt, frac=0.03, scale=1.0):
    """two 16-bit results of the same arithmetic in another fp32 accumulation order (conv64m_kernel against conv_s16_kernel, round 6): equal but for a
    few values that sat on a rounding boundary, and those differ by one step of the storage type"""
    af, bf = a.float(), b.float()
    eps = 2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10
    step = torch.maximum(af.abs(), bf.abs()) * eps + 3e-5 * max(1.0, float(af.abs().max()))      # (+ the accumulation noise of values that cancel to ~0)
    step = step * scale
    diff = (af - bf).abs()
    ok = bool((diff <= step).all()) and float((diff > 0).float().mean()) < frac
    if not ok:
        print(f"_same_or_one_step: worst diff / step = {float((diff / step).max()):.3f}, differing fraction = {float((diff > 0).float().mean()):.4f} (limit {frac})")
    return ok


ACTS = {0: lambda t: t, 1: lambda t: F.leaky_relu(t, 0.05), 2: F.relu, 3: lambda t: F.gelu(t)}


# The layer shapes that the per-layer / separate-launch sides of the fused kernels' bit-identity cases run on conv_s16_kernel, so that each of
# those cases rests on an fp64 case of the same widths: (cin, cout, k, act, res_mode) at 23 x 37 on an input of TIGHT pitch round_up(cin, 8),
# as those launches read it (the last chunk's second half is then the next pixel's bytes, on zero weight rows)
_HFAB_W = [(33, 1), (39, 9), (44, 16), (49, 8), (51, 1), (61, 16), (62, 9), (64, 8)]                       # tests/test_gpu_fmen.py: squeeze, conv1 / conv2
_CHAIN_W = [(33, 33), (41, 34), (40, 47), (48, 48)]                                                        # tests/test_gpu_chain.py: c1_r, c2_r
WIDTH_LAYERS = sorted({(c, m, 3, 1, 0) for c, m in _HFAB_W} | {(m, m, 3, 1, 0) for _, m in _HFAB_W} |
                      {(nf, mf, 3, 1, 0) for nf, mf in _CHAIN_W} | {(mf, mf, 3, 1, 0) for _, mf in _CHAIN_W} |
                      # tests/test_gpu_esan.py: the two 3x3s, esa.conv1 at 1 / 9 / 16 channels, the identity 1x1 that adds g
                      {(32, 32, 3, 2, 0), (32, 32, 3, 0, 0), (32, 1, 1, 0, 0), (32, 9, 1, 0, 0), (32, 16, 1, 0, 0), (32, 32, 1, 0, 1)} |
                      # the single-image side of the conv48r / conv64r / conv64m cases below (c{j}_r with and without + x, c4's two output tiles)
                      {(c, c, 3, 1, 0) for c in (33, 41, 47, 49, 57, 63)} | {(c, c, 3, 1, 1) for c in (49, 57, 63)} |
                      {(49, 24, 3, 1, 0), (57, 17, 3, 1, 0), (63, 32, 3, 1, 0)})
S16_CASES = [pytest.param(*c[:3], hw, *c[3:], False, id="-".join(str(v) for v in c[:3] + (f"hw{i}",) + c[3:])) for i, (hw, c) in enumerate([
    ((16, 32), (64, 64, 3, 1, 1)), ((23, 37), (48, 48, 3, 1, 2)), ((17, 15), (48, 16, 3, 0, 0)), ((40, 56), (64, 48, 3, 1, 0)),
    ((20, 36), (50, 50, 3, 1, 1)), ((5, 3), (16, 16, 3, 2, 0)), ((33, 18), (46, 46, 1, 0, 0)), ((40, 40), (50, 25, 1, 1, 0)),
    ((19, 70), (128, 50, 1, 0, 0)), ((35, 33), (256, 50, 1, 1, 0)), ((64, 64), (48, 48, 1, 3, 2)), ((70, 50), (32, 64, 3, 1, 1))])] + \
    [pytest.param(*c[:3], (23, 37), *c[3:], True, id="-".join(str(v) for v in c[:3] + ("23x37",) + c[3:])) for c in WIDTH_LAYERS]


@pytest.mark.parametrize("compute", ["bf16", "f16"])
@pytest.mark.parametrize("cin,cout,k,hw,act,res_mode,tight", S16_CASES)
def test_s16_conv_matches_fp64_reference(compute, cin, cout, k, hw, act, res_mode, tight):
    """16-bit storage conv (esr_conv2d_f32 with storage = bf16 / f16): inputs are exact 16-bit values, the reference uses
    the EFFECTIVE weights of the packed blob (error-diffused 3x3 taps / hi + lo 1x1) in fp64, so the only differences
    are fp32 accumulation order and the single rounding of the stored result."""
    dt = DT[compute]
    case = P.s16_conv(compute, cin, cout, k, hw, act, res_mode, tight)
    names, y, ref = case.names, case.outs[0], case.refs[0].cpu()
    assert len(names) == 1 and names[0].startswith("conv_s16_kernel<"), names
    assert y.dtype == dt and y.shape[-1] == (cout + 7) // 8 * 8
    got = y.float().cpu().permute(0, 3, 1, 2)
    print(f"conv_s16 {compute} {cin}->{cout} k={k} {hw}: max|got - ref| = {float((got[:, :cout].double() - ref).abs().max()):.3e}")
    if act == 3:            # GELU in the 16-bit modes is gelu16(): |error| <= 1.3e-4 on [-4, 4] (2.13e-4 below -4, tests/_sweep.py) on top of the rounding
        assert bool(((got[:, :cout].double() - ref).abs() <= ref.abs() * 2.0 ** (-8 if dt == torch.bfloat16 else -11) * 1.01 + 2.5e-4).all())
    else:
        ok, worst = _ulp_ok(got[:, :cout], ref, dt)
        assert ok, worst
    assert torch.all(got[:, cout:] == 0)                    # pad channels of the 16-byte granule are written as zeros


@pytest.mark.parametrize("compute", ["bf16", "f16"])
@pytest.mark.parametrize("n,cin,cout,k,hw,res_mode", [
    (1, 64, 64, 3, (270, 480), 0), (1, 64, 64, 3, (270, 480), 2), (1, 64, 64, 1, (270, 480), 2), (1, 48, 48, 3, (339, 510), 2),
    (1, 64, 64, 3, (339, 510), 1), (3, 48, 48, 3, (256, 256), 0), (1, 16, 16, 3, (270, 480), 1), (5, 50, 50, 1, (200, 200), 0),
    (2, 48, 48, 3, (339, 510), 0), (1, 40, 44, 3, (339, 510), 0)])      # three output tiles, no HBM residual, >= 256 tiles: conv48r_kernel (48 channels)
def test_s16_conv_more_tiles_than_blocks(compute, n, cin, cout, k, hw, res_mode):
    """Shapes with MORE 16x32 tiles than the 256 persistent blocks and partial tiles at both edges: the tile-to-tile path of a
    block (the epilogue of tile k inside the first MFMA group of tile k+1, residual registers reused across tiles, unequal
    tile counts per block, the drain iteration) -- the small shapes above give every block at most one tile.  The 3x3s over 48
    physical channels without a residual from HBM take conv48r_kernel (esr_conv_block_waves == 1)."""
    from ntire2022_esr_amd import ops
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    dt = DT[compute]
    g = torch.Generator().manual_seed(n + cin + cout + hw[0] + k)
    cp = (cin + 15) // 16 * 16
    x = torch.randn(n, cin, *hw, generator=g).to(dt)
    r = torch.randn(n, cout, *hw, generator=g).to(dt)
    w = torch.randn(cout, cin, k, k, generator=g) * (0.1 if k == 3 else 0.2)
    b = torch.randn(cout, generator=g)
    blob = pack_conv_s16(w, b, compute, cin_phys=cp)
    weff, _ = unpack_conv_s16(blob, cin, cout, k, compute, cin_phys=cp)
    conv = F.conv2d(x.double().to(DEV), weff.double().to(DEV), b.double().to(DEV), padding=k // 2)
    rd = r.double().to(DEV)
    ref = ACTS[1](conv + rd) if res_mode == 1 else (ACTS[1](conv) + rd if res_mode == 2 else ACTS[1](conv))
    xin = F.pad(_nhwc(x), (0, cp - cin)).to(DEV)
    rp = F.pad(_nhwc(r), (0, (-cout) % 8)).to(DEV) if res_mode else None
    for _ in range(3):                  # a race would not show every time
        y = ops.conv2d(xin, w, b, act=1, res=rp, res_mode=res_mode, cin=cin, packed=blob.to(DEV))
        got = y.permute(0, 3, 1, 2)[:, :cout].double()
        eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
        tol = ref.abs() * eps * 1.01 + 3e-5 * max(1.0, float(ref.abs().max()))
        bad = int(((got - ref).abs() > tol).sum())
        assert bad == 0, bad


@pytest.mark.parametrize("compute", ["bf16", "f16"])
@pytest.mark.parametrize("nseg,pp,cout,hw,res_mode", [(4, 32, 48, (40, 56), 0), (4, 16, 64, (33, 70), 1), (2, 48, 50, (270, 480), 0), (5, 16, 16, (20, 20), 2)])
def test_s16_segmented_input_equals_dense_concat(compute, nseg, pp, cout, hw, res_mode):
    """esr_conv_desc.in_seg_stride / in_seg_chunks: the 1x1 over a concat kept as `nseg` dense tensors must give exactly what it
    gives on the dense [.., nseg * pp] buffer holding the same channels (same blob, same chunk order, same arithmetic)."""
    from ntire2022_esr_amd import ops
    dt = DT[compute]
    g = torch.Generator().manual_seed(nseg + pp + cout)
    xs = torch.randn(nseg, 2, *hw, pp, generator=g).to(dt).to(DEV)                # planar
    xd = torch.cat([xs[j] for j in range(nseg)], dim=-1).contiguous()             # dense concat
    w = torch.randn(cout, nseg * pp, generator=g) * 0.1
    b = torch.randn(cout, generator=g)
    r = torch.randn(2, *hw, (cout + 7) // 8 * 8, generator=g).to(dt).to(DEV) if res_mode else None
    yd = ops.conv2d(xd, w, b, act=1, res=r, res_mode=res_mode)
    ys = ops.conv2d(xs, w, b, act=1, res=r, res_mode=res_mode)
    assert torch.equal(yd, ys)


@pytest.mark.parametrize("compute", ["bf16", "f16"])
def test_s16_split_store_slices_and_shuffle(compute):
    """channel-split store (IMDBlock: 16 -> concat slice, 48 -> next conv), reads from / writes into slices of wider
    buffers, and the PixelShuffle(4) tail writing the fp32 NCHW network output"""
    from ntire2022_esr_amd import ops
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    dt = DT[compute]
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, 64, 37, 21, generator=g).to(dt)
    w = torch.randn(64, 64, 3, 3, generator=g) * 0.1
    b = torch.randn(64, generator=g)
    weff, _ = unpack_conv_s16(pack_conv_s16(w, b, compute), 64, 64, 3, compute)
    ref = F.leaky_relu(F.conv2d(x.double(), weff.double(), b.double(), padding=1), 0.05)
    cat = torch.zeros(1, 37, 21, 64, dtype=dt, device=DEV)
    nxt = torch.zeros(1, 37, 21, 48, dtype=dt, device=DEV)
    wide = torch.zeros(1, 37, 21, 128, dtype=dt, device=DEV)
    wide[..., 64:] = _nhwc(x).to(DEV)
    ops.conv2d(wide, w, b, act=1, in_coff=64, cin=64, split=16, out=cat, out_coff=32, out1=nxt)
    ok, worst = _ulp_ok(cat[..., 32:48].float().cpu().permute(0, 3, 1, 2), ref[:, :16], dt)
    assert ok, worst
    ok, worst = _ulp_ok(nxt.float().cpu().permute(0, 3, 1, 2), ref[:, 16:], dt)
    assert ok, worst
    assert torch.all(cat[..., :32] == 0) and torch.all(cat[..., 48:] == 0)
    # PixelShuffle tail: 16-bit NHWC in, fp32 NCHW out (no rounding of the result)
    w2 = torch.randn(48, 64, 3, 3, generator=g) * 0.1
    b2 = torch.randn(48, generator=g)
    w2e, _ = unpack_conv_s16(pack_conv_s16(w2, b2, compute), 64, 48, 3, compute)
    y = ops.conv2d(_nhwc(x).to(DEV), w2, b2, shuffle_out=True)
    ref2 = F.pixel_shuffle(F.conv2d(x.double(), w2e.double(), b2.double(), padding=1), 4)
    assert y.dtype == torch.float32 and tuple(y.shape) == (1, 3, 148, 84)
    assert float((y.cpu().double() - ref2).abs().max()) < 3e-5 * float(ref2.abs().max())


@pytest.mark.parametrize("compute", ["bf16", "f16"])
def test_s16_head_from_nchw_fp32(compute):
    """network head of a 16-bit network: fp32 NCHW input (exact), fp32 MFMA, NHWC result stored as 16-bit"""
    from ntire2022_esr_amd import ops
    dt = DT[compute]
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 3, 33, 29, generator=g) * 255
    w = torch.randn(46, 3, 3, 3, generator=g) * 0.05
    b = torch.randn(46, generator=g)
    y = ops.conv2d(x.to(DEV), w, b, in_nchw=True, store=compute)
    assert y.dtype == dt and y.shape[-1] == 48
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    ok, worst = _ulp_ok(y.float().cpu().permute(0, 3, 1, 2)[:, :46], ref, dt)
    assert ok, worst
    assert torch.all(y[..., 46:] == 0)


# RLFN's widths (mf = 48 -> nf = 46 -> 46 -> 16) at every size under the ids they always had; the widths of tests/test_gpu_chain.py's new cases
# (their third launch) at the small size
RLFB_CASES = [pytest.param(n, hw, 48, 46, 16, id=f"{n}-hw{i}") for i, (n, hw) in enumerate([(2, (37, 29)), (1, (256, 250)), (2, (339, 510)), (3, (200, 123))])] + \
             [pytest.param(2, (37, 29), mf, nf, f, id=f"2-37x29-{mf}-{nf}-{f}") for nf, mf, f in [(33, 33, 1), (41, 34, 8), (40, 47, 9), (48, 48, 16)]]


@pytest.mark.parametrize("compute", ["bf16", "f16"])
@pytest.mark.parametrize("n,hw,mf,nf,f", RLFB_CASES)
def test_s16_post_chain_rlfb(compute, n, hw, mf, nf, f):
    """RLFB tail in one launch: u = lrelu(c3_r(x)) + r (never stored), v = c5(u), c1 = esa.conv1(v): the 1x1s run on the fp32
    tile (hi + lo operands), only v and c1 are rounded -- against fp64 with the blob's effective 3x3 weights.  The small shape runs
    on conv_s16_kernel, the others (>= 256 tiles of 16 x 16, < 1024 of 16 x 32) on conv48rp_kernel: weights in registers, the residual
    staged by each wave for its own rows, ragged edges in both directions."""
    dt = DT[compute]
    case = P.rlfb_post(compute, n, hw, mf, nf, f, 21 + n + hw[0])
    y, (yv, yc), (v, c1) = case.extra["main"], case.outs, [t.cpu() for t in case.refs]
    assert y is None and yv.dtype == dt and yv.shape[-1] == (nf + 7) // 8 * 8 and yc.shape[-1] == (f + 7) // 8 * 8
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11

    def close(got, want):
        # one rounding of the stored value + the dropped lo x lo terms of the hi/lo split (2^-16 bf16 / 2^-22 fp16 relative)
        # fp16: + the chain operands that sit on a rounding boundary in fp32 and round the other way in this fp64 reference
        # (|w| * ulp each, a handful per output)
        slack = (1e-3 * 32 if compute == "bf16" else 0.5) * eps * max(1.0, float(want.abs().max()))
        tol = want.abs() * eps * 1.01 + slack
        err = (got.double() - want).abs()
        if compute == "f16" and want.numel() > 1e6:
            # large images: the boundary cases are a fixed small FRACTION of the outputs, and a few of them stack up
            print(f"fraction beyond tol {float((err > tol).double().mean()):.2e}, worst {float((err / tol).max()):.2f} x tol")
            return float((err > tol).double().mean()) <= 2e-5 and bool((err <= 3 * tol).all())
        return bool((err <= tol).all())

    assert close(yv.float().cpu().permute(0, 3, 1, 2)[:, :nf], v)
    assert close(yc.float().cpu().permute(0, 3, 1, 2)[:, :f], c1)
    assert torch.all(yv[..., nf:] == 0) and torch.all(yc[..., f:] == 0)


@pytest.mark.parametrize("compute", ["bf16", "f16"])
@pytest.mark.parametrize("nf", [50, 40])
def test_s16_post_rfdb(compute, nf):
    """RFDB: r = lrelu(c_r(x) + x) stored, d = lrelu(c_d(r)) from the same launch (rfdn_baseline/block.py:150-160)"""
    from ntire2022_esr_amd import ops
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    dt = DT[compute]
    dc = nf // 2
    g = torch.Generator().manual_seed(nf)
    P = (nf + 15) // 16 * 16
    x = torch.randn(1, nf, 45, 33, generator=g).to(dt)
    w, b = torch.randn(nf, nf, 3, 3, generator=g) * 0.08, torch.randn(nf, generator=g)
    wd, bd = torch.randn(dc, nf, generator=g) * 0.2, torch.randn(dc, generator=g)
    weff, _ = unpack_conv_s16(pack_conv_s16(w, b, compute, cin_phys=P), nf, nf, 3, compute, cin_phys=P)
    rr = F.leaky_relu(F.conv2d(x.double(), weff.double(), b.double(), padding=1) + x.double(), 0.05)
    # hi + lo post weights for both shapes (the epilogue needs no LDS scratch any more: the low-part images fit next to nf = 50's
    # 80 KB of 3x3 weights too)
    # (fp16: the chain multiplies the fp16 roundings of the fp32 tile and of the weights, see test_s16_post_chain_rlfb)
    q = (lambda t: t) if compute == "bf16" else (lambda t: t.to(torch.float16).double())
    wd_eff = q(wd.double())
    dd = F.leaky_relu(F.conv2d(q(rr), wd_eff[:, :, None, None], bd.double()), 0.05)
    xin = F.pad(_nhwc(x), (0, P - nf)).to(DEV)
    y, yd = ops.conv2d(xin, w, b, act=1, res=xin, res_mode=1, cin=nf, post_weight=wd, post_bias=bd, post_act=1)
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11

    def close(got, want):
        slack = (2e-2 if compute == "bf16" else 0.5) * eps * max(1.0, float(want.abs().max()))      # fp16: see test_s16_post_chain_rlfb
        tol = want.abs() * eps * 1.01 + slack
        return bool(((got.double() - want).abs() <= tol).all())

    assert close(y.float().cpu().permute(0, 3, 1, 2)[:, :nf], rr)
    assert close(yd.float().cpu().permute(0, 3, 1, 2)[:, :dc], dd)


def test_s16_rejects_bad_descriptors():
    from ntire2022_esr_amd import _lib as L, ops
    x = torch.zeros(1, 8, 8, 16, dtype=torch.bfloat16, device=DEV)            # pitch 16 < round_up(cin, 8) = 24: the pixel does not hold the channels
    with pytest.raises(L.EsrError):
        ops.conv2d(x, torch.randn(16, 24, 3, 3), torch.randn(16))
    x = torch.zeros(1, 8, 8, 80, dtype=torch.float16, device=DEV)             # 3x3 with 80 input channels: weights do not fit LDS
    with pytest.raises(L.EsrError):
        ops.conv2d(x, torch.randn(64, 80, 3, 3), torch.randn(64))


@pytest.mark.parametrize("compute", ["bf16", "f16"])
@pytest.mark.parametrize("cin,cout,k,hw,n", [(24, 16, 3, (19, 23), 2), (50, 50, 3, (40, 37), 1), (50, 25, 1, (33, 18), 2), (50, 50, 3, (256, 256), 1), (40, 64, 3, (256, 272), 1)])
def test_tight_pitch_equals_whole_chunk_pitch(compute, cin, cout, k, hw, n):
    """TIGHT PITCH (round 6, esr_conv2d_s16): an input whose pixels hold round_up(cin, 8) channels -- 56 for RFDN's nf = 50, 112-byte pixels --
    instead of whole 16-channel K chunks.  The last chunk's second half is then the next pixel's first 16 bytes (NON-zero here: random data) and
    meets zero weight rows: the result is bit-identical to the same convolution on the zero-padded whole-chunk tensor, on the general kernel and
    (>= 256 tiles, 64 -> 64) on conv64m_kernel."""
    from ntire2022_esr_amd import ops
    dt = torch.bfloat16 if compute == "bf16" else torch.float16
    g = torch.Generator().manual_seed(cin + cout + hw[0])
    p8, p16 = (cin + 7) // 8 * 8, (cin + 15) // 16 * 16
    xt = torch.randn(n, *hw, p8, generator=g).to(dt)
    xt[..., cin:] = 0                                   # the pad channels inside the pixel are zeros, as every producer leaves them
    xp = torch.zeros(n, *hw, p16, dtype=dt)
    xp[..., :p8] = xt
    w, b = torch.randn(cout, cin, k, k, generator=g) * 0.1, torch.randn(cout, generator=g)
    xt_d, xp_d = xt.to(DEV), xp.to(DEV)
    y_t = ops.conv2d(xt_d, w, b, act=1)
    y_p = ops.conv2d(xp_d, w, b, act=1)
    assert y_t.shape[-1] >= cout and bool(torch.isfinite(y_t.float()).all())
    assert torch.equal(y_t[..., :cout], y_p[..., :cout])
    if cin == cout and k == 3:
        # RFDB's c{j}_r: + the input itself, before the activation (taken from the staged tile: the neighbour pixel's bytes land in channels that
        # are not stored)
        r_t = ops.conv2d(xt_d, w, b, act=1, res=xt_d, res_mode=1)
        r_p = ops.conv2d(xp_d, w, b, act=1, res=xp_d, res_mode=1)
        assert torch.equal(r_t[..., :cout], r_p[..., :cout]) and not torch.equal(r_t[..., :cout], y_t[..., :cout])


@pytest.mark.parametrize("mid,compute,max_dpsnr", [(-1, "f16", 0.005), (-1, "bf16", 0.01), (0, "bf16", 0.01), (4, "bf16", 0.01),
                                                   (4, "f16", 0.005), (18, "f16", 0.005), (0, "f16", 0.005), (18, "bf16", 0.01)])
def test_network_psnr_shift(mid, compute, max_dpsnr):
    """PSNR of the 16-bit-operand network vs the fp32 network's PSNR on the natural image (64x64 bicubic LR of
    utils/test.bmp -> 256x256 vs the original): |dPSNR| budget per SURVEY 8c / BASELINE.md section 4: fp16 <= 0.005 dB,
    bf16 <= 0.01 dB (the stated-size cases against the REFERENCE's PSNR are in test_gpu_big.py)."""
    from PIL import Image
    from ntire2022_esr_amd import image_util as util
    from ntire2022_esr_amd.registry import select_model
    model, name, dr, _ = select_model(mid, torch.device(DEV))
    hr = np.array(Image.open(os.path.join(GOLD, "test.bmp")).convert("RGB"))
    lr = np.array(Image.fromarray(hr).resize((64, 64), Image.BICUBIC))
    x = util.uint2tensor4(lr, dr).to(DEV)
    p32 = util.calculate_psnr(util.tensor2uint(model(x), dr), hr, border=4)
    y32 = model(x).clone()
    model.set_compute(compute)
    y16 = model(x)
    p16 = util.calculate_psnr(util.tensor2uint(y16, dr), hr, border=4)
    rel = float((y16 - y32).abs().max()) / dr
    print(f"{name} {compute}: PSNR {p32:.4f} -> {p16:.4f} dB (d = {p16 - p32:+.4f}), max|dy|/data_range = {rel:.2e}")
    # (rounds 2-3 allowed this single 4 k-pixel image 1.5 x the dataset-mean budget: RLFN bf16 sat at -0.011 dB; with the long skip in
    # hi + lo pairs -- round 4 -- it is -0.005 dB and the budget itself holds)
    assert abs(p16 - p32) < max_dpsnr
    model.set_compute("f32")
    assert torch.equal(model(x), y32)                       # switching back restores the exact fp32 path


@pytest.mark.parametrize("compute", ["bf16", "f16"])
@pytest.mark.parametrize("cin,cout,act,res_in,border,hw,n", [
    (48, 48, 1, False, False, (128, 128), 8),      # RLFB c1_r / c2_r: plain, LeakyReLU
    (46, 46, 1, False, False, (150, 97), 9),       # logical 46 channels, ragged edges, tiles not a multiple of the grid
    (48, 48, 3, True, True, (128, 128), 8),        # ESDB c{j}_r as a dense BSConvU: + input, border table, GELU
    (48, 48, 3, True, True, (90, 130), 12),
    (48, 24, 3, False, True, (128, 128), 8),       # ESDB c4: two output tiles
    (48, 48, 0, True, False, (128, 128), 8),       # residual == input without activation
    (48, 48, 1, False, False, (128, 128), 32),     # >= 1024 tiles of 16 x 32: the 8-rows-per-wave shape (the others: 16 x 16 tiles)
    (48, 48, 3, True, True, (128, 120), 33),
    # other widths of the three-chunk range 33 .. 48 at the kernel's threshold, 256 tiles of 16 x 32: both ends and one past a 16-byte granule
    (33, 33, 1, False, False, (128, 128), 8), (41, 41, 1, False, False, (128, 128), 8), (47, 47, 1, False, False, (128, 128), 8)])
def test_conv48r_equals_conv_s16(compute, cin, cout, act, res_in, border, hw, n):
    """conv48r_kernel (3x3 over 48 physical input channels, >= 256 tiles of 16 x 32: weights in registers, one wave per SIMD, row pairs
    as the outer loop) against conv_s16_kernel: the batch takes the new kernel (esr_conv_block_waves == 1), each image alone the old
    one (<= 72 tiles), same packed weights -- bit-identical results, and both within storage precision of the fp64 convolution."""
    from ntire2022_esr_amd import _lib as L
    dt = DT[compute]
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ksize = n, hw[0], hw[1], cin, cout, 3
    d.in_layout = d.out_layout = L.NHWC
    d.storage = L.STORE[compute]
    assert L.lib().esr_conv_block_waves(ctypes.byref(d)) == 1
    d.n = 1
    assert L.lib().esr_conv_block_waves(ctypes.byref(d)) != 1
    case = P.conv48r(compute, n, hw, cin, cout, act, res_in, border)
    names, y = case.names, case.outs[0]
    bf = "true" if compute == "bf16" else "false"
    want = f"conv64m_kernel<{bf}, false, false, 3, true>" if act == 3 and res_in and border and cout > 32 else \
        f"conv48r_kernel<{bf}, {(cout + 15) // 16}, {'true' if cout <= 32 or border or res_in or act == 3 else 'false'}, "
    assert len(names) == 1 and names[0].startswith(want), names
    for i in range(n):
        y1 = case.chunk(i, i + 1)[0][0]
        if act == 3 and res_in and border and cout > 32:
            # ESDB's c{j}_r shape: since round 6 the batch runs on conv64m_kernel<.., 3, true> (v_mfma_f32_32x32x16, another accumulation order;
            # its fp64-reference check: test_gpu_c64m.py) -- equal but for values on a rounding boundary, those one storage step apart
            assert _same_or_one_step(y[i:i + 1], y1, dt), i
        else:
            assert torch.equal(y[i:i + 1], y1), i
    if not border:
        ref = case.refs[0]
        got = y.permute(0, 3, 1, 2)[:, :cout].double()
        eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
        tol = ref.abs() * eps * 1.01 + (3e-4 if act == 3 else 5e-5) * max(1.0, float(ref.abs().max()))
        assert int(((got - ref).abs() > tol).sum()) == 0


@pytest.mark.parametrize("compute", ["bf16", "f16"])
@pytest.mark.parametrize("hw,n,mf,nf,f", [
    pytest.param((128, 128), 8, 48, 46, 16, id="hw0-8"), pytest.param((100, 77), 9, 48, 46, 16, id="hw1-9"),
    # other widths of the ranges: both ends and one past a 16-byte granule (mf -> nf with the block input, nf -> nf, nf -> f)
    ((128, 128), 8, 33, 33, 1), ((128, 128), 8, 34, 41, 8), ((128, 128), 8, 47, 40, 9)])
def test_conv48rp_equals_conv_s16(compute, hw, n, mf, nf, f):
    """conv48rp_kernel (RLFB c3_r + block input -> c5 -> esa.conv1: weights in registers, 16 x 16 tiles, the residual staged by each wave
    for its own rows, post images in LDS, the chain on both rows of a pair) against conv_s16_kernel: the batch takes the new kernel
    (>= 256 tiles of 16 x 16), each image alone the old one -- both outputs bit-identical, ragged edges included."""
    tiles16 = lambda nn: nn * ((hw[1] + 15) // 16) * ((hw[0] + 15) // 16)
    assert tiles16(n) >= 256 and tiles16(1) < 256
    case = P.rlfb_post(compute, n, hw, mf, nf, f, hw[0] + n)
    names, y, (yv, yc) = case.names, case.extra["main"], case.outs
    assert len(names) == 1 and names[0].startswith(f"conv48rp_kernel<{'true' if compute == 'bf16' else 'false'}, false>"), names
    assert y is None
    for i in range(n):
        v1, c1 = case.chunk(i, i + 1)[0]
        assert torch.equal(yv[i:i + 1], v1) and torch.equal(yc[i:i + 1], c1), i


def _hilo(t, cp):
    """NCHW fp32 -> bf16 pair [2, N, H, W, cp]: high parts, low parts (value = hi + lo; pad channels zero)"""
    t = F.pad(_nhwc(t), (0, cp - t.shape[1]))
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous()


@pytest.mark.parametrize("n,c,hw", [(2, 46, (37, 29)), (1, 50, (64, 80)), (3, 48, (100, 77)), (1, 64, (339, 510))])
def test_s16_hilo_skip_convs(n, c, hw):
    """esr_conv_desc.hilo (ABI v10): the three convolutions of the long skip on hi + lo tensors.
    head:       y = conv(x16)              -> hi + lo out: the high parts ARE the plain kernel's output (bit-identical), hi + lo is
                                              the fp64 result to 2^-16 relative (two bf16 numbers) instead of 2^-8
    LR_conv:    y = conv(x16) + (r_hi + r_lo)  -> hi + lo out, same bound
    upsampler:  y = shuffle(conv(x_hi + x_lo))  against the fp64 convolution of the SUM with the blob's effective weights"""
    from ntire2022_esr_amd import _lib as L, ops
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    cp = (c + 15) // 16 * 16
    head = P.hilo_head(n, c, c, hw)
    e = head.extra
    g, x, r32, w, b, blob, xin, conv, plain = e["g"], e["x"], e["r32"], e["w"], e["b"], e["blob"], e["xin"], e["conv"].cpu(), e["plain"]

    def check(y, ref, what):
        assert y.dtype == torch.bfloat16 and tuple(y.shape) == (2, n, *hw, cp)
        hi, lo = y[0].float().cpu(), y[1].float().cpu()
        got = (hi.double() + lo.double()).permute(0, 3, 1, 2)[:, :c]
        tol = ref.abs() * 2.0 ** -15 + 3e-5 * max(1.0, float(ref.abs().max()))           # fp32 accumulation noise dominates
        assert bool(((got - ref).abs() <= tol).all()), (what, float(((got - ref).abs() - tol).max()))
        assert float((lo.abs() > hi.abs() * 2.0 ** -7 + 1e-30).float().mean()) < 1e-3, what         # the low parts are remainders of the high ones
        return hi

    hi = check(head.outs[0], conv, "head")
    assert torch.equal(hi[..., :plain.shape[-1]], plain.float().cpu()), "the high parts are the plain kernel's output"
    rin = _hilo(r32, cp).to(DEV)
    rsum = (rin[0].double() + rin[1].double()).cpu().permute(0, 3, 1, 2)[:, :c]
    y = ops.conv2d(xin, w, b, cin=c, packed=blob.to(DEV), res=rin, res_mode=1, hilo=L.HILO_RES | L.HILO_OUT)
    check(y, conv + rsum, "LR_conv")
    # upsampler: 48 output channels, pixel shuffle, hi + lo input
    wu = torch.randn(48, c, 3, 3, generator=g) * 0.1
    bu = torch.randn(48, generator=g)
    blobu = pack_conv_s16(wu, bu, "bf16", cin_phys=cp)
    weffu, _ = unpack_conv_s16(blobu, c, 48, 3, "bf16", cin_phys=cp)
    x32 = torch.randn(n, c, *hw, generator=g) * 2.0
    xh = _hilo(x32, cp).to(DEV)
    xsum = (xh[0].double() + xh[1].double()).cpu().permute(0, 3, 1, 2)[:, :c]
    ref = F.pixel_shuffle(F.conv2d(xsum, weffu.double(), bu.double(), padding=1), 4)
    yu = ops.conv2d(xh, wu, bu, cin=c, packed=blobu.to(DEV), shuffle_out=True, hilo=L.HILO_IN)
    assert yu.dtype == torch.float32 and tuple(yu.shape) == (n, 3, 4 * hw[0], 4 * hw[1])
    err = float((yu.double().cpu() - ref).abs().max())
    assert err <= 3e-5 * max(1.0, float(ref.abs().max())), err
    # and the same input WITHOUT its low parts is off by the bf16 rounding of x: the low half is really read
    y0 = ops.conv2d(xh[0], wu, bu, cin=c, packed=blobu.to(DEV), shuffle_out=True)
    assert float((y0.double().cpu() - ref).abs().max()) > 20 * err


def test_s16_hilo_rejects_what_it_does_not_cover():
    from ntire2022_esr_amd import _lib as L, ops
    x = torch.zeros(1, 20, 20, 32, dtype=torch.bfloat16, device=DEV)
    w, b = torch.zeros(32, 32, 3, 3), torch.zeros(32)
    with pytest.raises(L.EsrError):                      # two output tiles: no hi + lo kernel
        ops.conv2d(x, w, b, hilo=L.HILO_OUT)
    x = torch.zeros(1, 20, 20, 48, dtype=torch.float16, device=DEV)
    w, b = torch.zeros(48, 48, 3, 3), torch.zeros(48)
    with pytest.raises(L.EsrError):                      # fp16 storage: 11 bits already
        ops.conv2d(x, w, b, hilo=L.HILO_OUT)
    x = torch.zeros(1, 20, 20, 48, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(L.EsrError):                      # the input is not a pair
        ops.conv2d(x, w, b, hilo=L.HILO_IN)
    x = torch.zeros(2, 1, 20, 20, 48, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(L.EsrError):                      # 1x1: not covered
        ops.conv2d(x, torch.zeros(48, 48, 1, 1), b, hilo=L.HILO_IN)


@pytest.mark.parametrize("compute", ["bf16", "f16"])
@pytest.mark.parametrize("cin,cout,act,res_in,hw,n", [
    (64, 64, 1, False, (128, 128), 4),       # plain, LeakyReLU
    (50, 50, 1, True, (100, 77), 9),         # RFDB c{j}_r: lrelu(conv(x) + x), 50 logical channels in 64, ragged edges
    (64, 32, 1, False, (128, 128), 5),       # RFDB c4: two output tiles
    (50, 25, 1, False, (64, 250), 7),
    (64, 64, 0, True, (128, 128), 4),        # residual == input without activation
    # other widths of the four-chunk range 49 .. 64 at the kernels' threshold, 256 tiles of 16 x 16 with a ragged right edge: four output tiles
    # (conv64m_kernel) and two (conv64r_kernel, 17 .. 32 outputs: both ends and a whole granule)
    (49, 49, 1, True, (128, 120), 4), (57, 57, 1, False, (128, 120), 4), (63, 63, 0, True, (128, 120), 4),
    (49, 24, 1, False, (128, 120), 4), (57, 17, 1, False, (128, 120), 4), (63, 32, 1, False, (128, 120), 4)])
def test_conv64r_equals_conv_s16(compute, cin, cout, act, res_in, hw, n):
    """The 3x3s over 64 physical input channels at >= 256 tiles of 16 x 16 (one wave per SIMD, weights in registers, row pairs as the outer
    loop, 160-byte LDS pixels) against conv_s16_kernel: the batch takes the register-resident kernel (esr_conv_block_waves == 1), each image
    alone the general one (< 256 tiles), same packed weights.  Two output tiles: conv64r_kernel, bit-identical results; four: conv64m_kernel
    (round 6, 32x32x16 MFMAs and nine taps: another accumulation order), equal to one storage step.  Both within storage precision of the
    fp64 convolution."""
    from ntire2022_esr_amd import _lib as L
    dt = DT[compute]
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ksize = n, hw[0], hw[1], cin, cout, 3
    d.in_layout = d.out_layout = L.NHWC
    d.storage = L.STORE[compute]
    assert L.lib().esr_conv_block_waves(ctypes.byref(d)) == 1
    d.n = 1
    assert L.lib().esr_conv_block_waves(ctypes.byref(d)) != 1
    case = P.conv64(compute, n, hw, cin, cout, act, res_in)
    names, y = case.names, case.outs[0]
    bf = "true" if compute == "bf16" else "false"
    assert len(names) == 1 and names[0].startswith(f"conv64m_kernel<{bf}, false, false, 4, false>" if cout > 48 else f"conv64r_kernel<{bf}, 2,"), names
    for i in range(n):
        y1 = case.chunk(i, i + 1)[0][0]
        if cout > 48:      # 64 outputs: the batch runs on conv64m_kernel (32x32x16 MFMAs, nine taps, another accumulation order) since round 6
            assert _same_or_one_step(y[i:i + 1], y1, dt), i
        else:
            assert torch.equal(y[i:i + 1], y1), i
    ref = case.refs[0]
    got = y.permute(0, 3, 1, 2)[:, :cout].double()
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    tol = ref.abs() * eps * 1.01 + (3e-4 if act == 3 else 5e-5) * max(1.0, float(ref.abs().max()))
    assert int(((got - ref).abs() > tol).sum()) == 0


@pytest.mark.parametrize("hw,n,c,act", [((128, 128), 8, 48, 0), ((100, 77), 9, 46, 0), ((64, 250), 5, 46, 1),
                                        ((128, 128), 8, 33, 0), ((128, 128), 8, 41, 0), ((128, 128), 8, 47, 1)])      # other widths of 33 .. 48
def test_conv48rl_equals_conv_s16(hw, n, c, act):
    """conv48rp_kernel<bf16, LRS> (the LR conv of a 48-channel network on hi + lo pairs: residual pair staged by each wave for its own rows,
    (conv + hi) + lo, hi / lo stores) against conv_s16_kernel's HILO instantiation: the batch takes the new kernel (>= 256 tiles of
    16 x 16, esr_conv_block_waves == 1), each image alone the old one -- both tensors of the output pair bit-identical, ragged edges
    included; and hi + lo is the fp64 result to two bf16 numbers."""
    from ntire2022_esr_amd import _lib as L
    cp = 48
    case = P.lr_hilo(n, c, hw, act, cp)
    names, y, rin = case.names, case.outs[0], case.extra["rin"]
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ksize = n, hw[0], hw[1], c, c, 3
    d.in_layout = d.out_layout = L.NHWC
    d.storage, d.act, d.res_mode, d.hilo, d.hilo_stride = L.STORE["bf16"], act, L.RES_PRE_ACT, L.HILO_RES | L.HILO_OUT, 4096
    d.res = L.View(ctypes.c_void_p(rin.data_ptr()), cp, 0)
    assert L.lib().esr_conv_block_waves(ctypes.byref(d)) == 1
    d.n = 1
    assert L.lib().esr_conv_block_waves(ctypes.byref(d)) == 8
    assert len(names) == 1 and names[0].startswith("conv48rp_kernel<true, true>"), names
    assert tuple(y.shape) == (2, n, *hw, cp)
    for i in range(n):
        y1 = case.chunk(i, i + 1)[0][0]
        assert torch.equal(y[:, i:i + 1], y1), i
    ref = case.refs[0]
    got = (y[0].double() + y[1].double()).permute(0, 3, 1, 2)[:, :c]
    tol = ref.abs() * 2.0 ** -15 + 3e-5 * max(1.0, float(ref.abs().max()))
    assert int(((got - ref).abs() > tol).sum()) == 0


@pytest.mark.parametrize("c,pc,hw", [(50, 25, (40, 56)), (48, 24, (64, 80))])
def test_s16_hilo_head_with_post(c, pc, hw):
    """ESR_HILO_OUT + one post 1x1 (the head of RFDN / BSRN in bf16: block 1's first distillation conv in its epilogue): the pair's high
    parts and the post output are the plain post-chain kernel's, bit for bit; hi + lo carries the fp32 result."""
    from ntire2022_esr_amd import _lib as L, ops
    g = torch.Generator().manual_seed(c + hw[0])
    x = torch.randn(2, hw[0], hw[1], 16, generator=g).to(torch.bfloat16).to(DEV)
    w, b = torch.randn(c, 9, 3, 3, generator=g) * 0.2, torch.randn(c, generator=g)
    wp, bp = torch.randn(pc, c, generator=g) * 0.2, torch.randn(pc, generator=g)
    y0, p0 = ops.conv2d(x, w, b, cin=9, post_weight=wp, post_bias=bp, post_act=1)
    y1, p1 = ops.conv2d(x, w, b, cin=9, post_weight=wp, post_bias=bp, post_act=1, hilo=L.HILO_OUT)
    assert y1.dim() == 5 and torch.equal(y1[0][..., :y0.shape[-1]], y0) and torch.equal(p1, p0)
    lo = y1[1].float()
    assert float(lo.abs().max()) > 0 and bool((lo.abs() <= y1[0].float().abs() * 2.0 ** -7 + 1e-30).all())


@pytest.mark.parametrize("hw,n,border,act,pact,c,pc", [
    pytest.param((128, 128), 8, True, 3, 3, 48, 24, id="hw0-8-True-3-3"), pytest.param((100, 77), 9, False, 3, 3, 48, 24, id="hw1-9-False-3-3"),
    pytest.param((64, 250), 5, True, 1, 1, 48, 24, id="hw2-5-True-1-1"),
    # other widths: c over 33 .. 48, the post 1x1's two output tiles over 17 .. 32
    ((128, 128), 8, False, 3, 3, 33, 17), ((128, 128), 8, True, 1, 1, 41, 24), ((128, 128), 8, False, 3, 3, 47, 32)])
def test_conv48rq_equals_conv_s16(hw, n, border, act, pact, c, pc):
    """conv48rq_kernel (fp16: ESDB c{j}_r as a dense BSConvU + input + GELU, stored, with the next distillation 1x1 + GELU as 87 micro-operations
    behind the next row pair's MFMAs) against conv_s16_kernel<3, 3, 8, .., 2, 0>: the batch takes the new kernel (>= 256 tiles of 16 x 16,
    esr_conv_block_waves == 1), each image alone the old one -- both outputs bit-identical, ragged edges and the border table included."""
    from ntire2022_esr_amd import _lib as L
    case = P.conv48rq(hw, n, border, act, pact, c, pc)
    names, (y, yp), x, blob = case.names, case.outs, case.extra["x"], case.extra["blob"]
    assert len(names) == 1 and names[0].startswith("conv64m_kernel<false, true, false, 3, true>" if border and act == 3 and pact == 3 else "conv48rq_kernel<false,"), names
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ksize = n, hw[0], hw[1], c, c, 3
    d.in_layout = d.out_layout = L.NHWC
    d.storage, d.act, d.res_mode, d.post_cout = L.STORE["f16"], act, L.RES_PRE_ACT, pc
    d.inp = d.res = L.View(ctypes.c_void_p(x.data_ptr()), 48, 0)
    d.out0 = L.View(ctypes.c_void_p(y.data_ptr()), y.shape[-1], 0)
    d.post_wpacked = ctypes.c_void_p(blob.data_ptr())                  # (any non-null pointer: the query does not read it)
    assert L.lib().esr_conv_block_waves(ctypes.byref(d)) == 1
    d.n = 1
    assert L.lib().esr_conv_block_waves(ctypes.byref(d)) == 8
    for i in range(n):
        y1, p1 = case.chunk(i, i + 1)[0]
        if border and act == 3 and pact == 3:
            # (the batch: conv64m_kernel<false, true, false, 3, true> since round 6 -- another accumulation order, see test_conv48r_equals_conv_s16)
            assert _same_or_one_step(y[i:i + 1], y1, torch.float16) and _same_or_one_step(yp[i:i + 1], p1, torch.float16, frac=0.2, scale=10.0), i
        else:
            assert torch.equal(y[i:i + 1], y1) and torch.equal(yp[i:i + 1], p1), i
    assert bool(torch.isfinite(y.float()).all()) and float(yp.float().abs().max()) > 0


@pytest.mark.parametrize("compute", ["bf16", "f16"])
@pytest.mark.parametrize("hw,n,c,pc,res_in", [((128, 128), 8, 50, 25, True), ((100, 77), 9, 64, 32, True), ((64, 250), 5, 50, 25, False),
                                              ((128, 120), 4, 49, 17, True), ((128, 120), 4, 57, 24, True), ((128, 120), 4, 63, 32, True)])      # other widths
def test_conv64m_post_agrees_with_conv_s16(compute, hw, n, c, pc, res_in):
    """conv64m_kernel<.., POST> (esr_c64m.hip, round 6: RFDB c{j}_r = lrelu(conv(x) + x), stored, with c{j+1}_d + LeakyReLU in its epilogue, on
    v_mfma_f32_32x32x16; rounds 4 / 5: conv64rq_kernel) against conv_s16_kernel<4, 3, 8, .., 2, 0>: the batch takes the register-resident kernel
    (>= 256 tiles of 16 x 16), each image alone the general one -- same weights, same arithmetic in another fp32 accumulation order: the outputs
    agree to one step of the storage type, ragged edges included (the fp64-reference check of the new kernel: test_gpu_c64m.py)."""
    from ntire2022_esr_amd import ops, _lib as L
    from ntire2022_esr_amd.engine import pack_conv_s16
    dt = DT[compute]
    g = torch.Generator().manual_seed(n * 10 + hw[0] + c)
    x = F.pad(torch.randn(n, *hw, c, generator=g), (0, 64 - c)).to(dt).to(DEV)
    w, b = torch.randn(c, c, 3, 3, generator=g) * 0.1, torch.randn(c, generator=g)
    wp, bp = torch.randn(pc, c, generator=g) * 0.2, torch.randn(pc, generator=g)
    blob = pack_conv_s16(w, b, compute, cin_phys=64).to(DEV)
    kw = dict(act=1, cin=c, packed=blob, post_weight=wp, post_bias=bp, post_act=1)
    if res_in:
        kw.update(res_mode=L.RES_PRE_ACT)
    with ops.kernel_trace() as names:
        y, yp = ops.conv2d(x, w, b, **(dict(res=x) if res_in else {}), **kw)
    assert len(names) == 1 and names[0].startswith(f"conv64m_kernel<{'true' if compute == 'bf16' else 'false'}, true, false, 4, false>"), names
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ksize = n, hw[0], hw[1], c, c, 3
    d.in_layout = d.out_layout = L.NHWC
    d.storage, d.act, d.post_cout, d.post_act = L.STORE[compute], 1, pc, 1
    d.inp = L.View(ctypes.c_void_p(x.data_ptr()), 64, 0)
    if res_in:
        d.res_mode, d.res = L.RES_PRE_ACT, d.inp
    d.out0 = L.View(ctypes.c_void_p(y.data_ptr()), y.shape[-1], 0)
    d.post_wpacked = ctypes.c_void_p(blob.data_ptr())
    assert L.lib().esr_conv_block_waves(ctypes.byref(d)) == 1
    d.n = 1
    assert L.lib().esr_conv_block_waves(ctypes.byref(d)) == 8
    for i in range(n):
        xi = x[i:i + 1].contiguous()
        y1, p1 = ops.conv2d(xi, w, b, **(dict(res=xi) if res_in else {}), **kw)
        # (round 6: the batch runs on conv64m_kernel -- same weights and arithmetic in another accumulation order)
        # (fp16: the 1x1 reads the ROUNDED activations, so a value of y that flipped by one step -- 1e-3 at |y| ~ 1 -- moves every post output it
        # feeds by up to |w| x that: a few steps of a small output)
        assert _same_or_one_step(y[i:i + 1], y1, dt) and _same_or_one_step(yp[i:i + 1], p1, dt, 0.03, 1.0 if compute == "bf16" else 10.0), i
    assert bool(torch.isfinite(y.float()).all()) and float(yp.float().abs().max()) > 0
