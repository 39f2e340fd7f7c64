"""-m gpu: FMEN (team03_fmen.py) on the MI355X.

  * the gate epilogue (ESR_RES_GATE, y = sigmoid(conv(x) + b) * r) per op against fp64 F.conv2d + sigmoid * r: fp32 within the suite's 2e-5,
    16-bit on the rounded inputs and the blob's effective weights within one rounding (test_gpu_h16.py's bound);
  * the fused HFAB (hfab_kernel, esr_conv_chain_s16 with ESR_RES_GATE) BIT-EXACT against the four per-layer launches it replaces, also with
    NaN in the input's pad slots and behind the tensor (nothing beyond channel cin is read);
  * the network against the reference's goldens (tools/gen_golden_fmen.py): fp32 e2e vectors, bf16 PSNR at 256 x 256 and 339 x 510 (fp16 storage
    is refused: the HFAB activations exceed its range);
  * bit-equalities: fuse_hfab on / off, a batch against its single images, graph replay against esr_run_ops."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
# bf16 PSNR against the reference's: measured -0.0033 dB (256 x 256) and -0.0036 dB (339 x 510), fused and per layer alike (bit-identical) -- the
# suite's usual bf16 budget.  The fixture checkpoint is the reference's ROUNDED TO BF16 (tools/gen_golden_fmen.py), so nothing here sees a weight
# bf16 cannot hold; with the unrounded checkpoint bf16 FMEN is OVER this budget (-0.0104 dB: tests/test_gpu_true_weights.py)
BUDGET = {"bf16": 0.01}
# max |y - y_ref| / data_range of the bf16 forwards on the big goldens' ::9 sample (measured 1.39e-2 at both sizes), with headroom
MAX_REL = {"bf16": 2.0e-2}


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _ulp_ok(got, ref, dt):
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    tol = ref.abs() * eps * 1.01 + 3e-5 * max(1.0, float(ref.abs().max()))
    return bool(((got.double() - ref).abs() <= tol).all()), float(((got.double() - ref).abs() - tol).max())


# (cin, cmid) of the fused HFAB's channel-width cases: both chunk counts of x (33 .. 48, 49 .. 64) with both ends of each, every residue
# 1 .. 7 of cin mod 8 (the kernel's pad-slot mask), cmid at both ends, at a whole granule and one past it
HFAB_WIDTHS = [(33, 1), (39, 9), (44, 16), (49, 8), (51, 1), (61, 16), (62, 9), (64, 8)]
_GATE_HW = [(17, 15), (5, 90), (23, 37)]
# FMEN's excitate (cmid 12 / 16 -> 50) at every size and both output pitches, under the ids it always had; then the excitate of every HFAB
# width case as the per-layer side launches it: cmid -> cin channels on an input of pitch round_up(cmid, 8) (8: the chunk's second half
# is the next pixel and meets zero weight rows), gate operand and output of pitch round_up(cin, 8)
# (16-bit storage: the fp32 kernels take no part in the fused HFAB)
GATE_CASES = [pytest.param(st, hw, pitch, cin, 50, 16, id=f"{st}-hw{i}-{pitch}-{cin}")
              for cin in (12, 16) for pitch in (56, 64) for i, hw in enumerate(_GATE_HW) for st in ("f32", "bf16", "f16")] + \
             [pytest.param(st, (23, 37), (c + 7) // 8 * 8, m, c, (m + 7) // 8 * 8, id=f"{st}-23x37-{m}-{c}") for c, m in HFAB_WIDTHS for st in ("bf16", "f16")]


@pytest.mark.parametrize("store,hw,pitch,cin,cout,xpitch", GATE_CASES)
def test_gate_epilogue_matches_fp64(store, hw, pitch, cin, cout, xpitch):
    from ntire2022_esr_amd import _lib as L, ops
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    n = 3
    c8 = (cout + 7) // 8 * 8
    g = torch.Generator().manual_seed(cin * 1000 + pitch + hw[0])
    x = torch.randn(n, cin, *hw, generator=g)
    r = torch.randn(n, cout, *hw, generator=g) * 3
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.3
    b = torch.randn(cout, generator=g)
    out = torch.zeros(n, *hw, pitch, device=DEV)
    if store == "f32":
        xin = F.pad(_nhwc(x), (0, xpitch - cin)).to(DEV)
        rin = F.pad(_nhwc(r), (0, pitch - cout)).to(DEV)
        y = ops.conv2d(xin, w, b, cin=cin, res=rin, res_mode=L.RES_GATE, out=out)
        ref = torch.sigmoid(F.conv2d(x.double(), w.double(), b.double(), padding=1)) * r.double()
        got = y.cpu().permute(0, 3, 1, 2)[:, :cout].double()
        err = float((got - ref).abs().max())
        print(f"gate f32 {cin}->{cout} {hw}: max|got - ref| = {err:.3e} ({err / (2e-5 * max(1.0, float(ref.abs().max()))):.3f} of the bound)")
        assert err <= 2e-5 * max(1.0, float(ref.abs().max())), err
        return
    dt = DT[store]
    x, r = x.to(dt), r.to(dt)
    blob = pack_conv_s16(w, b, store, cin_phys=16)
    weff, _ = unpack_conv_s16(blob, cin, cout, 3, store, cin_phys=16)
    ref = torch.sigmoid(F.conv2d(x.double(), weff.double(), b.double(), padding=1)) * r.double()
    xin = F.pad(_nhwc(x), (0, xpitch - cin)).to(DEV)
    rin = F.pad(_nhwc(r), (0, pitch - cout)).to(DEV)
    y = ops.conv2d(xin, w, b, cin=cin, res=rin, res_mode=L.RES_GATE, out=out.to(dt), packed=blob.to(DEV))
    got = y.float().cpu().permute(0, 3, 1, 2)
    print(f"gate {store} {cin}->{cout} {hw}: max|got - ref| = {float((got[:, :cout].double() - ref).abs().max()):.3e}")
    ok, worst = _ulp_ok(got[:, :cout], ref, dt)
    assert ok, worst
    assert torch.all(got[:, cout:c8] == 0)                    # sigmoid(0) * the residual's zero pad slots
    if pitch > c8:
        assert torch.all(got[:, c8:] == 0)                    # never written


def test_gate_rejects_an_activation_on_the_gpu():
    from ntire2022_esr_amd import _lib as L, ops
    x = torch.zeros(1, 8, 8, 16, device=DEV)
    r = torch.zeros(1, 8, 8, 56, device=DEV)
    with pytest.raises(L.EsrError, match="UNSUPPORTED"):
        ops.conv2d(x, torch.zeros(50, 16, 3, 3), torch.zeros(50), act=L.ACT_LRELU, res=r, res_mode=L.RES_GATE)


def _hfab_weights(seed, cin, cmid):
    g = torch.Generator().manual_seed(seed)
    shapes = [(cmid, cin), (cmid, cmid), (cmid, cmid), (cin, cmid)]
    ws = [torch.randn(o, i, 3, 3, generator=g) * (1.0 / (3 * i ** 0.5)) for o, i in shapes]
    bs = [torch.randn(o, generator=g) * 0.1 for o, _ in shapes]
    return ws, bs


def _hfab_per_layer(x, ws, bs, slope, cin, pitch):
    """the four launches of the unfused plan"""
    from ntire2022_esr_amd import _lib as L, ops
    t = x
    for i in range(3):
        t = ops.conv2d(t, ws[i], bs[i], act=L.ACT_LRELU, slope=slope, cin=cin if i == 0 else None)
    out = torch.zeros(*x.shape[:3], pitch, dtype=x.dtype, device=DEV)
    return ops.conv2d(t, ws[3], bs[3], res=x, res_mode=L.RES_GATE, out=out)


# FMEN's widths at both slopes (the ids they always had); HFAB_WIDTHS at the tight pitch, slope 0.05, one lone partial tile and one shape with
# six tiles and ragged edges in both directions
HFAB_CASES = [pytest.param(*c, sl, id="-".join(str(v) for v in c + (sl,))) for sl in (0.1, 0.05) for c in [
    (1, 17, 15, 50, 56, 16), (3, 5, 90, 50, 56, 16), (2, 23, 37, 50, 64, 16), (2, 40, 36, 50, 56, 12), (1, 64, 70, 48, 48, 16),
    (3, 33, 16, 64, 64, 16), (1, 1, 1, 50, 56, 16)]] + \
    [pytest.param(*nhw, c, (c + 7) // 8 * 8, m, 0.05, id="-".join(str(v) for v in nhw + (c, (c + 7) // 8 * 8, m, 0.05)))
     for c, m in HFAB_WIDTHS for nhw in [(1, 17, 15), (2, 23, 37)]]


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,w,cin,pitch,cmid,slope", HFAB_CASES)
def test_fused_hfab_equals_per_layer_launches(store, slope, n, h, w, cin, pitch, cmid):
    from ntire2022_esr_amd import _lib as L, ops
    dt = DT[store]
    ws, bs = _hfab_weights(n * 100 + h + cin, cin, cmid)
    g = torch.Generator().manual_seed(h * w + cin)
    x = F.pad(torch.randn(n, h, w, cin, generator=g) * 2, (0, pitch - cin)).to(dt).to(DEV)
    want = _hfab_per_layer(x, ws, bs, slope, cin, pitch)
    with ops.kernel_trace() as names:
        got = ops.conv_chain(x, ws, bs, slope=slope, res_mode=L.RES_GATE, cin=cin)
    torch.cuda.synchronize()
    assert len(names) == 1 and names[0].startswith(f"hfab_kernel<{'true' if store == 'bf16' else 'false'}, {(cin + 15) // 16}>"), names
    assert got.shape == want.shape and got.dtype == dt
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), int((got != want).sum())

    # NaN in the pad slots cin .. pitch - 1 and behind the tensor's last pixel: nothing beyond channel cin is read
    store_ = torch.full((n * h * w * pitch + 4096,), float("nan"), dtype=dt, device=DEV)
    xn = store_[:n * h * w * pitch].view(n, h, w, pitch)
    xn[..., :cin] = x[..., :cin]
    got_nan = ops.conv_chain(xn, ws, bs, slope=slope, res_mode=L.RES_GATE, cin=cin)
    torch.cuda.synchronize()
    assert torch.equal(got_nan.view(torch.int16), got.view(torch.int16))
    assert bool(torch.isfinite(got_nan[..., :cin].float()).all())


_models = {}


def _fmen(compute="f32"):
    from safetensors.torch import load_file
    from ntire2022_esr_amd import FMEN
    if "m" not in _models:
        m = FMEN()
        m.load_state_dict(load_file(os.path.join(GOLD, "team03_fmen.safetensors")), strict=True)
        _models["m"] = m.eval().to(DEV)
    m = _models["m"]
    m.set_compute(compute)
    m.fuse_hfab = True
    m.use_graphs = True
    return m


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_fp32_matches_reference_e2e(case):
    g = np.load(os.path.join(GOLD, "e2e_team03_fmen.npz"))
    m = _fmen("f32")
    dr = float(g["data_range"])
    x, ref = torch.from_numpy(g["x" + case]).to(DEV), g["y" + case]
    with torch.no_grad():
        y = m(x).cpu().numpy()
    assert y.shape == ref.shape
    err = float(np.abs(y.astype(np.float64) - ref).max())
    assert err <= 2e-5 * max(dr, float(np.abs(ref).max())), err


def _hr(h4, w4):
    from PIL import Image
    img = np.array(Image.open(os.path.join(GOLD, "test.bmp")).convert("RGB"))
    return np.pad(img, ((0, h4 - img.shape[0]), (0, w4 - img.shape[1]), (0, 0)), mode="symmetric")


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("h,w", [(256, 256), (339, 510)])
def test_psnr_against_reference_at_stated_size(h, w, compute):
    from ntire2022_esr_amd import image_util as util
    g = np.load(os.path.join(GOLD, f"big_team03_fmen_{h}x{w}.npz"))
    m = _fmen(compute)
    dr = float(g["data_range"])
    with torch.no_grad():
        y = m(util.uint2tensor4(g["lr"], dr).to(DEV))
    psnr = util.calculate_psnr(util.tensor2uint(y, dr), _hr(4 * h, 4 * w), border=4)
    rel = float(np.abs(y[0, :, ::9, ::9].cpu().numpy().astype(np.float64) - g["sr_sample"]).max()) / dr
    print(f"FMEN {h}x{w} {compute}: PSNR {psnr:.4f} vs reference {float(g['psnr']):.4f} dB (d = {psnr - float(g['psnr']):+.4f}), "
          f"max|dy|/range = {rel:.2e}")
    if compute == "f32":
        assert rel < 2e-5 and abs(psnr - float(g["psnr"])) <= 0.002
    else:
        assert abs(psnr - float(g["psnr"])) <= BUDGET[compute]
        assert rel <= MAX_REL[compute], rel


def test_fp16_storage_is_refused():
    """the checkpoint's HFAB intermediates reach ~2e7 on natural images: fp16 storage would overflow, the engine refuses it"""
    from ntire2022_esr_amd import _lib as L
    m = _fmen("f16")
    try:
        with pytest.raises(L.EsrError, match="fp16"):
            m(torch.rand(1, 3, 20, 20, device=DEV))
    finally:
        m.set_compute("f32")


@pytest.mark.parametrize("compute", ["bf16"])
def test_fuse_hfab_on_equals_off(compute):
    m = _fmen(compute)
    x = torch.rand(2, 3, 45, 70, generator=torch.Generator().manual_seed(3)).mul(255).to(DEV)
    with torch.no_grad():
        a = m(x)
        m.fuse_hfab = False
        b = m(x)
    m.fuse_hfab = True
    assert torch.equal(a, b), float((a - b).abs().max())


@pytest.mark.parametrize("compute", ["bf16"])
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("hw", [128, 256])
def test_16bit_batch_equals_per_image(compute, hw, fuse):
    m = _fmen(compute)
    m.fuse_hfab = fuse
    x = torch.rand(2, 3, hw, hw, generator=torch.Generator().manual_seed(hw)).mul(255).to(DEV)
    with torch.no_grad():
        yb = m(x)
        ys = [m(x[i:i + 1]) for i in range(2)]
    for i in range(2):
        assert torch.equal(yb[i:i + 1], ys[i]), (i, float((yb[i:i + 1] - ys[i]).abs().max()))


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_graph_forward_equals_run_ops(compute):
    from ntire2022_esr_amd import _lib as L
    m = _fmen(compute)
    shape = (1, 3, 40, 52)
    g = torch.Generator().manual_seed(9)
    xs = [(torch.rand(*shape, generator=g) * 255).to(DEV) for _ in range(4)]
    with torch.no_grad():
        m.use_graphs = False
        ref = [m(x).clone() for x in xs]
        torch.cuda.synchronize()
        m.use_graphs = True
        ys = [m(x) for x in xs]               # forwards 2 .. 4 are graph launches with new x / y each
    torch.cuda.synchronize()
    ent = m._plans[shape + (torch.device(DEV),)]
    assert ent.graph is not None and L.lib().esr_graph_nodes(ent.graph) >= len(ent.arr)
    for y, r in zip(ys, ref):
        assert torch.equal(y, r), float((y - r).abs().max())
