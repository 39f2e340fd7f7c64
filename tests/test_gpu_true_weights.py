"""-m gpu: FMEN, EFDN, FasterRFDN, ESAN, DWRFDN, BMDN and RFDNeXt with their UNROUNDED fp32 checkpoints against the reference with the same
(tools/gen_golden_true_weights.py; tests/_true_weights.py holds how each network's own test file builds and bounds it).

The networks' own files load a checkpoint rounded to bf16, so their budgets and their fp32 parity were measured with no weight rounding and
with folds and merges (fold_center, FMEN's and EFDN's merges, the border tables) that are exact for such weights only.  Here:

  (a) the fp32 plan against the reference: the e2e inputs xb and xc under the network's own bar, and at 256 x 256 rel < 2e-5 on the ::9
      sample and |dPSNR| <= 0.002 dB;
  (b) every 16-bit plan the network accepts, in every form, on a batch of two copies of the 256 x 256 image (512 tiles of 16 x 16, 256 of
      16 x 32: the persistent kernels run): the two outputs bit-identical, |PSNR - psnr_true| within the network's budget for the type, and
      rel <= MAX_REL[compute] + dw_rel_<compute>: the network's own bound on the activation rounding (measured with exact weights) plus
      the reference's own figure for rounding EVERY weight once to the type -- an upper scale for the engine, which keeps hi + lo pairs
      for most 1x1s and rounds the 3x3s and the fused kernels' 1x1s once;
  (c) teeth: BMDN's fp32 plan with the ROUNDED fixture misses (a)'s bars against the true goldens."""
import numpy as np
import pytest
import torch

import _true_weights as TW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEMS = list(TW.NETS)
_models, _goldens = {}, {}


def _golden(stem):
    if stem not in _goldens:
        _goldens[stem] = TW.golden(stem)
    return _goldens[stem]


def _model(net, compute, flag, sd=None, key=None):
    import ntire2022_esr_amd as E
    key = key or net.stem
    if key not in _models:
        m = getattr(E, net.cls)(**net.kwargs)
        m.load_state_dict(TW.load_true(net.stem) if sd is None else sd, strict=True)
        _models[key] = m.eval().to(DEV)
    m = _models[key]
    m.set_compute(compute)
    setattr(m, net.flag, flag)
    m.use_graphs = True
    return m


def _f32(net, **kw):
    return _model(net, "f32", TW.F32_FLAG.get(net.stem, False), **kw)


def _n_fused(m, kind, shape):
    return sum(o.kind == kind for o in m._plans[tuple(shape) + (torch.device(DEV),)].plan.ops)


def _hr():
    import os
    from PIL import Image
    img = np.array(Image.open(os.path.join(TW.GOLD, "test.bmp")).convert("RGB"))
    return np.pad(img, ((0, 1024 - img.shape[0]), (0, 1024 - img.shape[1]), (0, 0)), mode="symmetric")      # gen_golden_r2.hr_from_bmp


def _e2e(net, m, g, case):
    """max |y - ref| and the network's own e2e bar for it"""
    dr = float(g["data_range"])
    ref = g["y" + case]
    with torch.no_grad():
        y = m(torch.from_numpy(g["x" + case]).to(DEV)).cpu().numpy()
    assert y.shape == ref.shape
    err = float(np.abs(y.astype(np.float64) - ref).max())
    return err, 2e-5 * (max(dr, float(np.abs(ref).max())) if net.e2e_over_output else dr), float(np.abs(ref).max())


def _big(net, m, g, batch):
    """(outputs, PSNR of image 0 minus the reference's, max |dy| / range on image 0's ::9 sample)"""
    from ntire2022_esr_amd import image_util as util
    dr = float(g["data_range"])
    x = util.uint2tensor4(g["lr"], dr).to(DEV)
    assert x.shape == (1, 3, 256, 256)
    with torch.no_grad():
        y = m(x.repeat(batch, 1, 1, 1).contiguous())
    assert y.shape == (batch, 3, 1024, 1024) and bool(torch.isfinite(y).all())
    hr = _hr()
    assert hr.shape == (1024, 1024, 3)
    psnr = util.calculate_psnr(util.tensor2uint(y[0:1], dr), hr, border=4)
    rel = float(np.abs(y[0, :, ::9, ::9].cpu().numpy().astype(np.float64) - g["sr_sample"]).max()) / TW.rel_range(net, g)
    return y, psnr - float(g["psnr"]), rel


@pytest.mark.parametrize("case", ["b", "c"])
@pytest.mark.parametrize("stem", STEMS)
def test_fp32_matches_reference_e2e_true_weights(stem, case):
    net, g = TW.NETS[stem], _golden(stem)
    err, bar, top = _e2e(net, _f32(net), g, case)
    print(f"{stem} true weights e2e {case}: max|y - ref| = {err:.3e} (bar {bar:.3e}), max|ref| = {top:.3f}")
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("stem", STEMS)
def test_fp32_matches_reference_at_256_true_weights(stem):
    net, g = TW.NETS[stem], _golden(stem)
    y, dpsnr, rel = _big(net, _f32(net), g, 1)
    mean = float(y.double().mean().item())
    print(f"{stem} true weights 256x256 f32: dPSNR = {dpsnr:+.4f} dB, max|dy|/range = {rel:.2e}, mean {mean:.6f} vs {float(g['sr_mean']):.6f}")
    assert rel < 2e-5, rel
    assert abs(dpsnr) <= 0.002, dpsnr
    assert abs(mean - float(g["sr_mean"])) <= 2e-5 * TW.rel_range(net, g)


# FMEN in bf16 is OVER its budget with the real checkpoint, in both forms (they are bit-identical): measured on the MI355X -0.0104 dB at
# 256 x 256 against the budget of 0.01 (with the bf16-representable fixture: -0.0033 dB).  FMEN is 3x3s only and a 16-bit plan rounds every 3x3
# weight once; no plan switch changes that (hilo_skip off: -0.0115 dB; fuse_chain, fuse_esa_lowres, fuse_tail, tight_pitch: no effect).  The
# reference itself, with only the 3x3 weights behind the head rounded to bf16 and the biases kept, loses 0.0087 dB (the HFABs' weights
# 0.0052, the BasicBlocks' 0.0021).  DESIGN.md 7b and 7i; the budget is not raised
FMEN_BF16_OVER = pytest.mark.xfail(strict=True, reason="FMEN bf16 with the unrounded checkpoint: measured -0.0104 dB at 256 x 256, budget 0.01 dB "
                                   "(every 3x3 weight is rounded once; no plan-level remedy: DESIGN.md 7i)")
_FORMS16 = [(n, c, f) for n in TW.NETS.values() for c, f in n.forms]
CASES16 = [pytest.param(n.stem, c, f, id=f"{n.stem}-{c}-{n.flag}{int(f)}") for n, c, f in _FORMS16]
PSNR_CASES16 = [pytest.param(n.stem, c, f, id=f"{n.stem}-{c}-{n.flag}{int(f)}", marks=[FMEN_BF16_OVER] if n.stem == "team03_fmen" else [])
                for n, c, f in _FORMS16]
_runs16 = {}


def _run16(stem, compute, flag):
    """one forward per case on a batch of two copies of the image, shared by the two tests below: only its figures are kept"""
    key = (stem, compute, flag)
    if key not in _runs16:
        net, g = TW.NETS[stem], _golden(stem)
        m = _model(net, compute, flag)
        y, dpsnr, rel = _big(net, m, g, 2)
        n_fused = _n_fused(m, net.fused[0], (2, 3, 256, 256)) if net.fused else None
        print(f"{stem} true weights 2x256x256 {compute} {net.flag}={int(flag)}: dPSNR = {dpsnr:+.4f} dB (budget {TW.budget(net, compute)}), "
              f"max|dy|/range = {rel:.2e} (bound {TW.max_rel(net, compute):.2e} + {float(g['dw_rel_' + compute]):.2e})")
        _runs16[key] = dict(dpsnr=dpsnr, rel=rel, n_fused=n_fused, same=torch.equal(y[0], y[1]), diff=float((y[0] - y[1]).abs().max()))
    return _runs16[key]


@pytest.mark.parametrize("stem,compute,flag", CASES16)
def test_16bit_plans_with_true_weights_stay_within_the_rounding_bound(stem, compute, flag):
    net, g = TW.NETS[stem], _golden(stem)
    r = _run16(stem, compute, flag)
    if net.fused:
        assert r["n_fused"] == (net.fused[1] if flag else 0)
    assert r["same"], r["diff"]                                  # the two copies of the image: bit-identical outputs
    bound = TW.max_rel(net, compute) + float(g["dw_rel_" + compute])
    assert r["rel"] <= bound, (r["rel"], bound)


@pytest.mark.parametrize("stem,compute,flag", PSNR_CASES16)
def test_16bit_plans_meet_their_psnr_budget_with_true_weights(stem, compute, flag):
    r = _run16(stem, compute, flag)
    assert abs(r["dpsnr"]) <= TW.budget(TW.NETS[stem], compute), r["dpsnr"]


def test_rounded_fixture_misses_the_true_weight_bars():
    """teeth: the same fp32 plan with tests/golden/team37_bmdn.safetensors (every weight rounded to bf16) is nowhere near the true goldens"""
    net = TW.NETS["team37_bmdn"]
    g = _golden(net.stem)
    sd = TW.load_rounded(net.stem)
    assert all(v.dtype == torch.bfloat16 for v in sd.values())
    m = _f32(net, sd=sd, key="team37_bmdn-rounded")
    err, bar, _ = _e2e(net, m, g, "b")
    _, dpsnr, rel = _big(net, m, g, 1)
    print(f"team37_bmdn ROUNDED weights against the true goldens: e2e b {err:.3e} (bar {bar:.3e}), 256x256 rel {rel:.2e}, dPSNR {dpsnr:+.4f}")
    assert err > bar, (err, bar)
    assert rel > 2e-5, rel
    # ... and by what the reference itself says the rounding does, to the fp32 plan's accuracy
    assert abs(rel - float(g["dw_rel_bf16"])) <= 2 * 2e-5, (rel, float(g["dw_rel_bf16"]))
