"""The unrounded fp32 checkpoints of the seven newer networks (tools/gen_golden_true_weights.py; no GPU).

tests/golden/<stem>.safetensors is the reference checkpoint rounded to bf16: no test that loads it sees a weight the 16-bit storage types
cannot hold.  tests/golden/<stem>_f32*.safetensors is the same checkpoint unrounded.  Here: it loads into the HIP model class, it IS the same
checkpoint (rounding it gives the old fixture bit for bit), practically none of its values is a bf16 number, and the reference's outputs
with the two differ by far more than the fp32 parity bar -- so tests/test_gpu_true_weights.py cannot pass on the rounded file."""
import os

import numpy as np
import pytest
import torch

import _true_weights as TW

STEMS = list(TW.NETS)


@pytest.fixture(scope="module", params=STEMS)
def ck(request):
    net = TW.NETS[request.param]
    return net, TW.load_true(net.stem), TW.load_rounded(net.stem)


def test_loads_strictly_into_the_hip_model(ck):
    import ntire2022_esr_amd as E
    net, true, _ = ck
    m = getattr(E, net.cls)(**net.kwargs)
    m.load_state_dict(true, strict=True)
    sd = m.state_dict()
    assert all(torch.equal(sd[k].view(torch.int32), v.view(torch.int32)) for k, v in true.items())      # (fp32 in, the same fp32 held)


def test_same_keys_and_shapes_as_the_rounded_fixture(ck):
    _, true, rounded = ck
    assert set(true) == set(rounded)
    for k, v in true.items():
        assert v.dtype == torch.float32 and rounded[k].dtype == torch.bfloat16 and v.shape == rounded[k].shape, k
        assert bool(torch.isfinite(v).all()), k


def test_rounded_to_bf16_it_is_the_old_fixture_bit_for_bit(ck):
    _, true, rounded = ck
    for k, v in true.items():
        assert torch.equal(v.to(torch.bfloat16).view(torch.int16), rounded[k].view(torch.int16)), k


def test_practically_no_value_is_a_bf16_number(ck):
    net, true, _ = ck
    v = torch.cat([t.flatten() for t in true.values()])
    outside16 = {dt: int((v.to(dt).float() != v).sum()) for dt in (torch.bfloat16, torch.float16)}
    print(f"{net.stem}: {v.numel()} values, {outside16[torch.bfloat16]} outside bf16, {outside16[torch.float16]} outside fp16")
    assert outside16[torch.bfloat16] > 0.99 * v.numel()
    assert outside16[torch.float16] > 0.99 * v.numel()


def test_the_files_fit_the_repository(ck):
    net = ck[0]
    paths = TW.true_paths(net.stem) + [os.path.join(TW.GOLD, f"true_{net.stem}.npz")]
    assert 2 <= len(paths) <= 3
    for p in paths:
        assert os.path.getsize(p) <= TW.FILE_LIMIT, (p, os.path.getsize(p))


def test_goldens_differ_from_the_rounded_fixtures_by_far_more_than_the_fp32_bar(ck):
    """dw_rel_bf16 is the reference's own max |dy| / range at 256 x 256 between the two checkpoints: over 100 x the 2e-5 bar"""
    net = ck[0]
    g = TW.golden(net.stem)
    big = np.load(os.path.join(TW.GOLD, f"big_{net.stem}_256x256.npz"))
    assert float(g["data_range"]) == float(big["data_range"])
    assert g["sr_sample"].shape == big["sr_sample"].shape == (3, 114, 114)
    assert g["yb"].shape[2:] == tuple(4 * s for s in g["xb"].shape[2:]) and g["yc"].shape[2:] == tuple(4 * s for s in g["xc"].shape[2:])
    for k in ("dw_rel_bf16", "dw_rel_f16", "dw_psnr_bf16", "dw_psnr_f16", "psnr", "sr_mean"):
        assert np.isfinite(g[k]), k
    assert float(g["dw_rel_bf16"]) > 100 * 2e-5, float(g["dw_rel_bf16"])
    # the stored figure is what the two sets of goldens show: the old sample IS the reference's with every weight rounded to bf16
    d = float(np.abs(big["sr_sample"].astype(np.float64) - g["sr_sample"]).max()) / TW.rel_range(net, g)
    assert d == pytest.approx(float(g["dw_rel_bf16"]), rel=1e-6), (d, float(g["dw_rel_bf16"]))
    assert float(big["psnr"]) - float(g["psnr"]) == pytest.approx(float(g["dw_psnr_bf16"]), abs=1e-9)


def test_bounds_come_from_the_networks_own_test_files(ck):
    """BUDGET and MAX_REL are imported from each network's GPU test file; only the two files without a 16-bit MAX_REL use the table here"""
    net = ck[0]
    mod = TW.module(net)
    for compute, _ in net.forms:
        assert TW.budget(net, compute) == {"bf16": 0.01, "f16": 0.005}[compute]
        own = getattr(mod, "MAX_REL", {})
        assert (compute in own) != (net.stem in TW.MAX_REL_16), (net.stem, compute)
        assert 0 < TW.max_rel(net, compute) < 0.05
    forms = getattr(mod, "FORMS", None)
    if forms is not None:
        assert [f for f in forms if f[0] != "f32"] == net.forms
