"""-m gpu: IMDN fp32 on ragged tiles (2 x 45 x 70: no edge is a multiple of a tile or a strip): the images of a batch equal the same
images run alone, bit for bit.  The work walks of the Winograd kernels depend on the batch size (which block takes which tile and cout
half, which wave which strip); the arithmetic of an output must not."""
import pytest
import torch

from conftest import load_sd_torch

pytestmark = pytest.mark.gpu


def test_ragged_batch_equals_per_image():
    from ntire2022_esr_amd import IMDN
    assert torch.cuda.is_available(), "gpu-marked test needs an MI355X"
    m = IMDN(in_nc=3, out_nc=3, nc=64, nb=8, upscale=4)
    m.load_state_dict(load_sd_torch("imdn_baseline"), strict=True)
    m = m.eval().to("cuda:0")
    x = torch.rand(2, 3, 45, 70, generator=torch.Generator().manual_seed(45)).to("cuda:0")
    with torch.no_grad():
        y = m(x)
        assert y.shape == (2, 3, 180, 280) and bool(torch.isfinite(y).all())
        for i in range(2):
            assert torch.equal(y[i:i + 1], m(x[i:i + 1].contiguous())), i
