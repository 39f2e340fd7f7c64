"""-m gpu: wino_f32_kernel runs no MFMAs for a cout tile that is all padding (couts 48..63 of a 64 -> 48 layer: IMDN's upsampler), and
with that its work walk alternates the cout half a block takes from step to step.

Reference: the SAME layer with weights and bias zero-padded to 64 output channels, through the same entry point, sliced.  That launch
runs all four cout tiles; the live tiles see the same fp32 operations in the same order, so the comparison is torch.equal.  Sizes: one
ragged tile; ragged edges in a batch; more items than blocks (900 > 512); and enough items (4368 >= 8 x 512) that the first- and the
second-dispatched half of the grid walk ranges of different length (first_share = 9)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(1, 15, 16), (2, 150, 265), (5, 130, 150), (12, 200, 216)]
CIN = 64
SENTINEL = -77.0


def _layer(cout, n, h, w):
    assert torch.cuda.is_available(), "gpu-marked test needs an MI355X"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(cout * 100 + h)
    wt = torch.randn(cout, CIN, 3, 3, generator=g) * 0.05
    b = torch.randn(cout, generator=g)
    gd = torch.Generator(device=dev).manual_seed(n * 1000 + w)
    x = torch.randn(n, h, w, CIN, generator=gd, device=dev)
    w64 = torch.zeros(64, CIN, 3, 3)
    b64 = torch.zeros(64)
    w64[:cout], b64[:cout] = wt, b
    return x, wt, b, w64, b64


@pytest.mark.parametrize("nhw", SIZES)
def test_pixelshuffle_48_equals_zero_padded_64(nhw):
    """model.2's form: 64 -> 48 + PixelShuffle(4); the padded layer has a fourth colour plane that is sliced away"""
    from ntire2022_esr_amd import ops
    x, wt, b, w64, b64 = _layer(48, *nhw)
    ref = ops.conv2d(x, w64, b64, shuffle_out=True, wino=True)
    with ops.kernel_trace() as names:
        y = ops.conv2d(x, wt, b, shuffle_out=True, wino=True)
    assert names == ["wino_f32_kernel<0, 0, 2>"], names
    assert y.shape == (nhw[0], 3, 4 * nhw[1], 4 * nhw[2])
    assert torch.equal(y, ref[:, :3])
    assert not bool((ref[:, :3] == 0).all())


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("cout", [48, 36, 16])
@pytest.mark.parametrize("nhw", SIZES)
def test_nhwc_equals_zero_padded_64(nhw, cout, act):
    """NHWC store into a channel slice of a wider tensor: a dead tile next to a full one (48), next to a partial one (36), and a layer of
    one half whose second tile is dead (16).  Channels at or beyond cout and the neighbouring channels stay what they were"""
    from ntire2022_esr_amd import ops
    n, h, w = nhw
    x, wt, b, w64, b64 = _layer(cout, n, h, w)
    ref = ops.conv2d(x, w64, b64, act=act, wino=True)
    big = torch.full((n, h, w, 72), SENTINEL, device=x.device)
    with ops.kernel_trace() as names:
        ops.conv2d(x, wt, b, act=act, out=big, out_coff=4, wino=True)
    assert names == [f"wino_f32_kernel<{act}, 0, 0>"], names
    assert torch.equal(big[..., 4:4 + cout], ref[..., :cout])
    assert bool((big[..., :4] == SENTINEL).all()) and bool((big[..., 4 + cout:] == SENTINEL).all())
    assert not bool((ref[..., :cout] == 0).all())
