"""-m gpu: wino8_f32_kernel<., 1, 8> -- IMDBlock conv1 (64 -> 64, LeakyReLU 0.05, 16 / 48 split store with a channel-blocked second output)
on the resident-U plan with a halo ring of ONE slot per wave.  Per output the MFMAs run in wino_f32_kernel's order (chunks ascending, the
two k-steps, the bias at position 5 of the first stage), so the research switch esr_dbg_wino8_nch8(0) -- conv1's form back on
wino_f32_kernel<1, 0, 1> -- must give the same bits; the fp64 convolution is held at the bar of tests/test_gpu_wino.py (2e-5 x scale).
esr_dbg_wino8(2) puts the kernel on images far below its strip count."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (n, h, w), strips of 4 x 16 pixels.  The forced launch still has 256 blocks = 128 block pairs, a pair owns a run of ceil(strips / 128)
# strips, waves 0..3 take 10/16 of it (rounded up to whole steps of four) and waves 4..7 the rest.
# The first four are the issue's shapes -- 10 x 4 = 40; 2 x 4 x 2 = 16 with both edges no multiple of 4 / 16 (13 = 3 x 4 + 1, 21 = 16 + 5);
# 3 x 5 x 3 = 45; 1 x 2 x 3 = 6, fewer than the eight waves of a block -- and give runs of ONE strip: edges, strips of other images, idle
# waves and blocks, but a wave never walks a second strip.  What a second strip brings (the vmcnt(8) wait behind an epilogue, the DMA cursor
# moving on to a real next strip in stage 6, the next strip's chunks 0 / 1 staged in stages 6 / 7, both wave classes at work) needs longer runs:
# 5 x 16 x 3 = 240 (runs of 2: two waves, one strip each); 7 x 25 x 13 = 2275 (runs of 18: 12 + 6, waves walk up to 3 strips, and 325 strips
# per image are no multiple of 18: runs straddle image boundaries, so a wave's next strip lies in the next image; ragged right and bottom
# edges); 4 x 64 x 16 = 4096 (runs of 32: 20 + 12, five and three strips per wave)
SIZES = [(1, 40, 56), (2, 13, 21), (3, 20, 36), (1, 8, 48), (5, 64, 48), (7, 100, 200), (4, 256, 256)]
OLD, NEW = "wino_f32_kernel<1, 0, 1>", "wino8_f32_kernel<1, 1, 8>"


def _switch(mode, nch8):
    from ntire2022_esr_amd import _lib as L
    L.lib().esr_dbg_wino8(ctypes.c_int(mode))
    L.lib().esr_dbg_wino8_nch8(ctypes.c_int(nch8))


def _layer(n, h, w):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(100 * n + 10 * h + w)
    x = torch.randn(n, 64, h, w, generator=g)
    wt = torch.randn(64, 64, 3, 3, generator=g) * 0.1
    b = torch.randn(64, generator=g)
    ref = F.leaky_relu(F.conv2d(x.double().to(dev), wt.double().to(dev), b.double().to(dev), padding=1), 0.05)
    return x, wt, b, ref.permute(0, 2, 3, 1).contiguous()


_LAYERS = {}


def _shared(nhw):
    if nhw not in _LAYERS:
        _LAYERS[nhw] = _layer(*nhw)
    return _LAYERS[nhw]


def _launch(x, wt, b, blocked_in):
    """conv1 as IMDBlock launches it: 16 distilled channels into the concat buffer, 48 into the channel-blocked r1; both returned as NHWC"""
    from ntire2022_esr_amd import ops
    dev = torch.device("cuda:0")
    n, _, h, w = x.shape
    xd = (x.view(n, 8, 8, h, w).permute(0, 1, 3, 4, 2) if blocked_in else x.permute(0, 2, 3, 1)).contiguous().to(dev)
    cat = torch.full((n, h, w, 64), 7.0, device=dev)
    rem = torch.full((n, 6, h, w, 8), 9.0, device=dev)
    with ops.kernel_trace() as names:
        ops.conv2d(xd, wt, b, act=1, split=16, out=cat, out1=rem, blocked_out1=True, blocked_in=blocked_in, wino=True)
    assert bool((cat[..., 16:] == 7.0).all())
    return torch.cat([cat[..., :16], rem.permute(0, 2, 3, 1, 4).reshape(n, h, w, 48)], dim=-1), names


@pytest.mark.parametrize("blocked_in", [False, True])
@pytest.mark.parametrize("nhw", SIZES)
def test_one_slot_ring_equals_wino_f32_kernel(nhw, blocked_in):
    assert torch.cuda.is_available(), "gpu-marked test needs an MI355X"
    x, wt, b, _ = _shared(nhw)
    try:
        _switch(2, 0)
        y_old, names_old = _launch(x, wt, b, blocked_in)
        _switch(2, 1)
        y_new, names_new = _launch(x, wt, b, blocked_in)
    finally:
        _switch(1, 1)
    assert names_old == [OLD] and names_new == [NEW], (names_old, names_new)
    assert torch.equal(y_new, y_old)


@pytest.mark.parametrize("blocked_in", [False, True])
@pytest.mark.parametrize("nhw", SIZES)
def test_one_slot_ring_against_fp64(nhw, blocked_in):
    assert torch.cuda.is_available(), "gpu-marked test needs an MI355X"
    x, wt, b, ref = _shared(nhw)
    try:
        _switch(2, 1)
        y, names = _launch(x, wt, b, blocked_in)
    finally:
        _switch(1, 1)
    assert names == [NEW], names
    err = float((y.double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    assert err < 2e-5, err


def test_whole_imdn_with_and_without():
    """IMDN x4 at 2 x 40 x 56: the eight conv1 launches on either kernel, every other launch the same -- equal outputs"""
    assert torch.cuda.is_available(), "gpu-marked test needs an MI355X"
    from ntire2022_esr_amd.registry import select_model
    dev = torch.device("cuda:0")
    m, _, dr, _ = select_model(-1, dev)
    x = torch.rand(2, 3, 40, 56, generator=torch.Generator().manual_seed(5)).to(dev) * dr
    outs, kernels = [], []
    try:
        for nch8 in (0, 1):
            _switch(2, nch8)
            m.enable_profiling(1)
            outs.append(m(x).clone())
            torch.cuda.synchronize()
            kernels.append([o["kernel"] for o in m.collect_profile()])
            m.disable_profiling()
    finally:
        _switch(1, 1)
    assert kernels[0].count(OLD) == 8 and kernels[0].count(NEW) == 0, sorted(set(kernels[0]))
    assert kernels[1].count(NEW) == 8 and kernels[1].count(OLD) == 0, sorted(set(kernels[1]))
    assert torch.equal(outs[0], outs[1])
