"""-m gpu: wino8_f32_kernel's uneven split of a block's strips between the older and the younger wave of a SIMD (WinoK.first_share: waves
0..3 take s/16 of the block's run, waves 4..7 the rest).  Only the map from waves to strips changes, so every split must give the bits of
wino_f32_kernel (research switch off), as the even split does.  The research switches put the kernel on images far below its strip count
(esr_dbg_wino8(2)) and choose the split (esr_dbg_wino8_share): one strip, fewer strips than the eight waves of a block, runs that end in
the middle of a group of four, and whole runs."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# (n, h, w): strips of 4 x 16 pixels -- 1; 6 (fewer than 8 waves); 2 x 12 x 5 = 120 and 5 x 16 x 3 = 240 over 128 block pairs (runs of 1
# and 2: a run ends inside a group); 7 x 25 x 13 = 2275 (runs of 18: 12 + 6 at s = 9 and s = 10, both end inside a group, the last
# block's run is shorter); 4 x 64 x 16 = 4096 (runs of 32: 20 + 12, several steps per wave)
SIZES = [(1, 4, 16), (1, 8, 48), (2, 45, 70), (5, 64, 48), (7, 100, 200), (4, 256, 256)]
SHARES = [0, 9, 10, 15]          # 0: the launcher's constant


def _switch(mode, share=0):
    from ntire2022_esr_amd import _lib as L
    L.lib().esr_dbg_wino8(ctypes.c_int(mode))
    L.lib().esr_dbg_wino8_share(ctypes.c_int(share))


def _launch(x, wt, b, blocked):
    from ntire2022_esr_amd import ops
    n, h, w, _ = x.shape
    cat = torch.full((n, h, w, 64), 7.0, device=x.device)
    rem = torch.full((n, 6, h, w, 8) if blocked else (n, h, w, 48), 9.0, device=x.device)
    with ops.kernel_trace() as names:
        ops.conv2d(x, wt, b, act=1, in_coff=16, cin=48, split=16, out=cat, out_coff=32, out1=rem, blocked_out1=blocked, wino=True)
    return cat, rem, names


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("nhw", SIZES)
def test_every_split_equals_wino_f32_kernel(nhw, blocked):
    """IMDBlock conv2 / conv3: 48 of 64 input channels, 16 / 48 split store with an NHWC and a channel-blocked second output"""
    assert torch.cuda.is_available(), "gpu-marked test needs an MI355X"
    dev = torch.device("cuda:0")
    n, h, w = nhw
    g = torch.Generator().manual_seed(h * 10 + w)
    wt = torch.randn(64, 48, 3, 3, generator=g) * 0.1
    b = torch.randn(64, generator=g)
    x = torch.randn(n, h, w, 64, generator=torch.Generator(device=dev).manual_seed(n + h), device=dev)
    try:
        _switch(0)
        cat4, rem4, names4 = _launch(x, wt, b, blocked)
        assert names4 == [f"wino_f32_kernel<1, 0, {int(blocked)}>"], names4
        assert bool((cat4[..., :32] == 7.0).all()) and bool((cat4[..., 48:] == 7.0).all()) and not bool((rem4 == 9.0).any())
        for s in SHARES:
            _switch(2, s)
            cat8, rem8, names8 = _launch(x, wt, b, blocked)
            assert names8 == [f"wino8_f32_kernel<1, {int(blocked)}, 6>"], (s, names8)
            assert torch.equal(cat8, cat4) and torch.equal(rem8, rem4), s
    finally:
        _switch(1)
