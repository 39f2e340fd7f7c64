"""-m gpu: the Winograd F(2x2,3x3) fp32 convolution (wino_f32_kernel, through the C ABI: esr_conv_desc.wino_wpacked) against the
ATen fp32 op it replaces (models/basicblock.py:61-98 `conv`), evaluated on the CPU.  Tolerance 2e-5 * scale, the
same bar as the direct kernel's tests in test_gpu_conv.py."""
import pytest
import torch
import torch.nn.functional as F

import _persist_cases as P

pytestmark = pytest.mark.gpu

ACTS = {0: lambda v: v, 1: lambda v: F.leaky_relu(v, 0.05), 2: F.relu, 3: F.gelu}


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs an MI355X"
    return torch.device("cuda:0")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _check(y_gpu_nhwc, ref_nchw, tol=2e-5):
    y = y_gpu_nhwc.cpu().permute(0, 3, 1, 2)[:, :ref_nchw.shape[1]]
    s = max(1.0, float(ref_nchw.abs().max()))
    err = float((y - ref_nchw).abs().max()) / s
    assert err < tol, err


@pytest.mark.parametrize("cin,cout", [(64, 64), (48, 64), (32, 32), (64, 48), (48, 16), (64, 50)])
@pytest.mark.parametrize("hw", [(16, 16), (17, 15), (40, 56), (5, 3), (1, 1), (33, 64), (31, 49)])
def test_wino_plain(cin, cout, hw):
    from ntire2022_esr_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + hw[0])
    x = torch.randn(2, cin, *hw, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
    b = torch.randn(cout, generator=g)
    ref = F.conv2d(x, w, b, padding=1)
    y = ops.conv2d(_nhwc(x).to(dev), w, b, wino=True)
    _check(y, ref)


def test_wino_equals_direct_kernel_closely():
    """same input through both kernels: they differ by rounding only (different summation, ~1e-6)"""
    from ntire2022_esr_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    x = _nhwc(torch.randn(3, 64, 50, 70, generator=g)).to(dev)
    w = torch.randn(64, 64, 3, 3, generator=g) * 0.05
    b = torch.randn(64, generator=g)
    yd = ops.conv2d(x, w, b, act=1)
    yw = ops.conv2d(x, w, b, act=1, wino=True)
    assert float((yd - yw).abs().max()) < 2e-5 * max(1.0, float(yd.abs().max()))
    assert not torch.equal(yd, yw)          # it IS the other kernel


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("res_mode", [0, 1, 2])
def test_wino_epilogues(act, res_mode):
    from ntire2022_esr_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(7 + act * 3 + res_mode)
    x = torch.randn(1, 48, 23, 37, generator=g)
    r = torch.randn(1, 64, 23, 37, generator=g)
    w = torch.randn(64, 48, 3, 3, generator=g) * 0.1
    b = torch.randn(64, generator=g)
    c = F.conv2d(x, w, b, padding=1)
    ref = {0: ACTS[act](c), 1: ACTS[act](c + r), 2: ACTS[act](c) + r}[res_mode]
    y = ops.conv2d(_nhwc(x).to(dev), w, b, act=act, slope=0.05,
                   res=_nhwc(r).to(dev) if res_mode else None, res_mode=res_mode, wino=True)
    _check(y, ref)


def test_wino_channel_slices_and_split_store():
    """IMDBlock conv2 (basicblock.py:261): reads 48 channels of a wider buffer, 16 / 48 split store into a concat slice"""
    from ntire2022_esr_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    big = torch.randn(2, 64, 19, 21, generator=g)
    w = torch.randn(64, 48, 3, 3, generator=g) * 0.1
    b = torch.randn(64, generator=g)
    ref = F.leaky_relu(F.conv2d(big[:, 16:], w, b, padding=1), 0.05)
    cat = torch.full((2, 19, 21, 64), 7.0, device=dev)
    rem = torch.full((2, 19, 21, 48), 9.0, device=dev)
    ops.conv2d(_nhwc(big).to(dev), w, b, act=1, in_coff=16, cin=48, split=16,
               out=cat, out_coff=32, out1=rem, out1_coff=0, wino=True)
    cat_c, rem_c = cat.cpu(), rem.cpu()
    assert torch.all(cat_c[..., :32] == 7.0) and torch.all(cat_c[..., 48:] == 7.0)
    _check(cat_c[..., 32:48], ref[:, :16])
    _check(rem_c, ref[:, 16:])


def test_wino_blocked_split_store():
    """IMDBlock conv3: the 48 remaining channels go to a channel-blocked [N, 6, H, W, 8] tensor (esr_conv_desc.blocked8)"""
    from ntire2022_esr_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 48, 37, 29, generator=g)
    w = torch.randn(64, 48, 3, 3, generator=g) * 0.1
    b = torch.randn(64, generator=g)
    ref = F.leaky_relu(F.conv2d(x, w, b, padding=1), 0.05)
    cat = torch.zeros((2, 37, 29, 48), device=dev)
    rem = torch.full((2, 6, 37, 29, 8), 9.0, device=dev)
    ops.conv2d(_nhwc(x).to(dev), w, b, act=1, split=16, out=cat, out_coff=16, out1=rem, blocked_out1=True, wino=True)
    _check(cat.cpu()[..., 16:32], ref[:, :16])
    r = rem.cpu().permute(0, 1, 4, 2, 3).reshape(2, 48, 37, 29)          # [n][c/8][8][h][w]
    s = max(1.0, float(ref.abs().max()))
    assert float((r - ref[:, 16:]).abs().max()) / s < 2e-5


def test_wino_more_items_than_blocks_and_batch():
    """> 512 work items: persistent blocks walk several tiles, the staging ring crosses item boundaries"""
    from ntire2022_esr_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(13)
    x = torch.randn(5, 64, 130, 150, generator=g)
    w = torch.randn(64, 64, 3, 3, generator=g) * 0.05
    b = torch.randn(64, generator=g)
    ref = F.conv2d(x, w, b, padding=1)
    y = ops.conv2d(_nhwc(x).to(dev), w, b, wino=True)
    _check(y, ref)


def test_wino_unsupported_shapes_fall_back():
    """odd chunk counts / 1x1 / tiny cin: esr_wino_supported says no and ops.conv2d(wino=True) refuses; the engine keeps conv_f32_kernel"""
    from ntire2022_esr_amd import _lib as L, ops
    dev = _dev()
    x = torch.randn(1, 9, 9, 56, device=dev)
    w = torch.randn(50, 50, 3, 3) * 0.1
    with pytest.raises(L.EsrError):
        ops.conv2d(x, w, None, cin=50, wino=True)            # 7 chunks
    x = torch.randn(1, 9, 9, 16, device=dev)
    with pytest.raises(L.EsrError):
        ops.conv2d(x, torch.randn(16, 16, 3, 3), None, wino=True)      # 2 chunks


def test_wino_uneven_split_between_block_classes():
    """>= 8 items per block: the first-dispatched half of the grid takes 9/16 of the items (two walks over two ranges); every
    output pixel is still written exactly once"""
    from ntire2022_esr_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(21)
    x = torch.randn(12, 64, 200, 216, generator=g)
    w = torch.randn(64, 64, 3, 3, generator=g) * 0.05
    b = torch.randn(64, generator=g)
    ref = F.leaky_relu(F.conv2d(x, w, b, padding=1), 0.05)
    y = ops.conv2d(_nhwc(x).to(dev), w, b, act=1, wino=True)
    _check(y, ref)


@pytest.mark.parametrize("hw", [(21, 30), (32, 32), (17, 15)])
def test_wino_pixelshuffle_output(hw):
    """the network's last convolution: conv + nn.PixelShuffle(4) fused into the store (basicblock.py:446-449, 84-85)"""
    from ntire2022_esr_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(5 + hw[0])
    t = torch.randn(2, 64, *hw, generator=g)
    w2 = torch.randn(48, 64, 3, 3, generator=g) * 0.05
    b2 = torch.randn(48, generator=g)
    ref = F.pixel_shuffle(F.conv2d(t, w2, b2, padding=1), 4)
    out = ops.conv2d(_nhwc(t).to(dev), w2, b2, shuffle_out=True, wino=True).cpu()
    assert out.shape == ref.shape
    assert float((out - ref).abs().max()) / max(1.0, float(ref.abs().max())) < 2e-5


# ---- wino8_f32_kernel (round 4): resident U, wave-private halo rings, no barrier -- taken for 4 / 6 input chunks, no residual, when every
# one of the 2048 waves gets at least four 4 x 16-pixel strips
def _w8_on(on):
    import ctypes
    from ntire2022_esr_amd import _lib as L
    L.lib().esr_dbg_wino8(ctypes.c_int(1 if on else 0))


@pytest.mark.parametrize("cin,cout,n,h,w,act", [(48, 64, 4, 256, 256, 1), (48, 64, 5, 250, 251, 0), (32, 32, 9, 255, 258, 3),
                                                 (48, 48, 6, 253, 244, 1), (32, 64, 3, 300, 301, 2), (46, 64, 7, 203, 190, 1)])
def test_wino8_plain(cin, cout, n, h, w, act):
    """strip-autonomous kernel vs ATen fp32 on ragged sizes (partial strips on the right / bottom edge, several strips per wave, strips
    that straddle image boundaries of the batch), and vs wino_f32_kernel: the same fp32 operations per output -> bit-identical"""
    _dev()
    case = P.wino8(cin, cout, n, h, w, act)
    y8, y4, ref = case.outs[0], case.extra["general"][0], case.extra["ref32"]
    _check(y8, ref)
    assert torch.equal(y8, y4)


def test_wino8_split_and_blocked_stores():
    """IMDBlock conv2 / conv3 at batch size: 16 / 48 split into a concat slice + the remaining channels dense or channel-blocked"""
    from ntire2022_esr_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(21)
    n, h, w = 4, 256, 250
    big = torch.randn(n, 64, h, w, generator=g)
    wt = torch.randn(64, 48, 3, 3, generator=g) * 0.1
    b = torch.randn(64, generator=g)
    ref = F.leaky_relu(F.conv2d(big[:, 16:], wt, b, padding=1), 0.05)
    cat = torch.full((n, h, w, 64), 7.0, device=dev)
    rem = torch.full((n, h, w, 48), 9.0, device=dev)
    ops.conv2d(_nhwc(big).to(dev), wt, b, act=1, in_coff=16, cin=48, split=16, out=cat, out_coff=32, out1=rem, out1_coff=0, wino=True)
    cat_c, rem_c = cat.cpu(), rem.cpu()
    assert torch.all(cat_c[..., :32] == 7.0) and torch.all(cat_c[..., 48:] == 7.0)
    _check(cat_c[..., 32:48], ref[:, :16])
    _check(rem_c, ref[:, 16:])
    x = big[:, :48].contiguous()
    ref = F.leaky_relu(F.conv2d(x, wt, b, padding=1), 0.05)
    cat = torch.zeros((n, h, w, 48), device=dev)
    remb = torch.full((n, 6, h, w, 8), 9.0, device=dev)
    ops.conv2d(_nhwc(x).to(dev), wt, b, act=1, split=16, out=cat, out_coff=16, out1=remb, blocked_out1=True, wino=True)
    _check(cat.cpu()[..., 16:32], ref[:, :16])
    r = remb.cpu().permute(0, 1, 4, 2, 3).reshape(n, 48, h, w)
    assert float((r - ref[:, 16:]).abs().max()) / max(1.0, float(ref.abs().max())) < 2e-5
    assert torch.all(cat.cpu()[..., :16] == 0) and torch.all(cat.cpu()[..., 32:] == 0)


def test_wino8_is_the_kernel_that_ran():
    """the profiled op list names wino8_f32_kernel for IMDN's conv2 / conv3 at batch 32 and wino_f32_kernel for the 64-channel layers"""
    from ntire2022_esr_amd.registry import select_model
    dev = _dev()
    m, _, dr, _ = select_model(-1, dev)
    m.enable_profiling(1)
    m(torch.rand(8, 3, 256, 256, device=dev) * dr)
    torch.cuda.synchronize()
    names = [o["kernel"] for o in m.collect_profile()]
    m.disable_profiling()
    assert sum(k.startswith("wino8_f32_kernel") for k in names) == 16, sorted(set(names))
    assert sum(k.startswith("wino_f32_kernel") for k in names) == 10, sorted(set(names))      # conv1 x 8, LR conv, last conv


@pytest.mark.parametrize("n,h,w", [(4, 256, 256), (1, 37, 29), (2, 5, 3), (3, 130, 70)])
def test_wino8_blocked_input(n, h, w):
    """channel-blocked INPUT [N, C/8, H, W, 8] (esr_conv_desc.blocked8 & ESR_BLOCKED_IN: IMDBlock's r1 / r2 since round 4) -- both Winograd
    kernels read it (pix_floats / chunk_stride; wino8_f32_kernel from 4096 strips of 4 x 16, wino_f32_kernel below); bit-identical to the
    NHWC input through the same kernel family"""
    from ntire2022_esr_amd import ops
    dev = _dev()
    case = P.wino8(48, 64, n, h, w, 1, blocked_out1=True, blocked_in=True, seed=31 + h)
    x, wt, b, ref = case.extra["x"], case.extra["w"], case.extra["b"], case.extra["ref32"]
    cat, rem = case.outs[0][..., :16], case.outs[0][..., 16:]                 # the 16 / 48 split, the blocked out1 read back as NHWC
    _check(cat.cpu(), ref[:, :16])
    r = rem.cpu().permute(0, 3, 1, 2)
    assert float((r - ref[:, 16:]).abs().max()) / max(1.0, float(ref.abs().max())) < 2e-5
    y_nhwc = ops.conv2d(_nhwc(x).to(dev), wt, b, act=1, wino=True)
    assert torch.equal(y_nhwc[..., :16], cat) and torch.equal(y_nhwc[..., 16:].cpu(), r.permute(0, 2, 3, 1))
