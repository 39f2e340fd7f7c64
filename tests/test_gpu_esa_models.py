"""-m gpu: ESA kernels per op vs ATen fp32 (CPU), RFDN / RLFN end to end vs the committed reference outputs
and the C oracle.  Tolerance 2e-5 * data_range; both networks run at data_range 255."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLD, load_sd_numpy, load_sd_torch, rel_err

pytestmark = pytest.mark.gpu
TOL = 2e-5
DEV = "cuda:0"


def _nhwc16(t):
    """NCHW [N,f,H,W] -> NHWC pitch 16 with zero pads, on the GPU."""
    n, f, h, w = t.shape
    o = torch.zeros(n, h, w, 16)
    o[..., :f] = t.permute(0, 2, 3, 1)
    return o.to(DEV)


def _esa_desc(L, n, h, w, h_lo, w_lo, x, y, **kw):
    d = L.EsaDesc()
    d.n, d.h, d.w, d.h_lo, d.w_lo = n, h, w, h_lo, w_lo
    d.x = L.View(ctypes.c_void_p(x.data_ptr()), x.shape[-1], 0)
    d.y = L.View(ctypes.c_void_p(y.data_ptr()), y.shape[-1], 0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("f,hw", [(12, (31, 30)), (16, (15, 17)), (12, (127, 127)), (16, (64, 37))])
def test_conv3x3s2_and_maxpool(f, hw):
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd.engine import pack_dense
    lib = L.lib()
    g = torch.Generator().manual_seed(f + hw[0])
    x = torch.randn(2, f, *hw, generator=g)
    w, b = torch.randn(f, f, 3, 3, generator=g) * 0.2, torch.randn(f, generator=g)
    ref = F.conv2d(x, w, b, stride=2)
    h2, w2 = ref.shape[-2:]
    xg = _nhwc16(x)
    y = torch.zeros(2, h2, w2, 16, device=DEV)
    pk = pack_dense(w, b, 16, 16).to(DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d = _esa_desc(L, 2, hw[0], hw[1], h2, w2, xg, y, f=f, w0=pk.data_ptr())
    L.check(lib.esr_conv3x3s2_f32(ctypes.byref(d), st), "s2")
    yc = y.cpu()
    assert float((yc[..., :f].permute(0, 3, 1, 2) - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max()))
    assert torch.all(yc[..., f:] == 0)
    if h2 >= 7 and w2 >= 7:
        refp = F.max_pool2d(ref, 7, 3)
        h3, w3 = refp.shape[-2:]
        z = torch.zeros(2, h3, w3, 16, device=DEV)
        d2 = _esa_desc(L, 2, h2, w2, h3, w3, y, z)
        L.check(lib.esr_maxpool7s3_f32(ctypes.byref(d2), st), "pool")
        assert torch.equal(z.cpu()[..., :f].permute(0, 3, 1, 2), F.max_pool2d(yc[..., :f].permute(0, 3, 1, 2), 7, 3))
    d.h_lo += 1
    assert lib.esr_conv3x3s2_f32(ctypes.byref(d), st) == -1          # inconsistent low-res dims rejected


# (test_esa_apply, the fp32 cases of the apply against ATen, lives in tests/test_gpu_esa_apply.py with the op's other value tests)


def _post_ends():
    """the ends of what esr_esa_apply_post_supported accepts: c = 33 and 64 (two channel pairs of tiles), one post of 1 / 32 outputs (one
    pair), 33 / 64 outputs (two pairs) alone or with a second post of 1 / 32; storage, activations, residual and skip_y alternate"""
    out, k = [], 0
    for c in (33, 64):
        for c0, c1 in [(1, 0), (32, 0)] + [(a, b) for a in (33, 64) for b in (0, 1, 32)]:
            for store in ("bf16", "f16"):
                out.append((store, c, c0, c1, ("lrelu", "none", "gelu")[k % 3], ("gelu", "lrelu")[k % 2] if c1 else None, k % 4 < 2, k % 3 == 1))
                k += 1
    return out


@pytest.mark.parametrize("store,c,c0,c1,act0,act1,res,skip", [
    ("bf16", 50, 25, 0, "lrelu", None, False, False),          # RFDN: y + the next block's c1_d
    ("f16", 48, 48, 24, "none", "gelu", True, True),            # BSRN: conv_out + block input, then the next block's c1_d; y not stored
    ("bf16", 48, 48, 24, "none", "gelu", True, True),
    ("f16", 48, 48, 0, "none", None, True, True),               # BSRN's last block
] + _post_ends())
def test_esa_apply_post_chain(store, c, c0, c1, act0, act1, res, skip):
    """esr_esa_desc.post[]: 1x1 convolutions riding in the ESA apply launch, against ATen on the values the launch stores
    (post 0 reads y as stored; post 1 reads post 0's fp32 result)."""
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd import ops
    import _esa_apply_ref as R
    assert L.lib().esr_esa_apply_post_supported(c, c0, c1) == 1
    dt = torch.bfloat16 if store == "bf16" else torch.float16
    f, hw, lo = 12, (37, 45), (5, 7)
    g = torch.Generator().manual_seed(c + c0 + c1)
    x = torch.randn(2, c, *hw, generator=g) * 3
    c1_ = torch.randn(2, f, *hw, generator=g)
    c3 = torch.randn(2, f, *lo, generator=g)
    wf, bf = torch.randn(f, f, generator=g) * 0.3, torch.randn(f, generator=g)
    w4, b4 = torch.randn(c, f, generator=g) * 0.3, torch.randn(c, generator=g)
    w0, b0 = torch.randn(c0, c, generator=g) * 0.2, torch.randn(c0, generator=g)
    w1, b1 = (torch.randn(c1, c0, generator=g) * 0.2, torch.randn(c1, generator=g)) if c1 else (None, None)
    r = torch.randn(2, c0, *hw, generator=g)

    def nhwc(t, pitch):
        o = torch.zeros(t.shape[0], t.shape[2], t.shape[3], pitch)
        o[..., :t.shape[1]] = t.permute(0, 2, 3, 1)
        return o.to(dt).to(DEV)
    pitch = (c + 15) // 16 * 16
    xg, c1g, rg = nhwc(x, pitch), nhwc(c1_, 16), nhwc(r, (c0 + 15) // 16 * 16)
    c3g = _nhwc16(c3)
    acts = {"none": L.ACT_NONE, "lrelu": L.ACT_LRELU, "gelu": L.ACT_GELU}
    post = [dict(weight=w0, bias=b0, act=acts[act0], slope=0.05, res=rg if res else None)]
    if c1:
        post.append(dict(weight=w1, bias=b1, act=acts[act1], slope=0.05))
    ysent = torch.full((2, hw[0], hw[1], pitch), 7.0, dtype=dt, device=DEV)
    y, outs = ops.esa_apply(xg, c1g, c3g, wf, bf, w4, b4, out=ysent, post=post, skip_y=skip)
    # y as the kernel stores it = the plain launch's result, bit for bit; and that result is held to the fp64 restatement of the op on the
    # rounded inputs through the comparator of tests/_esa_apply_ref.py (as tests/test_gpu_esa_apply.py does for the plain launch's own matrix)
    yplain = ops.esa_apply(xg, c1g, c3g, wf, bf, w4, b4)
    r = R.ref64(xg.cpu()[..., :c], c1g.cpu()[..., :f], c3.permute(0, 2, 3, 1), wf, bf, w4, b4, storage=store)
    R.compare(yplain.cpu()[..., :c], r, f"esa apply {store} c={c} in front of posts ({c0}, {c1})")
    if skip:
        assert torch.all(y == 7.0)
    else:
        assert torch.equal(y[..., :c], yplain[..., :c])
    fa = {"none": lambda t: t, "lrelu": lambda t: F.leaky_relu(t, 0.05), "gelu": F.gelu}
    yin = yplain.float().cpu()[..., :c].permute(0, 3, 1, 2).double()
    v0 = F.conv2d(yin, w0.double()[:, :, None, None], b0.double())
    if res:
        v0 = v0 + rg.float().cpu()[..., :c0].permute(0, 3, 1, 2).double()
    v0 = fa[act0](v0)
    eps = 2.0 ** -8 if store == "bf16" else 2.0 ** -11
    got0 = outs[0].float().cpu()[..., :c0].permute(0, 3, 1, 2).double()
    # one rounding of the stored result (+ the 16-bit GELU polynomial's 1.3e-4 on [-4, 4]; 2.13e-4 below -4, tests/_sweep.py)
    assert float((got0 - v0).abs().max()) <= eps * float(v0.abs().max()) + 3e-4
    assert torch.all(outs[0].float().cpu()[..., c0:] == 0)
    if c1:
        v1 = fa[act1](F.conv2d(v0, w1.double()[:, :, None, None], b1.double()))
        got1 = outs[1].float().cpu()[..., :c1].permute(0, 3, 1, 2).double()
        # post 1 sees post 0's fp32 result: hi + lo for bf16 (16 bits), the fp16 high part only for fp16 (11 bits)
        tol_in = (2.0 ** -11) * float(v0.abs().max()) * float(w1.abs().sum(dim=1).max())
        assert float((got1 - v1).abs().max()) <= eps * float(v1.abs().max()) + 2 * tol_in + 3e-4     # (fp16: post 1 weights carry 11 bits too)
        assert torch.all(outs[1].float().cpu()[..., c1:] == 0)


def _model(name):
    from ntire2022_esr_amd import RFDN, RLFN_cut
    m = {"rfdn_baseline": RFDN, "team04_rlfn": lambda: RLFN_cut(in_nc=3, out_nc=3)}[name]()
    m.load_state_dict(load_sd_torch(name), strict=True)
    m.eval()
    for p in m.parameters():
        p.requires_grad = False
    return m.to(DEV)


@pytest.mark.parametrize("name", ["rfdn_baseline", "team04_rlfn"])
def test_golden_e2e(name):
    m = _model(name)
    g = np.load(os.path.join(GOLD, f"e2e_{name}.npz"))
    dr = float(g["data_range"])
    for k in ("a", "b", "c"):
        x = torch.from_numpy(g["x" + k]).to(DEV)
        x0 = x.clone()
        y = m(x)
        assert y.shape == g["y" + k].shape
        assert torch.equal(x, x0)
        assert rel_err(y.cpu().numpy(), g["y" + k], dr) < TOL, (name, k)


@pytest.mark.parametrize("name", ["rfdn_baseline", "team04_rlfn"])
def test_vs_c_oracle_and_natural_image(name):
    from oracle import models as OM
    from PIL import Image
    m = _model(name)
    sd = load_sd_numpy(name)
    dr = OM.DATA_RANGE[name]
    rng = np.random.RandomState(7)
    for shape in [(1, 3, 15, 15), (2, 3, 31, 18), (1, 3, 33, 47)]:
        x = (rng.rand(*shape) * dr).astype(np.float32)
        y = m(torch.from_numpy(x).to(DEV)).cpu().numpy()
        assert rel_err(y, OM.FORWARD[name](sd, x), dr) < TOL, shape
    with pytest.raises(Exception):
        m(torch.rand(1, 3, 14, 20, device=DEV))                    # below ESA's minimum size
    g = np.load(os.path.join(GOLD, f"img_{name}.npz"))
    img = np.array(Image.open(os.path.join(GOLD, "test.bmp")).convert("RGB"))
    x = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).float().div(255.0 / dr).unsqueeze(0)
    y = m(x.to(DEV)).cpu()
    assert tuple(y.shape) == (1, 3, 1024, 1024)
    assert rel_err(y[0, :, ::5, ::5].numpy(), g["sr_sample"], dr) < TOL
    u8 = np.uint8((y[0].clamp(0, dr).permute(1, 2, 0).numpy() * 255.0 / dr).round())
    crop = u8[400:528, 300:428]
    assert np.mean(crop != g["sr_u8_crop"]) < 2e-4 and np.max(np.abs(crop.astype(int) - g["sr_u8_crop"].astype(int))) <= 1


@pytest.mark.parametrize("storage", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("f,n,hw,layers", [(12, 1, (31, 30), 3), (16, 2, (64, 37), 1), (16, 3, (127, 150), 1), (12, 1, (339, 510), 3),
                                           (16, 4, (256, 256), 2)])
def test_esa_lowres_op(storage, f, n, hw, layers):
    """esr_esa_lowres_f32 (conv2 s2 + max_pool2d(7, 3) + 1..3 3x3 layers, two launches with halo recompute) against ATen on the values
    the kernel reads (the 16-bit storages hold the conv1 map as bf16 / fp16: the reference gets the same rounded map).  The 16-bit
    kernels multiply by the fp32 weights split into 16-bit parts (bf16: 24 mantissa bits, fp16: 22), accumulate in fp32."""
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd.engine import pack_dense
    lib = L.lib()
    g = torch.Generator().manual_seed(1000 * f + 10 * n + hw[0] + layers)
    h, w = hw
    x = torch.randn(n, f, h, w, generator=g)
    st = {"f32": (0, torch.float32), "bf16": (1, torch.bfloat16), "f16": (2, torch.float16)}[storage]
    xq = x.to(st[1]).float()
    w2, b2 = torch.randn(f, f, 3, 3, generator=g) * 0.2, torch.randn(f, generator=g) * 0.1
    ws = [(torch.randn(f, f, 3, 3, generator=g) * 0.2, torch.randn(f, generator=g) * 0.1) for _ in range(layers)]
    ref = F.max_pool2d(F.conv2d(xq.double(), w2.double(), b2.double(), stride=2), 7, 3)
    for i, (wl, bl) in enumerate(ws):
        ref = F.conv2d(ref, wl.double(), bl.double(), padding=1)
        if i + 1 < layers:
            ref = F.relu(ref)
    h3, w3 = ref.shape[2:]
    xd = _nhwc16(xq).to(st[1]).contiguous()
    blobs = [pack_dense(w2, b2, 16, 16).to(DEV)] + [pack_dense(wl, bl, 16, 16).to(DEV) for wl, bl in ws]
    pooled = torch.full((n, h3, w3, 16), float("nan"), device=DEV)
    y = torch.full((n, h3, w3, 16), float("nan"), device=DEV)
    d = L.EsaLowresDesc()
    d.n, d.h, d.w, d.f, d.storage, d.n_layers = n, h, w, f, st[0], layers
    d.x = L.View(ctypes.c_void_p(xd.data_ptr()), 16, 0)
    d.w_s2, d.pooled, d.y = blobs[0].data_ptr(), pooled.data_ptr(), y.data_ptr()
    for i in range(layers):
        d.layer[i].kind, d.layer[i].act, d.layer[i].w = 0, (L.ACT_RELU if i + 1 < layers else L.ACT_NONE), blobs[1 + i].data_ptr()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.esr_esa_lowres_f32(ctypes.byref(d), stream), "esr_esa_lowres_f32")
    torch.cuda.synchronize()
    got = y.cpu()[..., :f].permute(0, 3, 1, 2).double()
    pref = F.max_pool2d(F.conv2d(xq.double(), w2.double(), b2.double(), stride=2), 7, 3)
    perr = float((pooled.cpu()[..., :f].permute(0, 3, 1, 2).double() - pref).abs().max() / pref.abs().max())
    err = float((got - ref).abs().max() / ref.abs().max())
    assert perr < 2e-6 and err < 4e-6, (perr, err)
