"""-m gpu: the values of ops.esa_apply -- esa_apply_kernel<0> (fp32) and esa_apply_mfma_kernel<ST, NP, 0, 0> (bf16 / fp16 storage) -- against
the fp64 restatement of tests/_esa_apply_ref.py, through its comparator: (a) a derived per-element bound, (b) the share of stored values
that are not the correctly rounded reference, (c) the share that differs from the CPU emulation of the kernel's documented arithmetic.  tests/test_esa_apply_ref.py shows on the CPU that both are met by the kernel's documented
arithmetic and missed by each way of getting it subtly wrong.  Geometries and widths: _esa_apply_ref.GEOMS / WIDTHS (what each reaches is
in DESIGN.md section 2f).  y always goes into a channel slice of a sentinel-filled wider buffer; (50, 12) reads x from channel 8 of a
wider pitch.  No case has W < 8: the launcher refuses that (tests/test_abi_and_host.py), and the one test here that asks for it only
confirms the refusal -- nothing is launched."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _esa_apply_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 5.0
STORES = ["f32", "bf16", "f16"]
CASES = R.combos()
IDS = [R.case_id(g, wd) for g, wd in CASES]


def _pad16(t):
    """NHWC [..., f] -> pitch 16 with zero pad channels, on the GPU"""
    o = torch.zeros(*t.shape[:-1], 16, dtype=t.dtype)
    o[..., :t.shape[-1]] = t
    return o.to(DEV)


def _run(geom, width, storage, ref_device=None):
    """one launch under kernel_trace() and every assertion of a case; returns the comparator's figures"""
    from ntire2022_esr_amd import ops
    n, h, w, _ = geom
    c, f = width
    dt = R.DTYPES[storage]
    gran = 4 if storage == "f32" else 8
    cg = (c + gran - 1) // gran * gran
    inp = R.make_inputs(geom, width, storage)
    # x: the channels in front of and behind the view hold values that would show in y; its own pad channels are zero
    x_coff = 8 if width == (50, 12) else 0
    xb = torch.full((n, h, w, x_coff + cg + (8 if x_coff else 0)), 100.0, dtype=dt)
    xb[..., x_coff:x_coff + cg] = 0
    xb[..., x_coff:x_coff + c] = inp["x"]
    y = torch.full((n, h, w, 8 + cg + 8), SENTINEL, dtype=dt, device=DEV)
    with ops.kernel_trace() as names:
        ops.esa_apply(xb.to(DEV), _pad16(inp["c1"]), _pad16(inp["c3"]), inp["wf"], inp["bf"], inp["w4"], inp["b4"], out=y, x_coff=x_coff, out_coff=8)
    torch.cuda.synchronize()
    st = ops.L.STORE[storage]
    want = "esa_apply_kernel<0>" if storage == "f32" else f"esa_apply_mfma_kernel<{st}, {((c + 3) // 4 * 4 + 31) // 32}, 0, 0>"
    assert names == [want], (names, want)
    what = f"esa apply {storage} {R.case_id(geom, width)} {names[0]}"
    if ref_device is None:
        y = y.cpu()
    r = R.ref64(**inp, storage=storage, device=ref_device)
    fig = R.compare(y[..., 8:8 + c], r, what, emu=None if storage == "f32" else R.emulate32(**inp, storage=storage))
    # the pad channels of the last granule are x's zeros times a gate; every byte outside the slice keeps the sentinel
    assert bool((y[..., 8 + c:8 + cg] == 0).all()), what
    sent = torch.full_like(y[..., :8], SENTINEL)
    assert torch.equal(y[..., :8], sent) and torch.equal(y[..., 8 + cg:], sent), what
    return fig


@pytest.mark.parametrize("storage", STORES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_values(storage, case):
    _run(*case, storage)


@pytest.mark.parametrize("storage,width", [("bf16", (50, 12)), ("f16", (32, 16))])
def test_values_many_groups(storage, width):
    """67 500 groups of 16 pixels: more than the 4096 blocks x 4 waves x 2 groups of one pass, so every wave runs several two-group
    iterations with both fetches live.  The fp64 reference is built on the device."""
    _run(R.BIG, width, storage, ref_device=DEV)


@pytest.mark.parametrize("storage", STORES)
def test_w7_is_refused_and_nothing_is_written(storage):
    """W = 7 raises EsrError from the launcher's argument checks -- nothing is launched -- and `out` keeps its sentinel"""
    from ntire2022_esr_amd import ops
    dt = R.DTYPES[storage]
    inp = R.make_inputs((2, 19, 7, (3, 1)), (50, 12), storage)
    x = torch.zeros(2, 19, 7, 56, dtype=dt)
    x[..., :50] = inp["x"]
    y = torch.full((2, 19, 7, 56), SENTINEL, dtype=dt, device=DEV)
    with pytest.raises(ops.L.EsrError):
        ops.esa_apply(x.to(DEV), _pad16(inp["c1"]), _pad16(inp["c3"]), inp["wf"], inp["bf"], inp["w4"], inp["b4"], out=y)
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full_like(y, SENTINEL))


@pytest.mark.parametrize("c,f,hw,lo", [(50, 12, (40, 56), (5, 8)), (46, 16, (33, 17), (4, 1)), (48, 12, (64, 64), (9, 9)),
                                       (50, 12, (20, 36), (1, 4))])
def test_esa_apply(c, f, hw, lo):
    """y = x * sigmoid(conv4(bilinear(c3) + conv_f(c1_)))  (rfdn_baseline/block.py:124-129): the C entry point on fp32 storage with a
    hand-filled descriptor, against ATen's fp32 on the CPU, x ~ 30 randn (from tests/test_gpu_esa_models.py, unchanged)."""
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd.engine import pack_dense
    lib = L.lib()
    g = torch.Generator().manual_seed(c + f + hw[0])
    x = torch.randn(2, c, *hw, generator=g) * 30
    c1 = torch.randn(2, f, *hw, generator=g)
    c3 = torch.randn(2, f, *lo, generator=g)
    wf, bf = torch.randn(f, f, 1, 1, generator=g) * 0.3, torch.randn(f, generator=g)
    w4, b4 = torch.randn(c, f, 1, 1, generator=g) * 0.3, torch.randn(c, generator=g)
    ref = x * torch.sigmoid(F.conv2d(F.interpolate(c3, hw, mode="bilinear", align_corners=False) + F.conv2d(c1, wf, bf), w4, b4))
    pitch = (c + 7) // 8 * 8
    xg = torch.zeros(2, *hw, pitch)
    xg[..., :c] = x.permute(0, 2, 3, 1)
    xg = xg.to(DEV)
    y = torch.full((2, hw[0], hw[1], pitch + 8), 5.0, device=DEV)      # write into a slice of a wider buffer
    cp4 = (c + 3) // 4 * 4
    d = L.EsaDesc()
    d.n, d.h, d.w, d.c, d.f, d.h_lo, d.w_lo = 2, hw[0], hw[1], c, f, lo[0], lo[1]
    d.x = L.View(ctypes.c_void_p(xg.data_ptr()), pitch, 0)
    d.y = L.View(ctypes.c_void_p(y.data_ptr()), pitch + 8, 8)
    c1g, c3g = _pad16(c1.permute(0, 2, 3, 1)), _pad16(c3.permute(0, 2, 3, 1))
    pf, p4 = pack_dense(wf, bf, 16, 16).to(DEV), pack_dense(w4, b4, 16, cp4).to(DEV)
    d.c1, d.c3, d.w0, d.w1 = c1g.data_ptr(), c3g.data_ptr(), pf.data_ptr(), p4.data_ptr()
    L.check(lib.esr_esa_apply_f32(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "apply")
    yc = y.cpu()
    got = yc[..., 8:8 + c].permute(0, 3, 1, 2)
    assert float((got - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max()))
    assert torch.all(yc[..., :8] == 5.0) and torch.all(yc[..., 8 + cp4:] == 5.0)
