"""CPU-only (-m "not gpu"): the C-ABI library loads and exports every symbol include/esr_hip.h
declares, the host-side packer round-trips, argument validation rejects bad descriptors without a
GPU, and the product refuses to run without one (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, load_sd_torch


def _header_symbols():
    txt = open(os.path.join(REPO, "include", "esr_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(esr_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    syms = _header_symbols()
    assert len(syms) >= 10
    for s in syms:
        assert hasattr(lib, s), f"libesr_hip.so does not export {s}"
    assert set(L.EXPORTS) == set(syms), (set(L.EXPORTS) ^ set(syms))
    assert lib.esr_abi_version() == 12
    # the ctypes mirrors of the ABI structs have the library's sizes (also checked by _lib.lib() at load time)
    for which, st in enumerate((L.View, L.ConvDesc, L.EsaDesc, L.BsDesc, L.CaDesc, L.Op, L.EsaLowresDesc, L.ChainDesc)):
        assert lib.esr_sizeof(which) == ctypes.sizeof(st) > 0, st.__name__
    assert lib.esr_sizeof(99) == 0
    assert b"gfx950" in lib.esr_build_info()


def test_no_reference_or_oracle_import_in_product():
    """The product path must never route through oracle/ (or /root/reference)."""
    pkg = os.path.join(REPO, "ntire2022_esr_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(root, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f
                assert "/root/reference" not in src, f


@pytest.mark.parametrize("cin,cout,k", [(64, 64, 3), (48, 16, 3), (3, 64, 3), (100, 50, 1), (50, 25, 1), (12, 12, 3)])
def test_pack_roundtrip(cin, cout, k):
    from ntire2022_esr_amd.engine import pack_conv, unpack_conv
    g = torch.Generator().manual_seed(cin + cout + k)
    w, b = torch.randn(cout, cin, k, k, generator=g), torch.randn(cout, generator=g)
    blob = pack_conv(w, b)
    w2, b2 = unpack_conv(blob, cin, cout, k)
    assert torch.equal(w, w2) and torch.equal(b, b2)
    # padded lanes are exactly zero (keeps pad channels at act(0)=0 downstream)
    nz = int((blob != 0).sum())
    assert nz <= w.numel() + b.numel()


def test_pack_with_channel_map():
    from ntire2022_esr_amd.engine import pack_conv, unpack_conv
    w, b = torch.randn(32, 20, 1, 1), torch.randn(32)
    cmap = list(range(10)) + [-1, -1] + list(range(10, 20)) + [-1, -1]
    blob = pack_conv(w, b, cin_map=cmap)
    w2, b2 = unpack_conv(blob, 20, 32, 1, cin_map=cmap)
    assert torch.equal(w, w2) and torch.equal(b, b2)


def test_linear_weights_pack_as_1x1():
    from ntire2022_esr_amd.engine import pack_conv
    w, b = torch.randn(24, 48), torch.randn(24)
    assert torch.equal(pack_conv(w, b), pack_conv(w[:, :, None, None], b))


def test_descriptor_validation_without_gpu():
    """esr_conv2d_f32 validates before it launches: bad descriptors fail identically on a CPU-only host."""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    d = L.ConvDesc()
    assert lib.esr_conv2d_f32(ctypes.byref(d), None) == -1          # null pointers
    assert lib.esr_conv2d_f32(None, None) == -1
    buf = (ctypes.c_float * 16)()
    d.inp = L.View(ctypes.addressof(buf), 64, 0)
    d.out0 = L.View(ctypes.addressof(buf), 64, 0)
    d.wpacked = ctypes.addressof(buf)
    d.n, d.h, d.w, d.cin, d.cout, d.ksize = 1, 4, 4, 64, 64, 5
    assert lib.esr_conv2d_f32(ctypes.byref(d), None) == -2          # k = 5 unsupported
    d.ksize, d.cout = 3, 80
    assert lib.esr_conv2d_f32(ctypes.byref(d), None) == -2          # cout > 64
    d.cout, d.inp.pitch = 64, 62
    assert lib.esr_conv2d_f32(ctypes.byref(d), None) == -1          # pitch not a multiple of 4
    d.inp.pitch, d.inp.coff = 64, 16
    assert lib.esr_conv2d_f32(ctypes.byref(d), None) == -1          # chunked reads would leave the pixel
    assert lib.esr_run_ops(None, 1, None) == -1
    assert lib.esr_packed_conv_bytes(64, 64, 2) == 0
    if torch.cuda.device_count() == 0:
        # a VALID descriptor on a host without a GPU: the launch itself fails, and esr_check_launch reports it under the launcher's
        # name (only here: with a GPU the launch would run, on these host pointers)
        d.inp.coff = 0
        lib.esr_last_hip_error.restype = ctypes.c_char_p
        assert lib.esr_conv2d_f32(ctypes.byref(d), None) == -3          # ESR_ERR_LAUNCH
        assert lib.esr_last_hip_error().startswith(b"conv_f32_kernel launch: "), lib.esr_last_hip_error()
        # 16-bit storage: the LDS opt-in comes first and has no device to ask
        d.in_layout = d.out_layout = L.NHWC
        d.storage = d.compute = L.STORE["bf16"]
        assert lib.esr_conv2d_f32(ctypes.byref(d), None) == -3


@pytest.mark.parametrize("storage", ["f32", "bf16", "f16"])
def test_esa_apply_refuses_narrow_images_without_gpu(storage):
    """esr_esa_apply_f32 needs W >= 8 (both kernels carry a 16-pixel group's column over at most two rows): W < 8 is ESR_ERR_UNSUPPORTED in
    every storage type, with the other argument checks and before anything is launched -- on a CPU-only host as on a GPU box."""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)

    def desc(w, **kw):
        d = L.EsaDesc()
        d.n, d.h, d.w, d.c, d.f, d.h_lo, d.w_lo = 2, 19, w, 50, 12, 3, 1
        d.storage = L.STORE[storage]
        d.x, d.y = L.View(a, 56, 0), L.View(a, 56, 0)
        d.c1 = d.c3 = d.w0 = d.w1 = a
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.esr_esa_apply_f32(ctypes.byref(d), None)

    for w in (1, 5, 7):
        assert desc(w) == -2, w
        assert desc(w, skip_y=1) == -2, w                # ahead of the checks behind it
    assert desc(0) == -1 and desc(-3) == -1              # no width at all stays a bad argument
    # w = 8 passes the width check: the descriptor goes on to a LATER check (skip_y without a post chain: ESR_ERR_BAD_ARG), which stops it
    # in front of the launch on any host
    assert desc(8, skip_y=1) == -1 and desc(9, skip_y=1) == -1
    if torch.cuda.device_count() == 0:
        # and the valid descriptor reaches the launch, which fails for want of a device (as test_descriptor_validation_without_gpu)
        assert desc(8) == -3


def test_hilo_descriptor_validation_without_gpu():
    """esr_conv_desc.hilo (ABI v10) is validated before anything is launched: unknown bits, a missing stride, fp16 storage, a 1x1, two output
    tiles, a segmented input and a post chain next to the input / residual flags are refused on a CPU-only host as on a GPU box."""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)

    def desc(**kw):
        d = L.ConvDesc()
        d.n, d.h, d.w, d.cin, d.cout, d.ksize = 1, 32, 32, 48, 48, 3
        d.in_layout = d.out_layout = L.NHWC
        d.storage = d.compute = L.STORE["bf16"]
        d.inp, d.out0, d.res = L.View(a, 48, 0), L.View(a, 48, 0), L.View(a, 48, 0)
        d.wpacked = a
        d.hilo, d.hilo_stride = L.HILO_OUT, 4096
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.esr_conv2d_f32(ctypes.byref(d), None)

    assert desc(hilo=8) == -1                                              # unknown bit
    assert desc(hilo_stride=0) == -1 and desc(hilo_stride=24) == -1        # no stride / not a multiple of 16
    assert desc(storage=L.STORE["f16"], compute=L.STORE["f16"]) == -2      # fp16: 11 bits already
    assert desc(ksize=1) == -2 and desc(cout=32) == -2                      # 1x1; two output tiles
    assert desc(hilo=L.HILO_RES) == -1                                     # a residual pair without a residual
    assert desc(out_layout=L.NCHW_SHUFFLE4) == -1                          # the output pair is NHWC
    assert desc(hilo=L.HILO_IN | L.HILO_OUT, post_wpacked=a, post_cout=24, post_out=L.View(a, 32, 0)) == -2    # a post 1x1 rides with HILO_OUT alone
    assert desc(split=16, out1=L.View(a, 48, 0)) == -2                     # no split store
    # (round 5) the border table is staged by 16-byte LDS-DMA pieces: a misaligned one is refused before anything is launched
    assert desc(hilo=0, hilo_stride=0, border_bias=a + 4) == -1


def test_module_surface_and_no_cpu_fallback():
    from ntire2022_esr_amd import IMDN, _lib as L
    m = IMDN(in_nc=3, out_nc=3, nc=64, nb=8, upscale=4, act_mode='L', upsample_mode='pixelshuffle', negative_slope=0.05)
    missing, unexpected = m.load_state_dict(load_sd_torch("imdn_baseline"), strict=True)
    assert not missing and not unexpected
    assert sum(p.numel() for p in m.parameters()) == 893936                # figs/results.png: 0.894 M
    m.eval()
    for _, v in m.named_parameters():                                        # test_demo.py:338-339
        v.requires_grad = False
    assert list(m.parameters())[-1].device.type == "cpu"                    # model_summary.py:37 idiom
    with pytest.raises(L.EsrError, match="no CPU fallback"):
        m(torch.rand(1, 3, 16, 16))
    with pytest.raises(NotImplementedError):
        IMDN(upsample_mode="upconv")
    with pytest.raises(AssertionError):
        IMDN(act_mode="X")
    m7 = IMDN(nb=7)                                                           # id 26, test_demo.py:203-209
    assert len(m7.state_dict()) == 86 - 10


def test_imdn_plan_shape():
    """The op list is 3 + 4*nb launches (conv4 and the 1x1 share one) and its workspace matches the documented layout."""
    from ntire2022_esr_amd import IMDN
    from ntire2022_esr_amd.engine import Plan
    m = IMDN()
    plan = Plan(2, 40, 56)
    m._build_plan(plan, 3)
    assert len(plan.ops) == 3 + 4 * 8
    assert sum(o.tail is not None for o in plan.ops) == 8
    assert plan.total == 4 * 2 * 40 * 56 * (64 * 4 + 48 * 4)                  # bytes: fea, xa, xb, lr | cat (d1 d2 d3), r1, r2, r3
    blk = [bf for bf in plan.buffers if bf.blocked]
    # channel-blocked [n][c/8][h][w][8]: the IMDBlocks' x (ping-pong) and every "remaining" slice; fea, lr and cat stay NHWC
    assert [bf.name for bf in blk] == ["xa", "xb", "r1", "r2", "r3"]
    r3 = blk[-1]
    assert all((o.dst1 is r3) == o.w.endswith("conv3.0") and (o.src is r3) == (o.tail is not None) for o in plan.ops)
    m.winograd = False                                                          # the direct kernels read NHWC: only r3 stays blocked
    plan = Plan(2, 40, 56)
    m._build_plan(plan, 3)
    assert [bf.name for bf in plan.buffers if bf.blocked] == ["r3"]
    m.winograd = True
    plan = Plan(2, 40, 56)
    m._build_plan(plan, 3)
    assert m.workspace_bytes(2, 40, 56) == plan.total
    total_macs = sum(cin * cout * k * k for o in plan.ops for (cin, cout, k, _, _) in m._counted_convs(plan, o))
    assert total_macs == 891584                                                # MAC per LR pixel
    m32 = IMDN(nc=32)                                                          # no 16-channel distillation: unfused
    plan = Plan(1, 40, 56)
    m32._build_plan(plan, 3)
    assert len(plan.ops) == 3 + 5 * 8 and all(o.tail is None for o in plan.ops)
    for nc in (16, 48):                                                        # 3/4 nc is not a whole number of 8-channel chunks
        with pytest.raises(NotImplementedError):
            IMDN(nc=nc)


def test_s16_packer_layout_diffusion_and_split():
    """esr_pack_conv_s16: [chunk of 16][tap pair][tile][lane][8] 16-bit image + fp32 bias; 3x3 taps rounded with error
    diffusion (the filter's tap SUM stays exact to one rounding), 1x1 stored as hi + lo in the two tap slots of the pair."""
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    g = torch.Generator().manual_seed(3)
    w, b = torch.randn(16, 16, 3, 3, generator=g), torch.randn(16, generator=g)
    for mode, dt, eps in (("bf16", torch.bfloat16, 2.0 ** -8), ("f16", torch.float16, 2.0 ** -11)):
        blob = pack_conv_s16(w, b, mode)
        raw = blob.numpy().view(np.uint16)
        nw = 1 * 5 * 1 * 64 * 8                                 # chunks x pairs x tiles x lanes x 8
        vals = torch.from_numpy(raw[:nw].astype(np.int16)).view(dt).float().reshape(5, 64, 8)
        weff, beff = unpack_conv_s16(blob, 16, 16, 3, mode)
        assert torch.equal(beff, b)
        for tap in range(9):
            q, hk = tap // 2, tap % 2
            for half in range(2):
                kq = hk * 2 + half
                got = vals[q, kq * 16:(kq + 1) * 16, :]          # [cout i][j]: channels 8*half + j of tap `tap`
                assert torch.equal(got, weff[:, 8 * half:8 * half + 8, tap // 3, tap % 3]), (mode, tap, half)
        assert torch.all(vals[4, 32:, :] == 0)                   # the padding 10th tap
        # every effective weight is a 16-bit value; diffusion moves a tap by at most the rounding errors of its neighbours,
        # i.e. by less than an ulp of the filter's largest tap ...
        assert torch.equal(weff, weff.to(dt).float())
        assert float(((weff - w).abs() / w.abs().amax(dim=(2, 3), keepdim=True)).max()) < 2 * eps
        # ... and the tap sum of every (cout, cin) filter is far closer to the fp32 sum than independent rounding gets
        e_diff = (weff.sum(dim=(2, 3)) - w.sum(dim=(2, 3))).abs()
        e_rne = (w.to(dt).float().sum(dim=(2, 3)) - w.sum(dim=(2, 3))).abs()
        assert float(e_diff.mean()) < 0.5 * float(e_rne.mean())
        bias = torch.from_numpy(blob.numpy().view(np.uint8)[nw * 2:nw * 2 + 64].copy()).view(torch.float32)
        assert torch.equal(bias, b)
        # 1x1: hi + lo reproduces the fp32 weight to ~2^-16 (bf16) relative
        w1 = torch.randn(24, 40, generator=g)
        m = [i if i % 8 < 5 else -1 for i in range(64)]          # a padded concat layout: 8 slices of 5 channels in 8 slots
        m = [(s // 8) * 5 + s % 8 if s % 8 < 5 else -1 for s in range(64)]
        blob1 = pack_conv_s16(w1, None, mode, cin_map=m)
        w1e, b1e = unpack_conv_s16(blob1, 40, 24, 1, mode, cin_map=m)
        assert bool(((w1e[:, :, 0, 0] - w1).abs() <= (w1.abs() * eps * eps * 8).clamp_min(6.0e-8)).all())   # fp16 lo: subnormal floor
        assert torch.all(b1e == 0)
    lib = __import__("ntire2022_esr_amd._lib", fromlist=["lib"]).lib()
    assert lib.esr_packed_conv_s16_bytes(64, 64, 3) == 4 * 5 * 4 * 1024 + 256 + 72 * 1024      # + the 32x32x16 image (esr_c64m.hip)
    assert lib.esr_packed_conv_s16_bytes(256, 50, 1) == 16 * 1 * 4 * 1024 + 256
    assert lib.esr_packed_conv_s16_bytes(64, 64, 2) == 0


# (cin, cout, k) of the layers that the channel-width cases of the GPU tests launch (tests/test_gpu_{h16, fmen, chain, esan, bmdn, c64m}.py)
_HFAB_W = [(33, 1), (39, 9), (44, 16), (49, 8), (51, 1), (61, 16), (62, 9), (64, 8)]
WIDTH_LAYERS = sorted({(c, m, 3) for c, m in _HFAB_W} | {(m, m, 3) for _, m in _HFAB_W} | {(m, c, 3) for c, m in _HFAB_W} |                # HFAB
                      {(33, 33, 3), (41, 34, 3), (34, 34, 3), (34, 41, 3), (40, 47, 3), (47, 47, 3), (47, 40, 3), (48, 48, 3)} |            # RLFB
                      {(32, 32, 3), (32, 1, 1), (32, 9, 1), (32, 16, 1), (32, 32, 1)} |                                                     # ESAN's head
                      {(17, 17, 1), (27, 32, 1), (32, 25, 1), (18, 24, 1), (22, 32, 1), (31, 17, 1), (33, 17, 1), (45, 32, 1), (48, 25, 1)} |   # BMDN's d
                      {(c, c, 3) for c in (33, 41, 47, 49, 57, 63)} | {(49, 24, 3), (57, 17, 3), (63, 32, 3), (56, 31, 3)} |                # c{j}_r, c4
                      {(41, 31, 3), (47, 32, 3), (33, 17, 3)})                                                                              # ESDB's c4


def _s16_image_checks(blob, w, b, mode, cin_map, k):
    """what every 16-bit packer test here asserts of a blob: the effective weights within one storage ulp of w per tap, the bias exact, and every
    element of the tap-pair image, the bias block and the 32x32x16 image that no (slot, tap, output channel) of the layer owns exactly zero"""
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd.engine import unpack_conv_s16
    dt, eps = (torch.bfloat16, 2.0 ** -8) if mode == "bf16" else (torch.float16, 2.0 ** -11)
    cout, cin = w.shape[:2]
    cp = len(cin_map)
    weff, beff = unpack_conv_s16(blob, cin, cout, k, mode, cin_map=cin_map)
    assert torch.equal(beff, b)
    if k == 3:
        # error diffusion moves a tap by less than the rounding errors it carries: one ulp (2 eps relative) of the filter's largest tap
        assert torch.equal(weff, weff.to(dt).float())
        assert float(((weff - w).abs() / w.abs().amax(dim=(2, 3), keepdim=True)).max()) < 2 * eps
    else:
        # hi + lo: the fp32 weight to the square of the storage precision (fp16's low part: its subnormal floor)
        assert bool(((weff - w).abs() <= (w.abs() * eps * eps * 8).clamp_min(6.0e-8)).all())
    nt, nch, taps = (cout + 15) // 16, (cp + 15) // 16, k * k
    pairs = (taps + 1) // 2
    raw = torch.from_numpy(blob.numpy().view(np.int16).astype(np.int64))
    nw = nch * pairs * nt * 512
    owned = torch.zeros(nw, dtype=torch.bool)
    sl = torch.tensor([s_ for s_ in range(cp) if cin_map[s_] >= 0])
    ts = torch.arange(taps if k == 3 else 2)              # (1x1: the pair's second slot carries the low part)
    oc = torch.arange(cout)
    S, T, O = torch.meshgrid(sl, ts, oc, indexing="ij")
    idx = ((((S // 16) * pairs + T // 2) * nt + O // 16) * 64 + ((T & 1) * 2 + (S % 16) // 8) * 16 + O % 16) * 8 + S % 8       # (s16_index, esr_s16.hip)
    owned[idx.reshape(-1)] = True
    assert int(owned.sum()) == idx.numel() and torch.all(raw[:nw][~owned] == 0)
    bias = torch.from_numpy(blob.numpy().view(np.uint8)[nw * 2:nw * 2 + nt * 64].copy()).view(torch.float32)
    assert torch.equal(bias[:cout], b) and torch.all(bias[cout:] == 0)
    # the 32x32x16 image, where the blob has one: the same multiset of 16-bit values as the tap-pair image (so: no row dropped, nothing else set)
    total = L.lib().esr_packed_conv_s16_bytes(cp, cout, k)
    assert blob.numel() * 4 >= total
    m32 = raw[nw + nt * 32:total // 2]
    if len(m32):
        assert torch.equal(torch.sort(m32[m32 != 0]).values, torch.sort(raw[:nw][raw[:nw] != 0]).values)


@pytest.mark.parametrize("cin,cout,k", WIDTH_LAYERS)
def test_s16_pack_roundtrip_at_every_tested_width(cin, cout, k):
    """esr_pack_conv_s16 / esr_unpack_conv_s16 at the widths of the GPU tests' channel-width cases, both storage types"""
    from ntire2022_esr_amd.engine import pack_conv_s16
    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + k)
    w, b = torch.randn(cout, cin, k, k, generator=g) * 0.1, torch.randn(cout, generator=g)
    cp = (cin + 15) // 16 * 16
    for mode in ("bf16", "f16"):
        _s16_image_checks(pack_conv_s16(w, b, mode, cin_phys=cp), w, b, mode, [s_ if s_ < cin else -1 for s_ in range(cp)], k)


@pytest.mark.parametrize("cin,cmid,cout", [(17, 17, 17), (33, 17, 25), (48, 32, 32)])
def test_distill_fold_roundtrip_at_the_ends_of_its_ranges(cin, cmid, cout):
    """engine.pack_distill_s16 / distill_cin_map: the folded 3x3 over [in chunks | d chunks], its pad rows between and behind the two zero"""
    from ntire2022_esr_amd.engine import distill_cin_map, pack_distill_s16
    g = torch.Generator().manual_seed(100 * cin + cmid)
    w_r, b_r = torch.randn(cout, cin, 3, 3, generator=g) * 0.05, torch.randn(cout, generator=g) * 0.1
    w_b, b_b = torch.randn(cout, cmid, 3, 3, generator=g) * 0.05, torch.randn(cout, generator=g) * 0.1
    cmap = distill_cin_map(cin, cmid)
    assert len(cmap) == (cin + 15) // 16 * 16 + (cmid + 15) // 16 * 16 and sorted(c for c in cmap if c >= 0) == list(range(cin + cmid))
    for mode in ("bf16", "f16"):
        _s16_image_checks(pack_distill_s16(w_r, b_r, w_b, b_b, mode), torch.cat([w_r, w_b], 1), b_r + b_b, mode, cmap, 3)


def test_m32_images_hold_the_same_weights_as_the_tap_pair_images():
    """Round 6 (csrc/esr_c64m.hip): esr_pack_conv_s16 appends the 64 -> 64 3x3's weights in v_mfma_f32_32x32x16's fragment order -- fragment
    (chunk, tap, half) of 1 KB, lane 32 h + i, slot j = output channel 32 half + i, input slot 16 chunk + 8 h + j -- and esr_pack_post_s16 the
    post 1x1's images -- step c / 8, (hi, lo), lane 32 ((c % 8) / 4) + o, slots c % 4 (and + 4 in the hi image).  Both must hold exactly the
    16-bit values of the tap-pair / 16x16x32 images (what esr_unpack_conv_s16 reads), zeros elsewhere."""
    import numpy as np
    from ntire2022_esr_amd.engine import pack_conv_s16, pack_post_s16, unpack_conv_s16
    g = torch.Generator().manual_seed(11)
    for mode, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        cin = cout = 50
        w, b = torch.randn(cout, cin, 3, 3, generator=g) * 0.1, torch.randn(cout, generator=g)
        blob = pack_conv_s16(w, b, mode, cin_phys=64)
        weff, beff = unpack_conv_s16(blob, cin, cout, 3, mode, cin_phys=64)
        raw = blob.numpy().view(np.uint16)
        off = (4 * 5 * 4 * 1024 + 256) // 2
        img = torch.from_numpy(raw[off:off + 72 * 512].astype(np.int16)).view(dt).float().reshape(4, 9, 2, 2, 32, 8)   # [chunk][tap][half][h][i][j]
        got = torch.zeros(64, 64, 9)
        for c in range(4):
            for h in range(2):
                # img[c, tap, half, h, i, j] = W[32 half + i][16 c + 8 h + j][tap]
                blk = img[c, :, :, h]                                   # [tap][half][i][j]
                got[:, 16 * c + 8 * h:16 * c + 8 * h + 8, :] = blk.permute(1, 2, 3, 0).reshape(64, 8, 9)
        assert torch.equal(got[:cout, :cin].reshape(cout, cin, 3, 3), weff)
        assert torch.all(got[cout:] == 0) and torch.all(got[:, cin:] == 0)
        assert len(raw) * 2 == 4 * 5 * 4 * 1024 + 256 + 72 * 1024
        # the post 1x1 (64 -> 32 physical): hi + lo of the m32 images = the fp32 weight to the storage type's hi + lo accuracy
        pc = 25
        wp, bp = torch.randn(pc, cin, generator=g) * 0.2, torch.randn(pc, generator=g)
        pblob = pack_post_s16(wp, bp, mode)
        praw = pblob.numpy().view(np.uint16)
        poff = (2 * 4 * 2 * 1024 + 2 * 16 * 4) // 2
        pim = torch.from_numpy(praw[poff:poff + 16 * 512].astype(np.int16)).view(dt).float().reshape(8, 2, 2, 32, 8)     # [step][hi | lo][h][o][j]
        hi = torch.zeros(32, 64); lo = torch.zeros(32, 64)
        for st in range(8):
            for h in range(2):
                for jj in range(4):
                    c = 8 * st + 4 * h + jj
                    hi[:, c] = pim[st, 0, h, :, jj]
                    assert torch.equal(pim[st, 0, h, :, jj + 4], pim[st, 0, h, :, jj])         # slots 4 .. 7 meet the activations' low parts
                    lo[:, c] = pim[st, 1, h, :, jj]
                    assert torch.all(pim[st, 1, h, :, jj + 4] == 0)
        assert torch.equal(hi[:pc, :cin], wp.to(dt).float())
        assert torch.equal(lo[:pc, :cin], (wp - wp.to(dt).float()).to(dt).float())
        assert torch.all(hi[pc:] == 0) and torch.all(hi[:, cin:] == 0) and torch.all(lo[pc:] == 0)


@pytest.mark.parametrize("tight,stored", [(True, 288.0), (False, 320.0)])
def test_op_costs_count_a_residual_that_is_the_input_once(tight, stored):
    """RFDB's c{j}_r adds its own input (rfdn_baseline/block.py:150-158) -- 100 B in + 100 B out + 50 B distilled per
    pixel at nf = 50 / dc = 25 in 16-bit storage, not 350; the stored figure carries the pad channels: pitch 64 / 32 = 320 B with whole K chunks,
    56 / 32 = 288 B at the tight pitch of round 6 (model.tight_pitch, the default)."""
    from ntire2022_esr_amd import RFDN
    from ntire2022_esr_amd.engine import Plan
    m = RFDN()
    m.set_compute("bf16")
    m.tight_pitch = tight
    plan = Plan(1, 64, 64, m._store())
    m._build_plan(plan, 3)
    costs = {c["name"]: c for c in m.op_costs(plan)}
    npx = 64 * 64
    c1r, c3r = costs["B1.c1_r"], costs["B1.c3_r"]
    w3, wp = 4.0 * 50 * 50 * 9, 4.0 * 50 * 25                # weight bytes: the 3x3's (both figures), the post 1x1's (stored figure only)
    assert abs((c1r["read_bytes"] + c1r["write_bytes"] - w3) / npx - 250.0) < 1e-6
    assert abs((c1r["stored_bytes"] - w3 - wp) / npx - stored) < 1e-6
    assert abs((c3r["read_bytes"] + c3r["write_bytes"] - 4.0 * 50 * 50 * 9) / npx - 200.0) < 1e-6
    for c in costs.values():
        assert c["stored_bytes"] >= (c["read_bytes"] + c["write_bytes"]) * 0.9999, c["name"]


def test_pack_tail_s16_fragment_order():
    """ABI v12 (csrc/esr_c64m.hip, rfdb_tail_kernel): esr_pack_tail_s16 lays RFDB's c5 (rfdn_baseline/block.py:156, 1x1 over
    cat(d1, d2, d3, r4)) out as 8 k steps x 2 output halves x (hi, lo) fragments of 1 KB + 64 fp32 biases.  Lane 32 h + i, element j of k step
    2 s + u holds slot 16 u + 8 h + j of segment s (the B operand is 16 bytes of the stored pixel); k steps 6, 7 hold channel
    8 (2 t + (j >> 2)) + 4 h + (j & 3) of the 3x3's result (two of its D blocks).  hi + lo = the fp32 weight to hi + lo accuracy, pads zero."""
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd.engine import pack_tail_s16
    g = torch.Generator().manual_seed(5)
    for mode, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        for nf, dc in ((50, 25), (64, 32), (49, 17), (33, 17)):       # (.., the lower end of both forms' ranges: RFDB's, ESDB's)
            w, b = torch.randn(nf, 4 * dc, generator=g) * 0.3, torch.randn(nf, generator=g)
            blob = pack_tail_s16(w, b, 3, dc, dc, mode)
            assert blob.numel() * 4 == 32 * 1024 + 256 == L.lib().esr_packed_tail_s16_bytes(3, dc, dc, nf)
            raw = blob.numpy().view(np.uint16)
            img = torch.from_numpy(raw[:32 * 512].astype(np.int16)).view(dt).float().reshape(8, 2, 2, 2, 32, 8)     # [ks][half][hi | lo][h][i][j]
            hi = torch.zeros(64, 4 * 32); lo = torch.zeros(64, 4 * 32)                                             # columns: 4 segments of 32 slots
            for ks in range(8):
                for h in range(2):
                    for j in range(8):
                        col = (ks // 2) * 32 + 16 * (ks & 1) + 8 * h + j if ks < 6 else 96 + 8 * (2 * (ks - 6) + (j >> 2)) + 4 * h + (j & 3)
                        hi[:, col] = img[ks, :, 0, h, :, j].reshape(64)
                        lo[:, col] = img[ks, :, 1, h, :, j].reshape(64)
            for sgm in range(4):
                wh = w[:, sgm * dc:(sgm + 1) * dc]
                assert torch.equal(hi[:nf, 32 * sgm:32 * sgm + dc], wh.to(dt).float())
                assert torch.equal(lo[:nf, 32 * sgm:32 * sgm + dc], (wh - wh.to(dt).float()).to(dt).float())
                assert torch.all(hi[:, 32 * sgm + dc:32 * sgm + 32] == 0) and torch.all(lo[:, 32 * sgm + dc:32 * sgm + 32] == 0)
            assert torch.all(hi[nf:] == 0) and torch.all(lo[nf:] == 0)
            bias = torch.from_numpy(blob.numpy()[32 * 256:].copy())
            assert torch.equal(bias[:nf], b) and torch.all(bias[nf:] == 0)
    assert L.lib().esr_packed_tail_s16_bytes(2, 25, 25, 50) == 0 and L.lib().esr_packed_tail_s16_bytes(3, 33, 25, 50) == 0
    assert L.lib().esr_packed_tail_s16_bytes(3, 25, 25, 65) == 0
    with pytest.raises(L.EsrError):
        pack_tail_s16(torch.zeros(50, 99), None, 3, 25, 25, "bf16")


def test_rfdn_plan_folds_the_block_tail_into_one_op():
    """in RFDN's 16-bit plans RFDB's c4 -> cat -> c5 -> esa.conv1 (rfdn_baseline/block.py:154-157, 76) is ONE op (c4 with a
    16-bit tail + post) when the launch fills the device; model.fuse_tail = False keeps c4 and c5 (+ conv1) as two ops.  Either way the cost
    model counts the same convolutions, and the fused op reads r3 + d1 .. d3 and writes v + c1_ -- r4 never reaches memory."""
    from ntire2022_esr_amd import RFDN
    from ntire2022_esr_amd.engine import Plan
    m = RFDN()
    m.set_compute("bf16")
    plans = {}
    for fuse in (True, False):
        m.fuse_tail = fuse
        plan = Plan(32, 256, 256, m._store())
        m._build_plan(plan, 3)
        plans[fuse] = {c["name"]: c for c in m.op_costs(plan)}
    fused, separate = plans[True], plans[False]
    assert "B1.c5" in separate and "B1.c5" not in fused and len(separate) == len(fused) + 4
    npx = 32 * 256 * 256
    c4 = fused["B1.c4"]
    w = 4.0 * (25 * 50 * 9 + 50 * 100)                       # (a post 1x1's weights: stored figure only, as for c1_r above)
    # 100 B of r3 + 3 x 50 B of d1 .. d3 in, 100 B of v + 24 B of c1_ (f = 12) out per pixel
    assert abs((c4["read_bytes"] + c4["write_bytes"] - w) / npx - (100 + 150 + 100 + 24)) < 1e-6
    assert abs(c4["flops"] - separate["B1.c4"]["flops"] - separate["B1.c5"]["flops"]) < 1.0
    assert abs(sum(c["flops"] for c in fused.values()) - sum(c["flops"] for c in separate.values())) < 1.0
    both = separate["B1.c4"]["read_bytes"] + separate["B1.c4"]["write_bytes"] + separate["B1.c5"]["read_bytes"] + separate["B1.c5"]["write_bytes"]
    assert abs((both - w) / npx - (100 + 50 + 50 + 150 + 100 + 24)) < 1e-6          # the two launches write r4 and read it back
    # one image of 64 x 64 does not fill the device: the plan keeps the two launches
    m.fuse_tail = True
    small = Plan(1, 64, 64, m._store())
    m._build_plan(small, 3)
    assert "B1.c5" in {c["name"] for c in m.op_costs(small)}


def test_isa_lint():
    """tools/lint_isa.py over EVERY translation unit of the library (cross-compiled to gfx950 assembly, cached under build/isa; about a
    minute, no GPU): (1) no packed-fp32 instruction with an op_sel that reads a high dword -- the gfx950 erratum behind round 3's
    overlapped-forward defect (LAB_NOTES.md); (2) tools/lint_s16_isa.py: no scratch access / VGPR spill in any conv_s16_kernel variant
    (its vmcnt arithmetic counts every vector-memory instruction) and no copy out of a register an in-flight residual load writes."""
    import subprocess, sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "lint_isa.py")],
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout + r.stderr


def test_isa_lint_flags_the_round3_apply_loop():
    """The lint catches the defect it was written for: esr_esa.hip with the round-3 group loop (a fetched group carried over the back
    edge, lx / ly travelling as a register pair, no esr_lone) compiles to `v_pk_mul_f32 ... op_sel:[0,1]` in every
    esa_apply_mfma_kernel instantiation -- the encoding that returned 0 in lanes 48..63 beside another kernel's MFMAs; the same loop
    WITH esr_lone() is clean."""
    import subprocess, sys, tempfile
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(repo, "tools"))
    sys.path.insert(0, os.path.join(repo, "tools", "dbg"))
    import lint_isa
    import race_dump
    d = tempfile.mkdtemp(prefix="esr_lint_old_")
    counts = {}
    for tag, exps in (("round3", ("nolone",)), ("fixed", ())):
        src, asm = os.path.join(d, f"esr_esa_{tag}.hip"), os.path.join(d, f"esr_esa_{tag}.s")
        open(src, "w").write(race_dump.patched("old", dump=False, exps=exps))
        subprocess.check_call([lint_isa.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(repo, "include"), "-I", lint_isa.CSRC,
                               "-S", "--cuda-device-only", src, "-o", asm], stderr=subprocess.DEVNULL)
        counts[tag] = [k for k, _ in lint_isa.lint_opsel(asm)]
    assert counts["round3"] and all("esa_apply_mfma_kernel" in k for k in counts["round3"]), counts["round3"][:3]
    assert len({k for k in counts["round3"]}) >= 10            # every instantiation (5 shapes x 2 storages)
    assert counts["fixed"] == []


def test_isa_lint_flags_sunk_patch_loads():
    """rule 3 of the lint catches what it was written for: esa_s2pool16_kernel WITHOUT the opaque use of its nine patch loads compiles to
    four loads sunk into the predicated LDS stores (load, vmcnt(0), store -- round 5, LAB_NOTES 10.8); the product source is clean."""
    import subprocess, sys, tempfile
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(repo, "tools"))
    import lint_isa
    src = open(os.path.join(lint_isa.CSRC, "esr_esa_lowres.hip")).read()
    start = src.index("    // (an opaque use of every piece")
    end = src.index("#pragma unroll", src.index("asm volatile(\"\" : \"+v\"(t));"))
    old = src[:start] + src[end:]
    assert "asm volatile(\"\" : \"+v\"(t))" not in old
    d = tempfile.mkdtemp(prefix="esr_lint_sunk_")
    res = {}
    for tag, text in (("sunk", old), ("product", src)):
        f, asm = os.path.join(d, f"lowres_{tag}.hip"), os.path.join(d, f"lowres_{tag}.s")
        open(f, "w").write(text)
        subprocess.check_call([lint_isa.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(repo, "include"), "-I", lint_isa.CSRC,
                               "-S", "--cuda-device-only", f, "-o", asm], stderr=subprocess.DEVNULL)
        res[tag] = lint_isa.lint_prologues(asm, "esr_esa_lowres.hip")
    assert len(res["sunk"]) == 2 and all("esa_s2pool16_kernel" in r for r in res["sunk"]), res["sunk"]          # both storage types
    assert res["product"] == []


def test_merged_bsconv_algebra_cpu():
    """BSRN._merged_bsconv (host arithmetic, no GPU): dense 3x3 with weights dw[c,tap] * pw[c,k] + interior bias + the 16-row border
    table == the reference's BSConvU (pointwise Linear -> depthwise 3x3 over the zero-padded pointwise OUTPUT, team18_bsrn.py:82-88),
    in fp64, on images as small as 1 pixel wide (all sides outside at once)."""
    import torch.nn.functional as F
    from ntire2022_esr_amd.bsrn import BSRN
    g = torch.Generator().manual_seed(3)
    for (cin, c, h, w) in ((12, 8, 9, 7), (6, 5, 1, 6), (4, 4, 5, 1), (3, 2, 1, 1)):
        pw = torch.nn.Linear(cin, c).double()
        dw = torch.nn.Conv2d(c, c, 3, padding=1, groups=c).double()
        x = torch.randn(2, cin, h, w, generator=g, dtype=torch.float64)
        with torch.no_grad():
            ref = dw(pw(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2))
        wm, bias, table = BSRN._merged_bsconv(pw, dw)
        # fp64 re-derivation of what the kernel computes: conv + bias + table[outside mask of the pixel]
        wd = dw.weight.detach().reshape(c, 1, 3, 3)
        w64 = wd * pw.weight.detach().reshape(c, cin, 1, 1)
        y = F.conv2d(x, w64, None, padding=1)
        bp, bd = pw.bias.detach(), dw.bias.detach()
        y = y + (bd + bp * wd.sum(dim=(1, 2, 3))).reshape(1, c, 1, 1)
        ys, xs = torch.arange(h), torch.arange(w)
        mask = ((xs == 0).long() | ((xs == w - 1).long() << 1)).reshape(1, w) | (((ys == 0).long() << 2) | ((ys == h - 1).long() << 3)).reshape(h, 1)
        tab64 = torch.zeros(16, c, dtype=torch.float64)
        for m in range(1, 16):
            out = torch.zeros(3, 3, dtype=torch.bool)
            if m & 1: out[:, 0] = True
            if m & 2: out[:, 2] = True
            if m & 4: out[0, :] = True
            if m & 8: out[2, :] = True
            tab64[m] = -bp * (wd.reshape(c, 3, 3) * out.double()).sum(dim=(1, 2))
        y = y + tab64[mask].permute(2, 0, 1).unsqueeze(0)
        assert float((y - ref).abs().max()) < 1e-12
        # and the fp32 tensors the engine packs are those quantities
        assert float((wm.double() - w64).abs().max()) < 1e-7 and float((table[:, :c].double() - tab64).abs().max()) < 1e-7
        assert float((bias.double() - (bd + bp * wd.sum(dim=(1, 2, 3)))).abs().max()) < 1e-7


def test_head_hi_lo_weights_cpu():
    """engine.pack_head_s16: [w_hi | w_hi | w_lo] against the input slots [x_hi | x_lo | x_hi] reproduces w * x up to the dropped
    lo x lo term (2^-16 relative for bf16, 2^-22 for fp16) -- checked on the unpacked blob, no GPU."""
    from ntire2022_esr_amd.engine import pack_head_s16, unpack_conv_s16
    g = torch.Generator().manual_seed(5)
    w = torch.randn(20, 3, 3, 3, generator=g) * 0.1
    b = torch.randn(20, generator=g)
    x = torch.rand(3, generator=g) * 255
    for compute, dt, rel in (("bf16", torch.bfloat16, 2.0 ** -15), ("f16", torch.float16, 2.0 ** -21)):
        weff, beff = unpack_conv_s16(pack_head_s16(w, b, compute), 9, 20, 3, compute, cin_phys=16)
        xh = x.to(dt).float()
        slots = torch.cat([xh, (x - xh).to(dt).float(), xh])                                   # what esr_pack_input_s16 writes
        got = (weff.double() * slots.double().reshape(1, 9, 1, 1)).sum(dim=1)                  # per tap, per output channel
        want = (w.double() * x.double().reshape(1, 3, 1, 1)).sum(dim=1)
        assert float((got - want).abs().max()) <= rel * float((w.abs().double() * x.double().reshape(1, 3, 1, 1)).sum(dim=1).max()) * 4
        assert torch.equal(beff, b)


def test_block_shape_query_cpu():
    """esr_conv_block_waves (host-only): which block shape a descriptor's launch takes -- fp32: 8-wave blocks for large 3x3s with
    >= 3 output tiles; 16-bit storage: 1 = conv48r_kernel (3x3 over 48 physical input channels, 2 or 3 output tiles, >= 256 tiles of
    16x32, no residual from HBM / post chain), else two 4-wave blocks per CU for the plain 48-channel 3x3 with >= 512 tiles of 16x16, else 8"""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()

    def waves(n, h, w, cin, cout, k=3, store="f32", **kw):
        d = L.ConvDesc()
        d.n, d.h, d.w, d.cin, d.cout, d.ksize = n, h, w, cin, cout, k
        d.in_layout = d.out_layout = L.NHWC
        d.storage = L.STORE[store]
        for key, v in kw.items():
            setattr(d, key, v)
        return lib.esr_conv_block_waves(ctypes.byref(d))

    assert waves(32, 256, 256, 64, 64) == 8 and waves(1, 64, 64, 64, 64) == 4 and waves(32, 256, 256, 48, 16) == 4
    assert waves(32, 256, 256, 48, 48, store="bf16") == 1 and waves(1, 339, 510, 46, 46, store="f16") == 1
    assert waves(32, 256, 256, 48, 24, store="bf16") == 1 and waves(2, 256, 256, 48, 48, store="f16") == 1     # two output tiles; exactly 256 tiles
    assert waves(1, 256, 256, 48, 48, store="bf16") == 8 and waves(32, 256, 256, 32, 48, store="bf16") == 4     # 128 tiles; two input chunks (the two-blocks-per-CU shape)
    assert waves(1, 128, 128, 48, 48, store="bf16") == 8                        # 64 tiles: fewer than resident blocks
    # round 4: the plain 64-channel 3x3 with 2 or 4 output tiles and >= 256 tiles of 16 x 16 takes conv64r_kernel (1); GELU, a split store,
    # three output tiles or fewer tiles stay on conv_s16_kernel's 8-wave block (74 KB of weights: one block per CU)
    assert waves(32, 256, 256, 64, 64, store="bf16") == 1 and waves(1, 339, 510, 50, 25, store="f16") == 1
    assert waves(32, 256, 256, 64, 64, store="bf16", act=L.ACT_GELU) == 8 and waves(32, 256, 256, 64, 64, store="bf16", split=16) == 8
    assert waves(32, 256, 256, 64, 48, store="bf16") == 8 and waves(1, 128, 128, 64, 64, store="bf16") == 8
    assert waves(32, 256, 256, 48, 48, store="bf16", hilo=L.HILO_OUT) == 8      # hi + lo pairs: conv_s16_kernel's HILO instantiation
    assert waves(32, 256, 256, 48, 48, k=1, store="bf16") == 8
    assert waves(32, 256, 256, 48, 48, store="bf16", res_mode=L.RES_POST_ACT) == 8          # residual from HBM
    assert waves(32, 256, 256, 48, 48, store="bf16", out_layout=L.NCHW_SHUFFLE4) == 8
    # RLFB's c3_r (residual from HBM, own result not stored, c5 -> esa.conv1 in the epilogue): conv48rp_kernel from 256 tiles of 16 x 16
    fake = lambda a: ctypes.c_void_p(a)
    c3r = dict(store="bf16", compute=L.COMPUTE["bf16"], res_mode=L.RES_POST_ACT, res=L.View(fake(0x1000), 48, 0), inp=L.View(fake(0x2000), 48, 0),
               post_wpacked=fake(0x3000), post2_wpacked=fake(0x4000), post_cout=46, post2_cout=16)
    assert waves(32, 256, 256, 48, 46, **c3r) == 1 and waves(1, 339, 510, 48, 46, **c3r) == 1 and waves(1, 128, 128, 48, 46, **c3r) == 8
    assert waves(1, 339, 510, 48, 46, out0=L.View(fake(0x5000), 48, 0), **c3r) == 8          # its own result stored too: conv_s16_kernel
    # a 3x3 whose stored result also feeds one post 1x1 of two output tiles: conv48rq_kernel (fp16 only) / conv64m_kernel (no GELU)
    q = dict(out0=L.View(fake(0x5000), 64, 0), post_wpacked=fake(0x3000), post_cout=32)
    assert waves(32, 256, 256, 48, 48, store="f16", **q) == 1 and waves(32, 256, 256, 48, 48, store="bf16", **q) == 8
    assert waves(32, 256, 256, 64, 64, store="bf16", **q) == 1 and waves(32, 256, 256, 64, 64, store="bf16", post_act=L.ACT_GELU, **q) == 8
    # ESDB's c{j}_r (border table + GELU + residual == input): conv64m_kernel from 256 tiles of 16 x 16, where conv48r_kernel needs 16 x 32
    esdb = dict(store="bf16", act=L.ACT_GELU, border_bias=fake(0x6000), res_mode=L.RES_PRE_ACT, inp=L.View(fake(0x2000), 48, 0),
                res=L.View(fake(0x2000), 48, 0))
    assert waves(1, 256, 256, 48, 48, **esdb) == 1 and waves(1, 256, 240, 48, 48, **esdb) == 8
    # the LR conv on hi + lo pairs (residual pair from HBM): conv48rp_kernel<bf16, LRS> / conv64m_kernel<.., HL>, which needs the residual
    lr = dict(store="bf16", hilo=L.HILO_RES | L.HILO_OUT, hilo_stride=1 << 20, res_mode=L.RES_PRE_ACT, res=L.View(fake(0x1000), 64, 0))
    assert waves(32, 256, 256, 48, 48, **lr) == 1 and waves(1, 128, 128, 48, 48, **lr) == 8
    assert waves(32, 256, 256, 64, 64, **lr) == 1 and waves(32, 256, 256, 64, 64, **dict(lr, res=L.View(None, 64, 0))) == 8
    # a single image's 48-channel hi + lo head (16 input slots): the two-blocks-per-CU shape; a batch stays on the 8-wave one
    assert waves(1, 339, 510, 3, 48, store="bf16", hilo=L.HILO_OUT) == 4 and waves(32, 256, 256, 3, 48, store="bf16", hilo=L.HILO_OUT) == 8
    # conv48rp_kernel's shape beyond the 16 x 16 tiles' magic-division range still reports that kernel (the launch takes conv_s16_kernel)
    assert waves(16, 256, 65536, 48, 46, **c3r) == 1
    assert lib.esr_conv_block_waves(None) == 0


def test_wino_packer_is_G_g_Gt_rounded_once():
    """esr_pack_wino_f32 (host C++): U = G g G^T in fp64, one rounding; lane order round-trips; pad slots are zero
    (Lavin & Gray F(2x2,3x3); replaces the OIHW weights of basicblock.conv, models/basicblock.py:61-65)."""
    import torch
    from ntire2022_esr_amd import engine
    g = torch.Generator().manual_seed(0)
    w = torch.randn(50, 40, 3, 3, generator=g)
    b = torch.randn(50, generator=g)
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
    U = torch.einsum('ia,ocab,jb->ocij', G, w.double(), G).float().reshape(50, 40, 16)
    blob = engine.pack_wino(w, b)
    u, bb = engine.unpack_wino(blob, 40, 50)
    assert torch.equal(u, U) and torch.equal(bb, b)
    # padded concat map: physical slots 10, 11, 22, 23 are padding
    cmap = list(range(10)) + [-1, -1] + list(range(10, 20)) + [-1, -1]
    w2 = torch.randn(32, 20, 3, 3, generator=g)
    blob2 = engine.pack_wino(w2, None, cin_map=cmap)
    u2, b2 = engine.unpack_wino(blob2, 20, 32, cin_map=cmap)
    U2 = torch.einsum('ia,ocab,jb->ocij', G, w2.double(), G).float().reshape(32, 20, 16)
    assert torch.equal(u2, U2) and float(b2.abs().max()) == 0.0
    # everything that is not a (slot, cout) of the logical tensor is zero: total mass matches
    assert abs(float(blob2.double().abs().sum()) - float(U2.double().abs().sum())) < 1e-6 * float(U2.double().abs().sum())


def test_chain_descriptor_validation_and_rlfn_plan_without_gpu():
    """esr_conv_chain_s16 (ABI v11) validates before it launches; RLFN's 16-bit plans hold one chain op per RLFB whose sub-ops keep the
    complexity counters of the reference's five convolutions; fp32 plans and fuse_chain = False keep separate ops; graphs: argument checks."""
    import torch
    from ntire2022_esr_amd import RLFN_cut, _lib as L
    from ntire2022_esr_amd.engine import Plan
    from ntire2022_esr_amd.summary import model_complexity
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)

    def desc(**kw):
        d = L.ChainDesc()
        d.n, d.h, d.w, d.n_layers, d.cin, d.cmid, d.cout = 1, 32, 40, 3, 46, 48, 46
        d.act, d.slope, d.res_mode = L.ACT_LRELU, 0.05, L.RES_POST_ACT
        d.storage = d.compute = L.STORE["bf16"]
        d.inp, d.post_out, d.post2_out = L.View(a, 48, 0), L.View(a, 48, 0), L.View(a, 16, 0)
        for i in range(3):
            d.wpacked[i] = a
        d.post_wpacked, d.post2_wpacked, d.post_cout, d.post2_cout = a, a, 46, 16
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert lib.esr_conv_chain_supported(ctypes.byref(desc())) == 1
    assert lib.esr_conv_chain_supported(ctypes.byref(desc(storage=0, compute=0))) == 0            # 16-bit storage only
    assert lib.esr_conv_chain_supported(ctypes.byref(desc(n_layers=2))) == 0
    assert lib.esr_conv_chain_supported(ctypes.byref(desc(cmid=64))) == 0                          # three K chunks per layer
    assert lib.esr_conv_chain_supported(ctypes.byref(desc(res_mode=L.RES_PRE_ACT))) == 0
    assert lib.esr_conv_chain_supported(ctypes.byref(desc(act=L.ACT_GELU))) == 0
    assert lib.esr_conv_chain_supported(ctypes.byref(desc(post2_cout=24))) == 0
    assert lib.esr_conv_chain_s16(None, None) == -1
    assert lib.esr_conv_chain_s16(ctypes.byref(desc(post_out=L.View(None, 48, 0))), None) == -1     # null output
    assert lib.esr_conv_chain_s16(ctypes.byref(desc(cmid=64)), None) == -2
    assert lib.esr_conv_chain_s16(ctypes.byref(desc(inp=L.View(a, 48, 8))), None) == -1            # the 48 channels would leave the pixel
    assert lib.esr_graph_create(None, 0, None, None, None) == -1 and lib.esr_graph_launch(None, None, None, None) == -1
    assert lib.esr_graph_nodes(None) == 0
    lib.esr_graph_destroy(None)

    m = RLFN_cut()
    ref = model_complexity(m, (3, 64, 64))
    for store, fuse, nchain in (("bf16", True, 4), ("f16", True, 4), ("bf16", False, 0), ("f32", True, 0)):
        m.fuse_chain = fuse
        plan = Plan(1, 64, 64, store)
        m._build_plan(plan, 3)
        assert sum(o.kind == "chain" for o in plan.ops) == nchain, (store, fuse)
        for o in plan.ops:
            if o.kind == "chain":
                assert [s.w.split(".")[-1] for s in o.replaces] == ["c1_r", "c2_r", "c3_r"] and o.replaces[-1].post.post2 is not None
        terms = [m._complexity_terms(plan, o) for o in plan.ops]
        flops, acts, nconv = (sum(t[i] for t in terms) for i in range(3))
        assert (float(flops), float(acts), int(nconv)) == (ref["flops"], ref["activations"], ref["num_conv"]), (store, fuse)
    m.fuse_chain = True
    m.set_compute("bf16")._repack("cpu")              # the chain's convs and 1x1s get their 16-bit blobs
    assert {"B1.c1_r#s16", "B2.c2_r#s16", "B4.c3_r#s16"} <= set(m._packed)
    assert {"B1.c5#post", "B3.esa.conv1#post"} <= set(m._packed)
    m.set_compute("f32")
