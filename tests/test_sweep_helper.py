"""CPU: tests/_sweep.py is what tests/test_gpu_value_sweep.py takes it for -- the sweeps are complete, the tie pairs are ties, the 0 / 1
weights survive every packer unchanged, the emulated polynomial has the bound the sweep grants it, the comparators reject a store or an
activation that is subtly wrong -- and every __global__ kernel of csrc/ is either swept or exempt for a stated reason."""
import re

import numpy as np
import pytest
import torch

import _sweep as S

STORES = ["bf16", "f16"]


@pytest.mark.parametrize("store", STORES)
def test_all_finite_is_every_finite_pattern(store):
    dt = S.DTYPES[store]
    sw = S.all_finite(dt)
    assert sw.dtype == dt and sw.numel() == S.N_FINITE[dt]
    bits = S.to_bits(sw)
    assert torch.unique(bits).numel() == sw.numel() and bool(torch.isfinite(sw.float()).all())
    assert {0x0000, 0x8000, 0x0001, 0x8001} <= set(bits.tolist())                       # +-0 and the smallest subnormals
    assert float(sw.float().max()) == torch.finfo(dt).max and float(sw.float().min()) == -torch.finfo(dt).max
    # the identity route's exemption is the subnormal inputs and nothing else
    assert S.assert_exempt_share(sw) == S.N_SUBNORMAL[dt]
    m = S.flush_mask(sw)
    assert float(sw[m].float().abs().max()) < 2.0 ** S.EMIN[dt] and float(sw[m].float().abs().min()) > 0
    assert float(sw[~m & (sw.float() != 0)].float().abs().min()) == 2.0 ** S.EMIN[dt]
    p = S.permuted(sw)
    assert torch.equal(torch.sort(S.to_bits(p)).values, torch.sort(bits).values) and not torch.equal(p, sw)


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("shape,channels", [((1, 32, 32, 64), None), ((2, 23, 37, 48), None), ((2, 23, 37, 48), 46), ((1, 256, 256, 48), None)])
def test_tile_holds_every_value_at_changing_positions(store, shape, channels):
    sw = S.all_finite(S.DTYPES[store])
    t = S.tile(sw, shape, channels)
    cl = shape[3] if channels is None else channels
    assert tuple(t.shape) == shape and t.dtype == sw.dtype
    assert torch.unique(S.to_bits(t[..., :cl])).numel() == sw.numel()
    assert cl == shape[3] or float(t[..., cl:].float().abs().max()) == 0.0
    # the second row starts ROW_OFFSET values before the end of the first
    row0, row1 = t[0, 0, :, :cl].reshape(-1), t[0, 1, :, :cl].reshape(-1)
    assert torch.equal(S.to_bits(row0[-S.ROW_OFFSET:]), S.to_bits(row1[:S.ROW_OFFSET]))
    if t[..., :cl].numel() >= 3 * sw.numel():                                            # a repeated sweep: one value, several channel positions
        pos = (S.to_bits(t[..., :cl]).reshape(-1) == int(S.to_bits(sw[1000:1001])[0])).nonzero().reshape(-1)
        assert len({int(v) % cl for v in pos}) >= 3, pos[:8]
    with pytest.raises(AssertionError):
        S.tile(sw, (1, 8, 8, 16))                                                        # too small for one sweep


@pytest.mark.parametrize("channels", [16, 32, 48, 64])
def test_shape_for_holds_one_sweep_and_is_ragged(channels):
    for dt in S.DTYPES.values():
        sw = S.all_finite(dt)
        n, h, w = S.shape_for(sw, channels)
        assert h % 16 and w % 16 and n * h * w * channels < 2.2 * sw.numel()
        S.tile(sw, (n, h, w, channels))


@pytest.mark.parametrize("store", STORES)
def test_tie_pairs_are_ties(store):
    dt = S.DTYPES[store]
    x, r, info = S.tie_pairs(dt)
    print(f"tie pairs {store}: {info}")
    assert x.dtype == dt and r.dtype == dt and x.shape == r.shape
    assert info["even_below"] >= 30000 and info["even_above"] >= 30000
    s = x.double() + r.double()
    assert bool((s.float().double() == s).all())                                         # exact in fp32
    # the wanted result is one of the two neighbours of the exact sum
    want = (x.float() + r.float()).to(dt)
    lo, hi = S.neighbours(s, dt)
    assert bool(((want.double() == lo.double()) | (want.double() == hi.double())).all())
    if dt == torch.float16:
        top = (x.float().abs() == 65504.0) & (r.float().abs() == 16.0) & (torch.sign(x.float()) == torch.sign(r.float()))
        assert int(top.sum()) == 2 and bool(torch.isinf(want[top].float()).all())        # the tie at the top of the range: torch says Inf


@pytest.mark.parametrize("store", STORES)
def test_conv_packer_leaves_0_and_1_untouched(store):
    """esr_pack_conv_s16 (error diffusion over the 3x3 taps, hi + lo for 1x1): unpack(pack(w)) == w for zero, identity and selection weights"""
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    for cout, cin, k in [(48, 48, 3), (64, 64, 3), (46, 48, 3), (24, 48, 3), (32, 16, 3), (32, 32, 3), (16, 32, 1), (50, 25, 1), (25, 50, 1), (64, 64, 1),
                         (256, 64, 1), (64, 256, 1)]:
        for make in (S.zero_weight, S.identity_weight):
            w = make(cout, cin, k)
            for cp in {cin, (cin + 15) // 16 * 16}:
                blob = pack_conv_s16(w, torch.zeros(cout), store, cin_phys=cp)
                we, b = unpack_conv_s16(blob, cin, cout, k, store, cin_phys=cp)
                assert torch.equal(we, w) and float(b.abs().max()) == 0.0, (store, cout, cin, k, cp)


@pytest.mark.parametrize("store", STORES)
def test_post_tail_and_apply_packers_leave_0_and_1_untouched(store):
    """esr_pack_post_s16, esr_pack_tail_s16 and esr_pack_apply_post have no unpacking entry point: their blobs are read as 16-bit words,
    which must all be 0 or 1.0 (hi images of the ones, empty lo images, zero biases)"""
    from ntire2022_esr_amd.engine import pack_apply_post, pack_post_s16, pack_tail_s16
    dt = S.DTYPES[store]
    for cout, cin in [(46, 46), (16, 46), (25, 50), (24, 48), (16, 64), (48, 48), (1, 33)]:
        w = S.selection(cout, cin)
        S.assert_blob_is_0_1(pack_post_s16(w, torch.zeros(cout), store), dt, int(w.sum()), ("post", cout, cin))
        assert int(S.to_bits(S.blob_words(pack_post_s16(torch.zeros(cout, cin), None, store), dt)).max()) == 0
    for nf, dc in [(50, 25), (64, 32), (48, 24), (33, 17)]:
        w = S.selection(nf, 4 * dc)
        S.assert_blob_is_0_1(pack_tail_s16(w, torch.zeros(nf), 3, dc, dc, store), dt, int(w.sum()), ("tail", nf, dc))
    for cin, c0, c1 in [(50, 50, 0), (48, 48, 16), (64, 32, 0), (50, 25, 0), (46, 46, 16)]:
        w0 = S.selection(c0, cin)
        w1 = S.selection(c1, c0) if c1 else None
        blob = pack_apply_post(w0, torch.zeros(c0), w1, None if w1 is None else torch.zeros(c1), store)
        S.assert_blob_is_0_1(blob, dt, [int(w0.sum())] + ([int(w1.sum())] if c1 else []), ("apply", cin, c0, c1))
    with pytest.raises(AssertionError):                                                  # the check can fail: 0.3 has a low part
        S.assert_blob_is_0_1(pack_post_s16(S.selection(16, 46) * 0.3, torch.zeros(16), store), dt, 16, "0.3")


def test_gelu16_cpu_bound_pieces():
    """B(v) = |gelu16 - GELU| from the emulation over every finite bf16 and f16 value.  Printed (this run: 2.127e-04 on v < -4, 8.598e-05 on
    [-4, 4], 5.322e-05 v on v > 4); the last two are held to the documented 1.3e-4 and 5.3e-5 v -- the slope to the two digits the
    documents gave it: 5.3225e-5 is what they rounded, so B(v) takes 5.33e-5 --, the first is the figure the documents now carry where
    they said 1.3e-4 for every x <= 4."""
    below, mid, slope = S.gelu16_error_pieces([S.all_finite(dt) for dt in S.DTYPES.values()])
    print(f"gelu16_cpu: max|gelu16 - GELU| = {below:.4e} on v < -4, {mid:.4e} on [-4, 4], {slope:.4e} * v on v > 4")
    assert mid <= S.GELU16_BOUND_MID == 1.3e-4
    assert float(f"{slope:.1e}") == S.GELU16_DOC_SLOPE == 5.3e-5 and slope <= S.GELU16_BOUND_SLOPE == 5.33e-5
    assert 2.12e-4 < below <= S.GELU16_BOUND_BELOW == 2.13e-4
    # below -4 the function is one constant
    for dt in S.DTYPES.values():
        sw = S.all_finite(dt)
        tail = S.gelu16_cpu(sw[sw.float() < -4])
        assert float(tail.min()) == float(tail.max()) == pytest.approx(-2.127e-4, rel=1e-3)
    v = torch.tensor([-1e30, -5.0, -4.0, 0.0, 4.0, 100.0])
    assert S.gelu16_bound(v).tolist() == [2.13e-4, 2.13e-4, 1.3e-4, 1.3e-4, 1.3e-4, pytest.approx(5.33e-3)]


def test_fma_emulation_rounds_once():
    a, c = np.float32(1.0 + 2.0 ** -12), np.float32(-(1.0 + 2.0 ** -11))
    assert float(np.float32(a * a) + c) == 0.0                                           # a * a = 1 + 2^-11 + 2^-24 loses its last bit in fp32
    assert float(S._fma32(np.array([a]), np.array([a]), np.array([c]))[0]) == 2.0 ** -24


# ---- the comparators can fail --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_exact_rejects_wrong_stores(store):
    dt = S.DTYPES[store]
    x, r, _ = S.tie_pairs(dt)
    s = x.float() + r.float()
    want = s.to(dt)
    S.exact(S.store_rne(s, dt), want, dt, v=s)
    for wrong in (S.store_ties_away, S.store_truncate):
        with pytest.raises(S.Mismatch):
            S.exact(wrong(s, dt), want, dt, v=s, what=wrong.__name__)
    # +0 equals -0, an Inf must be where it is wanted, a NaN never passes, and the flush exemption covers a zero only where it is granted
    z = torch.tensor([0.0, -0.0, 1.0]).to(dt)
    S.exact(z, torch.tensor([-0.0, 0.0, 1.0]).to(dt), dt)
    inf = torch.tensor([float("inf"), 1.0]).to(dt)
    S.exact(inf, inf.clone(), dt)
    for got, want in ((inf, torch.tensor([torch.finfo(dt).max, 1.0]).to(dt)), (-inf, inf), (torch.tensor([float("nan"), 1.0]).to(dt), inf)):
        with pytest.raises(S.Mismatch):
            S.exact(got, want, dt)
    sub = torch.tensor([2.0 ** (S.EMIN[dt] - 2), 1.0]).to(dt)
    flushed = torch.where(S.flush_mask(sub), torch.zeros_like(sub), sub)
    assert S.exact(torch.tensor([0.0, 1.0]).to(dt), sub, dt, flushed=flushed) == 1
    assert S.exact(sub.clone(), sub, dt, flushed=flushed) == 0
    with pytest.raises(S.Mismatch):
        S.exact(torch.tensor([0.0, 0.0]).to(dt), sub, dt, flushed=flushed)                 # a normal input that came out as zero
    with pytest.raises(S.Mismatch):
        S.exact(torch.tensor([0.0, 1.0]).to(dt), sub, dt)                                  # no exemption on the residual route


@pytest.mark.parametrize("store", STORES)
def test_gelu_checks_reject_a_drifted_copy(store):
    """The two GELU assertions of the sweep on emulated outputs: a copy whose last coefficient is one fp32 step off and a copy that clamps
    at +-3.9 differ from the anchor's bits (`exact` rejects them) although both stay inside B(v) + half a step, which is why the sweep
    compares the copies bit for bit; a typo in a coefficient's seventh digit leaves B(v) as well.  The tenth printed digit of every
    coefficient is below fp32 resolution: changing it changes nothing, and is no drift."""
    dt = S.DTYPES[store]
    sw = S.all_finite(dt)
    anchor = S.gelu16_cpu(sw).to(dt)
    ref = S.gelu_f64(sw)
    tol = S.gelu16_bound(sw) + S.store_tol(ref, dt)
    worst, share = S.within(anchor, ref, tol, v=sw)
    print(f"gelu16_cpu {store}: max|stored - GELU| = {worst:.3e}, {share:.3f} of B(v) + half a step x 1.01")
    S.exact(S.gelu16_cpu(sw).to(dt), anchor, dt, v=sw)
    for i, c in enumerate(S.GELU16_COEFFS):
        text = f"{c:.9e}"
        mant, exp = text.split("e")
        typo = float(mant[:-1] + str((int(mant[-1]) + 1) % 10) + "e" + exp)
        assert np.float32(typo) == np.float32(c), (i, text)
    ulp = list(S.GELU16_COEFFS)
    ulp[7] = float(np.nextafter(np.float32(ulp[7]), np.float32(1.0)))
    seventh = list(S.GELU16_COEFFS)
    seventh[6] = -6.617547882e-02                                                        # -6.617537882e-02 with one digit mistyped
    for name, out, leaves_bound in (("one fp32 step in a coefficient", S.gelu16_cpu(sw, coeffs=ulp), False),
                                    ("clamp at 3.9", S.gelu16_cpu(sw, clamp=3.9), False),
                                    ("seventh digit of a coefficient", S.gelu16_cpu(sw, coeffs=seventh), True)):
        with pytest.raises(S.Mismatch):
            S.exact(out.to(dt), anchor, dt, v=sw, what=name)
        if leaves_bound:
            with pytest.raises(S.Mismatch):
                S.within(out.to(dt), ref, tol, v=sw, what=name)


@pytest.mark.parametrize("store", STORES)
def test_within_rejects_an_fp16_tanh_sigmoid(store):
    """the gate's tolerance (half a step x 1.01 of |ref| + the smallest fp32 normal x |r|) passes 1 / (1 + expf(-v)) in fp32 and rejects
    0.5 (1 + tanh(v / 2)) evaluated in fp16, with r = 1 and with r = the permuted sweep"""
    dt = S.DTYPES[store]
    sw = S.all_finite(dt)
    v = sw.double()
    for r in (torch.ones_like(sw), S.permuted(sw)):
        ref = S.sigmoid_f64(v) * r.double()
        tol = S.store_tol(ref, dt) + S.F32_MIN_NORMAL * r.double().abs()
        good = ((1.0 / (1.0 + torch.exp(-sw.float()))) * r.float()).to(dt)
        S.within(good, ref, tol, v=sw)
        with pytest.raises(S.Mismatch):
            S.within((S.sigmoid_tanh_f16(sw) * r.float()).to(dt), ref, tol, v=sw, what="fp16 tanh sigmoid")
    with pytest.raises(S.Mismatch):
        S.within(torch.tensor([float("nan")]), torch.tensor([0.0]), torch.tensor([1.0]))


# ---- closure: every kernel is swept or exempt -----------------------------------------------------------------------------------------------
def test_every_kernel_is_swept_or_exempt():
    """the __global__ kernels of csrc/ (parsed as tests/test_kernel_names.py parses them) against test_gpu_value_sweep.SWEPT and .EXEMPT: a
    kernel added without a sweep case fails here, on the CPU"""
    import glob
    import importlib
    import os
    import test_gpu_value_sweep as V
    from test_kernel_names import _sources
    # the newer sweeps live in files of their own and enter themselves into V.SWEPT when imported: a run of this file alone imports them here
    for path in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_sweep_*.py"))):
        importlib.import_module(os.path.basename(path)[:-3])
    tmpl = re.compile(r"__global__\s+(?:__launch_bounds__\s*\((?:[^()]|\([^()]*\))*\)\s*)?void\s+(\w+)\s*\(")
    kernels = {m.group(1) for _, text in _sources(strip=True) for m in tmpl.finditer(text)}
    assert len(kernels) >= 35, sorted(kernels)
    assert not set(V.SWEPT) & set(V.EXEMPT)
    missing = kernels - set(V.SWEPT) - set(V.EXEMPT)
    assert not missing, f"no value sweep and no exemption for {sorted(missing)}"
    gone = (set(V.SWEPT) | set(V.EXEMPT)) - kernels
    assert not gone, f"listed, but not a kernel of csrc/: {sorted(gone)}"
    for k, tests in V.SWEPT.items():
        assert tests and all(callable(getattr(V, t, None)) and t.startswith("test_") for t in tests), (k, tests)
    for k, why in V.EXEMPT.items():
        assert isinstance(why, str) and len(why) > 20 and "\n" not in why, k
    # only kernels that store nothing through an activation function or a 16-bit rounding may be exempt
    allowed = re.compile(r"^(ca_reduce_|esa_pool7|esa_s2pool|esa_chain_|conv3x3s2_|maxpool7s3_|ssim_|sqerr_|tensor2uint|bw_probe_|event_probe_|imdb_tail_|wino8_f32_)")
    assert all(allowed.match(k) for k in V.EXEMPT), sorted(k for k in V.EXEMPT if not allowed.match(k))
