"""CPU: ResDN (NTIRE 2022 ESR team 43, models.team43_resdn.ResDN) on the engine -- checkpoint surface and refusals, the slope blob read back,
the block as the plan runs it restated in fp64 against the plain block, the mean-shift fold, complexity counters in every storage, plan
shape, esr_prelu's validation without a GPU, and the shim and registry paths."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import _resdn as R
import _sweep as S
from conftest import GOLD, REPO

SHIM = os.path.join(REPO, "shim")
NAME = "team43_resdn"
CKPT = os.path.join(GOLD, NAME + ".safetensors")
WANT = {"activations": 155353536.0, "num_conv": 67, "flops": 25245922144.0, "num_parameters": 406504}
STORES = ["f32", "bf16", "f16"]


def _true_sd():
    from safetensors.torch import load_file
    sd = load_file(os.path.join(GOLD, NAME + "_f32.safetensors"))
    sd.update(load_file(os.path.join(GOLD, NAME + "_f32.part2.safetensors")))
    return sd


def _resdn(store="f32", fuse=False):
    from safetensors.torch import load_file
    from ntire2022_esr_amd import ResDN
    m = ResDN()
    m.load_state_dict(load_file(CKPT), strict=True)
    m.set_compute(store)
    m.fuse_resdb = fuse
    return m


def _plan(m, n, h, w):
    from ntire2022_esr_amd.engine import Plan
    plan = Plan(n, h, w, m._store())
    m._build_plan(plan, 3)
    return plan


# ---- loading and refusals -----------------------------------------------------------------------------------------------------------------
def test_checkpoint_loads_strict_with_the_reference_parameter_count():
    from safetensors.torch import load_file
    sd = load_file(CKPT)
    m = _resdn()
    assert len(sd) == 162 and set(m.state_dict()) == set(sd)
    assert sum(p.numel() for p in m.parameters()) == 406504
    assert all(tuple(m.state_dict()[k].shape) == tuple(v.shape) for k, v in sd.items())
    assert tuple(sd["body_unit1.expansion1.0.weight"].shape) == (48,) and tuple(sd["body_unit1.expansion1.1.weight"].shape) == (96, 48, 1, 1)
    assert tuple(sd["body_unit2.expansion3.0.weight"].shape) == (80,) and tuple(sd["body_unit2.expansion3.1.weight"].shape) == (64, 80, 1, 1)
    assert tuple(sd["body_unit3.conv_tail.0.weight"].shape) == (96,) and tuple(sd["body_unit3.compression2.1.weight"].shape) == (48, 48, 3, 3)
    assert tuple(sd["body_unit4.attention.conv_max.weight"].shape) == (12, 12, 3, 3) and tuple(sd["T_tdm2.0.weight"].shape) == (24, 48, 1, 1)
    assert tuple(sd["tail.1.weight"].shape) == (48, 48, 3, 3) and tuple(sd["sub_mean.weight"].shape) == (3, 3, 1, 1)
    # the unrounded checkpoint: the same keys, fp32, 1.55 MiB in two files under the file size limit; the fixture is its RNE rounding to bf16
    parts = [os.path.join(GOLD, NAME + sfx) for sfx in ("_f32.safetensors", "_f32.part2.safetensors")]
    assert all(os.path.getsize(p) <= 1 << 20 for p in parts) and sum(os.path.getsize(p) for p in parts) > 1 << 20
    assert all(os.path.getsize(os.path.join(GOLD, f)) <= 1 << 20 for f in os.listdir(GOLD) if NAME in f)
    assert not set(load_file(parts[0])) & set(load_file(parts[1]))
    true = _true_sd()
    assert set(true) == set(sd) and all(v.dtype == torch.float32 for v in true.values())
    assert all(torch.equal(true[k].to(torch.bfloat16).view(torch.int16), sd[k].view(torch.int16)) for k in sd)
    m.load_state_dict(true, strict=True)
    # what the issue states about the checkpoint: the mean shifts are pure shifts, the body's slopes leave [0, 1] on both sides
    eye = torch.eye(3).view(3, 3, 1, 1)
    assert torch.equal(true["sub_mean.weight"], eye) and torch.equal(true["add_mean.weight"], eye)
    a = torch.cat([v for k, v in true.items() if k.startswith("body_unit") and v.dim() == 1 and k.endswith(".0.weight")])
    assert a.numel() == 1728 and int((a < 0).sum()) == 352 and int((a > 1).sum()) == 89
    assert R.SLOPE_RANGE == (round(float(a.min()), 2), round(float(a.max()), 2))


def test_unsupported_constructor_arguments_are_refused():
    from ntire2022_esr_amd import ResDN
    for kw in (dict(upscale_factor=2), dict(upscale_factor=3), dict(in_channels=1), dict(in_channels=4), dict(n_feats=32), dict(n_feats=64),
               dict(out_channels=1), dict(out_channels=4)):
        with pytest.raises(NotImplementedError):
            ResDN(**kw)
    ResDN(upscale_factor=4, in_channels=3, n_feats=48, out_channels=3)


@pytest.mark.parametrize("store", STORES)
def test_inputs_below_15_pixels_are_refused_with_the_reason(store):
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd.engine import Plan
    m = _resdn(store)
    for h, w in ((14, 40), (40, 14)):
        with pytest.raises(L.EsrError, match="H, W >= 15"):
            _plan(m, 1, h, w)
    _plan(m, 1, 15, 15)
    with pytest.raises(L.EsrError, match="3 input channels"):
        m._build_plan(Plan(1, 20, 20, store), 4)


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("which", ["sub_mean", "add_mean"])
def test_a_mean_shift_that_is_not_a_pure_shift_is_refused_with_the_reason(store, which):
    """the plan folds both MeanShifts into biases: only the identity weight allows that.  Their biases are free."""
    from ntire2022_esr_amd import _lib as L
    m = _resdn(store)
    with torch.no_grad():
        m._leaf("sub_mean").bias.copy_(torch.tensor([-0.5, 0.25, 0.125]))
        m._leaf("add_mean").bias.copy_(torch.tensor([0.5, -0.25, 2.0]))
    m._repack("cpu")
    with torch.no_grad():
        m._leaf(which).weight[1, 1, 0, 0] = 0.5                               # rgb_std != 1
    with pytest.raises(L.EsrError, match=which + r"\.weight is not the 3x3 identity"):
        m._repack("cpu")
    with torch.no_grad():
        m._leaf(which).weight[1, 1, 0, 0] = 1.0
        m._leaf(which).weight[0, 2, 0, 0] = 1e-3                              # a colour mix
    with pytest.raises(L.EsrError, match="identity"):
        m._repack("cpu")


# ---- blobs ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 5, 48, 64, 80, 96, 512])
def test_prelu_blob_round_trip(c):
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd.engine import pack_prelu, unpack_prelu
    a = R.random_slopes(c, c)
    blob = pack_prelu(a)
    assert blob.dtype == torch.float32 and blob.numel() * 4 == L.lib().esr_packed_prelu_bytes(c) == (c + 7) // 8 * 8 * 4
    assert torch.equal(blob[:c], a) and bool((blob[c:] == 0).all())          # fp32 slopes as they are, zeros behind them
    assert torch.equal(unpack_prelu(blob, c), a)
    assert L.lib().esr_packed_prelu_bytes(0) == 0 and L.lib().esr_packed_prelu_bytes(513) == 0


@pytest.mark.parametrize("store", STORES)
def test_the_model_packs_the_checkpoints_slopes_and_the_split_expansions(store):
    from ntire2022_esr_amd.engine import unpack_conv, unpack_conv_s16, unpack_prelu
    m = _resdn(store)
    m._repack("cpu")
    sd = m.state_dict()
    n = 0
    for k in range(1, 5):
        b = f"body_unit{k}."
        for name, c in [(f"expansion{j}.0", 48 + 16 * (j - 1)) for j in (1, 2, 3)] + [(f"compression{j}.0", 48) for j in (1, 2, 3)] + [("conv_tail.0", 96)]:
            assert torch.equal(unpack_prelu(m._packed[b + name + "#prelu"], c), sd[b + name + ".weight"])          # never rounded
            n += c
        for j in (1, 2, 3):
            cin, w, bias = 48 + 16 * (j - 1), sd[b + f"expansion{j}.1.weight"], sd[b + f"expansion{j}.1.bias"]
            for sfx, sl in (("#res", slice(0, 48)), ("#dist", slice(48, None))):
                got_w, got_b = unpack_conv(m._packed[b + f"expansion{j}.1" + sfx], cin, w[sl].shape[0], 1)
                assert torch.equal(got_w, w[sl]) and torch.equal(got_b, bias[sl])
                if store != "f32":
                    w16, b16 = unpack_conv_s16(m._packed[b + f"expansion{j}.1" + sfx + "#s16"], cin, w[sl].shape[0], 1, store)
                    assert float((w16 - w[sl]).abs().max()) <= 2.0 ** -14 * float(w[sl].abs().max()) and torch.equal(b16, bias[sl])
    assert n == 1728
    # add_mean in tail.1's bias: colour c of the shuffled output is channels 16 c .. 16 c + 15
    unpack = (lambda blob: unpack_conv(blob, 48, 48, 3)) if store == "f32" else (lambda blob: unpack_conv_s16(blob, 48, 48, 3, store))
    _, bt = unpack(m._packed["tail.1" if store == "f32" else "tail.1#s16"])
    assert torch.equal(bt, sd["tail.1.bias"] + sd["add_mean.bias"].repeat_interleave(16))


# ---- the fp64 restatements --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4])
def test_the_block_as_the_plan_runs_it_equals_the_plain_block(k):
    """tests/_resdn.py: the per-layer form -- the PReLU launch gathers the concat, every expansion 1x1 in two parts, the distilled maps raw in
    one buffer that starts as NaN -- against the block as team43_resdn.py:90-108 writes it, both in fp64 with the unrounded checkpoint, at
    5 x 7 (every pixel but three is a border pixel of the 3x3s)"""
    sd = _true_sd()
    x = torch.randn(2, 48, 5, 7, generator=torch.Generator().manual_seed(k), dtype=torch.float64)
    plain, split = R.resdb_f64(sd, f"body_unit{k}.", x), R.resdb_split_f64(sd, f"body_unit{k}.", x)
    for a, b in zip(plain, split):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))


def test_the_restatement_is_torchs_prelu():
    x = torch.randn(3, 96, 4, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    a = R.random_slopes(96, 1).double()
    want = torch.nn.functional.prelu(x, a)
    assert torch.equal(R.prelu_f64(x.permute(0, 2, 3, 1), a).permute(0, 3, 1, 2), want)
    assert torch.equal(R._nchw_prelu(x, a), want)
    neg = (x < 0).permute(0, 2, 3, 1)
    wrong = R.prelu_max_f64(x.permute(0, 2, 3, 1), a)
    right = R.prelu_f64(x.permute(0, 2, 3, 1), a)
    big, small = a > 1, a <= 1
    assert bool((wrong != right)[..., big].all()) and bool((wrong == right)[..., small].all())      # max(v, a v) is PReLU for a <= 1 only
    assert bool(neg.any())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_store_once_rounds_once(dt):
    """the single rounding esr_prelu is held to: to nearest, ties to even, on values where fp64 -> fp32 -> 16-bit would round twice"""
    step = 2.0 ** -S.MBITS[dt]
    s = torch.tensor([1.0 + step / 2 + 2.0 ** -30, 1.0 + step / 2, 1.0 + 3 * step / 2, -(1.0 + step / 2 + 2.0 ** -30), float(torch.finfo(dt).max) * (1 + step / 4),
                      float(torch.finfo(dt).max) * (1 + step / 2)], dtype=torch.float64)
    got = R.store_once(s, dt).double()
    top = float(torch.finfo(dt).max)
    assert got.tolist() == [1.0 + step, 1.0, 1.0 + 2 * step, -(1.0 + step), top, float("inf")]
    assert float(s[0].float().to(dt)) == 1.0                                  # what two roundings give for the first value
    x = S.all_finite(dt)
    a = torch.full((x.numel(),), 0.3)
    y = R.prelu_stored(x, a)
    keep = x.float() >= 0
    assert torch.equal(S.to_bits(y)[keep], S.to_bits(x)[keep])
    err = (y.double() - float(torch.tensor(0.3)) * x.double()).abs()[~keep]                # the fp32 slope times x, exact in fp64
    assert bool((err <= S.half_step(y.double(), dt)[~keep] * 1.0000001).all())


def test_the_bias_folded_head_is_wrong_on_the_border_only():
    from safetensors.torch import load_file
    sd = {k: v.float() for k, v in load_file(CKPT).items()}
    x = torch.rand(1, 3, 15, 15, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    ref, folded = R.head_f64(sd, x), R.head_f64(sd, x, folded=True)
    miss = (ref - folded).abs()
    assert float(miss[..., 1:-1, 1:-1].max()) <= 1e-12 and float(miss[..., 0, :].min(dim=-1).values.max()) > 1e-3
    # the table the 16-bit plans use: full fold minus the taps outside, per outside-mask
    m = _resdn("bf16")
    m._repack("cpu")
    table = m._packed["fea_conv#ms#border"].double()
    assert tuple(table.shape) == (16, 48) and bool((table[0] == 0).all())
    for (y, xx), mask in (((0, 0), 1 | 4), ((0, 7), 4), ((14, 14), 2 | 8), ((7, 0), 1), ((7, 14), 2), ((14, 3), 8)):
        got = folded[0, :, y, xx] + table[mask]
        assert float((got - ref[0, :, y, xx]).abs().max()) <= 1e-6, (y, xx)


# ---- counters and plan shape ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_model_complexity_equals_the_reference_model_summary(store):
    from ntire2022_esr_amd.summary import model_complexity
    assert json.load(open(os.path.join(GOLD, f"summary_{NAME}.json"))) == WANT
    m = _resdn(store)
    assert model_complexity(m, (3, 256, 256)) == WANT
    # ... and from the plan of that storage itself (model_complexity builds an fp32-storage plan)
    plan = _plan(m, 1, 256, 256)
    terms = [m._complexity_terms(plan, o) for o in plan.ops]
    assert [float(sum(t[i] for t in terms)) for i in range(3)] == [WANT["flops"], WANT["activations"], float(WANT["num_conv"])]


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("nhw", [(1, 15, 15), (2, 45, 70), (32, 256, 256)], ids=lambda s: "x".join(str(v) for v in s))
def test_plan_shape(store, nhw):
    """A step is five launches -- esr_prelu, the expansion's two parts, esr_prelu, the 3x3 with the residual -- in every storage; the block tail's
    PReLU gathers four sources in one launch; no concat op exists; the mean shifts are ops of the plan (fp32: sub_mean as a convolution of the
    NCHW input; 16-bit: the packed head with a border table)."""
    from ntire2022_esr_amd import _lib as L
    m = _resdn(store)
    m._repack("cpu")
    plan = _plan(m, *nhw)
    arr, in_idx, out_idx = plan.finalize((0x10000000, plan.total_lo), m._packed)
    kinds = [o.kind for o in plan.ops]
    assert kinds.count("prelu") == 28 and kinds.count("apply") == 4 and kinds.count("lowres") == 4 and set(kinds) <= {"prelu", "conv", "apply", "lowres", "pack"}
    assert len(plan.ops) == (94 if store == "f32" else 90) and len(in_idx) == 1 and len(out_idx) == 1
    names = [getattr(o, "w", o.kind) for o in plan.ops]
    if store == "f32":
        assert names[:2] == ["sub_mean#c3", "fea_conv"] and plan.ops[0].src == "__input__"
    else:
        assert names[:2] == ["pack", "fea_conv#ms#head"] and arr[1].conv.border_bias == m._packed["fea_conv#ms#border"].data_ptr()
    n, h, w = nhw
    for k in range(1, 5):
        b = f"body_unit{k}."
        for j in (1, 2, 3):
            i = names.index(b + f"expansion{j}.0")
            assert names[i:i + 5] == [b + f"expansion{j}.0", b + f"expansion{j}.1#res", b + f"expansion{j}.1#dist", b + f"compression{j}.0", b + f"compression{j}.1"]
            d = arr[i].conv
            cin = 48 + 16 * (j - 1)
            assert arr[i].kind == L.OP_PRELU == 20 and L.lib().esr_prelu_supported(ctypes.byref(d)) == 1
            assert (d.n, d.h, d.w, d.cout, d.ksize, d.storage, d.compute) == (n, h, w, cin, 1, L.STORE[store], L.STORE[store])
            assert [c for c in (d.cin, d.split, d.tail_cat_c, d.tail_cout) if c] == [48] + [16] * (j - 1)
            assert (d.out0.pitch, d.out0.coff) == (cin, 0) and d.wpacked == m._packed[b + f"expansion{j}.0#prelu"].data_ptr()
            # the earlier distilled maps: slices of the block's 96-channel buffer [d11 d12 d13 | d21 d22 | d31]
            want = {1: [], 2: [(96, 0)], 3: [(96, 16), (96, 48)]}[j]
            assert [(v.pitch, v.coff) for v, c in ((d.res, d.split), (d.tail_cat, d.tail_cat_c)) if c] == want
            dist = arr[i + 2].conv
            assert (dist.out0.pitch, dist.out0.coff, dist.cout) == (96, {1: 0, 2: 48, 3: 80}[j], 16 * (4 - j))
            c3 = arr[i + 4].conv                                             # x' = x + W_c (*) t into the other buffer
            assert c3.res_mode == L.RES_PRE_ACT and c3.act == L.ACT_NONE and len({c3.inp.ptr, c3.out0.ptr, c3.res.ptr}) == 3
        i = names.index(b + "conv_tail.0")
        d = arr[i].conv
        assert (d.cin, d.split, d.tail_cat_c, d.tail_cout, d.cout) == (48, 16, 16, 16, 96)
        assert [(v.pitch, v.coff) for v in (d.res, d.tail_cat, d.out1)] == [(96, 32), (96, 64), (96, 80)]
        cost = m.op_costs(plan, arr)[i]
        assert cost["kernel"] == f"prelu_kernel<{L.STORE[store]}, true>" and cost["flops"] == float(n * h * w * 96)
    assert names[-8:] == ["T_tdm1.0", "L_tdm1.0", "T_tdm2.0", "L_tdm2.0", "T_tdm3.0", "L_tdm3.0", "tail.0", "tail.1"]


@pytest.mark.parametrize("store", STORES)
def test_op_kinds_do_not_depend_on_the_batch(store):
    m = _resdn(store)
    kinds = [[(o.kind, getattr(o, "w", None), getattr(getattr(o, "post", None), "w", None) if o.kind == "conv" else None) for o in _plan(m, n, 45, 45).ops]
             for n in (1, 8)]
    assert kinds[0] == kinds[1]


# ---- the one-launch step ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_counters_and_plan_shape_of_the_fused_form(store):
    """fuse_resdb is off by default (measured slower than the five launches: DESIGN.md 7l) and shapes no fp32 plan; with it on a
    16-bit plan has ONE resdb op per step whose descriptor satisfies
    esr_resdb_step_supported -- x and x' in tensors of their own, the extra inputs and the distilled outputs as disjoint slices of the block's
    96-channel buffer -- the rest of the plan unchanged, the same workspace, and the reference's counters"""
    from ntire2022_esr_amd import ResDN, _lib as L
    from ntire2022_esr_amd.summary import model_complexity
    assert ResDN().fuse_resdb is False
    per, m = _resdn(store, False), _resdn(store, True)
    assert model_complexity(m, (3, 256, 256)) == WANT
    for nhw in ((1, 15, 15), (8, 45, 70)):
        pp, plan = _plan(per, *nhw), _plan(m, *nhw)
        terms = [m._complexity_terms(plan, o) for o in plan.ops]
        want = [per._complexity_terms(pp, o) for o in pp.ops]
        assert [sum(t[i] for t in terms) for i in range(3)] == [sum(t[i] for t in want) for i in range(3)] and sum(t[2] for t in terms) == 67
        fused = [(i, o) for i, o in enumerate(plan.ops) if o.kind == "resdb"]
        if store == "f32":
            assert not fused and [o.kind for o in plan.ops] == [o.kind for o in pp.ops]
            continue
        m._repack("cpu")
        arr, _, _ = plan.finalize((0x10000000, plan.total_lo), m._packed)
        assert len(fused) == 12 and len(plan.ops) == len(pp.ops) - 48 and plan.total == pp.total
        key = lambda q: (q.kind, getattr(q, "w", None))
        rest = [key(q) for q in pp.ops if not (q.kind in ("prelu", "conv") and ".expansion" in q.w or q.kind in ("prelu", "conv") and ".compression" in q.w)]
        assert [key(q) for q in plan.ops if q.kind != "resdb"] == rest
        for idx, (i, o) in enumerate(fused):
            k, j = idx // 3 + 1, idx % 3 + 1
            b = f"body_unit{k}."
            d = arr[i].conv
            assert arr[i].kind == L.OP_RESDB_STEP == 21 and L.lib().esr_resdb_step_supported(ctypes.byref(d)) == 1
            assert [q.w for q in o.replaces] == [b + f"expansion{j}.0", b + f"expansion{j}.1#res", b + f"expansion{j}.1#dist", b + f"compression{j}.0", b + f"compression{j}.1"]
            assert (d.n, d.h, d.w, d.cin, d.cout, d.ksize, d.post_cout, d.tail_cat_c) == (*nhw, 48, 48, 3, 16 * (4 - j), 16 * (j - 1))
            assert d.wpacked == m._packed[b + f"compression{j}.1#s16"].data_ptr() and d.post_wpacked == m._packed[b + f"expansion{j}.1#s16"].data_ptr()
            assert d.tail_wpacked == m._packed[b + f"expansion{j}.0#step"].data_ptr()
            assert (d.post_out.pitch, d.post_out.coff) == (96, {1: 0, 2: 48, 3: 80}[j])
            assert [(v.pitch, v.coff) for v in (d.res, d.tail_cat) if v.ptr] == {1: [], 2: [(96, 0)], 3: [(96, 16), (96, 48)]}[j]
            assert len({d.inp.ptr, d.out0.ptr, d.post_out.ptr}) == 3 and d.inp.coff == d.out0.coff == 0
            cost = m.op_costs(plan, arr)[i]
            assert cost["kernel"] == f"resdb_step_kernel<{'true' if store == 'bf16' else 'false'}, {j - 1}, {4 - j}>"
    kinds = [[(o.kind, getattr(o, "w", None)) for o in _plan(m, n, 45, 45).ops] for n in (1, 8)]
    assert kinds[0] == kinds[1]                                              # op kinds do not depend on the batch


def test_the_step_blobs_are_the_stand_alone_launches():
    """the fused step multiplies by the images the per-layer launches multiply by: the expansion's two parts are the rows of the whole image,
    the slopes blob is cat(a_e, a_c) unrounded"""
    from ntire2022_esr_amd.engine import unpack_conv_s16, unpack_prelu
    m = _resdn("bf16", True)
    m._repack("cpu")
    sd = m.state_dict()
    for j in (1, 2, 3):
        b, cin, n1 = "body_unit2.", 48 + 16 * (j - 1), 48 + 16 * (4 - j)
        w, bias = unpack_conv_s16(m._packed[b + f"expansion{j}.1#s16"], cin, n1, 1, "bf16")
        wr, br = unpack_conv_s16(m._packed[b + f"expansion{j}.1#res#s16"], cin, 48, 1, "bf16")
        wd, bd = unpack_conv_s16(m._packed[b + f"expansion{j}.1#dist#s16"], cin, n1 - 48, 1, "bf16")
        assert torch.equal(w, torch.cat([wr, wd])) and torch.equal(bias, torch.cat([br, bd]))
        a = unpack_prelu(m._packed[b + f"expansion{j}.0#step"], cin + 48)
        assert torch.equal(a, torch.cat([sd[b + f"expansion{j}.0.weight"], sd[b + f"compression{j}.0.weight"]]))


@pytest.mark.parametrize("store", ["bf16", "f16"])
def test_exact_grid_cases_are_exact(store):
    """the derivation behind tests/test_gpu_resdn.py's bit-for-bit tests holds for every case they run, b_e = 3 included"""
    for v in R.STEP_CASES:
        case = R.step_case("grid", store, *v)
        ref = R.case_ref(case)
        assert R.grid_is_exact(case, ref), v
        assert float(ref["y"].abs().max()) >= 4 and float(ref["t"].abs().max()) >= 2 and float(ref["dists"].abs().max()) >= 2, v
    for nx, nd in R.RESDN_STEPS:
        case = R.step_case("grid", store, (16, 17), nx, nd, b_e=3.0)
        assert R.grid_is_exact(case, R.case_ref(case))


@pytest.mark.parametrize("nx,nd", R.RESDN_STEPS + R.OTHER_STEPS)
def test_the_steps_restatement_equals_the_plain_reference_step(nx, nd):
    """step_ref without its roundings against the step as team43_resdn.py:93-96 writes it (F.prelu, F.conv2d), fp64, 5 x 7; with its roundings
    it differs, and the bias-padded reading differs from it on the border only"""
    case = R.step_case("random", "bf16", (5, 7), nx, nd)
    w1, b1, w3, b3 = R.effective(case)
    free = R.case_ref(case, dt=torch.float64)
    d, y = R.step_plain_f64(case["x"], case["extras"], case["a_e"], w1, b1, case["a_c"], w3, b3)
    assert float((d - free["dists"]).abs().max()) <= 1e-12 and float((y - free["y"]).abs().max()) <= 1e-12
    ref, biased = R.case_ref(case), R.case_ref(case, pad="bias")
    assert float((ref["y"] - free["y"]).abs().max()) > 1e-4
    diff = (ref["y_raw"] - biased["y_raw"]).abs()
    assert float(diff[:, 1:-1, 1:-1].max()) == 0 and float(diff.max()) > 1e-3


def test_resdb_step_supported_is_exactly_n48_d16():
    """both ends of every admitted range, and the first value outside each; the predicate does not look at pointers"""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()

    def desc(**kw):
        d = L.ConvDesc()
        d.n, d.h, d.w, d.ksize, d.cin, d.cout, d.post_cout, d.tail_cat_c = 1, 1, 1, 3, 48, 48, 16, 0
        d.in_layout = d.out_layout = L.NHWC
        d.storage = d.compute = L.STORE["bf16"]
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    sup = lambda **kw: lib.esr_resdb_step_supported(ctypes.byref(desc(**kw)))
    for nd in (16, 32, 48):
        for nx in (0, 16, 32):
            for st in ("bf16", "f16"):
                assert sup(post_cout=nd, tail_cat_c=nx, storage=L.STORE[st], compute=L.STORE[st], h=1 + nd, w=1000) == 1
    for kw in (dict(post_cout=0), dict(post_cout=64), dict(post_cout=24), dict(tail_cat_c=48), dict(tail_cat_c=8), dict(cin=32), dict(cin=64), dict(cout=32),
               dict(cout=64), dict(ksize=1), dict(storage=0, compute=0), dict(compute=L.STORE["f16"]), dict(act=L.ACT_LRELU), dict(post_act=L.ACT_RELU),
               dict(res_mode=L.RES_PRE_ACT), dict(split=16), dict(hilo=1), dict(h=0), dict(border_bias=4096), dict(tail_cout=16)):
        assert sup(**kw) == 0, kw
    d = desc()
    assert lib.esr_resdb_step(ctypes.byref(d), None) == -1                    # ESR_ERR_BAD_ARG: null pointers
    assert lib.esr_resdb_step(ctypes.byref(desc(post_cout=64)), None) == -1   # (null pointers are looked at first)
    assert {"esr_resdb_step", "esr_resdb_step_supported"} <= set(L.EXPORTS)


# ---- the C ABI without a GPU ----------------------------------------------------------------------------------------------------------------
def _desc(L, store="bf16", counts=(48, 16), n=1, h=4, w=4):
    """a valid esr_prelu descriptor over fake addresses (nothing is launched where a check refuses it)"""
    es = 4 if store == "f32" else 2
    d = L.ConvDesc()
    d.n, d.h, d.w, d.ksize, d.cout = n, h, w, 1, sum(counts)
    d.in_layout = d.out_layout = L.NHWC
    d.storage = d.compute = L.STORE[store]
    base = 0x10000000
    for i, (c, (view, count)) in enumerate(zip(counts, (("inp", "cin"), ("res", "split"), ("tail_cat", "tail_cat_c"), ("out1", "tail_cout")))):
        setattr(d, view, L.View(ctypes.c_void_p(base + i * 0x100000), 96, 8 * i))
        setattr(d, count, c)
    d.out0 = L.View(ctypes.c_void_p(base + 0x800000), 96, 0)
    d.wpacked = base + 0x900000
    return d


def test_prelu_descriptor_validation_without_gpu():
    """esr_prelu_supported / esr_prelu validate before anything is launched; a VALID descriptor on a host without a GPU passes every check
    and fails in the launch"""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    BAD_ARG, UNSUPPORTED, LAUNCH = -1, -2, -3                                 # ESR_ERR_BAD_ARG, ESR_ERR_UNSUPPORTED, ESR_ERR_LAUNCH
    assert {"esr_prelu", "esr_prelu_supported", "esr_pack_prelu", "esr_unpack_prelu", "esr_packed_prelu_bytes"} <= set(L.EXPORTS)
    sup = lambda d: lib.esr_prelu_supported(ctypes.byref(d))
    run = lambda d: lib.esr_prelu(ctypes.byref(d), None)
    for store in STORES:
        for counts in ((48,), (48, 16), (48, 16, 16), (48, 16, 16, 16), (5, 3, 7, 2)):
            assert sup(_desc(L, store, counts)) == 1
    def bad(edit, store="bf16", counts=(48, 16)):
        d = _desc(L, store, counts)
        edit(d)
        return d
    unsupported = [lambda d: setattr(d, "cout", 63), lambda d: setattr(d, "ksize", 3), lambda d: setattr(d, "act", L.ACT_LRELU),
                   lambda d: setattr(d, "res_mode", L.RES_PRE_ACT), lambda d: setattr(d, "compute", 0), lambda d: setattr(d, "storage", 3),
                   lambda d: setattr(d, "hilo", 1), lambda d: setattr(d, "post_cout", 8), lambda d: setattr(d, "in_layout", L.NCHW_IN),
                   lambda d: setattr(d, "n", 0), lambda d: (setattr(d, "split", 0), setattr(d, "tail_cat_c", 16), setattr(d, "cout", 64)),       # a gap in the list
                   lambda d: setattr(d, "border_bias", 0x1000)]
    for e in unsupported:
        d = bad(e)
        assert sup(d) == 0 and run(d) == UNSUPPORTED
    bad_arg = [lambda d: setattr(d.inp, "ptr", None), lambda d: setattr(d.res, "ptr", None), lambda d: setattr(d.out0, "ptr", None),
               lambda d: setattr(d, "wpacked", None), lambda d: setattr(d.res, "coff", 4), lambda d: setattr(d.inp, "pitch", 44),
               lambda d: setattr(d.out0, "pitch", 56), lambda d: setattr(d.res, "coff", 88),
               lambda d: setattr(d.out0, "ptr", d.inp.ptr),                                       # the output over a source
               lambda d: (setattr(d.out0, "ptr", d.res.ptr), setattr(d.out0, "coff", 16), setattr(d.out0, "pitch", 96), setattr(d, "cout", 64)),
               lambda d: setattr(d.out0, "ptr", d.inp.ptr + 96 * 2 * 3 + 2)]                       # bytes of the source's tensor, another grid
    for e in bad_arg:
        assert run(bad(e)) == BAD_ARG
    # slices of one pixel grid that do not meet are fine: res channels 8 .. 23 of a tensor, the output its channels 32 .. 95
    d = _desc(L)
    d.out0 = L.View(ctypes.c_void_p(d.res.ptr), 96, 32)
    if torch.cuda.device_count() == 0:
        assert run(d) == LAUNCH and run(_desc(L, "f32", (5, 3, 7, 2))) == LAUNCH


# ---- the shim, the registry, and everything else unchanged ----------------------------------------------------------------------------------
def test_shim_resolves_team43_resdn():
    code = ("import json; from safetensors.torch import load_file; from models.team43_resdn import ResDN; "
            "m = ResDN(upscale_factor=4, in_channels=3, n_feats=48, out_channels=3); "
            f"m.load_state_dict(load_file({CKPT!r}), strict=True); import ntire2022_esr_amd as e; "
            "print(json.dumps([type(m).__module__, ResDN is e.ResDN, sum(p.numel() for p in m.parameters())]))")
    env = dict(os.environ, PYTHONPATH=SHIM + os.pathsep + REPO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=SHIM, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == ["ntire2022_esr_amd.resdn", True, 406504]


def test_select_model_serves_id_43(tmp_path):
    """`harness --model_id 43`: the reference's name and data_range (tests/golden/registry.json); the checkpoint from a model_zoo, or the
    unrounded fixture's two files; supported_ids() -- the ids with weights under weights/ -- and _entries() are unchanged"""
    from ntire2022_esr_amd import ResDN, registry
    ref = json.load(open(os.path.join(GOLD, "registry.json")))["43"]
    m, name, dr, tile = registry.select_model(43, "cpu")
    assert isinstance(m, ResDN) and name == ref["name"] == "43_ResDN" and dr == ref["data_range"] == 1.0 and tile is None
    assert 43 not in registry.supported_ids() and 43 not in registry._entries() and 43 in registry._more_entries()
    true = _true_sd()
    assert len(m.state_dict()) == 162 and all(torch.equal(v, true[k]) for k, v in m.state_dict().items())
    torch.save(true, str(tmp_path / (NAME + ".pth")))
    m2, _, _, _ = registry.select_model(43, "cpu", model_zoo=str(tmp_path))
    assert all(torch.equal(v, true[k]) for k, v in m2.state_dict().items())
