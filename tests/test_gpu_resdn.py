"""-m gpu: esr_prelu (prelu_kernel, csrc/esr_resdb.hip) against its single-rounding restatement, and ResDN (NTIRE 2022 ESR team 43) end to end
against the reference's goldens (tools/gen_golden_resdn.py) in fp32, bf16 and fp16 storage.  CPU side: tests/_resdn.py, tests/test_resdn.py."""
import os

import numpy as np
import pytest
import torch

import _guarded as G
import _poison as P
import _resdn as R
import _sweep as S
from conftest import GOLD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "team43_resdn"
STORES = ["f32", "bf16", "f16"]
BUDGET = {"f32": 0.002, "bf16": 0.01, "f16": 0.005}         # PSNR against the reference's, dB: the project's budgets
# max |dy| / range on the ::9 sample of the big images: fp32 the project's 2e-5; 16-bit: twice the largest value measured on the MI355X
# over both sizes and both forms (bf16 6.62e-3, f16 8.98e-4, at 339 x 510, per-layer and fused alike)
MAX_REL = {"f32": 2e-5, "bf16": 1.33e-2, "f16": 1.80e-3}
SENTINEL = 777.0
ST = {"f32": 0, "bf16": 1, "f16": 2}                        # esr_storage: prelu_kernel's first template argument


# ---- esr_prelu -----------------------------------------------------------------------------------------------------------------------------
def _sources(store, hw, counts, seed, nan_pads=True):
    """[(tensor, coff, channels)] of unequal pitch and offset, values around zero with both signs; every slot outside a view's channels is
    NaN (pad slots, the channels in front of coff), so a kernel that reads one poisons its output"""
    dt = R.DT[store]
    gran = 4 if store == "f32" else 8
    g = torch.Generator().manual_seed(seed)
    h, w = hw
    out = []
    for i, c in enumerate(counts):
        coff = gran * (i % 3)
        pitch = (coff + c + gran - 1) // gran * gran + gran * ((i + 1) % 2)
        t = torch.full((2, h, w, pitch), float("nan") if nan_pads else 0.0)
        t[..., coff:coff + c] = torch.randn(2, h, w, c, generator=g) * 3.0
        out.append((t.to(dt), coff, c))
    return out


def _prelu_case(store, hw, counts, seed, out_extra=0, out_coff=0):
    from ntire2022_esr_amd import ops
    dt = R.DT[store]
    gran = 4 if store == "f32" else 8
    srcs = _sources(store, hw, counts, seed)
    ctot = sum(counts)
    a = R.random_slopes(ctot, seed + 1)
    want = R.prelu_stored(torch.cat([t[..., o:o + c] for t, o, c in srcs], dim=-1), a)
    cst = (ctot + gran - 1) // gran * gran
    out = torch.full((2,) + tuple(hw) + (out_coff + cst + out_extra,), SENTINEL, dtype=dt).to(DEV)
    with ops.kernel_trace() as names:
        y = ops.prelu([(t.to(DEV), o, c) for t, o, c in srcs], a, out=out, out_coff=out_coff)
    torch.cuda.synchronize()
    vec = all(c % gran == 0 for c in counts)
    assert names == [f"prelu_kernel<{ST[store]}, {'true' if vec else 'false'}>"], names
    y = y.cpu()
    got = y[..., out_coff:out_coff + ctot]
    assert bool(torch.isfinite(got.float()).all()), "a NaN of a pad slot reached the output"
    assert torch.equal(got.view(torch.int32 if store == "f32" else torch.int16), want.view(torch.int32 if store == "f32" else torch.int16)), \
        (store, hw, counts, float((got.double() - want.double()).abs().max()))
    assert bool((y[..., out_coff + ctot:out_coff + cst] == 0).all()), "the pad slots up to the granule are zeros"
    assert bool((y[..., :out_coff] == SENTINEL).all()) and bool((y[..., out_coff + cst:] == SENTINEL).all()), "written outside the view"
    return srcs, a, want


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("hw", [(1, 1), (33, 18)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_prelu_four_sources_equal_the_single_rounding_bit_for_bit(store, hw):
    """four sources with unequal pitch and coff, whole granules (the vector path): every stored value equals v >= 0 ? v : store_once(a v) with
    slopes over the checkpoint's range; NaN in every pad slot of the sources changes no bit; the output lies inside a sentinel-filled tensor
    at an offset, and the sentinel stays intact"""
    _prelu_case(store, hw, (48, 16, 16, 16), 3, out_extra=8, out_coff=8)


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("counts", [(5,), (5, 3, 7, 2), (48, 16, 3)], ids=lambda v: "-".join(map(str, v)))
def test_prelu_ragged_channel_counts(store, counts):
    """counts that are no whole granules (the gathering path): a granule spans two sources, the output's pad slots are zeros"""
    _prelu_case(store, (16, 17), counts, 5, out_extra=8)


@pytest.mark.parametrize("store", STORES)
def test_prelu_resdn_layers(store):
    """the four source lists of a ResDB at the block's widths, dense output as the plan allocates it"""
    for counts in ((48,), (48, 16), (48, 16, 16), (48, 16, 16, 16)):
        _prelu_case(store, (15, 15), counts, 7)


@pytest.mark.parametrize("store", STORES)
def test_prelu_is_not_max_v_av(store):
    """The kernels' usual epilogue, max(v, a v), is nn.PReLU for a <= 1 only.  Shown on the CPU first: for a > 1 the two readings differ on
    BOTH signs of v by far more than a storage step (max picks a v for v > 0 and v for v < 0); for a < 0 they coincide (a v > 0 > v), so what
    the checkpoint's 352 negative slopes need is only that nothing clamps them.  Then the kernel is held to v >= 0 ? v : a v, bit for bit."""
    from ntire2022_esr_amd import ops
    dt = R.DT[store]
    a = torch.tensor([2.5, 1.5, 3.62, 2.0, -1.5, -0.5, -1.82, -0.25])
    x = (torch.randn(2, 16, 17, 8, generator=torch.Generator().manual_seed(1)) * 2).to(dt)
    x = torch.where(x.float().abs() < 0.01, torch.ones_like(x), x)
    right, wrong = R.prelu_f64(x, a), R.prelu_max_f64(x, a)
    step = S.half_step(right, dt) * 2 if store != "f32" else right.abs() * 2.0 ** -23
    assert bool(((right - wrong).abs()[..., :4] > 20 * step[..., :4]).all()), "a > 1: the readings differ everywhere"
    assert bool((right == wrong)[..., 4:].all()), "a < 0: the readings coincide"
    y = ops.prelu([x.to(DEV)], a).cpu()
    assert torch.equal(y.double(), R.prelu_stored(x, a).double())
    assert float((y.double() - wrong).abs()[..., :4].min()) > 0


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("counts", [(48, 16, 16, 16), (5, 3, 7, 2)], ids=lambda v: "-".join(map(str, v)))
def test_prelu_stays_inside_its_views(store, counts):
    """tests/_guarded.py: every tensor of the launch in one allocation with NaN in front of and behind each source (and in its pad slots) and
    sentinel bytes around and inside the output, of which only the view's channels up to the granule are declared writable -- no NaN reaches
    the result, and no other byte changes, at 33 x 18 and at a single pixel"""
    from ntire2022_esr_amd import ops
    dt = R.DT[store]
    gran = 4 if store == "f32" else 8
    for hw in ((33, 18), (1, 1)):
        srcs = _sources(store, hw, counts, 11)
        ctot = sum(counts)
        cst = (ctot + gran - 1) // gran * gran
        a = R.random_slopes(ctot, 12)
        arena = G.Arena(DEV, fill="nan")
        for i, (t, _, _) in enumerate(srcs):
            arena.add_input(f"src{i}", t)
        arena.add_output("out", (2,) + hw + (cst + 2 * gran,), dt, writable=(-1, gran, cst))
        arena.build()
        ops.prelu([(arena[f"src{i}"], o, c) for i, (_, o, c) in enumerate(srcs)], a, out=arena["out"], out_coff=gran)
        arena.check_untouched()
        got = arena.written("out").cpu()
        want = R.prelu_stored(torch.cat([t[..., o:o + c] for t, o, c in srcs], dim=-1), a)
        assert torch.equal(got[..., :ctot].double(), want.double()) and bool((got[..., ctot:] == 0).all())


def test_prelu_refusals_launch_nothing():
    from ntire2022_esr_amd import _lib as L, ops
    x = torch.zeros(1, 4, 4, 16, dtype=torch.bfloat16, device=DEV)
    a = torch.ones(16)
    with pytest.raises(L.EsrError):                          # the output's bytes meet a source's
        ops.prelu([x], a, out=x)
    big = torch.zeros(1, 4, 4, 32, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(L.EsrError):                          # ... as channel ranges of one tensor too
        ops.prelu([(big, 8, 16)], a, out=big, out_coff=16)
    y = ops.prelu([(big, 0, 16)], a, out=big, out_coff=16)   # disjoint slices of one pixel grid are fine
    assert y is big
    with pytest.raises(L.EsrError):                          # coff is not whole granules
        ops.prelu([(big, 4, 16)], a)
    with pytest.raises(L.EsrError):                          # the view does not hold its channels
        ops.prelu([(x, 8, 16)], a)
    with pytest.raises(L.EsrError):                          # five sources
        ops.prelu([x] * 5, torch.ones(80))
    with pytest.raises(L.EsrError):
        ops.prelu([x.cpu()], a)


# ---- esr_resdb_step ------------------------------------------------------------------------------------------------------------------------
STEP_PARAMS = [pytest.param(*v, id=f"{v[0][0]}x{v[0][1]}-{v[1]}-{v[2]}") for v in R.STEP_CASES]
KINDS_16 = ["bf16", "f16"]


def _run_step(case, x_pitch=48, x_coff=0, nan=False, **kw):
    """the step through ops.resdb_step under kernel_trace; x in a tensor of pitch x_pitch from x_coff, the extras and the distilled outputs
    as slices of ONE 96-channel tensor (as the plan keeps them): extras at 0 / 16, the outputs from 32.  nan: every slot that is no input is NaN"""
    from ntire2022_esr_amd import ops
    dt = case["dt"]
    n, h, w, _ = case["x"].shape
    fill = float("nan") if nan else 0.0
    x = torch.full((n, h, w, x_pitch), fill).to(dt)
    x[..., x_coff:x_coff + 48] = case["x"]
    D = torch.full((n, h, w, 96), fill).to(dt)
    for i, e in enumerate(case["extras"]):
        D[..., 16 * i:16 * i + 16] = e
    nd = case["w_e"].shape[0] - 48
    D[..., 32:32 + nd] = SENTINEL                       # (what the launch overwrites)
    Dd = D.to(DEV)
    y = torch.full((n, h, w, 64), SENTINEL, dtype=dt).to(DEV)
    with ops.kernel_trace() as names:
        dd, yy = ops.resdb_step(x.to(DEV), case["a_e"], case["w_e"], case["b_e"], case["a_c"], case["w_c"], case["b_c"],
                                extras=[(Dd, 16 * i) for i in range(len(case["extras"]))], x_coff=x_coff, d_out=Dd, d_coff=32, out=y, out_coff=8, **kw)
    torch.cuda.synchronize()
    assert names == [f"resdb_step_kernel<{'true' if dt == torch.bfloat16 else 'false'}, {len(case['extras'])}, {nd // 16}>"], names
    Dc, yc = dd.cpu(), yy.cpu()
    # nothing outside the views is written: the extras' slices and what lies behind the outputs keep their bits, y's tensor its sentinel
    keep = torch.ones(96, dtype=torch.bool)
    keep[32:32 + nd] = False
    assert torch.equal(Dc[..., keep].view(torch.int16), D[..., keep].view(torch.int16)), "the distilled outputs' tensor outside their slice"
    assert bool((yc[..., :8] == SENTINEL).all()) and bool((yc[..., 56:] == SENTINEL).all()), "y's tensor outside its slice"
    return Dc[..., 32:32 + nd], yc[..., 8:56]


@pytest.mark.parametrize("store", KINDS_16)
@pytest.mark.parametrize("hw,nx,nd", STEP_PARAMS)
def test_step_is_bit_exact_on_the_exact_grid(store, hw, nx, nd):
    """inputs and sparse weights in {-1, 0, 1}, integer biases, slopes from {-2, -1/2, 1/2, 2}: the CPU asserts that every intermediate is
    representable and every partial sum exact (tests/_resdn.py: grid_is_exact), then dists and y equal the restatement bit for bit"""
    case = R.step_case("grid", store, hw, nx, nd)
    ref = R.case_ref(case)
    assert R.grid_is_exact(case, ref)
    d, y = _run_step(case)
    assert torch.equal(d.double(), ref["dists"]), float((d.double() - ref["dists"]).abs().max())
    assert torch.equal(y.double(), ref["y"]), float((y.double() - ref["y"]).abs().max())


@pytest.mark.parametrize("store", KINDS_16)
@pytest.mark.parametrize("hw,nx,nd", STEP_PARAMS)
def test_step_matches_fp64_restatement(store, hw, nx, nd):
    """random data, slopes over the checkpoint's range (negative ones and values above 1 among them): dists within the one-store bound, y within
    it plus |W_c| (*) ulp(t) (tests/_resdn.py: step_bounds); NaN in every slot that is no input changes no bit"""
    case = R.step_case("random", store, hw, nx, nd)
    ref = R.case_ref(case)
    assert int((case["a_e"] < 0).sum()) and int((case["a_e"] > 1).sum()) and int((case["a_c"] < 0).sum()) and int((case["a_c"] > 1).sum())
    bd, by = R.step_bounds(case, ref)
    d, y = _run_step(case)
    rd, ry = float(((d.double() - ref["dists_raw"]).abs() / bd).max()), float(((y.double() - ref["y_raw"]).abs() / by).max())
    print(f"resdb step {store} {hw} nx={nx} nd={nd}: dists {rd:.2f}, y {ry:.2f} of the bound")
    assert rd <= 1 and ry <= 1, (rd, ry)
    d2, y2 = _run_step(case, x_pitch=64, x_coff=8, nan=True)
    assert torch.equal(d2.view(torch.int16), d.view(torch.int16)) and torch.equal(y2.view(torch.int16), y.view(torch.int16))


@pytest.mark.parametrize("store", KINDS_16)
@pytest.mark.parametrize("nx,nd", R.RESDN_STEPS)
def test_step_prelu_is_not_max_v_av(store, nx, nd):
    """with every slope above 1 the max(v, a v) reading of both PReLUs is far outside the bound -- shown on the CPU --, and the kernel is held to
    v >= 0 ? v : a v"""
    case = R.step_case("random", store, (16, 17), nx, nd, seed=3)
    case["a_e"] = case["a_e"].abs() + 1.25
    case["a_c"] = case["a_c"].abs() + 1.25
    ref = R.case_ref(case)
    w1, b1, w3, b3 = R.effective(case)
    orig = R.prelu_f64
    try:
        R.prelu_f64 = R.prelu_max_f64
        wrong = R.step_ref(case["x"], case["extras"], case["a_e"], w1, b1, case["a_c"], w3, b3, case["dt"])
    finally:
        R.prelu_f64 = orig
    bd, by = R.step_bounds(case, ref)
    assert float(((wrong["y"] - ref["y_raw"]).abs() / by).max()) > 30 and float(((wrong["dists"] - ref["dists_raw"]).abs() / bd).max()) > 30
    d, y = _run_step(case)
    assert bool(((d.double() - ref["dists_raw"]).abs() <= bd).all()) and bool(((y.double() - ref["y_raw"]).abs() <= by).all())


@pytest.mark.parametrize("store", KINDS_16)
@pytest.mark.parametrize("nx,nd", R.RESDN_STEPS)
def test_t_is_zero_padded_not_bias_padded(store, nx, nd):
    """b_e = 3 on the exact grid: the CPU first shows that the two readings of the halo -- 0, or prelu(b_e) -- differ on the border only; the
    kernel equals the zero-padded one bit for bit"""
    case = R.step_case("grid", store, (16, 17), nx, nd, b_e=3.0)
    ref, biased = R.case_ref(case), R.case_ref(case, pad="bias")
    assert R.grid_is_exact(case, ref)
    diff = (ref["y"] - biased["y"]).abs()
    assert float(diff[:, 1:-1, 1:-1].max()) == 0 and float(diff.max()) >= 1
    d, y = _run_step(case)
    assert torch.equal(y.double(), ref["y"]) and torch.equal(d.double(), ref["dists"])


@pytest.mark.parametrize("store", KINDS_16)
@pytest.mark.parametrize("nx,nd", R.RESDN_STEPS)
def test_step_stays_inside_its_views(store, nx, nd):
    """tests/_guarded.py: every tensor of the launch in one allocation -- NaN in front of and behind x and the tensor that holds the extra
    inputs (and in every slot of them that is no input), sentinel bytes around and inside the two outputs' tensors, of which only the views'
    channels are declared writable.  At 33 x 18 (the halo loads next to the last pixel, the ragged tiles' stores) and at a single pixel no NaN
    reaches a result, the results equal those of the plain run bit for bit, and no other byte changes."""
    from ntire2022_esr_amd import ops
    dt = R.DT[store]
    for hw in ((33, 18), (1, 1)):
        case = R.step_case("random", store, hw, nx, nd)
        d0, y0 = _run_step(case)
        n, (h, w) = 2, hw
        x = torch.full((n, h, w, 64), float("nan")).to(dt)
        x[..., 8:56] = case["x"]
        E = torch.full((n, h, w, 40), float("nan")).to(dt)
        for i, e in enumerate(case["extras"]):
            E[..., 8 + 16 * i:24 + 16 * i] = e
        arena = G.Arena(DEV, fill="nan")
        arena.add_input("x", x)
        arena.add_input("extras", E)
        arena.add_output("dists", (n, h, w, 16 * nd + 16), dt, writable=(-1, 8, 16 * nd))
        arena.add_output("y", (n, h, w, 64), dt, writable=(-1, 16, 48))
        arena.build()
        ops.resdb_step(arena["x"], case["a_e"], case["w_e"], case["b_e"], case["a_c"], case["w_c"], case["b_c"],
                       extras=[(arena["extras"], 8 + 16 * i) for i in range(nx)], x_coff=8, d_out=arena["dists"], d_coff=8, out=arena["y"], out_coff=16)
        arena.check_untouched()
        d, y = arena.written("dists").cpu(), arena.written("y").cpu()
        assert bool(torch.isfinite(d.float()).all()) and bool(torch.isfinite(y.float()).all())
        assert torch.equal(d.view(torch.int16), d0.contiguous().view(torch.int16)) and torch.equal(y.view(torch.int16), y0.contiguous().view(torch.int16))


def test_step_refusals_launch_nothing():
    from ntire2022_esr_amd import _lib as L, ops
    case = R.step_case("grid", "bf16", (4, 5), 1, 2)
    args = [case[k] for k in ("a_e", "w_e", "b_e", "a_c", "w_c", "b_c")]
    x = case["x"].to(DEV)
    e0 = torch.zeros(2, 4, 5, 96, dtype=torch.bfloat16, device=DEV)
    ops.resdb_step(x, *args, extras=[(e0, 0)], d_out=e0, d_coff=32)                     # dists next to the extra input in one tensor: fine
    with pytest.raises(L.EsrError):                                                     # y over x: the neighbouring tiles read x as halo
        ops.resdb_step(x, *args, extras=[(e0, 0)], out=x)
    with pytest.raises(L.EsrError):                                                     # dists over the extra input's channels
        ops.resdb_step(x, *args, extras=[(e0, 16)], d_out=e0, d_coff=0)
    big = torch.zeros(2, 4, 5, 96, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(L.EsrError):                                                     # y and dists in one slice
        ops.resdb_step(x, *args, extras=[(e0, 0)], d_out=big, d_coff=16, out=big, out_coff=0)
    with pytest.raises(L.EsrError):                                                     # coff is not whole granules
        ops.resdb_step(x, *args, extras=[(e0, 4)])
    with pytest.raises(L.EsrError):                                                     # the view does not hold 16 channels
        ops.resdb_step(x, *args, extras=[(e0, 88)])
    with pytest.raises(L.EsrError):                                                     # an extra input too few for the weights
        ops.resdb_step(x, *args)
    with pytest.raises(L.EsrError):                                                     # four distilled outputs
        ops.resdb_step(x, case["a_e"], torch.zeros(112, 64), torch.zeros(112), *args[3:], extras=[(e0, 0)])
    with pytest.raises(L.EsrError):                                                     # fp32 storage
        ops.resdb_step(x.float(), *args, extras=[(e0.float(), 0)])


# ---- the network ------------------------------------------------------------------------------------------------------------------------------
_models = {}


def _sd(true_weights):
    from safetensors.torch import load_file
    if not true_weights:
        return load_file(os.path.join(GOLD, NAME + ".safetensors"))
    sd = load_file(os.path.join(GOLD, NAME + "_f32.safetensors"))
    sd.update(load_file(os.path.join(GOLD, NAME + "_f32.part2.safetensors")))
    return sd


FORMS = [("f32", False), ("bf16", False), ("bf16", True), ("f16", False), ("f16", True)]      # (an fp32 plan has the per-layer form only)


def _n_fused(m, shape):
    return sum(o.kind == "resdb" for o in m._plans[_key(shape)].plan.ops)


def _resdn(compute, true_weights=False, fuse=False):
    from ntire2022_esr_amd import ResDN
    key = "true" if true_weights else "m"
    if key not in _models:
        m = ResDN()
        m.load_state_dict(_sd(true_weights), strict=True)
        _models[key] = m.eval().to(DEV)
    m = _models[key]
    m.set_compute(compute)
    m.fuse_resdb = fuse
    m.use_graphs = True
    return m


def _key(shape):
    return tuple(shape) + (torch.device(DEV),)


def _buffer(m, shape, name):
    """the plan's buffer `name` of the last forward of `shape`, as an [N, H, W, pitch] tensor of the plan's storage type"""
    dev = torch.device(DEV)
    ent = m._plans[_key(shape)]
    ctx = m._ctxs[(dev, torch.cuda.default_stream(dev).cuda_stream)]
    b = next(b for b in ent.plan.buffers if b.name == name)
    n = ent.plan.n * b.h * b.w * b.pitch * b.esize
    raw = ctx.ws[ctx.lo_cap + b.offset:ctx.lo_cap + b.offset + n]
    return raw.view(R.DT[ent.plan.store]).reshape(ent.plan.n, b.h, b.w, b.pitch).cpu()


@pytest.mark.parametrize("compute", STORES)
def test_head_shifts_the_mean_before_the_zero_padding(compute):
    """sub_mean + fea_conv on a constant image of value 1.0 at 15 x 15 against fp64.  The CPU first shows that the bias-folded reading (the
    padding ring at -mean instead of 0) misses on the border by far more than the bound and agrees inside.  The bound: fp32 -- 32 roundings
    of 2^-24 over sum |W| |x - mean| + |b|; 16-bit -- the input and the head's weights travel as hi + lo pairs (each within 2^-17 of its value,
    the lo x lo product dropped: 2^-15 of sum |W| |x| + sum |W| |mean| + |b| covers it) plus one rounding of the stored value."""
    sd = {k: v.float() for k, v in _sd(False).items()}
    x = torch.ones(1, 3, 15, 15)
    ref, folded = R.head_f64(sd, x), R.head_f64(sd, x, folded=True)
    wabs = sd["fea_conv.weight"].double().abs()
    mean = sd["sub_mean.bias"].double().abs()
    mag = wabs.sum(dim=(1, 2, 3)) * 1.0 + torch.einsum('ocij,c->o', wabs, mean) + sd["fea_conv.bias"].double().abs()
    if compute == "f32":
        tol = (32 * 2.0 ** -24 * mag).view(1, -1, 1, 1).expand_as(ref)
    else:
        tol = S.store_tol(ref, R.DT[compute]) + (2.0 ** -15 * mag).view(1, -1, 1, 1)
    miss = (folded - ref).abs()
    inner = torch.zeros(15, 15, dtype=torch.bool)
    inner[1:-1, 1:-1] = True
    assert float(miss[..., inner].max()) <= 1e-12 and float((miss / tol)[..., ~inner].max()) > 10
    m = _resdn(compute)
    with torch.no_grad():
        m(x.to(DEV))
    torch.cuda.synchronize()
    x0 = _buffer(m, (1, 3, 15, 15), "x0")[..., :48].permute(0, 3, 1, 2).double()
    err = (x0 - ref).abs()
    print(f"ResDN head {compute}: max err / bound = {float((err / tol).max()):.3f}; the folded reading misses by {float((miss / tol).max()):.1f} bounds")
    assert bool((err <= tol).all()), float((err / tol).max())


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_fp32_matches_reference_e2e(case):
    g = np.load(os.path.join(GOLD, f"e2e_{NAME}.npz"))
    m = _resdn("f32")
    x, ref = torch.from_numpy(g["x" + case]).to(DEV), g["y" + case]
    with torch.no_grad():
        y = m(x).cpu().numpy()
    assert y.shape == ref.shape
    err = float(np.abs(y.astype(np.float64) - ref).max())
    print(f"ResDN e2e {case}: max|y - ref| = {err:.3e}, max|ref| = {float(np.abs(ref).max()):.3f}")
    assert err <= 2e-5 * max(1.0, float(np.abs(ref).max())), err


def _hr(h4, w4):
    from PIL import Image
    img = np.array(Image.open(os.path.join(GOLD, "test.bmp")).convert("RGB"))
    return np.pad(img, ((0, h4 - img.shape[0]), (0, w4 - img.shape[1]), (0, 0)), mode="symmetric")


_big = {}


@pytest.mark.parametrize("compute,fuse", FORMS)
@pytest.mark.parametrize("h,w", [(256, 256), (339, 510)])
def test_psnr_against_reference_at_stated_size(h, w, compute, fuse):
    from ntire2022_esr_amd import image_util as util
    g = np.load(os.path.join(GOLD, f"big_{NAME}_{h}x{w}.npz"))
    m = _resdn(compute, fuse=fuse)
    dr = float(g["data_range"])
    with torch.no_grad():
        y = m(util.uint2tensor4(g["lr"], dr).to(DEV))
    psnr = util.calculate_psnr(util.tensor2uint(y, dr), _hr(4 * h, 4 * w), border=4)
    rel = float(np.abs(y[0, :, ::9, ::9].cpu().numpy().astype(np.float64) - g["sr_sample"]).max()) / dr
    print(f"ResDN {h}x{w} {compute} fuse_resdb={int(fuse)}: PSNR {psnr:.4f} vs reference {float(g['psnr']):.4f} dB (d = {psnr - float(g['psnr']):+.4f}), "
          f"max|dy|/range = {rel:.2e}")
    kinds = [o.kind for o in m._plans[_key((1, 3, h, w))].plan.ops]
    assert kinds.count("prelu") == (4 if fuse else 28) and kinds.count("resdb") == (12 if fuse else 0) and bool(torch.isfinite(y).all())
    _big[(h, w, compute, fuse)] = y[0, :, ::9, ::9].cpu().double()
    assert abs(psnr - float(g["psnr"])) <= BUDGET[compute]
    assert rel <= MAX_REL[compute], rel


@pytest.mark.parametrize("compute", KINDS_16)
@pytest.mark.parametrize("h,w", [(256, 256), (339, 510)])
def test_fused_against_per_layer(h, w, compute):
    """The fused step rounds u, r, t, dists and x' where the five launches round them and multiplies by the same weight images; only the order
    of the fp32 sums differs, so a value of r or x' near a tie may fall to the neighbouring 16-bit value.  The two forms' outputs therefore
    agree within the bound that holds each of them to the reference (MAX_REL, the ::9 sample), both of which the PSNR test has checked."""
    per, fused = _big.get((h, w, compute, False)), _big.get((h, w, compute, True))
    if per is None or fused is None:
        test_psnr_against_reference_at_stated_size(h, w, compute, False)
        test_psnr_against_reference_at_stated_size(h, w, compute, True)
        per, fused = _big[(h, w, compute, False)], _big[(h, w, compute, True)]
    rel = float((per - fused).abs().max())
    print(f"ResDN {h}x{w} {compute}: fused against per-layer max|dy|/range = {rel:.2e}")
    assert rel <= MAX_REL[compute], rel


@pytest.mark.parametrize("compute,fuse", FORMS)
@pytest.mark.parametrize("hw", [64, 128])
def test_batch_equals_per_image(compute, fuse, hw):
    m = _resdn(compute, fuse=fuse)
    x = torch.rand(2, 3, hw, hw, generator=torch.Generator().manual_seed(hw)).to(DEV)
    with torch.no_grad():
        yb = m(x)
        ys = [m(x[i:i + 1]) for i in range(2)]
    assert _n_fused(m, x.shape) == _n_fused(m, (1, 3, hw, hw)) == (12 if fuse else 0)
    for i in range(2):
        assert torch.equal(yb[i:i + 1], ys[i]), (i, float((yb[i:i + 1] - ys[i]).abs().max()))


@pytest.mark.parametrize("compute,fuse", FORMS)
def test_graph_forward_equals_run_ops(compute, fuse):
    from ntire2022_esr_amd import _lib as L
    m = _resdn(compute, fuse=fuse)
    shape = (1, 3, 40, 52)
    g = torch.Generator().manual_seed(9)
    xs = [torch.rand(*shape, generator=g).to(DEV) for _ in range(4)]
    with torch.no_grad():
        m.use_graphs = False
        ref = [m(x).clone() for x in xs]
        torch.cuda.synchronize()
        m.use_graphs = True
        ys = [m(x) for x in xs]               # forwards 2 .. 4 are ONE graph launch each, with new x / y: the mean shifts are part of the plan
    torch.cuda.synchronize()
    ent = m._plans[shape + (torch.device(DEV),)]
    assert ent.graph is not None and L.lib().esr_graph_nodes(ent.graph) >= len(ent.arr)
    for y, r in zip(ys, ref):
        assert torch.equal(y, r), float((y - r).abs().max())


@pytest.mark.parametrize("shape", [(1, 3, 15, 15), (2, 3, 20, 36)], ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("compute,fuse", FORMS)
def test_result_does_not_depend_on_stale_workspace_bytes(compute, fuse, shape):
    """tests/test_gpu_stale_workspace.py's first check for this network: the whole workspace overwritten with hostile finite patterns
    (tests/_poison.py) between two forwards of one shape, through esr_run_ops and through graph replay, bit for bit.  The fp32 plan's
    3-channel mean-shifted input lives in an 8-slot pixel whose last four slots nothing writes: they meet zero weights."""
    m = _resdn(compute, fuse=fuse)
    assert not m.rezero_on_switch
    dev = torch.device(DEV)
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(17 * shape[2] + shape[3])).to(DEV)
    try:
        results = []
        for graphs in (False, True):
            m.use_graphs = graphs
            m._drop_plans()                                     # a fresh context: prepare() zero-fills the workspace
            ent = m.prepare(shape, DEV)
            ctx = m._ctxs[(dev, torch.cuda.default_stream(dev).cuda_stream)]
            assert ctx.ws_owner == _key(shape) and not bool(ctx.ws.any())
            assert _n_fused(m, shape) == (12 if fuse else 0)
            y0 = m(x).clone()
            if graphs:
                m(x)                                            # the second forward of a shape captures the graph; replays from here on
                assert ent.graph is not None
            assert bool(torch.isfinite(y0).all())
            results.append(y0)
            for pat in P.PATTERNS:
                ctx.ws.copy_(P.pattern(pat, ctx.ws.numel(), ctx.lo_cap, compute, shape[2]).to(DEV))      # ws_owner stays: no zero fill
                y = m(x)
                assert m._plans[_key(shape)] is ent and ctx.ws_owner == _key(shape)
                assert torch.equal(y, y0), (pat, graphs, float((y - y0).abs().max()), int((y != y0).sum()))
        assert torch.equal(results[0], results[1])
    finally:
        m.invalidate_workspaces()                               # the next forward of this model starts from zeros again


# ---- the unrounded checkpoint (tests/test_gpu_true_weights.py's checks for this network) ------------------------------------------------------
_true = {}


def _true_golden():
    if "g" not in _true:
        g = dict(np.load(os.path.join(GOLD, f"true_{NAME}.npz")))
        e2e = np.load(os.path.join(GOLD, f"e2e_{NAME}.npz"))
        g["xb"], g["xc"] = e2e["xb"], e2e["xc"]
        g["lr"] = np.load(os.path.join(GOLD, f"big_{NAME}_256x256.npz"))["lr"]
        _true["g"] = g
    return _true["g"]


@pytest.mark.parametrize("case", ["b", "c"])
def test_fp32_matches_reference_e2e_true_weights(case):
    g = _true_golden()
    m = _resdn("f32", true_weights=True)
    with torch.no_grad():
        y = m(torch.from_numpy(g["x" + case]).to(DEV)).cpu().numpy()
    err = float(np.abs(y.astype(np.float64) - g["y" + case]).max())
    print(f"ResDN true weights e2e {case}: max|y - ref| = {err:.3e}")
    assert err <= 2e-5 * max(1.0, float(np.abs(g["y" + case]).max())), err


@pytest.mark.parametrize("compute,fuse", FORMS)
def test_true_weights_at_256(compute, fuse):
    """a batch of two copies of the 256 x 256 image with the unrounded checkpoint: bit-identical outputs, the PSNR budget of the type, and
    max |dy| / range within the bound measured with exact weights plus the reference's own figure for rounding every weight once to the type"""
    from ntire2022_esr_amd import image_util as util
    g = _true_golden()
    m = _resdn(compute, true_weights=True, fuse=fuse)
    dr = float(g["data_range"])
    x = util.uint2tensor4(g["lr"], dr).to(DEV)
    with torch.no_grad():
        y = m(x.repeat(2, 1, 1, 1).contiguous())
    assert y.shape == (2, 3, 1024, 1024) and bool(torch.isfinite(y).all())
    dpsnr = util.calculate_psnr(util.tensor2uint(y[0:1], dr), _hr(1024, 1024), border=4) - float(g["psnr"])
    rel = float(np.abs(y[0, :, ::9, ::9].cpu().numpy().astype(np.float64) - g["sr_sample"]).max()) / dr
    bound = MAX_REL[compute] + (float(g["dw_rel_" + compute]) if compute != "f32" else 0.0)
    print(f"ResDN true weights 2x256x256 {compute} fuse_resdb={int(fuse)}: dPSNR = {dpsnr:+.4f} dB (budget {BUDGET[compute]}), max|dy|/range = {rel:.2e} (bound {bound:.2e})")
    assert torch.equal(y[0], y[1]), float((y[0] - y[1]).abs().max())
    assert abs(dpsnr) <= BUDGET[compute], dpsnr
    assert rel <= bound, (rel, bound)
