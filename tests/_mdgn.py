"""CPU side of the MDGN tests (tests/test_mdgn.py, tests/test_gpu_mdgn.py, tests/test_gpu_sweep_mdgn.py): fp64 restatements, cases, bounds.

  conv_prelu_ref   include/esr_hip.h's definition of esr_conv_prelu in fp64: v = b + W (*) x with zero padding, f = prelu(v, a), ONE rounding
  mdsa_gate_ref    ... of esr_mdsa_gate: f = prelu(b_f + W_f . cat, a_f), s = sigmoid(b_s + w_s . x), y = f s, ONE rounding
  mdsa_f64         a whole MDSA block from those two, NHWC; mdsa_plain_f64: the block as team24_mdgn.py:22-28 writes it, torch functions, NCHW
  one_store_bound  the project's bound for a value that is rounded once: |ref| eps 1.01 + 3e-5 max(1, |ref|max), eps 2^-8 (bf16) / 2^-11 (fp16)
  MAX_REL          the 16-bit networks' bound on max |dy| / range over the ::9 sample: TWICE the largest distance at which the REFERENCE itself
                   lands when every tensor a plan stores is rounded once (tests/golden/emul_team24_mdgn.json, tools/gen_golden_mdgn.py) -- the
                   kernels' fp32 summation order, the error-diffused 3x3 taps and the hi + lo 1x1 weights put single roundings on the other side
                   of a tie than the emulation does, and each such flip is a whole storage step where the emulation counted half
"""
import json
import os

import torch
import torch.nn.functional as F

import _resdn as R
import _sweep as S

DT = R.DT
NF = 64
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = "team24_mdgn"
SLOPE_RANGE = (-0.88, 0.98)                                # the checkpoint's 1 024 slopes span this
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
BUDGET = {"f32": 0.002, "bf16": 0.01, "f16": 0.005}        # PSNR against the reference's, dB: the project's budgets
CONV_SIZES = [(1, 1), (1, 19), (19, 1), (15, 15), (16, 17), (33, 18)]       # ResDN's step sizes: a pixel, thinner than a tile, ragged tiles
GATE_SHAPES = [(1, 1, 1), (1, 3, 5), (1, 16, 16), (1, 17, 33), (2, 20, 36)]  # esr_pa_gate's list


def load_parts(stem):
    """<stem>.safetensors, .part2, .part3, ... while they exist: their union"""
    from safetensors.torch import load_file
    sd = load_file(os.path.join(GOLD, stem + ".safetensors"))
    k = 2
    while os.path.exists(os.path.join(GOLD, f"{stem}.part{k}.safetensors")):
        sd.update(load_file(os.path.join(GOLD, f"{stem}.part{k}.safetensors")))
        k += 1
    return sd


def emulated():
    return json.load(open(os.path.join(GOLD, f"emul_{NAME}.json")))


def max_rel():
    e = emulated()
    return {"f32": 2e-5, **{store: 2.0 * max(v["rel"] for v in e[store].values()) for store in ("bf16", "f16")}}


def one_store_bound(ref, dt):
    return ref.abs() * EPS[dt] * 1.01 + 3e-5 * max(1.0, float(ref.abs().max()))


def _keep(s, dt):
    return s.double() if dt == torch.float64 else R.store_once(s, dt).double()


def conv_prelu_ref(x, w, b, a, dt, pad="zero"):
    """x [N, H, W, 64] NHWC, w [64, 64, 3, 3], b, a [64] -> dict(v, f_raw, f), NHWC fp64; `f` rounded once to dt (torch.float64: not at all).
    pad: "zero" -- the definition; "prelu_bias" -- the WRONG reading in which the ring around the image holds prelu(b, a), what this layer
    makes of a zero image, instead of zeros"""
    w, b, a = w.double(), b.double(), a.double()
    xn = x.double().permute(0, 3, 1, 2)
    if pad == "prelu_bias":
        ring = R.prelu_f64(b, a).view(1, -1, 1, 1)
        xp = ring.expand(xn.shape[0], xn.shape[1], xn.shape[2] + 2, xn.shape[3] + 2).clone()
        xp[:, :, 1:-1, 1:-1] = xn
        v = F.conv2d(xp, w, b)
    else:
        v = F.conv2d(xn, w, b, padding=1)
    v = v.permute(0, 2, 3, 1)
    f_raw = R.prelu_f64(v, a)
    return dict(v=v, f_raw=f_raw, f=_keep(f_raw, dt))


def conv_prelu_max_ref(x, w, b, a):
    """the WRONG activation: max(v, a v), the kernels' usual epilogue"""
    v = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    return R.prelu_max_f64(v, a)


def sigmoid_f64(v):
    return 1.0 / (1.0 + torch.exp(-v.double()))


def mdsa_gate_ref(f, x, w_f, b_f, a_f, w_s, b_s, dt, act=None):
    """f [N, H, W, 192] = cat(f1, f2, f3), x [N, H, W, 64]; w_f [64, 192], w_s [64], b_s [1] -> dict(raw, arg, s, y_raw, y), NHWC fp64"""
    act = act or R.prelu_f64
    raw = f.double() @ w_f.double().T + b_f.double()
    arg = x.double() @ w_s.double().reshape(-1) + b_s.double().reshape(())
    s = sigmoid_f64(arg)
    y_raw = act(raw, a_f) * s.unsqueeze(-1)
    return dict(raw=raw, arg=arg, s=s, y_raw=y_raw, y=_keep(y_raw, dt))


def mdsa_f64(x, p):
    """a whole MDSA block, NHWC fp64, from the two restatements; p: w1, b1, a1, .. w3, b3, a3, w_f, b_f, a_f, w_s, b_s"""
    fs, src = [], x.double()
    for j in (1, 2, 3):
        src = conv_prelu_ref(src, p[f"w{j}"], p[f"b{j}"], p[f"a{j}"], torch.float64)["f"]
        fs.append(src)
    return mdsa_gate_ref(torch.cat(fs, dim=-1), x, p["w_f"], p["b_f"], p["a_f"], p["w_s"], p["b_s"], torch.float64)["y"]


def mdsa_plain_f64(x, p):
    """the block as team24_mdgn.py:22-28 computes it, torch's own functions in fp64, NCHW inside; returns NHWC"""
    xn = x.double().permute(0, 3, 1, 2)
    d = lambda k: p[k].double()
    f1 = F.prelu(F.conv2d(xn, d("w1"), d("b1"), padding=1), d("a1"))
    f2 = F.prelu(F.conv2d(f1, d("w2"), d("b2"), padding=1), d("a2"))
    f3 = F.prelu(F.conv2d(f2, d("w3"), d("b3"), padding=1), d("a3"))
    f = F.prelu(F.conv2d(torch.cat([f1, f2, f3], dim=1), d("w_f").reshape(NF, 3 * NF, 1, 1), d("b_f")), d("a_f"))
    s = torch.sigmoid(F.conv2d(xn, d("w_s").reshape(1, NF, 1, 1), d("b_s").reshape(1)))
    return (f * s).permute(0, 2, 3, 1)


def random_slopes(c, seed, above_one=True):
    """slopes with negatives, values in (0, 1), an exact 0 and 1 and -- the checkpoint has none, nn.PReLU allows them -- values above 1"""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(c, generator=g) * (SLOPE_RANGE[1] - SLOPE_RANGE[0]) + SLOPE_RANGE[0]
    fixed = torch.tensor([SLOPE_RANGE[0], SLOPE_RANGE[1], 0.25, 0.0, 1.0, -0.5] + ([2.0, 3.62, 1.25] if above_one else []))
    a[:fixed.numel()] = fixed
    return a.float()


def _sparse(rows, cols, per_row, g):
    w = torch.zeros(rows, cols)
    for r in range(rows):
        idx = torch.randperm(cols, generator=g)[:per_row]
        w[r, idx] = torch.randint(0, 2, (per_row,), generator=g).float() * 2 - 1
    return w


def _pick(c, g):
    return torch.tensor([-2.0, -0.5, 0.5, 2.0])[torch.randint(0, 4, (c,), generator=g)]


def conv_case(kind, store, hw, seed=0, bias=None, n=2):
    """inputs of one esr_conv_prelu launch: "grid" -- x in {-1, 0, 1}, three +-1 taps per filter, integer biases in -1 .. 1, slopes from
    {-2, -1/2, 1/2, 2}; "random" -- randn data, randn weights / sqrt(fan-in), slopes with negatives and values above 1"""
    dt = DT[store]
    h, w = hw
    g = torch.Generator().manual_seed(7000 * seed + 100 * h + w)
    if kind == "grid":
        x = torch.randint(-1, 2, (n, h, w, NF), generator=g).float()
        wt = _sparse(NF, NF * 9, 3, g).reshape(NF, NF, 3, 3)
        b, a = torch.randint(-1, 2, (NF,), generator=g).float(), _pick(NF, g)
    else:
        x = torch.randn(n, h, w, NF, generator=g)
        wt = torch.randn(NF, NF, 3, 3, generator=g) / (9 * NF) ** 0.5
        b, a = torch.randn(NF, generator=g) * 0.5, random_slopes(NF, seed + 1)
    if bias is not None:
        b = torch.full_like(b, bias)
    return dict(x=x.to(dt), w=wt, b=b, a=a, dt=dt, store=store)


def conv_effective(case):
    """the weights conv_prelu_kernel multiplies by: the esr_pack_conv_s16 image read back, error-diffused taps included"""
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    return unpack_conv_s16(pack_conv_s16(case["w"], case["b"], case["store"]), NF, NF, 3, case["store"])


def conv_case_ref(case, pad="zero", dt=None):
    w, b = conv_effective(case)
    return conv_prelu_ref(case["x"], w, b, case["a"], case["dt"] if dt is None else dt, pad)


def conv_grid_is_exact(case, ref):
    """tests/_resdn.py grid_is_exact's method: the packer leaves the weights as they are, every value is a value of the storage type, every
    partial sum is exact in fp32 (multiples of 1/2 below 2^10), and the rounded restatement equals the unrounded one"""
    dt = case["dt"]
    w, b = conv_effective(case)
    if not (torch.equal(w, case["w"]) and torch.equal(b, case["b"])):
        return False
    free = conv_prelu_ref(case["x"], w, b, case["a"], torch.float64)
    for k in ("v", "f_raw"):
        v = free[k]
        if not (torch.equal(R.store_once(v, dt).double(), v) and torch.equal(v * 2, (v * 2).round()) and float(v.abs().max()) < 1024):
            return False
    return torch.equal(free["f"], ref["f"])


def gate_case(kind, store, shape, seed=0, gate=True):
    """inputs of one esr_mdsa_gate launch: "grid" -- f and x in {-1, 0, 1}, three +-1 weights per row of W_f, integer b_f, slopes from
    {-2, -1/2, 1/2, 2}, and (gate=False) w_s = 0, b_s = 0: s = 1/2 exactly; "random" -- randn data, W_f randn / sqrt(192), slopes with negatives and
    values above 1, w_s scaled so that the gate's argument stays within +-8 (the checkpoint's reach 3.6 on test.bmp)"""
    dt = DT[store]
    n, h, w = shape
    g = torch.Generator().manual_seed(9000 * seed + 1000 * n + 100 * h + w)
    if kind == "grid":
        f, x = torch.randint(-1, 2, (n, h, w, 3 * NF), generator=g).float(), torch.randint(-1, 2, (n, h, w, NF), generator=g).float()
        w_f, b_f, a_f = _sparse(NF, 3 * NF, 3, g), torch.randint(-1, 2, (NF,), generator=g).float(), _pick(NF, g)
    else:
        f, x = torch.randn(n, h, w, 3 * NF, generator=g), torch.randn(n, h, w, NF, generator=g)
        w_f, b_f, a_f = torch.randn(NF, 3 * NF, generator=g) / (3 * NF) ** 0.5, torch.randn(NF, generator=g) * 0.5, random_slopes(NF, seed + 3)
    if gate:
        w_s, b_s = torch.randn(NF, generator=g) * 0.25, torch.randn(1, generator=g)
    else:
        w_s, b_s = torch.zeros(NF), torch.zeros(1)
    f, x = f.to(dt), x.to(dt)
    if gate:
        reach = float((x.double() @ w_s.double() + b_s.double()).abs().max())
        if reach > 7.5:                                     # scaled as a whole: the gate's argument stays within +-8
            w_s, b_s = w_s * (7.5 / reach), b_s * (7.5 / reach)
        assert float((x.double() @ w_s.double() + b_s.double()).abs().max()) <= 8.0
    return dict(f=f, x=x, w_f=w_f, b_f=b_f, a_f=a_f, w_s=w_s, b_s=b_s, dt=dt, store=store)


def gate_effective(case):
    """(W_f = hi + lo, b_f, a_f, w_s, b_s) as mdsa_gate_kernel holds them: read back from the esr_pack_mdsa_gate blob"""
    from ntire2022_esr_amd.engine import pack_mdsa_gate, unpack_mdsa_gate
    return unpack_mdsa_gate(pack_mdsa_gate(case["w_f"], case["b_f"], case["a_f"], case["w_s"], case["b_s"], case["store"]), case["store"])


def gate_case_ref(case, dt=None, act=None):
    w_f, b_f, a_f, w_s, b_s = gate_effective(case)
    return mdsa_gate_ref(case["f"], case["x"], w_f, b_f, a_f, w_s, b_s, case["dt"] if dt is None else dt, act)


def gate_grid_is_exact(case, ref):
    """the blob holds the weights as they are, s is exactly 1/2, every partial sum and f are exact, and y = store(f / 2)"""
    dt = case["dt"]
    eff = gate_effective(case)
    if not all(torch.equal(e, case[k]) for e, k in zip(eff, ("w_f", "b_f", "a_f", "w_s", "b_s"))):
        return False
    free = gate_case_ref(case, dt=torch.float64)
    if not (bool((free["s"] == 0.5).all()) and torch.equal(free["raw"], free["raw"].round()) and float(free["raw"].abs().max()) < 1024):
        return False
    f = R.prelu_f64(free["raw"], case["a_f"])
    return torch.equal(free["y_raw"], f / 2) and torch.equal(ref["y"], R.store_once(f / 2, dt).double())


def stacked(f, pitch=64, coff=0, fill=0.0):
    """cat(f1, f2, f3) [N, H, W, 192] as the planar form: [3, N, H, W, pitch] with the 64 channels of f_i from `coff`, `fill` elsewhere"""
    n, h, w, _ = f.shape
    out = torch.full((3, n, h, w, pitch), fill).to(f.dtype)
    for i in range(3):
        out[i, ..., coff:coff + NF] = f[..., i * NF:(i + 1) * NF]
    return out
