"""CPU side of the ResDN tests (tests/test_resdn.py, tests/test_gpu_resdn.py, tests/test_gpu_sweep_resdn.py): the fp64 restatements.

  prelu_f64        v >= 0 ? v : a v, the definition esr_prelu implements (include/esr_hip.h)
  prelu_max_f64    max(v, a v), what the kernels' usual epilogue computes: the same function for 0 <= a <= 1 only
  store_once       an fp64 tensor rounded ONCE (RNE) to a storage type -- torch's fp64 -> bf16 / fp16 conversion goes through fp32 and may round
                   twice, so the nearest neighbour is chosen here from _sweep.neighbours, ties to the even pattern, overflow to Inf
  prelu_stored     what esr_prelu stores for a tensor of a storage type and fp32 slopes
  resdb_f64        a whole ResDB (team43_resdn.py:90-111) in fp64 from a state dict, layer by layer as the reference runs it
  resdb_split_f64  the same block as the plan runs it: the concats gathered by the PReLU, every expansion 1x1 in two parts, the distilled maps
                   raw in one 96-channel buffer (NaN wherever nothing was written)
  head_f64         fea_conv(sub_mean(x)) with the shift BEFORE the zero padding, and its bias-folded (wrong at the border) reading
"""
import torch
import torch.nn.functional as F

import _sweep as S

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
NF, ND = 48, 16
SLOPE_RANGE = (-1.82, 3.62)                                # the checkpoint's 1 728 body slopes span this


def prelu_f64(v, a):
    """v [..., C] fp64, a [C]"""
    v, a = v.double(), a.double()
    return torch.where(v >= 0, v, a * v)


def prelu_max_f64(v, a):
    v, a = v.double(), a.double()
    return torch.maximum(v, a * v)


def store_once(s, dt):
    """fp64 -> dt with ONE rounding to nearest, ties to even; beyond the largest finite value + half a step: Inf"""
    s = s.double()
    if dt == torch.float32:
        return s.float()                                    # (fp64 -> fp32 is one rounding)
    lo, hi = S.neighbours(s, dt)
    lod, hid = lo.double(), hi.double()
    dl, dh = s - lod, hid - s
    even_lo = S.to_bits(lo) % 2 == 0
    pick_lo = (dl < dh) | ((dl == dh) & even_lo)
    out = torch.where(pick_lo, lo, hi)
    top = torch.finfo(dt).max
    half = 2.0 ** (1 - S.EMIN[dt] - S.MBITS[dt] - 1)       # half a step of the top binade (its exponent: 1 - EMIN)
    over = s.abs() >= top + half
    inf = torch.full_like(out, float("inf"))
    return torch.where(over, torch.where(s < 0, -inf, inf), out)


def prelu_stored(x, a):
    """x of a storage type [..., C], a fp32 [C] -> the tensor esr_prelu stores: non-negative values as they are, the exact product a v
    rounded once"""
    ref = store_once(a.float().double() * x.double(), x.dtype)
    return torch.where(x.float() >= 0, x, ref)


def conv_f64(x, w, b, pad):
    return F.conv2d(x.double(), w.double(), b.double(), padding=pad)


def _p(sd, name):
    return sd[name].double()


def _nchw_prelu(x, a):
    return torch.where(x >= 0, x, a.double().view(1, -1, 1, 1) * x)


def resdb_f64(sd, b, x):
    """the block `b` ('body_unit1.') WITHOUT its attention: returns (x1, x2, x3, t) -- the running x after each step and conv_tail's
    result -- from NCHW fp64 x, as team43_resdn.py:90-108 computes them"""
    x = x.double()
    conv = lambda n, v, pad: conv_f64(_nchw_prelu(v, _p(sd, b + n + '.0.weight')), _p(sd, b + n + '.1.weight'), _p(sd, b + n + '.1.bias'), pad)
    res = conv('expansion1', x, 0)
    res, d11, d12, d13 = torch.split(res, (NF, ND, ND, ND), dim=1)
    x1 = x + conv('compression1', res, 1)
    res = conv('expansion2', torch.cat((x1, d11), 1), 0)
    res, d21, d22 = torch.split(res, (NF, ND, ND), dim=1)
    x2 = x1 + conv('compression2', res, 1)
    res = conv('expansion3', torch.cat((x2, d12, d21), 1), 0)
    res, d31 = torch.split(res, (NF, ND), dim=1)
    x3 = x2 + conv('compression3', res, 1)
    t = conv('conv_tail', torch.cat((x3, d13, d22, d31), 1), 0)
    return x1, x2, x3, t


def resdb_split_f64(sd, b, x):
    """the same block as resdn.py's plan runs it (per-layer form): the PReLU launch gathers the sources, the expansion 1x1 runs as its
    `res` rows and its distilled rows, the distilled maps lie raw in ONE buffer [d11 d12 d13 | d21 d22 | d31] that starts as NaN"""
    x = x.double()
    n, _, h, w = x.shape
    D = torch.full((n, 6 * ND, h, w), float("nan"), dtype=torch.float64)
    d = lambda i: D[:, i * ND:(i + 1) * ND]
    outs = []
    for j, (extra, (lo, hi)) in enumerate((((), (0, 3)), ((0,), (3, 5)), ((1, 3), (5, 6))), start=1):
        e = b + f'expansion{j}.'
        u = _nchw_prelu(torch.cat([x] + [d(i) for i in extra], 1), _p(sd, e + '0.weight'))
        we, be = _p(sd, e + '1.weight'), _p(sd, e + '1.bias')
        r = F.conv2d(u, we[:NF], be[:NF])
        D[:, lo * ND:hi * ND] = F.conv2d(u, we[NF:], be[NF:])
        c = b + f'compression{j}.'
        x = x + F.conv2d(_nchw_prelu(r, _p(sd, c + '0.weight')), _p(sd, c + '1.weight'), _p(sd, c + '1.bias'), padding=1)
        outs.append(x)
    u = _nchw_prelu(torch.cat([x, d(2), d(4), d(5)], 1), _p(sd, b + 'conv_tail.0.weight'))
    t = F.conv2d(u, _p(sd, b + 'conv_tail.1.weight'), _p(sd, b + 'conv_tail.1.bias'))
    assert not bool(torch.isnan(D).any())
    return outs[0], outs[1], outs[2], t


def head_f64(sd, x, folded=False):
    """fea_conv(sub_mean(x)) in fp64.  folded: the WRONG reading -- the shift as a constant added to fea_conv's bias, as if the padding ring
    held -mean and not 0"""
    x = x.double()
    ws, bs = _p(sd, 'sub_mean.weight'), _p(sd, 'sub_mean.bias')
    wf, bf = _p(sd, 'fea_conv.weight'), _p(sd, 'fea_conv.bias')
    if folded:
        return F.conv2d(x, wf, bf + torch.einsum('ocij,c->o', wf, bs), padding=1)
    return F.conv2d(F.conv2d(x, ws, bs), wf, bf, padding=1)


def random_slopes(c, seed):
    """c slopes drawn over the checkpoint's own range, with its extremes, a value in (0, 1) and an exact 0 and 1 among them"""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(c, generator=g) * (SLOPE_RANGE[1] - SLOPE_RANGE[0]) + SLOPE_RANGE[0]
    fixed = torch.tensor([SLOPE_RANGE[0], SLOPE_RANGE[1], 0.25, 0.0, 1.0, -0.5, 2.0])
    a[:min(c, fixed.numel())] = fixed[:c]
    return a.float()


# ---- the one-launch step (esr_resdb_step) -------------------------------------------------------------------------------------------------
STEP_SIZES = [(1, 1), (1, 19), (19, 1), (15, 15), (16, 17), (33, 18)]
RESDN_STEPS = [(0, 3), (1, 2), (2, 1)]                    # (extra inputs, distilled outputs) of a ResDB's three steps
OTHER_STEPS = [(0, 1), (0, 2), (1, 1), (1, 3), (2, 2), (2, 3)]      # the rest of what esr_resdb_step_supported admits: both ends of both ranges
STEP_CASES = [(hw, nx, nd) for hw in STEP_SIZES for nx, nd in RESDN_STEPS] + [(hw, nx, nd) for hw in STEP_SIZES[-2:] for nx, nd in OTHER_STEPS]


def _keep(s, dt):
    return s.double() if dt == torch.float64 else store_once(s, dt).double()


def step_ref(x, extras, a_e, w_e, b_e, a_c, w_c, b_c, dt, pad="zero"):
    """include/esr_hip.h's definition of esr_resdb_step in fp64, every `~` one rounding to dt (torch.float64: none).  x [N, H, W, 48] and extras
    [N, H, W, 16] each, NHWC; w_e [48 + 16 nd, cin], w_c [48, 48, 3, 3].  pad: "zero" -- t is 0 outside the image; "bias" -- the WRONG reading, a
    halo pixel holds prelu(b_e).  Returns a dict of NHWC fp64 tensors u, e, r, t, dists, y, and dists_raw / y_raw: the two outputs in front of
    their store (what a bound for ONE rounding is measured against)."""
    a_e, a_c, w_e, w_c, b_e, b_c = (v.double() for v in (a_e, a_c, w_e, w_c, b_e, b_c))
    inp = torch.cat([x] + list(extras), dim=-1).double()
    u = _keep(prelu_f64(inp, a_e), dt)
    e = u @ w_e.reshape(w_e.shape[0], -1).T + b_e
    dists, r = _keep(e[..., NF:], dt), _keep(e[..., :NF], dt)
    t = _keep(prelu_f64(r, a_c), dt)
    tn = t.permute(0, 3, 1, 2)
    if pad == "bias":
        halo = _keep(prelu_f64(_keep(b_e[:NF], dt), a_c), dt).view(1, NF, 1, 1)
        tp = halo.expand(tn.shape[0], NF, tn.shape[2] + 2, tn.shape[3] + 2).clone()
        tp[:, :, 1:-1, 1:-1] = tn
        conv = F.conv2d(tp, w_c, b_c)
    else:
        conv = F.conv2d(tn, w_c, b_c, padding=1)
    y_raw = x.double() + conv.permute(0, 2, 3, 1)
    return dict(u=u, e=e, r=r, t=t, dists=dists, y=_keep(y_raw, dt), dists_raw=e[..., NF:], y_raw=y_raw)


def step_plain_f64(x, extras, a_e, w_e, b_e, a_c, w_c, b_c):
    """the step as team43_resdn.py:93-96 writes it, torch modules' functions in fp64, NCHW inside: (dists, y) as NHWC"""
    inp = torch.cat([x] + list(extras), dim=-1).double().permute(0, 3, 1, 2)
    res = F.conv2d(F.prelu(inp, a_e.double()), w_e.double().reshape(w_e.shape[0], -1, 1, 1), b_e.double())
    res, d = res[:, :NF], res[:, NF:]
    y = x.double().permute(0, 3, 1, 2) + F.conv2d(F.prelu(res, a_c.double()), w_c.double(), b_c.double(), padding=1)
    return d.permute(0, 2, 3, 1), y.permute(0, 2, 3, 1)


def _sparse(rows, cols, per_row, g):
    """[rows, cols] with `per_row` entries of +-1 per row, zeros elsewhere"""
    w = torch.zeros(rows, cols)
    for r in range(rows):
        idx = torch.randperm(cols, generator=g)[:per_row]
        w[r, idx] = torch.randint(0, 2, (per_row,), generator=g).float() * 2 - 1
    return w


def step_case(kind, store, hw, nx, nd, seed=0, b_e=None, n=2):
    """inputs of one step: kind "grid" -- x and extras in {-1, 0, 1}, three +-1 weights per expansion row and two per compression filter,
    integer biases in -1 .. 1, slopes drawn from {-2, -1/2, 1/2, 2}; "random" -- randn data, randn weights scaled by 1 / sqrt(fan-in), slopes
    over the checkpoint's range.  Batch n."""
    dt = DT[store]
    h, w = hw
    cin = NF + ND * nx
    g = torch.Generator().manual_seed(1000 * seed + 100 * h + 10 * w + 3 * nx + nd)
    if kind == "grid":
        draw = lambda *s: torch.randint(-1, 2, s, generator=g).float()
        pick = lambda c: torch.tensor([-2.0, -0.5, 0.5, 2.0])[torch.randint(0, 4, (c,), generator=g)]
        x, extras = draw(n, h, w, NF), [draw(n, h, w, ND) for _ in range(nx)]
        a_e, a_c = pick(cin), pick(NF)
        w_e, w_c = _sparse(NF + ND * nd, cin, 3, g), _sparse(NF, NF * 9, 2, g).reshape(NF, NF, 3, 3)
        be, bc = draw(NF + ND * nd), draw(NF)
    else:
        x, extras = torch.randn(n, h, w, NF, generator=g), [torch.randn(n, h, w, ND, generator=g) for _ in range(nx)]
        a_e, a_c = random_slopes(cin, seed + 1), random_slopes(NF, seed + 2)
        w_e = torch.randn(NF + ND * nd, cin, generator=g) / cin ** 0.5
        w_c = torch.randn(NF, NF, 3, 3, generator=g) / (9 * NF) ** 0.5
        be, bc = torch.randn(NF + ND * nd, generator=g) * 0.5, torch.randn(NF, generator=g) * 0.5
    if b_e is not None:
        be = torch.full_like(be, b_e)
    return dict(x=x.to(dt), extras=[e.to(dt) for e in extras], a_e=a_e, w_e=w_e, b_e=be, a_c=a_c, w_c=w_c, b_c=bc, dt=dt, store=store)


def effective(case):
    """the weights the kernel multiplies by: the expansion's hi + lo pairs and the 3x3 with its diffused rounding, read back from the
    esr_pack_conv_s16 blobs"""
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    n1, cin = case["w_e"].shape
    w1, b1 = unpack_conv_s16(pack_conv_s16(case["w_e"].reshape(n1, cin, 1, 1), case["b_e"], case["store"]), cin, n1, 1, case["store"])
    w3, b3 = unpack_conv_s16(pack_conv_s16(case["w_c"], case["b_c"], case["store"]), NF, NF, 3, case["store"])
    return w1.reshape(n1, cin), b1, w3, b3


def case_ref(case, pad="zero", dt=None):
    w1, b1, w3, b3 = effective(case)
    return step_ref(case["x"], case["extras"], case["a_e"], w1, b1, case["a_c"], w3, b3, case["dt"] if dt is None else dt, pad)


def grid_is_exact(case, ref):
    """every intermediate of the exact-grid case is a value of the storage type, the packers leave the weights as they are, and every
    partial sum is exact in fp32: all terms are multiples of 1/4 below 2^10"""
    dt = case["dt"]
    w1, b1, w3, b3 = effective(case)
    if not (torch.equal(w1, case["w_e"]) and torch.equal(w3, case["w_c"]) and torch.equal(b1, case["b_e"]) and torch.equal(b3, case["b_c"])):
        return False
    free = step_ref(case["x"], case["extras"], case["a_e"], w1, b1, case["a_c"], w3, b3, torch.float64)
    for k in ("u", "e", "t", "y"):
        v = free[k]
        if not (torch.equal(store_once(v, dt).double(), v) and torch.equal(v * 4, (v * 4).round()) and float(v.abs().max()) < 1024):
            return False
    return all(torch.equal(free[k], ref[k]) for k in ("dists", "y"))


def step_bounds(case, ref):
    """(bound of dists, bound of y) against ref's dists_raw / y_raw, the fp64 values in front of the store: tests/test_gpu_c64m.py's bound for
    one 16-bit store, and for y the same plus |W_c| (*) ulp(t), the issue's term: the kernel's fp32 sum and the fp64 one may round r to
    neighbouring values, which moves t by about one of its steps.  u is exact (a single rounding of an exact product), so it has no term.
    (Measured on the MI355X with the wider term |a_c| ulp(r) + ulp(t), at most 3 ulp(t): dists 0.97, y 0.27 of the bound -- DESIGN.md 7l.)"""
    dt = case["dt"]
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    tol = lambda v: v.abs() * eps * 1.01 + 3e-5 * max(1.0, float(v.abs().max()))
    _, _, w3, _ = effective(case)
    ulp_t = 2 * S.half_step(ref["t"], dt)
    extra = F.conv2d(ulp_t.permute(0, 3, 1, 2), w3.double().abs(), padding=1).permute(0, 2, 3, 1)
    return tol(ref["dists_raw"]), tol(ref["y_raw"]) + extra
